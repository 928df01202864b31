// resnetse.hip — the 2-D kernels of ResNetSE34V2 (reference models/ResNetBaseline.py:141-301, ResNetBlocks.py:211-246) for gfx950.
//
// Activations are channels-last (B, P, Q, C): P = frames (the reference's W), Q = mel rows (its H), C innermost, fp32 or bf16.
//
// rs_conv_kernel: a KS x KS convolution (KS = 3, zero padding 1; KS = 1, no padding: the downsample), stride 1 or 2, as an implicit GEMM
// on MFMA.  M = output positions, N = Cout, K = KS KS Cin.
//   tile    one workgroup = TP x TQ <= 128 output positions of ONE utterance (rs_conv_plan picks TP, TQ for the image) x BN = 32 / 64
//           output channels; four waves of 32 positions each, NT = BN / 32 accumulators of 32 x 32 per wave.  N = 32 gets the tall tile
//           (128 x 32), N >= 64 runs 128 x 64 tiles, Cout / 64 of them per position tile (the halo is then re-read from L2).
//   K loop  the input channels in chunks of 64 bytes (32 bf16 / 16 fp32).  Per chunk the workgroup stages the HALO of its tile —
//           ((TP - 1) s + KS) x ((TQ - 1) s + KS) positions, zero outside the image, the block's opening ReLU applied on the way — and the
//           KS KS x BN weight rows of the chunk in LDS once; the nine taps then read their A fragments from the halo at shifted positions.
//           An utterance's tile never reads another utterance's rows: the halo is addressed by (b, p, q), not by a flat row index.
//   LDS     64 bytes per position / weight row, its four 16-byte slots XOR-ed with (row >> 2) & 3: sixteen consecutive rows cover the sixteen
//           slots of a 256-byte bank row, so the ds_read_b128 fragment reads of stride-1 tiles are conflict-free (stride 2: two-way).
//   MFMA    bf16: v_mfma_f32_32x32x16_bf16, fp32 accumulation; fp32: v_mfma_f32_32x32x2_f32 (exact products, the parity path).
//   out     y = scale[n] acc + shift[n] (the folded BatchNorm), optional ReLU, stored in the activation type; with `part` also the
//           per-(tile, channel) sums of y over the tile's valid positions (fp32, fixed order) — the SE squeeze, finished by rs_se_gate in
//           tile order.  No atomics: permuting the batch permutes every value bit for bit.
//   packs   RAG = true: n utterances of different frame counts, their images back to back (launch_rs_conv_ragged).  A workgroup still owns
//           TP x TQ <= 128 positions of one utterance; it finds the utterance in a tile prefix built on the device from the level's row0
//           table (rs_rag_tiles_kernel), takes that utterance's own tile and frame counts, and runs the same body: an utterance's values
//           and tile sums are those of the fixed form on it alone.  The grid is the pack's tiles, no more.  The stem, the SE gate and the
//           block tail carry the same flag: their RAG instances read the utterance from the level's tables and run the fixed text.
// Every ReLU here is x < 0 ? 0 : x, which keeps a NaN (fmaxf would drop it): a NaN input reaches the embedding of its own utterance.
#include "common.h"
#include "kernels.h"

namespace svhip {

namespace {

constexpr int RS_ROWB = 64;            // bytes of one position's channel chunk / one weight row in LDS
constexpr int RS_HALO_MAX = 56 * 1024; // LDS bytes the halo may take (the weights of a 64-channel tile take 36 KiB)

template <typename T> struct RsMma;
template <> struct RsMma<float> {
    static constexpr int EPC = 4, CK = 16;
    typedef f32x4 chunk_t;
    static __device__ __forceinline__ void mma(const chunk_t& a, const chunk_t& b, f32x16& c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], c, 0, 0, 0);
    }
    static __device__ __forceinline__ chunk_t zero() { return chunk_t{0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ chunk_t relu(chunk_t v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] < 0.0f ? 0.0f : v[j];
        return v;
    }
};
template <> struct RsMma<bf16_t> {
    static constexpr int EPC = 8, CK = 32;
    typedef bf16x8 chunk_t;
    static __device__ __forceinline__ void mma(const chunk_t& a, const chunk_t& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ chunk_t zero() {
        chunk_t z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = static_cast<bf16_t>(0.0f);
        return z;
    }
    static __device__ __forceinline__ chunk_t relu(chunk_t v) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = static_cast<float>(v[j]) < 0.0f ? static_cast<bf16_t>(0.0f) : v[j];
        return v;
    }
};

// The tile rs_conv_plan gives an output image of Po x Qo positions.  One function for the host (rs_conv_plan; the grid and the LDS of a
// pack) and the device (rs_rag_tiles_kernel), which must agree on every image: the score is a few IEEE double operations, and contraction
// into fused multiply-adds, which only the device has, is switched off, so both sides round alike.
__host__ __device__ inline void rs_tile_of(int Po, int Qo, int stride, int ks, int& TP, int& TQ) {
#pragma clang fp contract(off)
    double best = -1.0;
    TP = TQ = 1;
    for (int tq = 1; tq <= 32 && tq <= Qo; ++tq) {
        const int tp = 128 / tq < Po ? 128 / tq : Po;
        const int64_t halo = (int64_t)((tp - 1) * stride + ks) * ((tq - 1) * stride + ks);
        if (halo * RS_ROWB > RS_HALO_MAX) continue;
        const double cover = (double)((Po + tp - 1) / tp * tp) * ((Qo + tq - 1) / tq * tq);
        // MFMA rows that carry an output, then (a tie-breaker) the halo positions staged per output
        const double score = ((double)Po * Qo / cover) * (tp * tq / 128.0) - 0.01 * (double)halo / ((double)tp * tq * stride * stride);
        if (score > best) { best = score; TP = tp; TQ = tq; }
    }
}

__device__ __forceinline__ int rs_slot(int row, int ch) { return row * RS_ROWB + ((ch ^ ((row >> 2) & 3)) << 4); }

// RAG false: a fixed-length batch, the tile found from the grid index alone.  RAG true: a pack (p.rag) — the workgroup finds its utterance u
// by a binary search of the tile prefix rag.tile0 (uniform over the workgroup, ceil(log2 n) <= 8 steps for n <= 256), then makes its copy
// of p describe that utterance alone: its own tile (rag.plan[u], rs_tile_of of its own image), its own frame counts (the two levels' row0
// tables) and X / Y at its first frame.  The K loop and the epilogue below are then the fixed form's on that image: the zero padding sits
// at the utterance's own first and last frame, and `part` is indexed by the pack's tile number, which runs through an utterance's tiles in
// its own tile order.
template <typename T, int BN, int KS, bool RAG>
__global__ __launch_bounds__(256) void rs_conv_kernel(RsConvParams p) {
    int tile_first = 0;                 // RAG: the pack's tiles before this utterance's
    if constexpr (RAG) {
        const RsRagConv& r = p.rag;
        const int t = blockIdx.x / (p.Cout / BN);
        int lo = 0, hi = r.n;           // tile0[lo] <= t < tile0[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (r.tile0[mid] <= t) lo = mid; else hi = mid;
        }
        const int ri = r.row0_in[lo], ro = r.row0_out[lo], pl = r.plan[lo];
        tile_first = r.tile0[lo];
        p.P = r.row0_in[lo + 1] - ri;
        p.Po = r.row0_out[lo + 1] - ro;
        p.TP = pl & 255;
        p.TQ = pl >> 8;
        p.ntp = (p.Po + p.TP - 1) / p.TP;
        p.ntq = (p.Qo + p.TQ - 1) / p.TQ;
        p.X = reinterpret_cast<const T*>(p.X) + (int64_t)ri * p.Q * p.Cin;
        p.Y = reinterpret_cast<T*>(p.Y) + (int64_t)ro * p.Qo * p.Cout;
    }
    typedef RsMma<T> TR;
    typedef typename TR::chunk_t chunk_t;
    constexpr int EPC = TR::EPC, CK = TR::CK, NT = BN / 32, NTAPS = KS * KS, PAD = KS / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int HP = (p.TP - 1) * p.stride + KS, HQ = (p.TQ - 1) * p.stride + KS;
    char* halo = smem;
    char* wl = smem + HP * HQ * RS_ROWB;

    const int nn = p.Cout / BN;         // the channel tiles of one position tile are neighbours in the grid: they share the halo in L2
    const int tile = blockIdx.x / nn;
    const int tq_i = (tile - tile_first) % p.ntq, t2 = (tile - tile_first) / p.ntq;
    const int tp_i = t2 % p.ntp, b = t2 / p.ntp;      // (RAG: b = 0)
    const int p0 = tp_i * p.TP, q0 = tq_i * p.TQ;
    const int ip0 = p0 * p.stride - PAD, iq0 = q0 * p.stride - PAD;
    const int n0 = (blockIdx.x - tile * nn) * BN;
    const T* __restrict__ X = reinterpret_cast<const T*>(p.X) + (int64_t)b * p.P * p.Q * p.Cin;
    const T* __restrict__ W = reinterpret_cast<const T*>(p.W);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5;
    const int mt = p.TP * p.TQ;
    int abase;                          // this lane's A row: the halo position of its output position at tap (0, 0)
    {
        int m = wave * 32 + fr;
        if (m >= mt) m = 0;             // (rows beyond the tile compute position 0 again; the epilogue drops them)
        const int tp = m / p.TQ, tq = m - tp * p.TQ;
        abase = tp * p.stride * HQ + tq * p.stride;
    }

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

    const int nchunks = p.Cin / CK;
    const int nhalo = HP * HQ * 4, nw = NTAPS * BN * 4;
    for (int c = 0; c < nchunks; ++c) {
        if (c) __syncthreads();         // the previous chunk's fragments have been read
        for (int idx = tid; idx < nhalo; idx += 256) {
            const int pos = idx >> 2, ch = idx & 3;
            const int hp = pos / HQ, hq = pos - hp * HQ;
            const int ip = ip0 + hp, iq = iq0 + hq;
            chunk_t v = TR::zero();
            if (ip >= 0 && ip < p.P && iq >= 0 && iq < p.Q) {
                v = *reinterpret_cast<const chunk_t*>(X + ((int64_t)ip * p.Q + iq) * p.Cin + c * CK + ch * EPC);
                if (p.relu_in) v = TR::relu(v);
            }
            *reinterpret_cast<chunk_t*>(halo + rs_slot(pos, ch)) = v;
        }
        for (int idx = tid; idx < nw; idx += 256) {
            const int row = idx >> 2, ch = idx & 3;
            const int tap = row / BN, n = row - tap * BN;
            *reinterpret_cast<chunk_t*>(wl + rs_slot(row, ch)) =
                *reinterpret_cast<const chunk_t*>(W + (((int64_t)c * NTAPS + tap) * p.Cout + n0 + n) * CK + ch * EPC);
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < NTAPS; ++tap) {
            const int pos = abase + (tap / KS) * HQ + (tap % KS);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int ch = 2 * s + fh;
                const chunk_t a = *reinterpret_cast<const chunk_t*>(halo + rs_slot(pos, ch));
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const chunk_t w = *reinterpret_cast<const chunk_t*>(wl + rs_slot(tap * BN + j * 32 + fr, ch));
                    TR::mma(a, w, acc[j]);
                }
            }
        }
    }

    // ---- epilogue: BN affine, optional ReLU, store; per-tile channel sums -------------------------------------------
    T* __restrict__ Y = reinterpret_cast<T*>(p.Y) + (int64_t)b * p.Po * p.Qo * p.Cout;
    float csum[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) csum[j] = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        const int tp = m / p.TQ, tq = m - tp * p.TQ;
        const int po = p0 + tp, qo = q0 + tq;
        const bool ok = m < mt && po < p.Po && qo < p.Qo;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = n0 + j * 32 + fr;
            float v = fmaf(acc[j][r], p.scale[n], p.shift[n]);
            if (p.relu_out) v = v < 0.0f ? 0.0f : v;
            if (ok) {
                Y[((int64_t)po * p.Qo + qo) * p.Cout + n] = from_f32<T>(v);
                csum[j] += v;
            }
        }
    }
    if (p.part) {
        __syncthreads();                // (the LDS is free: every wave has left the K loop)
        float* red = reinterpret_cast<float*>(smem);          // [4 waves][BN]
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const float other = __shfl_xor(csum[j], 32, 64);
            if (fh == 0) red[wave * BN + j * 32 + fr] = csum[j] + other;
        }
        __syncthreads();
        if (tid < BN) {
            const float s = ((red[tid] + red[BN + tid]) + red[2 * BN + tid]) + red[3 * BN + tid];
            p.part[(int64_t)tile * p.Cout + n0 + tid] = s;
        }
    }
}

template <typename T, int BN, int KS>
hipError_t rs_conv_launch(const RsConvParams& p, hipStream_t stream) {
    const int HP = (p.TP - 1) * p.stride + KS, HQ = (p.TQ - 1) * p.stride + KS;
    const size_t lds = (size_t)HP * HQ * RS_ROWB + (size_t)KS * KS * BN * RS_ROWB;
    static DeviceOnce attr;
    if (hipError_t e = set_max_dynamic_lds(attr, reinterpret_cast<const void*>(rs_conv_kernel<T, BN, KS, false>), RS_HALO_MAX + 9 * 64 * RS_ROWB)) return e;
    dim3 grid((unsigned)(p.B * p.ntp * p.ntq * (p.Cout / BN))), block(256);
    hipLaunchKernelGGL((rs_conv_kernel<T, BN, KS, false>), grid, block, lds, stream, p);
    return hipGetLastError();
}

template <typename T>
hipError_t rs_conv_t(const RsConvParams& p, hipStream_t stream) {
    if (p.Cout == 32) return p.ks == 3 ? rs_conv_launch<T, 32, 3>(p, stream) : rs_conv_launch<T, 32, 1>(p, stream);
    return p.ks == 3 ? rs_conv_launch<T, 64, 3>(p, stream) : rs_conv_launch<T, 64, 1>(p, stream);
}

// ---- stem: Conv2d(1, 32, 3, padding 1) + bias -> ReLU -> BatchNorm on the normalised (B, P, Q) fp32 input ------------------------
// One thread = one position x 8 channels (four threads per position write 16 / 32 consecutive bytes each); w tap-major [9][32].
// RAG (a pack: B counts its M frames and the P argument is not read): the frame's utterance from the level's utt table, the image's
// first frame and its P from row0, so the zero padding sits at each utterance's own first and last frame.
template <typename T, bool RAG>
__global__ __launch_bounds__(256) void rs_stem_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ scale, const float* __restrict__ shift, T* __restrict__ y,
                                                      int B, int P, int Q, const int* __restrict__ rag_row0, const int* __restrict__ rag_utt) {
    __shared__ float sw[9 * 32 + 3 * 32];
    for (int i = threadIdx.x; i < 9 * 32; i += 256) sw[i] = w[i];
    if (threadIdx.x < 32) {
        sw[288 + threadIdx.x] = bias[threadIdx.x];
        sw[320 + threadIdx.x] = scale[threadIdx.x];
        sw[352 + threadIdx.x] = shift[threadIdx.x];
    }
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t pos = idx >> 2;
    if (pos >= (int64_t)B * (RAG ? 1 : P) * Q) return;
    const int cg = (int)(idx & 3) * 8;
    const int q = (int)(pos % Q);
    const int64_t bp = pos / Q;                                // the frame: row b P + pp of the batch, row bp of a pack
    int pp;
    const float* __restrict__ xb;                              // the utterance's (P, Q) image
    if constexpr (RAG) {
        const int m = (int)bp;
        const int u = rag_utt[m];
        const int r0 = rag_row0[u];
        P = rag_row0[u + 1] - r0;
        pp = m - r0;
        xb = x + (int64_t)r0 * Q;
    } else {
        pp = (int)(bp % P);
        xb = x + (bp - pp) * Q;
    }
    float in[9];
#pragma unroll
    for (int dp = 0; dp < 3; ++dp)
#pragma unroll
        for (int dq = 0; dq < 3; ++dq) {
            const int ip = pp + dp - 1, iq = q + dq - 1;
            in[dp * 3 + dq] = (ip >= 0 && ip < P && iq >= 0 && iq < Q) ? xb[(int64_t)ip * Q + iq] : 0.0f;
        }
    T* __restrict__ yo = y + pos * 32 + cg;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = cg + k;
        float v = sw[288 + c];
#pragma unroll
        for (int t = 0; t < 9; ++t) v = fmaf(sw[t * 32 + c], in[t], v);
        v = v < 0.0f ? 0.0f : v;
        yo[k] = from_f32<T>(fmaf(v, sw[320 + c], sw[352 + c]));
    }
}

// ---- SE gate from the per-tile sums: gate[b, c] = sigmoid(W2 relu(W1 mean + b1) + b2), 16 hidden units ---------------------------
// One workgroup per utterance; the tiles are added in index order.  w1 [16][C], w2 [C][16], fp32.
// RAG (a pack): utterance b has its own tiles [rag_tile0[b], rag_tile0[b + 1]) and its own P_b Q positions (P_b from the level's row0).
template <bool RAG>
__global__ __launch_bounds__(256) void rs_se_gate_kernel(const float* __restrict__ part, int ntiles, int C, float inv_n, const float* __restrict__ w1,
                                                         const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                         float* __restrict__ gate, const int* __restrict__ rag_tile0, const int* __restrict__ rag_row0,
                                                         int Q) {
    __shared__ float mean[256], hid[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t tile_first;
    if constexpr (RAG) {
        tile_first = rag_tile0[b];
        ntiles = rag_tile0[b + 1] - (int)tile_first;
        inv_n = 1.0f / (float)((rag_row0[b + 1] - rag_row0[b]) * Q);
    } else {
        tile_first = (int64_t)b * ntiles;
    }
    if (tid < C) {
        const float* __restrict__ pp = part + tile_first * C + tid;
        float s = 0.0f;
        int t = 0;
        for (; t + 8 <= ntiles; t += 8) {          // eight loads in flight, added in index order (a 20 s file has 2500 tiles at level 0)
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = pp[(int64_t)(t + k) * C];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[k];
        }
        for (; t < ntiles; ++t) s += pp[(int64_t)t * C];
        mean[tid] = s * inv_n;
    }
    __syncthreads();
    for (int j = wave * 4; j < wave * 4 + 4; ++j) {
        float s = 0.0f;
        for (int c = lane; c < C; c += 64) s = fmaf(w1[j * C + c], mean[c], s);
        s = wave_sum(s) + b1[j];
        if (lane == 0) hid[j] = s < 0.0f ? 0.0f : s;
    }
    __syncthreads();
    if (tid < C) {
        float s = b2[tid];
#pragma unroll
        for (int j = 0; j < 16; ++j) s = fmaf(w2[tid * 16 + j], hid[j], s);
        gate[(int64_t)b * C + tid] = 1.0f / (1.0f + expf(-s));
    }
}

// ---- out = relu(res + y * gate[b, :]); res = relu(x) (the identity residual: the block's in-place ReLU has already overwritten x,
// ResNetBlocks.py:230-231) or the downsample output as it is ---------------------------------------------------------------------------
// RAG (a pack): per_utt_vec counts the vectors of one FRAME (Q C / N), and the gate row is that of the frame's utterance
template <typename T, bool RAG>
__global__ __launch_bounds__(256) void rs_se_apply_kernel(const T* __restrict__ y, const T* __restrict__ res, const float* __restrict__ gate,
                                                          T* __restrict__ out, int64_t nvec, int per_utt_vec, int cvec, int res_relu,
                                                          const int* __restrict__ rag_utt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    constexpr int N = Vec16<T>::N;
    int b = (int)(i / per_utt_vec);
    if constexpr (RAG) b = rag_utt[b];
    const int c0 = (int)(i % cvec) * N;
    const Vec16<T> yv = ld_nt(y + i * N), rv = ld_nt(res + i * N);
    const float* __restrict__ g = gate + (int64_t)b * cvec * N + c0;
    Vec16<T> o;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float r = rv.get(k);
        if (res_relu) r = r < 0.0f ? 0.0f : r;
        const float v = fmaf(yv.get(k), g[k], r);
        o.set(k, v < 0.0f ? 0.0f : v);
    }
    *reinterpret_cast<decltype(o.v)*>(out + i * N) = o.v;
}

// ---- the tile tables of a ragged pack's convolutions ---------------------------------------------------------------------------------
// tile0 / plan of one convolution of a pack from the input level's row0: thread u plans utterance u's output image (rs_tile_of, the
// function the host counts with), thread 0 adds the counts up in utterance order.  One workgroup; n > 256 runs in rounds of 256.
__global__ __launch_bounds__(256) void rs_rag_tiles_kernel(const int* __restrict__ row0_in, int n, int Q, int stride, int ks, int* __restrict__ tile0,
                                                           int* __restrict__ plan) {
    __shared__ int cnt[256];
    __shared__ int base;
    if (threadIdx.x == 0) base = 0;
    const int Qo = (Q - 1) / stride + 1;          // rs_out_size
    for (int u0 = 0; u0 < n; u0 += 256) {
        const int u = u0 + threadIdx.x;
        if (u < n) {
            const int Po = (row0_in[u + 1] - row0_in[u] - 1) / stride + 1;
            int TP, TQ;
            rs_tile_of(Po, Qo, stride, ks, TP, TQ);
            plan[u] = TP | TQ << 8;
            cnt[threadIdx.x] = ((Po + TP - 1) / TP) * ((Qo + TQ - 1) / TQ);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = base;
            const int m = min(256, n - u0);
            for (int i = 0; i < m; ++i) { tile0[u0 + i] = t; t += cnt[i]; }
            base = t;
            if (u0 + m == n) tile0[n] = t;
        }
        __syncthreads();
    }
}

template <typename T, int BN, int KS>
hipError_t rs_conv_rag_launch(const RsConvParams& p, const RsRagConv& r, hipStream_t stream) {
    const size_t lds = (size_t)r.halo_bytes + (size_t)KS * KS * BN * RS_ROWB;
    static DeviceOnce attr;
    if (hipError_t e = set_max_dynamic_lds(attr, reinterpret_cast<const void*>(rs_conv_kernel<T, BN, KS, true>), RS_HALO_MAX + 9 * 64 * RS_ROWB)) return e;
    dim3 grid((unsigned)((int64_t)r.ntiles * (p.Cout / BN))), block(256);
    hipLaunchKernelGGL((rs_conv_kernel<T, BN, KS, true>), grid, block, lds, stream, p);
    return hipGetLastError();
}

template <typename T>
hipError_t rs_conv_rag_t(const RsConvParams& p, const RsRagConv& r, hipStream_t stream) {
    if (p.Cout == 32) return p.ks == 3 ? rs_conv_rag_launch<T, 32, 3>(p, r, stream) : rs_conv_rag_launch<T, 32, 1>(p, r, stream);
    return p.ks == 3 ? rs_conv_rag_launch<T, 64, 3>(p, r, stream) : rs_conv_rag_launch<T, 64, 1>(p, r, stream);
}

}  // namespace

void rs_conv_plan(RsConvParams& p) {
    p.Po = rs_out_size(p.P, p.stride);
    p.Qo = rs_out_size(p.Q, p.stride);
    rs_tile_of(p.Po, p.Qo, p.stride, p.ks, p.TP, p.TQ);
    p.ntp = (p.Po + p.TP - 1) / p.TP;
    p.ntq = (p.Qo + p.TQ - 1) / p.TQ;
}

hipError_t launch_rs_conv(const RsConvParams& p, int dt, hipStream_t stream) {
    const int ck = dt == DT_F32 ? 16 : 32;
    if (dt != DT_F32 && dt != DT_BF16) return hipErrorInvalidValue;
    if (p.B <= 0 || p.P <= 0 || p.Q <= 0 || p.Cin <= 0 || p.Cin % ck != 0 || p.Cout <= 0 || p.Cout % 32 != 0 || (p.Cout != 32 && p.Cout % 64 != 0))
        return hipErrorInvalidValue;
    if ((p.ks != 3 && p.ks != 1) || (p.stride != 1 && p.stride != 2) || !p.X || !p.Y || !p.W || !p.scale || !p.shift) return hipErrorInvalidValue;
    if (p.Po != rs_out_size(p.P, p.stride) || p.Qo != rs_out_size(p.Q, p.stride) || p.TP < 1 || p.TQ < 1 || p.TP * p.TQ > 128 ||
        p.ntp != (p.Po + p.TP - 1) / p.TP || p.ntq != (p.Qo + p.TQ - 1) / p.TQ ||
        (int64_t)((p.TP - 1) * p.stride + p.ks) * ((p.TQ - 1) * p.stride + p.ks) * RS_ROWB > RS_HALO_MAX)
        return hipErrorInvalidValue;
    if ((int64_t)p.B * p.ntp * p.ntq * (p.Cout / 32) > 0x7fffffffLL) return hipErrorInvalidValue;
    return dt == DT_F32 ? rs_conv_t<float>(p, stream) : rs_conv_t<bf16_t>(p, stream);
}

hipError_t launch_rs_stem(const float* x, const float* w, const float* bias, const float* scale, const float* shift, void* y, int dt, int B, int P, int Q,
                          hipStream_t stream) {
    if (dt != DT_F32 && dt != DT_BF16) return hipErrorInvalidValue;
    const int64_t n = (int64_t)B * P * Q * 4;
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (dt == DT_F32) hipLaunchKernelGGL((rs_stem_kernel<float, false>), grid, block, 0, stream, x, w, bias, scale, shift, (float*)y, B, P, Q, nullptr, nullptr);
    else hipLaunchKernelGGL((rs_stem_kernel<bf16_t, false>), grid, block, 0, stream, x, w, bias, scale, shift, (bf16_t*)y, B, P, Q, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_rs_se_gate(const float* part, int ntiles, int B, int C, int positions, const float* w1, const float* b1, const float* w2, const float* b2,
                             float* gate, hipStream_t stream) {
    if (C > 256 || C % 32 != 0 || ntiles <= 0 || positions <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rs_se_gate_kernel<false>, dim3(B), dim3(256), 0, stream, part, ntiles, C, 1.0f / (float)positions, w1, b1, w2, b2, gate, nullptr, nullptr, 0);
    return hipGetLastError();
}

hipError_t launch_rs_se_apply(const void* y, const void* res, const float* gate, void* out, int dt, int B, int positions, int C, bool res_relu,
                              hipStream_t stream) {
    if (dt != DT_F32 && dt != DT_BF16) return hipErrorInvalidValue;
    const int nv = dt == DT_F32 ? 4 : 8;
    if (C % nv != 0) return hipErrorInvalidValue;
    const int cvec = C / nv;
    const int64_t per = (int64_t)positions * cvec, nvec = per * B;
    if (per > 0x7fffffffLL) return hipErrorInvalidValue;
    dim3 grid((unsigned)((nvec + 255) / 256)), block(256);
    if (dt == DT_F32)
        hipLaunchKernelGGL((rs_se_apply_kernel<float, false>), grid, block, 0, stream, (const float*)y, (const float*)res, gate, (float*)out, nvec, (int)per, cvec,
                           res_relu ? 1 : 0, nullptr);
    else
        hipLaunchKernelGGL((rs_se_apply_kernel<bf16_t, false>), grid, block, 0, stream, (const bf16_t*)y, (const bf16_t*)res, gate, (bf16_t*)out, nvec, (int)per, cvec,
                           res_relu ? 1 : 0, nullptr);
    return hipGetLastError();
}

// ---- ragged packs ----------------------------------------------------------------------------------------------------------------
void rs_rag_tiles_host(const int* hrow0_in, int n, int Q, int stride, int ks, int* ntiles, int* halo_bytes) {
    const int Qo = rs_out_size(Q, stride);
    int64_t tiles = 0;
    int halo = 0;
    for (int u = 0; u < n; ++u) {
        const int Po = rs_out_size(hrow0_in[u + 1] - hrow0_in[u], stride);
        int TP, TQ;
        rs_tile_of(Po, Qo, stride, ks, TP, TQ);
        tiles += (int64_t)((Po + TP - 1) / TP) * ((Qo + TQ - 1) / TQ);
        const int hb = ((TP - 1) * stride + ks) * ((TQ - 1) * stride + ks) * RS_ROWB;
        if (hb > halo) halo = hb;
    }
    *ntiles = tiles > 0x7fffffffLL ? -1 : (int)tiles;
    *halo_bytes = halo;
}

hipError_t launch_rs_rag_tiles(const int* row0_in, int n, int Q, int stride, int ks, int* tile0, int* plan, hipStream_t stream) {
    if (!row0_in || !tile0 || !plan || n <= 0 || Q <= 0 || (stride != 1 && stride != 2) || (ks != 3 && ks != 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rs_rag_tiles_kernel, dim3(1), dim3(256), 0, stream, row0_in, n, Q, stride, ks, tile0, plan);
    return hipGetLastError();
}

hipError_t launch_rs_conv_ragged(RsConvParams p, const RsRagConv& r, int dt, hipStream_t stream) {
    const int ck = dt == DT_F32 ? 16 : 32;
    if (dt != DT_F32 && dt != DT_BF16) return hipErrorInvalidValue;
    if (p.Q <= 0 || p.Cin <= 0 || p.Cin % ck != 0 || p.Cout <= 0 || p.Cout % 32 != 0 || (p.Cout != 32 && p.Cout % 64 != 0)) return hipErrorInvalidValue;
    if ((p.ks != 3 && p.ks != 1) || (p.stride != 1 && p.stride != 2) || !p.X || !p.Y || !p.W || !p.scale || !p.shift) return hipErrorInvalidValue;
    if (!r.row0_in || !r.row0_out || !r.tile0 || !r.plan || r.n <= 0 || r.ntiles <= 0 || r.halo_bytes <= 0 || r.halo_bytes > RS_HALO_MAX)
        return hipErrorInvalidValue;
    if ((int64_t)r.ntiles * (p.Cout / 32) > 0x7fffffffLL) return hipErrorInvalidValue;
    p.Qo = rs_out_size(p.Q, p.stride);
    p.rag = r;
    return dt == DT_F32 ? rs_conv_rag_t<float>(p, r, stream) : rs_conv_rag_t<bf16_t>(p, r, stream);
}

hipError_t launch_rs_stem_ragged(const float* x, const float* w, const float* bias, const float* scale, const float* shift, void* y, int dt,
                                 const int* row0, const int* utt, int M, int Q, hipStream_t stream) {
    if ((dt != DT_F32 && dt != DT_BF16) || !row0 || !utt || M <= 0 || Q <= 0) return hipErrorInvalidValue;
    const int64_t n = (int64_t)M * Q * 4;
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (dt == DT_F32) hipLaunchKernelGGL((rs_stem_kernel<float, true>), grid, block, 0, stream, x, w, bias, scale, shift, (float*)y, M, 0, Q, row0, utt);
    else hipLaunchKernelGGL((rs_stem_kernel<bf16_t, true>), grid, block, 0, stream, x, w, bias, scale, shift, (bf16_t*)y, M, 0, Q, row0, utt);
    return hipGetLastError();
}

hipError_t launch_rs_se_gate_ragged(const float* part, const int* tile0, const int* row0, int n, int C, int Q, const float* w1, const float* b1,
                                    const float* w2, const float* b2, float* gate, hipStream_t stream) {
    if (C > 256 || C % 32 != 0 || n <= 0 || Q <= 0 || !part || !tile0 || !row0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rs_se_gate_kernel<true>, dim3(n), dim3(256), 0, stream, part, 0, C, 0.0f, w1, b1, w2, b2, gate, tile0, row0, Q);
    return hipGetLastError();
}

hipError_t launch_rs_se_apply_ragged(const void* y, const void* res, const float* gate, void* out, int dt, const int* utt, int M, int Q, int C,
                                     bool res_relu, hipStream_t stream) {
    if ((dt != DT_F32 && dt != DT_BF16) || !utt || M <= 0 || Q <= 0) return hipErrorInvalidValue;
    const int nv = dt == DT_F32 ? 4 : 8;
    if (C % nv != 0) return hipErrorInvalidValue;
    const int cvec = C / nv;
    const int64_t per = (int64_t)Q * cvec, nvec = per * M;
    if (per > 0x7fffffffLL) return hipErrorInvalidValue;
    dim3 grid((unsigned)((nvec + 255) / 256)), block(256);
    if (dt == DT_F32)
        hipLaunchKernelGGL((rs_se_apply_kernel<float, true>), grid, block, 0, stream, (const float*)y, (const float*)res, gate, (float*)out, nvec, (int)per, cvec,
                           res_relu ? 1 : 0, utt);
    else
        hipLaunchKernelGGL((rs_se_apply_kernel<bf16_t, true>), grid, block, 0, stream, (const bf16_t*)y, (const bf16_t*)res, gate, (bf16_t*)out, nvec, (int)per,
                           cvec, res_relu ? 1 : 0, utt);
    return hipGetLastError();
}

}  // namespace svhip
