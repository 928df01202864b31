// conformer.hip — the Conformer encoder's own kernels (reference models/Conformer.py, models/conformer/conformer/*.py).
//
// Activations are frame-major (B T', C): the rows of B utterances stacked, d_model = 256.  Nothing here reads across utterances:
// every kernel's rows, taps and keys stay inside one utterance.
//
//   cf_conv1    Conv2d(1 -> 256, 3 x 3, stride 2) + ReLU of Conv2dSubampling on the (T, F) mel image of each utterance: out
//               (B, T1, F1, 256), channel-contiguous, so that conv2's operand row (b, t, f) is three contiguous 768-element runs
//               (conv1 rows (b, 2t + dt, 2f .. 2f + 2), dt = 0 .. 2) — the segmented row gather of the generic GEMM (gemm.hip)
//   cf_ln       LayerNorm(256) of every row (fp32 statistics, eps 1e-5); optionally a second LayerNorm of the (stored) first
//               output in the same pass: a block's final LayerNorm and the next block's feed-forward LayerNorm
//   cf_glu_dw   the convolution module's middle: GLU of the pointwise-conv output (B T', 512), depthwise conv k = 15 with zero
//               padding at each utterance's edges, the BatchNorm folded into the taps, Swish
//   cf_attn     multi-head self-attention with Transformer-XL relative positions, reproducing the reference's _relative_shift
//               (attention.py:110-118) exactly; see the kernel's comment
#include "kernels.h"

namespace svhip {

namespace {

template <typename T> struct V4;
template <> struct V4<float> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};
template <> struct V4<bf16_t> {
    typedef bf16_t bf16x4_ __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[4]) {
        const bf16x4_ a = *reinterpret_cast<const bf16x4_*>(p);
        v[0] = (float)a[0]; v[1] = (float)a[1]; v[2] = (float)a[2]; v[3] = (float)a[3];
    }
    static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[4]) {
        bf16x4_ a;
        a[0] = (bf16_t)v[0]; a[1] = (bf16_t)v[1]; a[2] = (bf16_t)v[2]; a[3] = (bf16_t)v[3];
        *reinterpret_cast<bf16x4_*>(p) = a;
    }
};

constexpr int CF_D = 256;         // d_model

// ---- cf_conv1: one thread per (b, t1, f1, 4 channels); 9 taps in the order (dt, df) row-major, bias first, then ReLU ----------------
// one output position: xp = the top-left input value of its 3 x 3 window (input rows F apart), yp = its 256 channels
template <typename T>
__device__ __forceinline__ void cf_conv1_point(const T* __restrict__ xp, int F, const float* __restrict__ w, const float* __restrict__ bias,
                                               T* __restrict__ yp, int c0) {
    float acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = bias[c0 + e];
#pragma unroll
    for (int dt = 0; dt < 3; ++dt)
#pragma unroll
        for (int df = 0; df < 3; ++df) {
            const float xv = to_f32<T>(xp[(int64_t)dt * F + df]);
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (dt * 3 + df) * CF_D + c0);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(wv[e], xv, acc[e]);
        }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = fmaxf(acc[e], 0.0f);
    V4<T>::store(yp + c0, acc);
}

template <typename T>
__global__ __launch_bounds__(256) void cf_conv1_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       T* __restrict__ y, int B, int Tn, int F, int T1, int F1) {
    const int64_t total = (int64_t)B * T1 * F1 * (CF_D / 4);
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int c0 = (int)(g % (CF_D / 4)) * 4;
        const int64_t pos = g / (CF_D / 4);
        const int f1 = (int)(pos % F1);
        const int64_t bt = pos / F1;
        const int t1 = (int)(bt % T1);
        const int b = (int)(bt / T1);
        cf_conv1_point<T>(x + ((int64_t)b * Tn + 2 * t1) * F + 2 * f1, F, w, bias, y + pos * CF_D, c0);
    }
}

// The same over a pack, grid (x, utterances of the slice): utterance u = u0 + blockIdx.y reads its mel rows mel0[u] .. of x and writes
// only the 2 T'_u + 1 conv1 rows that conv2 reads (T'_u = row0[u + 1] - row0[u]), at conv1 row 2 (row0[u] - row0[u0]) + (u - u0) of y
template <typename T>
__global__ __launch_bounds__(256) void cf_conv1_rag_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                           T* __restrict__ y, const int* __restrict__ mel0, const int* __restrict__ row0, int u0,
                                                           int F, int F1) {
    const int u = u0 + blockIdx.y;
    const int r0 = row0[u], rows = 2 * (row0[u + 1] - r0) + 1;
    const int64_t total = (int64_t)rows * F1 * (CF_D / 4);
    const int64_t out0 = 2 * (int64_t)(r0 - row0[u0]) + (u - u0);
    const T* __restrict__ xu = x + (int64_t)mel0[u] * F;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int c0 = (int)(g % (CF_D / 4)) * 4;
        const int64_t pos = g / (CF_D / 4);
        const int f1 = (int)(pos % F1);
        const int t1 = (int)(pos / F1);
        cf_conv1_point<T>(xu + (int64_t)(2 * t1) * F + 2 * f1, F, w, bias, y + (out0 * F1 + pos) * CF_D, c0);
    }
}

// ---- cf_ln: one wave per row (4 channels per lane), two-pass statistics in fp32 -----------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void ln4(float (&v)[4], const float* __restrict__ g, const float* __restrict__ b, int c0) {
    const float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.0f / CF_D);
    float d[4], s = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { d[e] = v[e] - mean; s = fmaf(d[e], d[e], s); }
    const float var = wave_sum(s) * (1.0f / CF_D);
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + c0), bv = *reinterpret_cast<const f32x4*>(b + c0);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(d[e] * rstd, gv[e], bv[e]);
}

template <typename T>
__global__ __launch_bounds__(256) void cf_ln_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ g1, const float* __restrict__ b1,
                                                    T* __restrict__ y2, const float* __restrict__ g2, const float* __restrict__ b2, int64_t M) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int c0 = (threadIdx.x & 63) * 4;
    float v[4];
    V4<T>::load(x + row * CF_D + c0, v);
    ln4(v, g1, b1, c0);
    V4<T>::store(y + row * CF_D + c0, v);
    if (y2) {
        // the second LayerNorm reads the first one's output as it was stored (rounded to T)
        T r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { r[e] = from_f32<T>(v[e]); v[e] = to_f32<T>(r[e]); }
        ln4(v, g2, b2, c0);
        V4<T>::store(y2 + row * CF_D + c0, v);
    }
}

// ---- cf_glu_dw: one thread per (utterance, tile of 16 frames, 4 channels) ---------------------------------------------------------
// g(t) = u(t, c) * sigmoid(u(t, 256 + c)) on the 16 + 14 rows the tile needs (zero outside [0, T') of the utterance), then
// y = swish(b' + sum_j w'_j g(t - 7 + j)) with the taps added in the order j = 0 .. 14 (BatchNorm folded: w' = s w, b' = shift)
constexpr int GDW_TT = 16, GDW_K = 15, GDW_R = 7;

// RAG (a pack, grid (x, n)): utterance blockIdx.y owns the rows [rag_row0[b], rag_row0[b + 1]); the tile and its halo are zero outside them
template <typename T, bool RAG>
__global__ __launch_bounds__(256) void cf_glu_dw_kernel(const T* __restrict__ u, const float* __restrict__ w, const float* __restrict__ bias,
                                                        T* __restrict__ y, int B, int Tn, const int* __restrict__ rag_row0) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c0 = (int)(g % (CF_D / 4)) * 4;
    const int64_t q = g / (CF_D / 4);
    int b, t0;
    int64_t row0;
    if (RAG) {
        b = blockIdx.y;
        row0 = rag_row0[b];
        Tn = rag_row0[b + 1] - (int)row0;
        if (q >= (Tn + GDW_TT - 1) / GDW_TT) return;
        t0 = (int)q * GDW_TT;
    } else {
        const int ntile = (Tn + GDW_TT - 1) / GDW_TT;
        if (q >= (int64_t)B * ntile) return;
        b = (int)(q / ntile);
        t0 = (int)(q - (int64_t)b * ntile) * GDW_TT;
        row0 = (int64_t)b * Tn;
    }
    float acc[GDW_TT][4];
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + c0);
#pragma unroll
    for (int o = 0; o < GDW_TT; ++o)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[o][e] = bv[e];
#pragma unroll
    for (int i = 0; i < GDW_TT + GDW_K - 1; ++i) {
        const int t = t0 - GDW_R + i;
        float gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (t >= 0 && t < Tn) {
            float a[4], s[4];
            V4<T>::load(u + (row0 + t) * (2 * CF_D) + c0, a);
            V4<T>::load(u + (row0 + t) * (2 * CF_D) + CF_D + c0, s);
#pragma unroll
            for (int e = 0; e < 4; ++e) gv[e] = a[e] * (1.0f / (1.0f + expf(-s[e])));
        }
#pragma unroll
        for (int o = 0; o < GDW_TT; ++o) {
            const int j = i - o;
            if (j >= 0 && j < GDW_K) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w + j * CF_D + c0);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[o][e] = fmaf(wv[e], gv[e], acc[o][e]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < GDW_TT; ++o) {
        const int t = t0 + o;
        if (t < Tn) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[o][e] / (1.0f + expf(-acc[o][e]));
            V4<T>::store(y + (row0 + t) * CF_D + c0, v);
        }
    }
}

// ---- cf_attn ------------------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per (tile of 64 queries, head, utterance); wave w owns queries i0 + 16 w .. + 15 and walks the keys in
// tiles of AK = 64 with an online softmax, so any T' works.  For query i and key j (d = j - i), with q' = q + u and q'' = q + v
// (per-head biases) and p_c = row c of P = pe[:T'] W_pos^T:
//   content = q'_i . k_j
//   pos     = q''_i . p_{T'-1+d}          d <= 0
//             0                           d == 1
//             q''_{i+1} . p_{d-2}          d >= 2   (the NEXT query row: the reference's cat / view shift)
//   score   = (content + pos) / 16        (sqrt(d_model) = 16, attention.py:62,98)
// Every product is an MFMA (16 x 16 tiles: v_mfma_f32_16x16x4_f32 on fp32 handles, v_mfma_f32_16x16x32_bf16 on bf16 handles, whose
// operands — q', q'', k, v, the band of P and the probabilities — are staged in bf16):
//   S = Q' K^T                    (16 x 64 per wave)
//   G0 = Q''_{rows i} B^T, G1 = Q''_{rows i+1} B^T   over the band B of 80 rows of P the wave's (query, key) pairs touch: band row n
//                                 serves d = j0 - i_w - 15 + n and holds p_{T'-1+d}, zero (d = 1) or p_{d-2}
//   pos(i, j) = (d >= 2 ? G1 : G0)[i][d - (j0 - i_w - 15)]   read back along the shifted diagonal from LDS
//   O += softmax-weights V        (the weights through LDS into the A-operand layout)
// Scores and the softmax are fp32; keys past T' score -inf; rows past T' are computed from zero queries and not written.
//
// RAG, a pack of n utterances laid out back to back (row0: n + 1 device ints): the grid is (ceil(max T' / 64), 4, n) and a workgroup
// takes its first row and its T' from row0[blockIdx.z]; a query tile past its utterance's end leaves at once (the test is uniform over
// the workgroup and comes before the first barrier).  Everything else is the fixed kernel: every operand load — q' and q'' (row i + 1
// included), k, v, the band of P — is already masked by T' where it is loaded, so the rows behind an utterance's end, which in a pack
// are the next utterance's, never enter a product (a weight of 0 would not stop a NaN); P is read from row 0 for every utterance.
// The plain grid was chosen over a device-built tile table: an idle workgroup costs one table read, and the whole-file packs this
// serves (2 - 20 s files, T' within a factor of ten) leave at most as many idle tiles as working ones, against a second launch and a
// prefix sum per block for the table.  LDS footprint and MFMA operand layouts are those of the fixed kernel (one body).
constexpr int AQ = 64, AK = 64, DH = 64, NBAND = AQ + AK, GW = 80, LDG = GW + 1;

template <typename E> struct AttnMma;
template <> struct AttnMma<float> {
    static constexpr int KS = 4, LDE = DH + 1;
    typedef float frag;
    // A[row][k] (or B^T[col][k]) row-major with row stride ld: lane l takes row l & 15, k = kk + (l >> 4)
    static __device__ __forceinline__ frag load(const float* p, int ld, int row0, int kk, int lane) {
        return p[(row0 + (lane & 15)) * ld + kk + (lane >> 4)];
    }
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};
template <> struct AttnMma<bf16_t> {
    static constexpr int KS = 32, LDE = DH + 8;          // (rows of 144 bytes: 16-byte fragments, spread over the banks)
    typedef bf16x8 frag;
    // lane l takes row l & 15, k = kk + 8 (l >> 4) .. + 7
    static __device__ __forceinline__ frag load(const bf16_t* p, int ld, int row0, int kk, int lane) {
        return *reinterpret_cast<const bf16x8*>(p + (row0 + (lane & 15)) * ld + kk + 8 * (lane >> 4));
    }
    static __device__ __forceinline__ f32x4 mma(const frag& a, const frag& b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

template <typename T>
constexpr size_t attn_lds_bytes() {
    return (size_t)(AQ + (AQ + 1) + AK + DH + NBAND) * AttnMma<T>::LDE * sizeof(T) + (size_t)4 * 2 * 16 * LDG * sizeof(float);
}

template <typename T, bool RAG>
__global__ __launch_bounds__(256) void cf_attn_kernel(const T* __restrict__ qkv, int ldq, const float* __restrict__ P, int ldp,
                                                      const float* __restrict__ ub, const float* __restrict__ vb, T* __restrict__ ctx,
                                                      int ldc, int Tn, const int* __restrict__ rag_row0) {
    typedef AttnMma<T> M;
    constexpr int LDE = M::LDE, KS = M::KS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* sQu = reinterpret_cast<T*>(smem);           // AQ x LDE          q + u
    T* sQv = sQu + AQ * LDE;                       // (AQ + 1) x LDE    q + v (rows i0 .. i0 + AQ; zero past T')
    T* sK = sQv + (AQ + 1) * LDE;                  // AK x LDE          keys
    T* sVt = sK + AK * LDE;                        // DH x LDE          values transposed: [dim][key]
    T* sB = sVt + DH * LDE;                        // NBAND x LDE       the workgroup's band of P
    float* sG = reinterpret_cast<float*>(sB + NBAND * LDE);       // per wave: [G0 | G1] 2 x 16 x LDG; then the wave's weights
    const int hh = blockIdx.y, b = blockIdx.z;
    const int i0 = blockIdx.x * AQ;
    int64_t rb;
    if (RAG) {
        rb = rag_row0[b];
        Tn = rag_row0[b + 1] - (int)rb;
        if (i0 >= Tn) return;
    } else {
        rb = (int64_t)b * Tn;
    }
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int qcol = hh * DH, kcol = CF_D + hh * DH, vcol = 2 * CF_D + hh * DH;
    float* gw = sG + w * (2 * 16 * LDG);
    T* pw = reinterpret_cast<T*>(gw);               // 16 x LDE weights (after G has been read)

    for (int e = tid; e < (AQ + 1) * DH; e += 256) {
        const int rr = e / DH, dd = e - rr * DH, i = i0 + rr;
        const float q = i < Tn ? to_f32<T>(qkv[(rb + i) * ldq + qcol + dd]) : 0.0f;
        if (rr < AQ) sQu[rr * LDE + dd] = from_f32<T>(q + ub[qcol + dd]);
        sQv[rr * LDE + dd] = from_f32<T>(i < Tn ? q + vb[qcol + dd] : 0.0f);
    }
    const int cl = lane & 15, rg = (lane >> 4) * 4;   // accumulator element e of a 16 x 16 tile: row rg + e, column cl
    const int ib = i0 + 16 * w;
    float m[4], lsum[4];
    f32x4 O[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { m[e] = -INFINITY; lsum[e] = 0.0f; O[e] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
    for (int j0 = 0; j0 < Tn; j0 += AK) {
        __syncthreads();                           // (the previous tile's K / V / band / weights are consumed)
        for (int e = tid; e < AK * DH; e += 256) {
            const int jj = e / DH, dd = e - jj * DH, j = j0 + jj;
            const bool ok = j < Tn;
            sK[jj * LDE + dd] = ok ? qkv[(rb + j) * ldq + kcol + dd] : from_f32<T>(0.0f);
            sVt[dd * LDE + jj] = ok ? qkv[(rb + j) * ldq + vcol + dd] : from_f32<T>(0.0f);
        }
        const int dmin = j0 - i0 - (AQ - 1);       // band row nb serves d = dmin + nb
        for (int e = tid; e < NBAND * DH; e += 256) {
            const int nb = e / DH, dd = e - nb * DH, d = dmin + nb;
            const int prow = d <= 0 ? Tn - 1 + d : (d >= 2 ? d - 2 : -1);
            sB[nb * LDE + dd] = from_f32<T>((prow >= 0 && prow < Tn) ? P[(int64_t)prow * ldp + qcol + dd] : 0.0f);
        }
        __syncthreads();
        // content scores and the two band products of this wave
        f32x4 S[4], G[2][5];
#pragma unroll
        for (int s = 0; s < 4; ++s) S[s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 5; ++t) G[0][t] = G[1][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const int nb0 = (AQ - 16) - 16 * w;        // the wave's band starts at d = j0 - ib - 15
#pragma unroll
        for (int kk = 0; kk < DH; kk += KS) {
            const typename M::frag qa = M::load(sQu, LDE, 16 * w, kk, lane);
            const typename M::frag v0 = M::load(sQv, LDE, 16 * w, kk, lane);
            const typename M::frag v1 = M::load(sQv, LDE, 16 * w + 1, kk, lane);
#pragma unroll
            for (int s = 0; s < 4; ++s) S[s] = M::mma(qa, M::load(sK, LDE, 16 * s, kk, lane), S[s]);
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const typename M::frag bb = M::load(sB, LDE, nb0 + 16 * t, kk, lane);
                G[0][t] = M::mma(v0, bb, G[0][t]);
                G[1][t] = M::mma(v1, bb, G[1][t]);
            }
        }
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int t = 0; t < 5; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) gw[(g * 16 + rg + e) * LDG + 16 * t + cl] = G[g][t][e];
        __syncthreads();
        // scores along the shifted diagonal, the online softmax per row (a row lives in the 16 lanes of one lane group)
        float sc[4][4], mx[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mx[e] = -INFINITY;
            const int r = rg + e;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int j = j0 + 16 * s + cl, d = j - (ib + r), n = 16 * s + cl - r + 15;
                const float pos = gw[((d >= 2 ? 16 : 0) + r) * LDG + n];
                sc[s][e] = j < Tn ? (S[s][e] + pos) * 0.0625f : -INFINITY;
                mx[e] = fmaxf(mx[e], sc[s][e]);
            }
        }
        float alpha[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) mx[e] = fmaxf(mx[e], __shfl_xor(mx[e], o, 64));
            const float mn = fmaxf(m[e], mx[e]);
            alpha[e] = expf(m[e] - mn);            // (0 on the first tile: m = -inf)
            m[e] = mn;
            float ps = 0.0f;
#pragma unroll
            for (int s = 0; s < 4; ++s) { sc[s][e] = expf(sc[s][e] - mn); ps += sc[s][e]; }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) ps += __shfl_xor(ps, o, 64);
            lsum[e] = fmaf(lsum[e], alpha[e], ps);
        }
        __syncthreads();                           // (every lane has read G before the weights overwrite it)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) pw[(rg + e) * LDE + 16 * s + cl] = from_f32<T>(sc[s][e]);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int e = 0; e < 4; ++e) O[t][e] *= alpha[e];
#pragma unroll
            for (int kk = 0; kk < AK; kk += KS) O[t] = M::mma(M::load(pw, LDE, 0, kk, lane), M::load(sVt, LDE, 16 * t, kk, lane), O[t]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = ib + rg + e;
        if (i < Tn) {
            const float inv = 1.0f / lsum[e];
#pragma unroll
            for (int t = 0; t < 4; ++t) ctx[(rb + i) * ldc + hh * DH + 16 * t + cl] = from_f32<T>(O[t][e] * inv);
        }
    }
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
unsigned grid_of(int64_t threads) {
    const int64_t g = (threads + 255) / 256;
    return (unsigned)(g > 65536 ? 65536 : g);
}

}  // namespace

hipError_t launch_cf_conv1(const void* x, const float* w, const float* bias, void* y, int dt, int B, int Tn, int F, hipStream_t stream) {
    const int T1 = (Tn - 3) / 2 + 1, F1 = (F - 3) / 2 + 1;
    if (!x || !w || !bias || !y || B <= 0 || Tn < 3 || F < 3 || (dt != DT_F32 && dt != DT_BF16)) return hipErrorInvalidValue;
    if (!al16(w) || !al16(bias) || !al16(y)) return hipErrorInvalidValue;
    const unsigned g = grid_of((int64_t)B * T1 * F1 * (CF_D / 4));
    if (dt == DT_BF16) hipLaunchKernelGGL(cf_conv1_kernel<bf16_t>, dim3(g), dim3(256), 0, stream, (const bf16_t*)x, w, bias, (bf16_t*)y, B, Tn, F, T1, F1);
    else hipLaunchKernelGGL(cf_conv1_kernel<float>, dim3(g), dim3(256), 0, stream, (const float*)x, w, bias, (float*)y, B, Tn, F, T1, F1);
    return hipGetLastError();
}

hipError_t launch_cf_conv1_ragged(const void* x, const float* w, const float* bias, void* y, int dt, const int* mel0, const int* row0, int u0,
                                  int n, int max_T_sub, int F, hipStream_t stream) {
    const int F1 = (F - 3) / 2 + 1;
    if (!x || !w || !bias || !y || !mel0 || !row0 || u0 < 0 || n <= 0 || n > 65535 || max_T_sub <= 0 || F < 3 || (dt != DT_F32 && dt != DT_BF16))
        return hipErrorInvalidValue;
    if (!al16(w) || !al16(bias) || !al16(y)) return hipErrorInvalidValue;
    const dim3 grid(grid_of((int64_t)(2 * max_T_sub + 1) * F1 * (CF_D / 4)), (unsigned)n);
    if (dt == DT_BF16)
        hipLaunchKernelGGL(cf_conv1_rag_kernel<bf16_t>, grid, dim3(256), 0, stream, (const bf16_t*)x, w, bias, (bf16_t*)y, mel0, row0, u0, F, F1);
    else hipLaunchKernelGGL(cf_conv1_rag_kernel<float>, grid, dim3(256), 0, stream, (const float*)x, w, bias, (float*)y, mel0, row0, u0, F, F1);
    return hipGetLastError();
}

hipError_t launch_cf_ln(const void* x, void* y, const float* g1, const float* b1, void* y2, const float* g2, const float* b2, int dt, int64_t M,
                        hipStream_t stream) {
    if (!x || !y || !g1 || !b1 || M <= 0 || (y2 && (!g2 || !b2)) || (dt != DT_F32 && dt != DT_BF16)) return hipErrorInvalidValue;
    if (!al16(x) || !al16(y) || !al16(g1) || !al16(b1) || (y2 && (!al16(y2) || !al16(g2) || !al16(b2)))) return hipErrorInvalidValue;
    const int64_t blocks = (M + 3) / 4;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    if (dt == DT_BF16)
        hipLaunchKernelGGL(cf_ln_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)y, g1, b1, (bf16_t*)y2, g2, b2, M);
    else hipLaunchKernelGGL(cf_ln_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, stream, (const float*)x, (float*)y, g1, b1, (float*)y2, g2, b2, M);
    return hipGetLastError();
}

hipError_t launch_cf_glu_dw(const void* u, const float* w, const float* bias, void* y, int dt, int B, int Tn, hipStream_t stream) {
    if (!u || !w || !bias || !y || B <= 0 || Tn <= 0 || (dt != DT_F32 && dt != DT_BF16)) return hipErrorInvalidValue;
    if (!al16(u) || !al16(w) || !al16(bias) || !al16(y)) return hipErrorInvalidValue;
    const int64_t threads = (int64_t)B * ((Tn + GDW_TT - 1) / GDW_TT) * (CF_D / 4);
    if (threads >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (dt == DT_BF16)
        hipLaunchKernelGGL((cf_glu_dw_kernel<bf16_t, false>), grid, dim3(256), 0, stream, (const bf16_t*)u, w, bias, (bf16_t*)y, B, Tn, nullptr);
    else hipLaunchKernelGGL((cf_glu_dw_kernel<float, false>), grid, dim3(256), 0, stream, (const float*)u, w, bias, (float*)y, B, Tn, nullptr);
    return hipGetLastError();
}

hipError_t launch_cf_glu_dw_ragged(const void* u, const float* w, const float* bias, void* y, int dt, const int* row0, int n, int max_T_sub,
                                   hipStream_t stream) {
    if (!u || !w || !bias || !y || !row0 || n <= 0 || n > 65535 || max_T_sub <= 0 || (dt != DT_F32 && dt != DT_BF16)) return hipErrorInvalidValue;
    if (!al16(u) || !al16(w) || !al16(bias) || !al16(y)) return hipErrorInvalidValue;
    const int64_t threads = (int64_t)((max_T_sub + GDW_TT - 1) / GDW_TT) * (CF_D / 4);
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)n);
    if (dt == DT_BF16)
        hipLaunchKernelGGL((cf_glu_dw_kernel<bf16_t, true>), grid, dim3(256), 0, stream, (const bf16_t*)u, w, bias, (bf16_t*)y, n, 0, row0);
    else hipLaunchKernelGGL((cf_glu_dw_kernel<float, true>), grid, dim3(256), 0, stream, (const float*)u, w, bias, (float*)y, n, 0, row0);
    return hipGetLastError();
}

namespace {

template <typename T, bool RAG>
hipError_t attn_launch(const void* qkv, int ldq, const float* P, int ldp, const float* u_bias, const float* v_bias, void* ctx, int ldc, int B, int Tn,
                       const int* row0, hipStream_t stream) {
    const size_t lds = attn_lds_bytes<T>();
    const dim3 grid((unsigned)((Tn + AQ - 1) / AQ), CF_D / DH, (unsigned)B);
    static DeviceOnce attr;
    if (hipError_t e = set_max_dynamic_lds(attr, reinterpret_cast<const void*>(cf_attn_kernel<T, RAG>), (int)lds)) return e;
    hipLaunchKernelGGL((cf_attn_kernel<T, RAG>), grid, dim3(256), lds, stream, (const T*)qkv, ldq, P, ldp, u_bias, v_bias, (T*)ctx, ldc, Tn, row0);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_cf_attn(const void* qkv, int ldq, const float* P, int ldp, const float* u_bias, const float* v_bias, void* ctx, int ldc, int dt,
                          int B, int Tn, hipStream_t stream) {
    if (!qkv || !P || !u_bias || !v_bias || !ctx || B <= 0 || B > 65535 || Tn <= 0 || (dt != DT_F32 && dt != DT_BF16)) return hipErrorInvalidValue;
    if (ldq < 3 * CF_D || ldp < CF_D || ldc < CF_D) return hipErrorInvalidValue;
    if (dt == DT_BF16) return attn_launch<bf16_t, false>(qkv, ldq, P, ldp, u_bias, v_bias, ctx, ldc, B, Tn, nullptr, stream);
    return attn_launch<float, false>(qkv, ldq, P, ldp, u_bias, v_bias, ctx, ldc, B, Tn, nullptr, stream);
}

hipError_t launch_cf_attn_ragged(const void* qkv, int ldq, const float* P, int ldp, const float* u_bias, const float* v_bias, void* ctx, int ldc,
                                 int dt, const int* row0, int n, int max_T_sub, hipStream_t stream) {
    if (!qkv || !P || !u_bias || !v_bias || !ctx || !row0 || n <= 0 || n > 65535 || max_T_sub <= 0 || (dt != DT_F32 && dt != DT_BF16))
        return hipErrorInvalidValue;
    if (ldq < 3 * CF_D || ldp < CF_D || ldc < CF_D) return hipErrorInvalidValue;
    if (dt == DT_BF16) return attn_launch<bf16_t, true>(qkv, ldq, P, ldp, u_bias, v_bias, ctx, ldc, n, max_T_sub, row0, stream);
    return attn_launch<float, true>(qkv, ldq, P, ldp, u_bias, v_bias, ctx, ldc, n, max_T_sub, row0, stream);
}

}  // namespace svhip
