// titanet.hip — TitaNet's depthwise time-context path (reference models/TitaNet.py:253-318, blocks/titanet_blocks.py:47-97).
//
// Activations are frame-major (B T, C): the rows of B utterances stacked — or, in a ragged pack, n utterances of T_u rows each, back to
// back, utterance u owning the rows [row0[u], row0[u + 1]) of a device table (the *_ragged forms).
// Both kernels walk a tile of TT frames of ONE utterance for
// one 16-byte vector of channels per thread (4 fp32 / 8 bf16): the TT + K - 1 input rows the tile needs are loaded into registers
// first (every load of the thread in flight at once), rows outside [0, T) of the utterance are zero — the "same" zero padding of
// Conv1dSamePadding at each utterance's own edges, so a tap never reads a neighbouring utterance — and the K taps are applied in a
// fixed order: y = ((bias + w_0 x_{t-R}) + w_1 x_{t-R+1}) + ... (fp32 fused multiply-adds).  Consecutive threads take consecutive
// channel vectors of the same rows, so every row is read as whole 1 KiB (C = 512, bf16) runs.  The halo rows (K - 1 per tile) are
// read by two neighbouring tiles; the second read is served by the L2.
//
//   tn_dw         d = dwconv(x) + bias
//   tn_mega_tail  y = relu(skip + g[b, :] * h3) (the mega-block output: BN'd 1 x 1 skip + SE-gated third sub-block), and with the next
//                 block's depthwise weights d = dwconv(y) + bias in the same pass: y is recomputed on the halo rows from skip and h3
//                 (rounded to the storage type as it is stored, so d is what tn_dw of the stored y gives), never read back.
#include "kernels.h"

namespace svhip {

namespace {

// frames per tile (registers: (TT + K - 1) rows + K weight vectors; no scratch at k = 11).  The fused tail loads two rows (skip, h3) per
// frame: half the tile keeps it at the depthwise kernel's register count
template <int K, bool TAIL> struct TnTile { static constexpr int TT = TAIL && K > 1 ? 8 : 16; };

// RAG (a pack, grid (x, n)): utterance blockIdx.y owns the rows [rag_row0[b], rag_row0[b + 1]) and Tn is its own length; grid.x holds the
// tiles of the longest utterance, and the threads past an utterance's last tile leave before they load anything.  From there on the
// thread runs the fixed kernel's code on (row0, Tn, t0), so an utterance's values are those of the fixed kernel at B = 1, Tn = T_u.
template <typename T, int K, bool TAIL, bool DW, bool RAG>
__global__ __launch_bounds__(256) void tn_dw_kernel(const T* __restrict__ x, const T* __restrict__ skip, const T* __restrict__ h3,
                                                    const float* __restrict__ gate, T* __restrict__ y, const float* __restrict__ w,
                                                    const float* __restrict__ bias, T* __restrict__ d, int B, int Tn, int C,
                                                    const int* __restrict__ rag_row0) {
    constexpr int VEC = Vec16<T>::N;
    constexpr int R = K / 2;
    constexpr int TT = TnTile<K, TAIL>::TT;
    constexpr int NR = DW ? TT + 2 * R : TT;          // rows held in registers
    const int nvec = C / VEC;
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int v = g % nvec;
    const int q = g / nvec;
    int b, t0;
    int64_t row0;
    if constexpr (RAG) {
        b = blockIdx.y;
        row0 = rag_row0[b];
        Tn = rag_row0[b + 1] - (int)row0;
        if (q >= (Tn + TT - 1) / TT) return;
        t0 = q * TT;
    } else {
        const int ntile = (Tn + TT - 1) / TT;
        b = q / ntile;
        if (b >= B) return;
        t0 = (q - b * ntile) * TT;
        row0 = (int64_t)b * Tn;
    }
    const int c0 = v * VEC;
    const int r0 = DW ? R : 0;                        // register row i holds frame t0 - r0 + i

    float gv[VEC];
    if constexpr (TAIL) {
        const f32x4* g4 = reinterpret_cast<const f32x4*>(gate + (int64_t)b * C + c0);
#pragma unroll
        for (int u = 0; u < VEC / 4; ++u) {
            const f32x4 a = g4[u];
#pragma unroll
            for (int e = 0; e < 4; ++e) gv[4 * u + e] = a[e];
        }
    }
    Vec16<T> xr[NR];
    if constexpr (TAIL) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int t = t0 - r0 + i;
            const bool ok = t >= 0 && t < Tn;
            const int64_t m = row0 + (ok ? t : 0);
            const Vec16<T> sr = *reinterpret_cast<const Vec16<T>*>(skip + m * C + c0);
            const Vec16<T> hr = *reinterpret_cast<const Vec16<T>*>(h3 + m * C + c0);
#pragma unroll
            for (int e = 0; e < VEC; ++e) xr[i].set(e, ok ? fmaxf(fmaf(gv[e], hr.get(e), sr.get(e)), 0.0f) : 0.0f);
            if (i >= r0 && i < r0 + TT && ok) *reinterpret_cast<Vec16<T>*>(y + (row0 + t) * C + c0) = xr[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int t = t0 - r0 + i;
            const bool ok = t >= 0 && t < Tn;
            xr[i] = *reinterpret_cast<const Vec16<T>*>(x + (row0 + (ok ? t : 0)) * C + c0);
            if (!ok)
#pragma unroll
                for (int e = 0; e < VEC; ++e) xr[i].set(e, 0.0f);
        }
    }
    if constexpr (DW) {
        float wv[K][VEC], bv[VEC];
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int u = 0; u < VEC / 4; ++u) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(w + (int64_t)j * C + c0 + 4 * u);
#pragma unroll
                for (int e = 0; e < 4; ++e) wv[j][4 * u + e] = a[e];
            }
#pragma unroll
        for (int u = 0; u < VEC / 4; ++u) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(bias + c0 + 4 * u);
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[4 * u + e] = a[e];
        }
#pragma unroll
        for (int i = 0; i < TT; ++i) {
            const int t = t0 + i;
            if (t < Tn) {
                Vec16<T> o;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    float a = bv[e];
#pragma unroll
                    for (int j = 0; j < K; ++j) a = fmaf(wv[j][e], xr[i + j].get(e), a);
                    o.set(e, a);
                }
                *reinterpret_cast<Vec16<T>*>(d + (row0 + t) * C + c0) = o;
            }
        }
    }
}

// row0 == null: B utterances of Tn frames.  A pack: B = n utterances by the device table row0, Tn = the longest utterance's frames
template <typename T, int K, bool TAIL, bool DW>
hipError_t launch_k(const void* x, const void* skip, const void* h3, const float* gate, void* y, const float* w, const float* bias, void* d,
                    int B, int Tn, int C, const int* row0, hipStream_t stream) {
    constexpr int TT = TnTile<K, TAIL>::TT;
    const int64_t per_utt = (int64_t)((Tn + TT - 1) / TT) * (C / Vec16<T>::N);
    const int64_t threads = row0 ? per_utt : B * per_utt;
    if (threads >= ((int64_t)1 << 31) || (row0 && B > 65535)) return hipErrorInvalidValue;
    const unsigned gx = (unsigned)((threads + 255) / 256);
    if (row0)
        hipLaunchKernelGGL((tn_dw_kernel<T, K, TAIL, DW, true>), dim3(gx, (unsigned)B), dim3(256), 0, stream, (const T*)x, (const T*)skip,
                           (const T*)h3, gate, (T*)y, w, bias, (T*)d, B, 0, C, row0);
    else
        hipLaunchKernelGGL((tn_dw_kernel<T, K, TAIL, DW, false>), dim3(gx), dim3(256), 0, stream, (const T*)x, (const T*)skip,
                           (const T*)h3, gate, (T*)y, w, bias, (T*)d, B, Tn, C, nullptr);
    return hipGetLastError();
}

template <typename T, bool TAIL>
hipError_t launch_by_k(int k, const void* x, const void* skip, const void* h3, const float* gate, void* y, const float* w, const float* bias, void* d,
                       int B, int Tn, int C, const int* row0, hipStream_t stream) {
    if (TAIL && !d) return launch_k<T, 1, true, false>(x, skip, h3, gate, y, w, bias, d, B, Tn, C, row0, stream);
    switch (k) {
        case 3: return launch_k<T, 3, TAIL, true>(x, skip, h3, gate, y, w, bias, d, B, Tn, C, row0, stream);
        case 7: return launch_k<T, 7, TAIL, true>(x, skip, h3, gate, y, w, bias, d, B, Tn, C, row0, stream);
        case 11: return launch_k<T, 11, TAIL, true>(x, skip, h3, gate, y, w, bias, d, B, Tn, C, row0, stream);
        default: return hipErrorInvalidValue;
    }
}

// rows[b, 0:n) = NaN for every utterance b whose input (per_utt floats from x + b per_utt) holds an inf / NaN: the ReLU epilogues
// (fmaxf) would turn such a value into 0, where the reference's forward propagates it to the embedding.
// RAG (a pack): utterance b's values start at x + rag_off[b] and number (rag_row0[b + 1] - rag_row0[b]) * per_utt, per_utt counting one ROW
template <bool RAG>
__global__ __launch_bounds__(256) void tn_nonfinite_rows_kernel(const float* __restrict__ x, int64_t per_utt, float* __restrict__ rows, int ld, int n,
                                                                const int64_t* __restrict__ rag_off, const int* __restrict__ rag_row0) {
    const int b = blockIdx.x;
    const uint32_t* __restrict__ p;
    if constexpr (RAG) {
        p = reinterpret_cast<const uint32_t*>(x + rag_off[b]);
        per_utt *= rag_row0[b + 1] - rag_row0[b];
    } else {
        p = reinterpret_cast<const uint32_t*>(x + (int64_t)b * per_utt);
    }
    int bad = 0;
    for (int64_t i = threadIdx.x; i < per_utt; i += 256) bad |= (p[i] & 0x7f800000u) == 0x7f800000u;
    bad = __syncthreads_or(bad);
    if (bad)
        for (int i = threadIdx.x; i < n; i += 256) rows[(int64_t)b * ld + i] = __builtin_nanf("");
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool shape_ok(int dt, int k, int B, int Tn, int C) {
    if (dt != DT_F32 && dt != DT_BF16) return false;
    if (B <= 0 || Tn <= 0 || C <= 0 || C % 8 != 0) return false;
    return k == 3 || k == 7 || k == 11;
}

}  // namespace

hipError_t launch_tn_nonfinite_rows(const float* x, int64_t per_utt, int B, float* rows, int ld, int n, hipStream_t stream) {
    if (!x || !rows || B <= 0 || per_utt <= 0 || n <= 0 || ld < n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tn_nonfinite_rows_kernel<false>, dim3(B), dim3(256), 0, stream, x, per_utt, rows, ld, n, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_tn_nonfinite_rows_ragged(const float* x, const int64_t* off, const int* row0, int per_row, int B, float* rows, int ld, int n,
                                           hipStream_t stream) {
    if (!x || !off || !row0 || !rows || B <= 0 || per_row <= 0 || n <= 0 || ld < n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tn_nonfinite_rows_kernel<true>, dim3(B), dim3(256), 0, stream, x, (int64_t)per_row, rows, ld, n, off, row0);
    return hipGetLastError();
}

// (ragged != 0: the pack forms, which need their table)
static hipError_t tn_dw_any(const void* x, void* d, const float* w, const float* bias, int dt, int k, int B, int Tn, int C, const int* row0, bool ragged,
                            hipStream_t stream) {
    if (!shape_ok(dt, k, B, Tn, C) || !x || !d || !w || !bias || (ragged && !row0)) return hipErrorInvalidValue;
    if (!aligned16(x) || !aligned16(d) || !aligned16(w) || !aligned16(bias)) return hipErrorInvalidValue;
    if (dt == DT_BF16) return launch_by_k<bf16_t, false>(k, x, nullptr, nullptr, nullptr, nullptr, w, bias, d, B, Tn, C, row0, stream);
    return launch_by_k<float, false>(k, x, nullptr, nullptr, nullptr, nullptr, w, bias, d, B, Tn, C, row0, stream);
}

static hipError_t tn_mega_tail_any(const void* skip, const void* h3, const float* gate, void* y, const float* w, const float* bias, void* d, int dt,
                                   int k, int B, int Tn, int C, const int* row0, bool ragged, hipStream_t stream) {
    if (!shape_ok(dt, d ? k : 3, B, Tn, C) || !skip || !h3 || !gate || !y || (d && (!w || !bias)) || (ragged && !row0)) return hipErrorInvalidValue;
    if (!aligned16(skip) || !aligned16(h3) || !aligned16(gate) || !aligned16(y) || (d && (!aligned16(d) || !aligned16(w) || !aligned16(bias))))
        return hipErrorInvalidValue;
    if (dt == DT_BF16) return launch_by_k<bf16_t, true>(k, nullptr, skip, h3, gate, y, w, bias, d, B, Tn, C, row0, stream);
    return launch_by_k<float, true>(k, nullptr, skip, h3, gate, y, w, bias, d, B, Tn, C, row0, stream);
}

hipError_t launch_tn_dw(const void* x, void* d, const float* w, const float* bias, int dt, int k, int B, int Tn, int C, hipStream_t stream) {
    return tn_dw_any(x, d, w, bias, dt, k, B, Tn, C, nullptr, false, stream);
}

hipError_t launch_tn_mega_tail(const void* skip, const void* h3, const float* gate, void* y, const float* w, const float* bias, void* d, int dt, int k,
                               int B, int Tn, int C, hipStream_t stream) {
    return tn_mega_tail_any(skip, h3, gate, y, w, bias, d, dt, k, B, Tn, C, nullptr, false, stream);
}

hipError_t launch_tn_dw_ragged(const void* x, void* d, const float* w, const float* bias, int dt, int k, const int* row0, int n, int max_T, int C,
                               hipStream_t stream) {
    return tn_dw_any(x, d, w, bias, dt, k, n, max_T, C, row0, true, stream);
}

hipError_t launch_tn_mega_tail_ragged(const void* skip, const void* h3, const float* gate, void* y, const float* w, const float* bias, void* d, int dt,
                                      int k, const int* row0, int n, int max_T, int C, hipStream_t stream) {
    return tn_mega_tail_any(skip, h3, gate, y, w, bias, d, dt, k, n, max_T, C, row0, true, stream);
}

}  // namespace svhip
