// ragged.hip — the kernels of a ragged ECAPA batch that must know where an utterance starts and ends (gfx950).
//
// n utterances of T_u frames are packed back to back into the frame-major workspace: row0[u] is the first row of utterance u,
// row0[n] the row count M, utt[m] the utterance of row m (rag_rows_kernel fills it from row0).  The reductions over time — the
// front-end's log-mel mean and instance norm, the SE squeeze, the ASP statistics, softmax and pooling — run as one workgroup per
// (utterance, channel block) that walks the utterance's own frames: wave w takes the frames t = w, w + 4, .. (t counted from the
// utterance's first frame), the four partial states meet in LDS in wave order.  So the order of every sum is fixed by the frame
// index alone, never by the tile or row-group boundaries of the packed matrix, and an utterance's values do not depend on what it
// is packed with or where.  The arithmetic is that of the fixed-length kernels (elementwise.hip, fbank.hip), so their error bars
// carry over.  Nothing here holds an utterance's time axis in LDS: a 60 s file (12 001 frames) is just a longer loop.
// All HBM-bound: 16-byte accesses along the channel axis.
#include "common.h"
#include "kernels.h"

namespace svhip {

namespace {

// utt[m] = u for the rows of utterance u: grid (ceil(maxT / 256), n)
__global__ __launch_bounds__(256) void rag_rows_kernel(const int* __restrict__ row0, int* __restrict__ utt) {
    const int u = blockIdx.y;
    const int r0 = row0[u], Tn = row0[u + 1] - r0;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < Tn) utt[r0 + t] = u;
}

// per (utterance, mel): the shift and scale of prologue_stats_kernel (fbank.hip) over the utterance's own T_u frames.
// grid (ceil(n_mels / 4), n), block 256: one wave per mel row, lane l takes t = l, l + 64, ..
__global__ __launch_bounds__(256) void rag_prologue_stats_kernel(const float* __restrict__ feat, const int64_t* __restrict__ feat_off,
                                                                 const int* __restrict__ row0, float* __restrict__ stats, int n_mels,
                                                                 int log_input, int inorm) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u = blockIdx.y, m = blockIdx.x * 4 + wave;
    if (m >= n_mels) return;
    const int T = row0[u + 1] - row0[u];
    const float* __restrict__ x = feat + feat_off[u] + (int64_t)m * T;
    float s = 0.0f;
    for (int t = lane; t < T; t += 64) {
        float v = x[t];
        if (log_input) v = logf(v + 1e-6f);
        s += v;
    }
    const float mean = wave_sum(s) / (float)T;
    float shift = log_input ? mean : 0.0f, scale = 1.0f;
    if (inorm) {
        const float mu = mean - shift;
        float q = 0.0f;
        for (int t = lane; t < T; t += 64) {
            float v = x[t];
            if (log_input) v = logf(v + 1e-6f);
            const float d = (v - shift) - mu;
            q += d * d;
        }
        const float var = wave_sum(q) / (float)T;
        shift = shift + mu;
        scale = 1.0f / sqrtf(var + 1e-5f);
    }
    if (lane == 0) {
        const int64_t o = 2 * ((int64_t)u * n_mels + m);
        stats[o] = shift;
        stats[o + 1] = scale;
    }
}

// (n_mels, T_u) blocks -> packed (M, n_mels) rows with log / shift / scale / affine applied; 32-frame LDS transpose tile.
// grid (ceil(maxT / 32), n): the tiles past an utterance's last frame leave at once.
template <typename T_>
__global__ __launch_bounds__(256) void rag_prologue_apply_kernel(const float* __restrict__ feat, const int64_t* __restrict__ feat_off,
                                                                 const int* __restrict__ row0, const float* __restrict__ stats,
                                                                 T_* __restrict__ out, int n_mels, int log_input,
                                                                 const float* __restrict__ in_w, const float* __restrict__ in_b) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tile = reinterpret_cast<float*>(smem);      // [n_mels][33]
    const int u = blockIdx.y, t0 = blockIdx.x * 32;
    const int r0 = row0[u], T = row0[u + 1] - r0;
    if (t0 >= T) return;
    const float* __restrict__ x = feat + feat_off[u];
    for (int idx = threadIdx.x; idx < n_mels * 32; idx += 256) {
        const int i = idx & 31, m = idx >> 5;
        const int t = t0 + i;
        float v = 0.0f;
        if (t < T) {
            v = x[(int64_t)m * T + t];
            if (log_input) v = logf(v + 1e-6f);
            const int64_t o = 2 * ((int64_t)u * n_mels + m);
            v = (v - stats[o]) * stats[o + 1];
            if (in_w) v = v * in_w[m] + in_b[m];
        }
        tile[m * 33 + i] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n_mels * 32; idx += 256) {
        const int m = idx % n_mels, i = idx / n_mels;
        const int t = t0 + i;
        if (t < T) out[((int64_t)r0 + t) * n_mels + m] = from_f32<T_>(tile[m * 33 + i]);
    }
}

// mean [| std] over the utterance's frames: colstats_kernel (elementwise.hip) with the rows taken from the segment table.
// grid (ceil(C / (64 VEC)), n), block 256
template <typename T, bool STD>
__global__ __launch_bounds__(256) void rag_colstats_kernel(const T* __restrict__ X, int ldx, const int* __restrict__ row0, int C,
                                                           float* __restrict__ out, int ld_out, float eps) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ float red[4][64 * VEC];
    const int u = blockIdx.y;
    const int r0 = row0[u], Tn = row0[u + 1] - r0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = (blockIdx.x * 64 + lane) * VEC;
    const bool ok = c0 < C;
    const T* __restrict__ base = X + (int64_t)r0 * ldx + c0;
    float s[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = 0.0f;
    if (ok)
        for (int t = wave; t < Tn; t += 4) {
            Vec16<T> v = *reinterpret_cast<const Vec16<T>*>(base + (int64_t)t * ldx);
#pragma unroll
            for (int j = 0; j < VEC; ++j) s[j] += v.get(j);
        }
#pragma unroll
    for (int j = 0; j < VEC; ++j) red[wave][lane * VEC + j] = s[j];
    __syncthreads();
    float mean[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const int e = lane * VEC + j;
        mean[j] = (red[0][e] + red[1][e] + red[2][e] + red[3][e]) / (float)Tn;
    }
    if (!STD) {
        if (wave == 0 && ok)
#pragma unroll
            for (int j = 0; j < VEC; ++j) out[(int64_t)u * ld_out + c0 + j] = mean[j];
        return;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = 0.0f;
    if (ok)
        for (int t = wave; t < Tn; t += 4) {
            Vec16<T> v = *reinterpret_cast<const Vec16<T>*>(base + (int64_t)t * ldx);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float d = v.get(j) - mean[j];
                s[j] = fmaf(d, d, s[j]);
            }
        }
#pragma unroll
    for (int j = 0; j < VEC; ++j) red[wave][lane * VEC + j] = s[j];
    __syncthreads();
    if (wave == 0 && ok)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int e = lane * VEC + j;
            const float var = (red[0][e] + red[1][e] + red[2][e] + red[3][e]) / (float)Tn;
            out[(int64_t)u * ld_out + c0 + j] = mean[j];
            out[(int64_t)u * ld_out + C + c0 + j] = sqrtf(fmaxf(var, eps));
        }
}

// SE gate + residual over the packed rows, the gate looked up per row.  grid ceil(M / RAG_SE_ROWS), block 256: a thread keeps one
// 16-byte column chunk and walks the block's rows four at a time; the gate row is re-read only where the utterance changes.
constexpr int RAG_SE_ROWS = 32;
template <typename T>
__global__ __launch_bounds__(256) void rag_se_apply_kernel(const T* __restrict__ h, int ldh, const float* __restrict__ s, const T* __restrict__ x,
                                                           int ldx, T* __restrict__ out, int ldo, const int* __restrict__ utt, int M, int C) {
    constexpr int VEC = Vec16<T>::N;
    const int cpr = C / VEC;
    const int m0 = blockIdx.x * RAG_SE_ROWS, m1 = min(m0 + RAG_SE_ROWS, M);
    for (int cc = threadIdx.x; cc < cpr * 4; cc += 256) {
        const int fl = cc / cpr, c = (cc - fl * cpr) * VEC;
        int ucur = -1;
        float g[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) g[j] = 0.0f;
        for (int m = m0 + fl; m < m1; m += 4) {
            const int u = utt[m];
            if (u != ucur) {
                ucur = u;
#pragma unroll
                for (int j = 0; j < VEC; ++j) g[j] = s[(int64_t)u * C + c + j];
            }
            const Vec16<T> hv = ld_nt(h + (int64_t)m * ldh + c);
            const Vec16<T> xv = ld_nt(x + (int64_t)m * ldx + c);
            Vec16<T> o;
#pragma unroll
            for (int j = 0; j < VEC; ++j) o.set(j, fmaf(hv.get(j), g[j], xv.get(j)));
            *reinterpret_cast<Vec16<T>*>(out + (int64_t)m * ldo + c) = o;
        }
    }
}

// attentive statistics pooling of one utterance: asp_pool_kernel (elementwise.hip) with the rows taken from the segment table.
// grid (ceil(C / 64), n), block 256: lane = channel, wave w takes the frames t = w, w + 4, ..
template <typename T>
__global__ __launch_bounds__(256) void rag_asp_pool_kernel(const float* __restrict__ logits, const T* __restrict__ X, int ldx,
                                                           const int* __restrict__ row0, int C, const float* __restrict__ bn_scale,
                                                           const float* __restrict__ bn_shift, float* __restrict__ pooled_raw,
                                                           float* __restrict__ pooled_bn, float eps, float var_max) {
    __shared__ float smx[4][64], sse[4][64], smean[4][64], sm2[4][64];
    const int b = blockIdx.y;
    const int r0 = row0[b], Tn = row0[b + 1] - r0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const bool ok = c < C;
    const float* __restrict__ lg = logits + (int64_t)r0 * C + c;
    const T* __restrict__ xp = X + (int64_t)r0 * ldx + c;
    float mx = -INFINITY, se = 0.0f, mean = 0.0f, m2 = 0.0f;
    if (ok) {
        for (int t0 = wave; t0 < Tn; t0 += 16) {
            float a[4], xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = min(t0 + 4 * u, Tn - 1);
                a[u] = lg[(int64_t)t * C];
                xv[u] = to_f32<T>(xp[(int64_t)t * ldx]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (t0 + 4 * u >= Tn) break;
                if (a[u] > mx) {
                    const float f = expf(mx - a[u]);
                    se *= f;
                    m2 *= f;
                    mx = a[u];
                }
                const float e = expf(a[u] - mx);
                se += e;
                const float d = xv[u] - mean;
                mean = fmaf(e / se, d, mean);
                m2 = fmaf(e * d, xv[u] - mean, m2);
            }
        }
    }
    smx[wave][lane] = mx; sse[wave][lane] = se; smean[wave][lane] = mean; sm2[wave][lane] = m2;
    __syncthreads();
    if (wave == 0 && ok) {
        const float Mx = fmaxf(fmaxf(smx[0][lane], smx[1][lane]), fmaxf(smx[2][lane], smx[3][lane]));
        float SE = 0.0f, MEAN = 0.0f, M2 = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float f = (smx[w][lane] == -INFINITY) ? 0.0f : expf(smx[w][lane] - Mx);
            const float sw = sse[w][lane] * f;
            if (sw > 0.0f) {
                const float tot = SE + sw;
                const float d = smean[w][lane] - MEAN;
                M2 += sm2[w][lane] * f + d * d * (SE * sw / tot);
                MEAN = fmaf(sw / tot, d, MEAN);
                SE = tot;
            }
        }
        float var = fmaxf(M2 / SE, eps);
        if (var_max > 0.0f && var > var_max) var = var_max;      // (Conformer: clamp(min = 1e-4, max = 1e4))
        const float sd = sqrtf(var);
        if (pooled_raw) {
            pooled_raw[(int64_t)b * 2 * C + c] = MEAN;
            pooled_raw[(int64_t)b * 2 * C + C + c] = sd;
        }
        pooled_bn[(int64_t)b * 2 * C + c] = fmaf(MEAN, bn_scale[c], bn_shift[c]);
        pooled_bn[(int64_t)b * 2 * C + C + c] = fmaf(sd, bn_scale[C + c], bn_shift[C + c]);
    }
}

// small-M linear, out[b, n] = act(bias[n] + W[n, :] . in[b, :]): rowvec_linear_small_kernel's arithmetic (elementwise.hip) at EVERY
// batch size.  grid (ceil(N / 8), ceil(B / 4)), block 1024: an 8 (n) x 4 (b) output block per workgroup; every output has its own
// accumulator, so a row's sum is the same whatever rides in the other three slots.
__global__ __launch_bounds__(1024) void rag_linear_kernel(const float* __restrict__ in, int ld_in, const float* __restrict__ W,
                                                          const float* __restrict__ bias, float* __restrict__ out, int ld_out, int B, int N,
                                                          int K, int act) {
    __shared__ float red[16][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 8, b0 = blockIdx.y * 4;
    const float* __restrict__ wrow[8];
    const float* __restrict__ xrow[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) wrow[i] = W + (int64_t)min(n0 + i, N - 1) * K;
#pragma unroll
    for (int j = 0; j < 4; ++j) xrow[j] = in + (int64_t)min(b0 + j, B - 1) * ld_in;
    float acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
    const int K4 = K >> 2;
#pragma unroll 2
    for (int c = threadIdx.x; c < K4; c += 1024) {
        f32x4 wv[8], xv[4];
#pragma unroll
        for (int i = 0; i < 8; ++i) wv[i] = *reinterpret_cast<const f32x4*>(wrow[i] + 4 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = *reinterpret_cast<const f32x4*>(xrow[j] + 4 * c);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j] = fmaf(wv[i][e], xv[j][e], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = wave_sum(acc[i][j]);
            if (lane == 0) red[wave][i * 4 + j] = s;
        }
    __syncthreads();
    if (threadIdx.x < 32) {
        const int i = threadIdx.x >> 2, j = threadIdx.x & 3;
        const int n = n0 + i, b = b0 + j;
        if (n < N && b < B) {
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < 16; ++w) s += red[w][threadIdx.x];
            out[(int64_t)b * ld_out + n] = apply_act(s + (bias ? bias[n] : 0.0f), act);
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_rag_rows(const int* row0, int n, int maxT, int* utt, hipStream_t stream) {
    if (!row0 || !utt || n <= 0 || maxT <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rag_rows_kernel, dim3((maxT + 255) / 256, n), dim3(256), 0, stream, row0, utt);
    return hipGetLastError();
}

hipError_t launch_rag_prologue(const float* feat, const int64_t* feat_off, const int* row0, int n, int maxT, void* out, bool out_bf16,
                               int n_mels, int log_input, const float* in_w, const float* in_b, float* stats, hipStream_t stream) {
    if (!feat || !feat_off || !row0 || !out || !stats || n <= 0 || maxT <= 0 || n_mels <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rag_prologue_stats_kernel, dim3((n_mels + 3) / 4, n), dim3(256), 0, stream, feat, feat_off, row0, stats, n_mels, log_input,
                       in_w != nullptr ? 1 : 0);
    const dim3 grid((maxT + 31) / 32, n);
    const size_t lds = (size_t)n_mels * 33 * sizeof(float);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    if (out_bf16)
        hipLaunchKernelGGL(rag_prologue_apply_kernel<bf16_t>, grid, dim3(256), lds, stream, feat, feat_off, row0, stats, reinterpret_cast<bf16_t*>(out),
                           n_mels, log_input, in_w, in_b);
    else
        hipLaunchKernelGGL(rag_prologue_apply_kernel<float>, grid, dim3(256), lds, stream, feat, feat_off, row0, stats, reinterpret_cast<float*>(out),
                           n_mels, log_input, in_w, in_b);
    return hipGetLastError();
}

hipError_t launch_rag_colstats(const void* X, bool bf16, int ldx, const int* row0, int n, int C, float* out, bool with_std, float eps,
                               hipStream_t stream) {
    const int vec = bf16 ? 8 : 4;
    if (!X || !row0 || !out || n <= 0 || C % vec != 0 || ldx % vec != 0 || !aligned16(X)) return hipErrorInvalidValue;
    const dim3 grid((C + 64 * vec - 1) / (64 * vec), n), block(256);
    if (with_std) {
        if (bf16) hipLaunchKernelGGL((rag_colstats_kernel<bf16_t, true>), grid, block, 0, stream, (const bf16_t*)X, ldx, row0, C, out, 2 * C, eps);
        else hipLaunchKernelGGL((rag_colstats_kernel<float, true>), grid, block, 0, stream, (const float*)X, ldx, row0, C, out, 2 * C, eps);
    } else {
        if (bf16) hipLaunchKernelGGL((rag_colstats_kernel<bf16_t, false>), grid, block, 0, stream, (const bf16_t*)X, ldx, row0, C, out, C, eps);
        else hipLaunchKernelGGL((rag_colstats_kernel<float, false>), grid, block, 0, stream, (const float*)X, ldx, row0, C, out, C, eps);
    }
    return hipGetLastError();
}

hipError_t launch_rag_se_apply(const void* h, int ldh, const float* s, const void* x, int ldx, void* out, int ldo, bool bf16,
                               const int* utt, int M, int C, hipStream_t stream) {
    const int vec = bf16 ? 8 : 4;
    if (!h || !s || !x || !out || !utt || M <= 0 || C % vec || ldh % vec || ldx % vec || ldo % vec) return hipErrorInvalidValue;
    if (!aligned16(h) || !aligned16(x) || !aligned16(out)) return hipErrorInvalidValue;
    const dim3 grid((M + RAG_SE_ROWS - 1) / RAG_SE_ROWS), block(256);
    if (bf16) hipLaunchKernelGGL(rag_se_apply_kernel<bf16_t>, grid, block, 0, stream, (const bf16_t*)h, ldh, s, (const bf16_t*)x, ldx, (bf16_t*)out, ldo, utt, M, C);
    else hipLaunchKernelGGL(rag_se_apply_kernel<float>, grid, block, 0, stream, (const float*)h, ldh, s, (const float*)x, ldx, (float*)out, ldo, utt, M, C);
    return hipGetLastError();
}

hipError_t launch_rag_asp_pool(const float* logits, const void* X, bool bf16, int ldx, const int* row0, int n, int C, const float* bn_scale,
                               const float* bn_shift, float* pooled_raw, float* pooled_bn, float eps, hipStream_t stream, float var_max) {
    if (!logits || !X || !row0 || !bn_scale || !bn_shift || !pooled_bn || n <= 0 || C <= 0) return hipErrorInvalidValue;
    const dim3 grid((C + 63) / 64, n), block(256);
    if (bf16) hipLaunchKernelGGL(rag_asp_pool_kernel<bf16_t>, grid, block, 0, stream, logits, (const bf16_t*)X, ldx, row0, C, bn_scale, bn_shift, pooled_raw, pooled_bn, eps, var_max);
    else hipLaunchKernelGGL(rag_asp_pool_kernel<float>, grid, block, 0, stream, logits, (const float*)X, ldx, row0, C, bn_scale, bn_shift, pooled_raw, pooled_bn, eps, var_max);
    return hipGetLastError();
}

hipError_t launch_rag_linear(const float* in, int ld_in, const float* W, const float* bias, float* out, int ld_out, int n, int N, int K,
                             int act, hipStream_t stream) {
    if (!in || !W || !out || K <= 0 || N <= 0 || n <= 0 || K % 4 != 0 || ld_in % 4 != 0 || !aligned16(in) || !aligned16(W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rag_linear_kernel, dim3((N + 7) / 8, (n + 3) / 4), dim3(1024), 0, stream, in, ld_in, W, bias, out, ld_out, n, N, K, act);
    return hipGetLastError();
}

}  // namespace svhip
