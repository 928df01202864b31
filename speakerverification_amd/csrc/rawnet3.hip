// rawnet3.hip — the kernels of RawNet3 (reference models/RawNet3.py, models/RawNet_baseline.py:27-159) that the conv GEMMs do not
// cover: the sinc front-end, the Bottle2neck block tail (max-pool + AFMS) and the single-head context pooling.
//
// Front-end (RawNet3.py:88-99), two launches per batch plus a column mean:
//   rn3_prenorm  per utterance: mean and biased variance of the pre-emphasised waveform (PreEmphasis with a left reflect pad,
//                InstanceNorm1d(1, eps = 1e-4)), in fp64
//   rn3_sinc     y = conv1d(in_norm(pre_emph(x)), 256 filters of 251 taps, stride 10), then log(|y| + 1e-6), fp32 out (B, T0, 256).
//                The filterbank products are accumulated in ACC: fp64 on fp32 handles — log(|y| + 1e-6) turns the ~1e-6 relative
//                rounding of an fp32 sum into O(1) errors at the outputs that sit near a zero crossing — and fp32 on 16-bit handles
//   (colmean)    the time mean of every (utterance, filter)
//   rn3_center   x0 = y - mean, stored in the handle's activation type: layer1's frame-major operand
//
// Block tail (RawNet_baseline.py:150-159; the residual rides in conv3's GEMM epilogue):
//   rn3_maxpool  MaxPool1d(P) over frames, strided rows on both sides (the stage outputs are column thirds of one (M, 3072) buffer)
//   (colmean, rowvec_linear with the sigmoid)   the AFMS gate sigmoid(fc(mean_t x))
//   rn3_afms     y = (x + alpha) * gate, and optionally y + add in the same pass (layer3's input mp3(x1) + x2)
//
// Context pooling (RawNet3.py:110-142):
//   rn3_tstats   [mean_t x | sqrt(clamp(var_t x, 1e-4, 1e4))] with the UNBIASED variance (torch.var), fp64 sums
//   rn3_logit    the per-frame logit w2 . h_t + b2 of the 128-wide attention activation (one logit per frame, all channels share it)
//   rn3_pool     softmax over T, mu = sum w x, sg = sqrt(clamp(sum w x^2 - mu^2, 1e-4, 1e4)), then the bn5 affine -> pooled (B, 3072).
//                The moments are fp64 sums on fp32 handles: sum w x^2 - mu^2 cancels, and fp32 sums leave ~1e-5 of scale in sg.
//                An utterance whose waveform is not finite (its rn3_prenorm statistics are not) pools to NaN, as in the reference: the
//                ReLU epilogues (fmaxf) map a NaN to 0 where torch.relu keeps it, so layer4's output would be finite and meaningless
//
// Ragged packs (launch_rn3_rag_*): n utterances of different lengths packed back to back at the three frame levels (T0_u frames after
// the filterbank, T0_u / 5 after layer1's pool, T0_u / 5 / 3 after layer2's), each level with its row0 / utt segment table
// (ragged.hip's layout).  Every kernel above has a segment-table form that runs the same per-utterance code on the utterance's own
// rows: a workgroup of the front-end sees one utterance's samples, a pooled row reads frames of its own utterance (the T_u % P
// left-over frames are dropped per utterance), the gate is looked up through utt[row], and the reductions over time walk the
// utterance's frames in the order of the fixed-length kernels.  So an utterance's values are those of a fixed-length forward of its
// own length through the same kernels, whatever it is packed with.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace svhip {

namespace {

constexpr int R3_THREADS = 256;
constexpr int R3_FRAMES = 32;                                   // frames per rn3_sinc workgroup
constexpr int R3_SEG = RN3_STRIDE * (R3_FRAMES - 1) + RN3_TAPS;   // waveform samples one workgroup reads

template <typename A>
__device__ __forceinline__ A block_sum(A v, A* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    A s = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    return s;
}

__device__ __forceinline__ float block_max(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float s = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s = fmaxf(s, red[w]);
    return s;
}

// pre-emphasised sample i of one utterance: f0 x[i-1] + f1 x[i], the left neighbour of x[0] being x[1] (reflect pad)
__device__ __forceinline__ double pre_emph(const float* __restrict__ s, int i, double f0, double f1) {
    return f0 * (double)s[i == 0 ? 1 : i - 1] + f1 * (double)s[i];
}

// stats = {mean, 1 / sqrt(var + 1e-4)} of the pre-emphasised waveform s[0, L) of one utterance, fp64, two passes (one workgroup)
__device__ __forceinline__ void prenorm_utt(const float* __restrict__ s, int L, double f0, double f1, double* __restrict__ stats, double* red) {
    double a = 0.0;
    for (int i = threadIdx.x; i < L; i += R3_THREADS) a += pre_emph(s, i, f0, f1);
    const double mean = block_sum(a, red) / L;
    double q = 0.0;
    for (int i = threadIdx.x; i < L; i += R3_THREADS) { const double d = pre_emph(s, i, f0, f1) - mean; q += d * d; }
    const double var = block_sum(q, red) / L;
    if (threadIdx.x == 0) { stats[0] = mean; stats[1] = 1.0 / sqrt(var + 1e-4); }
}

// grid B: stats[b] of utterance b of a (B, L) batch
__global__ __launch_bounds__(R3_THREADS) void rn3_prenorm_kernel(const float* __restrict__ wav, int L, double f0, double f1, double* __restrict__ stats) {
    __shared__ double red[R3_THREADS / 64];
    prenorm_utt(wav + (int64_t)blockIdx.x * L, L, f0, f1, stats + 2 * blockIdx.x, red);
}

// grid n: utterance u is the len[u] samples at wav + off[u]
__global__ __launch_bounds__(R3_THREADS) void rn3_rag_prenorm_kernel(const float* __restrict__ wav, const int64_t* __restrict__ off, const int* __restrict__ len,
                                                                     double f0, double f1, double* __restrict__ stats) {
    __shared__ double red[R3_THREADS / 64];
    prenorm_utt(wav + off[blockIdx.x], len[blockIdx.x], f0, f1, stats + 2 * blockIdx.x, red);
}

// The frames [t0, t0 + R3_FRAMES) of one utterance (s[0, L), T0 frames, statistics st), one thread per filter.  filt: [251][256] in
// ACC (tap-major, so one tap of all filters is one coalesced row); in_aff = {weight, bias} of the InstanceNorm.
// out (T0, 256) fp32 = log(|y| + 1e-6): the utterance's rows.
template <typename ACC>
__device__ __forceinline__ void sinc_tile(const float* __restrict__ s, int L, int T0, int t0, const double* __restrict__ st, const float* __restrict__ in_w,
                                          const float* __restrict__ in_b, double f0, double f1, const ACC* __restrict__ filt, float* __restrict__ out, ACC* seg) {
    const int f = threadIdx.x;
    const double mean = st[0], rstd = st[1], g = in_w[0], be = in_b[0];
    const int s0 = RN3_STRIDE * t0;
    for (int i = threadIdx.x; i < R3_SEG + 1; i += R3_THREADS) {
        const int j = s0 + i;
        seg[i] = j < L ? (ACC)((pre_emph(s, j, f0, f1) - mean) * rstd * g + be) : (ACC)0;      // (samples past L feed no frame < T0)
    }
    __syncthreads();
    ACC acc[R3_FRAMES];
#pragma unroll
    for (int j = 0; j < R3_FRAMES; ++j) acc[j] = 0;
    for (int k = 0; k < RN3_TAPS; ++k) {
        const ACC w = filt[k * RN3_FILTERS + f];
#pragma unroll
        for (int j = 0; j < R3_FRAMES; ++j) acc[j] = fma(w, seg[RN3_STRIDE * j + k], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < R3_FRAMES; ++j) {
        const int t = t0 + j;
        if (t < T0) out[(int64_t)t * RN3_FILTERS + f] = (float)log(fabs(acc[j]) + (ACC)1e-6);
    }
}

// grid (ceil(T0 / R3_FRAMES), B): out (B, T0, 256)
template <typename ACC>
__global__ __launch_bounds__(R3_THREADS) void rn3_sinc_kernel(const float* __restrict__ wav, const double* __restrict__ stats, const float* __restrict__ in_w,
                                                              const float* __restrict__ in_b, double f0, double f1, const ACC* __restrict__ filt,
                                                              float* __restrict__ out, int L, int T0) {
    __shared__ ACC seg[R3_SEG + 1];
    const int b = blockIdx.y;
    sinc_tile<ACC>(wav + (int64_t)b * L, L, T0, blockIdx.x * R3_FRAMES, stats + 2 * b, in_w, in_b, f0, f1, filt, out + (int64_t)b * T0 * RN3_FILTERS, seg);
}

// grid (ceil(maxT0 / R3_FRAMES), n): utterance u's frames go to the rows row0[u] .. of out; the tiles past its last frame leave at once
template <typename ACC>
__global__ __launch_bounds__(R3_THREADS) void rn3_rag_sinc_kernel(const float* __restrict__ wav, const int64_t* __restrict__ off, const int* __restrict__ len,
                                                                  const int* __restrict__ row0, const double* __restrict__ stats,
                                                                  const float* __restrict__ in_w, const float* __restrict__ in_b, double f0, double f1,
                                                                  const ACC* __restrict__ filt, float* __restrict__ out) {
    __shared__ ACC seg[R3_SEG + 1];
    const int u = blockIdx.y, t0 = blockIdx.x * R3_FRAMES;
    const int r0 = row0[u], T0 = row0[u + 1] - r0;
    if (t0 >= T0) return;
    sinc_tile<ACC>(wav + off[u], len[u], T0, t0, stats + 2 * u, in_w, in_b, f0, f1, filt, out + (int64_t)r0 * RN3_FILTERS, seg);
}

// x0[(b, t), f] = y[(b, t), f] - mean[b, f] in the storage type (y and x0 may be the same fp32 buffer).  RAG: b = utt[row]
template <typename T, bool RAG>
__global__ __launch_bounds__(R3_THREADS) void rn3_center_kernel(const float* __restrict__ y, const float* __restrict__ mean, T* __restrict__ x0, int T0, int64_t n,
                                                                const int* __restrict__ utt) {
    for (int64_t i = (int64_t)blockIdx.x * R3_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * R3_THREADS) {
        const int f = (int)(i % RN3_FILTERS);
        const int64_t b = RAG ? utt[i / RN3_FILTERS] : i / ((int64_t)T0 * RN3_FILTERS);
        x0[i] = from_f32<T>(y[i] - mean[b * RN3_FILTERS + f]);
    }
}

// one thread per 16 bytes of channels of one output row.  RAG: output row `row` is frame tn = row - row0_out[u] of utterance
// u = utt_out[row] and reads the frames P tn .. P tn + P - 1 of u's input rows row0_in[u] .. (Tin, Tn unused)
template <typename T, bool RAG>
__global__ __launch_bounds__(R3_THREADS) void rn3_maxpool_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy, int Tin, int Tn, int C, int P,
                                                                 int64_t n, const int* __restrict__ row0_in, const int* __restrict__ row0_out,
                                                                 const int* __restrict__ utt_out) {
    constexpr int V = Vec16<T>::N;
    const int cv = C / V;
    for (int64_t i = (int64_t)blockIdx.x * R3_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * R3_THREADS) {
        const int c0 = (int)(i % cv) * V;
        const int64_t row = i / cv;                        // b * Tn + tn
        int64_t first;                                     // the first of the P input rows
        if (RAG) {
            const int u = utt_out[row];
            first = row0_in[u] + (row - row0_out[u]) * P;
        } else {
            const int64_t b = row / Tn, tn = row % Tn;
            first = b * Tin + tn * P;
        }
        const T* src = x + first * ldx + c0;
        Vec16<T> m = *reinterpret_cast<const Vec16<T>*>(src);
        for (int p = 1; p < P; ++p) {
            const Vec16<T> v = *reinterpret_cast<const Vec16<T>*>(src + (int64_t)p * ldx);
#pragma unroll
            for (int e = 0; e < V; ++e) m.set(e, fmaxf(m.get(e), v.get(e)));
        }
        *reinterpret_cast<Vec16<T>*>(y + row * ldy + c0) = m;
    }
}

// y = (x + alpha) * gate; with `sum`: sum = y + add (y as stored, i.e. rounded to the storage type).  RAG: the gate row is utt[row]
template <typename T, bool RAG>
__global__ __launch_bounds__(R3_THREADS) void rn3_afms_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ alpha, const float* __restrict__ gate,
                                                              T* __restrict__ y, int ldy, const T* __restrict__ add, int ldadd, T* __restrict__ sum, int ldsum,
                                                              int Tn, int C, int64_t n, const int* __restrict__ utt) {
    constexpr int V = Vec16<T>::N;
    const int cv = C / V;
    for (int64_t i = (int64_t)blockIdx.x * R3_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * R3_THREADS) {
        const int c0 = (int)(i % cv) * V;
        const int64_t row = i / cv, b = RAG ? utt[row] : row / Tn;
        const Vec16<T> v = *reinterpret_cast<const Vec16<T>*>(x + row * ldx + c0);
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < V; ++e) o.set(e, (v.get(e) + alpha[c0 + e]) * gate[b * C + c0 + e]);
        *reinterpret_cast<Vec16<T>*>(y + row * ldy + c0) = o;
        if (sum) {
            const Vec16<T> a = *reinterpret_cast<const Vec16<T>*>(add + row * ldadd + c0);
            Vec16<T> s;
#pragma unroll
            for (int e = 0; e < V; ++e) s.set(e, o.get(e) + a.get(e));
            *reinterpret_cast<Vec16<T>*>(sum + row * ldsum + c0) = s;
        }
    }
}

// one thread per channel c of one utterance (p: its first row at column c, Tn frames): stats (2C) = [mean | sqrt(clamp(unbiased var,
// 1e-4, 1e4))], fp64 sums
template <typename T>
__device__ __forceinline__ void tstats_utt(const T* __restrict__ p, int ldx, int Tn, int C, int c, float* __restrict__ stats) {
    double s = 0.0;
    for (int t = 0; t < Tn; ++t) s += (double)to_f32(p[(int64_t)t * ldx]);
    const double mean = s / Tn;
    double q = 0.0;
    for (int t = 0; t < Tn; ++t) { const double d = (double)to_f32(p[(int64_t)t * ldx]) - mean; q += d * d; }
    const double var = q / (double)(Tn - 1);                 // (Tn == 1: NaN, as torch.var gives)
    stats[c] = (float)mean;
    stats[C + c] = sqrtf(fminf(fmaxf((float)var, 1e-4f), 1e4f));
}

// grid (ceil(C / 256), B): stats (B, 2C).  row0 (ragged packs): utterance b owns the rows [row0[b], row0[b + 1]) (null: Tn rows each)
template <typename T>
__global__ __launch_bounds__(R3_THREADS) void rn3_tstats_kernel(const T* __restrict__ x, int ldx, int Tn, int C, float* __restrict__ stats,
                                                                const int* __restrict__ row0) {
    const int b = blockIdx.y, c = blockIdx.x * R3_THREADS + threadIdx.x;
    if (c >= C) return;
    const int64_t r0 = row0 ? row0[b] : (int64_t)b * Tn;
    if (row0) Tn = row0[b + 1] - row0[b];
    tstats_utt(x + r0 * ldx + c, ldx, Tn, C, c, stats + (int64_t)b * 2 * C);
}

// one wave per frame row: logit[m] = b2 + sum_k w2[k] h[m, k], K = 128
template <typename T>
__global__ __launch_bounds__(R3_THREADS) void rn3_logit_kernel(const T* __restrict__ hbuf, int ldh, const float* __restrict__ w2, const float* __restrict__ b2,
                                                               float* __restrict__ logit, int64_t M) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * (R3_THREADS / 64) + (threadIdx.x >> 6);
    if (m >= M) return;
    const T* r = hbuf + m * ldh;
    float v = w2[lane] * to_f32(r[lane]) + w2[lane + 64] * to_f32(r[lane + 64]);
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) logit[m] = v + b2[0];
}

// grid (ceil(C / 256), B), one thread per channel: softmax over the utterance's Tn logits, weighted moments, clamp, bn5 affine.
// row0 (ragged packs): utterance b owns the rows [row0[b], row0[b + 1]) of logit and x (null: Tn rows each)
template <typename T>
__global__ __launch_bounds__(R3_THREADS) void rn3_pool_kernel(const float* __restrict__ logit, const T* __restrict__ x, int ldx, int Tn, int C,
                                                              const float* __restrict__ sc, const float* __restrict__ sh, const double* __restrict__ in_stats,
                                                              float* __restrict__ pooled, const int* __restrict__ row0) {
    typedef typename std::conditional<sizeof(T) == 4, double, float>::type A;       // (fp64 moments on fp32 handles)
    __shared__ float red[R3_THREADS / 64];
    const int b = blockIdx.y, c = blockIdx.x * R3_THREADS + threadIdx.x;
    const int64_t r0 = row0 ? row0[b] : (int64_t)b * Tn;
    if (row0) Tn = row0[b + 1] - row0[b];
    const float* lg = logit + r0;
    float mx = -INFINITY;
    for (int t = threadIdx.x; t < Tn; t += R3_THREADS) mx = fmaxf(mx, lg[t]);
    mx = block_max(mx, red);
    float se = 0.0f;
    for (int t = threadIdx.x; t < Tn; t += R3_THREADS) se += expf(lg[t] - mx);
    const float inv = 1.0f / block_sum(se, red);
    if (c >= C) return;
    const T* p = x + r0 * ldx + c;
    A mu = 0, m2 = 0;
    for (int t = 0; t < Tn; ++t) {
        const A w = (A)(expf(lg[t] - mx) * inv), v = (A)to_f32(p[(int64_t)t * ldx]);
        mu = fma(v, w, mu);
        m2 = fma(v * v, w, m2);
    }
    float sg = sqrtf(fminf(fmaxf((float)(m2 - mu * mu), 1e-4f), 1e4f)), m = (float)mu;
    if (!isfinite(in_stats[2 * b]) || !isfinite(in_stats[2 * b + 1])) m = sg = NAN;
    pooled[(int64_t)b * 2 * C + c] = m * sc[c] + sh[c];
    pooled[(int64_t)b * 2 * C + C + c] = sg * sc[C + c] + sh[C + c];
}

inline int grid_of(int64_t n) { return (int)std::min<int64_t>((n + R3_THREADS - 1) / R3_THREADS, 65536); }

}  // namespace

hipError_t launch_rn3_front(const float* wav, int B, int L, int T0, double f0, double f1, const float* in_w, const float* in_b, const void* filt,
                            bool filt_f64, double* stats, float* y, hipStream_t stream) {
    if (!wav || !in_w || !in_b || !filt || !stats || !y || B <= 0 || L < RN3_TAPS || T0 != (L - RN3_TAPS) / RN3_STRIDE + 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rn3_prenorm_kernel, dim3(B), dim3(R3_THREADS), 0, stream, wav, L, f0, f1, stats);
    const dim3 grid((T0 + R3_FRAMES - 1) / R3_FRAMES, B);
    if (filt_f64) hipLaunchKernelGGL(rn3_sinc_kernel<double>, grid, dim3(R3_THREADS), 0, stream, wav, stats, in_w, in_b, f0, f1, (const double*)filt, y, L, T0);
    else hipLaunchKernelGGL(rn3_sinc_kernel<float>, grid, dim3(R3_THREADS), 0, stream, wav, stats, in_w, in_b, f0, f1, (const float*)filt, y, L, T0);
    return hipGetLastError();
}

hipError_t launch_rn3_rag_front(const float* wav, const int64_t* off, const int* len, const int* row0, int n, int maxT0, double f0, double f1,
                                const float* in_w, const float* in_b, const void* filt, bool filt_f64, double* stats, float* y, hipStream_t stream) {
    if (!wav || !off || !len || !row0 || !in_w || !in_b || !filt || !stats || !y || n <= 0 || maxT0 <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rn3_rag_prenorm_kernel, dim3(n), dim3(R3_THREADS), 0, stream, wav, off, len, f0, f1, stats);
    const dim3 grid((maxT0 + R3_FRAMES - 1) / R3_FRAMES, n);
    if (filt_f64) hipLaunchKernelGGL(rn3_rag_sinc_kernel<double>, grid, dim3(R3_THREADS), 0, stream, wav, off, len, row0, stats, in_w, in_b, f0, f1, (const double*)filt, y);
    else hipLaunchKernelGGL(rn3_rag_sinc_kernel<float>, grid, dim3(R3_THREADS), 0, stream, wav, off, len, row0, stats, in_w, in_b, f0, f1, (const float*)filt, y);
    return hipGetLastError();
}

// utt != null: the ragged form over M packed rows (B, T0 unused)
static hipError_t center(const float* y, const float* mean, void* x0, int dt, int T0, int64_t rows, const int* utt, hipStream_t stream) {
    const int64_t n = rows * RN3_FILTERS;
    const dim3 grid(grid_of(n)), block(R3_THREADS);
    if (dt != DT_F32 && dt != DT_BF16) return hipErrorInvalidValue;
    if (utt) {
        if (dt == DT_F32) hipLaunchKernelGGL((rn3_center_kernel<float, true>), grid, block, 0, stream, y, mean, (float*)x0, T0, n, utt);
        else hipLaunchKernelGGL((rn3_center_kernel<bf16_t, true>), grid, block, 0, stream, y, mean, (bf16_t*)x0, T0, n, utt);
    } else {
        if (dt == DT_F32) hipLaunchKernelGGL((rn3_center_kernel<float, false>), grid, block, 0, stream, y, mean, (float*)x0, T0, n, utt);
        else hipLaunchKernelGGL((rn3_center_kernel<bf16_t, false>), grid, block, 0, stream, y, mean, (bf16_t*)x0, T0, n, utt);
    }
    return hipGetLastError();
}

hipError_t launch_rn3_center(const float* y, const float* mean, void* x0, int dt, int B, int T0, hipStream_t stream) {
    if (!y || !mean || !x0 || B <= 0 || T0 <= 0) return hipErrorInvalidValue;
    return center(y, mean, x0, dt, T0, (int64_t)B * T0, nullptr, stream);
}

hipError_t launch_rn3_rag_center(const float* y, const float* mean, void* x0, int dt, const int* utt, int M, hipStream_t stream) {
    if (!y || !mean || !x0 || !utt || M <= 0) return hipErrorInvalidValue;
    return center(y, mean, x0, dt, 0, M, utt, stream);
}

// rows: output rows; utt_out != null: the ragged form
static hipError_t maxpool(const void* x, int ldx, void* y, int ldy, int dt, int Tin, int Tn, int C, int P, int64_t rows, const int* row0_in,
                          const int* row0_out, const int* utt_out, hipStream_t stream) {
    const int V = dt == DT_F32 ? 4 : 8;
    if (!x || !y || rows <= 0 || P < 1 || C % V || ldx % V || ldy % V || (dt != DT_F32 && dt != DT_BF16)) return hipErrorInvalidValue;
    const int64_t n = rows * (C / V);
    const dim3 grid(grid_of(n)), block(R3_THREADS);
#define SV_POOL(TT, RAG) hipLaunchKernelGGL((rn3_maxpool_kernel<TT, RAG>), grid, block, 0, stream, (const TT*)x, ldx, (TT*)y, ldy, Tin, Tn, C, P, n, row0_in, \
                                            row0_out, utt_out)
    if (utt_out) { if (dt == DT_F32) SV_POOL(float, true); else SV_POOL(bf16_t, true); }
    else { if (dt == DT_F32) SV_POOL(float, false); else SV_POOL(bf16_t, false); }
#undef SV_POOL
    return hipGetLastError();
}

hipError_t launch_rn3_maxpool(const void* x, int ldx, void* y, int ldy, int dt, int B, int Tin, int C, int P, hipStream_t stream) {
    if (B <= 0 || P < 1 || Tin < P) return hipErrorInvalidValue;
    return maxpool(x, ldx, y, ldy, dt, Tin, Tin / P, C, P, (int64_t)B * (Tin / P), nullptr, nullptr, nullptr, stream);
}

hipError_t launch_rn3_rag_maxpool(const void* x, int ldx, void* y, int ldy, int dt, const int* row0_in, const int* row0_out, const int* utt_out, int M_out,
                                  int C, int P, hipStream_t stream) {
    if (!row0_in || !row0_out || !utt_out) return hipErrorInvalidValue;
    return maxpool(x, ldx, y, ldy, dt, 0, 0, C, P, M_out, row0_in, row0_out, utt_out, stream);
}

static hipError_t afms(const void* x, int ldx, const float* alpha, const float* gate, void* y, int ldy, const void* add, int ldadd, void* sum, int ldsum,
                       int dt, int Tn, int C, int64_t rows, const int* utt, hipStream_t stream) {
    const int V = dt == DT_F32 ? 4 : 8;
    if (!x || !alpha || !gate || !y || rows <= 0 || C % V || ldx % V || ldy % V || (sum && (!add || ldadd % V || ldsum % V))) return hipErrorInvalidValue;
    if (dt != DT_F32 && dt != DT_BF16) return hipErrorInvalidValue;
    const int64_t n = rows * (C / V);
#define SV_AFMS(TT, RAG) hipLaunchKernelGGL((rn3_afms_kernel<TT, RAG>), dim3(grid_of(n)), dim3(R3_THREADS), 0, stream, (const TT*)x, ldx, alpha, gate, (TT*)y, ldy, \
                                            (const TT*)add, ldadd, (TT*)sum, ldsum, Tn, C, n, utt)
    if (utt) { if (dt == DT_F32) SV_AFMS(float, true); else SV_AFMS(bf16_t, true); }
    else { if (dt == DT_F32) SV_AFMS(float, false); else SV_AFMS(bf16_t, false); }
#undef SV_AFMS
    return hipGetLastError();
}

hipError_t launch_rn3_afms(const void* x, int ldx, const float* alpha, const float* gate, void* y, int ldy, const void* add, int ldadd, void* sum, int ldsum,
                           int dt, int B, int Tn, int C, hipStream_t stream) {
    if (B <= 0 || Tn <= 0) return hipErrorInvalidValue;
    return afms(x, ldx, alpha, gate, y, ldy, add, ldadd, sum, ldsum, dt, Tn, C, (int64_t)B * Tn, nullptr, stream);
}

hipError_t launch_rn3_rag_afms(const void* x, int ldx, const float* alpha, const float* gate, void* y, int ldy, const void* add, int ldadd, void* sum, int ldsum,
                               int dt, const int* utt, int M, int C, hipStream_t stream) {
    if (!utt || M <= 0) return hipErrorInvalidValue;
    return afms(x, ldx, alpha, gate, y, ldy, add, ldadd, sum, ldsum, dt, 1, C, M, utt, stream);
}

hipError_t launch_rn3_tstats(const void* x, int ldx, int dt, int B, int Tn, int C, float* stats, hipStream_t stream, const int* row0) {
    if (!x || !stats || B <= 0 || Tn <= 0) return hipErrorInvalidValue;
    const dim3 grid((C + R3_THREADS - 1) / R3_THREADS, B);
    if (dt == DT_F32) hipLaunchKernelGGL(rn3_tstats_kernel<float>, grid, dim3(R3_THREADS), 0, stream, (const float*)x, ldx, Tn, C, stats, row0);
    else if (dt == DT_BF16) hipLaunchKernelGGL(rn3_tstats_kernel<bf16_t>, grid, dim3(R3_THREADS), 0, stream, (const bf16_t*)x, ldx, Tn, C, stats, row0);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_rn3_ctx_pool(const void* hatt, int ldh, const float* w2, const float* b2, float* logit, const void* x, int ldx, int dt, int B, int Tn, int C,
                               const float* bn_scale, const float* bn_shift, const double* in_stats, float* pooled, hipStream_t stream, const int* row0,
                               int64_t rows) {
    if (!hatt || !w2 || !b2 || !logit || !x || !bn_scale || !bn_shift || !in_stats || !pooled || B <= 0 || Tn <= 0 || ldh < 128) return hipErrorInvalidValue;
    if (row0 && rows <= 0) return hipErrorInvalidValue;
    const int64_t M = row0 ? rows : (int64_t)B * Tn;
    const dim3 lgrid((unsigned)((M + 3) / 4)), pgrid((C + R3_THREADS - 1) / R3_THREADS, B);
    if (dt == DT_F32) {
        hipLaunchKernelGGL(rn3_logit_kernel<float>, lgrid, dim3(R3_THREADS), 0, stream, (const float*)hatt, ldh, w2, b2, logit, M);
        hipLaunchKernelGGL(rn3_pool_kernel<float>, pgrid, dim3(R3_THREADS), 0, stream, logit, (const float*)x, ldx, Tn, C, bn_scale, bn_shift, in_stats, pooled, row0);
    } else if (dt == DT_BF16) {
        hipLaunchKernelGGL(rn3_logit_kernel<bf16_t>, lgrid, dim3(R3_THREADS), 0, stream, (const bf16_t*)hatt, ldh, w2, b2, logit, M);
        hipLaunchKernelGGL(rn3_pool_kernel<bf16_t>, pgrid, dim3(R3_THREADS), 0, stream, logit, (const bf16_t*)x, ldx, Tn, C, bn_scale, bn_shift, in_stats, pooled, row0);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace svhip
