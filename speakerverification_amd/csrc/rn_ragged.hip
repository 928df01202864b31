// rn_ragged.hip — RawNet2 'conv' over a ragged pack (gfx950): the kernels that must know where an utterance starts and ends.
//
// n utterances are packed back to back at seven frame levels (the conv front-end's T1_u = len_u / 3 frames, then what each of the six
// max_pool1d(3) stages leaves); level l's row0 table (n + 1 ints) holds each utterance's first row and the row count.  The GEMMs run on
// launch_gemm_ragged and the attentive pooling is the RAG instance of rn_attn_pool_kernel (rawnet2.hip); here are the front-end and the
// block tail.
//
// The block tail is rawnet2.hip's small-batch form (rn_tail_part -> rn_afms_gate -> rn_tail_apply) on a segment table: an utterance of Tn_u
// pooled frames is cut into ceil(Tn_u / RN_RAG_SLICE) slices of a CONSTANT RN_RAG_SLICE frames (uncapped: a 20 s file has 35 555 pooled
// frames after block 0, 741 slices), the grid is the pack's slices, and a workgroup finds its (utterance, slice) by bisection of the
// level's slice table (rn_rag_slices builds it from row0, once per pack).  The block output is read twice and written once; the
// un-gated pooled tensor never reaches HBM; the next pre-activation is formed from the gated value in fp32, before its store rounds
// it.  Batch invariance: a slice's sum is walked in an order fixed by the frame index, the channel count and the storage type; an
// utterance's mean adds its own slice sums in slice order; nothing looks at n, at a neighbour or at the device's compute units.
// Pool, sum and gate are rn_tail_kernel's arithmetic per element.
// All HBM-bound: 16-byte accesses along the channel axis.
#include "common.h"
#include "kernels.h"

namespace svhip {

namespace {

constexpr int RR_THREADS = 256;
constexpr int FR_ROWS_PER_THREAD = 8;

// Conv1d(1, 128, 3, stride 3) + bias of one utterance's samples -> x (rn_conv3_front's value, rn_conv3_y's order) and block 0's
// pre-activation lrelu(bn1(x)) from x as stored (rn_bn_act's value).  grid (ceil(maxT1 / rows per workgroup), n): a workgroup stages
// the 3 x rows consecutive samples of ITS utterance through LDS (coalesced 4-byte loads; a frame's three samples are then LDS
// broadcasts, not strided global loads) and a thread owns 16 bytes of channels for FR_ROWS_PER_THREAD frames, so a wave stores 1 KiB of
// consecutive rows per instruction.  cw = [w0 | w1 | w2 | bias] x 128 floats.
template <typename T>
__global__ __launch_bounds__(RR_THREADS) void rn_rag_front_kernel(const float* __restrict__ wav, const int64_t* __restrict__ off,
                                                                  const int* __restrict__ row0, const float* __restrict__ cw,
                                                                  const float* __restrict__ bsc, const float* __restrict__ bsh, float slope,
                                                                  T* __restrict__ x, T* __restrict__ pre) {
    constexpr int CPT = Vec16<T>::N;                    // channels per thread
    constexpr int TPR = 128 / CPT;                      // threads per frame row
    constexpr int RPP = RR_THREADS / TPR;               // frame rows per pass of the workgroup
    constexpr int ROWS = RPP * FR_ROWS_PER_THREAD;
    __shared__ float smp[3 * ROWS];
    const int u = blockIdx.y;
    const int r0 = row0[u], Tu = row0[u + 1] - r0;
    const int t0 = blockIdx.x * ROWS;
    if (t0 >= Tu) return;
    const int nrow = min(ROWS, Tu - t0);
    const float* __restrict__ s = wav + off[u] + 3 * (int64_t)t0;      // 3 (t0 + nrow) <= 3 T1_u <= len[u]
    for (int i = threadIdx.x; i < 3 * nrow; i += RR_THREADS) smp[i] = s[i];
    const int cg = threadIdx.x % TPR, rs = threadIdx.x / TPR;
    const int c0 = cg * CPT;
    float w0[CPT], w1[CPT], w2[CPT], bi[CPT], sc[CPT], sh[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        w0[i] = cw[c0 + i]; w1[i] = cw[128 + c0 + i]; w2[i] = cw[256 + c0 + i]; bi[i] = cw[384 + c0 + i];
        sc[i] = bsc[c0 + i]; sh[i] = bsh[c0 + i];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FR_ROWS_PER_THREAD; ++j) {
        const int r = rs + RPP * j;
        if (r < nrow) {
            const float s0 = smp[3 * r], s1 = smp[3 * r + 1], s2 = smp[3 * r + 2];
            Vec16<T> o, q;
#pragma unroll
            for (int i = 0; i < CPT; ++i) o.set(i, rn_conv3_y(w0[i], w1[i], w2[i], bi[i], s0, s1, s2));
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                const float v = fmaf(o.get(i), sc[i], sh[i]);
                q.set(i, v > 0.0f ? v : slope * v);
            }
            const int64_t at = ((int64_t)r0 + t0 + r) * 128 + c0;
            *reinterpret_cast<Vec16<T>*>(x + at) = o;
            *reinterpret_cast<Vec16<T>*>(pre + at) = q;
        }
    }
}

// slice0[l * ld + u] = sum over v < u of ceil(T_v / RN_RAG_SLICE) at level l, [.. + n] = the level's slices.  grid (levels), one thread each
__global__ void rn_rag_slices_kernel(const int* __restrict__ row0, int ld, int n, int* __restrict__ slice0) {
    if (threadIdx.x != 0) return;
    const int* r = row0 + (int64_t)blockIdx.x * ld;
    int* o = slice0 + (int64_t)blockIdx.x * ld;
    int acc = 0;
    for (int u = 0; u < n; ++u) {
        o[u] = acc;
        acc += (r[u + 1] - r[u] + RN_RAG_SLICE - 1) / RN_RAG_SLICE;
    }
    o[n] = acc;
}

// the utterance of slice sid: the last u with slice0[u] <= sid (every utterance has at least one slice, so slice0 rises strictly)
__device__ __forceinline__ int rr_find_utt(const int* __restrict__ slice0, int n, int sid) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (slice0[mid] <= sid) lo = mid; else hi = mid;
    }
    return lo;
}

// the pooled frame t of an utterance whose in-level rows start at xb (max of the rows 3 t .. 3 t + 2), or its row t
template <typename T, bool POOL, bool NT>
__device__ __forceinline__ Vec16<T> rr_value(const T* xb, int t, int C) {
    constexpr int VEC = Vec16<T>::N;
    if (!POOL) return NT ? ld_nt<T>(xb + (int64_t)t * C) : *reinterpret_cast<const Vec16<T>*>(xb + (int64_t)t * C);
    const T* q = xb + (int64_t)(3 * t) * C;
    const Vec16<T> a = NT ? ld_nt<T>(q) : *reinterpret_cast<const Vec16<T>*>(q);
    const Vec16<T> b = NT ? ld_nt<T>(q + C) : *reinterpret_cast<const Vec16<T>*>(q + C);
    const Vec16<T> d = NT ? ld_nt<T>(q + 2 * C) : *reinterpret_cast<const Vec16<T>*>(q + 2 * C);
    Vec16<T> v;
#pragma unroll
    for (int j = 0; j < VEC; ++j) v.set(j, fmaxf(fmaxf(a.get(j), b.get(j)), d.get(j)));
    return v;
}

// part[sid * C + c] = sum over the frames of slice sid.  grid (slices of the out level)
template <typename T, bool POOL>
__global__ __launch_bounds__(RR_THREADS) void rn_rag_tail_part_kernel(const T* __restrict__ x, const int* __restrict__ row0_in,
                                                                      const int* __restrict__ row0_out, const int* __restrict__ slice0, int n,
                                                                      int C, float* __restrict__ part) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ float red[RR_THREADS * VEC];             // [row group][channel]: (256 / cpr) x C = 256 VEC floats
    const int tid = threadIdx.x, sid = blockIdx.x;
    const int u = rr_find_utt(slice0, n, sid);
    const int s = sid - slice0[u];
    const int Tn = row0_out[u + 1] - row0_out[u];
    const int cpr = C / VEC, rstep = RR_THREADS / cpr;
    const int cc = tid % cpr, r0 = tid / cpr, c = cc * VEC;
    const T* xb = x + (int64_t)row0_in[u] * C + c;
    const int t0 = s * RN_RAG_SLICE, t1 = min(Tn, t0 + RN_RAG_SLICE);
    float sum[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) sum[j] = 0.0f;
#pragma unroll 4
    for (int t = t0 + r0; t < t1; t += rstep) {
        const Vec16<T> v = rr_value<T, POOL, false>(xb, t, C);
#pragma unroll
        for (int j = 0; j < VEC; ++j) sum[j] += v.get(j);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) red[r0 * C + c + j] = sum[j];
    __syncthreads();
    for (int k = tid; k < C; k += RR_THREADS) {
        float a = 0.0f;
        for (int r = 0; r < rstep; ++r) a += red[r * C + k];
        part[(int64_t)sid * C + k] = a;
    }
}

// gate[u, k] = sigmoid(bias[k] + sum_c WT[c][k] mean[c]), mean = (the utterance's slice sums added in slice order) / Tn_u.
// grid (C / 64, n): every workgroup forms the whole mean of its utterance in LDS; lane = output, the four waves split the inputs and
// meet in wave order.  WT = the fc weight transposed, so a wave reads 256 consecutive bytes per input channel.
__global__ __launch_bounds__(RR_THREADS) void rn_rag_gate_kernel(const float* __restrict__ part, const int* __restrict__ row0_out,
                                                                 const int* __restrict__ slice0, int C, const float* __restrict__ WT,
                                                                 const float* __restrict__ bias, float* __restrict__ gate) {
    __shared__ float mean[512];
    __shared__ float red[4][64];
    const int tid = threadIdx.x, u = blockIdx.y;
    const int s0 = slice0[u], s1 = slice0[u + 1];
    const float Tn = (float)(row0_out[u + 1] - row0_out[u]);
    for (int c = tid; c < C; c += RR_THREADS) {
        const float* src = part + (int64_t)s0 * C + c;
        float a = 0.0f;
#pragma unroll 8
        for (int s = 0; s < s1 - s0; ++s) a += src[(int64_t)s * C];
        mean[c] = a / Tn;
    }
    __syncthreads();
    const int lane = tid & 63, ks = tid >> 6;
    const int k = blockIdx.x * 64 + lane, per = C >> 2;
    const float* w = WT + (int64_t)(ks * per) * C + k;
    float acc = 0.0f;
#pragma unroll 8
    for (int c = 0; c < per; ++c) acc = fmaf(w[(int64_t)c * C], mean[ks * per + c], acc);
    red[ks][lane] = acc;
    __syncthreads();
    if (ks == 0) {
        const float a = (((bias[k] + red[0][lane]) + red[1][lane]) + red[2][lane]) + red[3][lane];
        gate[(int64_t)u * C + k] = 1.0f / (1.0f + expf(-a));
    }
}

// y = (v + alpha) gate[u] (null: not stored) and pre = lrelu(nscale y + nshift), v formed as in the part pass.  pre is formed from the
// fp32 y, before its rounding to T: on 16-bit handles the rounding of y (2^-9 y in bf16) would otherwise stand against a
// pre-activation that bn's shift nearly cancels (measured on the seeded test weights, block 0 -> 1, channel 62: 0.026 - 0.030 of the
// local scale in bf16 against 0.004 for the rounding of pre alone).  rn_afms_apply rounds first because its result must equal a
// separate rn_bn_act pass bit for bit; a pack has no such second route.
template <typename T, bool POOL>
__global__ __launch_bounds__(RR_THREADS) void rn_rag_tail_apply_kernel(const T* __restrict__ x, const int* __restrict__ row0_in,
                                                                       const int* __restrict__ row0_out, const int* __restrict__ slice0, int n,
                                                                       int C, const float* __restrict__ alpha, const float* __restrict__ gate,
                                                                       const float* __restrict__ nscale, const float* __restrict__ nshift,
                                                                       float slope, T* __restrict__ y, T* __restrict__ pre) {
    constexpr int VEC = Vec16<T>::N;
    const int tid = threadIdx.x, sid = blockIdx.x;
    const int u = rr_find_utt(slice0, n, sid);
    const int s = sid - slice0[u];
    const int ro = row0_out[u], Tn = row0_out[u + 1] - ro;
    const int cpr = C / VEC, rstep = RR_THREADS / cpr;
    const int cc = tid % cpr, r0 = tid / cpr, c = cc * VEC;
    const T* xb = x + (int64_t)row0_in[u] * C + c;
    float al[VEC], g[VEC], ns[VEC], nh[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        al[j] = alpha[c + j]; g[j] = gate[(int64_t)u * C + c + j];
        ns[j] = nscale[c + j]; nh[j] = nshift[c + j];
    }
    T* yb = y ? y + (int64_t)ro * C + c : nullptr;
    T* pb = pre + (int64_t)ro * C + c;
    const int t0 = s * RN_RAG_SLICE, t1 = min(Tn, t0 + RN_RAG_SLICE);
#pragma unroll 4
    for (int t = t0 + r0; t < t1; t += rstep) {
        const Vec16<T> v = rr_value<T, POOL, true>(xb, t, C);
        Vec16<T> o, q;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float yv = (v.get(j) + al[j]) * g[j];
            o.set(j, yv);
            const float w = fmaf(yv, ns[j], nh[j]);
            q.set(j, w > 0.0f ? w : slope * w);
        }
        if (yb) *reinterpret_cast<Vec16<T>*>(yb + (int64_t)t * C) = o;
        *reinterpret_cast<Vec16<T>*>(pb + (int64_t)t * C) = q;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the shapes the tail kernels are cut for: whole 16-byte chunks, a row of chunks divides the workgroup, the mean fits its LDS array
inline bool tail_shape_ok(int dt, int C) {
    const int vec = dt != DT_F32 ? 8 : 4;
    if (C <= 0 || C > 512 || C % 64 != 0 || C % vec != 0) return false;
    const int cpr = C / vec;
    return cpr <= RR_THREADS && RR_THREADS % cpr == 0;
}

}  // namespace

hipError_t launch_rn_rag_front(const float* wav, const int64_t* off, const int32_t* len, const int* row0, int n, int maxT1, const float* cw,
                               const float* bn_scale, const float* bn_shift, float slope, void* x, void* pre, int dt, hipStream_t stream) {
    if (!wav || !off || !len || !row0 || !cw || !bn_scale || !bn_shift || !x || !pre || n <= 0 || maxT1 <= 0 || !aligned16(x) || !aligned16(pre))
        return hipErrorInvalidValue;
    const int rows = (RR_THREADS / (dt == DT_F32 ? 32 : 16)) * FR_ROWS_PER_THREAD;
    const dim3 grid((maxT1 + rows - 1) / rows, n), block(RR_THREADS);
    if (dt == DT_F32) hipLaunchKernelGGL(rn_rag_front_kernel<float>, grid, block, 0, stream, wav, off, row0, cw, bn_scale, bn_shift, slope, (float*)x, (float*)pre);
    else if (dt == DT_BF16) hipLaunchKernelGGL(rn_rag_front_kernel<bf16_t>, grid, block, 0, stream, wav, off, row0, cw, bn_scale, bn_shift, slope, (bf16_t*)x, (bf16_t*)pre);
    else if (dt == DT_F16) hipLaunchKernelGGL(rn_rag_front_kernel<f16_t>, grid, block, 0, stream, wav, off, row0, cw, bn_scale, bn_shift, slope, (f16_t*)x, (f16_t*)pre);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_rn_rag_slices(const int* row0, int ld, int levels, int n, int* slice0, hipStream_t stream) {
    if (!row0 || !slice0 || ld < n + 1 || levels <= 0 || n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rn_rag_slices_kernel, dim3(levels), dim3(64), 0, stream, row0, ld, n, slice0);
    return hipGetLastError();
}

hipError_t launch_rn_rag_tail_part(const void* x, int dt, bool pool, const int* row0_in, const int* row0_out, const int* slice0, int n, int nslices,
                                   int C, float* part, hipStream_t stream) {
    if (!x || !row0_in || !row0_out || !slice0 || !part || n <= 0 || nslices < n || !tail_shape_ok(dt, C) || !aligned16(x)) return hipErrorInvalidValue;
    const dim3 grid(nslices), block(RR_THREADS);
#define SV_PART(TT, P) hipLaunchKernelGGL((rn_rag_tail_part_kernel<TT, P>), grid, block, 0, stream, (const TT*)x, row0_in, row0_out, slice0, n, C, part)
    if (dt == DT_F16) { if (pool) SV_PART(f16_t, true); else SV_PART(f16_t, false); }
    else if (dt == DT_BF16) { if (pool) SV_PART(bf16_t, true); else SV_PART(bf16_t, false); }
    else if (dt == DT_F32) { if (pool) SV_PART(float, true); else SV_PART(float, false); }
    else return hipErrorInvalidValue;
#undef SV_PART
    return hipGetLastError();
}

hipError_t launch_rn_rag_gate(const float* part, const int* row0_out, const int* slice0, int n, int C, const float* WT, const float* bias, float* gate,
                              hipStream_t stream) {
    if (!part || !row0_out || !slice0 || !WT || !bias || !gate || n <= 0 || C <= 0 || C > 512 || C % 64 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rn_rag_gate_kernel, dim3(C / 64, n), dim3(RR_THREADS), 0, stream, part, row0_out, slice0, C, WT, bias, gate);
    return hipGetLastError();
}

hipError_t launch_rn_rag_tail_apply(const void* x, int dt, bool pool, const int* row0_in, const int* row0_out, const int* slice0, int n, int nslices,
                                    int C, const float* alpha, const float* gate, const float* nscale, const float* nshift, float slope, void* y,
                                    void* pre, hipStream_t stream) {
    if (!x || !row0_in || !row0_out || !slice0 || !alpha || !gate || !nscale || !nshift || !pre || n <= 0 || nslices < n || !tail_shape_ok(dt, C) ||
        !aligned16(x) || !aligned16(y) || !aligned16(pre)) return hipErrorInvalidValue;
    const dim3 grid(nslices), block(RR_THREADS);
#define SV_APPLY(TT, P) hipLaunchKernelGGL((rn_rag_tail_apply_kernel<TT, P>), grid, block, 0, stream, (const TT*)x, row0_in, row0_out, slice0, n, C, \
                                           alpha, gate, nscale, nshift, slope, (TT*)y, (TT*)pre)
    if (dt == DT_F16) { if (pool) SV_APPLY(f16_t, true); else SV_APPLY(f16_t, false); }
    else if (dt == DT_BF16) { if (pool) SV_APPLY(bf16_t, true); else SV_APPLY(bf16_t, false); }
    else if (dt == DT_F32) { if (pool) SV_APPLY(float, true); else SV_APPLY(float, false); }
    else return hipErrorInvalidValue;
#undef SV_APPLY
    return hipGetLastError();
}

}  // namespace svhip
