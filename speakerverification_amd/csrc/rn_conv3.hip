// rn_conv3.hip — RawNet2's 'conv' front-end: x = Conv1d(1, 128, kernel_size=3, stride=3, padding=0)(wav) with bias
// (reference models/RawNet2_custom.py:45-52, applied at :166-169; no LayerNorm, no first_bn, no activation behind it).
//
//   x[b, t, c] = w[c, 0] * s[3t] + w[c, 1] * s[3t + 1] + w[c, 2] * s[3t + 2] + bias[c],   t < T1 = (L - 3) / 3 + 1
//
// fp32 arithmetic in the order of rn_conv3_y (common.h), rounded once to the handle's storage type.  The kernel reads 12 bytes
// per frame and writes 128 values: it is bound by its stores.  A thread owns 16 bytes of channels (8 16-bit values or 4 floats)
// for ROWS_PER_THREAD frames, so one wave instruction stores 1 KiB of consecutive frame rows; the per-channel constants stay in
// registers for all of them.  (bf16 / fp16 handles normally skip this kernel: block 0 of rn_block128 reads the waveform itself.)
// Measured at B = 256, fp16, L = 32000: 181 - 185 us = 4.0 TB/s of read + write bytes; non-temporal stores: the same.
#include "common.h"
#include "kernels.h"

namespace svhip {

namespace {

constexpr int CV_THREADS = 256;
constexpr int CV_ROWS_PER_THREAD = 8;

template <typename T> struct Conv3Store;
template <> struct Conv3Store<float> {
    static __device__ __forceinline__ u32x4 pack(const float (&y)[4]) {
        return u32x4{__float_as_uint(y[0]), __float_as_uint(y[1]), __float_as_uint(y[2]), __float_as_uint(y[3])};
    }
};
template <typename H> struct Conv3Store16 {
    static __device__ __forceinline__ u32x4 pack(const float (&y)[8]) {
        return u32x4{Half16<H>::pack2(y[0], y[1]), Half16<H>::pack2(y[2], y[3]), Half16<H>::pack2(y[4], y[5]), Half16<H>::pack2(y[6], y[7])};
    }
};
template <> struct Conv3Store<bf16_t> : Conv3Store16<bf16_t> {};
template <> struct Conv3Store<f16_t> : Conv3Store16<f16_t> {};

// grid (ceil(T1 / rows per block), B); cw = [w0 | w1 | w2 | bias] x 128 floats
template <typename T>
__global__ __launch_bounds__(CV_THREADS) void rn_conv3_front_kernel(const float* __restrict__ wav, const float* __restrict__ cw,
                                                                    T* __restrict__ x, int L, int T1) {
    constexpr int CPT = 16 / (int)sizeof(T);           // channels per thread
    constexpr int TPR = 128 / CPT;                      // threads per frame row
    constexpr int RPP = CV_THREADS / TPR;               // frame rows per pass of the block
    const int b = blockIdx.y;
    const int cg = threadIdx.x % TPR, rs = threadIdx.x / TPR;
    const int c0 = cg * CPT;
    float w0[CPT], w1[CPT], w2[CPT], bi[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        w0[i] = cw[c0 + i]; w1[i] = cw[128 + c0 + i]; w2[i] = cw[256 + c0 + i]; bi[i] = cw[384 + c0 + i];
    }
    const int t_base = blockIdx.x * (RPP * CV_ROWS_PER_THREAD) + rs;
    const float* s = wav + (int64_t)b * L;
    float sv[CV_ROWS_PER_THREAD][3];
#pragma unroll
    for (int j = 0; j < CV_ROWS_PER_THREAD; ++j) {     // every load in flight before the first store (3t + 2 <= 3 T1 - 1 <= L - 1)
        const int t = min(t_base + RPP * j, T1 - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) sv[j][k] = s[3 * t + k];
    }
#pragma unroll
    for (int j = 0; j < CV_ROWS_PER_THREAD; ++j) {
        const int t = t_base + RPP * j;
        float y[CPT];
#pragma unroll
        for (int i = 0; i < CPT; ++i) y[i] = rn_conv3_y(w0[i], w1[i], w2[i], bi[i], sv[j][0], sv[j][1], sv[j][2]);
        if (t < T1) *reinterpret_cast<u32x4*>(x + ((int64_t)b * T1 + t) * 128 + c0) = Conv3Store<T>::pack(y);
    }
}

}  // namespace

hipError_t launch_rn_conv3_front(const float* wav, const float* cw, void* x, int dt, int B, int L, int T1, hipStream_t stream) {
    if (!wav || !cw || !x || B <= 0 || T1 <= 0 || T1 != (L - 3) / 3 + 1) return hipErrorInvalidValue;
    const int rows_per_block = (CV_THREADS / (dt == DT_F32 ? 32 : 16)) * CV_ROWS_PER_THREAD;
    const dim3 grid((T1 + rows_per_block - 1) / rows_per_block, B);
    if (dt == DT_F32) hipLaunchKernelGGL(rn_conv3_front_kernel<float>, grid, dim3(CV_THREADS), 0, stream, wav, cw, static_cast<float*>(x), L, T1);
    else if (dt == DT_BF16) hipLaunchKernelGGL(rn_conv3_front_kernel<bf16_t>, grid, dim3(CV_THREADS), 0, stream, wav, cw, static_cast<bf16_t*>(x), L, T1);
    else if (dt == DT_F16) hipLaunchKernelGGL(rn_conv3_front_kernel<f16_t>, grid, dim3(CV_THREADS), 0, stream, wav, cw, static_cast<f16_t*>(x), L, T1);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace svhip
