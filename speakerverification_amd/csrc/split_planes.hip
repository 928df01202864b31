// split_planes.hip — the streamed operand of the half-plane kernels (h3w_walk.h; gfx950): its max |x|, then its two half planes.
//
// ---- operand scaling of the half-plane forms (round 5) --------------------------------------------------------------------------
// IEEE-half planes have fp16's exponent range: a component beyond 65504 overflows, one below 2^-14 loses bits of its hi part, and lo is a
// subnormal (2^-24 absolute) below 2^-3.  Embeddings are not always unit vectors (the reference scores raw embeddings when `normalize` is
// off: src/model.py:421, utils.py:142-150), so every operand is brought to a fixed magnitude by an EXACT power of two before it is split:
// a row of the register operand by its own max |x| (found in the kernel, per row: H3wWalk::load_operand), the streamed operand by the max |x|
// of the whole matrix (absmax_bits_kernel -> a device word the split pass and the kernels read: no host round trip).  max |x| lands in
// [64, 128): hi is exact to 11 bits and lo a normal half for every component down to 2^-10 of the largest; squares (the AS-norm moment rows)
// stay below 2^14.  Products and sums are formed on the scaled values — binary floating point is scale-invariant, so the fp32 accumulation
// rounds exactly as it would have — and the result is multiplied back by the exact inverse.  Zero rows keep scale 1; inf / NaN stay inf / NaN.
// (pow2_scale_of_bits, pow2_inverse, finite_abs_bits: common.h — round 6: the F32X3 network input uses them too)
#include "common.h"
#include "kernels.h"

namespace svhip {

namespace {

// max |x| over the FINITE elements of a matrix as the bit pattern of a non-negative float (ordered like an unsigned integer): ABSMAX_WGS
// workgroups leave one partial each in part[0 .. ABSMAX_WGS) (no atomics, no zero-fill launch); the consumer's first kernel folds them
// (absmax_fold: 256 loads per workgroup) and its workgroup 0 publishes the result in part[-1] = *pscale for the kernels after it
constexpr int ABSMAX_WGS = 256;
__global__ __launch_bounds__(256) void absmax_bits_kernel(const float* __restrict__ X, int64_t n, uint32_t* __restrict__ part) {
    __shared__ uint32_t wm[4];
    uint32_t m = 0;
    const int64_t n4 = n >> 2;
    const u32x4* __restrict__ X4 = reinterpret_cast<const u32x4*>(X);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const u32x4 v = X4[i];
        m = max(max(m, finite_abs_bits(v[0])), max(max(finite_abs_bits(v[1]), finite_abs_bits(v[2])), finite_abs_bits(v[3])));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = max(m, finite_abs_bits(__float_as_uint(X[(n4 << 2) + threadIdx.x])));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = max(max(wm[0], wm[1]), max(wm[2], wm[3]));
}
// (called by every thread of a 256-thread workgroup)
__device__ __forceinline__ uint32_t absmax_fold(const uint32_t* __restrict__ part) {
    __shared__ uint32_t fm[4];
    uint32_t m = part[threadIdx.x];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) fm[threadIdx.x >> 6] = m;
    __syncthreads();
    return max(max(fm[0], fm[1]), max(fm[2], fm[3]));
}

// fp32 rows -> two half planes [2][rows_total][D] (hi, lo): rows [0, n0) from A (the pseudo-cohort rows MB), the rest from B (the cohort)
// `pscale` (optional): the max-|x| word of B (absmax_bits_kernel): every row is multiplied by s = pow2_scale_of_bits(*pscale), the first
// `sq_rows` rows of A (second-moment rows: products of two cohort values) by s^2
__global__ __launch_bounds__(256) void split2_planes_kernel(const float* __restrict__ A, int n0, const float* __restrict__ B, int n1, int D,
                                                            f16_t* __restrict__ planes, uint32_t* __restrict__ pscale, int sq_rows) {
    const int64_t n = (int64_t)(n0 + n1) * D;
    float sc = 1.0f;
    if (pscale) {           // pscale[1 ..] = the partials of absmax_bits_kernel; pscale[0] <- their maximum, for the kernels behind this one
        const uint32_t bits = absmax_fold(pscale + 1);
        if (blockIdx.x == 0 && threadIdx.x == 0) *pscale = bits;
        sc = pow2_scale_of_bits(bits);
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / D;
        const float v = (r < n0 ? A[i] : B[i - (int64_t)n0 * D]) * (r < sq_rows ? sc * sc : sc);
        const f16_t a = static_cast<f16_t>(v);
        planes[i] = a;
        planes[n + i] = static_cast<f16_t>(v - static_cast<float>(a));
    }
}

}  // namespace

// with pscale: the max |x| of B -> pscale[1 ..] (partials; the split pass folds them into pscale[0]), and the planes hold the scaled rows
hipError_t launch_split_planes(const float* A, int n0, const float* B, int n1, int D, void* planes, uint32_t* pscale, int sq_rows,
                               hipStream_t stream) {
    const int64_t n = (int64_t)(n0 + n1) * D;
    const int64_t g = (n + 255) / 256;
    if (pscale) hipLaunchKernelGGL(absmax_bits_kernel, dim3(ABSMAX_WGS), dim3(256), 0, stream, B, (int64_t)n1 * D, pscale + 1);
    hipLaunchKernelGGL(split2_planes_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, stream, A, n0, B, n1, D,
                       reinterpret_cast<f16_t*>(planes), pscale, sq_rows);
    return hipGetLastError();
}

}  // namespace svhip
