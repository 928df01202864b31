// block_scan.h — the hand-written workgroup scan of the dense-id kernels (score_cluster.hip) and of the component table (score_linkage.hip).
#pragma once
#include "common.h"

namespace svhip {

// exclusive prefix of `n` over the 256 threads of a workgroup (ws: 4 ints of LDS); *all = the workgroup's sum
__device__ __forceinline__ int block_exclusive(int n, int* ws, int* all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    __syncthreads();                                                   // (ws may still be read from the round before)
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int x = ws[w];
        if (w < wave) before += x;
        sum += x;
    }
    *all = sum;
    return before + incl - n;
}

}  // namespace svhip
