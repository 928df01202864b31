// score_above.hip — threshold search: every (query, gallery row) pair whose score reaches a threshold, as CSR rows in ascending gallery
// index, WITHOUT the N x M score matrix (gfx950; svhip.h, svhip_score_above_count / _fill).
//
//   score_above_kernel  the gallery walk of score_walk.h - the ONE walk score_topk_kernel runs, so a score has the bits score_topk gives
//                       the pair - with another epilogue:
//                         count  a lane adds up its hits (v >= thr, the UPPER mask); one count per list
//                         fill   the same MFMAs in the same order; a lane writes its hits from its list's offset on
//                       A list is a CONTIGUOUS run of gallery blocks of one query: one per slice; FEW: four, wave w walks the w-th quarter
//                       of the slice (the walk's FEW_QUARTERS; score_topk's FEW deals blocks round robin).  The lists of a row, in list
//                       order, are therefore in ascending gallery index.  Inside a block the two lanes of a query (h = 0, 1) hold rows
//                       8 g + 4 h + 0..3: in a block with a hit they exchange their four per-g hit counts (one cross-lane move of one
//                       register) and each places its hits behind what comes before them in index order.  So the CSR segment is written
//                       in ascending index as it is met: no sort, no atomics, and a position depends on the data only.
//   score_above_scan    per row the sum of its list counts; fill: the lists' offsets inside the row's segment, and the guard
//                       (recount == row_ptr[n + 1] - row_ptr[n]: the first row that differs lands in *bad)
//   score_above_rows    the slab route: one workgroup per row of a score slab, 1024 columns a round, block-wide prefix of the hit counts
#include "common.h"
#include "kernels.h"
#include "score_walk.h"

namespace svhip {

namespace {

// The walk's epilogue (score_walk.h): count adds up the lane's hits, fill writes them from its list's offset on.
template <int D, bool FEW, bool NORM, bool FILL>
__global__ __launch_bounds__(256, 2) void score_above_kernel(ScoreAboveParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ScoreLane g(FEW, p.N);
    const int h = g.h;
    const bool valid = g.valid;

    // this lane's list: one per slice (FEW: per slice and wave) of its query; the two halves of a query share it
    const int lid = FEW ? (int)blockIdx.y * 4 + g.wave : (int)blockIdx.y;
    const int64_t lslot = (valid ? g.row : 0) * p.nl + lid;
    // a hit's gallery index lies in [lo, M): 32-bit, M < 2^31 and a block ends below 2^31 + 32 (UPPER: above row_base + row; no row: nothing)
    const int64_t first = p.upper ? p.row_base + g.row + 1 : 0;
    const uint32_t lo = valid && first < (int64_t)0xffffffffu ? (uint32_t)first : 0xffffffffu, hi = (uint32_t)p.M;
    int cnt = 0;                                    // count: this lane's hits
    int64_t pos = 0, end = 0;                       // fill: where the list's next hit goes, and where the list ends
    if (FILL && valid) {
        pos = p.loff[lslot];
        end = pos + p.lcnt[lslot];
    }

    auto process = [&](const f32x16& a, int b) {
        const uint32_t kb = (uint32_t)b * 32u + 4u * h;
        uint32_t hits = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t i = kb + (r & 3) + 8 * (r >> 2);
            if (i >= lo && i < hi && a[r] >= p.thr) hits |= 1u << r;                    // (a NaN score fails the comparison)
        }
        if (!FILL) {
            cnt += __popc(hits);
            return;
        }
        if (!__ballot(hits != 0)) return;                                               // (wave-uniform: most blocks hold no hit)
        // the hits of rows 8 g + 4 h + 0..3, g = 0..3, one byte each; the other half's come across the wave
        uint32_t mine = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) mine |= (uint32_t)__popc((hits >> (4 * g)) & 15u) << (8 * g);
        const uint32_t other = (uint32_t)__shfl_xor((int)mine, 32, 64);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cm = (mine >> (8 * g)) & 255, co = (other >> (8 * g)) & 255;
            int64_t w = pos + (h ? co : 0);                                             // h = 1 comes behind the four rows of h = 0
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if ((hits >> (4 * g + u)) & 1u) {
                    if (w < end) {                                                      // (never beyond what the count pass found)
                        p.out_index[w] = (int32_t)(kb + 8 * g + u);
                        p.out_score[w] = a[4 * g + u] + 0.0f;                           // -0 -> +0, as score_topk returns it
                    }
                    ++w;
                }
            }
            pos += cm + co;
        }
    };
    score_walk<D, FEW, NORM, true>(g, p.Q, p.N, p.G, p.M, p.per, p.qcoef, p.gcoef, smem, process);
    if (!FILL) {
        cnt += __shfl_xor(cnt, 32, 64);             // the list of a query: both halves
        if (valid && h == 0) p.lcnt[lslot] = cnt;
    }
}

// one thread per row: the row's nl list counts (a few to a few hundred) in list order
__global__ __launch_bounds__(256) void score_above_scan_kernel(const int32_t* __restrict__ lcnt, int64_t rows, int nl, int64_t* __restrict__ out_count,
                                                               const int64_t* __restrict__ row_ptr, int64_t row0, int64_t* __restrict__ loff,
                                                               unsigned long long* bad) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const int32_t* c = lcnt + row * nl;
    int64_t sum = 0;
    if (!row_ptr) {
        for (int l = 0; l < nl; ++l) sum += c[l];
        out_count[row] = sum;
        return;
    }
    const int64_t start = row_ptr[row];
    for (int l = 0; l < nl; ++l) {
        loff[row * nl + l] = start + sum;
        sum += c[l];
    }
    if (sum != row_ptr[row + 1] - start || (row0 + row == 0 && start != 0)) atomicMin(bad, (unsigned long long)(row0 + row));
}

// The slab route: one workgroup per row of a score slab.  A round takes 1024 columns, four consecutive ones per thread (one 16-byte read:
// the slab's rows are 16-byte aligned); the hit counts of the threads go through a wave prefix and the four waves' totals through LDS.
// NORM: every read of a score goes through the statement's fmaf (score_topk_rows_kernel).  MODE 0: count, 1: compare with row_ptr, 2: write.
template <bool NORM, int MODE>
__global__ __launch_bounds__(256) void score_above_rows_kernel(const float* __restrict__ S, int64_t M, int64_t ld, float thr, int upper, int64_t row_base,
                                                               const float2* __restrict__ qcoef, const float2* __restrict__ gcoef,
                                                               int64_t* __restrict__ out_count, const int64_t* __restrict__ row_ptr, int64_t row0,
                                                               unsigned long long* bad, int32_t* __restrict__ out_index, float* __restrict__ out_score) {
    __shared__ int wsum[2][4];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ s = S + row * ld;
    float aq = 0.0f, bq = 0.0f;
    if (NORM) {
        const float2 c = qcoef[row];
        aq = c.x; bq = c.y;
    }
    const int64_t above = upper ? row_base + row : -1;
    int64_t pos = 0, end = 0, total = 0;
    if (MODE == 2) { pos = row_ptr[row]; end = row_ptr[row + 1]; }
    int round = 0;
    for (int64_t c0 = 0; c0 < M; c0 += 1024, ++round) {
        const int64_t t0 = c0 + 4 * tid;
        float v[4];
        uint32_t hits = 0;
        if (t0 < M) {                                                  // (ld % 4 == 0: the four columns lie inside the row's stride)
            const f32x4 x = *reinterpret_cast<const f32x4*>(s + t0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = x[u];
                if (NORM && t0 + u < M) {
                    const float2 g = gcoef[t0 + u];
                    v[u] = __builtin_fmaf(x[u], aq + g.x, -(bq + g.y));
                }
                if (t0 + u < M && t0 + u > above && v[u] >= thr) hits |= 1u << u;
            }
        }
        const int n = __popc(hits);
        if (MODE != 2) {
            total += n;
            continue;
        }
        int incl = n;                                                  // inclusive prefix over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wsum[round & 1][wave] = incl;
        __syncthreads();                                               // (two buffers: one barrier a round)
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int x = wsum[round & 1][w];
            if (w < wave) before += x;
            all += x;
        }
        int64_t w = pos + before + incl - n;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if ((hits >> u) & 1u) {
                if (w < end) {
                    out_index[w] = (int32_t)(t0 + u);
                    out_score[w] = v[u] + 0.0f;
                }
                ++w;
            }
        }
        pos += all;
    }
    if (MODE == 2) return;
    // the row's count: the threads' totals added up (exact integers: any order)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
    __shared__ int64_t tsum[4];
    if (lane == 0) tsum[wave] = total;
    __syncthreads();
    if (tid != 0) return;
    total = tsum[0] + tsum[1] + tsum[2] + tsum[3];
    if (MODE == 0) out_count[row] = total;
    else if (total != row_ptr[row + 1] - row_ptr[row] || (row0 + row == 0 && row_ptr[0] != 0)) atomicMin(bad, (unsigned long long)(row0 + row));
}

template <int D, bool FEW, bool NORM, bool FILL>
hipError_t launch_above_d(const ScoreAboveParams& p, const dim3& grid, hipStream_t stream) {
    static DeviceOnce attr;
    constexpr int lds = score_walk_lds_bytes(D, FEW, NORM);
    if (!FEW)
        if (hipError_t e = set_max_dynamic_lds(attr, reinterpret_cast<const void*>(score_above_kernel<D, FEW, NORM, FILL>), lds)) return e;
    hipLaunchKernelGGL((score_above_kernel<D, FEW, NORM, FILL>), grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

template <int D, bool NORM>
hipError_t launch_above_form(const ScoreAboveParams& p, bool few, bool fill, const dim3& grid, hipStream_t stream) {
    if (few) return fill ? launch_above_d<D, true, NORM, true>(p, grid, stream) : launch_above_d<D, true, NORM, false>(p, grid, stream);
    return fill ? launch_above_d<D, false, NORM, true>(p, grid, stream) : launch_above_d<D, false, NORM, false>(p, grid, stream);
}

template <bool NORM>
void launch_above_rows_mode(int mode, const float* S, int64_t rows, int64_t M, int64_t ld, float thr, int upper, int64_t row_base, const float2* qcoef,
                            const float2* gcoef, int64_t* out_count, const int64_t* row_ptr, int64_t row0, unsigned long long* bad, int32_t* out_index,
                            float* out_score, hipStream_t stream) {
    auto* kernel = mode == 0 ? score_above_rows_kernel<NORM, 0> : mode == 1 ? score_above_rows_kernel<NORM, 1> : score_above_rows_kernel<NORM, 2>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(256), 0, stream, S, M, ld, thr, upper, row_base, qcoef, gcoef, out_count, row_ptr, row0, bad,
                       out_index, out_score);
}

}  // namespace

hipError_t launch_score_above(const ScoreAboveParams& p, int D, bool few, int slices, bool fill, hipStream_t stream) {
    if (p.N <= 0) return hipSuccess;
    if (!p.lcnt || p.thr != p.thr || p.row_base < 0) return hipErrorInvalidValue;
    if (p.nl != slices * (few ? 4 : 1)) return hipErrorInvalidValue;
    if (fill && (!p.loff || !p.out_index || !p.out_score)) return hipErrorInvalidValue;
    dim3 grid;
    if (hipError_t e = score_walk_launch(D, p.Q, p.N, p.G, p.M, p.per, p.qcoef, p.gcoef, few, slices, &grid)) return e;
    if (p.qcoef) return D == 192 ? launch_above_form<192, true>(p, few, fill, grid, stream) : launch_above_form<256, true>(p, few, fill, grid, stream);
    return D == 192 ? launch_above_form<192, false>(p, few, fill, grid, stream) : launch_above_form<256, false>(p, few, fill, grid, stream);
}

hipError_t launch_score_above_scan(const int32_t* lcnt, int64_t rows, int nl, int64_t* out_count, const int64_t* row_ptr, int64_t row0, int64_t* loff,
                                   unsigned long long* bad, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (!lcnt || nl < 1 || rows >= ((int64_t)1 << 31) || row0 < 0) return hipErrorInvalidValue;
    if (row_ptr ? (!loff || !bad || out_count) : (!out_count || loff || bad)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_above_scan_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, lcnt, rows, nl, out_count, row_ptr, row0, loff, bad);
    return hipGetLastError();
}

hipError_t launch_score_above_rows(const float* S, int64_t rows, int64_t M, int64_t ld, float thr, int upper, int64_t row_base, const float2* qcoef,
                                   const float2* gcoef, int64_t* out_count, const int64_t* row_ptr, int64_t row0, unsigned long long* bad,
                                   int32_t* out_index, float* out_score, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (!S || thr != thr || M < 1 || M >= ((int64_t)1 << 31) || ld < M || (ld & 3) || (reinterpret_cast<uintptr_t>(S) & 15) || rows >= ((int64_t)1 << 31) ||
        row_base < 0 || row0 < 0)
        return hipErrorInvalidValue;
    if (!qcoef != !gcoef) return hipErrorInvalidValue;
    const int mode = out_count ? 0 : bad ? 1 : 2;
    if (mode == 0 ? (row_ptr || bad || out_index || out_score) : mode == 1 ? (!row_ptr || out_index || out_score) : (!row_ptr || !out_index || !out_score))
        return hipErrorInvalidValue;
    if (qcoef) launch_above_rows_mode<true>(mode, S, rows, M, ld, thr, upper, row_base, qcoef, gcoef, out_count, row_ptr, row0, bad, out_index, out_score, stream);
    else launch_above_rows_mode<false>(mode, S, rows, M, ld, thr, upper, row_base, qcoef, gcoef, out_count, row_ptr, row0, bad, out_index, out_score, stream);
    return hipGetLastError();
}

}  // namespace svhip
