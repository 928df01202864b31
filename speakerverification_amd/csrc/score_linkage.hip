// score_linkage.hip — average / complete linkage cut at thr, INSIDE the components of the threshold graph (gfx950; svhip.h,
// svhip_cluster_linkage).  Every merge of either linkage at a level >= thr needs a pair with v >= thr, so a cluster never leaves its
// component: cluster_above's machinery finds the components, this file refines each one on its own, one workgroup per component.
//
//   linkage_count / _blocksum / _scan / _offsets / _members   the component table ("linkage_table"): rows per dense component id
//                       (integer atomics), an exclusive scan to offsets (block_scan.h's workgroup scan, cluster_ids' scheme: blocks of
//                       1024 ids, ONE workgroup scans the block sums), the member lists through an atomic cursor, and three work lists
//                       of component ids by size.  The order inside a member list and inside a work list is whatever the atomics gave:
//                       the owning workgroup sorts its members, and which workgroup owns a component changes no bit of its result.
//   linkage_agglo_kernel<LINKAGE, NORM, IN_LDS>   ("linkage_agglo") one workgroup per component of m >= 2 rows:
//       sort      the members ascending (rank sort in LDS): slot k is the k-th smallest row, so a cluster's slot - that of its smallest
//                 member - orders clusters as the statement's tie rule does
//       fill      v for every pair of slots i < j ONCE, written to (i, j) and (j, i): one fmaf chain over d = 0 .. D - 1, then the
//                 coefficient epilogue; NaN -> -inf.  Plain FMAs: a component of the bench's data has 8 - 66 rows
//       cache     per row k the best partner j > k (largest g, then smallest j): one wave per row
//       merge     argmax over the cached bests (largest g, then smallest k: the smallest (min A, min B)); stop unless g >= thr;
//                 L(a, k) <- L(a, k) (+ | fminf) L(b, k) for every live k, row and column of the surviving slot a < b; a row k < a whose
//                 partner was a or b, a row a < k < b whose partner was b, and row a itself are rescanned (a wave each), every other
//                 row k < a only compares the one entry that changed with its cache
//       roots     out_root[row] = the row of the slot its merge chain ends in
//     Three barriers per merge, all in workgroup-uniform control flow (every thread reads the same argmax words).  IN_LDS: the matrix
//     is m x (m | 1) floats of LDS (the odd stride keeps the column writes of a merge off one bank); otherwise the same body over an
//     m x m block of the scratch pool, which only this workgroup touches (__syncthreads orders a workgroup's global accesses); the
//     components of that list run in rounds whose matrices fit the pool (linkage_rounds_kernel; kernels.h).
#include <algorithm>

#include "block_scan.h"
#include "common.h"
#include "kernels.h"
#include "../../include/svhip.h"

namespace svhip {

namespace {

constexpr int TABLE_BLOCK = 1024;      // ids per workgroup of the table's scan, four per thread (cluster_ids' blocks)

// ---- the component table ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void linkage_count_kernel(const int32_t* __restrict__ comp, int64_t N, int32_t* cnt, int32_t* n_work,
                                                            unsigned long long* n_unrefined) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 4) n_work[i] = 0;
    if (i == 0) *n_unrefined = 0;
    if (i < N) atomicAdd(cnt + comp[i], 1);
}

__device__ __forceinline__ int four_counts(const int32_t* __restrict__ cnt, int64_t N, int64_t i0, int (&c)[4]) {
    int s = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        c[u] = i0 + u < N ? cnt[i0 + u] : 0;
        s += c[u];
    }
    return s;
}

__global__ __launch_bounds__(256) void linkage_blocksum_kernel(const int32_t* __restrict__ cnt, int64_t N, int32_t* __restrict__ bsum) {
    __shared__ int ws[4];
    int c[4], all;
    block_exclusive(four_counts(cnt, N, (int64_t)blockIdx.x * TABLE_BLOCK + 4 * threadIdx.x, c), ws, &all);
    if (threadIdx.x == 0) bsum[blockIdx.x] = all;
}

// ONE workgroup: bsum[b] <- the rows of the blocks before b (the sum of all sizes is N < 2^31)
__global__ __launch_bounds__(256) void linkage_scan_kernel(int32_t* __restrict__ bsum, int64_t nb) {
    __shared__ int ws[4];
    int carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        int all;
        const int before = block_exclusive(b < nb ? bsum[b] : 0, ws, &all);
        if (b < nb) bsum[b] = carry + before;
        carry += all;
    }
}

// offsets, cursors and the work lists (an id behind the last component has no rows and is on no list)
__global__ __launch_bounds__(256) void linkage_offsets_kernel(LinkageTable t, int64_t N, int small_rows, int lds_rows,
                                                              unsigned long long* n_unrefined) {
    __shared__ int ws[4];
    const int64_t i0 = (int64_t)blockIdx.x * TABLE_BLOCK + 4 * threadIdx.x;
    int c[4], all;
    int at = t.bsum[blockIdx.x] + block_exclusive(four_counts(t.cnt, N, i0, c), ws, &all);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (i0 + u >= N) break;
        t.off[i0 + u] = at;
        t.cursor[i0 + u] = at;
        at += c[u];
        if (c[u] > LINKAGE_MAX_ROWS) atomicAdd(n_unrefined, 1ull);
        else if (c[u] >= 2) {
            const int list = c[u] <= small_rows ? 0 : c[u] <= lds_rows ? 1 : 2;
            t.work[list * t.work_stride + atomicAdd(t.n_work + list, 1)] = (int32_t)(i0 + u);
        }
    }
}

// ONE thread: list 2 in list order into rounds whose matrices fit the pool (any packing gives the same labels)
__global__ void linkage_rounds_kernel(LinkageTable t, int64_t pool_floats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int n = t.n_work[2];
    int round = 0;
    int64_t used = 0;
    for (int w = 0; w < n; ++w) {
        const int64_t m = t.cnt[t.work[2 * t.work_stride + w]], need = m * m;
        if (used + need > pool_floats) { ++round; used = 0; }
        t.round[w] = round;
        t.place[w] = (int32_t)used;
        used += need;
    }
    t.n_work[3] = n ? round + 1 : 0;
}

__global__ __launch_bounds__(256) void linkage_members_kernel(const int32_t* __restrict__ comp, int64_t N, LinkageTable t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int32_t c = comp[i], m = t.cnt[c];
    if (m >= 2 && m <= LINKAGE_MAX_ROWS) t.members[atomicAdd(t.cursor + c, 1)] = (int32_t)i;
}

// ---- the agglomeration --------------------------------------------------------------------------------------------------------------------
constexpr float NEG_INF = -__builtin_huge_valf();

// is the candidate (g, j) ahead of (bv, bj)?  Largest g, then smallest index; j < 0 is no candidate, bj < 0 none yet; a NaN g never is
__device__ __forceinline__ bool ahead(float g, int j, float bv, int bj) { return j >= 0 && g == g && (bj < 0 || g > bv || (g == bv && j < bj)); }

__device__ __forceinline__ void wave_best(float& v, int& j) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oj = __shfl_xor(j, off, 64);
        if (ahead(ov, oj, v, j)) { v = ov; j = oj; }
    }
}

template <int LINKAGE>
__device__ __forceinline__ float link_value(float L, int na, int nb) {
    return LINKAGE == SVHIP_LINKAGE_AVERAGE ? L / (float)(na * nb) : L;      // (na nb <= LINKAGE_MAX_ROWS^2 / 4 < 2^24: the product is exact)
}

// one chain over d, whatever the alignment
__device__ __forceinline__ float dot_chain(const float* __restrict__ x, const float* __restrict__ y, int D, bool vec) {
    float v = 0.0f;
    if (vec) {
        for (int d = 0; d < D; d += 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(x + d), b = *reinterpret_cast<const f32x4*>(y + d);
#pragma unroll
            for (int u = 0; u < 4; ++u) v = __builtin_fmaf(a[u], b[u], v);
        }
    } else {
        for (int d = 0; d < D; ++d) v = __builtin_fmaf(x[d], y[d], v);
    }
    return v;
}

// the LDS of a launch whose components have at most `rows` rows: [matrix (IN_LDS)] | 6 arrays of `rows` words | 16 words
inline size_t agglo_lds_bytes(int rows, bool in_lds) { return ((in_lds ? (size_t)rows * (rows | 1) : 0) + (size_t)6 * rows + 16) * 4; }

template <int LINKAGE, bool NORM, bool IN_LDS>
__global__ __launch_bounds__(256) void linkage_agglo_kernel(LinkageParams p, int list, int rows, int round) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const mat_lds = reinterpret_cast<float*>(smem);
    int* const vec = reinterpret_cast<int*>(smem) + (IN_LDS ? (size_t)rows * (rows | 1) : 0);
    int* const mem = vec;                                              // slot -> row, ascending
    int* const sz = vec + rows;                                        // rows of the slot's cluster; 0: merged away
    float* const bestv = reinterpret_cast<float*>(vec + 2 * rows);     // per live slot k: the best g over the live slots j > k ...
    int* const bestj = vec + 3 * rows;                                 // ... and that j (-1: none)
    int* const par = vec + 4 * rows;                                   // the slot this one was merged into
    int* const lst = vec + 5 * rows;                                   // the unsorted members, then the rows to rescan
    int* const red = vec + 6 * rows;                                   // [0..3] / [4..7]: the waves' argmax (value / slot); [8]: rows in lst
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!IN_LDS && round >= p.t.n_work[3]) return;                     // (an empty round)
    const int n_work = p.t.n_work[list];
    const bool vec4 = (reinterpret_cast<uintptr_t>(p.E) & 15) == 0 && (p.D & 3) == 0;

    for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
        if (!IN_LDS && p.t.round[w] != round) continue;                // (workgroup-uniform)
        const int c = p.t.work[list * p.t.work_stride + w];
        const int m = p.t.cnt[c], first = p.t.off[c];
        if (m > rows) continue;                                        // (never: the work lists are cut by size; workgroup-uniform)
        const int ld = IN_LDS ? (m | 1) : m;
        float* const M = IN_LDS ? mat_lds : p.pool + p.t.place[IN_LDS ? 0 : w];
        __syncthreads();                                               // (the component before is done with the arrays)
        for (int k = tid; k < m; k += 256) lst[k] = p.t.members[first + k];
        __syncthreads();
        for (int k = tid; k < m; k += 256) {
            const int x = lst[k];
            int below = 0;
            for (int j = 0; j < m; ++j) below += lst[j] < x;
            mem[below] = x;
            sz[k] = 1;
            par[k] = k;
        }
        __syncthreads();
        // fill: slot pairs i < j, row r of the walk carrying the pairs of slot r and then those of slot m - 1 - r (m - 1 in all)
        const int half = (m + 1) / 2, total = half * (m - 1);
        for (int q = tid; q < total; q += 256) {
            const int r = q / (m - 1), e = q - r * (m - 1);
            int i, j;
            if (e < m - 1 - r) { i = r; j = r + 1 + e; }
            else {
                i = m - 1 - r; j = i + 1 + (e - (m - 1 - r));
                if (i == r) continue;                                  // (m odd: the middle slot's pairs were the first branch's)
            }
            const int ri = mem[i], rj = mem[j];
            float v = dot_chain(p.E + (int64_t)ri * p.D, p.E + (int64_t)rj * p.D, p.D, vec4);
            if (NORM) {
                const float2 ci = p.coef[ri], cj = p.coef[rj];
                v = __builtin_fmaf(v, ci.x + cj.x, -(ci.y + cj.y));
            }
            if (v != v) v = NEG_INF;
            M[(size_t)i * ld + j] = v;
            M[(size_t)j * ld + i] = v;
        }
        __syncthreads();
        // a wave rescans row k: the best live j > k.  (a, b, nab): the merge under way - slot a already counts nab rows, b is gone
        auto rescan = [&](int k, int a, int b, int nab) {
            const int nk = k == a ? nab : sz[k];
            float bv = NEG_INF;
            int bj = -1;
            for (int j = k + 1 + lane; j < m; j += 64) {
                const int nj = j == a ? nab : j == b ? 0 : sz[j];
                if (nj == 0) continue;
                const float g = link_value<LINKAGE>(M[(size_t)k * ld + j], nk, nj);
                if (ahead(g, j, bv, bj)) { bv = g; bj = j; }
            }
            wave_best(bv, bj);
            if (lane == 0) { bestv[k] = bv; bestj[k] = bj; }
        };
        for (int k = wave; k < m; k += 4) rescan(k, -1, -1, 0);
        __syncthreads();

        for (int merges = 1; merges < m && !p.fill_only; ++merges) {    // (m - 1 merges leave one cluster)
            // 1. argmax over the cached bests
            float gv = NEG_INF;
            int a = -1;
            for (int k = tid; k < m; k += 256)
                if (sz[k] > 0 && bestj[k] >= 0 && ahead(bestv[k], k, gv, a)) { gv = bestv[k]; a = k; }
            wave_best(gv, a);
            if (lane == 0) { reinterpret_cast<float*>(red)[wave] = gv; red[4 + wave] = a; }
            if (tid == 0) red[8] = 0;
            __syncthreads();
            gv = NEG_INF; a = -1;
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const float ov = reinterpret_cast<float*>(red)[x];
                const int oa = red[4 + x];
                if (ahead(ov, oa, gv, a)) { gv = ov; a = oa; }
            }
            if (a < 0 || !(gv >= p.thr)) break;                        // (every thread read the same words)
            const int b = bestj[a], na = sz[a], nb = sz[b], nab = na + nb;
            // 2. the surviving slot's row and column; who has to look again
            for (int k = tid; k < m; k += 256) {
                const int nk = sz[k];
                if (nk == 0 || k == a || k == b) continue;
                const float la = M[(size_t)a * ld + k], lb = M[(size_t)b * ld + k];
                const float L = LINKAGE == SVHIP_LINKAGE_AVERAGE ? la + lb : fminf(la, lb);
                M[(size_t)a * ld + k] = L;
                M[(size_t)k * ld + a] = L;
                if (k < a) {
                    const int bj = bestj[k];
                    if (bj == a || bj == b) lst[atomicAdd(red + 8, 1)] = k;
                    else {
                        const float g = link_value<LINKAGE>(L, nab, nk);
                        if (ahead(g, a, bestv[k], bj)) { bestv[k] = g; bestj[k] = a; }
                    }
                } else if (k < b && bestj[k] == b) lst[atomicAdd(red + 8, 1)] = k;
            }
            if (tid == 0) lst[atomicAdd(red + 8, 1)] = a;
            __syncthreads();
            // 3. the merge itself and the rescans
            if (tid == 0) { sz[a] = nab; sz[b] = 0; par[b] = a; }
            const int n_again = red[8];
            for (int x = wave; x < n_again; x += 4) rescan(lst[x], a, b, nab);
            __syncthreads();
        }
        __syncthreads();
        for (int k = tid; k < m; k += 256) {
            int r = k;
            while (par[r] != r) r = par[r];
            p.root[mem[k]] = mem[r];
        }
    }
}

template <int LINKAGE, bool NORM, bool IN_LDS>
hipError_t launch_agglo_form(const LinkageParams& p, int list, int rows, int round, unsigned grid, hipStream_t stream) {
    static DeviceOnce attr;
    const int lds = (int)agglo_lds_bytes(rows, IN_LDS);
    if (lds > 64 * 1024 - 512)
        if (hipError_t e = set_max_dynamic_lds(attr, reinterpret_cast<const void*>(linkage_agglo_kernel<LINKAGE, NORM, IN_LDS>), (int)agglo_lds_bytes(IN_LDS ? LINKAGE_LDS_ROWS : LINKAGE_MAX_ROWS, IN_LDS))) return e;
    hipLaunchKernelGGL((linkage_agglo_kernel<LINKAGE, NORM, IN_LDS>), dim3(grid), dim3(256), lds, stream, p, list, rows, round);
    return hipGetLastError();
}

template <bool IN_LDS>
hipError_t launch_agglo_home(const LinkageParams& p, int list, int rows, int round, unsigned grid, hipStream_t stream) {
    if (p.linkage == SVHIP_LINKAGE_AVERAGE)
        return p.coef ? launch_agglo_form<SVHIP_LINKAGE_AVERAGE, true, IN_LDS>(p, list, rows, round, grid, stream)
                      : launch_agglo_form<SVHIP_LINKAGE_AVERAGE, false, IN_LDS>(p, list, rows, round, grid, stream);
    return p.coef ? launch_agglo_form<SVHIP_LINKAGE_COMPLETE, true, IN_LDS>(p, list, rows, round, grid, stream)
                  : launch_agglo_form<SVHIP_LINKAGE_COMPLETE, false, IN_LDS>(p, list, rows, round, grid, stream);
}

inline unsigned blocks_of(int64_t N, int per) { return (unsigned)((N + per - 1) / per); }

}  // namespace

hipError_t launch_linkage_table(const int32_t* comp, int64_t N, int lds_rows, const LinkageTable& t, unsigned long long* n_unrefined,
                                hipStream_t stream) {
    if (N <= 0) return hipSuccess;
    if (!comp || !n_unrefined || !t.cnt || !t.off || !t.cursor || !t.members || !t.bsum || !t.work || !t.n_work || !t.round || !t.place || t.work_stride < N / 2 + 1 ||
        N >= ((int64_t)1 << 31) || lds_rows < 2 || lds_rows > LINKAGE_LDS_ROWS)
        return hipErrorInvalidValue;
    const int64_t nb = cluster_id_blocks(N);
    if (hipError_t e = hipMemsetAsync(t.cnt, 0, (size_t)N * 4, stream)) return e;
    hipLaunchKernelGGL(linkage_count_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, stream, comp, N, t.cnt, t.n_work, n_unrefined);
    hipLaunchKernelGGL(linkage_blocksum_kernel, dim3((unsigned)nb), dim3(256), 0, stream, t.cnt, N, t.bsum);
    hipLaunchKernelGGL(linkage_scan_kernel, dim3(1), dim3(256), 0, stream, t.bsum, nb);
    hipLaunchKernelGGL(linkage_offsets_kernel, dim3((unsigned)nb), dim3(256), 0, stream, t, N, std::min(LINKAGE_SMALL_ROWS, lds_rows), lds_rows, n_unrefined);
    hipLaunchKernelGGL(linkage_rounds_kernel, dim3(1), dim3(64), 0, stream, t, linkage_pool_floats(N));
    hipLaunchKernelGGL(linkage_members_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, stream, comp, N, t);
    return hipGetLastError();
}

hipError_t launch_linkage_agglo(const LinkageParams& p, int lds_rows, bool pool, int num_cu, hipStream_t stream) {
    if (p.N < 2) return hipSuccess;
    if (!p.E || !p.root || !p.pool || p.D < 1 || p.thr != p.thr || lds_rows < 2 || lds_rows > LINKAGE_LDS_ROWS ||
        (p.linkage != SVHIP_LINKAGE_AVERAGE && p.linkage != SVHIP_LINKAGE_COMPLETE))
        return hipErrorInvalidValue;
    const int cu = num_cu > 0 ? num_cu : 256;
    const int small = std::min(LINKAGE_SMALL_ROWS, lds_rows);
    const int64_t most = p.N / 2;                                      // components of at least two rows
    // every workgroup strides over its work list, whose length only the device knows; the grids are sized for the chip
    if (!pool) {
        if (hipError_t e = launch_agglo_home<true>(p, 0, small, 0, (unsigned)std::min<int64_t>(most, 8 * (int64_t)cu), stream)) return e;
        if (lds_rows > small && p.N > small)
            if (hipError_t e = launch_agglo_home<true>(p, 1, lds_rows, 0, (unsigned)std::min<int64_t>(std::max<int64_t>(1, p.N / (small + 1)), cu), stream)) return e;
        return hipSuccess;
    }
    if (p.N > lds_rows) {
        const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>(1, p.N / (lds_rows + 1)), cu);
        const int64_t rounds = linkage_max_rounds(p.N);
        for (int64_t r = 0; r < rounds; ++r)
            if (hipError_t e = launch_agglo_home<false>(p, 2, (int)std::min<int64_t>(p.N, LINKAGE_MAX_ROWS), (int)r, grid, stream)) return e;
    }
    return hipSuccess;
}

}  // namespace svhip
