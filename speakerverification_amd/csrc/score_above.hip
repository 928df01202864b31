// score_above.hip — threshold search: every (query, gallery row) pair whose score reaches a threshold, as CSR rows in ascending gallery
// index, WITHOUT the N x M score matrix (gfx950; svhip.h, svhip_score_above_count / _fill).
//
//   score_above_kernel  the operand path of score_topk_kernel (score_topk.hip), MFMA for MFMA: a wave owns 32 queries as the B operand of
//                       v_mfma_f32_32x32x2_f32, gallery blocks of 32 rows are the A operand (MANY: shared by the four waves through the
//                       double-buffered, XOR-swizzled LDS-DMA image; FEW: read straight from global memory), so a score has the bits
//                       score_topk gives the pair.  (A copy, not a shared template: score_topk's instances stay instruction for
//                       instruction what they are, and the two loops differ in how FEW deals the blocks out.)  Another epilogue:
//                         count  a lane adds up its hits (v >= thr, the UPPER mask); one count per list
//                         fill   the same MFMAs in the same order; a lane writes its hits from its list's offset on
//                       A list is a CONTIGUOUS run of gallery blocks of one query: one per slice; FEW: four, wave w walks the w-th quarter
//                       of the slice (score_topk's FEW deals blocks round robin; which wave computes a block does not change its
//                       scores).  The lists of a row, in list order, are therefore in ascending gallery index.  Inside a block the
//                       two lanes of a query (h = 0, 1) hold rows 8 g + 4 h + 0..3: in a block with a hit they exchange their four
//                       per-g hit counts (one cross-lane move of one register) and each places its hits behind what comes before them
//                       in index order.  So the CSR segment is written in ascending index as it is met: no sort, no atomics, and a
//                       position depends on the data only.
//   score_above_scan    per row the sum of its list counts; fill: the lists' offsets inside the row's segment, and the guard
//                       (recount == row_ptr[n + 1] - row_ptr[n]: the first row that differs lands in *bad)
//   score_above_rows    the slab route: one workgroup per row of a score slab, 1024 columns a round, block-wide prefix of the hit counts
#include "common.h"
#include "kernels.h"

namespace svhip {

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;

template <int D, bool FEW, bool NORM, bool FILL>
__global__ __launch_bounds__(256, 2) void score_above_kernel(ScoreAboveParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int CH = D / 4;                       // 16-byte chunks per gallery row
    constexpr int BLK = 32 * D * 4;                 // one block of 32 gallery rows
    constexpr int NDMA = 32 * CH / 256;             // DMA instructions per thread per block
    constexpr int NG = CH / 2;                      // 16-byte A fragments per lane per block
    static_assert(D % 64 == 0 && (32 * CH) % 256 == 0, "block image must be whole 4 KiB DMA rounds with 16-aligned chunk groups");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;         // query within the wave's 32 / half of the gallery rows of a block
    const int64_t row = FEW ? (int64_t)blockIdx.x * 32 + j : (int64_t)blockIdx.x * 128 + wave * 32 + j;
    const bool valid = row < p.N;
    const float* __restrict__ qrow = p.Q + (valid ? row : p.N - 1) * D;
    float aq = 0.0f, bq = 0.0f;
    if (NORM) {
        const float2 c = p.qcoef[valid ? row : p.N - 1];
        aq = c.x; bq = c.y;
    }

    // B operand: q[k], k = h * D/2 + s, for MFMA k-step s (both operands use the same k assignment)
    float eb[D / 2];
#pragma unroll
    for (int t = 0; t < D / 8; ++t) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(qrow + h * (D / 2) + t * 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) eb[t * 4 + u] = v[u];
    }

    const int nb_all = (int)((p.M + 31) / 32);
    const int b_first = min((int64_t)nb_all, (int64_t)blockIdx.y * p.per);
    const int b_last = (int)min((int64_t)nb_all, (int64_t)b_first + p.per);

    // this lane's list: one per slice (FEW: per slice and wave) of its query; the two halves of a query share it
    const int lid = FEW ? (int)blockIdx.y * 4 + wave : (int)blockIdx.y;
    const int64_t lslot = (valid ? row : 0) * p.nl + lid;
    // a hit's gallery index lies in [lo, M): 32-bit, M < 2^31 and a block ends below 2^31 + 32 (UPPER: above row_base + row; no row: nothing)
    const int64_t first = p.upper ? p.row_base + row + 1 : 0;
    const uint32_t lo = valid && first < (int64_t)0xffffffffu ? (uint32_t)first : 0xffffffffu, hi = (uint32_t)p.M;
    int cnt = 0;                                    // count: this lane's hits
    int64_t pos = 0, end = 0;                       // fill: where the list's next hit goes, and where the list ends
    if (FILL && valid) {
        pos = p.loff[lslot];
        end = pos + p.lcnt[lslot];
    }

    // acc[r] = score of gallery row 32 b + (r & 3) + 8 (r >> 2) + 4 h against query j: ascending in r
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
    // NORM: the lane's 16 scores through the statement (svhip.h), as score_topk_kernel: gc[2 g], gc[2 g + 1] the pairs of rows 8 g + 4 h + 0..3
    auto normalise8 = [&](f32x16& t, const f32x16& a, const f32x4* gc, int half) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const f32x4 c = gc[r >> 1];
            const float ag = (r & 1) ? c[2] : c[0], bg = (r & 1) ? c[3] : c[1];
            t[8 * half + r] = __builtin_fmaf(a[8 * half + r], aq + ag, -(bq + bg));
        }
    };
    auto normalised = [&](const f32x16& a, const f32x4* gc) {
        f32x16 t;
        normalise8(t, a, gc, 0);
        normalise8(t, a, gc + 4, 1);
        return t;
    };
    auto mfma_step = [&](f32x16& acc, const f32x4& a4, int t) {
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u], eb[t * 4 + u], acc, 0, 0, 0);
    };

    if (FEW) {
        // nothing to share: wave w takes the w-th quarter of the slice; a lane reads the half row it multiplies (rows past M repeat row M - 1)
        const int quarter = (p.per + 3) / 4;
        const int wb_first = min(b_last, b_first + wave * quarter);
        const int wb_last = min(b_last, wb_first + quarter);
        for (int b = wb_first; b < wb_last; ++b) {
            const int64_t r0 = (int64_t)b * 32;
            const int lim = (int)min((int64_t)31, p.M - 1 - r0);
            const float* __restrict__ arow = p.G + (r0 + min(j, lim)) * D + h * (D / 2);
            f32x4 af[NG];
#pragma unroll
            for (int t = 0; t < NG; ++t) af[t] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(arow) + t);
            f32x4 gc[8];
            if (NORM) {
                const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(p.gcoef + r0 + 4 * h);
#pragma unroll
                for (int g = 0; g < 4; ++g) { gc[2 * g] = src[4 * g]; gc[2 * g + 1] = src[4 * g + 1]; }
            }
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int t = 0; t < NG; ++t) mfma_step(acc, af[t], t);
            if (NORM) process(normalised(acc, gc), b);
            else process(acc, b);
        }
    } else {
        // per-lane source offsets of the NDMA chunks this lane moves per block (block-invariant: row within the block, swizzled chunk)
        int srow[NDMA], scol[NDMA];
#pragma unroll
        for (int q = 0; q < NDMA; ++q) {
            const int pidx = q * 256 + tid;
            const int i = pidx / CH, cs = pidx - i * CH;
            srow[q] = i;
            scol[q] = (cs ^ (i & 15)) * 4;            // the image is lane-linear: the swizzle goes on the source
        }
        auto issue = [&](int b, int buf) {
            const int64_t r0 = (int64_t)b * 32;
            const int lim = (int)min((int64_t)31, p.M - 1 - r0);       // the gallery's last block clamps its rows
            const float* bb = p.G + r0 * D;
#pragma unroll
            for (int q = 0; q < NDMA; ++q) {
                const float* s = bb + min(srow[q], lim) * D + scol[q];
                __builtin_amdgcn_global_load_lds((gbl_void*)s, (lds_void*)(smem + buf * BLK + (q * 256 + wave * 64) * 16), 16, 0, 0);
            }
            if (NORM && wave == 0 && lane < 16)         // the block's 32 pairs: 16 lanes x 16 bytes, lane-linear like the image
                __builtin_amdgcn_global_load_lds((gbl_void*)(p.gcoef + r0 + 2 * lane), (lds_void*)(smem + 2 * BLK + ((b - b_first) & 3) * 256), 16, 0, 0);
        };
        auto normalised_block = [&](const f32x16& a, int b) {      // with the pairs of block b from their LDS slot
            const char* src = smem + 2 * BLK + ((b - b_first) & 3) * 256 + 32 * h;
            f32x16 t;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 gc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) gc[u] = *reinterpret_cast<const f32x4*>(src + 128 * half + 64 * (u >> 1) + 16 * (u & 1));
                normalise8(t, a, gc, half);
                __builtin_amdgcn_sched_barrier(0);
            }
            return t;
        };
        auto rd = [&](int buf, int t) {
            return *reinterpret_cast<const f32x4*>(smem + buf * BLK + j * (D * 4) + (((h * NG + t) ^ (j & 15)) << 4));      // gallery row j of the block
        };
        auto mfma_block = [&](int buf) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            f32x4 a4 = rd(buf, 0);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int t = 0; t < NG; ++t) {
                f32x4 nx = a4;
                if (t + 1 < NG) nx = rd(buf, t + 1);       // one fragment ahead of its MFMAs, fenced (asnorm_fused.hip)
                __builtin_amdgcn_sched_barrier(0);
                mfma_step(acc, a4, t);
                __builtin_amdgcn_sched_barrier(0);
                a4 = nx;
            }
            __builtin_amdgcn_s_setprio(0);
            return acc;
        };
        if (b_first < b_last) {                                    // (workgroup-uniform)
            issue(b_first, 0);
            f32x16 accp;
#pragma unroll
            for (int r = 0; r < 16; ++r) accp[r] = 0.0f;
            for (int b = b_first; b < b_last; ++b) {
                const int buf = (b - b_first) & 1;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // block b has landed (and the hit stores of one block ago)
                __syncthreads();                                       // ... for every wave; nobody still reads the other buffer
                if (b + 1 < b_last) issue(b + 1, buf ^ 1);
                if (b > b_first) {                                     // the hits of the previous block
                    if (NORM) process(normalised_block(accp, b - 1), b - 1);
                    else process(accp, b - 1);
                }
                __builtin_amdgcn_sched_barrier(0);
                accp = mfma_block(buf);
            }
            if (NORM) process(normalised_block(accp, b_last - 1), b_last - 1);
            else process(accp, b_last - 1);
        }
    }
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
    const int lds = FEW ? 0 : 2 * 32 * D * 4 + (NORM ? 4 * 256 : 0);
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
    if (!score_topk_fused_supported(D) || !p.Q || !p.G || !p.lcnt) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(p.Q) | reinterpret_cast<uintptr_t>(p.G)) & 15) return hipErrorInvalidValue;
    if (p.thr != p.thr || p.M < 1 || p.M >= ((int64_t)1 << 31) || p.row_base < 0) return hipErrorInvalidValue;
    if (slices < 1 || slices > 65535 || p.per < 1 || (int64_t)slices * p.per * 32 < p.M) return hipErrorInvalidValue;      // every gallery block belongs to a slice
    if (p.nl != slices * (few ? 4 : 1)) return hipErrorInvalidValue;
    if (few && p.N > 32) return hipErrorInvalidValue;
    if (fill && (!p.loff || !p.out_index || !p.out_score)) return hipErrorInvalidValue;
    // the normalised form takes both tables (the gallery's is read in 16-byte pieces) or neither
    if (!p.qcoef != !p.gcoef || (reinterpret_cast<uintptr_t>(p.gcoef) & 15)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(few ? 1 : (p.N + 127) / 128), (unsigned)slices);
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
