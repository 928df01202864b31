// group_audit.hip — dataset audit (svhip_group_audit; gfx950): per file the number of files of its own group it does not match.
//
// The work is a block-diagonal, crop-batched self-join: s(i, j) = mean_c | cos(F[i, c], F[j, c]) | for the files i, j of one group
// (SVHIP_TRIAL_COSINE's statement), a mismatch iff s <= cut, and one int per file leaves the chip.
//
// MFMA route (D % 32 == 0, D <= 1024, 16-byte aligned F): tiles on the GLOBAL file axis.  Files are sorted by group, so the partners of
// file i are a run of files around it: workgroup (R, y) owns the 64 x 64 tile of row files [64 R, +64) against column files
// [64 (R + y), +64), and exists only while that column tile starts before the group of the row tile's last file ends.  Small groups
// share a tile; the block-diagonal mask is one comparison per score (column j's group starts at gs[j]: i pairs with j > i iff i >= gs[j]).
// Only the pairs j >= i are computed (the upper triangle of the join): a score is computed ONCE, counted for both files with integer
// atomics and written to both places of the score block, so s(i, j) and s(j, i) are the same bits by construction.
//   - the four waves of a workgroup own the four 32 x 32 sub-tiles (the one below the diagonal of a diagonal tile idles);
//   - per crop the operands are the rows F[., c, :] (row stride n_crops * D); they travel through LDS in K slices of 32 floats, double
//     buffered, one barrier per slice; the image is XOR-swizzled by row so that the 16-byte fragment reads spread over the banks;
//   - v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation) in score_walk.h's operand layout: lane (j, h) holds row / column j
//     and the k values h * 16 .. + 15 of a slice, so a dot product is accumulated in ONE order whatever tile, wave or launch computes it;
//   - the norms come from the tile's own loads: the threads that move a row through LDS add up its squares over the slices of a crop
//     and leave max(sqrt(|x|^2), 1e-5) in LDS with the crop's last slice (F is read once; a row's norm has the same bits in every tile);
//   - at the end of a crop the 32 x 32 accumulator is divided by the two clamped norms, goes through |.| and is added to a running
//     sum that stays in registers over the crops;
//   - the epilogue divides by (float)n_crops, compares with cut, reduces the mismatches per row (ballots) and per column (a lane's own
//     16 scores and its partner lane's) and adds them to out_miss; scores are written when they were asked for.
// No float atomics anywhere; a count is a sum of integers, so its value does not depend on the order of the additions.
//
// Plain route (every other width or alignment): no second scoring kernel.  A bounded chunk of the within-group pairs j >= i is
// enumerated into scratch (group_audit_pairs), launch_trial_crops(mode 0) scores it, and group_audit_count compares, counts and scatters.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace svhip {

namespace {

constexpr int GA_TILE = 64;      // files per side of a workgroup's tile
constexpr int GA_KS = 32;        // floats of a K slice

// first index in [0, n) with a[index] > v (a non-decreasing; n when there is none)
__device__ __forceinline__ int64_t upper_bound_i64(const int64_t* __restrict__ a, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// per file: where its group starts and ends, and (sq given) where the group's score block starts
__global__ __launch_bounds__(256) void group_audit_tables_kernel(const int64_t* __restrict__ gp, int64_t n_groups, const int64_t* __restrict__ sq,
                                                                 int64_t n_files, int32_t* __restrict__ gs, int32_t* __restrict__ ge,
                                                                 int64_t* __restrict__ sbase) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_files) return;
    const int64_t u = upper_bound_i64(gp, n_groups + 1, i);      // gp[u - 1] <= i < gp[u], 1 <= u <= n_groups
    gs[i] = (int32_t)gp[u - 1];
    ge[i] = (int32_t)gp[u];
    if (sq) sbase[i] = sq[u - 1];
}

__global__ __launch_bounds__(256) void group_audit_kernel(const GroupAuditParams p, int y_base) {
    __shared__ f32x4 lds[2][2][GA_TILE * (GA_KS / 4)];      // [buffer][row panel | column panel][row * 8 + swizzled chunk]: 32 KiB
    __shared__ __attribute__((aligned(16))) float nlds[2][2][GA_TILE];      // [crop parity][row panel | column panel][row]: clamped norms
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), j = lane & 31, h = lane >> 5;
    const int64_t n = p.n_files;
    const int64_t R = blockIdx.x;
    const int64_t rf = R * GA_TILE;
    const int64_t c_end = p.ge[min(rf + GA_TILE - 1, n - 1)];          // where the group of the tile's last file ends
    const int64_t cf = (R + y_base + (int64_t)blockIdx.y) * GA_TILE;
    if (cf >= c_end) return;                                           // (workgroup-uniform)

    const int wr = wave >> 1, wc = wave & 1;
    const int64_t r0 = rf + 32 * wr, c0 = cf + 32 * wc;
    // a sub-tile works if it holds a pair j >= i of one group: not below the diagonal, and its last row's group reaches its columns
    const bool active = r0 < n && c0 < n && c0 + 31 >= r0 && c0 < (int64_t)p.ge[min(r0 + 31, n - 1)];

    const int C = p.n_crops, D = p.D, nks = D / GA_KS;
    const int64_t rowstride = (int64_t)C * D;
    // the two chunks of each panel this thread moves per slice: rows tid / 8 and tid / 8 + 32 (clamped to the last file), chunk tid % 8
    const int lrow = tid >> 3, lch = tid & 7;
    const float* __restrict__ srcA[2];
    const float* __restrict__ srcB[2];
    int dst[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int row = lrow + 32 * q;
        srcA[q] = p.F + min(rf + row, n - 1) * rowstride + lch * 4;
        srcB[q] = p.F + min(cf + row, n - 1) * rowstride + lch * 4;
        dst[q] = row * 8 + (lch ^ (row & 7));
    }
    f32x4 ra[2], rb[2];
    float qa[2] = {0.0f, 0.0f}, qb[2] = {0.0f, 0.0f};      // |x|^2 of this thread's chunks over the slices of a crop
    auto fetch = [&](int step) {          // step = crop * nks + slice: its floats start (crop * D + slice * 32) into a row
        const int64_t o = (int64_t)step * GA_KS;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            ra[q] = *reinterpret_cast<const f32x4*>(srcA[q] + o);
            rb[q] = *reinterpret_cast<const f32x4*>(srcB[q] + o);
        }
    };
    // the fetched slice goes to LDS; its squares join the row's sum, and the crop's last slice (workgroup-uniform) ends it: the eight
    // threads of a row add up and the clamped norm goes to nlds[crop parity].  A row's norm is summed in ONE order - thread tid % 8 takes
    // the floats 32 s + 4 (tid % 8) + 0..3 of every slice s in turn, then an xor tree over the eight - wherever the row stands.
    auto stash = [&](int buf, bool crop_ends, int parity) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            lds[buf][0][dst[q]] = ra[q];
            lds[buf][1][dst[q]] = rb[q];
#pragma unroll
            for (int u = 0; u < 4; ++u) { qa[q] = fmaf(ra[q][u], ra[q][u], qa[q]); qb[q] = fmaf(rb[q][u], rb[q][u], qb[q]); }
        }
        if (crop_ends) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float a = qa[q], b = qb[q];
#pragma unroll
                for (int o = 1; o < 8; o <<= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
                if (lch == 0) {
                    nlds[parity][0][lrow + 32 * q] = fmaxf(sqrtf(a), 1e-5f);
                    nlds[parity][1][lrow + 32 * q] = fmaxf(sqrtf(b), 1e-5f);
                }
                qa[q] = 0.0f; qb[q] = 0.0f;
            }
        }
    };

    const int64_t jcol = c0 + j;
    const int64_t jc = min(jcol, n - 1);
    f32x16 acc, sum;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.0f; sum[r] = 0.0f; }

    // step s = (crop, ks) is computed from buffer s & 1 while slice s + 1 = (crop1, ks1) is fetched and, after the MFMAs, stashed
    const int steps = C * nks;
    fetch(0);
    stash(0, nks == 1, 0);
    __syncthreads();
    int ks = 0, crop = 0;
    for (int s = 0; s < steps; ++s) {
        const int buf = s & 1;
        const int ks1 = ks + 1 == nks ? 0 : ks + 1, crop1 = ks1 ? crop : crop + 1;
        if (s + 1 < steps) fetch(s + 1);
        if (active) {
            const f32x4* __restrict__ pa = &lds[buf][0][(32 * wr + j) * 8];
            const f32x4* __restrict__ pb = &lds[buf][1][(32 * wc + j) * 8];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 a4 = pa[(h * 4 + t) ^ (j & 7)];
                const f32x4 b4 = pb[(h * 4 + t) ^ (j & 7)];
#pragma unroll
                for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u], b4[u], acc, 0, 0, 0);
            }
            if (ks == nks - 1) {    // the crop ends: | dot / (norm_i * norm_j) | joins the running sum
                // its norms were written with its last slice, one barrier ago: 16 rows (four runs of four) and the lane's column
                const f32x4* __restrict__ nrow = reinterpret_cast<const f32x4*>(&nlds[crop & 1][0][32 * wr + 4 * h]);
                const float nc = nlds[crop & 1][1][32 * wc + j];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    sum[r] += fabsf(acc[r] / (nrow[2 * (r >> 2)][r & 3] * nc));
                    acc[r] = 0.0f;
                }
            }
        }
        // (nlds[crop1 & 1] was last read in the epilogue of crop1 - 2, at least one barrier ago)
        if (s + 1 < steps) stash(buf ^ 1, ks1 == nks - 1, crop1 & 1);
        ks = ks1; crop = crop1;
        __syncthreads();
    }
    if (!active) return;

    // acc / sum[r]: row file r0 + 8 (r >> 2) + 4 h + (r & 3) against column file c0 + j
    const int64_t gsj = p.gs[jc];
    const float fc = (float)C;
    int64_t sb = 0, ng = 0;
    if (p.score) { sb = p.sbase[jc]; ng = (int64_t)p.ge[jc] - gsj; }
    int colcnt = 0, rowcnt = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rl = 8 * (r >> 2) + (r & 3);
        const int64_t i = r0 + rl + 4 * h;
        const float sc = sum[r] / fc;
        const bool pair = jcol < n && i >= gsj && i <= jcol;
        const bool miss = pair && i < jcol && sc <= p.cut;          // (a NaN score compares false: never a mismatch)
        colcnt += miss ? 1 : 0;
        const unsigned long long m = __ballot(miss);
        const int lo = __popcll(m & 0xffffffffull), hi = __popcll(m >> 32);
        if (lane == rl) rowcnt = lo;
        if (lane == rl + 4) rowcnt = hi;
        if (p.score && pair) {
            const int64_t a = i - gsj, b = jcol - gsj;
            p.score[sb + a * ng + b] = sc;
            if (a != b) p.score[sb + b * ng + a] = sc;
        }
    }
    colcnt += __shfl_xor(colcnt, 32, 64);
    if (lane < 32) {
        if (rowcnt > 0) atomicAdd(p.miss + r0 + lane, rowcnt);      // (a counted row is a valid file: i <= j < n_files)
        if (colcnt > 0) atomicAdd(p.miss + jcol, colcnt);
    }
}

// ---- plain route ------------------------------------------------------------------------------------------------------------------
// pair q of a group of n files, rows first: (a, b), a <= b, with q = a n - a (a - 1) / 2 + (b - a)
__device__ __forceinline__ int64_t tri_off(int64_t a, int64_t n) { return a * n - a * (a - 1) / 2; }

// ia / ib [t] = the files of pair p0 + t of the call's pair list (group after group; pp[g] = pairs before group g)
__global__ __launch_bounds__(256) void group_audit_pairs_kernel(const int64_t* __restrict__ gp, const int64_t* __restrict__ pp, int64_t n_groups,
                                                                int64_t p0, int64_t P, int32_t* __restrict__ ia, int32_t* __restrict__ ib) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= P) return;
    const int64_t q_all = p0 + t;
    const int64_t g = upper_bound_i64(pp, n_groups + 1, q_all) - 1;      // pp[g] <= q_all < pp[g + 1]: never an empty group
    const int64_t q = q_all - pp[g], s = gp[g], n = gp[g + 1] - s;
    const double w = 2.0 * (double)n + 1.0;
    int64_t a = (int64_t)((w - sqrt(fmax(w * w - 8.0 * (double)q, 0.0))) * 0.5);
    a = max((int64_t)0, min(a, n - 1));
    while (a > 0 && tri_off(a, n) > q) --a;
    while (a + 1 < n && tri_off(a + 1, n) <= q) ++a;
    ia[t] = (int32_t)(s + a);
    ib[t] = (int32_t)(s + a + (q - tri_off(a, n)));
}

__global__ __launch_bounds__(256) void group_audit_count_kernel(const float* __restrict__ sc, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
                                                                int64_t P, float cut, const int32_t* __restrict__ gs, const int32_t* __restrict__ ge,
                                                                const int64_t* __restrict__ sbase, int32_t* __restrict__ miss, float* __restrict__ score) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= P) return;
    const int32_t a = ia[t], b = ib[t];
    const float s = sc[t];
    if (a != b && s <= cut) { atomicAdd(miss + a, 1); atomicAdd(miss + b, 1); }
    if (score) {
        const int64_t s0 = gs[a], n = (int64_t)ge[a] - s0, base = sbase[a];
        score[base + (a - s0) * n + (b - s0)] = s;
        if (a != b) score[base + (b - s0) * n + (a - s0)] = s;
    }
}

}  // namespace

bool group_audit_mfma_supported(int D) { return D >= GA_KS && D % GA_KS == 0 && D <= 1024; }

hipError_t launch_group_audit_tables(const int64_t* gp, int64_t n_groups, const int64_t* sq, int64_t n_files, int32_t* gs, int32_t* ge, int64_t* sbase,
                                     hipStream_t stream) {
    if (n_files <= 0) return hipSuccess;
    if (!gp || !gs || !ge || n_groups < 1 || (sq && !sbase) || n_files >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_audit_tables_kernel, dim3((unsigned)((n_files + 255) / 256)), dim3(256), 0, stream, gp, n_groups, sq, n_files, gs, ge, sbase);
    return hipGetLastError();
}

hipError_t launch_group_audit(const GroupAuditParams& p, int64_t max_cols, hipStream_t stream) {
    if (p.n_files <= 0) return hipSuccess;
    if (!group_audit_mfma_supported(p.D) || p.n_crops < 1 || !p.F || !p.gs || !p.ge || !p.miss || (p.score && !p.sbase)) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(p.F) & 15) return hipErrorInvalidValue;
    if (p.n_files >= ((int64_t)1 << 31) || max_cols < 1) return hipErrorInvalidValue;
    if ((int64_t)p.n_crops * (p.D / GA_KS) >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const int64_t tiles = (p.n_files + GA_TILE - 1) / GA_TILE;
    max_cols = std::min(max_cols, tiles);
    for (int64_t y0 = 0; y0 < max_cols; y0 += 65535) {       // (column tiles beyond the grid's y range: further launches)
        const dim3 grid((unsigned)tiles, (unsigned)std::min<int64_t>(65535, max_cols - y0));
        hipLaunchKernelGGL(group_audit_kernel, grid, dim3(256), 0, stream, p, (int)y0);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t launch_group_audit_pairs(const int64_t* gp, const int64_t* pp, int64_t n_groups, int64_t p0, int64_t P, int32_t* ia, int32_t* ib,
                                    hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    if (!gp || !pp || !ia || !ib || n_groups < 1 || p0 < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_audit_pairs_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, gp, pp, n_groups, p0, P, ia, ib);
    return hipGetLastError();
}

hipError_t launch_group_audit_count(const float* sc, const int32_t* ia, const int32_t* ib, int64_t P, float cut, const int32_t* gs, const int32_t* ge,
                                    const int64_t* sbase, int32_t* miss, float* score, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    if (!sc || !ia || !ib || !miss || (score && (!gs || !ge || !sbase))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_audit_count_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, sc, ia, ib, P, cut, gs, ge, sbase, miss, score);
    return hipGetLastError();
}

}  // namespace svhip
