// score_walk.h — the gallery walk of the fused search kernels (score_topk.hip, score_above.hip; gfx950): ONE MFMA loop, an epilogue per kernel.
//
// The MFMA loop of asnorm_fused_kernel: a wave owns 32 queries as the B operand of v_mfma_f32_32x32x2_f32 (exact fp32), gallery blocks of 32
// rows are the A operand, so a lane's 16 accumulators are 16 gallery scores of ONE query, ascending in gallery index.  The grid is query
// tiles x gallery slices.
//   MANY  a workgroup holds 128 queries; its four waves share each gallery block through the double-buffered, XOR-swizzled 16-byte
//         LDS-DMA image.
//   FEW   a launch of at most 32 queries: nothing is shared, so the four waves walk DIFFERENT blocks of the slice and read their A
//         fragments straight from global memory (every byte of the gallery is read once either way).
// Both forms issue the same MFMAs on the same operands in the same order: a score depends on its query row and its gallery row only, bit
// for bit, in whichever kernel, form or launch it is computed.  That is what lets threshold search promise score_topk's bits.
//
// NORM (the calls with statistics): process receives t = fmaf(s, aq + ag, -(bq + bg)) in place of s, one rounding per step (svhip.h): the
// sum of the two a, the sum of the two b, the fused multiply-add.  (aq, bq) are two registers of the lane (a lane holds one query), (ag, bg)
// come from the gallery's table of interleaved pairs, which score_topk_coef writes out to whole blocks of 32 rows (the entries past M
// repeat row M - 1: the last block reads in bounds; the epilogues mask its rows past M).  The 16 rows of a lane are four runs of four:
// rows 32 b + 8 g + 4 h + 0..3, 32 contiguous bytes per g.
//   FEW   the pairs are loaded into registers with the A fragments of the block, ahead of its MFMAs
//   MANY  256 bytes per block travel with the block's DMA image into a ring of four LDS slots (block b + 1 is written while block b - 1
//         is still read, so two slots are not enough); they are read from LDS, where the whole half wave reads one address
// The NORM = false instances take no coefficient path at all.
#pragma once
#include "common.h"
#include "kernels.h"

namespace svhip {

// where a lane stands: query j of its wave's 32, half h of the k range (and of the gallery rows of a block), query `row` of the launch
struct ScoreLane {
    int tid, lane, wave, j, h;
    int64_t row;
    bool valid;
    __device__ __forceinline__ ScoreLane(bool few, int64_t N)
        : tid(threadIdx.x), lane(tid & 63), wave(__builtin_amdgcn_readfirstlane(tid >> 6)), j(lane & 31), h(lane >> 5),
          row(few ? (int64_t)blockIdx.x * 32 + j : (int64_t)blockIdx.x * 128 + wave * 32 + j), valid(row < N) {}
};

// dynamic LDS of an instance: MANY's two block images and NORM's ring of four coefficient slots
constexpr int score_walk_lds_bytes(int D, bool few, bool norm) { return few ? 0 : 2 * 32 * D * 4 + (norm ? 4 * 256 : 0); }

// Walks the gallery blocks [blockIdx.y * per, + per) and hands each block's scores to process(const f32x16& scores, int block):
// scores[r] = score (NORM: t) of gallery row 32 block + (r & 3) + 8 (r >> 2) + 4 h against the lane's query, ascending in r.
// A wave meets its blocks in ascending order.  FEW_QUARTERS says how FEW deals the slice's blocks to the four waves: false, round robin
// (wave w takes blocks w, w + 4, ..: the waves end together, score_topk); true, wave w walks the w-th contiguous quarter (score_above: a
// wave's blocks are then one ascending run of gallery rows, which its CSR order needs; MANY ignores it).  Which wave computes a block does
// not change its scores.
template <int D, bool FEW, bool NORM, bool FEW_QUARTERS, class Process>
__device__ __forceinline__ void score_walk(const ScoreLane& g, const float* Q, int64_t N, const float* G, int64_t M, int per, const float2* qcoef,
                                           const float2* gcoef, char* smem, const Process& process) {
    typedef __attribute__((address_space(3))) void lds_void;
    typedef __attribute__((address_space(1))) const void gbl_void;
    constexpr int CH = D / 4;                       // 16-byte chunks per gallery row
    constexpr int BLK = 32 * D * 4;                 // one block of 32 gallery rows
    constexpr int NDMA = 32 * CH / 256;             // DMA instructions per thread per block
    constexpr int NG = CH / 2;                      // 16-byte A fragments per lane per block
    static_assert(D % 64 == 0 && (32 * CH) % 256 == 0, "block image must be whole 4 KiB DMA rounds with 16-aligned chunk groups");

    const int tid = g.tid, lane = g.lane, wave = g.wave, j = g.j, h = g.h;
    const float* __restrict__ qrow = Q + (g.valid ? g.row : N - 1) * D;
    float aq = 0.0f, bq = 0.0f;
    if (NORM) {
        const float2 c = qcoef[g.valid ? g.row : N - 1];
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

    const int nb_all = (int)((M + 31) / 32);
    const int b_first = min((int64_t)nb_all, (int64_t)blockIdx.y * per);
    const int b_last = (int)min((int64_t)nb_all, (int64_t)b_first + per);

    // gc: the pairs of rows 8 g + 4 h + 0..3 of the block in gc[2 g], gc[2 g + 1]
    // (normalise8: scores 8 half .. 8 half + 7 with gc[0 .. 3] = the pairs of g = 2 half, 2 half + 1)
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
        // nothing to share: a lane reads the half row it multiplies (rows past M repeat row M - 1)
        const int quarter = (per + 3) / 4;
        const int wb_first = FEW_QUARTERS ? min(b_last, b_first + wave * quarter) : b_first + wave;
        const int wb_last = FEW_QUARTERS ? min(b_last, wb_first + quarter) : b_last;
        for (int b = wb_first; b < wb_last; b += FEW_QUARTERS ? 1 : 4) {
            const int64_t r0 = (int64_t)b * 32;
            const int lim = (int)min((int64_t)31, M - 1 - r0);
            const float* __restrict__ arow = G + (r0 + min(j, lim)) * D + h * (D / 2);
            f32x4 af[NG];
#pragma unroll
            for (int t = 0; t < NG; ++t) af[t] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(arow) + t);
            f32x4 gc[8];
            if (NORM) {
                const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(gcoef + r0 + 4 * h);
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) { gc[2 * g4] = src[4 * g4]; gc[2 * g4 + 1] = src[4 * g4 + 1]; }
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
            const int lim = (int)min((int64_t)31, M - 1 - r0);         // the gallery's last block clamps its rows
            const float* bb = G + r0 * D;
#pragma unroll
            for (int q = 0; q < NDMA; ++q) {
                const float* s = bb + min(srow[q], lim) * D + scol[q];
                __builtin_amdgcn_global_load_lds((gbl_void*)s, (lds_void*)(smem + buf * BLK + (q * 256 + wave * 64) * 16), 16, 0, 0);
            }
            if (NORM && wave == 0 && lane < 16)         // the block's 32 pairs: 16 lanes x 16 bytes, lane-linear like the image
                __builtin_amdgcn_global_load_lds((gbl_void*)(gcoef + r0 + 2 * lane), (lds_void*)(smem + 2 * BLK + ((b - b_first) & 3) * 256), 16, 0, 0);
        };
        auto normalised_block = [&](const f32x16& a, int b) {      // with the pairs of block b from their LDS slot
            const char* src = smem + 2 * BLK + ((b - b_first) & 3) * 256 + 32 * h;
            f32x16 t;
#pragma unroll
            for (int half = 0; half < 2; ++half) {                 // (two rounds of 16 registers: D = 256 has no 32 to spare here)
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
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // block b has landed (and the epilogue's stores of one block ago)
                __syncthreads();                                       // ... for every wave; nobody still reads the other buffer
                if (b + 1 < b_last) issue(b + 1, buf ^ 1);
                if (b > b_first) {                                     // the epilogue of the previous block
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
}

// What launch_score_topk and launch_score_above check alike, and the grid (query tiles x gallery slices) of the launch.
inline hipError_t score_walk_launch(int D, const float* Q, int64_t N, const float* G, int64_t M, int per, const float2* qcoef, const float2* gcoef,
                                    bool few, int slices, dim3* grid) {
    if (!score_topk_fused_supported(D) || !Q || !G) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(G)) & 15) return hipErrorInvalidValue;
    if (M < 1 || M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    if (slices < 1 || slices > 65535 || per < 1 || (int64_t)slices * per * 32 < M) return hipErrorInvalidValue;      // every gallery block belongs to a slice
    if (few && N > 32) return hipErrorInvalidValue;
    // the normalised form takes both tables (the gallery's is read in 16-byte pieces) or neither
    if (!qcoef != !gcoef || (reinterpret_cast<uintptr_t>(gcoef) & 15)) return hipErrorInvalidValue;
    *grid = dim3((unsigned)(few ? 1 : (N + 127) / 128), (unsigned)slices);
    return hipSuccess;
}

}  // namespace svhip
