// asnorm_fused.hip — AS-norm cohort statistics WITHOUT the N x K score matrix (gfx950).
//
// Reference: src/utils.py:142-146 — per embedding e: S = cohort @ e, sort descending, keep [:top], mean / population std.
// The slab path (score.hip + the fp32 GEMM) wrote all N x K scores to HBM and read them back (28.8 GB each way for 1.2 M
// embeddings against 5 994 cohort speakers).  Here the scores live only in MFMA accumulators:
//
//   * a wave owns 32 embeddings as the B operand of v_mfma_f32_32x32x2_f32 (exact fp32), D / 2 VGPRs per lane, loaded once;
//     cohort rows stream through LDS in blocks of 32 (the A operand; one 16-byte-per-lane LDS-DMA image per block, XOR-swizzled
//     on the source chunk so that the ds_read_b128 lane groups are conflict-free), shared by the workgroup's four waves;
//   * with the cohort as A, a lane's 16 accumulators are 16 cohort scores of ONE embedding (C/D map: column = lane & 31), so the
//     selection is lane-local: a score above the embedding's threshold tau is appended to that lane's candidate list in a
//     handle-owned buffer (two lists of 256 per embedding: lanes l and l + 32), everything else is dropped;
//   * tau needs the row's first two score moments BEFORE the pass.  They are exact and cheap:  mean_k(e . c_k) = e . cbar and
//     mean_k (e . c_k)^2 = e^T M e with M = C^T C / K (D x D), so M's rows and cbar go through the same MFMA loop as D / 32 + 1
//     leading pseudo-cohort blocks; tau = mean + z sd with z the normal quantile that leaves ~1.6 top candidates;
//   * asnorm_cand_stats_kernel then selects the exact top-`top` of each embedding's <= 512 candidates (score_select.h) —
//     every score above tau is a candidate, so the answer is exact whenever top <= count and no list overflowed; the rare
//     embedding for which that fails (cohort scores far from normal) is flagged and redone by the slab path.
//
// Work per embedding: 2 K D FLOP on the fp32 matrix pipe (157 TFLOP/s peak), ~K/32 x 24 KB of LDS-DMA per 128 embeddings from an
// L2 / Infinity-Cache resident cohort, ~1.6 top x 4 bytes of candidate stores.
#include <type_traits>

#include "common.h"
#include "h3w_walk.h"
#include "kernels.h"
#include "score_select.h"

namespace svhip {

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;

constexpr int AF_CAPL = ASNORM_CAND_PER_LANE;      // candidate slots per lane (2 lanes per embedding)

template <int D>
__global__ __launch_bounds__(256, 2) void asnorm_fused_kernel(AsnormFusedParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int CH = D / 4;                       // 16-byte chunks per cohort row
    constexpr int BLK = 32 * D * 4;                 // one block of 32 cohort rows
    constexpr int NDMA = 32 * CH / 256;             // DMA instructions per thread per block
    constexpr int NP = D / 32 + 1;                  // pseudo-cohort blocks: rows of M, then cbar
    static_assert(D % 64 == 0 && (32 * CH) % 256 == 0, "block image must be whole 4 KiB DMA rounds with 16-aligned chunk groups");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;         // embedding within the wave's 32 / half of the k range (and of the cohort rows of a block)
    const int64_t row = (int64_t)blockIdx.x * 128 + wave * 32 + j;
    const bool valid = row < p.N;
    const float* __restrict__ erow = p.E + (valid ? row : p.N - 1) * D;

    // B operand: e[k], k = h * D/2 + s, for MFMA k-step s (both operands use the same k assignment, so any is as good as 0, 1, 2 ..)
    float eb[D / 2];
#pragma unroll
    for (int t = 0; t < D / 8; ++t) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(erow + h * (D / 2) + t * 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) eb[t * 4 + u] = v[u];
    }

    const int nc = (p.K + 31) / 32;
    const int nb = NP + nc;
    // per-lane source offsets of the NDMA chunks this lane moves per block (block-invariant: row within the block, swizzled chunk)
    int srow[NDMA], scol[NDMA];
#pragma unroll
    for (int q = 0; q < NDMA; ++q) {
        const int pidx = q * 256 + tid;               // position of this lane's chunk in the block image
        const int i = pidx / CH, cs = pidx - i * CH;
        srow[q] = i;
        scol[q] = (cs ^ (i & 15)) * 4;                // the image is lane-linear: the swizzle goes on the source
    }
    auto issue = [&](int b, int buf) {
        const bool pseudo = b < NP;
        const float* base = pseudo ? p.MB : p.cohort;
        const int r0 = pseudo ? b * 32 : (b - NP) * 32;
        const int limit = pseudo ? D + 31 : p.K - 1;
        const float* bb = base + (int64_t)r0 * D;
        const bool ragged = r0 + 31 > limit;          // wave-uniform: only the cohort's last block clamps its rows
#pragma unroll
        for (int q = 0; q < NDMA; ++q) {
            const int i = ragged ? min(srow[q], limit - r0) : srow[q];
            const float* s = bb + i * D + scol[q];
            __builtin_amdgcn_global_load_lds((gbl_void*)s, (lds_void*)(smem + buf * BLK + (q * 256 + wave * 64) * 16), 16, 0, 0);
        }
    };
    // A fragments (16-byte reads: four k-steps each) are requested NG1 groups ahead of their MFMAs (left alone hipcc issues each
    // ds_read right in front of the wait of the four MFMAs that use it).
    // Read-ahead depth NG1, measured on one box with two builds (1.2 M x 5 994, ms end to end):
    // none 26.1 - 26.4 (another box), 1 group 26.7 - 26.9, half a block (12) 27.5 - 29.3: the partner wave already covers the LDS
    // latency, and the deeper variants only cost registers.  PMC of this kernel (profiles/r03_asnorm_pmc.txt): matrix pipe busy
    // 0.80 of the CU cycles at 2.13 - 2.23 GHz, no LDS bank conflicts, LDS array 5 % active.
    constexpr int NG = CH / 2, NG1 = 1;
    f32x4 af[NG];
    auto rd = [&](int buf, int t) {
        return *reinterpret_cast<const f32x4*>(smem + buf * BLK + j * (D * 4) + (((h * NG + t) ^ (j & 15)) << 4));      // cohort row j of the block (A: row = lane & 31)
    };
    auto read_first = [&](int buf) {
#pragma unroll
        for (int t = 0; t < NG1; ++t) af[t] = rd(buf, t);
    };
    auto mfma_block = [&](int buf) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int t = 0; t < NG; ++t) {
            if (t + NG1 < NG) af[t + NG1] = rd(buf, t + NG1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t][u], eb[t * 4 + u], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(0);
        return acc;
    };

    float second = 0.0f, tau = 0.0f;
    int cnt = 0;
    float* candl = p.cand + ((valid ? row : 0) * 2 + h) * AF_CAPL;
    // acc[r] = score of cohort row 32 b' + (r & 3) + 8 (r >> 2) + 4 h against embedding j
    auto process = [&](const f32x16& a, int b) {
        if (b < NP - 1) {               // rows of M: (M e)_i . e_i
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 ev = *reinterpret_cast<const f32x4*>(erow + 32 * b + 8 * g + 4 * h);
#pragma unroll
                for (int u = 0; u < 4; ++u) second = fmaf(a[4 * g + u], ev[u], second);
            }
        } else if (b == NP - 1) {       // row 0 of the last pseudo block is cbar: the mean lives in register 0 of the h = 0 lanes
            const float m = __shfl(a[0], j, 64);
            const float sec = second + __shfl_xor(second, 32, 64);
            tau = m + (p.zrow ? p.zrow[valid ? row : 0] : p.z) * sqrtf(fmaxf(sec - m * m, 0.0f));
        } else {
            const int kb = (b - NP) * 32 + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = kb + (r & 3) + 8 * (r >> 2);
                const float v = a[r];
                if (i < p.K && v > tau) {
                    if (cnt < AF_CAPL && valid) candl[cnt] = v;
                    ++cnt;
                }
            }
        }
    };

    // (co-resident workgroups started half a block apart, by a sleep in every other one, measured +-0)
    issue(0, 0);
    f32x16 accp;
#pragma unroll
    for (int r = 0; r < 16; ++r) accp[r] = 0.0f;
    for (int b = 0; b < nb; ++b) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // block b has landed (and the candidate stores of one block ago, long since)
        __syncthreads();                                       // ... for every wave; nobody still reads the other buffer
        if (b + 1 < nb) issue(b + 1, (b + 1) & 1);
        read_first(b & 1);
        __builtin_amdgcn_sched_barrier(0);
        if (b > 0) process(accp, b - 1);                       // selection of the previous block (the first reads land meanwhile)
        accp = mfma_block(b & 1);
    }
    process(accp, nb - 1);
    if (valid) p.cnt[row * 2 + h] = cnt;
}

// ---- the same kernel on two IEEE-half planes and three fp16 MFMAs per product block ("h3w", round 4, the default) ----------------------
// Same structure as asnorm_fused_kernel (embeddings = B operand in registers, cohort blocks through LDS, lane-local selection, exact moments as
// leading pseudo-cohort blocks); the cohort image (pseudo rows first, then the K cohort rows) is split into two half planes once per call
// (split_planes.hip), and a product block is hi.hi + hi.lo + lo.hi with fp32 accumulation — the machinery of h3w_walk.h, shared with the
// dense score kernel (score_h3w.hip); this kernel keeps its block loop and the selection.  A half plane carries 11 significant bits, so
// hi + lo holds 22 (2^-23 relative) while lo is a normal half, and below |v| = 2^-3 — where the components of unit embeddings live — lo is a
// subnormal half with an ABSOLUTE quantum of 2^-24: a component is represented to 3e-8 absolute, a score of unit vectors to ~4e-8 (measured
// against the float64 oracle: tests).  That is the class of round 3's six-bf16-MFMA form (three exact bf16 parts per value, 1.5e-8 from the
// exact-fp32-MFMA kernel) at half its MFMAs, two thirds of its LDS bytes and 96 instead of 144 operand VGPRs (D = 256 fits as well); the
// 2^-17 of a three-product bf16 form is NOT enough (2e-4 on the normalised scores).  It runs on the 16-wide MFMA: on random
// data the chip holds a higher clock under the 16x16x32 instruction than under 32x32x16 (bare loops: 1.87 against 1.63 PFLOP/s,
// tools/mfma_rate.hip; MI355X_MICROARCH.md, DVFS give-back), and this kernel runs at the pace of its MFMAs.  A wave still owns 32 embeddings
// and walks the cohort in blocks of 32 rows: 2 row groups x 2 embedding groups of 16 per k step of 32.  Accumulator layout: lane (c = lane & 15,
// q = lane >> 4) holds the scores of cohort rows 16 rg + 4 q + e (e = 0..3) against embedding 16 eg + c — so a lane selects for TWO embeddings,
// and an embedding's candidates come from FOUR lanes: four candidate lists of ASNORM_CAND_PER_LANE / 2 per embedding (AsnormFusedParams::nlists).
template <int D>
__global__ __launch_bounds__(256, 2) void asnorm_h3w_kernel(AsnormFusedParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef H3wWalk<D> Walk;
    typedef typename Walk::acc_t acc_t;
    constexpr int NP = D / 32 + 1;                  // pseudo-cohort blocks: rows of M, then cbar
    constexpr int CAPQ = AF_CAPL / 2;               // candidate slots per (embedding, q)

    Walk w(smem, p.N);
    const int c = w.c, q = w.q;
    const int64_t row0 = w.row0;                                               // embedding of group 0 (group 1: + 16)
    const bool (&valid)[2] = w.valid;
    const float (&se)[2] = w.se;
    uint32_t eoff[2];                                                          // < 2^31 elements per launch (host check)
#pragma unroll
    for (int eg = 0; eg < 2; ++eg) eoff[eg] = (uint32_t)((valid[eg] ? row0 + 16 * eg : p.N - 1) * D);

    // B operand: embedding (16 eg + c), scaled by se ("operand scaling", split_planes.hip).  With p.pscale the planes are scaled too (cohort
    // and mean row by sC, moment rows by sC^2): every score of this kernel lives in the scaled domain — the threshold is formed and compared
    // there, the candidates are stored there — and the candidate kernel multiplies a row's mean and deviation back by p.rowscale[row] (exact).
    w.load_operand([&](int eg) { return p.E + eoff[eg]; }, p.pscale);

    const int rows_total = NP * 32 + p.K;
    const int nb = (rows_total + 31) / 32;
    w.stream(p.planes, rows_total);

    float second[2] = {0.0f, 0.0f}, tau[2] = {0.0f, 0.0f};
    // A lane's candidate list.  The four lists of an embedding (one per q) are INTERLEAVED in its 4 * CAPQ-float region: element k of list q at
    // float k * 4 + q — the four lanes fill neighbouring dwords at about the same pace (16-byte groups complete within a block or two instead of
    // a lane's own eight-element sector over ten), and the statistics kernel finds the region dense up to 4 * (shortest list) and can stop its
    // search registers there.  pos = BYTE offset of the next free slot (16 bytes per element), lim = byte offset of the last slot.
    uint32_t coff[2], pos[2], lim[2];
#pragma unroll
    for (int eg = 0; eg < 2; ++eg) {
        coff[eg] = (uint32_t)((valid[eg] ? row0 + 16 * eg : 0) * 4 * CAPQ + q);
        pos[eg] = coff[eg] << 2;
        lim[eg] = (coff[eg] + (uint32_t)(CAPQ - 1) * 4u) << 2;
    }
    auto process = [&](const acc_t& a, int b) {
        if (b < NP - 1) {               // rows of M: (M e)_i . e_i, i = 32 b + 16 rg + 4 q + e
#pragma unroll
            for (int eg = 0; eg < 2; ++eg)
#pragma unroll
                for (int rg = 0; rg < 2; ++rg) {
                    const f32x4 ev = *reinterpret_cast<const f32x4*>(p.E + eoff[eg] + 32 * b + 16 * rg + 4 * q);
#pragma unroll
                    for (int u = 0; u < 4; ++u) second[eg] = fmaf(a[rg][eg][u], ev[u] * se[eg], second[eg]);      // (scaled domain: sC^2 sE^2 e^T M e)
                }
        } else if (b == NP - 1) {       // row 0 of the last pseudo block is cbar: the mean lives in register 0 of row group 0 of the q = 0 lanes
#pragma unroll
            for (int eg = 0; eg < 2; ++eg) {
                const float m = __shfl(a[0][eg][0], c, 64);
                float sec = second[eg];
                sec += __shfl_xor(sec, 16, 64);
                sec += __shfl_xor(sec, 32, 64);
                // (rows past N never hit: no separate validity test in the selection below)
                const float zz = p.zrow ? p.zrow[valid[eg] ? row0 + 16 * eg : 0] : p.z;
                tau[eg] = valid[eg] ? m + zz * sqrtf(fmaxf(sec - m * m, 0.0f)) : __builtin_inff();
            }
        } else {
            // The selection, 32 scores per lane per block.  It issues for the whole wave whenever ONE lane hits (4.7 % of the scores pass:
            // 95 % of the instructions see a hit somewhere), so what counts is its instruction count, not how rarely a lane stores.  Round 4's
            // form — row-bound test, threshold test, list-capacity test as nested ifs, a 64-bit store address — was ~7 vector + ~8 scalar
            // instructions and two branches per score: ~1.7 k issue cycles per block beside 1.15 k of MFMAs.  Now: one compare, a clamped slot
            // (an overflowing list is flagged by its count and never read, so its last slot may be overwritten), a 32-bit offset from the
            // scalar base, one masked store, one add; the row-bound test exists only in the cohort's last block.
            const int kb0 = (b - NP) * 32;
            char* cbase = reinterpret_cast<char*>(p.cand);
            auto select = [&](auto bounded) {                   // bounded: the cohort's last block, whose rows past K repeat row K - 1
#pragma unroll
                for (int eg = 0; eg < 2; ++eg)
#pragma unroll
                    for (int rg = 0; rg < 2; ++rg)
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const float v = a[rg][eg][u];
                            bool hit = v > tau[eg];
                            if (decltype(bounded)::value) hit = hit && (kb0 + 4 * q + 16 * rg + u < p.K);
                            // branch-free: the slot address is formed for every lane, the store runs under the hit mask as EXEC (written
                            // as `if (hit)` the compiler adds an s_cbranch_execz per score and lays the two paths out alternately:
                            // a taken branch on most of the 32 scores of a block)
                            // (the list position is kept as a BYTE offset: clamp, store, advance by one element on a hit — four vector instructions per score)
                            const uint32_t off = min(pos[eg], lim[eg]);
                            const unsigned long long mask = __ballot(hit);
                            unsigned long long saved;
                            asm volatile("s_and_saveexec_b64 %0, %1\n\tglobal_store_dword %2, %3, %4\n\ts_mov_b64 exec, %0"
                                         : "=&s"(saved) : "s"(mask), "v"(off), "v"(v), "s"(cbase) : "memory", "scc");
                            pos[eg] += hit ? 16u : 0u;
                        }
            };
            if (kb0 + 32 <= p.K) select(std::false_type{});     // (wave-uniform)
            else select(std::true_type{});
        }
    };

    w.issue(0, 0);
    acc_t accp;
#pragma unroll
    for (int rg = 0; rg < 2; ++rg)
#pragma unroll
        for (int eg = 0; eg < 2; ++eg) accp[rg][eg] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < nb; ++b) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // block b has landed (and the candidate stores of one block ago, long since)
        __syncthreads();                                       // ... for every wave; nobody still reads the other buffer
        if (b + 1 < nb) w.issue(b + 1, (b + 1) & 1);
        // the selection of the PREVIOUS block goes first: its candidate stores are then a whole MFMA phase old at the next wait
        // (issued after the MFMAs they sat right in front of that wait: 18.8 ms for 1.2 M embeddings)
        if (b > 0) process(accp, b - 1);
        __builtin_amdgcn_sched_barrier(0);
        w.mfma_block(b & 1, accp);
    }
    process(accp, nb - 1);
#pragma unroll
    for (int eg = 0; eg < 2; ++eg)
        if (valid[eg]) {
            p.cnt[(row0 + 16 * eg) * 4 + q] = (int32_t)((pos[eg] - (coff[eg] << 2)) >> 4);      // every hit counted, stored or not
            if (q == 0 && p.rowscale) p.rowscale[row0 + 16 * eg] = w.unscale[eg];
        }
}

// one wave per embedding: exact statistics of the top-`top` of its candidates; rows that cannot be decided are flagged.
// NL candidate lists per embedding (2: one per half-wave lane of the fp32-MFMA kernel; 4: the half-plane kernel), 2 * AF_CAPL slots in all.
template <int NL>
__global__ __launch_bounds__(256) void asnorm_cand_stats_kernel(const float* __restrict__ cand, const int32_t* __restrict__ cnt, int64_t rows,
                                                                int top, float* __restrict__ mu, float* __restrict__ sigma,
                                                                int64_t row_base, int32_t* __restrict__ flagged, int32_t* __restrict__ nflag,
                                                                const float* __restrict__ rowscale, int32_t* __restrict__ finfo) {
    constexpr int CAP = 2 * AF_CAPL / NL;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    // every slot of the row is loaded at once, BEFORE the counts are known — one memory round trip instead of two (this kernel is one wave per
    // embedding and lives on latency); a slot past its list's count becomes key 0 below.  (Never-written slots hold whatever the scratch
    // held: they are masked by the counts.)
    const float* c = cand + row * 2 * AF_CAPL;
    uint32_t ck[2 * AF_CAPL / 64];
    float cv[2 * AF_CAPL / 64];
#pragma unroll
    for (int q = 0; q < 2 * AF_CAPL / 64; ++q) cv[q] = __builtin_nontemporal_load(c + lane + 64 * q);
    int cn[NL], total = 0;
    bool over = false;
#pragma unroll
    for (int l = 0; l < NL; ++l) { cn[l] = cnt[row * NL + l]; total += cn[l]; over |= cn[l] > CAP; }
    if (total < top || over) {
        if (lane == 0) {
            const int slot = atomicAdd(nflag, 1);
            flagged[slot] = (int32_t)(row_base + row);
            if (finfo) finfo[slot] = min(total, (1 << 30) - 1) | (over ? (1 << 30) : 0);       // what the refit pass starts from
        }
        return;
    }
    int nq = 2 * AF_CAPL / 64;
    if (NL == 4) {
        // the 16-wide kernel interleaves its four lists: float p of the region = element p >> 2 of list p & 3 — dense up to 4 * (shortest
        // list), empty past 4 * (longest): the search registers past that are skipped (typically 5 of 8)
        const int cl = (lane & 3) == 0 ? cn[0] : (lane & 3) == 1 ? cn[1] : (lane & 3) == 2 ? cn[2 % NL] : cn[3 % NL];
        int cmax = 0;
#pragma unroll
        for (int k = 0; k < NL; ++k) cmax = max(cmax, cn[k]);
        nq = min(nq, __builtin_amdgcn_readfirstlane((4 * cmax + 63) >> 6));
#pragma unroll
        for (int q = 0; q < 2 * AF_CAPL / 64; ++q) ck[q] = ((lane >> 2) + 16 * q) < cl ? fkey(cv[q]) : 0u;
    } else {
#pragma unroll
        for (int q = 0; q < 2 * AF_CAPL / 64; ++q) {
            const int pos = lane + 64 * q, l = pos / CAP, idx = pos - l * CAP;
            int cl = 0;
#pragma unroll
            for (int k = 0; k < NL; ++k) cl = l == k ? cn[k] : cl;
            ck[q] = idx < cl ? fkey(cv[q]) : 0u;
        }
    }
    float m, sd;
    // (total >= top populated keys was checked above: the search may start below the bits they share.  The register count of the search is a
    //  compile-time constant per case: with a run-time bound inside select_stats the eight ballot chains of a step sit behind eight uniform
    //  branches and no longer interleave — the guarded form measured 25 % SLOWER than searching all eight registers)
    auto run = [&](auto nreg) {
        constexpr int NR = decltype(nreg)::value;
        uint32_t c[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) c[j] = ck[j];
        select_stats<NR>(c, top, m, sd, NR, true);
    };
    if (nq <= 5) run(std::integral_constant<int, 5>{});
    else if (nq == 6) run(std::integral_constant<int, 6>{});
    else run(std::integral_constant<int, 2 * AF_CAPL / 64>{});
    // (candidates of the scaled kernels are stored in the scaled domain: mean and deviation are linear in the scale, a power of two)
    const float rs = rowscale ? rowscale[row] : 1.0f;
    if (lane == 0) { mu[row_base + row] = m * rs; sigma[row_base + row] = sd * rs; }
}

// MB = [M ; cbar ; 0]: M[i][j] = (1/K) sum_k C[k][i] C[k][j] (D x D), cbar[j] = (1/K) sum_k C[k][j].
// Stage 1: grid (D / 32, D / 32 + 1, MOM_SLICES): a 32 x 32 tile of C^T C over one slice of the cohort rows (thread = column j, 4 rows i;
// the extra block row sums the columns themselves); stage 2 adds the slices in a fixed order (no atomics: same bits every run).
constexpr int MOM_SLICES = 16;
__global__ __launch_bounds__(256) void cohort_moments_part_kernel(const float* __restrict__ C, int K, int D, float* __restrict__ part) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int j = blockIdx.x * 32 + tx;
    const int per = (K + MOM_SLICES - 1) / MOM_SLICES;
    const int k0 = blockIdx.z * per, k1 = min(K, k0 + per);
    float* out = part + (int64_t)blockIdx.z * (D + 32) * D;
    if (blockIdx.y == gridDim.y - 1) {          // cbar (row D), zeros below
        float s = 0.0f;
        if (ty == 0) for (int k = k0; k < k1; ++k) s += C[(int64_t)k * D + j];
        for (int r = ty; r < 32; r += 8) out[(int64_t)(D + r) * D + j] = r == 0 ? s : 0.0f;
        return;
    }
    const int i0 = blockIdx.y * 32 + ty * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = k0; k < k1; ++k) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(C + (int64_t)k * D + i0);
        const float b = C[(int64_t)k * D + j];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = fmaf(a[u], b, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) out[(int64_t)(i0 + u) * D + j] = acc[u];
}
__global__ __launch_bounds__(256) void cohort_moments_sum_kernel(const float* __restrict__ part, int n, float inv_k, float* __restrict__ MB) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
#pragma unroll
    for (int z = 0; z < MOM_SLICES; ++z) s += part[(int64_t)z * n + i];
    MB[i] = s * inv_k;
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ E, const int32_t* __restrict__ ids, int n, int D,
                                                          float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * D) return;
    const int r = (int)(i / D), k = (int)(i - (int64_t)r * D);
    out[i] = E[(int64_t)ids[r] * D + k];
}
__global__ __launch_bounds__(256) void scatter_stats_kernel(const float* __restrict__ m, const float* __restrict__ s, const int32_t* __restrict__ ids,
                                                            int n, float* __restrict__ mu, float* __restrict__ sigma) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    mu[ids[i]] = m[i];
    sigma[ids[i]] = s[i];
}

}  // namespace

bool asnorm_fused_supported(int D, int K, int top) {
    return (D == 192 || D == 256) && top >= 1 && top <= 256 && K >= 4 * top && K >= 64;
}

// Upper-tail normal quantile z with P(x > mean + z sd) = frac (Abramowitz-Stegun 26.2.22), frac <= 0.5
float asnorm_tail_z(int K, int top) {
    const float frac = fminf(0.5f, 1.6f * (float)top / (float)K);
    const float tq = sqrtf(-2.0f * logf(fmaxf(frac, 1e-6f)));
    return tq - (2.30753f + 0.27061f * tq) / (1.0f + 0.99229f * tq + 0.04481f * tq * tq);
}

size_t cohort_moments_scratch_bytes(int D) { return (size_t)MOM_SLICES * (D + 32) * D * sizeof(float); }

hipError_t launch_cohort_moments(const float* cohort, int K, int D, float* MB, float* part, hipStream_t stream) {
    if (D % 32 != 0 || K <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cohort_moments_part_kernel, dim3(D / 32, D / 32 + 1, MOM_SLICES), dim3(256), 0, stream, cohort, K, D, part);
    const int n = (D + 32) * D;
    hipLaunchKernelGGL(cohort_moments_sum_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, part, n, 1.0f / (float)K, MB);
    return hipGetLastError();
}

// two half planes and, in the room of a third, the cohort's max-|x| word and its partials
size_t asnorm_planes_bytes(int D, int K) { return (size_t)3 * (D + 32 + K) * D * 2; }

hipError_t launch_asnorm_planes(const float* MB, const float* cohort, int K, int D, void* planes, hipStream_t stream, uint32_t* pscale) {
    if (!MB || !cohort || !planes || K <= 0 || D % 32 != 0) return hipErrorInvalidValue;
    // (with pscale: cohort rows and the mean row are scaled by s, the D moment rows by s^2)
    return launch_split_planes(MB, D + 32, cohort, K, D, planes, pscale, D, stream);
}

hipError_t launch_asnorm_fused(const AsnormFusedParams& p, int D, hipStream_t stream) {
    if (p.N <= 0) return hipSuccess;
    if (!asnorm_fused_supported(D, p.K, 1) || !p.E || !p.cohort || !p.MB || !p.cand || !p.cnt) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(p.E) | reinterpret_cast<uintptr_t>(p.cohort) | reinterpret_cast<uintptr_t>(p.MB)) & 15) return hipErrorInvalidValue;
    if (p.nlists != (p.planes ? 4 : 2)) return hipErrorInvalidValue;      // (four lists: the half-plane kernel; two: the fp32-MFMA kernel)
    const dim3 grid((unsigned)((p.N + 127) / 128));       // (D is 192 or 256: asnorm_fused_supported)
    if (p.planes) {                                      // the split form: three fp16 MFMAs on two half planes
        if ((D != 192 && D != 256) || (reinterpret_cast<uintptr_t>(p.planes) & 15) || p.N > (int64_t)1 << 21) return hipErrorInvalidValue;      // (32-bit lane offsets)
        if (p.N * 2 * ASNORM_CAND_PER_LANE * 4 >= (int64_t)1 << 32) return hipErrorInvalidValue;      // (32-bit byte offsets into the candidate lists)
        if (p.pscale && !p.rowscale) return hipErrorInvalidValue;                                       // (scaled planes: the row factors go with them)
        if (D == 192) return launch_max_lds<AsnormFusedParams, asnorm_h3w_kernel<192>>(grid, h3w_lds_bytes(192), p, stream);
        return launch_max_lds<AsnormFusedParams, asnorm_h3w_kernel<256>>(grid, h3w_lds_bytes(256), p, stream);
    }
    if (D == 192) return launch_max_lds<AsnormFusedParams, asnorm_fused_kernel<192>>(grid, 2 * 32 * 192 * 4, p, stream);
    return launch_max_lds<AsnormFusedParams, asnorm_fused_kernel<256>>(grid, 2 * 32 * 256 * 4, p, stream);
}

hipError_t launch_asnorm_cand_stats(const float* cand, const int32_t* cnt, int64_t rows, int top, float* mu, float* sigma, int64_t row_base,
                                    int32_t* flagged, int32_t* nflag, hipStream_t stream, int nlists, const float* rowscale, int32_t* finfo) {
    if (rows <= 0) return hipSuccess;
    if (nlists == 4)
        hipLaunchKernelGGL(asnorm_cand_stats_kernel<4>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, cand, cnt, rows, top, mu, sigma, row_base,
                           flagged, nflag, rowscale, finfo);
    else if (nlists == 2)
        hipLaunchKernelGGL(asnorm_cand_stats_kernel<2>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, cand, cnt, rows, top, mu, sigma, row_base,
                           flagged, nflag, rowscale, finfo);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- refit state of the embeddings the normal-quantile threshold did not fit (round 6) -------------------------------------------------
// Structure of arrays, stride = the number of rows: [id (int bits) | z | z of the pass before | ln(count) of the pass before | zlo | zhi]
// (zlo: the largest z that passed too many, zhi: the smallest that passed too few; <= -50: none yet).  A row's next z from what its last pass
// counted: ln(count) against z is locally close to linear — slope ~ -(z + 1 / z) for a Gaussian tail, several times steeper when the
// threshold sits on the flank of a narrow mode (clustered speaker centroids) — so the FIRST step assumes a slope of -5 and every later step
// is the secant through the last two measurements, kept inside the bracket once both sides have been seen.
__device__ __forceinline__ void refit_next_z(float& z, float& zp, float& lcp, float& zlo, float& zhi, int32_t inf, float target) {
    const float lnT = __logf(target);
    const float c = (float)(inf & ((1 << 30) - 1));
    const bool many = ((inf >> 30) & 1) || c > target;       // (a flagged row with enough candidates overflowed a list)
    const float lc = __logf(fmaxf(many ? fmaxf(c, 1.25f * target) : c, 0.5f));
    if (many) zlo = zlo > -50.f ? fmaxf(zlo, z) : z; else zhi = zhi > -50.f ? fminf(zhi, z) : z;
    float slope = -5.0f;
    if (zp > -50.f && fabsf(z - zp) > 1e-3f) slope = fminf(-1.0f, fmaxf(-12.0f, (lc - lcp) / (z - zp)));
    float zn = z + fminf(0.6f, fmaxf(-0.6f, (lnT - lc) / slope));
    if (many) zn = fmaxf(zn, z + 0.02f); else zn = fminf(zn, z - 0.02f);
    if (zlo > -50.f && zhi > -50.f) {
        const float w = zhi - zlo;
        zn = fminf(zhi - 0.1f * w, fmaxf(zlo + 0.1f * w, zn));
    }
    zp = z; lcp = lc;
    z = fminf(12.0f, fmaxf(-2.0f, zn));
}
__global__ __launch_bounds__(256) void refit_init_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ info, int n, float z0, float target,
                                                         float* __restrict__ soa) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float z = z0, zp = -100.f, lcp = 0.f, zlo = -100.f, zhi = -100.f;
    refit_next_z(z, zp, lcp, zlo, zhi, info[i], target);
    reinterpret_cast<int32_t*>(soa)[i] = ids[i];
    soa[n + i] = z; soa[2 * (size_t)n + i] = zp; soa[3 * (size_t)n + i] = lcp; soa[4 * (size_t)n + i] = zlo; soa[5 * (size_t)n + i] = zhi;
}
__global__ __launch_bounds__(256) void refit_next_kernel(const float* __restrict__ in, int n_in, const int32_t* __restrict__ pos, const int32_t* __restrict__ info,
                                                         int left, float target, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= left) return;
    const int j = pos[i];
    float z = in[n_in + j], zp = in[2 * (size_t)n_in + j], lcp = in[3 * (size_t)n_in + j], zlo = in[4 * (size_t)n_in + j], zhi = in[5 * (size_t)n_in + j];
    refit_next_z(z, zp, lcp, zlo, zhi, info[i], target);
    reinterpret_cast<int32_t*>(out)[i] = reinterpret_cast<const int32_t*>(in)[j];
    out[left + i] = z; out[2 * (size_t)left + i] = zp; out[3 * (size_t)left + i] = lcp; out[4 * (size_t)left + i] = zlo; out[5 * (size_t)left + i] = zhi;
}
hipError_t launch_asnorm_refit_init(const int32_t* ids, const int32_t* info, int n, float z0, float target, float* soa, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(refit_init_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, ids, info, n, z0, target, soa);
    return hipGetLastError();
}
hipError_t launch_asnorm_refit_next(const float* in, int n_in, const int32_t* pos, const int32_t* info, int left, float target, float* out, hipStream_t stream) {
    if (left <= 0) return hipSuccess;
    hipLaunchKernelGGL(refit_next_kernel, dim3((left + 255) / 256), dim3(256), 0, stream, in, n_in, pos, info, left, target, out);
    return hipGetLastError();
}

hipError_t launch_gather_rows(const float* E, const int32_t* ids, int n, int D, float* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(((int64_t)n * D + 255) / 256)), dim3(256), 0, stream, E, ids, n, D, out);
    return hipGetLastError();
}

hipError_t launch_scatter_stats(const float* m, const float* s, const int32_t* ids, int n, float* mu, float* sigma, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_stats_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, m, s, ids, n, mu, sigma);
    return hipGetLastError();
}

}  // namespace svhip
