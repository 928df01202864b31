// score_h3w.hip — dense score matrix on the half-plane machinery (h3w_walk.h; gfx950): out[i][j] = A_i . B_j (svhip_score_matrix, the slab
// path's cohort GEMM).
//
// K = D = 192 / 256 is six / eight k steps: as a tiled GEMM (gemm_pw's split form, 256 x 128 tiles) the kernel spent its time fetching fp32
// operands (43 FLOP per byte) — 152 TFLOP/s, 0.68 ms for 16 384 x 16 384.  Here a wave keeps 32 rows of A in registers as half hi | lo parts
// and streams B (pre-split half planes, blocks of 32 rows through the LDS image of the AS-norm kernel) past them: three fp16 MFMAs per
// product block on v_mfma_f32_16x16x32_f16, scores stored straight from the accumulators (lane = 4 consecutive columns of one row: 16-byte
// stores, a 128-byte line per row per block).  Grid (row panels of 128, column slices): every workgroup walks `per` blocks of B.
#include "common.h"
#include "h3w_walk.h"
#include "kernels.h"

namespace svhip {

namespace {

template <int D>
__global__ __launch_bounds__(256, 2) void score_h3w_kernel(ScoreH3Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef H3wWalk<D> Walk;
    constexpr int BLK = Walk::BLK;
    Walk w(smem, p.Na);
    const int lane = w.lane, wave = w.wave, c = w.c, q = w.q;
    // unscale: per row of A, 1 / (its own scale * the scale of the B planes) ("operand scaling", split_planes.hip)
    w.load_operand([&](int eg) { return p.A + (w.valid[eg] ? w.row0 + 16 * eg : p.Na - 1) * D; }, p.pscale);
    const int nb_all = (p.Nb + 31) / 32;
    const int b_first = blockIdx.y * p.per, b_last = min(nb_all, b_first + p.per);
    if (b_first >= b_last) return;                                                  // workgroup-uniform
    w.stream(p.planes, p.Nb);
    const bool vec_ok = (p.ldo & 3) == 0 && (reinterpret_cast<uintptr_t>(p.out) & 15) == 0;
    // a wave whose 32 rows are all inside A issues exactly four 16-byte store instructions per interior block, AFTER the next block's DMAs:
    // the wait for block b may then leave those four (the newest entries of the in-order counter) in flight instead of draining them
    const bool rows_full = vec_ok && ((int64_t)blockIdx.x * 128 + wave * 32 + 32 <= p.Na);      // wave-uniform
    bool four_stores_behind = false;
    // Round 6: stored straight from the accumulators a wave instruction writes sixteen 64-byte row pieces (2.8 TB/s of
    // output at 16 384^2; plain stores of 256 contiguous bytes per row run at 6 TB/s: MI355X_MICROARCH.md).  Where the LDS has room beside
    // the two operand blocks (D = 192: 48 KiB + 4 x 8 KiB = 80 KiB, still two workgroups per CU) a wave keeps the scores of TWO blocks — 32
    // rows x 64 columns — in a private 8 KiB image (16-byte slot s of row r at s ^ (r & 15): conflict-free both ways) and writes them as
    // four rows x 256 contiguous bytes per instruction.  No barrier: the image is the wave's own, and a wave's LDS operations run in order.
    constexpr bool STAGED = D == 192;
    char* stg = smem + 2 * BLK + wave * 8192;
    const bool stage = STAGED && vec_ok;
    int stores_behind = 0;                      // stores this wave issued behind the next block's DMAs (-1: not known)
    w.issue(b_first, 0);
    for (int b = b_first; b < b_last; ++b) {
        const int buf = (b - b_first) & 1;
        if (stage) {
            if (stores_behind == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (four_stores_behind) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");      // block b has landed; the previous block's stores may still fly
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        four_stores_behind = rows_full && (32 * b + 32 <= p.Nb);
        __syncthreads();
        if (b + 1 < b_last) w.issue(b + 1, buf ^ 1);
        typename Walk::acc_t acc;
        w.mfma_block(buf, acc);
        // acc[rg][eg][e] = A row (16 eg + c of the wave) . B row 32 b + 16 rg + 4 q + e
        if (stage) {
            const int hb = (b - b_first) & 1;           // which half of the image this block fills
#pragma unroll
            for (int eg = 0; eg < 2; ++eg)
#pragma unroll
                for (int rg = 0; rg < 2; ++rg) {
                    const int slot = hb * 8 + rg * 4 + q;
                    *reinterpret_cast<f32x4*>(stg + (16 * eg + c) * 256 + ((slot ^ c) << 4)) = acc[rg][eg] * w.unscale[eg];
                }
            stores_behind = 0;
            if (hb == 1 || b + 1 == b_last) {
                asm volatile("" ::: "memory");
                const int jb = 32 * (b - hb);           // first column of the image
                const int t = lane & 15;
                const int64_t wrow0 = (int64_t)blockIdx.x * 128 + wave * 32;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int R = 4 * k + (lane >> 4);
                    const f32x4 o4 = *reinterpret_cast<const f32x4*>(stg + R * 256 + ((t ^ (R & 15)) << 4));
                    const int j0 = jb + 4 * t;
                    if (wrow0 + R < p.Na && t < 8 * (hb + 1)) {
                        float* orow = p.out + (wrow0 + R) * p.ldo;
                        if (j0 + 4 <= p.Nb) {
                            __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(orow + j0));
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (j0 + e < p.Nb) orow[j0 + e] = o4[e];
                        }
                    }
                }
                // (exactly eight 16-byte store instructions when every row is inside A and both blocks are whole)
                stores_behind = (rows_full && hb == 1 && jb + 64 <= p.Nb) ? 8 : -1;
            }
            continue;
        }
        // straight from the accumulators (round 5's form): D = 256, and any output that takes no 16-byte stores
#pragma unroll
        for (int eg = 0; eg < 2; ++eg) {
            if (!w.valid[eg]) continue;
            float* orow = p.out + (w.row0 + 16 * eg) * p.ldo;
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) {
                const int j0 = 32 * b + 16 * rg + 4 * q;
                const f32x4 o4 = acc[rg][eg] * w.unscale[eg];
                if (vec_ok && j0 + 4 <= p.Nb) {
                    __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(orow + j0));      // (written once, read by a later kernel at best)
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (j0 + e < p.Nb) orow[j0 + e] = o4[e];
                }
            }
        }
    }
}

}  // namespace

bool score_h3w_supported(int D, int64_t Na, int64_t Nb) { return (D == 192 || D == 256) && Na > 0 && Nb > 0 && Nb < ((int64_t)1 << 30) && Na < ((int64_t)1 << 31); }
size_t score_h3w_planes_bytes(int D, int64_t Nb) { return (size_t)2 * Nb * D * 2 + 2048; }      // two half planes + the scale word of B and its 256 partials behind them

// out (Na, ldo) = A (Na, D) . B (Nb, D)^T; `planes` = score_h3w_planes_bytes of scratch (filled here with the half parts of B)
hipError_t launch_score_h3w(const float* A, int64_t Na, const float* B, int64_t Nb, int D, float* out, int64_t ldo, void* planes, int num_cu,
                            hipStream_t stream) {
    if (!score_h3w_supported(D, Na, Nb) || !A || !B || !out || !planes || ldo < Nb) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(planes)) & 15) return hipErrorInvalidValue;
    uint32_t* pscale = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(planes) + (size_t)2 * Nb * D * 2);      // (16-byte aligned: Nb * D * 4 bytes in)
    if (hipError_t e = launch_split_planes(B, 0, B, (int)Nb, D, planes, pscale, 0, stream)) return e;
    ScoreH3Params p;
    p.A = A; p.Na = Na; p.planes = planes; p.Nb = (int)Nb; p.out = out; p.ldo = ldo; p.pscale = pscale;
    const int panels = (int)((Na + 127) / 128), nb_all = (int)((Nb + 31) / 32);
    // column slices: enough workgroups for ~4 per CU, at least 8 blocks per slice
    int slices = (4 * (num_cu > 0 ? num_cu : 256) + panels - 1) / panels;
    if (slices > (nb_all + 7) / 8) slices = (nb_all + 7) / 8;
    if (slices < 1) slices = 1;
    if (slices > 65535) slices = 65535;
    p.per = (nb_all + slices - 1) / slices;
    slices = (nb_all + p.per - 1) / p.per;
    const dim3 grid((unsigned)panels, (unsigned)slices);
    // LDS: the operand image + at D = 192 the waves' store images (score_h3w_kernel)
    if (D == 192) return launch_max_lds<ScoreH3Params, score_h3w_kernel<192>>(grid, h3w_lds_bytes(192) + 4 * 8192, p, stream);
    return launch_max_lds<ScoreH3Params, score_h3w_kernel<256>>(grid, h3w_lds_bytes(256), p, stream);
}

}  // namespace svhip
