// h3w_walk.h — the half-plane machinery of asnorm_h3w_kernel (asnorm_fused.hip) and score_h3w_kernel (score_h3w.hip; gfx950): ONE operand
// preparation, ONE LDS image, ONE MFMA block; a block loop and an epilogue per kernel.
//
// A wave owns 32 rows of the REGISTER operand (embeddings; rows of A) as IEEE-half hi | lo parts, each row scaled by an exact power of two
// (its own max |x| into [64, 128): "operand scaling", split_planes.hip).  The STREAMED operand (pseudo rows + cohort; B) was split into two
// half planes [2][rows_total][D] once per call (split2_planes_kernel) and passes in blocks of 32 rows through a double-buffered LDS image
// the workgroup's four waves share: 16 bytes per lane per LDS-DMA, lane-linear, the XOR swizzle on the source chunk.  A product block is
// hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation: 2 row groups x 2 register-row groups of 16 per k step of 32.
// Accumulator layout: lane (c = lane & 15, q = lane >> 4) holds acc[rg][eg][e] = streamed row 32 b + 16 rg + 4 q + e (e = 0..3) against
// register row 16 eg + c of the wave.
//
// The two block LOOPS stay in their kernels, because they differ on purpose:
//   asnorm_h3w  runs the selection of block b - 1 in front of the MFMAs of block b (its candidate stores are then a whole MFMA phase old
//               at the next wait) and waits vmcnt(0);
//   score_h3w   stores a block's scores at once, behind the next block's DMAs, and lets the wait for that block leave those 4 (or, staged
//               through LDS, 8) store instructions in flight.
// Both issue the same MFMAs on the same operands in the same order.
#pragma once
#include "common.h"
#include "kernels.h"

namespace svhip {

// dynamic LDS of the operand image: two buffers of two planes of 32 rows
constexpr int h3w_lds_bytes(int D) { return 2 * 2 * 32 * D * 2; }

template <int D>
struct H3wWalk {
    static constexpr int CH = D / 8;                       // 16-byte chunks (8 values) per row of a plane
    static constexpr int PL = 32 * D * 2;                  // one plane of a block of 32 rows
    static constexpr int BLK = 2 * PL;
    static constexpr int NDMA = 2 * 32 * CH / 256;         // DMA instructions per thread per block
    static constexpr int NS = D / 32;                      // MFMA k steps (32 wide) per block
    static_assert(D % 64 == 0 && (2 * 32 * CH) % 256 == 0 && CH % 8 == 0, "block image: whole DMA rounds, chunk groups of 8");
    static_assert(2 * BLK == h3w_lds_bytes(D), "the launchers' LDS size is the image's");
    typedef f32x4 acc_t[2][2];
    typedef __attribute__((address_space(3))) void lds_void;
    typedef __attribute__((address_space(1))) const void gbl_void;

    // where a lane stands: register row (16 eg + c) of its wave's 32, k range 8 q .. 8 q + 7 of a step; row0 = its row of group 0 in the launch
    char* smem;
    int tid, lane, wave, c, q;
    int64_t row0;
    bool valid[2];
    // the register operand, the scale of each of its two rows, and 1 / (that scale * the planes' scale): exact powers of two
    bf16x8 bh[2][NS], bl[2][NS];
    float se[2] = {1.0f, 1.0f}, unscale[2] = {1.0f, 1.0f};
    // the streamed operand
    const char* planes;
    int64_t plane_bytes;
    int rows_total;

    __device__ __forceinline__ H3wWalk(char* smem_, int64_t N)
        : smem(smem_), tid(threadIdx.x), lane(tid & 63), wave(__builtin_amdgcn_readfirstlane(tid >> 6)), c(lane & 15), q(lane >> 4),
          row0((int64_t)blockIdx.x * 128 + wave * 32 + c) {
#pragma unroll
        for (int eg = 0; eg < 2; ++eg) valid[eg] = row0 + 16 * eg < N;
    }

    // row(eg): the fp32 row of group eg (a row past N: any row inside the matrix).  k = 32 s + 8 q .. + 7 of the row, as half hi | lo
    // parts of the row SCALED by a power of two; with pscale (the max-|x| word of the streamed operand) the planes are scaled too
    template <class Row>
    __device__ __forceinline__ void load_operand(const Row& row, const uint32_t* pscale) {
#pragma unroll
        for (int eg = 0; eg < 2; ++eg) {
            if (pscale) {
                uint32_t m = 0;
#pragma unroll
                for (int s_ = 0; s_ < NS; ++s_) {
                    const u32x4 w0 = *reinterpret_cast<const u32x4*>(row(eg) + 32 * s_ + 8 * q);
                    const u32x4 w1 = *reinterpret_cast<const u32x4*>(row(eg) + 32 * s_ + 8 * q + 4);
#pragma unroll
                    for (int u = 0; u < 4; ++u) m = max(m, max(finite_abs_bits(w0[u]), finite_abs_bits(w1[u])));
                }
                m = max(m, (uint32_t)__shfl_xor((int)m, 16, 64));
                m = max(m, (uint32_t)__shfl_xor((int)m, 32, 64));
                se[eg] = pow2_scale_of_bits(m);
                unscale[eg] = pow2_inverse(se[eg]) * pow2_inverse(pow2_scale_of_bits(*pscale));
            }
#pragma unroll
            for (int s_ = 0; s_ < NS; ++s_) {
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(row(eg) + 32 * s_ + 8 * q);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(row(eg) + 32 * s_ + 8 * q + 4);
                f16x8 a8, b8;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float v = (u < 4 ? v0[u] : v1[u - 4]) * se[eg];
                    const f16_t a = static_cast<f16_t>(v);
                    a8[u] = a;
                    b8[u] = static_cast<f16_t>(v - static_cast<float>(a));
                }
                bh[eg][s_] = __builtin_bit_cast(bf16x8, a8);
                bl[eg][s_] = __builtin_bit_cast(bf16x8, b8);
            }
        }
    }

    __device__ __forceinline__ void stream(const void* planes_, int rows_total_) {
        planes = reinterpret_cast<const char*>(planes_);
        plane_bytes = (int64_t)rows_total_ * D * 2;
        rows_total = rows_total_;
    }

    // the image is lane-linear (16 bytes per lane): position -> (plane, row, chunk slot); the swizzle goes on the source chunk
    __device__ __forceinline__ void issue(int b, int buf) const {
        const int r0 = b * 32;
        const int limit = rows_total - 1 - r0;          // the last block clamps its rows
#pragma unroll
        for (int qq = 0; qq < NDMA; ++qq) {
            const int pidx = qq * 256 + tid;
            const int pl = pidx / (32 * CH), rem = pidx - pl * (32 * CH);
            const int i = rem / CH, cs = rem - i * CH;
            const int cc = (cs & ~7) | ((cs ^ (i >> 1)) & 7);
            const char* src = planes + pl * plane_bytes + ((int64_t)(r0 + min(i, limit)) * D + cc * 8) * 2;
            __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(smem + buf * BLK + (qq * 256 + wave * 64) * 16), 16, 0, 0);
        }
    }
    // A fragment: streamed row 16 rg + c of the block, k = 32 s + 8 q .. + 7 (chunk 4 s + q of the row).  The 16 lanes of one q read 16 rows at
    // one logical chunk: 8 keys x even / odd row (row stride 384 B = 1.5 bank periods at D = 192): 16 distinct 16-byte slots, no conflict
    __device__ __forceinline__ bf16x8 rd(int buf, int pl, int rg, int s_) const {
        const int i = 16 * rg + c, cs = 4 * s_ + q;
        return *reinterpret_cast<const bf16x8*>(smem + buf * BLK + pl * PL + i * (D * 2) + (((cs & ~7) | ((cs ^ (i >> 1)) & 7)) << 4));
    }
    __device__ __forceinline__ void mfma_block(int buf, acc_t& acc) const {
#pragma unroll
        for (int rg = 0; rg < 2; ++rg)
#pragma unroll
            for (int eg = 0; eg < 2; ++eg) acc[rg][eg] = f32x4{0.f, 0.f, 0.f, 0.f};
        // A fragments are read ONE k step ahead of their MFMAs, fenced (left alone hipcc issues each ds_read right in front of the wait
        // of the MFMAs that use it, and a wave then sits out the LDS latency every k step whenever its SIMD partner is not in its own MFMA
        // phase: matrix pipe busy 0.58 in round 3's form)
        bf16x8 ah[2] = {rd(buf, 0, 0, 0), rd(buf, 0, 1, 0)}, al[2] = {rd(buf, 1, 0, 0), rd(buf, 1, 1, 0)};
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_) {
            bf16x8 nh[2] = {ah[0], ah[1]}, nl[2] = {al[0], al[1]};
            if (s_ + 1 < NS) {
#pragma unroll
                for (int rg = 0; rg < 2; ++rg) { nh[rg] = rd(buf, 0, rg, s_ + 1); nl[rg] = rd(buf, 1, rg, s_ + 1); }
            }
            __builtin_amdgcn_sched_barrier(0);
            // small terms first; the four accumulators of a term are independent
#pragma unroll
            for (int rg = 0; rg < 2; ++rg)
#pragma unroll
                for (int eg = 0; eg < 2; ++eg) acc[rg][eg] = Half16<f16_t>::mfma16(al[rg], bh[eg][s_], acc[rg][eg]);
#pragma unroll
            for (int rg = 0; rg < 2; ++rg)
#pragma unroll
                for (int eg = 0; eg < 2; ++eg) acc[rg][eg] = Half16<f16_t>::mfma16(ah[rg], bl[eg][s_], acc[rg][eg]);
#pragma unroll
            for (int rg = 0; rg < 2; ++rg)
#pragma unroll
                for (int eg = 0; eg < 2; ++eg) acc[rg][eg] = Half16<f16_t>::mfma16(ah[rg], bh[eg][s_], acc[rg][eg]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) { ah[rg] = nh[rg]; al[rg] = nl[rg]; }
        }
        __builtin_amdgcn_s_setprio(0);
    }
};

}  // namespace svhip
