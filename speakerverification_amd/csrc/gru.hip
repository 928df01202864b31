// gru.hip — the recurrence of RawNet2's GRU aggregation (aggregate='gru', RawNet2_custom.py:196-207; torch.nn.GRU, gate order r, z, n).
//
// The input projection x_t W_ih^T + b_ih (+ b_hr, b_hz) of every frame is ONE conv GEMM ahead of this (api_rawnet2.hip, "rn_gru_proj").
// What stays is a dependent chain of T small GEMMs h W_hh^T (M = B, K = 1024, N = 3072): one launch per step ("rn_gru_step") fuses the
// GEMM, the gate epilogue and the state update.  No grid-wide barrier: a grid that is not fully resident would deadlock on one.
//
//   r = sigmoid(gi_r + W_hr h),  z = sigmoid(gi_z + W_hz h),  n = tanh(gi_n + r (W_hn h + b_hn)),  h' = (1 - z) n + z h
//
// W_hh is packed at load time (api_rawnet2.hip) with the gates interleaved per tile of 16 hidden units: row ut * 48 + g * 16 + j holds
// W_hh row g * 1024 + ut * 16 + j.  A workgroup owns one tile of 16 units and 32 batch rows and keeps r, z and n of the same units in its
// accumulators, so the epilogue needs nothing from another workgroup.  Its four waves split K (256 each): a wave's chain of dependent
// L2 loads is a quarter as long, and eight waves per CU hide their latency (one wave over the whole K: 26.6 us per step at B = 256, f16);
// waves 1 - 3 hand their partial sums to wave 0 through LDS, which adds them in a fixed order.
//   MFMA operands: A = the packed W rows (16 rows of one gate), B = h^T (16 batch rows); D[unit][batch]: lane l holds units 4 (l / 16) + v of
//   batch row l % 16 — four consecutive units of one row, so the gate inputs, h and h' move as 16-byte vectors.  Within a K block a lane
//   carries a contiguous run of k (8 on the 16-bit forms, 4 on fp32) for both operands: any k order gives the same sum set, and a lane's
//   loads are single 16-byte vectors.
//   16-bit handles: W in the handle's type, h converted to it on the way into the MFMA (v_mfma_f32_16x16x32_{f16,bf16}); fp32 accumulate,
//   fp32 gate math.  fp32-grade handles (f32, f32x3): W and h in fp32 on v_mfma_f32_16x16x4f32.
// h lives in fp32 and ping-pongs between two buffers; h_in == nullptr is the step from h0 = 0 (no GEMM).
#include "common.h"
#include "kernels.h"

namespace svhip {

namespace {

constexpr int GRU_H = RN_GRU_HIDDEN;         // 1024
constexpr int GRU_UNITS = 16;                // hidden units per wave tile
constexpr int GRU_ROWS = 32;                 // batch rows per workgroup (two MFMA column groups of 16)
constexpr int GRU_KSPLIT = 4;                // waves per workgroup, each over GRU_H / GRU_KSPLIT of K

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

template <typename WT>
struct GruMma;

template <>
struct GruMma<float> {
    static constexpr int KB = 16;            // k per block: 4 per lane group
    // acc[g][rg] += W rows (gate g) . h rows (group rg) over k in [k0, k0 + 16)
    static __device__ __forceinline__ void block(const float* __restrict__ w, const float* const (&hr)[2], int k, f32x4 (&acc)[3][2]) {
        f32x4 wv[3], hv[2];
#pragma unroll
        for (int g = 0; g < 3; ++g) wv[g] = *reinterpret_cast<const f32x4*>(w + (size_t)g * GRU_UNITS * GRU_H + k);
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) hv[rg] = *reinterpret_cast<const f32x4*>(hr[rg] + k);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int rg = 0; rg < 2; ++rg) acc[g][rg] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[g][j], hv[rg][j], acc[g][rg], 0, 0, 0);
    }
};

template <typename H>
struct GruMma16 {
    static constexpr int KB = 32;            // k per block: 8 per lane group
    static __device__ __forceinline__ void block(const H* __restrict__ w, const float* const (&hr)[2], int k, f32x4 (&acc)[3][2]) {
        bf16x8 wv[3], hv[2];
#pragma unroll
        for (int g = 0; g < 3; ++g) wv[g] = *reinterpret_cast<const bf16x8*>(w + (size_t)g * GRU_UNITS * GRU_H + k);
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(hr[rg] + k), b = *reinterpret_cast<const f32x4*>(hr[rg] + k + 4);
            const u32x4 p = {Half16<H>::pack2(a[0], a[1]), Half16<H>::pack2(a[2], a[3]), Half16<H>::pack2(b[0], b[1]), Half16<H>::pack2(b[2], b[3])};
            hv[rg] = __builtin_bit_cast(bf16x8, p);
        }
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) acc[g][rg] = Half16<H>::mfma16(wv[g], hv[rg], acc[g][rg]);
    }
};
template <> struct GruMma<bf16_t> : GruMma16<bf16_t> {};
template <> struct GruMma<f16_t> : GruMma16<f16_t> {};

// grid (1024 / 16 unit tiles, ceil(B / 32)), GRU_KSPLIT waves per workgroup.  gi: (B, T, 3072) fp32 gate inputs of the slice, row b * T + t;
// h_in / h_out: (B, 1024) fp32 (h_in may be null: h = 0); b_hn: (1024) fp32.
template <typename WT>
__global__ __launch_bounds__(GRU_KSPLIT * WAVE) void rn_gru_step_kernel(const WT* __restrict__ Wp, const float* __restrict__ gi, const float* __restrict__ b_hn,
                                                         const float* __restrict__ h_in, float* __restrict__ h_out, int B, int T, int t) {
    using Mma = GruMma<WT>;
    __shared__ f32x4 red[GRU_KSPLIT - 1][6][WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE, c = lane & 15, q = lane >> 4;
    const int ut = blockIdx.x, row0 = blockIdx.y * GRU_ROWS;
    f32x4 acc[3][2];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) acc[g][rg] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (h_in) {                                   // (uniform over the grid)
        // lane: A row c of each gate, B column c of each row group; its k run starts at KB / 4 * q within a block.  Rows past B read row
        // B - 1 (in bounds); their results are never stored.
        constexpr int KW = GRU_H / GRU_KSPLIT;
        const int kofs = wv * KW + Mma::KB / 4 * q;
        const WT* w = Wp + ((size_t)ut * 3 * GRU_UNITS + c) * GRU_H + kofs;
        const float* hr[2];
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) hr[rg] = h_in + (size_t)min(row0 + 16 * rg + c, B - 1) * GRU_H + kofs;
#pragma unroll
        for (int k = 0; k < KW; k += Mma::KB) Mma::block(w, hr, k, acc);
        if (wv > 0) {
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int rg = 0; rg < 2; ++rg) red[wv - 1][g * 2 + rg][lane] = acc[g][rg];
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll
            for (int s = 0; s < GRU_KSPLIT - 1; ++s)
#pragma unroll
                for (int g = 0; g < 3; ++g)
#pragma unroll
                    for (int rg = 0; rg < 2; ++rg) acc[g][rg] += red[s][g * 2 + rg][lane];
        }
    }
    if (wv != 0) return;
    const int u = ut * GRU_UNITS + 4 * q;
    const f32x4 bn = *reinterpret_cast<const f32x4*>(b_hn + u);
#pragma unroll
    for (int rg = 0; rg < 2; ++rg) {
        const int b = row0 + 16 * rg + c;
        if (b >= B) continue;
        const float* x = gi + ((size_t)b * T + t) * (3 * GRU_H) + u;
        const f32x4 xr = *reinterpret_cast<const f32x4*>(x), xz = *reinterpret_cast<const f32x4*>(x + GRU_H),
                    xn = *reinterpret_cast<const f32x4*>(x + 2 * GRU_H);
        const f32x4 hp = h_in ? *reinterpret_cast<const f32x4*>(h_in + (size_t)b * GRU_H + u) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        f32x4 hn;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float r = sigmoid_f(xr[v] + acc[0][rg][v]);
            const float z = sigmoid_f(xz[v] + acc[1][rg][v]);
            const float n = tanhf(xn[v] + r * (acc[2][rg][v] + bn[v]));
            hn[v] = (1.0f - z) * n + z * hp[v];
        }
        *reinterpret_cast<f32x4*>(h_out + (size_t)b * GRU_H + u) = hn;
    }
}

}  // namespace

hipError_t launch_rn_gru_step(const void* Wp, int dt, const float* gi, const float* b_hn, const float* h_in, float* h_out, int B, int T, int t,
                              hipStream_t stream) {
    if (B <= 0 || T <= 0 || t < 0 || t >= T || !Wp || !gi || !b_hn || !h_out || h_in == h_out) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(Wp) | reinterpret_cast<uintptr_t>(gi) | reinterpret_cast<uintptr_t>(b_hn) | reinterpret_cast<uintptr_t>(h_in) |
         reinterpret_cast<uintptr_t>(h_out)) & 15)
        return hipErrorInvalidValue;
    const dim3 grid(GRU_H / GRU_UNITS, (B + GRU_ROWS - 1) / GRU_ROWS), block(GRU_KSPLIT * WAVE);
    if (dt == DT_F16)
        hipLaunchKernelGGL(rn_gru_step_kernel<f16_t>, grid, block, 0, stream, static_cast<const f16_t*>(Wp), gi, b_hn, h_in, h_out, B, T, t);
    else if (dt == DT_BF16)
        hipLaunchKernelGGL(rn_gru_step_kernel<bf16_t>, grid, block, 0, stream, static_cast<const bf16_t*>(Wp), gi, b_hn, h_in, h_out, B, T, t);
    else
        hipLaunchKernelGGL(rn_gru_step_kernel<float>, grid, block, 0, stream, static_cast<const float*>(Wp), gi, b_hn, h_in, h_out, B, T, t);
    return hipGetLastError();
}

}  // namespace svhip
