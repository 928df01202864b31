// fusion_head.hip — the attention head of Raw_ECAPA_hype (models/Raw_ECAPA_hype.py:65-85, eval mode) as ONE kernel, fp32 throughout.
//
//   x  = lrelu_0.3(bn_before_agg([e1 | e2]))                        704 channels
//   h  = attention.2(silu(attention.0 x + b))                       128
//   w  = softmax over the 704 channels of (attention.3 h + b)
//   m  = x w ;  s = sqrt(max(x^2 w - m^2, 1e-9))                    per channel: the reference's time axis has length 1
//   out = fc(bn_final([m | s]))                                     nOut
//
// A workgroup of 512 threads owns a tile of UT = 4 utterances and 128 of the output columns (grid: tiles x column blocks).  The blocks of
// a tile each compute the head up to bn_final again, a fifth of the work, so that a batch of 256 is 256 workgroups, one per compute
// unit, and a workgroup streams 1.4 MB of weights instead of 3.6 MB.  x, h, the logits / w and bn_final([m | s]) live in LDS as one
// float4 per channel (the tile's four utterances side by side), so a weight that a thread has loaded is used four times against one
// 16-byte LDS broadcast; nothing but the inputs, the weights and `out` touches HBM.  The three weight matrices are stored K-major (the
// output index contiguous: W0t [704][128], W3t [128][704], Wft [1408][nOutP]), so the lanes of a wave read consecutive addresses.  The
// two long sums are cut into K slices that thread groups own (attention.0: 8 slices of 88 channels; fc: 16 slices of 88 rows) and the
// slices are added in slice order (fc: the two slices of a wave first, then the waves in order).
// BATCH INVARIANCE: every sum of an utterance — the slice sums, the slice order, the softmax's per-lane partial sums and its xor
// butterfly — has an order fixed by the channel index alone; B decides only how many workgroups there are and which rows of a tile
// are live, and the column blocks do not share a sum.  So a row's output is bit for bit the same whatever B is and wherever the row
// sits.  No atomics touch the values.
#include "kernels.h"

namespace svhip {

namespace {

constexpr int HC = HYPE_HEAD_C, HA = HYPE_HEAD_A, UT = HYPE_HEAD_UT;
constexpr int NT = 512;                    // threads of a workgroup
constexpr int S0 = 8, K0 = HC / S0;        // attention.0: K slices, channels per slice (64 threads x 2 outputs each)
constexpr int CF = HYPE_HEAD_COLS;         // fc: output columns of a workgroup
constexpr int SF = 16, KF = 2 * HC / SF;   // fc: K slices, rows per slice (32 threads x 4 outputs each)
static_assert(UT == 4, "the LDS rows are one float4 per channel: the tile's four utterances");
static_assert(HC % S0 == 0 && (2 * HC) % SF == 0 && HA == 2 * (NT / S0) && HC % 2 == 0 && HC / 2 <= NT && CF == 4 * (NT / SF) &&
              (NT / 64) * UT * 32 <= 2 * HC, "thread maps");

__device__ __forceinline__ float& at(float4& v, int u) { return reinterpret_cast<float*>(&v)[u]; }
__device__ __forceinline__ float4 fma4(float w, const float4& x, const float4& a) {
    return make_float4(fmaf(w, x.x, a.x), fmaf(w, x.y, a.y), fmaf(w, x.z, a.z), fmaf(w, x.w, a.w));
}
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(NT) void hype_head_kernel(HypeHeadParams p) {
    __shared__ float4 xw[2 * HC];          // x | the logits, then w; at the end the fc's sums per wave, [8][UT][32]
    float4 *xs = xw, *ws = xw + HC;
    __shared__ float4 ps[2 * HC];          // bn_final([m | s]); before that: the slice sums of attention.0, [S0][HA]
    __shared__ float4 hs[HA];
    const int tid = threadIdx.x, u0 = blockIdx.x * UT;
    const int live = min(UT, p.B - u0);    // rows of this tile that exist (the others compute on zeros and are never stored)

    // x = lrelu(bn_before_agg([e1 | e2]))
    for (int c = tid; c < HC; c += NT) {
        const float sc = p.s0[c], sh = p.t0[c];
        float4 v;
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            float e = 0.0f;
            if (u < live) e = c < p.d1 ? p.e1[(size_t)(u0 + u) * p.d1 + c] : p.e2[(size_t)(u0 + u) * p.d2 + (c - p.d1)];
            const float y = fmaf(sc, e, sh);
            at(v, u) = y > 0.0f ? y : 0.3f * y;
        }
        xs[c] = v;
    }
    __syncthreads();

    // attention.0: slice sl of K0 channels, outputs a, a + 1
    {
        const int sl = tid >> 6, a = (tid & 63) * 2;
        float4 acc0 = make_float4(0, 0, 0, 0), acc1 = acc0;
        const float* w = p.W0t + (size_t)sl * K0 * HA + a;
#pragma unroll 8
        for (int i = 0; i < K0; ++i) {
            const float2 wv = *reinterpret_cast<const float2*>(w + (size_t)i * HA);
            const float4 x = xs[sl * K0 + i];
            acc0 = fma4(wv.x, x, acc0);
            acc1 = fma4(wv.y, x, acc1);
        }
        ps[sl * HA + a] = acc0;
        ps[sl * HA + a + 1] = acc1;
    }
    __syncthreads();
    if (tid < HA) {                        // the slices in order, bias, SiLU, attention.2
        float4 acc = ps[tid];
        for (int sl = 1; sl < S0; ++sl) acc = add4(acc, ps[sl * HA + tid]);
        const float b = p.b0[tid], sc = p.s2[tid], sh = p.t2[tid];
        float4 v;
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const float y = at(acc, u) + b;
            at(v, u) = fmaf(sc, y / (1.0f + expf(-y)), sh);
        }
        hs[tid] = v;
    }
    __syncthreads();

    // attention.3: channels c, c + 1
    if (tid < HC / 2) {
        const int c = tid * 2;
        float4 acc0 = make_float4(0, 0, 0, 0), acc1 = acc0;
        const float* w = p.W3t + c;
#pragma unroll 8
        for (int a = 0; a < HA; ++a) {
            const float2 wv = *reinterpret_cast<const float2*>(w + (size_t)a * HC);
            const float4 hv = hs[a];
            acc0 = fma4(wv.x, hv, acc0);
            acc1 = fma4(wv.y, hv, acc1);
        }
        const float b0 = p.b3[c], b1 = p.b3[c + 1];
        ws[c] = make_float4(acc0.x + b0, acc0.y + b0, acc0.z + b0, acc0.w + b0);
        ws[c + 1] = make_float4(acc1.x + b1, acc1.y + b1, acc1.z + b1, acc1.w + b1);
    }
    __syncthreads();

    // softmax over the channels: wave u owns utterance u (the logits came through LDS from the threads that own channels); lane l
    // holds channels l, l + 64, ..: its partial max / sum in that order, then a butterfly over the 64 lanes
    if (tid < UT * 64) {
        const int u = tid >> 6, lane = tid & 63;
        float mx = -INFINITY;
        for (int c = lane; c < HC; c += 64) mx = fmaxf(mx, at(ws[c], u));
        mx = wave_max(mx);
        float sum = 0.0f;
        for (int c = lane; c < HC; c += 64) {
            const float e = expf(at(ws[c], u) - mx);
            at(ws[c], u) = e;
            sum += e;
        }
        sum = wave_sum(sum);
        for (int c = lane; c < HC; c += 64) at(ws[c], u) = at(ws[c], u) / sum;
    }
    __syncthreads();

    // m = x w, s = sqrt(max(x^2 w - m^2, 1e-9)) as the reference writes them (three roundings, no fused multiply-add), then bn_final
    for (int c = tid; c < HC; c += NT) {
        float4 x = xs[c], w = ws[c];
        const float sm = p.sF[c], tm = p.tF[c], ss = p.sF[HC + c], ts = p.tF[HC + c];
        float4 vm, vs;
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const float xv = at(x, u), wv = at(w, u);
            const float m = __fmul_rn(xv, wv);
            const float var = __fsub_rn(__fmul_rn(__fmul_rn(xv, xv), wv), __fmul_rn(m, m));
            at(vm, u) = fmaf(sm, m, tm);
            at(vs, u) = fmaf(ss, sqrtf(fmaxf(var, 1e-9f)), ts);
        }
        ps[c] = vm;
        ps[HC + c] = vs;
    }
    __syncthreads();

    // fc, this workgroup's CF columns: slice sl of KF rows, outputs 4 g .. 4 g + 3.  The two slices of a wave add up by a shuffle, the
    // eight waves' sums go through LDS (over x and w, which are spent) and are added in wave order
    const int sl = tid >> 5, gl = tid & 31, g = blockIdx.y * (CF / 4) + gl;
    {
        float4 acc[UT];
#pragma unroll
        for (int u = 0; u < UT; ++u) acc[u] = make_float4(0, 0, 0, 0);
        if (4 * g < p.nOutP) {
            const float* w = p.Wft + (size_t)sl * KF * p.nOutP + 4 * g;
#pragma unroll 8
            for (int i = 0; i < KF; ++i) {
                const float4 wv = *reinterpret_cast<const float4*>(w + (size_t)i * p.nOutP);
                const float4 pv = ps[sl * KF + i];
                acc[0] = fma4(pv.x, wv, acc[0]);
                acc[1] = fma4(pv.y, wv, acc[1]);
                acc[2] = fma4(pv.z, wv, acc[2]);
                acc[3] = fma4(pv.w, wv, acc[3]);
            }
        }
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            float4 o;                           // the other slice of this wave: even + odd, the same sum on both sides
            o.x = __shfl_xor(acc[u].x, 32, 64); o.y = __shfl_xor(acc[u].y, 32, 64);
            o.z = __shfl_xor(acc[u].z, 32, 64); o.w = __shfl_xor(acc[u].w, 32, 64);
            if ((tid & 32) == 0) xw[((tid >> 6) * UT + u) * 32 + gl] = add4(acc[u], o);
        }
    }
    __syncthreads();
    int bad = 0;
    if (tid < UT * 32) {                        // thread (u, gl): the waves in order, the bias, the store and its check
        const int u = tid >> 5;
        float4 acc = xw[u * 32 + gl];
        for (int wv = 1; wv < NT / 64; ++wv) acc = add4(acc, xw[(wv * UT + u) * 32 + gl]);
        if (u < live)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = 4 * g + j;
                if (n < p.nOut) {
                    const float v = at(acc, j) + p.bf[n];
                    p.out[(size_t)(u0 + u) * p.nOut + n] = v;
                    bad += !(fabsf(v) <= 3.4028234663852886e38f);         // inf or NaN
                }
            }
    }
    // the numeric status of the call, as emb_out_kernel records it
    const uint32_t nbad = (uint32_t)wave_sum(bad);
    if (nbad && (tid & 63) == 0) {
        atomicOr(p.status, 1u);
        atomicAdd(p.status + 1, nbad);
        __threadfence_system();
        *p.host_flag = 1u;
    }
}

}  // namespace

hipError_t launch_hype_head(const HypeHeadParams& p, hipStream_t stream) {
    if (p.B <= 0) return hipSuccess;
    if (p.d1 < 0 || p.d2 < 0 || p.d1 + p.d2 != HC || p.nOut < 1 || p.nOutP % 4 != 0 || p.nOutP < p.nOut) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hype_head_kernel, dim3((p.B + UT - 1) / UT, (p.nOutP + CF - 1) / CF), dim3(NT), 0, stream, p);
    return hipGetLastError();
}

}  // namespace svhip
