// api_gemm.hip — the GEMM of one conv layer: its parameters and the kernel conv_gemm routes them to.
#include "handle.h"

namespace svhip {

// zero page of a conv-gather GEMM whose A operand starts at `A`: the zero tail of the zero-tailed activation buffer that holds A (behind
// the operand, within 4 GiB: what gemm_pw3's 16-bit conv-gather form needs), else the handle's stand-alone zero page
static const void* zero_page_for(const svhip_handle* h, const void* A) {
    const char* a = static_cast<const char*>(A);
    for (const TailedBuf& b : h->tailed)
        if (a >= b.base && a < b.base + b.bytes) return b.base + b.bytes;
    return h->d_zero;
}

// The parameters of a GEMM over conv layer L: A (M, lda) in, Y (M, ldy) out, T frames per utterance; the layer's operand set; the
// handle-wide fields (CU count, the persistent-GEMM options pw3_cus / pw3_tail_off, the constant vectors, the 16-bit type, the
// developer switches cv_off / n128_off).  The caller adds what belongs to its launch: epilogue, padding, residual, column sums, the
// zero page, a split form of the weights.
GemmParams conv_params(const svhip_handle* h, const ConvLayer& L, const void* A, int lda, void* Y, int ldy, int M, int T) {
    GemmParams p;
    p.A = A; p.lda = lda; p.Y = Y; p.ldy = ldy;
    p.W = L.W; p.Wrows = L.Np; p.bias = L.bias; p.scale = L.scale; p.shift = L.shift;
    p.M = M; p.N = L.N; p.K = L.K; p.Kp = L.Kp; p.T = T; p.taps = L.taps; p.dil = L.dil; p.cin = L.cin;
    p.num_cu = h->num_cu; p.pw3_cus = h->opt.pw3_cus; p.tail_split = h->opt.pw3_tail_off ? 0 : 1;
    p.zeros = h->d_zeros; p.ones = h->d_ones; p.f16 = h->f16 ? 1 : 0;
    p.cv_off = h->opt.cv_off; p.n128_off = h->opt.n128_off;
    return p;
}

// ---- the kernel of a conv GEMM ----------------------------------------------------------------------
// p: conv_params of L and the fields of this launch.  A_s32 / lda_s32: the A operand in the S32 split layout, when its producer wrote it
// (F32X3 handles; p.A may then be null).
GemmPlan conv_plan(const svhip_handle* h, const ConvLayer& L, GemmParams p, const void* A_s32, int lda_s32) {
    GemmPlan g;
    p.zero_page = zero_page_for(h, p.A);
    const int M = p.M;
    const bool bf = h->bf16;
    g.flops = (double)M * (L.flops_per_row + 2.0 * L.N * p.K3);      // (K3: the pointwise segment appended to a conv-gather GEMM)
    if (h->x3 && L.Ws32 && h->s32_buf && !p.A2 && !p.bias_utt && !p.out_f32 && !p.R) {
        // the GELU layers of an F32X3 handle on the persistent 256 x 256 kernel: A is split into the S32 layout by one elementwise
        // pass, W was split at load time
        GemmParams q = p;
        q.A = A_s32 ? A_s32 : h->s32_buf; q.lda = A_s32 ? lda_s32 : L.K; q.W = L.Ws32; q.x3 = 2;
        if (!gemm_pw3x3_supported(q)) q.side_a = q.side_b = nullptr, q.side_c = 0;
        // (utterances shorter than a tile: no column sums from this kernel — the caller then takes the squeeze / statistics kernels)
        if (!gemm_pw3x3_supported(q) && q.colsum) q.colsum = nullptr;
        if (gemm_pw3x3_supported(q)) {
            g.q = q; g.x3 = true; g.side = q.side_c != 0; g.colsum_groups = q.colsum ? 2 : 0;
            snprintf(g.label, sizeof(g.label), "gemm_pw3x3");
            return g;
        }
    }
    if (h->x3) {              // gemm_pw takes the pre-split weights, the generic kernel (A2 / ragged shapes) the fp32 ones
        p.x3 = 1;
        if (gemm_pw_supported(p, false) && L.Wsplit) p.W = L.Wsplit;
    }
    if (p.colsum) {                       // only the pw2 / pw3 epilogues produce the partials; otherwise the caller falls back
        if (gemm_pw2_supported(p, bf) && p.taps == 1) g.colsum_groups = gemm_colsum_groups(p, bf);
        else p.colsum = nullptr;
    }
    g.q = p;
    const GemmRoute route = g.route = gemm_route(p, bf);
    const char* klabel = route == ROUTE_PW3 ? "gemm_pw3" : route == ROUTE_PW3CV ? "gemm_pw3cv16" : route == ROUTE_N128 ? "gemm_n128" : route == ROUTE_PW2 ? (L.taps > 1 ? "gemm_pw2_conv" : "gemm_pw2")
                         : L.taps > 1 ? (p.A2 ? "gemm_conv_add" : "gemm_conv") : (route == ROUTE_GENERIC ? "gemm_generic" : "gemm_pw");
    if (!h->opt.layer_labels) snprintf(g.label, sizeof(g.label), "%s", klabel);
    else if (!p.K3) snprintf(g.label, sizeof(g.label), "%s M%d N%d K%d", klabel, M, L.N, L.K);      // developer hook (SVHIP_LAYER_LABELS):
    else snprintf(g.label, sizeof(g.label), "%s M%d N%d K%d+%d", klabel, M, L.N, L.K, p.K3);      // one profile row per GEMM shape
    return g;
}

int conv_gemm(svhip_handle* h, const ConvLayer& L, const GemmParams& p, const void* A_s32, int lda_s32, GemmPlan* plan) {
    const GemmPlan g = conv_plan(h, L, p, A_s32, lda_s32);
    if (plan) *plan = g;
    hipStream_t st = h->cur;
    if (g.x3) {
        int rc = A_s32 ? SVHIP_OK      // (the producer already wrote the split form: se_apply)
                       : run(h, "split_s32", 0, [&]() { return launch_split_s32(reinterpret_cast<const float*>(p.A), p.lda, h->s32_buf, p.M, L.K, st); });
        return rc ? rc : run(h, g.label, g.flops, [&]() { return launch_gemm_pw3x3(g.q, st); });
    }
    if (!p.A)
        SV_FAIL(h, SVHIP_ERR_STATE, "GEMM M%d N%d K%d: the operand exists only in the split layout and the kernel that reads it does not take this shape",
                p.M, L.N, L.K);
    return run(h, g.label, g.flops, [&]() { return launch_gemm(g.q, h->bf16, st); });
}

}  // namespace svhip
