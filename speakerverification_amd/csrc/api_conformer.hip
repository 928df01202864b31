// api_conformer.hip — the Conformer forward of libsvhip (reference models/Conformer.py:100-154, models/conformer/conformer/*.py).
//
// From the mel power (B, n_mels, T):
//   front-end   log(x + 1e-6) - mean_t (log_input), InstanceNorm1d(n_mels, affine) -> X_in (B T, n_mels)        prologue
//   subsample   per slice of cf_chunk utterances (the conv1 output is the largest tensor of the net):
//               conv1 + ReLU -> (n, T1, F1, 256)                                                               cf_conv1
//               conv2 + ReLU as a GEMM whose operand rows are gathered as three 768-element runs -> (n T' F2, 256)   generic GEMM, SEG form
//               input_projection: the (n T', F2 256) view of that output, its columns permuted at finalize -> cf_in
//   6 blocks    x += 0.5 FF(x); x += MHSA(x); x += Conv(x); x += 0.5 FF'(x); x = LN(x)                          see below
//   pooling     w = softmax_T(attention.3(BN(relu(attention.0 x)))); [mu | sqrt(clamp(var, 1e-4, 1e4))]; attention_norm; fc
// Every Linear / pointwise conv goes through conv_plan / conv_gemm.  The half-step residuals are the GEMM epilogue's scale (0.5) and
// residual R; the residual stream stays in the handle's storage type.
#include "handle.h"

namespace svhip {

static int cf_ln(svhip_handle* h, const void* x, void* y, const float* g, const float* b, int64_t M, void* y2 = nullptr,
                 const float* g2 = nullptr, const float* b2 = nullptr) {
    return run(h, "cf_ln", 0, [&]() { return launch_cf_ln(x, y, g, b, y2, g2, b2, h->dt, M, h->cur); });
}

static int conformer_forward_part(svhip_handle* h, const float* d_feat, int b0, int B) {
    (void)b0;
    const svhip_config& c = h->cfg;
    const int T = h->T, Tp = h->cf_Tp, F = c.n_mels, T1 = h->cf_T1, F1 = h->cf_F1, F2 = h->cf_F2, e = h->esz, D = CF_D;
    const int M = B * Tp;
    const bool bf = h->bf16;
    hipStream_t st = h->cur;
    int rc;
    if ((rc = run(h, "prologue", 0, [&]() {
             return launch_prologue(d_feat, h->X_in, bf, B, F, T, c.log_input, h->in_w, h->in_b, h->d_pstats, st);
         }))) return rc;
    // Conv2dSubampling + input_projection (convolution.py:152-185, encoder.py:160-163), cf_chunk utterances at a time
    for (int s0 = 0; s0 < B; s0 += h->cf_chunk) {
        const int n = std::min(h->cf_chunk, B - s0);
        if ((rc = run(h, "cf_conv1", 2.0 * 9 * D * n * T1 * F1, [&]() {
                 return launch_cf_conv1(off(h->X_in, (size_t)s0 * T * F, e), h->cf_c1_w, h->cf_c1_b, h->cf_c1, h->dt, n, T, F, st);
             }))) return rc;
        GemmParams p2 = conv_params(h, h->cf_c2, h->cf_c1, D, h->cf_s2, D, n * Tp * F2, Tp * F2);
        p2.act1 = ACT_RELU;
        p2.seg_off = h->cf_seg_off; p2.seg_rows = Tp * F2; p2.seg_len = 3 * D;
        p2.seg_stride = (int64_t)F1 * D; p2.seg_utt = (int64_t)T1 * F1 * D;
        if ((rc = conv_gemm(h, h->cf_c2, p2))) return rc;
        GemmParams pp = conv_params(h, h->cf_proj, h->cf_s2, F2 * D, off(h->cf_in, (size_t)s0 * Tp * D, e), D, n * Tp, Tp);
        if ((rc = conv_gemm(h, h->cf_proj, pp))) return rc;
    }
    // the blocks (encoder.py:32-110).  Buffers: x (block input) -> r -> xo -> r -> ln2 -> xo = LN(.) (+ the next block's FF LayerNorm)
    const void* x = h->cf_in;
    const int nb = (int)h->cf.size();
    if ((rc = cf_ln(h, x, h->cf_ln, h->cf[0].ff_g[0], h->cf[0].ff_b[0], M))) return rc;
    for (int i = 0; i < nb; ++i) {
        const svhip_handle::CfBlock& K = h->cf[i];
        void* xo = i == 0 ? h->cf_b0 : i == nb - 1 ? h->cf_last : h->cf_x[i & 1];
        void* ctx = i == 0 ? h->cf_attn0 : h->cf_ctx;
        // r = x + 0.5 FF(x); cf_ln already holds LN(x)                                                 feed_forward.py:23-57
        GemmParams f1 = conv_params(h, K.ff1[0], h->cf_ln, D, h->cf_hid, 4 * D, M, Tp);
        f1.act1 = ACT_SWISH;
        if ((rc = conv_gemm(h, K.ff1[0], f1))) return rc;
        GemmParams f2 = conv_params(h, K.ff2[0], h->cf_hid, 4 * D, h->cf_r, D, M, Tp);
        f2.scale = h->cf_half; f2.shift = h->d_zeros; f2.R = x; f2.ldr = D;
        if ((rc = conv_gemm(h, K.ff2[0], f2))) return rc;
        // xo = r + out_proj(attention(LN(r)))                                                        attention.py:75-159
        if ((rc = cf_ln(h, h->cf_r, h->cf_ln, K.att_g, K.att_b, M))) return rc;
        if ((rc = conv_gemm(h, K.qkv, conv_params(h, K.qkv, h->cf_ln, D, h->cf_hid, 3 * D, M, Tp)))) return rc;
        if ((rc = run(h, "cf_attn", 4.0 * B * Tp * (double)Tp * 3 * 2 * 64, [&]() {
                 return launch_cf_attn(h->cf_hid, 3 * D, K.P, D, K.u, K.v, ctx, D, h->dt, B, Tp, st);
             }))) return rc;
        GemmParams po = conv_params(h, K.out, ctx, D, xo, D, M, Tp);
        po.R = h->cf_r; po.ldr = D;
        if ((rc = conv_gemm(h, K.out, po))) return rc;
        // r = xo + pw2(swish(BN(dw15(GLU(pw1(LN(xo)))))))                                             convolution.py:108-149
        if ((rc = cf_ln(h, xo, h->cf_ln, K.cv_g, K.cv_b, M))) return rc;
        if ((rc = conv_gemm(h, K.pw1, conv_params(h, K.pw1, h->cf_ln, D, h->cf_hid, 2 * D, M, Tp)))) return rc;
        if ((rc = run(h, "cf_glu_dw", 2.0 * 15 * D * M, [&]() { return launch_cf_glu_dw(h->cf_hid, K.dw_w, K.dw_b, h->cf_ctx, h->dt, B, Tp, st); })))
            return rc;
        GemmParams pw = conv_params(h, K.pw2, h->cf_ctx, D, h->cf_r, D, M, Tp);
        pw.R = xo; pw.ldr = D;
        if ((rc = conv_gemm(h, K.pw2, pw))) return rc;
        // ln2 = r + 0.5 FF'(r); xo = LN(ln2), and the next block's LN(xo) in the same pass
        if ((rc = cf_ln(h, h->cf_r, h->cf_ln, K.ff_g[1], K.ff_b[1], M))) return rc;
        GemmParams g1 = conv_params(h, K.ff1[1], h->cf_ln, D, h->cf_hid, 4 * D, M, Tp);
        g1.act1 = ACT_SWISH;
        if ((rc = conv_gemm(h, K.ff1[1], g1))) return rc;
        GemmParams g2 = conv_params(h, K.ff2[1], h->cf_hid, 4 * D, h->cf_ln2, D, M, Tp);
        g2.scale = h->cf_half; g2.shift = h->d_zeros; g2.R = h->cf_r; g2.ldr = D;
        if ((rc = conv_gemm(h, K.ff2[1], g2))) return rc;
        const svhip_handle::CfBlock* nx = i + 1 < nb ? &h->cf[i + 1] : nullptr;
        if ((rc = cf_ln(h, h->cf_ln2, xo, K.fin_g, K.fin_b, M, nx ? h->cf_ln : nullptr, nx ? nx->ff_g[0] : nullptr, nx ? nx->ff_b[0] : nullptr)))
            return rc;
        x = xo;
    }
    // attentive statistics pooling (Conformer.py:130-142)
    GemmParams pa = conv_params(h, h->cf_att0, x, D, h->cf_hid, 128, M, Tp);
    pa.act1 = ACT_RELU;
    if ((rc = conv_gemm(h, h->cf_att0, pa))) return rc;
    GemmParams pl = conv_params(h, h->cf_att3, h->cf_hid, 128, h->cf_logits, D, M, Tp);
    pl.out_f32 = 1;
    if ((rc = conv_gemm(h, h->cf_att3, pl))) return rc;
    if ((rc = run(h, "cf_asp_pool", 0, [&]() {
             return launch_asp_pool(h->cf_logits, x, bf, D, B, Tp, D, h->cf_pbn_scale, h->cf_pbn_shift, h->cf_pool_raw, h->cf_pool, 1e-4f, 1e4f, st);
         }))) return rc;
    // an utterance with a non-finite input value gets a NaN embedding, as in the reference (the ReLU epilogues would have dropped it)
    if ((rc = run(h, "cf_in_check", 0, [&]() {
             return launch_tn_nonfinite_rows(d_feat, (int64_t)F * T, B, h->cf_pool, 2 * D, 2 * D, st);
         }))) return rc;
    return run(h, "cf_fc", 2.0 * B * h->cf_fc.N * h->cf_fc.K, [&]() {
        return launch_rowvec_linear(h->cf_pool, 2 * D, h->cf_fc.W, h->cf_fc.bias, h->d_emb, c.embed_dim, B, c.embed_dim, 2 * D, ACT_NONE, st);
    });
}

int conformer_forward(svhip_handle* h, const float* d_feat, int B) { return forward_lanes(h, conformer_forward_part, d_feat, B, 1, B); }

}  // namespace svhip

extern "C" int svhip_conformer_attention(const void* qkv, const float* P, const float* u_bias, const float* v_bias, void* ctx, int32_t compute,
                                         int32_t B, int32_t T_sub, void* stream) {
    using namespace svhip;
    if ((compute != SVHIP_F32 && compute != SVHIP_BF16) || T_sub < 1 || T_sub > CF_MAX_T) return SVHIP_ERR_INVALID;
    const hipError_t e = launch_cf_attn(qkv, 3 * CF_D, P, CF_D, u_bias, v_bias, ctx, CF_D, compute == SVHIP_BF16 ? DT_BF16 : DT_F32, B, T_sub,
                                        reinterpret_cast<hipStream_t>(stream));
    return e == hipSuccess ? SVHIP_OK : e == hipErrorInvalidValue ? SVHIP_ERR_INVALID : SVHIP_ERR_HIP;
}
