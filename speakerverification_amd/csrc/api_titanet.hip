// api_titanet.hip — the TitaNet forward of libsvhip (reference models/TitaNet.py:184-431, blocks/titanet_blocks.py).
//
// Buffers (alloc_workspace): six (B T, H) activations — PRO (prolog output), X (block output), D0 (block 0's first depthwise output),
// D (depthwise outputs), S (pointwise outputs), K (skip) — then ENC (B T, 1536), ATT (B T, 128) and the fp32 energies (B T, 1536).
// Every BatchNorm is folded into the conv before it (finalize_titanet), so the GEMM epilogues apply at most a ReLU.
//
// One mega-block (TitaNet.py:293-318) on x:
//   skip     K = BN(conv1x1(x))                                  conv_gemm
//   sub 1    d = dw_1(x) + b                                     tn_dw (block 0; later blocks get it from the previous tn_mega_tail)
//            S = relu(BN(pw_1 d))                                conv_gemm
//   sub 2, 3 D = dw_j(S) + b, S = relu(BN(pw_j D))               tn_dw, conv_gemm (the third also leaves the SE squeeze as column sums
//                                                              when its kernel writes them; otherwise colmean)
//   SE       g = sigmoid(W2 relu(W1 mean_t S))                   se_mlp (zero biases)
//   tail     X = relu(K + g S) and D = dw_1'(X) + b' of the next block in the same pass      tn_mega_tail
#include "handle.h"

namespace svhip {

static int titanet_forward_part(svhip_handle* h, const float* d_feat, int b0, int B) {
    (void)b0;
    const svhip_config& c = h->cfg;
    const int T = h->T, M = B * T, H = c.channels, E = 1536, k = h->tn_k, dt = h->dt;
    const bool bf = h->bf16;
    hipStream_t st = h->cur;
    void *PRO = h->tn_buf[0], *X = h->tn_buf[1], *D0 = h->tn_buf[2], *D = h->tn_buf[3], *S = h->tn_buf[4], *K = h->tn_buf[5];
    float* cs = bf ? h->d_colsum : nullptr;
    int rc;
    // the mel power (B, n_mels, T) as it is (no log, no normalisation) -> frame-major (B T, n_mels) in the compute type
    if ((rc = run(h, "prologue", 0, [&]() {
             return launch_prologue(d_feat, h->X_in, bf, B, c.n_mels, T, 0, nullptr, nullptr, h->d_pstats, st);
         }))) return rc;
    // prolog: relu(BN(Conv1dSamePadding(n_mels, H, 3)))                          TitaNet.py:226-227, titanet_blocks.py:123-139
    GemmParams pp = conv_params(h, h->tn_prolog, h->X_in, c.n_mels, PRO, H, M, T);
    pp.act1 = ACT_RELU; pp.pad_mode = PAD_ZERO;
    if ((rc = conv_gemm(h, h->tn_prolog, pp))) return rc;
    const int nb = (int)h->tn.size();
    const void* x = PRO;
    for (int i = 0; i < nb; ++i) {
        const svhip_handle::TnBlock& Bk = h->tn[i];
        if ((rc = conv_gemm(h, Bk.skip, conv_params(h, Bk.skip, x, H, K, H, M, T)))) return rc;
        if (i == 0 && (rc = run(h, "tn_dw", 2.0 * k * H * M, [&]() { return launch_tn_dw(x, D0, Bk.dw_w[0], Bk.dw_b[0], dt, k, B, T, H, st); })))
            return rc;
        const void* d = i == 0 ? D0 : D;
        GemmPlan g3;
        for (int j = 0; j < 3; ++j) {
            GemmParams p = conv_params(h, Bk.pw[j], d, H, S, H, M, T);
            p.act1 = ACT_RELU;
            if (j == 2) { p.colsum = cs; p.colsum_stride = h->colsum_region; }
            if ((rc = conv_gemm(h, Bk.pw[j], p, nullptr, 0, &g3))) return rc;
            if (j < 2) {
                if ((rc = run(h, "tn_dw", 2.0 * k * H * M, [&]() { return launch_tn_dw(S, D, Bk.dw_w[j + 1], Bk.dw_b[j + 1], dt, k, B, T, H, st); })))
                    return rc;
                d = D;
            }
        }
        // squeeze-excitation (titanet_blocks.py:162-192): the squeeze from the GEMM's column sums when its kernel wrote them
        const bool from_part = g3.colsum_groups != 0;
        if (!from_part && (rc = run(h, "tn_se_mean", 0, [&]() { return launch_colmean(S, dt, H, B, T, H, h->tn_mean, st); }))) return rc;
        if ((rc = run(h, "tn_se_mlp", 4.0 * B * (H / 16) * H, [&]() {
                 return launch_se_mlp(from_part ? nullptr : h->tn_mean, from_part ? cs : nullptr, T, bf ? Bk.se1_bf : (const void*)Bk.se1, h->d_zeros,
                                      bf ? Bk.se2T_bf : (const void*)Bk.se2T, h->d_zeros, h->tn_gate, bf, B, H, H / 16, st, from_part ? g3.colsum_groups : 8);
             }))) return rc;
        // relu(skip + SE(sub_blocks(x))) and the next block's first depthwise conv                     TitaNet.py:306-318
        const svhip_handle::TnBlock* nx = i + 1 < nb ? &h->tn[i + 1] : nullptr;
        if ((rc = run(h, "tn_mega_tail", nx ? 2.0 * k * H * M : 0.0, [&]() {
                 return launch_tn_mega_tail(K, S, h->tn_gate, X, nx ? nx->dw_w[0] : nullptr, nx ? nx->dw_b[0] : nullptr, nx ? D : nullptr, dt, k, B, T, H, st);
             }))) return rc;
        x = X;
    }
    // epilog: relu(BN(conv1x1(x)))                                                   TitaNet.py:244-245
    GemmParams pe = conv_params(h, h->tn_epilog, x, H, h->tn_enc, E, M, T);
    pe.act1 = ACT_RELU;
    if ((rc = conv_gemm(h, h->tn_epilog, pe))) return rc;
    // attentive statistics pooling (TitaNet.py:389-431): energies = out_linear(tanh(in_linear(x))), softmax over T, mean and
    // sqrt(clamp(var, 1e-6)) (the variance in the centred form), then decoder.pool.1
    GemmParams pa = conv_params(h, h->tn_att_in, h->tn_enc, E, h->tn_att, 128, M, T);
    pa.act2 = ACT_TANH;
    if ((rc = conv_gemm(h, h->tn_att_in, pa))) return rc;
    GemmParams pl = conv_params(h, h->tn_att_out, h->tn_att, 128, h->tn_logits, E, M, T);
    pl.out_f32 = 1;
    if ((rc = conv_gemm(h, h->tn_att_out, pl))) return rc;
    if ((rc = run(h, "tn_asp_pool", 0, [&]() {
             return launch_asp_pool(h->tn_logits, h->tn_enc, bf, E, B, T, E, h->tn_pbn_scale, h->tn_pbn_shift, h->tn_pool_raw, h->tn_pool, 1e-6f, 0.0f, st);
         }))) return rc;
    // an utterance with a non-finite input value gets a NaN embedding, as in the reference (the ReLU epilogues would have dropped it)
    if ((rc = run(h, "tn_in_check", 0, [&]() {
             return launch_tn_nonfinite_rows(d_feat, (int64_t)c.n_mels * T, B, h->tn_pool, 2 * E, 2 * E, st);
         }))) return rc;
    // decoder.linear: Linear(3072, nOut) with BatchNorm1d(nOut) folded in                                     TitaNet.py:355-358
    return run(h, "tn_fc", 2.0 * B * h->tn_fc.N * h->tn_fc.K, [&]() {
        return launch_rowvec_linear(h->tn_pool, 2 * E, h->tn_fc.W, h->tn_fc.bias, h->d_emb, c.embed_dim, B, c.embed_dim, 2 * E, ACT_NONE, st);
    });
}

int titanet_forward(svhip_handle* h, const float* d_feat, int B) { return forward_lanes(h, titanet_forward_part, d_feat, B, 1, B); }

}  // namespace svhip
