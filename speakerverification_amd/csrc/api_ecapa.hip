// api_ecapa.hip — ECAPA-TDNN in libsvhip: its create rules, weight names and packing, workspace, forward and stages.
#include <algorithm>

#include "handle.h"

namespace svhip {

namespace {

struct EcapaState : ModelState {
    // ECAPA layers
    ConvLayer blocks0, mfa, asp_tdnn, asp_conv;
    ConvLayer tdnn1[3], tdnn2[3], res2[3][7];
    LinearLayer se1[3], se2[3], asp_ctx, fc;
    float* se2T[3] = {};                      // se_block.conv2 weight transposed to [128][C]
    void *se1_bf[3] = {}, *se2T_bf[3] = {};   // bf16 copies of both SE matrices (bf16 handles: half the L2 bytes per workgroup)
    float *aspbn_scale = nullptr, *aspbn_shift = nullptr;

    bool xin_ready = false;       // the fused front-end has written X_in: ecapa_forward_part skips its prologue
    bool x0_is_s32 = false;       // SVHIP_F32X3: the last forward wrote blocks.0's output (X0) in the split layout
    bool cat_f32_stale = false;   // SVHIP_F32X3: the last forward left the block outputs only in cat_s32 (svhip_get_stage converts on demand)
    bool h2_is_s32 = false;       // SVHIP_F32X3: the last forward's block-3 Res2Net chain output exists only in h2_s32 (the R2 step kernels)
    bool h1_split = false;        // ... and block 3's tdnn1 wrote its first two chunks in the split layout only (H1 does not hold them)
    void* cat_s32 = nullptr;      // SVHIP_F32X3: the SE-Res2Net block outputs (the CAT buffer) in the S32 layout, written by se_apply
    void* h2_s32 = nullptr;       // SVHIP_F32X3: the Res2Net chain output (H2's twin, S32 only) and the two step-input buffers (M x C/8)
    void* u_s32[2] = {};
    void* X0 = nullptr;           // (M, C)
    void *H1 = nullptr, *H2 = nullptr, *H3 = nullptr;   // (M, C)
    void* CAT = nullptr;          // (M, 3C)
    void* MFA = nullptr;          // (M, 3C)
    void* ATT = nullptr;          // (M, 128)
    float* LOGITS = nullptr;      // (M, 3C) fp32
    float *d_mean = nullptr, *d_s1 = nullptr, *d_s2 = nullptr, *d_gstats = nullptr, *d_ctx = nullptr;
    float *d_pool_raw = nullptr, *d_pool_bn = nullptr;

    // ragged batches (svhip_embed_wave_ragged / svhip_embed_features_ragged): allocated by the handle's first ragged call
    RagTables rag;                            // the tables of a call (one level: mel frames, max_batch * T rows) and the waveform staging buffer
    float* rag_stats = nullptr;               // (max_batch * n_mels * 2) shift / scale of the front-end normalisation
};

EcapaState& S(svhip_handle* h) { return static_cast<EcapaState&>(*h->model); }

}  // namespace

int ecapa_check(const svhip_config& c, const char*& err) {
    if (c.channels <= 0 || c.channels % 64 != 0) { err = "ECAPA channels must be a positive multiple of 64"; return SVHIP_ERR_INVALID; }
    if (c.compute == SVHIP_F16) { err = "SVHIP_F16 is RawNet2's 16-bit mode (ECAPA's is SVHIP_BF16)"; return SVHIP_ERR_UNSUPPORTED; }
    if (c.hop_length > 0 && c.samples / c.hop_length + 1 <= 4) {
        err = "ECAPA needs T = L / hop + 1 >= 5 frames: block 3 reflect-pads 4 frames on each side of every utterance";
        return SVHIP_ERR_INVALID;
    }
    return SVHIP_OK;
}

// ---- expected weight names / shapes ----------------------------------------------------------------
const int ECAPA_K[5] = {5, 3, 3, 3, 1};
const int ECAPA_D[5] = {1, 2, 3, 4, 1};

void ecapa_spec(const svhip_config& c, WeightSpec& spec) {
    const int64_t C = c.channels, C3 = 3 * C, nm = c.n_mels;
    auto tdnn = [&](const std::string& p, int64_t cin, int64_t cout, int64_t k) {
        spec[p + ".conv.conv.weight"] = {cout, cin, k}; spec[p + ".conv.conv.bias"] = {cout};
        spec_bn(spec, p + ".norm.norm", cout);
    };
    if (c.input_norm) { spec["instance_norm.weight"] = {nm}; spec["instance_norm.bias"] = {nm}; }
    tdnn("blocks.0", nm, C, ECAPA_K[0]);
    for (int i = 1; i <= 3; ++i) {
        const std::string p = "blocks." + std::to_string(i);
        tdnn(p + ".tdnn1", C, C, 1);
        for (int j = 0; j < 7; ++j) tdnn(p + ".res2net_block.blocks." + std::to_string(j), C / 8, C / 8, ECAPA_K[i]);
        tdnn(p + ".tdnn2", C, C, 1);
        spec[p + ".se_block.conv1.conv.weight"] = {128, C, 1}; spec[p + ".se_block.conv1.conv.bias"] = {128};
        spec[p + ".se_block.conv2.conv.weight"] = {C, 128, 1}; spec[p + ".se_block.conv2.conv.bias"] = {C};
    }
    tdnn("mfa", C3, C3, 1);
    tdnn("asp.tdnn", 3 * C3, 128, 1);
    spec["asp.conv.conv.weight"] = {C3, 128, 1}; spec["asp.conv.conv.bias"] = {C3};
    spec_bn(spec, "asp_bn.norm", 2 * C3);
    spec["fc.conv.weight"] = {(int64_t)c.embed_dim, 2 * C3, 1}; spec["fc.conv.bias"] = {(int64_t)c.embed_dim};
}

static int make_tdnn(svhip_handle* h, ConvLayer& L, const std::string& p, int dil) {
    return make_conv(h, L, p + ".conv.conv.weight", p + ".conv.conv.bias", p + ".norm.norm", dil);
}

int ecapa_finalize(svhip_handle* h) {
    auto& s = S(h);
    const int C = h->cfg.channels, C3 = 3 * C;
    int rc;
    if ((rc = make_tdnn(h, s.blocks0, "blocks.0", ECAPA_D[0]))) return rc;
    for (int i = 1; i <= 3; ++i) {
        const std::string p = "blocks." + std::to_string(i);
        if ((rc = make_tdnn(h, s.tdnn1[i - 1], p + ".tdnn1", 1))) return rc;
        for (int j = 0; j < 7; ++j)
            if ((rc = make_tdnn(h, s.res2[i - 1][j], p + ".res2net_block.blocks." + std::to_string(j), ECAPA_D[i]))) return rc;
        if ((rc = make_tdnn(h, s.tdnn2[i - 1], p + ".tdnn2", 1))) return rc;
        if ((rc = make_linear(h, s.se1[i - 1], p + ".se_block.conv1.conv.weight", p + ".se_block.conv1.conv.bias"))) return rc;
        if ((rc = make_linear(h, s.se2[i - 1], p + ".se_block.conv2.conv.weight", p + ".se_block.conv2.conv.bias"))) return rc;
        {
            const HostTensor* w2 = getw(h, p + ".se_block.conv2.conv.weight");      // (C, 128, 1)
            std::vector<float> t((size_t)128 * C);
            for (int c = 0; c < C; ++c)
                for (int n = 0; n < 128; ++n) t[(size_t)n * C + c] = w2->data[(size_t)c * 128 + n];
            if ((rc = dev_upload(h, &s.se2T[i - 1], t))) return rc;
            if (h->bf16) {
                const HostTensor* w1 = getw(h, p + ".se_block.conv1.conv.weight");  // (128, C, 1)
                if ((rc = upload_h16(h, w1->data, &s.se1_bf[i - 1])) || (rc = upload_h16(h, t, &s.se2T_bf[i - 1]))) return rc;
            }
        }
    }
    if ((rc = make_tdnn(h, s.mfa, "mfa", 1))) return rc;
    // asp.tdnn over cat[x, mean, std]: the x columns go through the GEMM, the time-constant columns
    // become a per-utterance bias (ctx) computed by a small linear layer.
    if ((rc = make_conv(h, s.asp_tdnn, "asp.tdnn.conv.conv.weight", "", "asp.tdnn.norm.norm", 1, 0, C3))) return rc;
    if ((rc = make_linear(h, s.asp_ctx, "asp.tdnn.conv.conv.weight", "asp.tdnn.conv.conv.bias", C3, 3 * C3))) return rc;
    if ((rc = make_conv(h, s.asp_conv, "asp.conv.conv.weight", "asp.conv.conv.bias", "", 1))) return rc;
    if ((rc = make_bn(h, "asp_bn.norm", 2 * C3, &s.aspbn_scale, &s.aspbn_shift))) return rc;
    if ((rc = make_linear(h, s.fc, "fc.conv.weight", "fc.conv.bias"))) return rc;
    if (h->cfg.input_norm) {
        const HostTensor *w = getw(h, "instance_norm.weight"), *b = getw(h, "instance_norm.bias");
        if (!w || !b) SV_FAIL(h, SVHIP_ERR_MISSING, "missing instance_norm tensors");
        if ((rc = dev_upload(h, &h->in_w, w->data))) return rc;
        if ((rc = dev_upload(h, &h->in_b, b->data))) return rc;
    }
    // algorithmic FLOPs per utterance: 2 x MACs of every conv / linear (SURVEY §8d counts the same)
    const double T = h->T;
    double f = T * s.blocks0.flops_per_row + T * s.mfa.flops_per_row + T * s.asp_conv.flops_per_row;
    f += T * 2.0 * 128 * (3.0 * C3);                                  // asp.tdnn over the full 9C input, as the reference computes it
    for (int i = 0; i < 3; ++i) {
        f += T * (s.tdnn1[i].flops_per_row + s.tdnn2[i].flops_per_row);
        for (int j = 0; j < 7; ++j) f += T * s.res2[i][j].flops_per_row;
        f += 2.0 * s.se1[i].N * s.se1[i].K + 2.0 * s.se2[i].N * s.se2[i].K;
    }
    f += 2.0 * s.fc.N * s.fc.K;
    h->flops_per_utt = f;
    return SVHIP_OK;
}

int ecapa_alloc(svhip_handle* h) {
    h->model = std::make_unique<EcapaState>();
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const size_t B = c.max_batch, T = h->T, M = B * T, C = c.channels, C3 = 3 * C;
    int rc;
    if ((rc = actbuf(h, &h->X_in, M * c.n_mels))) return rc;
    if ((rc = actbuf(h, &s.X0, M * C))) return rc;
    if ((rc = actbuf(h, &s.H1, M * C))) return rc;
    if ((rc = actbuf(h, &s.H2, M * C))) return rc;
    if ((rc = actbuf(h, &s.H3, M * C))) return rc;
    if ((rc = actbuf(h, &s.CAT, M * C3))) return rc;
    if ((rc = actbuf(h, &s.MFA, M * C3))) return rc;
    if ((rc = actbuf(h, &s.ATT, M * 128))) return rc;
    if ((rc = dev_alloc(h, &s.LOGITS, M * C3))) return rc;
    if ((rc = dev_alloc(h, &s.d_mean, B * C))) return rc;
    if ((rc = dev_alloc(h, &s.d_s1, B * 128))) return rc;
    if ((rc = dev_alloc(h, &s.d_s2, B * C))) return rc;
    if ((rc = dev_alloc(h, &s.d_gstats, B * 2 * C3))) return rc;
    if ((rc = dev_alloc(h, &s.d_ctx, B * 128))) return rc;
    h->lin_part_per_utt = (size_t)((2 * C3 + 383) / 384) * (size_t)std::max(128, c.embed_dim);
    if ((rc = dev_alloc(h, &h->d_lin_part, B * h->lin_part_per_utt))) return rc;
    if ((rc = dev_alloc(h, &s.d_pool_raw, B * 2 * C3))) return rc;
    if ((rc = dev_alloc(h, &s.d_pool_bn, B * 2 * C3))) return rc;
    if (h->x3 && (rc = dev_alloc(h, reinterpret_cast<char**>(&h->s32_buf), M * C3 * 4 + 256))) return rc;
    if (h->x3 && C % 32 == 0 && (rc = dev_alloc(h, reinterpret_cast<char**>(&s.cat_s32), M * C3 * 4 + 256))) return rc;
    if (h->x3 && (C == 512 || C == 1024)) {
        if ((rc = dev_alloc(h, reinterpret_cast<char**>(&s.h2_s32), M * C * 4 + 256))) return rc;
        for (int i = 0; i < 2; ++i) if ((rc = dev_alloc(h, reinterpret_cast<char**>(&s.u_s32[i]), M * (C / 8) * 4 + 256))) return rc;
    }
    h->colsum_region = (int64_t)((M + 255) / 256 + 2) * 16 * C3;
    if ((rc = dev_alloc(h, &h->d_colsum, (size_t)4 * h->colsum_region))) return rc;
    return SVHIP_OK;
}

// ECAPA_TDNN.forward (models/ECAPA_TDNN.py:460-502) on device-resident features (B, n_mels, T)
// for the utterances [b0, b0 + B) of the call, enqueued on h->cur.  Every workspace buffer is frame-major, so a
// batch slice is just a row offset: two slices can run concurrently on two streams (lanes).
static int ecapa_forward_part(svhip_handle* h, const float* d_feat_all, int b0, int B) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const int T = h->T, M = B * T, C = c.channels, C3 = 3 * C, C8 = C / 8, e = h->esz;
    const bool bf = h->bf16;
    hipStream_t st = h->cur;
    const size_t r0 = (size_t)b0 * T;                       // first activation row of the slice
    const float* d_feat = d_feat_all + (size_t)b0 * c.n_mels * T;
    void* X_in = off(h->X_in, r0 * c.n_mels, e);
    void* X0 = off(s.X0, r0 * C, e);
    void* H1 = off(s.H1, r0 * C, e);
    void* H2 = off(s.H2, r0 * C, e);
    void* H3 = off(s.H3, r0 * C, e);
    void* CAT = off(s.CAT, r0 * C3, e);
    void* MFA = off(s.MFA, r0 * C3, e);
    void* ATT = off(s.ATT, r0 * 128, e);
    float* LOGITS = s.LOGITS + r0 * C3;
    float* d_pstats = h->d_pstats + (size_t)b0 * c.n_mels * 2;
    float* d_mean = s.d_mean + (size_t)b0 * C;
    float* d_s2 = s.d_s2 + (size_t)b0 * C;
    float* d_gstats = s.d_gstats + (size_t)b0 * 2 * C3;
    float* d_ctx = s.d_ctx + (size_t)b0 * 128;
    float* d_pool_raw = s.d_pool_raw + (size_t)b0 * 2 * C3;
    float* d_pool_bn = s.d_pool_bn + (size_t)b0 * 2 * C3;
    float* d_emb = h->d_emb + (size_t)b0 * c.embed_dim;
    float* cs_base = ((bf || h->x3) && h->d_colsum) ? h->d_colsum + (b0 ? 2 * h->colsum_region : 0) : nullptr;
    int rc;
    // F32X3: se_apply also leaves each block output in the S32 split layout (CAT's twin), so tdnn1 of the next block and mfa read
    // their A operand without a conversion pass
    char* cat32 = s.cat_s32 ? static_cast<char*>(s.cat_s32) + r0 * C3 * 4 : nullptr;
    // ... and when every consumer of a block output takes the split operand at this batch size (tdnn1 of the next block, mfa with its
    // column sums: the persistent X3 kernel; the next se_apply reads its residual as hi + lo), the fp32 copy is not written at all
    auto tdnn1_params = [&](int i, const void* a, int lda) { GemmParams p = conv_params(h, s.tdnn1[i], a, lda, H1, C, M, T); p.act1 = ACT_GELU; return p; };
    GemmParams pm = conv_params(h, s.mfa, CAT, C3, MFA, C3, M, T);
    pm.act1 = ACT_GELU;
    pm.colsum = cs_base; pm.colsum_sq = 1; pm.colsum_stride = h->colsum_region;
    GemmPlan gm = conv_plan(h, s.mfa, pm, cat32, C3);
    const bool s32_only = cat32 && conv_plan(h, s.tdnn1[1], tdnn1_params(1, nullptr, C3), cat32, C3).x3 &&
                          conv_plan(h, s.tdnn1[2], tdnn1_params(2, nullptr, C3), cat32 + (size_t)C * 4, C3).x3 && gm.x3 && (gm.colsum_groups || !pm.colsum) &&
                          !h->opt.x3_keep_f32;
    if (s32_only) s.cat_f32_stale = true;
    bool b0_done = false, x0_s32 = false, b0_cv = false;
    GemmParams q0;
    float* xscale = h->d_xscale ? h->d_xscale + (b0 ? 4 + 256 : 0) : nullptr;
    if (h->x3 && s.blocks0.Wcv && h->s32_buf) {
        // F32X3: blocks.0 on the persistent kernel's conv-gather form: the features go to the S32 layout with rows zero-padded to
        // cv_cin channels (one small pass), the im2col view is formed by the operand DMAs
        const ConvLayer& L = s.blocks0;
        GemmParams& q = q0;
        q = conv_params(h, L, h->s32_buf, L.cv_cin, X0, C, M, T);
        q.W = L.Wcv; q.Wrows = L.N; q.x3 = 2; q.K = L.taps * L.cv_cin; q.Kp = L.cv_Kp; q.cin = L.cv_cin; q.act1 = ACT_GELU;
        // (with s32_only and tdnn1 of the first block on the X3 kernel, X0 itself is written in the split layout: no conversion pass,
        //  block 1's residual is read as hi + lo, svhip_get_stage rebuilds the fp32 view)
        q.y_s32 = (s32_only && conv_plan(h, s.tdnn1[0], tdnn1_params(0, nullptr, C), X0, C).x3) ? 1 : 0;
        q.in_scale = xscale;
        b0_cv = gemm_pw3cv_supported(q);
    }
    // the prologue's range guard (F32X3: half-precision planes carry |x| <= 65504): with the scaled first convolution only a non-finite
    // input is reported — a finite one of any magnitude is brought into the planes' range by an exact power of two (round 6)
    if (!s.xin_ready && (rc = run(h, "prologue", 0, [&]() {
             return launch_prologue(d_feat, X_in, bf, B, c.n_mels, T, c.log_input, h->in_w, h->in_b, d_pstats, st,
                                    h->x3 ? h->d_status : nullptr, h->host_flag_dev, (b0_cv && xscale) ? 3.0e38f : 65504.0f);
         }))) return rc;
    if (b0_cv) {
        const ConvLayer& L = s.blocks0;
        if (xscale && (rc = run(h, "in_scale", 0, [&]() {
                 return launch_in_scale(static_cast<const float*>(X_in), (int64_t)M * c.n_mels, reinterpret_cast<uint32_t*>(xscale + 4), xscale, st, L.cv_wscale);
             }))) return rc;
        if ((rc = run(h, "split_s32", 0, [&]() { return launch_split_s32(static_cast<const float*>(X_in), c.n_mels, h->s32_buf, M, L.cv_cin, st, L.cv_cin, c.n_mels, xscale); }))) return rc;
        if ((rc = run(h, "gemm_pw3cv", (double)M * L.flops_per_row, [&]() { return launch_gemm_pw3cv(q0, st); }))) return rc;
        b0_done = true;
        x0_s32 = q0.y_s32 != 0;
    }
    if (!b0_done) {
        GemmParams p = conv_params(h, s.blocks0, X_in, c.n_mels, X0, C, M, T);
        p.act1 = ACT_GELU;
        if ((rc = conv_gemm(h, s.blocks0, p))) return rc;
    }
    s.x0_is_s32 = x0_s32;
    const void* xin = x0_s32 ? nullptr : X0;
    int ldin = C;
    const void* xin32 = x0_s32 ? X0 : nullptr;
    int ldin32 = C;
    for (int i = 0; i < 3; ++i) {
        // F32X3: seven launches of gemm_pw3's Res2Net step form; step j reads U_j = c_j + y_{j-1} (S32) and writes y_j (S32, into the
        // chain output) and U_{j+1}; no fp32 copy of the chain exists
        char* h2s = s.h2_s32 ? static_cast<char*>(s.h2_s32) + r0 * C * 4 : nullptr;
        char* us[2] = {s.u_s32[0] ? static_cast<char*>(s.u_s32[0]) + r0 * C8 * 4 : nullptr, s.u_s32[1] ? static_cast<char*>(s.u_s32[1]) + r0 * C8 * 4 : nullptr};
        auto step_params = [&](int j) {
            const ConvLayer& L = s.res2[i][j - 1];
            GemmParams q = conv_params(h, L, us[(j - 1) & 1], C8, h2s + (size_t)j * C8 * 4, C, M, T);
            q.W = L.Ws32; q.Wrows = L.N; q.x3 = 2; q.act1 = ACT_RELU;
            if (j < 7) { q.R = static_cast<const float*>(H1) + (size_t)(j + 1) * C8; q.ldr = C; q.Y2 = us[j & 1]; q.lda2 = C8; }
            return q;
        };
        // tdnn2; its epilogue also leaves per-utterance column sums (the SE squeeze) when the pw2 kernel runs
        GemmParams p2 = conv_params(h, s.tdnn2[i], H2, C, H3, C, M, T);
        p2.act1 = ACT_GELU;
        p2.colsum = cs_base; p2.colsum_stride = h->colsum_region;
        // (C / 8 = 128: the dedicated 128 x 128 kernel, two workgroups per CU, any batch size; C / 8 = 64, or SVHIP_R2_BIG=1: the R2 form
        //  of the persistent 256 x 256 kernel)
        const bool r2_small = h->x3 && h2s && us[0] && us[1] && s.res2[i][0].Ws32 && !h->opt.r2_big && r2_step_supported(step_params(1)) &&
                              conv_plan(h, s.tdnn2[i], p2, h2s, C).x3;      // (tdnn2 must be able to read the chain output in the split layout)
        const bool r2_plan = r2_small || (h->x3 && h2s && us[0] && us[1] && s.res2[i][0].Ws32 && gemm_pw3r2_supported(step_params(1)));
        GemmParams p1 = tdnn1_params(i, (s32_only && (i > 0 || x0_s32)) ? nullptr : xin, ldin);
        if (r2_plan) {      // tdnn1 writes the pass-through chunk and the first step's input in the split layout itself (when it takes the X3 kernel)
            p1.side_a = h2s; p1.side_lda = C; p1.side_b = us[0]; p1.side_ldb = C8; p1.side_c = C8;
        }
        GemmPlan g1;
        if ((rc = conv_gemm(h, s.tdnn1[i], p1, xin32, ldin32, &g1))) return rc;
        if (i == 2) { s.h2_is_s32 = r2_plan; s.h1_split = r2_plan && g1.side; }      // (what svhip_get_stage can read back of block 3)
        if (r2_plan) {
            if (!g1.side) {
                if ((rc = run(h, "split_s32", 0, [&]() { return launch_split_s32(static_cast<const float*>(H1), C, h2s, M, C8, st, C); }))) return rc;
                if ((rc = run(h, "split_s32", 0, [&]() { return launch_split_s32(static_cast<const float*>(H1) + C8, C, us[0], M, C8, st, C8); }))) return rc;
            }
            for (int j = 1; j < 8; ++j) {
                const GemmParams q = step_params(j);
                if (r2_small) {
                    if ((rc = run(h, "r2_step", (double)M * s.res2[i][j - 1].flops_per_row, [&]() { return launch_r2_step(q, st); }))) return rc;
                } else if ((rc = run(h, "gemm_pw3r2", (double)M * s.res2[i][j - 1].flops_per_row, [&]() { return launch_gemm_pw3r2(q, st); }))) return rc;
            }
            p2.A = nullptr;      // (tdnn2 reads the chain output in the S32 layout only)
        } else if (bf && res2net_chain_supported(C, T, s.res2[i][0].dil, s.res2[i][0].Kp)) {
            Res2Params rp;
            rp.H1 = H1; rp.H2 = H2; rp.ld = C; rp.T = T; rp.dil = s.res2[i][0].dil; rp.Kp = s.res2[i][0].Kp;
            // small batches (the reference's per-file calls: B = num_eval crops): time slices, so that the chip is not left to B workgroups
            rp.slices = h->opt.r2_slices >= 0 ? std::max(1, h->opt.r2_slices) : res2net_chain_slices(B, C, T, rp.dil, h->num_cu);
            double fl = 0;
            for (int j = 0; j < 7; ++j) {
                rp.W[j] = s.res2[i][j].W; rp.bias[j] = s.res2[i][j].bias;
                rp.scale[j] = s.res2[i][j].scale; rp.shift[j] = s.res2[i][j].shift;
                fl += (double)M * s.res2[i][j].flops_per_row;
            }
            if ((rc = run(h, rp.slices > 1 ? "res2net_slices" : "res2net_chain", fl, [&]() { return launch_res2net_chain(rp, B, C, st); }))) return rc;
        } else {
            if ((rc = run(h, "copy_cols", 0, [&]() { return launch_copy_cols(H1, C, H2, C, bf, M, C8, st); }))) return rc;
            for (int j = 1; j < 8; ++j) {
                GemmParams p = conv_params(h, s.res2[i][j - 1], off(H1, (size_t)j * C8, e), C, off(H2, (size_t)j * C8, e), C, M, T);
                p.act1 = ACT_RELU;
                p.A2 = j >= 2 ? off(H2, (size_t)(j - 1) * C8, e) : nullptr; p.lda2 = C;
                if ((rc = conv_gemm(h, s.res2[i][j - 1], p))) return rc;
            }
        }
        GemmPlan g2;
        if ((rc = conv_gemm(h, s.tdnn2[i], p2, r2_plan ? h2s : nullptr, C, &g2))) return rc;
        const bool from_part = g2.colsum_groups != 0;      // the squeeze comes straight from the GEMM's column-sum partials
        if (!from_part) {
            if ((rc = run(h, "se_mean", 0, [&]() { return launch_colmean(H3, bf, C, B, T, C, d_mean, st); }))) return rc;
        }
        if ((rc = run(h, "se_mlp", 4.0 * B * 128 * C, [&]() {
                 return launch_se_mlp(from_part ? nullptr : d_mean, from_part ? cs_base : nullptr, T,
                                      bf ? (const void*)s.se1_bf[i] : (const void*)s.se1[i].W, s.se1[i].bias,
                                      bf ? (const void*)s.se2T_bf[i] : (const void*)s.se2T[i], s.se2[i].bias, d_s2, bf, B, C, 128, st,
                                      from_part ? g2.colsum_groups : 8);      // (8: any count the kernel takes; no partials are read)
             }))) return rc;
        void* xout = off(CAT, (size_t)i * C, e);
        void* xout32 = cat32 ? cat32 + (size_t)i * C * 4 : nullptr;
        if ((rc = run(h, "se_apply", 0, [&]() {
                 return launch_se_apply(H3, C, d_s2, xin, ldin, s32_only ? nullptr : xout, C3, bf, B, T, C, st, xout32, C3,
                                        s32_only && (i > 0 || x0_s32) ? xin32 : nullptr, ldin32);
             })))
            return rc;
        xin = xout;
        xin32 = xout32;
        ldin = C3;
        ldin32 = C3;
    }
    if (s32_only) pm.A = nullptr;
    if ((rc = conv_gemm(h, s.mfa, pm, cat32, C3, &gm))) return rc;
    if (gm.colsum_groups) {
        if ((rc = run(h, "colsum_finalize", 0, [&]() { return launch_colsum_finalize(cs_base, h->colsum_region, true, B, T, C3, M, d_gstats, 1e-12f, st, gm.colsum_groups); }))) return rc;
    } else {
        if ((rc = run(h, "asp_gstats", 0, [&]() { return launch_colstats(MFA, bf, C3, B, T, C3, d_gstats, 1e-12f, st); }))) return rc;
    }
    if ((rc = run(h, "asp_ctx", 2.0 * B * 128 * 2 * C3, [&]() {
             return launch_rowvec_linear(d_gstats, 2 * C3, s.asp_ctx.W, s.asp_ctx.bias, d_ctx, 128, B, 128, 2 * C3, ACT_NONE, st, h->d_lin_part + (size_t)b0 * h->lin_part_per_utt);
         }))) return rc;
    GemmParams pa = conv_params(h, s.asp_tdnn, MFA, C3, ATT, 128, M, T);
    pa.act1 = ACT_RELU; pa.act2 = ACT_TANH;
    pa.bias_utt = d_ctx; pa.ld_bu = 128;
    if ((rc = conv_gemm(h, s.asp_tdnn, pa))) return rc;
    // bf16: 16 waves per CU, lane-local online softmax (asp_x3.hip's bf16 form: 0.195 against 0.264 ms at B = 256, any T); the
    // one-wave-per-SIMD kernel keeps the channel counts that are not multiples of 256 (and SVHIP_ASP_V1=1: the tests compare the two)
    const bool asp_v2 = bf && C3 % 256 == 0 && s.asp_tdnn.N == 128 && s.asp_conv.Kp == 128 && !h->opt.asp_v1;
    if (asp_v2 || (bf && asp_fused_supported(T, C3, s.asp_tdnn.N, s.asp_conv.Kp))) {
        AspFusedParams ap;
        ap.att = ATT; ap.W = s.asp_conv.W; ap.Kp = s.asp_conv.Kp; ap.bias = s.asp_conv.bias;
        ap.X = MFA; ap.ldx = C3; ap.T = T; ap.C = C3;
        ap.bn_scale = s.aspbn_scale; ap.bn_shift = s.aspbn_shift;
        ap.pooled_raw = d_pool_raw; ap.pooled_bn = d_pool_bn; ap.eps = 1e-12f;
        if (asp_v2) {
            if ((rc = run(h, "asp_bf16", (double)M * s.asp_conv.flops_per_row, [&]() { return launch_asp_bf16(ap, d_gstats, 2 * C3, B, st); }))) return rc;
        } else
        if ((rc = run(h, "asp_fused", (double)M * s.asp_conv.flops_per_row, [&]() { return launch_asp_fused(ap, B, st); }))) return rc;
    } else if (h->x3 && s.asp_conv.Ws32 && asp_x3_supported(T, C3, s.asp_tdnn.N, s.asp_conv.K)) {
        AspX3Params ap;
        ap.att = (const float*)ATT; ap.Ws32 = s.asp_conv.Ws32; ap.X = (const float*)MFA; ap.ldx = C3; ap.T = T; ap.C = C3;
        ap.mref = d_gstats; ap.mref_ld = 2 * C3;                  // [mean | std] per utterance: the means
        ap.bn_scale = s.aspbn_scale; ap.bn_shift = s.aspbn_shift;
        ap.pooled_raw = d_pool_raw; ap.pooled_bn = d_pool_bn; ap.eps = 1e-12f;
        if ((rc = run(h, "asp_x3", (double)M * s.asp_conv.flops_per_row, [&]() { return launch_asp_x3(ap, B, st); }))) return rc;
    } else {
        GemmParams p = conv_params(h, s.asp_conv, ATT, 128, LOGITS, C3, M, T);
        p.out_f32 = 1;
        if ((rc = conv_gemm(h, s.asp_conv, p))) return rc;
        if ((rc = run(h, "asp_pool", 0, [&]() {
                 return launch_asp_pool(LOGITS, MFA, bf, C3, B, T, C3, s.aspbn_scale, s.aspbn_shift, d_pool_raw, d_pool_bn, 1e-12f, 0.0f, st);
             }))) return rc;
    }
    if ((rc = run(h, "fc", 2.0 * B * s.fc.N * s.fc.K, [&]() {
             return launch_rowvec_linear(d_pool_bn, 2 * C3, s.fc.W, s.fc.bias, d_emb, c.embed_dim, B, c.embed_dim, 2 * C3, ACT_NONE, st, h->d_lin_part + (size_t)b0 * h->lin_part_per_utt);
         }))) return rc;
    return SVHIP_OK;
}

// whole batch: one lane, or two half-batches on two streams so that kernel tails, launch gaps and the
// small latency-bound kernels of one half overlap the big GEMMs of the other
int ecapa_forward(svhip_handle* h, const float* d_feat, int B) {
    S(h).cat_f32_stale = false;
    const bool two = h->lanes == 2 && B >= 64 && !h->x3;      // (F32X3: the lanes would share the split-operand staging buffer)
    return forward_lanes(h, ecapa_forward_part, d_feat, B, two ? 2 : 1, (B / 2 + 3) & ~3);
}

// the waveform path: bf16 handles without the instance-norm prologue go from the waveform to the 16-bit operand of blocks.0 in two
// launches (fbank.hip, round 6); the others run the fbank, then the forward from the mel power
int ecapa_embed_wave(svhip_handle* h, const float* d_wav, int B) {
    auto& s = S(h);
    const int L = h->cfg.samples, T = h->T;
    const bool fused = h->bf16 && !h->in_w && h->d_logmel && !h->opt.fbank_unfused && !h->opt.fbank32 && fbank_fused_supported(h->fb, L);
    int rc;
    if (fused) {
        if ((rc = run(h, "fbank_fused", 0, [&]() {
                 return launch_fbank_fused(h->fb, d_wav, B, L, T, h->cfg.log_input, h->d_logmel, h->d_fpart, h->X_in, h->stream);
             }))) return rc;
    } else if ((rc = run(h, "fbank", 0, [&]() { return launch_fbank(h->fb, d_wav, B, L, T, h->d_feat, h->stream); }))) return rc;
    s.xin_ready = fused;
    h->feat_is_stale = fused;
    rc = ecapa_forward(h, h->d_feat, B);
    s.xin_ready = false;
    return rc;
}

// ---- ragged batches ------------------------------------------------------------------------------------
// ECAPA's rules for a pack (RaggedCheckFn; include/svhip.h), on the host alone
int ecapa_ragged_check(const svhip_config& c, const int32_t* lengths, int n, bool is_wave, std::string& err) {
    return rag_mel_check(c, lengths, n, is_wave, err, true, "hop_length / max_batch / samples", 5, " (block 3 reflect-pads 4 frames on each side)");
}

// one frame level: the mel frames
static void ecapa_rag_frames(const svhip_config& c, int64_t len, bool is_wave, int T[RAG_LEVELS]) { T[0] = (int)mel_frames(c, len, is_wave); }
static const RagRule kEcapaRag = {1, ecapa_rag_frames, true};

// ECAPA_TDNN.forward over the packed rows of a ragged batch (features at pk.in + pk.off[u]; tables on the device).  One slice on
// the handle's stream.  Every GEMM goes to the generic kernel (launch_gemm_ragged: one kernel at every row count, so that a row's sums
// do not depend on the pack); the convolutions gather through the segment table; the reductions over time are ragged.hip's.
// It stays apart from ecapa_forward_part: that one is mostly route decisions (F32X3 planes, the Res2Net step kernels, fused attention
// heads, two lanes) that this one has none of, and what the two share is too little to pay for one walk.
static int ecapa_forward_ragged(svhip_handle* h, const RagPack& pk) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const int C = c.channels, C3 = 3 * C, C8 = C / 8, e = h->esz;
    const bool bf = h->bf16;
    hipStream_t st = h->cur = h->stream;
    const int n = pk.n, M = pk.lv[0].M, maxT = pk.lv[0].maxT;
    const int *row0 = pk.lv[0].row0, *utt = pk.lv[0].utt;
    int rc;
    auto gemm = [&](const ConvLayer& L, GemmParams p, const char* label) {
        p.rag_utt = utt; p.rag_row0 = row0;
        return run(h, label, (double)M * L.flops_per_row, [&]() { return launch_gemm_ragged(p, bf, st); });
    };
    if ((rc = run(h, "rag_rows", 0, [&]() { return launch_rag_rows(row0, n, maxT, pk.lv[0].utt, st); }))) return rc;
    if ((rc = run(h, "rag_prologue", 0, [&]() {
             return launch_rag_prologue(pk.in, pk.off, row0, n, maxT, h->X_in, bf, c.n_mels, c.log_input, h->in_w, h->in_b, s.rag_stats, st);
         }))) return rc;
    {
        GemmParams p = conv_params(h, s.blocks0, h->X_in, c.n_mels, s.X0, C, M, 1);
        p.act1 = ACT_GELU;
        if ((rc = gemm(s.blocks0, p, "rag_gemm_conv"))) return rc;
    }
    const void* xin = s.X0;
    int ldin = C;
    for (int i = 0; i < 3; ++i) {
        GemmParams p1 = conv_params(h, s.tdnn1[i], xin, ldin, s.H1, C, M, 1);
        p1.act1 = ACT_GELU;
        if ((rc = gemm(s.tdnn1[i], p1, "rag_gemm"))) return rc;
        if ((rc = run(h, "copy_cols", 0, [&]() { return launch_copy_cols(s.H1, C, s.H2, C, bf, M, C8, st); }))) return rc;
        for (int j = 1; j < 8; ++j) {
            GemmParams p = conv_params(h, s.res2[i][j - 1], off(s.H1, (size_t)j * C8, e), C, off(s.H2, (size_t)j * C8, e), C, M, 1);
            p.act1 = ACT_RELU;
            p.A2 = j >= 2 ? off(s.H2, (size_t)(j - 1) * C8, e) : nullptr; p.lda2 = C;
            if ((rc = gemm(s.res2[i][j - 1], p, j >= 2 ? "rag_gemm_conv_add" : "rag_gemm_conv"))) return rc;
        }
        GemmParams p2 = conv_params(h, s.tdnn2[i], s.H2, C, s.H3, C, M, 1);
        p2.act1 = ACT_GELU;
        if ((rc = gemm(s.tdnn2[i], p2, "rag_gemm"))) return rc;
        if ((rc = run(h, "rag_se_mean", 0, [&]() { return launch_rag_colstats(s.H3, bf, C, row0, n, C, s.d_mean, false, 0.0f, st); }))) return rc;
        if ((rc = run(h, "se_mlp", 4.0 * n * 128 * C, [&]() {
                 return launch_se_mlp(s.d_mean, nullptr, 1, bf ? (const void*)s.se1_bf[i] : (const void*)s.se1[i].W, s.se1[i].bias,
                                      bf ? (const void*)s.se2T_bf[i] : (const void*)s.se2T[i], s.se2[i].bias, s.d_s2, bf, n, C, 128, st, 8);
             }))) return rc;
        void* xout = off(s.CAT, (size_t)i * C, e);
        if ((rc = run(h, "rag_se_apply", 0, [&]() { return launch_rag_se_apply(s.H3, C, s.d_s2, xin, ldin, xout, C3, bf, utt, M, C, st); }))) return rc;
        xin = xout;
        ldin = C3;
    }
    GemmParams pm = conv_params(h, s.mfa, s.CAT, C3, s.MFA, C3, M, 1);
    pm.act1 = ACT_GELU;
    if ((rc = gemm(s.mfa, pm, "rag_gemm"))) return rc;
    if ((rc = run(h, "rag_asp_gstats", 0, [&]() { return launch_rag_colstats(s.MFA, bf, C3, row0, n, C3, s.d_gstats, true, 1e-12f, st); }))) return rc;
    if ((rc = run(h, "rag_asp_ctx", 2.0 * n * 128 * 2 * C3, [&]() {
             return launch_rag_linear(s.d_gstats, 2 * C3, s.asp_ctx.W, s.asp_ctx.bias, s.d_ctx, 128, n, 128, 2 * C3, ACT_NONE, st);
         }))) return rc;
    GemmParams pa = conv_params(h, s.asp_tdnn, s.MFA, C3, s.ATT, 128, M, 1);
    pa.act1 = ACT_RELU; pa.act2 = ACT_TANH;
    pa.bias_utt = s.d_ctx; pa.ld_bu = 128;
    if ((rc = gemm(s.asp_tdnn, pa, "rag_gemm_ctx"))) return rc;
    GemmParams pl = conv_params(h, s.asp_conv, s.ATT, 128, s.LOGITS, C3, M, 1);
    pl.out_f32 = 1;
    if ((rc = gemm(s.asp_conv, pl, "rag_gemm"))) return rc;
    if ((rc = run(h, "rag_asp_pool", 0, [&]() {
             return launch_rag_asp_pool(s.LOGITS, s.MFA, bf, C3, row0, n, C3, s.aspbn_scale, s.aspbn_shift, s.d_pool_raw, s.d_pool_bn, 1e-12f, st);
         }))) return rc;
    return run(h, "rag_fc", 2.0 * n * s.fc.N * s.fc.K, [&]() {
        return launch_rag_linear(s.d_pool_bn, 2 * C3, s.fc.W, s.fc.bias, h->d_emb, c.embed_dim, n, c.embed_dim, 2 * C3, ACT_NONE, st);
    });
}

int ecapa_embed_ragged(svhip_handle* h, const float* in, bool in_host, bool is_wave, const int64_t* in_off, const int32_t* lengths, int n) {
    auto& s = S(h);
    const size_t B = h->cfg.max_batch, utt_cap[RAG_LEVELS] = {B * (size_t)h->T};
    RagPack pk;
    int rc;
    if (!s.rag_stats && (rc = dev_alloc(h, &s.rag_stats, B * h->cfg.n_mels * 2))) return rc;
    if ((rc = rag_pack(h, s.rag, kEcapaRag, utt_cap, in, in_host, is_wave, in_off, lengths, n, pk)) || (rc = ecapa_forward_ragged(h, pk))) return rc;
    set_rag_rows(h, pk);
    s.x0_is_s32 = s.cat_f32_stale = s.h2_is_s32 = s.h1_split = false;
    return SVHIP_OK;
}

int ecapa_stage(svhip_handle* h, const std::string& n, bool fill, StageView& v) {
    auto& s = S(h);
    const int C = h->cfg.channels, C3 = 3 * C, B = h->lastB;
    const int64_t M = (int64_t)B * h->T;
    if (n == "blocks.0") {
        v.src = s.X0; v.cols = v.ld = C;
        if (s.x0_is_s32 && fill) {           // F32X3: X0 holds hi | lo planes; the fp32 view goes to the (idle) operand staging buffer
            SV_HIP(h, launch_unsplit_s32(s.X0, C, static_cast<float*>(h->s32_buf), C, M, C, h->stream));
            v.src = h->s32_buf;
        }
    } else if (n == "blocks.1" || n == "blocks.2" || n == "blocks.3") {
        const int i = n.back() - '1';
        v.src = off(s.CAT, (size_t)i * C, h->esz); v.cols = C; v.ld = C3;
        if (s.cat_f32_stale && fill) {       // F32X3: the block outputs exist only in the split layout; rebuild the fp32 view
            SV_HIP(h, launch_unsplit_s32(s.cat_s32, C3, static_cast<float*>(s.CAT), C3, M, C3, h->stream));
            s.cat_f32_stale = false;
        }
    }
    // block 3's inner tensors, the SE gate, the ASP statistics and attention: the forward leaves them in buffers that no later kernel of
    // it writes (H1 / H2 / H3 / ATT and the per-utterance vectors are indexed by the lane's first row or utterance, so the two lanes of a
    // B >= 64 batch fill disjoint parts of them)
    else if (n == "blocks.3.tdnn1") {
        if (s.h1_split)
            SV_FAIL(h, SVHIP_ERR_STATE, "stage blocks.3.tdnn1: the last forward wrote its first two chunks only in the split layout of the "
                                        "Res2Net step kernels, which the chain then overwrote");
        v.src = s.H1; v.cols = v.ld = C;
    } else if (n == "blocks.3.res2net") {
        v.src = s.H2; v.cols = v.ld = C;
        if (s.h2_is_s32 && fill) {           // F32X3 R2 steps: the chain output exists only in h2_s32; the fp32 view goes to the staging buffer
            SV_HIP(h, launch_unsplit_s32(s.h2_s32, C, static_cast<float*>(h->s32_buf), C, M, C, h->stream));
            v.src = h->s32_buf;
        }
    }
    else if (n == "blocks.3.tdnn2") { v.src = s.H3; v.cols = v.ld = C; }
    else if (n == "blocks.3.se_gate") { v.src = s.d_s2; v.rows = B; v.cols = v.ld = C; v.f32 = true; }
    else if (n == "asp_gstats") { v.src = s.d_gstats; v.rows = B; v.cols = v.ld = 2 * C3; v.f32 = true; }      // [mean | std]
    else if (n == "asp_att") { v.src = s.ATT; v.cols = v.ld = 128; }
    else if (n == "mfa") { v.src = s.MFA; v.cols = v.ld = C3; }
    else if (n == "asp") { v.src = s.d_pool_raw; v.rows = B; v.cols = v.ld = 2 * C3; v.f32 = true; }
    else if (n == "asp_bn") { v.src = s.d_pool_bn; v.rows = B; v.cols = v.ld = 2 * C3; v.f32 = true; }
    else return unknown_stage(h, n);
    return SVHIP_OK;
}

}  // namespace svhip
