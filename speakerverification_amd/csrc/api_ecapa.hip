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

    bool xin_ready = false;       // the fused front-end has written X_in: ec_front skips the prologue
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
    float *d_mean = nullptr, *d_s2 = nullptr, *d_gstats = nullptr, *d_ctx = nullptr;
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

// ECAPA_TDNN.forward (models/ECAPA_TDNN.py:460-502) on device-resident features (B, n_mels, T), as steps over one slice of the call:
// utterances [b0, b0 + B), enqueued on `st`.  Every workspace buffer is frame-major, so a batch slice is just a row offset: two slices
// can run concurrently on two streams (lanes).
struct EcPass {
    svhip_handle* h;
    EcapaState& s;
    int b0 = 0, B = 0, M = 0;
    hipStream_t st = nullptr;
    const float* feat = nullptr;              // (B, n_mels, T)
    void *X_in = nullptr, *X0 = nullptr, *H1 = nullptr, *H2 = nullptr, *H3 = nullptr, *CAT = nullptr, *MFA = nullptr, *ATT = nullptr;
    float *LOGITS = nullptr, *d_pstats = nullptr, *d_mean = nullptr, *d_s2 = nullptr, *d_gstats = nullptr, *d_ctx = nullptr;
    float *d_pool_raw = nullptr, *d_pool_bn = nullptr, *d_emb = nullptr;
    float* cs_base = nullptr;                 // the lane's column-sum partials (16-bit and F32X3 handles), or null
    float* xscale = nullptr;                  // F32X3: the lane's scale of the network input and its partial max words, or null
    float* lin_part = nullptr;                // K-slice partials of asp_ctx and fc
    char *h2s = nullptr, *us[2] = {};         // F32X3: the Res2Net chain output and the two step-input buffers (S32 only), or null
    // F32X3: se_apply also leaves each block output in the S32 split layout (CAT's twin), so tdnn1 of the next block and mfa read
    // their A operand without a conversion pass
    char* cat32 = nullptr;
    // ... and when every consumer of a block output takes the split operand at this batch size (tdnn1 of the next block, mfa with its
    // column sums: the persistent X3 kernel; the next se_apply reads its residual as hi + lo), the fp32 copy is not written at all
    bool s32_only = false;
    bool x0_s32 = false;                      // ... nor that of blocks.0's output: X0 is written in the split layout
    // the block loop's cursor, the input of the next block: xin in the handle's type (null where only the split layout holds it),
    // xin32 its S32 twin (null where there is none)
    const void *xin = nullptr, *xin32 = nullptr;
    int ldin = 0, ldin32 = 0;
};

static GemmParams ec_tdnn1_params(const EcPass& p, int i, const void* a, int lda) {
    GemmParams q = conv_params(p.h, p.s.tdnn1[i], a, lda, p.H1, p.h->cfg.channels, p.M, p.h->T);
    q.act1 = ACT_GELU;
    return q;
}

// tdnn2; its epilogue also leaves per-utterance column sums (the SE squeeze) when the pw2 kernel runs
static GemmParams ec_tdnn2_params(const EcPass& p, int i) {
    const int C = p.h->cfg.channels;
    GemmParams q = conv_params(p.h, p.s.tdnn2[i], p.H2, C, p.H3, C, p.M, p.h->T);
    q.act1 = ACT_GELU;
    q.colsum = p.cs_base; q.colsum_stride = p.h->colsum_region;
    return q;
}

// mfa; its epilogue leaves the column sums and sums of squares of the ASP statistics where its kernel can
static GemmParams ec_mfa_params(const EcPass& p) {
    const int C3 = 3 * p.h->cfg.channels;
    GemmParams q = conv_params(p.h, p.s.mfa, p.CAT, C3, p.MFA, C3, p.M, p.h->T);
    q.act1 = ACT_GELU;
    q.colsum = p.cs_base; q.colsum_sq = 1; q.colsum_stride = p.h->colsum_region;
    return q;
}

// EcPass::s32_only: do tdnn1 of blocks 2 and 3 and mfa (with its column sums) all take the split operand at this batch size?
static bool ec_s32_only(const EcPass& p) {
    svhip_handle* h = p.h;
    const int C = h->cfg.channels, C3 = 3 * C;
    if (!p.cat32) return false;
    const GemmParams pm = ec_mfa_params(p);
    const GemmPlan gm = conv_plan(h, p.s.mfa, pm, p.cat32, C3);
    return conv_plan(h, p.s.tdnn1[1], ec_tdnn1_params(p, 1, nullptr, C3), p.cat32, C3).x3 &&
           conv_plan(h, p.s.tdnn1[2], ec_tdnn1_params(p, 2, nullptr, C3), p.cat32 + (size_t)C * 4, C3).x3 && gm.x3 && (gm.colsum_groups || !pm.colsum) &&
           !h->opt.x3_keep_f32;
}

// F32X3: step j (1..7) of block i's Res2Net chain on gemm_pw3's step form; it reads U_j = c_j + y_{j-1} (S32) and writes y_j (S32, into
// the chain output) and U_{j+1}; no fp32 copy of the chain exists
static GemmParams ec_r2_step_params(const EcPass& p, int i, int j) {
    const int C = p.h->cfg.channels, C8 = C / 8;
    const ConvLayer& L = p.s.res2[i][j - 1];
    GemmParams q = conv_params(p.h, L, p.us[(j - 1) & 1], C8, p.h2s + (size_t)j * C8 * 4, C, p.M, p.h->T);
    q.W = L.Ws32; q.Wrows = L.N; q.x3 = 2; q.act1 = ACT_RELU;
    if (j < 7) { q.R = static_cast<const float*>(p.H1) + (size_t)(j + 1) * C8; q.ldr = C; q.Y2 = p.us[j & 1]; q.lda2 = C8; }
    return q;
}

// the Res2Net route of block i: seven launches of a split step kernel (F32X3), the bf16 chain in one launch, or seven per-layer GEMMs
// (C / 8 = 128: the dedicated 128 x 128 step kernel, two workgroups per CU, any batch size; C / 8 = 64, or SVHIP_R2_BIG=1: the R2 form
//  of the persistent 256 x 256 kernel)
enum EcRes2 { RES2_STEP, RES2_PW3R2, RES2_CHAIN, RES2_LAYERS };
static bool ec_res2_split(EcRes2 r) { return r == RES2_STEP || r == RES2_PW3R2; }
static EcRes2 ec_res2_plan(const EcPass& p, int i) {
    svhip_handle* h = p.h;
    const int C = h->cfg.channels;
    const ConvLayer& L = p.s.res2[i][0];
    if (h->x3 && p.h2s && p.us[0] && p.us[1] && L.Ws32) {
        const GemmParams q1 = ec_r2_step_params(p, i, 1);
        if (!h->opt.r2_big && r2_step_supported(q1) &&
            conv_plan(h, p.s.tdnn2[i], ec_tdnn2_params(p, i), p.h2s, C).x3)      // (tdnn2 must be able to read the chain output in the split layout)
            return RES2_STEP;
        if (gemm_pw3r2_supported(q1)) return RES2_PW3R2;
    }
    return h->bf16 && res2net_chain_supported(C, h->T, L.dil, L.Kp) ? RES2_CHAIN : RES2_LAYERS;
}

// the attention-head route.  bf16: 16 waves per CU, lane-local online softmax (asp_x3.hip's bf16 form: 0.195 against 0.264 ms at
// B = 256, any T); the one-wave-per-SIMD kernel keeps the channel counts that are not multiples of 256 (and SVHIP_ASP_V1=1: the tests
// compare the two).  F32X3: asp_x3.  Otherwise the asp.conv GEMM and asp_pool
enum EcHead { HEAD_BF16, HEAD_FUSED, HEAD_X3, HEAD_POOL };
static EcHead ec_head_plan(const EcPass& p) {
    svhip_handle* h = p.h;
    const auto& s = p.s;
    const int T = h->T, C3 = 3 * h->cfg.channels;
    if (h->bf16 && C3 % 256 == 0 && s.asp_tdnn.N == 128 && s.asp_conv.Kp == 128 && !h->opt.asp_v1) return HEAD_BF16;
    if (h->bf16 && asp_fused_supported(T, C3, s.asp_tdnn.N, s.asp_conv.Kp)) return HEAD_FUSED;
    if (h->x3 && s.asp_conv.Ws32 && asp_x3_supported(T, C3, s.asp_tdnn.N, s.asp_conv.K)) return HEAD_X3;
    return HEAD_POOL;
}

// the front-end: the prologue (unless the fused fbank wrote X_in), then blocks.0 on the conv-gather split kernel or on conv_gemm
static int ec_front(EcPass& p) {
    svhip_handle* h = p.h;
    auto& s = p.s;
    const svhip_config& c = h->cfg;
    const int T = h->T, M = p.M, C = c.channels;
    const ConvLayer& L = s.blocks0;
    float* xscale = p.xscale;
    bool b0_cv = false;
    GemmParams q;
    int rc;
    if (h->x3 && L.Wcv && h->s32_buf) {
        // F32X3: blocks.0 on the persistent kernel's conv-gather form: the features go to the S32 layout with rows zero-padded to
        // cv_cin channels (one small pass), the im2col view is formed by the operand DMAs
        q = conv_params(h, L, h->s32_buf, L.cv_cin, p.X0, C, M, T);
        q.W = L.Wcv; q.Wrows = L.N; q.x3 = 2; q.K = L.taps * L.cv_cin; q.Kp = L.cv_Kp; q.cin = L.cv_cin; q.act1 = ACT_GELU;
        // (with s32_only and tdnn1 of the first block on the X3 kernel, X0 itself is written in the split layout: no conversion pass,
        //  block 1's residual is read as hi + lo, svhip_get_stage rebuilds the fp32 view)
        q.y_s32 = (p.s32_only && conv_plan(h, s.tdnn1[0], ec_tdnn1_params(p, 0, nullptr, C), p.X0, C).x3) ? 1 : 0;
        q.in_scale = xscale;
        b0_cv = gemm_pw3cv_supported(q);
    }
    // the prologue's range guard (F32X3: half-precision planes carry |x| <= 65504): with the scaled first convolution only a non-finite
    // input is reported — a finite one of any magnitude is brought into the planes' range by an exact power of two (round 6)
    if (!s.xin_ready && (rc = run(h, "prologue", 0, [&]() {
             return launch_prologue(p.feat, p.X_in, h->bf16, p.B, c.n_mels, T, c.log_input, h->in_w, h->in_b, p.d_pstats, p.st,
                                    h->x3 ? h->d_status : nullptr, h->host_flag_dev, (b0_cv && xscale) ? 3.0e38f : 65504.0f);
         }))) return rc;
    if (b0_cv) {
        if (xscale && (rc = run(h, "in_scale", 0, [&]() {
                 return launch_in_scale(static_cast<const float*>(p.X_in), (int64_t)M * c.n_mels, reinterpret_cast<uint32_t*>(xscale + 4), xscale, p.st, L.cv_wscale);
             }))) return rc;
        if ((rc = run(h, "split_s32", 0, [&]() { return launch_split_s32(static_cast<const float*>(p.X_in), c.n_mels, h->s32_buf, M, L.cv_cin, p.st, L.cv_cin, c.n_mels, xscale); }))) return rc;
        if ((rc = run(h, "gemm_pw3cv", (double)M * L.flops_per_row, [&]() { return launch_gemm_pw3cv(q, p.st); }))) return rc;
        p.x0_s32 = q.y_s32 != 0;
    } else {
        GemmParams g = conv_params(h, L, p.X_in, c.n_mels, p.X0, C, M, T);
        g.act1 = ACT_GELU;
        if ((rc = conv_gemm(h, L, g))) return rc;
    }
    s.x0_is_s32 = p.x0_s32;
    p.xin = p.x0_s32 ? nullptr : p.X0;
    p.xin32 = p.x0_s32 ? p.X0 : nullptr;
    p.ldin = p.ldin32 = C;
    return SVHIP_OK;
}

// block i's Res2Net: H1 -> H2, or on the split routes the S32 chain output h2s (tdnn1_side: tdnn1 already wrote the pass-through
// chunk and the first step's input in the split layout)
static int ec_res2(EcPass& p, int i, EcRes2 route, bool tdnn1_side) {
    svhip_handle* h = p.h;
    auto& s = p.s;
    const int T = h->T, M = p.M, C = h->cfg.channels, C8 = C / 8, e = h->esz;
    const bool bf = h->bf16;
    int rc;
    if (route == RES2_CHAIN) {
        Res2Params rp;
        rp.H1 = p.H1; rp.H2 = p.H2; rp.ld = C; rp.T = T; rp.dil = s.res2[i][0].dil; rp.Kp = s.res2[i][0].Kp;
        // small batches (the reference's per-file calls: B = num_eval crops): time slices, so that the chip is not left to B workgroups
        rp.slices = h->opt.r2_slices >= 0 ? std::max(1, h->opt.r2_slices) : res2net_chain_slices(p.B, C, T, rp.dil, h->num_cu);
        double fl = 0;
        for (int j = 0; j < 7; ++j) {
            rp.W[j] = s.res2[i][j].W; rp.bias[j] = s.res2[i][j].bias;
            rp.scale[j] = s.res2[i][j].scale; rp.shift[j] = s.res2[i][j].shift;
            fl += (double)M * s.res2[i][j].flops_per_row;
        }
        return run(h, rp.slices > 1 ? "res2net_slices" : "res2net_chain", fl, [&]() { return launch_res2net_chain(rp, p.B, C, p.st); });
    }
    if (route == RES2_LAYERS) {
        if ((rc = run(h, "copy_cols", 0, [&]() { return launch_copy_cols(p.H1, C, p.H2, C, bf, M, C8, p.st); }))) return rc;
        for (int j = 1; j < 8; ++j) {
            GemmParams q = conv_params(h, s.res2[i][j - 1], off(p.H1, (size_t)j * C8, e), C, off(p.H2, (size_t)j * C8, e), C, M, T);
            q.act1 = ACT_RELU;
            q.A2 = j >= 2 ? off(p.H2, (size_t)(j - 1) * C8, e) : nullptr; q.lda2 = C;
            if ((rc = conv_gemm(h, s.res2[i][j - 1], q))) return rc;
        }
        return SVHIP_OK;
    }
    if (!tdnn1_side) {
        if ((rc = run(h, "split_s32", 0, [&]() { return launch_split_s32(static_cast<const float*>(p.H1), C, p.h2s, M, C8, p.st, C); }))) return rc;
        if ((rc = run(h, "split_s32", 0, [&]() { return launch_split_s32(static_cast<const float*>(p.H1) + C8, C, p.us[0], M, C8, p.st, C8); }))) return rc;
    }
    for (int j = 1; j < 8; ++j) {
        const GemmParams q = ec_r2_step_params(p, i, j);
        if ((rc = run(h, route == RES2_STEP ? "r2_step" : "gemm_pw3r2", (double)M * s.res2[i][j - 1].flops_per_row, [&]() {
                 return route == RES2_STEP ? launch_r2_step(q, p.st) : launch_gemm_pw3r2(q, p.st);
             }))) return rc;
    }
    return SVHIP_OK;
}

// SE-Res2Net block i: tdnn1 (with its side outputs), the Res2Net, tdnn2 (with its column sums), the SE squeeze, gate and residual;
// the cursor moves on to the block's output in CAT
static int ec_block(EcPass& p, int i) {
    svhip_handle* h = p.h;
    auto& s = p.s;
    const int T = h->T, B = p.B, C = h->cfg.channels, C3 = 3 * C, C8 = C / 8, e = h->esz;
    const bool bf = h->bf16;
    const EcRes2 route = ec_res2_plan(p, i);
    const bool split = ec_res2_split(route);
    GemmParams p1 = ec_tdnn1_params(p, i, p.xin, p.ldin), p2 = ec_tdnn2_params(p, i);
    GemmPlan g1, g2;
    int rc;
    if (split) {
        // tdnn1 writes the pass-through chunk and the first step's input in the split layout itself (when it takes the X3 kernel)
        p1.side_a = p.h2s; p1.side_lda = C; p1.side_b = p.us[0]; p1.side_ldb = C8; p1.side_c = C8;
        p2.A = nullptr;      // (tdnn2 reads the chain output in the S32 layout only)
    }
    if ((rc = conv_gemm(h, s.tdnn1[i], p1, p.xin32, p.ldin32, &g1))) return rc;
    if (i == 2) { s.h2_is_s32 = split; s.h1_split = split && g1.side; }      // (what svhip_get_stage can read back of block 3)
    if ((rc = ec_res2(p, i, route, g1.side))) return rc;
    if ((rc = conv_gemm(h, s.tdnn2[i], p2, split ? p.h2s : nullptr, C, &g2))) return rc;
    const bool from_part = g2.colsum_groups != 0;      // the squeeze comes straight from the GEMM's column-sum partials
    if (!from_part) {
        if ((rc = run(h, "se_mean", 0, [&]() { return launch_colmean(p.H3, bf, C, B, T, C, p.d_mean, p.st); }))) return rc;
    }
    if ((rc = run(h, "se_mlp", 4.0 * B * 128 * C, [&]() {
             return launch_se_mlp(from_part ? nullptr : p.d_mean, from_part ? p.cs_base : nullptr, T,
                                  bf ? (const void*)s.se1_bf[i] : (const void*)s.se1[i].W, s.se1[i].bias,
                                  bf ? (const void*)s.se2T_bf[i] : (const void*)s.se2T[i], s.se2[i].bias, p.d_s2, bf, B, C, 128, p.st,
                                  from_part ? g2.colsum_groups : 8);      // (8: any count the kernel takes; no partials are read)
         }))) return rc;
    void* xout = p.s32_only ? nullptr : off(p.CAT, (size_t)i * C, e);
    void* xout32 = p.cat32 ? p.cat32 + (size_t)i * C * 4 : nullptr;
    // (the residual is read in the split layout only where the input has no copy in the handle's type)
    if ((rc = run(h, "se_apply", 0, [&]() {
             return launch_se_apply(p.H3, C, p.d_s2, p.xin, p.ldin, xout, C3, bf, B, T, C, p.st, xout32, C3, p.xin ? nullptr : p.xin32, p.ldin32);
         }))) return rc;
    p.xin = xout;
    p.xin32 = xout32;
    p.ldin = p.ldin32 = C3;
    return SVHIP_OK;
}

// mfa over the three block outputs, and the ASP statistics [mean | std] per utterance: from mfa's column sums, or by their own kernel
static int ec_mfa(EcPass& p) {
    svhip_handle* h = p.h;
    const int T = h->T, B = p.B, C3 = 3 * h->cfg.channels;
    GemmParams pm = ec_mfa_params(p);
    GemmPlan gm;
    int rc;
    if (p.s32_only) pm.A = nullptr;
    if ((rc = conv_gemm(h, p.s.mfa, pm, p.cat32, C3, &gm))) return rc;
    if (gm.colsum_groups)
        return run(h, "colsum_finalize", 0, [&]() { return launch_colsum_finalize(p.cs_base, h->colsum_region, true, B, T, C3, p.M, p.d_gstats, 1e-12f, p.st, gm.colsum_groups); });
    return run(h, "asp_gstats", 0, [&]() { return launch_colstats(p.MFA, h->bf16, C3, B, T, C3, p.d_gstats, 1e-12f, p.st); });
}

// the attention head: asp.tdnn (the time-constant columns of its input as the per-utterance bias asp_ctx), asp.conv, softmax over
// time and the weighted statistics, asp_bn — on the route of ec_head_plan
static int ec_head(EcPass& p) {
    svhip_handle* h = p.h;
    auto& s = p.s;
    const int T = h->T, B = p.B, M = p.M, C3 = 3 * h->cfg.channels;
    int rc;
    if ((rc = run(h, "asp_ctx", 2.0 * B * 128 * 2 * C3, [&]() {
             return launch_rowvec_linear(p.d_gstats, 2 * C3, s.asp_ctx.W, s.asp_ctx.bias, p.d_ctx, 128, B, 128, 2 * C3, ACT_NONE, p.st, p.lin_part);
         }))) return rc;
    GemmParams pa = conv_params(h, s.asp_tdnn, p.MFA, C3, p.ATT, 128, M, T);
    pa.act1 = ACT_RELU; pa.act2 = ACT_TANH;
    pa.bias_utt = p.d_ctx; pa.ld_bu = 128;
    if ((rc = conv_gemm(h, s.asp_tdnn, pa))) return rc;
    const EcHead head = ec_head_plan(p);
    const double fl = (double)M * s.asp_conv.flops_per_row;
    if (head == HEAD_BF16 || head == HEAD_FUSED) {
        AspFusedParams ap;
        ap.att = p.ATT; ap.W = s.asp_conv.W; ap.Kp = s.asp_conv.Kp; ap.bias = s.asp_conv.bias;
        ap.X = p.MFA; ap.ldx = C3; ap.T = T; ap.C = C3;
        ap.bn_scale = s.aspbn_scale; ap.bn_shift = s.aspbn_shift;
        ap.pooled_raw = p.d_pool_raw; ap.pooled_bn = p.d_pool_bn; ap.eps = 1e-12f;
        if (head == HEAD_BF16) return run(h, "asp_bf16", fl, [&]() { return launch_asp_bf16(ap, p.d_gstats, 2 * C3, B, p.st); });
        return run(h, "asp_fused", fl, [&]() { return launch_asp_fused(ap, B, p.st); });
    }
    if (head == HEAD_X3) {
        AspX3Params ap;
        ap.att = (const float*)p.ATT; ap.Ws32 = s.asp_conv.Ws32; ap.X = (const float*)p.MFA; ap.ldx = C3; ap.T = T; ap.C = C3;
        ap.mref = p.d_gstats; ap.mref_ld = 2 * C3;                  // [mean | std] per utterance: the means
        ap.bn_scale = s.aspbn_scale; ap.bn_shift = s.aspbn_shift;
        ap.pooled_raw = p.d_pool_raw; ap.pooled_bn = p.d_pool_bn; ap.eps = 1e-12f;
        return run(h, "asp_x3", fl, [&]() { return launch_asp_x3(ap, B, p.st); });
    }
    GemmParams pl = conv_params(h, s.asp_conv, p.ATT, 128, p.LOGITS, C3, M, T);
    pl.out_f32 = 1;
    if ((rc = conv_gemm(h, s.asp_conv, pl))) return rc;
    return run(h, "asp_pool", 0, [&]() {
        return launch_asp_pool(p.LOGITS, p.MFA, h->bf16, C3, B, T, C3, s.aspbn_scale, s.aspbn_shift, p.d_pool_raw, p.d_pool_bn, 1e-12f, 0.0f, p.st);
    });
}

static int ec_fc(EcPass& p) {
    svhip_handle* h = p.h;
    const LinearLayer& fc = p.s.fc;
    const int E = h->cfg.embed_dim, K = 2 * 3 * h->cfg.channels;      // [mean | std] of 3C channels
    return run(h, "fc", 2.0 * p.B * fc.N * fc.K, [&]() {
        return launch_rowvec_linear(p.d_pool_bn, K, fc.W, fc.bias, p.d_emb, E, p.B, E, K, ACT_NONE, p.st, p.lin_part);
    });
}

// utterances [b0, b0 + B) of the call, enqueued on h->cur: front-end, the three SE-Res2Net blocks, mfa, attention head, fc
static int ecapa_forward_part(svhip_handle* h, const float* d_feat_all, int b0, int B) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const int T = h->T, C = c.channels, C3 = 3 * C, C8 = C / 8, e = h->esz;
    const size_t r0 = (size_t)b0 * T;                       // first activation row of the slice
    EcPass p{h, s};
    p.b0 = b0; p.B = B; p.M = B * T; p.st = h->cur;
    p.feat = d_feat_all + (size_t)b0 * c.n_mels * T;
    p.X_in = off(h->X_in, r0 * c.n_mels, e);
    p.X0 = off(s.X0, r0 * C, e);
    p.H1 = off(s.H1, r0 * C, e); p.H2 = off(s.H2, r0 * C, e); p.H3 = off(s.H3, r0 * C, e);
    p.CAT = off(s.CAT, r0 * C3, e); p.MFA = off(s.MFA, r0 * C3, e);
    p.ATT = off(s.ATT, r0 * 128, e);
    p.LOGITS = s.LOGITS + r0 * C3;
    p.d_pstats = h->d_pstats + (size_t)b0 * c.n_mels * 2;
    p.d_mean = s.d_mean + (size_t)b0 * C; p.d_s2 = s.d_s2 + (size_t)b0 * C;
    p.d_gstats = s.d_gstats + (size_t)b0 * 2 * C3;
    p.d_ctx = s.d_ctx + (size_t)b0 * 128;
    p.d_pool_raw = s.d_pool_raw + (size_t)b0 * 2 * C3; p.d_pool_bn = s.d_pool_bn + (size_t)b0 * 2 * C3;
    p.d_emb = h->d_emb + (size_t)b0 * c.embed_dim;
    p.cs_base = ((h->bf16 || h->x3) && h->d_colsum) ? h->d_colsum + (b0 ? 2 * h->colsum_region : 0) : nullptr;
    p.xscale = h->d_xscale ? h->d_xscale + (b0 ? 4 + 256 : 0) : nullptr;
    p.lin_part = h->d_lin_part + (size_t)b0 * h->lin_part_per_utt;
    p.cat32 = s.cat_s32 ? static_cast<char*>(s.cat_s32) + r0 * C3 * 4 : nullptr;
    p.h2s = s.h2_s32 ? static_cast<char*>(s.h2_s32) + r0 * C * 4 : nullptr;
    for (int k = 0; k < 2; ++k) p.us[k] = s.u_s32[k] ? static_cast<char*>(s.u_s32[k]) + r0 * C8 * 4 : nullptr;
    p.s32_only = ec_s32_only(p);
    if (p.s32_only) s.cat_f32_stale = true;      // (svhip_get_stage converts on demand)
    int rc;
    if ((rc = ec_front(p))) return rc;
    for (int i = 0; i < 3; ++i)
        if ((rc = ec_block(p, i))) return rc;
    if ((rc = ec_mfa(p)) || (rc = ec_head(p))) return rc;
    return ec_fc(p);
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
// do not depend on the pack); the convolutions gather through the segment table; the reductions over time are the fixed kernels' RAG instances (launch_rag_*).
// It stays apart from the steps of ecapa_forward_part (ec_front .. ec_fc): those are mostly route decisions (F32X3 planes, the Res2Net
// step kernels, fused attention heads, two lanes) that this one has none of, and what the two share is too little to pay for one walk.
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
