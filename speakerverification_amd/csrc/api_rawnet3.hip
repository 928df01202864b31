// api_rawnet3.hip — RawNet3 in libsvhip (reference models/RawNet3.py:88-150, Bottle2neck: RawNet_baseline.py:71-159): its create rules,
// weight names and packing, workspace, forward and stages.
//
// Buffers (rawnet3_alloc): three (B T0, 1024) activations P0 .. P2 and CAT (B T2, 3072), whose column thirds are the three stage
// outputs [mp3(x1) | x2 | x3], so that layer4 reads the concatenation as one operand.
//   front-end   y (fp32) in P1, x0 in its own buffer (kept for svhip_get_stage)
//   layer1      residual(x0) -> P0, conv1(x0) -> P1, Res2Net steps P1 -> P2, conv3(P2) + P0 -> P1, pool 5 -> P2, AFMS -> x1 in P0
//   layer2      conv1(x1) -> P1, steps -> P2, conv3(P2) + x1 -> P1, mp3(x1) -> CAT[0], pool 3 -> P2, AFMS -> x2 in CAT[1] and
//               mp3(x1) + x2 -> P1 (layer3's input and its identity residual)
//   layer3      conv1(P1) and conv3 -> the head of P2, steps -> the next (B T2, 1024) of P2, AFMS -> x3 in CAT[2] (x1 stays in P0)
//   layer4      relu(W4 CAT + b4) -> P1; context pooling (attention activation in P2) -> pooled; fc6 -> embeddings
//
// A ragged pack (svhip_rawnet3_embed_ragged) runs the same walk (rawnet3_walk) over n utterances of different lengths packed back to
// back: level 0 holds the sum of T0_u rows, level 1 the sum of T0_u / 5, level 2 the sum of T0_u / 5 / 3, each with its segment table
// (Seg).  The buffers are the fixed-length ones: a pack holds at most max_batch * T0 level-0 rows, hence at most a fifth of that at
// level 1 and floor(max_batch * T0 / 15) at level 2, which is what CAT and the logits are sized for (the sum of T0_u / 15 can pass
// max_batch * T2 by a few rows).  Every GEMM goes to launch_gemm_ragged and every small linear to launch_rag_linear — one kernel at
// every row count — and the reductions over time are the per-utterance kernels of rawnet3.hip and the launch_rag_* forms, so an utterance's values
// do not depend on the pack.
#include <algorithm>
#include <cmath>

#include "handle.h"

namespace svhip {

namespace {

constexpr int C = 1024, W = 128, D = 1536;

int rn3_frames(int L) { return (L - RN3_TAPS) / RN3_STRIDE + 1; }      // T0 of RawNet3's front-end

struct Rn3Layer {                         // Bottle2neck(k = 3, scale = 8): every BatchNorm follows a ReLU, so it is its conv's epilogue affine
    ConvLayer conv1, convs[7], conv3, residual;      // conv1 + bn1, convs[i] + bns[i], conv3 + bn3; residual: 1 x 1, no bias (layer1)
    bool has_residual = false;
    float* alpha = nullptr;               // AFMS
    LinearLayer afms_fc;
};

// RawNet3 layers (SVHIP_MODEL_RAWNET3: RawNet3.py with the defaults of its MainModel, RawNet_baseline.py:71-159)
struct RawNet3State : ModelState {
    Rn3Layer layers[3];
    ConvLayer l4, att;                    // layer4 (3072 -> 1536, bias, ReLU); attention.0 columns [0, 1536) with attention.2 as epilogue
    LinearLayer att_ctx, fc6;             // attention.0 columns [1536, 4608) + its bias: the per-utterance bias of the time-constant inputs; fc6
    float *w2 = nullptr, *b2 = nullptr;                 // attention.3: the per-frame logit
    float *bn5_scale = nullptr, *bn5_shift = nullptr;
    float *in_w = nullptr, *in_b = nullptr;             // preprocess.1 (InstanceNorm1d affine)
    double pre[2] = {-0.97, 1.0};                       // preprocess.0.flipped_filter: y[i] = pre[0] x[i - 1] + pre[1] x[i]
    void* filt = nullptr;                 // [251][256] tap-major sinc filters: fp64 on fp32 handles, fp32 on bf16 handles
    int T0 = 0;                           // front-end frames; layer1 pools to T0 / 5, layer2 to T0 / 5 / 3
    void* buf[3] = {};                    // (Bmax * T0, 1024) activations each (the front-end's fp32 output passes through buf[1])
    void* x0 = nullptr;                   // (Bmax * T0, 256): the front-end output, layer1's operand
    void* cat = nullptr;                  // (Bmax * T2, 3072): [mp3(x1) | x2 | x3], layer4's operand
    double* stats = nullptr;              // (Bmax, 2) pre-emphasis / InstanceNorm statistics
    float *mean = nullptr, *gate = nullptr;             // (Bmax, 1024): time means, AFMS gates
    float *tstat = nullptr, *ctx = nullptr;             // (Bmax, 3072) [mean | std] of layer4's output; (Bmax, 128) attention bias
    float *logit = nullptr, *pooled = nullptr;          // (Bmax * T2) per-frame logits; (Bmax, 3072) bn5(pooled)
    const void* stage[5] = {};            // svhip_get_stage: front-end, layer1, layer2, layer3, layer4 outputs of the last forward
    int stage_T[5] = {}, stage_C[5] = {}, stage_ld[5] = {};
    // ragged packs (allocated by the first ragged call)
    RagTables rag;                        // the tables of a call (three levels) and the staging buffer: the utterances back to back,
                                          // Bmax * (samples + 16) floats
};

RawNet3State& S(svhip_handle* h) { return static_cast<RawNet3State&>(*h->model); }

// The GEMM of one layer in either form: fixed-length (g null) through conv_gemm and its routes; over a pack, whose level g holds its rows,
// on the generic kernel under `label`
int rn3_gemm(svhip_handle* h, const ConvLayer& K, GemmParams p, const Seg* g, const char* label) {
    if (!g) return conv_gemm(h, K, p);
    p.rag_utt = g->utt; p.rag_row0 = g->row0;
    return run(h, label, (double)g->M * K.flops_per_row, [&]() { return launch_gemm_ragged(p, h->bf16, h->cur); });
}

// One Bottle2neck on x (B T, cin) at row stride ldx, T frames in; its output y = AFMS(pool(.)) goes to (ydst, ldy), and with `add` the
// same pass writes y + add to `sum`.  res: the identity residual (null: the layer's 1 x 1 residual conv of x into `rbuf`).
// h1, h2, o: scratch (B T, 1024) buffers (o may be h1); pooled: (B T / P, 1024) scratch when P > 1.
// in / out (ragged packs; B = n, T unused): the segment tables of the input rows and of the rows after the pool (out == in when P == 1).
int bottle2neck(svhip_handle* h, const Rn3Layer& Ly, const void* x, int ldx, int cin, int B, int T, int P, const void* res, void* rbuf,
                void* h1, void* h2, void* o, void* pooled, void* ydst, int ldy, const void* add, int ldadd, void* sum, int ldsum,
                const Seg* in = nullptr, const Seg* out = nullptr) {
    auto& s = S(h);
    const int M = in ? in->M : B * T, e = h->esz, dt = h->dt;
    hipStream_t st = h->cur;
    int rc;
    auto gemm = [&](const ConvLayer& K, const GemmParams& p) {
        return rn3_gemm(h, K, p, in, K.taps > 1 ? (p.A2 ? "rag_gemm_conv_add" : "rag_gemm_conv") : "rag_gemm");
    };
    if (!res) {                                                                      // residual = Conv1d(cin, C, 1, bias=False)(x)
        if ((rc = gemm(Ly.residual, conv_params(h, Ly.residual, x, ldx, rbuf, C, M, T)))) return rc;
        res = rbuf;
    }
    GemmParams p1 = conv_params(h, Ly.conv1, x, ldx, h1, C, M, T);                   // bn1(relu(conv1(x)))
    p1.act1 = ACT_RELU;
    if ((rc = gemm(Ly.conv1, p1))) return rc;
    for (int i = 0; i < 7; ++i) {                                                    // sp = bns[i](relu(convs[i](sp + spx[i])))
        const ConvLayer& K = Ly.convs[i];
        const void* a = i == 0 ? h1 : off(h2, (size_t)(i - 1) * W, e);
        GemmParams q = conv_params(h, K, a, C, off(h2, (size_t)i * W, e), C, M, T);
        q.act1 = ACT_RELU; q.pad_mode = PAD_ZERO;
        if (i > 0) { q.A2 = off(h1, (size_t)i * W, e); q.lda2 = C; }
        if ((rc = gemm(K, q))) return rc;
    }
    if ((rc = run(h, "rn3_copy_chunk", 0, [&]() { return launch_copy_cols(off(h1, (size_t)7 * W, e), C, off(h2, (size_t)7 * W, e), C, h->bf16, M, W, st); })))
        return rc;                                                                   // the eighth chunk passes unchanged
    GemmParams p3 = conv_params(h, Ly.conv3, h2, C, o, C, M, T);                     // bn3(relu(conv3(.))) + residual
    p3.act1 = ACT_RELU; p3.R = res; p3.ldr = C;
    if ((rc = gemm(Ly.conv3, p3))) return rc;
    const void* z = o;
    const int Tn = T / P;
    if (P > 1) {
        if ((rc = run(h, "rn3_maxpool", 0, [&]() {
                 return in ? launch_rn3_rag_maxpool(o, C, pooled, C, dt, in->row0, out->row0, out->utt, out->M, C, P, st)
                           : launch_rn3_maxpool(o, C, pooled, C, dt, B, T, C, P, st);
             }))) return rc;
        z = pooled;
    }
    // AFMS: (z + alpha) * sigmoid(fc(mean_t z))                                        RawNet_baseline.py:58-65
    if (in) {
        if ((rc = run(h, "rn3_afms_mean", 0, [&]() { return launch_rag_colstats(z, h->bf16, C, out->row0, B, C, s.mean, false, 0.0f, st); }))) return rc;
        if ((rc = run(h, "rn3_afms_gate", 2.0 * B * C * C, [&]() {
                 return launch_rag_linear(s.mean, C, Ly.afms_fc.W, Ly.afms_fc.bias, s.gate, C, B, C, C, ACT_SIGMOID, st);
             }))) return rc;
        return run(h, "rn3_afms", 0, [&]() {
            return launch_rn3_rag_afms(z, C, Ly.alpha, s.gate, ydst, ldy, add, ldadd, sum, ldsum, dt, out->utt, out->M, C, st);
        });
    }
    if ((rc = run(h, "rn3_afms_mean", 0, [&]() { return launch_colmean(z, dt, C, B, Tn, C, s.mean, st); }))) return rc;
    if ((rc = run(h, "rn3_afms_gate", 2.0 * B * C * C, [&]() {
             return launch_rowvec_linear(s.mean, C, Ly.afms_fc.W, Ly.afms_fc.bias, s.gate, C, B, C, C, ACT_SIGMOID, st);
         }))) return rc;
    return run(h, "rn3_afms", 0, [&]() { return launch_rn3_afms(z, C, Ly.alpha, s.gate, ydst, ldy, add, ldadd, sum, ldsum, dt, B, Tn, C, st); });
}

}  // namespace

int rawnet3_check(const svhip_config& c, const char*& err) {
    if (c.compute != SVHIP_F32 && c.compute != SVHIP_BF16) { err = "RawNet3 runs on SVHIP_F32 and SVHIP_BF16 handles only"; return SVHIP_ERR_INVALID; }
    if (c.channels != 0 && c.channels != 1024) { err = "RawNet3 is built for C = 1024 (channels 0 or 1024)"; return SVHIP_ERR_INVALID; }
    if (c.samples < RN3_MIN_SAMPLES) {
        err = "RawNet3 needs at least 541 samples: (L - 251) / 10 + 1 frames pooled by 5 and 3 must leave two (the unbiased variance)";
        return SVHIP_ERR_INVALID;
    }
    return SVHIP_OK;
}

// RawNet3.MainModel's defaults (RawNet3.py:172-186): the 234 names of its state dict, the unused bn1.*, bn6.* and the pre-emphasis
// buffer included (the filterbank's window_ / n_ buffers are read: the checkpoint's values are the ones the filters are built from)
void rawnet3_spec(const svhip_config& c, WeightSpec& spec) {
    const int64_t nOut = c.embed_dim;
    spec["preprocess.0.flipped_filter"] = {1, 1, 2}; spec["preprocess.1.weight"] = {1}; spec["preprocess.1.bias"] = {1};
    spec["conv1.filterbank.low_hz_"] = {C / 8, 1}; spec["conv1.filterbank.band_hz_"] = {C / 8, 1};
    spec["conv1.filterbank.window_"] = {125}; spec["conv1.filterbank.n_"] = {1, 125};
    spec_bn(spec, "bn1", C / 4);
    for (int li = 1; li <= 3; ++li) {
        const std::string p = "layer" + std::to_string(li);
        const int64_t cin = li == 1 ? C / 4 : C;
        spec[p + ".conv1.weight"] = {C, cin, 1}; spec[p + ".conv1.bias"] = {C};
        spec_bn(spec, p + ".bn1", C);
        for (int i = 0; i < 7; ++i) {
            spec[p + ".convs." + std::to_string(i) + ".weight"] = {W, W, 3}; spec[p + ".convs." + std::to_string(i) + ".bias"] = {W};
            spec_bn(spec, p + ".bns." + std::to_string(i), W);
        }
        spec[p + ".conv3.weight"] = {C, C, 1}; spec[p + ".conv3.bias"] = {C};
        spec_bn(spec, p + ".bn3", C);
        spec[p + ".afms.alpha"] = {C, 1}; spec[p + ".afms.fc.weight"] = {C, C}; spec[p + ".afms.fc.bias"] = {C};
        if (cin != C) spec[p + ".residual.0.weight"] = {C, cin, 1};
    }
    spec["layer4.weight"] = {D, 3 * C, 1}; spec["layer4.bias"] = {D};
    spec["attention.0.weight"] = {128, 3 * D, 1}; spec["attention.0.bias"] = {128};
    spec_bn(spec, "attention.2", 128);
    spec["attention.3.weight"] = {1, 128, 1}; spec["attention.3.bias"] = {1};
    spec_bn(spec, "bn5", 2 * D);
    spec["fc6.weight"] = {nOut, 2 * D}; spec["fc6.bias"] = {nOut};
    spec_bn(spec, "bn6", nOut);
}

// ParamSincFB(256, 251).filters() (asteroid-filterbanks 0.4; its cos half is RawNet_baseline.py:339-357's formula) from the
// checkpoint's low_hz_, band_hz_, window_ and n_, in fp64, stored tap-major [251][256]: cos filters 0..127, sin filters 128..255
static int bake_sinc3(svhip_handle* h) {
    auto& s = S(h);
    const HostTensor *lo = getw(h, "conv1.filterbank.low_hz_"), *bd = getw(h, "conv1.filterbank.band_hz_"),
                     *win = getw(h, "conv1.filterbank.window_"), *nn = getw(h, "conv1.filterbank.n_");
    if (!lo || !bd || !win || !nn) SV_FAIL(h, SVHIP_ERR_MISSING, "missing conv1.filterbank tensors");
    const int NF = RN3_FILTERS / 2, HK = 125;
    std::vector<double> f((size_t)RN3_TAPS * RN3_FILTERS);
    for (int i = 0; i < NF; ++i) {
        const double low = 50.0 + std::fabs((double)lo->data[i]);
        const double high = std::min(std::max(low + 50.0 + std::fabs((double)bd->data[i]), 50.0), 8000.0);
        const double band = high - low;
        for (int k = 0; k < HK; ++k) {
            const double n = nn->data[k], w = win->data[k];
            const double c = (std::sin(high * n) - std::sin(low * n)) / (n / 2) * w;     // cos half, left side
            const double s = (std::cos(low * n) - std::cos(high * n)) / (n / 2) * w;     // sin half, left side
            f[(size_t)k * RN3_FILTERS + i] = c / (2 * band);
            f[(size_t)(RN3_TAPS - 1 - k) * RN3_FILTERS + i] = c / (2 * band);
            f[(size_t)k * RN3_FILTERS + NF + i] = s / (2 * band);
            f[(size_t)(RN3_TAPS - 1 - k) * RN3_FILTERS + NF + i] = -s / (2 * band);
        }
        f[(size_t)HK * RN3_FILTERS + i] = 2 * band / (2 * band);
        f[(size_t)HK * RN3_FILTERS + NF + i] = 0.0;
    }
    if (!h->bf16) {
        double* d;
        int rc = dev_upload(h, &d, f);
        s.filt = d;
        return rc;
    }
    std::vector<float> ff(f.begin(), f.end());
    float* d;
    int rc = dev_upload(h, &d, ff);
    s.filt = d;
    return rc;
}

int rawnet3_finalize(svhip_handle* h) {
    auto& s = S(h);
    int rc;
    const HostTensor* pf;
    if ((rc = needw(h, "preprocess.0.flipped_filter", pf))) return rc;
    s.pre[0] = pf->data[0]; s.pre[1] = pf->data[1];
    if ((rc = upload_f32(h, "preprocess.1.weight", &s.in_w))) return rc;
    if ((rc = upload_f32(h, "preprocess.1.bias", &s.in_b))) return rc;
    if ((rc = bake_sinc3(h))) return rc;
    const int T0 = s.T0;
    double fl = 2.0 * RN3_FILTERS * RN3_TAPS * T0;
    const int dil[3] = {2, 3, 4}, pool[3] = {5, 3, 1};
    int T = T0;
    for (int li = 0; li < 3; ++li) {
        Rn3Layer& Ly = s.layers[li];
        const std::string p = "layer" + std::to_string(li + 1);
        if ((rc = make_conv(h, Ly.conv1, p + ".conv1.weight", p + ".conv1.bias", p + ".bn1", 1))) return rc;
        for (int i = 0; i < 7; ++i)
            if ((rc = make_conv(h, Ly.convs[i], p + ".convs." + std::to_string(i) + ".weight", p + ".convs." + std::to_string(i) + ".bias",
                                p + ".bns." + std::to_string(i), dil[li]))) return rc;
        if ((rc = make_conv(h, Ly.conv3, p + ".conv3.weight", p + ".conv3.bias", p + ".bn3", 1))) return rc;
        Ly.has_residual = li == 0;
        if (Ly.has_residual && (rc = make_conv(h, Ly.residual, p + ".residual.0.weight", "", "", 1))) return rc;
        if ((rc = upload_f32(h, p + ".afms.alpha", &Ly.alpha))) return rc;
        if ((rc = make_linear(h, Ly.afms_fc, p + ".afms.fc.weight", p + ".afms.fc.bias"))) return rc;
        double per_row = Ly.conv1.flops_per_row + 7 * Ly.convs[0].flops_per_row + Ly.conv3.flops_per_row + (Ly.has_residual ? Ly.residual.flops_per_row : 0.0);
        fl += (double)T * per_row + 2.0 * 1024 * 1024;
        T /= pool[li];
    }
    if ((rc = make_conv(h, s.l4, "layer4.weight", "layer4.bias", "", 1))) return rc;
    if ((rc = make_conv(h, s.att, "attention.0.weight", "", "attention.2", 1, 0, 1536))) return rc;
    if ((rc = make_linear(h, s.att_ctx, "attention.0.weight", "attention.0.bias", 1536, 3 * 1536))) return rc;
    if ((rc = upload_f32(h, "attention.3.weight", &s.w2))) return rc;
    if ((rc = upload_f32(h, "attention.3.bias", &s.b2))) return rc;
    if ((rc = make_bn(h, "bn5", 2 * 1536, &s.bn5_scale, &s.bn5_shift))) return rc;
    if ((rc = make_linear(h, s.fc6, "fc6.weight", "fc6.bias"))) return rc;
    fl += (double)T * (s.l4.flops_per_row + s.att.flops_per_row + 2.0 * 128) + 2.0 * 128 * 3072 + 2.0 * s.fc6.N * s.fc6.K;
    h->flops_per_utt = fl;
    return SVHIP_OK;
}

int rawnet3_alloc(svhip_handle* h) {
    h->model = std::make_unique<RawNet3State>();
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const size_t B = c.max_batch;
    int rc;
    // three (B T0, 1024) activation buffers carry layer1 (rawnet3_forward_part); the later stages reuse them
    s.T0 = rn3_frames(c.samples);
    const size_t M0 = B * (size_t)s.T0, T2 = (size_t)(s.T0 / 5 / 3);
    if (T2 < 2) SV_FAIL(h, SVHIP_ERR_INVALID, "utterance too short for RawNet3 (%d samples)", c.samples);
    // level-2 rows: B * T2 of a fixed-length batch; a ragged pack that fills the M0 level-0 rows can hold up to M0 / 15
    const size_t M2 = M0 / 15 + 1;
    for (int i = 0; i < 3; ++i) if ((rc = actbuf(h, &s.buf[i], M0 * C))) return rc;
    if ((rc = actbuf(h, &s.cat, M2 * 3 * C))) return rc;
    if ((rc = actbuf(h, &s.x0, M0 * RN3_FILTERS))) return rc;
    if ((rc = dev_alloc(h, &s.stats, B * 2))) return rc;
    if ((rc = dev_alloc(h, &s.mean, B * 1024))) return rc;
    if ((rc = dev_alloc(h, &s.gate, B * 1024))) return rc;
    if ((rc = dev_alloc(h, &s.tstat, B * 3072))) return rc;
    if ((rc = dev_alloc(h, &s.ctx, B * 128))) return rc;
    if ((rc = dev_alloc(h, &s.logit, M2))) return rc;
    if ((rc = dev_alloc(h, &s.pooled, B * 3072))) return rc;
    return SVHIP_OK;
}

int rawnet3_stage(svhip_handle* h, const std::string& n, bool, StageView& v) {      // rn3_front, rn3_layer1 .. 3, rn3_layer4, rn3_pooled
    auto& s = S(h);
    static const char* kStages[5] = {"rn3_front", "rn3_layer1", "rn3_layer2", "rn3_layer3", "rn3_layer4"};
    int i = 0;
    while (i < 5 && n != kStages[i]) ++i;
    if (n == "rn3_pooled") { v.src = s.pooled; v.rows = h->lastB; v.cols = v.ld = 3072; v.f32 = true; }
    else if (i == 5) return unknown_stage(h, n);
    else {
        static const int kLevel[5] = {0, 1, 2, 2, 2};       // after a ragged forward: the packed rows of the stage's level, in utterance order
        v.src = s.stage[i]; v.cols = s.stage_C[i]; v.ld = s.stage_ld[i];
        v.rows = h->rag_levels ? (size_t)h->rag_rows[kLevel[i]] : (size_t)h->lastB * s.stage_T[i];
    }
    return SVHIP_OK;
}

// RawNet3.forward, written once for both forms.  pk null: a fixed-length batch of B waveforms (B, L) at d_wav, on h->cur (one slice).
// pk set: its n = B utterances (utterance u: pk->len[u] samples at d_wav + pk->off[u]) as packed rows at three frame levels, on the
// handle's stream, every step in its segment-table form.  T0 .. T2 are the frames per utterance of the fixed form (a pack's rows are their
// own frames: 1) and M2 the level-2 rows.
static int rawnet3_walk(svhip_handle* h, const float* d_wav, int B, const RagPack* pk) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const Seg *g0 = pk ? &pk->lv[0] : nullptr, *g1 = pk ? &pk->lv[1] : nullptr, *g2 = pk ? &pk->lv[2] : nullptr;
    const int L = c.samples, e = h->esz, dt = h->dt;
    const int T0 = pk ? 1 : s.T0, T1 = pk ? 1 : T0 / 5, T2 = pk ? 1 : T1 / 3;
    const int M0 = pk ? g0->M : B * T0, M2 = pk ? g2->M : B * T2;
    const bool bf = h->bf16;
    if (pk) h->cur = h->stream;
    hipStream_t st = h->cur;
    void *P0 = s.buf[0], *P1 = s.buf[1], *P2 = s.buf[2], *CAT = s.cat;
    int rc;
    // svhip_get_stage: (stage_T 0: a pack's rows are counted by the handle's rag_rows)
    auto stage = [&](int i, const void* src, int T, int Cn, int ld) { s.stage[i] = src; s.stage_T[i] = pk ? 0 : T; s.stage_C[i] = Cn; s.stage_ld[i] = ld; };
    auto colmean = [&](const char* label, const float* y) {          // mean_t of the fp32 front-end output -> s.mean
        return run(h, label, 0, [&]() {
            return pk ? launch_rag_colstats(y, false, RN3_FILTERS, g0->row0, B, RN3_FILTERS, s.mean, false, 0.0f, st)
                      : launch_colmean(y, DT_F32, RN3_FILTERS, B, T0, RN3_FILTERS, s.mean, st);
        });
    };
    auto mp3 = [&](const void* x, void* y, int ldy) {                // MaxPool1d(3) of the level-1 rows x -> the level-2 rows y
        return run(h, "rn3_maxpool", 0, [&]() {
            return pk ? launch_rn3_rag_maxpool(x, C, y, ldy, dt, g1->row0, g2->row0, g2->utt, g2->M, C, 3, st)
                      : launch_rn3_maxpool(x, C, y, ldy, dt, B, T1, C, 3, st);
        });
    };
    auto linear = [&](const char* label, const LinearLayer& K, const float* in, float* out, int ld_out) {      // per utterance, from 2 D inputs
        return run(h, label, 2.0 * B * K.N * K.K, [&]() {
            return pk ? launch_rag_linear(in, 2 * D, K.W, K.bias, out, ld_out, B, K.N, 2 * D, ACT_NONE, st)
                      : launch_rowvec_linear(in, 2 * D, K.W, K.bias, out, ld_out, B, K.N, 2 * D, ACT_NONE, st);
        });
    };
    if (pk)
        for (int l = 0; l < 3; ++l)
            if ((rc = run(h, "rag_rows", 0, [&]() { return launch_rag_rows(pk->lv[l].row0, B, pk->lv[l].maxT, pk->lv[l].utt, st); }))) return rc;

    // front-end: log(|sinc(in_norm(pre_emph(x)))| + 1e-6) - mean_t                  RawNet3.py:88-99
    float* y = static_cast<float*>(P1);
    void* x0 = s.x0;
    if ((rc = run(h, "rn3_sinc", 2.0 * RN3_FILTERS * RN3_TAPS * (double)M0, [&]() {
             return pk ? launch_rn3_rag_front(d_wav, pk->off, pk->len, g0->row0, B, g0->maxT, s.pre[0], s.pre[1], s.in_w, s.in_b, s.filt, !bf, s.stats, y, st)
                       : launch_rn3_front(d_wav, B, L, T0, s.pre[0], s.pre[1], s.in_w, s.in_b, s.filt, !bf, s.stats, y, st);
         }))) return rc;
    if ((rc = colmean("rn3_front_mean", y))) return rc;
    if ((rc = run(h, "rn3_center", 0, [&]() {
             return pk ? launch_rn3_rag_center(y, s.mean, x0, dt, g0->utt, g0->M, st) : launch_rn3_center(y, s.mean, x0, dt, B, T0, st);
         }))) return rc;
    stage(0, x0, T0, RN3_FILTERS, RN3_FILTERS);

    // layer1 = Bottle2neck(256, 1024, dilation 2, pool 5): x1 -> P0 (level 1)
    if ((rc = bottle2neck(h, s.layers[0], x0, RN3_FILTERS, RN3_FILTERS, B, T0, 5, nullptr, P0, P1, P2, P1, P2, P0, C, nullptr, 0, nullptr, 0, g0, g1)))
        return rc;
    stage(1, P0, T1, C, C);
    // mp3(x1) -> CAT[:, 0:1024), written once
    if ((rc = mp3(P0, CAT, 3 * C))) return rc;
    // layer2 = Bottle2neck(1024, 1024, dilation 3, pool 3), identity residual x1: x2 -> CAT[:, 1024:2048), mp3(x1) + x2 -> P1 (level 2)
    if ((rc = bottle2neck(h, s.layers[1], P0, C, C, B, T1, 3, P0, nullptr, P1, P2, P1, P2, off(CAT, C, e), 3 * C, CAT, 3 * C, P1, C, g1, g2)))
        return rc;
    stage(2, off(CAT, C, e), T2, C, 3 * C);
    // layer3 = Bottle2neck(1024, 1024, dilation 4) on mp3(x1) + x2, which is also its residual: x3 -> CAT[:, 2048:3072)
    void* h1 = P2;
    void* h2 = off(P2, (size_t)M2 * C, e);
    if ((rc = bottle2neck(h, s.layers[2], P1, C, C, B, T2, 1, P1, nullptr, h1, h2, h1, nullptr, off(CAT, 2 * C, e), 3 * C, nullptr, 0, nullptr, 0, g2, g2)))
        return rc;
    stage(3, off(CAT, 2 * C, e), T2, C, 3 * C);

    // layer4: relu(Conv1d(3072, 1536, 1)(cat(mp3(x1), x2, x3)))                       RawNet3.py:107-108
    GemmParams p4 = conv_params(h, s.l4, CAT, 3 * C, P1, D, M2, T2);
    p4.act1 = ACT_RELU;
    if ((rc = rn3_gemm(h, s.l4, p4, g2, "rag_gemm"))) return rc;
    stage(4, P1, T2, D, D);

    // context attentive statistics pooling (per utterance: a pack's from the level-2 table)            RawNet3.py:112-142
    // attention.0 on cat(x, mean_t x, std_t x): the time-constant two thirds are a per-utterance bias
    if ((rc = run(h, "rn3_tstats", 0, [&]() { return launch_rn3_tstats(P1, D, dt, B, T2, D, s.tstat, st, pk ? g2->row0 : nullptr); }))) return rc;
    if ((rc = linear("rn3_att_ctx", s.att_ctx, s.tstat, s.ctx, 128))) return rc;
    GemmParams pa = conv_params(h, s.att, P1, D, P2, 128, M2, T2);              // attention.2(relu(attention.0(.)))
    pa.act1 = ACT_RELU; pa.bias_utt = s.ctx; pa.ld_bu = 128;
    if ((rc = rn3_gemm(h, s.att, pa, g2, "rag_gemm_ctx"))) return rc;
    if ((rc = run(h, "rn3_pool", 0, [&]() {
             return launch_rn3_ctx_pool(P2, 128, s.w2, s.b2, s.logit, P1, D, dt, B, T2, D, s.bn5_scale, s.bn5_shift, s.stats, s.pooled, st,
                                        pk ? g2->row0 : nullptr, pk ? M2 : 0);
         }))) return rc;
    // fc6 (out_bn=False: bn6 is not applied)                                         RawNet3.py:144-148
    return linear("rn3_fc6", s.fc6, s.pooled, h->d_emb, c.embed_dim);
}

static int rawnet3_forward_part(svhip_handle* h, const float* d_wav, int, int B) { return rawnet3_walk(h, d_wav, B, nullptr); }
int rawnet3_forward(svhip_handle* h, const float* d_wav, int B) { return forward_lanes(h, rawnet3_forward_part, d_wav, B, 1, B); }

// ---- ragged packs ------------------------------------------------------------------------------------------
// RawNet3's rules for a pack of waveforms (RaggedCheckFn; include/svhip.h), on the host alone
int rawnet3_ragged_check(const svhip_config& c, const int32_t* lengths, int n, bool, std::string& err) {
    if (c.max_batch <= 0 || c.samples < RN3_MIN_SAMPLES) return refuse(err, SVHIP_ERR_INVALID, "bad max_batch / samples");
    const int64_t cap = (int64_t)c.max_batch * rn3_frames(c.samples);
    int64_t rows = 0;
    for (int i = 0; i < n; ++i) {
        if (lengths[i] < RN3_MIN_SAMPLES)
            return refuse(err, SVHIP_ERR_INVALID, "utterance %d: %d samples, fewer than RawNet3's minimum of %d", i, lengths[i], RN3_MIN_SAMPLES);
        if (int rc = rag_rows_fit(err, i, rows += rn3_frames(lengths[i]), cap, "T0")) return rc;
    }
    return SVHIP_OK;
}

// three frame levels: the front-end's frames, then what layer1's and layer2's pools leave
static void rn3_rag_frames(const svhip_config&, int64_t len, bool, int T[RAG_LEVELS]) {
    T[0] = rn3_frames((int)len);
    T[1] = T[0] / 5;
    T[2] = T[1] / 3;
}
static const RagRule kRawnet3Rag = {3, rn3_rag_frames, false};

int rawnet3_embed_ragged(svhip_handle* h, const float* in, bool in_host, bool, const int64_t* in_off, const int32_t* lengths, int n) {
    auto& s = S(h);
    const size_t M0 = (size_t)h->cfg.max_batch * s.T0, utt_cap[RAG_LEVELS] = {M0, M0 / 5 + 1, M0 / 15 + 1};
    RagPack pk;
    int rc;
    if ((rc = rag_pack(h, s.rag, kRawnet3Rag, utt_cap, in, in_host, true, in_off, lengths, n, pk)) || (rc = rawnet3_walk(h, pk.in, n, &pk))) return rc;
    set_rag_rows(h, pk);
    return SVHIP_OK;
}

}  // namespace svhip
