// api_rawnet2.hip — RawNet2 in libsvhip (the 'sinc' and 'conv' front-ends, the 'asp' and 'gru' aggregations): its create rules, weight
// names and packing, workspace, forward and stages; for the 'conv' model also the forward over a ragged pack (rawnet2_rag_walk, at the end).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "handle.h"

namespace svhip {

namespace {

bool rn_is_sinc(int model) { return model == SVHIP_MODEL_RAWNET2 || model == SVHIP_MODEL_RAWNET2_GRU; }     // front_proc='sinc'
bool rn_is_gru(int model) { return model == SVHIP_MODEL_RAWNET2_GRU; }                                       // aggregate='gru'

struct RnBlock {
    int cin = 0, cout = 0;
    bool downsample = false, has_shortcut = false;
    float *bn1_scale = nullptr, *bn1_shift = nullptr;
    ConvLayer conv1, conv2, shortcut;       // conv1 carries bn2 as its epilogue
    void* conv2sc_W = nullptr;              // bf16 handles: [Np][conv2.K + cin] = conv2 | 1 x 1 shortcut, one GEMM for both (gemm_pw2 A3)
    float* alpha = nullptr;
    LinearLayer afms_fc;
    float* afms_fcT = nullptr;              // fc weight transposed [cin][cout] (the gate kernel reads consecutive outputs per wave)
};

// RawNet2 layers (front_proc='sinc' or 'conv', aggregate='asp'; RawNet2_custom.py:230-243)
struct RawNet2State : ModelState {
    RnBlock blocks[8];
    float *gamma = nullptr, *beta = nullptr, *fbn_scale = nullptr, *fbn_shift = nullptr;
    void* filt = nullptr;
    void* filt_sym = nullptr;              // fp16 handles: [128][128] slot-major table of the symmetric sinc form (round 6)
    void* filt_x3 = nullptr;               // F32X3 handles: [2][128][256] half hi | lo parts of the sinc filters
    float* cw = nullptr;                   // 'conv' front-end (SVHIP_MODEL_RAWNET2_CONV): [w0 | w1 | w2 | bias] x 128 floats of conv1
    float *agg_scale = nullptr, *agg_shift = nullptr;
    ConvLayer att0, att3;
    LinearLayer fc;
    // aggregate='gru' (SVHIP_MODEL_RAWNET2_GRU): bn_before_gru is agg_scale / agg_shift; W_ih a 1 x 1 conv layer whose bias is
    // b_ih + [b_hr | b_hz | 0]; W_hh packed gate-interleaved (gru.hip) in the compute type; b_hn; fc_after_gru
    ConvLayer gru_ih;
    void* gru_whh = nullptr;
    float* gru_bhn = nullptr;
    LinearLayer gru_fc;
    float* gru_gi = nullptr;           // (Bmax, T, 3072) fp32 gate inputs
    float* gru_hbuf[2] = {};           // (Bmax, 1024) fp32 state, ping-pong
    int gru_T = 0;                     // frames that reach the GRU
    const void* gru_in = nullptr;      // svhip_get_stage "rn_gru_in": the GRU input of the last forward (one slice only)
    const float* gru_h = nullptr;      //                 "rn_gru_h": the buffer that holds the last state
    void* buf[6] = {};                 // activation ping-pong buffers; a 256-byte zero tail follows each payload (h->tailed lists them)
    float* scratch = nullptr;
    void* xn = nullptr;
    int Lp = 0;
    float *stats = nullptr, *mean = nullptr, *gate = nullptr, *logits = nullptr, *pooled = nullptr;
    float* part = nullptr;             // fused 128-channel blocks: per-tile column sums (B, ntiles, 128)
    int T1 = 0;
    KeptStages keep;                   // option rn_keep: copies of what the forward stored, by stage name (keep_stage fills them)
    // ragged packs of the 'conv' model: all allocated by the first ragged call, each under its own null check
    RagTables rag;                     // the tables of a call (seven levels) and the staging buffer of host waveforms
    int* rag_slice0 = nullptr;         // (RAG_LEVELS, max_batch + 1): the first slice of every utterance at every level (rn_rag_slices)
    float* rag_part = nullptr;         // the slice sums of one block tail, (slices of its out level, channels)
    float* rag_gate = nullptr;         // (8 blocks, max_batch, 512): every block's gates stay until the next forward (stages)
    float* rag_logits = nullptr;       // (last-level rows, 512) fp32
};

RawNet2State& S(svhip_handle* h) { return static_cast<RawNet2State&>(*h->model); }

}  // namespace

// RawNet2 needs six max_pool1d(3) stages behind the front-end to leave at least one frame: 3^6 front-end frames
constexpr int RN_MIN_FRAMES = 3 * 3 * 3 * 3 * 3 * 3;

int rawnet2_check(const svhip_config& c, const char*& err) {
    if (rn_is_sinc(c.model) && c.samples < 251 + 3 * RN_MIN_FRAMES) { err = "RawNet2 needs at least 2438 samples"; return SVHIP_ERR_INVALID; }
    if (!rn_is_sinc(c.model) && c.samples < 3 * RN_MIN_FRAMES) {
        err = "RawNet2 (front_proc='conv') needs at least 2187 samples: floor(L / 3) frames pass six max_pool1d(3) stages";
        return SVHIP_ERR_INVALID;
    }
    return SVHIP_OK;
}

// ---- expected weight names / shapes ----------------------------------------------------------------
const int RN_LAYERS[6] = {1, 1, 1, 2, 1, 2};                   // RawNet2_custom.py:231

const int RN_FILTERS[6] = {128, 128, 256, 256, 512, 512};      // RawNet2_custom.py:232

void rawnet2_spec(const svhip_config& c, WeightSpec& spec) {
    if (c.model == SVHIP_MODEL_RAWNET2_CONV) {          // conv1 = Conv1d(1, 128, 3, stride=3) with bias (RawNet2_custom.py:45-52)
        spec["conv1.weight"] = {128, 1, 3}; spec["conv1.bias"] = {128};
    } else {
        spec["ln.gamma"] = {(int64_t)c.samples}; spec["ln.beta"] = {(int64_t)c.samples};
        spec["first_conv.low_hz_"] = {128, 1}; spec["first_conv.band_hz_"] = {128, 1};
        spec_bn(spec, "first_bn", 128);
    }
    int64_t inpl = 128;
    for (int li = 0; li < 6; ++li)
        for (int b = 0; b < RN_LAYERS[li]; ++b) {
            const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
            const int64_t planes = RN_FILTERS[li];
            spec_bn(spec, p + ".bn1", inpl);
            spec[p + ".conv1.weight"] = {planes, inpl, 3};
            spec_bn(spec, p + ".bn2", planes);
            spec[p + ".conv2.weight"] = {planes, planes, 3};
            spec[p + ".afms.alpha"] = {planes, 1};
            spec[p + ".afms.fc.weight"] = {planes, planes}; spec[p + ".afms.fc.bias"] = {planes};
            if (inpl != planes) spec[p + ".shortcut.0.weight"] = {planes, inpl, 1};
            inpl = planes;
        }
    if (rn_is_gru(c.model)) {                        // aggregate='gru' (RawNet2_custom.py:84-95): fc is built too, and never used (:196-207)
        const int64_t G = 3 * RN_GRU_HIDDEN;
        spec_bn(spec, "bn_before_gru", 512);
        spec["gru.weight_ih_l0"] = {G, 512}; spec["gru.weight_hh_l0"] = {G, RN_GRU_HIDDEN};
        spec["gru.bias_ih_l0"] = {G}; spec["gru.bias_hh_l0"] = {G};
        spec["fc_after_gru.weight"] = {(int64_t)c.embed_dim, RN_GRU_HIDDEN}; spec["fc_after_gru.bias"] = {(int64_t)c.embed_dim};
    } else {
        spec_bn(spec, "bn_before_agg", 512);
        spec["attention.0.weight"] = {128, 512, 1}; spec["attention.0.bias"] = {128};
        spec_bn(spec, "attention.2", 128);
        spec["attention.3.weight"] = {512, 128, 1}; spec["attention.3.bias"] = {512};
    }
    spec["fc.weight"] = {(int64_t)c.embed_dim, 1024}; spec["fc.bias"] = {(int64_t)c.embed_dim};
}

// a conv layer of a RawNet2 handle: F32X3 handles also get the S32 split layout of r2_step.hip's modes 1 / 2 where its shape fits
static int rn_conv(svhip_handle* h, ConvLayer& L, const std::string& w, const std::string& b, const std::string& bn) {
    return make_conv(h, L, w, b, bn, 1, 0, -1, true);
}

// sinc band-pass filters baked once per weight load (RawNet_baseline.py:313-318,339-357), float32 arithmetic, at the handle's sample
// rate (cfg.sinc_sr; SincConv_fast's sample_rate: the time axis n_ and the clamp of the upper band edge at sr / 2)
static int bake_sinc(svhip_handle* h) {
    auto& s = S(h);
    const HostTensor *lo = getw(h, "first_conv.low_hz_"), *bd = getw(h, "first_conv.band_hz_");
    if (!lo || !bd) SV_FAIL(h, SVHIP_ERR_MISSING, "missing sinc parameters");
    const int NF = 128, KS = 251, HALF = 125;
    const float sr = (float)(h->cfg.sinc_sr ? h->cfg.sinc_sr : 16000), min_low = 50.0f, min_band = 50.0f;
    const float PI = 3.14159265358979323846f;
    std::vector<float> win(HALF), n_(HALF);
    for (int i = 0; i < HALF; ++i) {
        const float n_lin = (float)(124.5 * i / 124.0);                         // torch.linspace(0, 124.5, 125)
        win[i] = 0.54f - 0.46f * std::cos(2.0f * PI * n_lin / (float)KS);
        n_[i] = 2.0f * PI * (float)(-125 + i) / sr;                             // 2*pi*arange(-125, 0)/sample_rate
    }
    std::vector<float> filt((size_t)NF * KS);
    for (int f = 0; f < NF; ++f) {
        const float low = min_low + std::fabs(lo->data[f]);
        float high = low + min_band + std::fabs(bd->data[f]);
        high = std::fmin(std::fmax(high, min_low), sr / 2);
        const float band = high - low;
        for (int i = 0; i < HALF; ++i) {
            const float left = ((std::sin(high * n_[i]) - std::sin(low * n_[i])) / (n_[i] / 2.0f)) * win[i];
            filt[(size_t)f * KS + i] = left / (2.0f * band);
            filt[(size_t)f * KS + (KS - 1 - i)] = left / (2.0f * band);
        }
        filt[(size_t)f * KS + HALF] = (2.0f * band) / (2.0f * band);
    }
    int rc;
    if (h->bf16) {
        std::vector<uint16_t> pk((size_t)NF * 256, 0);
        for (int f = 0; f < NF; ++f)
            for (int k = 0; k < KS; ++k) pk[(size_t)f * 256 + k] = to_h16(h, filt[(size_t)f * KS + k]);
        uint16_t* d;
        if ((rc = dev_upload(h, &d, pk))) return rc;
        s.filt = d;
        if (h->f16) {
            // the symmetric form (rawnet2.hip, SYM): slot k' = 2 + m carries h[125 + m] (the centre tap halved: its operand is x[c] + x[c]),
            // slots 0 and 1 are zero; right and left halves of a filter are the same numbers by construction (checked here)
            bool symmetric = true;
            for (int f = 0; f < NF && symmetric; ++f)
                for (int i = 0; i < HALF; ++i) symmetric = symmetric && filt[(size_t)f * KS + i] == filt[(size_t)f * KS + (KS - 1 - i)];
            if (symmetric) {
                std::vector<uint16_t> ps((size_t)NF * 128, 0);
                for (int f = 0; f < NF; ++f) {
                    ps[(size_t)f * 128 + 2] = to_h16(h, 0.5f * filt[(size_t)f * KS + HALF]);
                    for (int m = 1; m <= HALF; ++m) ps[(size_t)f * 128 + 2 + m] = to_h16(h, filt[(size_t)f * KS + HALF + m]);
                }
                uint16_t* ds;
                if ((rc = dev_upload(h, &ds, ps))) return rc;
                s.filt_sym = ds;
            }
        }
    } else {
        std::vector<float> pk((size_t)NF * 252, 0.0f);
        for (int f = 0; f < NF; ++f)
            for (int k = 0; k < KS; ++k) pk[(size_t)f * 252 + k] = filt[(size_t)f * KS + k];
        float* d;
        if ((rc = dev_upload(h, &d, pk))) return rc;
        s.filt = d;
        if (h->x3) {        // the split front-end (rn_sinc_x3): hi and lo half planes, k contiguous, zero beyond the 251 taps
            std::vector<uint16_t> pl((size_t)2 * NF * 256, 0);
            for (int f = 0; f < NF; ++f)
                for (int k = 0; k < KS; ++k) {
                    const uint32_t w = x3_split_word(filt[(size_t)f * KS + k]);
                    pl[(size_t)f * 256 + k] = (uint16_t)(w >> 16);
                    pl[(size_t)(NF + f) * 256 + k] = (uint16_t)(w & 0xffffu);
                }
            uint16_t* dx;
            if ((rc = dev_upload(h, &dx, pl))) return rc;
            s.filt_x3 = dx;
        }
    }
    return SVHIP_OK;
}

// the 'conv' front-end's constants: conv1.weight (128, 1, 3) and conv1.bias as [w0 | w1 | w2 | bias] x 128 floats
static int make_conv3_front(svhip_handle* h) {
    const HostTensor *w, *b;
    int rc;
    if ((rc = needw(h, "conv1.weight", w)) || (rc = needw(h, "conv1.bias", b))) return rc;
    std::vector<float> cw(4 * 128);
    for (int c = 0; c < 128; ++c) {
        for (int k = 0; k < 3; ++k) cw[k * 128 + c] = w->data[c * 3 + k];
        cw[3 * 128 + c] = b->data[c];
    }
    return dev_upload(h, &S(h).cw, cw);
}

// aggregate='gru' (RawNet2_custom.py:84-95,196-207): bn_before_gru is the pass block 7's AFMS pass applies (agg_scale / agg_shift); the input
// projection W_ih is a 1 x 1 conv layer whose bias folds b_ih + [b_hr | b_hz | 0] (b_hn stays inside r * (W_hn h + b_hn)); W_hh is packed
// gate-interleaved (gru.hip) in the compute type; fc_after_gru is a small linear.  fc.* is loaded and not used, as in the reference.
static int rawnet2_finalize_gru(svhip_handle* h) {
    auto& s = S(h);
    const int H = RN_GRU_HIDDEN, G = 3 * H;
    int rc;
    if ((rc = make_bn(h, "bn_before_gru", 512, &s.agg_scale, &s.agg_shift))) return rc;
    const HostTensor *whh = getw(h, "gru.weight_hh_l0"), *bih = getw(h, "gru.bias_ih_l0"), *bhh = getw(h, "gru.bias_hh_l0");
    if (!whh || !bih || !bhh) SV_FAIL(h, SVHIP_ERR_MISSING, "missing GRU tensors (gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)");
    if ((rc = rn_conv(h, s.gru_ih, "gru.weight_ih_l0", "", ""))) return rc;
    std::vector<float> bias(G), bhn(H);
    for (int j = 0; j < G; ++j) bias[j] = j < 2 * H ? (float)((double)bih->data[j] + (double)bhh->data[j]) : bih->data[j];
    for (int j = 0; j < H; ++j) bhn[j] = bhh->data[2 * H + j];
    if ((rc = dev_upload(h, &s.gru_ih.bias, bias))) return rc;
    if ((rc = dev_upload(h, &s.gru_bhn, bhn))) return rc;
    // packed row ut * 48 + g * 16 + j = W_hh row g * H + ut * 16 + j
    std::vector<float> pk((size_t)G * H);
    for (int ut = 0; ut < H / 16; ++ut)
        for (int g = 0; g < 3; ++g)
            for (int j = 0; j < 16; ++j)
                memcpy(&pk[((size_t)ut * 48 + g * 16 + j) * H], &whh->data[((size_t)g * H + ut * 16 + j) * H], (size_t)H * 4);
    if (h->bf16) {
        std::vector<uint16_t> pb(pk.size());
        for (size_t i = 0; i < pk.size(); ++i) pb[i] = to_h16(h, pk[i]);
        uint16_t* d;
        if ((rc = dev_upload(h, &d, pb))) return rc;
        s.gru_whh = d;
    } else {
        float* d;
        if ((rc = dev_upload(h, &d, pk))) return rc;
        s.gru_whh = d;
    }
    return make_linear(h, s.gru_fc, "fc_after_gru.weight", "fc_after_gru.bias");
}

int rawnet2_finalize(svhip_handle* h) {
    auto& s = S(h);
    int rc;
    const bool conv = h->cfg.model == SVHIP_MODEL_RAWNET2_CONV;
    if (conv) {
        if ((rc = make_conv3_front(h))) return rc;
    } else {
        if ((rc = upload_f32(h, "ln.gamma", &s.gamma))) return rc;
        if ((rc = upload_f32(h, "ln.beta", &s.beta))) return rc;
        if ((rc = bake_sinc(h))) return rc;
        if ((rc = make_bn(h, "first_bn", 128, &s.fbn_scale, &s.fbn_shift))) return rc;
    }
    int inpl = 128, bi = 0;
    int T = s.T1;
    double fl = conv ? 2.0 * 128 * 3 * (double)T : 2.0 * 128 * 251 * (double)(h->cfg.samples - 250);
    for (int li = 0; li < 6; ++li)
        for (int b = 0; b < RN_LAYERS[li]; ++b, ++bi) {
            RnBlock& B = s.blocks[bi];
            const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
            const int planes = RN_FILTERS[li];
            B.cin = inpl; B.cout = planes; B.downsample = (b == RN_LAYERS[li] - 1); B.has_shortcut = inpl != planes;
            if ((rc = make_bn(h, p + ".bn1", inpl, &B.bn1_scale, &B.bn1_shift))) return rc;
            if ((rc = rn_conv(h, B.conv1, p + ".conv1.weight", "", p + ".bn2"))) return rc;
            if ((rc = rn_conv(h, B.conv2, p + ".conv2.weight", "", ""))) return rc;
            if (B.has_shortcut && (rc = rn_conv(h, B.shortcut, p + ".shortcut.0.weight", "", ""))) return rc;
            if (B.has_shortcut && h->bf16 && B.conv2.K % 64 == 0 && inpl % 64 == 0) {
                // conv2 and the shortcut share their output: [conv2 columns (tap-major) | shortcut columns] as one K axis
                const HostTensor* w2 = getw(h, p + ".conv2.weight");           // (planes, planes, 3)
                const HostTensor* ws = getw(h, p + ".shortcut.0.weight");      // (planes, inpl, 1)
                const int K2 = B.conv2.K, Kt = K2 + inpl, Np = B.conv2.Np;
                std::vector<uint16_t> pk((size_t)Np * Kt, 0);
                for (int n = 0; n < planes; ++n) {
                    for (int t = 0; t < 3; ++t)
                        for (int c = 0; c < planes; ++c) pk[(size_t)n * Kt + t * planes + c] = to_h16(h, w2->data[((size_t)n * planes + c) * 3 + t]);
                    for (int c = 0; c < inpl; ++c) pk[(size_t)n * Kt + K2 + c] = to_h16(h, ws->data[(size_t)n * inpl + c]);
                }
                uint16_t* d;
                if ((rc = dev_upload(h, &d, pk))) return rc;
                B.conv2sc_W = d;
            }
            if ((rc = upload_f32(h, p + ".afms.alpha", &B.alpha))) return rc;
            if ((rc = make_linear(h, B.afms_fc, p + ".afms.fc.weight", p + ".afms.fc.bias"))) return rc;
            {
                const HostTensor* fw = getw(h, p + ".afms.fc.weight");                  // (planes, planes)
                std::vector<float> t((size_t)planes * planes);
                for (int n = 0; n < planes; ++n)
                    for (int c = 0; c < planes; ++c) t[(size_t)c * planes + n] = fw->data[(size_t)n * planes + c];
                if ((rc = dev_upload(h, &B.afms_fcT, t))) return rc;
            }
            fl += (double)T * (B.conv1.flops_per_row + B.conv2.flops_per_row + (B.has_shortcut ? B.shortcut.flops_per_row : 0.0));
            fl += 2.0 * planes * planes;
            if (B.downsample) T /= 3;
            inpl = planes;
        }
    if (rn_is_gru(h->cfg.model)) {
        if ((rc = rawnet2_finalize_gru(h))) return rc;
        fl += (double)T * (s.gru_ih.flops_per_row + 2.0 * 3 * RN_GRU_HIDDEN * RN_GRU_HIDDEN) + 2.0 * s.gru_fc.N * s.gru_fc.K;
        h->flops_per_utt = fl;
        return SVHIP_OK;
    }
    if ((rc = make_bn(h, "bn_before_agg", 512, &s.agg_scale, &s.agg_shift))) return rc;
    if ((rc = rn_conv(h, s.att0, "attention.0.weight", "attention.0.bias", "attention.2"))) return rc;
    if ((rc = rn_conv(h, s.att3, "attention.3.weight", "attention.3.bias", ""))) return rc;
    if ((rc = make_linear(h, s.fc, "fc.weight", "fc.bias"))) return rc;
    fl += (double)T * (s.att0.flops_per_row + s.att3.flops_per_row) + 2.0 * s.fc.N * s.fc.K;
    h->flops_per_utt = fl;
    return SVHIP_OK;
}

int rawnet2_alloc(svhip_handle* h) {
    h->model = std::make_unique<RawNet2State>();
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const size_t B = c.max_batch, e = h->esz;
    int rc;
    const bool conv = c.model == SVHIP_MODEL_RAWNET2_CONV;
    s.T1 = conv ? (c.samples - 3) / 3 + 1 : (c.samples - 250) / 3;       // conv1 (kernel 3, stride 3) | sinc (251 taps) + max_pool1d(3)
    const size_t per_utt = (size_t)s.T1 * 128;           // largest activation: (T1, 128); later stages shrink 3x per doubling
    const size_t buf_bytes = B * per_utt * e;                // payload bytes of each activation buffer; a 256-byte zero tail follows
    for (int i = 0; i < 6; ++i) {
        if ((rc = actbuf(h, &s.buf[i], B * per_utt))) return rc;
        SV_HIP(h, hipMemset(off(s.buf[i], buf_bytes, 1), 0, 256));      // the zero tail (no kernel writes past the payload)
        h->tailed.push_back({static_cast<const char*>(s.buf[i]), buf_bytes});
    }
    if (!conv && (rc = dev_alloc(h, &s.stats, B * 2))) return rc;
    if (!conv && (h->bf16 || h->x3)) {                                  // LayerNorm output in 16 bits, zero-tailed rows (operand of the 16-bit / split sinc kernels)
        s.Lp = (int)round_up(c.samples + RN_XN_TAIL, 64);
        uint16_t* q;
        if ((rc = dev_alloc(h, &q, (h->x3 ? 4 : 2) * B * (size_t)s.Lp))) return rc;      // (F32X3: hi and lo parts of both copies)
        s.xn = q;
    }
    if ((rc = dev_alloc(h, &s.part, B * (size_t)(rn_block128_ntiles(s.T1) + 1) * 4 * 128))) return rc;
    if ((rc = dev_alloc(h, &s.mean, B * 512))) return rc;
    if ((rc = dev_alloc(h, &s.scratch, B * 16 * 512))) return rc;
    if ((rc = dev_alloc(h, &s.gate, B * 512 * 2))) return rc;
    int tf = s.T1;
    for (int i = 0; i < 6; ++i) tf /= 3;                      // six max_pool1d(3) stages follow the front-end
    if (tf < 1) SV_FAIL(h, SVHIP_ERR_INVALID, "utterance too short for RawNet2 (%d samples)", c.samples);
    if ((rc = dev_alloc(h, &s.logits, B * (size_t)tf * 512))) return rc;
    if (rn_is_gru(c.model)) {                                 // (256 x 14 frames: 11 MB of gate inputs)
        s.gru_T = tf;
        if ((rc = dev_alloc(h, &s.gru_gi, B * (size_t)tf * 3 * RN_GRU_HIDDEN))) return rc;
        for (int i = 0; i < 2; ++i) if ((rc = dev_alloc(h, &s.gru_hbuf[i], B * (size_t)RN_GRU_HIDDEN))) return rc;
    }
    if ((rc = dev_alloc(h, &s.pooled, B * 1024))) return rc;
    if (h->bf16) {          // K-slice partials of fc (K = 1 024: four slices of 256) at full batches, 16-bit handles
        h->lin_part_per_utt = (size_t)4 * (size_t)std::max(128, c.embed_dim);
        if ((rc = dev_alloc(h, &h->d_lin_part, B * h->lin_part_per_utt))) return rc;
    }
    return SVHIP_OK;
}

// the stages of option rn_keep: rn_front, rn_agg_in, rn_logits, rn_b<block>_pre | _x | _o | _c2 | _pool | _gate
static bool rn_keep_name(const std::string& n) {
    if (n == "rn_front" || n == "rn_agg_in" || n == "rn_logits") return true;
    if (n.size() < 7 || n.compare(0, 4, "rn_b") != 0 || n[4] < '0' || n[4] > '7' || n[5] != '_') return false;
    const std::string w = n.substr(6);
    return w == "pre" || w == "x" || w == "o" || w == "c2" || w == "pool" || w == "gate";
}

int rawnet2_stage(svhip_handle* h, const std::string& n, bool, StageView& v) {
    auto& s = S(h);
    const int B = h->lastB;
    if (n == "rn_pooled") { v.src = s.pooled; v.rows = B; v.cols = v.ld = 1024; v.f32 = true; }
    else if (n == "rn_gru_h" && rn_is_gru(h->cfg.model)) { v.src = s.gru_h; v.rows = B; v.cols = v.ld = RN_GRU_HIDDEN; v.f32 = true; }
    else if (n == "rn_gru_in" && rn_is_gru(h->cfg.model)) {
        if (!s.gru_in) SV_FAIL(h, SVHIP_ERR_STATE, "stage rn_gru_in: the last forward ran as several batch slices (SVHIP_LANES)");
        v.src = s.gru_in; v.rows = (size_t)B * s.gru_T; v.cols = v.ld = 512;
    }
    else if (rn_keep_name(n)) return kept_view(h, s.keep, n, B, "rn_keep", h->opt.rn_keep != 0, v);
    else return unknown_stage(h, n);
    return SVHIP_OK;
}

// conv2 + 1 x 1 shortcut of a RawNet2 block as ONE conv-gather GEMM: K = 3 * cout conv columns of hb, then cin columns of `pre`
static GemmParams conv2sc_params(svhip_handle* h, const RnBlock& K, const void* pre, const void* hb, void* o, int M, int T) {
    GemmParams p = conv_params(h, K.conv2, hb, K.cout, o, K.cout, M, T);
    p.W = K.conv2sc_W; p.Kp = K.conv2.K + K.cin; p.pad_mode = PAD_ZERO;
    p.A3 = pre; p.lda3 = K.cin; p.K3 = K.cin;
    return p;
}

// Option rn_keep, for both forwards: keep_stage (handle.h) on this model's stages
static int rn_keep(svhip_handle* h, hipStream_t st, const std::string& name, const void* src, int kind, size_t rows, bool packed, size_t cap_rows,
                   int cols, size_t row0, size_t nrows, int utts) {
    return keep_stage(h, S(h).keep, st, name, src, kind, rows, packed, cap_rows, cols, row0, nrows, utts);
}
static std::string blk(int i, const char* what) { return "rn_b" + std::to_string(i) + "_" + what; }

// RawNet2.forward (models/RawNet2_custom.py:161-227) on device-resident waveforms, as steps over one slice of the call: utterances
// [b0, b0 + B), enqueued on `st`.  Every workspace buffer is per-utterance contiguous, so a slice's pointers are offsets into each.
struct RnPass {
    svhip_handle* h;
    RawNet2State& s;
    int b0 = 0, B = 0;
    hipStream_t st = nullptr;
    int dt = DT_F32;
    const float* wav = nullptr;               // (B, L)
    // activations: the block input x, its pre-activation lrelu(bn1(x)), conv1's output, conv2's, the projected shortcut, the next x
    void *x = nullptr, *pre = nullptr, *hb = nullptr, *o = nullptr, *sc = nullptr, *xn = nullptr;
    float* stats = nullptr;                   // LayerNorm statistics
    void* ln = nullptr;                       // ... and its output in 16 bits / split halves (operand of the 16-bit / split sinc kernels)
    float *mean = nullptr, *scratch = nullptr, *part = nullptr, *gate[2] = {}, *pooled = nullptr, *emb = nullptr;
    float* lin_part = nullptr;                // K-slice partials of the last linear layer (16-bit handles), or null
    int T = 0;                                // frames of x
    bool pre_is_s32 = false;                  // F32X3: `pre` is in the S32 layout (its producer asked rn_step_plan for the block that reads it)
    bool sinc_x3 = false;                     // F32X3: the sinc front-end on three fp16 MFMAs per product
    bool fuse_ok = false;                     // 16-bit handles: 128 -> 128 pooled blocks run as the fused chain (rn_block128 + gate)
    bool chain0 = false;                      // ... and block 0 opens it: it forms its pre-activation itself
    bool conv_fused = false;                  // ... from the waveform ('conv' front-end): x is never stored

    int keep(const std::string& name, const void* src, size_t rows, int cols, int kind) const {
        if (!h->opt.rn_keep) return SVHIP_OK;
        return rn_keep(h, st, name, src, kind, rows, false, (size_t)h->cfg.max_batch * rows, cols, (size_t)b0 * rows, (size_t)B * rows, B);
    }
    // (the pre-activation block `bn` will read, or after block 7 the aggregation's input)
    int keep_pre(int bn, int Tn, int Cn) const { return keep(bn < 8 ? blk(bn, "pre") : std::string("rn_agg_in"), pre, Tn, Cn, pre_is_s32 ? KEEP_S32 : KEEP_DT); }
};

// F32X3: does block `bn`, entered with Tn frames, run its convolutions (and its projection shortcut) on the 128 x 128 split kernel
// (r2_step.hip, modes 1 / 2)?  Its operand is `pre` in the S32 layout; xb: its input x.  (Otherwise they run on the tiled kernel
// that splits its fp32 operands in registers: 170 - 190 TFLOP/s.)  The producer of `pre` asks, and writes the S32 layout where the
// answer is yes; the block asks again with the same arguments.
struct RnStep { bool ok = false; GemmParams q0, q1, q2; };
static RnStep rn_step_plan(const RnPass& p, int bn, int Tn, const void* xb) {
    svhip_handle* h = p.h;
    RnStep sp;
    if (bn > 7 || !h->x3 || h->opt.rn_step_off) return sp;
    const RnBlock& K = p.s.blocks[bn];
    GemmParams& q1 = sp.q1;                           // conv1: pre (S32) -> lrelu(bn2(.)) in S32, conv2's operand
    q1 = conv_params(h, K.conv1, p.pre, K.cin, p.hb, K.cout, p.B * Tn, Tn);
    q1.W = K.conv1.Ws32; q1.x3 = 2; q1.pad_mode = PAD_ZERO; q1.zero_page = h->d_zeros;
    GemmParams& q2 = sp.q2 = q1;                      // conv2: h (S32) -> fp32, + the shortcut (identity x, or the projected one)
    q2.A = p.hb; q2.lda = K.cout; q2.cin = K.cout; q2.K = 3 * K.cout; q2.Kp = q2.K; q2.W = K.conv2.Ws32; q2.scale = nullptr; q2.shift = nullptr;
    q2.Y = p.o; q2.out_f32 = 1; q2.R = reinterpret_cast<const float*>(K.has_shortcut ? p.sc : xb); q2.ldr = K.cout;
    GemmParams& q0 = sp.q0 = q1;                      // projection shortcut (k = 1) of pre -> fp32, into the spare activation buffer
    q0.W = K.shortcut.Ws32; q0.taps = 1; q0.K = K.cin; q0.Kp = K.cin; q0.scale = nullptr; q0.shift = nullptr; q0.Y = p.sc; q0.out_f32 = 1;
    // (rn_step_supported also asks for the split weights and the shapes: cin % 32 == 0, cout % 128 == 0, Tn >= 2)
    sp.ok = rn_step_supported(q1, 1) && rn_step_supported(q2, 2) && (!K.has_shortcut || rn_step_supported(q0, 2));
    return sp;
}

// the front-end: [LayerNorm statistics,] x = sinc | split sinc | conv1 of the waveform, and block 0's pre-activation lrelu(bn1(x))
// unless block 0 opens the fused chain
static int rn_front(RnPass& p) {
    svhip_handle* h = p.h;
    auto& s = p.s;
    const int B = p.B, L = h->cfg.samples, T = p.T, dt = p.dt;
    const bool conv = h->cfg.model == SVHIP_MODEL_RAWNET2_CONV;        // front_proc='conv': no LayerNorm, no sinc, no first_bn
    const RnBlock& K0 = s.blocks[0];
    int rc;
    if (!conv && (rc = run(h, "rn_ln_stats", 0, [&]() { return launch_rn_ln_stats(p.wav, B, L, p.stats, p.st, p.ln, s.Lp, s.gamma, s.beta, dt, p.sinc_x3); }))) return rc;
    // (the split front-end writes block 0's pre-activation itself, in the S32 layout, when block 0 runs on the split convolution kernel)
    const bool pre_s32 = rn_step_plan(p, 0, T, p.x).ok, sinc_pre = p.sinc_x3 && pre_s32;
    if (conv) {
        // (16-bit handles: the fused chain's first block computes the conv front-end itself from the waveform — rn_block128's CONV
        //  form; option rn_conv_unfused stores x with rn_conv3_front and runs the plain block, bit-identical)
        if (!p.conv_fused && (rc = run(h, "rn_conv3_front", 2.0 * B * 128.0 * 3.0 * T, [&]() { return launch_rn_conv3_front(p.wav, s.cw, p.x, dt, B, L, T, p.st); })))
            return rc;
    } else if ((rc = run(h, "rn_sinc", 2.0 * B * 128.0 * 251.0 * (L - 250), [&]() {
             // (the kernel can also write block 0's pre-activation, but its 8-byte scattered stores make that as dear as the
             //  separate coalesced rn_bn_act pass: measured 0.85 + 0.29 ms either way)
             if (p.sinc_x3) return launch_rn_sinc_x3(s.filt_x3, s.fbn_scale, s.fbn_shift, reinterpret_cast<float*>(p.x), B, L, T, p.ln, s.Lp, h->num_cu, p.st,
                                                     sinc_pre ? p.pre : nullptr, K0.bn1_scale, K0.bn1_shift);
             // fp16 handles: the symmetric form of the sinc convolution (K = 126 instead of 251; option rn_sinc_full keeps round 5's kernel)
             const bool sym = h->f16 && s.filt_sym && !h->opt.rn_sinc_full;
             return launch_rn_sinc(p.wav, p.stats, s.gamma, s.beta, sym ? s.filt_sym : s.filt, s.fbn_scale, s.fbn_shift, p.x, dt, B, L, T, p.st,
                                   nullptr, nullptr, nullptr, p.ln, s.Lp, h->num_cu, sym);
         }))) return rc;
    if (!p.conv_fused && (rc = p.keep("rn_front", p.x, T, 128, KEEP_DT))) return rc;        // (the conv-fused block 0 reads the waveform: no front-end tensor)
    if (p.chain0) return SVHIP_OK;
    // out = lrelu(bn1(x))                                                             RawNet_baseline.py:222
    // (blocks 1..7 get it from the previous block's AFMS pass, which writes x and lrelu(bn1(x)) together)
    p.pre_is_s32 = pre_s32;
    if (!sinc_pre && (rc = run(h, "rn_bn_act", 0, [&]() { return launch_rn_bn_act(p.x, p.pre, dt, K0.bn1_scale, K0.bn1_shift, B * T, K0.cin, 0.3f, p.st, p.pre_is_s32); })))
        return rc;
    return p.keep_pre(0, T, K0.cin);
}

// 16-bit handles: the leading 128 -> 128 pooled blocks (layer1, layer2) each run as ONE fused kernel + the AFMS gate kernel; the gate
// of block i is applied by block i + 1 on the way in, the last one's by the closing rn_afms_apply pass in front of the first GEMM
// block.  first: the blocks taken
static int rn_fused_chain(RnPass& p, int& first) {
    svhip_handle* h = p.h;
    auto& s = p.s;
    const int B = p.B, dt = p.dt;
    int rc;
    const float *g_alpha = nullptr, *g_gate = nullptr;          // pending gate of the previous fused block
    const void* xin = p.x;
    for (first = 0; p.fuse_ok && first < 8; ++first) {
        const RnBlock& K = s.blocks[first];
        if (!rn_block128_supported(K.cin, K.cout, p.T, K.downsample, K.has_shortcut, K.conv1.Kp, K.conv2.Kp)) break;
        RnBlock128Params bp;
        bp.xin = reinterpret_cast<const bf16_t*>(xin);
        bp.alpha = g_alpha; bp.gate = g_gate;
        bp.bn1_scale = K.bn1_scale; bp.bn1_shift = K.bn1_shift;
        bp.W1 = reinterpret_cast<const bf16_t*>(K.conv1.W); bp.bn2_scale = K.conv1.scale; bp.bn2_shift = K.conv1.shift;
        bp.W2 = reinterpret_cast<const bf16_t*>(K.conv2.W);
        void* dst = (first & 1) ? p.hb : p.o;                    // ping-pong: never the buffer being read
        bp.opool = reinterpret_cast<bf16_t*>(dst);
        bp.colsum = p.part;
        bp.B = B; bp.T = p.T; bp.Tout = p.T / 3; bp.ntiles = rn_block128_ntiles(p.T); bp.f16 = h->f16 ? 1 : 0;
        const bool from_wave = first == 0 && p.conv_fused;
        if (from_wave) { bp.xin = nullptr; bp.wav = p.wav; bp.cw = s.cw; bp.L = h->cfg.samples; }
        const double fl = (double)B * p.T * (K.conv1.flops_per_row + K.conv2.flops_per_row + (from_wave ? 2.0 * 128 * 3 : 0.0));
        if ((rc = run(h, from_wave ? "rn_block128_conv" : "rn_block128", fl, [&]() { return launch_rn_block128(bp, h->num_cu, p.st); }))) return rc;
        float* gate = p.gate[first & 1];                         // two gate buffers: block i + 1 reads i's while writing its own
        if ((rc = run(h, "rn_afms_gate", 2.0 * B * K.cout * K.cout, [&]() {
                 return launch_rn_afms_gate(p.part, rn_block128_nparts(B, bp.T, h->num_cu), B, K.cout, bp.Tout, K.afms_fcT, K.afms_fc.bias, gate, p.st);
             }))) return rc;
        if ((rc = p.keep(blk(first, "pool"), dst, bp.Tout, K.cout, KEEP_DT)) || (rc = p.keep(blk(first, "gate"), gate, 1, K.cout, KEEP_F32))) return rc;
        p.T /= 3;
        xin = dst;
        g_alpha = K.alpha; g_gate = gate;
    }
    if (first == 0) return SVHIP_OK;
    // x = (o + alpha) * gate and, in the same pass, the next consumer's lrelu(bn(x))
    const RnBlock& Kp = s.blocks[first - 1];
    const float* nsc = first < 8 ? s.blocks[first].bn1_scale : s.agg_scale;
    const float* nsh = first < 8 ? s.blocks[first].bn1_shift : s.agg_shift;
    // x itself is read only as an identity shortcut: not written when the next block projects its input
    void* xdst = (first < 8 && s.blocks[first].has_shortcut) ? nullptr : p.x;
    if ((rc = run(h, "rn_afms_apply", 0, [&]() { return launch_rn_afms_apply(xin, xdst, dt, Kp.alpha, g_gate, B, p.T, Kp.cout, p.st, nsc, nsh, p.pre, 0.3f); }))) return rc;
    if ((rc = p.keep_pre(first, p.T, Kp.cout))) return rc;
    return xdst && first < 8 ? p.keep(blk(first, "x"), p.x, p.T, Kp.cout, KEEP_DT) : SVHIP_OK;
}

// A block's convolutions on the split kernel (F32X3, `pre` in the S32 layout): [projection shortcut,] conv1 -> bn2 -> lrelu, conv2 +
// shortcut.  pooled_by_conv: conv2 pooled on its way out (a pooled block whose tail is not the fused kernel — the long utterances
// of layers 1 - 3)
static int rn_convs_split(RnPass& p, const RnBlock& K, const RnStep& sp, bool tail_fused, bool& pooled_by_conv) {
    svhip_handle* h = p.h;
    const int M = p.B * p.T;
    int rc;
    if (K.has_shortcut && (rc = run(h, "rn_step", (double)M * K.shortcut.flops_per_row, [&]() { return launch_rn_step(sp.q0, 2, p.st); }))) return rc;
    if ((rc = run(h, "rn_step", (double)M * K.conv1.flops_per_row, [&]() { return launch_rn_step(sp.q1, 1, p.st); }))) return rc;
    pooled_by_conv = K.downsample && !tail_fused && p.T >= 3 && !h->opt.rn_pool_off && rn_step_supported(sp.q2, 3);
    return run(h, "rn_step", (double)M * K.conv2.flops_per_row, [&]() { return launch_rn_step(sp.q2, pooled_by_conv ? 3 : 2, p.st); });
}

// ... and on the tiled GEMMs (conv_plan picks each kernel).  resid_in_tail: the block input, where the tail adds the identity shortcut
static int rn_convs_tiled(RnPass& p, const RnBlock& K, bool tail_fused, const void*& resid_in_tail) {
    svhip_handle* h = p.h;
    const int T = p.T, M = p.B * T;
    int rc;
    // A 1 x 1 shortcut rides in conv2's GEMM as extra K columns when the 256 x 256 kernel takes it (no shortcut tensor in HBM)
    const GemmParams psc = conv2sc_params(h, K, p.pre, p.hb, p.o, M, T);
    const bool fold_sc = K.has_shortcut && K.conv2sc_W && !h->opt.rn_unfused && conv_plan(h, K.conv2, psc).route == ROUTE_PW2;
    const void* resid = p.x;                                                 // identity shortcut takes the pre-BN x (:223)
    if (K.has_shortcut && !fold_sc) {
        if ((rc = conv_gemm(h, K.shortcut, conv_params(h, K.shortcut, p.pre, K.cin, p.sc, K.cout, M, h->T)))) return rc;
        resid = p.sc;
    }
    GemmParams p1 = conv_params(h, K.conv1, p.pre, K.cin, p.hb, K.cout, M, T);
    p1.act2 = ACT_LRELU03; p1.pad_mode = PAD_ZERO;
    if ((rc = conv_gemm(h, K.conv1, p1))) return rc;
    if (fold_sc) return conv_gemm(h, K.conv2, psc);
    GemmParams p2 = conv_params(h, K.conv2, p.hb, K.cout, p.o, K.cout, M, T);
    p2.pad_mode = PAD_ZERO;
    // identity shortcut: with the fused block tail and conv2 on the persistent conv-gather kernel (which has no residual
    // operand) the tail adds the block input; otherwise conv2's epilogue does
    if (!K.has_shortcut && tail_fused && conv_plan(h, K.conv2, p2).route == ROUTE_PW3CV) resid_in_tail = p.x;
    else p2.R = resid, p2.ldr = K.cout;
    return conv_gemm(h, K.conv2, p2);
}

// A block's tail, as one rn_tail launch or as separate passes: [max_pool1d(3)] -> AFMS gate -> the next step's x and, in the same pass,
// its pre-activation lrelu(bn(.)) (block bi + 1's bn1, or the aggregation BN after block 7); p.x / p.pre / p.T move on to them
static int rn_block_tail(RnPass& p, int bi, bool tail_fused, bool pooled_by_conv, const void* resid_in_tail) {
    svhip_handle* h = p.h;
    const RnBlock& K = p.s.blocks[bi];
    const int B = p.B, dt = p.dt, T = p.T, Tn = K.downsample ? T / 3 : T;
    const float* nsc = bi < 7 ? p.s.blocks[bi + 1].bn1_scale : p.s.agg_scale;
    const float* nsh = bi < 7 ? p.s.blocks[bi + 1].bn1_shift : p.s.agg_shift;
    // the block output itself is read only by an identity shortcut of the next block
    const bool x_dead = bi == 7 || p.s.blocks[bi + 1].has_shortcut;
    // (F32X3: when the next block runs on the split convolution kernel its pre-activation is written in the S32 layout right here)
    const bool next_s32 = rn_step_plan(p, bi + 1, Tn, p.xn).ok;
    int rc;
    if (tail_fused) {
        // max-pool + AFMS + next pre-activation in one launch, the pooled activation held in registers      :228-229, :62-68
        char tl[48] = "rn_tail";
        if (h->opt.layer_labels) snprintf(tl, sizeof(tl), "rn_tail T%d C%d", T, K.cout);
        // (small batches: slice sums in `scratch`, the gate in gate[0]; option rn_tail_big keeps one workgroup per utterance)
        const bool sliced = !h->opt.rn_tail_big;
        if ((rc = run(h, tl, 2.0 * B * K.cout * K.cout, [&]() {
                 return launch_rn_tail(p.o, x_dead ? nullptr : p.xn, p.pre, dt, K.downsample, K.alpha, K.afms_fcT, K.afms_fc.bias, nsc, nsh, B, T, K.cout, 0.3f, p.st,
                                       resid_in_tail, sliced ? p.scratch : nullptr, sliced ? p.gate[0] : nullptr, h->num_cu, next_s32);
             }))) return rc;
        // (only the sliced form stores its gate; one workgroup per utterance keeps it on chip)
        if (sliced && rn_tail_slices(dt, B, Tn, K.cout, h->num_cu) > 0 && (rc = p.keep(blk(bi, "gate"), p.gate[0], 1, K.cout, KEEP_F32))) return rc;
    } else {
        const void* y = p.o;                                                          // (F32X3: or conv2 pooled on its way out, into o)
        if (K.downsample && !pooled_by_conv) {                                        // :228-229
            if ((rc = run(h, "rn_maxpool3", 0, [&]() { return launch_rn_maxpool3(p.o, p.hb, dt, B, T, K.cout, p.st); }))) return rc;
            y = p.hb;
        }
        // AFMS: (y + alpha) * sigmoid(fc(mean_t y))                                     :62-68
        if ((rc = run(h, "rn_afms_mean", 0, [&]() { return launch_colmean(y, dt, K.cout, B, Tn, K.cout, p.mean, p.st, p.scratch, 16); }))) return rc;
        if ((rc = run(h, "rn_afms_gate", 2.0 * B * K.cout * K.cout, [&]() {
                 return launch_rn_afms_gate(p.mean, 1, B, K.cout, 1, K.afms_fcT, K.afms_fc.bias, p.gate[0], p.st);
             }))) return rc;
        if ((rc = run(h, "rn_afms_apply", 0, [&]() { return launch_rn_afms_apply(y, x_dead ? nullptr : p.xn, dt, K.alpha, p.gate[0], B, Tn, K.cout, p.st, nsc, nsh, p.pre, 0.3f, next_s32); }))) return rc;
        if ((rc = p.keep(blk(bi, "gate"), p.gate[0], 1, K.cout, KEEP_F32))) return rc;
    }
    std::swap(p.x, p.xn);
    p.T = Tn;
    p.pre_is_s32 = next_s32;
    if ((rc = p.keep_pre(bi + 1, Tn, K.cout))) return rc;
    return x_dead ? SVHIP_OK : p.keep(blk(bi + 1, "x"), p.x, Tn, K.cout, KEEP_DT);
}

// residual block bi (RawNet_baseline.py:222-229) from x and its pre-activation: the convolutions, then the tail
static int rn_block(RnPass& p, int bi) {
    svhip_handle* h = p.h;
    const RnBlock& K = p.s.blocks[bi];
    const int T = p.T;
    const RnStep sp = rn_step_plan(p, bi, T, p.x);
    // (every producer of `pre` asked the same question with the same arguments)
    if (p.pre_is_s32 != sp.ok) SV_FAIL(h, SVHIP_ERR_STATE, "RawNet2 block %d: the pre-activation's layout is not the one its convolution route reads", bi);
    const bool tail_fused = !h->opt.rn_unfused && rn_tail_supported(p.dt, K.downsample ? T / 3 : T, K.cout);
    bool pooled_by_conv = false;
    const void* resid_in_tail = nullptr;
    int rc;
    // conv1 -> bn2 -> lrelu (epilogue), conv2 + shortcut                            :224-226
    if ((rc = sp.ok ? rn_convs_split(p, K, sp, tail_fused, pooled_by_conv) : rn_convs_tiled(p, K, tail_fused, resid_in_tail))) return rc;
    // conv2 + shortcut (F32X3: pooled where conv2 pools), or conv2 alone ("c2") where the tail adds the identity shortcut
    if ((rc = p.keep(blk(bi, resid_in_tail ? "c2" : "o"), p.o, pooled_by_conv ? T / 3 : T, K.cout, KEEP_DT))) return rc;
    return rn_block_tail(p, bi, tail_fused, pooled_by_conv, resid_in_tail);
}

// aggregation: attentive statistics pooling                                          RawNet2_custom.py:215-224
// (pre = lrelu(bn_before_agg(x)) came out of block 7's AFMS pass)
static int rn_aggregate_asp(RnPass& p) {
    svhip_handle* h = p.h;
    auto& s = p.s;
    const int B = p.B, T = p.T, M = B * T, E = h->cfg.embed_dim;
    int rc;
    // (1 x 1 layers, like the projection shortcut, are given the handle's T: no frame index enters a pointwise GEMM without column sums or bias_utt)
    GemmParams pa = conv_params(h, s.att0, p.pre, 512, p.hb, 128, M, h->T);
    pa.act1 = ACT_LRELU001;
    if ((rc = conv_gemm(h, s.att0, pa))) return rc;
    float* logits = s.logits + (size_t)p.b0 * T * 512;
    GemmParams pl = conv_params(h, s.att3, p.hb, 128, logits, 512, M, h->T);
    pl.out_f32 = 1;
    if ((rc = conv_gemm(h, s.att3, pl))) return rc;
    if ((rc = p.keep("rn_logits", logits, T, 512, KEEP_F32))) return rc;
    if ((rc = run(h, "rn_attn_pool", 0, [&]() { return launch_rn_attn_pool(logits, p.pre, p.dt, B, T, 512, p.pooled, p.st); }))) return rc;
    return run(h, "rn_fc", 2.0 * B * s.fc.N * s.fc.K, [&]() {
        // (16-bit handles, full batches: the K-split MFMA form — fp32-grade handles keep ONE kernel for every batch size here)
        return launch_rowvec_linear(p.pooled, 1024, s.fc.W, s.fc.bias, p.emb, E, B, E, 1024, ACT_NONE, p.st, p.lin_part, true);
    });
}

// aggregation: GRU over the T frames, its last state through fc_after_gru            RawNet2_custom.py:196-207
// (pre = lrelu(bn_before_gru(x)), (B T, 512) frame-major, came out of block 7's AFMS pass)
static int rn_aggregate_gru(RnPass& p) {
    svhip_handle* h = p.h;
    auto& s = p.s;
    const int B = p.B, T = p.T, G = 3 * RN_GRU_HIDDEN, E = h->cfg.embed_dim;
    int rc;
    float* gi = s.gru_gi + (size_t)p.b0 * T * G;
    GemmParams pg = conv_params(h, s.gru_ih, p.pre, 512, gi, G, B * T, h->T);
    pg.out_f32 = 1;
    const GemmPlan plan = conv_plan(h, s.gru_ih, pg);          // (an fp32 output never takes the S32 form: plan.x3 is false)
    if (plan.x3) SV_FAIL(h, SVHIP_ERR_STATE, "rn_gru_proj: unexpected split-operand route");
    if ((rc = run(h, "rn_gru_proj", plan.flops, [&]() { return launch_gemm(plan.q, h->bf16, p.st); }))) return rc;
    float* hb[2] = {s.gru_hbuf[0] + (size_t)p.b0 * RN_GRU_HIDDEN, s.gru_hbuf[1] + (size_t)p.b0 * RN_GRU_HIDDEN};
    for (int t = 0; t < T; ++t)          // step t reads hb[t & 1] (h0 = 0: nothing) and writes hb[(t + 1) & 1]
        if ((rc = run(h, "rn_gru_step", 2.0 * B * G * RN_GRU_HIDDEN, [&]() {
                 return launch_rn_gru_step(s.gru_whh, p.dt, gi, s.gru_bhn, t ? hb[t & 1] : nullptr, hb[(t + 1) & 1], B, T, t, p.st);
             }))) return rc;
    if (p.b0 == 0) s.gru_in = p.pre;                             // (rawnet2_forward forgets it after a sliced forward)
    s.gru_h = s.gru_hbuf[T & 1];
    return run(h, "rn_gru_fc", 2.0 * B * s.gru_fc.N * s.gru_fc.K, [&]() {
        return launch_rowvec_linear(hb[T & 1], RN_GRU_HIDDEN, s.gru_fc.W, s.gru_fc.bias, p.emb, E, B, E, RN_GRU_HIDDEN, ACT_NONE, p.st, p.lin_part, true);
    });
}

// utterances [b0, b0 + B) of the call, enqueued on h->cur: front-end, fused chain, the remaining blocks, aggregation
static int rawnet2_forward_part(svhip_handle* h, const float* d_wav_all, int b0, int B) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const int e = h->esz;
    const size_t at = (size_t)b0 * s.T1 * 128;                   // the slice's offset into an activation buffer (T1 x 128: the largest activation)
    const bool conv = c.model == SVHIP_MODEL_RAWNET2_CONV;
    RnPass p{h, s};
    p.b0 = b0; p.B = B; p.st = h->cur; p.dt = h->dt;
    p.wav = d_wav_all + (size_t)b0 * c.samples;
    p.x = off(s.buf[0], at, e); p.pre = off(s.buf[1], at, e); p.hb = off(s.buf[2], at, e);
    p.o = off(s.buf[3], at, e); p.sc = off(s.buf[4], at, e); p.xn = off(s.buf[5], at, e);
    p.sinc_x3 = !conv && h->x3 && s.filt_x3 && !h->opt.rn_sinc_f32;
    p.stats = conv ? nullptr : s.stats + (size_t)b0 * 2;
    p.ln = conv ? nullptr : h->bf16 ? static_cast<char*>(s.xn) + (size_t)b0 * 2 * s.Lp * 2 : p.sinc_x3 ? static_cast<char*>(s.xn) + (size_t)b0 * 4 * s.Lp * 2 : nullptr;
    p.mean = s.mean + (size_t)b0 * 512;
    p.scratch = s.scratch + (size_t)b0 * 16 * 512;
    p.part = s.part + (size_t)b0 * (rn_block128_ntiles(s.T1) + 1) * 4 * 128;
    p.gate[0] = s.gate + (size_t)b0 * 512; p.gate[1] = s.gate + ((size_t)c.max_batch + b0) * 512;
    p.pooled = s.pooled + (size_t)b0 * 1024;
    p.emb = h->d_emb + (size_t)b0 * c.embed_dim;
    p.lin_part = h->bf16 && h->d_lin_part ? h->d_lin_part + (size_t)b0 * h->lin_part_per_utt : nullptr;
    p.T = s.T1;
    const RnBlock& K0 = s.blocks[0];
    p.fuse_ok = h->bf16 && !h->opt.rn_unfused;
    p.chain0 = p.fuse_ok && rn_block128_supported(K0.cin, K0.cout, p.T, K0.downsample, K0.has_shortcut, K0.conv1.Kp, K0.conv2.Kp);
    p.conv_fused = conv && p.chain0 && !h->opt.rn_conv_unfused;
    int rc, first = 0;
    if ((rc = rn_front(p)) || (rc = rn_fused_chain(p, first))) return rc;
    for (int bi = first; bi < 8; ++bi)
        if ((rc = rn_block(p, bi))) return rc;
    return rn_is_gru(c.model) ? rn_aggregate_gru(p) : rn_aggregate_asp(p);
}

// whole batch: one slice, or `lanes` slices on as many streams, so that the small and under-filled kernels of one slice (the late
// blocks are grids of 86 - 400 workgroups, the AFMS passes are latency-bound) run beside the big ones of another
int rawnet2_forward(svhip_handle* h, const float* d_wav, int B) {
    const int lanes = (h->lanes > 1 && B >= 16 * h->lanes) ? h->lanes : 1;
    ++S(h).keep.epoch;
    const int rc = forward_lanes(h, rawnet2_forward_part, d_wav, B, lanes, ((B + lanes - 1) / lanes + 3) & ~3);
    if (lanes > 1) S(h).gru_in = nullptr;          // the slices' GRU inputs are not one (B T, 512) block
    return rc;
}


// ---- ragged packs of the 'conv' model --------------------------------------------------------------------------------------
// RawNet2's rules for a pack of waveforms (RaggedCheckFn; include/svhip.h), on the host alone
int rawnet2_ragged_check(const svhip_config& c, const int32_t* lengths, int n, bool, std::string& err) {
    const int min_samples = 3 * RN_MIN_FRAMES;
    if (c.max_batch <= 0 || c.samples < min_samples) return refuse(err, SVHIP_ERR_INVALID, "bad max_batch / samples (RawNet2 'conv' needs samples >= %d)", min_samples);
    const int64_t cap = (int64_t)c.max_batch * (c.samples / 3);
    int64_t rows = 0;
    for (int i = 0; i < n; ++i) {
        if (lengths[i] < min_samples)
            return refuse(err, SVHIP_ERR_INVALID, "utterance %d: %d samples, fewer than RawNet2's minimum of %d (729 front-end frames: one frame reaches the aggregation)",
                          i, lengths[i], min_samples);
        if (int rc = rag_rows_fit(err, i, rows += lengths[i] / 3, cap, "T1")) return rc;
    }
    return SVHIP_OK;
}

// seven frame levels: the front-end's T1 = floor(L / 3) frames, then what each of the six max_pool1d(3) stages leaves
static void rn_rag_frames(const svhip_config&, int64_t len, bool, int T[RAG_LEVELS]) {
    T[0] = (int)(len / 3);
    for (int l = 1; l < RAG_LEVELS; ++l) T[l] = T[l - 1] / 3;
}
static const RagRule kRawnet2Rag = {7, rn_rag_frames, false};

// RawNet2.forward over a pack: n utterances (utterance u: pk.len[u] samples at d_wav + pk.off[u]) as packed rows at seven frame levels,
// on the handle's stream.  A walk of its own, not a `pk` threaded through rawnet2_forward_part: the fixed forward is a tree of routes
// (the fused rn_block128 chain, rn_step, the conv2 + shortcut fold, three tail forms, lanes, the developer options that pick among
// them), chosen by the batch size and the device, and a pack takes none of them — every GEMM is the generic kernel
// (launch_gemm_ragged), every tail the segment-table form (rn_ragged.hip), so that nothing depends on n, on the neighbours or on
// num_cu.  A pk pointer would double every branch of that tree for a path that shares only the layer order with it.  Of the
// developer options it reads rn_keep and layer_labels alone.
// Buffers: the six activation buffers of rawnet2_alloc, max_batch * T1 * 128 elements each, hold every tensor of every level: level l
// has sum_u floor(T_u / 3^l) <= floor(M0 / 3^l) rows (M0 <= max_batch * T1 by the capacity rule) of at most 128 * 2^ceil(l / 2)
// channels, so the rows shrink 3 x where the channels at most double.  What is sized per utterance in rawnet2_alloc does not fit a
// pack (its last level can have more rows than max_batch * tf, its slices are not capped at 16): rawnet2_rag_alloc.
static int rawnet2_rag_alloc(svhip_handle* h) {
    auto& s = S(h);
    const size_t B = h->cfg.max_batch, M0 = B * (size_t)s.T1;
    int rc;
    if (!s.rag_slice0 && (rc = dev_alloc(h, &s.rag_slice0, (size_t)RAG_LEVELS * (B + 1)))) return rc;
    if (!s.rag_part) {          // a tail's slices: level l has at most M0 / 3^l / RN_RAG_SLICE + max_batch of them, of the block's channels
        size_t need = 0, rows = M0;
        for (int bi = 0; bi < 8; ++bi) {
            const RnBlock& K = s.blocks[bi];
            if (K.downsample) rows /= 3;
            need = std::max(need, (rows / RN_RAG_SLICE + B + 1) * (size_t)K.cout);
        }
        if ((rc = dev_alloc(h, &s.rag_part, need))) return rc;
    }
    if (!s.rag_gate && (rc = dev_alloc(h, &s.rag_gate, 8 * B * 512))) return rc;
    if (!s.rag_logits && (rc = dev_alloc(h, &s.rag_logits, (M0 / 729 + 1) * 512))) return rc;
    return SVHIP_OK;
}

static int rawnet2_rag_walk(svhip_handle* h, const RagPack& pk) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const int n = pk.n, dt = h->dt;
    const size_t B = c.max_batch, M0cap = B * (size_t)s.T1;
    h->cur = h->stream;
    hipStream_t st = h->cur;
    int rc;
    ++s.keep.epoch;
    // option rn_keep: a packed tensor the forward has just stored (level `lvl` rows; lvl < 0: one row per utterance)
    auto keep = [&](const std::string& name, const void* src, int lvl, int cols, bool f32) -> int {
        if (!h->opt.rn_keep) return SVHIP_OK;
        size_t cap_rows = lvl < 0 ? B : M0cap, rows = lvl < 0 ? (size_t)n : (size_t)pk.lv[lvl].M;
        for (int l = 0; l < lvl; ++l) cap_rows /= 3;
        return rn_keep(h, st, name, src, f32 ? KEEP_F32 : KEEP_DT, rows, true, cap_rows, cols, 0, rows, n);
    };
    // a GEMM over the rows of level g on the generic kernel (pointwise layers need no table)
    auto gemm = [&](const ConvLayer& K, GemmParams p, const Seg& g) {
        p.rag_utt = g.utt; p.rag_row0 = g.row0;
        char label[96];
        const char* kl = K.taps > 1 ? "gemm_conv" : "gemm_pw";
        if (h->opt.layer_labels) snprintf(label, sizeof(label), "%s M%d N%d K%d", kl, p.M, K.N, K.K);
        else snprintf(label, sizeof(label), "%s", kl);
        return run(h, label, (double)p.M * K.flops_per_row, [&]() { return launch_gemm_ragged(p, h->bf16, st); });
    };
    for (int l = 0; l < 6; ++l)          // the levels a k = 3 convolution reads
        if ((rc = run(h, "rag_rows", 0, [&]() { return launch_rag_rows(pk.lv[l].row0, n, pk.lv[l].maxT, pk.lv[l].utt, st); }))) return rc;
    const int ld = (int)(pk.lv[1].row0 - pk.lv[0].row0);          // the levels' row0 tables lie max_batch + 1 ints apart (rag_pack)
    if ((rc = run(h, "rn_rag_slices", 0, [&]() { return launch_rn_rag_slices(pk.lv[0].row0, ld, RAG_LEVELS, n, s.rag_slice0, st); }))) return rc;

    void *x = s.buf[0], *pre = s.buf[1], *hb = s.buf[2], *o = s.buf[3], *sc = s.buf[4], *xn = s.buf[5];
    // front-end: x = conv1(wav) and block 0's pre-activation lrelu(bn1(x))                  RawNet2_custom.py:166-169, RawNet_baseline.py:222
    if ((rc = run(h, "rn_rag_front", 2.0 * 128.0 * 3.0 * pk.lv[0].M, [&]() {
             return launch_rn_rag_front(pk.in, pk.off, pk.len, pk.lv[0].row0, n, pk.lv[0].maxT, s.cw, s.blocks[0].bn1_scale, s.blocks[0].bn1_shift, 0.3f,
                                        x, pre, dt, st);
         }))) return rc;
    if ((rc = keep("rn_front", x, 0, 128, false)) || (rc = keep(blk(0, "pre"), pre, 0, 128, false))) return rc;
    int li = 0;
    for (int bi = 0; bi < 8; ++bi) {
        const RnBlock& K = s.blocks[bi];
        const Seg& g = pk.lv[li];
        const int M = g.M;
        const void* resid = x;                                                    // identity shortcut takes the pre-BN x (:223)
        if (K.has_shortcut) {
            if ((rc = gemm(K.shortcut, conv_params(h, K.shortcut, pre, K.cin, sc, K.cout, M, 1), g))) return rc;
            resid = sc;
        }
        GemmParams p1 = conv_params(h, K.conv1, pre, K.cin, hb, K.cout, M, 1);      // conv1 -> bn2 -> lrelu (epilogue)       :224-225
        p1.act2 = ACT_LRELU03; p1.pad_mode = PAD_ZERO;
        if ((rc = gemm(K.conv1, p1, g))) return rc;
        GemmParams p2 = conv_params(h, K.conv2, hb, K.cout, o, K.cout, M, 1);       // conv2 + shortcut                       :226
        p2.pad_mode = PAD_ZERO; p2.R = resid; p2.ldr = K.cout;
        if ((rc = gemm(K.conv2, p2, g))) return rc;
        if ((rc = keep(blk(bi, "o"), o, li, K.cout, false))) return rc;
        // the tail: [max_pool1d(3)] -> AFMS -> the next consumer's lrelu(bn(.)), over the slices of the out level       :228-229, :62-68
        const int lo = K.downsample ? li + 1 : li;
        const Seg& go = pk.lv[lo];
        int nslices = 0;
        for (int u = 0; u < n; ++u) nslices += (go.hrow0[u + 1] - go.hrow0[u] + RN_RAG_SLICE - 1) / RN_RAG_SLICE;
        const int* sl0 = s.rag_slice0 + (size_t)lo * ld;
        float* gate = s.rag_gate + (size_t)bi * B * 512;
        const float* nsc = bi < 7 ? s.blocks[bi + 1].bn1_scale : s.agg_scale;
        const float* nsh = bi < 7 ? s.blocks[bi + 1].bn1_shift : s.agg_shift;
        const bool x_dead = bi == 7 || s.blocks[bi + 1].has_shortcut;              // x is read only as an identity shortcut
        // (layer_labels: one profile row per block, "<kernel> M<in rows> C<channels>")
        auto tl = [&](const char* k) {
            std::string l = k;
            if (h->opt.layer_labels) l += " M" + std::to_string(M) + " C" + std::to_string(K.cout);
            return l;
        };
        if ((rc = run(h, tl("rn_rag_tail_part").c_str(), 0, [&]() { return launch_rn_rag_tail_part(o, dt, K.downsample, g.row0, go.row0, sl0, n, nslices, K.cout, s.rag_part, st); })))
            return rc;
        if ((rc = run(h, tl("rn_rag_gate").c_str(), 2.0 * n * K.cout * K.cout, [&]() { return launch_rn_rag_gate(s.rag_part, go.row0, sl0, n, K.cout, K.afms_fcT, K.afms_fc.bias, gate, st); })))
            return rc;
        if ((rc = run(h, tl("rn_rag_tail_apply").c_str(), 0, [&]() {
                 return launch_rn_rag_tail_apply(o, dt, K.downsample, g.row0, go.row0, sl0, n, nslices, K.cout, K.alpha, gate, nsc, nsh, 0.3f,
                                                 x_dead ? nullptr : xn, pre, st);
             }))) return rc;
        std::swap(x, xn);
        li = lo;
        if ((rc = keep(blk(bi, "gate"), gate, -1, K.cout, true))) return rc;
        if ((rc = keep(bi < 7 ? blk(bi + 1, "pre") : std::string("rn_agg_in"), pre, li, K.cout, false))) return rc;
        if (!x_dead && (rc = keep(blk(bi + 1, "x"), x, li, K.cout, false))) return rc;
    }
    // aggregation: attentive statistics pooling over each utterance's own frames of the last level         RawNet2_custom.py:215-224
    const Seg& g6 = pk.lv[6];
    GemmParams pa = conv_params(h, s.att0, pre, 512, hb, 128, g6.M, 1);
    pa.act1 = ACT_LRELU001;
    if ((rc = gemm(s.att0, pa, g6))) return rc;
    GemmParams pl = conv_params(h, s.att3, hb, 128, s.rag_logits, 512, g6.M, 1);
    pl.out_f32 = 1;
    if ((rc = gemm(s.att3, pl, g6))) return rc;
    if ((rc = keep("rn_logits", s.rag_logits, 6, 512, true))) return rc;
    if ((rc = run(h, "rn_rag_attn_pool", 0, [&]() { return launch_rn_rag_attn_pool(s.rag_logits, pre, dt, g6.row0, n, 512, s.pooled, st); }))) return rc;
    return run(h, "rn_fc", 2.0 * n * s.fc.N * s.fc.K, [&]() {
        return launch_rag_linear(s.pooled, 1024, s.fc.W, s.fc.bias, h->d_emb, c.embed_dim, n, c.embed_dim, 1024, ACT_NONE, st);
    });
}

int rawnet2_embed_ragged(svhip_handle* h, const float* in, bool in_host, bool, const int64_t* in_off, const int32_t* lengths, int n) {
    auto& s = S(h);
    // utt tables for the levels a k = 3 convolution reads (0 - 5); nothing reads the last level's
    size_t utt_cap[RAG_LEVELS] = {};
    size_t rows = (size_t)h->cfg.max_batch * s.T1;
    for (int l = 0; l < 6; ++l, rows /= 3) utt_cap[l] = rows + 1;
    RagPack pk;
    int rc;
    if ((rc = rawnet2_rag_alloc(h)) || (rc = rag_pack(h, s.rag, kRawnet2Rag, utt_cap, in, in_host, true, in_off, lengths, n, pk)) ||
        (rc = rawnet2_rag_walk(h, pk))) return rc;
    set_rag_rows(h, pk);
    return SVHIP_OK;
}

}  // namespace svhip
