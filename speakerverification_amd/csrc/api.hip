// api.hip — C ABI of libsvhip: handle lifetime, developer options, weight loading, embedding, staging, stages and profiling
// (see include/svhip.h).  The handle is in handle.h; what the models share when weights are loaded in api_weights.hip, the conv-layer
// GEMM in api_gemm.hip, what the ragged calls share in api_ragged.hip, each model's own host code and state in its api_<model>.hip
// (kModels below lists them); the scoring side in api_scoring.hip (what its calls share, the simple calls), api_asnorm.hip, api_search.hip,
// api_audit.hip and api_metrics.hip, over scoring_host.h.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "handle.h"

using namespace svhip;

namespace svhip {      // the ragged hooks of the models that have them: only kModels names them
RaggedCheckFn ecapa_ragged_check, rawnet2_ragged_check, rawnet3_ragged_check, conformer_ragged_check, titanet_ragged_check, resnetse_ragged_check;
RaggedEmbedFn ecapa_embed_ragged, rawnet2_embed_ragged, rawnet3_embed_ragged, conformer_embed_ragged, titanet_embed_ragged, resnetse_embed_ragged;      // (RawNet2 / RawNet3: waveforms only, is_wave is true)
}

namespace {

thread_local std::string g_create_error;

// The developer / test options, one row each: svhip_set_option's names (include/svhip.h lists the same), the DevOpts field, the
// SVHIP_* environment variable (nullptr: none) and the default.  svhip_create reads the variables ONCE, as a new handle's defaults;
// afterwards only svhip_set_option changes the fields — no getenv on any forward or scoring call.  Each variable keeps its own parse:
// OPT_SET: set at all -> 1 (SVHIP_LAYER_LABELS=0 turns labels on); OPT_IS1: a value starting with '1' -> 1; OPT_NUM: atoi.
enum DevOptParse { OPT_NO_ENV, OPT_SET, OPT_IS1, OPT_NUM };
struct DevOptRow { const char* name; int svhip_handle::DevOpts::*field; const char* env; DevOptParse parse; int dflt; };
#define SV_OPT(name, env, parse, dflt) {#name, &svhip_handle::DevOpts::name, env, parse, dflt}
const DevOptRow kDevOpts[] = {
    SV_OPT(layer_labels, "SVHIP_LAYER_LABELS", OPT_SET, 0),
    SV_OPT(x3_keep_f32, "SVHIP_X3_KEEP_F32", OPT_SET, 0),
    SV_OPT(r2_big, "SVHIP_R2_BIG", OPT_IS1, 0),
    SV_OPT(asp_v1, "SVHIP_ASP_V1", OPT_IS1, 0),
    SV_OPT(rn_unfused, "SVHIP_RN_UNFUSED", OPT_SET, 0),
    SV_OPT(asnorm_slab, "SVHIP_ASNORM_SLAB", OPT_SET, 0),
    SV_OPT(asnorm_f32mfma, "SVHIP_ASNORM_F32MFMA", OPT_SET, 0),
    SV_OPT(score_f32mfma, "SVHIP_SCORE_F32MFMA", OPT_SET, 0),
    SV_OPT(score_tiled, "SVHIP_SCORE_TILED", OPT_SET, 0),
    SV_OPT(asnorm_norefit, nullptr, OPT_NO_ENV, 0),
    SV_OPT(rn_sinc_full, "SVHIP_RN_SINC_FULL", OPT_IS1, 0),
    SV_OPT(fbank32, "SVHIP_FBANK32", OPT_IS1, 0),
    SV_OPT(fbank_unfused, "SVHIP_FBANK_UNFUSED", OPT_IS1, 0),
    SV_OPT(pw3_cus, "SVHIP_PW3_CUS", OPT_NUM, -1),
    SV_OPT(pw3_tail_off, "SVHIP_PW3_TAIL_OFF", OPT_IS1, 0),
    SV_OPT(cv_off, "SVHIP_CV_OFF", OPT_IS1, 0),
    SV_OPT(n128_off, "SVHIP_N128_OFF", OPT_IS1, 0),
    SV_OPT(rn_pool_off, "SVHIP_RN_POOL_OFF", OPT_IS1, 0),
    SV_OPT(rn_step_off, "SVHIP_RN_STEP_OFF", OPT_IS1, 0),
    SV_OPT(rn_sinc_f32, "SVHIP_RN_SINC_F32", OPT_IS1, 0),
    SV_OPT(rn_tail_big, "SVHIP_RN_TAIL_BIG", OPT_IS1, 0),
    SV_OPT(r2_slices, "SVHIP_R2_SLICES", OPT_NUM, -1),
    SV_OPT(rn_conv_unfused, "SVHIP_RN_CONV_UNFUSED", OPT_IS1, 0),
    SV_OPT(rn_keep, "SVHIP_RN_KEEP", OPT_IS1, 0),
    SV_OPT(cf_keep, "SVHIP_CF_KEEP", OPT_IS1, 0),
    SV_OPT(tn_keep, "SVHIP_TN_KEEP", OPT_IS1, 0),
    SV_OPT(rs_keep, "SVHIP_RS_KEEP", OPT_IS1, 0),
    SV_OPT(linkage_lds_rows, "SVHIP_LINKAGE_LDS_ROWS", OPT_NUM, 0),
    SV_OPT(linkage_fill_only, nullptr, OPT_NO_ENV, 0),
};
#undef SV_OPT

int none_check(const svhip_config& c, const char*& err) {
    if (c.compute == SVHIP_F16) { err = "SVHIP_F16 is RawNet2's 16-bit mode (ECAPA's is SVHIP_BF16)"; return SVHIP_ERR_UNSUPPORTED; }
    return SVHIP_OK;
}
int fbank_then_features(svhip_handle* h, const float* d_wav, int B);

// The models, one row per model id.  The three RawNet2 models share their functions (front_proc / aggregate follow cfg.model).
const ModelOps kModels[] = {
    // model                   check            spec            finalize            alloc            embed_wave           embed_feat         stage            lanes
    {SVHIP_MODEL_ECAPA,        ecapa_check,     ecapa_spec,     ecapa_finalize,     ecapa_alloc,     ecapa_embed_wave,    ecapa_forward,     ecapa_stage,     2,
     nullptr, ecapa_ragged_check, ecapa_embed_ragged},
    {SVHIP_MODEL_RAWNET2,      rawnet2_check,   rawnet2_spec,   rawnet2_finalize,   rawnet2_alloc,   rawnet2_forward,     nullptr,           rawnet2_stage,   4},
    {SVHIP_MODEL_RAWNET2_CONV, rawnet2_check,   rawnet2_spec,   rawnet2_finalize,   rawnet2_alloc,   rawnet2_forward,     nullptr,           rawnet2_stage,   4,
     nullptr, rawnet2_ragged_check, rawnet2_embed_ragged},       // (the sinc models' LayerNorm(nb_samp) fixes their length: no ragged forward)
    {SVHIP_MODEL_RAWNET2_GRU,  rawnet2_check,   rawnet2_spec,   rawnet2_finalize,   rawnet2_alloc,   rawnet2_forward,     nullptr,           rawnet2_stage,   4},
    {SVHIP_MODEL_RAWNET3,      rawnet3_check,   rawnet3_spec,   rawnet3_finalize,   rawnet3_alloc,   rawnet3_forward,     nullptr,           rawnet3_stage,   4,
     nullptr, rawnet3_ragged_check, rawnet3_embed_ragged},
    {SVHIP_MODEL_TITANET,      titanet_check,   titanet_spec,   titanet_finalize,   titanet_alloc,   fbank_then_features, titanet_forward,   titanet_stage,   4,
     "encoder.mega_blocks.", titanet_ragged_check, titanet_embed_ragged},      // (the block count follows from what was loaded: titanet_finalize checks its blocks)
    {SVHIP_MODEL_CONFORMER,    conformer_check, conformer_spec, conformer_finalize, conformer_alloc, fbank_then_features, conformer_forward, conformer_stage, 4,
     nullptr, conformer_ragged_check, conformer_embed_ragged},
    {SVHIP_MODEL_RESNETSE,     resnetse_check,  resnetse_spec,  resnetse_finalize,  resnetse_alloc,  fbank_then_features, resnetse_forward,  resnetse_stage,  4,
     nullptr, resnetse_ragged_check, resnetse_embed_ragged},
    {SVHIP_MODEL_NONE,         none_check,      nullptr,        nullptr,            nullptr,         nullptr,             nullptr,           nullptr,         1},   // fbank + scoring
    {SVHIP_MODEL_FUSION_HEAD,  fusion_head_check, fusion_head_spec, fusion_head_finalize, fusion_head_alloc, nullptr,     nullptr,           nullptr,         1},   // svhip_fusion_head
};

const ModelOps* model_ops(int model) {
    for (const ModelOps& m : kModels)
        if (m.model == model) return &m;
    return nullptr;
}

WeightSpec model_spec(const svhip_handle* h) {
    WeightSpec spec;
    if (const ModelOps* m = model_ops(h->cfg.model); m->spec) m->spec(h->cfg, spec);
    return spec;
}

// the spectral models' waveform path: the mel power in fp32, then the net
int fbank_then_features(svhip_handle* h, const float* d_wav, int B) {
    int rc;
    if ((rc = run(h, "fbank", 0, [&]() { return launch_fbank(h->fb, d_wav, B, h->cfg.samples, h->T, h->d_feat, h->stream); }))) return rc;
    h->feat_is_stale = false;
    return model_ops(h->cfg.model)->embed_feat(h, h->d_feat, B);
}

}  // namespace

namespace svhip {

// ---- profiling-aware launch wrapper --------------------------------------------------------------
hipEvent_t prof_event(svhip_handle* h) {
    if (!h->ev_free.empty()) { hipEvent_t e = h->ev_free.back(); h->ev_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

void prof_collect(svhip_handle* h) {
    if (h->ev_pending.empty()) return;
    (void)hipStreamSynchronize(h->stream);
    for (int i = 0; i < 4; ++i) if (h->lane_stream[i]) (void)hipStreamSynchronize(h->lane_stream[i]);
    for (auto& pe : h->ev_pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pe.e0, pe.e1) == hipSuccess) h->prof_entries[pe.entry].ms += ms;
        h->ev_free.push_back(pe.e0);
        h->ev_free.push_back(pe.e1);
    }
    h->ev_pending.clear();
}

int unknown_stage(svhip_handle* h, const std::string& name) { SV_FAIL(h, SVHIP_ERR_INVALID, "unknown stage %s", name.c_str()); }

int keep_stage(svhip_handle* h, KeptStages& ks, hipStream_t st, const std::string& name, const void* src, int kind, size_t rows, bool packed,
               size_t cap_rows, int cols, size_t row0, size_t nrows, int utts) {
    const bool f32 = kind != KEEP_DT || !h->bf16;
    const size_t es = f32 ? 4 : 2, need = cap_rows * cols * es;
    KeptStages::Kept& k = ks.kept[name];
    if (!k.buf || k.cap < need) {
        void* q = nullptr;
        SV_HIP(h, hipMalloc(&q, need));
        h->allocs.push_back(q);
        k.buf = q; k.cap = need; k.epoch = 0;
    }
    // (the first copy of a forward, or another shape than the earlier slices': what the buffer held does not count)
    if (k.epoch != ks.epoch || k.rows != rows || k.cols != (size_t)cols || k.f32 != f32 || k.packed != packed) {
        k.rows = rows; k.cols = cols; k.f32 = f32; k.packed = packed; k.epoch = ks.epoch; k.utts = 0;
    }
    void* dst = static_cast<char*>(k.buf) + row0 * cols * es;
    if (kind == KEEP_S32) SV_HIP(h, launch_unsplit_s32(src, cols, static_cast<float*>(dst), cols, (int64_t)nrows, cols, st));
    else SV_HIP(h, hipMemcpyAsync(dst, src, nrows * cols * es, hipMemcpyDeviceToDevice, st));
    k.utts += utts;
    return SVHIP_OK;
}

int kept_view(svhip_handle* h, const KeptStages& ks, const std::string& name, int B, const char* option, bool option_on, StageView& v) {
    const auto it = ks.kept.find(name);
    if (it == ks.kept.end() || it->second.epoch != ks.epoch || it->second.utts != B) {
        if (option_on) SV_FAIL(h, SVHIP_ERR_STATE, "stage %s: the route of the last forward never stored it", name.c_str());
        SV_FAIL(h, SVHIP_ERR_STATE, "stage %s: option %s was not set", name.c_str(), option);
    }
    const KeptStages::Kept& k = it->second;
    // (a pack's rows are those of the stage's level, counted when it was kept; a fixed-length forward has `rows` per utterance)
    v.src = k.buf; v.rows = k.packed ? k.rows : (size_t)B * k.rows; v.cols = v.ld = k.cols; v.f32 = k.f32;
    return SVHIP_OK;
}

// A whole-batch forward: one slice on the handle's stream, or `lanes` slices of `per` utterances (the last one takes the rest) on the
// lane streams, forked from and joined back into the handle's stream.
int forward_lanes(svhip_handle* h, ForwardPart part, const float* in, int B, int lanes, int per) {
    int rc = SVHIP_OK;
    if (lanes > 1) {
        SV_HIP(h, hipEventRecord(h->lane_ev[4], h->stream));
        for (int l = 0; l < lanes && !rc; ++l) {
            const int b0 = l * per, n = l + 1 < lanes ? std::min(per, B - b0) : B - b0;
            if (n <= 0) break;
            SV_HIP(h, hipStreamWaitEvent(h->lane_stream[l], h->lane_ev[4], 0));
            h->cur = h->lane_stream[l];
            rc = part(h, in, b0, n);
            h->cur = h->stream;
            if (rc) break;
            SV_HIP(h, hipEventRecord(h->lane_ev[l], h->lane_stream[l]));
            SV_HIP(h, hipStreamWaitEvent(h->stream, h->lane_ev[l], 0));
        }
    } else {
        h->cur = h->stream;
        rc = part(h, in, 0, B);
    }
    if (!rc) { h->lastB = B; h->rag_levels = 0; }
    return rc;
}

}  // namespace svhip

namespace {

int check_ready(svhip_handle* h, int B) {
    if (!h) return SVHIP_ERR_INVALID;
    if (!h->finalized) SV_FAIL(h, SVHIP_ERR_STATE, "weights not finalized (call svhip_finalize_weights first)");
    if (B <= 0 || B > h->cfg.max_batch) SV_FAIL(h, SVHIP_ERR_INVALID, "batch %d outside [1, max_batch=%d]", B, h->cfg.max_batch);
    return SVHIP_OK;
}

// The numeric status of the forwards since the last reset (the stream must be idle): the kernels that raise a bit also set the mapped
// host flag, so the common case costs one host load.  When both bits are set the RANGE report is the one returned: it names the cause (an input the
// planes cannot carry ends as inf / NaN embeddings) and carries the count of non-finite embedding values in its text.
enum { SVHIP_STATUS_NONFINITE = 1, SVHIP_STATUS_RANGE = 2 };
int numeric_status(svhip_handle* h, bool reset) {
    if (!h->host_flag || !*h->host_flag) return SVHIP_OK;
    uint32_t st[4] = {0, 0, 0, 0};
    SV_HIP(h, hipMemcpy(st, h->d_status, 16, hipMemcpyDeviceToHost));
    if (reset) {
        SV_HIP(h, hipMemset(h->d_status, 0, 16));
        *h->host_flag = 0;
    }
    // (the range report outranks the non-finite one: it names the cause — an input the planes cannot carry ends as inf / NaN embeddings)
    if (st[0] & SVHIP_STATUS_RANGE)
        SV_FAIL(h, SVHIP_ERR_RANGE, "%u input feature value(s) exceed 65504 in magnitude (or are not finite): SVHIP_F32X3 carries operands as IEEE-half "
                "hi | lo planes and cannot represent them; %u embedding value(s) came out non-finite (normalise the input - log_input / input_norm - "
                "or use compute = f32)", st[2], st[1]);
    if (st[0] & SVHIP_STATUS_NONFINITE)
        SV_FAIL(h, SVHIP_ERR_NONFINITE, "%u embedding value(s) are not finite%s (the embeddings were written as computed)", st[1],
                h->f16 ? ": an fp16 activation overflowed 65504 (or the input was not finite) - this checkpoint needs compute = f32 (exact); bf16 is "
                         "range-safe and fast but loses accuracy on RawNet2 (bf16 weight rounding)"
                : h->x3 ? ": a GEMM operand exceeded 65504, the range of SVHIP_F32X3's half-precision hi | lo planes (or the input was not finite) - "
                          "use compute = f32 (exact); bf16 is range-safe and fast at 16-bit accuracy"
                        : ": the input was not finite, or the weights overflow fp32");
    return SVHIP_OK;
}

int finish(svhip_handle* h, int flags) {
    if (flags & SVHIP_ASYNC) return SVHIP_OK;
    SV_HIP(h, hipStreamSynchronize(h->stream));
    return numeric_status(h, true);
}

// the embeddings leave the workspace: device output through emb_out_kernel (copy + finite check in one pass), host output checked in
// place and copied
int emit_embeddings(svhip_handle* h, int B, float* emb_out, int flags) {
    const int n = B * h->cfg.embed_dim;
    h->cur = h->stream;
    float* dst = (flags & SVHIP_OUT_DEVICE) ? emb_out : h->d_emb;
    int rc = run(h, "emb_out", 0, [&]() { return launch_emb_out(h->d_emb, dst, n, h->d_status, h->host_flag_dev, h->stream); });
    if (rc) return rc;
    if (!(flags & SVHIP_OUT_DEVICE)) SV_HIP(h, hipMemcpyAsync(emb_out, h->d_emb, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    return SVHIP_OK;
}

// ---- ragged calls: utterances of different lengths in one call --------------------------------------------------
// Each ragged export serves one model (kModels names its check and its forward) and refuses the others by its name; computes: the
// compute types it accepts, as a mask of 1 << SVHIP_*, and their names for the refusal
struct RaggedExport { int model; const char* name; unsigned computes; const char* compute_names; };
constexpr unsigned kRagF32Bf16 = 1u << SVHIP_F32 | 1u << SVHIP_BF16;
constexpr RaggedExport kRagEcapa{SVHIP_MODEL_ECAPA, "ECAPA", kRagF32Bf16, "SVHIP_F32 or SVHIP_BF16"},
                       kRagRawnet2{SVHIP_MODEL_RAWNET2_CONV, "RAWNET2_CONV", kRagF32Bf16 | 1u << SVHIP_F16, "SVHIP_F32, SVHIP_BF16 or SVHIP_F16"},
                       kRagRawnet3{SVHIP_MODEL_RAWNET3, "RAWNET3", kRagF32Bf16, "SVHIP_F32 or SVHIP_BF16"},
                       kRagConformer{SVHIP_MODEL_CONFORMER, "CONFORMER", kRagF32Bf16, "SVHIP_F32 or SVHIP_BF16"},
                       kRagTitanet{SVHIP_MODEL_TITANET, "TITANET", kRagF32Bf16, "SVHIP_F32 or SVHIP_BF16"},
                       kRagResnetse{SVHIP_MODEL_RESNETSE, "RESNETSE", kRagF32Bf16, "SVHIP_F32 or SVHIP_BF16"};

// the rules of a pack, on the host alone, in this order: the scope, the model's rules on the configuration, the pack size, the model's
// rules on every utterance in index order
int ragged_rules(const RaggedExport& x, const svhip_config& c, const int32_t* lengths, int n, bool is_wave, std::string& err) {
    if (x.model == SVHIP_MODEL_RAWNET2_CONV && (c.model == SVHIP_MODEL_RAWNET2 || c.model == SVHIP_MODEL_RAWNET2_GRU))
        return refuse(err, SVHIP_ERR_UNSUPPORTED, "ragged %s packs: SVHIP_MODEL_%s only (the sinc front-end of SVHIP_MODEL_RAWNET2 and SVHIP_MODEL_RAWNET2_GRU "
                      "starts with LayerNorm(nb_samp), whose weights fix the input length)", x.name, x.name);
    if (c.model != x.model)
        return refuse(err, SVHIP_ERR_UNSUPPORTED, "ragged %s packs: SVHIP_MODEL_%s only (ECAPA, RawNet2 'conv', RawNet3, Conformer, TitaNet and ResNetSE packs have their own "
                      "calls; the other models embed one length per handle)", x.name, x.name);
    if (c.compute < 0 || c.compute >= 32 || !(x.computes >> c.compute & 1u))
        return refuse(err, SVHIP_ERR_UNSUPPORTED, "ragged %s packs: compute %s only", x.name, x.compute_names);
    // The pack size is tested between the model's two kinds of rules, as it always was, so that the first failing rule stays the same
    // one.  A RaggedCheckFn looks at no utterance when it is given n = 0, so the first call is its rules on the configuration alone
    // (they also make max_batch and the divisions of the second call safe); the second adds every utterance in index order.
    RaggedCheckFn* check = model_ops(x.model)->ragged_check;
    if (int rc = check(c, lengths, 0, is_wave, err)) return rc;
    if (n < 1 || n > c.max_batch) return refuse(err, SVHIP_ERR_INVALID, "ragged batch of %d utterances outside [1, max_batch=%d]", n, c.max_batch);
    return check(c, lengths, n, is_wave, err);
}

int ragged_check(const RaggedExport& x, const svhip_config* cfg, const int32_t* lengths, int32_t n, bool is_wave) {
    if (!cfg || cfg->struct_size != (int32_t)sizeof(svhip_config)) { g_create_error = "bad config / struct_size"; return SVHIP_ERR_INVALID; }
    if (!lengths) { g_create_error = "null pointer"; return SVHIP_ERR_INVALID; }
    return ragged_rules(x, *cfg, lengths, n, is_wave, g_create_error);
}

// argument and capacity checks on the host, then the model's ragged forward
int embed_ragged(const RaggedExport& x, svhip_handle* h, const float* in, const int64_t* offsets, const int32_t* lengths, int32_t n, float* emb_out,
                 int32_t flags, bool is_wave) {
    if (!h) return SVHIP_ERR_INVALID;
    if (!h->finalized) SV_FAIL(h, SVHIP_ERR_STATE, "weights not finalized (call svhip_finalize_weights first)");
    if (!in || !offsets || !lengths || !emb_out) SV_FAIL(h, SVHIP_ERR_INVALID, "null pointer");
    if (int rc = ragged_rules(x, h->cfg, lengths, n, is_wave, h->err)) return rc;
    for (int i = 0; i < n; ++i)
        if (offsets[i] < 0) SV_FAIL(h, SVHIP_ERR_INVALID, "utterance %d: negative offset (the limit is 0)", i);
    if ((flags & SVHIP_ASYNC) && (flags & (SVHIP_IN_DEVICE | SVHIP_OUT_DEVICE)) != (SVHIP_IN_DEVICE | SVHIP_OUT_DEVICE))
        SV_FAIL(h, SVHIP_ERR_INVALID, "SVHIP_ASYNC needs device pointers");
    SV_HIP(h, hipSetDevice(h->cfg.device));
    int rc = model_ops(x.model)->embed_ragged(h, in, !(flags & SVHIP_IN_DEVICE), is_wave, offsets, lengths, n);
    if (rc) return rc;
    if ((rc = emit_embeddings(h, n, emb_out, flags))) return rc;
    return finish(h, flags);
}

}  // namespace

// =====================================================================================================
extern "C" {

void svhip_default_config(svhip_config* c) {
    memset(c, 0, sizeof(*c));
    c->struct_size = (int32_t)sizeof(svhip_config);
    c->model = SVHIP_MODEL_ECAPA;
    c->compute = SVHIP_F32;
    c->device = 0;
    c->channels = 1024;
    c->n_mels = 80;
    c->embed_dim = 192;
    c->max_batch = 8;
    c->samples = 32000;
    c->log_input = 1;
    c->input_norm = 0;
    c->fb_sr = 8000; c->n_fft = 512; c->win_length = 200; c->hop_length = 80;
    c->fmin = 0.0f; c->fmax = -1.0f; c->preemph = 0.97f;
    c->stream = nullptr;
    c->sinc_sr = 16000;
}

int svhip_abi_version(void) { return SVHIP_ABI_VERSION; }

const char* svhip_last_error(const svhip_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int svhip_create(const svhip_config* cfg, svhip_handle** out) {
    if (!cfg || !out || cfg->struct_size != (int32_t)sizeof(svhip_config)) { g_create_error = "bad config / struct_size"; return SVHIP_ERR_INVALID; }
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { g_create_error = std::string("no HIP device: ") + hipGetErrorString(e); return SVHIP_ERR_HIP; }
    if (cfg->device < 0 || cfg->device >= ndev) { g_create_error = "device ordinal out of range"; return SVHIP_ERR_INVALID; }
    const ModelOps* m = model_ops(cfg->model);
    if (!m) { g_create_error = "unknown model"; return SVHIP_ERR_INVALID; }
    const char* msg = "";
    if (int rc = m->check(*cfg, msg)) { g_create_error = msg; return rc; }
    if (cfg->compute != SVHIP_F32 && cfg->compute != SVHIP_BF16 && cfg->compute != SVHIP_F32X3 && cfg->compute != SVHIP_F16) { g_create_error = "unknown compute mode"; return SVHIP_ERR_INVALID; }
    // the sinc front-end's sample rate (0: 16000): min_low_hz + min_band_hz = 100 Hz must lie below the clamp at sinc_sr / 2
    if (cfg->sinc_sr < 0 || (cfg->sinc_sr ? cfg->sinc_sr : 16000) / 2 <= 100) { g_create_error = "bad sinc_sr: the sinc front-end needs sinc_sr / 2 > 100 Hz (0 means 16000)"; return SVHIP_ERR_INVALID; }
    if (cfg->n_mels <= 0 || cfg->n_mels % 8 != 0 || cfg->max_batch <= 0 || cfg->samples < cfg->n_fft || cfg->hop_length <= 0) { g_create_error = "bad n_mels / max_batch / samples"; return SVHIP_ERR_INVALID; }
    if ((e = hipSetDevice(cfg->device)) != hipSuccess) { g_create_error = hipGetErrorString(e); return SVHIP_ERR_HIP; }
    svhip_handle* h = new svhip_handle();
    h->cfg = *cfg;
    h->f16 = cfg->compute == SVHIP_F16;
    h->bf16 = cfg->compute == SVHIP_BF16 || h->f16;
    h->dt = h->f16 ? DT_F16 : h->bf16 ? DT_BF16 : DT_F32;
    h->x3 = cfg->compute == SVHIP_F32X3;
    for (const DevOptRow& r : kDevOpts) {       // the developer switches' defaults come from the environment, once
        const char* e = r.env ? getenv(r.env) : nullptr;
        h->opt.*r.field = !e ? r.dflt : r.parse == OPT_SET ? 1 : r.parse == OPT_IS1 ? (e[0] == '1' ? 1 : 0) : atoi(e);
    }
    h->esz = h->bf16 ? 2 : 4;
    h->T = cfg->samples / cfg->hop_length + 1;
    if (cfg->stream) { h->stream = reinterpret_cast<hipStream_t>(cfg->stream); h->own_stream = false; }
    else {
        if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) { g_create_error = hipGetErrorString(e); delete h; return SVHIP_ERR_HIP; }
        h->own_stream = true;
    }
    h->cur = h->stream;
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && ncu > 0) h->num_cu = ncu;
    }
    {
        // batch slices on separate streams, SVHIP_LANES = 1 .. 4 (default 1).  Measured at B = 256: ECAPA -1.5 .. +3.7 % with two
        // (its big GEMMs fill the chip either way); RawNet2 +3 % with two or three, -22 % with four — slices of ONE call all sit in
        // the same phase of the network, so little complements.  What does pay for RawNet2 is whole batches in flight on
        // separate handles / streams (+12 .. 21 %, bench.py `rawnet2_3_streams`): a serving-loop choice, not a library default.
        const char* le = getenv("SVHIP_LANES");
        h->lanes = le ? atoi(le) : 1;
        if (h->lanes < 1 || h->lanes > 4) h->lanes = 1;
        h->lanes = std::min(h->lanes, m->max_lanes);
        if (h->lanes > 1) {
            for (int i = 0; i < h->lanes; ++i) (void)hipStreamCreateWithFlags(&h->lane_stream[i], hipStreamNonBlocking);
            for (int i = 0; i < 5; ++i) (void)hipEventCreateWithFlags(&h->lane_ev[i], hipEventDisableTiming);
        }
    }
    int rc = build_fbank_tables(h);
    h->fb.force32 = h->opt.fbank32;
    if (rc == SVHIP_OK) rc = alloc_workspace(h);
    if (rc == SVHIP_OK && m->alloc) rc = m->alloc(h);
    if (rc != SVHIP_OK) { g_create_error = h->err; svhip_destroy(h); return rc; }
    if (!m->finalize) h->finalized = true;         // (no weights to load)
    *out = h;
    return SVHIP_OK;
}

int svhip_destroy(svhip_handle* h) {
    if (!h) return SVHIP_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->comm) (void)svhip_comm_destroy(h);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->crop_pcm) (void)hipFree(h->crop_pcm);
    if (h->aux_stream) { (void)hipStreamSynchronize(h->aux_stream); (void)hipStreamDestroy(h->aux_stream); }
    for (hipEvent_t e : h->aux_ev) if (e) (void)hipEventDestroy(e);
    for (void* q : h->scr) if (q) (void)hipFree(q);
    h->model.reset();          // (a model with ragged calls releases the pinned slots and events of its RagTables)
    for (auto& sl : h->crop_slot) {
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.dev) (void)hipFree(sl.dev);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->host_flag) (void)hipHostFree(h->host_flag);
    prof_collect(h);
    for (hipEvent_t e : h->ev_free) (void)hipEventDestroy(e);
    for (int i = 0; i < 4; ++i) if (h->lane_stream[i]) { (void)hipStreamSynchronize(h->lane_stream[i]); (void)hipStreamDestroy(h->lane_stream[i]); }
    for (int i = 0; i < 5; ++i) if (h->lane_ev[i]) (void)hipEventDestroy(h->lane_ev[i]);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SVHIP_OK;
}

int svhip_synchronize(svhip_handle* h) {
    if (!h) return SVHIP_ERR_INVALID;
    SV_HIP(h, hipStreamSynchronize(h->stream));
    return numeric_status(h, true);
}

int svhip_numeric_status(svhip_handle* h, int32_t reset) {
    if (!h) return SVHIP_ERR_INVALID;
    SV_HIP(h, hipSetDevice(h->cfg.device));
    SV_HIP(h, hipStreamSynchronize(h->stream));
    return numeric_status(h, reset != 0);
}

int svhip_load_tensor(svhip_handle* h, const char* name, const void* data, const int64_t* shape, int32_t ndim, int32_t dtype) {
    if (!h || !name || !shape || ndim < 0 || ndim > 4) return SVHIP_ERR_INVALID;
    if (!data) SV_FAIL(h, SVHIP_ERR_INVALID, "null data for %s (a 0-d tensor still holds one element)", name);
    if (h->finalized) SV_FAIL(h, SVHIP_ERR_STATE, "weights already finalized");
    const WeightSpec spec = model_spec(h);
    auto it = spec.find(name);
    if (it == spec.end()) SV_FAIL(h, SVHIP_ERR_INVALID, "%s is not in the model.", name);
    std::vector<int64_t> shp(shape, shape + ndim);
    if (shp != it->second) SV_FAIL(h, SVHIP_ERR_INVALID, "Wrong parameter shape: %s", name);
    HostTensor t;
    t.shape = shp;
    const int64_t n = t.numel();
    t.data.resize((size_t)n);
    if (dtype == SVHIP_F32) memcpy(t.data.data(), data, (size_t)n * 4);
    else if (dtype == SVHIP_I64) for (int64_t i = 0; i < n; ++i) t.data[i] = (float)reinterpret_cast<const int64_t*>(data)[i];
    else SV_FAIL(h, SVHIP_ERR_INVALID, "unsupported dtype %d for %s", dtype, name);
    h->host_w[name] = std::move(t);
    return SVHIP_OK;
}

int svhip_finalize_weights(svhip_handle* h) {
    if (!h) return SVHIP_ERR_INVALID;
    if (h->finalized) SV_FAIL(h, SVHIP_ERR_STATE, "weights already finalized");
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const ModelOps* m = model_ops(h->cfg.model);
    for (auto& kv : model_spec(h))
        if (!h->host_w.count(kv.first) && kv.first.find("num_batches_tracked") == std::string::npos &&
            !(m->optional_prefix && kv.first.rfind(m->optional_prefix, 0) == 0))
            SV_FAIL(h, SVHIP_ERR_MISSING, "tensor %s was never loaded", kv.first.c_str());
    if (!m->finalize) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "model %d has no forward path in this build", h->cfg.model);
    if (int rc = m->finalize(h)) return rc;
    SV_HIP(h, hipDeviceSynchronize());
    h->host_w.clear();
    h->finalized = true;
    return SVHIP_OK;
}

int svhip_load_blob(svhip_handle* h, const char* path) {
    if (!h || !path) return SVHIP_ERR_INVALID;
    if (h->finalized) SV_FAIL(h, SVHIP_ERR_STATE, "weights already finalized");
    svhip_blob* b = nullptr;
    if (int rc = svhip_blob_open(path, &b)) SV_FAIL(h, rc, "%s", svhip_blob_last_error());
    if (svhip_blob_model(b) != h->cfg.model) {
        const int m = svhip_blob_model(b);
        svhip_blob_close(b);
        SV_FAIL(h, SVHIP_ERR_INVALID, "%s holds weights of model %d, this handle is model %d", path, m, h->cfg.model);
    }
    const WeightSpec spec = model_spec(h);
    const int32_t n = svhip_blob_count(b);
    for (int32_t i = 0; i < n; ++i) {
        const char* name; const void* data; int64_t shape[4]; int32_t ndim, dtype;
        svhip_blob_tensor(b, i, &name, &data, shape, &ndim, &dtype);
        if (!spec.count(name)) continue;                       // e.g. loss-head tensors of a training checkpoint
        if (int rc = svhip_load_tensor(h, name, data, shape, ndim, dtype)) { svhip_blob_close(b); return rc; }
    }
    svhip_blob_close(b);
    return svhip_finalize_weights(h);
}

int svhip_fbank(svhip_handle* h, const float* wav, int32_t B, int32_t L, float* mel_out, int32_t flags) {
    if (!h || !wav || !mel_out) return SVHIP_ERR_INVALID;
    if (B <= 0 || B > h->cfg.max_batch) SV_FAIL(h, SVHIP_ERR_INVALID, "batch %d outside [1, max_batch=%d]", B, h->cfg.max_batch);
    if (L != h->cfg.samples) SV_FAIL(h, SVHIP_ERR_INVALID, "L=%d but the handle was created for %d samples", L, h->cfg.samples);
    if ((flags & SVHIP_ASYNC) && (flags & (SVHIP_IN_DEVICE | SVHIP_OUT_DEVICE)) != (SVHIP_IN_DEVICE | SVHIP_OUT_DEVICE))
        SV_FAIL(h, SVHIP_ERR_INVALID, "SVHIP_ASYNC needs device pointers");
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const float* d_in = wav;
    if (!(flags & SVHIP_IN_DEVICE)) {
        SV_HIP(h, hipMemcpyAsync(h->d_wav, wav, (size_t)B * L * 4, hipMemcpyHostToDevice, h->stream));
        d_in = h->d_wav;
    }
    float* d_out = (flags & SVHIP_OUT_DEVICE) ? mel_out : h->d_feat;
    const int T = h->T;
    int rc = run(h, "fbank", 0, [&]() { return launch_fbank(h->fb, d_in, B, L, T, d_out, h->stream); });
    if (rc) return rc;
    if (!(flags & SVHIP_OUT_DEVICE))
        SV_HIP(h, hipMemcpyAsync(mel_out, d_out, (size_t)B * h->cfg.n_mels * T * 4, hipMemcpyDeviceToHost, h->stream));
    return finish(h, flags);
}

int svhip_embed_features(svhip_handle* h, const float* feat, int32_t B, int32_t T, float* emb_out, int32_t flags) {
    int rc = check_ready(h, B);
    if (rc) return rc;
    if (!feat || !emb_out) SV_FAIL(h, SVHIP_ERR_INVALID, "null pointer");
    const ModelOps* m = model_ops(h->cfg.model);
    if (!m->embed_feat) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "embed_features needs a spectral model (ECAPA, TitaNet, Conformer, ResNetSE)");
    if (T != h->T) SV_FAIL(h, SVHIP_ERR_INVALID, "T=%d but the handle was created for T=%d frames", T, h->T);
    if ((flags & SVHIP_ASYNC) && (flags & (SVHIP_IN_DEVICE | SVHIP_OUT_DEVICE)) != (SVHIP_IN_DEVICE | SVHIP_OUT_DEVICE))
        SV_FAIL(h, SVHIP_ERR_INVALID, "SVHIP_ASYNC needs device pointers");
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const float* d_in = feat;
    if (!(flags & SVHIP_IN_DEVICE)) {
        SV_HIP(h, hipMemcpyAsync(h->d_feat, feat, (size_t)B * h->cfg.n_mels * T * 4, hipMemcpyHostToDevice, h->stream));
        d_in = h->d_feat;
    }
    h->feat_is_stale = false;
    if ((rc = m->embed_feat(h, d_in, B))) return rc;
    if ((rc = emit_embeddings(h, B, emb_out, flags))) return rc;
    return finish(h, flags);
}

int svhip_embed_wave(svhip_handle* h, const float* wav, int32_t B, int32_t L, float* emb_out, int32_t flags) {
    int rc = check_ready(h, B);
    if (rc) return rc;
    if (!wav || !emb_out) SV_FAIL(h, SVHIP_ERR_INVALID, "null pointer");
    if (L != h->cfg.samples) SV_FAIL(h, SVHIP_ERR_INVALID, "L=%d but the handle was created for %d samples", L, h->cfg.samples);
    if ((flags & SVHIP_ASYNC) && (flags & (SVHIP_IN_DEVICE | SVHIP_OUT_DEVICE)) != (SVHIP_IN_DEVICE | SVHIP_OUT_DEVICE))
        SV_FAIL(h, SVHIP_ERR_INVALID, "SVHIP_ASYNC needs device pointers");
    const ModelOps* m = model_ops(h->cfg.model);
    if (!m->embed_wave) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "model %d has no forward path in this build", h->cfg.model);
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const float* d_in = wav;
    if (!(flags & SVHIP_IN_DEVICE)) {
        SV_HIP(h, hipMemcpyAsync(h->d_wav, wav, (size_t)B * L * 4, hipMemcpyHostToDevice, h->stream));
        d_in = h->d_wav;
    }
    if ((rc = m->embed_wave(h, d_in, B))) return rc;
    if ((rc = emit_embeddings(h, B, emb_out, flags))) return rc;
    return finish(h, flags);
}

int svhip_fusion_head(svhip_handle* h, const float* e1, int32_t d1, const float* e2, int32_t d2, int32_t B, float* out, int32_t flags) {
    int rc = check_ready(h, B);
    if (rc) return rc;
    if (h->cfg.model != SVHIP_MODEL_FUSION_HEAD) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "svhip_fusion_head needs a SVHIP_MODEL_FUSION_HEAD handle, this handle is model %d", h->cfg.model);
    if (!e1 || !e2 || !out) SV_FAIL(h, SVHIP_ERR_INVALID, "null pointer");
    if (d1 < 1 || d2 < 1 || d1 + d2 != HYPE_HEAD_C) SV_FAIL(h, SVHIP_ERR_INVALID, "d1 + d2 = %d + %d, the head mixes %d channels", d1, d2, HYPE_HEAD_C);
    if ((flags & SVHIP_ASYNC) && (flags & (SVHIP_IN_DEVICE | SVHIP_OUT_DEVICE)) != (SVHIP_IN_DEVICE | SVHIP_OUT_DEVICE))
        SV_FAIL(h, SVHIP_ERR_INVALID, "SVHIP_ASYNC needs device pointers");
    SV_HIP(h, hipSetDevice(h->cfg.device));
    float* d_out = (flags & SVHIP_OUT_DEVICE) ? out : h->d_emb;
    if ((rc = fusion_head_forward(h, e1, d1, e2, d2, B, !(flags & SVHIP_IN_DEVICE), d_out))) return rc;
    if (!(flags & SVHIP_OUT_DEVICE)) SV_HIP(h, hipMemcpyAsync(out, d_out, (size_t)B * h->cfg.embed_dim * 4, hipMemcpyDeviceToHost, h->stream));
    h->lastB = 0;          // (no stages)
    return finish(h, flags);
}

int svhip_embed_wave_ragged(svhip_handle* h, const float* wav, const int64_t* offsets, const int32_t* lengths, int32_t n, float* emb_out,
                            int32_t flags) {
    return embed_ragged(kRagEcapa, h, wav, offsets, lengths, n, emb_out, flags, true);
}

int svhip_embed_features_ragged(svhip_handle* h, const float* feat, const int64_t* frame_offsets, const int32_t* frames, int32_t n,
                                float* emb_out, int32_t flags) {
    return embed_ragged(kRagEcapa, h, feat, frame_offsets, frames, n, emb_out, flags, false);
}

int svhip_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n, int32_t is_wave) {
    return ragged_check(kRagEcapa, cfg, lengths, n, is_wave != 0);
}

int svhip_rawnet3_embed_ragged(svhip_handle* h, const float* wav, const int64_t* offsets, const int32_t* lengths, int32_t n, float* emb_out,
                               int32_t flags) {
    return embed_ragged(kRagRawnet3, h, wav, offsets, lengths, n, emb_out, flags, true);
}

int svhip_rawnet3_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n) {
    return ragged_check(kRagRawnet3, cfg, lengths, n, true);
}

int svhip_rawnet2_embed_ragged(svhip_handle* h, const float* wav, const int64_t* offsets, const int32_t* lengths, int32_t n, float* emb_out,
                               int32_t flags) {
    return embed_ragged(kRagRawnet2, h, wav, offsets, lengths, n, emb_out, flags, true);
}

int svhip_rawnet2_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n) {
    return ragged_check(kRagRawnet2, cfg, lengths, n, true);
}

int svhip_conformer_embed_ragged(svhip_handle* h, const float* in, const int64_t* offsets, const int32_t* lengths, int32_t n, float* emb_out,
                                 int32_t flags, int32_t is_wave) {
    return embed_ragged(kRagConformer, h, in, offsets, lengths, n, emb_out, flags, is_wave != 0);
}

int svhip_conformer_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n, int32_t is_wave) {
    return ragged_check(kRagConformer, cfg, lengths, n, is_wave != 0);
}

int svhip_titanet_embed_ragged(svhip_handle* h, const float* in, const int64_t* offsets, const int32_t* lengths, int32_t n, float* emb_out,
                               int32_t flags, int32_t is_wave) {
    return embed_ragged(kRagTitanet, h, in, offsets, lengths, n, emb_out, flags, is_wave != 0);
}

int svhip_titanet_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n, int32_t is_wave) {
    return ragged_check(kRagTitanet, cfg, lengths, n, is_wave != 0);
}

int svhip_resnetse_embed_ragged(svhip_handle* h, const float* in, const int64_t* offsets, const int32_t* lengths, int32_t n, float* emb_out,
                                int32_t flags, int32_t is_wave) {
    return embed_ragged(kRagResnetse, h, in, offsets, lengths, n, emb_out, flags, is_wave != 0);
}

int svhip_resnetse_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n, int32_t is_wave) {
    return ragged_check(kRagResnetse, cfg, lengths, n, is_wave != 0);
}

int svhip_crop_pcm16(svhip_handle* h, const int16_t* pcm, int64_t n_samples, const int64_t* offsets, const int32_t* lengths,
                     int32_t n_files, int32_t num_eval, int32_t L, float* crops_out, int32_t flags) {
    if (!h || !pcm || !offsets || !lengths || !crops_out || n_files <= 0 || num_eval <= 0 || L <= 0 || n_samples <= 0) return SVHIP_ERR_INVALID;
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const bool din = flags & SVHIP_IN_DEVICE, dout = flags & SVHIP_OUT_DEVICE;
    if ((flags & SVHIP_ASYNC) && !dout) SV_FAIL(h, SVHIP_ERR_INVALID, "SVHIP_ASYNC needs a device output pointer");
    if (!din)      // host metadata is range-checked before it reaches the GPU
        for (int f = 0; f < n_files; ++f)
            if (lengths[f] <= 0 || offsets[f] < 0 || offsets[f] + lengths[f] > n_samples)
                SV_FAIL(h, SVHIP_ERR_INVALID, "file %d: offset/length outside the PCM buffer", f);
    const void *d_pcm = pcm, *d_off = offsets, *d_len = lengths;
    void* d_out = crops_out;
    const size_t out_bytes = (size_t)n_files * num_eval * L * 4;
    svhip_handle::CropSlot* slot = nullptr;
    if (!din) {
        // PCM: one device buffer (the copy is ordered behind the previous call's kernel on this stream); pageable host memory makes
        // the copy call itself block until the bytes are staged, pinned memory makes it truly asynchronous
        const size_t pcm_bytes = (size_t)n_samples * 2;
        if (h->crop_pcm_cap < pcm_bytes) {
            SV_HIP(h, hipStreamSynchronize(h->stream));
            if (h->crop_pcm) (void)hipFree(h->crop_pcm);
            h->crop_pcm = nullptr; h->crop_pcm_cap = 0;
            SV_HIP(h, hipMalloc(&h->crop_pcm, pcm_bytes + pcm_bytes / 4));
            h->crop_pcm_cap = pcm_bytes + pcm_bytes / 4;
        }
        // metadata: copied into a pinned slot of the handle, so the caller's arrays are free on return
        slot = &h->crop_slot[h->crop_next];
        h->crop_next = (h->crop_next + 1) & 3;
        if (slot->busy) { SV_HIP(h, hipEventSynchronize(slot->done)); slot->busy = false; }
        const size_t meta = (size_t)n_files * 12;
        if (slot->cap < meta) {
            if (slot->host) (void)hipHostFree(slot->host);
            if (slot->dev) (void)hipFree(slot->dev);
            slot->host = slot->dev = nullptr; slot->cap = 0;
            SV_HIP(h, hipHostMalloc((void**)&slot->host, meta * 2, hipHostMallocDefault));
            SV_HIP(h, hipMalloc((void**)&slot->dev, meta * 2));
            slot->cap = meta * 2;
            if (!slot->done) SV_HIP(h, hipEventCreateWithFlags(&slot->done, hipEventDisableTiming));
        }
        memcpy(slot->host, offsets, (size_t)n_files * 8);
        memcpy(slot->host + (size_t)n_files * 8, lengths, (size_t)n_files * 4);
        SV_HIP(h, hipMemcpyAsync(h->crop_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice, h->stream));
        SV_HIP(h, hipMemcpyAsync(slot->dev, slot->host, meta, hipMemcpyHostToDevice, h->stream));
        d_pcm = h->crop_pcm; d_off = slot->dev; d_len = slot->dev + (size_t)n_files * 8;
    }
    void* tmp_out = nullptr;
    if (!dout) { SV_HIP(h, hipMalloc(&tmp_out, out_bytes)); d_out = tmp_out; }
    h->cur = h->stream;
    int rc = run(h, "crop_pcm16", 0, [&]() { return launch_crop_pcm16((const int16_t*)d_pcm, (const int64_t*)d_off, (const int32_t*)d_len, n_files, num_eval, L, (float*)d_out, h->stream); });
    hipError_t e = hipSuccess;
    if (slot && !rc) { e = hipEventRecord(slot->done, h->stream); slot->busy = e == hipSuccess; }
    if (!rc && !dout && e == hipSuccess) e = hipMemcpyAsync(crops_out, d_out, out_bytes, hipMemcpyDeviceToHost, h->stream);
    if (!(flags & SVHIP_ASYNC)) { const hipError_t e2 = hipStreamSynchronize(h->stream); if (e == hipSuccess) e = e2; }
    if (tmp_out) (void)hipFree(tmp_out);
    if (rc) return rc;
    if (e != hipSuccess) SV_FAIL(h, SVHIP_ERR_HIP, "crop staging / copy failed: %s", hipGetErrorString(e));
    return SVHIP_OK;
}

int svhip_synth_waveforms(svhip_handle* h, uint64_t seed, int64_t first_utt, int32_t B, int32_t L, float* wav_out, int32_t flags) {
    if (!h || !wav_out || B <= 0 || L <= 0 || first_utt < 0) return SVHIP_ERR_INVALID;
    if (L % 4 != 0) SV_FAIL(h, SVHIP_ERR_INVALID, "L=%d must be a multiple of 4", L);
    if ((flags & SVHIP_ASYNC) && !(flags & SVHIP_OUT_DEVICE)) SV_FAIL(h, SVHIP_ERR_INVALID, "SVHIP_ASYNC needs device pointers");
    SV_HIP(h, hipSetDevice(h->cfg.device));
    float* d_out = wav_out;
    void* tmp = nullptr;
    if (!(flags & SVHIP_OUT_DEVICE)) {
        SV_HIP(h, hipMalloc(&tmp, (size_t)B * L * 4));
        d_out = reinterpret_cast<float*>(tmp);
    }
    h->cur = h->stream;
    int rc = run(h, "synth_wave", 0, [&]() { return launch_synth_wave(d_out, seed, first_utt, B, L, h->stream); });
    hipError_t e = hipSuccess;
    if (!rc && tmp) e = hipMemcpyAsync(wav_out, d_out, (size_t)B * L * 4, hipMemcpyDeviceToHost, h->stream);
    if (tmp || !(flags & SVHIP_ASYNC)) { const hipError_t e2 = hipStreamSynchronize(h->stream); if (e == hipSuccess) e = e2; }
    if (tmp) (void)hipFree(tmp);
    if (rc) return rc;
    SV_HIP(h, e);
    return SVHIP_OK;
}

// ---- introspection ---------------------------------------------------------------------------------------
int svhip_get_stage(svhip_handle* h, const char* name, float* out, int64_t* count) {
    if (!h || !name || !count) return SVHIP_ERR_INVALID;
    if (h->lastB <= 0) SV_FAIL(h, SVHIP_ERR_STATE, "no forward has run yet");
    const int B = h->lastB;
    const size_t rag_in = h->rag_levels ? (size_t)h->rag_rows[0] : 0;      // a ragged forward: the packed rows of its input level
    StageView v{nullptr, rag_in ? rag_in : (size_t)B * h->T, 0, 0, !h->bf16};
    const std::string n(name);
    if (n == "input" && h->X_in) { v.src = h->X_in; v.cols = v.ld = h->cfg.n_mels; }
    else if (n == "mel") {
        if (h->feat_is_stale) SV_FAIL(h, SVHIP_ERR_STATE, "stage mel: the last forward ran the fused front-end, which never forms the mel power "
                                      "tensor (option fbank_unfused = 1 keeps the separate kernels)");
        v.src = h->d_feat; v.rows = (size_t)B * h->cfg.n_mels; v.cols = v.ld = h->T; v.f32 = true;
        if (rag_in) { v.rows = 1; v.cols = v.ld = rag_in * h->cfg.n_mels; }      // the (n_mels, T_u) blocks back to back
    }
    else {                                    // every other name is the model's
        const ModelOps* m = model_ops(h->cfg.model);
        if (!m->stage) return unknown_stage(h, n);
        if (int rc = m->stage(h, n, out != nullptr, v)) return rc;
    }
    const size_t rows = v.rows, cols = v.cols;
    *count = (int64_t)(rows * cols);
    if (!out) return SVHIP_OK;
    SV_HIP(h, hipStreamSynchronize(h->stream));
    const size_t es = v.f32 ? 4 : 2;
    std::vector<char> tmp(rows * cols * es);
    SV_HIP(h, hipMemcpy2D(tmp.data(), cols * es, v.src, v.ld * es, cols * es, rows, hipMemcpyDeviceToHost));
    if (v.f32) memcpy(out, tmp.data(), tmp.size());
    else {
        const uint16_t* s = reinterpret_cast<const uint16_t*>(tmp.data());
        if (h->f16) for (size_t i = 0; i < rows * cols; ++i) { _Float16 hv; memcpy(&hv, &s[i], 2); out[i] = static_cast<float>(hv); }
        else for (size_t i = 0; i < rows * cols; ++i) { uint32_t u = (uint32_t)s[i] << 16; memcpy(&out[i], &u, 4); }
    }
    return SVHIP_OK;
}

int svhip_profile_enable(svhip_handle* h, int32_t on) { if (!h) return SVHIP_ERR_INVALID; h->prof = on != 0; return SVHIP_OK; }
int svhip_profile_filter(svhip_handle* h, const char* label) { if (!h) return SVHIP_ERR_INVALID; h->prof_filter = label ? label : ""; return SVHIP_OK; }
int svhip_profile_reset(svhip_handle* h) { if (!h) return SVHIP_ERR_INVALID; prof_collect(h); h->prof_entries.clear(); return SVHIP_OK; }
int svhip_profile_get(svhip_handle* h, int32_t idx, char* name, int32_t name_cap, double* ms, int64_t* launches, double* flops) {
    if (!h) return SVHIP_ERR_INVALID;
    prof_collect(h);
    if (idx < 0 || idx >= (int32_t)h->prof_entries.size()) return SVHIP_ERR_INVALID;
    const ProfEntry& p = h->prof_entries[idx];
    if (name && name_cap > 0) { strncpy(name, p.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (ms) *ms = p.ms;
    if (launches) *launches = p.launches;
    if (flops) *flops = p.flops;
    return SVHIP_OK;
}
double svhip_workload_flops(const svhip_handle* h) { return h ? h->flops_per_utt : 0.0; }

int svhip_set_option(svhip_handle* h, const char* name, int32_t value) {
    if (!h || !name) return SVHIP_ERR_INVALID;
    for (const DevOptRow& r : kDevOpts)
        if (strcmp(name, r.name) == 0) {
            h->opt.*r.field = value;
            h->fb.force32 = h->opt.fbank32;
            return SVHIP_OK;
        }
    SV_FAIL(h, SVHIP_ERR_INVALID, "unknown option %s", name);
}

// Release the scoring / metrics scratch slots (they are grown on demand and otherwise kept for the life of the handle: one slab-path
// AS-norm call or one large host-pointer call would hold gigabytes of HBM beside the model engines' workspaces).
int svhip_trim_scratch(svhip_handle* h) {
    if (!h) return SVHIP_ERR_INVALID;
    SV_HIP(h, hipSetDevice(h->cfg.device));
    SV_HIP(h, hipStreamSynchronize(h->stream));
    if (h->aux_stream) SV_HIP(h, hipStreamSynchronize(h->aux_stream));
    for (int i = 0; i < svhip_handle::SCR_COUNT; ++i)
        if (h->scr[i]) { (void)hipFree(h->scr[i]); h->scr[i] = nullptr; h->scr_cap[i] = 0; }
    return SVHIP_OK;
}

// host-only self checks (no GPU needed): the per-device one-time flag every LDS-hungry launcher keeps
int svhip_selftest(void) {
    svhip::DeviceOnce once;
    for (int d = -1; d < 66; ++d) if (once.done(d)) return 1;                 // nothing marked yet, out-of-range ordinals never are
    once.mark(0);
    if (!once.done(0) || once.done(1) || once.done(63)) return 2;            // device 0 set up says nothing about device 1
    once.mark(5); once.mark(63); once.mark(64); once.mark(-3);                // out-of-range marks are ignored
    if (!once.done(5) || !once.done(63) || once.done(64) || once.done(-3) || once.done(4)) return 3;
    once.mark(0);
    if (!once.done(0) || once.mask.load() != ((1ull << 0) | (1ull << 5) | (1ull << 63))) return 4;
    // cluster_join's seed clamp (kernels.h): whatever the entry, the result lies in [0, i] - the forest's climbs end on nothing else -
    // and a legal entry comes back as it is
    const int32_t entries[] = {INT32_MIN, INT32_MIN + 1, -2, -1, 0, 1, 2, 31, 32, 33, 1 << 20, INT32_MAX - 1, INT32_MAX};
    const int64_t places[] = {0, 1, 2, 31, 32, 33, 1 << 20, (int64_t)INT32_MAX - 1};
    for (int64_t i : places)
        for (int32_t v : entries) {
            const int32_t got = svhip::cluster_seed_parent(v, i);
            if (got < 0 || got > i) return 5;
            if (got != ((v >= 0 && v <= i) ? v : (int32_t)i)) return 6;
        }
    for (int64_t i = 0; i < 300; ++i)
        for (int32_t v = -3; v < 304; ++v) {
            const int32_t got = svhip::cluster_seed_parent(v, i);
            if (got < 0 || got > i || (v >= 0 && v <= i && got != v) || ((v < 0 || v > i) && got != i)) return 7;
        }
    return 0;
}

}  // extern "C"
