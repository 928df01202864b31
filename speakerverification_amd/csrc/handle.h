// handle.h — the handle of libsvhip and what the host-side translation units of the C ABI share (api*.hip, comm.hip): the state every
// model needs (configuration, streams, options, the common workspace, profiling, scoring scratch) and the few buffers several models
// use.  What one model alone uses — its layers, its workspace, what its last forward left where — is a struct private to its
// api_<model>.hip, derived from ModelState and owned by the handle through `model`.
// Internal: kernel translation units see kernels.h / common.h only.
#pragma once
#include "../../include/svhip.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace svhip {

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
    int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

struct ConvLayer {            // one conv1d as a GEMM operand set (device pointers)
    int N = 0, K = 0, Kp = 0, Np = 0, taps = 1, dil = 1, cin = 0;
    void* W = nullptr;        // packed [Np][Kp] in the compute dtype
    void* Wsplit = nullptr;   // SVHIP_F32X3 handles: the same matrix as (hi bf16 << 16 | lo bf16) words, for gemm_pw's split path
    float cv_wscale = 1.0f;   // ... whose planes hold cv_wscale * W (an exact power of two; 1 unless max |w| lies outside [2^-8, 2^13))
    void* Wcv = nullptr;      // SVHIP_F32X3 handles, odd-tap convolutions with N % 256 == 0 (blocks.0): [N][cv_Kp] S32, k = tap * cv_cin + c with the
    int cv_cin = 0, cv_Kp = 0; // input channels zero-padded to cv_cin (a multiple of 32) and cv_Kp = taps * cv_cin rounded up to 64: gemm_pw3's CV form
    void* Ws32 = nullptr;     // SVHIP_F32X3 handles, pointwise layers with N % 256 == 0 and K % 64 == 0: the S32 split layout (per row, per
                              // 32 k: 32 hi bf16 | 32 lo bf16) of gemm_pw3's X3 form
    float* bias = nullptr;    // [N] or null
    float* scale = nullptr;   // folded BatchNorm (eval): y = x*scale + shift, or null
    float* shift = nullptr;
    double flops_per_row = 0;
};

struct LinearLayer {          // small-M fp32 linear (rowvec kernel)
    int N = 0, K = 0;
    float* W = nullptr;       // [N][K]
    float* bias = nullptr;
};

// What one model keeps on a handle: each api_<model>.hip derives its own state struct, creates it first thing in its alloc hook and
// reaches it through its file-local accessor S(h); svhip_destroy releases it
struct ModelState { virtual ~ModelState() = default; };
// an activation buffer whose `bytes` of payload are followed by a 256-byte zero tail (api_gemm.hip's zero_page_for)
struct TailedBuf { const char* base; size_t bytes; };

// the most frame levels a ragged pack has (RawNet2: the front-end's frames and what each of its six max_pool1d(3) stages leaves)
constexpr int RAG_LEVELS = 7;

struct ProfEntry { std::string name; double ms = 0; int64_t launches = 0; double flops = 0; };
struct PendingEvent { hipEvent_t e0, e1; int entry; };

}  // namespace svhip

struct svhip_handle {
    svhip_config cfg{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t cur = nullptr;                // stream the launch helpers enqueue on (main stream or a lane)
    hipStream_t lane_stream[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t lane_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};       // [lane] done events, [4] = fork point
    int lanes = 1;                            // > 1: the forward runs as that many batch slices on as many streams
    // developer / test switches: what the call sites read.  Defaults, environment variables and names: kDevOpts (api.hip)
    struct DevOpts {
        int layer_labels;         // one profile row per GEMM shape
        int x3_keep_f32;          // F32X3: keep the fp32 copies of the block outputs beside the split layout
        int r2_big;               // F32X3: Res2Net steps on the R2 form of the 256 x 256 kernel instead of r2_step
        int asp_v1;               // bf16: asp_fused_kernel instead of asp_bf16_kernel
        int rn_unfused;           // RawNet2: the separate kernel sequence instead of rn_block128 / rn_tail / the folded shortcut
        int asnorm_slab;          // AS-norm statistics on the slab path
        int asnorm_f32mfma;       // AS-norm fused kernel on the exact fp32 MFMA instead of the split form
        int score_f32mfma;        // dense score GEMMs (svhip_score_matrix, the slab path's cohort GEMM) on the exact fp32 MFMA instead of the split form
        int score_tiled;          // dense score GEMMs on the tiled split kernel (gemm_pw) instead of the row-streaming one (score_h3w)
        int asnorm_norefit;       // AS-norm: embeddings the normal-quantile threshold does not fit go straight to the slab path (round 5's behaviour)
        int rn_sinc_full;         // RawNet2 fp16 handles: the 251-tap sinc kernel (round 5) instead of the symmetric 126-tap form
        int fbank32;              // the 32-frame front-end kernel
        int fbank_unfused;        // bf16 handles: fbank -> prologue_stats -> prologue_apply (round 5) instead of the fused front-end
        int pw3_cus;              // cap of the persistent GEMM grids (0: persistent kernels off)
        int pw3_tail_off;         // persistent 16-bit GEMMs: the last partial round as whole tiles (round 4) instead of column halves
        int cv_off;               // 16-bit handles: conv-gather GEMMs on the per-tile kernel instead of the persistent one
        int n128_off;             // bf16: asp.tdnn on gemm_pw instead of gemm_n128
        int rn_pool_off;          // F32X3 handles: conv2 of the long pooled blocks writes the un-pooled output, rn_maxpool3 pools it (tests)
        int rn_step_off;          // F32X3 handles: the 128 -> 128 blocks' convolutions on the tiled in-register-split kernel (tests)
        int rn_sinc_f32;          // F32X3 handles: the sinc front-end on the exact fp32 MFMA (tests) instead of three fp16 MFMAs per product
        int rn_tail_big;          // RawNet2 block tail: one workgroup per utterance at every batch size (tests)
        int r2_slices;            // bf16 Res2Net chain: time slices per utterance (-1: by batch size, 0 / 1: whole utterances, n: forced)
        int rn_conv_unfused;      // 16-bit RawNet2 'conv' handles: rn_conv3_front + plain rn_block128 instead of block 0 reading the waveform (tests, A/B)
        int rn_keep;              // RawNet2: copy what the forward stores (block inputs, outputs, gates, logits) for svhip_get_stage; the kernels enqueued stay the same (tests)
        int cf_keep;              // Conformer: the same for every block's steps, the pooling logits and the pooled vector before attention_norm (tests)
        int tn_keep;              // TitaNet: the same for every mega-block's steps, its SE squeeze and gate, the attention layer, the logits and the pooled vector before BN (tests)
        int rs_keep;              // ResNetSE: the same for the normalised input, every block's two convolutions, SE tile sums, gate, downsample and output, the attention layer, the logits and the pooled vector (tests)
        int linkage_lds_rows;     // cluster_linkage: the largest component whose matrix lives in LDS (2 .. SVHIP_LINKAGE_LDS_ROWS; else the default) (tests)
        int linkage_fill_only;    // cluster_linkage: build the score matrices and make no merge - every row stays its own cluster (measurements: the fill's share)
    } opt;
    bool bf16 = false;                        // 16-bit storage handle: bf16, or fp16 when `f16` is set (the flag keeps its round-1 name)
    bool f16 = false;                         // SVHIP_F16: the 16-bit type is IEEE half (RawNet2)
    int dt = svhip::DT_F32;                   // DT_F32 / DT_BF16 / DT_F16: what the element-wise launchers are told
    bool x3 = false;                          // SVHIP_F32X3: fp32 handle whose conv GEMMs run as split-bf16 MFMA triples
    bool finalized = false;
    std::string err;
    std::map<std::string, svhip::HostTensor> host_w;
    std::vector<void*> allocs;               // everything hipMalloc'ed, freed in destroy

    int T = 0;                                // frames per utterance
    int esz = 4;                              // activation element size

    // front-end tables
    svhip::FbankTables fb;
    int num_cu = 256;                         // compute units of the device

    std::unique_ptr<svhip::ModelState> model;  // the model's own layers, workspace and forward flags (its api_<model>.hip)

    // workspace (device)
    float* d_wav = nullptr;       // (Bmax, L)
    float* d_feat = nullptr;      // (Bmax, n_mels, T) mel power
    float* d_pstats = nullptr;    // (Bmax*n_mels*2)
    float* d_xscale = nullptr;    // F32X3: [0] = s, [1] = 1 / s of the network input (launch_in_scale), then 256 partial max words
    float* d_logmel = nullptr;    // fused front-end (bf16 handles): (Bmax, T, n_mels) log-mel rows before the mean is taken off
    float* d_fpart = nullptr;     //   and their per-tile column sums (Bmax, ceil(T / 64), n_mels)
    bool feat_is_stale = false;   // the last forward ran the fused front-end or read a caller's feature array: d_feat does not hold its mel
                                  // power (svhip_get_stage "mel")
    float* d_zero = nullptr;      // 256 zero bytes (DMA source for padded conv chunks)
    float *d_ones = nullptr, *d_zeros = nullptr;      // 4096 ones / zeros: stand-ins for absent per-channel vectors (GemmParams::ones / zeros)
    float* d_emb = nullptr;
    int lastB = 0;
    // the last forward when it was a ragged one (svhip_get_stage): the packed rows of each of its rag_levels frame levels (RagPack), the
    // input's first.  rag_levels = 0: a fixed-length forward
    int64_t rag_rows[svhip::RAG_LEVELS] = {};
    int rag_levels = 0;
    // shared by several models: each is allocated by the alloc / finalize hook of the models named, and null on the others' handles
    void* X_in = nullptr;         // (M, n_mels): the network input (ECAPA, TitaNet, Conformer; svhip_get_stage "input")
    float *in_w = nullptr, *in_b = nullptr;   // instance norm affine (ECAPA, Conformer)
    float* d_colsum = nullptr;    // pw2 column-sum partials, per lane: [sum | sumsq] x (tiles*4) x 3C floats (ECAPA, TitaNet)
    int64_t colsum_region = 0;    // floats per (lane, kind) region
    float* d_lin_part = nullptr;              // K-slice partials of the small-M linear layers (fc, asp_ctx) at full batches (ECAPA, RawNet2)
    size_t lin_part_per_utt = 0;
    void* s32_buf = nullptr;      // SVHIP_F32X3: the A operand of the current big GEMM in the S32 split layout (M x 3C x 4 bytes); ECAPA
                                  // allocates it, api_gemm.hip splits into it
    std::vector<svhip::TailedBuf> tailed;     // zero-tailed activation buffers (RawNet2's: the zero page of the persistent conv-gather kernel
                                  // must sit behind its A operand, within 4 GiB)
    // numeric status of the forwards since the last reset: d_status[0] = SVHIP_STATUS_* bits, [1] = non-finite embedding values,
    // [2] = input values beyond the split planes' range; host_flag (pinned, mapped) is set by the same kernels, so that a synchronous
    // call learns of a problem without a copy
    uint32_t* d_status = nullptr;
    uint32_t* host_flag = nullptr;
    uint32_t* host_flag_dev = nullptr;

    // profiling: event pairs are recorded around every launch without blocking the host and
    // resolved (hipEventElapsedTime) when results are read
    bool prof = false;
    std::string prof_filter;                  // non-empty: only launches with exactly this label are bracketed by events
    std::vector<hipEvent_t> ev_free;
    std::vector<svhip::PendingEvent> ev_pending;
    std::vector<svhip::ProfEntry> prof_entries;
    double flops_per_utt = 0;
    void* comm = nullptr;                     // RCCL communicator state, owned by comm.hip
    // svhip_crop_pcm16 staging (host-pointer calls): one grow-only device PCM buffer (copies and kernels are ordered on the
    // handle's stream) and a ring of pinned host / device metadata slots, each guarded by an event, so that SVHIP_ASYNC calls
    // can return before the copy has run
    void* crop_pcm = nullptr; size_t crop_pcm_cap = 0;
    // scoring / metrics scratch: handle-owned slots, grown on demand (no hipMalloc / hipFree per call once warm).  The scoring files
    // (api_scoring.hip, api_asnorm.hip, api_search.hip, api_audit.hip, api_metrics.hip) reach them through scoring_host.h
    enum { SCR_IN0 = 0, SCR_IN1, SCR_IN2, SCR_IN3, SCR_IN4, SCR_OUT0, SCR_OUT1, SCR_OUT2, SCR_SLAB, SCR_SPLIT, SCR_CAND, SCR_CNT, SCR_MB,
           SCR_FLAG, SCR_GATHER, SCR_WS, SCR_TOPK, SCR_IN5, SCR_COEF, SCR_IN6, SCR_IN7, SCR_COUNT };
    void* scr[SCR_COUNT] = {};
    size_t scr_cap[SCR_COUNT] = {};
    hipStream_t aux_stream = nullptr;         // second stream of the scoring entry points (candidate statistics under the next MFMA launch)
    hipEvent_t aux_ev[4] = {};
    int64_t last_asnorm_refit = 0;            // embeddings of the last call that the refit passes of the fused kernel decided (round 6)
    int last_asnorm_refit_passes = 0;
    int last_asnorm_flagged = -1;             // embeddings the fused AS-norm kernel handed to the slab path in the last call (-1: slab path)
    struct CropSlot { char* host = nullptr; char* dev = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool busy = false; };
    CropSlot crop_slot[4];
    int crop_next = 0;
};

#define SV_FAIL(h, code, ...)                                   \
    do {                                                        \
        char _b[512];                                           \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                  \
        (h)->err = _b;                                          \
        return (code);                                          \
    } while (0)

#define SV_HIP(h, expr)                                                                            \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) SV_FAIL(h, SVHIP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

namespace svhip {

hipEvent_t prof_event(svhip_handle* h);
void prof_collect(svhip_handle* h);

template <typename T>
int dev_alloc(svhip_handle* h, T** p, size_t count) {
    void* q = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) SV_FAIL(h, SVHIP_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    h->allocs.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return SVHIP_OK;
}

template <typename T>
int dev_upload(svhip_handle* h, T** p, const std::vector<T>& v) {
    int rc = dev_alloc(h, p, v.size());
    if (rc) return rc;
    if (!v.empty()) SV_HIP(h, hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return SVHIP_OK;
}

// the profiling-aware launch wrapper: every launch goes through it (event pairs around it while profiling is on)
template <typename F>
int run(svhip_handle* h, const char* label, double flops, F&& launch) {
    PendingEvent pe{nullptr, nullptr, -1};
    const bool prof = h->prof && (h->prof_filter.empty() || h->prof_filter == label);
    if (prof) {
        for (size_t i = 0; i < h->prof_entries.size(); ++i)
            if (h->prof_entries[i].name == label) { pe.entry = (int)i; break; }
        if (pe.entry < 0) { h->prof_entries.push_back(ProfEntry{label}); pe.entry = (int)h->prof_entries.size() - 1; }
        pe.e0 = prof_event(h);
        pe.e1 = prof_event(h);
        (void)hipEventRecord(pe.e0, h->cur);
    }
    hipError_t e = launch();
    if (e != hipSuccess) SV_FAIL(h, SVHIP_ERR_HIP, "launch %s failed: %s", label, hipGetErrorString(e));
    if (prof) {
        (void)hipEventRecord(pe.e1, h->cur);
        h->prof_entries[pe.entry].launches += 1;
        h->prof_entries[pe.entry].flops += flops;
        h->ev_pending.push_back(pe);
        if (h->ev_pending.size() >= 8192) prof_collect(h);
    }
    return SVHIP_OK;
}

inline void* off(void* base, size_t elems, int esz) { return reinterpret_cast<char*>(base) + elems * esz; }
inline const void* off(const void* base, size_t elems, int esz) { return reinterpret_cast<const char*>(base) + elems * esz; }

// api_weights.hip: what several models share when a handle is created and its weights are loaded — the front-end tables, the 16-bit
// and split conversions, the weight packers and the common workspace (d_wav, d_feat, status, ones / zeros)
using WeightSpec = std::map<std::string, std::vector<int64_t>>;      // the expected weight names and shapes of a model
int build_fbank_tables(svhip_handle* h);
int alloc_workspace(svhip_handle* h);
uint16_t f32_to_bf16_rne(float f);
uint32_t x3_split_word(float v);                                     // (hi plane << 16) | lo plane, x3_t of common.h
uint16_t to_h16(const svhip_handle* h, float f);                     // a weight in the handle's 16-bit storage type
const HostTensor* getw(svhip_handle* h, const std::string& name);    // a loaded tensor, or null
int needw(svhip_handle* h, const std::string& name, const HostTensor*& t);   // ... or SVHIP_ERR_MISSING "missing tensor <name>"
void spec_bn(WeightSpec& spec, const std::string& p, int64_t n);     // the five tensors of BatchNorm1d(n) `p`
// BatchNorm1d(eval, eps 1e-5) `p` as y = s x + t per channel, in double: s = gamma / sqrt(var + eps), t = beta - mean s
int bn_fold(svhip_handle* h, const std::string& p, int n, std::vector<double>& s, std::vector<double>& t);
int make_bn(svhip_handle* h, const std::string& p, int n, float** scale, float** shift);        // bn_fold as fp32 device vectors
// conv weight (N, cin, taps) columns [c_lo, c_hi) packed to [Np][Kp], k = tap * cin' + c, in the compute type (F32X3: and its split
// layouts); rn_s32: RawNet2's rule for the S32 layout of r2_step.hip's modes 1 / 2
int make_conv(svhip_handle* h, ConvLayer& L, const HostTensor& w, const std::vector<float>* bias, int dil, int c_lo = 0, int c_hi = -1,
              bool rn_s32 = false);
int make_conv(svhip_handle* h, ConvLayer& L, const std::string& wname, const std::string& bname, const std::string& bnname, int dil,
              int c_lo = 0, int c_hi = -1, bool rn_s32 = false);        // by name; bname / bnname empty: no bias / no BatchNorm epilogue
int make_linear(svhip_handle* h, LinearLayer& L, const std::string& wname, const std::string& bname, int c_lo = 0, int c_hi = -1);
int upload_f32(svhip_handle* h, const std::string& name, float** dst);
int upload_h16(svhip_handle* h, const std::vector<float>& m, void** dst);      // as bf16
int actbuf(svhip_handle* h, void** dst, size_t elems);               // an activation buffer: elems in the storage type, 256 spare bytes

// One row per model id (kModels, api.hip): everything outside a model's own file needs to know about it.  Null entries: the model has
// no such step.
struct StageView { const void* src; size_t rows, cols, ld; bool f32; };   // svhip_get_stage: rows x cols at row stride ld
using CheckFn = int(const svhip_config& c, const char*& err);       // svhip_create's rules for the model: SVHIP_OK, or a code and err
using SpecFn = void(const svhip_config& c, WeightSpec& spec);
using HandleFn = int(svhip_handle* h);
using EmbedFn = int(svhip_handle* h, const float* in, int B);       // device input (B, L) or (B, n_mels, T) -> h->d_emb
using StageFn = int(svhip_handle* h, const std::string& name, bool fill, StageView& v);     // fill: the caller reads the data next
// A ragged pack: utterance u is lengths[u] long (samples, is_wave; else mel frames).  RaggedCheckFn: the model's own rules — with n = 0 those on
// the configuration alone, else also those on every utterance in index order and on the pack's rows; the caller has checked the scope and n.
// RaggedEmbedFn: the forward -> h->d_emb after those rules passed; utterance u starts at in + in_off[u] (samples of a waveform array;
// frames of a feature array of (n_mels, T_u) blocks), a device array or with in_host a host one
using RaggedCheckFn = int(const svhip_config& c, const int32_t* lengths, int n, bool is_wave, std::string& err);
using RaggedEmbedFn = int(svhip_handle* h, const float* in, bool in_host, bool is_wave, const int64_t* in_off, const int32_t* lengths, int n);
struct ModelOps {
    int model;
    CheckFn* check;
    SpecFn* spec;
    HandleFn *finalize, *alloc;              // alloc: creates h->model, then the model's part of the workspace; runs at create, before finalize
    EmbedFn *embed_wave, *embed_feat;        // embed_feat: from the mel power; null for a waveform model
    StageFn* stage;
    int max_lanes;                           // cap of SVHIP_LANES
    const char* optional_prefix;             // spec names that finalize may find absent (it checks them itself)
    RaggedCheckFn* ragged_check;             // utterances of different lengths in one call: null for a model without a ragged forward
    RaggedEmbedFn* embed_ragged;
};
int unknown_stage(svhip_handle* h, const std::string& name);         // SVHIP_ERR_INVALID "unknown stage <name>"

// api.hip: the options that keep what a forward stored on its way (rn_keep, cf_keep, tn_keep, rs_keep).  A model's state holds one KeptStages: copies of
// what the forward stored, by stage name, `rows` per utterance or, after a ragged forward, the packed rows of all its utterances
// (`packed`); `cap`: the buffer's bytes.  A stage counts as kept when every utterance of the last forward (`epoch`, which the forward
// advances before its first copy) wrote it.
struct KeptStages {
    struct Kept { void* buf = nullptr; size_t rows = 0, cols = 0; bool f32 = false; uint64_t epoch = 0; int utts = 0; bool packed = false; size_t cap = 0; };
    std::map<std::string, Kept> kept;
    uint64_t epoch = 0;
};
// Copy `nrows` x `cols` values the forward has just stored — in the handle's type, in fp32 (KEEP_F32) or in the S32 layout (KEEP_S32,
// kept as fp32) — to rows [row0, row0 + nrows) of stage `name`, on the forward's stream, for `utts` utterances.  A fixed-length forward
// counts `rows` per utterance and fills a buffer of max_batch utterances slice by slice; a ragged one (`packed`) keeps the `rows`
// packed rows of a level at once.  The buffer holds `cap_rows` rows and grows when a call needs more.  The caller reads its option
// first; nothing else does: the kernels enqueued, their operands and their routes are those of a forward without it.
enum { KEEP_DT, KEEP_F32, KEEP_S32 };
int keep_stage(svhip_handle* h, KeptStages& ks, hipStream_t st, const std::string& name, const void* src, int kind, size_t rows, bool packed,
               size_t cap_rows, int cols, size_t row0, size_t nrows, int utts);
// svhip_get_stage of a kept stage after a forward of B utterances; option / option_on: the model's option, for SVHIP_ERR_STATE's text
int kept_view(svhip_handle* h, const KeptStages& ks, const std::string& name, int B, const char* option, bool option_on, StageView& v);

// api_ragged.hip: what the ragged calls of the models share on the host
int refuse(std::string& err, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));      // err = the text; returns code
// the running row sum of a pack after utterance i against the handle's rows (frames_name: what max_batch multiplies in the text)
int rag_rows_fit(std::string& err, int i, int64_t rows, int64_t cap, const char* frames_name);
// in int64: a length near INT32_MAX at hop_length 1 must reach the capacity rule, not wrap
inline int64_t mel_frames(const svhip_config& c, int64_t len, bool is_wave) { return is_wave ? len / c.hop_length + 1 : len; }
// The tables of a ragged call: one device block (layout: rag_view, api_ragged.hip), a ring of four pinned host copies of it, each
// guarded by an event (an SVHIP_ASYNC call returns before the copy has run, and the caller's arrays are free on return), the device
// utt table of every frame level and the device staging buffer of host-pointer waveforms.  One per model state; the device memory is
// the handle's (dev_alloc)
struct RagSlot { char* host = nullptr; hipEvent_t done = nullptr; bool busy = false; };
struct RagTables {
    char* dev = nullptr;
    float* wav = nullptr;
    int* utt[RAG_LEVELS] = {};
    RagSlot slot[4], *cur = nullptr;
    int next = 0;
    int alloc(svhip_handle* h, size_t table_bytes, size_t wav_floats);      // once per handle (later calls do nothing)
    int acquire(svhip_handle* h, char** host);          // the next pinned copy to fill, after a wait if its last call's copy has not run yet
    int commit(svhip_handle* h, size_t bytes);          // its first `bytes` to `dev` on the handle's stream; it is busy until that copy has run
    ~RagTables();
};
// One frame level of a pack: utterance u owns the rows [row0[u], row0[u + 1]), utt[m] is the utterance of row m, M rows in all and maxT in
// the longest utterance.  row0 / utt are device tables (utt: the forward fills it from row0, launch_rag_rows); hrow0 is row0 in the call's
// pinned slot, for what slices the pack while enqueueing (readable until the ring hands the slot out again, four calls later)
struct Seg { const int* row0 = nullptr; int* utt = nullptr; const int* hrow0 = nullptr; int M = 0, maxT = 0; };
// A pack as a forward sees it: n utterances at `levels` frame levels, lv[0] the input's.  in + off[u] (device tables off / len) is
// utterance u's first element — of its (n_mels, T_u) block of mel power, or of its len[u] samples for a waveform model
struct RagPack { int n = 0, levels = 0; Seg lv[RAG_LEVELS]; const int64_t* off = nullptr; const int32_t* len = nullptr; const float* in = nullptr; };
// How a model packs: the frames of one utterance at each of its levels, and whether its input is the mel power (rag_mel_input; staging
// slack hop_length floats per utterance) or the waveform itself (staged as it is, off / len for the front-end kernel; slack 16 floats)
struct RagRule { int levels; void (*frames)(const svhip_config& c, int64_t len, bool is_wave, int T[RAG_LEVELS]); bool mel; };
// The host side of a ragged forward, after the model's check has passed: allocates on the handle's first ragged call (utt_cap: the
// rows of each level's utt table; 0: nothing reads that level's), takes a table slot, lays out the pack (all four models: offsets
// max_batch x int64 | lengths max_batch x int32 | one row0 of max_batch + 1 ints per level), stages the input, enqueues the table
// upload and fills pk for the model's forward
int rag_pack(svhip_handle* h, RagTables& rag, const RagRule& rule, const size_t utt_cap[RAG_LEVELS], const float* in, bool in_host, bool is_wave,
             const int64_t* in_off, const int32_t* lengths, int n, RagPack& pk);
// that forward has run: what svhip_get_stage needs of it
inline void set_rag_rows(svhip_handle* h, const RagPack& pk) {
    h->lastB = pk.n;
    h->rag_levels = pk.levels;
    for (int l = 0; l < pk.levels; ++l) h->rag_rows[l] = pk.lv[l].M;
}
// What the packs of the three mel models must all pass, in this order: the configuration (hop_length, max_batch, samples >= n_fft and
// the model's cfg_extra_ok; cfg_names ends the text), every waveform n_fft samples, every utterance min_frames frames (why: the text's
// explanation, "" or " (...)"), the model's further rules on an utterance of T frames (more with its own figure `bound`, or null), the
// running row sum, in which an utterance counts as its frames rounded up to a multiple of row_unit (ResNetSE: 8, which keeps every
// subsampled level of the pack within the handle's rows; the others: 1)
using RagUttRule = int(int64_t bound, int i, int64_t T, std::string& err);
int rag_mel_check(const svhip_config& c, const int32_t* lengths, int n, bool is_wave, std::string& err, bool cfg_extra_ok, const char* cfg_names,
                  int min_frames, const char* why, RagUttRule* more = nullptr, int64_t bound = 0, int row_unit = 1);

// api_gemm.hip: the GEMM of one conv layer.  conv_plan is the one place that decides its kernel: conv_gemm launches what it returns,
// and the producers of an operand ask it too, so that they write the layout that kernel reads.
struct GemmPlan {
    GemmParams q;                     // the parameters of the launch
    bool x3 = false;                  // gemm_pw3x3 (F32X3, S32 operands); otherwise launch_gemm, which takes `route`
    GemmRoute route = ROUTE_GENERIC;
    bool side = false;                // the launch writes the side outputs (GemmParams::side_*)
    int colsum_groups = 0;            // ... and column-sum partials with this many row groups per tile (0: none)
    double flops = 0;
    char label[96] = "";              // profile label: names the kernel instance (one label == one kernel symbol in a rocprofv3 trace)
};
GemmParams conv_params(const svhip_handle* h, const ConvLayer& L, const void* A, int lda, void* Y, int ldy, int M, int T);
GemmPlan conv_plan(const svhip_handle* h, const ConvLayer& L, GemmParams p, const void* A_s32 = nullptr, int lda_s32 = 0);
int conv_gemm(svhip_handle* h, const ConvLayer& L, const GemmParams& p, const void* A_s32 = nullptr, int lda_s32 = 0, GemmPlan* plan = nullptr);

// api.hip: a forward over the utterances [b0, b0 + B) of the call, enqueued on h->cur, as `lanes` batch slices
using ForwardPart = int (*)(svhip_handle* h, const float* in, int b0, int B);
int forward_lanes(svhip_handle* h, ForwardPart part, const float* in, int B, int lanes, int per);

// api_ecapa.hip, api_rawnet2.hip (the three RawNet2 models; ragged packs of the 'conv' one), api_rawnet3.hip, api_titanet.hip, api_conformer.hip, api_resnetse.hip: each
// model's functions (its state struct stays inside its file)
CheckFn ecapa_check, rawnet2_check, rawnet3_check, titanet_check, conformer_check, resnetse_check;
SpecFn ecapa_spec, rawnet2_spec, rawnet3_spec, titanet_spec, conformer_spec, resnetse_spec;
HandleFn ecapa_finalize, rawnet2_finalize, rawnet3_finalize, titanet_finalize, conformer_finalize, resnetse_finalize;
HandleFn ecapa_alloc, rawnet2_alloc, rawnet3_alloc, titanet_alloc, conformer_alloc, resnetse_alloc;
EmbedFn ecapa_embed_wave, rawnet2_forward, rawnet3_forward;                    // from the waveform
EmbedFn ecapa_forward, titanet_forward, conformer_forward, resnetse_forward;   // from the mel power
StageFn ecapa_stage, rawnet2_stage, rawnet3_stage, titanet_stage, conformer_stage, resnetse_stage;
// api_fusionhead.hip: the attention head of Raw_ECAPA_hype, a handle kind without a waveform model (no embed hooks, no stages)
CheckFn fusion_head_check;
SpecFn fusion_head_spec;
HandleFn fusion_head_finalize, fusion_head_alloc;
int fusion_head_forward(svhip_handle* h, const float* e1, int d1, const float* e2, int d2, int B, bool in_host, float* d_out);

}  // namespace svhip
