/*
 * svhip.h — C ABI of the MI355X-native speaker-embedding + scoring hot path (libsvhip.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / C++ types.
 * Every entry point names the reference interface it replaces (paths relative to the reference
 * checkout, hiimmuc/SpeakerVerification).  The reference is pure Python, so the "FFI" a maintainer
 * adds is a ctypes binding — see INTEGRATION.md and speakerverification_amd/_lib.py.
 *
 * Conventions
 *   - every function returns an svhip_status (0 = ok, negative = error) and never throws;
 *     svhip_last_error(h) returns the message of the last failing call on that handle.
 *   - one handle = one HIP device + one HIP stream + one model's device weights + workspace.
 *     Handles are thread-compatible, not thread-safe (one host thread per handle).
 *   - the caller owns every buffer it passes.  `flags` says where they live:
 *     SVHIP_IN_DEVICE / SVHIP_OUT_DEVICE mark device pointers; otherwise host pointers are
 *     staged through the handle's own device buffers.  With SVHIP_ASYNC the call returns after
 *     enqueueing on the handle's stream (device pointers only); otherwise it synchronises.
 *   - activations inside the library are frame-major (B, T, C); the boundary keeps the
 *     reference's layouts: waveforms (B, L) fp32, features (B, n_mels, T) fp32, embeddings
 *     (B, nOut) fp32, all contiguous.
 */
#ifndef SVHIP_H
#define SVHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVHIP_ABI_VERSION 5

typedef struct svhip_handle svhip_handle;

typedef enum svhip_status {
    SVHIP_OK = 0,
    SVHIP_ERR_INVALID = -1,     /* bad argument / shape */
    SVHIP_ERR_HIP = -2,         /* a HIP runtime call failed */
    SVHIP_ERR_STATE = -3,       /* call order violated (e.g. embed before finalize) */
    SVHIP_ERR_NOMEM = -4,
    SVHIP_ERR_UNSUPPORTED = -5,
    SVHIP_ERR_MISSING = -6,     /* a required weight tensor was never loaded */
    SVHIP_ERR_NONFINITE = -7,   /* the call completed and wrote its embeddings, but some of them are inf / NaN: an fp16 activation
                                   overflowed (SVHIP_F16 stores activations as IEEE half: 65504), or the input was not finite */
    SVHIP_ERR_RANGE = -8        /* the call completed, but input values left the range the handle's arithmetic represents (SVHIP_F32X3:
                                   operands travel as IEEE-half hi | lo planes, |x| <= 65504): such values become inf in the planes and the
                                   embeddings come out non-finite */
} svhip_status;

/* SVHIP_MODEL_RAWNET2: front_proc='sinc' (LayerNorm + sinc filters + first_bn; L fixed by the LayerNorm, >= 2438 samples).
 * SVHIP_MODEL_RAWNET2_CONV (added under ABI v5): front_proc='conv' — conv1 = Conv1d(1, 128, 3, stride=3) with bias straight on the
 * waveform (RawNet2_custom.py:45-52,166-169), the same residual stack and aggregate='asp', att_dim=128 behind it; any L >= 2187
 * (floor(L / 3) frames pass six max_pool1d(3) stages), one handle per L like every model.  Weights: conv1.* instead of ln.*,
 * first_conv.* and first_bn.* (140 tensors).
 * SVHIP_MODEL_RAWNET3 (added under ABI v5): RawNet3.MainModel with its defaults, the RawNet3 branch of Raw3_ECAPA (models/RawNet3.py,
 * RawNet_baseline.py:27-159): pre-emphasis + InstanceNorm1d(1) + ParamSincFB(256, 251, stride 10) + log + time-mean front-end, three
 * Bottle2neck layers (C = 1024, scale 8, dilations 2 / 3 / 4, max-pools 5 / 3 / none), layer4 (3072 -> 1536), context attentive
 * statistics pooling with one attention logit per frame, bn5 and fc6.  embed_dim = nOut, samples = L (any L >= 541: T0 = (L - 251) / 10 + 1
 * frames, T0 / 5 / 3 >= 2 frames reach the pooling, whose unbiased variance needs two); channels 0 or 1024; compute SVHIP_F32 (the
 * filterbank sums in fp64) or SVHIP_BF16 only.  Weights: the 234 names of its state dict (bn1.*, bn6.* and preprocess.0.flipped_filter
 * included; bn1 and bn6 are not used by the forward, the filters are built from conv1.filterbank.{low_hz_, band_hz_, window_, n_}).
 * SVHIP_MODEL_RAWNET2_GRU (added under ABI v5): front_proc='sinc', aggregate='gru' — RawNet2_custom.MainModel's defaults and the RawNet2
 * branch of Raw_ECAPA_sinc_gru: the sinc front-end and residual stack of SVHIP_MODEL_RAWNET2, then lrelu(bn_before_gru(x)), a one-layer
 * GRU (input 512, hidden 1024, h0 = 0; RawNet2_custom.py:196-207) whose last state feeds fc_after_gru.  L >= 2438 samples; compute
 * SVHIP_F32, SVHIP_F32X3, SVHIP_F16 or SVHIP_BF16.  Weights: the 144 names of its state dict (fc.* is part of it and is not used).
 * SVHIP_MODEL_TITANET (added under ABI v5): TitaNet.MainModel (models/TitaNet.py, blocks/titanet_blocks.py), the spectral branch of
 * Tita_ECAPA and Raw_tita: on the mel POWER spectrogram (no log, no normalisation), prolog Conv1d(n_mels, H, 3) + BN + ReLU, n mega-blocks
 * of three depthwise-separable sub-blocks (depthwise k, pointwise H -> H, BN, ReLU) + squeeze-excitation (H / 16) + a 1 x 1 BN'd skip,
 * epilog 1 x 1 H -> 1536 + BN + ReLU, attentive statistics pooling (hidden 128, eps 1e-6) + BN(3072), Linear(3072, nOut) + BN(nOut).
 * channels = H in {256, 512, 1024}, which fixes the depthwise kernel at 3, 7 and 11 (sizes s / m / l); embed_dim = nOut; log_input =
 * input_norm = 0; compute SVHIP_F32 or SVHIP_BF16 (others: SVHIP_ERR_UNSUPPORTED).  Weights: the reference state-dict names (encoder.prolog.*,
 * encoder.mega_blocks.<i>.*, encoder.epilog.*, decoder.*) for block indices 0 .. SVHIP_TITANET_MAX_BLOCKS - 1; svhip_finalize_weights takes
 * the block count from the indices loaded contiguously from 0 (a gap or a missing tensor of a present block: SVHIP_ERR_MISSING; a depthwise
 * weight whose kernel size is not H's: SVHIP_ERR_INVALID).  Both svhip_embed_wave (mel front-end, then the net) and svhip_embed_features. */
#define SVHIP_TITANET_MAX_BLOCKS 32
/* SVHIP_MODEL_CONFORMER (added under ABI v5): Conformer.MainModel (models/Conformer.py with models/conformer/conformer/*), the model of
 * yaml/model_plot.yaml: on the mel power, log(x + 1e-6) - mean_t (log_input = 1 for features='melspectrogram', else 0) and
 * InstanceNorm1d(n_mels, affine) (input_norm must be 1); Conv2dSubampling (two Conv2d(3 x 3, stride 2) + ReLU, 256 channels) and
 * Linear(256 F2, 256); six Conformer blocks (d_model 256, 4 heads, FF x 4, depthwise kernel 15; eval: dropouts are identities); attentive
 * statistics pooling with the variance clamped to [1e-4, 1e4], attention_norm, fc = Conv1d(512, nOut, 1).  Multi-head attention uses
 * Transformer-XL relative positions, and the reference's _relative_shift (cat / view, attention.py:110-118) is reproduced exactly:
 * key j of query i takes the positional score of query row i + 1 when j >= i + 2, zero when j == i + 1.
 * channels 0 or 256; embed_dim = nOut; n_mels >= 7 (a multiple of 8, as for every model); compute SVHIP_F32 or SVHIP_BF16 (others:
 * SVHIP_ERR_UNSUPPORTED).  Length: T = L / hop + 1 >= 7 frames (T' = ((T - 3) / 2 + 1 - 3) / 2 + 1 >= 1) and T' <= 10000, the length of the
 * positional-encoding buffer (svhip_create refuses longer inputs); L >= n_fft as for every model.  Weights: the 278 reference state-dict
 * names, positional_encoding.pe (1, 10000, 256) of every layer included; asp.* / asp_bn.* are required and ignored (the reference never
 * calls them).  Both svhip_embed_wave and svhip_embed_features.
 * SVHIP_MODEL_RESNETSE (added under ABI v5): ResNetSE34V2.MainModel (models/ResNetSE34V2.py, ResNetBaseline.py:141-301, ResNetBlocks.py), the
 * 2-D "Fast ResNet" baseline: on the mel power, log(x + 1e-6) - mean_t (log_input = 1 for features='melspectrogram', else 0) and
 * InstanceNorm1d(n_mels) without affine (input_norm must be 1); Conv2d(1, 32, 3) with bias -> ReLU -> BatchNorm; four stages of 3 / 4 / 6 / 3
 * SEBasicBlockV2 at 32 / 64 / 128 / 256 channels, stages 2 - 4 opening with stride (2, 2) and a 1 x 1 BN'd downsample (the block's in-place
 * ReLU makes the residual relu(x)); squeeze-excitation with 16 hidden units; attention Conv1d(256 n_mels / 8, 128) -> ReLU -> BN ->
 * Conv1d(128, 256 n_mels / 8) -> softmax over frames; weighted mean and sqrt(clamp(weighted variance, 1e-5)); fc.  channels selects the
 * pooling: 0 or 2 = encoder_type 'ASP' (mean | std, fc reads 512 n_mels / 8 values), 1 = 'SAP' (mean only); embed_dim = nOut; n_mels a
 * multiple of 8 (as for every model); compute SVHIP_F32 or SVHIP_BF16 (others: SVHIP_ERR_UNSUPPORTED).  Length: T = L / hop + 1 >= 2 frames
 * and L >= n_fft as for every model.  Weights: the 292 reference state-dict names.  Both svhip_embed_wave and svhip_embed_features.
 * SVHIP_MODEL_FUSION_HEAD (added under ABI v5): the attention head of Raw_ECAPA_hype (models/Raw_ECAPA_hype.py:34-45,65-86), which mixes the
 * 704-d concatenation of its two branch embeddings: lrelu_0.3(bn_before_agg(.)), channel attention Conv1d(704, 128, 1) -> SiLU -> BatchNorm ->
 * Conv1d(128, 704, 1) -> softmax over the 704 channels, weighted mean | std (variance clamped at 1e-9), bn_final, fc.  Like SVHIP_MODEL_NONE
 * the handle has no waveform model: svhip_embed_* return SVHIP_ERR_UNSUPPORTED, its one forward is svhip_fusion_head.  channels = 704
 * (anything else: SVHIP_ERR_INVALID); embed_dim = nOut >= 1; the arithmetic is fp32 whatever `compute` says.  Weights: the 21 reference
 * state-dict names bn_before_agg.*, attention.0.{weight (128, 704, 1), bias}, attention.2.*, attention.3.{weight (704, 128, 1), bias},
 * bn_final.* (1408), fc.{weight (nOut, 1408), bias}. */
enum { SVHIP_MODEL_ECAPA = 0, SVHIP_MODEL_RAWNET2 = 1, SVHIP_MODEL_NONE = 2 /* fbank + scoring only */, SVHIP_MODEL_RAWNET2_CONV = 3,
       SVHIP_MODEL_RAWNET3 = 4, SVHIP_MODEL_RAWNET2_GRU = 5, SVHIP_MODEL_TITANET = 6, SVHIP_MODEL_CONFORMER = 7, SVHIP_MODEL_RESNETSE = 8,
       SVHIP_MODEL_FUSION_HEAD = 9 };
enum { SVHIP_F32 = 0, SVHIP_BF16 = 1, SVHIP_I64 = 2, SVHIP_F32X3 = 3 /* compute only */, SVHIP_F16 = 4 /* compute only */ };
enum { SVHIP_IN_DEVICE = 1, SVHIP_OUT_DEVICE = 2, SVHIP_ASYNC = 4 };

typedef struct svhip_config {
    int32_t struct_size;    /* = sizeof(svhip_config), for ABI evolution */
    int32_t model;          /* SVHIP_MODEL_* */
    int32_t compute;        /* SVHIP_F32: fp32 MFMA, 1e-4 parity path; SVHIP_BF16: bf16 MFMA, fp32 accumulate;
                               SVHIP_F32X3: fp32 storage and arithmetic everywhere except the convolution GEMMs, whose products are three
                               fp16 MFMAs on operands split into IEEE-half hi | lo parts (11 + 11 significant bits: 2^-23 relative while
                               |x| >= 2^-3, at most 2^-25 absolute below that): 1e-4 parity at ~3x the fp32 speed.  RANGE CONTRACT: an operand
                               of such a GEMM must satisfy |x| <= 65504 (the conversion to the planes is the plain one: beyond that hi is inf
                               and the embeddings come out inf / NaN).  Activations behind a BatchNorm are O(10); the network INPUT is checked on every
                               call (SVHIP_ERR_RANGE), the embeddings are checked for inf / NaN on every call (SVHIP_ERR_NONFINITE);
                               SVHIP_F16 (RawNet2 handles only): fp16 storage + fp16 MFMA, fp32 accumulate — the same speed as bf16 with
                               three more mantissa bits (RawNet2's un-normalised residual stack loses two digits to bf16 WEIGHT rounding);
                               an fp16 value overflows at 65504: on SVHIP_MODEL_RAWNET2 the input is LayerNorm'ed, so only the weights decide
                               the activation scale; on SVHIP_MODEL_RAWNET2_CONV the input is NOT LayerNorm'ed, so the waveform's scale and the
                               weights both decide whether an fp16 activation overflows (reported as SVHIP_ERR_NONFINITE like any other) */
    int32_t device;         /* HIP device ordinal */
    int32_t channels;       /* ECAPA C (channels = [C,C,C,C,3C], ECAPA_TDNN.py:378) */
    int32_t n_mels;         /* 80 */
    int32_t embed_dim;      /* nOut: 192 (ECAPA) / 320 (RawNet2) */
    int32_t max_batch;      /* workspace is sized for max_batch utterances per call */
    int32_t samples;        /* L: samples per utterance (32000); fixes T = L/hop + 1 of the fixed-length calls and the row capacity max_batch * T of the ragged ones */
    int32_t log_input;      /* ECAPA: 1 = features=='melspectrogram' -> log(x+1e-6) - mean_t (ECAPA_TDNN.py:473-476) */
    int32_t input_norm;     /* ECAPA: InstanceNorm1d(n_mels, affine) (ECAPA_TDNN.py:406-409,477-478) */
    /* mel front-end — defaults of models/FeatureExtraction/feature.py:66-71.  Served: an even n_fft <= 574, win_length % 8 == 0,
       win_length <= n_fft, hop_length % 4 == 0 and a hop whose 32-frame tile (31 hops + one window of samples) fits a workgroup's
       LDS; anything else is refused by svhip_create (SVHIP_ERR_UNSUPPORTED, the geometry in the message), never at a launch */
    int32_t fb_sr;          /* 8000 */
    int32_t n_fft;          /* 512 */
    int32_t win_length;     /* 200 */
    int32_t hop_length;     /* 80 */
    float   fmin;           /* 0 */
    float   fmax;           /* <=0 -> sr/2 */
    float   preemph;        /* 0.97; <0 disables pre-emphasis */
    void*   stream;         /* optional hipStream_t to enqueue on (NULL: the handle creates its own) */
    int32_t sinc_sr;        /* added under ABI v5: the sample rate of RawNet2's sinc front-end (SincConv_fast's sample_rate, RawNet2_custom.py:55-67:
                               n_ = 2 pi arange(-125, 0) / sinc_sr and the clamp high <= sinc_sr / 2); 16000 by default, 0 means 16000; svhip_create
                               refuses a negative value and sinc_sr / 2 <= 100 (min_low_hz + min_band_hz) with SVHIP_ERR_INVALID */
} svhip_config;

/* Fill *cfg with the reference defaults (ECAPA C=1024, fp32, 80 mels, nOut 192, L=32000). */
void svhip_default_config(svhip_config* cfg);
int  svhip_abi_version(void);

/* Lifetime.  Replaces: SpeakerEncoder.__init__ building compute_features + __S__ on a device
 * (src/model.py:61-73).  */
int svhip_create(const svhip_config* cfg, svhip_handle** out);
int svhip_destroy(svhip_handle* h);
const char* svhip_last_error(const svhip_handle* h);   /* h may be NULL: last create() error */
int svhip_synchronize(svhip_handle* h);      /* also reports (and clears) the numeric status of the asynchronous calls it waited for */
/* Numeric status of the forwards since the last reset.  Every forward checks (a) its embeddings for inf / NaN (in the kernel that writes
 * them out) and (b), on SVHIP_F32X3 handles, its input features against the split planes' range.  A synchronous call returns
 * SVHIP_ERR_NONFINITE / SVHIP_ERR_RANGE itself (after writing its outputs); after SVHIP_ASYNC calls ask here (waits for the stream) or
 * call svhip_synchronize.  reset != 0 clears the status.  Returns SVHIP_OK, SVHIP_ERR_NONFINITE or SVHIP_ERR_RANGE (message: last_error). */
int svhip_numeric_status(svhip_handle* h, int32_t reset);

/* Weights.  Replaces: ModelHandling.loadParameters' name-matched state_dict copy
 * (src/model.py:718-746).  `name` is the reference state_dict key of the __S__ module (e.g.
 * "blocks.1.tdnn1.conv.conv.weight"); data is host memory, dtype SVHIP_F32 or SVHIP_I64
 * (num_batches_tracked, ignored).  Unknown names return SVHIP_ERR_INVALID, shape mismatches too —
 * the Python shim decides whether to skip them as the reference does.  finalize folds BatchNorm
 * into scale/shift, packs conv weights [N][tap][cin] (bf16 copy for the bf16 path), bakes the
 * sinc filters (RawNet_baseline.py:339-357) and uploads everything. */
int svhip_load_tensor(svhip_handle* h, const char* name, const void* data,
                      const int64_t* shape, int32_t ndim, int32_t dtype);
int svhip_finalize_weights(svhip_handle* h);

/* Feature front-end.  Replaces: compute_features(inp) = Sequential(PreEmphasis, nnAudio
 * MelSpectrogram) (models/FeatureExtraction/feature.py:66-94, src/utils.py:53-71;
 * call site src/model.py:112-113).  wav (B, L) fp32 -> mel power (B, n_mels, T) fp32,
 * T = L / hop + 1. */
int svhip_fbank(svhip_handle* h, const float* wav, int32_t B, int32_t L, float* mel_out, int32_t flags);

/* Model forward.  Replaces: self.__S__.forward(inp) (src/model.py:119-121) ==
 * ECAPA_TDNN.forward (models/ECAPA_TDNN.py:460-502) on features (B, n_mels, T) — T >= 5: block 3 reflect-pads 4 frames (a shorter
 * L is refused at svhip_create with SVHIP_ERR_INVALID) — or
 * RawNet2.forward (models/RawNet2_custom.py:161-227) on waveforms (B, L).  emb_out (B, nOut) fp32
 * (the Python shim applies the reference's squeeze()). */
int svhip_embed_features(svhip_handle* h, const float* feat, int32_t B, int32_t T, float* emb_out, int32_t flags);
/* Fused waveform -> embedding: SpeakerEncoder.forward with label=None (src/model.py:104-125):
 * compute_features then __S__.forward (ECAPA), or __S__.forward directly (RawNet2). */
int svhip_embed_wave(svhip_handle* h, const float* wav, int32_t B, int32_t L, float* emb_out, int32_t flags);

/* The fusion head of Raw_ECAPA_hype (added under ABI v5; SVHIP_MODEL_FUSION_HEAD handles only, others: SVHIP_ERR_UNSUPPORTED).  Replaces
 * models/Raw_ECAPA_hype.py:65-85 in eval mode: out (B, nOut) fp32 from the two branch embeddings e1 (B, d1) and e2 (B, d2), d1 + d2 == 704
 * and 1 <= B <= max_batch (else SVHIP_ERR_INVALID).  The two inputs are separate pointers: no concatenated copy is made.  e1 / e2 / out
 * follow `flags` like svhip_embed_wave (SVHIP_IN_DEVICE covers both inputs; SVHIP_ASYNC needs device pointers).  One kernel launch (profile
 * label "hype_head"), fp32 on every handle; the kernel that writes `out` checks it for inf / NaN (SVHIP_ERR_NONFINITE, as after any forward).
 * BATCH INVARIANCE: a row's output is bit for bit the same whatever B is and wherever the row sits in the batch. */
int svhip_fusion_head(svhip_handle* h, const float* e1, int32_t d1, const float* e2, int32_t d2, int32_t B, float* out, int32_t flags);

/* Ragged batches (added under ABI v5): n utterances of DIFFERENT lengths, packed back to back, embedded by one call on one handle, each
 * exactly as if it had been forwarded alone at its own length — whole-file evaluation (num_eval = 0: loadWAV returns the entire file,
 * src/processing/audio_loader.py:144-145, and evaluateFromList runs one forward per file, src/model.py:386-394) without a handle per length.
 *   wave     : utterance i is wav[offsets[i] .. offsets[i] + lengths[i]); T_i = lengths[i] / hop + 1 frames.
 *   features : utterance i is an (n_mels, frames[i]) fp32 block (mel power, as svhip_fbank writes it) at feat + n_mels * frame_offsets[i].
 * offsets / lengths (frame_offsets / frames) are HOST arrays, copied before the call returns; wav / feat / emb_out follow `flags` like
 * svhip_embed_wave (SVHIP_ASYNC needs device pointers).  emb_out is (n, nOut) fp32.
 * CAPACITY, checked on the host before anything is enqueued (svhip_ragged_check is the same test without a handle):
 *   1 <= n <= max_batch;  sum_i T_i <= max_batch * T, the rows of the workspace the handle owns (T = samples / hop + 1);  every
 *   T_i >= 5 (block 3 reflect-pads 4 frames);  wave: every lengths[i] >= n_fft;  offsets >= 0.
 * Anything else is SVHIP_ERR_INVALID with a message that names the utterance and the limit.  SVHIP_MODEL_ECAPA with compute SVHIP_F32 or
 * SVHIP_BF16 only: every other model and SVHIP_F32X3 return SVHIP_ERR_UNSUPPORTED.  The first ragged call of a handle allocates the
 * segment tables and a waveform staging buffer (once; nothing is allocated per call).
 * BATCH INVARIANCE: an utterance's embedding and stages are bit-for-bit the same whatever it is packed with and wherever it sits in the
 * pack — every reduction over time walks the utterance's own frames in an order fixed by the frame index, and every GEMM of the ragged
 * forward runs on one kernel whatever the row count.  Against a fixed-length call of the same utterance the values agree to the
 * precision of the compute type (the two forwards take different kernels), not bit for bit.
 * STAGES after a ragged call (svhip_get_stage): the names of the ECAPA forward; per-frame tensors come back with the rows packed,
 * (sum_i T_i, channels) in utterance order, per-utterance vectors as (n, .); "mel" is the utterances' (n_mels, T_i) blocks back to back.
 * The numeric status (SVHIP_ERR_NONFINITE) is reported as after any forward. */
int svhip_embed_wave_ragged(svhip_handle* h, const float* wav, const int64_t* offsets, const int32_t* lengths,
                            int32_t n, float* emb_out, int32_t flags);
int svhip_embed_features_ragged(svhip_handle* h, const float* feat, const int64_t* frame_offsets, const int32_t* frames,
                                int32_t n, float* emb_out, int32_t flags);
/* The capacity and scope rules of the two calls above for a handle of configuration *cfg, on the host alone (no GPU is touched):
 * lengths[i] are samples (is_wave != 0) or frames.  SVHIP_OK, SVHIP_ERR_INVALID or SVHIP_ERR_UNSUPPORTED; the message is
 * svhip_last_error(NULL). */
int svhip_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n, int32_t is_wave);

/* Ragged RawNet3 packs (added under ABI v5): the same call for SVHIP_MODEL_RAWNET3, the raw-waveform branch of Raw3_ECAPA.  The two
 * calls above are specified in mel frames and stay ECAPA's; they refuse a RawNet3 handle with SVHIP_ERR_UNSUPPORTED.
 *   utterance i is wav[offsets[i] .. offsets[i] + lengths[i]) and has T0_i = (lengths[i] - 251) / 10 + 1 frames after the sinc
 *   filterbank, T0_i / 5 after layer1's pool and T0_i / 5 / 3 after layer2's; the pack is laid out back to back at each of the three
 *   levels (an utterance's T % 5 / T % 3 left-over frames are dropped per utterance, as its own forward would drop them).
 * wav / offsets / lengths / emb_out / flags: the rules of svhip_embed_wave_ragged.
 * CAPACITY, checked on the host before anything is enqueued (svhip_rawnet3_ragged_check is the same test without a handle):
 *   1 <= n <= max_batch;  every lengths[i] >= 541;  offsets >= 0;  sum_i T0_i <= max_batch * T0, the level-0 rows of the workspace the
 *   handle owns (T0 = (samples - 251) / 10 + 1).  That one rule bounds the other levels: the level-2 buffers hold
 *   floor(max_batch * T0 / 15) + 1 rows (the sum of T0_i / 5 / 3 can pass max_batch * (T0 / 5 / 3) by a few rows).
 * Anything else is SVHIP_ERR_INVALID with a message that names the utterance and the limit.  Compute SVHIP_F32 or SVHIP_BF16 only:
 * every other model and compute type return SVHIP_ERR_UNSUPPORTED.  The first ragged call of a handle allocates the segment tables
 * and a waveform staging buffer (once; nothing is allocated per call).
 * BATCH INVARIANCE as above: bit-for-bit the same embedding and stages whatever the pack; to the precision of the compute type against
 * a fixed-length call.  A non-finite waveform gives NaN for its own utterance only, and SVHIP_ERR_NONFINITE.
 * STAGES after a ragged call: rn3_front (sum T0_i, 256), rn3_layer1 (sum T0_i / 5, 1024), rn3_layer2 / rn3_layer3 (sum T0_i / 5 / 3, 1024),
 * rn3_layer4 (sum T0_i / 5 / 3, 1536), rows packed in utterance order; rn3_pooled (n, 3072). */
int svhip_rawnet3_embed_ragged(svhip_handle* h, const float* wav, const int64_t* offsets, const int32_t* lengths,
                               int32_t n, float* emb_out, int32_t flags);
/* lengths[i] are samples.  SVHIP_OK, SVHIP_ERR_INVALID or SVHIP_ERR_UNSUPPORTED; the message is svhip_last_error(NULL). */
int svhip_rawnet3_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n);

/* Ragged RawNet2 packs (added under ABI v5): the same call for SVHIP_MODEL_RAWNET2_CONV, the raw-waveform branch of Raw_ECAPA_conv_asp.
 * The sinc models (SVHIP_MODEL_RAWNET2, SVHIP_MODEL_RAWNET2_GRU) are refused with SVHIP_ERR_UNSUPPORTED: their LayerNorm(nb_samp) fixes
 * the input length by the weights.  The other ragged calls keep refusing every RawNet2 handle.
 *   utterance i is wav[offsets[i] .. offsets[i] + lengths[i]) and has T1_i = lengths[i] / 3 frames after the conv front-end, then
 *   T1_i / 3, / 9, .. / 729 after the six max_pool1d(3) stages; the pack is laid out back to back at each of the seven levels (an
 *   utterance's left-over frames of a pool are dropped per utterance, as its own forward would drop them).
 * wav / offsets / lengths / emb_out / flags: the rules of svhip_embed_wave_ragged.
 * CAPACITY, checked on the host before anything is enqueued (svhip_rawnet2_ragged_check is the same test without a handle):
 *   1 <= n <= max_batch;  every lengths[i] >= 2187 (729 front-end frames: one frame reaches the aggregation);  offsets >= 0;
 *   sum_i T1_i <= max_batch * T1, the level-0 rows of the workspace the handle owns (T1 = samples / 3, samples >= 2187).  That one
 *   rule bounds the other levels; what a pack can hold beyond max_batch * (T1 / 729) rows at the last level lives in buffers the
 *   first ragged call allocates (once; nothing is allocated per call), with the segment tables and a waveform staging buffer.
 * Anything else is SVHIP_ERR_INVALID with a message that names the utterance and the limit.  Compute SVHIP_F32, SVHIP_BF16 or SVHIP_F16
 * (this model's 16-bit mode); SVHIP_F32X3 and every other model return SVHIP_ERR_UNSUPPORTED.
 * BATCH INVARIANCE as above: bit-for-bit the same embedding and stages whatever the pack — no grid size, slice count or kernel
 * choice of the ragged forward depends on n, on the neighbours or on the device's compute units; to the precision of the compute
 * type against a fixed-length call.  A non-finite waveform (or an fp16 overflow) gives a non-finite embedding for its own utterance
 * only, and SVHIP_ERR_NONFINITE.
 * STAGES after a ragged call, rows packed in utterance order: rn_pooled (n, 1024) always; with option rn_keep also rn_front (sum T1_i,
 * 128), rn_b<i>_pre / rn_b<i>_o (block i's level, its channels), rn_b<i>_x (where the next block's identity shortcut reads it),
 * rn_b<i>_gate (n, channels), rn_agg_in and rn_logits (last level, 512). */
int svhip_rawnet2_embed_ragged(svhip_handle* h, const float* wav, const int64_t* offsets, const int32_t* lengths,
                               int32_t n, float* emb_out, int32_t flags);
/* lengths[i] are samples.  SVHIP_OK, SVHIP_ERR_INVALID or SVHIP_ERR_UNSUPPORTED; the message is svhip_last_error(NULL). */
int svhip_rawnet2_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n);

/* Ragged Conformer packs (added under ABI v5): the same calls for SVHIP_MODEL_CONFORMER.  The ECAPA and RawNet3 calls above keep
 * refusing a Conformer handle with SVHIP_ERR_UNSUPPORTED.
 *   in / offsets / lengths / emb_out / flags: the rules of svhip_embed_wave_ragged (is_wave != 0: lengths and offsets in samples) and of
 *   svhip_embed_features_ragged (is_wave == 0: lengths are frames, offsets frame offsets).  Utterance i has T_i mel frames and
 *   T'_i = (T_i - 3) / 4 subsampled frames; the pack is laid out back to back at both levels.
 * CAPACITY, checked on the host before anything is enqueued (svhip_conformer_ragged_check is the same test without a handle):
 *   1 <= n <= max_batch;  every T_i >= 7;  wave: every lengths[i] >= n_fft;  offsets >= 0;  every T'_i <= 10000 (the positional
 *   encoding);  every T'_i <= chunk * T', what one subsampling slice of the handle holds (T' of the handle's own length; chunk =
 *   min(max_batch, 256 MiB / the conv1 output of one utterance of that length): an utterance's conv1 image must fit the slice buffer);
 *   sum_i T_i <= max_batch * T, the mel rows of the workspace the handle owns.  That one sum rule bounds the subsampled level: the row
 *   buffers of the blocks hold floor((max_batch * T - 3) / 4) rows (the sum of T'_i can pass max_batch * T' by about 1.5 max_batch rows).
 * Anything else is SVHIP_ERR_INVALID with a message that names the utterance and the limit.  Compute SVHIP_F32 or SVHIP_BF16 only: every
 * other model and SVHIP_F32X3 return SVHIP_ERR_UNSUPPORTED.  The first ragged call of a handle allocates the segment tables and a
 * waveform staging buffer (once); P = pe W_pos^T is formed for rows 0 .. the longest T'_i seen so far (the double-precision row sums of
 * svhip_finalize_weights, so its first T' rows are the handle's own), on the first ragged call and again only when a longer utterance
 * arrives.  Nothing else is allocated per call, and a handle that never sees a ragged call pays nothing.
 * BATCH INVARIANCE as above: bit-for-bit the same embedding and stages whatever the pack; to the precision of the compute type against
 * a fixed-length call.  A non-finite input gives NaN for its own utterance only, and SVHIP_ERR_NONFINITE.
 * STAGES after a ragged call: cf_in, cf_attn0, cf_block0, cf_last (sum T'_i, 256), rows packed in utterance order; cf_pool (n, 512);
 * with option cf_keep also cf_b<i>_ff1 | _qkv | _ctx | _att | _pw1 | _dw | _conv | _ff2 | _out and cf_logits (sum T'_i rows), cf_pool_raw (n, 512);
 * "input" (sum T_i, n_mels). */
int svhip_conformer_embed_ragged(svhip_handle* h, const float* in, const int64_t* offsets, const int32_t* lengths, int32_t n, float* emb_out,
                                 int32_t flags, int32_t is_wave);
/* lengths[i] are samples (is_wave != 0) or frames.  SVHIP_OK, SVHIP_ERR_INVALID or SVHIP_ERR_UNSUPPORTED; the message is svhip_last_error(NULL). */
int svhip_conformer_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n, int32_t is_wave);

/* Ragged TitaNet packs (added under ABI v5): the same calls for SVHIP_MODEL_TITANET, the spectral branch of Tita_ECAPA.  The ECAPA,
 * RawNet3 and Conformer calls above keep refusing a TitaNet handle with SVHIP_ERR_UNSUPPORTED.
 *   in / offsets / lengths / emb_out / flags / is_wave: the rules of svhip_conformer_embed_ragged.  TitaNet does not subsample, so the
 *   pack has one frame level: utterance i owns T_i rows of every activation, back to back in utterance order.
 * CAPACITY, checked on the host before anything is enqueued (svhip_titanet_ragged_check is the same test without a handle):
 *   1 <= n <= max_batch;  every T_i >= 1;  wave: every lengths[i] >= n_fft;  offsets >= 0;  sum_i T_i <= max_batch * T, T = samples / hop + 1
 *   (the rows of the workspace the handle owns).
 * Anything else is SVHIP_ERR_INVALID with a message that names the utterance and the limit.  Compute SVHIP_F32 or SVHIP_BF16 only: every
 * other model returns SVHIP_ERR_UNSUPPORTED.  The first ragged call of a handle allocates the segment tables and a waveform staging
 * buffer (once); nothing is allocated per call, and a handle that never sees a ragged call pays nothing.
 * BATCH INVARIANCE as above: bit-for-bit the same embedding and stages whatever the pack (every GEMM of the ragged forward runs on one
 * kernel, the depthwise convolutions pad at each utterance's own edges, and the SE squeeze is taken over the utterance's own frames at
 * both computes); to the precision of the compute type against a fixed-length call, which stays bit for bit what it was.  A non-finite
 * input gives NaN for its own utterance only, and SVHIP_ERR_NONFINITE.
 * STAGES after a ragged call: tn_prolog, tn_dw0, tn_mega_last (sum T_i, H) and tn_enc (sum T_i, 1536), rows packed in utterance order;
 * tn_pool (n, 3072); with option tn_keep also tn_b<i>_skip | _dw0 | _pw0 | _dw1 | _pw1 | _dw2 | _pw2 | _out, tn_att and tn_logits (sum T_i rows),
 * tn_b<i>_mean, tn_b<i>_gate and tn_pool_raw (n rows); "mel" the packed (n_mels, T_i) blocks. */
int svhip_titanet_embed_ragged(svhip_handle* h, const float* in, const int64_t* offsets, const int32_t* lengths, int32_t n, float* emb_out,
                               int32_t flags, int32_t is_wave);
/* lengths[i] are samples (is_wave != 0) or frames.  SVHIP_OK, SVHIP_ERR_INVALID or SVHIP_ERR_UNSUPPORTED; the message is svhip_last_error(NULL). */
int svhip_titanet_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n, int32_t is_wave);

/* Ragged ResNetSE34V2 packs (added under ABI v5): the same calls for SVHIP_MODEL_RESNETSE.  The ECAPA, RawNet2, RawNet3, Conformer and
 * TitaNet calls above keep refusing a ResNetSE handle with SVHIP_ERR_UNSUPPORTED, and these refuse every other model.
 *   in / offsets / lengths / emb_out / flags / is_wave: the rules of svhip_titanet_embed_ragged.  Utterance i has T_i mel frames and is a
 *   (P_l,i, Q_l, C_l) channels-last image at each of four frame levels: P_0,i = T_i (the stem and layer1), P_l+1,i = ceil(P_l,i / 2)
 *   (layer2 .. layer4); Q_l and C_l are the handle's.  The images lie back to back in utterance order at every level.
 * CAPACITY, checked on the host before anything is enqueued (svhip_resnetse_ragged_check is the same test without a handle):
 *   1 <= n <= max_batch;  every T_i >= 2 (InstanceNorm1d over one frame is undefined);  wave: every lengths[i] >= n_fft;  offsets >= 0;
 *   sum_i 8 ceil(T_i / 8) <= max_batch * T, T = samples / hop + 1.  An utterance counts as its frames rounded up to a multiple of 8 because
 *   the subsampling rounds up: sum T_i <= max_batch * T alone would let a deeper level overflow (max_batch = 4, T = 40, frames 37 + 41 +
 *   41 + 41 = 160, but 19 + 21 + 21 + 21 = 82 rows at level 1, over 4 * 20).  With the rounding, sum_i P_l,i <= max_batch * P_l at every
 *   level, since ceil(T_i / 2^l) <= 8 ceil(T_i / 8) / 2^l for l <= 3.
 * Anything else is SVHIP_ERR_INVALID with a message that names the utterance and the limit.  Compute SVHIP_F32 or SVHIP_BF16 only: every
 * other model returns SVHIP_ERR_UNSUPPORTED.  The first ragged call of a handle allocates the segment tables, the tile tables of the
 * convolutions, the SE tile sums of a pack and a waveform staging buffer (once); nothing is allocated per call, and a handle that never
 * sees a ragged call pays nothing.
 * BATCH INVARIANCE as above: bit-for-bit the same embedding and stages whatever the pack.  Every utterance is tiled by the convolution's
 * plan for its own image and padded with zeros at its own first and last frame, its SE squeeze adds its own tiles in its own order, and
 * the two attention convolutions run on one kernel; so rs_stem .. rs_layer4 of an utterance are also bit for bit those of a fixed-length
 * handle of its length at B = 1, and the embedding agrees with it to the precision of the compute type.  The fixed-length call stays bit
 * for bit what it was.  A non-finite input gives NaN for its own utterance only, and SVHIP_ERR_NONFINITE.
 * STAGES after a ragged call: rs_stem, rs_layer1 .. rs_layer4 (sum_i P_l,i * Q_l, C_l), the images packed in utterance order; rs_pool
 * (n, 2 F); with option rs_keep also rs_xin (sum T_i rows), rs_b<i>_conv1 | _conv2 | _down | _out (the packed images of the block's
 * level), rs_b<i>_part (the pack's tiles in pack order: utterance by utterance, each in its own tile order), rs_b<i>_gate and
 * rs_pool_raw (n rows), rs_att and rs_logits (sum_i P_4,i rows); "mel" the packed (n_mels, T_i) blocks. */
int svhip_resnetse_embed_ragged(svhip_handle* h, const float* in, const int64_t* offsets, const int32_t* lengths, int32_t n, float* emb_out,
                                int32_t flags, int32_t is_wave);
/* lengths[i] are samples (is_wave != 0) or frames.  SVHIP_OK, SVHIP_ERR_INVALID or SVHIP_ERR_UNSUPPORTED; the message is svhip_last_error(NULL). */
int svhip_resnetse_ragged_check(const svhip_config* cfg, const int32_t* lengths, int32_t n, int32_t is_wave);

/* Eval-mode cropping on device.  Replaces, for decoded 16-bit PCM, the cropping half of loadWAV
 * (src/processing/audio_loader.py:110-150): wrap-pad files not longer than L to L+1 samples, take num_eval
 * crops of L samples at int(linspace(0, len - L, num_eval)), scale by 1/32768 (soundfile float32).  pcm holds
 * the files back to back; file f is pcm[offsets[f] .. offsets[f] + lengths[f]).  crops_out is
 * (n_files * num_eval, L) fp32.  Ships int16 over PCIe instead of num_eval overlapping fp32 crops.  Host PCM is staged in a
 * buffer of the handle; with SVHIP_ASYNC (host or device input, device output) the call returns once the copy and the kernel
 * are enqueued — offsets / lengths are copied before it returns, the PCM array must stay valid until the stream has passed
 * the copy (immediately for pageable memory; a later synchronisation for pinned memory, which is what makes it overlap). */
int svhip_crop_pcm16(svhip_handle* h, const int16_t* pcm, int64_t n_samples, const int64_t* offsets, const int32_t* lengths,
                     int32_t n_files, int32_t num_eval, int32_t L, float* crops_out, int32_t flags);

/* Scoring.  Replaces the per-trial loop of ModelHandling.evaluateFromList / testFromList
 * (src/model.py:415-448,526-553) and src/utils.py:126-169.
 *   l2norm       : F.normalize(p=2, dim=1) in place (src/model.py:421-423), eps 1e-12.
 *   score_pairs  : out[p] = | cos(E[ia[p]], E[ib[p]]) |, per-norm clamp 1e-5 (utils.py:163-164,
 *                  one crop per row).  Any D and any 4-byte aligned E: the pair kernels (asnorm_pairs too) read 16 bytes at a time only
 *                  where D % 4 == 0 and E sits on a 16-byte boundary (the kernel looks at its base address), element by element otherwise.
 *   score_matrix : out (Na, Nb) = A @ B^T (np.inner, utils.py:150).  On every handle the product runs as three fp16 MFMAs on IEEE-half
 *                  hi | lo planes of the operands (fp32-grade: ~1e-7 of |a||b| from the float64 product); both operands are first scaled
 *                  by exact powers of two on the device (a row of A by its own max |x|, B by its global max |x|), so for D in {192, 256}
 *                  (the row-streaming kernel; 16-byte aligned operands) ANY finite magnitude is served, and an inf / NaN element stays in
 *                  its own row or column (non-finite elements are left out of the max |x| searches).  Every other multiple of 32, and
 *                  D in {192, 256} with an operand that is not 16-byte aligned, takes the tiled route, WITHOUT the scaling: B is split
 *                  into hi | lo half words (profile label "split_words"), and the GEMM runs the split form where both operands and the
 *                  output are 16-byte aligned and the output rows are too (Nb % 4 == 0; the slabs of asnorm_stats and score_topk
 *                  always are), the exact fp32 MFMA on the unsplit operands otherwise (the words are then not read).  That second form
 *                  reads 16 bytes at a time from rows that are only 4-byte aligned: it relies on the unaligned global access of the
 *                  hardware, which needs dword alignment only.  The served range of the route is that of its split form: rows of
 *                  both operands with an L2 norm in [1, 30000] (L2-normalised embeddings and their sums over crops or
 *                  enrolments; every |x| <= 65504), where a score lies within 1e-6 of |a||b| from the float64 product.  Below it the lo
 *                  half of a component goes subnormal and the error grows as 1 / norm: 8e-7 of |a||b| at a norm of 0.1 against a row inside
 *                  the range, 1.05e-6 with both at 0.1, 1e-5 at 0.01, 1e-4 at 1e-3 (measured on the MI355X, D = 64 .. 512); beyond
 *                  |x| = 65504 the scores come out inf / NaN.  An inf / NaN element stays in its own row or column there too.  Option
 *                  score_f32mfma keeps the exact fp32 MFMA on every width and at any magnitude (5.5e-7 of |a||b|, row norms 1e-6 .. 3e5)
 *                  and is the way to score rows outside that range at those widths.  D % 32 != 0 is refused with SVHIP_ERR_UNSUPPORTED
 *                  before anything is copied or launched.
 *   asnorm_stats : per row of E: S = cohort @ e (utils.py:142), top-`top` largest, population
 *                  mean / std (utils.py:143-146) -> mu[N], sigma[N].  For D in {192, 256}, top <= 256 and K >= 4 top the cohort
 *                  scores never reach memory (fused selection in the half-plane MFMA kernel, csrc/asnorm_fused.hip: the same three-MFMA
 *                  products and the same power-of-two operand scaling as score_matrix; option asnorm_f32mfma: exact fp32 MFMA); otherwise, and for
 *                  the embeddings that kernel cannot decide even with a threshold re-derived from its own counts (up to three more passes over those
 *                  embeddings only: svhip_asnorm_last_refit()), they exist only as <= 2 GiB slabs.  svhip_asnorm_last_fallback():
 *                  how many embeddings of the last call took the slab path after the fused kernel (-1: the whole call did).  The slab
 *                  path serves every K and every top: its cohort GEMM is score_matrix's (its routes, its magnitude contract, D % 32 != 0
 *                  refused with SVHIP_ERR_UNSUPPORTED before anything is launched; an operand that is not 16-byte aligned sends the whole
 *                  call here), and the selection runs with the row in registers (K <= 6144), in LDS (K <= 37 888) or read from the slab
 *                  (longer cohorts); profile labels "asnorm_cohort_gemm", then "asnorm_topk_reg8" | "_reg24" | "_lds" | "_global".
 *   asnorm_pairs : out[p] = 0.5*((s-mu[a])/sd[a] + (s-mu[b])/sd[b]), s = E[a].E[b] (utils.py:148-160).
 *   score_topk   : 1:N identification (what the `predict` branch of the reference's driver asks, src/inference.py:254-327): per row of Q
 *                  the k largest entries of Q @ G^T and the gallery rows they belong to, best first, without the N x M matrix.  Order:
 *                  score descending; equal scores by the lower gallery index; a NaN score below every number (-inf included), NaNs among
 *                  themselves by the lower index; +inf first.  A row's result depends on that row of Q and on G only - not on N, on the
 *                  row's place in Q or on how the gallery is sliced.  1 <= k <= 128, k <= M <= 2^31 - 1, D >= 1 (else SVHIP_ERR_INVALID,
 *                  the message names the value; nothing is launched); N = 0 is SVHIP_OK.  fp32-grade on every handle: a returned score
 *                  of L2-normalised rows lies within 1e-6 of the float64 inner product of the row it names.  D in {192, 256} with
 *                  16-byte aligned operands: the fused kernel (csrc/score_topk.hip, exact fp32 MFMA, any finite magnitude; profile
 *                  labels "score_topk", "score_topk_merge") - no score reaches memory.  Every other width: slabs of query rows through
 *                  score_matrix's GEMM (its magnitude contract: the tiled route's served range of row norms, option score_f32mfma
 *                  outside it; at most 2 GiB, at least 128 rows: M <= 4 194 304, beyond it SVHIP_ERR_UNSUPPORTED; D % 32 != 0 is
 *                  SVHIP_ERR_UNSUPPORTED before anything is launched) and a row kernel ("score_topk_gemm", "score_topk_rows").  An
 *                  operand that is not 16-byte aligned takes this route at D = 192 / 256 as well.
 *   score_topk_norm : open-set 1:N identification: score_topk over adaptive-S-normalised scores, so that the best score can be compared
 *                  with one threshold across speakers and channels.  Inputs: Q (N, D) with q_mu[N], q_sigma[N], G (M, D) with g_mu[M],
 *                  g_sigma[M]; every statistic is fp32, as svhip_asnorm_stats writes them.  The coefficients are computed in fp32, one
 *                  IEEE operation each,
 *                      a = 0.5f / sigma          b = mu * a
 *                  and the score is
 *                      t(n, m) = fmaf( s(n, m), aq[n] + ag[m], -(bq[n] + bg[m]) )
 *                  with s the fp32 inner product exactly as score_topk computes it on the same route: the algebraic
 *                  0.5*((s-mu_q)/sd_q + (s-mu_g)/sd_g) of asnorm_pairs in a form with one rounding per step (exact on integer data).
 *                  Result: per query the k largest t and their gallery rows, best first, in score_topk's order (t descending, ties to
 *                  the lower index, NaN below every number, +inf first); out_score holds t.  Every gallery row has its own mean and
 *                  deviation, so the ranking differs from the cosine ranking: the selection itself sees t.  No constraint is placed
 *                  on the statistics: a zero, negative or non-finite sigma or mu gives whatever IEEE gives, and a NaN t sorts last.
 *                  A row's result depends only on that row of Q, its two statistics, G and G's statistics - not on N, on the row's
 *                  place in Q, on the gallery slicing or on which form of the kernel ran it: bit for bit.  Bounds, refusals, N = 0,
 *                  pointer spaces and SVHIP_ASYNC as score_topk (messages start "score_topk_norm:"); a NULL statistic pointer is
 *                  SVHIP_ERR_INVALID "NULL pointer".  Routes as score_topk; profile labels "score_topk_coef" (the coefficients, once per
 *                  call), then "score_topk_norm", "score_topk_merge" (fused) or "score_topk_gemm", "score_topk_rows_norm" (slab).
 *   score_above  : threshold search ("which enrolled speakers match at all?"): EVERY pair (n, m) of a row of Q (N, D) and a row of G (M, D)
 *                  whose score reaches a threshold, however many or few there are, without the N x M matrix.  A pair is a HIT iff
 *                  v(n, m) >= thr, with v = s, the fp32 inner product exactly as score_topk computes it on the same route, or - when the
 *                  four statistic arrays are given - v = t exactly as score_topk_norm computes it (its statement above; the coefficients
 *                  under the profile label "score_above_coef").  A NaN v is never a hit; thr = -inf makes every pair whose v is not NaN a
 *                  hit, thr = +inf only the pairs whose v is +inf; a NaN thr is SVHIP_ERR_INVALID, refused before anything is launched.
 *                  Result: CSR.  row_ptr[N + 1] int64 (row_ptr[0] = 0), index[total] int32 and score[total] fp32 (v; -0 is returned as
 *                  +0, as score_topk does) with total = row_ptr[N]; the hits of query n are the entries row_ptr[n] .. row_ptr[n + 1] - 1,
 *                  in ASCENDING gallery index.  A row's hits (indices and score bits) depend only on that row of Q, its two statistics,
 *                  G, G's statistics and thr - not on N, on the row's place in Q, on how the gallery is sliced or on which form of the
 *                  kernel ran: bit for bit; and the score bits of a hit are the bits score_topk / score_topk_norm returns for that pair
 *                  on the same route.  `mode`: 0, or SVHIP_ABOVE_UPPER: keep a pair only if m > q_base + n - the self-join of one set,
 *                  Q being the rows q_base .. q_base + N - 1 of G: every unordered pair appears once and no row matches itself; a long
 *                  set is joined in query chunks, each with its own q_base (q_base >= 0; it is not looked at without the flag).
 *                  Two calls, so that the caller owns the allocation and nothing overflows silently:
 *                    svhip_score_above_count   out_count[n] = the number of hits of query n (int64[N]).  The caller takes the
 *                                              exclusive prefix sum (row_ptr) and allocates index and score for row_ptr[N] entries.
 *                    svhip_score_above_fill    the same arguments plus row_ptr: counts again, and only if row_ptr[0] = 0 and EVERY row's
 *                                              recount equals row_ptr[n + 1] - row_ptr[n] writes the hits.  Otherwise (the inputs
 *                                              changed between the two calls) SVHIP_ERR_INVALID, the message names the first such row, and
 *                                              NOTHING is written: no entry outside [0, row_ptr[N]) is ever touched.
 *                  All four statistic pointers NULL: the plain score; some but not all NULL: SVHIP_ERR_INVALID.  Bounds (1 <= M <=
 *                  2^31 - 1, D >= 1, N >= 0), N = 0 (SVHIP_OK, nothing is read or written), pointer spaces (row_ptr is an input,
 *                  out_count / out_index / out_score are outputs) as score_topk; messages start "score_above:".  SVHIP_ASYNC: count as
 *                  score_topk; fill waits for its own recount on the host before it writes and skips only the final wait.  A device
 *                  row_ptr is read on the handle's stream (row_ptr[N] first, for the size of the outputs): work enqueued there is
 *                  waited for, a row_ptr produced on ANOTHER stream must be complete before the call, like every device input.
 *                  Routes as score_topk.  D in {192, 256} with 16-byte aligned operands: the fused kernel (csrc/score_above.hip: the MFMA
 *                  loop of score_topk's kernel, no score reaches memory), once to count ("score_above_count", then "score_above_scan":
 *                  the per-row sums, in fill the offsets of a row's lists and the comparison with row_ptr) and once more to write
 *                  ("score_above_fill": the two lanes that share the 32 rows of a gallery block for one query exchange their hit counts
 *                  in registers, so a list is written in ascending index as it is met and no ordering pass follows).  Every other width
 *                  or alignment: slabs of score_matrix's GEMM and a row kernel that counts, then compacts, a slab row in index order
 *                  ("score_above_gemm", "score_above_rows"); the refusals of score_topk's slab route hold (D % 32 != 0 and
 *                  M > 4 194 304: SVHIP_ERR_UNSUPPORTED before anything is launched), and so does its magnitude contract.
 *   cluster_above: speaker clustering ("which rows are the same speaker?"): the connected components of the threshold graph of ONE set,
 *                  without an edge list and without the N x N matrix.  Input: E (N, D) and a threshold thr.  Rows i < j are LINKED iff
 *                  v(i, j) >= thr, v being the inner product exactly as score_above computes it for Q = G = E on the same route, or -
 *                  with mu[N] and sigma[N], the rows' AS-norm statistics - t = fmaf(s, a_i + a_j, -(b_i + b_j)) as score_topk_norm /
 *                  score_above compute it (a = 0.5f / sigma, b = mu * a; profile label "cluster_coef").  A NaN v links nothing; thr =
 *                  -inf links every pair whose v is not NaN.  A CLUSTER is a connected component of that graph (single linkage).
 *                  Outputs: out_root[i] (int32[N]) = the smallest row index in i's cluster; out_cluster[i] (int32[N], optional: NULL =
 *                  not wanted) = the dense id, clusters numbered 0 .. C - 1 in order of their smallest member; *out_n_clusters
 *                  (int64) = C.  The result is a function of the data only: the same bits on every run, whatever order the hardware
 *                  meets the links in, and by definition the components of the pair set score_above(E, E, thr, SVHIP_ABOVE_UPPER)
 *                  returns.  SVHIP_ERR_INVALID before any copy or launch (messages start "cluster_above:"): a NaN thr, D < 1, N < 0,
 *                  N > 2^31 - 1, mu without sigma or sigma without mu, a NULL E, out_root or out_n_clusters; D % 32 != 0:
 *                  SVHIP_ERR_UNSUPPORTED; the outputs are then untouched.  N = 0: SVHIP_OK, *out_n_clusters = 0.  Pointer spaces (E, mu,
 *                  sigma in; out_root, out_cluster, out_n_clusters out) and SVHIP_ASYNC as score_topk.
 *                  Routes as score_above.  D in {192, 256} with a 16-byte aligned E: ONE pass of the fused walk per part of the launch
 *                  plan ("cluster_link"; csrc/score_cluster.hip): each surviving pair is unioned at once in a lock-free disjoint-set
 *                  forest held in out_root (parent[x] <= x, the larger root hooked under the smaller by compare-and-swap), and a
 *                  workgroup whose gallery slice lies at or below its query rows returns before the walk.  Every other width or
 *                  alignment: slabs of score_matrix's GEMM and a row kernel that links a slab row's hits above the diagonal
 *                  ("cluster_gemm", "cluster_link_rows"; score_topk's slab refusals and magnitude contract hold).  Both: "cluster_init"
 *                  before, "cluster_flatten" and "cluster_ids" (a hand-written scan of the root flags) behind.  Scratch is O(N) plus
 *                  the slab: no buffer's size depends on the number of links.
 *   cluster_join : two-set clustering ("which clusters do these NEW rows belong to?"): joins the rows B (NB, D) to a set A (NA, D) that
 *                  may already be clustered, without walking A x A again.  The rows are numbered jointly: A's are 0 .. NA - 1, B's
 *                  NA .. NA + NB - 1.  The graph has three kinds of edges.  SEED links: where root_a (int32[NA]) is given, A's own
 *                  pairs are NOT scored; row i of A is linked to row root_a[i].  Any array with 0 <= root_a[i] <= i is legal -
 *                  cluster_above's out_root, or any parent-pointer forest whose pointers go downwards; an entry outside [0, i] is
 *                  read as i (the row starts alone).  root_b (int32[NB]) likewise, in B's own numbering 0 .. NB - 1.  INTERNAL links
 *                  of a side whose root_x is NULL: its pairs i < j are scored and linked exactly as cluster_above does on that side
 *                  alone.  CROSS links, always walked: every pair (a in A, b in B) with v(a, b) >= thr.  v(a, b) is the score
 *                  score_above returns for the query row a and the gallery row b (the lower joint index is the query, as in
 *                  cluster_above), or - with the four statistic arrays a_mu[NA], a_sigma[NA], b_mu[NB], b_sigma[NB], all or none -
 *                  t = fmaf(s, a_a + a_b, -(b_a + b_b)) from the two sides' coefficients ("cluster_join_coef").  A NaN v links
 *                  nothing; thr = -inf links every pair whose v is not NaN.  Outputs as cluster_above's over the NA + NB joint rows:
 *                  out_root[i] = the smallest joint index of i's cluster, out_cluster (optional) the dense ids in order of the
 *                  smallest member, *out_n_clusters their number.  The result is a function of the data only, the same bits on
 *                  every run.  The components of a graph do not depend on the order its edges are met in, and a score depends only
 *                  on its two rows, so: both seeds NULL; root_a = cluster_above(A)'s out_root with root_b NULL; and root_a, root_b
 *                  = cluster_above's out_root of A and of B - all three give cluster_above([A; B]), exactly.  A new row may bridge
 *                  two old clusters: out_root[i] != root_a[i] for the absorbed cluster's rows is the answer, not an error.
 *                  Refusals are cluster_above's, before any copy or launch, outputs untouched, messages starting "cluster_join:".
 *                  SVHIP_ERR_INVALID: a NaN thr, D < 1, a negative NA or NB, NA + NB > 2^31 - 1, some but not all of the four
 *                  statistic pointers, a NULL A where NA > 0 (likewise B), a NULL out_root where NA + NB > 0, a NULL
 *                  out_n_clusters; D % 32 != 0: SVHIP_ERR_UNSUPPORTED.  Seeds handed over as HOST arrays are checked on the host too:
 *                  an entry outside [0, i] is SVHIP_ERR_INVALID and names the first offending index (device seeds get the
 *                  read-as-i rule).  NA + NB = 0: SVHIP_OK, *out_n_clusters = 0.  NA = 0 or NB = 0 is legal: one side alone, seeded
 *                  (no MFMA pass at all) or walked.  Pointer spaces (A, B, root_a, root_b and the statistics in; the three outputs
 *                  out) and SVHIP_ASYNC as cluster_above.
 *                  Device side (csrc/score_cluster.hip).  "cluster_seed" writes the joint forest (the clamp above is one function,
 *                  shared with the host check and exercised by svhip_selftest: the forest's climbs end only because parent[x] <= x).
 *                  Fused route (D in {192, 256}, A and B 16-byte aligned): one link launch per part of the plan over queries = A,
 *                  gallery = B - or the other way round where B is the smaller side: on this route v(a, b) and v(b, a) are the same
 *                  bits ("cluster_join_link": cluster_link's body with an index offset per side and no mask); an unseeded
 *                  side's self-join runs cluster_above's plan behind the side's offset ("cluster_join_self").  Every other width or
 *                  alignment: slabs and a row kernel ("cluster_join_gemm" / "cluster_join_rows", "cluster_join_self_gemm" /
 *                  "cluster_join_self_rows"; score_topk's slab refusals hold, for NB as the gallery and for an unseeded side).  Then
 *                  "cluster_flatten" and "cluster_ids" over NA + NB rows.  Scratch is O(NA + NB) plus the slab.
 *   cluster_linkage: speaker clustering that does not chain: AVERAGE or COMPLETE linkage cut at thr, without the N x N matrix.  Every
 *                  merge of either linkage at a level >= thr needs one pair with v >= thr, so every such cluster lies inside ONE
 *                  component of cluster_above(E, thr, mu, sigma): the COMPONENTS are cluster_above's (its kernels, its routes, its
 *                  bits), and the agglomeration runs inside each component alone, one workgroup per component.
 *                  Scores inside a component: v(i, j) = ONE fp32 chain fmaf(E[i][d], E[j][d], v) over d = 0 .. D - 1 from +0 - the
 *                  exact fp32 inner product of exactly representable data, within (D + 1) 2^-24 sum|e_i e_j| of the float64 one, NOT
 *                  bound to the bits of score_above's MFMA order - or, with mu / sigma, t = fmaf(v, a_i + a_j, -(b_i + b_j)) from
 *                  cluster_above's coefficients.  v(i, j) and v(j, i) are the same bits (the pair is computed once); a NaN v is
 *                  taken as -inf.  Inside a component every row starts as its own cluster.  L(A, B) = the sum (average) or the
 *                  minimum (complete) of v(a, b) over a in A, b in B, kept per pair of clusters and updated by L(A u B, C) = L(A, C) +
 *                  L(B, C) (one fp32 add) or fminf of the two; g(A, B) = L / (float)(|A| |B|) (average: one fp32 division) or L
 *                  (complete).  Repeat: among all pairs of current clusters of the component take the largest g, equal values going
 *                  to the smallest (min A, min B) with min A < min B; if g >= thr merge, otherwise stop (a NaN g is never taken).
 *                  Outputs: out_root[i] = the smallest row of i's final cluster; out_cluster / *out_n_clusters as cluster_above's
 *                  (dense ids in order of the smallest member); *out_n_unrefined (int64, optional: NULL = not wanted) = the number
 *                  of components of more than SVHIP_LINKAGE_MAX_ROWS rows: one workgroup owns a component, so such a component is
 *                  NOT refined and stays one cluster (the cap is a measured value: one component of 256 / 512 / 1 024 rows
 *                  takes 2.2 / 7.0 / 25 ms on an MI355X whatever else the call holds, 2 048 / 4 096 rows took 104 / 450 ms).
 *                  The result is a function of the data only, the same bits on every run, and
 *                  a row's cluster depends only on the rows of its own component: not on N, the component's place, the other
 *                  components or the launch.  `linkage`: SVHIP_LINKAGE_AVERAGE or SVHIP_LINKAGE_COMPLETE, anything else
 *                  SVHIP_ERR_INVALID.  Refusals as cluster_above's, messages starting "cluster_linkage:", before any copy or launch,
 *                  outputs untouched.  N = 0: SVHIP_OK, both counts 0.  thr = -inf is legal (everything whose v is not NaN is one
 *                  component, and merges down to one cluster).  Pointer spaces and SVHIP_ASYNC as cluster_above.
 *                  Device side (csrc/score_linkage.hip).  "linkage_table": per component its size (integer atomics on the dense id),
 *                  an exclusive scan to offsets (cluster_ids' hand-written block scan), the member list through an atomic cursor
 *                  (the owning workgroup sorts it ascending) and three work lists by size.  "linkage_agglo": one workgroup per
 *                  component of >= 2 rows builds the m x m matrix with plain FMAs and agglomerates in place - per row the best partner
 *                  above it is cached, a merge is one argmax over the caches, the row / column update of the surviving slot (the
 *                  cluster's smallest member) and a rescan of the rows whose cached partner was merged.  m <= 64 and m <=
 *                  SVHIP_LINKAGE_LDS_ROWS (option "linkage_lds_rows" lowers it; tests) keep the matrix in LDS; larger components keep
 *                  it in a pool of scratch of min(2^24, N min(N, SVHIP_LINKAGE_MAX_ROWS)) floats - 64 MiB at most, the fixed budget;
 *                  the handle's scratch slots grow by half again, so up to 96 MiB are held.  The pool exists whenever N exceeds the
 *                  LDS cap, whether or not a component needs it, in the slot of the slab route's slab: where it is larger than the
 *                  slab the slot is reallocated behind a stream synchronise, in an SVHIP_ASYNC call too.  One thread packs those
 *                  components into rounds whose matrices fit the pool, and one launch per round the host cannot rule out follows
 *                  ("linkage_agglo_pool": 2 floor(N min(N, SVHIP_LINKAGE_MAX_ROWS) / pool) + 1 launches, 33 at 262 144 rows; an empty
 *                  round returns at once); both homes run one body and give the same bits.  No
 *                  host round trip: the sizes never leave the device.  Then "cluster_ids" over the refined roots.  Nothing's size
 *                  depends on the number of links.
 *   group_audit  : dataset audit ("which files of a speaker folder do not sound like the rest of it?", the label-noise audit of the
 *                  reference's src/benchmark/benchmark_dataset.py:32-84): per file the number of files of its OWN group it does not match.
 *                  Inputs: F (n_files, n_crops, D) fp32 crop embeddings, the files sorted by group; group_ptr[n_groups + 1] int64, ALWAYS
 *                  a host pointer whatever `flags` say, group_ptr[0] = 0, non-decreasing, group_ptr[n_groups] = n_files: group g is the
 *                  files group_ptr[g] .. group_ptr[g + 1] - 1 (empty groups and groups of one file are legal); cut, a float.  For two
 *                  files i, j of the SAME group
 *                      s(i, j) = ( sum_c | dot(F[i,c], F[j,c]) / (max(sqrt(|F[i,c]|^2), 1e-5f) * max(sqrt(|F[j,c]|^2), 1e-5f)) | ) / (float)n_crops
 *                  - SVHIP_TRIAL_COSINE's statement (utils.py:163-164), the crops added in index order, one final division.  (i, j) is a
 *                  MISMATCH iff s(i, j) <= cut; a NaN score is never a mismatch (the reference's check_matching turns it into a match).
 *                  out_miss[i] (int32[n_files]) = the number of files j != i of i's group that i mismatches (the reference's
 *                  imposters[file]).  out_score is optional (NULL: not wanted): the dense per-group score blocks back to back, block g
 *                  starting at the sum of n_h^2 over the groups h < g, row-major n_g x n_g, both (i, j) and (j, i) written, the diagonal
 *                  written as computed and never counted; the caller allocates sum n_g^2 floats.  Promises, on each route: s(i, j) and
 *                  s(j, i) are the same bits; a file's count and its row of scores depend only on the rows of its own group and on cut -
 *                  not on the other groups, on the group's place in F, on n_files or n_groups or on the launch geometry: bit for bit; a
 *                  NaN / inf element changes only scores of its own file.  n_files = 0 or n_groups = 0: SVHIP_OK, nothing is read or
 *                  written.  SVHIP_ERR_INVALID before any copy or launch (messages start "group_audit:"): n_crops < 1, D < 1, a NULL F,
 *                  group_ptr or out_miss, group_ptr[0] != 0, a decrease, group_ptr[n_groups] != n_files; more than 2^31 - 1 files:
 *                  SVHIP_ERR_UNSUPPORTED.  Pointer spaces (F in, out_miss / out_score out) and SVHIP_ASYNC as score_topk;
 *                  group_ptr has been read when the call returns (its device copy is waited for, so an asynchronous call also waits
 *                  for what the handle's stream held before it).
 *                  Routes, from D and the alignment of the device F alone.  D % 32 == 0, D <= 1024, 16-byte aligned: the MFMA kernel
 *                  (csrc/group_audit.hip: 64 x 64 tiles on the file axis, small groups share a tile under a block-diagonal mask, exact
 *                  fp32 v_mfma_f32_32x32x2_f32, the upper triangle of the join computed once and counted for both files with integer
 *                  atomics, the norms from the tile's own loads; profile labels "group_audit_tables", "group_audit"): within (2 D + n_crops + 16) * 2^-24
 *                  of the float64 statement on unit rows.  Every other width or alignment: chunks of 2^21 within-group pairs are
 *                  enumerated on the device, scored by score_trials' kernel and counted ("group_audit_tables", then per chunk
 *                  "group_audit_pairs", "score_trials", "group_audit_count"): a score's bits are svhip_score_trials(SVHIP_TRIAL_COSINE)'s.
 * Pointers follow `flags` (indices are int32, device or host like the other inputs). */
int svhip_l2norm(svhip_handle* h, float* E, int64_t N, int32_t D, int32_t flags);
int svhip_score_pairs(svhip_handle* h, const float* E, int64_t N, int32_t D,
                      const int32_t* ia, const int32_t* ib, int64_t P, float* out, int32_t flags);
int svhip_score_matrix(svhip_handle* h, const float* A, int64_t Na, const float* B, int64_t Nb,
                       int32_t D, float* out, int32_t flags);
int svhip_asnorm_stats(svhip_handle* h, const float* E, int64_t N, int32_t D, const float* cohort,
                       int32_t K, int32_t top, float* mu, float* sigma, int32_t flags);
/* out_score (N, k), out_index (N, k): per row of Q the k largest entries of Q @ G^T (np.inner, as score_matrix) and the
 * gallery rows they belong to, best first.  Pointers follow `flags`. */
int svhip_score_topk(svhip_handle* h, const float* Q, int64_t N, const float* G, int64_t M, int32_t D, int32_t k,
                     float* out_score, int32_t* out_index, int32_t flags);
/* as svhip_score_topk over t = fmaf(s, aq + ag, -(bq + bg)), a = 0.5f / sigma, b = mu * a (statement above); out_score holds t. */
int svhip_score_topk_norm(svhip_handle* h, const float* Q, int64_t N, const float* q_mu, const float* q_sigma,
                          const float* G, int64_t M, const float* g_mu, const float* g_sigma,
                          int32_t D, int32_t k, float* out_score, int32_t* out_index, int32_t flags);
/* threshold search (score_above above): count, then fill.  q_mu / q_sigma / g_mu / g_sigma: all NULL (plain score) or none; mode: 0 or
 * SVHIP_ABOVE_UPPER (q_base then places Q inside G). */
enum { SVHIP_ABOVE_UPPER = 1 };
int svhip_score_above_count(svhip_handle* h, const float* Q, int64_t N, const float* G, int64_t M, int32_t D, float thr,
                            const float* q_mu, const float* q_sigma, const float* g_mu, const float* g_sigma,
                            int64_t q_base, int32_t mode, int64_t* out_count /* int64[N] */, int32_t flags);
int svhip_score_above_fill(svhip_handle* h, const float* Q, int64_t N, const float* G, int64_t M, int32_t D, float thr,
                           const float* q_mu, const float* q_sigma, const float* g_mu, const float* g_sigma,
                           int64_t q_base, int32_t mode, const int64_t* row_ptr /* int64[N + 1] */,
                           int32_t* out_index, float* out_score, int32_t flags);
/* speaker clustering (cluster_above above): mu / sigma both NULL (plain score) or both given; out_cluster may be NULL. */
int svhip_cluster_above(svhip_handle* h, const float* E, int64_t N, int32_t D, float thr, const float* mu, const float* sigma,
                        int32_t* out_root /* int32[N] */, int32_t* out_cluster /* int32[N], or NULL */,
                        int64_t* out_n_clusters, int32_t flags);
/* two-set clustering (cluster_join above): B's rows joined to A's; root_a / root_b: a known grouping of that side, or NULL (the side is
 * walked); the four statistic arrays all or none; out_cluster may be NULL.  Joint rows: A's 0 .. NA - 1, B's NA .. NA + NB - 1. */
int svhip_cluster_join(svhip_handle* h, const float* A, int64_t NA, const int32_t* root_a /* int32[NA] or NULL */,
                       const float* B, int64_t NB, const int32_t* root_b /* int32[NB] or NULL */, int32_t D, float thr,
                       const float* a_mu, const float* a_sigma, const float* b_mu, const float* b_sigma,
                       int32_t* out_root /* int32[NA + NB] */, int32_t* out_cluster /* int32[NA + NB], or NULL */,
                       int64_t* out_n_clusters, int32_t flags);
/* average / complete linkage inside cluster_above's components (cluster_linkage above); out_cluster and out_n_unrefined may be NULL. */
enum { SVHIP_LINKAGE_AVERAGE = 1, SVHIP_LINKAGE_COMPLETE = 2 };
#define SVHIP_LINKAGE_MAX_ROWS 1024
#define SVHIP_LINKAGE_LDS_ROWS 176      /* the largest component whose matrix lives in LDS */
int svhip_cluster_linkage(svhip_handle* h, const float* E, int64_t N, int32_t D, float thr, const float* mu, const float* sigma,
                          int32_t linkage, int32_t* out_root /* int32[N] */, int32_t* out_cluster /* int32[N], or NULL */,
                          int64_t* out_n_clusters, int64_t* out_n_unrefined /* or NULL */, int32_t flags);
/* dataset audit (group_audit above): group_ptr is always a HOST array; out_score may be NULL. */
int svhip_group_audit(svhip_handle* h, const float* F, int64_t n_files, int32_t n_crops, int32_t D,
                      const int64_t* group_ptr /* host, int64[n_groups + 1] */, int64_t n_groups, float cut,
                      int32_t* out_miss /* int32[n_files] */, float* out_score /* sum n_g^2 floats, or NULL */, int32_t flags);
int svhip_asnorm_pairs(svhip_handle* h, const float* E, int64_t N, int32_t D, const float* mu,
                       const float* sigma, const int32_t* ia, const int32_t* ib, int64_t P,
                       float* out, int32_t flags);
int64_t svhip_asnorm_last_fallback(const svhip_handle* h);
/* ABI v5: embeddings of the last svhip_asnorm_stats call whose threshold the fused kernel re-derived from its own counts (cohort scores that
 * are not normally distributed: clustered speaker centroids) and decided in `*passes` extra passes (NULL: not wanted) instead of the slab path. */
int64_t svhip_asnorm_last_refit(const svhip_handle* h, int32_t* passes);

/* Whole-trial scores over the crops of two files (what ModelHandling.evaluateFromList needs per trial, src/model.py:413-448):
 * F is the (n_files, n_crops, D) embedding block, ia / ib index files, out[p] is
 *   SVHIP_TRIAL_COSINE : mean_i | cos(F[a, i], F[b, i]) |, per-norm clamp 1e-5              (utils.py:163-164)
 *   SVHIP_TRIAL_PNORM  : mean_i || F[a, i] - F[b, i] + 1e-6 ||_2                            (utils.py:167-169)
 *   SVHIP_TRIAL_PDIST  : - mean_{i,d} sqrt( sum_j (F[a, i, d] - F[b, j, d] + 1e-6)^2 )      (model.py:425-431, cohorts_path = None)
 * mean_crops: out (n_files, D) = mean over the crops (the AS-norm statement runs on crop means).
 * Pointers follow `flags`. */
enum { SVHIP_TRIAL_COSINE = 0, SVHIP_TRIAL_PNORM = 1, SVHIP_TRIAL_PDIST = 2 };
int svhip_score_trials(svhip_handle* h, int32_t mode, const float* F, int64_t n_files, int32_t n_crops, int32_t D,
                       const int32_t* ia, const int32_t* ib, int64_t P, float* out, int32_t flags);
int svhip_mean_crops(svhip_handle* h, const float* F, int64_t n_files, int32_t n_crops, int32_t D, float* out, int32_t flags);
/* SVHIP_TRIAL_PNORM with the reference's `p` argument (pnorm_similarity(ref, com, p), utils.py:167-169 -> F.pairwise_distance(p=p, eps=1e-6)):
 * out[t] = mean_i || F[a, i] - F[b, i] + 1e-6 ||_p; p = +-inf: max / min |d|, p = 0: the count of non-zero d, otherwise (sum |d|^p)^(1/p).
 * p = 2 is svhip_score_trials(SVHIP_TRIAL_PNORM). */
int svhip_score_trials_pnorm(svhip_handle* h, float p, const float* F, int64_t n_files, int32_t n_crops, int32_t D,
                             const int32_t* ia, const int32_t* ib, int64_t P, float* out, int32_t flags);

/* Verification metrics over a scored trial list: the sort-and-accumulate core of the reference's
 * evaluation tail, which it runs as Python list sorts and loops (src/utils.py:221-275) and sklearn calls (utils.py:74-121).
 * scores fp32, labels int32 in {0, 1}, P trials (< 2^31); pointers follow `flags`, the scalar results are host pointers.
 *   roc_points  : sklearn's _binary_clf_curve as roc_curve / precision_recall_curve use it in tuneThresholdfromScore
 *                 (utils.py:77-80,112): scores through nan_to_num, then one point per DISTINCT score value, highest first:
 *                 thr[k], fps[k] / tps[k] = negatives / positives scoring >= thr[k].  *n_out distinct values; the output
 *                 buffers hold P entries.  The caller finishes with the reference's own O(n) selection (drop_intermediate,
 *                 argmin / argmax, trapezoid) — speakerverification_amd/metrics.py does, in float64 like the reference.
 *   error_rates : ComputeErrorRates (utils.py:221-256): stable ascending sort (ties keep list order, as sorted() does);
 *                 fnrs[i] = positives among the i+1 lowest / positives, fprs[i] = 1 - negatives among them / negatives
 *                 (float64), thresholds[i] = the i-th lowest score.
 *   min_dcf     : ComputeErrorRates + ComputeMinDcf (utils.py:262-275) fused: the FIRST minimum over i of
 *                 c_miss*fnrs[i]*p_target + c_fa*fprs[i]*(1-p_target), divided by min(c_miss*p_target, c_fa*(1-p_target));
 *                 float64, Python's operation order, no fused multiply-add. */
int svhip_roc_points(svhip_handle* h, const float* scores, const int32_t* labels, int64_t P, int64_t* n_out, float* thr,
                     int64_t* fps, int64_t* tps, int32_t flags);
int svhip_error_rates(svhip_handle* h, const float* scores, const int32_t* labels, int64_t P, double* fnrs, double* fprs,
                      float* thresholds, int32_t flags);
int svhip_min_dcf(svhip_handle* h, const float* scores, const int32_t* labels, int64_t P, double p_target, double c_miss,
                  double c_fa, double* min_dcf, float* threshold, int32_t flags);

/* Packed checkpoint blob.  Replaces, at deployment time, the Python-side checkpoint handling of
 * ModelHandling.loadParameters (src/model.py:718-746: torch.load of a '.model' file + name-matched copy, and
 * src/trainer.py:145-205 which writes those files): speakerverification_amd/checkpoint.py converts a reference state dict
 * once (host-side torch.load) into a flat, versioned, FNV-1a-checksummed tensor archive; svhip_load_blob mmaps it and feeds
 * every tensor through svhip_load_tensor + svhip_finalize_weights (BatchNorm fold, weight packing, sinc filter bake), so no
 * Python / torch is needed at run time and the result is bit-identical to the state-dict path.
 *   blob_write  : n tensors (names are reference state_dict keys of __S__), shapes n x 4 (unused dims ignored), dtypes SVHIP_*.
 *   blob_open   : mmap + validate (magic, version, size, checksum, every table entry in bounds).  Errors: svhip_blob_last_error().
 *   blob_tensor : borrow tensor idx (pointers stay valid until blob_close).
 *   load_blob   : tensors whose names the handle's model does not know are skipped (as loadParameters skips them,
 *                 model.py:730-736); a known name with the wrong shape, a missing tensor, or a model mismatch is an error. */
typedef struct svhip_blob svhip_blob;
int svhip_blob_write(const char* path, int32_t model, int32_t n, const char* const* names, const void* const* data,
                     const int64_t* shapes, const int32_t* ndims, const int32_t* dtypes);
int svhip_blob_open(const char* path, svhip_blob** out);
int32_t svhip_blob_count(const svhip_blob* b);
int32_t svhip_blob_model(const svhip_blob* b);
int svhip_blob_tensor(const svhip_blob* b, int32_t idx, const char** name, const void** data, int64_t* shape4,
                      int32_t* ndim, int32_t* dtype);
int svhip_blob_close(svhip_blob* b);
const char* svhip_blob_last_error(void);
int svhip_load_blob(svhip_handle* h, const char* path);

/* Multi-GPU exchange.  Replaces the reference's `torch.distributed.all_gather_object` of per-rank
 * feature dicts (src/model.py:400-411): one process per GPU, utterances sharded in contiguous blocks, ONE RCCL all-gather
 * of the dense (rows, D) fp32 block per rank on the handle's stream — embed -> gather -> score stays on the device.
 *   comm_unique_id : rank 0 draws the 128-byte RCCL id; the host ships it to the other ranks by any side channel
 *                    (speakerverification_amd/distributed.py: the torch.distributed store).  Errors: svhip_comm_last_error().
 *   comm_init      : ncclCommInitRank on the handle's device (collective: every rank of `world` must call it).
 *   allgather_rows : out (world * rows, D) <- every rank's local (rows, D); rank r's block lands at out + r * rows * D.
 *                    All ranks pass the same `rows` (pad the last block).  Pointers follow `flags`.
 *   comm_destroy   : also called by svhip_destroy.
 * RCCL is bound at the first svhip_comm_* call (dlopen librccl.so.1); without it these return SVHIP_ERR_UNSUPPORTED. */
#define SVHIP_COMM_ID_BYTES 128
int svhip_comm_unique_id(void* id_out);
int svhip_comm_init(svhip_handle* h, const void* id, int32_t rank, int32_t world);
int svhip_comm_rank(const svhip_handle* h, int32_t* rank, int32_t* world);
int svhip_allgather_rows(svhip_handle* h, const float* local, int64_t rows, int32_t D, float* out, int32_t flags);
int svhip_comm_destroy(svhip_handle* h);
const char* svhip_comm_last_error(void);

/* Synthetic workload generator (nothing in the reference corresponds — its evaluation reads files):
 * utterances [first_utt, first_utt + B) of the counter-based stream `seed` (Philox4x32-10 + Box-Muller, 0.1 * N(0,1)
 * clipped to [-1, 1]), (B, L) fp32, L % 4 == 0.  A pure function of (seed, utterance, sample): every rank of a sharded
 * run generates exactly its own block without moving waveforms over PCIe.  oracle/synthwave.py restates it. */
int svhip_synth_waveforms(svhip_handle* h, uint64_t seed, int64_t first_utt, int32_t B, int32_t L, float* wav_out, int32_t flags);

/* Introspection used by tests and bench.py (not part of the reference's surface).
 *   get_stage    : copy an intermediate activation of the LAST forward to host as fp32, frame-major
 *                  (B, T, C).  Names: "input","blocks.0".."blocks.3","mfa","asp","asp_bn" (ECAPA), and of block 3 "blocks.3.tdnn1",
 *                  "blocks.3.res2net", "blocks.3.tdnn2" (B T, C), "blocks.3.se_gate" (B, C), then "asp_gstats" (B, 6C: mean | std)
 *                  and "asp_att" (B T, 128: asp.tdnn after tanh) — SVHIP_ERR_STATE where the last forward's route did not keep the
 *                  value (blocks.3.tdnn1 of SVHIP_F32X3 handles whose tdnn1 wrote its first chunks in the split layout only; "mel"
 *                  after the fused front-end); "rn_gru_in" (the (B T, 512) GRU
 *                  input of a one-slice forward) and "rn_gru_h" (the (B, 1024) fp32 last GRU state) of SVHIP_MODEL_RAWNET2_GRU;
 *                  with option "rn_keep" what a RawNet2 forward stored on its way (INTEGRATION.md lists the names: "rn_front",
 *                  "rn_b<i>_pre", "rn_b<i>_x", "rn_b<i>_o", "rn_b<i>_c2", "rn_b<i>_pool", "rn_b<i>_gate", "rn_agg_in", "rn_logits") — SVHIP_ERR_STATE
 *                  where the route taken never stored the tensor;
 *                  "tn_prolog" (B T, H), "tn_dw0" (block 0's first depthwise output, its bias included), "tn_mega_last" (the last
 *                  mega-block's output), "tn_enc" (B T, 1536) and "tn_pool" (B, 3072, after BN) of SVHIP_MODEL_TITANET, and with option
 *                  "tn_keep" what its forward stored on its way: per mega-block i "tn_b<i>_skip" (B T, H: the 1 x 1 skip + BN),
 *                  "tn_b<i>_dw0" | "_pw0" | "_dw1" | "_pw1" | "_dw2" | "_pw2" (the three depthwise and pointwise outputs; dw0 of block 0 is
 *                  tn_dw's, of a later block the previous block tail's), "tn_b<i>_out" (the block's output), "tn_b<i>_gate" (B, H fp32:
 *                  the SE gate) and "tn_b<i>_mean" (B, H fp32: the SE squeeze, only where the squeeze kernel ran — SVHIP_ERR_STATE
 *                  where the gate came from the GEMM's column sums), then "tn_att" (B T, 128), "tn_logits" (B T, 1536 fp32) and
 *                  "tn_pool_raw" (B, 3072 fp32: [mean | std] before BN) — SVHIP_ERR_STATE without the option;
 *                  "cf_in" (B T', 256: the input projection), "cf_block0", "cf_attn0" (block 0's per-head attention context before
 *                  out_proj), "cf_last" (the last block's output) and "cf_pool" (B, 512, after attention_norm) of SVHIP_MODEL_CONFORMER,
 *                  and with option "cf_keep" what its forward stored on its way: per block i = 0 .. 5 "cf_b<i>_ff1" (B T', 256: after
 *                  the first half-step), "cf_b<i>_qkv" (B T', 768), "cf_b<i>_ctx" (the attention context), "cf_b<i>_att" (after
 *                  out_proj and its residual), "cf_b<i>_pw1" (B T', 512), "cf_b<i>_dw" (GLU, depthwise conv, BN, Swish),
 *                  "cf_b<i>_conv" (after pw2 and its residual), "cf_b<i>_ff2" (after the second half-step), "cf_b<i>_out" (the
 *                  block's LayerNorm), then "cf_logits" (B T', 256 fp32: the pooling's logits) and "cf_pool_raw" (B, 512 fp32:
 *                  [mean | std] before attention_norm) — SVHIP_ERR_STATE without the option;
 *                  "rs_stem" (B P Q, 32: channels-last, P frames x Q mel rows), "rs_layer1" .. "rs_layer4" (each stage's output, B P' Q' x C)
 *                  and "rs_pool" (B, 512 n_mels / 8 fp32: [mean | std], feature q 256 + c) of SVHIP_MODEL_RESNETSE, and with option
 *                  "rs_keep" what its forward stored on its way: "rs_xin" (B T, n_mels fp32: the normalised input), per block
 *                  i = 0 .. 15 "rs_b<i>_conv1" | "_conv2" | "_out" (B P' Q', C: conv1 + bn1 + ReLU, conv2 + bn2, the block's output),
 *                  "rs_b<i>_down" (the downsample + BN; blocks 3, 7, 13), "rs_b<i>_part" (B ntp ntq, C fp32: the SE sums of conv2's
 *                  fp32 values over each tile's positions inside the image, tiles in the order tp ntq + tq) and "rs_b<i>_gate"
 *                  (B, C fp32), then "rs_att" (B P4, 128), "rs_logits" (B P4, 256 n_mels / 8 fp32) and "rs_pool_raw" (B, 512
 *                  n_mels / 8 fp32: [mean | std] before the pooling's affine, the identity here) — SVHIP_ERR_STATE without the
 *                  option; "rs_layer<s>" is bit for bit the "_out" of the stage's last block.
 *                  Returns the element count through *count (out may be NULL to query).
 *   profile_*    : when enabled every kernel launch is bracketed by HIP events on the handle's
 *                  stream; profile_get returns accumulated milliseconds / launch count per kernel
 *                  label since the last reset (enumerate idx = 0.. until SVHIP_ERR_INVALID).
 *   workload_flops: algorithmic FLOPs (2 x MACs of conv/linear layers) of one utterance. */
int svhip_get_stage(svhip_handle* h, const char* name, float* out, int64_t* count);
int svhip_profile_enable(svhip_handle* h, int32_t on);
int svhip_profile_filter(svhip_handle* h, const char* label);   /* NULL / "": every kernel; else only this label (fewer events in the stream) */
int svhip_profile_reset(svhip_handle* h);
int svhip_profile_get(svhip_handle* h, int32_t idx, char* name, int32_t name_cap, double* ms, int64_t* launches, double* flops);
double svhip_workload_flops(const svhip_handle* h);
/* Developer / test options (not part of the reference's surface).  The SVHIP_<NAME> environment variables are read ONCE, by
 * svhip_create, as a new handle's defaults; afterwards only this call changes them — no getenv on the hot path.  Names:
 * "pw3_cus" (cap of the persistent GEMM grids; 0: off), "rn_unfused", "asp_v1", "r2_big", "x3_keep_f32",
 * "asnorm_slab", "asnorm_f32mfma", "asnorm_norefit", "score_f32mfma", "score_tiled", "fbank32", "fbank_unfused", "rn_sinc_full", "cv_off",
 * "pw3_tail_off", "n128_off", "r2_slices", "rn_tail_big", "rn_sinc_f32", "rn_step_off", "rn_pool_off", "layer_labels", "rn_conv_unfused",
 * "rn_keep", "cf_keep", "tn_keep", "rs_keep", "linkage_lds_rows" (cluster_linkage: the largest component held in LDS, 2 ..
 * SVHIP_LINKAGE_LDS_ROWS; anything else: the default), "linkage_fill_only" (cluster_linkage builds the score matrices and merges
 * nothing: every row stays its own cluster; measurements).
 * Unknown names: SVHIP_ERR_INVALID. */
int svhip_set_option(svhip_handle* h, const char* name, int32_t value);
/* Free the scoring / metrics scratch slots of the handle (grown on demand, otherwise kept until svhip_destroy). */
int svhip_trim_scratch(svhip_handle* h);
int svhip_selftest(void);   /* host-only self checks (per-device launch-attribute bookkeeping); 0 = ok, no GPU needed */
/* Conformer's relative-position attention kernel on its own (tests): device pointers, enqueued on `stream` (NULL: the null stream),
 * not synchronised.  qkv (B T', 768) in the compute type (SVHIP_F32 / SVHIP_BF16) holds q | k | v; P (T', 256) fp32; u_bias, v_bias
 * [4][64] fp32; ctx (B T', 256) in the compute type receives the four heads' contexts.  1 <= T' <= 10000.  SVHIP_OK,
 * SVHIP_ERR_INVALID (arguments) or SVHIP_ERR_HIP (launch). */
int svhip_conformer_attention(const void* qkv, const float* P, const float* u_bias, const float* v_bias, void* ctx, int32_t compute,
                              int32_t B, int32_t T_sub, void* stream);

/* The attention kernel over a pack (tests), the counterpart of svhip_conformer_attention: utterance u owns the rows
 * [row0_dev[u], row0_dev[u + 1]) of qkv and ctx (row0_dev: a DEVICE table of n + 1 ints) and is attended exactly as
 * svhip_conformer_attention attends it alone (B = 1, T_sub = its length), bit for bit; P holds at least max_T_sub rows and
 * max_T_sub >= every utterance's length. */
int svhip_conformer_attention_ragged(const void* qkv, const float* P, const float* u_bias, const float* v_bias, void* ctx, int32_t compute,
                                     const int32_t* row0_dev, int32_t n, int32_t max_T_sub, void* stream);

/* TitaNet's depthwise kernels on their own (tests): device pointers, enqueued on `stream` (NULL: the null stream), not synchronised.
 * Activations are frame-major (B T, C) in the compute type (SVHIP_F32 / SVHIP_BF16), C % 8 == 0, 16-byte aligned; w is tap-major [k][C]
 * fp32, bias [C] fp32, k is 3, 7 or 11; gate (B, C) fp32.
 *   x != NULL:  d = dwconv(x) + bias, zero "same" padding at each utterance's edges (tn_dw; skip / h3 / gate / y are not read).
 *   x == NULL:  y = relu(skip + gate[b] * h3), and with d != NULL also d = dwconv(y) + bias in the same pass (tn_mega_tail; without d,
 *               w and bias may be NULL).
 * SVHIP_OK, SVHIP_ERR_INVALID (arguments, NULL pointers included: nothing is launched) or SVHIP_ERR_HIP (launch). */
int svhip_titanet_depthwise(const void* x, const void* skip, const void* h3, const float* gate, void* y, const float* w, const float* bias,
                            void* d, int32_t compute, int32_t k, int32_t B, int32_t T, int32_t C, void* stream);

/* The same kernels over a pack (tests): utterance u owns the rows [row0_dev[u], row0_dev[u + 1]) of every activation (row0_dev: a DEVICE
 * table of n + 1 ints), gate is (n, C), max_T >= every utterance's length.  The padding sits at each utterance's own edges and no tap reads
 * a neighbour's row; each utterance comes out exactly as svhip_titanet_depthwise gives it alone (B = 1, T = its length), bit for bit. */
int svhip_titanet_depthwise_ragged(const void* x, const void* skip, const void* h3, const float* gate, void* y, const float* w,
                                   const float* bias, void* d, int32_t compute, int32_t k, const int32_t* row0_dev, int32_t n, int32_t max_T,
                                   int32_t C, void* stream);

/* ResNetSE's 3 x 3 convolution kernel on its own (tests): y = [relu](scale[n] conv3x3_stride([relu](x)) + shift[n]) with zero padding 1.
 * x (B, P, Q, Cin) and y (B, Po, Qo, Cout), Po = (P - 1) / stride + 1, are DEVICE pointers, channels-last, in the compute type (SVHIP_F32 /
 * SVHIP_BF16); scale / shift are device fp32 [Cout]; w is the HOST weight (Cout, Cin, 3, 3) in the reference's layout, whose [kh][kw] run
 * over Q and P.  Cin a multiple of 32, Cout 32 or a multiple of 64, stride 1 or 2.  Enqueued on `stream` (NULL: the null stream) and
 * synchronised.  SVHIP_OK, SVHIP_ERR_INVALID (arguments), SVHIP_ERR_NOMEM or SVHIP_ERR_HIP. */
int svhip_resnetse_conv3x3(const void* x, const float* w, const float* scale, const float* shift, void* y, int32_t compute, int32_t B,
                           int32_t P, int32_t Q, int32_t Cin, int32_t Cout, int32_t stride, int32_t relu_in, int32_t relu_out, void* stream);

/* The same kernel over a pack (tests): n utterances, utterance u a (P_host[u], Q, Cin) image; the images lie back to back in x, and their
 * (Po_u, Qo, Cout) outputs back to back in y.  P_host holds n HOST int32 frame counts; the entry builds and uploads the segment tables,
 * builds the tile tables on the device, launches the packed kernel and synchronises.  Every utterance comes out exactly as
 * svhip_resnetse_conv3x3 gives it alone (B = 1, P = P_host[u]), bit for bit, and nothing outside the pack's rows is written. */
int svhip_resnetse_conv3x3_ragged(const void* x, const float* w, const float* scale, const float* shift, void* y, int32_t compute,
                                  const int32_t* P_host, int32_t n, int32_t Q, int32_t Cin, int32_t Cout, int32_t stride, int32_t relu_in,
                                  int32_t relu_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVHIP_H */
