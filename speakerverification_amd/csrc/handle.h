// handle.h — the handle of libsvhip and what the host-side translation units of the C ABI share (api*.hip, comm.hip).
// Internal: kernel translation units see kernels.h / common.h only.
#pragma once
#include "../../include/svhip.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <map>
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
        int rn_stop;              // RawNet2: return after this many residual blocks (0: after the sinc front-end), unfused kernel sequence
        int rn_snap;              // RawNet2: keep block n's pre-activation as stage "rn_snap"
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

    // ECAPA layers
    svhip::ConvLayer blocks0, mfa, asp_tdnn, asp_conv;
    svhip::ConvLayer tdnn1[3], tdnn2[3], res2[3][7];
    svhip::LinearLayer se1[3], se2[3], asp_ctx, fc;
    float* se2T[3] = {};                      // se_block.conv2 weight transposed to [128][C]
    void *se1_bf[3] = {}, *se2T_bf[3] = {};   // bf16 copies of both SE matrices (bf16 handles: half the L2 bytes per workgroup)
    float *aspbn_scale = nullptr, *aspbn_shift = nullptr;
    float *in_w = nullptr, *in_b = nullptr;   // instance norm affine

    // RawNet2 layers (front_proc='sinc' or 'conv', aggregate='asp'; RawNet2_custom.py:230-243)
    struct RnBlock {
        int cin = 0, cout = 0;
        bool downsample = false, has_shortcut = false;
        float *bn1_scale = nullptr, *bn1_shift = nullptr;
        svhip::ConvLayer conv1, conv2, shortcut;       // conv1 carries bn2 as its epilogue
        void* conv2sc_W = nullptr;              // bf16 handles: [Np][conv2.K + cin] = conv2 | 1 x 1 shortcut, one GEMM for both (gemm_pw2 A3)
        float* alpha = nullptr;
        svhip::LinearLayer afms_fc;
        float* afms_fcT = nullptr;              // fc weight transposed [cin][cout] (the gate kernel reads consecutive outputs per wave)
    };
    RnBlock rn_blocks[8];
    float *rn_gamma = nullptr, *rn_beta = nullptr, *rn_fbn_scale = nullptr, *rn_fbn_shift = nullptr;
    void* rn_filt = nullptr;
    void* rn_filt_sym = nullptr;              // fp16 handles: [128][128] slot-major table of the symmetric sinc form (round 6)
    void* rn_filt_x3 = nullptr;               // F32X3 handles: [2][128][256] half hi | lo parts of the sinc filters
    float* rn_cw = nullptr;                   // 'conv' front-end (SVHIP_MODEL_RAWNET2_CONV): [w0 | w1 | w2 | bias] x 128 floats of conv1
    float *rn_agg_scale = nullptr, *rn_agg_shift = nullptr;
    svhip::ConvLayer rn_att0, rn_att3;
    svhip::LinearLayer rn_fc;
    // aggregate='gru' (SVHIP_MODEL_RAWNET2_GRU): bn_before_gru is rn_agg_scale / rn_agg_shift; W_ih a 1 x 1 conv layer whose bias is
    // b_ih + [b_hr | b_hz | 0]; W_hh packed gate-interleaved (gru.hip) in the compute type; b_hn; fc_after_gru
    svhip::ConvLayer rn_gru_ih;
    void* rn_gru_whh = nullptr;
    float* rn_gru_bhn = nullptr;
    svhip::LinearLayer rn_gru_fc;
    float* rn_gru_gi = nullptr;           // (Bmax, T, 3072) fp32 gate inputs
    float* rn_gru_hbuf[2] = {};           // (Bmax, 1024) fp32 state, ping-pong
    int rn_gru_T = 0;                     // frames that reach the GRU
    const void* rn_gru_in = nullptr;      // svhip_get_stage "rn_gru_in": the GRU input of the last forward (one slice only)
    const float* rn_gru_h = nullptr;      //                 "rn_gru_h": the buffer that holds the last state
    void* rn_buf[6] = {};                 // activation ping-pong buffers
    float* rn_scratch = nullptr;
    void* rn_xn = nullptr;
    int rn_Lp = 0;
    float *rn_stats = nullptr, *rn_mean = nullptr, *rn_s = nullptr, *rn_logits = nullptr, *rn_pooled = nullptr;
    float* rn_part = nullptr;             // fused 128-channel blocks: per-tile column sums (B, ntiles, 128)
    int num_cu = 256;
    int rn_T1 = 0;
    const void* rn_dbg_x = nullptr; int rn_dbg_T = 0, rn_dbg_C = 0;   // SVHIP_RN_STOP developer hook (tests)
    void* rn_snap = nullptr; size_t rn_snap_cap = 0; int rn_snap_T = 0, rn_snap_C = 0;      // SVHIP_RN_SNAP=2: copy of block 2's pre-activation (stage "rn_snap")

    // RawNet3 layers (SVHIP_MODEL_RAWNET3: RawNet3.py with the defaults of its MainModel, RawNet_baseline.py:71-159)
    struct Rn3Layer {                         // Bottle2neck(k = 3, scale = 8): every BatchNorm follows a ReLU, so it is its conv's epilogue affine
        svhip::ConvLayer conv1, convs[7], conv3, residual;      // conv1 + bn1, convs[i] + bns[i], conv3 + bn3; residual: 1 x 1, no bias (layer1)
        bool has_residual = false;
        float* alpha = nullptr;               // AFMS
        svhip::LinearLayer afms_fc;
    };
    Rn3Layer rn3[3];
    svhip::ConvLayer rn3_l4, rn3_att;         // layer4 (3072 -> 1536, bias, ReLU); attention.0 columns [0, 1536) with attention.2 as epilogue
    svhip::LinearLayer rn3_att_ctx, rn3_fc6;  // attention.0 columns [1536, 4608) + its bias: the per-utterance bias of the time-constant inputs; fc6
    float *rn3_w2 = nullptr, *rn3_b2 = nullptr;                 // attention.3: the per-frame logit
    float *rn3_bn5_scale = nullptr, *rn3_bn5_shift = nullptr;
    float *rn3_in_w = nullptr, *rn3_in_b = nullptr;             // preprocess.1 (InstanceNorm1d affine)
    double rn3_pre[2] = {-0.97, 1.0};                           // preprocess.0.flipped_filter: y[i] = pre[0] x[i - 1] + pre[1] x[i]
    void* rn3_filt = nullptr;                 // [251][256] tap-major sinc filters: fp64 on fp32 handles, fp32 on bf16 handles
    int rn3_T0 = 0;                           // front-end frames; layer1 pools to T0 / 5, layer2 to T0 / 5 / 3
    void* rn3_buf[3] = {};                    // (Bmax * T0, 1024) activations each (the front-end's fp32 output passes through rn3_buf[1])
    void* rn3_x0 = nullptr;                   // (Bmax * T0, 256): the front-end output, layer1's operand
    void* rn3_cat = nullptr;                  // (Bmax * T2, 3072): [mp3(x1) | x2 | x3], layer4's operand
    double* rn3_stats = nullptr;              // (Bmax, 2) pre-emphasis / InstanceNorm statistics
    float *rn3_mean = nullptr, *rn3_gate = nullptr;             // (Bmax, 1024): time means, AFMS gates
    float *rn3_tstat = nullptr, *rn3_ctx = nullptr;             // (Bmax, 3072) [mean | std] of layer4's output; (Bmax, 128) attention bias
    float *rn3_logit = nullptr, *rn3_pooled = nullptr;          // (Bmax * T2) per-frame logits; (Bmax, 3072) bn5(pooled)
    const void* rn3_stage[5] = {};            // svhip_get_stage: front-end, layer1, layer2, layer3, layer4 outputs of the last forward
    int rn3_stage_T[5] = {}, rn3_stage_C[5] = {}, rn3_stage_ld[5] = {};

    // TitaNet layers (SVHIP_MODEL_TITANET: models/TitaNet.py).  Every BatchNorm follows its conv directly, so it is folded into that
    // conv's weights and bias at finalize (the GEMM epilogues apply at most the ReLU)
    struct TnBlock {
        float* dw_w[3] = {};                  // depthwise weights, tap-major [k][H] fp32
        float* dw_b[3] = {};                  // depthwise biases [H]
        svhip::ConvLayer pw[3], skip;         // pointwise convs + BN (ReLU in the epilogue); the 1 x 1 skip + BN
        float* se1 = nullptr;                 // excitation.0 [H / 16][H] (bf16 handles: bf16 copy in se1_bf)
        float* se2T = nullptr;                // excitation.2 transposed [H / 16][H]
        void *se1_bf = nullptr, *se2T_bf = nullptr;
    };
    std::vector<TnBlock> tn;                  // one per mega-block
    int tn_k = 0;                             // depthwise kernel size (3 / 7 / 11 for H = 256 / 512 / 1024)
    svhip::ConvLayer tn_prolog, tn_epilog, tn_att_in, tn_att_out;     // prolog (k = 3, zero padding), epilog, attention in_linear / out_linear
    float *tn_pbn_scale = nullptr, *tn_pbn_shift = nullptr;        // decoder.pool.1 (BatchNorm1d(3072))
    svhip::LinearLayer tn_fc;                 // decoder.linear.0 with decoder.linear.1 (BatchNorm1d(nOut)) folded in
    void* tn_buf[6] = {};                     // (Bmax T, H) each: prolog output, block output, block 0's first depthwise output, depthwise
                                              // output, sub-block output, skip (the first three are the stages tn_prolog / tn_mega_last / tn_dw0)
    void* tn_enc = nullptr;                   // (Bmax T, 1536) epilog output
    void* tn_att = nullptr;                   // (Bmax T, 128) tanh(in_linear(.))
    float* tn_logits = nullptr;               // (Bmax T, 1536) fp32 attention energies
    float *tn_mean = nullptr, *tn_gate = nullptr;                  // (Bmax, H) SE squeeze, SE gate
    float *tn_pool_raw = nullptr, *tn_pool = nullptr;              // (Bmax, 3072) pooled [mean | std], after BN

    // Conformer layers (SVHIP_MODEL_CONFORMER: models/Conformer.py, models/conformer/conformer/*).  d_model 256, 4 heads of 64, six blocks
    struct CfBlock {
        float *ff_g[2] = {}, *ff_b[2] = {};   // the two feed-forward modules' LayerNorms (FF, FF')
        svhip::ConvLayer ff1[2], ff2[2];      // Linear(256, 1024) (Swish in the epilogue), Linear(1024, 256)
        float *att_g = nullptr, *att_b = nullptr;
        svhip::ConvLayer qkv, out;            // query | key | value projections as one 256 -> 768 layer; out_proj
        float* P = nullptr;                   // (T', 256) fp32: pe[:T'] pos_proj^T (the same for every utterance: formed at finalize)
        float *u = nullptr, *v = nullptr;     // u_bias, v_bias [4][64]
        float *cv_g = nullptr, *cv_b = nullptr;
        svhip::ConvLayer pw1, pw2;            // pointwise 256 -> 512 (GLU follows), 256 -> 256
        float *dw_w = nullptr, *dw_b = nullptr;   // depthwise k = 15, tap-major [15][256], with BatchNorm(256) folded in
        float *fin_g = nullptr, *fin_b = nullptr; // the block's final LayerNorm
    };
    std::vector<CfBlock> cf;
    int cf_T1 = 0, cf_F1 = 0, cf_Tp = 0, cf_F2 = 0;   // conv1 / conv2 output sizes: T1 x F1, T' x F2
    int cf_chunk = 0;                         // utterances per subsampling slice (bounds the conv1 output buffer)
    float *cf_c1_w = nullptr, *cf_c1_b = nullptr;   // conv_subsample.sequential.0: tap-major [9][256], bias
    svhip::ConvLayer cf_c2;                   // conv_subsample.sequential.2 as a GEMM, k = dt * 768 + df * 256 + c (the segmented gather)
    int* cf_seg_off = nullptr;                // (T' F2) row offsets of that gather within an utterance's conv1 output
    svhip::ConvLayer cf_proj;                 // input_projection, columns permuted from c * F2 + f to f * 256 + c
    svhip::ConvLayer cf_att0, cf_att3;        // attention.0 (+ ReLU, attention.2 as the epilogue affine), attention.3 (fp32 logits)
    float *cf_pbn_scale = nullptr, *cf_pbn_shift = nullptr;   // attention_norm (BatchNorm1d(512))
    svhip::LinearLayer cf_fc;                 // fc (Conv1d(512, nOut, 1))
    float* cf_half = nullptr;                 // 256 x 0.5: the half-step residual as the epilogue scale
    void *cf_c1 = nullptr, *cf_s2 = nullptr;  // per slice: conv1 output (chunk, T1, F1, 256); conv2 output (chunk T' F2, 256)
    void *cf_in = nullptr, *cf_b0 = nullptr, *cf_x[2] = {}, *cf_r = nullptr;   // (Bmax T', 256): input projection, block 0's output,
                                              // later blocks' outputs (ping-pong), the residual stream inside a block
    void *cf_ln = nullptr, *cf_ln2 = nullptr; // (Bmax T', 256) LayerNorm outputs
    void* cf_hid = nullptr;                   // (Bmax T', 1024): FF hidden / q | k | v / pointwise-conv output
    void *cf_ctx = nullptr, *cf_attn0 = nullptr;   // (Bmax T', 256): attention context (block 0's is kept: stage cf_attn0); GLU-dw output
    void* cf_last = nullptr;                  // the last block's output
    float* cf_logits = nullptr;               // (Bmax T', 256) fp32 attention logits of the pooling
    float *cf_pool_raw = nullptr, *cf_pool = nullptr;         // (Bmax, 512) [mean | std], after attention_norm

    // ResNetSE layers (SVHIP_MODEL_RESNETSE: models/ResNetSE34V2.py).  Activations are channels-last (B, P, Q, C), P frames x Q mel rows; every
    // BatchNorm is the scale / shift of the convolution before it
    struct RsConv {
        void* W = nullptr;                    // [cin / CK][taps][cout][CK] in the compute type (resnetse.hip)
        float *scale = nullptr, *shift = nullptr;
        int cin = 0, cout = 0, stride = 1, ks = 3;
    };
    struct RsBlock {
        RsConv c1, c2, down;                  // conv1 + bn1, conv2 + bn2, downsample.0 + downsample.1 (the first block of stages 2 - 4)
        bool has_down = false;
        float *se_w1 = nullptr, *se_b1 = nullptr, *se_w2 = nullptr, *se_b2 = nullptr;      // se.fc.0 [16][C], se.fc.2 [C][16]
    };
    std::vector<RsBlock> rs;                  // the blocks of all stages in order
    int rs_stage_end[4] = {};                 // index one past the last block of each stage
    int rs_P[5] = {}, rs_Q[5] = {}, rs_C[5] = {};     // image size and channels of the stem output [0] and of each stage's output [1 .. 4]
    float *rs_stem_w = nullptr, *rs_stem_b = nullptr, *rs_stem_scale = nullptr, *rs_stem_shift = nullptr;     // conv1 tap-major [9][32], bn1
    svhip::ConvLayer rs_att0, rs_att3;        // attention.0 (+ ReLU, attention.2 as the epilogue affine), attention.3; K permuted to q C + c
    svhip::LinearLayer rs_fc;                 // fc, columns permuted the same way
    bool rs_sap = false;                      // encoder_type 'SAP': fc reads the weighted means only
    float* rs_xin = nullptr;                  // (Bmax, P, Q) fp32: the normalised input
    void* rs_out[5] = {};                     // the stem output and each stage's output (stages rs_stem, rs_layer1 .. rs_layer4)
    void* rs_tmp[5] = {};                     // block outputs inside a stage (ping-pong), conv1 output, conv2 output, downsample output
    float *rs_part = nullptr, *rs_gate = nullptr;      // SE: per-tile channel sums of conv2's output, (Bmax, C) gates
    void* rs_att = nullptr;                   // (Bmax P4, 128)
    float* rs_logits = nullptr;               // (Bmax P4, Q4 C4) fp32
    float *rs_pool_raw = nullptr, *rs_pool = nullptr, *rs_pool_one = nullptr, *rs_pool_zero = nullptr;     // (Bmax, 2 Q4 C4) [mu | sg]

    // workspace (device)
    float* d_wav = nullptr;       // (Bmax, L)
    float* d_feat = nullptr;      // (Bmax, n_mels, T) mel power
    float* d_pstats = nullptr;    // (Bmax*n_mels*2)
    float* d_xscale = nullptr;    // F32X3: [0] = s, [1] = 1 / s of the network input (launch_in_scale), then 256 partial max words
    float* d_logmel = nullptr;    // fused front-end (bf16 handles): (Bmax, T, n_mels) log-mel rows before the mean is taken off
    float* d_fpart = nullptr;     //   and their per-tile column sums (Bmax, ceil(T / 64), n_mels)
    bool xin_ready = false;       // the fused front-end has written X_in: ecapa_forward_part skips its prologue
    bool feat_is_stale = false;   // ... and d_feat does not hold this forward's mel power (svhip_get_stage "mel")
    float* d_zero = nullptr;      // 256 zero bytes (DMA source for padded conv chunks)
    float *d_ones = nullptr, *d_zeros = nullptr;      // 4096 ones / zeros: stand-ins for absent per-channel vectors (GemmParams::ones / zeros)
    size_t rn_buf_bytes = 0;      // RawNet2: payload bytes of each activation buffer; a 256-byte zero tail follows (the zero page of the
                                  // persistent conv-gather kernel must sit behind its A operand, within 4 GiB)
    void* s32_buf = nullptr;      // SVHIP_F32X3: the A operand of the current big GEMM in the S32 split layout (M x 3C x 4 bytes)
    bool x0_is_s32 = false;       // SVHIP_F32X3: the last forward wrote blocks.0's output (X0) in the split layout
    bool cat_f32_stale = false;   // SVHIP_F32X3: the last forward left the block outputs only in cat_s32 (svhip_get_stage converts on demand)
    bool h2_is_s32 = false;       // SVHIP_F32X3: the last forward's block-3 Res2Net chain output exists only in h2_s32 (the R2 step kernels)
    bool h1_split = false;        // ... and block 3's tdnn1 wrote its first two chunks in the split layout only (H1 does not hold them)
    void* cat_s32 = nullptr;      // SVHIP_F32X3: the SE-Res2Net block outputs (the CAT buffer) in the S32 layout, written by se_apply
    void* h2_s32 = nullptr;       // SVHIP_F32X3: the Res2Net chain output (H2's twin, S32 only) and the two step-input buffers (M x C/8)
    void* u_s32[2] = {};
    float* d_colsum = nullptr;    // pw2 column-sum partials, per lane: [sum | sumsq] x (tiles*4) x 3C floats
    int64_t colsum_region = 0;    // floats per (lane, kind) region
    void* X_in = nullptr;         // (M, n_mels)
    void* X0 = nullptr;           // (M, C)
    void *H1 = nullptr, *H2 = nullptr, *H3 = nullptr;   // (M, C)
    void* CAT = nullptr;          // (M, 3C)
    void* MFA = nullptr;          // (M, 3C)
    void* ATT = nullptr;          // (M, 128)
    float* LOGITS = nullptr;      // (M, 3C) fp32
    float *d_mean = nullptr, *d_s1 = nullptr, *d_s2 = nullptr, *d_gstats = nullptr, *d_ctx = nullptr;
    float* d_lin_part = nullptr;              // K-slice partials of the small-M linear layers (fc, asp_ctx) at full batches
    size_t lin_part_per_utt = 0;
    float *d_pool_raw = nullptr, *d_pool_bn = nullptr, *d_emb = nullptr;
    int lastB = 0;
    // ragged batches (svhip_embed_wave_ragged / svhip_embed_features_ragged; api_ecapa.hip): allocated by the handle's first ragged call
    int64_t* rag_feat_off = nullptr;          // (max_batch) element offset of every utterance's (n_mels, T_u) block in the feature array
    int* rag_row0 = nullptr;                  // (max_batch + 1) first workspace row of every utterance, then the row count (behind rag_feat_off)
    int* rag_utt = nullptr;                   // (max_batch * T) utterance of every row
    float* rag_wav = nullptr;                 // host-pointer calls: max_batch * (samples + hop) floats, the utterances back to back
    float* rag_stats = nullptr;               // (max_batch * n_mels * 2) shift / scale of the front-end normalisation
    struct RagSlot { char* host = nullptr; hipEvent_t done = nullptr; bool busy = false; };
    RagSlot rag_slot[4];                      // pinned copies of the tables of the calls in flight (SVHIP_ASYNC returns before the copy has run)
    int rag_next = 0;
    int64_t rag_rows = 0;                     // rows of the last forward when it was a ragged one (svhip_get_stage), else 0
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
    // scoring / metrics scratch: handle-owned slots, grown on demand (no hipMalloc / hipFree per call once warm)
    enum { SCR_IN0 = 0, SCR_IN1, SCR_IN2, SCR_IN3, SCR_IN4, SCR_OUT0, SCR_OUT1, SCR_OUT2, SCR_SLAB, SCR_SPLIT, SCR_CAND, SCR_CNT, SCR_MB,
           SCR_FLAG, SCR_GATHER, SCR_WS, SCR_COUNT };
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

inline bool rn_is_sinc(int model) { return model == SVHIP_MODEL_RAWNET2 || model == SVHIP_MODEL_RAWNET2_GRU; }     // front_proc='sinc'
inline bool rn_is_gru(int model) { return model == SVHIP_MODEL_RAWNET2_GRU; }                                       // aggregate='gru'
inline int tn_kernel_size(int H) { return H == 256 ? 3 : H == 512 ? 7 : H == 1024 ? 11 : 0; }      // TitaNet s / m / l (TitaNet.py:152-157)
inline int cf_sub(int n) { return (n - 3) / 2 + 1; }                  // one Conv2d(3, stride 2) of Conformer's subsampling (n >= 3)
constexpr int CF_D = 256, CF_LAYERS = 6, CF_MAX_T = 10000;           // d_model, blocks, the length of the pe buffer
inline int rn3_frames(int L) { return (L - RN3_TAPS) / RN3_STRIDE + 1; }      // T0 of RawNet3's front-end
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
struct ModelOps {
    int model;
    CheckFn* check;
    SpecFn* spec;
    HandleFn *finalize, *alloc;              // alloc: the model's part of the workspace
    EmbedFn *embed_wave, *embed_feat;        // embed_feat: from the mel power; null for a waveform model
    StageFn* stage;
    int max_lanes;                           // cap of SVHIP_LANES
    const char* optional_prefix;             // spec names that finalize may find absent (it checks them itself)
};
int unknown_stage(svhip_handle* h, const std::string& name);         // SVHIP_ERR_INVALID "unknown stage <name>"

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

// api_ecapa.hip, api_rawnet2.hip (the three RawNet2 models), api_rawnet3.hip, api_titanet.hip, api_conformer.hip, api_resnetse.hip: each
// model's functions
CheckFn ecapa_check, rawnet2_check, rawnet3_check, titanet_check, conformer_check, resnetse_check;
SpecFn ecapa_spec, rawnet2_spec, rawnet3_spec, titanet_spec, conformer_spec, resnetse_spec;
HandleFn ecapa_finalize, rawnet2_finalize, rawnet3_finalize, titanet_finalize, conformer_finalize, resnetse_finalize;
HandleFn ecapa_alloc, rawnet2_alloc, rawnet3_alloc, titanet_alloc, conformer_alloc, resnetse_alloc;
EmbedFn ecapa_embed_wave, rawnet2_forward, rawnet3_forward;                    // from the waveform
// a ragged ECAPA batch: utterance u is `frames[u]` frames long; in_off[u] is where it starts in `in` (samples of a device waveform array,
// wave; elements of a device feature array, features) or, with in_host, in the host array `in`
int ecapa_ragged_check(const svhip_config& c, const int32_t* lengths, int n, bool is_wave, std::string& err);
int ecapa_embed_ragged(svhip_handle* h, const float* in, bool in_host, bool is_wave, const int64_t* in_off, const int32_t* lengths, int n);
EmbedFn ecapa_forward, titanet_forward, conformer_forward, resnetse_forward;   // from the mel power
StageFn ecapa_stage, rawnet2_stage, rawnet3_stage, titanet_stage, conformer_stage, resnetse_stage;

}  // namespace svhip
