// kernels.h — internal launcher API of libsvhip (host side). All launchers enqueue on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "../../include/svhip.h"
#include "common.h"

namespace svhip {

// ---------------------------------------------------------------------------------------------
// One-time per-DEVICE setup flag.  hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the function on the
// CURRENT device only, so a launcher that raises a kernel's LDS limit keeps one bit per device ordinal (a process may
// own handles on several GPUs).  Lock-free: two threads racing on the same device both set the (idempotent) attribute.
// ---------------------------------------------------------------------------------------------
struct DeviceOnce {
    std::atomic<uint64_t> mask{0};
    bool done(int dev) const { return dev >= 0 && dev < 64 && ((mask.load(std::memory_order_acquire) >> dev) & 1u); }
    void mark(int dev) { if (dev >= 0 && dev < 64) mask.fetch_or(1ull << dev, std::memory_order_release); }
};
inline hipError_t set_max_dynamic_lds(DeviceOnce& once, const void* fn, int bytes) {
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (once.done(dev)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) once.mark(dev);
    return e;
}
// a 256-thread kernel over one parameter struct that needs `lds` bytes of dynamic LDS: raise its limit once per device, launch
template <class P, void (*Kernel)(P)>
hipError_t launch_max_lds(const dim3& grid, int lds, const P& p, hipStream_t stream) {
    static DeviceOnce attr;         // (one per kernel: a static of the template instance)
    if (hipError_t e = set_max_dynamic_lds(attr, reinterpret_cast<const void*>(Kernel), lds)) return e;
    hipLaunchKernelGGL(Kernel, grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Tiled MFMA GEMM with fused conv-gather prologue and bias/activation/BN epilogue.
//   Y[m, n] = act2( scale[n] * act1( sum_k A'[m, k] * W[n, k] + bias[n] (+ bias_utt[m / T, n]) ) + shift[n] )
// A' is A (frame-major, row stride lda) or, with taps > 1, the im2col view of a dilated 1-D
// convolution over the T rows of each utterance: k = tap*cin + c reads row t + (tap - taps/2)*dil
// (reflect or zero padded).  With A2 != nullptr the operand is A + A2 (Res2Net chain).
// W is packed [Np][Kp] (K contiguous; zero padded to the tile sizes) in the compute dtype.
// ---------------------------------------------------------------------------------------------
struct GemmParams {
    const void* A = nullptr;
    const void* A2 = nullptr;
    const void* W = nullptr;
    void* Y = nullptr;
    const float* bias = nullptr;
    const float* bias_utt = nullptr;
    const float* scale = nullptr;
    const float* shift = nullptr;
    // pw2 / pw3 only: per-utterance column sums of the output (pw2: of the bf16-rounded LDS output tile, 8 row groups of 32 rows
    // per tile; pw3: of the activated fp32 accumulators, 2 row groups of 128 rows — gemm_colsum_groups says which):
    //   colsum[((tile_m*RG + rg)*2 + seg) * N + n] = sum over the rows of row group rg that belong to
    //   utterance (tile_m*256 / T + seg); with colsum_sq the sums of squares follow at offset colsum_stride.
    float* colsum = nullptr;
    int colsum_sq = 0;
    int64_t colsum_stride = 0;
    const float* zeros = nullptr;    // >= N zero floats / >= N ones: stand-ins for absent bias / scale / shift vectors in the kernels that
    const float* ones = nullptr;     // read all three by DMA (gemm_pw3's 16-bit conv-gather form)
    const void* zero_page = nullptr; // >= 64 zero bytes (LDS-DMA source for padded k / out-of-range frames in the conv-gather pw2 path)
    void* Y2 = nullptr;             // gemm_pw3's Res2Net step form only: second output (the next step's input), row stride lda2
    const void* R = nullptr;        // optional residual (M, ldr) in the activation dtype, added last
    int ldr = 0;
    // conv-gather GEMMs on the 256 x 256 bf16 kernel only: K3 extra K columns appended after the taps * cin conv columns, read
    // from row m of a second matrix (the 1 x 1 shortcut of a RawNet2 block as part of conv2's GEMM: W is [N][K + K3], Kp = K + K3)
    const void* A3 = nullptr;
    int lda3 = 0, K3 = 0;
    // x3 == 2, pointwise form only: channels [0, side_c) of the output go to side_a and [side_c, 2 side_c) to side_b in the S32 split
    // layout (row strides in elements) INSTEAD of the fp32 output — the Res2Net pass-through chunk and the first step's input of
    // an F32X3 handle (side_c = C / 8 = 64 or 128)
    int y_s32 = 0;                  // x3 == 2, pointwise / conv-gather forms: Y is written in the S32 split layout (ldy in elements) instead of fp32
    void* side_a = nullptr;
    void* side_b = nullptr;
    int side_lda = 0, side_ldb = 0, side_c = 0;
    int num_cu = 256;               // compute units of the device (grid-size routing, gemm_route)
    int n128_off = 0;               // developer option n128_off: N = 128 layers stay on gemm_pw
    int cv_off = 0;                 // developer option cv_off: 16-bit conv-gather GEMMs stay on the per-tile kernel
    int pw3_cus = -1;               // developer option pw3_cus (svhip_set_option / SVHIP_PW3_CUS at create): the persistent kernels launch at most this
                                    // many workgroups, so that a small test problem walks several tiles per workgroup; 0: persistent kernels off
    const float* in_scale = nullptr; // gemm_pw3's X3 conv-gather form: (device) [0] = s, [1] = 1 / (s sw), [2] = s sw — A holds s * x, W holds sw * w (launch_in_scale):
                                    // the accumulators start at s sw * bias and the epilogue multiplies by 1 / (s sw) before the activation
    int tail_split = 1;             // persistent 16-bit GEMMs: a last partial round of <= G / 2 tiles is walked as column halves (gemm_pw3.hip)
    void* ts = nullptr;             // developer builds (SVHIP_GEMM_DEBUG, debug bit 16384): per-workgroup stage timestamps
    int M = 0, N = 0, K = 0, Kp = 0;
    int lda = 0, lda2 = 0, ldy = 0, ld_bu = 0;
    int T = 1;
    uint32_t t_magic = 0;     // gemm_pw3's gather forms: ceil(2^32 / T), filled by their launchers (frame index = row mod T without a division)
    int taps = 1, dil = 1, cin = 0, pad_mode = 0;
    int act1 = 0, act2 = 0;
    int out_f32 = 0;          // bf16 compute only: store fp32 instead of bf16
    int f16 = 0;              // 16-bit compute only: operands and outputs are fp16 (SVHIP_F16 handles), not bf16
    int x3 = 0;               // fp32 operands only: products as three bf16 MFMAs on hi / lo-split fragments.  1: gemm_pw expects W as
                              // (hi bf16 << 16 | lo bf16) words (ConvLayer::Wsplit), the generic kernel splits true fp32 W itself;
                              // 2: A and W are both in the S32 split layout (gemm_pw3's X3 form, launch_gemm_pw3x3)
    int debug = 0;            // developer ablations (tools/gemm_bench): 1 no loads in the loop, 2 no MFMA, 4 no epilogue
    int Wrows = 0;            // allocated rows of W (loads clamp to Wrows-1); packed weights: N rounded up to 128
    // segmented row gather (the generic kernel only; gemm_route sends such a GEMM there): with seg_off != null the operand is
    //   A'[m, k] = A[(m / seg_rows) * seg_utt + seg_off[m % seg_rows] + (k / seg_len) * seg_stride + k % seg_len]
    // — per utterance a table of row offsets and K made of K / seg_len contiguous runs (Conformer's strided 3 x 3 conv, conformer.hip)
    const int* seg_off = nullptr;
    int seg_rows = 0, seg_len = 0;
    int64_t seg_utt = 0, seg_stride = 0;
    // ... over a ragged batch (launch_gemm_ragged with rag_utt): m / seg_rows is a packed frame m' instead of an utterance, and the
    // frame's utterance shifts the row by whole runs:  A'[m, k] = A[m' * seg_utt + (rag_utt[m'] - seg_u0) * seg_stride +
    // seg_off[m % seg_rows] + (k / seg_len) * seg_stride + k % seg_len]  (Conformer: utterance u's conv1 rows start at 2 row0[u] + u)
    int seg_u0 = 0;
    // ragged batch (the generic kernel only, through launch_gemm_ragged): utterance u owns the rows [rag_row0[u], rag_row0[u + 1]) and
    // rag_utt[m] is the utterance of row m.  The conv gather reflects at each utterance's own ends and bias_utt is read at rag_utt[m];
    // T is not used.  Null (the default): every utterance has T rows.
    const int* rag_utt = nullptr;
    const int* rag_row0 = nullptr;
};

constexpr int GEMM_BM = 128;
constexpr int GEMM_BN = 128;
constexpr int GEMM_BK_BYTES = 128;   // K-step = 128 bytes per row: 32 fp32 or 64 bf16

inline int gemm_bk(bool bf16) { return bf16 ? 64 : 32; }
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

hipError_t launch_gemm(const GemmParams& p, bool bf16, hipStream_t stream);
// pointwise fast path (gemm_pw.hip): 256 x 128 tiles, LDS-DMA ring; launch_gemm routes to it when supported
// Which kernel launch_gemm runs for a shape (the profile labels of api_gemm.hip's conv_gemm name the same choice):
//   PW2        256 x 256 role-staggered bf16 kernel (gemm_pw2.hip)
//   PW_NARROW  gemm_pw's 256 x 128 tile: a pw2 grid of at most half the CUs finishes in one round either way, and the half-size
//              tile takes about half as long (RawNet2 blocks 6 / 7, 86 tiles: 370 -> 470 - 510 TFLOP/s)
//   PW         gemm_pw with its default tile;  GENERIC  the register-staged kernel of gemm.hip
//   PW3        the persistent form of PW2 with the epilogue taken from the accumulators (gemm_pw3.hip): plain pointwise layers
//              with more tiles than CUs (ECAPA's tdnn1 / tdnn2 / mfa)
//   PW3CV      the persistent kernel's conv-gather form on 16-bit operands: k = 3 / 5 convolutions with cin % 64 == 0 and more tiles
//              than CUs (RawNet2 blocks 2 - 5, ECAPA blocks.0 with padded input rows)
//   N128       bf16 pointwise layers with N = 128 and the ReLU -> BN -> tanh epilogue (ECAPA's asp.tdnn): 128 x 128 tiles, two workgroups
//              per CU (gemm_n128.hip), every batch size
enum GemmRoute : int { ROUTE_PW2 = 0, ROUTE_PW = 1, ROUTE_PW_NARROW = 2, ROUTE_GENERIC = 3, ROUTE_PW3 = 4, ROUTE_PW3CV = 5, ROUTE_N128 = 6 };
GemmRoute gemm_route(const GemmParams& p, bool bf16);
bool gemm_pw_supported(const GemmParams& p, bool bf16);
hipError_t launch_gemm_pw(const GemmParams& p, bool bf16, hipStream_t stream, bool narrow = false);
// bf16 256 x 256 role-staggered variant for the big layers (gemm_pw2.hip); launch_gemm_pw routes to it
bool gemm_pw2_supported(const GemmParams& p, bool bf16);
hipError_t launch_gemm_pw2(const GemmParams& p, hipStream_t stream);
// persistent variant (gemm_pw3.hip); pw3_grid_cap: workgroups it launches at most (the CU count, or the developer override
// SVHIP_PW3_CUS, which lets small test problems run more than one tile per workgroup)
bool gemm_pw3_supported(const GemmParams& p, bool bf16);
hipError_t launch_gemm_pw3(const GemmParams& p, hipStream_t stream);
int pw3_grid_cap(const GemmParams& p);
// the X3 form of the persistent kernel (x3 == 2): A (M, K) and W (N, K) in the S32 split layout (per row, per 32 k: 32 hi bf16 |
// 32 lo bf16), fp32 output, exact GELU + BN affine, optional column sums: the GELU layers of SVHIP_F32X3 handles
bool gemm_pw3x3_supported(const GemmParams& p);
hipError_t launch_gemm_pw3x3(const GemmParams& p, hipStream_t stream);
bool r2_step_supported(const GemmParams& p);               // r2_step.hip: the Res2Net step on 128 x 128 tiles, two workgroups per CU (cin = 128)
hipError_t launch_r2_step(const GemmParams& p, hipStream_t stream);
// RawNet2's 128 -> 128, k = 3 convolutions on F32X3 handles (r2_step.hip, modes 1 / 2): S32 operands, zero padding (GemmParams::zero_page),
// mode 1: S32 output of lrelu0.3(BN(.)); mode 2: fp32 output of conv (+ R)
bool rn_step_supported(const GemmParams& p, int mode);
hipError_t launch_rn_step(const GemmParams& p, int mode, hipStream_t stream);
bool gemm_pw3cv_supported(const GemmParams& p);          // conv-gather X3 form (odd taps, reflect): see gemm_pw3.hip
hipError_t launch_gemm_pw3cv(const GemmParams& p, hipStream_t stream);
bool gemm_n128_supported(const GemmParams& p);           // gemm_n128.hip
hipError_t launch_gemm_n128(const GemmParams& p, hipStream_t stream);
bool gemm_pw3cv16_supported(const GemmParams& p);        // conv-gather form on bf16 / fp16 operands (reflect or zero padding)
hipError_t launch_gemm_pw3cv16(const GemmParams& p, hipStream_t stream);
// one Res2Net step of an F32X3 handle on the same kernel (dilated k = 3 conv gathered from an S32 input, outputs in S32)
bool gemm_pw3r2_supported(const GemmParams& p);
hipError_t launch_gemm_pw3r2(const GemmParams& p, hipStream_t stream);
// fp32 (M, K) rows (stride ld) -> S32 layout, rows of ldd elements (4 bytes each; 0: dense, ldd = K)
hipError_t launch_split_s32(const float* src, int ld, void* dst, int64_t M, int K, hipStream_t stream, int ldd = 0, int kvalid = 0,
                            const float* scale = nullptr);      // scale (device, optional): [0] = a power of two every value is multiplied by
// the input scale of an F32X3 handle's first convolution: scale[0] = s, scale[1] = 1 / s from the max |x| of X (elementwise.hip)
hipError_t launch_in_scale(const float* X, int64_t n, uint32_t* part256, float* scale, hipStream_t stream, float wscale = 1.0f);
hipError_t launch_unsplit_s32(const void* src, int lds32, float* dst, int ld, int64_t M, int K, hipStream_t stream);   // v = hi + lo
// row groups per 256-row tile in the column-sum partials the routed kernel writes (8: pw2, 2: pw3)
int gemm_colsum_groups(const GemmParams& p, bool bf16);
// a GEMM of a ragged batch (fp32 / bf16; fp16 with p.f16: RawNet2's instances): ALWAYS the generic kernel, whatever M is — gemm_route picks its kernel by the size of the
// problem, and the kernels add a row's K products in different orders, so a routed GEMM would make an utterance's values depend on
// what it is packed with.  With rag_utt / rag_row0 the conv gather and bias_utt follow the segment table (GemmParams).
hipError_t launch_gemm_ragged(const GemmParams& p, bool bf16, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Ragged batches: n utterances of T_u frames packed back to back; row0 (n + 1 ints) holds each utterance's first row
// and the total, utt (M ints) the utterance of every row (ragged.hip).  Every reduction over time is one workgroup per (utterance, channel
// block) that walks the utterance's own frames in an order fixed by the frame index: a value never depends on the neighbours.  These
// launch the fixed-length kernels' own bodies (RAG instances in elementwise.hip, packed entries in fbank.hip), so the two forms cannot
// drift apart.
// ---------------------------------------------------------------------------------------------
hipError_t launch_rag_rows(const int* row0, int n, int maxT, int* utt, hipStream_t stream);
// features: utterance u is a (n_mels, T_u) fp32 block at feat + feat_off[u] -> rows row0[u] .. of out (M, n_mels) in the compute type:
// log(x + 1e-6) minus its time mean (log_input), InstanceNorm1d with affine (in_w != null); stats: n * n_mels * 2 floats of scratch
hipError_t launch_rag_prologue(const float* feat, const int64_t* feat_off, const int* row0, int n, int maxT, void* out, bool out_bf16,
                               int n_mels, int log_input, const float* in_w, const float* in_b, float* stats, hipStream_t stream);
// out (n, ld_out) = mean over each utterance's frames of X[:, 0:C) [| population std, two passes, variance clamped below at eps]
hipError_t launch_rag_colstats(const void* X, bool bf16, int ldx, const int* row0, int n, int C, float* out, bool with_std, float eps,
                               hipStream_t stream);
// out[m, c] = h[m, c] * s[utt[m], c] + x[m, c]
hipError_t launch_rag_se_apply(const void* h, int ldh, const float* s, const void* x, int ldx, void* out, int ldo, bool bf16,
                               const int* utt, int M, int C, hipStream_t stream);
// launch_asp_pool's arithmetic over each utterance's own frames
// (var_max > 0: the variance is also clamped above, as launch_asp_pool's — the Conformer's clamp(1e-4, 1e4))
hipError_t launch_rag_asp_pool(const float* logits, const void* X, bool bf16, int ldx, const int* row0, int n, int C, const float* bn_scale,
                               const float* bn_shift, float* pooled_raw, float* pooled_bn, float eps, hipStream_t stream, float var_max = 0.0f);
// launch_rowvec_linear on ONE kernel at every batch size (a row's sum does not depend on how many rows ride along)
hipError_t launch_rag_linear(const float* in, int ld_in, const float* W, const float* bias, float* out, int ld_out, int n, int N, int K,
                             int act, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Fused Res2Net chain (bf16 path): one workgroup per utterance runs the 7 dependent dilated convs
// of one SE-Res2Net block with the conv input resident in LDS (res2net.hip).
// H1 = tdnn1 output (M, ld), H2 = chain output (M, ld): y_0 = c_0, y_j = BN(ReLU(conv(c_j + y_{j-1}))).
// ---------------------------------------------------------------------------------------------
struct Res2Params {
    const void* H1 = nullptr;
    void* H2 = nullptr;
    int ld = 0, T = 0, dil = 1, Kp = 0;
    const void* W[7] = {};       // packed [>= C/8 rows][Kp] bf16, k = tap * C/8 + c
    const float* bias[7] = {};
    const float* scale[7] = {};
    const float* shift[7] = {};
    int debug = 0;               // tools/res2_bench ablations (only read in -DSVHIP_GEMM_DEBUG builds)
    unsigned long long* ts = nullptr;   // the same builds, debug bit 64: per workgroup [8 stages][4] cycle totals {taps, epilogue, row pass, -}
    int slices = 1;              // > 1: every utterance is cut into this many time slices, one workgroup each (res2net_chain_slices)
    int Tc = 0;                  // filled by the launcher: core frames per slice
};
bool res2net_chain_supported(int C, int T, int dil, int Kp);
int res2net_chain_slices(int B, int C, int T, int dil, int num_cu);
hipError_t launch_res2net_chain(const Res2Params& p, int B, int C, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Mel front-end
// ---------------------------------------------------------------------------------------------
struct FbankTables {           // device pointers, built once per handle
    const float* basis = nullptr;      // [q][tile][lane] float4: windowed cos/sin taps laid out for MFMA B operands
    const void* basis_hi = nullptr;    // bf16x3 path: [k16][pair][part][lane] 8 x bf16 (hi / lo parts of the same taps)
    const void* basis_lo = nullptr;
    const void* basis_l3 = nullptr;    // bf16x6 path (F32X3 handles): the third part of the exact split basis = hi + lo + l3
    const void* sym_hi = nullptr;      // fused front-end (bf16 handles): [7 k steps][8 bin groups][cos | sin][lane] 8 x bf16 of the symmetric basis
    const void* sym_lo = nullptr;      //   w_m cos(2 pi k m / 512) | w_m sin(2 pi k m / 512), m = 0 .. 100 (fbank.hip, "the fused front-end")
    int split6 = 0;
    int n_k16 = 13;                    // ceil(win_length / 16)
    int split_bf16 = 0;                // 1: bf16x3 DFT (bf16-compute handles)
    const float* mel_w = nullptr;      // packed non-zero mel weights
    int n_melw = 0;                    // number of packed weights
    const int* mel_start = nullptr;    // [n_mels] first bin
    const int* mel_len = nullptr;      // [n_mels] number of bins
    const int* mel_off = nullptr;      // [n_mels] offset into mel_w
    int n_fft = 512, win_length = 200, hop = 80, n_mels = 80, n_bins = 257, lpad = 156;
    int n_pairs = 9;                   // ceil(n_bins / 32) re/im tile pairs
    int n_q = 25;                      // win_length / 8
    int mel_max_bin = 256;             // highest bin with a non-zero mel weight
    int force32 = 0;                   // developer option fbank32: the 32-frame kernel whatever the bank
    float preemph = 0.97f;
};
// wav (B, L) fp32 -> mel power (B, n_mels, T) fp32
hipError_t launch_fbank(const FbankTables& tb, const float* wav, int B, int L, int T, float* mel, hipStream_t stream);
// the largest dynamic LDS launch_fbank sends for these (complete) tables, and the most its kernels are allowed: a geometry above the
// limit, or above what the device offers one workgroup, is refused when the handle is created, never at its first launch
size_t fbank_lds_needed(const FbankTables& tb);
size_t fbank_lds_limit();

// round 6, bf16 handles: wav (B, L) -> the 16-bit frame-major operand of blocks.0 (log-mel minus its time mean) in two launches
bool fbank_fused_supported(const FbankTables& tb, int L);
hipError_t launch_fbank_fused(const FbankTables& tb, const float* wav, int B, int L, int T, int log_input, float* logmel, float* partial,
                              void* out, hipStream_t stream);

// (B, n_mels, T) fp32 features -> frame-major (B, T, n_mels) activations in the compute dtype,
// with optional log(x+1e-6) - mean_t and optional InstanceNorm1d(affine).
// `stats` is a (B * n_mels * 2) fp32 scratch buffer.
hipError_t launch_prologue(const float* feat, void* out, bool out_bf16, int B, int n_mels, int T,
                           int log_input, const float* in_w, const float* in_b, float* stats, hipStream_t stream,
                           uint32_t* status = nullptr, uint32_t* host_flag = nullptr, float limit = 3.0e38f);       // range guard: fbank.hip

// ---------------------------------------------------------------------------------------------
// Frame-major reductions / elementwise (activation dtype templated inside)
// ---------------------------------------------------------------------------------------------
// mean over the T rows of each utterance: X (B*T, ldx) cols [0,C) -> mean (B, C) fp32
// (optional scratch of B * scratch_slices * C floats: long T with few channels is reduced in two stages)
hipError_t launch_colmean(const void* X, int dt, int ldx, int B, int T, int C, float* mean, hipStream_t stream,
                          float* scratch = nullptr, int scratch_slices = 0);
// mean and population std over T (two pass, clamp 1e-12 as ECAPA_TDNN.py:222-227): -> stats (B, 2C) = [mean | std]
hipError_t launch_colstats(const void* X, bool bf16, int ldx, int B, int T, int C, float* stats, float eps, hipStream_t stream);
// out[b, n] = act( bias[n] + sum_k W[n, k] * in[b, k] ), all fp32 (small-M linear layers)
// `part` (optional, rowvec_linear_scratch_bytes(B, N, K) > 0 bytes): full batches (B > 64) of long rows (K a multiple of 384, >= 3 072) run on the
// exact fp32 MFMA with K split over workgroups and the slices added in a fixed order
// `short_rows`: also rows that are a multiple of 256 (>= 1 024) but not of 384, on slices of 256 (RawNet2's fc, 16-bit handles)
size_t rowvec_linear_scratch_bytes(int B, int N, int K, bool short_rows = false);
hipError_t launch_rowvec_linear(const float* in, int ld_in, const float* W, const float* bias, float* out, int ld_out,
                                int B, int N, int K, int act, hipStream_t stream, float* part = nullptr, bool short_rows = false);
// the embeddings leave the workspace (dst == src: no copy) and the call's numeric status is recorded: a non-finite value raises bit 0 of
// status[0], is counted in status[1] and sets *host_flag (mapped pinned memory).  SVHIP_STATUS_* bits: api.hip
hipError_t launch_emb_out(const float* src, float* dst, int n, uint32_t* status, uint32_t* host_flag, hipStream_t stream);

// The attention head of Raw_ECAPA_hype (fusion_head.hip): out (B, nOut) from the branch embeddings e1 (B, d1) | e2 (B, d2), d1 + d2 ==
// HYPE_HEAD_C, in one launch, fp32.  s0 / t0, s2 / t2, sF / tF: bn_before_agg, attention.2 and bn_final folded to scale / shift; the
// weights K-major: W0t [704][128] = attention.0, W3t [128][704] = attention.3, Wft [1408][nOutP] = fc with the rows padded with zeros to
// nOutP = nOut rounded up to 4.  The kernel checks what it writes for inf / NaN (status / host_flag as launch_emb_out).  A row's output
// does not depend on B or on its place in the batch, bit for bit.
constexpr int HYPE_HEAD_C = 704, HYPE_HEAD_A = 128, HYPE_HEAD_UT = 4, HYPE_HEAD_COLS = 128;       // channels, attention width; utterances and output columns per workgroup
struct HypeHeadParams {
    const float *e1, *e2;
    int d1, d2, B, nOut, nOutP;
    const float *s0, *t0, *W0t, *b0, *s2, *t2, *W3t, *b3, *sF, *tF, *Wft, *bf;
    float* out;
    uint32_t* status;
    volatile uint32_t* host_flag;
};
hipError_t launch_hype_head(const HypeHeadParams& p, hipStream_t stream);
// s[b, :] = sigmoid(W2 relu(W1 mean[b, :] + b1) + b2); W1 [H][C], W2T = W2 transposed [H][C]
hipError_t launch_se_mlp(const float* mean, const float* part, int T, const void* W1, const float* b1, const void* W2T,
                         const float* b2, float* s, bool w_bf16, int B, int C, int H, hipStream_t stream, int row_groups = 8);
// out[(b,t), c] = h[(b,t), c] * s[b, c] + x[(b,t), c]   (SE gate + residual, ECAPA_TDNN.py:177,336)
// (fp32: s32 != null also writes out in the S32 split layout, row stride ld32 elements of 4 bytes: gemm_pw3's X3 A operand)
hipError_t launch_se_apply(const void* h, int ldh, const float* s, const void* x, int ldx, void* out, int ldo,
                           bool bf16, int B, int T, int C, hipStream_t stream, void* s32 = nullptr, int ld32 = 0, const void* x32 = nullptr, int ldx32 = 0);
// reduce the pw2 column-sum partials: out (B, C) = mean over T  [and out (B, 2C) = [mean | std] with sq]
hipError_t launch_colsum_finalize(const float* part, int64_t sq_stride, bool with_std, int B, int T, int C, int M,
                                  float* out, float eps, hipStream_t stream, int row_groups = 8);
// fp32 matrix -> (hi bf16 << 16 | lo bf16) words (the pre-split weight operand of gemm_pw's F32X3 path)
hipError_t launch_split_words(const float* src, void* dst, int64_t n, hipStream_t stream);
// eval-mode crops of int16 PCM files (back to back in `pcm`) -> (n_files * num_eval, L) fp32, 1/32768 scaling
hipError_t launch_crop_pcm16(const int16_t* pcm, const int64_t* off, const int32_t* len, int n_files, int num_eval, int L,
                             float* out, hipStream_t stream);
// strided 2-D copy of a column block: dst[m, 0:C) = src[m, 0:C)
hipError_t launch_copy_cols(const void* src, int lds, void* dst, int ldd, bool bf16, int M, int C, hipStream_t stream);
// attentive statistics: softmax over T of logits (fp32, ld = C), weighted mean / std of X, then
// BatchNorm affine over the 2C pooled values -> pooled (B, 2C) fp32   (ECAPA_TDNN.py:252-259,496)
// The variance is clamped below at eps and, with var_max > 0, above at var_max (Conformer's [1e-4, 1e4]; 0: no upper clamp)
hipError_t launch_asp_pool(const float* logits, const void* X, bool bf16, int ldx, int B, int T, int C,
                           const float* bn_scale, const float* bn_shift, float* pooled_raw, float* pooled_bn,
                           float eps, float var_max, hipStream_t stream);

// Fused attention tail (bf16 path, asp_fused.hip): logits = conv1x1(att) + b, softmax over T, weighted
// mean / std of X, BatchNorm affine -> pooled (B, 2C).  The logits never reach memory.
struct AspFusedParams {
    const void* att = nullptr;      // (B*T, 128) bf16
    const void* W = nullptr;        // asp.conv packed [>= C rows][Kp = 128] bf16
    const float* bias = nullptr;    // [C]
    const void* X = nullptr;        // (B*T, ldx) bf16, the mfa output
    const float* bn_scale = nullptr;
    const float* bn_shift = nullptr;
    float* pooled_raw = nullptr;    // optional (B, 2C)
    float* pooled_bn = nullptr;     // (B, 2C)
    int ldx = 0, T = 0, C = 0, Kp = 0;
    float eps = 1e-12f;
    unsigned long long* dbg = nullptr;   // tools/asp_bench: per-phase s_memtime totals of wave 0 (only read in -DSVHIP_GEMM_DEBUG builds)
};
bool asp_fused_supported(int T, int C, int att_channels, int Kp);
hipError_t launch_asp_fused(const AspFusedParams& p, int B, hipStream_t stream);

// the same fusion for SVHIP_F32X3 handles (asp_x3.hip): fp32 att and x, logits as split-bf16 MFMA triples, never stored
struct AspX3Params {
    const float* att = nullptr;     // (B*T, 128) fp32, asp.tdnn's output
    const void* Ws32 = nullptr;     // asp.conv in the S32 split layout: [C rows][128 k]: per 32 k, 32 hi | 32 lo bf16
    const float* X = nullptr;       // (B*T, ldx) fp32, the mfa output
    const float* mref = nullptr;    // (B, mref_ld): the plain mean over time of every channel of X (the shift of the moments)
    const float* bn_scale = nullptr;
    const float* bn_shift = nullptr;
    float* pooled_raw = nullptr;    // optional (B, 2C)
    float* pooled_bn = nullptr;     // (B, 2C)
    int ldx = 0, mref_ld = 0, T = 0, C = 0, B = 0;
    float eps = 1e-12f;
};
hipError_t launch_asp_bf16(const AspFusedParams& p, const float* mref, int mref_ld, int B, hipStream_t stream);      // asp_x3.hip: the bf16 form of asp_x3
bool asp_x3_supported(int T, int C, int att_channels, int K);
hipError_t launch_asp_x3(const AspX3Params& p, int B, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// RawNet2 (rawnet2.hip)
// ---------------------------------------------------------------------------------------------
// (xn: optional bf16 copies of the LayerNorm output, per utterance two zero-tailed rows of Lp >= L + RN_XN_TAIL samples (Lp % 64
//  == 0): sample j at index j, then sample j + 1 at index j — the operand of the bf16 sinc kernel, which reads up to 470 samples
//  past its last tile's first sample)
constexpr int RN_XN_TAIL = 512;
// (xn_lo: the split form of F32X3 handles — FOUR rows of Lp halves per utterance: hi parts of the two copies, then their lo parts)
hipError_t launch_rn_ln_stats(const float* wav, int B, int L, float* stats, hipStream_t stream, void* xn = nullptr, int Lp = 0,
                              const float* gamma = nullptr, const float* beta = nullptr, int xn_dt = DT_BF16, bool xn_lo = false);
// the sinc front-end on three fp16 MFMAs per product (F32X3 handles): filt_planes = [2][128][256] halves (hi | lo), fp32 out
// (pre_s32: optional second output lrelu0.3(next_scale * out + next_shift) in the S32 split layout, (B * T1, 128))
hipError_t launch_rn_sinc_x3(const void* filt_planes, const float* bn_scale, const float* bn_shift, float* out, int B, int L, int T1,
                             const void* xn, int Lp, int num_cu, hipStream_t stream, void* pre_s32 = nullptr, const float* next_scale = nullptr,
                             const float* next_shift = nullptr);
// LayerNorm + sinc conv (k=251) + abs + maxpool3 + BN + LeakyReLU(0.3): wav (B, L) -> out (B, T1, 128), T1 = (L-250)/3
hipError_t launch_rn_sinc(const float* wav, const float* stats, const float* gamma, const float* beta, const void* filt,
                          const float* bn_scale, const float* bn_shift, void* out, int dt, int B, int L, int T1,
                          hipStream_t stream, void* pre = nullptr, const float* next_scale = nullptr, const float* next_shift = nullptr,
                          const void* xn = nullptr, int Lp = 0, int num_cu = 256, bool sym = false);
// (sym, DT_F16 only: `filt` is the [128][128] slot-major table of the symmetric form — rawnet2.hip, rn_sinc_kernel<.., SYM>)
// (dt: DT_F32 / DT_BF16 / DT_F16 — the storage type of the activations)
// (y_s32 / pre_s32, fp32 only: that output in the S32 split layout — the operand of the split convolution kernels — instead of fp32)
// RawNet2 'conv' front-end (rn_conv3.hip): x (B, T1, 128) in dt = Conv1d(1, 128, 3, stride 3) of wav (B, L) fp32, T1 = (L - 3) / 3 + 1;
// cw = [w0 | w1 | w2 | bias] x 128 floats
hipError_t launch_rn_conv3_front(const float* wav, const float* cw, void* x, int dt, int B, int L, int T1, hipStream_t stream);
hipError_t launch_rn_bn_act(const void* x, void* y, int dt, const float* scale, const float* shift, int64_t rows, int C,
                            float slope, hipStream_t stream, bool y_s32 = false);
hipError_t launch_rn_maxpool3(const void* x, void* y, int dt, int B, int Tin, int C, hipStream_t stream);
hipError_t launch_rn_afms_apply(const void* x, void* y, int dt, const float* alpha, const float* s, int B, int T, int C,
                                hipStream_t stream, const float* next_scale = nullptr, const float* next_shift = nullptr,
                                void* pre = nullptr, float slope = 0.3f, bool pre_s32 = false);
// fused block tail (rawnet2.hip): [max_pool1d(3)] + AFMS + the next consumer's lrelu(bn(.)), one workgroup per utterance with the
// pooled activation held in registers; rn_tail_supported says whether (Tn, C) fits (else the four separate passes run)
bool rn_tail_supported(int dt, int Tn, int C);
hipError_t launch_rn_tail(const void* x, void* y, void* pre, int dt, bool pool, const float* alpha, const float* WT, const float* bias,
                          const float* next_scale, const float* next_shift, int B, int Tin, int C, float slope, hipStream_t stream,
                          const void* res = nullptr, float* part = nullptr, float* gate = nullptr, int num_cu = 0, bool pre_s32 = false);
// small batches (B * 4 <= num_cu) with `part` (B x 16 x C floats) and `gate` (B x C floats): the utterance in frame slices over several
// workgroups (slice sums -> rn_afms_gate -> apply); returns the slice count, 0 = the one-workgroup-per-utterance kernel
int rn_tail_slices(int dt, int B, int Tn, int C, int num_cu);       // res: the block input, added to x before the pool (16-bit handles; see rn_tail_kernel)
// Fused 128 -> 128 pooled RawNetBasicBlock (rn_block128.hip, bf16): previous block's AFMS gate on the way in, BN + LeakyReLU,
// conv1 + BN + LeakyReLU, conv2 + identity shortcut, max_pool1d(3), per-tile column sums of the pooled output.
struct RnBlock128Params {
    const bf16_t* xin = nullptr;         // (B, T, 128): the stage input before the previous block's gate
    const float* alpha = nullptr;        // [128] previous block's AFMS alpha, or null (first block)
    const float* gate = nullptr;         // (B, 128) previous block's AFMS sigmoid(fc(mean)), or null
    const float* bn1_scale = nullptr;    // [128] folded bn1
    const float* bn1_shift = nullptr;
    const bf16_t* W1 = nullptr;          // packed [128][384], k = tap * 128 + c
    const float* bn2_scale = nullptr;    // [128] folded bn2 (conv1's epilogue)
    const float* bn2_shift = nullptr;
    const bf16_t* W2 = nullptr;
    bf16_t* opool = nullptr;             // (B, T / 3, 128)
    float* colsum = nullptr;             // (B, rn_block128_nparts(B, T, num_cu), 128) partial sums of opool over pooled frames
    int B = 0, T = 0, Tout = 0, ntiles = 0;
    int per_wg = 0, nseg = 0;            // filled by the launcher: items per workgroup, workgroups that can share an utterance
    unsigned long long* dbg = nullptr;   // tools/rb_bench: per-workgroup phase cycle totals (only read in -DSVHIP_GEMM_DEBUG builds)
    int debug = 0;                       // tools/rb_bench ablations (debug builds): 1 no fragment reads, 2 no MFMA, 4 no conversion, 8 no pool
    int f16 = 0;                         // the 16-bit tensors (xin, W1, W2, opool) hold fp16, not bf16
    // RawNet2 'conv' front-end fused into block 0 (xin unused, no gate): the item's input rows are computed from the waveform
    // (B, L) fp32 as rn_conv3_front would store them; cw = [w0 | w1 | w2 | bias] x 128 floats.  T = (L - 3) / 3 + 1.
    const float* wav = nullptr;
    const float* cw = nullptr;
    int L = 0;
};
int rn_block128_ntiles(int T);
int rn_block128_nparts(int B, int T, int num_cu);
bool rn_block128_supported(int cin, int cout, int T, bool downsample, bool has_shortcut, int Kp1, int Kp2);
hipError_t launch_rn_block128(const RnBlock128Params& p, int num_cu, hipStream_t stream);
// AFMS gate from partial column sums: s (B, C) = sigmoid(fc(sum(part) / Tn)); part (B, nparts, C), WT = fc weight TRANSPOSED [C][C] fp32
hipError_t launch_rn_afms_gate(const float* part, int nparts, int B, int C, int Tn, const float* WT, const float* bias, float* s,
                               hipStream_t stream);
hipError_t launch_rn_attn_pool(const float* logits, const void* x, int dt, int B, int T, int C, float* out, hipStream_t stream);
// RawNet2 'conv' over a ragged pack (rn_ragged.hip): n utterances packed back to back at seven frame levels (T1_u = len_u / 3, then / 3
// per pooled block), each level described by its row0 table (n + 1 device ints).  No grid, slice length or kernel choice depends on n,
// on the neighbours or on the device: an utterance's values are bit for bit the same in every pack.
//   front     utterance u = len[u] samples at wav + off[u] (device tables) -> x rows row0[u] .. (rn_conv3_front's value) and, from the
//             value as stored, pre = lrelu(bn_scale x + bn_shift) (rn_bn_act's value); maxT1 >= every T1_u
//   slices    slice0[l * ld + u] = the first slice of utterance u at level l when every utterance is cut into slices of
//             RN_RAG_SLICE frames (slice0[l * ld + n]: the level's slice count); row0 + l * ld is level l's table
//   tail      rn_tail_part / rn_afms_gate / rn_tail_apply over the slices of the OUT level (nslices of them, counted on the host):
//             part (nslices, C) = the column sums of each slice of [max_pool1d(3) of] the utterance's in-level rows; gate (n, C) =
//             sigmoid(fc(sum of the utterance's slice sums in slice order / Tn_u)); apply forms the pooled value again and writes
//             y = (v + alpha) gate (null: nothing reads it) and pre = lrelu(nscale y + nshift) from y in fp32, before its rounding
//   attn_pool softmax over the utterance's own frames of the fp32 logits, weighted mean and sqrt(max(sum w (x - m)^2, 1e-5)) -> out (n, 2 C)
constexpr int RN_RAG_SLICE = 48;
hipError_t launch_rn_rag_front(const float* wav, const int64_t* off, const int32_t* len, const int* row0, int n, int maxT1, const float* cw,
                               const float* bn_scale, const float* bn_shift, float slope, void* x, void* pre, int dt, hipStream_t stream);
hipError_t launch_rn_rag_slices(const int* row0, int ld, int levels, int n, int* slice0, hipStream_t stream);
hipError_t launch_rn_rag_tail_part(const void* x, int dt, bool pool, const int* row0_in, const int* row0_out, const int* slice0, int n, int nslices,
                                   int C, float* part, hipStream_t stream);
hipError_t launch_rn_rag_gate(const float* part, const int* row0_out, const int* slice0, int n, int C, const float* WT, const float* bias, float* gate,
                              hipStream_t stream);
hipError_t launch_rn_rag_tail_apply(const void* x, int dt, bool pool, const int* row0_in, const int* row0_out, const int* slice0, int n, int nslices,
                                    int C, const float* alpha, const float* gate, const float* nscale, const float* nshift, float slope, void* y,
                                    void* pre, hipStream_t stream);
hipError_t launch_rn_rag_attn_pool(const float* logits, const void* x, int dt, const int* row0, int n, int C, float* out, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// RawNet2's GRU aggregation (gru.hip): one launch per time step of h' = GRU(gi_t, h), hidden size 1024
// ---------------------------------------------------------------------------------------------
constexpr int RN_GRU_HIDDEN = 1024;
// Wp: W_hh (3072, 1024) in the gate-interleaved packing of gru.hip, element type by dt (DT_F32 / DT_BF16 / DT_F16); gi: (B, T, 3072) fp32
// input projections (b_ih, b_hr, b_hz folded in); b_hn (1024); h_in (B, 1024) fp32 or null (h = 0); h_out (B, 1024) fp32, not h_in
hipError_t launch_rn_gru_step(const void* Wp, int dt, const float* gi, const float* b_hn, const float* h_in, float* h_out, int B, int T, int t,
                              hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// RawNet3 (rawnet3.hip)
// ---------------------------------------------------------------------------------------------
constexpr int RN3_FILTERS = 256, RN3_TAPS = 251, RN3_STRIDE = 10;     // ParamSincFB(256, 251, stride=10) (RawNet3.py:35-41)
constexpr int RN3_MIN_SAMPLES = 541;       // T0 = 30 frames -> 6 -> 2: the shortest input whose pooled statistics are finite
// pre-emphasis [f0, f1] (the checkpoint's preprocess.0.flipped_filter) + InstanceNorm1d(1, eps 1e-4, affine in_w / in_b) + the
// sinc filterbank (filt: [251][256] tap-major, fp64 when filt_f64, else fp32) + log(|.| + 1e-6): wav (B, L) -> y (B, T0, 256) fp32,
// T0 = (L - 251) / 10 + 1; stats: (B, 2) doubles of scratch
hipError_t launch_rn3_front(const float* wav, int B, int L, int T0, double f0, double f1, const float* in_w, const float* in_b, const void* filt,
                            bool filt_f64, double* stats, float* y, hipStream_t stream);
// x0 (B, T0, 256) in dt = y - mean[b, :] (the time mean, colmean of y); y and x0 may alias (fp32)
hipError_t launch_rn3_center(const float* y, const float* mean, void* x0, int dt, int B, int T0, hipStream_t stream);
// MaxPool1d(P) over frames: x (B * Tin, ldx) -> y (B * (Tin / P), ldy), columns [0, C)
hipError_t launch_rn3_maxpool(const void* x, int ldx, void* y, int ldy, int dt, int B, int Tin, int C, int P, hipStream_t stream);
// AFMS apply: y = (x + alpha) * gate[b] (gate (B, C) fp32); with `sum`: sum = y + add in the same pass
hipError_t launch_rn3_afms(const void* x, int ldx, const float* alpha, const float* gate, void* y, int ldy, const void* add, int ldadd, void* sum, int ldsum,
                           int dt, int B, int Tn, int C, hipStream_t stream);
// stats (B, 2C) fp32 = [mean_t x | sqrt(clamp(unbiased var_t x, 1e-4, 1e4))]
hipError_t launch_rn3_tstats(const void* x, int ldx, int dt, int B, int Tn, int C, float* stats, hipStream_t stream, const int* row0 = nullptr);
// single-head context pooling: logit (B * Tn) = hatt . w2 + b2 (hatt (B * Tn, 128)), softmax over Tn, weighted mean / std of x, bn5 affine
// -> pooled (B, 2C) fp32; NaN for an utterance whose in_stats (rn3_prenorm's (B, 2) statistics of the waveform) are not finite
hipError_t launch_rn3_ctx_pool(const void* hatt, int ldh, const float* w2, const float* b2, float* logit, const void* x, int ldx, int dt, int B, int Tn, int C,
                               const float* bn_scale, const float* bn_shift, const double* in_stats, float* pooled, hipStream_t stream,
                               const int* row0 = nullptr, int64_t rows = 0);
// The same kernels over a ragged pack: n utterances packed back to back at each frame level, a level's rows described by its row0
// (n + 1) / utt (M) tables (ragged.hip).  launch_rn3_tstats / launch_rn3_ctx_pool take the level-2 row0 (B = n; Tn: any positive
// value, unused; rows: the level's row count); the others have their own entry:
//   front     utterance u = len[u] samples at wav + off[u] (device tables) -> y rows row0[u] .. (two launches for the whole pack)
//   center    x0[m] = y[m] - mean[utt[m]]
//   maxpool   output row m (utterance u = utt_out[m], frame t = m - row0_out[u]) = max of the input rows row0_in[u] + P t .. + P - 1:
//             an utterance's T_u % P left-over frames are dropped
//   afms      the gate row is utt[m]
hipError_t launch_rn3_rag_front(const float* wav, const int64_t* off, const int* len, const int* row0, int n, int maxT0, double f0, double f1,
                                const float* in_w, const float* in_b, const void* filt, bool filt_f64, double* stats, float* y, hipStream_t stream);
hipError_t launch_rn3_rag_center(const float* y, const float* mean, void* x0, int dt, const int* utt, int M, hipStream_t stream);
hipError_t launch_rn3_rag_maxpool(const void* x, int ldx, void* y, int ldy, int dt, const int* row0_in, const int* row0_out, const int* utt_out, int M_out,
                                  int C, int P, hipStream_t stream);
hipError_t launch_rn3_rag_afms(const void* x, int ldx, const float* alpha, const float* gate, void* y, int ldy, const void* add, int ldadd, void* sum, int ldsum,
                               int dt, const int* utt, int M, int C, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// TitaNet (titanet.hip): the depthwise 1-D convolution over frame-major (B T, C) activations, odd k in {3, 7, 11}, zero "same" padding
// at each utterance's edges, fp32 accumulation in a fixed tap order; fp32 or bf16 storage (dt), C % 8 == 0, 16-byte aligned pointers.
// w: tap-major [k][C] fp32; bias [C] fp32.
// ---------------------------------------------------------------------------------------------
// d = dwconv(x) + bias
hipError_t launch_tn_dw(const void* x, void* d, const float* w, const float* bias, int dt, int k, int B, int Tn, int C, hipStream_t stream);
// y = relu(skip + gate[b, :] * h3) (gate (B, C) fp32); with d != null also d = dwconv(y) + bias (w, bias, k: the next block's first
// depthwise layer) in the same pass, y recomputed on the halo rows
hipError_t launch_tn_mega_tail(const void* skip, const void* h3, const float* gate, void* y, const float* w, const float* bias, void* d, int dt, int k,
                               int B, int Tn, int C, hipStream_t stream);
// The same two over a ragged pack: utterance u owns the rows [row0[u], row0[u + 1]) (row0: n + 1 ints on the device), max_T >= every
// T_u, gate (n, C).  The padding sits at each utterance's own edges and no tap reads a neighbour's row; an utterance's values are bit for
// bit those of the fixed form at B = 1, Tn = T_u.  n <= 65535.
hipError_t launch_tn_dw_ragged(const void* x, void* d, const float* w, const float* bias, int dt, int k, const int* row0, int n, int max_T, int C,
                               hipStream_t stream);
hipError_t launch_tn_mega_tail_ragged(const void* skip, const void* h3, const float* gate, void* y, const float* w, const float* bias, void* d, int dt,
                                      int k, const int* row0, int n, int max_T, int C, hipStream_t stream);

// rows[b, 0:n) (row stride ld) = NaN for every utterance b whose input x[b * per_utt .. (b + 1) * per_utt) holds an inf / NaN
hipError_t launch_tn_nonfinite_rows(const float* x, int64_t per_utt, int B, float* rows, int ld, int n, hipStream_t stream);
// the same over a pack: utterance b is the (row0[b + 1] - row0[b]) * per_row values at x + off[b] (off, row0: device tables)
hipError_t launch_tn_nonfinite_rows_ragged(const float* x, const int64_t* off, const int* row0, int per_row, int B, float* rows, int ld, int n,
                                           hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Conformer (conformer.hip): d_model = 256, frame-major (B T', 256) activations, fp32 or bf16 storage (dt), 16-byte aligned pointers.
// ---------------------------------------------------------------------------------------------
// Conv2d(1, 256, 3, stride 2) + ReLU over the (T, F) image of each utterance (x: (B T, F)): y (B, T1, F1, 256), T1 = (T - 3) / 2 + 1,
// F1 = (F - 3) / 2 + 1; w tap-major [9][256] fp32 (tap = 3 dt + df), bias [256]
hipError_t launch_cf_conv1(const void* x, const float* w, const float* bias, void* y, int dt, int B, int Tn, int F, hipStream_t stream);
// ... over the utterances [u0, u0 + n) of a pack: utterance u's mel rows start at row mel0[u] of x (packed (sum T_u, F)); row0 is the
// table of the SUBSAMPLED level (T'_u = row0[u + 1] - row0[u]).  Only the 2 T'_u + 1 conv1 rows conv2 reads are written, utterance u's at
// conv1 row 2 (row0[u] - row0[u0]) + (u - u0) of y; max_T_sub >= every T'_u of the slice
hipError_t launch_cf_conv1_ragged(const void* x, const float* w, const float* bias, void* y, int dt, const int* mel0, const int* row0, int u0,
                                  int n, int max_T_sub, int F, hipStream_t stream);
// y = LayerNorm(x) (g1, b1; eps 1e-5, fp32 statistics); with y2 != null also y2 = LayerNorm(y as stored) (g2, b2)
hipError_t launch_cf_ln(const void* x, void* y, const float* g1, const float* b1, void* y2, const float* g2, const float* b2, int dt, int64_t M,
                        hipStream_t stream);
// u (B T', 512) -> y (B T', 256) = swish(dw15(u[:, :256] * sigmoid(u[:, 256:])) + bias), zero padding 7 per utterance;
// w tap-major [15][256] fp32 with the BatchNorm scale folded in, bias = the BatchNorm shift
hipError_t launch_cf_glu_dw(const void* u, const float* w, const float* bias, void* y, int dt, int B, int Tn, hipStream_t stream);
// ... over a pack (row0: n + 1 device ints, max_T_sub >= every T'_u): the zero padding sits at each utterance's own edges
hipError_t launch_cf_glu_dw_ragged(const void* u, const float* w, const float* bias, void* y, int dt, const int* row0, int n, int max_T_sub,
                                   hipStream_t stream);
// relative-position self-attention, 4 heads of 64: qkv (B T', ldq) holds q | k | v in columns [0, 768); P (T', ldp) fp32 = pe[:T'] W_pos^T;
// u_bias, v_bias [4][64] fp32; ctx (B T', ldc) = the heads' contexts concatenated (before out_proj).  Any T' >= 1.
hipError_t launch_cf_attn(const void* qkv, int ldq, const float* P, int ldp, const float* u_bias, const float* v_bias, void* ctx, int ldc, int dt,
                          int B, int Tn, hipStream_t stream);
// ... over a pack: utterance u owns the rows [row0[u], row0[u + 1]) of qkv and ctx (row0: n + 1 device ints) and is attended exactly as
// launch_cf_attn attends it alone (B = 1, Tn = T'_u), bit for bit; P holds at least max_T_sub >= every T'_u rows
hipError_t launch_cf_attn_ragged(const void* qkv, int ldq, const float* P, int ldp, const float* u_bias, const float* v_bias, void* ctx, int ldc,
                                 int dt, const int* row0, int n, int max_T_sub, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// ResNetSE (resnetse.hip): channels-last (B, P, Q, C) activations — P frames, Q mel rows — fp32 or bf16 storage (dt), 16-byte aligned.
// ---------------------------------------------------------------------------------------------
inline int rs_out_size(int n, int stride) { return (n - 1) / stride + 1; }      // Conv2d(3, stride, padding 1) and Conv2d(1, stride)
// y (B, Po, Qo, Cout) = [relu](scale[n] conv(x) + shift[n]), conv = ks x ks (3: zero padding 1; 1: none) at stride 1 / 2 over
// [relu](x) (B, P, Q, Cin); W packed [Cin / CK][ks ks taps][Cout][CK] in the compute type, CK = 32 (bf16) / 16 (fp32) channels, tap =
// 3 dp + dq.  Cin % CK == 0; Cout 32 or a multiple of 64.  part (optional): (B, ntp ntq, Cout) fp32 sums of y over each tile's positions.
// the tables of a convolution over a ragged pack (launch_rs_conv_ragged below)
struct RsRagConv {
    const int* row0_in = nullptr;
    const int* row0_out = nullptr;
    const int* tile0 = nullptr;
    const int* plan = nullptr;
    int n = 0;
    int ntiles = 0;                      // host: tile0[n]
    int halo_bytes = 0;                  // host: the largest halo of the pack, in LDS bytes
};
struct RsConvParams {
    const void* X = nullptr;
    void* Y = nullptr;
    const void* W = nullptr;
    const float* scale = nullptr;
    const float* shift = nullptr;
    float* part = nullptr;
    int B = 0, P = 0, Q = 0, Cin = 0, Cout = 0, stride = 1, ks = 3, relu_in = 0, relu_out = 0;
    int Po = 0, Qo = 0, TP = 0, TQ = 0, ntp = 0, ntq = 0;      // rs_conv_plan: output size, tile (TP x TQ <= 128 positions), tiles per utterance
    RsRagConv rag;                       // launch_rs_conv_ragged fills it; the fixed form never reads it
};
void rs_conv_plan(RsConvParams& p);
hipError_t launch_rs_conv(const RsConvParams& p, int dt, hipStream_t stream);
// The same convolution over a ragged pack: n utterances, utterance u a (P_u, Q, Cin) image at the rows [row0_in[u], row0_in[u + 1]) of x and
// a (Po_u, Qo, Cout) image at [row0_out[u], row0_out[u + 1]) of y, Po_u = rs_out_size(P_u, stride) (a row = one frame, Q C values).  Every
// utterance is tiled by rs_conv_plan of its OWN image, so its values, and its rows of `part`, are bit for bit those of launch_rs_conv on it
// alone (B = 1).  tile0 (n + 1) is the prefix of the utterances' tile counts and plan (n) their tiles, TP | TQ << 8: device tables that
// launch_rs_rag_tiles builds from row0_in on the stream (no host synchronisation).  The host counts the same tiles from its copy of the
// table (rs_rag_tiles_host: the grid, and the dynamic LDS of the pack's largest halo); one function serves both sides.
void rs_rag_tiles_host(const int* hrow0_in, int n, int Q, int stride, int ks, int* ntiles, int* halo_bytes);
hipError_t launch_rs_rag_tiles(const int* row0_in, int n, int Q, int stride, int ks, int* tile0, int* plan, hipStream_t stream);
// p: X, Y, W, scale, shift, part, Q, Cin, Cout, stride, ks, relu_* as for launch_rs_conv; B / P / Po / TP / TQ / ntp / ntq are not read.
// part (optional): (r.ntiles, Cout), the pack's tiles in utterance order, each utterance's in its own tile order
hipError_t launch_rs_conv_ragged(RsConvParams p, const RsRagConv& r, int dt, hipStream_t stream);
// stem: y (B, P, Q, 32) = scale relu(conv3x3(x) + bias) + shift on the fp32 (B, P, Q) input; w tap-major [9][32]
hipError_t launch_rs_stem(const float* x, const float* w, const float* bias, const float* scale, const float* shift, void* y, int dt, int B, int P, int Q,
                          hipStream_t stream);
// gate (B, C) = sigmoid(w2 relu(w1 mean + b1) + b2), mean = the tile sums of rs_conv added in tile order / positions; w1 [16][C], w2 [C][16]
hipError_t launch_rs_se_gate(const float* part, int ntiles, int B, int C, int positions, const float* w1, const float* b1, const float* w2, const float* b2,
                             float* gate, hipStream_t stream);
// out = relu(res' + y gate[b, :]); res' = relu(res) (identity residual) or res (downsample output)
hipError_t launch_rs_se_apply(const void* y, const void* res, const float* gate, void* out, int dt, int B, int positions, int C, bool res_relu,
                              hipStream_t stream);
// The three over a pack (row0 / utt: one frame level's tables, ragged.hip; M = row0[n] frames of Q positions): the stem pads at each
// utterance's own first and last frame; the gate of utterance u adds its own tiles part[tile0[u] .. tile0[u + 1]) in index order and divides
// by its own P_u Q positions; the tail takes the gate row of its frame's utterance.  An utterance's values are those of the fixed forms at
// B = 1, bit for bit.
hipError_t launch_rs_stem_ragged(const float* x, const float* w, const float* bias, const float* scale, const float* shift, void* y, int dt,
                                 const int* row0, const int* utt, int M, int Q, hipStream_t stream);
hipError_t launch_rs_se_gate_ragged(const float* part, const int* tile0, const int* row0, int n, int C, int Q, const float* w1, const float* b1,
                                    const float* w2, const float* b2, float* gate, hipStream_t stream);
hipError_t launch_rs_se_apply_ragged(const void* y, const void* res, const float* gate, void* out, int dt, const int* utt, int M, int Q, int C,
                                     bool res_relu, hipStream_t stream);

// synthetic waveforms from a counter-based RNG (synth.hip): out (B, L) fp32 = utterances [first_utt, first_utt + B) of the stream `seed`
hipError_t launch_synth_wave(float* out, uint64_t seed, int64_t first_utt, int B, int L, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Scoring
// ---------------------------------------------------------------------------------------------
hipError_t launch_l2norm(float* E, int64_t N, int D, hipStream_t stream);
hipError_t launch_score_pairs(const float* E, int D, const int32_t* ia, const int32_t* ib, int64_t P, float* out, hipStream_t stream);
hipError_t launch_asnorm_pairs(const float* E, int D, const float* mu, const float* sigma, const int32_t* ia,
                               const int32_t* ib, int64_t P, float* out, hipStream_t stream);
// whole-trial forms over the aligned crops of two files, F (n_files, n_crops, D): mode 0 mean |cos|, 1 mean p-2 distance (+1e-6),
// 2 minus the mean pairwise distance over the (n, D, n) broadcast (src/utils.py:163-169, src/model.py:425-431)
hipError_t launch_trial_crops(int mode, float pexp, const float* F, int n_crops, int D, const int32_t* ia, const int32_t* ib, int64_t P, float* out,
                              hipStream_t stream);
hipError_t launch_mean_crops(const float* F, int64_t n_files, int n_crops, int D, float* out, hipStream_t stream);
// S (rows x K, row stride ld) fp32 cohort scores -> mean / population std of the `top` largest per row.  Every K is served, by one of
// four forms of the same selection: the row in registers (K <= 2048 / 6144, 16-byte rows), in LDS (Kp <= 37 888, rows_per_wg rows per
// workgroup) or read from the slab itself on every pass (longer rows).  topk_stats_form is the launcher's own choice for a shape, so a
// caller can name it beforehand (rows_per_wg: the rows a workgroup of the LDS form holds, 4 for the others).
enum TopkStatsForm { TOPK_STATS_REG8 = 0, TOPK_STATS_REG24 = 1, TOPK_STATS_LDS = 2, TOPK_STATS_GLOBAL = 3 };
TopkStatsForm topk_stats_form(const float* S, int K, int ld, int* rows_per_wg = nullptr);
hipError_t launch_topk_stats(const float* S, int64_t rows, int K, int ld, int top, float* mu, float* sigma, hipStream_t stream);

// Fused AS-norm cohort statistics (asnorm_fused.hip): scores stay in the MFMA accumulators; per embedding two candidate lists of
// ASNORM_CAND_PER_LANE scores above a moment-based threshold, then the exact top-`top` statistics of the candidates.
constexpr int ASNORM_CAND_PER_LANE = 256;
struct AsnormFusedParams {
    const float* E = nullptr;       // (N, D) embeddings of this launch
    int64_t N = 0;
    const float* cohort = nullptr;  // (K, D)
    int K = 0;
    const float* MB = nullptr;      // (D + 32, D): rows of M = C^T C / K, then the cohort mean, then zeros (launch_cohort_moments)
    float z = 0.0f;                 // threshold = row mean + z * row std (asnorm_tail_z)
    const float* zrow = nullptr;    // optional (N): a z of its own per embedding — the refit passes over the embeddings whose cohort scores the
                                    // normal quantile did not fit (round 6)
    float* cand = nullptr;          // (N, 2, ASNORM_CAND_PER_LANE) candidate scores
    int32_t* cnt = nullptr;         // (N, 2) scores above the threshold seen by each of the two lanes (may exceed the list size)
    const void* planes = nullptr;   // optional: [2][D + 32 + K][D] half hi | lo parts of [MB ; cohort] (launch_asnorm_planes): the split form,
                                    // three fp16 MFMAs per product block
    int nlists = 2;                 // candidate lists per embedding: 2 (cnt (N, 2), lists of ASNORM_CAND_PER_LANE), or 4 with planes: the
                                    // 16-wide-MFMA kernel (cnt (N, 4), lists of ASNORM_CAND_PER_LANE / 2)
    float* rowscale = nullptr;      // the 16-wide half-plane kernel with pscale: (N) factor that takes a row's candidates (stored in the scaled
                                    // domain) back to scores: asnorm_cand_stats multiplies mu and sigma by it
    const uint32_t* pscale = nullptr;   // the 16-wide half-plane kernel: max-|x| word of the cohort the planes were scaled by (launch_asnorm_planes)
};
// The streamed operand of the half-plane kernels (split_planes.hip): rows [0, n0) of A, then the n1 rows of B, as two half planes
// [2][n0 + n1][D] (hi, lo).  With pscale — 257 device words — the max |x| of B goes to pscale[0] (its partials behind it) and every row is
// multiplied by the exact power of two that brings that maximum into [64, 128), the first sq_rows rows by its square ("operand scaling")
hipError_t launch_split_planes(const float* A, int n0, const float* B, int n1, int D, void* planes, uint32_t* pscale, int sq_rows,
                               hipStream_t stream);
// dense score matrix on half planes / 16x16x32 fp16 MFMAs (score_h3w.hip): out (Na, ldo) = A (Na, D) . B (Nb, D)^T, D = 192 / 256
struct ScoreH3Params {
    const float* A = nullptr;
    int64_t Na = 0;
    const void* planes = nullptr;   // [2][Nb][D] half parts of B
    int Nb = 0;
    float* out = nullptr;
    int64_t ldo = 0;
    int per = 0;                    // blocks of 32 rows of B per workgroup (column slice)
    const uint32_t* pscale = nullptr;   // max-|x| word of B: the planes hold B * 2^k (split_planes.hip, "operand scaling")
};
bool score_h3w_supported(int D, int64_t Na, int64_t Nb);
size_t score_h3w_planes_bytes(int D, int64_t Nb);
hipError_t launch_score_h3w(const float* A, int64_t Na, const float* B, int64_t Nb, int D, float* out, int64_t ldo, void* planes, int num_cu,
                            hipStream_t stream);
size_t asnorm_planes_bytes(int D, int K);
// pscale: a device word that receives the cohort's max |x|; the planes are then scaled by an exact power of two
hipError_t launch_asnorm_planes(const float* MB, const float* cohort, int K, int D, void* planes, hipStream_t stream, uint32_t* pscale = nullptr);
bool asnorm_fused_supported(int D, int K, int top);
float asnorm_tail_z(int K, int top);
// `part`: cohort_moments_scratch_bytes(D) of scratch (slice partials, summed in a fixed order)
size_t cohort_moments_scratch_bytes(int D);
hipError_t launch_cohort_moments(const float* cohort, int K, int D, float* MB, float* part, hipStream_t stream);
hipError_t launch_asnorm_fused(const AsnormFusedParams& p, int D, hipStream_t stream);
// mu / sigma [row_base + r] for r < rows; embeddings that cannot be decided from their candidates: flagged[atomicAdd(nflag, 1)] = index
// (finfo, optional, parallel to `flagged`: the candidate count of a flagged embedding, bit 30 = one of its lists overflowed)
hipError_t launch_asnorm_cand_stats(const float* cand, const int32_t* cnt, int64_t rows, int top, float* mu, float* sigma, int64_t row_base,
                                    int32_t* flagged, int32_t* nflag, hipStream_t stream, int nlists = 2, const float* rowscale = nullptr, int32_t* finfo = nullptr);
hipError_t launch_gather_rows(const float* E, const int32_t* ids, int n, int D, float* out, hipStream_t stream);
// refit state of flagged embeddings (asnorm_fused.hip): structure of arrays [id | z | zp | lcp | zlo | zhi], stride = the row count
hipError_t launch_asnorm_refit_init(const int32_t* ids, const int32_t* info, int n, float z0, float target, float* soa, hipStream_t stream);
hipError_t launch_asnorm_refit_next(const float* in, int n_in, const int32_t* pos, const int32_t* info, int left, float target, float* out, hipStream_t stream);
hipError_t launch_scatter_stats(const float* m, const float* s, const int32_t* ids, int n, float* mu, float* sigma, hipStream_t stream);

// 1:N identification (score_topk.hip): per row of Q the k best rows of G by score, ties to the lower index, NaN last — without the N x M
// matrix.  The grid is query tiles x gallery slices; every lane of the fused kernel keeps the k best of the gallery rows it saw as a list of
// (score bits, index) pairs in `lists`, score_topk_merge orders the `nlists` lists of a query.
struct ScoreTopkParams {
    const float* Q = nullptr;       // (N, D) queries of this launch
    int64_t N = 0;
    const float* G = nullptr;       // (M, D) gallery
    int64_t M = 0;
    int k = 0;
    int cap = 0;                    // slots per list (score_topk_cap)
    int per = 0;                    // blocks of 32 gallery rows per slice
    int nlists = 0;                 // lists per query: 2 per slice (8 where the waves of a workgroup walk different blocks: `few`)
    uint2* lists = nullptr;         // (N, nlists, cap)
    int32_t* cnt = nullptr;         // (N, nlists) entries each list holds (<= k when the kernel has ended)
    // the normalised form (svhip_score_topk_norm): both tables or neither.  The lists then hold t = fmaf(s, aq + ag, -(bq + bg))
    const float2* qcoef = nullptr;  // (N) pairs (a, b) of this launch's queries
    const float2* gcoef = nullptr;  // (score_topk_coef_rows(M)) pairs of the gallery, 16-byte aligned
};
constexpr int SCORE_TOPK_MAX_K = 128;
bool score_topk_fused_supported(int D);
int score_topk_cap(int k);
// few: the launch's queries fit one wave (N <= 32): the four waves of a workgroup take different gallery blocks of the slice
hipError_t launch_score_topk(const ScoreTopkParams& p, int D, bool few, int slices, hipStream_t stream);
hipError_t launch_score_topk_merge(const uint2* lists, const int32_t* cnt, int64_t rows, int nlists, int cap, int k, float* out_score,
                                   int32_t* out_index, hipStream_t stream);
// the slab route: the k best of each row of S (rows x M, row stride ld), same order
// (qcoef, gcoef: the normalised form — the pairs of the slab's rows and of the gallery; every read of a score goes through the fmaf)
hipError_t launch_score_topk_rows(const float* S, int64_t rows, int64_t M, int64_t ld, int k, float* out_score, int32_t* out_index, hipStream_t stream,
                                  const float2* qcoef = nullptr, const float2* gcoef = nullptr);
// a = 0.5f / sigma, b = mu * a per query and per gallery row, interleaved; the gallery's table has score_topk_coef_rows(M) entries
// (whole blocks of 32 rows, the last row repeated)
int64_t score_topk_coef_rows(int64_t M);
hipError_t launch_score_topk_coef(const float* q_mu, const float* q_sigma, int64_t N, const float* g_mu, const float* g_sigma, int64_t M,
                                  float2* qcoef, float2* gcoef, hipStream_t stream);

// Threshold search (score_above.hip): every (query, gallery row) pair whose score v reaches `thr` (v = s, or t with the coefficient tables
// of score_topk_coef), as CSR rows in ascending gallery index — without the N x M matrix.  The fused kernel is score_topk_kernel's MFMA loop
// with another epilogue; the grid is query tiles x gallery slices as there.  A query's lists are CONTIGUOUS runs of gallery blocks in
// ascending order: one per slice (`few`: four, each wave of the workgroup walks a quarter of the slice).  The count form adds up the hits
// of a list, launch_score_above_scan sums the lists of a row (and places them inside the row's CSR segment), the fill form writes.
struct ScoreAboveParams {
    const float* Q = nullptr;       // (N, D) queries of this launch
    int64_t N = 0;
    const float* G = nullptr;       // (M, D) gallery
    int64_t M = 0;
    float thr = 0.0f;               // a hit: v >= thr (never NaN)
    int upper = 0;                  // SVHIP_ABOVE_UPPER: only the pairs with m > row_base + n
    int64_t row_base = 0;           // q_base + the place of this launch's first query in the call
    int per = 0;                    // blocks of 32 gallery rows per slice
    int nl = 0;                     // lists per query: slices (few: 4 slices)
    int32_t* lcnt = nullptr;        // (N, nl) hits per list: written by the count form, the fill form's write bound
    const int64_t* loff = nullptr;  // fill: (N, nl) where each list starts in out_index / out_score
    int32_t* out_index = nullptr;   // fill
    float* out_score = nullptr;     // fill
    const float2* qcoef = nullptr;  // the normalised form: both tables or neither (ScoreTopkParams)
    const float2* gcoef = nullptr;
};
hipError_t launch_score_above(const ScoreAboveParams& p, int D, bool few, int slices, bool fill, hipStream_t stream);
// per row of a launch the sum of its nl list counts.  out_count (count): out_count[row] = the sum.  row_ptr (fill; both offset to the
// launch's first row, row0 = that row's place in the call): loff[row, l] = row_ptr[row] + the hits of the lists before l, and a row whose
// sum is not row_ptr[row + 1] - row_ptr[row] (or row 0 of the call with row_ptr[0] != 0) lowers *bad to its place in the call
hipError_t launch_score_above_scan(const int32_t* lcnt, int64_t rows, int nl, int64_t* out_count, const int64_t* row_ptr, int64_t row0,
                                   int64_t* loff, unsigned long long* bad, hipStream_t stream);
// the slab route: one workgroup per row of S (rows x M, row stride ld % 4 == 0, 16-byte aligned).  Exactly one of: out_count (count),
// bad (compare the count with row_ptr, as the scan does), out_index + out_score (write the row's hits at row_ptr[row], ascending)
hipError_t launch_score_above_rows(const float* S, int64_t rows, int64_t M, int64_t ld, float thr, int upper, int64_t row_base, const float2* qcoef,
                                   const float2* gcoef, int64_t* out_count, const int64_t* row_ptr, int64_t row0, unsigned long long* bad,
                                   int32_t* out_index, float* out_score, hipStream_t stream);

// Speaker clustering (score_cluster.hip): the connected components of "rows i < j of ONE set are linked iff v(i, j) >= thr" (v as threshold
// search computes it in UPPER mode), without an edge list.  `parent` (M int32, the call's out_root) holds a lock-free disjoint-set forest
// with parent[x] <= x: launch_cluster_init, then one launch_cluster_link per part of the fused plan (or one launch_cluster_link_rows per
// slab), then launch_cluster_flatten: parent[i] = the smallest row of i's component.
struct ClusterLinkParams {
    const float* Q = nullptr;       // (N, D) the rows row_base .. row_base + N - 1 of G: the queries of this launch
    int64_t N = 0;
    const float* G = nullptr;       // (M, D) the whole set
    int64_t M = 0;
    float thr = 0.0f;               // a link: v >= thr (never NaN)
    int64_t row_base = 0;           // the place of this launch's first query in the set
    int per = 0;                    // blocks of 32 gallery rows per slice
    int32_t* parent = nullptr;      // (M) the forest
    const float2* qcoef = nullptr;  // the normalised form: both tables or neither (ScoreTopkParams)
    const float2* gcoef = nullptr;
};
hipError_t launch_cluster_init(int32_t* parent, int64_t N, hipStream_t stream);
hipError_t launch_cluster_link(const ClusterLinkParams& p, int D, bool few, int slices, hipStream_t stream);
// the slab route: one workgroup per row of S (rows x M, row stride ld % 4 == 0, 16-byte aligned), row r being row row_base + r of the set
hipError_t launch_cluster_link_rows(const float* S, int64_t rows, int64_t M, int64_t ld, float thr, int64_t row_base, const float2* qcoef,
                                    const float2* gcoef, int32_t* parent, hipStream_t stream);
hipError_t launch_cluster_flatten(int32_t* root, int64_t N, hipStream_t stream);
// Two-set clustering (svhip_cluster_join): A's rows are 0 .. NA - 1 of the joint forest, B's NA .. NA + NB - 1.
// The clamp of a seed entry, written once for the seed kernel and for the host check of host seeds: row i of a side may point at any row
// of [0, i] of that side; every other value is read as i, so the row starts alone.  The forest's climbs end only because parent[x] <= x
// holds everywhere (score_cluster.hip): whatever a seed array holds, what this returns keeps that.
__host__ __device__ inline int32_t cluster_seed_parent(int32_t seed, int64_t i) { return seed >= 0 && (int64_t)seed <= i ? seed : (int32_t)i; }
// parent[i] = root_a[i] clamped (NULL: i); parent[NA + j] = NA + root_b[j] clamped (NULL: NA + j)
hipError_t launch_cluster_seed(const int32_t* root_a, int64_t NA, const int32_t* root_b, int64_t NB, int32_t* parent, hipStream_t stream);
// The link launches with an index offset on either side: a link is (q_off + row_base + the query's place in the launch, g_off + the
// gallery row), and every such index must lie below `forest`, the size of `parent`.
//   CLUSTER_LINK_SET    cluster_above's own launch (launch_cluster_link / _rows: no offsets)
//   CLUSTER_LINK_SIDE   the self-join of one side: the masks of CLUSTER_LINK_SET, q_off == g_off == the side's first joint row
//   CLUSTER_LINK_CROSS  the rectangle: every (query, gallery row) pair, no mask
enum { CLUSTER_LINK_SET = 0, CLUSTER_LINK_SIDE = 1, CLUSTER_LINK_CROSS = 2 };
hipError_t launch_cluster_join_link(const ClusterLinkParams& p, int D, bool few, int slices, int form, int64_t q_off, int64_t g_off, int64_t forest,
                                    hipStream_t stream);
hipError_t launch_cluster_join_rows(const float* S, int64_t rows, int64_t M, int64_t ld, float thr, int64_t row_base, const float2* qcoef,
                                    const float2* gcoef, int32_t* parent, int form, int64_t q_off, int64_t g_off, int64_t forest, hipStream_t stream);
// dense ids from flattened roots: *out_n = the number of roots; cluster (optional) [i] = the roots below root[i].  bcnt: cluster_id_blocks(N)
// int32 of scratch (per-block root counts, scanned in place by one workgroup)
int64_t cluster_id_blocks(int64_t N);
hipError_t launch_cluster_ids(const int32_t* root, int64_t N, int32_t* bcnt, int32_t* cluster, int64_t* out_n, hipStream_t stream);

// Average / complete linkage inside the components (score_linkage.hip; svhip.h, cluster_linkage).  The component table, all int32 and all
// on the device (no size ever reaches the host): per dense component id c its rows cnt[c], the start off[c] of its member list, the
// list itself (filled through cursor[c], sorted by the workgroup that owns the component), and three work lists of component ids by size:
//   0: 2 .. min(64, lds_rows) rows   1: .. lds_rows rows (both: the matrix in LDS)   2: .. LINKAGE_MAX_ROWS rows (the matrix in scratch)
// The matrices of work list 2 live in a POOL of scratch, at most LINKAGE_POOL_FLOATS (64 MiB: sixteen matrices of LINKAGE_MAX_ROWS rows):
// one thread packs the list into rounds that fit the pool (round[w], place[w]), and the host enqueues one launch per round it cannot rule
// out - a launch whose round is empty returns at once.
constexpr int LINKAGE_MAX_ROWS = SVHIP_LINKAGE_MAX_ROWS, LINKAGE_LDS_ROWS = SVHIP_LINKAGE_LDS_ROWS, LINKAGE_SMALL_ROWS = 64;
constexpr int64_t LINKAGE_POOL_FLOATS = (int64_t)16 << 20;
struct LinkageTable {
    int32_t* cnt = nullptr;         // [N], zero behind the last component
    int32_t* off = nullptr;         // [N]
    int32_t* cursor = nullptr;      // [N]
    int32_t* members = nullptr;     // [N]
    int32_t* bsum = nullptr;        // [cluster_id_blocks(N)]
    int32_t* work = nullptr;        // [3][work_stride]
    int32_t* n_work = nullptr;      // [4]: the lengths of the three lists, the rounds of list 2
    int32_t* round = nullptr;       // [work_stride] per entry of list 2: its round ...
    int32_t* place = nullptr;       // [work_stride] ... and where its matrix starts in the pool
    int64_t work_stride = 0;        // N / 2 + 1: the components of at least two rows
};
inline size_t linkage_table_ints(int64_t N) { return (size_t)4 * N + (size_t)cluster_id_blocks(N) + 5 * (size_t)(N / 2 + 1) + 4; }
// The pool of a call over N rows, and the rounds it may take.  The matrices of list 2 hold at most T = N min(N, LINKAGE_MAX_ROWS) floats in
// all (sum m <= N, m <= min(N, LINKAGE_MAX_ROWS)).  pool == T: everything fits in round 0.  Otherwise a round is closed only when the next
// matrix does not fit, so a closed round and the first matrix of the round behind it hold more than the pool together: every PAIR of
// consecutive rounds holds more than the pool, there are at most floor(T / pool) disjoint such pairs, hence at most 2 floor(T / pool) + 1 rounds.
inline int64_t linkage_pool_floats(int64_t N) { return std::min<int64_t>(LINKAGE_POOL_FLOATS, N * std::min<int64_t>(N, LINKAGE_MAX_ROWS)); }
inline int64_t linkage_max_rounds(int64_t N) { return 2 * (N * std::min<int64_t>(N, LINKAGE_MAX_ROWS) / linkage_pool_floats(N)) + 1; }
// comp: the dense component id of every row (cluster_ids' output); *n_unrefined <- the components of more than LINKAGE_MAX_ROWS rows
hipError_t launch_linkage_table(const int32_t* comp, int64_t N, int lds_rows, const LinkageTable& t, unsigned long long* n_unrefined,
                                hipStream_t stream);
struct LinkageParams {
    const float* E = nullptr;       // (N, D)
    int64_t N = 0;
    int D = 0;
    float thr = 0.0f;
    int linkage = 0;                // SVHIP_LINKAGE_AVERAGE / _COMPLETE
    const float2* coef = nullptr;   // the normalised form: (a, b) per row (cluster_above's query table), or NULL
    LinkageTable t;
    int32_t* root = nullptr;        // [N]: holds the component roots, receives the refined ones
    float* pool = nullptr;          // linkage_pool_floats(N) floats: the matrices of work list 2, round by round
    int fill_only = 0;              // option linkage_fill_only: the matrices are built and no merge is made (a measurement's switch)
};
// the launches of linkage_agglo_kernel: one per LDS work list (pool = false), or one per round of list 2 that N cannot rule out (pool = true)
hipError_t launch_linkage_agglo(const LinkageParams& p, int lds_rows, bool pool, int num_cu, hipStream_t stream);

// Dataset audit (group_audit.hip): files sorted by group; s(i, j) = mean_c | cos(F[i, c], F[j, c]) | (launch_trial_crops mode 0's
// statement) for the files of one group, a mismatch iff s <= cut; miss[i] counts the files j != i of i's group that i mismatches.
// Per-file tables (launch_group_audit_tables, from the device copy of group_ptr): gs / ge = where the file's group starts / ends,
// sbase = where its group's n_g x n_g score block starts (sq[g] = the sum of n_h^2 over the groups before g; only with scores).
// Both routes compute the pairs j >= i once and count / write them for both files; `miss` must be zero before the first launch.
struct GroupAuditParams {
    const float* F = nullptr;       // (n_files, n_crops, D), 16-byte aligned
    int64_t n_files = 0;
    int n_crops = 0, D = 0;
    const int32_t* gs = nullptr;
    const int32_t* ge = nullptr;
    const int64_t* sbase = nullptr; // with score
    float cut = 0.0f;
    int32_t* miss = nullptr;
    float* score = nullptr;         // optional: the dense per-group blocks, back to back
};
bool group_audit_mfma_supported(int D);      // D % 32 == 0, D <= 1024 (and a 16-byte aligned F: the caller's check)
hipError_t launch_group_audit_tables(const int64_t* gp, int64_t n_groups, const int64_t* sq, int64_t n_files, int32_t* gs, int32_t* ge, int64_t* sbase,
                                     hipStream_t stream);
// the MFMA route: 64 x 64 tiles on the file axis; max_cols = the most column tiles any row tile meets (a bound is enough: a workgroup
// whose column tile starts past its row tile's last group exits at once)
hipError_t launch_group_audit(const GroupAuditParams& p, int64_t max_cols, hipStream_t stream);
// the plain route: pairs [p0, p0 + P) of the call's list of within-group pairs j >= i (pp[g] = the pairs before group g, n_groups + 1
// entries) -> ia / ib; then launch_trial_crops(mode 0); then the comparison, the counts and the scatter of the scores
hipError_t launch_group_audit_pairs(const int64_t* gp, const int64_t* pp, int64_t n_groups, int64_t p0, int64_t P, int32_t* ia, int32_t* ib,
                                    hipStream_t stream);
hipError_t launch_group_audit_count(const float* sc, const int32_t* ia, const int32_t* ib, int64_t P, float cut, const int32_t* gs, const int32_t* ge,
                                    const int64_t* sbase, int32_t* miss, float* score, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Verification metrics (metrics.hip): one workspace of metrics_workspace_bytes(P) holds the sorted trial list
// ---------------------------------------------------------------------------------------------
size_t metrics_workspace_bytes(int64_t P);
hipError_t metrics_sort_scan(const float* scores, const int32_t* labels, int64_t P, bool nan_to_num, void* ws, size_t ws_bytes, hipStream_t st);
hipError_t metrics_roc_points(int64_t P, void* ws, size_t ws_bytes, float* thr, int64_t* fps, int64_t* tps, int32_t** n_runs_dev, hipStream_t st);
hipError_t metrics_error_rates(int64_t P, void* ws, size_t ws_bytes, double* fnrs, double* fprs, float* thresholds, hipStream_t st);
hipError_t metrics_min_dcf(int64_t P, void* ws, size_t ws_bytes, double p_target, double c_miss, double c_fa, double* dcf_dev, float* thr_dev,
                           hipStream_t st);

}  // namespace svhip
