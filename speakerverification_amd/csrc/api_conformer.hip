// api_conformer.hip — the Conformer in libsvhip (reference models/Conformer.py:100-154, models/conformer/conformer/*.py): its create
// rules, weight names and packing, workspace, forward and stages.
//
// From the mel power (B, n_mels, T):
//   front-end   log(x + 1e-6) - mean_t (log_input), InstanceNorm1d(n_mels, affine) -> X_in (B T, n_mels)        prologue
//   subsample   per slice of cf_chunk utterances (the conv1 output is the largest tensor of the net):
//               conv1 + ReLU -> (n, T1, F1, 256)                                                               cf_conv1
//               conv2 + ReLU as a GEMM whose operand rows are gathered as three 768-element runs -> (n T' F2, 256)   generic GEMM, SEG form
//               input_projection: the (n T', F2 256) view of that output, its columns permuted at finalize -> cf_in
//   6 blocks    x += 0.5 FF(x); x += MHSA(x); x += Conv(x); x += 0.5 FF'(x); x = LN(x)                          see below
//   pooling     w = softmax_T(attention.3(BN(relu(attention.0 x)))); [mu | sqrt(clamp(var, 1e-4, 1e4))]; attention_norm; fc
// Every Linear / pointwise conv goes through conv_plan / conv_gemm.  The half-step residuals are the GEMM epilogue's scale (0.5) and
// residual R; the residual stream stays in the handle's storage type.
//
// A ragged pack (conformer_embed_ragged): n utterances of T_u mel frames, packed back to back at the mel level and, T'_u rows each, at
// the subsampled level (row0 / utt tables, as ECAPA's and RawNet3's packs).  The same layers over the packed rows, enqueued by the same
// walk (conformer_walk): every GEMM through launch_gemm_ragged, LayerNorm unchanged (row-wise), and the five steps that know where an
// utterance begins and ends in their segment-table forms — the input normalisation (launch_rag_prologue), the subsampling (conv1
// keeps only the 2 T'_u + 1 rows conv2 reads, utterance u's at conv1 row 2 row0[u] + u; conv2's operand gather adds that
// per-utterance offset), the attention, the GLU + depthwise conv and the pooling.  P = pe W_pos^T is kept for rows 0 .. the longest
// T'_u seen (row c depends on c only).
#include <algorithm>
#include <cstring>
#include <thread>

#include "handle.h"

namespace svhip {

namespace {

int cf_sub(int n) { return (n - 3) / 2 + 1; }                         // one Conv2d(3, stride 2) of Conformer's subsampling (n >= 3)
constexpr int CF_D = 256, CF_LAYERS = 6, CF_MAX_T = 10000;           // d_model, blocks, the length of the pe buffer

struct CfBlock {
    float *ff_g[2] = {}, *ff_b[2] = {};   // the two feed-forward modules' LayerNorms (FF, FF')
    ConvLayer ff1[2], ff2[2];             // Linear(256, 1024) (Swish in the epilogue), Linear(1024, 256)
    float *att_g = nullptr, *att_b = nullptr;
    ConvLayer qkv, out;                   // query | key | value projections as one 256 -> 768 layer; out_proj
    float* P = nullptr;                   // (T', 256) fp32: pe[:T'] pos_proj^T (the same for every utterance: formed at finalize)
    float *u = nullptr, *v = nullptr;     // u_bias, v_bias [4][64]
    float *cv_g = nullptr, *cv_b = nullptr;
    ConvLayer pw1, pw2;                   // pointwise 256 -> 512 (GLU follows), 256 -> 256
    float *dw_w = nullptr, *dw_b = nullptr;   // depthwise k = 15, tap-major [15][256], with BatchNorm(256) folded in
    float *fin_g = nullptr, *fin_b = nullptr; // the block's final LayerNorm
};

// Conformer layers (SVHIP_MODEL_CONFORMER: models/Conformer.py, models/conformer/conformer/*).  d_model 256, 4 heads of 64, six blocks.
// The InstanceNorm affine of the front-end is the handle's in_w / in_b
struct ConformerState : ModelState {
    std::vector<CfBlock> blocks;
    int T1 = 0, F1 = 0, Tp = 0, F2 = 0;   // conv1 / conv2 output sizes: T1 x F1, T' x F2
    int chunk = 0;                        // utterances per subsampling slice (bounds the conv1 output buffer)
    float *c1_w = nullptr, *c1_b = nullptr;   // conv_subsample.sequential.0: tap-major [9][256], bias
    ConvLayer c2;                         // conv_subsample.sequential.2 as a GEMM, k = dt * 768 + df * 256 + c (the segmented gather)
    int* seg_off = nullptr;               // (T' F2) row offsets of that gather within an utterance's conv1 output
    ConvLayer proj;                       // input_projection, columns permuted from c * F2 + f to f * 256 + c
    ConvLayer att0, att3;                 // attention.0 (+ ReLU, attention.2 as the epilogue affine), attention.3 (fp32 logits)
    float *pbn_scale = nullptr, *pbn_shift = nullptr;   // attention_norm (BatchNorm1d(512))
    LinearLayer fc;                       // fc (Conv1d(512, nOut, 1))
    float* half = nullptr;                // 256 x 0.5: the half-step residual as the epilogue scale
    void *c1 = nullptr, *s2 = nullptr;    // per slice: conv1 output (chunk, T1, F1, 256); conv2 output (chunk T' F2, 256)
    void *in = nullptr, *b0 = nullptr, *x[2] = {}, *r = nullptr;   // (Bmax T', 256): input projection, block 0's output,
                                          // later blocks' outputs (ping-pong), the residual stream inside a block
    void *ln = nullptr, *ln2 = nullptr;   // (Bmax T', 256) LayerNorm outputs
    void* hid = nullptr;                  // (Bmax T', 1024): FF hidden / q | k | v / pointwise-conv output
    void *ctx = nullptr, *attn0 = nullptr;   // (Bmax T', 256): attention context (block 0's is kept: stage cf_attn0); GLU-dw output
    void* last = nullptr;                 // the last block's output
    float* logits = nullptr;              // (Bmax T', 256) fp32 attention logits of the pooling
    float *pool_raw = nullptr, *pool = nullptr;         // (Bmax, 512) [mean | std], after attention_norm
    KeptStages keep;                      // option cf_keep: copies of what the walk stored, by stage name (keep_stage fills them)
    // ragged packs (allocated by the first ragged call; the row buffers above hold rows_cap >= floor((Bmax T - 3) / 4) rows for them)
    size_t rows_cap = 0;
    std::vector<std::vector<float>> pe_host, wpos_host;   // kept from finalize: each layer's pos_proj weight; pe_host[pe_of[i]] is layer
    std::vector<int> pe_of;                               // i's positional encoding (layers whose buffers are equal share one copy)
    float* rag_P = nullptr;               // (layers, rag_P_rows, 256): P for rows 0 .. rag_P_rows - 1, grown to the longest T'_u seen
    int rag_P_rows = 0;
    RagTables rag;                        // the tables of a call (two levels: mel frames, subsampled frames) and the waveform staging buffer
    float* rag_stats = nullptr;           // (Bmax n_mels 2) shift / scale of the front-end

    ~ConformerState() override { if (rag_P) (void)hipFree(rag_P); }
};

ConformerState& S(svhip_handle* h) { return static_cast<ConformerState&>(*h->model); }

// utterances per subsampling slice: what keeps the conv1 output of a slice within 256 MiB
int cf_chunk(const svhip_config& c, int T) {
    const size_t e = c.compute == SVHIP_BF16 ? 2 : 4;
    const size_t per_utt = (size_t)cf_sub(T) * cf_sub(c.n_mels) * CF_D * e;          // conv1 output bytes of one utterance
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)c.max_batch, ((size_t)256 << 20) / per_utt));
}

// rows [0, rows) of P = pe W_pos^T, every element a double-precision sum over k in order: a row depends on its index only
// (rows split over up to 16 host threads: 6 x 655 M multiply-adds at T' = 10^4; every row is the same sum whatever the split)
void cf_pos_rows(const float* pe, const float* wp, int rows, float* P) {
    const int D = CF_D;
    auto part = [&](int t0, int t1) {
        for (int t = t0; t < t1; ++t) {
            const float* pr = pe + (size_t)t * D;
            for (int n = 0; n < D; ++n) {
                const float* wr = wp + (size_t)n * D;
                double acc = 0.0;
                for (int k = 0; k < D; ++k) acc += (double)pr[k] * (double)wr[k];
                P[(size_t)t * D + n] = (float)acc;
            }
        }
    };
    const int nt = std::max(1, std::min({16, (int)std::thread::hardware_concurrency(), (rows + 63) / 64}));
    std::vector<std::thread> pool;
    for (int q = 1; q < nt; ++q) pool.emplace_back(part, (int)((int64_t)rows * q / nt), (int)((int64_t)rows * (q + 1) / nt));
    part(0, rows / nt);
    for (auto& th : pool) th.join();
}

}  // namespace

int conformer_check(const svhip_config& c, const char*& err) {
    if (c.compute != SVHIP_F32 && c.compute != SVHIP_BF16) { err = "Conformer runs on SVHIP_F32 and SVHIP_BF16 handles only"; return SVHIP_ERR_UNSUPPORTED; }
    if (c.channels != 0 && c.channels != CF_D) { err = "Conformer is built for d_model = 256 (channels 0 or 256)"; return SVHIP_ERR_INVALID; }
    if (!c.input_norm) { err = "Conformer always applies its InstanceNorm1d: input_norm must be 1"; return SVHIP_ERR_INVALID; }
    if (c.embed_dim <= 0) { err = "Conformer needs embed_dim > 0"; return SVHIP_ERR_INVALID; }
    if (c.n_mels < 7) { err = "Conformer needs n_mels >= 7 (two 3 x 3 stride-2 convolutions)"; return SVHIP_ERR_INVALID; }
    if (c.hop_length > 0) {
        const int T = c.samples / c.hop_length + 1;
        if (T < 7) { err = "Conformer needs at least 7 frames (T' = ((T - 3) / 2 + 1 - 3) / 2 + 1 >= 1)"; return SVHIP_ERR_INVALID; }
        if (cf_sub(cf_sub(T)) > CF_MAX_T) {
            err = "Conformer's positional encoding holds 10000 positions: T' = ((T - 3) / 2 + 1 - 3) / 2 + 1 must be <= 10000";
            return SVHIP_ERR_INVALID;
        }
    }
    return SVHIP_OK;
}

// Conformer.MainModel (models/Conformer.py:13-97 with models/conformer/conformer/encoder.py's ConformerEncoder(n_mels, 256, 6 layers,
// 4 heads, FF x 4, conv kernel 15)): the 278 names of its state dict.  asp.* / asp_bn.* are in it but never called (Conformer.py:144-148)
static void cf_block_spec(const std::string& p, WeightSpec& spec) {
    const int64_t D = CF_D;
    auto ln = [&](const std::string& q) { spec[q + ".weight"] = {D}; spec[q + ".bias"] = {D}; };
    auto ff = [&](const std::string& q) {
        ln(q + "module.sequential.0");
        spec[q + "module.sequential.1.linear.weight"] = {4 * D, D}; spec[q + "module.sequential.1.linear.bias"] = {4 * D};
        spec[q + "module.sequential.4.linear.weight"] = {D, 4 * D}; spec[q + "module.sequential.4.linear.bias"] = {D};
    };
    ff(p + "sequential.0.");
    const std::string a = p + "sequential.1.module.";
    spec[a + "positional_encoding.pe"] = {1, CF_MAX_T, D};
    ln(a + "layer_norm");
    spec[a + "attention.u_bias"] = {4, 64}; spec[a + "attention.v_bias"] = {4, 64};
    for (const char* q : {"query_proj", "key_proj", "value_proj", "out_proj"}) {
        spec[a + "attention." + q + ".linear.weight"] = {D, D}; spec[a + "attention." + q + ".linear.bias"] = {D};
    }
    spec[a + "attention.pos_proj.linear.weight"] = {D, D};
    const std::string cv = p + "sequential.2.module.sequential.";
    ln(cv + "0");
    spec[cv + "2.conv.weight"] = {2 * D, D, 1}; spec[cv + "2.conv.bias"] = {2 * D};
    spec[cv + "4.conv.weight"] = {D, 1, 15};
    spec_bn(spec, cv + "5", D);
    spec[cv + "7.conv.weight"] = {D, D, 1}; spec[cv + "7.conv.bias"] = {D};
    ff(p + "sequential.3.");
    ln(p + "sequential.4");
}
void conformer_spec(const svhip_config& c, WeightSpec& spec) {
    const int64_t D = CF_D, nm = c.n_mels, F2 = cf_sub(cf_sub((int)nm)), nOut = c.embed_dim;
    spec["instance_norm.weight"] = {nm}; spec["instance_norm.bias"] = {nm};
    const std::string s = "conformer_block.conv_subsample.sequential.";
    spec[s + "0.weight"] = {D, 1, 3, 3}; spec[s + "0.bias"] = {D};
    spec[s + "2.weight"] = {D, D, 3, 3}; spec[s + "2.bias"] = {D};
    spec["conformer_block.input_projection.0.linear.weight"] = {D, D * F2}; spec["conformer_block.input_projection.0.linear.bias"] = {D};
    for (int i = 0; i < CF_LAYERS; ++i) cf_block_spec("conformer_block.layers." + std::to_string(i) + ".", spec);
    spec["asp.tdnn.conv.conv.weight"] = {128, 3 * D, 1}; spec["asp.tdnn.conv.conv.bias"] = {128};
    spec_bn(spec, "asp.tdnn.norm.norm", 128);
    spec["asp.conv.weight"] = {D, 128, 1}; spec["asp.conv.bias"] = {D};
    spec_bn(spec, "asp_bn.norm", 2 * D);
    spec["attention.0.weight"] = {128, D, 1}; spec["attention.0.bias"] = {128};
    spec_bn(spec, "attention.2", 128);
    spec["attention.3.weight"] = {D, 128, 1}; spec["attention.3.bias"] = {D};
    spec_bn(spec, "attention_norm", 2 * D);
    spec["fc.conv.weight"] = {nOut, 2 * D, 1}; spec["fc.conv.bias"] = {nOut};
}

int conformer_finalize(svhip_handle* h) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const int D = CF_D, Tp = s.Tp, F2 = s.F2, nOut = c.embed_dim;
    int rc;
    if ((rc = upload_f32(h, "instance_norm.weight", &h->in_w))) return rc;
    if ((rc = upload_f32(h, "instance_norm.bias", &h->in_b))) return rc;
    const std::string sub = "conformer_block.conv_subsample.sequential.";
    {
        const HostTensor* w;                                   // (256, 1, 3, 3) -> tap-major [9][256]
        if ((rc = needw(h, sub + "0.weight", w))) return rc;
        std::vector<float> tw(9 * D);
        for (int ch = 0; ch < D; ++ch)
            for (int t = 0; t < 9; ++t) tw[(size_t)t * D + ch] = w->data[(size_t)ch * 9 + t];
        if ((rc = dev_upload(h, &s.c1_w, tw))) return rc;
        if ((rc = upload_f32(h, sub + "0.bias", &s.c1_b))) return rc;
    }
    {
        const HostTensor *w, *b;                               // (256, 256, 3, 3) [n][c][dt][df] -> [n][dt * 768 + df * 256 + c]
        if ((rc = needw(h, sub + "2.weight", w))) return rc;
        std::vector<float> pw((size_t)D * 9 * D);
        for (int n = 0; n < D; ++n)
            for (int ch = 0; ch < D; ++ch)
                for (int t = 0; t < 9; ++t) pw[(size_t)n * 9 * D + (size_t)(t / 3) * 3 * D + (t % 3) * D + ch] = w->data[((size_t)n * D + ch) * 9 + t];
        if ((rc = needw(h, sub + "2.bias", b)) || (rc = make_conv(h, s.c2, HostTensor{std::move(pw), {D, 9 * D, 1}}, &b->data, 1))) return rc;
        std::vector<int> so((size_t)Tp * F2);
        for (int t = 0; t < Tp; ++t)
            for (int f = 0; f < F2; ++f) so[(size_t)t * F2 + f] = ((2 * t) * s.F1 + 2 * f) * D;
        if ((rc = dev_upload(h, &s.seg_off, so))) return rc;
    }
    {
        const std::string p = "conformer_block.input_projection.0.linear.";
        const HostTensor *w, *b;                               // (256, 256 F2), column c F2 + f -> f 256 + c (the GEMM writes (b, t, f) rows)
        if ((rc = needw(h, p + "weight", w))) return rc;
        std::vector<float> pw((size_t)D * D * F2);
        for (int n = 0; n < D; ++n)
            for (int ch = 0; ch < D; ++ch)
                for (int f = 0; f < F2; ++f) pw[(size_t)n * D * F2 + (size_t)f * D + ch] = w->data[(size_t)n * D * F2 + (size_t)ch * F2 + f];
        if ((rc = needw(h, p + "bias", b)) || (rc = make_conv(h, s.proj, HostTensor{std::move(pw), {D, D * F2}}, &b->data, 1))) return rc;
    }
    double fl = 2.0 * 9 * D * s.T1 * s.F1 + (double)Tp * F2 * s.c2.flops_per_row + (double)Tp * s.proj.flops_per_row;
    s.blocks.assign(CF_LAYERS, CfBlock{});
    s.pe_host.assign(CF_LAYERS, {}); s.wpos_host.assign(CF_LAYERS, {}); s.pe_of.assign(CF_LAYERS, 0);
    for (int i = 0; i < CF_LAYERS; ++i) {
        CfBlock& K = s.blocks[i];
        const std::string p = "conformer_block.layers." + std::to_string(i) + ".";
        for (int j = 0; j < 2; ++j) {
            const std::string q = p + (j == 0 ? "sequential.0." : "sequential.3.") + "module.sequential.";
            if ((rc = upload_f32(h, q + "0.weight", &K.ff_g[j]))) return rc;
            if ((rc = upload_f32(h, q + "0.bias", &K.ff_b[j]))) return rc;
            if ((rc = make_conv(h, K.ff1[j], q + "1.linear.weight", q + "1.linear.bias", "", 1))) return rc;
            if ((rc = make_conv(h, K.ff2[j], q + "4.linear.weight", q + "4.linear.bias", "", 1))) return rc;
            fl += (double)Tp * (K.ff1[j].flops_per_row + K.ff2[j].flops_per_row);
        }
        const std::string a = p + "sequential.1.module.";
        if ((rc = upload_f32(h, a + "layer_norm.weight", &K.att_g))) return rc;
        if ((rc = upload_f32(h, a + "layer_norm.bias", &K.att_b))) return rc;
        {
            std::vector<float> w, b;
            for (const char* q : {"query_proj", "key_proj", "value_proj"}) {
                const HostTensor *wq = getw(h, a + "attention." + q + ".linear.weight"), *bq = getw(h, a + "attention." + q + ".linear.bias");
                if (!wq || !bq) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %sattention.%s.linear.*", a.c_str(), q);
                w.insert(w.end(), wq->data.begin(), wq->data.end());
                b.insert(b.end(), bq->data.begin(), bq->data.end());
            }
            if ((rc = make_conv(h, K.qkv, HostTensor{std::move(w), {3 * D, D}}, &b, 1))) return rc;
        }
        if ((rc = make_conv(h, K.out, a + "attention.out_proj.linear.weight", a + "attention.out_proj.linear.bias", "", 1))) return rc;
        if ((rc = upload_f32(h, a + "attention.u_bias", &K.u))) return rc;
        if ((rc = upload_f32(h, a + "attention.v_bias", &K.v))) return rc;
        {
            // P = pe[:T'] pos_proj^T in double: the positional term depends on T' only
            const HostTensor *pe = getw(h, a + "positional_encoding.pe"), *wp = getw(h, a + "attention.pos_proj.linear.weight");
            if (!pe || !wp) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s%s", a.c_str(), !pe ? "positional_encoding.pe" : "attention.pos_proj.linear.weight");
            if (pe->numel() < (int64_t)CF_MAX_T * D || wp->numel() != (int64_t)D * D)
                SV_FAIL(h, SVHIP_ERR_INVALID, "%spositional_encoding.pe must be (1, %d, %d) and pos_proj (%d, %d)", a.c_str(), CF_MAX_T, D, D, D);
            std::vector<float> P((size_t)Tp * D);
            cf_pos_rows(pe->data.data(), wp->data.data(), Tp, P.data());
            if ((rc = dev_upload(h, &K.P, P))) return rc;
            // a ragged call forms P for its own lengths: the two host tensors outlive finalize (the loaded weights are dropped after it)
            s.wpos_host[i] = wp->data;
            int same = -1;
            for (int j = 0; j < i && same < 0; ++j)
                if (s.pe_of[j] == j && !memcmp(s.pe_host[j].data(), pe->data.data(), (size_t)CF_MAX_T * D * 4)) same = j;
            s.pe_of[i] = same < 0 ? i : same;
            if (same < 0) s.pe_host[i] = std::move(const_cast<HostTensor*>(pe)->data);
        }
        fl += (double)Tp * (K.qkv.flops_per_row + K.out.flops_per_row) + 4.0 * Tp * (double)Tp * 3 * 2 * 64;
        const std::string cv = p + "sequential.2.module.sequential.";
        if ((rc = upload_f32(h, cv + "0.weight", &K.cv_g))) return rc;
        if ((rc = upload_f32(h, cv + "0.bias", &K.cv_b))) return rc;
        if ((rc = make_conv(h, K.pw1, cv + "2.conv.weight", cv + "2.conv.bias", "", 1))) return rc;
        if ((rc = make_conv(h, K.pw2, cv + "7.conv.weight", cv + "7.conv.bias", "", 1))) return rc;
        {
            // depthwise (256, 1, 15), no bias, then BatchNorm(256) (eval, eps 1e-5): w' = s w, b' = t (double on the host)
            const HostTensor* dw;
            std::vector<double> bs, bt;
            if ((rc = needw(h, cv + "4.conv.weight", dw)) || (rc = bn_fold(h, cv + "5", D, bs, bt))) return rc;
            std::vector<float> tw((size_t)15 * D), tb(D);
            for (int ch = 0; ch < D; ++ch) {
                for (int t = 0; t < 15; ++t) tw[(size_t)t * D + ch] = (float)(bs[ch] * (double)dw->data[(size_t)ch * 15 + t]);
                tb[ch] = (float)bt[ch];
            }
            if ((rc = dev_upload(h, &K.dw_w, tw))) return rc;
            if ((rc = dev_upload(h, &K.dw_b, tb))) return rc;
        }
        fl += (double)Tp * (K.pw1.flops_per_row + K.pw2.flops_per_row + 2.0 * 15 * D);
        if ((rc = upload_f32(h, p + "sequential.4.weight", &K.fin_g))) return rc;
        if ((rc = upload_f32(h, p + "sequential.4.bias", &K.fin_b))) return rc;
    }
    // pooling: attention.0 + ReLU with attention.2 (BatchNorm1d(128)) as the epilogue affine, attention.3 to fp32 logits
    if ((rc = make_conv(h, s.att0, "attention.0.weight", "attention.0.bias", "attention.2", 1))) return rc;
    if ((rc = make_conv(h, s.att3, "attention.3.weight", "attention.3.bias", "", 1))) return rc;
    if ((rc = make_bn(h, "attention_norm", 2 * D, &s.pbn_scale, &s.pbn_shift))) return rc;
    if ((rc = make_linear(h, s.fc, "fc.conv.weight", "fc.conv.bias"))) return rc;
    if (s.fc.N != nOut || s.fc.K != 2 * D) SV_FAIL(h, SVHIP_ERR_INVALID, "fc.conv.weight must be (%d, %d, 1)", nOut, 2 * D);
    {
        std::vector<float> half(D, 0.5f);
        if ((rc = dev_upload(h, &s.half, half))) return rc;
    }
    fl += (double)Tp * (s.att0.flops_per_row + s.att3.flops_per_row) + 2.0 * nOut * 2 * D;
    h->flops_per_utt = fl;
    return SVHIP_OK;
}

int conformer_alloc(svhip_handle* h) {
    h->model = std::make_unique<ConformerState>();
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const size_t B = c.max_batch, M = B * h->T;
    int rc;
    // the subsampling slice buffers, eleven (B T', <= 1024) activations, logits, pooled rows
    s.T1 = cf_sub(h->T); s.F1 = cf_sub(c.n_mels);
    s.Tp = cf_sub(s.T1); s.F2 = cf_sub(s.F1);
    // (the row buffers: a ragged pack of sum T_i <= B T mel frames has up to floor((B T - 3) / 4) subsampled rows, a few more than B T')
    const size_t Tp = s.Tp, Mp = std::max(B * Tp, (B * (size_t)h->T - 3) / 4), D = CF_D;
    s.rows_cap = Mp;
    s.chunk = cf_chunk(c, h->T);
    if ((rc = actbuf(h, &h->X_in, M * c.n_mels))) return rc;
    if ((rc = actbuf(h, &s.c1, (size_t)s.chunk * s.T1 * s.F1 * D))) return rc;
    if ((rc = actbuf(h, &s.s2, (size_t)s.chunk * Tp * s.F2 * D))) return rc;
    void** bufs[] = {&s.in, &s.b0, &s.x[0], &s.x[1], &s.r, &s.ln, &s.ln2, &s.ctx, &s.attn0, &s.last};
    for (void** b : bufs) if ((rc = actbuf(h, b, Mp * D))) return rc;
    if ((rc = actbuf(h, &s.hid, Mp * 4 * D))) return rc;
    if ((rc = dev_alloc(h, &s.logits, Mp * D))) return rc;
    if ((rc = dev_alloc(h, &s.pool_raw, B * 2 * D))) return rc;
    if ((rc = dev_alloc(h, &s.pool, B * 2 * D))) return rc;
    return SVHIP_OK;
}

static int cf_ln(svhip_handle* h, const void* x, void* y, const float* g, const float* b, int64_t M, void* y2 = nullptr,
                 const float* g2 = nullptr, const float* b2 = nullptr) {
    return run(h, "cf_ln", 0, [&]() { return launch_cf_ln(x, y, g, b, y2, g2, b2, h->dt, M, h->cur); });
}

// A GEMM over the rows of a pack: the generic kernel, one label (the subsampling's conv2 brings its own rag_utt / rag_row0; the pointwise
// layers need none)
static int cf_rag_gemm(svhip_handle* h, const ConvLayer& L, const GemmParams& p) {
    return run(h, "rag_gemm", (double)p.M * L.flops_per_row, [&]() { return launch_gemm_ragged(p, h->bf16, h->cur); });
}

// The front-end and the subsampling have a form each (fixed-length chunks and whole-utterance slices are different algorithms); both
// leave the input projection in s.in.
// Fixed: Conv2dSubampling + input_projection (convolution.py:152-185, encoder.py:160-163), cf_chunk utterances at a time
static int cf_front_fixed(svhip_handle* h, const float* d_feat, int B) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const int T = h->T, Tp = s.Tp, F = c.n_mels, T1 = s.T1, F1 = s.F1, F2 = s.F2, e = h->esz, D = CF_D;
    hipStream_t st = h->cur;
    int rc;
    if ((rc = run(h, "prologue", 0, [&]() {
             return launch_prologue(d_feat, h->X_in, h->bf16, B, F, T, c.log_input, h->in_w, h->in_b, h->d_pstats, st);
         }))) return rc;
    for (int s0 = 0; s0 < B; s0 += s.chunk) {
        const int n = std::min(s.chunk, B - s0);
        if ((rc = run(h, "cf_conv1", 2.0 * 9 * D * n * T1 * F1, [&]() {
                 return launch_cf_conv1(off(h->X_in, (size_t)s0 * T * F, e), s.c1_w, s.c1_b, s.c1, h->dt, n, T, F, st);
             }))) return rc;
        GemmParams p2 = conv_params(h, s.c2, s.c1, D, s.s2, D, n * Tp * F2, Tp * F2);
        p2.act1 = ACT_RELU;
        p2.seg_off = s.seg_off; p2.seg_rows = Tp * F2; p2.seg_len = 3 * D;
        p2.seg_stride = (int64_t)F1 * D; p2.seg_utt = (int64_t)T1 * F1 * D;
        if ((rc = conv_gemm(h, s.c2, p2))) return rc;
        GemmParams pp = conv_params(h, s.proj, s.s2, F2 * D, off(s.in, (size_t)s0 * Tp * D, e), D, n * Tp, Tp);
        if ((rc = conv_gemm(h, s.proj, pp))) return rc;
    }
    return SVHIP_OK;
}

// A pack (features at pk.in + pk.off[u]; levels: mel frames, subsampled frames), whole utterances at a time: a slice holds at most
// `chunk` utterances and chunk * T' subsampled frames, so that its conv1 image (2 T'_u + 1 <= T1 rows per utterance) and its conv2
// output fit the buffers of the fixed-length slices
static int cf_front_ragged(svhip_handle* h, const RagPack& pk) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const int n = pk.n, F = c.n_mels, F1 = s.F1, F2 = s.F2, e = h->esz, D = CF_D;
    const Seg &mel = pk.lv[0], &sub = pk.lv[1];
    const int* hrow0 = sub.hrow0;
    const bool bf = h->bf16;
    hipStream_t st = h->cur;
    int rc;
    if ((rc = run(h, "rag_rows", 0, [&]() { return launch_rag_rows(sub.row0, n, sub.maxT, sub.utt, st); }))) return rc;
    if ((rc = run(h, "rag_prologue", 0, [&]() {
             return launch_rag_prologue(pk.in, pk.off, mel.row0, n, mel.maxT, h->X_in, bf, F, c.log_input, h->in_w, h->in_b, s.rag_stats, st);
         }))) return rc;
    const int64_t slice_rows = (int64_t)s.chunk * s.Tp;
    for (int u0 = 0; u0 < n;) {
        int u1 = u0, mt = 0;
        while (u1 < n && u1 - u0 < s.chunk && hrow0[u1 + 1] - hrow0[u0] <= slice_rows) { mt = std::max(mt, hrow0[u1 + 1] - hrow0[u1]); ++u1; }
        const int rows = hrow0[u1] - hrow0[u0];
        if ((rc = run(h, "cf_conv1_rag", 2.0 * 9 * D * (2.0 * rows + (u1 - u0)) * F1, [&]() {
                 return launch_cf_conv1_ragged(h->X_in, s.c1_w, s.c1_b, s.c1, h->dt, mel.row0, sub.row0, u0, u1 - u0, mt, F, st);
             }))) return rc;
        GemmParams p2 = conv_params(h, s.c2, s.c1, D, s.s2, D, rows * F2, 1);
        p2.act1 = ACT_RELU;
        p2.seg_off = s.seg_off; p2.seg_rows = F2; p2.seg_len = 3 * D;          // (seg_off[f] = 2 f D: its first F2 entries, frame 0's)
        p2.seg_stride = (int64_t)F1 * D; p2.seg_utt = 2 * (int64_t)F1 * D; p2.seg_u0 = u0;
        p2.rag_utt = sub.utt + hrow0[u0]; p2.rag_row0 = sub.row0;
        if ((rc = cf_rag_gemm(h, s.c2, p2))) return rc;
        if ((rc = cf_rag_gemm(h, s.proj, conv_params(h, s.proj, s.s2, F2 * D, off(s.in, (size_t)hrow0[u0] * D, e), D, rows, 1)))) return rc;
        u0 = u1;
    }
    return SVHIP_OK;
}

// Conformer_.forward, written once for both forms.  pk null: a fixed-length batch of B utterances of h->T frames, (B, n_mels, T) at
// d_feat, on h->cur; the GEMMs take their routes through conv_gemm.  pk set: its n = B utterances as packed rows, on the handle's stream;
// every GEMM goes to the generic kernel (launch_gemm_ragged), LayerNorm is row-wise in both, and the steps that know where an utterance
// begins and ends run in their segment-table forms.  The helpers pick the form; below them the network reads once.
static int conformer_walk(svhip_handle* h, const float* d_feat, int B, const RagPack* pk) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const Seg* g = pk ? &pk->lv[1] : nullptr;          // the subsampled level: the rows of everything behind the subsampling
    const int T = g ? 1 : s.Tp, M = g ? g->M : B * T, F = c.n_mels, D = CF_D;      // (T: of the GEMMs; a pack's rows are their own frames)
    const bool bf = h->bf16;
    if (g) h->cur = h->stream;
    hipStream_t st = h->cur;
    int rc;
    auto gemm = [&](const ConvLayer& L, const GemmParams& p) { return g ? cf_rag_gemm(h, L, p) : conv_gemm(h, L, p); };
    // option cf_keep: the M x cols tensor block i has just stored (i < 0: the pooling's; `utt_rows`: one row per utterance), copied on st
    ++s.keep.epoch;
    auto keep = [&](int i, const char* what, const void* src, int cols, bool f32 = false, bool utt_rows = false) -> int {
        if (!h->opt.cf_keep) return SVHIP_OK;
        const std::string name = i < 0 ? std::string("cf_") + what : "cf_b" + std::to_string(i) + "_" + what;
        const int kind = f32 ? KEEP_F32 : KEEP_DT;
        if (utt_rows) return keep_stage(h, s.keep, st, name, src, kind, g ? (size_t)B : 1, g != nullptr, (size_t)c.max_batch, cols, 0, (size_t)B, B);
        return keep_stage(h, s.keep, st, name, src, kind, g ? (size_t)M : (size_t)T, g != nullptr, s.rows_cap, cols, 0, (size_t)M, B);
    };
    // relative-position attention of block i over hid = q | k | v -> ctx; a pack's P: rows 0 .. the longest T'_u seen (conformer_ragged_pos)
    auto attn = [&](int i, void* ctx) {
        const CfBlock& K = s.blocks[i];
        if (!g) return run(h, "cf_attn", 4.0 * B * T * (double)T * 3 * 2 * 64, [&]() {
            return launch_cf_attn(s.hid, 3 * D, K.P, D, K.u, K.v, ctx, D, h->dt, B, T, st);
        });
        const float* P = s.rag_P + (size_t)i * s.rag_P_rows * D;
        return run(h, "cf_attn_rag", 0, [&]() { return launch_cf_attn_ragged(s.hid, 3 * D, P, D, K.u, K.v, ctx, D, h->dt, g->row0, B, g->maxT, st); });
    };
    auto glu_dw = [&](const CfBlock& K) {          // BN(dw15(GLU(hid))) -> s.ctx
        return run(h, g ? "cf_glu_dw_rag" : "cf_glu_dw", 2.0 * 15 * D * M, [&]() {
            return g ? launch_cf_glu_dw_ragged(s.hid, K.dw_w, K.dw_b, s.ctx, h->dt, g->row0, B, g->maxT, st)
                     : launch_cf_glu_dw(s.hid, K.dw_w, K.dw_b, s.ctx, h->dt, B, T, st);
        });
    };
    if ((rc = g ? cf_front_ragged(h, *pk) : cf_front_fixed(h, d_feat, B))) return rc;
    // the blocks (encoder.py:32-110).  Buffers: x (block input) -> r -> xo -> r -> ln2 -> xo = LN(.) (+ the next block's FF LayerNorm)
    const void* x = s.in;
    const int nb = (int)s.blocks.size();
    if ((rc = cf_ln(h, x, s.ln, s.blocks[0].ff_g[0], s.blocks[0].ff_b[0], M))) return rc;
    for (int i = 0; i < nb; ++i) {
        const CfBlock& K = s.blocks[i];
        void* xo = i == 0 ? s.b0 : i == nb - 1 ? s.last : s.x[i & 1];
        void* ctx = i == 0 ? s.attn0 : s.ctx;
        // r = x + 0.5 FF(x); cf_ln already holds LN(x)                                                 feed_forward.py:23-57
        GemmParams f1 = conv_params(h, K.ff1[0], s.ln, D, s.hid, 4 * D, M, T);
        f1.act1 = ACT_SWISH;
        if ((rc = gemm(K.ff1[0], f1))) return rc;
        GemmParams f2 = conv_params(h, K.ff2[0], s.hid, 4 * D, s.r, D, M, T);
        f2.scale = s.half; f2.shift = h->d_zeros; f2.R = x; f2.ldr = D;
        if ((rc = gemm(K.ff2[0], f2)) || (rc = keep(i, "ff1", s.r, D))) return rc;
        // xo = r + out_proj(attention(LN(r)))                                                        attention.py:75-159
        if ((rc = cf_ln(h, s.r, s.ln, K.att_g, K.att_b, M))) return rc;
        if ((rc = gemm(K.qkv, conv_params(h, K.qkv, s.ln, D, s.hid, 3 * D, M, T))) || (rc = keep(i, "qkv", s.hid, 3 * D))) return rc;
        if ((rc = attn(i, ctx)) || (rc = keep(i, "ctx", ctx, D))) return rc;
        GemmParams po = conv_params(h, K.out, ctx, D, xo, D, M, T);
        po.R = s.r; po.ldr = D;
        if ((rc = gemm(K.out, po)) || (rc = keep(i, "att", xo, D))) return rc;
        // r = xo + pw2(swish(BN(dw15(GLU(pw1(LN(xo)))))))                                             convolution.py:108-149
        if ((rc = cf_ln(h, xo, s.ln, K.cv_g, K.cv_b, M))) return rc;
        if ((rc = gemm(K.pw1, conv_params(h, K.pw1, s.ln, D, s.hid, 2 * D, M, T))) || (rc = keep(i, "pw1", s.hid, 2 * D))) return rc;
        if ((rc = glu_dw(K)) || (rc = keep(i, "dw", s.ctx, D))) return rc;
        GemmParams pw = conv_params(h, K.pw2, s.ctx, D, s.r, D, M, T);
        pw.R = xo; pw.ldr = D;
        if ((rc = gemm(K.pw2, pw)) || (rc = keep(i, "conv", s.r, D))) return rc;
        // ln2 = r + 0.5 FF'(r); xo = LN(ln2), and the next block's LN(xo) in the same pass
        if ((rc = cf_ln(h, s.r, s.ln, K.ff_g[1], K.ff_b[1], M))) return rc;
        GemmParams g1 = conv_params(h, K.ff1[1], s.ln, D, s.hid, 4 * D, M, T);
        g1.act1 = ACT_SWISH;
        if ((rc = gemm(K.ff1[1], g1))) return rc;
        GemmParams g2 = conv_params(h, K.ff2[1], s.hid, 4 * D, s.ln2, D, M, T);
        g2.scale = s.half; g2.shift = h->d_zeros; g2.R = s.r; g2.ldr = D;
        if ((rc = gemm(K.ff2[1], g2)) || (rc = keep(i, "ff2", s.ln2, D))) return rc;
        const CfBlock* nx = i + 1 < nb ? &s.blocks[i + 1] : nullptr;
        if ((rc = cf_ln(h, s.ln2, xo, K.fin_g, K.fin_b, M, nx ? s.ln : nullptr, nx ? nx->ff_g[0] : nullptr, nx ? nx->ff_b[0] : nullptr)))
            return rc;
        if ((rc = keep(i, "out", xo, D))) return rc;
        x = xo;
    }
    // attentive statistics pooling (Conformer.py:130-142)
    GemmParams pa = conv_params(h, s.att0, x, D, s.hid, 128, M, T);
    pa.act1 = ACT_RELU;
    if ((rc = gemm(s.att0, pa))) return rc;
    GemmParams pl = conv_params(h, s.att3, s.hid, 128, s.logits, D, M, T);
    pl.out_f32 = 1;
    if ((rc = gemm(s.att3, pl)) || (rc = keep(-1, "logits", s.logits, D, true))) return rc;
    if ((rc = run(h, g ? "rag_asp_pool" : "cf_asp_pool", 0, [&]() {
             return g ? launch_rag_asp_pool(s.logits, x, bf, D, g->row0, B, D, s.pbn_scale, s.pbn_shift, s.pool_raw, s.pool, 1e-4f, st, 1e4f)
                      : launch_asp_pool(s.logits, x, bf, D, B, T, D, s.pbn_scale, s.pbn_shift, s.pool_raw, s.pool, 1e-4f, 1e4f, st);
         }))) return rc;
    if ((rc = keep(-1, "pool_raw", s.pool_raw, 2 * D, true, true))) return rc;
    // an utterance with a non-finite input value gets a NaN embedding, as in the reference (the ReLU epilogues would have dropped it): its
    // own row only
    if ((rc = run(h, "cf_in_check", 0, [&]() {
             return g ? launch_tn_nonfinite_rows_ragged(d_feat, pk->off, pk->lv[0].row0, F, B, s.pool, 2 * D, 2 * D, st)
                      : launch_tn_nonfinite_rows(d_feat, (int64_t)F * h->T, B, s.pool, 2 * D, 2 * D, st);
         }))) return rc;
    return run(h, g ? "rag_fc" : "cf_fc", 2.0 * B * s.fc.N * s.fc.K, [&]() {
        return g ? launch_rag_linear(s.pool, 2 * D, s.fc.W, s.fc.bias, h->d_emb, c.embed_dim, B, c.embed_dim, 2 * D, ACT_NONE, st)
                 : launch_rowvec_linear(s.pool, 2 * D, s.fc.W, s.fc.bias, h->d_emb, c.embed_dim, B, c.embed_dim, 2 * D, ACT_NONE, st);
    });
}

static int conformer_forward_part(svhip_handle* h, const float* d_feat, int, int B) { return conformer_walk(h, d_feat, B, nullptr); }
int conformer_forward(svhip_handle* h, const float* d_feat, int B) { return forward_lanes(h, conformer_forward_part, d_feat, B, 1, B); }

// ---- ragged packs ------------------------------------------------------------------------------------------
// the Conformer's own rules on an utterance of T >= 7 frames: T' within the positional encoding and within one subsampling slice
// (slice: the subsampled frames a slice of the handle holds)
static int cf_ragged_utt_rule(int64_t slice, int i, int64_t T, std::string& err) {
    const int64_t Tp = (T - 3) / 4;
    if (Tp > CF_MAX_T)
        return refuse(err, SVHIP_ERR_INVALID, "utterance %d: T' = %lld subsampled frames, over the %d positions of the positional encoding", i,
                      (long long)Tp, CF_MAX_T);
    if (Tp > slice)
        return refuse(err, SVHIP_ERR_INVALID, "utterance %d: T' = %lld subsampled frames, over the %lld one subsampling slice of this handle holds (its "
                      "conv1 image must fit the slice buffer)", i, (long long)Tp, (long long)slice);
    return SVHIP_OK;
}

// The Conformer's rules for a pack (RaggedCheckFn; include/svhip.h), on the host alone
int conformer_ragged_check(const svhip_config& c, const int32_t* lengths, int n, bool is_wave, std::string& err) {
    const bool cfg_ok = c.n_mels >= 7 && (c.hop_length <= 0 || c.samples / c.hop_length + 1 >= 7);      // (hop_length <= 0: refused by the shared rules)
    int64_t slice = 0;          // (of a configuration the shared rules take: cf_chunk divides by the conv1 image of T >= 7 frames)
    if (cfg_ok && c.hop_length > 0) {
        const int Th = (int)mel_frames(c, c.samples, true);
        slice = (int64_t)cf_chunk(c, Th) * cf_sub(cf_sub(Th));
    }
    return rag_mel_check(c, lengths, n, is_wave, err, cfg_ok, "hop_length / max_batch / samples / n_mels", 7,
                         " (two 3 x 3 stride-2 convolutions leave T' = (T - 3) / 4 >= 1)", cf_ragged_utt_rule, slice);
}

// two frame levels: the mel frames and the subsampled frames
static void cf_rag_frames(const svhip_config& c, int64_t len, bool is_wave, int T[RAG_LEVELS]) {
    T[0] = (int)mel_frames(c, len, is_wave);
    T[1] = cf_sub(cf_sub(T[0]));
}
static const RagRule kConformerRag = {2, cf_rag_frames, true};

// P of every layer for rows [0, rows): the double-precision row sums of finalize, so the first T' rows are the handle's own P bit for
// bit.  Grown (in steps of 256 rows) when a pack brings a longer utterance than any before it; a handle without ragged calls never
// gets here.
static int conformer_ragged_pos(svhip_handle* h, int rows) {
    auto& s = S(h);
    if (rows <= s.rag_P_rows) return SVHIP_OK;
    rows = std::min(CF_MAX_T, (rows + 255) & ~255);
    SV_HIP(h, hipStreamSynchronize(h->stream));        // (earlier calls may still read the old table)
    if (s.rag_P) (void)hipFree(s.rag_P);
    s.rag_P = nullptr; s.rag_P_rows = 0;
    const size_t per = (size_t)rows * CF_D;
    hipError_t e = hipMalloc((void**)&s.rag_P, CF_LAYERS * per * 4);
    if (e != hipSuccess) SV_FAIL(h, SVHIP_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", CF_LAYERS * per * 4, hipGetErrorString(e));
    std::vector<float> P(CF_LAYERS * per);
    for (int i = 0; i < CF_LAYERS; ++i) cf_pos_rows(s.pe_host[s.pe_of[i]].data(), s.wpos_host[i].data(), rows, P.data() + i * per);
    SV_HIP(h, hipMemcpy(s.rag_P, P.data(), P.size() * 4, hipMemcpyHostToDevice));
    s.rag_P_rows = rows;
    return SVHIP_OK;
}

int conformer_embed_ragged(svhip_handle* h, const float* in, bool in_host, bool is_wave, const int64_t* in_off, const int32_t* lengths, int n) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const size_t utt_cap[RAG_LEVELS] = {0, s.rows_cap};          // (nothing reads the mel level's utt table)
    RagPack pk;
    int rc;
    if (!s.rag_stats && (rc = dev_alloc(h, &s.rag_stats, (size_t)c.max_batch * c.n_mels * 2))) return rc;
    if ((rc = rag_pack(h, s.rag, kConformerRag, utt_cap, in, in_host, is_wave, in_off, lengths, n, pk))) return rc;
    // (a guard in front of the walk's writes: a pack that passed conformer_ragged_check has sum (T_u - 3) / 4 <= rows_cap rows)
    const Seg& sub = pk.lv[1];
    if ((size_t)sub.M > s.rows_cap) SV_FAIL(h, SVHIP_ERR_INVALID, "the pack has %d subsampled rows, over the %zu the handle holds", sub.M, s.rows_cap);
    if ((rc = conformer_ragged_pos(h, sub.maxT)) || (rc = conformer_walk(h, pk.in, n, &pk))) return rc;
    set_rag_rows(h, pk);
    return SVHIP_OK;
}

// the stages of option cf_keep: cf_logits, cf_pool_raw, cf_b<block>_ff1 | _qkv | _ctx | _att | _pw1 | _dw | _conv | _ff2 | _out
static bool cf_keep_name(const std::string& n) {
    if (n == "cf_logits" || n == "cf_pool_raw") return true;
    if (n.size() < 7 || n.compare(0, 4, "cf_b") != 0 || n[4] < '0' || n[4] >= '0' + CF_LAYERS || n[5] != '_') return false;
    const std::string w = n.substr(6);
    for (const char* q : {"ff1", "qkv", "ctx", "att", "pw1", "dw", "conv", "ff2", "out"}) if (w == q) return true;
    return false;
}

int conformer_stage(svhip_handle* h, const std::string& n, bool, StageView& v) {      // cf_in, cf_block0, cf_attn0, cf_last, cf_pool; option cf_keep's
    auto& s = S(h);
    v.rows = h->rag_levels ? (size_t)h->rag_rows[1] : (size_t)h->lastB * s.Tp; v.cols = v.ld = CF_D;      // (a ragged forward: the packed rows)
    if (n == "cf_in") v.src = s.in;
    else if (n == "cf_block0") v.src = s.b0;
    else if (n == "cf_attn0") v.src = s.attn0;
    else if (n == "cf_last") v.src = s.last;
    else if (n == "cf_pool") { v.src = s.pool; v.rows = h->lastB; v.cols = v.ld = 2 * CF_D; v.f32 = true; }
    else if (cf_keep_name(n)) return kept_view(h, s.keep, n, h->lastB, "cf_keep", h->opt.cf_keep != 0, v);
    else return unknown_stage(h, n);
    return SVHIP_OK;
}

}  // namespace svhip

extern "C" int svhip_conformer_attention(const void* qkv, const float* P, const float* u_bias, const float* v_bias, void* ctx, int32_t compute,
                                         int32_t B, int32_t T_sub, void* stream) {
    using namespace svhip;
    if ((compute != SVHIP_F32 && compute != SVHIP_BF16) || T_sub < 1 || T_sub > CF_MAX_T) return SVHIP_ERR_INVALID;
    const hipError_t e = launch_cf_attn(qkv, 3 * CF_D, P, CF_D, u_bias, v_bias, ctx, CF_D, compute == SVHIP_BF16 ? DT_BF16 : DT_F32, B, T_sub,
                                        reinterpret_cast<hipStream_t>(stream));
    return e == hipSuccess ? SVHIP_OK : e == hipErrorInvalidValue ? SVHIP_ERR_INVALID : SVHIP_ERR_HIP;
}

extern "C" int svhip_conformer_attention_ragged(const void* qkv, const float* P, const float* u_bias, const float* v_bias, void* ctx,
                                                int32_t compute, const int32_t* row0_dev, int32_t n, int32_t max_T_sub, void* stream) {
    using namespace svhip;
    if ((compute != SVHIP_F32 && compute != SVHIP_BF16) || max_T_sub < 1 || max_T_sub > CF_MAX_T) return SVHIP_ERR_INVALID;
    const hipError_t e = launch_cf_attn_ragged(qkv, 3 * CF_D, P, CF_D, u_bias, v_bias, ctx, CF_D, compute == SVHIP_BF16 ? DT_BF16 : DT_F32, row0_dev,
                                               n, max_T_sub, reinterpret_cast<hipStream_t>(stream));
    return e == hipSuccess ? SVHIP_OK : e == hipErrorInvalidValue ? SVHIP_ERR_INVALID : SVHIP_ERR_HIP;
}
