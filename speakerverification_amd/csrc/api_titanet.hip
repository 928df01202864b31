// api_titanet.hip — TitaNet in libsvhip (reference models/TitaNet.py:184-431, blocks/titanet_blocks.py): its create rules, weight names
// and packing, workspace, forward and stages.
//
// Buffers (titanet_alloc): six (B T, H) activations — PRO (prolog output), X (block output), D0 (block 0's first depthwise output),
// D (depthwise outputs), S (pointwise outputs), K (skip) — then ENC (B T, 1536), ATT (B T, 128) and the fp32 energies (B T, 1536).
// Every BatchNorm is folded into the conv before it (titanet_finalize), so the GEMM epilogues apply at most a ReLU.
//
// One mega-block (TitaNet.py:293-318) on x:
//   skip     K = BN(conv1x1(x))                                  conv_gemm
//   sub 1    d = dw_1(x) + b                                     tn_dw (block 0; later blocks get it from the previous tn_mega_tail)
//            S = relu(BN(pw_1 d))                                conv_gemm
//   sub 2, 3 D = dw_j(S) + b, S = relu(BN(pw_j D))               tn_dw, conv_gemm (the third also leaves the SE squeeze as column sums
//                                                              when its kernel writes them; otherwise colmean)
//   SE       g = sigmoid(W2 relu(W1 mean_t S))                   se_mlp (zero biases)
//   tail     X = relu(K + g S) and D = dw_1'(X) + b' of the next block in the same pass      tn_mega_tail
//
// A ragged pack (titanet_embed_ragged): n utterances of T_u mel frames back to back, sum T_u <= Bmax T rows of the same buffers.  The
// network has no subsampling, so the pack has one frame level and one row0 table.  titanet_walk is the one walk of the layers: for a
// pack every GEMM goes through launch_gemm_ragged (the prolog's three taps zero-padded at each utterance's own ends), the depthwise
// convs and the block tail run in their segment-table forms, and the SE squeeze, the pooling, the input test and the last linear layer
// are the fixed kernels' RAG instances (launch_rag_*): no value of an utterance depends on what it is packed with.
#include <cmath>
#include <cstdlib>

#include "handle.h"

namespace svhip {

namespace {

int tn_kernel_size(int H) { return H == 256 ? 3 : H == 512 ? 7 : H == 1024 ? 11 : 0; }      // TitaNet s / m / l (TitaNet.py:152-157)

struct TnBlock {
    float* dw_w[3] = {};                  // depthwise weights, tap-major [k][H] fp32
    float* dw_b[3] = {};                  // depthwise biases [H]
    ConvLayer pw[3], skip;                // pointwise convs + BN (ReLU in the epilogue); the 1 x 1 skip + BN
    float* se1 = nullptr;                 // excitation.0 [H / 16][H] (bf16 handles: bf16 copy in se1_bf)
    float* se2T = nullptr;                // excitation.2 transposed [H / 16][H]
    void *se1_bf = nullptr, *se2T_bf = nullptr;
};

// TitaNet layers (SVHIP_MODEL_TITANET: models/TitaNet.py).  Every BatchNorm follows its conv directly, so it is folded into that
// conv's weights and bias at finalize (the GEMM epilogues apply at most the ReLU)
struct TitaNetState : ModelState {
    std::vector<TnBlock> blocks;          // one per mega-block
    int k = 0;                            // depthwise kernel size (3 / 7 / 11 for H = 256 / 512 / 1024)
    ConvLayer prolog, epilog, att_in, att_out;     // prolog (k = 3, zero padding), epilog, attention in_linear / out_linear
    float *pbn_scale = nullptr, *pbn_shift = nullptr;        // decoder.pool.1 (BatchNorm1d(3072))
    LinearLayer fc;                       // decoder.linear.0 with decoder.linear.1 (BatchNorm1d(nOut)) folded in
    void* buf[6] = {};                    // (Bmax T, H) each: prolog output, block output, block 0's first depthwise output, depthwise
                                          // output, sub-block output, skip (the first three are the stages tn_prolog / tn_mega_last / tn_dw0)
    void* enc = nullptr;                  // (Bmax T, 1536) epilog output
    void* att = nullptr;                  // (Bmax T, 128) tanh(in_linear(.))
    float* logits = nullptr;              // (Bmax T, 1536) fp32 attention energies
    float *mean = nullptr, *gate = nullptr;                  // (Bmax, H) SE squeeze, SE gate
    float *pool_raw = nullptr, *pool = nullptr;              // (Bmax, 3072) pooled [mean | std], after BN
    // ragged packs (allocated by the first ragged call; the buffers above already hold Bmax T rows)
    RagTables rag;                        // the tables of a call (one level: mel frames, Bmax T rows) and the waveform staging buffer
    KeptStages keep;                      // option tn_keep: copies of what the walk stored, by stage name (keep_stage fills them)
};

TitaNetState& S(svhip_handle* h) { return static_cast<TitaNetState&>(*h->model); }

}  // namespace

int titanet_check(const svhip_config& c, const char*& err) {
    if (c.compute != SVHIP_F32 && c.compute != SVHIP_BF16) { err = "TitaNet runs on SVHIP_F32 and SVHIP_BF16 handles only"; return SVHIP_ERR_UNSUPPORTED; }
    if (!tn_kernel_size(c.channels)) { err = "TitaNet is built for H = 256 / 512 / 1024 (sizes s / m / l: channels)"; return SVHIP_ERR_INVALID; }
    if (c.log_input || c.input_norm) { err = "TitaNet reads the mel power as it is: log_input and input_norm must be 0"; return SVHIP_ERR_INVALID; }
    if (c.embed_dim <= 0) { err = "TitaNet needs embed_dim > 0"; return SVHIP_ERR_INVALID; }
    return SVHIP_OK;
}

// TitaNet.MainModel (TitaNet.py:124-159,202-318,321-431): the names of its state dict for SVHIP_TITANET_MAX_BLOCKS mega-blocks; a checkpoint
// holds the first n of them (titanet_finalize)
static void tn_block_spec(int64_t H, int64_t k, const std::string& p, WeightSpec& spec) {
    for (int j = 0; j < 3; ++j) {
        const std::string q = p + "sub_blocks." + std::to_string(j) + ".conv_block.";
        spec[q + "0.conv.0.weight"] = {H, 1, k}; spec[q + "0.conv.0.bias"] = {H};
        spec[q + "0.conv.1.weight"] = {H, H, 1}; spec[q + "0.conv.1.bias"] = {H};
        spec_bn(spec, q + "1", H);
    }
    spec[p + "sub_blocks.3.excitation.0.weight"] = {H / 16, H}; spec[p + "sub_blocks.3.excitation.2.weight"] = {H, H / 16};
    spec[p + "skip_connection.0.weight"] = {H, H, 1}; spec[p + "skip_connection.0.bias"] = {H};
    spec_bn(spec, p + "skip_connection.1", H);
}

void titanet_spec(const svhip_config& c, WeightSpec& spec) {
    const int64_t H = c.channels, k = tn_kernel_size(c.channels), D = 1536, nOut = c.embed_dim;
    spec["encoder.prolog.conv_block.0.weight"] = {H, (int64_t)c.n_mels, 3}; spec["encoder.prolog.conv_block.0.bias"] = {H};
    spec_bn(spec, "encoder.prolog.conv_block.1", H);
    for (int i = 0; i < SVHIP_TITANET_MAX_BLOCKS; ++i) tn_block_spec(H, k, "encoder.mega_blocks." + std::to_string(i) + ".", spec);
    spec["encoder.epilog.conv_block.0.weight"] = {D, H, 1}; spec["encoder.epilog.conv_block.0.bias"] = {D};
    spec_bn(spec, "encoder.epilog.conv_block.1", D);
    spec["decoder.pool.0.in_linear.weight"] = {128, D}; spec["decoder.pool.0.in_linear.bias"] = {128};
    spec["decoder.pool.0.out_linear.weight"] = {D, 128}; spec["decoder.pool.0.out_linear.bias"] = {D};
    spec_bn(spec, "decoder.pool.1", 2 * D);
    spec["decoder.linear.0.weight"] = {nOut, 2 * D}; spec["decoder.linear.0.bias"] = {nOut};
    spec_bn(spec, "decoder.linear.1", nOut);
}

// contiguous mega-block indices loaded from 0
static int titanet_blocks_loaded(const svhip_handle* h) {
    int n = 0;
    while (n < SVHIP_TITANET_MAX_BLOCKS) {
        const std::string p = "encoder.mega_blocks." + std::to_string(n) + ".";
        auto it = h->host_w.lower_bound(p);
        if (it == h->host_w.end() || it->first.compare(0, p.size(), p) != 0) break;
        ++n;
    }
    return n;
}

// conv (N, cin, taps) + bias followed directly by BatchNorm1d(eval, eps 1e-5): the BN folded into the conv, W' = s W, b' = s b + t (double
// arithmetic on the host), packed as a plain conv layer
static int make_conv_bn(svhip_handle* h, ConvLayer& L, const std::string& conv, const std::string& bnp) {
    const HostTensor *w, *b;
    std::vector<double> s, t;
    int rc;
    if ((rc = needw(h, conv + ".weight", w)) || (rc = needw(h, conv + ".bias", b)) || (rc = bn_fold(h, bnp, (int)w->shape[0], s, t))) return rc;
    const int64_t N = w->shape[0], per = w->numel() / N;
    HostTensor fw = *w;
    std::vector<float> fb(N);
    for (int64_t n = 0; n < N; ++n) {
        for (int64_t i = 0; i < per; ++i) fw.data[n * per + i] = (float)(s[n] * (double)w->data[n * per + i]);
        fb[n] = (float)(s[n] * (double)b->data[n] + t[n]);
    }
    if ((rc = make_conv(h, L, fw, &fb, 1))) return rc;
    L.scale = h->d_ones;          // (an identity affine: the persistent 16-bit GEMM takes layers that carry all three vectors)
    L.shift = h->d_zeros;
    return SVHIP_OK;
}

int titanet_finalize(svhip_handle* h) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const int H = c.channels, k = tn_kernel_size(H), Hh = H / 16, D = 1536, nOut = c.embed_dim, T = h->T;
    const int nb = titanet_blocks_loaded(h);
    if (nb == 0) SV_FAIL(h, SVHIP_ERR_MISSING, "no mega-block was loaded (encoder.mega_blocks.0.*)");
    for (auto& kv : h->host_w)          // a gap: tensors of a block beyond the contiguous run
        if (kv.first.rfind("encoder.mega_blocks.", 0) == 0 && atoi(kv.first.c_str() + 20) >= nb)
            SV_FAIL(h, SVHIP_ERR_MISSING, "%s is loaded but mega-block %d is missing (blocks are counted contiguously from 0)", kv.first.c_str(), nb);
    {
        WeightSpec bspec;
        for (int i = 0; i < nb; ++i) tn_block_spec(H, k, "encoder.mega_blocks." + std::to_string(i) + ".", bspec);
        for (auto& kv : bspec)
            if (!h->host_w.count(kv.first) && kv.first.find("num_batches_tracked") == std::string::npos)
                SV_FAIL(h, SVHIP_ERR_MISSING, "tensor %s was never loaded (mega-block count %d)", kv.first.c_str(), nb);
    }
    s.k = k;
    s.blocks.assign(nb, TnBlock{});
    int rc;
    if ((rc = make_conv_bn(h, s.prolog, "encoder.prolog.conv_block.0", "encoder.prolog.conv_block.1"))) return rc;
    double fl = s.prolog.flops_per_row;
    for (int i = 0; i < nb; ++i) {
        TnBlock& Bk = s.blocks[i];
        const std::string p = "encoder.mega_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < 3; ++j) {
            const std::string q = p + "sub_blocks." + std::to_string(j) + ".conv_block.";
            const HostTensor* dw = getw(h, q + "0.conv.0.weight");            // (H, 1, k)
            if (!dw || dw->shape.size() != 3 || dw->shape[2] != k) SV_FAIL(h, SVHIP_ERR_INVALID, "%s0.conv.0.weight: depthwise kernel size must be %d", q.c_str(), k);
            std::vector<float> tw((size_t)k * H);
            for (int cch = 0; cch < H; ++cch)
                for (int t = 0; t < k; ++t) tw[(size_t)t * H + cch] = dw->data[(size_t)cch * k + t];
            if ((rc = dev_upload(h, &Bk.dw_w[j], tw))) return rc;
            if ((rc = upload_f32(h, q + "0.conv.0.bias", &Bk.dw_b[j]))) return rc;
            if ((rc = make_conv_bn(h, Bk.pw[j], q + "0.conv.1", q + "1"))) return rc;
            fl += Bk.pw[j].flops_per_row + 2.0 * k * H;
        }
        if ((rc = make_conv_bn(h, Bk.skip, p + "skip_connection.0", p + "skip_connection.1"))) return rc;
        fl += Bk.skip.flops_per_row;
        const HostTensor *w1 = getw(h, p + "sub_blocks.3.excitation.0.weight"), *w2 = getw(h, p + "sub_blocks.3.excitation.2.weight");
        std::vector<float> m1(w1->data), m2((size_t)Hh * H);
        for (int cch = 0; cch < H; ++cch)
            for (int n = 0; n < Hh; ++n) m2[(size_t)n * H + cch] = w2->data[(size_t)cch * Hh + n];
        if ((rc = dev_upload(h, &Bk.se1, m1))) return rc;
        if ((rc = dev_upload(h, &Bk.se2T, m2))) return rc;
        if (h->bf16) {
            if ((rc = upload_h16(h, m1, &Bk.se1_bf))) return rc;
            if ((rc = upload_h16(h, m2, &Bk.se2T_bf))) return rc;
        }
    }
    if ((rc = make_conv_bn(h, s.epilog, "encoder.epilog.conv_block.0", "encoder.epilog.conv_block.1"))) return rc;
    if ((rc = make_conv(h, s.att_in, "decoder.pool.0.in_linear.weight", "decoder.pool.0.in_linear.bias", "", 1))) return rc;
    if ((rc = make_conv(h, s.att_out, "decoder.pool.0.out_linear.weight", "decoder.pool.0.out_linear.bias", "", 1))) return rc;
    if ((rc = make_bn(h, "decoder.pool.1", 2 * D, &s.pbn_scale, &s.pbn_shift))) return rc;
    {
        // decoder.linear = Linear(3072, nOut) + BatchNorm1d(nOut): folded into one fp32 linear
        const HostTensor *w = getw(h, "decoder.linear.0.weight"), *b = getw(h, "decoder.linear.0.bias");
        std::vector<double> bs, bt;
        if ((rc = bn_fold(h, "decoder.linear.1", nOut, bs, bt))) return rc;
        std::vector<float> fw((size_t)nOut * 2 * D), fb(nOut);
        for (int n = 0; n < nOut; ++n) {
            for (int i = 0; i < 2 * D; ++i) fw[(size_t)n * 2 * D + i] = (float)(bs[n] * (double)w->data[(size_t)n * 2 * D + i]);
            fb[n] = (float)(bs[n] * (double)b->data[n] + bt[n]);
        }
        s.fc.N = nOut; s.fc.K = 2 * D;
        if ((rc = dev_upload(h, &s.fc.W, fw))) return rc;
        if ((rc = dev_upload(h, &s.fc.bias, fb))) return rc;
    }
    fl += s.epilog.flops_per_row + s.att_in.flops_per_row + s.att_out.flops_per_row;
    h->flops_per_utt = (double)T * fl + 2.0 * nOut * 2 * D;
    return SVHIP_OK;
}

int titanet_alloc(svhip_handle* h) {
    h->model = std::make_unique<TitaNetState>();
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const size_t B = c.max_batch, M = B * h->T, H = c.channels;
    int rc;
    // six (B T, H) activation buffers, the encoder output, the attention activation and energies
    if ((rc = actbuf(h, &h->X_in, M * c.n_mels))) return rc;
    for (int i = 0; i < 6; ++i) if ((rc = actbuf(h, &s.buf[i], M * H))) return rc;
    if ((rc = actbuf(h, &s.enc, M * 1536))) return rc;
    if ((rc = actbuf(h, &s.att, M * 128))) return rc;
    if ((rc = dev_alloc(h, &s.logits, M * 1536))) return rc;
    if ((rc = dev_alloc(h, &s.mean, B * H))) return rc;
    if ((rc = dev_alloc(h, &s.gate, B * H))) return rc;
    if ((rc = dev_alloc(h, &s.pool_raw, B * 3072))) return rc;
    if ((rc = dev_alloc(h, &s.pool, B * 3072))) return rc;
    if (h->bf16) {          // the third pointwise GEMM's column-sum partials (the SE squeeze)
        h->colsum_region = (int64_t)((M + 255) / 256 + 2) * 16 * H;
        if ((rc = dev_alloc(h, &h->d_colsum, (size_t)2 * h->colsum_region))) return rc;
    }
    return SVHIP_OK;
}
// TitaNet.forward, written once for both forms.  pk null: a fixed-length batch of B utterances of h->T frames, (B, n_mels, T) at d_feat,
// on h->cur; the GEMMs take their routes through conv_gemm.  pk set: its n = B utterances as packed rows (features at d_feat + pk->off[u]),
// on the handle's stream; every GEMM goes to the generic kernel (launch_gemm_ragged: one kernel at every row count, so a row's sums do not
// depend on the pack), which is why the bf16 handles' column-sum squeeze is not used there.  The helpers pick the form; below them the
// network reads once.
static int titanet_walk(svhip_handle* h, const float* d_feat, int B, const RagPack* pk) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const Seg* g = pk ? &pk->lv[0] : nullptr;
    const int T = g ? 1 : h->T, M = g ? g->M : B * T, H = c.channels, E = 1536, k = s.k, dt = h->dt;      // (T: of the GEMMs; a pack's rows are their own frames)
    const bool bf = h->bf16;
    if (g) h->cur = h->stream;
    hipStream_t st = h->cur;
    void *PRO = s.buf[0], *X = s.buf[1], *D0 = s.buf[2], *D = s.buf[3], *Sb = s.buf[4], *K = s.buf[5];
    float* cs = !g && bf ? h->d_colsum : nullptr;       // the third pointwise GEMM's column-sum partials (fixed form, bf16)
    int rc;
    // option tn_keep: the M x cols tensor block i has just stored (i < 0: the pooling's; `utt_rows`: one row per utterance), copied on st
    ++s.keep.epoch;
    auto keep = [&](int i, const std::string& what, const void* src, int cols, bool f32 = false, bool utt_rows = false) -> int {
        if (!h->opt.tn_keep) return SVHIP_OK;
        const std::string name = i < 0 ? "tn_" + what : "tn_b" + std::to_string(i) + "_" + what;
        const int kind = f32 ? KEEP_F32 : KEEP_DT;
        if (utt_rows) return keep_stage(h, s.keep, st, name, src, kind, g ? (size_t)B : 1, g != nullptr, (size_t)c.max_batch, cols, 0, (size_t)B, B);
        return keep_stage(h, s.keep, st, name, src, kind, g ? (size_t)M : (size_t)T, g != nullptr, (size_t)c.max_batch * h->T, cols, 0, (size_t)M, B);
    };
    auto gemm = [&](const ConvLayer& L, GemmParams p, GemmPlan* plan = nullptr) {
        if (!g) return conv_gemm(h, L, p, nullptr, 0, plan);
        p.rag_utt = g->utt; p.rag_row0 = g->row0;
        return run(h, "rag_gemm", (double)M * L.flops_per_row, [&]() { return launch_gemm_ragged(p, bf, st); });
    };
    auto dw = [&](const void* x, void* d, const float* w, const float* b) {
        return run(h, g ? "tn_dw_rag" : "tn_dw", 2.0 * k * H * M, [&]() {
            return g ? launch_tn_dw_ragged(x, d, w, b, dt, k, g->row0, B, g->maxT, H, st) : launch_tn_dw(x, d, w, b, dt, k, B, T, H, st);
        });
    };
    auto squeeze = [&]() {          // mean_t Sb -> s.mean
        return g ? run(h, "rag_se_mean", 0, [&]() { return launch_rag_colstats(Sb, bf, H, g->row0, B, H, s.mean, false, 0.0f, st); })
                 : run(h, "tn_se_mean", 0, [&]() { return launch_colmean(Sb, dt, H, B, T, H, s.mean, st); });
    };
    // relu(skip + gate * Sb) -> X and, with a next block, its first depthwise conv -> D
    auto tail = [&](const TnBlock* nx) {
        const float *w = nx ? nx->dw_w[0] : nullptr, *b = nx ? nx->dw_b[0] : nullptr;
        void* d = nx ? D : nullptr;
        return run(h, g ? "tn_mega_tail_rag" : "tn_mega_tail", nx ? 2.0 * k * H * M : 0.0, [&]() {
            return g ? launch_tn_mega_tail_ragged(K, Sb, s.gate, X, w, b, d, dt, k, g->row0, B, g->maxT, H, st)
                     : launch_tn_mega_tail(K, Sb, s.gate, X, w, b, d, dt, k, B, T, H, st);
        });
    };
    // the mel power as it is (no log, no normalisation) -> frame-major rows (M, n_mels) in the compute type
    if (g) {
        if ((rc = run(h, "rag_rows", 0, [&]() { return launch_rag_rows(g->row0, B, g->maxT, g->utt, st); }))) return rc;
        if ((rc = run(h, "rag_prologue", 0, [&]() {
                 return launch_rag_prologue(d_feat, pk->off, g->row0, B, g->maxT, h->X_in, bf, c.n_mels, 0, nullptr, nullptr, h->d_pstats, st);
             }))) return rc;
    } else if ((rc = run(h, "prologue", 0, [&]() {
                    return launch_prologue(d_feat, h->X_in, bf, B, c.n_mels, T, 0, nullptr, nullptr, h->d_pstats, st);
                }))) return rc;
    // prolog: relu(BN(Conv1dSamePadding(n_mels, H, 3))), zero-padded at each utterance's own ends      TitaNet.py:226-227, titanet_blocks.py:123-139
    GemmParams pp = conv_params(h, s.prolog, h->X_in, c.n_mels, PRO, H, M, T);
    pp.act1 = ACT_RELU; pp.pad_mode = PAD_ZERO;
    if ((rc = gemm(s.prolog, pp))) return rc;
    const int nb = (int)s.blocks.size();
    const void* x = PRO;
    for (int i = 0; i < nb; ++i) {
        const TnBlock& Bk = s.blocks[i];
        if ((rc = gemm(Bk.skip, conv_params(h, Bk.skip, x, H, K, H, M, T))) || (rc = keep(i, "skip", K, H))) return rc;
        if (i == 0 && ((rc = dw(x, D0, Bk.dw_w[0], Bk.dw_b[0])) || (rc = keep(0, "dw0", D0, H)))) return rc;
        const void* d = i == 0 ? D0 : D;
        GemmPlan g3;
        for (int j = 0; j < 3; ++j) {
            GemmParams p = conv_params(h, Bk.pw[j], d, H, Sb, H, M, T);
            p.act1 = ACT_RELU;
            if (j == 2 && !g) { p.colsum = cs; p.colsum_stride = h->colsum_region; }
            if ((rc = gemm(Bk.pw[j], p, &g3)) || (rc = keep(i, "pw" + std::to_string(j), Sb, H))) return rc;
            if (j < 2) {
                if ((rc = dw(Sb, D, Bk.dw_w[j + 1], Bk.dw_b[j + 1])) || (rc = keep(i, "dw" + std::to_string(j + 1), D, H))) return rc;
                d = D;
            }
        }
        // squeeze-excitation (titanet_blocks.py:162-192): the squeeze from the GEMM's column sums when its kernel wrote them (never for a
        // pack: launch_gemm_ragged leaves g3 as it is)
        const bool from_part = g3.colsum_groups != 0;
        if (!from_part && ((rc = squeeze()) || (rc = keep(i, "mean", s.mean, H, true, true)))) return rc;
        if ((rc = run(h, "tn_se_mlp", 4.0 * B * (H / 16) * H, [&]() {
                 return launch_se_mlp(from_part ? nullptr : s.mean, from_part ? cs : nullptr, T, bf ? Bk.se1_bf : (const void*)Bk.se1, h->d_zeros,
                                      bf ? Bk.se2T_bf : (const void*)Bk.se2T, h->d_zeros, s.gate, bf, B, H, H / 16, st, from_part ? g3.colsum_groups : 8);
             })) || (rc = keep(i, "gate", s.gate, H, true, true))) return rc;
        // relu(skip + SE(sub_blocks(x))) and the next block's first depthwise conv                     TitaNet.py:306-318
        if ((rc = tail(i + 1 < nb ? &s.blocks[i + 1] : nullptr)) || (rc = keep(i, "out", X, H))) return rc;
        if (i + 1 < nb && (rc = keep(i + 1, "dw0", D, H))) return rc;
        x = X;
    }
    // epilog: relu(BN(conv1x1(x)))                                                   TitaNet.py:244-245
    GemmParams pe = conv_params(h, s.epilog, x, H, s.enc, E, M, T);
    pe.act1 = ACT_RELU;
    if ((rc = gemm(s.epilog, pe))) return rc;
    // attentive statistics pooling (TitaNet.py:389-431): energies = out_linear(tanh(in_linear(x))), softmax over T, mean and
    // sqrt(clamp(var, 1e-6)) (the variance in the centred form), then decoder.pool.1
    GemmParams pa = conv_params(h, s.att_in, s.enc, E, s.att, 128, M, T);
    pa.act2 = ACT_TANH;
    if ((rc = gemm(s.att_in, pa)) || (rc = keep(-1, "att", s.att, 128))) return rc;
    GemmParams pl = conv_params(h, s.att_out, s.att, 128, s.logits, E, M, T);
    pl.out_f32 = 1;
    if ((rc = gemm(s.att_out, pl)) || (rc = keep(-1, "logits", s.logits, E, true))) return rc;
    if ((rc = run(h, g ? "rag_asp_pool" : "tn_asp_pool", 0, [&]() {
             return g ? launch_rag_asp_pool(s.logits, s.enc, bf, E, g->row0, B, E, s.pbn_scale, s.pbn_shift, s.pool_raw, s.pool, 1e-6f, st)
                      : launch_asp_pool(s.logits, s.enc, bf, E, B, T, E, s.pbn_scale, s.pbn_shift, s.pool_raw, s.pool, 1e-6f, 0.0f, st);
         })) || (rc = keep(-1, "pool_raw", s.pool_raw, 2 * E, true, true))) return rc;
    // an utterance with a non-finite input value gets a NaN embedding, as in the reference (the ReLU epilogues would have dropped it): its
    // own row only
    if ((rc = run(h, "tn_in_check", 0, [&]() {
             return g ? launch_tn_nonfinite_rows_ragged(d_feat, pk->off, g->row0, c.n_mels, B, s.pool, 2 * E, 2 * E, st)
                      : launch_tn_nonfinite_rows(d_feat, (int64_t)c.n_mels * T, B, s.pool, 2 * E, 2 * E, st);
         }))) return rc;
    // decoder.linear: Linear(3072, nOut) with BatchNorm1d(nOut) folded in                                     TitaNet.py:355-358
    return run(h, g ? "rag_fc" : "tn_fc", 2.0 * B * s.fc.N * s.fc.K, [&]() {
        return g ? launch_rag_linear(s.pool, 2 * E, s.fc.W, s.fc.bias, h->d_emb, c.embed_dim, B, c.embed_dim, 2 * E, ACT_NONE, st)
                 : launch_rowvec_linear(s.pool, 2 * E, s.fc.W, s.fc.bias, h->d_emb, c.embed_dim, B, c.embed_dim, 2 * E, ACT_NONE, st);
    });
}

static int titanet_forward_part(svhip_handle* h, const float* d_feat, int, int B) { return titanet_walk(h, d_feat, B, nullptr); }
int titanet_forward(svhip_handle* h, const float* d_feat, int B) { return forward_lanes(h, titanet_forward_part, d_feat, B, 1, B); }

// ---- ragged packs ------------------------------------------------------------------------------------------
// TitaNet's rules for a pack (RaggedCheckFn; include/svhip.h), on the host alone
int titanet_ragged_check(const svhip_config& c, const int32_t* lengths, int n, bool is_wave, std::string& err) {
    return rag_mel_check(c, lengths, n, is_wave, err, true, "hop_length / max_batch / samples", 1, "");
}

// one frame level (the network has no subsampling): the mel frames
static void titanet_rag_frames(const svhip_config& c, int64_t len, bool is_wave, int T[RAG_LEVELS]) { T[0] = (int)mel_frames(c, len, is_wave); }
static const RagRule kTitanetRag = {1, titanet_rag_frames, true};

int titanet_embed_ragged(svhip_handle* h, const float* in, bool in_host, bool is_wave, const int64_t* in_off, const int32_t* lengths, int n) {
    const size_t utt_cap[RAG_LEVELS] = {(size_t)h->cfg.max_batch * h->T};
    RagPack pk;
    int rc;
    if ((rc = rag_pack(h, S(h).rag, kTitanetRag, utt_cap, in, in_host, is_wave, in_off, lengths, n, pk)) || (rc = titanet_walk(h, pk.in, n, &pk))) return rc;
    set_rag_rows(h, pk);
    return SVHIP_OK;
}

// the stages of option tn_keep: tn_att, tn_logits, tn_pool_raw, tn_b<block>_skip | _dw0 | _pw0 | _dw1 | _pw1 | _dw2 | _pw2 | _mean | _gate | _out
static bool tn_keep_name(const std::string& n) {
    if (n == "tn_att" || n == "tn_logits" || n == "tn_pool_raw") return true;
    if (n.compare(0, 4, "tn_b") != 0) return false;
    size_t i = 4;
    while (i < n.size() && n[i] >= '0' && n[i] <= '9') ++i;
    if (i == 4 || i > 6 || i >= n.size() || n[i] != '_' || atoi(n.c_str() + 4) >= SVHIP_TITANET_MAX_BLOCKS) return false;
    const std::string w = n.substr(i + 1);
    for (const char* q : {"skip", "dw0", "pw0", "dw1", "pw1", "dw2", "pw2", "mean", "gate", "out"}) if (w == q) return true;
    return false;
}

// (after a ragged forward the (rows, H) stages and tn_enc are the packed sum T_i rows: svhip_get_stage sets them from rag_rows)
int titanet_stage(svhip_handle* h, const std::string& n, bool, StageView& v) {      // tn_prolog, tn_dw0, tn_mega_last, tn_enc, tn_pool; option tn_keep's
    auto& s = S(h);
    const int H = h->cfg.channels;
    if (n == "tn_prolog") { v.src = s.buf[0]; v.cols = v.ld = H; }
    else if (n == "tn_mega_last") { v.src = s.buf[1]; v.cols = v.ld = H; }
    else if (n == "tn_dw0") { v.src = s.buf[2]; v.cols = v.ld = H; }
    else if (n == "tn_enc") { v.src = s.enc; v.cols = v.ld = 1536; }
    else if (n == "tn_pool") { v.src = s.pool; v.rows = h->lastB; v.cols = v.ld = 3072; v.f32 = true; }
    else if (tn_keep_name(n)) return kept_view(h, s.keep, n, h->lastB, "tn_keep", h->opt.tn_keep != 0, v);
    else return unknown_stage(h, n);
    return SVHIP_OK;
}

}  // namespace svhip

// ---- test exports: the depthwise kernels alone (include/svhip.h) ---------------------------------------------------
namespace {

// x != null: tn_dw; x == null: the block tail (with d also the next depthwise conv).  ragged: the pack forms, B = n and T = max_T
int tn_depthwise_export(const void* x, const void* skip, const void* h3, const float* gate, void* y, const float* w, const float* bias, void* d,
                        int compute, int k, int B, int T, int C, const int* row0, bool ragged, void* stream) {
    using namespace svhip;
    if (compute != SVHIP_F32 && compute != SVHIP_BF16) return SVHIP_ERR_INVALID;
    if (k != 3 && k != 7 && k != 11) return SVHIP_ERR_INVALID;
    if (ragged && !row0) return SVHIP_ERR_INVALID;
    const int dt = compute == SVHIP_BF16 ? DT_BF16 : DT_F32;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t e;
    if (x) e = ragged ? launch_tn_dw_ragged(x, d, w, bias, dt, k, row0, B, T, C, st) : launch_tn_dw(x, d, w, bias, dt, k, B, T, C, st);
    else e = ragged ? launch_tn_mega_tail_ragged(skip, h3, gate, y, w, bias, d, dt, k, row0, B, T, C, st)
                    : launch_tn_mega_tail(skip, h3, gate, y, w, bias, d, dt, k, B, T, C, st);
    return e == hipSuccess ? SVHIP_OK : e == hipErrorInvalidValue ? SVHIP_ERR_INVALID : SVHIP_ERR_HIP;
}

}  // namespace

extern "C" int svhip_titanet_depthwise(const void* x, const void* skip, const void* h3, const float* gate, void* y, const float* w, const float* bias,
                                       void* d, int32_t compute, int32_t k, int32_t B, int32_t T, int32_t C, void* stream) {
    return tn_depthwise_export(x, skip, h3, gate, y, w, bias, d, compute, k, B, T, C, nullptr, false, stream);
}

extern "C" int svhip_titanet_depthwise_ragged(const void* x, const void* skip, const void* h3, const float* gate, void* y, const float* w,
                                              const float* bias, void* d, int32_t compute, int32_t k, const int32_t* row0_dev, int32_t n,
                                              int32_t max_T, int32_t C, void* stream) {
    return tn_depthwise_export(x, skip, h3, gate, y, w, bias, d, compute, k, n, max_T, C, row0_dev, true, stream);
}
