// api_resnetse.hip — ResNetSE34V2 in libsvhip (reference models/ResNetSE34V2.py, ResNetBaseline.py:141-301, ResNetBlocks.py:211-246,292-307): its
// create rules, weight names and packing, workspace, forward and stages.
//
// Activations are channels-last (B, P, Q, C): P = frames (the reference's W), Q = mel rows (its H).  A reference weight (Cout, Cin, kh, kw)
// has kh over mel rows and kw over frames, so the kernels' tap (dp, dq) is its element [dq][dp].
//
// Buffers (resnetse_alloc): XIN (B, P, Q) fp32 normalised input; OUT[0] the stem output, OUT[1 .. 4] the stages' outputs; TMP[0 / 1] block
// outputs inside a stage, TMP[2] conv1's output, TMP[3] conv2's output, TMP[4] the downsample output; PART / GATE the SE squeeze and gates.
//
// One SEBasicBlockV2 on x (ResNetBlocks.py:229-246; `self.relu` is in place, so the residual is relu(x)):
//   conv1   u = relu(bn1(conv3x3_s(relu(x))))                     rs_conv (ReLU on the operand, BN + ReLU in the epilogue)
//   conv2   v = bn2(conv3x3(u)), tile sums of v                   rs_conv
//   SE      g = sigmoid(W2 relu(W1 mean(v) + b1) + b2)            rs_se_gate (the tile sums in tile order)
//   down    d = bn(conv1x1_s(relu(x)))   (first block of stages 2 - 4)      rs_conv, KS = 1
//   tail    out = relu((d | relu(x)) + g v)                       rs_se_apply
//
// A ragged pack (resnetse_embed_ragged): n utterances of T_u mel frames in ONE call.  Utterance u at frame level l is a (P_l,u, Q_l, C_l)
// image, P_0,u = T_u (the stem and layer1) and P_l+1,u = rs_out_size(P_l,u, 2) = ceil(P_l,u / 2) (layer2 .. layer4); the images lie back to
// back in utterance order in the buffers above, one row0 / utt table per level (RagRule: four levels).  resnetse_walk is the one walk of
// the layers: for a pack the convolutions run on the packed form of rs_conv (every utterance tiled by rs_conv_plan of its own image, the
// padding at its own first and last frame), the stem, the SE gate and the block tail in their segment-table forms, the two attention
// convolutions on launch_gemm_ragged and the pooling, the input test and fc on the launch_rag_* forms, so no value of an utterance depends
// on what it is packed with, and its stages are bit for bit those of a fixed-length handle of its length at B = 1.
// CAPACITY of a pack: 1 <= n <= max_batch and sum_u 8 ceil(T_u / 8) <= max_batch T.  The subsampling rounds up, so sum T_u <= max_batch T
// alone does not protect the deeper levels (max_batch = 4, T = 40, frames 37 + 41 + 41 + 41 = 160, but 19 + 21 + 21 + 21 = 82 > 4 * 20 rows
// at level 1); counting an utterance as 8 ceil(T_u / 8) rows does, at every level: P_l,u = ceil(T_u / 2^l) <= 8 ceil(T_u / 8) / 2^l for
// l <= 3 (the right side is an integer >= T_u / 2^l), and max_batch T / 2^l <= max_batch ceil(T / 2^l) = max_batch P_l.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "handle.h"

namespace svhip {

namespace {

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

// ResNetSE layers (SVHIP_MODEL_RESNETSE: models/ResNetSE34V2.py).  Activations are channels-last (B, P, Q, C), P frames x Q mel rows; every
// BatchNorm is the scale / shift of the convolution before it
struct ResNetSEState : ModelState {
    std::vector<RsBlock> blocks;          // the blocks of all stages in order
    int stage_end[4] = {};                // index one past the last block of each stage
    int P[5] = {}, Q[5] = {}, C[5] = {};  // image size and channels of the stem output [0] and of each stage's output [1 .. 4]
    float *stem_w = nullptr, *stem_b = nullptr, *stem_scale = nullptr, *stem_shift = nullptr;     // conv1 tap-major [9][32], bn1
    ConvLayer att0, att3;                 // attention.0 (+ ReLU, attention.2 as the epilogue affine), attention.3; K permuted to q C + c
    LinearLayer fc;                       // fc, columns permuted the same way
    bool sap = false;                     // encoder_type 'SAP': fc reads the weighted means only
    float* xin = nullptr;                 // (Bmax, P, Q) fp32: the normalised input
    void* out[5] = {};                    // the stem output and each stage's output (stages rs_stem, rs_layer1 .. rs_layer4)
    void* tmp[5] = {};                    // block outputs inside a stage (ping-pong), conv1 output, conv2 output, downsample output
    float *part = nullptr, *gate = nullptr;      // SE: per-tile channel sums of conv2's output, (Bmax, C) gates
    void* att = nullptr;                  // (Bmax P4, 128)
    float* logits = nullptr;              // (Bmax P4, Q4 C4) fp32
    float *pool_raw = nullptr, *pool = nullptr, *pool_one = nullptr, *pool_zero = nullptr;     // (Bmax, 2 Q4 C4) [mu | sg]
    // ragged packs (all allocated by the first ragged call; the buffers above already hold a pack's rows at every level)
    RagTables rag;                        // the tables of a call (four frame levels) and the waveform staging buffer
    int* rag_tiles = nullptr;             // RS_RAG_KINDS x (tile0 (Bmax + 1) | plan (Bmax)): the tile tables of a pack's convolutions
    float* rag_part = nullptr;            // the SE tile sums of a pack: rag_part_floats (rs_rag_part_floats) of them
    size_t rag_part_floats = 0;
    KeptStages keep;                      // option rs_keep: copies of what the walk stored, by stage name (keep_stage fills them)
};

ResNetSEState& S(svhip_handle* h) { return static_cast<ResNetSEState&>(*h->model); }

// The 2-D ResNet family as data: blocks per stage, widths, block kind.  A sibling depth is another row.
enum RsBlockKind { RS_SE_BASIC_V2 = 0 };
struct RsArch { int blocks[4]; int widths[4]; RsBlockKind kind; int se_hidden; int att_dim; };
const RsArch kResNetSE34V2 = {{3, 4, 6, 3}, {32, 64, 128, 256}, RS_SE_BASIC_V2, 16, 128};

const RsArch& arch_of(const svhip_config&) { return kResNetSE34V2; }
bool rs_is_sap(const svhip_config& c) { return c.channels == 1; }

// (Cout, Cin, ks, ks) -> [Cin / CK][ks ks][Cout][CK], tap = ks dp + dq = the reference's element [dq][dp], in fp32
std::vector<float> rs_pack(const float* w, int cout, int cin, int ks, int ck) {
    std::vector<float> out((size_t)cout * cin * ks * ks);
    const int taps = ks * ks;
    for (int n = 0; n < cout; ++n)
        for (int c = 0; c < cin; ++c)
            for (int dp = 0; dp < ks; ++dp)
                for (int dq = 0; dq < ks; ++dq)
                    out[((((size_t)(c / ck) * taps) + dp * ks + dq) * cout + n) * ck + c % ck] = w[(((size_t)n * cin + c) * ks + dq) * ks + dp];
    return out;
}

int rs_upload_packed(svhip_handle* h, const std::vector<float>& m, void** dst) {
    if (h->bf16) return upload_h16(h, m, dst);
    float* d;
    int rc = dev_upload(h, &d, m);
    *dst = d;
    return rc;
}

int make_rs_conv(svhip_handle* h, RsConv& L, const std::string& wname, const std::string& bnname, int cin, int cout, int ks, int stride) {
    const HostTensor* w;
    int rc;
    if ((rc = needw(h, wname, w))) return rc;
    L.cin = cin; L.cout = cout; L.ks = ks; L.stride = stride;
    if ((rc = rs_upload_packed(h, rs_pack(w->data.data(), cout, cin, ks, h->bf16 ? 32 : 16), &L.W))) return rc;
    return make_bn(h, bnname, cout, &L.scale, &L.shift);
}

RsConvParams rs_params(const RsConv& L, const void* x, void* y, int B, int P, int Q, bool relu_in, bool relu_out, float* part) {
    RsConvParams p;
    p.X = x; p.Y = y; p.W = L.W; p.scale = L.scale; p.shift = L.shift; p.part = part;
    p.B = B; p.P = P; p.Q = Q; p.Cin = L.cin; p.Cout = L.cout; p.stride = L.stride; p.ks = L.ks;
    p.relu_in = relu_in; p.relu_out = relu_out;
    rs_conv_plan(p);
    return p;
}

// ---- ragged packs: the tile tables of the convolutions ----------------------------------------------------------------------------
// A pack's convolutions come in ten kinds, each with its own tiles: 3 x 3 stride 1 inside level l (kind l, 0 .. 3), 3 x 3 stride 2 into
// level l (kind 3 + l, l = 1 .. 3) and the 1 x 1 stride-2 downsample into level l (kind 6 + l)
constexpr int RS_RAG_KINDS = 10;
struct RsRagKind { int l_in, l_out, stride, ks; };
RsRagKind rs_rag_kind(int k) {
    if (k < 4) return {k, k, 1, 3};
    return k < 7 ? RsRagKind{k - 4, k - 3, 2, 3} : RsRagKind{k - 7, k - 6, 2, 1};
}
int rs_rag_kind_of(const RsConv& L, int l_out) { return L.stride == 1 ? l_out : L.ks == 3 ? 3 + l_out : 6 + l_out; }

// The most SE tiles (of conv2: 3 x 3 stride 1 inside a level) a pack can have at level l, times C_l, maximised over the levels.  An
// utterance is tiled on its own, so short utterances give more tiles per row than max_batch ntp ntq of the fixed image.  The bound follows
// from the capacity rule: with w(T) = 8 ceil(T / 8) and rho_l = max over P of tiles_l(P) / w(the shortest T with P_l = P),
//   sum_u tiles_l(P_l,u) <= rho_l sum_u w(T_u) <= rho_l max_batch T.
size_t rs_rag_part_floats(const ResNetSEState& s, size_t cap) {
    size_t best = 0;
    for (int l = 0; l < 4; ++l) {
        double rho = 0.0;
        for (size_t P = 1; ((P - 1) << l) + 1 <= cap; ++P) {
            RsConvParams p;
            p.P = (int)P; p.Q = s.Q[l + 1]; p.stride = 1; p.ks = 3;
            rs_conv_plan(p);
            const size_t Tmin = ((P - 1) << l) + 1;
            rho = std::max(rho, (double)p.ntp * p.ntq / (double)((Tmin + 7) / 8 * 8));
        }
        best = std::max(best, ((size_t)std::ceil(rho * (double)cap) + 1) * s.C[l + 1]);
    }
    return best;
}

}  // namespace

int resnetse_check(const svhip_config& c, const char*& err) {
    if (c.compute != SVHIP_F32 && c.compute != SVHIP_BF16) { err = "ResNetSE runs on SVHIP_F32 and SVHIP_BF16 handles only"; return SVHIP_ERR_UNSUPPORTED; }
    if (c.channels < 0 || c.channels > 2) { err = "ResNetSE: channels selects the pooling, 0 / 2 = 'ASP' (mean | std), 1 = 'SAP' (mean)"; return SVHIP_ERR_INVALID; }
    if (!c.input_norm) { err = "ResNetSE applies InstanceNorm1d(n_mels): input_norm must be 1"; return SVHIP_ERR_INVALID; }
    if (c.embed_dim <= 0) { err = "ResNetSE needs embed_dim > 0"; return SVHIP_ERR_INVALID; }
    if (c.hop_length > 0 && c.samples / c.hop_length + 1 < 2) { err = "ResNetSE needs T >= 2 frames (InstanceNorm1d over one frame is undefined)"; return SVHIP_ERR_INVALID; }
    return SVHIP_OK;
}

void resnetse_spec(const svhip_config& c, WeightSpec& spec) {
    const RsArch& a = arch_of(c);
    spec["conv1.weight"] = {a.widths[0], 1, 3, 3}; spec["conv1.bias"] = {a.widths[0]};
    spec_bn(spec, "bn1", a.widths[0]);
    int inpl = a.widths[0];
    for (int s = 0; s < 4; ++s) {
        const int64_t C = a.widths[s];
        for (int j = 0; j < a.blocks[s]; ++j) {
            const std::string p = "layer" + std::to_string(s + 1) + "." + std::to_string(j) + ".";
            spec[p + "conv1.weight"] = {C, inpl, 3, 3}; spec_bn(spec, p + "bn1", C);
            spec[p + "conv2.weight"] = {C, C, 3, 3}; spec_bn(spec, p + "bn2", C);
            spec[p + "se.fc.0.weight"] = {a.se_hidden, C}; spec[p + "se.fc.0.bias"] = {a.se_hidden};
            spec[p + "se.fc.2.weight"] = {C, a.se_hidden}; spec[p + "se.fc.2.bias"] = {C};
            if (j == 0 && s > 0) { spec[p + "downsample.0.weight"] = {C, inpl, 1, 1}; spec_bn(spec, p + "downsample.1", C); }
            inpl = (int)C;
        }
    }
    const int64_t F = (int64_t)a.widths[3] * (c.n_mels / 8), nOut = c.embed_dim;
    spec["attention.0.weight"] = {a.att_dim, F, 1}; spec["attention.0.bias"] = {a.att_dim};
    spec_bn(spec, "attention.2", a.att_dim);
    spec["attention.3.weight"] = {F, a.att_dim, 1}; spec["attention.3.bias"] = {F};
    spec["fc.weight"] = {nOut, rs_is_sap(c) ? F : 2 * F}; spec["fc.bias"] = {nOut};
}

int resnetse_finalize(svhip_handle* h) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const RsArch& a = arch_of(c);
    int rc;
    {
        // stem: conv1 (32, 1, 3, 3) tap-major [3 dp + dq][32], bias, bn1
        const HostTensor* w;
        if ((rc = needw(h, "conv1.weight", w))) return rc;
        const int C0 = a.widths[0];
        std::vector<float> tw((size_t)9 * C0);
        for (int n = 0; n < C0; ++n)
            for (int dp = 0; dp < 3; ++dp)
                for (int dq = 0; dq < 3; ++dq) tw[(size_t)(dp * 3 + dq) * C0 + n] = w->data[(size_t)n * 9 + dq * 3 + dp];
        if ((rc = dev_upload(h, &s.stem_w, tw)) || (rc = upload_f32(h, "conv1.bias", &s.stem_b)) ||
            (rc = make_bn(h, "bn1", C0, &s.stem_scale, &s.stem_shift))) return rc;
    }
    double fl = 2.0 * 9 * a.widths[0] * s.P[0] * s.Q[0];
    s.blocks.clear();
    int inpl = a.widths[0];
    for (int sg = 0; sg < 4; ++sg) {
        const int C = a.widths[sg];
        const double pos = (double)s.P[sg + 1] * s.Q[sg + 1];
        for (int j = 0; j < a.blocks[sg]; ++j) {
            const std::string p = "layer" + std::to_string(sg + 1) + "." + std::to_string(j) + ".";
            RsBlock K;
            const int stride = (j == 0 && sg > 0) ? 2 : 1;
            if ((rc = make_rs_conv(h, K.c1, p + "conv1.weight", p + "bn1", inpl, C, 3, stride)) ||
                (rc = make_rs_conv(h, K.c2, p + "conv2.weight", p + "bn2", C, C, 3, 1))) return rc;
            K.has_down = j == 0 && sg > 0;
            if (K.has_down && (rc = make_rs_conv(h, K.down, p + "downsample.0.weight", p + "downsample.1", inpl, C, 1, 2))) return rc;
            if ((rc = upload_f32(h, p + "se.fc.0.weight", &K.se_w1)) || (rc = upload_f32(h, p + "se.fc.0.bias", &K.se_b1)) ||
                (rc = upload_f32(h, p + "se.fc.2.weight", &K.se_w2)) || (rc = upload_f32(h, p + "se.fc.2.bias", &K.se_b2))) return rc;
            fl += pos * (2.0 * 9 * inpl * C + 2.0 * 9 * C * C + (K.has_down ? 2.0 * inpl * C : 0.0));
            s.blocks.push_back(K);
            inpl = C;
        }
        s.stage_end[sg] = (int)s.blocks.size();
    }
    // The reference flattens (B, C, Q, P) to rows c Q + q; the channels-last rows here run q C + c.  The permutation goes once into the
    // K axis of attention.0 and fc and the N axis of attention.3, never into activations.
    const int C4 = a.widths[3], Q4 = s.Q[4], F = C4 * Q4, A = a.att_dim, nOut = c.embed_dim;
    auto perm = [&](int k) { return (k % C4) * Q4 + k / C4; };        // column q C + c of this layout -> the reference's c Q + q
    {
        const HostTensor *w, *b;
        if ((rc = needw(h, "attention.0.weight", w)) || (rc = needw(h, "attention.0.bias", b))) return rc;
        HostTensor pw; pw.shape = {A, F}; pw.data.resize((size_t)A * F);
        for (int n = 0; n < A; ++n)
            for (int k = 0; k < F; ++k) pw.data[(size_t)n * F + k] = w->data[(size_t)n * F + perm(k)];
        if ((rc = make_conv(h, s.att0, pw, &b->data, 1)) || (rc = make_bn(h, "attention.2", A, &s.att0.scale, &s.att0.shift))) return rc;
        if ((rc = needw(h, "attention.3.weight", w)) || (rc = needw(h, "attention.3.bias", b))) return rc;
        HostTensor pw3; pw3.shape = {F, A}; pw3.data.resize((size_t)F * A);
        std::vector<float> pb(F);
        for (int k = 0; k < F; ++k) {
            memcpy(&pw3.data[(size_t)k * A], &w->data[(size_t)perm(k) * A], (size_t)A * 4);
            pb[k] = b->data[perm(k)];
        }
        if ((rc = make_conv(h, s.att3, pw3, &pb, 1))) return rc;
        if ((rc = needw(h, "fc.weight", w))) return rc;
        const int halves = s.sap ? 1 : 2, K = halves * F;
        std::vector<float> fw((size_t)nOut * K);
        for (int n = 0; n < nOut; ++n)
            for (int hf = 0; hf < halves; ++hf)
                for (int k = 0; k < F; ++k) fw[(size_t)n * K + hf * F + k] = w->data[(size_t)n * K + hf * F + perm(k)];
        s.fc.N = nOut; s.fc.K = K;
        if ((rc = dev_upload(h, &s.fc.W, fw)) || (rc = upload_f32(h, "fc.bias", &s.fc.bias))) return rc;
    }
    fl += (double)s.P[4] * (s.att0.flops_per_row + s.att3.flops_per_row) + 2.0 * nOut * s.fc.K;
    h->flops_per_utt = fl;
    return SVHIP_OK;
}

int resnetse_alloc(svhip_handle* h) {
    h->model = std::make_unique<ResNetSEState>();
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const RsArch& a = arch_of(c);
    const size_t B = c.max_batch;
    s.sap = rs_is_sap(c);
    s.P[0] = h->T; s.Q[0] = c.n_mels; s.C[0] = a.widths[0];
    for (int sg = 0; sg < 4; ++sg) {
        const int st = sg == 0 ? 1 : 2;
        s.P[sg + 1] = rs_out_size(s.P[sg], st);
        s.Q[sg + 1] = rs_out_size(s.Q[sg], st);
        s.C[sg + 1] = a.widths[sg];
    }
    int rc;
    if ((rc = dev_alloc(h, &s.xin, B * s.P[0] * s.Q[0]))) return rc;
    size_t big = 0, part = 0;
    for (int sg = 0; sg <= 4; ++sg) {
        const size_t n = (size_t)s.P[sg] * s.Q[sg] * s.C[sg];
        if (n > big) big = n;
        if ((rc = actbuf(h, &s.out[sg], B * n))) return rc;
        if (sg > 0) {          // the SE tile sums of conv2 in this stage
            RsConvParams p;
            p.P = s.P[sg]; p.Q = s.Q[sg]; p.stride = 1; p.ks = 3;
            rs_conv_plan(p);
            const size_t m = (size_t)p.ntp * p.ntq * s.C[sg];
            if (m > part) part = m;
        }
    }
    for (int i = 0; i < 5; ++i) if ((rc = actbuf(h, &s.tmp[i], B * big))) return rc;
    if ((rc = dev_alloc(h, &s.part, B * part)) || (rc = dev_alloc(h, &s.gate, B * 256))) return rc;
    const size_t F = (size_t)s.C[4] * s.Q[4], M = B * s.P[4];
    if ((rc = actbuf(h, &s.att, M * a.att_dim)) || (rc = dev_alloc(h, &s.logits, M * F)) ||
        (rc = dev_alloc(h, &s.pool_raw, B * 2 * F)) || (rc = dev_alloc(h, &s.pool, B * 2 * F))) return rc;
    std::vector<float> one(2 * F, 1.0f), zero(2 * F, 0.0f);
    if ((rc = dev_upload(h, &s.pool_one, one)) || (rc = dev_upload(h, &s.pool_zero, zero))) return rc;
    return SVHIP_OK;
}

// ResNetSE.forward, written once for both forms.  pk null: a fixed-length batch of B utterances of h->T frames, (B, n_mels, T) at d_feat,
// on h->cur; the two attention convolutions take their routes through conv_gemm.  pk set: its n = B utterances as packed images
// (features at d_feat + pk->off[u]), on the handle's stream; lv[l] are the tables of frame level l, the convolutions read the tile
// tables built here, and the attention convolutions go to the generic kernel (launch_gemm_ragged: one kernel at every row count).  The
// helpers pick the form; below them the network reads once.
static int resnetse_walk(svhip_handle* h, const float* d_feat, int B, const RagPack* pk) {
    auto& s = S(h);
    const svhip_config& c = h->cfg;
    const Seg* g = pk ? pk->lv : nullptr;                 // g[l]: frame level l of the pack
    const int dt = h->dt, Bmax = c.max_batch;
    const bool bf = h->bf16;
    if (g) h->cur = h->stream;
    hipStream_t st = h->cur;
    int rc;
    // a pack: the tile tables of its ten kinds of convolution — counted on the host for the grids and the LDS, built on the device from
    // the row0 tables (the upload is already enqueued on this stream; nothing here waits for it)
    RsRagConv rk[RS_RAG_KINDS];
    if (g) {
        for (int l = 0; l < 4; ++l)
            if ((rc = run(h, "rag_rows", 0, [&]() { return launch_rag_rows(g[l].row0, B, g[l].maxT, g[l].utt, st); }))) return rc;
        for (int k = 0; k < RS_RAG_KINDS; ++k) {
            const RsRagKind kd = rs_rag_kind(k);
            RsRagConv& r = rk[k];
            int* tab = s.rag_tiles + (size_t)k * (2 * Bmax + 1);
            r.row0_in = g[kd.l_in].row0; r.row0_out = g[kd.l_out].row0; r.tile0 = tab; r.plan = tab + Bmax + 1; r.n = B;
            rs_rag_tiles_host(g[kd.l_in].hrow0, B, s.Q[kd.l_in + 1], kd.stride, kd.ks, &r.ntiles, &r.halo_bytes);
            if ((rc = run(h, "rs_rag_tiles", 0, [&]() {
                     return launch_rs_rag_tiles(r.row0_in, B, s.Q[kd.l_in + 1], kd.stride, kd.ks, tab, tab + Bmax + 1, st);
                 }))) return rc;
            if (r.ntiles <= 0 || (k < 4 && (size_t)r.ntiles * s.C[k + 1] > s.rag_part_floats))
                SV_FAIL(h, SVHIP_ERR_STATE, "ragged ResNetSE: %d tiles at level %d are over the bound of the SE tile sums", r.ntiles, k);
        }
    }
    float* part = g ? s.rag_part : s.part;
    // option rs_keep: what block i has just stored (i < 0: outside the blocks), copied on st.  `rows` x cols per utterance of a fixed-length
    // batch (`cap_rows` per utterance at most), or the `rag_rows` packed rows of a pack; utt_rows: one row per utterance
    ++s.keep.epoch;
    auto keep = [&](int i, const std::string& what, const void* src, size_t rows, size_t rag_rows, size_t cap_rows, int cols, bool f32 = false,
                    bool utt_rows = false) -> int {
        if (!h->opt.rs_keep) return SVHIP_OK;
        const std::string name = i < 0 ? "rs_" + what : "rs_b" + std::to_string(i) + "_" + what;
        const int kind = f32 ? KEEP_F32 : KEEP_DT;
        if (utt_rows) return keep_stage(h, s.keep, st, name, src, kind, g ? (size_t)B : 1, g != nullptr, (size_t)Bmax, cols, 0, (size_t)B, B);
        // (a pack of short utterances can have more tiles than max_batch fixed images: keep_stage grows the buffer then)
        return keep_stage(h, s.keep, st, name, src, kind, g ? rag_rows : rows, g != nullptr, std::max(rag_rows, (size_t)Bmax * cap_rows), cols, 0,
                          g ? rag_rows : (size_t)B * rows, B);
    };
    // an activation of level lv (0: the stem's image; 1 .. 4: a stage's) or of frame level lv - 1 of a pack
    auto keep_act = [&](int i, const std::string& what, const void* src, int lv) {
        const size_t q = s.Q[lv];
        return keep(i, what, src, (size_t)s.P[lv] * q, g ? (size_t)g[lv ? lv - 1 : 0].M * q : 0, (size_t)s.P[lv] * q, s.C[lv]);
    };
    // one convolution L of the block that writes level `lv` (= its stage), x -> y
    auto conv = [&](const char* label, const RsConv& L, const void* x, void* y, int P, int Q, int lv, bool relu_in, bool relu_out, float* pt,
                    RsConvParams& p) {
        p = rs_params(L, x, y, B, P, Q, relu_in, relu_out, pt);
        const double taps = L.ks * L.ks, pos = g ? (double)g[lv].M * p.Qo : (double)B * p.Po * p.Qo;
        return run(h, label, 2.0 * taps * L.cin * L.cout * pos, [&]() {
            return g ? launch_rs_conv_ragged(p, rk[rs_rag_kind_of(L, lv)], dt, st) : launch_rs_conv(p, dt, st);
        });
    };
    // log(x + 1e-6) - mean_t for features == 'melspectrogram', then InstanceNorm1d(n_mels) without affine: (B, n_mels, T) -> (B, T, n_mels) fp32
    // (a pack: rag_prologue's arithmetic is launch_prologue's over each utterance's own frames; the identity affine selects the norm)
    if (g) {
        if ((rc = run(h, "rag_prologue", 0, [&]() {
                 return launch_rag_prologue(d_feat, pk->off, g[0].row0, B, g[0].maxT, s.xin, false, c.n_mels, c.log_input, h->d_ones, h->d_zeros, h->d_pstats, st);
             }))) return rc;
    } else if ((rc = run(h, "prologue", 0, [&]() {
                    return launch_prologue(d_feat, s.xin, false, B, c.n_mels, h->T, c.log_input, h->d_ones, h->d_zeros, h->d_pstats, st);
                }))) return rc;
    if ((rc = keep(-1, "xin", s.xin, s.P[0], g ? (size_t)g[0].M : 0, s.P[0], s.Q[0], true))) return rc;
    // conv1 (with bias) -> ReLU -> bn1                                                       ResNetBaseline.py:260-262
    if ((rc = run(h, g ? "rs_stem_rag" : "rs_stem", 2.0 * 9 * s.C[0] * (g ? (double)g[0].M : (double)B * s.P[0]) * s.Q[0], [&]() {
             return g ? launch_rs_stem_ragged(s.xin, s.stem_w, s.stem_b, s.stem_scale, s.stem_shift, s.out[0], dt, g[0].row0, g[0].utt, g[0].M, s.Q[0], st)
                      : launch_rs_stem(s.xin, s.stem_w, s.stem_b, s.stem_scale, s.stem_shift, s.out[0], dt, B, s.P[0], s.Q[0], st);
         }))) return rc;
    const void* x = s.out[0];
    int P = s.P[0], Q = s.Q[0], stage = 0, pp = 0;      // (P: of the fixed form; a pack's frames are in its tables)
    static const char* const kConvLabel[4] = {"rs_conv3x3_s1", "rs_conv3x3_s2", "rs_conv3x3_s3", "rs_conv3x3_s4"};
    for (size_t i = 0; i < s.blocks.size(); ++i) {
        const RsBlock& K = s.blocks[i];
        while ((int)i >= s.stage_end[stage]) ++stage;
        const bool last = (int)i + 1 == s.stage_end[stage];
        void* out = last ? s.out[stage + 1] : s.tmp[pp];
        RsConvParams p1, p2, pd;
        const int bi = (int)i, lv = stage + 1;
        if ((rc = conv(kConvLabel[stage], K.c1, x, s.tmp[2], P, Q, stage, true, true, nullptr, p1)) || (rc = keep_act(bi, "conv1", s.tmp[2], lv))) return rc;
        if ((rc = conv(kConvLabel[stage], K.c2, s.tmp[2], s.tmp[3], p1.Po, p1.Qo, stage, false, false, part, p2)) ||
            (rc = keep_act(bi, "conv2", s.tmp[3], lv))) return rc;
        // the tile sums: ntp ntq rows per utterance, or the pack's tiles in pack order
        if ((rc = keep(bi, "part", part, (size_t)p2.ntp * p2.ntq, g ? (size_t)rk[stage].ntiles : 0, (size_t)p2.ntp * p2.ntq, K.c2.cout, true))) return rc;
        if ((rc = run(h, g ? "rs_se_gate_rag" : "rs_se_gate", 0, [&]() {
                 return g ? launch_rs_se_gate_ragged(part, rk[stage].tile0, g[stage].row0, B, K.c2.cout, p2.Qo, K.se_w1, K.se_b1, K.se_w2, K.se_b2, s.gate, st)
                          : launch_rs_se_gate(part, p2.ntp * p2.ntq, B, K.c2.cout, p2.Po * p2.Qo, K.se_w1, K.se_b1, K.se_w2, K.se_b2, s.gate, st);
             })) || (rc = keep(bi, "gate", s.gate, 1, 0, 1, K.c2.cout, true, true))) return rc;
        const void* res = x;
        if (K.has_down) {
            if ((rc = conv("rs_down", K.down, x, s.tmp[4], P, Q, stage, true, false, nullptr, pd)) || (rc = keep_act(bi, "down", s.tmp[4], lv))) return rc;
            res = s.tmp[4];
        }
        if ((rc = run(h, g ? "rs_se_apply_rag" : "rs_se_apply", 0, [&]() {
                 return g ? launch_rs_se_apply_ragged(s.tmp[3], res, s.gate, out, dt, g[stage].utt, g[stage].M, p2.Qo, K.c2.cout, !K.has_down, st)
                          : launch_rs_se_apply(s.tmp[3], res, s.gate, out, dt, B, p2.Po * p2.Qo, K.c2.cout, !K.has_down, st);
             })) || (rc = keep_act(bi, "out", out, lv))) return rc;
        x = out;
        P = p1.Po; Q = p1.Qo;
        if (!last) pp ^= 1;
    }
    // attention (ResNetBaseline.py:186-194,269-279) on rows (B P4, Q4 C4): Conv1d -> ReLU -> BN -> Conv1d -> softmax over frames, then the
    // weighted mean and sqrt(clamp(weighted variance, 1e-5)).  Both convolutions are 1 x 1: no tap crosses an utterance's edge
    const int F = s.C[4] * s.Q[4], M = g ? g[3].M : B * P, Tg = g ? 1 : P;
    auto gemm = [&](const ConvLayer& L, GemmParams p) {
        if (!g) return conv_gemm(h, L, p);
        p.rag_utt = g[3].utt; p.rag_row0 = g[3].row0;
        return run(h, "rag_gemm", (double)M * L.flops_per_row, [&]() { return launch_gemm_ragged(p, bf, st); });
    };
    GemmParams pa = conv_params(h, s.att0, x, F, s.att, 128, M, Tg);
    pa.act1 = ACT_RELU;
    if ((rc = gemm(s.att0, pa)) || (rc = keep(-1, "att", s.att, s.P[4], (size_t)M, s.P[4], 128))) return rc;
    GemmParams pl = conv_params(h, s.att3, s.att, 128, s.logits, F, M, Tg);
    pl.out_f32 = 1;
    if ((rc = gemm(s.att3, pl)) || (rc = keep(-1, "logits", s.logits, s.P[4], (size_t)M, s.P[4], F, true))) return rc;
    if ((rc = run(h, g ? "rag_asp_pool" : "rs_asp_pool", 0, [&]() {
             return g ? launch_rag_asp_pool(s.logits, x, bf, F, g[3].row0, B, F, s.pool_one, s.pool_zero, s.pool_raw, s.pool, 1e-5f, st)
                      : launch_asp_pool(s.logits, x, bf, F, B, P, F, s.pool_one, s.pool_zero, s.pool_raw, s.pool, 1e-5f, 0.0f, st);
         })) || (rc = keep(-1, "pool_raw", s.pool_raw, 1, 0, 1, 2 * F, true, true))) return rc;
    // an utterance with a non-finite input value gets a NaN embedding, as in the reference (the GEMM's ReLU epilogue would have dropped it):
    // its own row only
    if ((rc = run(h, "rs_in_check", 0, [&]() {
             return g ? launch_tn_nonfinite_rows_ragged(d_feat, pk->off, g[0].row0, c.n_mels, B, s.pool, 2 * F, 2 * F, st)
                      : launch_tn_nonfinite_rows(d_feat, (int64_t)c.n_mels * h->T, B, s.pool, 2 * F, 2 * F, st);
         }))) return rc;
    // fc; 'SAP' reads the weighted means only (K = F of the 2 F columns)
    return run(h, g ? "rag_fc" : "rs_fc", 2.0 * B * s.fc.N * s.fc.K, [&]() {
        return g ? launch_rag_linear(s.pool, 2 * F, s.fc.W, s.fc.bias, h->d_emb, c.embed_dim, B, c.embed_dim, s.fc.K, ACT_NONE, st)
                 : launch_rowvec_linear(s.pool, 2 * F, s.fc.W, s.fc.bias, h->d_emb, c.embed_dim, B, c.embed_dim, s.fc.K, ACT_NONE, st);
    });
}

static int resnetse_forward_part(svhip_handle* h, const float* d_feat, int, int B) { return resnetse_walk(h, d_feat, B, nullptr); }
int resnetse_forward(svhip_handle* h, const float* d_feat, int B) { return forward_lanes(h, resnetse_forward_part, d_feat, B, 1, B); }

// ---- ragged packs ------------------------------------------------------------------------------------------
// ResNetSE's rules for a pack (RaggedCheckFn; include/svhip.h), on the host alone.  An utterance counts as 8 ceil(T_u / 8) rows against
// max_batch T: then sum_u P_l,u <= max_batch P_l at every level, since P_l,u = ceil(T_u / 2^l) <= 8 ceil(T_u / 8) / 2^l (file header).
// T_u >= 2: InstanceNorm1d over one frame is the reference's own ValueError
int resnetse_ragged_check(const svhip_config& c, const int32_t* lengths, int n, bool is_wave, std::string& err) {
    return rag_mel_check(c, lengths, n, is_wave, err, true, "hop_length / max_batch / samples", 2, " (InstanceNorm1d over one frame is undefined)", nullptr,
                         0, 8);
}

// four frame levels: the mel frames (the stem, layer1), then what each stride-2 stage leaves
static void resnetse_rag_frames(const svhip_config& c, int64_t len, bool is_wave, int T[RAG_LEVELS]) {
    T[0] = (int)mel_frames(c, len, is_wave);
    for (int l = 1; l < 4; ++l) T[l] = rs_out_size(T[l - 1], 2);
}
static const RagRule kResnetseRag = {4, resnetse_rag_frames, true};

int resnetse_embed_ragged(svhip_handle* h, const float* in, bool in_host, bool is_wave, const int64_t* in_off, const int32_t* lengths, int n) {
    auto& s = S(h);
    const size_t B = h->cfg.max_batch;
    const size_t utt_cap[RAG_LEVELS] = {B * s.P[1], B * s.P[2], B * s.P[3], B * s.P[4]};
    RagPack pk;
    int rc;
    // the handle's first ragged call: the tile tables and the SE tile sums of a pack (rag_pack: the segment tables and the staging buffer)
    if (!s.rag_tiles && (rc = dev_alloc(h, &s.rag_tiles, (size_t)RS_RAG_KINDS * (2 * B + 1)))) return rc;
    if (!s.rag_part) {
        s.rag_part_floats = rs_rag_part_floats(s, B * h->T);
        if ((rc = dev_alloc(h, &s.rag_part, s.rag_part_floats))) return rc;
    }
    if ((rc = rag_pack(h, s.rag, kResnetseRag, utt_cap, in, in_host, is_wave, in_off, lengths, n, pk)) || (rc = resnetse_walk(h, pk.in, n, &pk))) return rc;
    set_rag_rows(h, pk);
    return SVHIP_OK;
}

// the stages of option rs_keep: rs_xin, rs_att, rs_logits, rs_pool_raw, rs_b<block>_conv1 | _conv2 | _part | _gate | _down | _out
static bool rs_keep_name(const std::string& n) {
    if (n == "rs_xin" || n == "rs_att" || n == "rs_logits" || n == "rs_pool_raw") return true;
    if (n.compare(0, 4, "rs_b") != 0) return false;
    size_t i = 4;
    while (i < n.size() && n[i] >= '0' && n[i] <= '9') ++i;
    if (i == 4 || i > 6 || i >= n.size() || n[i] != '_') return false;
    const std::string w = n.substr(i + 1);
    for (const char* q : {"conv1", "conv2", "part", "gate", "down", "out"}) if (w == q) return true;
    return false;
}

// rs_stem, rs_layer1 .. rs_layer4 (B P Q, C), rs_pool (B, 2 F); after a ragged forward the packed rows (sum_u P_l,u Q_l, C_l) in utterance order;
// option rs_keep's
int resnetse_stage(svhip_handle* h, const std::string& n, bool, StageView& v) {
    auto& s = S(h);
    int sg = -1;
    if (n == "rs_stem") sg = 0;
    else if (n.size() == 9 && n.compare(0, 8, "rs_layer") == 0 && n[8] >= '1' && n[8] <= '4') sg = n[8] - '0';
    if (sg >= 0) {
        const size_t frames = h->rag_levels ? (size_t)h->rag_rows[sg ? sg - 1 : 0] : (size_t)h->lastB * s.P[sg];
        v.src = s.out[sg]; v.rows = frames * s.Q[sg]; v.cols = v.ld = s.C[sg];
    }
    else if (n == "rs_pool") { v.src = s.pool; v.rows = h->lastB; v.cols = v.ld = 2 * (size_t)s.C[4] * s.Q[4]; v.f32 = true; }
    else if (rs_keep_name(n)) return kept_view(h, s.keep, n, h->lastB, "rs_keep", h->opt.rs_keep != 0, v);
    else return unknown_stage(h, n);
    return SVHIP_OK;
}

}  // namespace svhip

// The 3 x 3 convolution kernel on its own (tests): x (B, P, Q, Cin) and y (B, Po, Qo, Cout) are device pointers in the compute type, scale /
// shift device fp32 [Cout]; w is the HOST weight (Cout, Cin, 3, 3) in the reference's layout, packed and uploaded here.  Synchronises.
extern "C" int svhip_resnetse_conv3x3(const void* x, const float* w, const float* scale, const float* shift, void* y, int32_t compute, int32_t B,
                                      int32_t P, int32_t Q, int32_t Cin, int32_t Cout, int32_t stride, int32_t relu_in, int32_t relu_out, void* stream) {
    using namespace svhip;
    if ((compute != SVHIP_F32 && compute != SVHIP_BF16) || !x || !w || !scale || !shift || !y) return SVHIP_ERR_INVALID;
    if (B <= 0 || P <= 0 || Q <= 0 || Cin <= 0 || Cin % 32 != 0 || Cout <= 0 || (stride != 1 && stride != 2)) return SVHIP_ERR_INVALID;
    const bool bf = compute == SVHIP_BF16;
    const std::vector<float> packed = rs_pack(w, Cout, Cin, 3, bf ? 32 : 16);
    std::vector<uint16_t> pb;
    if (bf) {
        pb.resize(packed.size());
        for (size_t i = 0; i < packed.size(); ++i) pb[i] = f32_to_bf16_rne(packed[i]);
    }
    void* dW = nullptr;
    const size_t bytes = packed.size() * (bf ? 2 : 4);
    if (hipMalloc(&dW, bytes) != hipSuccess) return SVHIP_ERR_NOMEM;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpy(dW, bf ? (const void*)pb.data() : (const void*)packed.data(), bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        RsConvParams p;
        p.X = x; p.Y = y; p.W = dW; p.scale = scale; p.shift = shift;
        p.B = B; p.P = P; p.Q = Q; p.Cin = Cin; p.Cout = Cout; p.stride = stride; p.ks = 3; p.relu_in = relu_in != 0; p.relu_out = relu_out != 0;
        rs_conv_plan(p);
        e = launch_rs_conv(p, bf ? DT_BF16 : DT_F32, st);
        if (e == hipErrorInvalidValue) { (void)hipFree(dW); return SVHIP_ERR_INVALID; }
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipFree(dW);
    return (e == hipSuccess && e2 == hipSuccess) ? SVHIP_OK : SVHIP_ERR_HIP;
}

// The same kernel over a pack (tests): n utterances, utterance u a (P_host[u], Q, Cin) image, the images back to back in x and (Po_u, Qo,
// Cout) back to back in y.  Builds and uploads the row0 tables of the two levels, builds the tile tables on the device, launches the packed
// kernel and synchronises.
extern "C" int svhip_resnetse_conv3x3_ragged(const void* x, const float* w, const float* scale, const float* shift, void* y, int32_t compute,
                                             const int32_t* P_host, int32_t n, int32_t Q, int32_t Cin, int32_t Cout, int32_t stride, int32_t relu_in,
                                             int32_t relu_out, void* stream) {
    using namespace svhip;
    if ((compute != SVHIP_F32 && compute != SVHIP_BF16) || !x || !w || !scale || !shift || !y || !P_host) return SVHIP_ERR_INVALID;
    if (n <= 0 || Q <= 0 || Cin <= 0 || Cin % 32 != 0 || Cout <= 0 || (stride != 1 && stride != 2)) return SVHIP_ERR_INVALID;
    std::vector<int> tab(2 * (size_t)(n + 1), 0);          // row0 of the input level | row0 of the output level
    for (int u = 0; u < n; ++u) {
        if (P_host[u] <= 0 || (int64_t)tab[u] + P_host[u] > 0x7fffffffLL / Q) return SVHIP_ERR_INVALID;
        tab[u + 1] = tab[u] + P_host[u];
        tab[n + 1 + u + 1] = tab[n + 1 + u] + rs_out_size(P_host[u], stride);
    }
    const bool bf = compute == SVHIP_BF16;
    const std::vector<float> packed = rs_pack(w, Cout, Cin, 3, bf ? 32 : 16);
    std::vector<uint16_t> pb;
    if (bf) {
        pb.resize(packed.size());
        for (size_t i = 0; i < packed.size(); ++i) pb[i] = f32_to_bf16_rne(packed[i]);
    }
    void* dW = nullptr;
    int* dT = nullptr;                                     // the two row0 tables, then tile0 (n + 1) and plan (n)
    const size_t bytes = packed.size() * (bf ? 2 : 4), tints = 4 * (size_t)(n + 1);
    if (hipMalloc(&dW, bytes) != hipSuccess) return SVHIP_ERR_NOMEM;
    if (hipMalloc((void**)&dT, tints * 4) != hipSuccess) { (void)hipFree(dW); return SVHIP_ERR_NOMEM; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpy(dW, bf ? (const void*)pb.data() : (const void*)packed.data(), bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dT, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        RsRagConv r;
        r.row0_in = dT; r.row0_out = dT + (n + 1); r.tile0 = dT + 2 * (n + 1); r.plan = dT + 3 * (n + 1); r.n = n;
        rs_rag_tiles_host(tab.data(), n, Q, stride, 3, &r.ntiles, &r.halo_bytes);
        RsConvParams p;
        p.X = x; p.Y = y; p.W = dW; p.scale = scale; p.shift = shift;
        p.B = n; p.Q = Q; p.Cin = Cin; p.Cout = Cout; p.stride = stride; p.ks = 3; p.relu_in = relu_in != 0; p.relu_out = relu_out != 0;
        e = launch_rs_rag_tiles(r.row0_in, n, Q, stride, 3, dT + 2 * (n + 1), dT + 3 * (n + 1), st);
        if (e == hipSuccess) e = launch_rs_conv_ragged(p, r, bf ? DT_BF16 : DT_F32, st);
        if (e == hipErrorInvalidValue) { (void)hipFree(dW); (void)hipFree(dT); return SVHIP_ERR_INVALID; }
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipFree(dW);
    (void)hipFree(dT);
    return (e == hipSuccess && e2 == hipSuccess) ? SVHIP_OK : SVHIP_ERR_HIP;
}
