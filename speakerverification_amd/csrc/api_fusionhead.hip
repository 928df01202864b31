// api_fusionhead.hip — the attention head of Raw_ECAPA_hype in libsvhip (SVHIP_MODEL_FUSION_HEAD): its create rules, weight names and
// packing, staging buffer and forward (one launch of fusion_head.hip).  A handle of this kind has no waveform model; svhip_fusion_head
// (api.hip) is its one entry.
#include "handle.h"

namespace svhip {

namespace {

constexpr int C = HYPE_HEAD_C, A = HYPE_HEAD_A;

struct FusionHeadState : ModelState {
    float *s0 = nullptr, *t0 = nullptr;            // bn_before_agg
    float *W0t = nullptr, *b0 = nullptr;           // attention.0, [C][A]
    float *s2 = nullptr, *t2 = nullptr;            // attention.2
    float *W3t = nullptr, *b3 = nullptr;           // attention.3, [A][C]
    float *sF = nullptr, *tF = nullptr;            // bn_final
    float *Wft = nullptr, *bf = nullptr;           // fc, [2 C][nOutP]
    int nOutP = 0;
    float* stage = nullptr;                        // (max_batch, C): host-pointer inputs, e1's rows then e2's
};

FusionHeadState& S(svhip_handle* h) { return static_cast<FusionHeadState&>(*h->model); }

// (N, K[, 1]) -> [K][Np], the rows padded with zeros
int upload_transposed(svhip_handle* h, const std::string& name, int N, int K, int Np, float** dst) {
    const HostTensor* w;
    if (int rc = needw(h, name, w)) return rc;
    std::vector<float> t((size_t)K * Np, 0.0f);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) t[(size_t)k * Np + n] = w->data[(size_t)n * K + k];
    return dev_upload(h, dst, t);
}

}  // namespace

int fusion_head_check(const svhip_config& c, const char*& err) {
    if (c.channels != C) { err = "the fusion head mixes 704 channels (192 ECAPA-TDNN + 512 RawNet2): channels must be 704"; return SVHIP_ERR_INVALID; }
    if (c.embed_dim < 1) { err = "the fusion head needs embed_dim (nOut) >= 1"; return SVHIP_ERR_INVALID; }
    return SVHIP_OK;
}

void fusion_head_spec(const svhip_config& c, WeightSpec& spec) {       // Raw_ECAPA_hype.py:34-44
    spec_bn(spec, "bn_before_agg", C);
    spec["attention.0.weight"] = {A, C, 1}; spec["attention.0.bias"] = {A};
    spec_bn(spec, "attention.2", A);
    spec["attention.3.weight"] = {C, A, 1}; spec["attention.3.bias"] = {C};
    spec_bn(spec, "bn_final", 2 * C);
    spec["fc.weight"] = {(int64_t)c.embed_dim, 2 * C}; spec["fc.bias"] = {(int64_t)c.embed_dim};
}

int fusion_head_alloc(svhip_handle* h) {
    h->model = std::make_unique<FusionHeadState>();
    return dev_alloc(h, &S(h).stage, (size_t)h->cfg.max_batch * C);
}

int fusion_head_finalize(svhip_handle* h) {
    auto& s = S(h);
    const int nOut = h->cfg.embed_dim;
    s.nOutP = round_up(nOut, 4);
    int rc;
    if ((rc = make_bn(h, "bn_before_agg", C, &s.s0, &s.t0)) || (rc = make_bn(h, "attention.2", A, &s.s2, &s.t2)) ||
        (rc = make_bn(h, "bn_final", 2 * C, &s.sF, &s.tF)))
        return rc;
    if ((rc = upload_transposed(h, "attention.0.weight", A, C, A, &s.W0t)) || (rc = upload_f32(h, "attention.0.bias", &s.b0)) ||
        (rc = upload_transposed(h, "attention.3.weight", C, A, C, &s.W3t)) || (rc = upload_f32(h, "attention.3.bias", &s.b3)) ||
        (rc = upload_transposed(h, "fc.weight", nOut, 2 * C, s.nOutP, &s.Wft)) || (rc = upload_f32(h, "fc.bias", &s.bf)))
        return rc;
    h->flops_per_utt = 2.0 * (2.0 * A * C + 2.0 * C * nOut);
    return SVHIP_OK;
}

// e1 (B, d1) | e2 (B, d2) -> d_out (B, nOut), a device pointer; the inputs are device pointers or, with in_host, host arrays staged
// through the handle's buffer on its stream
int fusion_head_forward(svhip_handle* h, const float* e1, int d1, const float* e2, int d2, int B, bool in_host, float* d_out) {
    auto& s = S(h);
    if (in_host) {
        SV_HIP(h, hipMemcpyAsync(s.stage, e1, (size_t)B * d1 * 4, hipMemcpyHostToDevice, h->stream));
        SV_HIP(h, hipMemcpyAsync(s.stage + (size_t)B * d1, e2, (size_t)B * d2 * 4, hipMemcpyHostToDevice, h->stream));
        e1 = s.stage;
        e2 = s.stage + (size_t)B * d1;
    }
    HypeHeadParams p{e1, e2, d1, d2, B, h->cfg.embed_dim, s.nOutP, s.s0, s.t0, s.W0t, s.b0, s.s2, s.t2, s.W3t, s.b3, s.sF, s.tF, s.Wft, s.bf,
                     d_out, h->d_status, h->host_flag_dev};
    h->cur = h->stream;
    return run(h, "hype_head", B * h->flops_per_utt, [&]() { return launch_hype_head(p, h->stream); });
}

}  // namespace svhip
