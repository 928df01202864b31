// api_scoring.hip — what the scoring entry points of libsvhip share on the host (scoring_host.h: scratch slots, staging and the ending of
// a call, the dense score GEMM and its routes, the slab walk) and the simple calls: l2norm, pair and trial scores, mean_crops and the dense
// score matrix (see include/svhip.h).  AS-norm statistics: api_asnorm.hip; the search calls: api_search.hip; the dataset audit:
// api_audit.hip; the verification metrics: api_metrics.hip.
#include <string>

#include "scoring_host.h"

using namespace svhip;

namespace svhip {

int scratch(svhip_handle* h, int slot, size_t bytes, void** out) {
    if (h->scr_cap[slot] < bytes || !h->scr[slot]) {
        if (h->scr[slot]) { SV_HIP(h, hipStreamSynchronize(h->stream)); if (h->aux_stream) SV_HIP(h, hipStreamSynchronize(h->aux_stream)); (void)hipFree(h->scr[slot]); h->scr[slot] = nullptr; h->scr_cap[slot] = 0; }
        const size_t cap = std::max<size_t>(bytes + bytes / 2, 256);
        if (hipMalloc(&h->scr[slot], cap) != hipSuccess) {
            if (hipMalloc(&h->scr[slot], std::max<size_t>(bytes, 256)) != hipSuccess) { h->scr[slot] = nullptr; SV_FAIL(h, SVHIP_ERR_NOMEM, "scratch slot %d: %zu bytes", slot, bytes); }
            h->scr_cap[slot] = std::max<size_t>(bytes, 256);
        } else {
            h->scr_cap[slot] = cap;
        }
    }
    *out = h->scr[slot];
    return SVHIP_OK;
}
// Scratch retention policy: the slab of the AS-norm / top-k slab paths (up to 2 GiB), the top-k lists and the staging copies of HOST-pointer calls
// (N x D x 4 bytes for the embedding matrix) are released at the end of the call once they exceed 256 MiB — they would otherwise sit
// beside the model engines' workspaces for the life of the process-wide scoring handle.  The slots of the device-resident fast path
// (candidate lists, cohort planes: re-used every call) stay; svhip_trim_scratch frees everything.
void release_big_scratch(svhip_handle* h, bool staged_host) {
    const size_t cap = (size_t)256 << 20;
    auto drop = [&](int slot) {
        if (h->scr[slot] && h->scr_cap[slot] > cap) {
            (void)hipStreamSynchronize(h->stream);
            if (h->aux_stream) (void)hipStreamSynchronize(h->aux_stream);
            (void)hipFree(h->scr[slot]);
            h->scr[slot] = nullptr; h->scr_cap[slot] = 0;
        }
    };
    drop(svhip_handle::SCR_SLAB);
    drop(svhip_handle::SCR_TOPK);
    drop(svhip_handle::SCR_COEF);
    if (staged_host)
        for (int s_ : {svhip_handle::SCR_IN0, svhip_handle::SCR_IN1, svhip_handle::SCR_IN2, svhip_handle::SCR_IN3, svhip_handle::SCR_IN4,
                       svhip_handle::SCR_IN5, svhip_handle::SCR_IN6, svhip_handle::SCR_IN7, svhip_handle::SCR_OUT0, svhip_handle::SCR_OUT1, svhip_handle::SCR_OUT2, svhip_handle::SCR_SPLIT}) drop(s_);
}

static int select_device(svhip_handle* h) {
    SV_HIP(h, hipSetDevice(h->cfg.device));
    return SVHIP_OK;
}
Staged::Staged(svhip_handle* hh, int32_t flags)
    : h(hh), din(flags & SVHIP_IN_DEVICE), dout(flags & SVHIP_OUT_DEVICE), async(flags & SVHIP_ASYNC), rc(select_device(hh)) {}

int Staged::stage(int slot, size_t bytes, const void* host_src, void** dev) {
    if (int e = scratch(h, slot, bytes, dev)) return e;
    if (host_src) SV_HIP(h, hipMemcpyAsync(*dev, host_src, bytes, hipMemcpyHostToDevice, h->stream));
    return SVHIP_OK;
}

int Staged::finish(const char* name, int res, bool release) {
    if (!dout)
        for (int i = 0; i < n_outs && !res; ++i) {
            const hipError_t e = hipMemcpyAsync(outs[i].host, outs[i].dev, outs[i].bytes, hipMemcpyDeviceToHost, h->stream);
            if (e != hipSuccess) { h->err = std::string(name) + ": copy of the results failed: " + hipGetErrorString(e); res = SVHIP_ERR_HIP; }
        }
    if (res || !(din && dout && async)) {
        const hipError_t e = hipStreamSynchronize(h->stream);
        if (!res && e != hipSuccess) { h->err = std::string(name) + ": " + hipGetErrorString(e); res = SVHIP_ERR_HIP; }
        if (release) release_big_scratch(h, !din || !dout);
    }
    return res;
}

ScoreRoute score_route(const svhip_handle* h, const float* dA, int64_t Na, const float* dB, int64_t Nb, int D) {
    if (h->opt.score_f32mfma && !h->x3) return SCORE_F32MFMA;
    if (!h->opt.score_tiled && score_h3w_supported(D, Na, Nb) && aligned16(dA, dB)) return SCORE_H3W;
    return SCORE_WORDS;
}

int score_gemm(svhip_handle* h, const char* label, const float* dA, int64_t Na, const float* dB, int64_t Nb, int D, float* dO, int64_t ldo,
               ScoreRoute route, const void* dBsplit) {
    if (D % 32 != 0) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "embedding dim %d must be a multiple of 32", D);
    if (Na > (1 << 30) / 1 || Nb > (1 << 30)) SV_FAIL(h, SVHIP_ERR_INVALID, "matrix too large");
    hipStream_t st = h->stream;
    if (route == SCORE_H3W) {
        if (!dBsplit || !aligned16(dA)) SV_FAIL(h, SVHIP_ERR_STATE, "score route: the row-streaming kernel was chosen without its plane scratch");
        return run(h, label, 2.0 * Na * Nb * D, [&]() { return launch_score_h3w(dA, Na, dB, Nb, D, dO, ldo, const_cast<void*>(dBsplit), h->num_cu, st); });
    }
    GemmParams p;
    p.A = dA; p.W = dB; p.Y = dO;
    p.M = (int)Na; p.N = (int)Nb; p.K = D; p.Kp = D; p.Wrows = (int)Nb;
    p.lda = D; p.ldy = (int)ldo; p.T = 1;
    if (route == SCORE_WORDS && dBsplit && gemm_pw_supported(p, false)) { p.W = dBsplit; p.x3 = 1; }      // (the words exist: split_b ran launch_split_words)
    return run(h, label, 2.0 * Na * Nb * D, [&]() { return launch_gemm(p, false, st); });
}

int split_b(svhip_handle* h, ScoreRoute route, const float* dB, int64_t Nb, int D, void** out) {
    *out = nullptr;
    if (route == SCORE_F32MFMA) return SVHIP_OK;
    if (int rc = scratch(h, svhip_handle::SCR_SPLIT, std::max((size_t)Nb * D * 4, score_h3w_planes_bytes(D, Nb)), out)) return rc;
    if (route == SCORE_H3W) return SVHIP_OK;
    return run(h, "split_words", 0, [&]() { return launch_split_words(dB, *out, Nb * D, h->stream); });
}

int SlabWalk::open(const char* name) {
    ldk = (M + 3) & ~(int64_t)3;                                  // row stride of the slab (16-byte rows for the DMA GEMM)
    const int64_t max_m = (((int64_t)1 << 31) / (128 * 4)) & ~(int64_t)3;
    if (name && ldk > max_m)
        SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "%s: D = %d takes the slab route, whose 128-row slab holds at most M = %lld gallery rows (M = %lld)", name, D,
                (long long)max_m, (long long)M);
    slab_rows = std::min<int64_t>(N, std::max<int64_t>(128, ((int64_t)1 << 31) / (ldk * 4)));
    route = score_route(h, dA, slab_rows, dB, M, D);              // (every slab starts r0 * D * 4 bytes into A: the same alignment)
    if (int rc = split_b(h, route, dB, M, D, &bsplit)) return rc;
    return scratch(h, svhip_handle::SCR_SLAB, (size_t)slab_rows * ldk * 4, &slab);
}

int SlabWalk::pass(const char* label, bool gemm, const std::function<int(int64_t, int64_t, const float*, int64_t)>& rows_fn) {
    for (int64_t r0 = 0; r0 < N; r0 += slab_rows) {
        const int64_t rows = std::min(slab_rows, N - r0);
        if (gemm)
            if (int rc = score_gemm(h, label, dA + r0 * D, rows, dB, M, D, (float*)slab, ldk, route, bsplit)) return rc;
        if (int rc = rows_fn(r0, rows, (const float*)slab, ldk)) return rc;
    }
    return SVHIP_OK;
}

}  // namespace svhip

extern "C" {

int svhip_l2norm(svhip_handle* h, float* E, int64_t N, int32_t D, int32_t flags) {
    if (!h || !E || N < 0 || D <= 0) return SVHIP_ERR_INVALID;
    // in place: SVHIP_IN_DEVICE says where E is, as the input and as the output (staged through one slot: out() finds in()'s copy there)
    Staged s(h, (flags & SVHIP_IN_DEVICE) ? flags | SVHIP_OUT_DEVICE : flags & ~SVHIP_OUT_DEVICE);
    s.in(svhip_handle::SCR_IN0, E, (size_t)N * D * 4);
    float* de = s.out(svhip_handle::SCR_IN0, E, (size_t)N * D * 4);
    if (s.rc) return s.rc;
    return s.finish("l2norm", run(h, "l2norm", 0, [&]() { return launch_l2norm(de, N, D, h->stream); }), false);
}

static int pairs_common(svhip_handle* h, int mode, const float* E, int64_t N, int32_t D, const float* mu, const float* sigma,
                        const int32_t* ia, const int32_t* ib, int64_t P, float* out, int32_t flags) {
    if (!h || !E || !ia || !ib || !out || N <= 0 || D <= 0 || P < 0) return SVHIP_ERR_INVALID;
    if (mode == 1 && (!mu || !sigma)) return SVHIP_ERR_INVALID;
    Staged s(h, flags);
    if (!s.din) {   // host indices are range-checked before they reach the GPU
        for (int64_t p = 0; p < P; ++p)
            if (ia[p] < 0 || ia[p] >= N || ib[p] < 0 || ib[p] >= N) SV_FAIL(h, SVHIP_ERR_INVALID, "pair %lld indexes outside [0, %lld)", (long long)p, (long long)N);
    }
    const float* dE = s.in(svhip_handle::SCR_IN0, E, (size_t)N * D * 4);
    const int32_t* dA = s.in(svhip_handle::SCR_IN1, ia, (size_t)P * 4);
    const int32_t* dB = s.in(svhip_handle::SCR_IN2, ib, (size_t)P * 4);
    const float* dM = mode == 1 ? s.in(svhip_handle::SCR_IN3, mu, (size_t)N * 4) : nullptr;
    const float* dS = mode == 1 ? s.in(svhip_handle::SCR_IN4, sigma, (size_t)N * 4) : nullptr;
    float* dO = s.out(svhip_handle::SCR_OUT0, out, (size_t)P * 4);
    if (s.rc) return s.rc;
    if (mode == 0)
        return s.finish("score_pairs", run(h, "score_pairs", 2.0 * P * D, [&]() { return launch_score_pairs(dE, D, dA, dB, P, dO, h->stream); }), false);
    return s.finish("asnorm_pairs", run(h, "asnorm_pairs", 2.0 * P * D, [&]() { return launch_asnorm_pairs(dE, D, dM, dS, dA, dB, P, dO, h->stream); }), false);
}

int svhip_score_pairs(svhip_handle* h, const float* E, int64_t N, int32_t D, const int32_t* ia, const int32_t* ib, int64_t P,
                      float* out, int32_t flags) {
    return pairs_common(h, 0, E, N, D, nullptr, nullptr, ia, ib, P, out, flags);
}

int svhip_asnorm_pairs(svhip_handle* h, const float* E, int64_t N, int32_t D, const float* mu, const float* sigma,
                       const int32_t* ia, const int32_t* ib, int64_t P, float* out, int32_t flags) {
    return pairs_common(h, 1, E, N, D, mu, sigma, ia, ib, P, out, flags);
}

static int score_trials_impl(svhip_handle* h, int32_t mode, float pexp, const float* F, int64_t n_files, int32_t n_crops, int32_t D, const int32_t* ia,
                       const int32_t* ib, int64_t P, float* out, int32_t flags) {
    if (!h || !F || !ia || !ib || !out || n_files <= 0 || n_crops <= 0 || D <= 0 || P < 0) return SVHIP_ERR_INVALID;
    if (mode < SVHIP_TRIAL_COSINE || mode > SVHIP_TRIAL_PDIST) SV_FAIL(h, SVHIP_ERR_INVALID, "unknown trial scoring mode %d", mode);
    Staged s(h, flags);
    if (!s.din)
        for (int64_t p = 0; p < P; ++p)
            if (ia[p] < 0 || ia[p] >= n_files || ib[p] < 0 || ib[p] >= n_files) SV_FAIL(h, SVHIP_ERR_INVALID, "trial %lld indexes outside [0, %lld)", (long long)p, (long long)n_files);
    const float* dF = s.in(svhip_handle::SCR_IN0, F, (size_t)n_files * n_crops * D * 4);
    const int32_t* dA = s.in(svhip_handle::SCR_IN1, ia, (size_t)P * 4);
    const int32_t* dB = s.in(svhip_handle::SCR_IN2, ib, (size_t)P * 4);
    float* dO = s.out(svhip_handle::SCR_OUT0, out, (size_t)P * 4);
    if (s.rc) return s.rc;
    const int rc = run(h, "score_trials", 2.0 * P * n_crops * D, [&]() { return launch_trial_crops(mode, pexp, dF, n_crops, D, dA, dB, P, dO, h->stream); });
    return s.finish("score_trials", rc, false);
}

int svhip_score_trials(svhip_handle* h, int32_t mode, const float* F, int64_t n_files, int32_t n_crops, int32_t D, const int32_t* ia,
                       const int32_t* ib, int64_t P, float* out, int32_t flags) {
    return score_trials_impl(h, mode, 2.0f, F, n_files, n_crops, D, ia, ib, P, out, flags);
}

int svhip_score_trials_pnorm(svhip_handle* h, float p, const float* F, int64_t n_files, int32_t n_crops, int32_t D, const int32_t* ia,
                             const int32_t* ib, int64_t P, float* out, int32_t flags) {
    if (h && p != p) SV_FAIL(h, SVHIP_ERR_INVALID, "pnorm: p is NaN");
    return score_trials_impl(h, SVHIP_TRIAL_PNORM, p, F, n_files, n_crops, D, ia, ib, P, out, flags);
}

int svhip_mean_crops(svhip_handle* h, const float* F, int64_t n_files, int32_t n_crops, int32_t D, float* out, int32_t flags) {
    if (!h || !F || !out || n_files <= 0 || n_crops <= 0 || D <= 0) return SVHIP_ERR_INVALID;
    Staged s(h, flags);
    const float* dF = s.in(svhip_handle::SCR_IN0, F, (size_t)n_files * n_crops * D * 4);
    float* dO = s.out(svhip_handle::SCR_OUT0, out, (size_t)n_files * D * 4);
    if (s.rc) return s.rc;
    return s.finish("mean_crops", run(h, "mean_crops", 0, [&]() { return launch_mean_crops(dF, n_files, n_crops, D, dO, h->stream); }), false);
}

int svhip_score_matrix(svhip_handle* h, const float* A, int64_t Na, const float* B, int64_t Nb, int32_t D, float* out, int32_t flags) {
    if (!h || !A || !B || !out || Na <= 0 || Nb <= 0 || D <= 0) return SVHIP_ERR_INVALID;
    if (D % 32 != 0) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "score_matrix: embedding dim %d must be a multiple of 32", (int)D);      // before any copy or launch
    Staged s(h, flags);
    const float* dA = s.in(svhip_handle::SCR_IN0, A, (size_t)Na * D * 4);
    const float* dB = s.in(svhip_handle::SCR_IN1, B, (size_t)Nb * D * 4);
    float* dO = s.out(svhip_handle::SCR_OUT0, out, (size_t)Na * Nb * 4);
    if (s.rc) return s.rc;
    void* bsplit = nullptr;
    const ScoreRoute route = score_route(h, dA, Na, dB, Nb, D);
    if (int rc = split_b(h, route, dB, Nb, D, &bsplit)) return rc;
    return s.finish("score_matrix", score_gemm(h, "score_matrix", dA, Na, dB, Nb, D, dO, Nb, route, bsplit), false);
}

}  // extern "C"
