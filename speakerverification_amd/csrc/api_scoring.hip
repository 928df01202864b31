// api_scoring.hip — scoring, AS-norm and verification metrics entry points of libsvhip (see include/svhip.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "handle.h"

using namespace svhip;

extern "C" {

// ---- scoring ------------------------------------------------------------------------------------------
namespace {
// a scratch slot of at least `bytes` (grown by half again; the old block is freed only after the stream has drained)
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
                       svhip_handle::SCR_IN5, svhip_handle::SCR_OUT0, svhip_handle::SCR_OUT1, svhip_handle::SCR_OUT2, svhip_handle::SCR_SPLIT}) drop(s_);
}
struct TempBuf {      // device staging for host-pointer calls, in a scratch slot of the handle
    svhip_handle* h; int slot;
    int in(const void* src, size_t bytes, bool is_dev, const void** out) {
        if (is_dev) { *out = src; return SVHIP_OK; }
        void* d;
        if (int rc = scratch(h, slot, bytes, &d)) return rc;
        SV_HIP(h, hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, h->stream));
        *out = d;
        return SVHIP_OK;
    }
    int out(void* dst, size_t bytes, bool is_dev, void** o) {
        if (is_dev) { *o = dst; return SVHIP_OK; }
        return scratch(h, slot, bytes, o);
    }
};
}  // namespace

int svhip_l2norm(svhip_handle* h, float* E, int64_t N, int32_t D, int32_t flags) {
    if (!h || !E || N < 0 || D <= 0) return SVHIP_ERR_INVALID;
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const bool dev = flags & SVHIP_IN_DEVICE;
    TempBuf t{h, svhip_handle::SCR_IN0};
    const void* d;
    int rc = t.in(E, (size_t)N * D * 4, dev, &d);
    if (rc) return rc;
    float* de = const_cast<float*>(reinterpret_cast<const float*>(d));
    if ((rc = run(h, "l2norm", 0, [&]() { return launch_l2norm(de, N, D, h->stream); }))) return rc;
    if (!dev) SV_HIP(h, hipMemcpyAsync(E, de, (size_t)N * D * 4, hipMemcpyDeviceToHost, h->stream));
    if (!dev || !(flags & SVHIP_ASYNC)) SV_HIP(h, hipStreamSynchronize(h->stream));
    return SVHIP_OK;
}

static int pairs_common(svhip_handle* h, int mode, const float* E, int64_t N, int32_t D, const float* mu, const float* sigma,
                        const int32_t* ia, const int32_t* ib, int64_t P, float* out, int32_t flags) {
    if (!h || !E || !ia || !ib || !out || N <= 0 || D <= 0 || P < 0) return SVHIP_ERR_INVALID;
    if (mode == 1 && (!mu || !sigma)) return SVHIP_ERR_INVALID;
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const bool din = flags & SVHIP_IN_DEVICE, dout = flags & SVHIP_OUT_DEVICE;
    if (!din) {   // host indices are range-checked before they reach the GPU
        for (int64_t p = 0; p < P; ++p)
            if (ia[p] < 0 || ia[p] >= N || ib[p] < 0 || ib[p] >= N) SV_FAIL(h, SVHIP_ERR_INVALID, "pair %lld indexes outside [0, %lld)", (long long)p, (long long)N);
    }
    TempBuf tE{h, svhip_handle::SCR_IN0}, tA{h, svhip_handle::SCR_IN1}, tB{h, svhip_handle::SCR_IN2}, tM{h, svhip_handle::SCR_IN3},
        tS{h, svhip_handle::SCR_IN4}, tO{h, svhip_handle::SCR_OUT0};
    const void *dE, *dA, *dB, *dM = nullptr, *dS = nullptr;
    void* dO;
    int rc;
    if ((rc = tE.in(E, (size_t)N * D * 4, din, &dE))) return rc;
    if ((rc = tA.in(ia, (size_t)P * 4, din, &dA))) return rc;
    if ((rc = tB.in(ib, (size_t)P * 4, din, &dB))) return rc;
    if (mode == 1) {
        if ((rc = tM.in(mu, (size_t)N * 4, din, &dM))) return rc;
        if ((rc = tS.in(sigma, (size_t)N * 4, din, &dS))) return rc;
    }
    if ((rc = tO.out(out, (size_t)P * 4, dout, &dO))) return rc;
    if (mode == 0)
        rc = run(h, "score_pairs", 2.0 * P * D, [&]() { return launch_score_pairs((const float*)dE, D, (const int32_t*)dA, (const int32_t*)dB, P, (float*)dO, h->stream); });
    else
        rc = run(h, "asnorm_pairs", 2.0 * P * D, [&]() { return launch_asnorm_pairs((const float*)dE, D, (const float*)dM, (const float*)dS, (const int32_t*)dA, (const int32_t*)dB, P, (float*)dO, h->stream); });
    if (rc) return rc;
    if (!dout) SV_HIP(h, hipMemcpyAsync(out, dO, (size_t)P * 4, hipMemcpyDeviceToHost, h->stream));
    if (!(din && dout && (flags & SVHIP_ASYNC))) SV_HIP(h, hipStreamSynchronize(h->stream));
    return SVHIP_OK;
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
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const bool din = flags & SVHIP_IN_DEVICE, dout = flags & SVHIP_OUT_DEVICE;
    if (!din)
        for (int64_t p = 0; p < P; ++p)
            if (ia[p] < 0 || ia[p] >= n_files || ib[p] < 0 || ib[p] >= n_files) SV_FAIL(h, SVHIP_ERR_INVALID, "trial %lld indexes outside [0, %lld)", (long long)p, (long long)n_files);
    TempBuf tF{h, svhip_handle::SCR_IN0}, tA{h, svhip_handle::SCR_IN1}, tB{h, svhip_handle::SCR_IN2}, tO{h, svhip_handle::SCR_OUT0};
    const void *dF, *dA, *dB;
    void* dO;
    int rc;
    if ((rc = tF.in(F, (size_t)n_files * n_crops * D * 4, din, &dF))) return rc;
    if ((rc = tA.in(ia, (size_t)P * 4, din, &dA))) return rc;
    if ((rc = tB.in(ib, (size_t)P * 4, din, &dB))) return rc;
    if ((rc = tO.out(out, (size_t)P * 4, dout, &dO))) return rc;
    if ((rc = run(h, "score_trials", 2.0 * P * n_crops * D, [&]() {
             return launch_trial_crops(mode, pexp, (const float*)dF, n_crops, D, (const int32_t*)dA, (const int32_t*)dB, P, (float*)dO, h->stream);
         }))) return rc;
    if (!dout) SV_HIP(h, hipMemcpyAsync(out, dO, (size_t)P * 4, hipMemcpyDeviceToHost, h->stream));
    if (!(din && dout && (flags & SVHIP_ASYNC))) SV_HIP(h, hipStreamSynchronize(h->stream));
    return SVHIP_OK;
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
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const bool din = flags & SVHIP_IN_DEVICE, dout = flags & SVHIP_OUT_DEVICE;
    TempBuf tF{h, svhip_handle::SCR_IN0}, tO{h, svhip_handle::SCR_OUT0};
    const void* dF;
    void* dO;
    int rc;
    if ((rc = tF.in(F, (size_t)n_files * n_crops * D * 4, din, &dF))) return rc;
    if ((rc = tO.out(out, (size_t)n_files * D * 4, dout, &dO))) return rc;
    if ((rc = run(h, "mean_crops", 0, [&]() { return launch_mean_crops((const float*)dF, n_files, n_crops, D, (float*)dO, h->stream); }))) return rc;
    if (!dout) SV_HIP(h, hipMemcpyAsync(out, dO, (size_t)n_files * D * 4, hipMemcpyDeviceToHost, h->stream));
    if (!(din && dout && (flags & SVHIP_ASYNC))) SV_HIP(h, hipStreamSynchronize(h->stream));
    return SVHIP_OK;
}

// out (Na, Nb) = A @ B^T.  The route is decided ONCE (split_b and score_gemm used to re-derive it from different predicates):
//   SCORE_H3W     rows of A in registers, B streamed past them as half planes (score_h3w.hip; D = 192 / 256, aligned operands);
//                 the kernel's launcher fills the planes itself (and scales both operands by exact powers of two)
//   SCORE_WORDS   the tiled GEMM with B as (hi half << 16 | lo half) words, A split in registers (gemm_pw's x3 form)
//   SCORE_F32MFMA the exact fp32 MFMA GEMM (option score_f32mfma, or shapes gemm_pw's split form does not take)
// The split forms run as three fp16 MFMAs per product on every handle since round 4 (a score of unit vectors within ~4e-8 of the float64
// oracle, the exact fp32 MFMA 3.5e-8) at twice the fp32 matrix rate.
enum ScoreRoute { SCORE_F32MFMA = 0, SCORE_WORDS = 1, SCORE_H3W = 2 };
static ScoreRoute score_route(const svhip_handle* h, const float* dA, int64_t Na, const float* dB, int64_t Nb, int D) {
    if (h->opt.score_f32mfma && !h->x3) return SCORE_F32MFMA;
    if (!h->opt.score_tiled && score_h3w_supported(D, Na, Nb) && ((reinterpret_cast<uintptr_t>(dA) | reinterpret_cast<uintptr_t>(dB)) & 15) == 0) return SCORE_H3W;
    return SCORE_WORDS;
}

static int score_gemm(svhip_handle* h, const char* label, const float* dA, int64_t Na, const float* dB, int64_t Nb, int D, float* dO, int64_t ldo,
                      ScoreRoute route, const void* dBsplit) {
    if (D % 32 != 0) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "embedding dim %d must be a multiple of 32", D);
    if (Na > (1 << 30) / 1 || Nb > (1 << 30)) SV_FAIL(h, SVHIP_ERR_INVALID, "matrix too large");
    hipStream_t st = h->stream;
    if (route == SCORE_H3W) {
        if (!dBsplit || (reinterpret_cast<uintptr_t>(dA) & 15)) SV_FAIL(h, SVHIP_ERR_STATE, "score route: the row-streaming kernel was chosen without its plane scratch");
        return run(h, label, 2.0 * Na * Nb * D, [&]() { return launch_score_h3w(dA, Na, dB, Nb, D, dO, ldo, const_cast<void*>(dBsplit), h->num_cu, st); });
    }
    GemmParams p;
    p.A = dA; p.W = dB; p.Y = dO;
    p.M = (int)Na; p.N = (int)Nb; p.K = D; p.Kp = D; p.Wrows = (int)Nb;
    p.lda = D; p.ldy = (int)ldo; p.T = 1;
    if (route == SCORE_WORDS && dBsplit && gemm_pw_supported(p, false)) { p.W = dBsplit; p.x3 = 1; }      // (the words exist: split_b ran launch_split_words)
    return run(h, label, 2.0 * Na * Nb * D, [&]() { return launch_gemm(p, false, st); });
}

// the split operand of the chosen route in a scratch slot of the handle: half planes (filled by the row-streaming kernel's own launcher:
// [2][Nb][D] halves + its scale word) or split words (filled here)
static int split_b(svhip_handle* h, ScoreRoute route, const float* dB, int64_t Nb, int D, void** out) {
    *out = nullptr;
    if (route == SCORE_F32MFMA) return SVHIP_OK;
    if (int rc = scratch(h, svhip_handle::SCR_SPLIT, std::max((size_t)Nb * D * 4, score_h3w_planes_bytes(D, Nb)), out)) return rc;
    if (route == SCORE_H3W) return SVHIP_OK;
    return run(h, "split_words", 0, [&]() { return launch_split_words(dB, *out, Nb * D, h->stream); });
}

int svhip_score_matrix(svhip_handle* h, const float* A, int64_t Na, const float* B, int64_t Nb, int32_t D, float* out, int32_t flags) {
    if (!h || !A || !B || !out || Na <= 0 || Nb <= 0 || D <= 0) return SVHIP_ERR_INVALID;
    if (D % 32 != 0) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "score_matrix: embedding dim %d must be a multiple of 32", (int)D);      // before any copy or launch
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const bool din = flags & SVHIP_IN_DEVICE, dout = flags & SVHIP_OUT_DEVICE;
    TempBuf tA{h, svhip_handle::SCR_IN0}, tB{h, svhip_handle::SCR_IN1}, tO{h, svhip_handle::SCR_OUT0};
    const void *dA, *dB;
    void* dO;
    int rc;
    if ((rc = tA.in(A, (size_t)Na * D * 4, din, &dA))) return rc;
    if ((rc = tB.in(B, (size_t)Nb * D * 4, din, &dB))) return rc;
    if ((rc = tO.out(out, (size_t)Na * Nb * 4, dout, &dO))) return rc;
    void* bsplit = nullptr;
    const ScoreRoute route = score_route(h, (const float*)dA, Na, (const float*)dB, Nb, D);
    if ((rc = split_b(h, route, (const float*)dB, Nb, D, &bsplit))) return rc;
    rc = score_gemm(h, "score_matrix", (const float*)dA, Na, (const float*)dB, Nb, D, (float*)dO, Nb, route, bsplit);
    if (!rc && !dout) { const hipError_t e = hipMemcpyAsync(out, dO, (size_t)Na * Nb * 4, hipMemcpyDeviceToHost, h->stream); if (e != hipSuccess) rc = SVHIP_ERR_HIP; }
    if (!(din && dout && (flags & SVHIP_ASYNC))) (void)hipStreamSynchronize(h->stream);
    return rc;
}

// The slab route of asnorm_stats, score_topk and score_above: A @ B^T goes through an HBM scratch (SCR_SLAB) in slabs of A's rows - at most
// 2 GiB, at least 128 rows, row stride ldk - and a row kernel consumes each slab.  open() decides everything once per call, pass() walks.
namespace {
struct SlabWalk {
    svhip_handle* h;
    const float* dA; int64_t N;
    const float* dB; int64_t M;
    int D;
    int64_t ldk = 0, slab_rows = 0;
    ScoreRoute route = SCORE_F32MFMA;
    void *bsplit = nullptr, *slab = nullptr;
    // name: the call that refuses, in its own words, an M no 128-row slab holds (NULL: no refusal, as asnorm_stats always ran)
    int open(const char* name) {
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
    // per slab: score_gemm under `label` (gemm = false: the call's one slab still holds its scores), then rows_fn(r0, rows, slab, ldk)
    int pass(const char* label, bool gemm, const std::function<int(int64_t, int64_t, const float*, int64_t)>& rows_fn) {
        for (int64_t r0 = 0; r0 < N; r0 += slab_rows) {
            const int64_t rows = std::min(slab_rows, N - r0);
            if (gemm)
                if (int rc = score_gemm(h, label, dA + r0 * D, rows, dB, M, D, (float*)slab, ldk, route, bsplit)) return rc;
            if (int rc = rows_fn(r0, rows, (const float*)slab, ldk)) return rc;
        }
        return SVHIP_OK;
    }
};
}  // namespace

// the slab path: cohort scores of `rows` embeddings into an HBM scratch (rows x K fp32), slab by slab, reduced per row.
// Used for shapes the fused kernel does not take (small cohorts, top > 256, other embedding widths, F32X3 handles) and for
// the embeddings the fused kernel flags.
static int asnorm_stats_slab(svhip_handle* h, const float* dE, int64_t N, int D, const float* dC, int K, int top, float* dM, float* dS) {
    SlabWalk w{h, dE, N, dC, K, D};
    if (int rc = w.open(nullptr)) return rc;
    return w.pass("asnorm_cohort_gemm", true, [&](int64_t r0, int64_t rows, const float* slab, int64_t ldk) {
        // the profile label names the form of the selection the launcher takes for this shape
        static const char* const labels[4] = {"asnorm_topk_reg8", "asnorm_topk_reg24", "asnorm_topk_lds", "asnorm_topk_global"};
        return run(h, labels[topk_stats_form(slab, K, (int)ldk)], 0, [&]() { return launch_topk_stats(slab, rows, K, (int)ldk, top, dM + r0, dS + r0, h->stream); });
    });
}

int svhip_asnorm_stats(svhip_handle* h, const float* E, int64_t N, int32_t D, const float* cohort, int32_t K, int32_t top,
                       float* mu, float* sigma, int32_t flags) {
    if (!h || !E || !cohort || !mu || !sigma || N <= 0 || D <= 0 || K <= 0) return SVHIP_ERR_INVALID;
    if (top < 0) top = K + top;             // python slice semantics of S[:top] (utils.py:143); top=-1 drops the smallest
    if (top > K) top = K;
    if (top <= 0) SV_FAIL(h, SVHIP_ERR_INVALID, "top must select at least one cohort score");
    if (N >= ((int64_t)1 << 31)) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "at most 2^31 - 1 embeddings per call");
    if (D % 32 != 0) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "asnorm_stats: embedding dim %d must be a multiple of 32", (int)D);      // before any copy or launch
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const bool din = flags & SVHIP_IN_DEVICE, dout = flags & SVHIP_OUT_DEVICE;
    TempBuf tE{h, svhip_handle::SCR_IN0}, tC{h, svhip_handle::SCR_IN1}, tM{h, svhip_handle::SCR_OUT0}, tS{h, svhip_handle::SCR_OUT1};
    const void *dE, *dC;
    void *dM, *dS;
    int rc;
    if ((rc = tE.in(E, (size_t)N * D * 4, din, &dE))) return rc;
    if ((rc = tC.in(cohort, (size_t)K * D * 4, din, &dC))) return rc;
    if ((rc = tM.out(mu, (size_t)N * 4, dout, &dM))) return rc;
    if ((rc = tS.out(sigma, (size_t)N * 4, dout, &dS))) return rc;
    const bool aligned = ((reinterpret_cast<uintptr_t>(dE) | reinterpret_cast<uintptr_t>(dC)) & 15) == 0;
    if (!h->x3 && aligned && asnorm_fused_supported(D, K, top) && !h->opt.asnorm_slab) {
        // fused path: the scores never leave the MFMA accumulators (csrc/asnorm_fused.hip)
        // chunks of 131 072 embeddings: the candidate statistics of chunk c run on a second stream under the MFMA kernel of
        // chunk c + 1 (two candidate buffers; the kernels meet through events)
        const int64_t chunk = std::min<int64_t>(N, 131072);
        void *mb, *cand, *cnt, *flag;
        const size_t mb_bytes = (size_t)(D + 32) * D * 4;          // [MB | slice partials of its computation]
        const size_t cand_elems = (size_t)chunk * 2 * ASNORM_CAND_PER_LANE, cnt_elems = (size_t)chunk * 4;      // (2 or 4 candidate lists per embedding)
        // (the exact default is the split form where it is built: scores to fp32 rounding at several times the fp32 matrix rate — two half
        //  planes / three fp16 MFMAs, D = 192, 256)
        const bool split = (D == 192 || D == 256) && !h->opt.asnorm_f32mfma;
        // (split: the candidate kernel takes 1.7 ms of 17 on its own and 7 when it shares the CUs with the matrix kernel: one stream.
        //  The fp32-MFMA form keeps the second stream: 26.1 - 26.9 against 27.5 ms)
        const int nbuf = (N > chunk && !split) ? 2 : 1;
        const size_t mom_bytes = (cohort_moments_scratch_bytes(D) + 255) & ~(size_t)255;
        if ((rc = scratch(h, svhip_handle::SCR_MB, mb_bytes + mom_bytes + (split ? asnorm_planes_bytes(D, K) : 0), &mb))) return rc;
        if ((rc = scratch(h, svhip_handle::SCR_CAND, cand_elems * 4 * nbuf, &cand))) return rc;
        if ((rc = scratch(h, svhip_handle::SCR_CNT, (cnt_elems + (size_t)chunk) * 4 * nbuf, &cnt))) return rc;      // per buffer: [counts (chunk, 4) | row factors (chunk)]
        if ((rc = scratch(h, svhip_handle::SCR_FLAG, (size_t)(2 * N + 1) * 4, &flag))) return rc;        // [count | flagged ids (N) | their candidate counts (N)]
        if (nbuf == 2 && !h->aux_stream) {
            SV_HIP(h, hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
            for (int i = 0; i < 4; ++i) SV_HIP(h, hipEventCreateWithFlags(&h->aux_ev[i], hipEventDisableTiming));
        }
        int32_t* nflag = (int32_t*)flag;                    // [0] = number of flagged embeddings, [1 ..] their indices
        SV_HIP(h, hipMemsetAsync(nflag, 0, 4, h->stream));
        if ((rc = run(h, "asnorm_cohort_moments", 0, [&]() { return launch_cohort_moments((const float*)dC, K, D, (float*)mb, (float*)((char*)mb + mb_bytes), h->stream); }))) return rc;
        AsnormFusedParams fp;
        fp.cohort = (const float*)dC; fp.K = K; fp.MB = (const float*)mb; fp.z = asnorm_tail_z(K, top);
        if (split) {
            void* planes = (char*)mb + mb_bytes + mom_bytes;
            fp.planes = planes;
            fp.nlists = 4;                  // the 16-wide-MFMA kernel: four lists per embedding
            // the kernel scales its operands by exact powers of two (split_planes.hip, "operand scaling"): the cohort's max |x| goes to
            // a device word behind the two planes (the buffer is sized for three)
            uint32_t* pscale = reinterpret_cast<uint32_t*>((char*)planes + (size_t)2 * (D + 32 + K) * D * 2);
            if ((rc = run(h, "asnorm_planes", 0, [&]() { return launch_asnorm_planes((const float*)mb, (const float*)dC, K, D, planes, h->stream, pscale); }))) return rc;
            fp.pscale = pscale;
        }
        int c = 0;
        for (int64_t r0 = 0; r0 < N; r0 += chunk, ++c) {
            const int64_t rows = std::min(chunk, N - r0);
            const int b = c & (nbuf - 1);
            fp.E = (const float*)dE + r0 * D; fp.N = rows;
            fp.cand = (float*)cand + b * cand_elems; fp.cnt = (int32_t*)cnt + b * (cnt_elems + (size_t)chunk);
            fp.rowscale = fp.pscale ? reinterpret_cast<float*>(fp.cnt + cnt_elems) : nullptr;
            if (nbuf == 2 && c >= 2) SV_HIP(h, hipStreamWaitEvent(h->stream, h->aux_ev[2 + b], 0));       // the statistics of chunk c - 2 have read this buffer
            if ((rc = run(h, "asnorm_fused", 2.0 * rows * K * D, [&]() { return launch_asnorm_fused(fp, D, h->stream); }))) {
                if (nbuf == 2 && h->aux_stream) (void)hipStreamSynchronize(h->aux_stream);
                return rc;
            }
            hipStream_t st2 = h->stream;
            if (nbuf == 2) {
                SV_HIP(h, hipEventRecord(h->aux_ev[b], h->stream));
                SV_HIP(h, hipStreamWaitEvent(h->aux_stream, h->aux_ev[b], 0));
                st2 = h->aux_stream;
            }
            h->cur = st2;
            rc = run(h, "asnorm_cand_stats", 0, [&]() {
                return launch_asnorm_cand_stats(fp.cand, fp.cnt, rows, top, (float*)dM, (float*)dS, r0, nflag + 1, nflag, st2, fp.nlists, fp.rowscale, nflag + 1 + N);
            });
            h->cur = h->stream;
            if (rc) {           // leave no aux-stream work pending behind a failed call
                if (nbuf == 2) (void)hipStreamSynchronize(h->aux_stream);
                return rc;
            }
            if (nbuf == 2) SV_HIP(h, hipEventRecord(h->aux_ev[2 + b], h->aux_stream));
        }
        if (nbuf == 2) for (int b = 0; b < std::min(c, 2); ++b) SV_HIP(h, hipStreamWaitEvent(h->stream, h->aux_ev[2 + b], 0));
        int32_t nf = 0;
        SV_HIP(h, hipMemcpyAsync(&nf, nflag, 4, hipMemcpyDeviceToHost, h->stream));
        SV_HIP(h, hipStreamSynchronize(h->stream));
        int64_t refit_rows = 0;
        int refit_passes = 0;
        if (nf > 0 && split && !h->opt.asnorm_norefit) {
            // REFIT (round 6).  tau = mean + z sd with z the normal quantile fits isotropic embeddings; real cohorts are not isotropic
            // (speaker centroids cluster by gender / language: bimodal cohort scores), and a row whose threshold passes fewer than `top`
            // scores, or overflows a list, used to take the slab path — N x K scores through HBM.  Such rows now go through the SAME fused
            // kernel again with a z of their own, derived from what the last pass counted (refit_next_z, asnorm_fused.hip).  At most ASNORM_REFIT_PASSES
            // passes; what is still undecided after them takes the slab path as before.
            constexpr int ASNORM_REFIT_PASSES = 3;
            const float target = fminf(1.6f * (float)top, 0.7f * (float)(2 * ASNORM_CAND_PER_LANE));
            // everything lives on the device: the state of the undecided rows (asnorm_fused.hip, "refit state": ids, z, the last measurement, the
            // bracket), the gathered rows, their statistics and the flag list of the pass; the host reads ONE word per pass (how many are left)
            void* g;
            const size_t cap = (size_t)nf;
            const size_t gbytes = cap * D * 4 + cap * 4 * (2 + 6 + 6 + 2) + 256;
            if ((rc = scratch(h, svhip_handle::SCR_GATHER, gbytes, &g))) return rc;
            float* gE = (float*)g;
            float* gM = gE + cap * D;
            float* gS = gM + cap;
            float* soa[2] = {gS + cap, gS + cap + 6 * cap};
            int32_t* gF = (int32_t*)(soa[1] + 6 * cap);      // [0] = count, [1 ..] positions within the gathered list
            int32_t* gInfo = gF + 1 + cap;                   // (gbytes: + 256 covers the counter word)
            if ((rc = run(h, "asnorm_refit_state", 0, [&]() { return launch_asnorm_refit_init(nflag + 1, nflag + 1 + N, nf, fp.z, target, soa[0], h->stream); }))) return rc;
            int cur = nf, a = 0;
            while (cur > 0 && refit_passes < ASNORM_REFIT_PASSES) {
                ++refit_passes;
                const int32_t* gI = reinterpret_cast<const int32_t*>(soa[a]);
                const float* gZ = soa[a] + cur;
                SV_HIP(h, hipMemsetAsync(gF, 0, 4, h->stream));
                if ((rc = run(h, "asnorm_gather", 0, [&]() { return launch_gather_rows((const float*)dE, gI, cur, D, gE, h->stream); }))) return rc;
                for (int64_t r0 = 0; r0 < cur; r0 += chunk) {
                    const int64_t rows = std::min<int64_t>(chunk, cur - r0);
                    fp.E = gE + r0 * D; fp.N = rows; fp.zrow = gZ + r0;
                    fp.cand = (float*)cand; fp.cnt = (int32_t*)cnt;
                    fp.rowscale = fp.pscale ? reinterpret_cast<float*>(fp.cnt + cnt_elems) : nullptr;
                    if ((rc = run(h, "asnorm_fused_refit", 2.0 * rows * K * D, [&]() { return launch_asnorm_fused(fp, D, h->stream); }))) return rc;
                    if ((rc = run(h, "asnorm_cand_stats", 0, [&]() {
                            return launch_asnorm_cand_stats(fp.cand, fp.cnt, rows, top, gM, gS, r0, gF + 1, gF, h->stream, fp.nlists, fp.rowscale, gInfo);
                        }))) return rc;
                }
                fp.zrow = nullptr;
                // (rows that are still undecided scatter whatever their slots hold: a later pass or the slab path overwrites them)
                if ((rc = run(h, "asnorm_scatter", 0, [&]() { return launch_scatter_stats(gM, gS, gI, cur, (float*)dM, (float*)dS, h->stream); }))) return rc;
                int32_t left = 0;
                SV_HIP(h, hipMemcpyAsync(&left, gF, 4, hipMemcpyDeviceToHost, h->stream));
                SV_HIP(h, hipStreamSynchronize(h->stream));
                refit_rows += cur - left;
                // (the flag order is whatever the atomics gave; a row's result does not depend on where it sits in the gathered list)
                if (left > 0 && (rc = run(h, "asnorm_refit_state", 0, [&]() {
                                     return launch_asnorm_refit_next(soa[a], cur, gF + 1, gInfo, left, target, soa[a ^ 1], h->stream);
                                 }))) return rc;
                a ^= 1;
                cur = left;
            }
            // what the refit passes could not decide: back into the flag list for the slab path
            nf = cur;
            if (nf > 0) SV_HIP(h, hipMemcpyAsync(nflag + 1, soa[a], (size_t)nf * 4, hipMemcpyDeviceToDevice, h->stream));
        }
        h->last_asnorm_refit = refit_rows;
        h->last_asnorm_refit_passes = refit_passes;
        if (nf > 0) {
            // cohort scores too far from normal for the threshold (fewer than `top` candidates, or a list overflowed) even after the refit
            // passes: these embeddings are gathered and take the slab path; results are scattered back
            void* g;
            const size_t gbytes = (size_t)nf * D * 4 + 2 * (size_t)nf * 4 + 64;
            if ((rc = scratch(h, svhip_handle::SCR_GATHER, gbytes, &g))) return rc;
            float* gE = (float*)g;
            float* gM = gE + (size_t)nf * D;
            float* gS = gM + nf;
            if ((rc = run(h, "asnorm_gather", 0, [&]() { return launch_gather_rows((const float*)dE, nflag + 1, nf, D, gE, h->stream); }))) return rc;
            if ((rc = asnorm_stats_slab(h, gE, nf, D, (const float*)dC, K, top, gM, gS))) return rc;
            if ((rc = run(h, "asnorm_scatter", 0, [&]() { return launch_scatter_stats(gM, gS, nflag + 1, nf, (float*)dM, (float*)dS, h->stream); }))) return rc;
        }
        h->last_asnorm_flagged = nf;
    } else {
        if ((rc = asnorm_stats_slab(h, (const float*)dE, N, D, (const float*)dC, K, top, (float*)dM, (float*)dS))) return rc;
        h->last_asnorm_flagged = -1;
        h->last_asnorm_refit = 0; h->last_asnorm_refit_passes = 0;
    }
    if (!dout) {
        SV_HIP(h, hipMemcpyAsync(mu, dM, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream));
        SV_HIP(h, hipMemcpyAsync(sigma, dS, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (!(din && dout && (flags & SVHIP_ASYNC))) {
        SV_HIP(h, hipStreamSynchronize(h->stream));
        release_big_scratch(h, !din || !dout);
    }
    return SVHIP_OK;
}

// ---- the search calls: top-k (score_topk.hip) and threshold search (score_above.hip) over one gallery walk (score_walk.h) ----------------
// Both decide their route from the shape and the pointers alone:
//   fused  D = 192 / 256, 16-byte aligned operands: no score reaches memory.  fused_plan cuts the call into launches
//   slab   every other width: SlabWalk writes slabs of query rows, a row kernel selects
// and the calls with statistics take the same routes with the same parts and slabs: `qc` / `gc` are their tables of (a, b) pairs.
namespace {
// One launch of the fused route: queries [r0, r0 + rows) of the call, `slices` gallery slices of `per` blocks of 32 rows.
struct FusedPart { int64_t r0, rows; bool few; int slices, per; };

// Queries go in chunks of 16 384; the whole 128-query tiles of a chunk run the shared-block form of the walk (MANY), a last tile of at most
// 32 queries the form whose waves walk different gallery blocks (FEW).  Each launch cuts the gallery into enough slices to fill the chip:
// two workgroups per CU (FEW: one, since every wave of it keeps lists of its own), a workgroup walks at least 8 (FEW: 16) gallery blocks.
// slice_bytes[few]: the scratch a launch needs per (query, slice), held within 256 MiB per launch (0: the caller's scratch has no such cap).
void fused_plan(int64_t N, int64_t M, int num_cu, const int64_t (&slice_bytes)[2], std::vector<FusedPart>& parts) {
    constexpr int64_t CHUNK = 16384;
    const int64_t nb_all = (M + 31) / 32;
    const int cu = num_cu > 0 ? num_cu : 256;
    auto add = [&](int64_t r0, int64_t rows, bool few) {
        const int64_t tiles = few ? 1 : (rows + 127) / 128;
        int64_t slices = ((few ? 1 : 2) * (int64_t)cu + tiles - 1) / tiles;
        const int64_t min_blocks = few ? 16 : 8;
        slices = std::min(slices, (nb_all + min_blocks - 1) / min_blocks);
        if (slice_bytes[few]) slices = std::min(slices, std::max<int64_t>(1, ((int64_t)256 << 20) / (rows * slice_bytes[few])));
        slices = std::max<int64_t>(1, std::min<int64_t>(slices, 65535));
        const int64_t per = (nb_all + slices - 1) / slices;
        parts.push_back({r0, rows, few, (int)((nb_all + per - 1) / per), (int)per});
    };
    for (int64_t r0 = 0; r0 < N; r0 += CHUNK) {
        const int64_t rows = std::min(CHUNK, N - r0);
        const int64_t tail = rows % 128;
        const int64_t n_few = (tail >= 1 && tail <= 32) ? tail : 0, n_many = rows - n_few;
        if (n_many) add(r0, n_many, false);
        if (n_few) add(r0 + n_many, n_few, true);
    }
}

// The coefficient tables of a call with statistics ({q_mu, q_sigma, g_mu, g_sigma}), once per call, in SCR_COEF:
// [queries (N) | gallery (whole blocks of 32 rows), on a 16-byte boundary]
int coef_tables(svhip_handle* h, const char* label, const float* const* stats, int64_t N, int64_t M, bool din, const float2** qc, const float2** gc) {
    const int slot[4] = {svhip_handle::SCR_IN2, svhip_handle::SCR_IN3, svhip_handle::SCR_IN4, svhip_handle::SCR_IN5};
    const void* d[4];
    for (int i = 0; i < 4; ++i) {
        TempBuf t{h, slot[i]};
        if (int rc = t.in(stats[i], (size_t)(i < 2 ? N : M) * 4, din, &d[i])) return rc;
    }
    const size_t q_bytes = ((size_t)N * 8 + 15) & ~(size_t)15;
    void* c = nullptr;
    if (int rc = scratch(h, svhip_handle::SCR_COEF, q_bytes + (size_t)score_topk_coef_rows(M) * 8, &c)) return rc;
    float2* qcw = reinterpret_cast<float2*>(c);
    float2* gcw = reinterpret_cast<float2*>((char*)c + q_bytes);
    *qc = qcw; *gc = gcw;
    return run(h, label, 0, [&]() {
        return launch_score_topk_coef((const float*)d[0], (const float*)d[1], N, (const float*)d[2], (const float*)d[3], M, qcw, gcw, h->stream);
    });
}

// The end of a call whose results are enqueued (rc: what the call came to so far): wait unless the call is asynchronous, report what the
// stream reports under the call's name, and release the scratch that is not kept between calls.
int search_end(svhip_handle* h, const char* name, int rc, bool din, bool dout, int32_t flags) {
    if (rc || !(din && dout && (flags & SVHIP_ASYNC))) {
        const hipError_t e = hipStreamSynchronize(h->stream);
        if (!rc && e != hipSuccess) { h->err = std::string(name) + ": " + hipGetErrorString(e); rc = SVHIP_ERR_HIP; }
        release_big_scratch(h, !din || !dout);
    }
    return rc;
}
}  // namespace

// one part of score_topk's fused route: its lists (SCR_TOPK, sized for this launch alone), the launch, its merge.  dQ, dS, dI, qc: the call's
static int topk_fused_part(svhip_handle* h, const FusedPart& t, const float* dQ, const float* dG, int64_t M, int D, int k, float* dS, int32_t* dI,
                           const float2* qc, const float2* gc) {
    const int cap = score_topk_cap(k);
    ScoreTopkParams p;
    p.Q = dQ + t.r0 * D; p.N = t.rows; p.G = dG; p.M = M; p.k = k; p.cap = cap; p.per = t.per; p.nlists = t.slices * (t.few ? 8 : 2);
    void* s = nullptr;
    const size_t list_bytes = (size_t)t.rows * p.nlists * cap * 8;
    if (int rc = scratch(h, svhip_handle::SCR_TOPK, list_bytes + (size_t)t.rows * p.nlists * 4, &s)) return rc;
    p.lists = reinterpret_cast<uint2*>(s);
    p.cnt = reinterpret_cast<int32_t*>((char*)s + list_bytes);
    p.qcoef = qc ? qc + t.r0 : nullptr; p.gcoef = gc;
    if (int rc = run(h, qc ? "score_topk_norm" : "score_topk", 2.0 * t.rows * M * D, [&]() { return launch_score_topk(p, D, t.few, t.slices, h->stream); })) return rc;
    return run(h, "score_topk_merge", 0, [&]() {
        return launch_score_topk_merge(p.lists, p.cnt, t.rows, p.nlists, cap, k, dS + t.r0 * k, dI + t.r0 * k, h->stream);
    });
}

static int topk_slab(svhip_handle* h, const char* name, const float* dQ, int64_t N, const float* dG, int64_t M, int D, int k, float* dS, int32_t* dI,
                     const float2* qc, const float2* gc) {
    SlabWalk w{h, dQ, N, dG, M, D};
    if (int rc = w.open(name)) return rc;
    return w.pass("score_topk_gemm", true, [&](int64_t r0, int64_t rows, const float* slab, int64_t ldk) {
        return run(h, qc ? "score_topk_rows_norm" : "score_topk_rows", 0, [&]() {
            return launch_score_topk_rows(slab, rows, M, ldk, k, dS + r0 * k, dI + r0 * k, h->stream, qc ? qc + r0 : nullptr, gc);
        });
    });
}

// both entry points: `stats` = {q_mu, q_sigma, g_mu, g_sigma} for the normalised call, NULL for the plain one; `name` prefixes the messages
static int score_topk_impl(svhip_handle* h, const char* name, const float* Q, int64_t N, const float* G, int64_t M, const float* const* stats,
                           int32_t D, int32_t k, float* out_score, int32_t* out_index, int32_t flags) {
    if (!h) return SVHIP_ERR_INVALID;
    if (k < 1 || k > SCORE_TOPK_MAX_K) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: k = %d is outside [1, %d]", name, (int)k, SCORE_TOPK_MAX_K);
    if (M < 1 || M > (int64_t)INT32_MAX) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: M = %lld is outside [1, 2^31 - 1]", name, (long long)M);
    if (k > M) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: k = %d exceeds the gallery's M = %lld rows", name, (int)k, (long long)M);
    if (D < 1) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: D = %d must be at least 1", name, (int)D);
    if (N < 0) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: N = %lld is negative", name, (long long)N);
    if (N == 0) return SVHIP_OK;
    if (!Q || !G || !out_score || !out_index) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: NULL pointer", name);
    if (stats && (!stats[0] || !stats[1] || !stats[2] || !stats[3])) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: NULL pointer", name);
    if (D % 32 != 0) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "%s: embedding dim %d must be a multiple of 32", name, (int)D);      // before any copy or launch
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const bool din = flags & SVHIP_IN_DEVICE, dout = flags & SVHIP_OUT_DEVICE;
    TempBuf tQ{h, svhip_handle::SCR_IN0}, tG{h, svhip_handle::SCR_IN1}, tS{h, svhip_handle::SCR_OUT0}, tI{h, svhip_handle::SCR_OUT1};
    const void *dQ, *dG;
    void *dS, *dI;
    int rc;
    if ((rc = tQ.in(Q, (size_t)N * D * 4, din, &dQ))) return rc;
    if ((rc = tG.in(G, (size_t)M * D * 4, din, &dG))) return rc;
    if ((rc = tS.out(out_score, (size_t)N * k * 4, dout, &dS))) return rc;
    if ((rc = tI.out(out_index, (size_t)N * k * 4, dout, &dI))) return rc;
    const float2 *qc = nullptr, *gc = nullptr;
    if (stats && (rc = coef_tables(h, "score_topk_coef", stats, N, M, din, &qc, &gc))) return rc;
    const bool aligned = ((reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dG)) & 15) == 0;
    if (score_topk_fused_supported(D) && aligned) {
        const int64_t list_bytes = (int64_t)score_topk_cap(k) * 8 + 4;      // a list and its count; 2 lists per slice, FEW 8
        std::vector<FusedPart> parts;
        fused_plan(N, M, h->num_cu, {2 * list_bytes, 8 * list_bytes}, parts);
        for (const FusedPart& t : parts)
            if ((rc = topk_fused_part(h, t, (const float*)dQ, (const float*)dG, M, D, k, (float*)dS, (int32_t*)dI, qc, gc))) break;
    } else {
        rc = topk_slab(h, name, (const float*)dQ, N, (const float*)dG, M, D, k, (float*)dS, (int32_t*)dI, qc, gc);
    }
    if (!rc && !dout) {
        hipError_t e = hipMemcpyAsync(out_score, dS, (size_t)N * k * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out_index, dI, (size_t)N * k * 4, hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) { h->err = std::string(name) + ": copy of the results failed: " + hipGetErrorString(e); rc = SVHIP_ERR_HIP; }
    }
    return search_end(h, name, rc, din, dout, flags);
}

int svhip_score_topk(svhip_handle* h, const float* Q, int64_t N, const float* G, int64_t M, int32_t D, int32_t k, float* out_score,
                     int32_t* out_index, int32_t flags) {
    return score_topk_impl(h, "score_topk", Q, N, G, M, nullptr, D, k, out_score, out_index, flags);
}

int svhip_score_topk_norm(svhip_handle* h, const float* Q, int64_t N, const float* q_mu, const float* q_sigma, const float* G, int64_t M,
                          const float* g_mu, const float* g_sigma, int32_t D, int32_t k, float* out_score, int32_t* out_index, int32_t flags) {
    const float* stats[4] = {q_mu, q_sigma, g_mu, g_sigma};
    return score_topk_impl(h, "score_topk_norm", Q, N, G, M, stats, D, k, out_score, out_index, flags);
}

// ---- threshold search: every gallery row at or above a score, as CSR rows (score_above.hip) -----------------------------------------------
// Routes, fused_plan's parts and the slabs are score_topk's.  Both entry points count first (every launch of the call, into one scratch: a
// few list counts per row); fill then reads ONE word back - the first row whose recount is not what row_ptr says - and writes only if there
// is none, so no entry outside [0, row_ptr[N]) is ever touched.
namespace {
struct AboveArgs {
    const float *dQ, *dG;
    int64_t N, M;
    int D;
    float thr;
    int upper;
    int64_t q_base;
    const float2 *qc, *gc;
    int64_t* dCount;              // count
    const int64_t* dRowPtr;       // fill
    int32_t* dIndex;
    float* dScore;
    int64_t total;                // fill: row_ptr[N]
};

// fill: the word the scan / row kernels lowered -> OK, or the refusal that names the row
int above_guard(svhip_handle* h, const unsigned long long* bad) {
    unsigned long long row = 0;
    SV_HIP(h, hipMemcpyAsync(&row, bad, 8, hipMemcpyDeviceToHost, h->stream));
    SV_HIP(h, hipStreamSynchronize(h->stream));
    if (row != ~0ull)
        SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: row %llu now holds another number of hits than row_ptr[%llu + 1] - row_ptr[%llu] (or row_ptr[0] is not 0): "
                "the inputs changed between count and fill; nothing was written", row, row, row);
    return SVHIP_OK;
}

int above_fused(svhip_handle* h, const AboveArgs& a) {
    const bool fill = a.dRowPtr != nullptr;
    std::vector<FusedPart> parts;
    fused_plan(a.N, a.M, h->num_cu, {0, 0}, parts);
    auto nl = [](const FusedPart& t) { return t.slices * (t.few ? 4 : 1); };      // lists per query
    std::vector<size_t> first;                                                    // a part's place in the list-count scratch
    size_t entries = 0;
    for (const FusedPart& t : parts) {
        first.push_back(entries);
        entries += (size_t)t.rows * nl(t);
    }
    // [the guard's word (256 bytes) | list counts (int32) | fill: list offsets (int64)]
    const size_t cnt_bytes = (entries * 4 + 255) & ~(size_t)255;
    void* s = nullptr;
    if (int rc = scratch(h, svhip_handle::SCR_TOPK, 256 + cnt_bytes + (fill ? entries * 8 : 0), &s)) return rc;
    unsigned long long* bad = reinterpret_cast<unsigned long long*>(s);
    int32_t* lcnt = reinterpret_cast<int32_t*>((char*)s + 256);
    int64_t* loff = reinterpret_cast<int64_t*>((char*)s + 256 + cnt_bytes);
    if (fill) SV_HIP(h, hipMemsetAsync(bad, 0xff, 8, h->stream));
    auto params = [&](size_t i) {
        const FusedPart& t = parts[i];
        ScoreAboveParams p;
        p.Q = a.dQ + t.r0 * a.D; p.N = t.rows; p.G = a.dG; p.M = a.M; p.thr = a.thr; p.upper = a.upper; p.row_base = a.q_base + t.r0;
        p.per = t.per; p.nl = nl(t); p.lcnt = lcnt + first[i]; p.loff = loff + first[i]; p.out_index = a.dIndex; p.out_score = a.dScore;
        p.qcoef = a.qc ? a.qc + t.r0 : nullptr; p.gcoef = a.gc;
        return p;
    };
    for (size_t i = 0; i < parts.size(); ++i) {
        const FusedPart& t = parts[i];
        const ScoreAboveParams p = params(i);
        if (int rc = run(h, "score_above_count", 2.0 * t.rows * a.M * a.D, [&]() { return launch_score_above(p, a.D, t.few, t.slices, false, h->stream); })) return rc;
        if (int rc = run(h, "score_above_scan", 0, [&]() {
                return launch_score_above_scan(p.lcnt, t.rows, p.nl, fill ? nullptr : a.dCount + t.r0, fill ? a.dRowPtr + t.r0 : nullptr, t.r0,
                                               fill ? loff + first[i] : nullptr, fill ? bad : nullptr, h->stream);
            })) return rc;
    }
    if (!fill) return SVHIP_OK;
    if (int rc = above_guard(h, bad)) return rc;
    if (a.total == 0) return SVHIP_OK;
    for (size_t i = 0; i < parts.size(); ++i) {
        const FusedPart& t = parts[i];
        const ScoreAboveParams p = params(i);
        if (int rc = run(h, "score_above_fill", 2.0 * t.rows * a.M * a.D, [&]() { return launch_score_above(p, a.D, t.few, t.slices, true, h->stream); })) return rc;
    }
    return SVHIP_OK;
}

int above_slab(svhip_handle* h, const AboveArgs& a) {
    const bool fill = a.dRowPtr != nullptr;
    SlabWalk w{h, a.dQ, a.N, a.dG, a.M, a.D};
    void* word = nullptr;
    int rc;
    if ((rc = w.open("score_above"))) return rc;
    if ((rc = scratch(h, svhip_handle::SCR_TOPK, 256, &word))) return rc;
    unsigned long long* bad = reinterpret_cast<unsigned long long*>(word);
    if (fill) SV_HIP(h, hipMemsetAsync(bad, 0xff, 8, h->stream));
    // one pass over the slabs: count, compare with row_ptr (check) or write
    auto pass = [&](bool check, bool gemm) {
        return w.pass("score_above_gemm", gemm, [&](int64_t r0, int64_t rows, const float* slab, int64_t ldk) {
            return run(h, "score_above_rows", 0, [&]() {
                return launch_score_above_rows(slab, rows, a.M, ldk, a.thr, a.upper, a.q_base + r0, a.qc ? a.qc + r0 : nullptr, a.gc,
                                               fill ? nullptr : a.dCount + r0, fill ? a.dRowPtr + r0 : nullptr, r0, check ? bad : nullptr,
                                               fill && !check ? a.dIndex : nullptr, fill && !check ? a.dScore : nullptr, h->stream);
            });
        });
    };
    if (!fill) return pass(false, true);
    if ((rc = pass(true, true))) return rc;
    if ((rc = above_guard(h, bad))) return rc;
    if (a.total == 0) return SVHIP_OK;
    return pass(false, w.slab_rows < a.N);                          // (one slab: its scores are still there)
}

int score_above_impl(svhip_handle* h, bool fill, const float* Q, int64_t N, const float* G, int64_t M, int32_t D, float thr, const float* const* stats,
                     int64_t q_base, int32_t mode, int64_t* out_count, const int64_t* row_ptr, int32_t* out_index, float* out_score, int32_t flags) {
    if (!h) return SVHIP_ERR_INVALID;
    if (thr != thr) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: the threshold is NaN");
    if (M < 1 || M > (int64_t)INT32_MAX) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: M = %lld is outside [1, 2^31 - 1]", (long long)M);
    if (D < 1) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: D = %d must be at least 1", (int)D);
    if (N < 0) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: N = %lld is negative", (long long)N);
    if (mode & ~SVHIP_ABOVE_UPPER) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: unknown mode bits %d", (int)mode);
    const int upper = mode & SVHIP_ABOVE_UPPER;
    if (upper && q_base < 0) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: q_base = %lld is negative", (long long)q_base);
    const int n_stats = !!stats[0] + !!stats[1] + !!stats[2] + !!stats[3];
    if (n_stats != 0 && n_stats != 4) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: %d of the four statistic arrays are NULL: give all four or none", 4 - n_stats);
    if (N == 0) return SVHIP_OK;
    if (!Q || !G || (fill ? !row_ptr : !out_count)) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: NULL pointer");
    if (D % 32 != 0) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "score_above: embedding dim %d must be a multiple of 32", (int)D);      // before any copy or launch
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const bool din = flags & SVHIP_IN_DEVICE, dout = flags & SVHIP_OUT_DEVICE;
    AboveArgs a{};
    a.N = N; a.M = M; a.D = D; a.thr = thr; a.upper = upper; a.q_base = upper ? q_base : 0;
    TempBuf tQ{h, svhip_handle::SCR_IN0}, tG{h, svhip_handle::SCR_IN1}, tR{h, svhip_handle::SCR_OUT2}, tI{h, svhip_handle::SCR_OUT0}, tS{h, svhip_handle::SCR_OUT1};
    const void *dQ, *dG;
    int rc;
    if ((rc = tQ.in(Q, (size_t)N * D * 4, din, &dQ))) return rc;
    if ((rc = tG.in(G, (size_t)M * D * 4, din, &dG))) return rc;
    a.dQ = (const float*)dQ; a.dG = (const float*)dG;
    if (fill) {
        const void* dR;
        if ((rc = tR.in(row_ptr, (size_t)(N + 1) * 8, din, &dR))) return rc;
        a.dRowPtr = (const int64_t*)dR;
        if (din) {          // (on the handle's stream: a row_ptr produced there needs no wait by the caller)
            SV_HIP(h, hipMemcpyAsync(&a.total, row_ptr + N, 8, hipMemcpyDeviceToHost, h->stream));
            SV_HIP(h, hipStreamSynchronize(h->stream));
        }
        else a.total = row_ptr[N];
        if (a.total < 0) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: row_ptr[N] = %lld is negative", (long long)a.total);
        if (a.total > 0 && (!out_index || !out_score)) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: NULL pointer");
        void *dI = nullptr, *dS = nullptr;
        if (a.total > 0 && ((rc = tI.out(out_index, (size_t)a.total * 4, dout, &dI)) || (rc = tS.out(out_score, (size_t)a.total * 4, dout, &dS)))) return rc;
        a.dIndex = (int32_t*)dI; a.dScore = (float*)dS;
    } else {
        void* dC;
        if ((rc = tI.out(out_count, (size_t)N * 8, dout, &dC))) return rc;
        a.dCount = (int64_t*)dC;
    }
    if (n_stats && (rc = coef_tables(h, "score_above_coef", stats, N, M, din, &a.qc, &a.gc))) return rc;
    const bool aligned = ((reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dG)) & 15) == 0;
    rc = score_topk_fused_supported(D) && aligned ? above_fused(h, a) : above_slab(h, a);
    if (!rc && !dout) {
        hipError_t e = hipSuccess;
        if (!fill) e = hipMemcpyAsync(out_count, a.dCount, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream);
        else if (a.total > 0) {
            e = hipMemcpyAsync(out_index, a.dIndex, (size_t)a.total * 4, hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(out_score, a.dScore, (size_t)a.total * 4, hipMemcpyDeviceToHost, h->stream);
        }
        if (e != hipSuccess) { h->err = std::string("score_above: copy of the results failed: ") + hipGetErrorString(e); rc = SVHIP_ERR_HIP; }
    }
    return search_end(h, "score_above", rc, din, dout, flags);
}
}  // namespace

int svhip_score_above_count(svhip_handle* h, const float* Q, int64_t N, const float* G, int64_t M, int32_t D, float thr, const float* q_mu,
                            const float* q_sigma, const float* g_mu, const float* g_sigma, int64_t q_base, int32_t mode, int64_t* out_count, int32_t flags) {
    const float* stats[4] = {q_mu, q_sigma, g_mu, g_sigma};
    return score_above_impl(h, false, Q, N, G, M, D, thr, stats, q_base, mode, out_count, nullptr, nullptr, nullptr, flags);
}

int svhip_score_above_fill(svhip_handle* h, const float* Q, int64_t N, const float* G, int64_t M, int32_t D, float thr, const float* q_mu,
                           const float* q_sigma, const float* g_mu, const float* g_sigma, int64_t q_base, int32_t mode, const int64_t* row_ptr,
                           int32_t* out_index, float* out_score, int32_t flags) {
    const float* stats[4] = {q_mu, q_sigma, g_mu, g_sigma};
    return score_above_impl(h, true, Q, N, G, M, D, thr, stats, q_base, mode, nullptr, row_ptr, out_index, out_score, flags);
}

// ---- dataset audit: per-file mismatch counts inside groups of files (group_audit.hip) ------------------------------------------------------
// group_ptr is a host array: it is checked here, and the host derives from it what the launches need (the score block and pair-list
// prefix sums, the widest group in tiles).  The per-file tables are made on the device from its uploaded copy.
int svhip_group_audit(svhip_handle* h, const float* F, int64_t n_files, int32_t n_crops, int32_t D, const int64_t* group_ptr, int64_t n_groups,
                      float cut, int32_t* out_miss, float* out_score, int32_t flags) {
    if (!h) return SVHIP_ERR_INVALID;
    if (n_crops < 1) SV_FAIL(h, SVHIP_ERR_INVALID, "group_audit: n_crops = %d must be at least 1", (int)n_crops);
    if (D < 1) SV_FAIL(h, SVHIP_ERR_INVALID, "group_audit: D = %d must be at least 1", (int)D);
    if (n_files < 0) SV_FAIL(h, SVHIP_ERR_INVALID, "group_audit: n_files = %lld is negative", (long long)n_files);
    if (n_groups < 0) SV_FAIL(h, SVHIP_ERR_INVALID, "group_audit: n_groups = %lld is negative", (long long)n_groups);
    if (n_files == 0 || n_groups == 0) return SVHIP_OK;
    if (!F || !group_ptr || !out_miss) SV_FAIL(h, SVHIP_ERR_INVALID, "group_audit: NULL pointer");
    if (group_ptr[0] != 0) SV_FAIL(h, SVHIP_ERR_INVALID, "group_audit: group_ptr[0] = %lld is not 0", (long long)group_ptr[0]);
    for (int64_t g = 0; g < n_groups; ++g)
        if (group_ptr[g + 1] < group_ptr[g])
            SV_FAIL(h, SVHIP_ERR_INVALID, "group_audit: group_ptr decreases at entry %lld (%lld after %lld)", (long long)(g + 1), (long long)group_ptr[g + 1],
                    (long long)group_ptr[g]);
    if (group_ptr[n_groups] != n_files)
        SV_FAIL(h, SVHIP_ERR_INVALID, "group_audit: group_ptr[n_groups] = %lld is not n_files = %lld", (long long)group_ptr[n_groups], (long long)n_files);
    if (n_files > (int64_t)INT32_MAX) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "group_audit: at most 2^31 - 1 files per call (n_files = %lld)", (long long)n_files);
    SV_HIP(h, hipSetDevice(h->cfg.device));
    const bool din = flags & SVHIP_IN_DEVICE, dout = flags & SVHIP_OUT_DEVICE;

    // host tables: [group_ptr | sq: score-block starts | pp: pair-list starts], n_groups + 1 entries each
    const int64_t G1 = n_groups + 1;
    std::vector<int64_t> tab((size_t)3 * G1);
    int64_t max_cols = 1;
    for (int64_t g = 0; g < n_groups; ++g) {
        const int64_t s = group_ptr[g], e = group_ptr[g + 1], n = e - s;
        tab[g] = s;
        tab[G1 + g + 1] = tab[G1 + g] + n * n;
        tab[2 * G1 + g + 1] = tab[2 * G1 + g] + n * (n + 1) / 2;
        if (n > 0) max_cols = std::max(max_cols, (e - 1) / 64 - s / 64 + 1);
    }
    tab[n_groups] = n_files;
    const int64_t n_scores = tab[2 * G1 - 1], n_pairs = tab[3 * G1 - 1];

    TempBuf tF{h, svhip_handle::SCR_IN0}, tT{h, svhip_handle::SCR_IN3}, tM{h, svhip_handle::SCR_OUT0}, tS{h, svhip_handle::SCR_OUT1};
    const void *dF, *dT;
    void *dM, *dS = nullptr, *ft = nullptr;
    int rc;
    if ((rc = tF.in(F, (size_t)n_files * n_crops * D * 4, din, &dF))) return rc;
    if ((rc = tT.in(tab.data(), tab.size() * 8, false, &dT))) return rc;
    SV_HIP(h, hipStreamSynchronize(h->stream));                       // `tab` is pageable host memory of this call: its copy has run
    if ((rc = tM.out(out_miss, (size_t)n_files * 4, dout, &dM))) return rc;
    if (out_score && n_scores > 0 && (rc = tS.out(out_score, (size_t)n_scores * 4, dout, &dS))) return rc;
    if ((rc = scratch(h, svhip_handle::SCR_COEF, (size_t)n_files * 16, &ft))) return rc;      // [sbase (int64) | gs | ge]
    const int64_t *dGp = (const int64_t*)dT, *dSq = dGp + G1, *dPp = dGp + 2 * G1;
    int64_t* dBase = (int64_t*)ft;
    int32_t *dGs = (int32_t*)(dBase + n_files), *dGe = dGs + n_files;
    SV_HIP(h, hipMemsetAsync(dM, 0, (size_t)n_files * 4, h->stream));
    rc = run(h, "group_audit_tables", 0, [&]() { return launch_group_audit_tables(dGp, n_groups, dS ? dSq : nullptr, n_files, dGs, dGe, dBase, h->stream); });
    const bool mfma = group_audit_mfma_supported(D) && (reinterpret_cast<uintptr_t>(dF) & 15) == 0;
    if (!rc && mfma) {
        GroupAuditParams p;
        p.F = (const float*)dF; p.n_files = n_files; p.n_crops = n_crops; p.D = D;
        p.gs = dGs; p.ge = dGe; p.sbase = dBase; p.cut = cut; p.miss = (int32_t*)dM; p.score = (float*)dS;
        rc = run(h, "group_audit", 2.0 * n_crops * D * (double)n_pairs, [&]() { return launch_group_audit(p, max_cols, h->stream); });
    } else if (!rc) {
        // chunks of 2^21 pairs: 24 MiB of scratch (two index lists and the scores)
        const int64_t chunk = std::min<int64_t>(n_pairs, (int64_t)1 << 21);
        void *ia = nullptr, *ib = nullptr, *sc = nullptr;
        if ((rc = scratch(h, svhip_handle::SCR_IN1, (size_t)chunk * 4, &ia)) || (rc = scratch(h, svhip_handle::SCR_IN2, (size_t)chunk * 4, &ib)) ||
            (rc = scratch(h, svhip_handle::SCR_OUT2, (size_t)chunk * 4, &sc))) return rc;
        for (int64_t p0 = 0; p0 < n_pairs && !rc; p0 += chunk) {
            const int64_t P = std::min(chunk, n_pairs - p0);
            rc = run(h, "group_audit_pairs", 0, [&]() { return launch_group_audit_pairs(dGp, dPp, n_groups, p0, P, (int32_t*)ia, (int32_t*)ib, h->stream); });
            if (!rc) rc = run(h, "score_trials", 2.0 * P * n_crops * D, [&]() {
                return launch_trial_crops(0, 2.0f, (const float*)dF, n_crops, D, (const int32_t*)ia, (const int32_t*)ib, P, (float*)sc, h->stream);
            });
            if (!rc) rc = run(h, "group_audit_count", 0, [&]() {
                return launch_group_audit_count((const float*)sc, (const int32_t*)ia, (const int32_t*)ib, P, cut, dGs, dGe, dBase, (int32_t*)dM, (float*)dS, h->stream);
            });
        }
    }
    if (!rc && !dout) {
        hipError_t e = hipMemcpyAsync(out_miss, dM, (size_t)n_files * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && dS) e = hipMemcpyAsync(out_score, dS, (size_t)n_scores * 4, hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) { h->err = std::string("group_audit: copy of the results failed: ") + hipGetErrorString(e); rc = SVHIP_ERR_HIP; }
    }
    return search_end(h, "group_audit", rc, din, dout, flags);
}

int64_t svhip_asnorm_last_fallback(const svhip_handle* h) { return h ? h->last_asnorm_flagged : -1; }
int64_t svhip_asnorm_last_refit(const svhip_handle* h, int32_t* passes) {
    if (passes) *passes = h ? h->last_asnorm_refit_passes : 0;
    return h ? h->last_asnorm_refit : 0;
}

// ---- verification metrics (metrics.hip) ------------------------------------------------------------------------------------
namespace {
// shared front half: stage scores / labels, sort, scan.  Labels must be 0 / 1 (host labels are checked).
struct MetricsRun {
    svhip_handle* h;
    TempBuf tS{nullptr, svhip_handle::SCR_IN0}, tL{nullptr, svhip_handle::SCR_IN1};
    void* ws = nullptr;
    size_t ws_bytes = 0;
    explicit MetricsRun(svhip_handle* hh) : h(hh) { tS.h = hh; tL.h = hh; }
    int start(const float* scores, const int32_t* labels, int64_t P, bool din, bool nan_to_num, const char* label) {
        if (P >= ((int64_t)1 << 31)) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "trial lists are limited to 2^31 - 1 entries");
        if (!din)
            for (int64_t i = 0; i < P; ++i)
                if (labels[i] != 0 && labels[i] != 1) SV_FAIL(h, SVHIP_ERR_INVALID, "label %lld of trial %lld is not 0 / 1", (long long)labels[i], (long long)i);
        SV_HIP(h, hipSetDevice(h->cfg.device));
        const void *dS, *dL;
        int rc;
        if ((rc = tS.in(scores, (size_t)P * 4, din, &dS))) return rc;
        if ((rc = tL.in(labels, (size_t)P * 4, din, &dL))) return rc;
        ws_bytes = metrics_workspace_bytes(P);
        if ((rc = scratch(h, svhip_handle::SCR_WS, ws_bytes, &ws))) return rc;
        return run(h, label, 0, [&]() { return metrics_sort_scan((const float*)dS, (const int32_t*)dL, P, nan_to_num, ws, ws_bytes, h->stream); });
    }
};
}  // namespace

int svhip_roc_points(svhip_handle* h, const float* scores, const int32_t* labels, int64_t P, int64_t* n_out, float* thr, int64_t* fps,
                     int64_t* tps, int32_t flags) {
    if (!h || !scores || !labels || !n_out || !thr || !fps || !tps || P <= 0) return SVHIP_ERR_INVALID;
    const bool din = flags & SVHIP_IN_DEVICE, dout = flags & SVHIP_OUT_DEVICE;
    MetricsRun m(h);
    int rc;
    if ((rc = m.start(scores, labels, P, din, true, "metrics_sort"))) return rc;
    TempBuf tT{h, svhip_handle::SCR_OUT0}, tF{h, svhip_handle::SCR_OUT1}, tP{h, svhip_handle::SCR_OUT2};
    void *dT, *dF, *dP;
    if ((rc = tT.out(thr, (size_t)P * 4, dout, &dT)) || (rc = tF.out(fps, (size_t)P * 8, dout, &dF)) || (rc = tP.out(tps, (size_t)P * 8, dout, &dP))) return rc;
    int32_t* n_dev = nullptr;
    if ((rc = run(h, "metrics_roc", 0, [&]() { return metrics_roc_points(P, m.ws, m.ws_bytes, (float*)dT, (int64_t*)dF, (int64_t*)dP, &n_dev, h->stream); }))) return rc;
    int32_t n32 = 0;
    SV_HIP(h, hipMemcpyAsync(&n32, n_dev, 4, hipMemcpyDeviceToHost, h->stream));
    SV_HIP(h, hipStreamSynchronize(h->stream));
    *n_out = n32;
    if (!dout) {
        SV_HIP(h, hipMemcpy(thr, dT, (size_t)n32 * 4, hipMemcpyDeviceToHost));
        SV_HIP(h, hipMemcpy(fps, dF, (size_t)n32 * 8, hipMemcpyDeviceToHost));
        SV_HIP(h, hipMemcpy(tps, dP, (size_t)n32 * 8, hipMemcpyDeviceToHost));
    }
    return SVHIP_OK;
}

int svhip_error_rates(svhip_handle* h, const float* scores, const int32_t* labels, int64_t P, double* fnrs, double* fprs, float* thresholds,
                      int32_t flags) {
    if (!h || !scores || !labels || !fnrs || !fprs || !thresholds || P <= 0) return SVHIP_ERR_INVALID;
    const bool din = flags & SVHIP_IN_DEVICE, dout = flags & SVHIP_OUT_DEVICE;
    MetricsRun m(h);
    int rc;
    if ((rc = m.start(scores, labels, P, din, false, "metrics_sort"))) return rc;
    TempBuf tA{h, svhip_handle::SCR_OUT0}, tB{h, svhip_handle::SCR_OUT1}, tC{h, svhip_handle::SCR_OUT2};
    void *dA, *dB, *dC;
    if ((rc = tA.out(fnrs, (size_t)P * 8, dout, &dA)) || (rc = tB.out(fprs, (size_t)P * 8, dout, &dB)) || (rc = tC.out(thresholds, (size_t)P * 4, dout, &dC))) return rc;
    if ((rc = run(h, "metrics_rates", 0, [&]() { return metrics_error_rates(P, m.ws, m.ws_bytes, (double*)dA, (double*)dB, (float*)dC, h->stream); }))) return rc;
    if (!dout) {
        SV_HIP(h, hipMemcpyAsync(fnrs, dA, (size_t)P * 8, hipMemcpyDeviceToHost, h->stream));
        SV_HIP(h, hipMemcpyAsync(fprs, dB, (size_t)P * 8, hipMemcpyDeviceToHost, h->stream));
        SV_HIP(h, hipMemcpyAsync(thresholds, dC, (size_t)P * 4, hipMemcpyDeviceToHost, h->stream));
    }
    SV_HIP(h, hipStreamSynchronize(h->stream));
    return SVHIP_OK;
}

int svhip_min_dcf(svhip_handle* h, const float* scores, const int32_t* labels, int64_t P, double p_target, double c_miss, double c_fa,
                  double* min_dcf, float* threshold, int32_t flags) {
    if (!h || !scores || !labels || !min_dcf || !threshold || P <= 0) return SVHIP_ERR_INVALID;
    MetricsRun m(h);
    int rc;
    if ((rc = m.start(scores, labels, P, flags & SVHIP_IN_DEVICE, false, "metrics_sort"))) return rc;
    void* res = nullptr;
    if ((rc = scratch(h, svhip_handle::SCR_OUT0, 16, &res))) return rc;
    rc = run(h, "metrics_min_dcf", 0, [&]() { return metrics_min_dcf(P, m.ws, m.ws_bytes, p_target, c_miss, c_fa, (double*)res, (float*)((char*)res + 8), h->stream); });
    char host[16];
    hipError_t e = rc ? hipSuccess : hipMemcpyAsync(host, res, 16, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (rc) return rc;
    SV_HIP(h, e);
    memcpy(min_dcf, host, 8);
    memcpy(threshold, host + 8, 4);
    return SVHIP_OK;
}

}  // extern "C"
