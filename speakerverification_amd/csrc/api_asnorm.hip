// api_asnorm.hip — AS-norm cohort statistics of libsvhip (see include/svhip.h): the slab route, and the fused route as steps over one pass
// struct (setup, walk, refit, rest).
#include <cmath>

#include "scoring_host.h"

using namespace svhip;

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

namespace {
// The fused route: the scores never leave the MFMA accumulators (csrc/asnorm_fused.hip).  What every step of it reads:
struct AsnormPass {
    svhip_handle* h;
    const float* dE; int64_t N; int D;
    const float* dC; int K, top;
    float *dM, *dS;
    int64_t chunk;              // embeddings per launch
    bool split;                 // the half-plane form of the kernel
    int nbuf;                   // candidate buffers: 2 when the candidate statistics run on a second stream
    // the carved scratch (setup)
    float* cand[2];             // SCR_CAND, per buffer: (chunk, 2 or 4 candidate lists)
    int32_t* cnt[2];            // SCR_CNT, per buffer: [counts (chunk, 4) | row factors (chunk)]
    float* rowscale[2];
    int32_t *nflag, *flag_ids, *flag_cnt;       // SCR_FLAG: [count | flagged ids (N) | their candidate counts (N)]
    AsnormFusedParams fp;       // what every launch shares (cohort, moments, z, planes); a step fills E, N, zrow and the buffer into a copy
    AsnormFusedParams launch_params(int b, const float* E, int64_t rows, const float* zrow = nullptr) const {
        AsnormFusedParams p = fp;
        p.E = E; p.N = rows; p.zrow = zrow;
        p.cand = cand[b]; p.cnt = cnt[b];
        p.rowscale = p.pscale ? rowscale[b] : nullptr;
        return p;
    }
};

// scratch, the lazy second stream and its events, the cohort's moments and, for the split form, its half planes
int asnorm_setup(AsnormPass& a) {
    svhip_handle* h = a.h;
    const int D = a.D, K = a.K;
    // chunks of 131 072 embeddings: the candidate statistics of chunk c run on a second stream under the MFMA kernel of
    // chunk c + 1 (two candidate buffers; the kernels meet through events)
    a.chunk = std::min<int64_t>(a.N, 131072);
    // (the exact default is the split form where it is built: scores to fp32 rounding at several times the fp32 matrix rate — two half
    //  planes / three fp16 MFMAs, D = 192, 256)
    a.split = (D == 192 || D == 256) && !h->opt.asnorm_f32mfma;
    // (split: the candidate kernel takes 1.7 ms of 17 on its own and 7 when it shares the CUs with the matrix kernel: one stream.
    //  The fp32-MFMA form keeps the second stream: 26.1 - 26.9 against 27.5 ms)
    a.nbuf = (a.N > a.chunk && !a.split) ? 2 : 1;
    const size_t cand_elems = (size_t)a.chunk * 2 * ASNORM_CAND_PER_LANE;      // (2 or 4 candidate lists per embedding)
    const size_t plane = (size_t)(D + 32 + K) * D * 2;                         // one half plane of [MB ; cohort]
    Bump mb, cn, fl;
    const size_t o_mb = mb.take((size_t)(D + 32) * D * 4);                      // MB
    const size_t o_mom = mb.take(cohort_moments_scratch_bytes(D));             // the slice partials of its computation
    const size_t o_planes = mb.take(a.split ? 2 * plane : 0, 256);
    // the kernel scales its operands by exact powers of two (split_planes.hip, "operand scaling"): the cohort's max |x| goes to
    // a device word directly behind the two planes, its 256 partials behind it
    const size_t o_pscale = mb.take(a.split ? 257 * 4 : 0);
    mb.take(a.split ? asnorm_planes_bytes(D, K) - 2 * plane - 257 * 4 : 0);    // slack: asnorm_planes_bytes is three planes
    size_t o_cnt[2] = {}, o_rowscale[2] = {};
    for (int b = 0; b < a.nbuf; ++b) {
        o_cnt[b] = cn.take((size_t)a.chunk * 4 * 4);
        o_rowscale[b] = cn.take((size_t)a.chunk * 4);                           // (the kernel finds the row factors behind the counts)
    }
    const size_t o_nflag = fl.take(4), o_ids = fl.take((size_t)a.N * 4), o_fcnt = fl.take((size_t)a.N * 4);
    void *m, *cand, *cnt, *flag;
    int rc;
    if ((rc = scratch(h, svhip_handle::SCR_MB, mb.size, &m))) return rc;
    if ((rc = scratch(h, svhip_handle::SCR_CAND, cand_elems * 4 * a.nbuf, &cand))) return rc;
    if ((rc = scratch(h, svhip_handle::SCR_CNT, cn.size, &cnt))) return rc;
    if ((rc = scratch(h, svhip_handle::SCR_FLAG, fl.size, &flag))) return rc;
    for (int b = 0; b < a.nbuf; ++b) {
        a.cand[b] = (float*)cand + b * cand_elems;
        a.cnt[b] = at<int32_t>(cnt, o_cnt[b]);
        a.rowscale[b] = at<float>(cnt, o_rowscale[b]);
    }
    a.nflag = at<int32_t>(flag, o_nflag); a.flag_ids = at<int32_t>(flag, o_ids); a.flag_cnt = at<int32_t>(flag, o_fcnt);
    if (a.nbuf == 2 && !h->aux_stream) {
        SV_HIP(h, hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
        for (int i = 0; i < 4; ++i) SV_HIP(h, hipEventCreateWithFlags(&h->aux_ev[i], hipEventDisableTiming));
    }
    SV_HIP(h, hipMemsetAsync(a.nflag, 0, 4, h->stream));
    float* MB = at<float>(m, o_mb);
    if ((rc = run(h, "asnorm_cohort_moments", 0, [&]() { return launch_cohort_moments(a.dC, K, D, MB, at<float>(m, o_mom), h->stream); }))) return rc;
    a.fp.cohort = a.dC; a.fp.K = K; a.fp.MB = MB; a.fp.z = asnorm_tail_z(K, a.top);
    if (a.split) {
        void* planes = at<char>(m, o_planes);
        uint32_t* pscale = at<uint32_t>(m, o_pscale);
        if ((rc = run(h, "asnorm_planes", 0, [&]() { return launch_asnorm_planes(MB, a.dC, K, D, planes, h->stream, pscale); }))) return rc;
        a.fp.planes = planes; a.fp.pscale = pscale;
        a.fp.nlists = 4;                  // the 16-wide-MFMA kernel: four lists per embedding
    }
    return SVHIP_OK;
}

// the chunk loop, on one stream or two; *nf: how many embeddings the candidate statistics flagged
int asnorm_walk(AsnormPass& a, int32_t* nf) {
    svhip_handle* h = a.h;
    const int nbuf = a.nbuf;
    int rc, c = 0;
    for (int64_t r0 = 0; r0 < a.N; r0 += a.chunk, ++c) {
        const int64_t rows = std::min(a.chunk, a.N - r0);
        const int b = c & (nbuf - 1);
        const AsnormFusedParams fp = a.launch_params(b, a.dE + r0 * a.D, rows);
        if (nbuf == 2 && c >= 2) SV_HIP(h, hipStreamWaitEvent(h->stream, h->aux_ev[2 + b], 0));       // the statistics of chunk c - 2 have read this buffer
        if ((rc = run(h, "asnorm_fused", 2.0 * rows * a.K * a.D, [&]() { return launch_asnorm_fused(fp, a.D, h->stream); }))) {
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
            return launch_asnorm_cand_stats(fp.cand, fp.cnt, rows, a.top, a.dM, a.dS, r0, a.flag_ids, a.nflag, st2, fp.nlists, fp.rowscale, a.flag_cnt);
        });
        h->cur = h->stream;
        if (rc) {           // leave no aux-stream work pending behind a failed call
            if (nbuf == 2) (void)hipStreamSynchronize(h->aux_stream);
            return rc;
        }
        if (nbuf == 2) SV_HIP(h, hipEventRecord(h->aux_ev[2 + b], h->aux_stream));
    }
    if (nbuf == 2) for (int b = 0; b < std::min(c, 2); ++b) SV_HIP(h, hipStreamWaitEvent(h->stream, h->aux_ev[2 + b], 0));
    SV_HIP(h, hipMemcpyAsync(nf, a.nflag, 4, hipMemcpyDeviceToHost, h->stream));
    SV_HIP(h, hipStreamSynchronize(h->stream));
    return SVHIP_OK;
}

// SCR_GATHER for `cap` flagged embeddings: the gathered rows and their statistics; refit: also the state of the undecided rows (asnorm_fused.hip,
// "refit state": ids, z, the last measurement, the bracket; 6 * cap per buffer, two buffers) and the flag list of a pass
struct Gathered {
    float *E, *M, *S, *soa[2];
    int32_t *F, *info;          // F[0] = count, F[1 ..] positions within the gathered list; info: parallel to them
};
int gather_scratch(const AsnormPass& a, size_t cap, bool refit, Gathered* g) {
    Bump b;
    const size_t oE = b.take(cap * a.D * 4), oM = b.take(cap * 4), oS = b.take(cap * 4);
    const size_t o0 = b.take(refit ? 6 * cap * 4 : 0), o1 = b.take(refit ? 6 * cap * 4 : 0);
    const size_t oF = b.take(refit ? (1 + cap) * 4 : 0), oI = b.take(refit ? cap * 4 : 0);
    b.take(refit ? 252 : 64);       // slack: the totals were (...) + 256, which covered the counter word, and (...) + 64
    void* s;
    if (int rc = scratch(a.h, svhip_handle::SCR_GATHER, b.size, &s)) return rc;
    *g = {at<float>(s, oE), at<float>(s, oM), at<float>(s, oS), {at<float>(s, o0), at<float>(s, o1)}, at<int32_t>(s, oF), at<int32_t>(s, oI)};
    return SVHIP_OK;
}

// gather the embeddings `ids`, let `body` write the statistics of the gathered rows to g.M / g.S, scatter them to the call's mu / sigma
template <typename F>
int asnorm_gathered(const AsnormPass& a, const int32_t* ids, int n, const Gathered& g, F&& body) {
    svhip_handle* h = a.h;
    if (int rc = run(h, "asnorm_gather", 0, [&]() { return launch_gather_rows(a.dE, ids, n, a.D, g.E, h->stream); })) return rc;
    if (int rc = body()) return rc;
    return run(h, "asnorm_scatter", 0, [&]() { return launch_scatter_stats(g.M, g.S, ids, n, a.dM, a.dS, h->stream); });
}

// REFIT (round 6).  tau = mean + z sd with z the normal quantile fits isotropic embeddings; real cohorts are not isotropic
// (speaker centroids cluster by gender / language: bimodal cohort scores), and a row whose threshold passes fewer than `top`
// scores, or overflows a list, used to take the slab path — N x K scores through HBM.  Such rows now go through the SAME fused
// kernel again with a z of their own, derived from what the last pass counted (refit_next_z, asnorm_fused.hip).  At most ASNORM_REFIT_PASSES
// passes; what is still undecided after them takes the slab path as before: *nf flagged embeddings go in, what is left comes out.
int asnorm_refit(AsnormPass& a, int32_t* nf) {
    svhip_handle* h = a.h;
    int64_t refit_rows = 0;
    int refit_passes = 0;
    if (*nf > 0 && a.split && !h->opt.asnorm_norefit) {
        constexpr int ASNORM_REFIT_PASSES = 3;
        const float target = fminf(1.6f * (float)a.top, 0.7f * (float)(2 * ASNORM_CAND_PER_LANE));
        // everything lives on the device: the state of the undecided rows, the gathered rows, their statistics and the flag list of the
        // pass; the host reads ONE word per pass (how many are left)
        Gathered g;
        int rc;
        if ((rc = gather_scratch(a, (size_t)*nf, true, &g))) return rc;
        if ((rc = run(h, "asnorm_refit_state", 0, [&]() { return launch_asnorm_refit_init(a.flag_ids, a.flag_cnt, *nf, a.fp.z, target, g.soa[0], h->stream); }))) return rc;
        int cur = *nf, s = 0;
        while (cur > 0 && refit_passes < ASNORM_REFIT_PASSES) {
            ++refit_passes;
            const int32_t* gI = reinterpret_cast<const int32_t*>(g.soa[s]);
            const float* gZ = g.soa[s] + cur;
            SV_HIP(h, hipMemsetAsync(g.F, 0, 4, h->stream));
            // (rows that are still undecided scatter whatever their slots hold: a later pass or the slab path overwrites them)
            rc = asnorm_gathered(a, gI, cur, g, [&]() {
                for (int64_t r0 = 0; r0 < cur; r0 += a.chunk) {
                    const int64_t rows = std::min<int64_t>(a.chunk, cur - r0);
                    const AsnormFusedParams fp = a.launch_params(0, g.E + r0 * a.D, rows, gZ + r0);
                    if (int e = run(h, "asnorm_fused_refit", 2.0 * rows * a.K * a.D, [&]() { return launch_asnorm_fused(fp, a.D, h->stream); })) return e;
                    if (int e = run(h, "asnorm_cand_stats", 0, [&]() {
                            return launch_asnorm_cand_stats(fp.cand, fp.cnt, rows, a.top, g.M, g.S, r0, g.F + 1, g.F, h->stream, fp.nlists, fp.rowscale, g.info);
                        })) return e;
                }
                return (int)SVHIP_OK;
            });
            if (rc) return rc;
            int32_t left = 0;
            SV_HIP(h, hipMemcpyAsync(&left, g.F, 4, hipMemcpyDeviceToHost, h->stream));
            SV_HIP(h, hipStreamSynchronize(h->stream));
            refit_rows += cur - left;
            // (the flag order is whatever the atomics gave; a row's result does not depend on where it sits in the gathered list)
            if (left > 0 && (rc = run(h, "asnorm_refit_state", 0, [&]() {
                                 return launch_asnorm_refit_next(g.soa[s], cur, g.F + 1, g.info, left, target, g.soa[s ^ 1], h->stream);
                             }))) return rc;
            s ^= 1;
            cur = left;
        }
        // what the refit passes could not decide: back into the flag list for the slab path
        *nf = cur;
        if (cur > 0) SV_HIP(h, hipMemcpyAsync(a.flag_ids, g.soa[s], (size_t)cur * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    h->last_asnorm_refit = refit_rows;
    h->last_asnorm_refit_passes = refit_passes;
    return SVHIP_OK;
}

// cohort scores too far from normal for the threshold (fewer than `top` candidates, or a list overflowed) even after the refit
// passes: these embeddings are gathered and take the slab path; results are scattered back
int asnorm_rest(AsnormPass& a, int32_t nf) {
    if (nf > 0) {
        Gathered g;
        if (int rc = gather_scratch(a, (size_t)nf, false, &g)) return rc;
        if (int rc = asnorm_gathered(a, a.flag_ids, nf, g, [&]() { return asnorm_stats_slab(a.h, g.E, nf, a.D, a.dC, a.K, a.top, g.M, g.S); })) return rc;
    }
    a.h->last_asnorm_flagged = nf;
    return SVHIP_OK;
}
}  // namespace

extern "C" {

int svhip_asnorm_stats(svhip_handle* h, const float* E, int64_t N, int32_t D, const float* cohort, int32_t K, int32_t top,
                       float* mu, float* sigma, int32_t flags) {
    if (!h || !E || !cohort || !mu || !sigma || N <= 0 || D <= 0 || K <= 0) return SVHIP_ERR_INVALID;
    if (top < 0) top = K + top;             // python slice semantics of S[:top] (utils.py:143); top=-1 drops the smallest
    if (top > K) top = K;
    if (top <= 0) SV_FAIL(h, SVHIP_ERR_INVALID, "top must select at least one cohort score");
    if (N >= ((int64_t)1 << 31)) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "at most 2^31 - 1 embeddings per call");
    if (D % 32 != 0) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "asnorm_stats: embedding dim %d must be a multiple of 32", (int)D);      // before any copy or launch
    Staged s(h, flags);
    const float* dE = s.in(svhip_handle::SCR_IN0, E, (size_t)N * D * 4);
    const float* dC = s.in(svhip_handle::SCR_IN1, cohort, (size_t)K * D * 4);
    float* dM = s.out(svhip_handle::SCR_OUT0, mu, (size_t)N * 4);
    float* dS = s.out(svhip_handle::SCR_OUT1, sigma, (size_t)N * 4);
    if (s.rc) return s.rc;
    int rc;
    const bool aligned = aligned16(dE, dC);
    if (!h->x3 && aligned && asnorm_fused_supported(D, K, top) && !h->opt.asnorm_slab) {
        AsnormPass a{h, dE, N, D, dC, K, top, dM, dS};
        int32_t nf = 0;
        if (!(rc = asnorm_setup(a)) && !(rc = asnorm_walk(a, &nf)) && !(rc = asnorm_refit(a, &nf))) rc = asnorm_rest(a, nf);
    } else if (!(rc = asnorm_stats_slab(h, dE, N, D, dC, K, top, dM, dS))) {
        h->last_asnorm_flagged = -1;
        h->last_asnorm_refit = 0; h->last_asnorm_refit_passes = 0;
    }
    return s.finish("asnorm_stats", rc, true);
}

int64_t svhip_asnorm_last_fallback(const svhip_handle* h) { return h ? h->last_asnorm_flagged : -1; }
int64_t svhip_asnorm_last_refit(const svhip_handle* h, int32_t* passes) {
    if (passes) *passes = h ? h->last_asnorm_refit_passes : 0;
    return h ? h->last_asnorm_refit : 0;
}

}  // extern "C"
