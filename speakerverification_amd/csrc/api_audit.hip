// api_audit.hip — the dataset audit of libsvhip (see include/svhip.h): per-file mismatch counts inside groups of files (group_audit.hip).
#include <vector>

#include "scoring_host.h"

using namespace svhip;

extern "C" {

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

    Staged s(h, flags);
    const float* dF = s.in(svhip_handle::SCR_IN0, F, (size_t)n_files * n_crops * D * 4);
    const int64_t* dGp = s.in(svhip_handle::SCR_IN3, tab.data(), tab.size() * 8, true);
    SV_HIP(h, hipStreamSynchronize(h->stream));                       // `tab` is pageable host memory of this call: its copy has run
    int32_t* dM = s.out(svhip_handle::SCR_OUT0, out_miss, (size_t)n_files * 4);
    float* dS = out_score && n_scores > 0 ? s.out(svhip_handle::SCR_OUT1, out_score, (size_t)n_scores * 4) : nullptr;
    if (s.rc) return s.rc;
    void* ft = nullptr;
    int rc;
    Bump b;         // the per-file tables
    const size_t o_base = b.take((size_t)n_files * 8), o_gs = b.take((size_t)n_files * 4), o_ge = b.take((size_t)n_files * 4);
    if ((rc = scratch(h, svhip_handle::SCR_COEF, b.size, &ft))) return rc;
    const int64_t *dSq = dGp + G1, *dPp = dGp + 2 * G1;
    int64_t* dBase = at<int64_t>(ft, o_base);
    int32_t *dGs = at<int32_t>(ft, o_gs), *dGe = at<int32_t>(ft, o_ge);
    SV_HIP(h, hipMemsetAsync(dM, 0, (size_t)n_files * 4, h->stream));
    rc = run(h, "group_audit_tables", 0, [&]() { return launch_group_audit_tables(dGp, n_groups, dS ? dSq : nullptr, n_files, dGs, dGe, dBase, h->stream); });
    const bool mfma = group_audit_mfma_supported(D) && aligned16(dF);
    if (!rc && mfma) {
        GroupAuditParams p;
        p.F = dF; p.n_files = n_files; p.n_crops = n_crops; p.D = D;
        p.gs = dGs; p.ge = dGe; p.sbase = dBase; p.cut = cut; p.miss = dM; p.score = dS;
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
                return launch_trial_crops(0, 2.0f, dF, n_crops, D, (const int32_t*)ia, (const int32_t*)ib, P, (float*)sc, h->stream);
            });
            if (!rc) rc = run(h, "group_audit_count", 0, [&]() {
                return launch_group_audit_count((const float*)sc, (const int32_t*)ia, (const int32_t*)ib, P, cut, dGs, dGe, dBase, dM, dS, h->stream);
            });
        }
    }
    return s.finish("group_audit", rc, true);
}

}  // extern "C"
