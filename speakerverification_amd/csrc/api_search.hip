// api_search.hip — the search calls of libsvhip (see include/svhip.h): top-k (score_topk.hip), threshold search (score_above.hip) and
// clustering (score_cluster.hip) over one gallery walk (score_walk.h).  All decide their route from the shape and the pointers alone:
//   fused  D = 192 / 256, 16-byte aligned operands: no score reaches memory.  fused_plan cuts the call into launches
//   slab   every other width: SlabWalk writes slabs of query rows, a row kernel selects
// and the calls with statistics take the same routes with the same parts and slabs: `qc` / `gc` are their tables of (a, b) pairs.
#include <vector>

#include "scoring_host.h"

using namespace svhip;

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
int coef_tables(Staged& s, const char* label, const float* const* stats, int64_t N, int64_t M, const float2** qc, const float2** gc) {
    svhip_handle* h = s.h;
    const int slot[4] = {svhip_handle::SCR_IN2, svhip_handle::SCR_IN3, svhip_handle::SCR_IN4, svhip_handle::SCR_IN5};
    const float* d[4];
    for (int i = 0; i < 4; ++i) d[i] = s.in(slot[i], stats[i], (size_t)(i < 2 ? N : M) * 4);
    if (s.rc) return s.rc;
    Bump b;
    const size_t o_q = b.take((size_t)N * 8), o_g = b.take((size_t)score_topk_coef_rows(M) * 8, 16);
    void* c = nullptr;
    if (int rc = scratch(h, svhip_handle::SCR_COEF, b.size, &c)) return rc;
    float2* qcw = at<float2>(c, o_q);
    float2* gcw = at<float2>(c, o_g);
    *qc = qcw; *gc = gcw;
    return run(h, label, 0, [&]() { return launch_score_topk_coef(d[0], d[1], N, d[2], d[3], M, qcw, gcw, h->stream); });
}
}  // namespace

extern "C" {

// one part of score_topk's fused route: its lists (SCR_TOPK, sized for this launch alone), the launch, its merge.  dQ, dS, dI, qc: the call's
static int topk_fused_part(svhip_handle* h, const FusedPart& t, const float* dQ, const float* dG, int64_t M, int D, int k, float* dS, int32_t* dI,
                           const float2* qc, const float2* gc) {
    const int cap = score_topk_cap(k);
    ScoreTopkParams p;
    p.Q = dQ + t.r0 * D; p.N = t.rows; p.G = dG; p.M = M; p.k = k; p.cap = cap; p.per = t.per; p.nlists = t.slices * (t.few ? 8 : 2);
    void* s = nullptr;
    Bump b;
    const size_t o_lists = b.take((size_t)t.rows * p.nlists * cap * 8), o_cnt = b.take((size_t)t.rows * p.nlists * 4);
    if (int rc = scratch(h, svhip_handle::SCR_TOPK, b.size, &s)) return rc;
    p.lists = at<uint2>(s, o_lists);
    p.cnt = at<int32_t>(s, o_cnt);
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
    Staged s(h, flags);
    const float* dQ = s.in(svhip_handle::SCR_IN0, Q, (size_t)N * D * 4);
    const float* dG = s.in(svhip_handle::SCR_IN1, G, (size_t)M * D * 4);
    float* dS = s.out(svhip_handle::SCR_OUT0, out_score, (size_t)N * k * 4);
    int32_t* dI = s.out(svhip_handle::SCR_OUT1, out_index, (size_t)N * k * 4);
    if (s.rc) return s.rc;
    int rc;
    const float2 *qc = nullptr, *gc = nullptr;
    if (stats && (rc = coef_tables(s, "score_topk_coef", stats, N, M, &qc, &gc))) return rc;
    if (score_topk_fused_supported(D) && aligned16(dQ, dG)) {
        const int64_t list_bytes = (int64_t)score_topk_cap(k) * 8 + 4;      // a list and its count; 2 lists per slice, FEW 8
        std::vector<FusedPart> parts;
        fused_plan(N, M, h->num_cu, {2 * list_bytes, 8 * list_bytes}, parts);
        for (const FusedPart& t : parts)
            if ((rc = topk_fused_part(h, t, dQ, dG, M, D, k, dS, dI, qc, gc))) break;
    } else {
        rc = topk_slab(h, name, dQ, N, dG, M, D, k, dS, dI, qc, gc);
    }
    return s.finish(name, rc, true);
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

constexpr size_t ABOVE_GUARD_BYTES = 256;      // SCR_TOPK of both routes starts with the guard's word (the slab route holds nothing else there)
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
    // [the guard's word | list counts (int32) | fill: list offsets (int64), on a 256-byte boundary]
    Bump b;
    const size_t o_bad = b.take(ABOVE_GUARD_BYTES), o_cnt = b.take(entries * 4), o_off = b.take(fill ? entries * 8 : 0, 256);
    void* s = nullptr;
    if (int rc = scratch(h, svhip_handle::SCR_TOPK, b.size, &s)) return rc;
    unsigned long long* bad = at<unsigned long long>(s, o_bad);
    int32_t* lcnt = at<int32_t>(s, o_cnt);
    int64_t* loff = at<int64_t>(s, o_off);
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
    if ((rc = scratch(h, svhip_handle::SCR_TOPK, ABOVE_GUARD_BYTES, &word))) return rc;
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
    Staged s(h, flags);
    AboveArgs a{};
    a.N = N; a.M = M; a.D = D; a.thr = thr; a.upper = upper; a.q_base = upper ? q_base : 0;
    a.dQ = s.in(svhip_handle::SCR_IN0, Q, (size_t)N * D * 4);
    a.dG = s.in(svhip_handle::SCR_IN1, G, (size_t)M * D * 4);
    if (fill) {
        a.dRowPtr = s.in(svhip_handle::SCR_OUT2, row_ptr, (size_t)(N + 1) * 8);
        if (s.rc) return s.rc;
        // row_ptr[N] is read mid-call: it sizes the outputs
        if (s.din) {          // (on the handle's stream: a row_ptr produced there needs no wait by the caller)
            SV_HIP(h, hipMemcpyAsync(&a.total, row_ptr + N, 8, hipMemcpyDeviceToHost, h->stream));
            SV_HIP(h, hipStreamSynchronize(h->stream));
        }
        else a.total = row_ptr[N];
        if (a.total < 0) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: row_ptr[N] = %lld is negative", (long long)a.total);
        if (a.total > 0 && (!out_index || !out_score)) SV_FAIL(h, SVHIP_ERR_INVALID, "score_above: NULL pointer");
        if (a.total > 0) {
            a.dIndex = s.out(svhip_handle::SCR_OUT0, out_index, (size_t)a.total * 4);
            a.dScore = s.out(svhip_handle::SCR_OUT1, out_score, (size_t)a.total * 4);
        }
    } else {
        a.dCount = s.out(svhip_handle::SCR_OUT0, out_count, (size_t)N * 8);
    }
    if (s.rc) return s.rc;
    int rc;
    if (n_stats && (rc = coef_tables(s, "score_above_coef", stats, N, M, &a.qc, &a.gc))) return rc;
    rc = score_topk_fused_supported(D) && aligned16(a.dQ, a.dG) ? above_fused(h, a) : above_slab(h, a);
    return s.finish("score_above", rc, true);
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

// ---- speaker clustering: the components of the self-join's pair set, without the pair set (score_cluster.hip) ---------------------------
// Routes, fused_plan's parts and the slabs are score_above's for Q = G = E in UPPER mode; the forest lives in out_root.  ONE link launch per
// part (or per slab) and no second MFMA pass; the scratch is O(N): the coefficient tables and the per-block root counts of the dense ids.
namespace {
struct ClusterArgs {
    const float* dE;
    int64_t N;
    int D;
    float thr;
    const float2 *qc, *gc;
    int32_t* dRoot;
    // cluster_join: the set is one side of a joint forest of `forest` rows and starts at its row `off` (forest = 0: cluster_above itself)
    int64_t off, forest;
};

int cluster_fused(svhip_handle* h, const ClusterArgs& a) {
    // The plan as for four chips' worth of CUs: four times the slices, so the workgroups under the diagonal, which return at once, leave
    // their places to walking ones instead of leaving the launch as long as one whole walk (slices still hold >= 8 / 16 gallery blocks).
    std::vector<FusedPart> parts;
    fused_plan(a.N, a.N, 4 * (h->num_cu > 0 ? h->num_cu : 256), {0, 0}, parts);
    for (const FusedPart& t : parts) {
        ClusterLinkParams p;
        p.Q = a.dE + t.r0 * a.D; p.N = t.rows; p.G = a.dE; p.M = a.N; p.thr = a.thr; p.row_base = t.r0; p.per = t.per; p.parent = a.dRoot;
        p.qcoef = a.qc ? a.qc + t.r0 : nullptr; p.gcoef = a.gc;
        // the profile's flops: the (query tile, gallery slice) workgroups that walk - the kernel's own diagonal skip leaves the others out
        const int64_t tile = t.few ? 32 : 128, span = (int64_t)t.per * 32;
        double pairs = 0;
        for (int64_t q0 = 0; q0 < t.rows; q0 += tile)
            for (int64_t y = (t.r0 + q0) / span; y < t.slices; ++y)      // (the first slice that ends above the tile's first row)
                pairs += (double)std::min(tile, t.rows - q0) * std::min(span, a.N - y * span);
        if (int rc = run(h, a.forest ? "cluster_join_self" : "cluster_link", 2.0 * pairs * a.D, [&]() {
                return a.forest ? launch_cluster_join_link(p, a.D, t.few, t.slices, CLUSTER_LINK_SIDE, a.off, a.off, a.forest, h->stream)
                                : launch_cluster_link(p, a.D, t.few, t.slices, h->stream);
            })) return rc;
    }
    return SVHIP_OK;
}

int cluster_slab(svhip_handle* h, const ClusterArgs& a) {
    SlabWalk w{h, a.dE, a.N, a.dE, a.N, a.D};
    if (int rc = w.open(a.forest ? "cluster_join" : "cluster_above")) return rc;
    return w.pass(a.forest ? "cluster_join_self_gemm" : "cluster_gemm", true, [&](int64_t r0, int64_t rows, const float* slab, int64_t ldk) {
        return run(h, a.forest ? "cluster_join_self_rows" : "cluster_link_rows", 0, [&]() {
            const float2* qc = a.qc ? a.qc + r0 : nullptr;
            return a.forest ? launch_cluster_join_rows(slab, rows, a.N, ldk, a.thr, r0, qc, a.gc, a.dRoot, CLUSTER_LINK_SIDE, a.off, a.off, a.forest, h->stream)
                            : launch_cluster_link_rows(slab, rows, a.N, ldk, a.thr, r0, qc, a.gc, a.dRoot, h->stream);
        });
    });
}

// both entry points: linkage = 0 is cluster_above (single linkage: the components themselves), else svhip_cluster_linkage's enum; `name`
// prefixes the messages.  With a linkage the components' dense ids go to scratch, the table and the agglomeration (score_linkage.hip)
// rewrite out_root inside each component, and cluster_ids runs once more over the refined roots.
int cluster_impl(svhip_handle* h, const char* name, int32_t linkage, const float* E, int64_t N, int32_t D, float thr, const float* mu,
                 const float* sigma, int32_t* out_root, int32_t* out_cluster, int64_t* out_n_clusters, int64_t* out_n_unrefined, int32_t flags) {
    if (!h) return SVHIP_ERR_INVALID;
    if (thr != thr) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: the threshold is NaN", name);
    if (D < 1) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: D = %d must be at least 1", name, (int)D);
    if (N < 0) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: N = %lld is negative", name, (long long)N);
    if (N > (int64_t)INT32_MAX) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: N = %lld is outside [0, 2^31 - 1]", name, (long long)N);
    if (!mu != !sigma) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: %s is NULL: give mu and sigma or neither", name, mu ? "sigma" : "mu");
    if (!out_n_clusters || (N > 0 && (!E || !out_root))) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: NULL pointer", name);
    if (D % 32 != 0) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "%s: embedding dim %d must be a multiple of 32", name, (int)D);      // before any copy or launch
    Staged s(h, flags);
    if (N == 0) {
        int64_t* dN = s.out(svhip_handle::SCR_OUT2, out_n_clusters, 8);
        int64_t* dU = out_n_unrefined ? s.out(svhip_handle::SCR_CNT, out_n_unrefined, 8) : nullptr;
        if (s.rc) return s.rc;
        SV_HIP(h, hipMemsetAsync(dN, 0, 8, h->stream));
        if (dU) SV_HIP(h, hipMemsetAsync(dU, 0, 8, h->stream));
        return s.finish(name, SVHIP_OK, false);
    }
    ClusterArgs a{};
    a.N = N; a.D = D; a.thr = thr;
    a.dE = s.in(svhip_handle::SCR_IN0, E, (size_t)N * D * 4);
    a.dRoot = s.out(svhip_handle::SCR_OUT0, out_root, (size_t)N * 4);
    int32_t* dCluster = out_cluster ? s.out(svhip_handle::SCR_OUT1, out_cluster, (size_t)N * 4) : nullptr;
    int64_t* dN = s.out(svhip_handle::SCR_OUT2, out_n_clusters, 8);
    int64_t* dU = out_n_unrefined ? s.out(svhip_handle::SCR_CNT, out_n_unrefined, 8) : nullptr;
    if (s.rc) return s.rc;
    int rc;
    // the rows are queries and gallery at once: both coefficient tables come from the one (mu, sigma) pair
    const float* stats[4] = {mu, sigma, mu, sigma};
    if (mu && (rc = coef_tables(s, "cluster_coef", stats, N, N, &a.qc, &a.gc))) return rc;
    // [per-block root counts | linkage: the components' dense ids | the component table | the unrefined count where the caller wants none]
    Bump b;
    const size_t o_bcnt = b.take((size_t)cluster_id_blocks(N) * 4);
    const size_t o_comp = b.take(linkage ? (size_t)N * 4 : 0, 4), o_table = b.take(linkage ? linkage_table_ints(N) * 4 : 0, 4), o_unref = b.take(linkage ? 8 : 0, 8);
    void* sc = nullptr;
    if ((rc = scratch(h, svhip_handle::SCR_TOPK, b.size, &sc))) return rc;
    int32_t* bcnt = at<int32_t>(sc, o_bcnt);
    rc = run(h, "cluster_init", 0, [&]() { return launch_cluster_init(a.dRoot, N, h->stream); });
    if (!rc) rc = score_topk_fused_supported(D) && aligned16(a.dE) ? cluster_fused(h, a) : cluster_slab(h, a);
    if (!rc) rc = run(h, "cluster_flatten", 0, [&]() { return launch_cluster_flatten(a.dRoot, N, h->stream); });
    if (!rc && linkage) {
        int32_t* comp = at<int32_t>(sc, o_comp);
        int32_t* ti = at<int32_t>(sc, o_table);
        LinkageParams p;
        p.E = a.dE; p.N = N; p.D = D; p.thr = thr; p.linkage = linkage; p.coef = a.qc; p.root = a.dRoot;
        LinkageTable& t = p.t;
        t.work_stride = N / 2 + 1;
        t.cnt = ti; t.off = ti + N; t.cursor = ti + 2 * N; t.members = ti + 3 * N; t.bsum = ti + 4 * N;
        t.work = t.bsum + cluster_id_blocks(N); t.round = t.work + 3 * t.work_stride; t.place = t.round + t.work_stride; t.n_work = t.place + t.work_stride;
        unsigned long long* unref = reinterpret_cast<unsigned long long*>(dU ? dU : at<int64_t>(sc, o_unref));
        int lds_rows = h->opt.linkage_lds_rows;
        if (lds_rows < 2 || lds_rows > LINKAGE_LDS_ROWS) lds_rows = LINKAGE_LDS_ROWS;
        // the matrices of the components beyond LDS: a pool of 64 MiB at most (the slab, if there was one, is done with)
        void* pool = nullptr;
        rc = scratch(h, svhip_handle::SCR_SLAB, N > lds_rows ? (size_t)linkage_pool_floats(N) * 4 : 256, &pool);
        p.pool = static_cast<float*>(pool);
        if (!rc) rc = run(h, "cluster_ids", 0, [&]() { return launch_cluster_ids(a.dRoot, N, bcnt, comp, dN, h->stream); });
        if (!rc) rc = run(h, "linkage_table", 0, [&]() { return launch_linkage_table(comp, N, lds_rows, t, unref, h->stream); });
        p.fill_only = h->opt.linkage_fill_only;
        if (!rc) rc = run(h, "linkage_agglo", 0, [&]() { return launch_linkage_agglo(p, lds_rows, false, h->num_cu, h->stream); });
        if (!rc && N > lds_rows) rc = run(h, "linkage_agglo_pool", 0, [&]() { return launch_linkage_agglo(p, lds_rows, true, h->num_cu, h->stream); });
    }
    if (!rc) rc = run(h, "cluster_ids", 0, [&]() { return launch_cluster_ids(a.dRoot, N, bcnt, dCluster, dN, h->stream); });
    return s.finish(name, rc, true);
}

// ---- two-set clustering: rows B joined to an already clustered (or not yet clustered) set A (svhip_cluster_join) -------------------------
// The joint forest over NA + NB rows is seeded (cluster_seed), then takes the links of up to three walks in any order: the rectangle A x B
// (always), and the self-join of every side that brought no seed - cluster_above's own plan and kernels behind the side's offset.  The
// components of a graph do not depend on the order its edges are met in, so the result is cluster_above's on [A; B] whenever the seeds
// are cluster_above's on their sides.
struct JoinSide {
    const float* d;               // (n, D)
    int64_t n, off;               // rows, the side's first joint row
    const int32_t* seed;          // int32[n] on the device, or NULL
    bool seeded;                  // the caller gave a seed (an empty side has no array to show for it): the side's own pairs are not walked
    const float2 *qc, *gc;        // its coefficient tables in the query and in the gallery layout, or NULL
};

// The rectangle on the fused route.  The SMALLER side is the query side (A where they are equal): the queries sit in registers and the
// gallery streams past them, so a long gallery gives every workgroup a long walk and the call few launches - at 1 048 576 x 64 one
// launch over A instead of 64 launches of two-block walks.  That is free on this route: both operands of the walk use one k assignment
// and one accumulation order, and a * b == b * a, so v(a, b) has the same bits whichever row is the query (asserted on the GPU:
// tests/test_gpu_cluster_join.py), and the normalised score adds its coefficients commutatively.
int join_cross_fused(svhip_handle* h, const JoinSide& a, const JoinSide& b, int D, float thr, int32_t* dRoot) {
    const bool swap = b.n < a.n;
    const JoinSide &q = swap ? b : a, &g = swap ? a : b;
    std::vector<FusedPart> parts;
    fused_plan(q.n, g.n, h->num_cu, {0, 0}, parts);
    for (const FusedPart& t : parts) {
        ClusterLinkParams p;
        p.Q = q.d + t.r0 * D; p.N = t.rows; p.G = g.d; p.M = g.n; p.thr = thr; p.row_base = t.r0; p.per = t.per; p.parent = dRoot;
        p.qcoef = q.qc ? q.qc + t.r0 : nullptr; p.gcoef = q.qc ? g.gc : nullptr;
        if (int rc = run(h, "cluster_join_link", 2.0 * t.rows * g.n * D, [&]() {
                return launch_cluster_join_link(p, D, t.few, t.slices, CLUSTER_LINK_CROSS, q.off, g.off, a.n + b.n, h->stream);
            })) return rc;
    }
    return SVHIP_OK;
}

// the slab route keeps the definitional orientation (the row of A is the query): its GEMM's bits are not promised to be symmetric
int join_cross_slab(svhip_handle* h, const JoinSide& a, const JoinSide& b, int D, float thr, int32_t* dRoot) {
    SlabWalk w{h, a.d, a.n, b.d, b.n, D};
    if (int rc = w.open("cluster_join")) return rc;
    return w.pass("cluster_join_gemm", true, [&](int64_t r0, int64_t rows, const float* slab, int64_t ldk) {
        return run(h, "cluster_join_rows", 0, [&]() {
            return launch_cluster_join_rows(slab, rows, b.n, ldk, thr, r0, a.qc ? a.qc + r0 : nullptr, a.qc ? b.gc : nullptr, dRoot, CLUSTER_LINK_CROSS,
                                            a.off, b.off, a.n + b.n, h->stream);
        });
    });
}

// a HOST seed array against the rule of cluster_seed_parent (kernels.h): the first entry the seed kernel would not take as it is, or -1
int64_t first_bad_seed(const int32_t* seed, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (cluster_seed_parent(seed[i], i) != seed[i]) return i;
    return -1;
}

int cluster_join_impl(svhip_handle* h, const float* A, int64_t NA, const int32_t* root_a, const float* B, int64_t NB, const int32_t* root_b, int32_t D,
                      float thr, const float* const* stats, int32_t* out_root, int32_t* out_cluster, int64_t* out_n_clusters, int32_t flags) {
    if (!h) return SVHIP_ERR_INVALID;
    const char* name = "cluster_join";
    if (thr != thr) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: the threshold is NaN", name);
    if (D < 1) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: D = %d must be at least 1", name, (int)D);
    if (NA < 0) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: NA = %lld is negative", name, (long long)NA);
    if (NB < 0) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: NB = %lld is negative", name, (long long)NB);
    if (NA > (int64_t)INT32_MAX || NB > (int64_t)INT32_MAX || NA + NB > (int64_t)INT32_MAX)
        SV_FAIL(h, SVHIP_ERR_INVALID, "%s: NA + NB = %lld + %lld is outside [0, 2^31 - 1]", name, (long long)NA, (long long)NB);
    const int n_stats = !!stats[0] + !!stats[1] + !!stats[2] + !!stats[3];
    if (n_stats != 0 && n_stats != 4) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: %d of the four statistic arrays are NULL: give all four or none", name, 4 - n_stats);
    const int64_t N = NA + NB;
    if (!out_n_clusters || (NA > 0 && !A) || (NB > 0 && !B) || (N > 0 && !out_root)) SV_FAIL(h, SVHIP_ERR_INVALID, "%s: NULL pointer", name);
    if (D % 32 != 0) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "%s: embedding dim %d must be a multiple of 32", name, (int)D);      // before any copy or launch
    if (!(flags & SVHIP_IN_DEVICE)) {          // host seeds are checked where they are read; device seeds are clamped by the seed kernel
        int64_t bad;
        if (root_a && (bad = first_bad_seed(root_a, NA)) >= 0)
            SV_FAIL(h, SVHIP_ERR_INVALID, "%s: root_a[%lld] = %d is outside [0, %lld]", name, (long long)bad, (int)root_a[bad], (long long)bad);
        if (root_b && (bad = first_bad_seed(root_b, NB)) >= 0)
            SV_FAIL(h, SVHIP_ERR_INVALID, "%s: root_b[%lld] = %d is outside [0, %lld]", name, (long long)bad, (int)root_b[bad], (long long)bad);
    }
    Staged s(h, flags);
    if (N == 0) {
        int64_t* dN = s.out(svhip_handle::SCR_OUT2, out_n_clusters, 8);
        if (s.rc) return s.rc;
        SV_HIP(h, hipMemsetAsync(dN, 0, 8, h->stream));
        return s.finish(name, SVHIP_OK, false);
    }
    JoinSide a{}, b{};
    a.n = NA; a.off = 0; a.seeded = root_a != nullptr;
    b.n = NB; b.off = NA; b.seeded = root_b != nullptr;
    a.d = NA ? s.in(svhip_handle::SCR_IN0, A, (size_t)NA * D * 4) : nullptr;
    b.d = NB ? s.in(svhip_handle::SCR_IN1, B, (size_t)NB * D * 4) : nullptr;
    a.seed = root_a && NA ? s.in(svhip_handle::SCR_IN6, root_a, (size_t)NA * 4) : nullptr;
    b.seed = root_b && NB ? s.in(svhip_handle::SCR_IN7, root_b, (size_t)NB * 4) : nullptr;
    int32_t* dRoot = s.out(svhip_handle::SCR_OUT0, out_root, (size_t)N * 4);
    int32_t* dCluster = out_cluster ? s.out(svhip_handle::SCR_OUT1, out_cluster, (size_t)N * 4) : nullptr;
    int64_t* dN = s.out(svhip_handle::SCR_OUT2, out_n_clusters, 8);
    if (s.rc) return s.rc;
    int rc = SVHIP_OK;
    if (n_stats) {
        // per side ONE (mu, sigma) pair and both of score_topk_coef's layouts of it: the side's rows are queries (of the rectangle, of its
        // own self-join) and gallery rows (B: of the rectangle; both: of their self-join) - cluster_above's tables, side by side
        const int slot[4] = {svhip_handle::SCR_IN2, svhip_handle::SCR_IN3, svhip_handle::SCR_IN4, svhip_handle::SCR_IN5};
        const float* d[4];
        for (int i = 0; i < 4; ++i) d[i] = s.in(slot[i], stats[i], (size_t)(i < 2 ? NA : NB) * 4);
        if (s.rc) return s.rc;
        Bump bt;
        const size_t o_qa = bt.take((size_t)NA * 8, 16), o_ga = bt.take(NA ? (size_t)score_topk_coef_rows(NA) * 8 : 0, 16);
        const size_t o_qb = bt.take((size_t)NB * 8, 16), o_gb = bt.take(NB ? (size_t)score_topk_coef_rows(NB) * 8 : 0, 16);
        void* c = nullptr;
        if ((rc = scratch(h, svhip_handle::SCR_COEF, bt.size, &c))) return rc;
        float2 *qa = at<float2>(c, o_qa), *ga = at<float2>(c, o_ga), *qb = at<float2>(c, o_qb), *gb = at<float2>(c, o_gb);
        if (NA) { a.qc = qa; a.gc = ga; }
        if (NB) { b.qc = qb; b.gc = gb; }
        if (NA) rc = run(h, "cluster_join_coef", 0, [&]() { return launch_score_topk_coef(d[0], d[1], NA, d[0], d[1], NA, qa, ga, h->stream); });
        if (!rc && NB) rc = run(h, "cluster_join_coef", 0, [&]() { return launch_score_topk_coef(d[2], d[3], NB, d[2], d[3], NB, qb, gb, h->stream); });
        if (rc) return rc;
    }
    void* sc = nullptr;
    if ((rc = scratch(h, svhip_handle::SCR_TOPK, (size_t)cluster_id_blocks(N) * 4, &sc))) return rc;
    int32_t* bcnt = static_cast<int32_t*>(sc);
    const bool fused = score_topk_fused_supported(D) && aligned16(a.d, b.d);      // (an empty side's pointer is NULL here)
    rc = run(h, "cluster_seed", 0, [&]() { return launch_cluster_seed(a.seed, NA, b.seed, NB, dRoot, h->stream); });
    if (!rc && NA && NB) rc = fused ? join_cross_fused(h, a, b, D, thr, dRoot) : join_cross_slab(h, a, b, D, thr, dRoot);
    for (const JoinSide* side : {&a, &b}) {
        if (rc || !side->n || side->seeded) continue;      // a seeded side is trusted, not rescored
        ClusterArgs ca{};
        ca.dE = side->d; ca.N = side->n; ca.D = D; ca.thr = thr; ca.qc = side->qc; ca.gc = side->gc; ca.dRoot = dRoot; ca.off = side->off; ca.forest = N;
        rc = fused ? cluster_fused(h, ca) : cluster_slab(h, ca);
    }
    if (!rc) rc = run(h, "cluster_flatten", 0, [&]() { return launch_cluster_flatten(dRoot, N, h->stream); });
    if (!rc) rc = run(h, "cluster_ids", 0, [&]() { return launch_cluster_ids(dRoot, N, bcnt, dCluster, dN, h->stream); });
    return s.finish(name, rc, true);
}
}  // namespace

int svhip_cluster_above(svhip_handle* h, const float* E, int64_t N, int32_t D, float thr, const float* mu, const float* sigma, int32_t* out_root,
                        int32_t* out_cluster, int64_t* out_n_clusters, int32_t flags) {
    return cluster_impl(h, "cluster_above", 0, E, N, D, thr, mu, sigma, out_root, out_cluster, out_n_clusters, nullptr, flags);
}

int svhip_cluster_linkage(svhip_handle* h, const float* E, int64_t N, int32_t D, float thr, const float* mu, const float* sigma, int32_t linkage,
                          int32_t* out_root, int32_t* out_cluster, int64_t* out_n_clusters, int64_t* out_n_unrefined, int32_t flags) {
    if (h && linkage != SVHIP_LINKAGE_AVERAGE && linkage != SVHIP_LINKAGE_COMPLETE)
        SV_FAIL(h, SVHIP_ERR_INVALID, "cluster_linkage: linkage = %d is neither SVHIP_LINKAGE_AVERAGE nor SVHIP_LINKAGE_COMPLETE", (int)linkage);
    return cluster_impl(h, "cluster_linkage", linkage, E, N, D, thr, mu, sigma, out_root, out_cluster, out_n_clusters, out_n_unrefined, flags);
}

int svhip_cluster_join(svhip_handle* h, const float* A, int64_t NA, const int32_t* root_a, const float* B, int64_t NB, const int32_t* root_b, int32_t D,
                       float thr, const float* a_mu, const float* a_sigma, const float* b_mu, const float* b_sigma, int32_t* out_root,
                       int32_t* out_cluster, int64_t* out_n_clusters, int32_t flags) {
    const float* stats[4] = {a_mu, a_sigma, b_mu, b_sigma};
    return cluster_join_impl(h, A, NA, root_a, B, NB, root_b, D, thr, stats, out_root, out_cluster, out_n_clusters, flags);
}

}  // extern "C"
