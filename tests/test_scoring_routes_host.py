"""CPU: tests/scoring_routes_check.py against the sources it restates, its tables against its predicates, and the properties of its
inputs that tests/test_gpu_scoring_routes.py relies on."""
import os
import re

import numpy as np
import pytest

from oracle import scoring as o_scoring
from tests import scoring_routes_check as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*path):
    return open(os.path.join(ROOT, *path)).read()


def _body(text, start, end="\n}\n"):
    i = text.index(start)
    return text[i:text.index(end, i)]


def _flat(s):
    return re.sub(r"\s+", " ", s)


# ---- the predicates against the sources -------------------------------------------------------------------------------------------------
def test_selection_form_predicate_restates_score_hip():
    score = _src("speakerverification_amd", "csrc", "score.hip")
    assert int(re.search(r"constexpr int TOPK_CAP = (\d+);", score).group(1)) == chk.TOPK_CAP
    form = _flat(_body(score, "TopkStatsForm topk_stats_form("))
    assert "ld % 4 == 0 && (reinterpret_cast<uintptr_t>(S) & 15) == 0 && K <= 256 * 24" in form and chk.REG24_MAX_K == 256 * 24
    assert "K <= 256 * 8 ? TOPK_STATS_REG8 : TOPK_STATS_REG24" in form and chk.REG8_MAX_K == 256 * 8
    assert "const int Kp = (K + 3) & ~3;" in form
    assert "(size_t)(Kp + TOPK_CAP) * sizeof(uint32_t)" in form
    assert "(int)((150 * 1024) / row_bytes)" in form and chk.LDS_ROW_BUDGET == 150 * 1024
    assert "if (rpw < 1) return TOPK_STATS_GLOBAL;" in form
    assert "rpw > 4 ? 4 : rpw" in form and chk.LDS_MAX_ROWS == 4
    # both kernels enter the fast path on the same condition
    assert len(re.findall(r"if \(top <= 256 && K >= 4 \* top\) \{", score)) == 2 and chk.FAST_MAX_TOP == 256
    kernels = _src("speakerverification_amd", "csrc", "kernels.h")
    assert "enum TopkStatsForm { TOPK_STATS_REG8 = 0, TOPK_STATS_REG24 = 1, TOPK_STATS_LDS = 2, TOPK_STATS_GLOBAL = 3 };" in kernels
    # the launcher has no refusal left for a long row: every K is served
    launch = _body(score, "hipError_t launch_topk_stats(")
    assert launch.count("hipErrorInvalidValue") == 1 and "top <= 0 || top > K || ld < K" in launch


def test_route_predicates_restate_the_api_and_the_fused_kernels():
    fused = _src("speakerverification_amd", "csrc", "asnorm_fused.hip")
    assert "return (D == 192 || D == 256) && top >= 1 && top <= 256 && K >= 4 * top && K >= 64;" in _body(fused, "bool asnorm_fused_supported(")
    assert ("bool score_h3w_supported(int D, int64_t Na, int64_t Nb) { return (D == 192 || D == 256) && Na > 0 && Nb > 0 && "
            "Nb < ((int64_t)1 << 30) && Na < ((int64_t)1 << 31); }") in _src("speakerverification_amd", "csrc", "score_h3w.hip")
    host = _src("speakerverification_amd", "csrc", "scoring_host.h")
    api = _src("speakerverification_amd", "csrc", "api_scoring.hip")
    asnorm = _src("speakerverification_amd", "csrc", "api_asnorm.hip")
    search = _src("speakerverification_amd", "csrc", "api_search.hip")
    # the slab geometry is SlabWalk's, with asnorm_stats_slab's cohort of K rows as its B operand of M rows
    assert "const float* dA; int64_t N;\n    const float* dB; int64_t M;\n    int D;\n" in _body(host, "struct SlabWalk {", "\n};\n")
    walk = _body(api, "int SlabWalk::open(")
    assert "ldk = (M + 3) & ~(int64_t)3;" in walk
    assert "slab_rows = std::min<int64_t>(N, std::max<int64_t>(128, ((int64_t)1 << 31) / (ldk * 4)));" in walk
    slab = _body(asnorm, "static int asnorm_stats_slab(")
    assert "SlabWalk w{h, dE, N, dC, K, D};" in slab and "w.open(nullptr)" in slab
    assert re.findall(r'"(asnorm_topk_\w+)"', slab)[:4] == [chk.LABEL[f] for f in chk.FORMS]
    assert "const size_t cap = (size_t)256 << 20;" in _body(api, "void release_big_scratch(") and chk.BIG_SCRATCH == 256 << 20
    # the one alignment predicate of the routes: both pointers on 16 bytes
    assert ("inline bool aligned16(const void* a, const void* b = nullptr) { return ((reinterpret_cast<uintptr_t>(a) | "
            "reinterpret_cast<uintptr_t>(b)) & 15) == 0; }") in host
    route = _flat(_body(api, "ScoreRoute score_route("))
    assert route.index("if (h->opt.score_f32mfma && !h->x3) return SCORE_F32MFMA;") < route.index("score_h3w_supported(D, Na, Nb)")
    assert "score_h3w_supported(D, Na, Nb) && aligned16(dA, dB)) return SCORE_H3W;" in route
    stats = _flat(_body(asnorm, "int svhip_asnorm_stats("))
    assert "const bool aligned = aligned16(dE, dC);" in stats
    assert "if (!h->x3 && aligned && asnorm_fused_supported(D, K, top) && !h->opt.asnorm_slab) {" in stats
    # the multiple-of-32 rule stands before the first staging copy of all three entry points
    for src, fn in ((api, "int svhip_score_matrix("), (asnorm, "int svhip_asnorm_stats("), (search, "static int score_topk_impl(")):
        body = _body(src, fn)
        assert body.index("D % 32 != 0) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED") < body.index("Staged"), fn
    header = _src("include", "svhip.h")
    assert int(re.search(r"SVHIP_ERR_UNSUPPORTED = (-\d+)", header).group(1)) == chk.ERR_UNSUPPORTED
    # the split form inside the tiled route: where gemm_pw takes the shape
    assert "if (route == SCORE_WORDS && dBsplit && gemm_pw_supported(p, false)) { p.W = dBsplit; p.x3 = 1; }" in _body(api, "\nint score_gemm(")
    pw = _body(_src("speakerverification_amd", "csrc", "gemm_pw.hip"), "bool gemm_pw_supported(")
    assert "if (p.ldy % 4 != 0 || p.ldy < ((p.N + 3) & ~3)) return false;" in pw
    assert "if ((reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.W) | reinterpret_cast<uintptr_t>(p.Y)) & 15) return false;" in pw
    pair = _body(_src("speakerverification_amd", "csrc", "score.hip"), "void pair_kernel(")
    assert "if ((D & 3) == 0 && (reinterpret_cast<uintptr_t>(E) & 15) == 0) {" in pair


def test_the_header_states_what_the_tests_pin():
    header = _flat(_src("include", "svhip.h").replace(" *", " "))
    lo, hi = chk.TILED_NORM_RANGE
    assert f"L2 norm in [{lo:g}, {hi:g}]" in header
    assert "multiple of 32" in header and "SVHIP_ERR_UNSUPPORTED" in header
    assert "every K" in header
    assert "its base address" in header
    integration = _flat(_src("INTEGRATION.md"))
    assert f"L2 norm in [{lo:g}, {hi:g}]" in integration and "multiple of 32" in integration


# ---- the tables against the predicates ---------------------------------------------------------------------------------------------------
def test_band_edges_follow_from_the_formula():
    assert chk.lds_band_edges() == {4: 9088, 3: 12288, 2: 18688, 1: 37888}
    for rpw, edge in chk.lds_band_edges().items():
        assert chk.topk_form(edge) == ("lds", rpw)
        assert chk.topk_form(edge + 4) == (("lds", rpw - 1) if rpw > 1 else ("global", 4))
        assert chk.topk_form(edge - 3) == ("lds", rpw)                  # a ragged K pads up to the edge
        assert {edge, edge + 4} <= set(chk.SWITCH_K) or rpw == 1
    assert 37888 in chk.SWITCH_K and chk.topk_form(chk.BEYOND_K[0]) == ("global", 4) and chk.BEYOND_K[0] == 37888 + 4
    assert chk.topk_form(2048)[0] == "reg8" and chk.topk_form(2049)[0] == "reg24"
    assert chk.topk_form(6144)[0] == "reg24" and chk.topk_form(6145)[0] == "lds"
    # rows that are not 16-byte aligned leave the register forms
    assert chk.topk_form(2048, ld=2049)[0] == "lds" and chk.topk_form(2048, aligned=False)[0] == "lds"
    assert chk.slab_rows(10 ** 9, chk.TWO_SLAB["K"]) == 14169 and chk.slab_rows(5, 64) == 5 and chk.slab_rows(10 ** 9, 1 << 24) == 128


def test_the_case_table_reaches_every_form_and_both_sides_of_every_switch():
    cases = chk.SELECT_CASES + chk.BEYOND_CASES
    reached = {chk.topk_form(c["K"]) for c in cases}
    assert {f for f, _ in reached} == set(chk.FORMS)
    assert {r for f, r in reached if f == "lds"} == {1, 2, 3, 4}
    ks = {c["K"] for c in chk.SELECT_CASES if c["D"] == 64}
    assert set(chk.SWITCH_K) | set(chk.RAGGED_K) == ks
    assert {chk.topk_form(K)[1] for K in chk.RAGGED_K} == {1, 2, 3, 4} and all(K % 4 and chk.topk_form(K)[0] == "lds" for K in chk.RAGGED_K)
    assert {c["D"] for c in chk.SELECT_CASES} == {64, 192, 320, 512}
    for c in cases:
        K = c["K"]
        tops = chk.tops_of(K)
        assert [chk.exact_search(K, t) for t in tops] == [False] * 3 + [True] * 4, c["id"]
        assert all(1 <= chk.resolve_top(K, t) <= K for t in tops) and chk.resolve_top(K, -1) == K - 1
        assert 9 <= c["N"] <= 130
        # every SELECT case is a slab call as a whole; D = 192 only under the option
        if c in chk.SELECT_CASES:
            assert all(chk.asnorm_route(c["D"], K, t, slab_option=c["slab_option"]) == "slab" for t in tops)
            assert c["slab_option"] == (c["D"] == 192)
    # 11 rows leave a partly filled last workgroup at every rows_per_wg above 1
    assert all(c["N"] == 11 and 11 % r for r in (2, 3, 4) for c in cases if c["D"] == 64)
    # reg<24>'s exact search: a K in (2048, 6144] with an exact top
    assert any(chk.topk_form(c["K"])[0] == "reg24" and chk.exact_search(c["K"], 257) for c in chk.SELECT_CASES)
    for c in chk.BEYOND_CASES:
        if c["D"] == 192:
            assert [chk.asnorm_route(192, c["K"], t) for t in chk.tops_of(c["K"])] == ["fused"] * 3 + ["slab"] * 4
    t = chk.TWO_SLAB
    assert chk.slab_rows(10 ** 9, t["K"]) * chk.kp(t["K"]) * 4 <= chk.SLAB_BYTES < (chk.slab_rows(10 ** 9, t["K"]) + 1) * chk.kp(t["K"]) * 4
    assert chk.score_route(64, 70, 130) == "words" and chk.score_route(192, 70, 130) == "h3w"
    assert chk.score_route(192, 70, 130, aligned=False) == "words" and chk.score_route(192, 70, 130, f32mfma=True) == "f32mfma"
    assert any(c["data"] == "int" and chk.topk_form(c["K"])[0] == "global" for c in chk.BEYOND_CASES)
    assert [sz for sz in chk.ALL_SIZES if chk.split_form_taken(*sz)] == [(129, 64), chk.RAGGED_SPLIT_SIZE]
    assert not chk.split_form_taken(129, 64, aligned=False) and all(n % 32 for n in chk.RAGGED_SPLIT_SIZE)
    assert chk.F32MFMA_BAR * 10 <= chk.SPLIT_PROOF_ERR <= chk.EMULATED[chk.SPLIT_PROOF_NORM] / 2 / 2
    assert chk.REFUSED_WIDTH % 32 and all(D % 32 == 0 for D in chk.TILED_WIDTHS + chk.UNALIGNED_WIDTHS)
    assert chk.is_aligned(64, 4096) and not chk.is_aligned(64, 4100)
    assert chk.pair_vector_loads(192, True) and not chk.pair_vector_loads(192, False) and not chk.pair_vector_loads(30, True)


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------
INT_CASES = [c for c in chk.SELECT_CASES + chk.BEYOND_CASES if c["data"] == "int"]


@pytest.mark.parametrize("case", INT_CASES, ids=[c["id"] for c in INT_CASES])
def test_integer_data_ties_at_the_threshold_and_the_reference_is_the_plain_statement(case):
    """scores are exact integers; at every top of TIE_TOPS the top-th and (top + 1)-th largest are equal in at least half of the rows
    (top = 1, K - 1 and K look at the thin tails, where a unique extreme is the rule, and top = K has no (top + 1)-th).  The float64
    reference equals sort, slice, np.mean / np.std."""
    E, C = chk.inputs(case)
    K = case["K"]
    assert set(np.unique(E)) <= {-2, -1, 0, 1, 2} and set(np.unique(C)) <= {-2, -1, 0, 1, 2}
    ref = chk.Reference(E, C)
    assert np.array_equal(ref.sorted, np.round(ref.sorted))
    # every partial sum an fp32 adder can see stays exact: K max|s| < 2^24
    assert K * ref.smax < 2 ** 24
    for top in chk.TIE_TOPS(K):
        tied = ref.sorted[:, top - 1] == ref.sorted[:, top]
        assert tied.mean() >= 0.5, (top, tied.mean())
    S = (E.astype(np.float64) @ C.astype(np.float64).T)
    for top in chk.tops_of(K):
        rmu, rsd = ref.stats(top)
        omu, osd = o_scoring.asnorm_stats(E.astype(np.float64), C.astype(np.float64), top)
        assert np.array_equal(rmu, omu) and np.array_equal(rsd, osd)
        for r in (0, case["N"] - 1):
            s = sorted(S[r].tolist(), reverse=True)[:top]
            assert rmu[r] == np.mean(s) and rsd[r] == np.std(s)


def test_unit_inputs_hold_their_duplicates_and_zero_row():
    case = [c for c in chk.BEYOND_CASES if c["data"] == "unit_zero"][-1]
    E, C = chk.inputs(case)
    assert case["data"] == "unit_zero" and not E[case["N"] // 2].any() and np.array_equal(C[3], C[5]) and np.array_equal(C[-1], C[case["K"] // 2])
    assert float(np.abs(np.linalg.norm(C, axis=1) - 1).max()) <= 1e-6
    ref = chk.Reference(E, C)
    for top in chk.tops_of(case["K"]):
        omu, osd = o_scoring.asnorm_stats(E.astype(np.float64), C.astype(np.float64), chk.resolve_top(case["K"], top))
        assert np.array_equal(ref.stats(top)[0], omu) and np.array_equal(ref.stats(top)[1], osd)
    E2, C2 = chk.odd_inputs()
    s = C2[100:800].astype(np.float64) @ E2[10].astype(np.float64)
    assert s.min() > 0.9 and not E2[12].any() and C2.shape[0] == chk.ODD_K and chk.topk_form(chk.ODD_K) == ("lds", 4)
    assert chk.asnorm_route(192, chk.ODD_K, 200) == "fused"


def test_bars_come_from_the_summation_not_from_the_kernel():
    assert chk.summation_bar(50000, 256, 1.0) == 0.0
    assert chk.summation_bar(50000, 257, 1.0) == pytest.approx(4 * (257 / 64 + 6) * 2.0 ** -24)
    assert chk.summation_bar(6400, -1, 2.0) == pytest.approx(4 * (6399 / 64 + 6) * 2.0 ** -24 * 2.0)
    rmu, rsd = np.array([0.5, 0.25]), np.array([0.05, 0.1])
    assert chk.stat_errors("unit", 5000, 200, rmu + 1e-6, rsd + 5e-6, rmu, rsd, 1.0) == pytest.approx((1.0, 1.0), rel=1e-6)
    assert chk.stat_errors("unit", 5000, 1, rmu, np.array([1e-6, 0.0]), rmu, np.zeros(2), 1.0)[1] == pytest.approx(1.0)
    e = chk.stat_errors("int", 5000, 200, np.array([100.0 * (1 + 6e-8)]), np.array([16.0 * (1 + 1e-6)]), np.array([100.0]), np.array([16.0]), 80.0)
    assert e == pytest.approx((1.0, 1.0), rel=1e-3)
    # a row of equal scores beside ordinary rows: held to the absolute top = 1 bar, the others to 1e-4 of the smallest sd
    e = chk.stat_errors("unit", 5000, 200, np.zeros(3), np.array([0.05, 1e-6, 0.1 + 5e-6]), np.zeros(3), np.array([0.05, 0.0, 0.1]), 1.0)
    assert e[1] == pytest.approx(1.0)
    assert chk.stat_errors("unit", 5000, 200, np.zeros(2), np.array([0.05, 2e-6]), np.zeros(2), np.array([0.05, 0.0]), 1.0)[1] == pytest.approx(2.0)
    z = np.zeros(1)
    assert chk.stat_errors("int", 5000, 1, z, z, z, z, 80.0) == (0.0, 0.0) and chk.stat_errors("int", 5000, 1, z, z + 1e-9, z, z, 80.0)[1] == np.inf
    lo, hi = chk.TILED_NORM_RANGE
    assert [m for m in chk.MAGS if chk.in_tiled_range(m, m)] == [m for m in chk.MAGS if lo <= m <= hi] and chk.in_tiled_range(1.0, 3e4)
    assert not chk.in_tiled_range(1.0, 0.1) and not chk.in_tiled_range(0.1, 1.0)


# ---- the half split, emulated ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", chk.TILED_WIDTHS)
def test_half_split_emulation_reproduces_its_table(D):
    """hi = half(x), lo = half(x - hi), three products, float64 sums: the error relative to |a||b| grows as 1 / norm once the lo parts go
    subnormal (quantum 2^-24), the same at every width"""
    for norm, want in chk.EMULATED.items():
        A, B = chk.matrix_inputs(70, 130, D, norm, norm)
        err = chk.matrix_error(chk.half_split_product(A, B), A, B)
        print(f"emulated half split D {D} norm {norm:g}: {err:.2e}")
        assert want / 2 <= err <= want * 2, (norm, err)
    # the upper end: finite up to the largest half, 1e-7 at norms 1e3 and 3e4
    for norm in (1e3, 3e4):
        A, B = chk.matrix_inputs(70, 130, D, norm, norm)
        assert float(np.abs(A).max()) < 65504 and chk.matrix_error(chk.half_split_product(A, B), A, B) <= 2e-7
