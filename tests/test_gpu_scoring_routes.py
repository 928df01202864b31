"""GPU: dense scoring and the AS-norm statistics on every route against float64 (tables, inputs, predicates and bars:
tests/scoring_routes_check.py).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from oracle import scoring as o_scoring
from speakerverification_amd import _lib
from speakerverification_amd.engine import Engine
from tests import scoring_routes_check as chk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(model="none", max_batch=1)
    yield e
    e.close()


def _profiled(eng, fn):
    """(labels -> launches of the call, its result)"""
    eng.profile(True)
    try:
        out = fn()
        return {k: v["launches"] for k, v in eng.profile_results().items()}, out
    finally:
        eng.profile(False)


def _topk_labels(labels):
    return {k for k in labels if k.startswith("asnorm_topk")}


def _one_float_in(a):
    """a device copy of `a` that starts one float into its buffer: 4-byte aligned, not 16"""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(*a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


# ---- a. the selection kernels of the slab path -------------------------------------------------------------------------------------------
def _check_stats(eng, case, E, C, tops):
    """asnorm_stats of a case at every top: route, form label and both errors against the float64 reference; -> failures"""
    K, D = case["K"], case["D"]
    ref = chk.Reference(E, C)
    form, rpw = chk.topk_form(K)
    bad = []
    for top in tops:
        labels, (mu, sd) = _profiled(eng, lambda: eng.asnorm_stats(E, C, top))
        route = chk.asnorm_route(D, K, top, slab_option=case["slab_option"])
        rmu, rsd = ref.stats(top)
        emu, esd = chk.stat_errors(case["data"], K, top, mu, sd, rmu, rsd, ref.smax)
        fb = eng.asnorm_last_fallback
        print(f"MEASURED {case['id']} top {top} ({'exact' if chk.exact_search(K, top) else 'fast'}) {route} {form} rows_per_wg {rpw}: "
              f"mu {np.abs(mu - rmu).max():.2e} = {emu:.2f} of its bar, sd {np.abs(sd - rsd).max():.2e} = {esd:.2f} of its bar; fallback {fb}")
        if route == "slab":
            if fb != -1 or _topk_labels(labels) != {chk.LABEL[form]}:
                bad.append((top, "route", fb, sorted(labels)))
        elif fb < 0 or "asnorm_fused" not in labels or not _topk_labels(labels) <= {chk.LABEL[form]}:
            bad.append((top, "route", fb, sorted(labels)))
        if not (np.isfinite(mu).all() and np.isfinite(sd).all() and emu <= 1.0 and esd <= 1.0):
            bad.append((top, "error", emu, esd))
    return bad


@pytest.mark.parametrize("case", chk.SELECT_CASES, ids=[c["id"] for c in chk.SELECT_CASES])
def test_selection_forms_of_the_slab_path(eng, case):
    """reg8 | reg24 | lds at 4 / 3 / 2 / 1 rows per workgroup, on both sides of every switch, threshold fast path (top 1, 200, 256) and
    exact search (257, K // 4 + 1, K, -1); D = 192 under option asnorm_slab"""
    E, C = chk.inputs(case)
    eng.set_option("asnorm_slab", int(case["slab_option"]))
    try:
        bad = _check_stats(eng, case, E, C, chk.tops_of(case["K"]))
    finally:
        eng.set_option("asnorm_slab", 0)
    assert not bad, bad


def test_odd_embeddings_reach_the_lds_kernel(eng):
    """the shapes of test_fused_asnorm_hands_odd_embeddings_to_the_slab_path at K = 7000: what the fused kernel hands over is answered by
    the LDS form (a heavy upper tail of 700 near-duplicates; an all-zero embedding: every key equal)"""
    E, C = chk.odd_inputs()
    labels, (mu, sd) = _profiled(eng, lambda: eng.asnorm_stats(E, C, 200))
    rmu, rsd = o_scoring.asnorm_stats(E.astype(np.float64), C.astype(np.float64), 200)
    ok = rsd > 1e-6
    emu, esd = float(np.abs(mu - rmu).max()), float((np.abs(sd - rsd)[ok] / rsd[ok]).max())
    print(f"MEASURED odd K {chk.ODD_K}: mu {emu:.2e}, sd rel {esd:.2e}, zero row sd {np.abs(sd[~ok]).max(initial=0.0):.2e}; "
          f"fallback {eng.asnorm_last_fallback}, labels {sorted(labels)}")
    assert eng.asnorm_last_fallback >= 1 and _topk_labels(labels) == {chk.LABEL["lds"]}
    assert emu <= chk.MU_BAR and esd <= chk.SD_REL_BAR and float(np.abs(sd[~ok]).max(initial=0.0)) <= chk.SD_TOP1_BAR
    # the same rows through the slab path alone: exact search (top = K // 4 + 1) on the heavy tail
    eng.set_option("asnorm_slab", 1)
    try:
        top = chk.ODD_K // 4 + 1
        mu2, sd2 = eng.asnorm_stats(E, C, top)
    finally:
        eng.set_option("asnorm_slab", 0)
    ref = chk.Reference(E, C)
    e2 = chk.stat_errors("unit", chk.ODD_K, top, mu2, sd2, *ref.stats(top), ref.smax)
    print(f"MEASURED odd K {chk.ODD_K} top {top} slab: {e2[0]:.2f}, {e2[1]:.2f} of the bars")
    assert eng.asnorm_last_fallback == -1 and max(e2) <= 1.0


# ---- b. cohorts beyond the LDS limit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", chk.BEYOND_CASES, ids=[c["id"] for c in chk.BEYOND_CASES])
def test_cohorts_beyond_the_lds_limit(eng, case):
    """K = 37 892 and 50 000: rows too long for the LDS are selected from the slab itself.  D = 512: the whole call; D = 192: the fused
    kernel plus the one all-zero embedding it flags (top <= 256), the whole call for a larger top"""
    E, C = chk.inputs(case)
    assert chk.topk_form(case["K"])[0] == "global"
    bad = _check_stats(eng, case, E, C, chk.tops_of(case["K"]))
    assert not bad, bad
    if case["data"] == "unit_zero":
        labels, _ = _profiled(eng, lambda: eng.asnorm_stats(E, C, 200))
        assert eng.asnorm_last_fallback >= 1 and _topk_labels(labels) == {chk.LABEL["global"]}, (eng.asnorm_last_fallback, sorted(labels))


def test_census_of_the_selection_forms(eng):
    """the tables reach all four forms on the device (by their profile labels) and all four rows_per_wg values of the LDS form"""
    rng = np.random.Generator(np.random.PCG64(5))
    E = chk.unit_rows(rng, 2, 64)
    seen, rpws = set(), set()
    for K in sorted({c["K"] for c in chk.SELECT_CASES + chk.BEYOND_CASES}):
        labels, _ = _profiled(eng, lambda: eng.asnorm_stats(E, chk.unit_rows(rng, K, 64), 1))
        got = _topk_labels(labels)
        form, rpw = chk.topk_form(K)
        assert got == {chk.LABEL[form]}, (K, got)
        seen |= got
        if form == "lds":
            rpws.add(rpw)
    print("MEASURED census", sorted(seen), sorted(rpws))
    assert seen == set(chk.LABEL.values()) and rpws == {1, 2, 3, 4}


# ---- c. two slabs ------------------------------------------------------------------------------------------------------------------------
def test_the_slab_loop_makes_a_second_trip():
    """N = slab_rows + 5 at K = 37 888: two trips of the slab loop (outputs at dM + r0, operands at dE + r0 D); the rows on both sides of
    the seam against float64; the 2 GiB slab is released after the call, and a second call gives the same bits"""
    t = chk.TWO_SLAB
    K, D, top = t["K"], t["D"], t["top"]
    rows = chk.slab_rows(10 ** 9, K)
    assert rows == 14169
    N = rows + t["extra"]
    assert chk.slab_rows(N, K) == rows and rows * chk.kp(K) * 4 > chk.BIG_SCRATCH
    eng = Engine(model="none", max_batch=1)
    try:
        g = torch.Generator(device="cuda").manual_seed(11)
        E = torch.randn((N, D), generator=g, device="cuda")
        C = torch.randn((K, D), generator=g, device="cuda")
        eng.l2norm_(E)
        eng.l2norm_(C)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        labels, (mu, sd) = _profiled(eng, lambda: eng.asnorm_stats(E, C, top))
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        assert eng.asnorm_last_fallback == -1 and labels.get(chk.LABEL["lds"]) == 2 and labels.get("asnorm_cohort_gemm") == 2, labels
        idx = [0, rows - 1, rows, N - 1]
        rmu, rsd = o_scoring.asnorm_stats(E[idx].cpu().numpy().astype(np.float64), C.cpu().numpy().astype(np.float64), top)
        emu = float(np.abs(mu[idx].cpu().numpy() - rmu).max())
        esd = float(np.abs(sd[idx].cpu().numpy() - rsd).max() / rsd.min())
        print(f"MEASURED two slabs N {N}: mu {emu:.2e}, sd rel {esd:.2e}; free memory before {free0 >> 20} MiB, after {free1 >> 20} MiB")
        assert emu <= chk.MU_BAR and esd <= chk.SD_REL_BAR
        assert bool(torch.isfinite(mu).all()) and bool(torch.isfinite(sd).all())
        assert free0 - free1 < (1 << 30), "the slab (2 GiB) is still held by the handle"
        mu2, sd2 = eng.asnorm_stats(E, C, top)
        assert torch.equal(mu2.view(torch.int32), mu.view(torch.int32)) and torch.equal(sd2.view(torch.int32), sd.view(torch.int32))
    finally:
        eng.close()


# ---- d. score_matrix by route ------------------------------------------------------------------------------------------------------------
def _tiled_sweep(eng, D, Na, Nb, unaligned):
    bad = []
    for sa in chk.MAGS:
        for sb in chk.MAGS:
            A, B = chk.matrix_inputs(Na, Nb, D, sa, sb)
            a, b = (_one_float_in(A), _one_float_in(B)) if unaligned else (A, B)
            labels, got = _profiled(eng, lambda: _host(eng.score_matrix(a, b)))
            err = chk.matrix_error(got, A, B)
            inside = chk.in_tiled_range(sa, sb)
            print(f"MEASURED tiled D {D} {Na} x {Nb} |a| {sa:g} |b| {sb:g}: {err:.2e} of |a||b| ({'inside' if inside else 'outside'} the stated range)")
            # split_words runs for the tiled route only (api_scoring.hip::split_b: the row-streaming kernel fills its planes in its own launch)
            if "split_words" not in labels:
                bad.append((sa, sb, "route", sorted(labels)))
            if not np.isfinite(got).all() or (inside and err > chk.TILED_BAR):
                bad.append((sa, sb, err))
            if not inside:
                eng.set_option("score_f32mfma", 1)
                try:
                    e32 = chk.matrix_error(_host(eng.score_matrix(a, b)), A, B)
                finally:
                    eng.set_option("score_f32mfma", 0)
                if e32 > chk.F32MFMA_BAR:
                    bad.append((sa, sb, "f32mfma", e32))
            # which GEMM ran inside the route shows at the smallest norm: the split form far above the fp32 MFMA's error, and only there
            if sa == sb == chk.SPLIT_PROOF_NORM and (err > chk.SPLIT_PROOF_ERR) != chk.split_form_taken(Na, Nb, not unaligned):
                bad.append((sa, sb, "form", err))
    return bad


@pytest.mark.parametrize("Na,Nb", chk.ALL_SIZES)
@pytest.mark.parametrize("D", chk.TILED_WIDTHS)
def test_tiled_split_gemm_by_magnitude(eng, D, Na, Nb):
    """the tiled split GEMM at widths 64 / 320 / 512, operands of row norm 1e-3 .. 3e4: 1e-6 of |a||b| inside the range the header states;
    outside it a finite answer, and option score_f32mfma serves the same operands at its own bar.  129 x 64 and 70 x 132 run the split form,
    the other sizes the fp32 MFMA inside the same route; the error at norm 1e-3 shows which"""
    bad = _tiled_sweep(eng, D, Na, Nb, unaligned=False)
    assert not bad, bad


@pytest.mark.parametrize("Na,Nb", chk.ALL_SIZES)
@pytest.mark.parametrize("D", chk.UNALIGNED_WIDTHS)
def test_unaligned_operands_take_the_tiled_route(eng, D, Na, Nb):
    """D = 192 / 256 with device operands one float into their buffers: the tiled route (its split_words launch; the GEMM itself is the
    fp32 MFMA, the split form wanting 16-byte rows), same bars; the same operands on a 16-byte boundary take the row-streaming kernel
    (no split_words launch)"""
    bad = _tiled_sweep(eng, D, Na, Nb, unaligned=True)
    assert not bad, bad
    A, B = chk.matrix_inputs(Na, Nb, D, 1.0, 1.0)
    labels, got = _profiled(eng, lambda: _host(eng.score_matrix(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda())))
    assert "split_words" not in labels and chk.matrix_error(got, A, B) <= chk.H3W_BAR


@pytest.mark.parametrize("D", chk.TILED_WIDTHS + chk.UNALIGNED_WIDTHS)
def test_option_score_f32mfma_serves_every_width_and_magnitude(eng, D):
    """option score_f32mfma: the exact fp32 MFMA at every width, row norms 1e-6 .. 3e5.  The half-plane test's 2e-7 of |a||b| is not
    met (2.75e-7 at D = 64, 2.59e-7 at 256, at unrelated magnitudes: the rounding of an fp32 sum, not a range effect), so the bar is
    twice the worst figure measured against float64 (scoring_routes_check.F32MFMA_BAR = 5.5e-7)"""
    eng.set_option("score_f32mfma", 1)
    worst, bad = 0.0, []
    try:
        for Na, Nb in chk.SIZES:
            for sa in chk.MAGS + chk.F32_EXTRA_MAGS:
                for sb in chk.MAGS + chk.F32_EXTRA_MAGS:
                    A, B = chk.matrix_inputs(Na, Nb, D, sa, sb)
                    labels, got = _profiled(eng, lambda: eng.score_matrix(A, B))
                    err = chk.matrix_error(got, A, B)
                    worst = max(worst, err)
                    if "split_words" in labels or not np.isfinite(got).all() or err > chk.F32MFMA_BAR:
                        bad.append((Na, Nb, sa, sb, err, sorted(labels)))
    finally:
        eng.set_option("score_f32mfma", 0)
    print(f"MEASURED f32mfma D {D}: worst {worst:.2e} of |a||b|")
    assert not bad, bad


def test_option_score_f32mfma_through_asnorm_stats_and_score_topk(eng):
    """one row each: the slab path of asnorm_stats and score_topk at D = 320 under the option"""
    case = dict(id="f32mfma-D320-K2049", D=320, K=2049, N=33, data="unit", slab_option=False)
    E, C = chk.inputs(case)
    eng.set_option("score_f32mfma", 1)
    try:
        labels, (mu, sd) = _profiled(eng, lambda: eng.asnorm_stats(E, C, 200))
        l2, (sc, ix) = _profiled(eng, lambda: eng.score_topk(E, C, 10))
    finally:
        eng.set_option("score_f32mfma", 0)
    ref = chk.Reference(E, C)
    emu, esd = chk.stat_errors("unit", 2049, 200, mu, sd, *ref.stats(200), ref.smax)
    S = E.astype(np.float64) @ C.astype(np.float64).T
    named = np.take_along_axis(S, ix.astype(np.int64), axis=1)
    etk = float(np.abs(sc - named).max())
    print(f"MEASURED f32mfma asnorm_stats {emu:.2f}, {esd:.2f} of the bars; score_topk {etk:.2e}; labels {sorted(labels)} {sorted(l2)}")
    assert "split_words" not in labels and "split_words" not in l2 and "score_topk_rows" in l2
    assert emu <= 1.0 and esd <= 1.0 and etk <= 1e-6
    assert float(np.abs(named - ref.sorted[:, :10]).max()) <= 1e-6       # the rows it names are the 10 best to the same bar


@pytest.mark.parametrize("route,Na,Nb", [("split", 129, 64), ("split", chk.RAGGED_SPLIT_SIZE[0], chk.RAGGED_SPLIT_SIZE[1]), ("tiled_fp32", 70, 130),
                                         ("unaligned", 70, 130), ("f32mfma", 70, 130)])
def test_a_non_finite_element_stays_in_its_row_or_column(eng, route, Na, Nb):
    """a NaN element of A, a NaN or inf element of B: its own row / column and nothing else, on the split form of the tiled route (hi | lo
    half words: the lo of an inf is inf - inf), on the fp32 MFMA the route falls to, with unaligned operands and under option score_f32mfma.
    The "split" cases first prove that the split form ran: its error at norm 1e-3 is far above the fp32 MFMA's."""
    D = 192 if route == "unaligned" else 320
    A, B = chk.matrix_inputs(Na, Nb, D, 1.0, 1.0)
    put = _one_float_in if route == "unaligned" else (lambda x: x)
    eng.set_option("score_f32mfma", int(route == "f32mfma"))
    try:
        small = np.float32(chk.SPLIT_PROOF_NORM)
        As, Bs = (A * small).astype(np.float32), (B * small).astype(np.float32)
        labels, gs = _profiled(eng, lambda: _host(eng.score_matrix(put(As), put(Bs))))
        err = chk.matrix_error(gs, As, Bs)
        print(f"MEASURED non-finite {route} {Na} x {Nb}: {err:.2e} of |a||b| at norm {chk.SPLIT_PROOF_NORM:g}; labels {sorted(labels)}")
        assert ("split_words" in labels) == (route != "f32mfma")
        assert (err > chk.SPLIT_PROOF_ERR) == (route == "split") == (route != "f32mfma" and chk.split_form_taken(Na, Nb, route != "unaligned"))
        got = _host(eng.score_matrix(put(A), put(B)))
        A2 = A.copy(); A2[3, 5] = np.nan
        g2 = _host(eng.score_matrix(put(A2), put(B)))
        assert np.isnan(g2[3]).all() and np.array_equal(np.delete(g2, 3, axis=0), np.delete(got, 3, axis=0))
        for badv in (np.nan, np.inf):
            B2 = B.copy(); B2[11, 2] = badv
            g3 = _host(eng.score_matrix(put(A), put(B2)))
            assert not np.isfinite(g3[:, 11]).any(), badv
            assert np.array_equal(np.delete(g3, 11, axis=1), np.delete(got, 11, axis=1)), badv
    finally:
        eng.set_option("score_f32mfma", 0)


def test_a_width_that_is_no_multiple_of_32_is_refused_before_any_launch(eng):
    rng = np.random.Generator(np.random.PCG64(3))
    A, B = chk.unit_rows(rng, 9, chk.REFUSED_WIDTH), chk.unit_rows(rng, 70, chk.REFUSED_WIDTH)
    for call in (lambda: eng.score_matrix(A, B), lambda: eng.asnorm_stats(A, B, 20), lambda: eng.score_topk(A, B, 5)):
        eng.profile(True)
        try:
            with pytest.raises(_lib.SvhipError) as ei:
                call()
            assert ei.value.code == chk.ERR_UNSUPPORTED and "multiple of 32" in str(ei.value)
            assert eng.profile_results() == {}
        finally:
            eng.profile(False)


# ---- e. unaligned operands elsewhere -----------------------------------------------------------------------------------------------------
def test_unaligned_operands_through_asnorm_stats_and_score_topk(eng):
    """device views one float in, D = 192: asnorm_stats takes the slab path as a whole, score_topk its slab route; the slab bars"""
    case = dict(id="unaligned-D192-K5994", D=192, K=5994, N=130, data="unit", slab_option=False)
    E, C = chk.inputs(case)
    Ed, Cd = _one_float_in(E), _one_float_in(C)
    labels, (mu, sd) = _profiled(eng, lambda: eng.asnorm_stats(Ed, Cd, 200))
    ref = chk.Reference(E, C)
    emu, esd = chk.stat_errors("unit", 5994, 200, _host(mu), _host(sd), *ref.stats(200), ref.smax)
    print(f"MEASURED unaligned asnorm_stats: {emu:.2f}, {esd:.2f} of the bars; labels {sorted(labels)}")
    assert eng.asnorm_last_fallback == -1 and _topk_labels(labels) == {chk.LABEL["reg24"]} and "split_words" in labels
    assert emu <= 1.0 and esd <= 1.0
    l2, (sc, ix) = _profiled(eng, lambda: eng.score_topk(Ed, Cd, 10))
    assert {"score_topk_gemm", "score_topk_rows"} <= set(l2) and "score_topk" not in l2 and "score_topk_merge" not in l2, sorted(l2)
    S = E.astype(np.float64) @ C.astype(np.float64).T
    named = np.take_along_axis(S, _host(ix).astype(np.int64), axis=1)
    assert float(np.abs(_host(sc) - named).max()) <= 1e-6 and float(np.abs(named - ref.sorted[:, :10]).max()) <= 1e-6


def _pair_data(D, N=257, P=1000):
    rng = np.random.Generator(np.random.PCG64(D))
    E = (rng.standard_normal((N, D)) * 3.0).astype(np.float32)
    ia, ib = rng.integers(0, N, P).astype(np.int32), rng.integers(0, N, P).astype(np.int32)
    mu = rng.uniform(-0.2, 0.2, N).astype(np.float32)
    sg = rng.uniform(0.5, 1.5, N).astype(np.float32)
    s = np.sum(E[ia].astype(np.float64) * E[ib].astype(np.float64), axis=1)
    want_as = 0.5 * ((s - mu[ia]) / sg[ia].astype(np.float64) + (s - mu[ib]) / sg[ib].astype(np.float64))
    return E, ia, ib, mu, sg, o_scoring.cosine_pairs(E, ia, ib), want_as, float(np.abs(s).max())


@pytest.mark.parametrize("D", [192, 320, 512])
def test_pair_kernels_on_an_unaligned_embedding_matrix(eng, D):
    """score_pairs / asnorm_pairs with E one float into its buffer (element loads: pair_kernel looks at the base address as well as at
    D % 4) against float64, 1e-5 (asnorm_pairs: of the largest raw score, its statistics being inputs of order 1)"""
    E, ia, ib, mu, sg, want_cos, want_as, smax = _pair_data(D)
    dev = lambda x: torch.from_numpy(x).cuda()
    for Ed in (_one_float_in(E), dev(E)):
        assert chk.pair_vector_loads(D, Ed.data_ptr() % 16 == 0) == (Ed.data_ptr() % 16 == 0)
        got = _host(eng.score_pairs(Ed, dev(ia), dev(ib)))
        gas = _host(eng.asnorm_pairs(Ed, dev(mu), dev(sg), dev(ia), dev(ib)))
        ec, ea = float(np.abs(got - want_cos).max()), float(np.abs(gas - want_as).max() / max(1.0, smax))
        print(f"MEASURED pairs D {D} base % 16 = {Ed.data_ptr() % 16}: cosine {ec:.2e}, asnorm {ea:.2e}")
        assert ec <= 1e-5 and ea <= 1e-5


@pytest.mark.parametrize("D", [1, 30])
def test_pair_kernels_scalar_path(eng, D):
    """widths that are no multiple of 4: element loads, aligned operands"""
    E, ia, ib, mu, sg, want_cos, want_as, smax = _pair_data(D)
    assert not chk.pair_vector_loads(D, True)
    ec = float(np.abs(eng.score_pairs(E, ia, ib) - want_cos).max())
    ea = float(np.abs(eng.asnorm_pairs(E, mu, sg, ia, ib) - want_as).max() / max(1.0, smax))
    print(f"MEASURED pairs D {D}: cosine {ec:.2e}, asnorm {ea:.2e}")
    assert ec <= 1e-5 and ea <= 1e-5
