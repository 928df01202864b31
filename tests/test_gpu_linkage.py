"""GPU: average / complete linkage inside the threshold components (svhip_cluster_linkage, Engine.cluster_linkage, scoring.cluster and
ModelHandling.cluster with a linkage) against its statement.

Statement (svhip.h, tests/linkage_statement.py): the components are cluster_above's; inside one, the two clusters with the largest link
value - ties to the smallest rows - merge while that value is at least thr.  The canonical form leaves no freedom, so the comparisons
are exact, on root, cluster and the count; tests/test_linkage_host.py proves without a GPU that no decision of the cases walked here
lies within its accuracy bar.  D = 192 / 256 with an aligned E: the components come from the fused walk; D = 64 or an unaligned view:
from the slab route.  The matrix of a component lives in LDS up to _lib.LINKAGE_LDS_ROWS rows and in scratch beyond; option
"linkage_lds_rows" = 2 sends every component of three rows or more to scratch."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, engine as sv_engine
from speakerverification_amd.engine import Engine
from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
from tests import cluster_statement as cs
from tests import linkage_statement as ls
from tests.test_gpu_cluster import _off4

pytestmark = pytest.mark.gpu

ROUTES = [(192, False), (256, False), (64, False), (192, True)]
ROUTE_IDS = ["fused192", "fused256", "slab64", "slab192_unaligned"]
routes = pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
norms = pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
LDS_ROWS = _lib.LINKAGE_LDS_ROWS


@pytest.fixture(scope="module")
def eng():
    return Engine(model="none", max_batch=1)


_CASES, _WANT = {}, {}


def _cases(D, norm):
    if (D, norm) not in _CASES:
        _CASES[D, norm] = ls.cases(D, LDS_ROWS, norm)
    return _CASES[D, norm]


def _want(D, norm, name, linkage):
    """the statement of a case, computed once"""
    key = (D, norm, name, linkage)
    if key not in _WANT:
        E, thr, stats, _, exact = _cases(D, norm)[name]
        _WANT[key] = ls.statement(E, thr, stats, linkage, exact=exact)
        assert _WANT[key][3] == 0, key                                   # (the host test's claim, for the very arrays used here)
    return _WANT[key][:3]


def _linkage(eng, E, thr, route, stats=None, linkage="average"):
    """-> (root, cluster, C, n_unrefined) as numpy / int, from host arrays (aligned scratch) or from the unaligned device view"""
    if not route[1]:
        return eng.cluster_linkage(E, thr, stats, linkage)
    st = None if stats is None else tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in stats)
    root, cluster, C, U = eng.cluster_linkage(_off4(E), thr, st, linkage)
    return root.cpu().numpy(), cluster.cpu().numpy(), int(C), int(U)


def _same(got, want):
    root, cluster, C = got[:3]
    assert root.dtype == np.int32 and cluster.dtype == np.int32 and isinstance(C, int)
    return np.array_equal(root, want[0]) and np.array_equal(cluster, want[1]) and C == want[2]


def _walk(eng, route, norm):
    D = route[0]
    got = {}
    for name, (E, thr, stats, linkages, _) in _cases(D, norm).items():
        for linkage in linkages:
            got[name, linkage] = _linkage(eng, E, thr, route, stats, linkage)
            assert got[name, linkage][3] == 0
            assert _same(got[name, linkage], _want(D, norm, name, linkage)), (name, linkage)
    return got


# ---- 1. every case against the statement, both matrix homes -----------------------------------------------------------------------------
def test_the_header_the_binding_and_the_kernel_agree_on_the_caps():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svhip.h")).read()
    assert int(re.search(r"#define SVHIP_LINKAGE_LDS_ROWS (\d+)", text).group(1)) == LDS_ROWS
    assert int(re.search(r"#define SVHIP_LINKAGE_MAX_ROWS (\d+)", text).group(1)) == _lib.LINKAGE_MAX_ROWS == ls.MAX_ROWS


@norms
@routes
def test_cases_against_the_statement(eng, route, norm):
    """Components of 1, 2, 3, 31 .. 33, 63 .. 65 rows (the 64-row work list and its edge), of the LDS cap and one more (the first in
    scratch) and a run of 300 identical rows, on exact data: runs of identical rows (every g = 1), two-level sets (g in {2, 1, 0} at
    any size), two-level sets with a bridge row (the tie rule decides which run the bridge joins, and with it whether the other runs
    of the super-group may follow under complete linkage), integer rows under complete linkage; the small float speaker sets; the
    49-row bridge set.  Then the same calls with every matrix in scratch: the same bits."""
    in_lds = _walk(eng, route, norm)
    eng.set_option("linkage_lds_rows", 2)
    try:
        in_scratch = _walk(eng, route, norm)
    finally:
        eng.set_option("linkage_lds_rows", 0)
    for key, got in in_lds.items():
        assert _same(in_scratch[key], got), key


@routes
def test_bridge_set_single_chains_and_average_does_not(eng, route):
    E, thr, who = ls.bridge_rows(route[0], ls.BRIDGE_SEED)
    single = eng.cluster_above(E, thr)
    assert single[2] == 1                                              # one borderline chain joins the two speakers
    for linkage in ls.LINKAGES:
        root, _, C, _ = _linkage(eng, E, thr, route, None, linkage)
        a, b = root[who == 0], root[who == 1]
        assert (a == a[0]).all() and (b == b[0]).all() and a[0] != b[0], linkage
    root, cluster, C, _ = _linkage(eng, E, thr, route)
    assert C == 2 and sorted(np.bincount(cluster).tolist()) == [24, 25]


# ---- 2. larger float components: what does not depend on the merge order ------------------------------------------------------------------
@pytest.mark.parametrize("per", [60, 100], ids=["129", "209"])
@pytest.mark.parametrize("linkage", ls.LINKAGES)
def test_larger_bridge_sets_order_independent_properties(eng, per, linkage):
    """2 x 60 + 9 and 2 x 100 + 9 rows: merge-order margins fall below the fp32 bar here (the statement's `undecided` is not 0), so
    the labels are not compared.  What holds whatever the order: a cluster lies in one component; no two final clusters of a
    component still have g >= thr + bar in float64 (the stopping rule held); the two speakers end in different clusters.  Both
    matrix homes (209 rows are beyond the LDS cap anyway)."""
    E, thr, who = ls.bridge_rows(192, ls.BRIDGE_SEED, per=per)
    comp = cs.statement(E, thr)[0]
    V = cs.scores64(E)
    vbar = cs.BAR
    for lds_rows in (0, 2):                                            # (0: the default cap)
        eng.set_option("linkage_lds_rows", lds_rows)
        try:
            root, cluster, C, U = eng.cluster_linkage(E, thr, None, linkage)
        finally:
            eng.set_option("linkage_lds_rows", 0)
        assert U == 0 and ls.refines(root, comp)
        a, b = root[who == 0], root[who == 1]
        assert not np.intersect1d(a, b).size
        worst = -np.inf
        for x in range(C):
            for y in range(x + 1, C):
                A, B = np.flatnonzero(cluster == x), np.flatnonzero(cluster == y)
                if comp[A[0]] != comp[B[0]]:
                    continue
                block = V[np.ix_(A, B)]
                g = block.mean() if linkage == "average" else block.min()
                bar = vbar + ((A.size + B.size) * 2.0 ** -24 * np.abs(V).max() if linkage == "average" else 0.0)
                worst = max(worst, g - thr - bar)
        print(f"{linkage} {E.shape[0]} rows: {C} clusters, largest g - thr - bar between final clusters {worst:.3e}")
        assert worst < 0


# ---- 3. edge values ---------------------------------------------------------------------------------------------------------------------
@routes
def test_edge_values(eng, route):
    D = route[0]
    E, _ = cs.int_rows(40, D)
    one = (np.zeros(40, np.int32), np.zeros(40, np.int32), 1)
    for linkage in ls.LINKAGES:
        assert _same(_linkage(eng, E, -np.inf, route, None, linkage), one), linkage      # thr = -inf: one component, merged to one cluster
    # a NaN row and a row whose inf element meets zeros (inf * 0 = NaN) score NaN against everybody: alone, and the others as without them
    E, thr, stats, _, exact = _cases(D, False)["two_level_bridge"]
    N = E.shape[0]
    En = np.concatenate([E, np.zeros((2, D), np.float32)])
    En[:, D // 2] = 0.0                                                 # (no builder row uses the middle coordinate)
    assert np.array_equal(En[:N], E)
    En[N, 0] = np.nan
    En[N + 1, D // 2] = np.inf
    for linkage in ls.LINKAGES:
        want = _want(D, False, "two_level_bridge", linkage)
        got = _linkage(eng, En, thr, route, None, linkage)
        assert got[2] == want[2] + 2 and got[0][N] == N and got[0][N + 1] == N + 1 and np.array_equal(got[0][:N], want[0]), linkage


def test_a_component_beyond_the_row_cap_is_counted_and_left_whole(eng):
    E = np.zeros((_lib.LINKAGE_MAX_ROWS + 1 + 5, 192), np.float32)
    E[:_lib.LINKAGE_MAX_ROWS + 1, 7] = 1.0                               # one row more than the cap, all identical
    E[_lib.LINKAGE_MAX_ROWS + 1:, 9] = 1.0                               # and a component of five behind them
    root, cluster, C, U = eng.cluster_linkage(E, 0.5)
    assert U == 1 and C == 2
    assert not root[:_lib.LINKAGE_MAX_ROWS + 1].any() and (root[_lib.LINKAGE_MAX_ROWS + 1:] == _lib.LINKAGE_MAX_ROWS + 1).all()
    assert np.array_equal(cluster, (root > 0).astype(np.int32))


def test_components_beyond_one_round_of_the_scratch_pool(eng):
    """17 runs of 1 024 identical rows and runs of 700 and 900: 18.7 million matrix floats against a pool of 2^24, so the scratch-home
    components are packed into two rounds - a round of 1, matrices at non-zero places, launches that skip the other round's entries.
    Rows shuffled, so no member list is contiguous.  Every g is exactly 1: each run is one cluster."""
    E, thr, run = ls.identical_runs((_lib.LINKAGE_MAX_ROWS,) * 17 + (700, 900), 192)
    assert int((np.bincount(run).astype(np.int64) ** 2).sum()) > 2 ** 24
    order = np.random.default_rng(3).permutation(E.shape[0])
    E, run = E[order], run[order]
    want = cs.canonical(run)
    for linkage in ls.LINKAGES:
        got = eng.cluster_linkage(E, thr, None, linkage)
        assert got[3] == 0 and _same(got, want), linkage


def test_fill_only_option_merges_nothing(eng):
    E, thr, _, _, _ = _cases(192, False)["two_level_bridge_226"]
    eng.set_option("linkage_fill_only", 1)
    try:
        for lds_rows in (0, 2):
            eng.set_option("linkage_lds_rows", lds_rows)
            root, cluster, C, U = eng.cluster_linkage(E, thr)
            assert C == E.shape[0] and U == 0 and np.array_equal(root, np.arange(C)) and np.array_equal(cluster, np.arange(C))
    finally:
        eng.set_option("linkage_fill_only", 0)
        eng.set_option("linkage_lds_rows", 0)
    assert eng.cluster_linkage(E, thr)[2] == 3


# ---- 4. independence --------------------------------------------------------------------------------------------------------------------
@routes
def test_a_components_labels_do_not_depend_on_the_rest(eng, route):
    D = route[0]
    E, thr, _, _, _ = _cases(D, False)["speakers"]
    for linkage in ls.LINKAGES:
        first = _linkage(eng, E, thr, route, None, linkage)
        assert _same(_linkage(eng, E, thr, route, None, linkage), first)                   # the same bits on every run
        comp = cs.statement(E, thr)[0]
        comps = np.unique(comp)
        # every other component removed
        keep = np.isin(comp, comps[::2])
        assert _same(_linkage(eng, E[keep], thr, route, None, linkage), cs.canonical(first[0][keep]))
        # the components in reverse order (each one's rows still ascending), behind 70 rows nobody is linked to
        order = np.concatenate([np.flatnonzero(comp == c) for c in comps[::-1]])
        far = np.zeros((70, D), np.float32)
        far[np.arange(70), np.arange(70) % D] = 0.25
        got = _linkage(eng, np.concatenate([far, E[order]]), thr, route, None, linkage)
        assert np.array_equal(got[0][:70], np.arange(70))
        assert _same((got[0][70:] - 70, got[1][70:] - 70, got[2] - 70), cs.canonical(first[0][order]))


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------------------------
def test_device_tensors_stay_on_the_device_and_numpy_stays_numpy(eng):
    E, thr, stats, _, _ = _cases(192, True)["speakers"]
    want = _want(192, True, "speakers", "complete")
    got = eng.cluster_linkage(E, thr, stats, "complete")
    assert all(isinstance(x, np.ndarray) for x in got[:2]) and isinstance(got[2], int) and isinstance(got[3], int) and _same(got, want)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Ed, st = dev(E), tuple(dev(x) for x in stats)
    torch.cuda.synchronize()
    before = dict(sv_engine.TRANSFER_STATS)
    root, cluster, C, U = eng.cluster_linkage(Ed, thr, st, "complete")
    assert dict(sv_engine.TRANSFER_STATS) == before
    assert all(torch.is_tensor(x) and x.is_cuda for x in (root, cluster, C, U)) and C.dtype == U.dtype == torch.int64 and C.dim() == U.dim() == 0
    assert _same((root.cpu().numpy(), cluster.cpu().numpy(), int(C)), want) and int(U) == 0
    with pytest.raises(ValueError):
        eng.cluster_linkage(Ed, thr, stats, "complete")                                    # one memory space per call
    with pytest.raises(ValueError, match="neither"):
        eng.cluster_linkage(E, thr, None, "single")


def test_raw_abi_null_outputs_refusals_and_empty_input(eng):
    lib, h = eng.lib, eng.h
    E, thr, _, _, _ = _cases(192, False)["two_level_bridge"]
    N = E.shape[0]
    want = _want(192, False, "two_level_bridge", "average")
    root, n = np.full(N, -7, np.int32), np.full(1, -7, np.int64)
    p = lambda a: a.ctypes.data
    # out_cluster = NULL, out_n_unrefined = NULL
    assert lib.svhip_cluster_linkage(h, p(E), N, 192, thr, None, None, _lib.LINKAGE_AVERAGE, p(root), None, p(n), None, 0) == 0
    assert np.array_equal(root, want[0]) and int(n[0]) == want[2]
    # device pointers, asynchronously
    Ed = torch.from_numpy(E).cuda()
    rd = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    nd = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    flags = _lib.IN_DEVICE | _lib.OUT_DEVICE | _lib.ASYNC
    assert lib.svhip_cluster_linkage(h, Ed.data_ptr(), N, 192, thr, None, None, _lib.LINKAGE_AVERAGE, rd.data_ptr(), None, nd.data_ptr(),
                                     nd.data_ptr() + 8, flags) == 0
    eng.synchronize()
    assert np.array_equal(rd.cpu().numpy(), want[0]) and nd.tolist() == [want[2], 0]
    # refusals: by name, before any copy or launch - the outputs keep their canaries
    root[:], n[:] = -7, -7
    cluster, u = np.full(N, -7, np.int32), np.full(1, -7, np.int64)
    call = lambda N=N, D=192, thr=thr, E=E, linkage=_lib.LINKAGE_AVERAGE, root=root, n=n: lib.svhip_cluster_linkage(
        h, None if E is None else p(E), N, D, thr, None, None, linkage, None if root is None else p(root), p(cluster),
        None if n is None else p(n), p(u), 0)
    for kw, code, text in ((dict(thr=float("nan")), -1, "cluster_linkage: the threshold is NaN"),
                           (dict(D=0), -1, "cluster_linkage: D = 0 must be at least 1"),
                           (dict(D=48), -5, "cluster_linkage: embedding dim 48 must be a multiple of 32"),
                           (dict(N=-1), -1, "cluster_linkage: N = -1 is negative"),
                           (dict(N=2 ** 31), -1, "cluster_linkage: N = 2147483648 is outside"),
                           (dict(E=None), -1, "cluster_linkage: NULL pointer"),
                           (dict(root=None), -1, "cluster_linkage: NULL pointer"),
                           (dict(n=None), -1, "cluster_linkage: NULL pointer"),
                           (dict(linkage=0), -1, "cluster_linkage: linkage = 0 is neither"),
                           (dict(linkage=3), -1, "cluster_linkage: linkage = 3 is neither")):
        rc = call(**kw)
        assert rc == code, kw
        with pytest.raises(_lib.SvhipError, match=text):
            eng._ck(rc)
        assert np.all(root == -7) and np.all(cluster == -7) and n[0] == -7 and u[0] == -7, kw
    # N = 0: OK, both counts 0, nothing else touched
    assert call(N=0, E=None, root=None) == 0 and n[0] == 0 and u[0] == 0 and np.all(cluster == -7)
    r0, c0, C0, U0 = eng.cluster_linkage(E[:0], thr)
    assert r0.shape == c0.shape == (0,) and C0 == 0 and U0 == 0


def test_profile_labels_and_the_unchanged_single_linkage_call(eng):
    E, thr, _, _, _ = _cases(192, False)["two_level_bridge"]
    eng.profile(True)
    try:
        eng.cluster_linkage(E, thr)
        labels = eng.profile_results()
        eng.profile(True)
        eng.cluster_above(E, thr)
        single = eng.profile_results()
    finally:
        eng.profile(False)
    assert {"cluster_init", "cluster_link", "cluster_flatten", "cluster_ids", "linkage_table", "linkage_agglo"} <= set(labels)
    assert "linkage_agglo_pool" not in labels                          # (34 rows: no component can need the scratch pool)
    assert labels["cluster_ids"]["launches"] == 2 and labels["cluster_link"]["launches"] == 1
    assert not [k for k in single if k.startswith("linkage")] and single["cluster_ids"]["launches"] == 1


# ---- 6. model level ---------------------------------------------------------------------------------------------------------------------
def test_model_cluster_with_a_linkage_on_the_bridge_set(tmp_path):
    from tests.test_gpu_e2e import ARGS
    args = dict(ARGS, save_folder=str(tmp_path))
    mh = ModelHandling(WrappedModel(SpeakerEncoder(**args)), **args)
    E, thr, who = ls.bridge_rows(192, ls.BRIDGE_SEED)
    labels, groups = mh.cluster(embeds=E.copy(), thresh_score=thr)
    assert set(labels.tolist()) == {0} and len(groups) == 1            # single linkage: one cluster of 49
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # (nothing unrefined: no warning)
        labels, groups = mh.cluster(embeds=E.copy(), thresh_score=thr, linkage="average")
    want = _want(192, False, "bridge_49", "average")
    assert labels.dtype == np.int32 and labels.tolist() == want[1].tolist() and sorted(len(g) for g in groups) == [24, 25]
    labels, groups = mh.cluster(embeds=E.copy(), thresh_score=thr, linkage="complete", min_size=5)
    wc = _want(192, False, "bridge_49", "complete")
    sizes = np.bincount(wc[1])
    assert (labels >= 0).sum() == sizes[sizes >= 5].sum() and len(groups) == int((sizes >= 5).sum())
    with pytest.raises(ValueError, match="linkage"):
        mh.cluster(embeds=E.copy(), thresh_score=thr, linkage="bogus")


def test_model_cluster_warns_about_unrefined_components(tmp_path):
    from tests.test_gpu_e2e import ARGS
    args = dict(ARGS, save_folder=str(tmp_path))
    mh = ModelHandling(WrappedModel(SpeakerEncoder(**args)), **args)
    E = np.zeros((_lib.LINKAGE_MAX_ROWS + 1, 192), np.float32)
    E[:, 3] = 1.0
    with pytest.warns(RuntimeWarning, match="1 component"):
        labels, groups = mh.cluster(embeds=E, thresh_score=0.5, linkage="average")
    assert not labels.any() and len(groups) == 1
