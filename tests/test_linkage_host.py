"""CPU: the statement of svhip_cluster_linkage (tests/linkage_statement.py) decides every case the GPU tests compare exactly, agrees with
scipy where scipy's answer is unique, and nests as the theory says; the header, the binding and the Python surface carry the call."""
import os
import re
import warnings

import numpy as np
import pytest
from scipy.cluster.hierarchy import fcluster, linkage as scipy_linkage
from scipy.spatial.distance import squareform

from speakerverification_amd import _lib, scoring
from tests import cluster_statement as cs
from tests import linkage_statement as ls
from tests.test_engine_calls_host import P, _arrays, _engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (192, 256, 64)


@pytest.fixture(scope="module")
def results():
    """(D, norm, name, linkage) -> (case, statement): computed once for the whole file"""
    out = {}
    for D in WIDTHS:
        for norm in (False, True):
            for name, case in ls.cases(D, _lib.LINKAGE_LDS_ROWS, norm).items():
                for linkage in case[3]:
                    out[D, norm, name, linkage] = (case, ls.statement(case[0], case[1], case[2], linkage, exact=case[4]))
    return out


def test_no_decision_of_any_case_lies_within_its_bar(results):
    assert len(results) >= 6 * 11
    for key, (_, st) in results.items():
        assert st[3] == 0, (key, st[3])
        assert st[4] == 0, key
    # the float cases keep a real distance: the closest decision is at least 1.7 bars away
    closest = {key: st[5] for key, (case, st) in results.items() if not case[4]}
    print({k: round(float(v), 2) for k, v in closest.items()})
    assert min(closest.values()) > 1.5


def test_the_larger_bridge_sets_are_not_decided(results):
    """why tests/test_gpu_linkage.py compares only order-independent properties at 129 and 209 rows"""
    undecided = [ls.statement(*ls.bridge_rows(192, ls.BRIDGE_SEED, per=per)[:2], None, "average")[3] for per in (60, 100)]
    assert all(u > 0 for u in undecided), undecided


def _scipy_labels(E, thr, stats, method):
    """fcluster(linkage(1 - V), 1 - thr) per single-linkage component would be the same partition; here on the whole set, as a user would"""
    V = cs.scores64(E, stats)
    top = float(np.nanmax(V)) + 1.0
    dist = top - V
    np.fill_diagonal(dist, 0.0)
    Z = scipy_linkage(squareform(dist, checks=False), method)
    return fcluster(Z, top - thr, "distance")


def test_statement_equals_scipy_on_the_tie_free_float_cases(results):
    seen = 0
    for (D, norm, name, linkage), (case, st) in results.items():
        if case[4]:
            continue                                                     # (exact data is full of ties, which scipy breaks its own way)
        seen += 1
        want = cs.canonical(_scipy_labels(case[0], case[1], case[2], linkage))
        assert np.array_equal(st[0], want[0]) and st[2] == want[2], (D, norm, name, linkage)
    assert seen >= 2 * (3 * 2 + 3)


def test_clusters_lie_in_components_and_the_linkages_nest(results):
    for (D, norm, name, linkage), (case, st) in results.items():
        single = cs.statement(case[0], case[1], case[2])
        assert ls.refines(st[0], single[0]), (D, norm, name, linkage)
        if linkage == "complete" and (D, norm, name, "average") in results:
            average = results[D, norm, name, "average"][1]
            assert ls.refines(st[0], average[0]), (D, norm, name)
    # and the refinement is strict where the data was built for it
    for D in WIDTHS:
        assert results[D, False, "bridge_49", "average"][1][2] == 2 and cs.statement(*ls.bridge_rows(D, ls.BRIDGE_SEED)[:2])[2] == 1
        assert results[D, False, "two_level_bridge", "complete"][1][2] > 1


def test_tie_rule_on_a_hand_made_component():
    """four rows, v = 1 between (0, 1), (1, 2), (2, 3) and (0, 2), 0 elsewhere, thr = 1: all ties at 1.  The smallest pair (0, 1) merges
    first; complete linkage then stops ((01, 2) holds the 1 of (1, 2) and the 1 of (0, 2): min 1 -> merges; then (012, 3) holds a 0)."""
    V = np.zeros((4, 4))
    for i, j in ((0, 1), (1, 2), (2, 3), (0, 2)):
        V[i, j] = V[j, i] = 1.0
    lab, und, _ = ls.agglomerate(V, 1.0, "complete", exact=True)
    assert lab.tolist() == [0, 0, 0, 3] and und == 0
    lab, _, _ = ls.agglomerate(V, 1.0, "average", exact=True)
    assert lab.tolist() == [0, 0, 0, 3]                                  # g(012, 3) = 1 / 3
    lab, _, _ = ls.agglomerate(V, 1 / 3, "average", exact=True)
    assert lab.tolist() == [0, 0, 0, 0]
    # NaN counts as -inf and a NaN g is never taken
    V[0, 1] = V[1, 0] = np.nan
    lab, _, _ = ls.agglomerate(V, 1.0, "complete", exact=True)
    assert lab.tolist() == [0, 1, 0, 3]                                  # (0, 2) merges; (02, 1) holds -inf; (02, 3) holds 0


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_call_and_the_binding_carries_it():
    text = open(os.path.join(ROOT, "include", "svhip.h")).read()
    assert re.search(r"int svhip_cluster_linkage\(svhip_handle\* h, const float\* E, int64_t N, int32_t D, float thr,", text)
    assert re.search(r"enum \{ SVHIP_LINKAGE_AVERAGE = 1, SVHIP_LINKAGE_COMPLETE = 2 \};", text)
    assert f"#define SVHIP_LINKAGE_MAX_ROWS {_lib.LINKAGE_MAX_ROWS}" in text and f"#define SVHIP_LINKAGE_LDS_ROWS {_lib.LINKAGE_LDS_ROWS}" in text
    assert (_lib.LINKAGE_AVERAGE, _lib.LINKAGE_COMPLETE) == (1, 2)
    assert "svhip_cluster_linkage" in _lib.exported_symbols()
    assert len(_lib._SIGNATURES["svhip_cluster_linkage"][1]) == 13
    assert hasattr(_lib.load(), "svhip_cluster_linkage")
    assert '"linkage_lds_rows"' in text and "SV_OPT(linkage_lds_rows," in open(os.path.join(ROOT, "speakerverification_amd", "csrc", "api.hip")).read()


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_engine_call_and_its_transfers(kind):
    from speakerverification_amd import engine as sv_engine
    eng, a = _engine(), _arrays(kind)
    before = dict(sv_engine.TRANSFER_STATS)
    root, cluster, n, u = eng.cluster_linkage(a.E, 0.25, a.q_stats, "complete")
    assert eng.lib.calls == [("svhip_cluster_linkage", (None, P, 3, 192, 0.25, P, P, 2, P, P, P, P, 0))]
    assert sv_engine.TRANSFER_STATS["h2d_bytes"] - before["h2d_bytes"] == 2304 + 24
    assert sv_engine.TRANSFER_STATS["d2h_bytes"] - before["d2h_bytes"] == 12 + 12 + 8 + 8
    assert tuple(root.shape) == tuple(cluster.shape) == (3,)
    eng.lib.calls.clear()
    eng.cluster_linkage(a.E, 0.25)
    assert eng.lib.calls == [("svhip_cluster_linkage", (None, P, 3, 192, 0.25, None, None, 1, P, P, P, P, 0))]
    with pytest.raises(ValueError, match="neither"):
        eng.cluster_linkage(a.E, 0.25, None, "single")
    with pytest.raises(ValueError, match="NaN"):
        eng.cluster_linkage(a.E, float("nan"))


def test_scoring_cluster_routes_by_linkage(monkeypatch):
    eng, a = _engine(), _arrays("numpy")
    monkeypatch.setattr(scoring, "scoring_engine", lambda device=0: eng)
    with pytest.raises(ValueError, match="bogus"):
        scoring.cluster(a.E, 0.25, linkage="bogus")
    assert eng.lib.calls == []
    # the default and "single": today's call, argument for argument, and not the new export
    want = [("svhip_cluster_above", (None, P, 3, 192, 0.25, None, None, P, P, P, 0))]
    assert len(scoring.cluster(a.E, 0.25)) == 3 and eng.lib.calls == want
    eng.lib.calls.clear()
    assert len(scoring.cluster(a.E, 0.25, linkage="single")) == 3 and eng.lib.calls == want
    eng.lib.calls.clear()
    assert len(scoring.cluster(a.E, 0.25, stats=a.q_stats, linkage="average")) == 4
    assert eng.lib.calls == [("svhip_cluster_linkage", (None, P, 3, 192, 0.25, P, P, 1, P, P, P, P, 0))]


def test_model_cluster_default_issues_the_same_library_call(tmp_path, monkeypatch):
    from tests.fakes import fake_model_handling
    eng = _engine()
    eng.l2norm_ = lambda E: E
    monkeypatch.setattr(scoring, "scoring_engine", lambda device=0: eng)
    mh, _, _ = fake_model_handling(tmp_path, dim=192)
    E = np.eye(5, 192, dtype=np.float32)
    mh.cluster(embeds=E.copy(), thresh_score=0.25)
    assert eng.lib.calls == [("svhip_cluster_above", (None, P, 5, 192, 0.25, None, None, P, P, P, 0))]
    eng.lib.calls.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                  # (the stand-in writes no count: whatever the buffer held)
        mh.cluster(embeds=E.copy(), thresh_score=0.25, linkage="complete")
    assert eng.lib.calls == [("svhip_cluster_linkage", (None, P, 5, 192, 0.25, None, None, 2, P, P, P, P, 0))]
    with pytest.raises(ValueError, match="bogus"):
        mh.cluster(embeds=E.copy(), thresh_score=0.25, linkage="bogus")
