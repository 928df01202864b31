"""CPU: speaker clustering without a GPU — svhip_cluster_above is declared, bound and exported and refuses without a handle; the
statement helper (tests/cluster_statement.py) against scipy's connected components; every data builder of the GPU tests, with its
precondition (no float64 score within the accuracy bar of the threshold); the Python wrappers' refusals before any launch; and
ModelHandling.cluster's argument rules, preparation and min_size renumbering over a stand-in engine."""
import os
import re

import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from speakerverification_amd import _lib, scoring
from speakerverification_amd import model as sv_model
from speakerverification_amd.engine import Engine
from tests import cluster_statement as cs
from tests import fakes
from tests.e2e_data import make_e2e_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cluster_above_is_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svhip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+svhip_cluster_above\s*\(", header)
    assert "svhip_cluster_above" in _lib.exported_symbols()
    lib = _lib.load()
    assert hasattr(lib, "svhip_cluster_above") and lib.svhip_abi_version() == 5        # additive: the ABI version stays
    assert callable(getattr(Engine, "cluster_above")) and callable(scoring.cluster) and callable(getattr(sv_model.ModelHandling, "cluster"))
    e = np.zeros((2, 192), np.float32)
    root, n = np.full(2, -7, np.int32), np.full(1, -7, np.int64)
    assert lib.svhip_cluster_above(None, e.ctypes.data, 2, 192, 0.5, None, None, root.ctypes.data, None, n.ctypes.data, 0) == -1
    assert np.all(root == -7) and n[0] == -7


# ---- the helper against scipy -------------------------------------------------------------------------------------------------------------
def _scipy_components(n, i, j):
    g = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n))
    return connected_components(g, directed=False)


@pytest.mark.parametrize("n,m", [(1, 0), (2, 1), (50, 20), (400, 150), (400, 390), (400, 2000), (3000, 2500)])
def test_helper_against_scipy_on_random_graphs(n, m):
    rng = np.random.default_rng(n + m)
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    i, j = np.minimum(i, j), np.maximum(i, j)
    root, cluster, C = cs.components(n, i, j)
    c_scipy, lab = _scipy_components(n, i, j)
    assert C == c_scipy and root.dtype == cluster.dtype == np.int32
    # the same partition ...
    assert np.array_equal(cs.canonical(lab)[0], root)
    # ... in the canonical form: the root is the smallest member, ids count the roots below, C of them
    for c in range(C):
        members = np.nonzero(cluster == c)[0]
        assert np.all(root[members] == members[0])
    roots = np.unique(root)
    assert np.array_equal(cluster[roots], np.arange(C)) and np.all(np.diff(roots) > 0)
    assert all(np.array_equal(x, y) for x, y in zip(cs.canonical(root)[:2], (root, cluster)))


def test_helper_statement_ignores_nan_and_the_lower_triangle():
    E = np.eye(4, 8, dtype=np.float32)
    E[1] = E[0]
    E[2, 5] = np.nan
    root, cluster, C = cs.statement(E, 0.5)
    assert root.tolist() == [0, 0, 2, 3] and cluster.tolist() == [0, 0, 1, 2] and C == 3
    assert cs.statement(E, -np.inf)[0].tolist() == [0, 0, 2, 0]            # everything finite joins; the NaN row stays alone
    assert cs.statement(E[:0], 0.5)[2] == 0


# ---- the data builders: what they promise, and their precondition -------------------------------------------------------------------------
SIZES = (1, 2, 31, 32, 33, 128, 129, 160, 161, 300)
WIDTHS = (64, 192, 256, 320, 512)


@pytest.mark.parametrize("D", WIDTHS)
def test_graph_shapes_are_decided_in_float64(D):
    for N in SIZES:
        for name, (E, thr, lab) in cs.graph_shapes(N, D).items():
            assert E.shape == (N, D) and E.dtype == np.float32
            assert np.allclose(np.linalg.norm(E.astype(np.float64), axis=1), 1.0, atol=1e-6)
            assert cs.undecided(E, thr) == 0, (name, N)                                  # no pair within the bar of thr
            want = cs.canonical(lab)
            got = cs.statement(E, thr)
            assert all(np.array_equal(a, b) for a, b in zip(got[:2], want[:2])) and got[2] == want[2], (name, N)
    # the margin itself: the nearest scores sit orders of magnitude beyond the bar
    assert min(np.cos(cs.DELTA) - cs.circle_thr(), cs.circle_thr() - np.cos(2 * cs.DELTA)) > 200 * cs.BAR
    E, thr, lab = cs.star(D)
    assert cs.undecided(E, thr) == 0 and cs.statement(E, thr)[2] == 1 and np.all(cs.statement(E, thr)[0] == 0)
    assert int(cs.links64(E, thr).sum()) == E.shape[0] - 1 and np.all(np.nonzero(cs.links64(E, thr))[1] == E.shape[0] - 1)   # only centre links


def test_path_shapes_have_the_depth_they_are_built_for():
    shapes = cs.graph_shapes(300, 192)
    assert cs.statement(*shapes["path"][:2])[2] == 1 and int(cs.links64(*shapes["path"][:2]).sum()) == 299
    i, j = np.nonzero(cs.links64(*shapes["path_reversed"][:2]))
    assert np.array_equal(j - i, np.ones(299, np.int64))                                 # the same chain: hooking it back to front is the hardware's doing
    i, j = np.nonzero(cs.links64(*shapes["path_permuted"][:2]))
    assert i.size == 299 and (j - i).max() > 100
    assert cs.statement(*shapes["two_paths"][:2])[2] == 2
    root, _, C = cs.statement(*shapes["matching"][:2])
    assert C == 150 and np.all(np.bincount(root)[np.unique(root)] == 2)


@pytest.mark.parametrize("D", WIDTHS)
def test_exact_builders(D):
    # shared coordinates: scores 0, 1, 2; the labelling by construction is the statement's at a size where the matrix fits
    E, thr, lab = cs.shared_coordinate_rows(300, D)
    V = cs.scores64(E)
    assert set(np.unique(V)) <= {0.0, 1.0, 2.0} and np.array_equal(V, V.astype(np.float32))
    assert cs.statement(E, thr)[0].tolist() == cs.canonical(lab)[0].tolist()
    E, thr, lab = cs.shared_coordinate_rows(16384 + 33, D)
    C = cs.canonical(lab)[2]
    assert E.shape[0] == 16417 and 1 <= C <= D // 4 and np.all(np.bincount(cs.canonical(lab)[1]) > 32)
    assert int((cs.canonical(lab)[0] < 16384).all())                                    # every row of the second chunk hangs on a row of the first
    # blocks of 40 identical rows
    N = 40 * min(D, 16)
    E, lab = cs.blocks_of_identical_rows(N, D)
    assert cs.statement(E, 1.0)[2] == N // 40 and np.array_equal(cs.statement(E, 1.0)[0], cs.canonical(lab)[0])
    assert cs.undecided(E, 1.0) > 0 and set(np.unique(cs.scores64(E))) == {0.0, 1.0}     # AT the threshold, and exact: >= decides
    # integer rows: exact scores, exact t
    E, stats = cs.int_rows(300, D)
    V, T = cs.scores64(E), cs.scores64(E, stats)
    assert np.array_equal(V, np.round(V)) and np.abs(V).max() <= 4 * D and np.array_equal(T, np.round(4 * T) / 4)
    assert np.array_equal(T.astype(np.float32).astype(np.float64), T)
    for M, q in ((V, 0.999), (T, 0.999)):
        thr = cs.occurring(M, q)
        assert (M[np.triu_indices(300, 1)] == thr).any()                                 # ties at thr exist


def test_speaker_rows_precondition():
    """the agreement test clusters synthetic speaker rows at a threshold between the same-speaker and the different-speaker scores;
    here: what the float64 statement makes of them (GPU test: the library's own pair set gives the same components)"""
    from speakerverification_amd import synth
    E, _, spk = synth.synth_speaker_embeddings(3000, n_speakers=300, dim=192, seed=5)
    root, cluster, C = cs.statement(E, 0.45)
    assert 100 < C < 3000 and np.bincount(cluster).max() >= 3


# ---- the wrappers refuse before any launch ------------------------------------------------------------------------------------------------
def test_wrappers_refuse_before_any_launch():
    eng = Engine.__new__(Engine)                            # no handle, no library: a call that got past the checks fails on `self.lib`
    E = np.zeros((3, 192), np.float32)
    with pytest.raises(ValueError, match="threshold is NaN"):
        eng.cluster_above(E, float("nan"))
    with pytest.raises(ValueError, match="threshold is NaN"):
        scoring.cluster(E, np.float32("nan"))
    with pytest.raises(ValueError, match=r"\(mu, sigma\) pair"):
        eng.cluster_above(E, 0.5, stats=(np.zeros(3, np.float32),))
    with pytest.raises(ValueError, match="stats: sigma must hold 3"):
        eng.cluster_above(E, 0.5, stats=(np.zeros(3, np.float32), np.ones(2, np.float32)))
    with pytest.raises(ValueError, match="stats: mu"):
        eng.cluster_above(E, 0.5, stats=(None, np.ones(3, np.float32)))
    with pytest.raises(AttributeError):                     # (the control: good arguments do reach the library)
        eng.cluster_above(E, 0.5)


def test_engine_call_over_a_faked_library():
    seen = {}

    class _Lib:
        def svhip_cluster_above(self, h, e, N, D, thr, mu, sigma, root, cluster, n, flags):
            seen.update(N=N, D=D, thr=thr, stats=(mu is not None, sigma is not None), flags=flags)
            np.ctypeslib.as_array((_lib.C.c_int32 * N).from_address(root))[:] = [0, 0, 2]
            np.ctypeslib.as_array((_lib.C.c_int32 * N).from_address(cluster))[:] = [0, 0, 1]
            np.ctypeslib.as_array((_lib.C.c_int64 * 1).from_address(n))[:] = [2]
            return 0

    eng = Engine.__new__(Engine)
    eng.lib, eng.h, eng.on_numeric, eng.device, eng._stream = _Lib(), None, "raise", 0, None
    root, cluster, C = eng.cluster_above(np.zeros((3, 192), np.float32), 0.25, stats=(np.zeros(3, np.float32), np.ones(3, np.float32)))
    assert seen == dict(N=3, D=192, thr=0.25, stats=(True, True), flags=0)
    assert root.tolist() == [0, 0, 2] and cluster.tolist() == [0, 0, 1] and C == 2 and isinstance(C, int)
    assert root.dtype == cluster.dtype == np.int32
    eng.cluster_above(np.zeros((3, 192), np.float32), 0.25)
    assert seen["stats"] == (False, False)


# ---- ModelHandling.cluster over a stand-in engine -----------------------------------------------------------------------------------------
class _ClusterEngine(fakes.FakeScoringEngine):
    """the scoring engine's part in ModelHandling.cluster, answered by the float64 statement"""
    def __init__(self):
        self.calls = []

    def cluster_above(self, E, thr, stats=None):
        self.calls.append((np.array(E), float(thr), stats))
        return cs.statement(E, thr, stats)


@pytest.fixture
def handler(monkeypatch, tmp_path):
    eng = _ClusterEngine()
    monkeypatch.setattr(scoring, "scoring_engine", lambda device=0: eng)
    mh = fakes.fake_model_handling(tmp_path)[0]
    return mh, eng


def test_model_cluster_argument_rules(handler):
    mh, eng = handler
    gal = np.eye(4, 16, dtype=np.float32)
    with pytest.raises(ValueError, match="exactly one of source"):
        mh.cluster(thresh_score=0.5)
    with pytest.raises(ValueError, match="exactly one of source"):
        mh.cluster(source=["a.wav"], embeds=gal, thresh_score=0.5)
    with pytest.raises(ValueError, match="thresh_score"):
        mh.cluster(embeds=gal)
    with pytest.raises(ValueError, match="min_size = 0"):
        mh.cluster(embeds=gal, thresh_score=0.5, min_size=0)
    with pytest.raises(ValueError):
        mh.cluster(source=[], thresh_score=0.5)
    with pytest.raises(ValueError, match="cohort"):
        mh.cluster(embeds=gal, thresh_score=0.5, scoring_mode="norm")
    with pytest.raises(ValueError, match="scoring_mode"):
        mh.cluster(embeds=gal, thresh_score=0.5, scoring_mode="pnorm")
    with pytest.raises(ValueError, match="class names"):
        mh.cluster(embeds=gal, thresh_score=0.5, classes=["a", "b"])
    assert eng.calls == []                                  # all of it before anything was clustered


def test_model_cluster_groups_and_min_size(handler, tmp_path):
    mh, eng = handler
    # a gallery: rows 0, 3, 5 one speaker, rows 1, 4 another, rows 2 and 6 alone (orthogonal unit rows, copies score 1)
    owner = np.array([0, 1, 2, 0, 1, 0, 3])
    gal = np.eye(4, 16, dtype=np.float32)[owner] * 3.0     # not normalised: cluster prepares the rows as duplicates does
    labels, groups = mh.cluster(embeds=gal, thresh_score=0.5)
    assert labels.dtype == np.int32 and labels.tolist() == [0, 1, 2, 0, 1, 0, 3]
    assert groups == [[0, 3, 5], [1, 4], [2], [6]]
    assert len(eng.calls) == 1 and np.allclose(np.linalg.norm(eng.calls[0][0], axis=1), 1.0) and eng.calls[0][1] == 0.5 and eng.calls[0][2] is None
    labels, groups = mh.cluster(embeds=gal, thresh_score=0.5, min_size=2, classes=list("abcdefg"))
    assert labels.tolist() == [0, 1, -1, 0, 1, 0, -1] and groups == [["a", "d", "f"], ["b", "e"]]
    labels, groups = mh.cluster(embeds=gal, thresh_score=0.5, min_size=3)
    assert labels.tolist() == [0, -1, -1, 0, -1, 0, -1] and groups == [[0, 3, 5]]
    labels, groups = mh.cluster(embeds=gal, thresh_score=0.5, min_size=4)
    assert labels.tolist() == [-1] * 7 and groups == []
    # a kept cluster behind a dropped one is renumbered in order
    labels, groups = mh.cluster(embeds=gal[[2, 1, 4]], thresh_score=0.5, min_size=2)
    assert labels.tolist() == [-1, 0, 0] and groups == [[1, 2]]
    # the (num_eval, nOut, n_class) form goes through the crop mean, as identify's gallery does
    three = torch.from_numpy(np.stack([gal.T, gal.T]))
    assert mh.cluster(embeds=three, thresh_score=0.5)[0].tolist() == [0, 1, 2, 0, 1, 0, 3]
    # norm mode: the rows' statistics come from the cohort, once, and go into the one call
    eng.calls.clear()
    cohort = fakes.unit(np.random.default_rng(3).standard_normal((12, 16))).astype(np.float32)
    labels, _ = mh.cluster(embeds=gal, thresh_score=-50.0, scoring_mode="norm", cohorts=cohort, cohort_top=5)
    assert len(eng.calls) == 1 and eng.calls[0][2] is not None and eng.calls[0][2][0].shape == (7,)
    assert labels.tolist() == cs.statement(fakes.unit(gal), -50.0, eng.calls[0][2])[1].tolist()


def test_model_cluster_from_files(handler, tmp_path):
    mh, eng = handler
    files, _, _ = make_e2e_files(str(tmp_path))
    num_eval = 3
    q = fakes.unit(np.stack([fakes.unit(mh.embed_utterance(f, num_eval=num_eval, normalize=False).numpy().astype(np.float64)).mean(axis=0) for f in files]))
    S = q @ q.T
    v = np.sort(S[np.triu_indices(len(files), 1)])
    k = int(np.argmax(np.diff(v)))
    thr = float(0.5 * (v[k] + v[k + 1]))                   # the widest gap of the pairs' scores
    assert v[k + 1] - v[k] > 1e-4
    labels, groups = mh.cluster(source=files, thresh_score=thr, num_eval=num_eval)
    assert len(eng.calls) == 1 and eng.calls[0][0].shape == (len(files), 16)
    assert float(np.abs(eng.calls[0][0] - q).max()) <= 1e-5            # identify's preparation of the queries
    root, cluster, C = cs.statement(q, thr)
    assert labels.tolist() == cluster.tolist() and len(groups) == C
    assert groups == [[files[i] for i in np.nonzero(cluster == c)[0]] for c in range(C)]
