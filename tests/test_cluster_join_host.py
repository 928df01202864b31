"""CPU: two-set clustering (svhip_cluster_join, Engine.cluster_join, scoring.cluster_join, ModelHandling.cluster_extend) without a GPU -
the float64 join statement against cluster_statement's on every split the GPU test runs, the data's distance from its thresholds, the
seed clamp, label-to-root conversion, the wrappers' refusals, the Engine call over a recording library and cluster_extend over a
stand-in engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, scoring
from speakerverification_amd import engine as sv_engine
from speakerverification_amd import model as sv_model
from speakerverification_amd.engine import Engine
from tests import cluster_join_statement as cj
from tests import cluster_statement as cs
from tests import fakes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (192, 256, 64, 320, 512)          # the widths of the GPU test's six routes


def _cuts(n):
    return sorted({min(c, n) for c in cj.CUTS})


def _equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_cluster_join_is_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "svhip.h")).read()
    assert re.search(r"\bint\s+svhip_cluster_join\s*\(", text) and "cluster_join :" in text
    assert "svhip_cluster_join" in _lib.exported_symbols()
    lib = _lib.load()
    assert lib.svhip_cluster_join.argtypes[2] is C.c_int64 and lib.svhip_cluster_join.argtypes[5] is C.c_int64 and len(lib.svhip_cluster_join.argtypes) == 17
    assert callable(getattr(Engine, "cluster_join")) and callable(scoring.cluster_join) and callable(getattr(sv_model.ModelHandling, "cluster_extend"))
    assert re.search(r"SVHIP_ABI_VERSION\s+5\b", text)                       # the ABI version stays


def test_seed_clamp_on_the_host():
    """The one clamp function of the seed kernel and of the host check (csrc/kernels.h, cluster_seed_parent), exercised by
    svhip_selftest on the CPU: whatever the entry, the result lies in [0, i] - the forest's climbs end on nothing else.  The
    statement's own clamp says the same."""
    assert _lib.load().svhip_selftest() == 0
    seed = np.array([0, 5, -1, 3, 2, 2 ** 31 - 1, -2 ** 31, 7], np.int64)
    got = cj.clamp(seed)
    assert got.tolist() == [0, 1, 2, 3, 2, 5, 6, 7] and np.all(got <= np.arange(8)) and np.all(got >= 0)


# ---- the statement: every split equals the whole ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_every_split_of_every_shape_is_the_whole(D):
    """For every data set of the GPU test's split cases and every cut: the join statement equals cluster_statement's on the
    concatenation in all three seed modes, that is the labelling the shape has by construction, and no pair lies within the fp32 bar of
    thr - so the GPU comparison may be exact."""
    for name, (E, thr, lab) in cj.split_cases(D).items():
        whole = cs.statement(E, thr)
        assert _equal(whole, cs.canonical(lab)) and cs.undecided(E, thr) == 0, name
        for NA in _cuts(E.shape[0]):
            for mode in cj.MODES:
                ra, rb = cj.seeds(E, NA, thr, mode)
                assert _equal(cj.join_statement(E[:NA], E[NA:], thr, ra, rb), whole), (name, NA, mode)


@pytest.mark.parametrize("D", (192, 64))
def test_chunk_case_and_integer_data(D):
    # the second-chunk case: exact scores 0, 1, 2 at thr = 1 - decided by construction (the labelling is a union-find over coordinates)
    E, thr, lab = cs.shared_coordinate_rows(16384 + 33 + 161, D)
    assert thr == 1.0 and set(np.unique(E)) == {0.0, 1.0} and np.all(E.sum(axis=1) == 2.0)      # every score is 0, 1 or 2 on every route
    for NA in (16417, 161):                               # both cuts leave clusters on either side of the cut
        assert np.intersect1d(lab[:NA], lab[NA:]).size > 0
    head = slice(0, 600)                                  # the labelling rule itself, where the float64 statement is affordable
    assert np.array_equal(cs.statement(E[head], thr)[0], cs.components(600, *np.nonzero(np.triu(E[head] @ E[head].T >= 1.0, 1)))[0])
    # integer rows cut at 139, plain and norm, at the thresholds of tests/test_gpu_cluster.py: exact data, ties AT thr, nothing undecided
    E, stats = cs.int_rows(300, D)
    for st in (None, stats):
        V = cs.scores64(E, st)
        for q in (0.9995, 0.999, 0.99):
            t0 = cs.occurring(V, q)
            for thr in (t0, t0 + (0.125 if st is not None else 0.5)):
                whole = cs.statement(E, thr, st)
                cut = lambda lo, hi: None if st is None else tuple(x[lo:hi] for x in st)
                for mode in cj.MODES:
                    ra, rb = cj.seeds(E, 139, thr, mode, st)
                    got = cj.join_statement(E[:139], E[139:], thr, ra, rb, cut(0, 139), cut(139, None))
                    assert _equal(got, whole), (q, thr, mode)


def test_seeds_are_trusted_and_bridges_merge():
    D = 64
    e = np.eye(8, D, dtype=np.float32)
    A = e[[0, 0, 1, 2]]                                   # rows 0, 1 identical; 2 and 3 orthogonal to everything
    B = e[[5]]
    # identical rows seeded apart stay apart; orthogonal rows seeded together stay together
    got = cj.join_statement(A, B, 0.5, root_a=[0, 1, 2, 2])
    assert got[0].tolist() == [0, 1, 2, 2, 4] and got[2] == 4
    # one B row above thr against two separate A clusters merges them under the smaller root
    bridge = ((e[1] + e[2]) / np.sqrt(2)).astype(np.float32)[None]
    got = cj.join_statement(A, bridge, 0.5, root_a=[0, 1, 2, 3])
    assert got[0].tolist() == [0, 1, 2, 2, 2]
    # a downward chain is its flat form
    chain = cj.join_statement(A, B, 0.5, root_a=[0, 0, 1, 2])
    flat = cj.join_statement(A, B, 0.5, root_a=[0, 0, 0, 0])
    assert _equal(chain, flat) and chain[0].tolist() == [0, 0, 0, 0, 4]


# ---- labels -> roots ----------------------------------------------------------------------------------------------------------------------
def test_label_to_root_conversion():
    for labels, want in (([7, 7, 3, 7, 3, 9], [0, 0, 2, 0, 2, 5]),            # arbitrary values
                         ([5, 1, 5, 0, 1, 0], [0, 1, 0, 3, 1, 3]),            # unsorted: no order among the labels
                         ([0, 1, 2, 3, 9, 9, 0], [0, 1, 2, 3, 4, 4, 0]),      # a first occurrence that comes late
                         ([-4, -4, 2 ** 40, -4], [0, 0, 2, 0]),               # negative and wide labels
                         ([], [])):
        got = scoring.labels_to_roots(np.array(labels, np.int64))
        assert got.dtype == np.int32 and got.tolist() == want
        assert got.tolist() == cj.labels_to_roots(np.array(labels, np.int64)).tolist()
        assert np.all(got <= np.arange(len(labels)))                          # a legal seed
        t = scoring._first_rows_torch(torch.tensor(labels, dtype=torch.int64))    # the device branch's arithmetic, on a CPU tensor
        assert t.dtype == torch.int32 and t.tolist() == want
    rng = np.random.default_rng(5)
    lab = rng.integers(-50, 50, 1000)
    got = scoring.labels_to_roots(lab)
    assert all(got[i] == np.nonzero(lab == lab[i])[0][0] for i in range(1000))
    assert scoring.labels_to_roots(torch.from_numpy(lab)).tolist() == got.tolist()      # a CPU tensor is host data
    with pytest.raises(ValueError, match="labels_a must hold 4"):
        scoring.labels_to_roots(np.arange(3), 4, "labels_a")
    with pytest.raises(ValueError, match="must be integers"):
        scoring.labels_to_roots(np.zeros(3, np.float32))


# ---- refusals before any launch -----------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_before_any_launch(monkeypatch):
    eng = Engine.__new__(Engine)                            # no handle, no library: a call that got past the checks fails on `self.lib`
    monkeypatch.setattr(scoring, "scoring_engine", lambda device=0: eng)
    A, B = np.zeros((3, 192), np.float32), np.zeros((2, 192), np.float32)
    for call in (eng.cluster_join, scoring.cluster_join):
        with pytest.raises(ValueError, match="threshold is NaN"):
            call(A, B, float("nan"))
    with pytest.raises(ValueError, match="A is 192 wide, B 64"):
        eng.cluster_join(A, np.zeros((2, 64), np.float32), 0.5)
    with pytest.raises(ValueError, match="go together"):
        eng.cluster_join(A, B, 0.5, a_stats=(np.zeros(3, np.float32), np.ones(3, np.float32)))
    with pytest.raises(ValueError, match="go together"):
        scoring.cluster_join(A, B, 0.5, b_stats=(np.zeros(2, np.float32), np.ones(2, np.float32)))
    with pytest.raises(ValueError, match="b_stats: sigma must hold 2"):
        eng.cluster_join(A, B, 0.5, a_stats=(np.zeros(3, np.float32), np.ones(3, np.float32)), b_stats=(np.zeros(2, np.float32), np.ones(3, np.float32)))
    with pytest.raises(ValueError, match="root_a must hold 3"):
        eng.cluster_join(A, B, 0.5, root_a=np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="root_b must hold 2"):
        eng.cluster_join(A, B, 0.5, root_b=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="labels_a must hold 3"):
        scoring.cluster_join(A, B, 0.5, labels_a=[0, 1])
    with pytest.raises(ValueError, match="labels_b must be integers"):
        scoring.cluster_join(A, B, 0.5, labels_b=np.zeros(2, np.float32))
    with pytest.raises(AttributeError):                     # (the control: good arguments do reach the library)
        scoring.cluster_join(A, B, 0.5, labels_a=[4, 4, 1])


# ---- the Engine call over a recording library -----------------------------------------------------------------------------------------------
class _RecordingLib:
    def __init__(self):
        self.calls = []

    def svhip_cluster_join(self, *args):
        self.calls.append(tuple("ptr" if isinstance(a, int) and a > 1 << 20 else a for a in args))
        root, cluster, n = args[13], args[14], args[15]
        N = args[2] + args[5]
        np.ctypeslib.as_array((C.c_int32 * N).from_address(root))[:] = [0, 0, 2, 0, 4]
        np.ctypeslib.as_array((C.c_int32 * N).from_address(cluster))[:] = [0, 0, 1, 0, 2]
        np.ctypeslib.as_array((C.c_int64 * 1).from_address(n))[:] = [3]
        return 0


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_engine_call_over_a_recording_library(kind):
    P = "ptr"
    eng = Engine.__new__(Engine)
    eng.lib, eng.h, eng.on_numeric, eng.device, eng._stream = _RecordingLib(), None, "raise", 0, None
    conv = torch.from_numpy if kind == "torch" else (lambda x: x)
    f32 = lambda *s: conv(np.zeros(s, np.float32))
    A, B = f32(3, 192), f32(2, 192)
    ra, rb = conv(np.array([0, 0, 2], np.int32)), conv(np.array([0, 1], np.int32))
    sa, sb = (f32(3), f32(3)), (f32(2), f32(2))
    # sizes: A 3*192*4 = 2304, B 2*192*4 = 1536, root_a 12, root_b 8, a_stats 24, b_stats 16; down: root 20, cluster 20, the count 8
    for kw, want, h2d in ((dict(), (None, P, 3, None, P, 2, None, 192, 0.25, None, None, None, None, P, P, P, 0), 2304 + 1536),
                          (dict(root_a=ra), (None, P, 3, P, P, 2, None, 192, 0.25, None, None, None, None, P, P, P, 0), 2304 + 1536 + 12),
                          (dict(root_b=rb), (None, P, 3, None, P, 2, P, 192, 0.25, None, None, None, None, P, P, P, 0), 2304 + 1536 + 8),
                          (dict(root_a=ra, root_b=rb, a_stats=sa, b_stats=sb), (None, P, 3, P, P, 2, P, 192, 0.25, P, P, P, P, P, P, P, 0),
                           2304 + 1536 + 12 + 8 + 24 + 16)):
        eng.lib.calls.clear()
        before = dict(sv_engine.TRANSFER_STATS)
        root, cluster, n = eng.cluster_join(A, B, 0.25, **kw)
        assert eng.lib.calls == [want], kw
        assert sv_engine.TRANSFER_STATS["h2d_bytes"] - before["h2d_bytes"] == h2d
        assert sv_engine.TRANSFER_STATS["d2h_bytes"] - before["d2h_bytes"] == 20 + 20 + 8
        assert isinstance(root, np.ndarray) and root.dtype == cluster.dtype == np.int32 and root.tolist() == [0, 0, 2, 0, 4]
        assert cluster.tolist() == [0, 0, 1, 0, 2] and n == 3 and isinstance(n, int)
    # a seed of another integer type is converted, not reinterpreted
    eng.lib.calls.clear()
    eng.cluster_join(A, B, 0.25, root_a=np.array([0, 0, 2], np.int64))
    assert eng.lib.calls[0][3] == P


# ---- ModelHandling.cluster_extend over a stand-in engine ----------------------------------------------------------------------------------
class _JoinEngine(fakes.FakeScoringEngine):
    """the scoring engine's part in cluster_extend: answers with the float64 join statement, or with a root array given in advance"""
    def __init__(self):
        self.calls, self.answer = [], None

    def cluster_join(self, A, B, thr, root_a=None, root_b=None, a_stats=None, b_stats=None):
        self.calls.append(dict(A=np.array(A), B=np.array(B), thr=float(thr), root_a=root_a, root_b=root_b, a_stats=a_stats, b_stats=b_stats))
        if self.answer is not None:
            return cs.canonical(self.answer)
        return cj.join_statement(A, B, thr, root_a, root_b, a_stats, b_stats)


@pytest.fixture
def handler(monkeypatch, tmp_path):
    eng = _JoinEngine()
    monkeypatch.setattr(scoring, "scoring_engine", lambda device=0: eng)
    return fakes.fake_model_handling(tmp_path)[0], eng


def test_cluster_extend_argument_rules(handler):
    mh, eng = handler
    gal = np.eye(4, 16, dtype=np.float32)
    with pytest.raises(ValueError, match="exactly one of source"):
        mh.cluster_extend(gal, thresh_score=0.5)
    with pytest.raises(ValueError, match="exactly one of source"):
        mh.cluster_extend(gal, source=["a.wav"], embeds=gal, thresh_score=0.5)
    with pytest.raises(ValueError, match="thresh_score"):
        mh.cluster_extend(gal, embeds=gal)
    with pytest.raises(ValueError, match="cohort"):
        mh.cluster_extend(gal, embeds=gal, thresh_score=0.5, scoring_mode="norm")
    with pytest.raises(ValueError, match="scoring_mode"):
        mh.cluster_extend(gal, embeds=gal, thresh_score=0.5, scoring_mode="pnorm")
    with pytest.raises(ValueError, match="3 base labels for 4 base rows"):
        mh.cluster_extend(gal, [0, 1, 2], embeds=gal, thresh_score=0.5)
    with pytest.raises(ValueError):
        mh.cluster_extend(gal, source=[], thresh_score=0.5)
    with pytest.raises(ValueError, match="wide"):
        mh.cluster_extend(gal, embeds=np.eye(2, 8, dtype=np.float32), thresh_score=0.5)
    assert eng.calls == []                                  # all of it before anything was joined
    assert "single linkage" in sv_model.ModelHandling.cluster_extend.__doc__.lower()


def test_cluster_extend_ids_and_merged(handler):
    mh, eng = handler
    e = np.eye(8, 16, dtype=np.float32)
    base = e[[0, 1, 0, 2, 1]] * 3.0                        # not normalised: prepared as cluster(embeds=) prepares a gallery
    labels = np.array([40, 7, 40, 9, 7])                   # arbitrary, unsorted labels
    new = np.stack([e[2], e[5], (e[0] + e[1]) / np.sqrt(2.0)]).astype(np.float32) * 2.0     # joins 9; alone; bridges 40 and 7
    base_ids, new_ids, merged = mh.cluster_extend(base, labels, embeds=new, thresh_score=0.5)
    assert base_ids.dtype == new_ids.dtype == np.int32
    assert base_ids.tolist() == [0, 0, 0, 1, 0] and new_ids.tolist() == [1, 2, 0] and merged == [[7, 40]]
    call = eng.calls[0]
    assert np.allclose(np.linalg.norm(call["A"], axis=1), 1.0) and np.allclose(np.linalg.norm(call["B"], axis=1), 1.0) and call["thr"] == 0.5
    assert np.asarray(call["root_a"]).tolist() == [0, 1, 0, 3, 1] and call["root_b"] is None and call["a_stats"] is None
    # nothing bridged: merged is empty, and base_labels = None makes every base row its own cluster
    base_ids, new_ids, merged = mh.cluster_extend(base, labels, embeds=new[:2], thresh_score=0.5)
    assert base_ids.tolist() == [0, 1, 0, 2, 1] and new_ids.tolist() == [2, 3] and merged == []
    base_ids, new_ids, merged = mh.cluster_extend(base, None, embeds=new[:2], thresh_score=0.5)
    assert np.asarray(eng.calls[-1]["root_a"]).tolist() == [0, 1, 2, 3, 4]
    assert base_ids.tolist() == [0, 1, 2, 3, 4] and new_ids.tolist() == [3, 5] and merged == []      # identical base rows seeded apart stay apart
    # ids and merged are built from whatever root array the engine returns: three bridged labels and a pair, in order of the cluster id
    eng.answer = np.array([0, 0, 0, 3, 3, 0, 6, 3])
    base_ids, new_ids, merged = mh.cluster_extend(e[:5], [5, 3, 9, 1, 2], embeds=e[5:8], thresh_score=0.5)
    assert base_ids.tolist() == [0, 0, 0, 1, 1] and new_ids.tolist() == [0, 2, 1] and merged == [[3, 5, 9], [1, 2]]
    eng.answer = None
    # norm mode: both sides' statistics come from the cohort and go into the one call
    eng.calls.clear()
    cohort = fakes.unit(np.random.default_rng(3).standard_normal((12, 16))).astype(np.float32)
    mh.cluster_extend(base, labels, embeds=new, thresh_score=-50.0, scoring_mode="norm", cohorts=cohort, cohort_top=5)
    assert len(eng.calls) == 1 and eng.calls[0]["a_stats"][0].shape == (5,) and eng.calls[0]["b_stats"][0].shape == (3,)
