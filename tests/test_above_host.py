"""CPU: the threshold-search surface without a GPU — svhip_score_above_count / _fill are declared, bound and exported and fail cleanly
without a handle; the Python wrappers refuse bad arguments before anything is launched (no handle exists here: a launch would fail
otherwise); the step between the two calls (the prefix sum and the max_hits refusal) on faked counts; ModelHandling.matches /
duplicates' host logic with the search replaced by the numpy statement of its rule."""
import os
import re

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, scoring
from speakerverification_amd import model as sv_model
from speakerverification_amd.engine import Engine
from tests import fakes
from tests.e2e_data import make_e2e_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("svhip_score_above_count", "svhip_score_above_fill")


def test_score_above_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "svhip.h")).read()
    assert "SVHIP_ABOVE_UPPER = 1" in header and _lib.ABOVE_UPPER == 1
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in EXPORTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.exported_symbols()
        assert hasattr(lib, name)
    assert lib.svhip_abi_version() == 5                     # additive: the ABI version stays
    assert callable(getattr(Engine, "score_above")) and callable(scoring.score_above)
    assert callable(getattr(sv_model.ModelHandling, "matches")) and callable(getattr(sv_model.ModelHandling, "duplicates"))


def test_score_above_fails_cleanly_without_a_handle():
    lib = _lib.load()
    assert lib.svhip_score_above_count(None, None, 0, None, 0, 0, 0.0, None, None, None, None, 0, 0, None, 0) == -1
    q = np.zeros((2, 192), np.float32)
    cnt, rp = np.zeros(2, np.int64), np.zeros(3, np.int64)
    assert lib.svhip_score_above_count(None, q.ctypes.data, 2, q.ctypes.data, 2, 192, 0.5, None, None, None, None, 0, 0, cnt.ctypes.data, 0) == -1
    assert lib.svhip_score_above_fill(None, q.ctypes.data, 2, q.ctypes.data, 2, 192, 0.5, None, None, None, None, 0, 0, rp.ctypes.data, None, None, 0) == -1


def test_wrappers_refuse_before_any_launch():
    """an Engine WITHOUT a handle or a library: whatever got past the argument checks would fail on `self.lib`, not with ValueError"""
    eng = Engine.__new__(Engine)
    Q, G = np.zeros((3, 192), np.float32), np.zeros((5, 192), np.float32)
    qs, gs = (np.zeros(3, np.float32), np.ones(3, np.float32)), (np.zeros(5, np.float32), np.ones(5, np.float32))
    with pytest.raises(ValueError, match="threshold is NaN"):
        eng.score_above(Q, G, float("nan"))
    with pytest.raises(ValueError, match="threshold is NaN"):
        scoring.score_above(Q, G, np.float32("nan"))
    with pytest.raises(ValueError, match="192 wide, the gallery 256"):
        eng.score_above(Q, np.zeros((5, 256), np.float32), 0.5)
    for q_stats, g_stats in ((qs, None), (None, gs)):
        with pytest.raises(ValueError, match="both .* or neither"):
            eng.score_above(Q, G, 0.5, q_stats=q_stats, g_stats=g_stats)
    with pytest.raises(ValueError, match="g_stats: sigma"):
        eng.score_above(Q, G, 0.5, q_stats=qs, g_stats=(gs[0], None))
    with pytest.raises(ValueError, match="q_stats: mu must hold 3"):
        eng.score_above(Q, G, 0.5, q_stats=(qs[0][:2], qs[1]), g_stats=gs)
    with pytest.raises(AttributeError):                    # (the control: good arguments do reach the library)
        eng.score_above(Q, G, 0.5)


def test_row_ptr_and_max_hits_on_faked_counts():
    count = np.array([3, 0, 5, 1], np.int64)
    row_ptr, total = Engine._above_row_ptr(count, max_hits=9)
    assert row_ptr.dtype == np.int64 and row_ptr.tolist() == [0, 3, 3, 8, 9] and total == 9
    with pytest.raises(ValueError, match=r"\b9 hits exceed max_hits = 8\b"):
        Engine._above_row_ptr(count, max_hits=8)
    row_ptr, total = Engine._above_row_ptr(np.zeros(0, np.int64), max_hits=0)
    assert row_ptr.tolist() == [0] and total == 0
    # counts beyond int32 in all: the sum is taken in int64
    big = np.full(3, 2 ** 31 - 1, np.int64)
    with pytest.raises(ValueError, match=str(3 * (2 ** 31 - 1))):
        Engine._above_row_ptr(big, max_hits=2 ** 28)
    # the same step on a torch tensor (what a device-resident call hands over)
    rp_t, total_t = Engine._above_row_ptr(torch.from_numpy(count), max_hits=9)
    assert rp_t.dtype == torch.int64 and rp_t.tolist() == [0, 3, 3, 8, 9] and total_t == 9

    # ... and through score_above itself: a faked library whose count call reports 3 + 0 + 5 hits
    class _Lib:
        def __init__(self):
            self.filled = False

        def svhip_score_above_count(self, h, q, N, g, M, D, thr, a, b, c, d, q_base, mode, out, flags):
            np.ctypeslib.as_array((_lib.C.c_int64 * N).from_address(out))[:] = [3, 0, 5]
            return 0

        def svhip_score_above_fill(self, *args):
            self.filled = True
            return 0

    eng = Engine.__new__(Engine)
    eng.lib, eng.h, eng.on_numeric, eng.device, eng._stream = _Lib(), None, "raise", 0, None
    Q, G = np.zeros((3, 192), np.float32), np.zeros((5, 192), np.float32)
    with pytest.raises(ValueError, match=r"\b8 hits exceed max_hits = 7\b"):
        eng.score_above(Q, G, 0.5, max_hits=7)
    assert not eng.lib.filled                               # refused before the allocation and the second call
    row_ptr, index, score = eng.score_above(Q, G, 0.5, max_hits=8)
    assert eng.lib.filled and row_ptr.tolist() == [0, 3, 3, 8] and index.shape == score.shape == (8,)
    assert index.dtype == np.int32 and score.dtype == np.float32


def _numpy_above(Q, G, thr, cohort=None, top=200, g_stats=None, upper=False, q_base=0, max_hits=2 ** 28, device=0):
    """the statement of score_above (cosine): every pair at or above thr, CSR, ascending index"""
    S = (np.asarray(Q, np.float64) @ np.asarray(G, np.float64).T).astype(np.float32)
    keep = S >= thr
    if upper:
        keep &= np.arange(S.shape[1])[None, :] > (q_base + np.arange(S.shape[0]))[:, None]
    row_ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    n, m = np.nonzero(keep)
    return row_ptr, m.astype(np.int32), S[n, m]


@pytest.fixture
def handler(monkeypatch, tmp_path):
    eng = fakes.FakeScoringEngine()
    monkeypatch.setattr(scoring, "scoring_engine", lambda device=0: eng)
    calls = []

    def above(Q, G, thr, **kw):
        calls.append((np.array(Q), np.array(G), thr, kw))
        return _numpy_above(Q, G, thr, **kw)

    monkeypatch.setattr(scoring, "score_above", above)
    mh = fakes.fake_model_handling(tmp_path)[0]
    return mh, calls


def test_matches_and_duplicates_host_logic(handler, tmp_path):
    mh, calls = handler
    files, _, _ = make_e2e_files(str(tmp_path))
    num_eval, n_class = 3, 4
    per_file = [mh.embed_utterance(f, num_eval=num_eval, normalize=True).numpy() for f in files]
    embeds = np.stack([np.stack(per_file[2 * c:2 * c + 2], 0).mean(axis=0) for c in range(n_class)], -1).astype(np.float32)
    classes = {c: f"spk{c}" for c in range(n_class)}
    gal = fakes.unit(embeds.astype(np.float64).mean(axis=0).T)
    q = fakes.unit(np.stack([fakes.unit(mh.embed_utterance(f, num_eval=num_eval, normalize=False).numpy().astype(np.float64)).mean(axis=0)
                        for f in files]))
    want = q @ gal.T
    thr = float(np.sort(want.ravel())[want.size // 2])       # about half of the pairs match; some files have several matches

    # matches: ONE search call on identify's operands; per file everything at or above thr, best first
    scores, index, names = mh.matches(files, torch.from_numpy(embeds), thr, classes=classes, num_eval=num_eval)
    assert len(calls) == 1 and calls[0][0].shape == (len(files), 16) and calls[0][1].shape == (n_class, 16) and calls[0][2] == thr
    assert np.allclose(np.linalg.norm(calls[0][0], axis=1), 1.0, atol=1e-5) and np.allclose(np.linalg.norm(calls[0][1], axis=1), 1.0, atol=1e-5)
    assert len(scores) == len(index) == len(names) == len(files)
    assert max(len(r) for r in index) >= 2
    for n in range(len(files)):
        order = np.argsort(-want[n], kind="stable")
        keep = [int(m) for m in order if abs(want[n, m] - thr) > 1e-5 and want[n, m] > thr]
        maybe = [int(m) for m in order if abs(want[n, m] - thr) <= 1e-5]
        assert index[n].dtype == np.int32 and scores[n].dtype == np.float32
        assert [m for m in index[n].tolist() if m not in maybe] == keep
        assert np.all(np.diff(scores[n]) <= 0) and np.all(scores[n] >= np.float32(thr))
        assert float(np.abs(scores[n] - want[n, index[n]]).max(initial=0.0)) <= 1e-5
        assert names[n] == [classes[int(m)] for m in index[n]]
    # no names without classes; an unreachable threshold gives empty rows, not an error
    out = mh.matches(files[:2], embeds, 2.0, num_eval=num_eval)
    assert len(out) == 2 and all(len(r) == 0 for r in out[0]) and all(len(r) == 0 and r.dtype == np.int32 for r in out[1])
    with pytest.raises(ValueError):
        mh.matches([], embeds, thr, num_eval=num_eval)
    with pytest.raises(ValueError, match="cohort"):
        mh.matches(files, embeds, thr, num_eval=num_eval, scoring_mode="norm")

    # duplicates: the UPPER self-join in query chunks; classes 1 and 3 enrolled twice as 4 and 5
    calls.clear()
    flat = np.ascontiguousarray(embeds.mean(axis=0).T)
    doubled = np.concatenate([flat, flat[[1, 3]]])
    i, j, s = mh.duplicates(doubled, 0.9999, chunk=4)
    assert [c[3]["q_base"] for c in calls] == [0, 4] and all(c[3]["upper"] for c in calls)
    assert list(zip(i.tolist(), j.tolist())) == [(1, 4), (3, 5)] and np.all(s >= np.float32(0.9999))
    assert i.dtype == np.int32 and j.dtype == np.int32 and s.dtype == np.float32
    i2, j2, s2, pairs = mh.duplicates(doubled, 0.9999, classes=["a", "b", "c", "d", "b2", "d2"])
    assert pairs == [("b", "b2"), ("d", "d2")] and np.array_equal(i2, i) and np.array_equal(j2, j)
