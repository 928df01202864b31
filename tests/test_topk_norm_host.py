"""CPU: the AS-normalised 1:N identification surface without a GPU — svhip_score_topk_norm is declared, bound and exported and fails
cleanly without a handle; ModelHandling.identify's host logic for scoring_mode="norm" and thresh_score with the search replaced by the
numpy statement of its rule."""
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


def test_score_topk_norm_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "svhip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+svhip_score_topk_norm\s*\(([^)]*)\)", header)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "Q", "N", "q_mu", "q_sigma", "G", "M", "g_mu", "g_sigma", "D", "k", "out_score",
                                                         "out_index", "flags"]
    assert "svhip_score_topk_norm" in _lib.exported_symbols()
    lib = _lib.load()
    assert hasattr(lib, "svhip_score_topk_norm")
    assert lib.svhip_abi_version() == 5                     # additive: the ABI version stays
    assert callable(getattr(Engine, "score_topk_norm")) and callable(scoring.score_topk_norm)


def test_score_topk_norm_fails_cleanly_without_a_handle():
    lib = _lib.load()
    assert lib.svhip_score_topk_norm(None, None, 0, None, None, None, 0, None, None, 0, 0, None, None, 0) == -1
    q = np.zeros((2, 192), np.float32)
    st = np.ones(2, np.float32)
    out_s, out_i = np.zeros((2, 1), np.float32), np.zeros((2, 1), np.int32)
    assert lib.svhip_score_topk_norm(None, q.ctypes.data, 2, st.ctypes.data, st.ctypes.data, q.ctypes.data, 2, st.ctypes.data, st.ctypes.data,
                                     192, 1, out_s.ctypes.data, out_i.ctypes.data, 0) == -1


def _stats64(E, cohort, top):
    """utils.py:142-146 in float64: the `top` largest cohort scores of every row, population mean and deviation"""
    S = -np.sort(-(np.asarray(E, np.float64) @ np.asarray(cohort, np.float64).T), axis=1)[:, :top]
    return S.mean(axis=1), S.std(axis=1)


def _numpy_topk_norm(Q, G, k, cohort, top=200, g_stats=None, device=0):
    """the statement of score_topk_norm in float64: 0.5*((s-mu_q)/sd_q + (s-mu_g)/sd_g), best first, ties to the lower index"""
    mq, sq = _stats64(Q, cohort, top)
    mg, sg = _stats64(G, cohort, top) if g_stats is None else g_stats
    S = np.asarray(Q, np.float64) @ np.asarray(G, np.float64).T
    T = 0.5 * ((S - mq[:, None]) / sq[:, None] + (S - mg[None, :]) / sg[None, :])
    order = np.argsort(-T, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(T, order, axis=1).astype(np.float32), order.astype(np.int32), (mg, sg)


def _numpy_topk(Q, G, k, device=0):
    S = np.asarray(Q, np.float64) @ np.asarray(G, np.float64).T
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(S, order, axis=1).astype(np.float32), order.astype(np.int32)


@pytest.fixture
def handler(monkeypatch, tmp_path):
    eng = fakes.FakeScoringEngine()
    monkeypatch.setattr(scoring, "scoring_engine", lambda device=0: eng)
    calls = []

    def topk(Q, G, k, device=0):
        calls.append(("cosine", np.array(Q), np.array(G), k))
        return _numpy_topk(Q, G, k)

    def topk_norm(Q, G, k, cohort, top=200, g_stats=None, device=0):
        calls.append(("norm", np.array(Q), np.array(G), k, np.array(cohort), top))
        return _numpy_topk_norm(Q, G, k, cohort, top, g_stats)

    monkeypatch.setattr(scoring, "score_topk", topk)
    monkeypatch.setattr(scoring, "score_topk_norm", topk_norm)
    mh = fakes.fake_model_handling(tmp_path)[0]
    return mh, calls


def test_identify_norm_host_logic(handler, tmp_path):
    mh, calls = handler
    files, _, _ = make_e2e_files(str(tmp_path))
    num_eval, n_class, top_c = 3, 4, 5
    per_file = [mh.embed_utterance(f, num_eval=num_eval, normalize=True).numpy() for f in files]
    embeds = np.stack([np.stack(per_file[2 * c:2 * c + 2], 0).mean(axis=0) for c in range(n_class)], -1).astype(np.float32)
    names = [f"spk{c}" for c in range(n_class)]
    cohort = fakes.unit(np.random.default_rng(3).standard_normal((12, 16))).astype(np.float32)
    gal = fakes.unit(embeds.astype(np.float64).mean(axis=0).T)
    q = fakes.unit(np.stack([fakes.unit(mh.embed_utterance(f, num_eval=num_eval, normalize=False).numpy().astype(np.float64)).mean(axis=0)
                        for f in files]))
    want_s, want_i, _ = _numpy_topk_norm(q, gal, 2, cohort, top_c)

    # default arguments take the plain path, and say so to nobody else
    s0, i0 = mh.identify(files, embeds, top=2, num_eval=num_eval)
    assert [c[0] for c in calls] == ["cosine"]
    sc, ic = mh.identify(files, embeds, top=2, num_eval=num_eval, scoring_mode="cosine", cohorts=cohort)
    assert [c[0] for c in calls] == ["cosine", "cosine"] and np.array_equal(ic, i0) and np.array_equal(sc, s0)

    # norm: ONE normalised search on unit queries and unit gallery rows, with the cohort and cohort_top handed through
    del calls[:]
    s1, i1, n1 = mh.identify(files, embeds, classes=names, top=2, num_eval=num_eval, scoring_mode="norm", cohorts=cohort, cohort_top=top_c)
    assert len(calls) == 1 and calls[0][0] == "norm" and calls[0][3] == 2 and calls[0][5] == top_c
    assert np.allclose(np.linalg.norm(calls[0][1], axis=1), 1.0, atol=1e-5) and np.allclose(np.linalg.norm(calls[0][2], axis=1), 1.0, atol=1e-5)
    assert np.array_equal(calls[0][4], cohort)
    assert i1.dtype == np.int32 and np.array_equal(i1, want_i)
    assert float(np.abs(s1 - want_s).max()) <= 1e-3                        # (float32 embeddings into float64 statistics of 5 scores)
    assert n1 == [[names[int(i)] for i in row] for row in want_i]

    # the cohort as an .npy path, as evaluateFromList takes it
    path = str(tmp_path / "cohorts.npy")
    np.save(path, cohort)
    s2, i2 = mh.identify(files, embeds, top=2, num_eval=num_eval, scoring_mode="norm", cohorts_path=path, cohort_top=top_c)
    assert np.array_equal(i2, i1) and np.array_equal(s2, s1)

    # a missing cohort, a cohort of another width and an unknown mode are refused
    with pytest.raises(ValueError, match="cohort"):
        mh.identify(files, embeds, top=2, num_eval=num_eval, scoring_mode="norm")
    with pytest.raises(ValueError):
        mh.identify(files, embeds, top=2, num_eval=num_eval, scoring_mode="norm", cohorts=np.zeros((12, 8), np.float32))
    with pytest.raises(ValueError, match="scoring_mode"):
        mh.identify(files, embeds, top=2, num_eval=num_eval, scoring_mode="pnorm", cohorts=cohort)

    # thresh_score, either mode: entries below it get -1 / None, the scores stay as computed
    for mode, s_ref, i_ref in (("norm", s1, i1), ("cosine", s0, i0)):
        r = int(np.argmax(s_ref[:, 0] - s_ref[:, 1]))
        thr = float(0.5 * (s_ref[r, 0].astype(np.float64) + s_ref[r, 1]))
        s3, i3, n3 = mh.identify(files, embeds, classes=names, top=2, num_eval=num_eval, scoring_mode=mode, cohorts=cohort, cohort_top=top_c,
                                 thresh_score=thr)
        assert np.array_equal(s3, s_ref) and i3.dtype == np.int32
        assert np.array_equal(i3, np.where(s_ref < thr, -1, i_ref))
        assert i3[r, 0] == i_ref[r, 0] and i3[r, 1] == -1
        assert n3 == [[names[int(i)] if i >= 0 else None for i in row] for row in i3]
    # a threshold above every score: nobody is identified
    _, i4 = mh.identify(files, embeds, top=2, num_eval=num_eval, thresh_score=2.0)
    assert np.all(i4 == -1)
