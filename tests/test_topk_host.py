"""CPU: the 1:N identification surface without a GPU — svhip_score_topk is declared, bound and exported and fails cleanly without a
handle; ModelHandling.identify's host logic (the three gallery forms, class names, argument checks) with the search replaced by the
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


def test_score_topk_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "svhip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+svhip_score_topk\s*\(", header)
    assert "svhip_score_topk" in _lib.exported_symbols()
    lib = _lib.load()
    assert hasattr(lib, "svhip_score_topk")
    assert lib.svhip_abi_version() == 5                     # additive: the ABI version stays
    assert callable(getattr(Engine, "score_topk")) and callable(scoring.score_topk)
    assert callable(getattr(sv_model.ModelHandling, "identify"))


def test_score_topk_fails_cleanly_without_a_handle():
    lib = _lib.load()
    assert lib.svhip_score_topk(None, None, 0, None, 0, 0, 0, None, None, 0) == -1
    q = np.zeros((2, 192), np.float32)
    out_s, out_i = np.zeros((2, 1), np.float32), np.zeros((2, 1), np.int32)
    assert lib.svhip_score_topk(None, q.ctypes.data, 2, q.ctypes.data, 2, 192, 1, out_s.ctypes.data, out_i.ctypes.data, 0) == -1


def _numpy_topk(Q, G, k, device=0):
    """the statement of score_topk: inner products, best first, ties to the lower index"""
    S = np.asarray(Q, np.float64) @ np.asarray(G, np.float64).T
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(S, order, axis=1).astype(np.float32), order.astype(np.int32)


@pytest.fixture
def handler(monkeypatch, tmp_path):
    eng = fakes.FakeScoringEngine()
    monkeypatch.setattr(scoring, "scoring_engine", lambda device=0: eng)
    calls = []

    def topk(Q, G, k, device=0):
        calls.append((np.array(Q), np.array(G), k))
        return _numpy_topk(Q, G, k)

    monkeypatch.setattr(scoring, "score_topk", topk)
    mh = fakes.fake_model_handling(tmp_path)[0]
    return mh, calls


def test_identify_host_logic(handler, tmp_path):
    mh, calls = handler
    files, _, _ = make_e2e_files(str(tmp_path))
    num_eval = 3
    # a gallery in prepare('embed')'s layout: (num_eval, nOut, n_class), class c = the mean of files 2c, 2c + 1
    per_file = [mh.embed_utterance(f, num_eval=num_eval, normalize=True).numpy() for f in files]
    n_class = 4
    embeds = np.stack([np.stack(per_file[2 * c:2 * c + 2], 0).mean(axis=0) for c in range(n_class)], -1).astype(np.float32)
    assert embeds.shape == (num_eval, 16, n_class)
    classes = {c: f"spk{c}" for c in range(n_class)}
    gal = fakes.unit(embeds.astype(np.float64).mean(axis=0).T)
    q = fakes.unit(np.stack([fakes.unit(mh.embed_utterance(f, num_eval=num_eval, normalize=False).numpy().astype(np.float64)).mean(axis=0)
                        for f in files]))
    want = q @ gal.T
    order = np.argsort(-want, axis=1, kind="stable")[:, :2]

    # 1. the tensor form, no names: ONE search call for all files, queries and gallery are unit rows
    scores, index = mh.identify(files, torch.from_numpy(embeds), top=2, num_eval=num_eval)
    assert len(calls) == 1 and calls[0][0].shape == (len(files), 16) and calls[0][1].shape == (n_class, 16) and calls[0][2] == 2
    assert np.allclose(np.linalg.norm(calls[0][0], axis=1), 1.0, atol=1e-5) and np.allclose(np.linalg.norm(calls[0][1], axis=1), 1.0, atol=1e-5)
    assert index.dtype == np.int32 and np.array_equal(index, order)
    assert float(np.abs(scores - np.take_along_axis(want, order, axis=1)).max()) <= 1e-5

    # 2. the (n_class, nOut) array form with a sequence of names; the caller's array is left as it was
    flat = np.ascontiguousarray(embeds.mean(axis=0).T)
    keep = flat.copy()
    s2, i2, names = mh.identify(files, flat, classes=[f"spk{c}" for c in range(n_class)], top=2, num_eval=num_eval)
    assert np.array_equal(flat, keep)
    assert np.array_equal(i2, index) and float(np.abs(s2 - scores).max()) <= 1e-6
    assert names == [[classes[int(i)] for i in row] for row in index]

    # 3. the directory prepare('embed') writes; classes.npy is picked up, an explicit mapping wins
    d = tmp_path / "prep"
    d.mkdir()
    torch.save(torch.from_numpy(embeds), d / "embeds.pt")
    s3, i3 = mh.identify(files[0], str(d), top=1, num_eval=num_eval)                    # one source, no classes.npy: no names
    assert s3.shape == (1, 1) and i3[0, 0] == order[0, 0]
    np.save(str(d / "classes.npy"), classes)
    s4, i4, n4 = mh.identify(files[:3], str(d), top=n_class, num_eval=num_eval)
    assert np.array_equal(i4[:, :2], index[:3]) and [r[0] for r in n4] == [classes[int(i)] for i in index[:3, 0]]
    _, _, n5 = mh.identify(files[:3], d, classes={c: f"other{c}" for c in range(n_class)}, top=1, num_eval=num_eval)
    assert n5 == [[f"other{int(i)}"] for i in index[:3, 0]]

    # refusals: top outside [1, n_class], a wrong number of names, a gallery of another width or rank, no source
    for bad in (0, n_class + 1):
        with pytest.raises(ValueError, match=f"top = {bad}"):
            mh.identify(files, embeds, top=bad, num_eval=num_eval)
    with pytest.raises(ValueError):
        mh.identify(files, embeds, classes=["a", "b"], top=1, num_eval=num_eval)
    with pytest.raises(ValueError):
        mh.identify(files, np.zeros((n_class, 8), np.float32), top=1, num_eval=num_eval)
    with pytest.raises(ValueError):
        mh.identify(files, np.zeros(16, np.float32), top=1, num_eval=num_eval)
    with pytest.raises(ValueError):
        mh.identify([], embeds, top=1, num_eval=num_eval)
