"""CPU: the dataset-audit surface without a GPU — svhip_group_audit is declared, bound and exported and fails cleanly without a handle;
audit_cut against the reference's rule restated in float64; the wrappers refuse a bad group_ptr before anything is launched;
ModelHandling.audit's host logic (folder discovery, max_files chunking, the return value, the report text) with the device call
replaced by the numpy statement of its rule."""
import os
import re

import numpy as np
import pytest

from speakerverification_amd import _lib, scoring
from speakerverification_amd import model as sv_model
from speakerverification_amd.engine import Engine
from tests import audit_statement as st
from tests import fakes
from tests.e2e_data import make_e2e_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_audit_is_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svhip.h")).read(), flags=re.S)
    lib = _lib.load()
    assert re.search(r"\bint\s+svhip_group_audit\s*\(", header)
    assert "svhip_group_audit" in _lib.exported_symbols() and hasattr(lib, "svhip_group_audit")
    assert lib.svhip_abi_version() == 5                     # additive: the ABI version stays
    assert callable(getattr(Engine, "group_audit")) and callable(scoring.group_audit) and callable(scoring.audit_cut)
    assert callable(getattr(sv_model.ModelHandling, "audit"))


def test_group_audit_fails_cleanly_without_a_handle():
    lib = _lib.load()
    assert lib.svhip_group_audit(None, None, 0, 0, 0, None, 0, 0.0, None, None, 0) == -1
    F = np.zeros((2, 1, 192), np.float32)
    gp, miss = np.array([0, 2], np.int64), np.zeros(2, np.int32)
    assert lib.svhip_group_audit(None, F.ctypes.data, 2, 1, 192, gp.ctypes.data, 1, 0.5, miss.ctypes.data, None, 0) == -1


def _rule_mismatch(s32, threshold):
    """benchmark_dataset.py:24-29 in float64 on the float32 score: not (min(score / ratio, 1) > 0.5)"""
    ratio = float(threshold) / 0.5
    v = float(np.float32(s32)) / ratio
    return not ((v if v < 1 else 1) > 0.5)


@pytest.mark.parametrize("threshold, shown", [(0.4, "0.39999998"), (0.38405078649520874, "0.3840508"), (0.5, "0.5"), (0.25, "0.25"),
                                              (1.0 / 3.0, "0.3333333")])
def test_audit_cut_is_the_last_mismatching_float32(threshold, shown):
    cut = scoring.audit_cut(threshold)
    assert isinstance(cut, np.float32) and str(cut) == shown
    up = np.nextafter(cut, np.float32(np.inf))
    assert _rule_mismatch(cut, threshold) and not _rule_mismatch(up, threshold)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="audit_cut"):
            scoring.audit_cut(bad)


def test_wrappers_refuse_a_bad_group_ptr_before_any_launch():
    """an Engine WITHOUT a handle or a library: whatever got past the argument checks would fail on `self.lib`, not with ValueError"""
    eng = Engine.__new__(Engine)
    F = np.zeros((5, 2, 192), np.float32)
    for call in (lambda gp: eng.group_audit(F, gp, 0.5), lambda gp: scoring.group_audit(F, gp, 0.4)):
        with pytest.raises(ValueError, match=r"group_ptr\[0\] = 1 is not 0"):
            call([1, 5])
        with pytest.raises(ValueError, match="decreases at entry 2"):
            call([0, 3, 2, 5])
        with pytest.raises(ValueError, match=r"group_ptr\[n_groups\] = 4 is not n_files = 5"):
            call([0, 2, 4])
        with pytest.raises(ValueError, match="at least one entry"):
            call([])
    with pytest.raises(ValueError, match="n_files, n_crops, D"):
        eng.group_audit(F[0], [0, 2], 0.5)
    with pytest.raises(AttributeError):                     # (the control: good arguments do reach the library)
        eng.group_audit(F, [0, 2, 2, 5], 0.5)


@pytest.fixture
def handler(monkeypatch, tmp_path):
    eng = fakes.FakeScoringEngine()
    monkeypatch.setattr(scoring, "scoring_engine", lambda device=0: eng)
    calls = []

    def audit(feats, group_ptr, threshold, **kw):
        calls.append((np.array(feats), np.array(group_ptr), threshold))
        return st.numpy_group_audit(feats, group_ptr, threshold, **kw)

    monkeypatch.setattr(scoring, "group_audit", audit)
    mh = fakes.fake_model_handling(tmp_path)[0]
    return mh, calls


def _reference_audit(mh, folders, threshold, num_eval):
    """the reference's loop (benchmark_dataset.py:53-84), restated: embed_utterance(normalize=True), all pairs, the rule in float64 on
    the float32 mean |cos| -> the return value of ModelHandling.audit and the report text"""
    result, text = [], ""
    for folder, files in folders:
        emb = {f: np.asarray(mh.embed_utterance(f, num_eval=num_eval, normalize=True), np.float32) for f in files}
        imposters = {}
        for a in range(len(files)):
            for b in range(a + 1, len(files)):
                ea, eb = emb[files[a]].astype(np.float64), emb[files[b]].astype(np.float64)
                na = np.maximum(np.linalg.norm(ea, axis=1), 1e-5)
                nb = np.maximum(np.linalg.norm(eb, axis=1), 1e-5)
                score = np.float32(np.mean(np.abs(np.sum(ea * eb, axis=1) / (na * nb))))
                if _rule_mismatch(score, threshold):
                    for f in (files[a], files[b]):
                        imposters[f] = imposters.get(f, 0) + 1
        found = sorted(imposters.items())
        result.append((folder, len(files), found))
        if found:
            text += f"Folder:{folder}\n" + "".join(f"[{c}/{len(files)}] - {f}\n" for f, c in found) + "//================//\n"
    return result, text


def test_audit_host_logic(handler, tmp_path):
    mh, calls = handler
    files, _, _ = make_e2e_files(str(tmp_path))
    root = tmp_path / "spk"
    layout = {"a": files[0:3], "b": files[3:4], "c": files[4:8], "d": []}
    import shutil
    for name, fl in layout.items():
        (root / name).mkdir(parents=True)
        for f in fl:
            shutil.copy(f, root / name / os.path.basename(f))
    (root / "notes.txt").write_text("not a speaker")
    (root / "a" / "readme.md").write_text("not a wav")
    num_eval = 3

    # discovery: prepare('embed')'s — the sub-directories, *.wav inside
    found = [(str(d), [str(f) for f in d.glob("*.wav")]) for d in root.iterdir() if d.is_dir()]
    assert sorted(len(fl) for _, fl in found) == [0, 1, 3, 4]
    # a threshold from the scores themselves: the median pair score, so that some pairs mismatch and some do not
    every = []
    for _, fl in found:
        e = np.stack([np.asarray(mh.embed_utterance(f, num_eval=num_eval, normalize=True), np.float32) for f in fl]) if fl else None
        if e is not None and len(fl) > 1:
            S = st.group_scores(e, [0, len(fl)])[0]
            every += S[np.triu_indices(len(fl), 1)].tolist()
    threshold = float(np.sort(every)[len(every) // 2]) + 1e-4
    want, want_text = _reference_audit(mh, found, threshold, num_eval)
    assert any(f for _, _, f in want) and sum(len(f) for _, _, f in want) < 8

    report = tmp_path / "report.txt"
    got = mh.audit(str(root), threshold, num_eval=num_eval, save_file=str(report))
    assert got == want
    assert len(calls) == 1 and calls[0][0].shape == (8, num_eval, 16) and calls[0][2] == threshold
    assert sorted(np.diff(calls[0][1]).tolist()) == [0, 1, 3, 4]
    assert np.allclose(np.linalg.norm(calls[0][0], axis=-1), 1.0, atol=1e-5)          # every crop row was L2-normalised
    assert report.read_bytes() == want_text.encode()

    # max_files chunking: whole folders per call, a larger folder alone; the same result, appended once more to the report
    calls.clear()
    assert mh.audit(str(root), threshold, num_eval=num_eval, max_files=3, save_file=str(report)) == want
    assert [int(c[1][-1]) for c in calls if c[1][-1]] and all(int(c[1][-1]) <= 4 for c in calls) and len(calls) >= 3
    assert report.read_bytes() == 2 * want_text.encode()

    # {name: [files]} sources keep their order and names
    as_dict = {name: fl for name, fl in found}
    assert mh.audit(as_dict, threshold, num_eval=num_eval) == want
    # nothing suspicious: no report is written
    quiet = tmp_path / "quiet.txt"
    out = mh.audit(as_dict, 1e-6, num_eval=num_eval, save_file=str(quiet))
    assert all(f == [] for _, _, f in out) and (not quiet.exists() or quiet.read_bytes() == b"")
    with pytest.raises(ValueError):
        mh.audit(None, threshold)
