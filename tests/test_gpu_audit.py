"""GPU: the dataset audit (svhip_group_audit, csrc/group_audit.hip) against numpy's statement of it (tests/audit_statement.py): exact
counts and score bits on data whose scores have fixed bits, the block-diagonal mask at group boundaries, the plain route and its
score_trials bits, the routes by width and alignment, float data against float64, independence of the launch and symmetry bit for bit,
edge values, refusals, device pointers, and ModelHandling.audit on the committed speaker fixture."""
import os
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, scoring, synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
from tests import audit_statement as st

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    return Engine(model="none", max_batch=1)


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _bits(a):
    return np.ascontiguousarray(_np(a), np.float32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _off4(a):
    """the array on the device, its first float 4 bytes past a 16-byte boundary"""
    flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(a.reshape(-1)).cuda()
    t = flat[1:].view(a.shape)
    assert t.data_ptr() % 16 == 4
    return t


def _labels(eng, fn):
    eng.profile(True)
    try:
        out = fn()
        return out, set(eng.profile_results())
    finally:
        eng.profile(False)


MFMA, PLAIN = {"group_audit"}, {"group_audit_pairs", "group_audit_count"}


def _offdiag(blocks):
    return np.concatenate([S[~np.eye(len(S), dtype=bool)] for S in blocks])


def _cuts(blocks):
    """a score that occurs (the median off-diagonal value) and a float32 strictly between two neighbouring values that occur"""
    vals = np.unique(_offdiag(blocks))
    k = len(vals) // 2
    at, mid = vals[k], np.float32(0.5 * (float(vals[k]) + float(vals[k + 1])))
    assert vals[k] < mid < vals[k + 1]
    return np.float32(at), mid


def _check_exact(eng, F, gp, blocks, give=None):
    """counts and every score bit equal the statement, at a cut that occurs and at one between two that occur"""
    Fin = F if give is None else give(F)
    at, mid = _cuts(blocks)
    n_at = int((_offdiag(blocks) == at).sum())
    assert n_at > 0                                                                    # pairs exactly AT the cut are present ...
    below = np.nextafter(at, np.float32(-np.inf))
    for cut in (at, mid):
        miss, score, score_ptr = eng.group_audit(Fin, gp, cut, scores=True)
        assert _np(miss).dtype == np.int32 and np.array_equal(_np(miss), st.miss_counts(blocks, cut)), cut
        assert np.array_equal(_bits(score), _bits(st.flat_scores(blocks)))
        assert np.array_equal(score_ptr, np.concatenate([[0], np.cumsum(np.diff(gp) ** 2)]))
        assert np.array_equal(_np(eng.group_audit(Fin, gp, cut)), _np(miss))              # (the call without scores counts the same)
    assert int(st.miss_counts(blocks, at).sum()) - int(st.miss_counts(blocks, below).sum()) == n_at       # ... and count as mismatches
    return n_at


# ---- 1. exact counts and scores ------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 31, 32, 33, 64, 65, 129, 130, 300)       # below, at and just over the tile widths; several tiles both ways


@pytest.mark.parametrize("D", [192, 256, 512])
@pytest.mark.parametrize("n_crops", [1, 4, 20])
def test_exact_counts_and_scores(eng, n_crops, D):
    F, gp = st.exact_data(SIZES, n_crops, D, seed=1000 * n_crops + D)
    blocks = st.group_scores(F, gp)
    (n_at), labels = _labels(eng, lambda: _check_exact(eng, F, gp, blocks))
    assert n_at > 0 and MFMA <= labels and not PLAIN & labels


# ---- 2. group boundaries -------------------------------------------------------------------------------------------------------------------------
def _boundary_sizes():
    return [int(x) for x in np.random.default_rng(60).integers(1, 18, 60)]


def test_boundaries_shared_inside_orthogonal_outside(eng):
    """files of a group share their rows, other groups' rows are far: every count is 0, and ANY pairing across a boundary adds to it"""
    sizes = _boundary_sizes()
    rng = np.random.default_rng(61)
    D, n_crops = 192, 2
    rows = []
    for g, n in enumerate(sizes):
        r = np.zeros((n_crops, D), np.float32)
        r[:, 64 * (g % 3):64 * (g % 3) + 64] = rng.choice(np.float32([-1.0, 1.0]), (n_crops, 64))      # neighbours: disjoint columns
        rows += [r] * n
    F = np.stack(rows)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    blocks = st.group_scores(F, gp)
    assert all(np.all(S == 1.0) for S in blocks)
    whole = st.group_scores(F, [0, len(F)])[0]
    other = np.ones_like(whole, dtype=bool)
    for g in range(len(sizes)):
        other[gp[g]:gp[g + 1], gp[g]:gp[g + 1]] = False
    assert whole[other].max() <= 0.5                                                  # every cross pair WOULD be a mismatch
    miss, score, _ = eng.group_audit(F, gp, 0.5, scores=True)
    assert not miss.any() and np.all(score == 1.0)


def test_boundaries_orthogonal_inside_shared_outside(eng):
    """the reverse: orthogonal inside a group, file k of every group the same row: every count is n_g - 1, and a tile that took a partner
    from the wrong group undercounts"""
    sizes = _boundary_sizes()
    D, n_crops = 192, 2
    rows = []
    for n in sizes:
        for k in range(n):
            r = np.zeros((n_crops, D), np.float32)
            r[:, 4 * k:4 * k + 4] = 1.0                                              # norm 2; file k meets only the files k elsewhere
            rows.append(r)
    F = np.stack(rows)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    miss, score, sp = eng.group_audit(F, gp, 0.5, scores=True)
    assert np.array_equal(miss, np.repeat(np.asarray(sizes) - 1, sizes).astype(np.int32))
    assert np.array_equal(score, st.flat_scores([np.eye(n, dtype=np.float32) for n in sizes]))


# ---- 3. the plain route --------------------------------------------------------------------------------------------------------------------------
PLAIN_SIZES = (1, 2, 31, 33, 0, 65, 130)


@pytest.mark.parametrize("D, give", [(64, _off4), (100, None), (192, _off4)], ids=["64-unaligned", "100", "192-unaligned"])
def test_plain_route_exact(eng, D, give):
    F, gp = st.exact_data(PLAIN_SIZES, 4, D, seed=300 + D, flips=min(24, D // 3))
    blocks = st.group_scores(F, gp)
    n_at, labels = _labels(eng, lambda: _check_exact(eng, F, gp, blocks, give))
    assert n_at > 0 and PLAIN <= labels and not MFMA & labels


def _float_groups(sizes, n_crops, D, seed):
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((int(sum(sizes)), n_crops, D)).astype(np.float32)
    return F, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def test_plain_route_score_bits_are_score_trials(eng):
    F, gp = _float_groups((5, 40, 1, 70), 4, 100, seed=31)
    (miss, score, sp), labels = _labels(eng, lambda: eng.group_audit(F, gp, 0.08, scores=True))
    assert PLAIN <= labels
    for g in range(len(gp) - 1):
        n = int(gp[g + 1] - gp[g])
        ia, ib = (x.ravel().astype(np.int32) + int(gp[g]) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
        want = eng.score_trials(F, ia, ib, "cosine")
        assert np.array_equal(_bits(score[sp[g]:sp[g + 1]]), _bits(want)), g
    assert miss.sum() > 0 and np.array_equal(miss, st.miss_counts([score[sp[g]:sp[g + 1]].reshape(int(gp[g + 1] - gp[g]), -1)
                                                                   for g in range(len(gp) - 1)], np.float32(0.08)))


# ---- 4. routes -----------------------------------------------------------------------------------------------------------------------------------
def test_routes_by_width_and_alignment(eng):
    for D in (192, 256, 512, 704):
        F, gp = _float_groups((3, 40), 2, D, seed=D)
        _, labels = _labels(eng, lambda: eng.group_audit(_dev(F), gp, 0.1))
        assert MFMA <= labels and not PLAIN & labels, D
        _, labels = _labels(eng, lambda: eng.group_audit(F, gp, 0.1))                 # (host operands are staged on aligned scratch)
        assert MFMA <= labels and not PLAIN & labels, D
    for D, give in ((64, _off4), (100, _dev), (1056, _dev)):
        F, gp = _float_groups((3, 40), 2, D, seed=D)
        _, labels = _labels(eng, lambda: eng.group_audit(give(F), gp, 0.1))
        assert PLAIN <= labels and "score_trials" in labels and not MFMA & labels, D


# ---- 5. float data against float64 ---------------------------------------------------------------------------------------------------------------
def test_float_data_against_float64(eng):
    """300 files in groups of 7 .. 130, 20 crops, D = 192: unit rows around six centroids (noise 1.2).  Bar (2 D + n_crops + 16) 2^-24 =
    2.5e-5: any-order fp32 accumulation costs at most about D 2^-24 on each of the dot and the two squared norms, the mean over the
    crops adds n_crops 2^-24, the sqrt, products and divisions a few roundings.  Pairs whose float64 score lies within the bar of the
    cut may fall either way (at most 1 % of the pairs); every other pair's decision is float64's."""
    sizes, n_crops, D = (7, 130, 33, 64, 66), 20, 192
    rng = np.random.default_rng(20261021)
    cen = rng.standard_normal((6, D))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    which = rng.integers(0, 6, sum(sizes))
    X = cen[which][:, None, :] + 1.2 * rng.standard_normal((sum(sizes), n_crops, D)) / np.sqrt(D)
    F = (X / np.linalg.norm(X, axis=-1, keepdims=True)).astype(np.float32)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    want = st.group_scores(F, gp, np.float64)
    bar = (2 * D + n_crops + 16) * EPS
    cut = np.float32(np.quantile(_offdiag(want), 0.7))
    miss, score, sp = eng.group_audit(F, gp, cut, scores=True)
    worst, undecided_all, pairs = 0.0, 0, 0
    for g, S in enumerate(want):
        n = len(S)
        got = score[sp[g]:sp[g + 1]].reshape(n, n)
        worst = max(worst, float(np.abs(got - S).max()))
        off = ~np.eye(n, dtype=bool)
        undecided = (np.abs(S - float(cut)) <= bar) & off
        decided = (S <= float(cut)) & off & ~undecided
        m = miss[gp[g]:gp[g + 1]]
        assert np.all(m >= decided.sum(axis=1)) and np.all(m <= decided.sum(axis=1) + undecided.sum(axis=1)), g
        undecided_all += int(undecided.sum())
        pairs += int(off.sum())
    print(f"group_audit float data: worst |score - float64| = {worst:.3e} (bar {bar:.3e}), undecided pairs {undecided_all} of {pairs}")
    assert undecided_all <= 0.01 * pairs
    assert worst <= bar


# ---- 6. independence and symmetry, bit for bit, on both routes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 100], ids=["mfma", "plain"])
def test_independence_and_symmetry(eng, D):
    sizes = (70, 5, 33, 1, 40)
    F, gp = _float_groups(sizes, 3, D, seed=600 + D)
    F /= np.linalg.norm(F, axis=-1, keepdims=True)
    cut = np.float32(0.06)
    miss, score, sp = eng.group_audit(F, gp, cut, scores=True)
    assert 0 < miss.sum() < sum(n * (n - 1) for n in sizes)
    rows = lambda g: F[gp[g]:gp[g + 1]]
    for g, n in enumerate(sizes):
        blk = score[sp[g]:sp[g + 1]].reshape(n, n)
        assert np.array_equal(_bits(blk), _bits(blk.T)), g                            # s(i, j) and s(j, i): the same bits
        m1, s1, _ = eng.group_audit(rows(g), [0, n], cut, scores=True)                # alone
        assert np.array_equal(m1, miss[gp[g]:gp[g + 1]]) and np.array_equal(_bits(s1), _bits(blk.ravel())), g
        pad = np.random.default_rng(g).standard_normal((13, 3, D)).astype(np.float32)
        m2, s2, p2 = eng.group_audit(np.concatenate([pad, rows(g)]), [0, 13, 13 + n], cut, scores=True)      # at another place in F
        assert np.array_equal(m2[13:], miss[gp[g]:gp[g + 1]]) and np.array_equal(_bits(s2[p2[1]:]), _bits(blk.ravel())), g
    order = [3, 0, 4, 2, 1]                                                           # among permuted groups
    Fp = np.concatenate([rows(g) for g in order])
    gpp = np.concatenate([[0], np.cumsum([sizes[g] for g in order])]).astype(np.int64)
    mp, sp_, pp = eng.group_audit(Fp, gpp, cut, scores=True)
    for k, g in enumerate(order):
        assert np.array_equal(mp[gpp[k]:gpp[k + 1]], miss[gp[g]:gp[g + 1]])
        assert np.array_equal(_bits(sp_[pp[k]:pp[k + 1]]), _bits(score[sp[g]:sp[g + 1]]))


# ---- 7. edge values ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 100], ids=["mfma", "plain"])
def test_edge_values(eng, D):
    n, n_crops = 40, 2
    F, _ = _float_groups((n + 1,), n_crops, D, seed=700 + D)
    F /= np.linalg.norm(F, axis=-1, keepdims=True)
    gp = np.array([0, 0, n, n + 1], np.int64)                                        # an empty group, the group under test, a group of one
    cut = np.float32(0.07)
    base_m, base_s, sp = eng.group_audit(F, gp, cut, scores=True)
    assert base_m[n] == 0 and sp.tolist() == [0, 0, n * n, n * n + 1] and abs(base_s[-1] - 1.0) < 1e-6
    ZERO, NAN, INF, TINY = 3, 17, 32, 39
    E = F.copy()
    E[ZERO] = 0.0
    E[NAN, 1, 5] = np.nan
    E[INF, 0, 7] = np.inf
    E[TINY] = 0.0
    E[TINY, :, 11] = 2.0 ** -20                                                      # norm 2^-20: under the 1e-5 clamp
    miss, score, _ = eng.group_audit(E, gp, cut, scores=True)
    S, B = score[:n * n].reshape(n, n), base_s[:n * n].reshape(n, n)
    plain_rows = np.setdiff1d(np.arange(n), [ZERO, NAN, INF, TINY])
    # no other file's score changes, and every count is the count of the scores returned
    assert np.array_equal(_bits(S[np.ix_(plain_rows, plain_rows)]), _bits(B[np.ix_(plain_rows, plain_rows)]))
    assert np.array_equal(miss[:n], st.miss_counts([S], cut)) and np.array_equal(_bits(S), _bits(S.T))
    ok = np.setdiff1d(np.arange(n), [NAN, INF])
    assert np.all(S[ZERO, ok] == 0.0) and miss[ZERO] == n - 3                        # a zero row: 0 against everyone, a mismatch for cut > 0
    assert np.all(np.isnan(S[NAN])) and np.all(np.isnan(S[INF])) and miss[NAN] == 0 and miss[INF] == 0      # never counted
    for i in plain_rows:                                                             # ... and they cost nobody a count
        with np.errstate(invalid="ignore"):
            assert miss[i] == int((S[i, ok] <= cut).sum()) - int(S[i, i] <= cut)
    want = st.group_scores(E[:n], [0, n], np.float64)[0]
    rel = np.abs(S[TINY, plain_rows] - want[TINY, plain_rows]) / np.abs(want[TINY, plain_rows])
    assert np.all(want[TINY, plain_rows] > 0) and rel.max() <= 8 * EPS, rel.max()


# ---- 8. refusals by name -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_name(eng):
    F = np.ones((5, 2, 192), np.float32)
    good = np.array([0, 2, 5], np.int64)
    miss = np.full(5, -7, np.int32)

    def call(F_=F, n_files=5, n_crops=2, D=192, gp=good, n_groups=2, out=miss):
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = eng.lib.svhip_group_audit(eng.h, ptr(F_), n_files, n_crops, D, ptr(gp), n_groups, 0.5, ptr(out), None, 0)
        return rc, (eng.lib.svhip_last_error(eng.h) or b"").decode()

    for kw, text in ((dict(n_crops=0), "n_crops = 0"), (dict(D=0), "D = 0"), (dict(F_=None), "NULL pointer"), (dict(gp=None), "NULL pointer"),
                     (dict(out=None), "NULL pointer"), (dict(gp=np.array([1, 2, 5], np.int64)), "group_ptr[0] = 1 is not 0"),
                     (dict(gp=np.array([0, 3, 2, 5], np.int64), n_groups=3), "decreases at entry 2"),
                     (dict(gp=np.array([0, 2, 4], np.int64)), "group_ptr[n_groups] = 4 is not n_files = 5"),
                     (dict(n_files=-1), "n_files = -1"), (dict(n_groups=-1), "n_groups = -1")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("group_audit:") and text in msg, (kw, rc, msg)
        assert np.all(miss == -7)                                                    # nothing was written
    assert call(n_files=0)[0] == 0 and call(n_groups=0)[0] == 0 and np.all(miss == -7)      # nothing to do: nothing read or written
    assert call()[0] == 0 and miss.tolist() == [0, 0, 0, 0, 0]                      # (the control: ones everywhere, every score 1)


# ---- 9. device pointers with SVHIP_ASYNC ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 100], ids=["mfma", "plain"])
def test_device_pointers_async(eng, D):
    sizes = (33, 2, 70)
    F, gp = _float_groups(sizes, 4, D, seed=900 + D)
    F /= np.linalg.norm(F, axis=-1, keepdims=True)
    cut = np.float32(0.05)
    miss, score, sp = eng.group_audit(F, gp, cut, scores=True)
    got = eng.group_audit(_dev(F), gp, cut, scores=True)                              # device tensors in, device tensors out
    assert torch.is_tensor(got[0]) and got[0].is_cuda and got[1].is_cuda
    assert np.array_equal(_np(got[0]), miss) and np.array_equal(_bits(got[1]), _bits(score))
    dF = _dev(F)
    dm = torch.full((len(F),), -1, dtype=torch.int32, device="cuda")
    ds = torch.full((int(sp[-1]),), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    flags = _lib.IN_DEVICE | _lib.OUT_DEVICE | _lib.ASYNC
    rc = eng.lib.svhip_group_audit(eng.h, dF.data_ptr(), len(F), 4, D, gp.ctypes.data, len(gp) - 1, float(cut), dm.data_ptr(), ds.data_ptr(), flags)
    assert rc == 0
    eng.synchronize()
    assert np.array_equal(_np(dm), miss) and np.array_equal(_bits(ds), _bits(score))


# ---- 10. ModelHandling.audit on the committed speaker fixture -----------------------------------------------------------------------------------
def test_audit_on_the_speaker_fixture(tmp_path):
    from tests.e2e_data import E2E_SEED_W, make_e2e_files
    from tests.test_gpu_e2e import ARGS
    tmp = str(tmp_path)
    net = WrappedModel(SpeakerEncoder(**ARGS))
    mh = ModelHandling(net, **dict(ARGS, save_folder=tmp))
    sd = synth.synth_state_dict(synth.ecapa_param_spec(C=512), seed=E2E_SEED_W)
    net.module.load_state_dict({"__S__." + k: v for k, v in sd.items()})
    files, _, _ = make_e2e_files(tmp)
    root = os.path.join(tmp, "spk")
    for s in range(3):
        os.makedirs(os.path.join(root, f"speaker{s}"))
        for f in files[2 * s:2 * s + 2]:
            shutil.copy(f, os.path.join(root, f"speaker{s}", os.path.basename(f)))
    shutil.copy(files[2], os.path.join(root, "speaker0", "zz_" + os.path.basename(files[2])))      # a file of speaker 1 in speaker 0's folder
    num_eval = 4
    folders = [(str(d), [str(f) for f in d.glob("*.wav")]) for d in sorted(Path(root).iterdir()) if d.is_dir()]
    assert sorted(len(fl) for _, fl in folders) == [2, 2, 3]
    # the reference's loop restated: embed_utterance(normalize=True), all pairs of a folder, scoring.cosine_similarity, the rule
    emb = {f: mh.embed_utterance(f, num_eval=num_eval, normalize=True).numpy() for _, fl in folders for f in fl}
    pairs = [(folder, a, b) for folder, fl in folders for i, a in enumerate(fl) for b in fl[i + 1:]]
    s64 = []
    for _, a, b in pairs:
        x, y = emb[a].astype(np.float64), emb[b].astype(np.float64)
        s64.append(float(np.mean(np.abs(np.sum(x * y, axis=1) / (np.maximum(np.linalg.norm(x, axis=1), 1e-5) * np.maximum(np.linalg.norm(y, axis=1), 1e-5))))))
    # the threshold comes from the float64 scores alone: half way between the two neighbouring distinct values that lie farthest apart, so
    # that some pairs mismatch, some match, and the fp32 score has room on either side
    vals = np.unique(s64)
    k = int(np.argmax(np.diff(vals)))
    bar = (2 * 192 + num_eval + 16) * EPS
    assert vals[k + 1] - vals[k] > 2 * bar
    threshold = 0.5 * (vals[k] + vals[k + 1])
    ratio = threshold / 0.5
    want, text = [], ""
    for folder, fl in folders:
        imposters = {}
        for a, b in ((a, b) for f_, a, b in pairs if f_ == folder):
            score = scoring.cosine_similarity(emb[a], emb[b], device=mh.gpu)
            v = float(np.float32(score)) / ratio
            if not ((v if v < 1 else 1) > 0.5):
                for f in (a, b):
                    imposters[f] = imposters.get(f, 0) + 1
        found = sorted(imposters.items())
        want.append((folder, len(fl), found))
        if found:
            text += f"Folder:{folder}\n" + "".join(f"[{c}/{len(fl)}] - {f}\n" for f, c in found) + "//================//\n"
    assert any(f for _, _, f in want)
    as_dict = {folder: fl for folder, fl in folders}
    report = os.path.join(tmp, "report.txt")
    got = mh.audit(as_dict, threshold, num_eval=num_eval, save_file=report)
    assert got == want
    assert open(report, "rb").read() == text.encode()
    assert mh.audit(as_dict, threshold, num_eval=num_eval, max_files=2) == want
    by_dir = mh.audit(root, threshold, num_eval=num_eval)                             # the directory form finds the same folders
    assert sorted(by_dir) == sorted(want)
