"""GPU: 1:N identification (svhip_score_topk, Engine.score_topk, ModelHandling.identify) against float64 numpy.

Order under test: score descending, equal scores by the lower gallery index, NaN below every number.  D in {192, 256} takes the fused
route (csrc/score_topk.hip: no score reaches memory), every other width the slab route (score GEMM + a row kernel)."""
import os
import shutil

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel

pytestmark = pytest.mark.gpu

FUSED, SLAB = (192, 256), (320, 512)


@pytest.fixture(scope="module")
def eng():
    return Engine(model="none", max_batch=1)


def _reference(S64, k):
    """the stated order on a float64 score matrix: NaN last, ties to the lower index"""
    S = np.where(np.isnan(S64), -np.inf, S64)
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
    # (a NaN and a -inf score would tie here; no test below has both in one row)
    return order, np.take_along_axis(S64, order, axis=1)


# ---- 1. exact order on integer data ------------------------------------------------------------------------------------------------
_INT = {}


def _int_data(D):
    """entries uniform in {-4..4}: every product and sum is exact in fp32 and in fp16 planes (|score| <= 16 D)"""
    if D not in _INT:
        rng = np.random.default_rng(7)
        G = rng.integers(-4, 5, (4097, D)).astype(np.float32)
        Q = rng.integers(-4, 5, (129, D)).astype(np.float32)
        _INT[D] = (Q, G, Q.astype(np.float64) @ G.astype(np.float64).T)
    return _INT[D]


@pytest.mark.parametrize("N", [1, 20, 33, 129])
@pytest.mark.parametrize("D", FUSED + SLAB)
def test_exact_order_on_integer_data(eng, D, N):
    Q, G, S64 = _int_data(D)
    crossing = 0
    for M in (1, 31, 32, 33, 4097):
        for k in sorted({kk for kk in (1, 2, 10, 128, M) if kk <= min(M, 128)}):
            sc, ix = eng.score_topk(Q[:N], G[:M], k)
            assert sc.shape == ix.shape == (N, k) and sc.dtype == np.float32 and ix.dtype == np.int32
            order, want = _reference(S64[:N, :M], k)
            assert np.array_equal(ix, order), (D, N, M, k)
            assert np.array_equal(sc, want.astype(np.float32)), (D, N, M, k)
            if k < M:
                s = -np.sort(-S64[:N, :M], axis=1)
                crossing += int((s[:, k - 1] == s[:, k]).sum())
    if N == 129:
        assert crossing > 0     # rows whose k-th and (k + 1)-th score tie: the tie rule was exercised


def test_more_than_one_query_chunk(eng):
    """N = 16 384 + 148, M = 1 283, D = 192, k = 5: three launches of the fused route with three list strides (_chunk_data)"""
    from tests.test_gpu_topk_norm import _chunk_data
    d = _chunk_data()
    sc, ix = eng.score_topk(d["Q"], d["G"], 5)
    order, want = _reference(d["S"], 5)
    assert np.array_equal(ix, order)
    assert np.array_equal(sc.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("D", [192, 320])
def test_planted_rows_on_block_and_slice_edges(eng, D):
    """the unique best row at index 0, at M - 1 and at a multiple of 32; duplicate gallery rows across 32-row boundaries"""
    rng = np.random.default_rng(11)
    M = 4097
    Q = rng.integers(-4, 5, (129, D)).astype(np.float32)
    Q[Q == 0] = 1.0
    G0 = rng.integers(-4, 5, (M, D)).astype(np.float32)
    best = 4.0 * np.sign(Q[3])              # the one row that reaches 4 sum |q| for query 3
    for N in (20, 129):
        for at in (0, M - 1, 64, 2048):
            G = G0.copy()
            G[at] = best
            sc, ix = eng.score_topk(Q[:N], G, 10)
            order, want = _reference(Q[:N].astype(np.float64) @ G.astype(np.float64).T, 10)
            assert ix[3, 0] == at and sc[3, 0] == 4.0 * np.abs(Q[3]).sum()
            assert np.array_equal(ix, order) and np.array_equal(sc, want.astype(np.float32))
        G = G0.copy()
        for a in (31, 2047, 4095):
            G[a] = best
            G[a + 1] = best
        for k in (2, 6, 10):
            sc, ix = eng.score_topk(Q[:N], G, k)
            order, want = _reference(Q[:N].astype(np.float64) @ G.astype(np.float64).T, k)
            assert list(ix[3, :min(k, 6)]) == [31, 32, 2047, 2048, 4095, 4096][:k]
            assert np.array_equal(ix, order) and np.array_equal(sc, want.astype(np.float32))


# ---- 2. unit vectors against float64 ---------------------------------------------------------------------------------------------------
_UNIT = {}


def _unit_data(D):
    """Q (300, D), G (70001, D) unit rows and, from the float64 scores, each row's 129 best values and indices"""
    if D not in _UNIT:
        rng = np.random.default_rng(20260101 + D)
        Q = rng.standard_normal((300, D)).astype(np.float32)
        G = rng.standard_normal((70001, D)).astype(np.float32)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True).astype(np.float32)
        G /= np.linalg.norm(G, axis=1, keepdims=True).astype(np.float32)
        S64 = Q.astype(np.float64) @ G.astype(np.float64).T
        part = np.argpartition(-S64, 129, axis=1)[:, :130]
        pv = np.take_along_axis(S64, part, axis=1)
        o = np.argsort(-pv, axis=1, kind="stable")[:, :129]
        _UNIT[D] = (Q, G, np.take_along_axis(pv, o, axis=1), np.take_along_axis(part, o, axis=1))
    return _UNIT[D]


def _check_against_float64(Q, G, top_v, top_i, sc, ix, k):
    N, M = Q.shape[0], G.shape[0]
    assert sc.shape == ix.shape == (N, k)
    assert np.all(sc[:, :-1] >= sc[:, 1:])                                     # non-increasing
    assert ix.min() >= 0 and ix.max() < M
    assert all(len(set(r)) == k for r in ix.tolist())                           # distinct
    exact = np.einsum("nd,nkd->nk", Q.astype(np.float64), G[ix].astype(np.float64))
    err = float(np.abs(sc - exact).max())
    print(f"max |score - float64| = {err:.3e}")
    assert err <= 1e-6
    kth, nxt = top_v[:, k - 1], top_v[:, k]
    close = (kth - nxt) < 4e-6
    print(f"rows whose k-th gap is under 4e-6: {int(close.sum())}")
    assert int(close.sum()) <= 15                                               # at most 5 % of the rows take the looser rule
    for r in range(N):
        if not close[r]:
            assert set(ix[r].tolist()) == set(top_i[r, :k].tolist()), r
        else:
            assert np.all(exact[r] >= kth[r] - 2e-6), r
            must = top_i[r, :k][top_v[r, :k] > kth[r] + 2e-6]
            assert set(must.tolist()) <= set(ix[r].tolist()), r


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("D", [192, 256, 320])
def test_unit_vectors_against_float64(eng, D, k):
    Q, G, top_v, top_i = _unit_data(D)
    sc, ix = eng.score_topk(Q, G, k)
    _check_against_float64(Q, G, top_v, top_i, sc, ix, k)


# ---- 3. route and invariance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 320])
def test_route_labels_invariance_and_device_pointers(eng, D):
    Q, G, _, _ = _unit_data(D)
    eng.profile(True)
    try:
        sc, ix = eng.score_topk(Q, G, 10)
        labels = set(eng.profile_results())
    finally:
        eng.profile(False)
    if D in FUSED:
        assert {"score_topk", "score_topk_merge"} <= labels and "score_topk_rows" not in labels
    else:
        assert "score_topk_rows" in labels and "score_topk" not in labels and "score_topk_merge" not in labels
    # a row's result depends on that row and the gallery only: not on N, nor on the row's place in Q
    sc20, ix20 = eng.score_topk(Q[:20], G, 10)
    assert np.array_equal(ix20, ix[:20]) and np.array_equal(sc20.view(np.uint32), sc[:20].view(np.uint32))
    sc1, ix1 = eng.score_topk(Q[150:151], G, 10)
    assert np.array_equal(ix1, ix[150:151]) and np.array_equal(sc1.view(np.uint32), sc[150:151].view(np.uint32))
    # device pointers, preallocated outputs
    Qd, Gd = torch.from_numpy(Q).cuda(), torch.from_numpy(G).cuda()
    out = (torch.empty((300, 10), dtype=torch.float32, device="cuda"), torch.empty((300, 10), dtype=torch.int32, device="cuda"))
    sd, idd = eng.score_topk(Qd, Gd, 10, out=out)
    assert sd is out[0] and idd is out[1]
    assert np.array_equal(idd.cpu().numpy(), ix) and np.array_equal(sd.cpu().numpy().view(np.uint32), sc.view(np.uint32))
    with pytest.raises(ValueError):
        eng.score_topk(Qd, G, 10)                                              # one memory space per call


# ---- 4. non-finite inputs and bad arguments --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 320])
def test_nan_rows_stay_in_their_place(eng, D):
    rng = np.random.default_rng(5)
    N, M, k = 40, 1000, 10
    Q = rng.integers(-4, 5, (N, D)).astype(np.float32)
    G = rng.integers(-4, 5, (M, D)).astype(np.float32)
    Qc, Gc = Q.copy(), G.copy()
    Gc[123] = 0.0                                     # the clean stand-in of the NaN row: a zero score, far below every row's 10 best
    Qc[5] = 0.0
    clean_sc, clean_ix = eng.score_topk(Qc, Gc, k)
    assert clean_sc[np.arange(N) != 5].min() > 0
    Q[5] = np.nan
    G[123] = np.nan
    sc, ix = eng.score_topk(Q, G, k)
    others = np.arange(N) != 5
    assert np.array_equal(ix[others], clean_ix[others]) and np.array_equal(sc[others], clean_sc[others])
    assert np.all(np.isnan(sc[5])) and ix[5].min() >= 0 and ix[5].max() < M and len(set(ix[5].tolist())) == k
    # the NaN row is never returned while k <= M - 1, and is the last one at k = M
    for M2, k2 in ((33, 32), (33, 33), (129, 128)):
        G2 = G[100:100 + M2].copy()                   # row 23 of it is the NaN row
        sc2, ix2 = eng.score_topk(Q[:4], G2, k2)
        order, want = _reference(Q[:4].astype(np.float64) @ np.nan_to_num(G2, nan=0.0).astype(np.float64).T
                                 + np.where(np.arange(M2) == 23, np.nan, 0.0)[None, :], k2)
        assert np.array_equal(ix2, order)
        assert np.array_equal(np.isnan(sc2), np.isnan(want)) and np.array_equal(np.nan_to_num(sc2), np.nan_to_num(want).astype(np.float32))
        if k2 < M2:
            assert 23 not in ix2
        else:
            assert np.all(ix2[:, -1] == 23) and np.all(np.isnan(sc2[:, -1]))
    if D not in FUSED:
        return                  # (the slab route has score_matrix's magnitude contract: |x| <= 65504 at these widths)
    # infinities: +inf first, -inf last of the numbers
    G3 = G[200:264].copy()
    q = np.zeros((1, D), np.float32)
    q[0, 0] = 1.0
    G3[7, 0], G3[40, 0] = np.inf, -np.inf
    sc3, ix3 = eng.score_topk(q, G3, 64)
    assert ix3[0, 0] == 7 and sc3[0, 0] == np.inf and ix3[0, -1] == 40 and sc3[0, -1] == -np.inf


def test_bad_arguments_are_refused_by_name(eng):
    Q = np.zeros((3, 192), np.float32)
    G = np.zeros((50, 192), np.float32)
    for k, text in ((0, "k = 0"), (129, "k = 129"), (51, "k = 51")):
        with pytest.raises(_lib.SvhipError, match=text):
            eng.score_topk(Q, G, k)
    with pytest.raises(ValueError):
        eng.score_topk(Q, np.zeros((50, 256), np.float32), 1)
    sc, ix = eng.score_topk(Q[:0], G, 5)
    assert sc.shape == ix.shape == (0, 5) and sc.dtype == np.float32 and ix.dtype == np.int32


# ---- 5. identify on the committed speaker fixture ---------------------------------------------------------------------------------------
def test_identify_matches_the_numpy_statement(tmp_path):
    """enroll two speakers through prepare('embed'), identify every file; the stated rule in numpy on the same embeddings must give
    the same best class and scores within 1e-5"""
    from tests.e2e_data import E2E_SEED_W, make_e2e_files
    from tests.test_gpu_e2e import ARGS
    tmp = str(tmp_path)
    net = WrappedModel(SpeakerEncoder(**ARGS))
    mh = ModelHandling(net, **dict(ARGS, save_folder=tmp))
    sd = synth.synth_state_dict(synth.ecapa_param_spec(C=512), seed=E2E_SEED_W)
    net.module.load_state_dict({"__S__." + k: v for k, v in sd.items()})
    files, _, _ = make_e2e_files(tmp)
    root = os.path.join(tmp, "spk")
    for s in range(2):
        os.makedirs(os.path.join(root, f"speaker{s}"))
        for f in files[3 * s:3 * s + 3]:
            shutil.copy(f, os.path.join(root, f"speaker{s}", os.path.basename(f)))
    out = os.path.join(tmp, "prep")
    os.makedirs(out)
    assert mh.prepare(save_path=out, prepare_type="embed", num_eval=4, source=root) is True
    probe = list(files[:6])
    scores, index, names = mh.identify(probe, out, top=2, num_eval=4)
    assert scores.shape == index.shape == (6, 2) and index.dtype == np.int32

    def unit(a):
        return a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-12)

    embeds = torch.load(os.path.join(out, "embeds.pt")).numpy().astype(np.float64)          # (num_eval, nOut, n_class)
    classes = np.load(os.path.join(out, "classes.npy"), allow_pickle=True).item()
    gal = unit(embeds.mean(axis=0).T)
    q = unit(np.stack([unit(mh.embed_utterance(f, num_eval=4, normalize=False).numpy().astype(np.float64)).mean(axis=0) for f in probe]))
    want = q @ gal.T
    order = np.argsort(-want, axis=1, kind="stable")
    assert np.array_equal(index[:, 0], order[:, 0])
    assert float(np.abs(scores - np.take_along_axis(want, index.astype(np.int64), axis=1)).max()) <= 1e-5
    assert names == [[classes[int(i)] for i in row] for row in index]
    # the other two gallery forms give the same answer
    s2, i2 = mh.identify(probe, torch.load(os.path.join(out, "embeds.pt")), top=2, num_eval=4)
    s3, i3, n3 = mh.identify(probe, embeds.mean(axis=0).T.astype(np.float32), classes=["a", "b"], top=2, num_eval=4)
    assert np.array_equal(i2, index) and np.array_equal(i3, index)
    assert float(np.abs(s2 - scores).max()) <= 1e-6 and float(np.abs(s3 - scores).max()) <= 1e-6
    assert n3 == [[["a", "b"][int(i)] for i in row] for row in index]


def test_slab_row_kernel_when_the_best_scores_share_a_few_strides(eng):
    """the slab route's row kernel takes a threshold from the maxima of 256 strided shares of the row; here every large score sits in
    127 of the shares (3 048 of them, more than the kernel's candidate list holds), so the row takes the kernel's other path"""
    D, M, k = 320, 256 * 24, 128
    t = np.arange(M)
    v = np.where(t % 256 < 127, 10000.0 + (M - t), np.where(t % 256 == 127, 5000.0 + t, (t % 97).astype(np.float64)))
    G = np.zeros((M, D), np.float32)
    G[:, 0] = v
    G[:, 1] = (t % 5).astype(np.float32)
    Q = np.zeros((3, D), np.float32)
    Q[0, 0], Q[1, 0], Q[2, 0] = 1.0, 2.0, -1.0
    Q[:, 1] = 1.0
    sc, ix = eng.score_topk(Q, G, k)
    order, want = _reference(Q.astype(np.float64) @ G.astype(np.float64).T, k)
    assert np.array_equal(ix, order) and np.array_equal(sc, want.astype(np.float32))
