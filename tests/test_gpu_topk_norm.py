"""GPU: AS-normalised 1:N identification (svhip_score_topk_norm, Engine.score_topk_norm, ModelHandling.identify(scoring_mode="norm"))
against the float64 statement.

Statement (svhip.h): a = 0.5f / sigma, b = mu * a in fp32, t = fmaf(s, aq + ag, -(bq + bg)); per query the k largest t, best first, ties
to the lower gallery index, NaN below every number.  D in {192, 256} takes the fused route (the fmaf sits on the MFMA accumulators,
before the selection), every other width the slab route (score GEMM + a row kernel that applies the fmaf on every read)."""
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
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    return Engine(model="none", max_batch=1)


def _coef(mu, sigma):
    """the two coefficients of the statement, each one IEEE fp32 operation"""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.float32(0.5) / np.asarray(sigma, np.float32)
        b = np.asarray(mu, np.float32) * a
    return a, b


def _statement(S64, q_stats, g_stats):
    """t in float64 from the fp32 coefficients: s (aq + ag) - (bq + bg)"""
    aq, bq = _coef(*q_stats)
    ag, bg = _coef(*g_stats)
    with np.errstate(invalid="ignore"):
        return S64 * (aq.astype(np.float64)[:, None] + ag.astype(np.float64)[None, :]) - (bq.astype(np.float64)[:, None] + bg.astype(np.float64)[None, :])


def _reference(T64, k):
    """the stated order on a float64 matrix: NaN last, ties to the lower index"""
    T = np.where(np.isnan(T64), -np.inf, T64)
    order = np.argsort(-T, axis=1, kind="stable")[:, :k]
    # (a NaN and a -inf score would tie here; no test below has both in one row)
    return order, np.take_along_axis(T64, order, axis=1)


def _same(sc, want):
    """float32 results equal a float64 reference, NaN in the same places"""
    return np.array_equal(np.isnan(sc), np.isnan(want)) and np.array_equal(np.nan_to_num(sc), np.nan_to_num(want).astype(np.float32))


# ---- 1. exact order on integer data ------------------------------------------------------------------------------------------------
_INT = {}


def _int_data(D):
    """Q, G uniform in {-4..4}; sigma in {0.25, 0.5, 1, 2} (a in {2, 1, 0.5, 0.25}), mu integer in [-8, 8] (b a multiple of 0.25):
    every coefficient, product and sum is exact in fp32 for D <= 512 (|s| <= 16 D, |t| <= 4 * 8192 + 64 in steps of 0.25)"""
    if D not in _INT:
        rng = np.random.default_rng(7)
        G = rng.integers(-4, 5, (4097, D)).astype(np.float32)
        Q = rng.integers(-4, 5, (129, D)).astype(np.float32)
        sig = np.array([0.25, 0.5, 1.0, 2.0], np.float32)
        q_stats = (rng.integers(-8, 9, 129).astype(np.float32), sig[rng.integers(0, 4, 129)])
        g_stats = (rng.integers(-8, 9, 4097).astype(np.float32), sig[rng.integers(0, 4, 4097)])
        T64 = _statement(Q.astype(np.float64) @ G.astype(np.float64).T, q_stats, g_stats)
        _INT[D] = (Q, G, q_stats, g_stats, T64)
    return _INT[D]


def _crossing_ties(T64, k):
    s = -np.sort(-T64, axis=1)
    return int((s[:, k - 1] == s[:, k]).sum())


@pytest.mark.parametrize("N", [1, 20, 33, 129])
@pytest.mark.parametrize("D", FUSED + SLAB)
def test_exact_order_on_integer_data(eng, D, N):
    Q, G, (qm, qs), (gm, gs), T64 = _int_data(D)
    crossing = 0
    for M in (1, 31, 32, 33, 4097):
        for k in sorted({kk for kk in (1, 2, 10, 128, M) if kk <= min(M, 128)}):
            sc, ix = eng.score_topk_norm(Q[:N], (qm[:N], qs[:N]), G[:M], (gm[:M], gs[:M]), k)
            assert sc.shape == ix.shape == (N, k) and sc.dtype == np.float32 and ix.dtype == np.int32
            order, want = _reference(T64[:N, :M], k)
            assert np.array_equal(ix, order), (D, N, M, k)
            assert np.array_equal(sc, want.astype(np.float32)), (D, N, M, k)
            if k < M:
                crossing += _crossing_ties(T64[:N, :M], k)
    if N == 129:
        assert crossing > 0     # rows whose k-th and (k + 1)-th t tie: the tie rule was exercised


_CHUNK = {}


def _chunk_data():
    """A call of more than one query chunk, shared with tests/test_gpu_topk.py and tests/test_gpu_above.py: N = 16 384 + 148 queries, so
    the fused route (csrc/api_search.hip, fused_plan) runs three launches - a full chunk of 128 MANY tiles, and from the second chunk
    one MANY tile of 128 queries and a FEW launch of 20 - each with its own offset into the queries, the coefficient table and the
    outputs.  M = 1 283 is 41 gallery blocks with a ragged last one: on a 256-CU chip 4, 5 and 3 slices, so the three launches have
    three different list strides.  _int_data's generators at D = 192; S and t are exact in fp32 and kept as fp32 (85 MB each)."""
    if not _CHUNK:
        rng = np.random.default_rng(16384 + 148)
        N, M, D = 16384 + 148, 1283, 192
        G = rng.integers(-4, 5, (M, D)).astype(np.float32)
        Q = rng.integers(-4, 5, (N, D)).astype(np.float32)
        sig = np.array([0.25, 0.5, 1.0, 2.0], np.float32)
        q_stats = (rng.integers(-8, 9, N).astype(np.float32), sig[rng.integers(0, 4, N)])
        g_stats = (rng.integers(-8, 9, M).astype(np.float32), sig[rng.integers(0, 4, M)])
        S64 = Q.astype(np.float64) @ G.astype(np.float64).T
        T64 = _statement(S64, q_stats, g_stats)
        S, T = S64.astype(np.float32), T64.astype(np.float32)
        assert np.array_equal(S, S64) and np.array_equal(T, T64)                # (nothing was rounded)
        _CHUNK.update(Q=Q, G=G, q_stats=q_stats, g_stats=g_stats, S=S, T=T)
    return _CHUNK


def test_more_than_one_query_chunk(eng):
    d = _chunk_data()
    k = 5
    sc, ix = eng.score_topk_norm(d["Q"], d["q_stats"], d["G"], d["g_stats"], k)
    order, want = _reference(d["T"], k)
    assert np.array_equal(ix, order)
    assert np.array_equal(sc.view(np.uint32), want.view(np.uint32))


# ---- 2. the coefficients alone order the gallery ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 129])
@pytest.mark.parametrize("D", [192, 320])
def test_coefficients_alone_order_the_gallery(eng, D, N):
    """Q = 0 and sigma = 0.5 everywhere (a = 1, b = mu): t = -(q_mu + g_mu).  With g_mu a permutation of 0 .. M - 1 the answer is the k
    rows of smallest g_mu, in order, for every query: any error in the accumulator-to-row mapping, in the clamped last block or in the
    slice offsets returns another row.  An implementation that selects on s (all zero here) and normalises afterwards returns rows 0 .. k - 1."""
    Q = np.zeros((N, D), np.float32)
    q_stats = (np.arange(N, dtype=np.float32) % 5, np.full(N, 0.5, np.float32))
    for M in (33, 4097, 70001):
        rng = np.random.default_rng(100 + M)
        G = rng.integers(-4, 5, (M, D)).astype(np.float32)
        g_mu = rng.permutation(M).astype(np.float32)
        g_sig = np.full(M, 0.5, np.float32)
        by_mu = np.argsort(g_mu, kind="stable")
        for k in (1, 10, 128):
            if k > M:
                continue
            sc, ix = eng.score_topk_norm(Q, q_stats, G, (g_mu, g_sig), k)
            assert np.array_equal(ix, np.broadcast_to(by_mu[:k].astype(np.int32), (N, k))), (D, N, M, k)
            assert np.array_equal(sc, -(q_stats[0][:, None] + g_mu[by_mu[:k]][None, :])), (D, N, M, k)
        for at in (0, M - 1, 64, 2048):
            if at >= M:
                continue
            mu2 = g_mu.copy()
            mu2[at] = -1.0                                   # the one row below every other mean
            sc, ix = eng.score_topk_norm(Q, q_stats, G, (mu2, g_sig), 10)
            want = np.argsort(mu2, kind="stable")[:10].astype(np.int32)
            assert want[0] == at and np.array_equal(ix, np.broadcast_to(want, (N, 10))), (D, N, M, at)
            assert np.array_equal(sc[:, 0], 1.0 - q_stats[0])


# ---- 3. unit vectors against float64 ---------------------------------------------------------------------------------------------------
_UNIT = {}
TOP = 100


def _stats64(S, top):
    """utils.py:142-146 in float64: the `top` largest cohort scores of every row, population mean and deviation"""
    part = -np.partition(-S, top - 1, axis=1)[:, :top]
    return part.mean(axis=1), part.std(axis=1)


def _unit_data(D):
    """Q (300, D), G (70001, D), cohort (600, D) unit rows; the statistics of the float64 statement cast to fp32; from the float64 t of
    the fp32 coefficients each row's 129 best values and indices; the raw-cosine best row"""
    if D not in _UNIT:
        rng = np.random.default_rng(20261020 + D)
        Q = rng.standard_normal((300, D)).astype(np.float32)
        G = rng.standard_normal((70001, D)).astype(np.float32)
        C = rng.standard_normal((600, D)).astype(np.float32)
        for X in (Q, G, C):
            X /= np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
        C64 = C.astype(np.float64)
        q_stats = tuple(x.astype(np.float32) for x in _stats64(Q.astype(np.float64) @ C64.T, TOP))
        g_stats = tuple(x.astype(np.float32) for x in _stats64(G.astype(np.float64) @ C64.T, TOP))
        S64 = Q.astype(np.float64) @ G.astype(np.float64).T
        T64 = _statement(S64, q_stats, g_stats)
        part = np.argpartition(-T64, 129, axis=1)[:, :130]
        pv = np.take_along_axis(T64, part, axis=1)
        o = np.argsort(-pv, axis=1, kind="stable")[:, :129]
        _UNIT[D] = dict(Q=Q, G=G, C=C, q_stats=q_stats, g_stats=g_stats, top_v=np.take_along_axis(pv, o, axis=1),
                        top_i=np.take_along_axis(part, o, axis=1), raw_best=S64.argmax(axis=1))
    return _UNIT[D]


def _bound(Q, G, q_stats, g_stats, ix):
    """for every returned pair: the float64 t of the fp32 coefficients and the bar on |t - t64|.  The plain call's contract puts s
    within 1e-6 of s64, which A = aq + ag scales; the statement adds six roundings (two coefficients a side are data here; the sums
    aq + ag and bq + bg, and the fmaf), each at most 2^-24 of a term no larger than |s64| A + |bq| + |bg|: 8 of them bound the lot."""
    aq, bq = (x.astype(np.float64) for x in _coef(*q_stats))
    ag, bg = (x.astype(np.float64) for x in _coef(*g_stats))
    s64 = np.einsum("nd,nkd->nk", Q.astype(np.float64), G[ix].astype(np.float64))
    A = aq[:, None] + ag[ix]
    t64 = s64 * A - (bq[:, None] + bg[ix])
    return t64, 1e-6 * A + 8 * EPS * (np.abs(s64) * A + np.abs(bq)[:, None] + np.abs(bg[ix]))


GAP = 2e-4


def _check_against_float64(d, sc, ix, k):
    Q, G, top_v, top_i = d["Q"], d["G"], d["top_v"], d["top_i"]
    N, M = Q.shape[0], G.shape[0]
    assert sc.shape == ix.shape == (N, k)
    assert np.all(sc[:, :-1] >= sc[:, 1:])                                     # non-increasing
    assert ix.min() >= 0 and ix.max() < M
    assert all(len(set(r)) == k for r in ix.tolist())                           # distinct
    t64, bound = _bound(Q, G, d["q_stats"], d["g_stats"], ix)
    assert float(bound.max()) <= 6.4e-5
    err = np.abs(sc - t64)
    print(f"max |t - float64| = {float(err.max()):.3e}, largest bound {float(bound.max()):.3e}, worst err / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)
    kth, nxt = top_v[:, k - 1], top_v[:, k]
    close = (kth - nxt) < GAP
    print(f"rows whose k-th gap is under {GAP}: {int(close.sum())}")
    assert int(close.sum()) <= 15                                               # at most 5 % of the rows take the looser rule
    for r in range(N):
        if not close[r]:
            assert set(ix[r].tolist()) == set(top_i[r, :k].tolist()), r
        else:
            assert np.all(t64[r] >= kth[r] - GAP / 2), r
            must = top_i[r, :k][top_v[r, :k] > kth[r] + GAP / 2]
            assert set(must.tolist()) <= set(ix[r].tolist()), r


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("D", [192, 256, 320])
def test_unit_vectors_against_float64(eng, D, k):
    d = _unit_data(D)
    differ = int((d["top_i"][:, 0] != d["raw_best"]).sum())
    print(f"queries whose normalised best row is not their raw-cosine best row: {differ} of 300")
    assert differ >= 50                                                         # the normalisation decides the ranking here
    sc, ix = eng.score_topk_norm(d["Q"], d["q_stats"], d["G"], d["g_stats"], k)
    _check_against_float64(d, sc, ix, k)


# ---- 4. end to end with the library's own statistics -----------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 320])
def test_end_to_end_with_the_librarys_statistics(eng, D):
    d = _unit_data(D)
    Q, G = d["Q"], d["G"]
    N, k = Q.shape[0], 10
    E = np.ascontiguousarray(np.concatenate([Q, G]))
    mu, sd = eng.asnorm_stats(E, d["C"], TOP)
    q_stats, g_stats = (mu[:N], sd[:N]), (mu[N:], sd[N:])
    sc, ix = eng.score_topk_norm(Q, q_stats, G, g_stats, k)
    ia = np.repeat(np.arange(N, dtype=np.int32), k)
    ib = (N + ix.reshape(-1)).astype(np.int32)
    pairs = eng.asnorm_pairs(E, mu, sd, ia, ib).reshape(N, k)
    _, bound = _bound(Q, G, q_stats, g_stats, ix)
    diff = np.abs(sc - pairs)
    print(f"max |score_topk_norm - asnorm_pairs| = {float(diff.max()):.3e}, worst diff / (2 bound) {float((diff / (2 * bound)).max()):.3f}")
    assert np.all(diff <= 2 * bound)


# ---- 5. routes, invariance, device pointers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 320])
def test_route_labels_invariance_and_device_pointers(eng, D):
    d = _unit_data(D)
    Q, G, (qm, qs), g_stats = d["Q"], d["G"], d["q_stats"], d["g_stats"]
    eng.profile(True)
    try:
        sc, ix = eng.score_topk_norm(Q, (qm, qs), G, g_stats, 10)
        labels = set(eng.profile_results())
    finally:
        eng.profile(False)
    assert "score_topk_coef" in labels and "score_topk" not in labels and "score_topk_rows" not in labels
    if D in FUSED:
        assert {"score_topk_norm", "score_topk_merge"} <= labels and "score_topk_rows_norm" not in labels
    else:
        assert "score_topk_rows_norm" in labels and "score_topk_norm" not in labels and "score_topk_merge" not in labels
    # a row's result depends on that row, its statistics and the gallery only: not on N, nor on the row's place in Q, nor on the form
    # of the kernel (300 queries: shared-block form; 20 and 1: the form whose waves walk different blocks)
    for sl in (slice(0, 20), slice(150, 151)):
        s2, i2 = eng.score_topk_norm(Q[sl], (qm[sl], qs[sl]), G, g_stats, 10)
        assert np.array_equal(i2, ix[sl]) and np.array_equal(s2.view(np.uint32), sc[sl].view(np.uint32))
    # device pointers, preallocated outputs
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Qd, Gd, qd, gd = dev(Q), dev(G), (dev(qm), dev(qs)), (dev(g_stats[0]), dev(g_stats[1]))
    out = (torch.empty((300, 10), dtype=torch.float32, device="cuda"), torch.empty((300, 10), dtype=torch.int32, device="cuda"))
    sd_, id_ = eng.score_topk_norm(Qd, qd, Gd, gd, 10, out=out)
    assert sd_ is out[0] and id_ is out[1]
    assert np.array_equal(id_.cpu().numpy(), ix) and np.array_equal(sd_.cpu().numpy().view(np.uint32), sc.view(np.uint32))
    with pytest.raises(ValueError):
        eng.score_topk_norm(Qd, (qm, qs), Gd, gd, 10)                          # one memory space per call
    with pytest.raises(ValueError):
        eng.score_topk_norm(Qd, qd, G, gd, 10)


# ---- 6. non-finite statistics stay in their place --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["g_mu_nan", "g_sigma_zero"])
@pytest.mark.parametrize("D", [192, 320])
def test_non_finite_statistics_stay_in_their_place(eng, D, case):
    rng = np.random.default_rng(5)
    N, M, k = 40, 1000, 10
    Q = rng.integers(-4, 5, (N, D)).astype(np.float32)
    G = rng.integers(-4, 5, (M, D)).astype(np.float32)
    G[123] = 0.0
    sig = np.array([0.25, 0.5, 1.0, 2.0], np.float32)
    qm, qs = rng.integers(-8, 9, N).astype(np.float32), sig[rng.integers(0, 4, N)]
    gm, gs = rng.integers(-8, 9, M).astype(np.float32), sig[rng.integers(0, 4, M)]
    gm[123], gs[123] = 8.0, 0.25            # the clean stand-in of the bad row: t = -(bq + 16), below every row's 10 best
    clean_sc, clean_ix = eng.score_topk_norm(Q, (qm, qs), G, (gm, gs), k)
    others = np.arange(N) != 5
    assert 123 not in clean_ix[others] and clean_sc[others].min() > 0.0
    qm2, gm2, gs2 = qm.copy(), gm.copy(), gs.copy()
    qm2[5] = np.nan
    if case == "g_mu_nan":
        gm2[123] = np.nan
    else:
        gm2[123], gs2[123] = 0.0, 0.0       # a = inf, b = 0 * inf = NaN: t is NaN whatever s is
    sc, ix = eng.score_topk_norm(Q, (qm2, qs), G, (gm2, gs2), k)
    assert np.array_equal(ix[others], clean_ix[others]) and np.array_equal(sc[others].view(np.uint32), clean_sc[others].view(np.uint32))
    assert np.all(np.isnan(sc[5])) and ix[5].min() >= 0 and ix[5].max() < M and len(set(ix[5].tolist())) == k
    # the bad gallery row is never returned while k <= M - 1, and is the last one at k = M
    S64 = Q.astype(np.float64) @ G.astype(np.float64).T
    for M2, k2 in ((33, 32), (33, 33), (129, 128)):
        cols = slice(100, 100 + M2)                   # row 23 of it is the bad row
        g2 = (gm2[cols], gs2[cols])
        sc2, ix2 = eng.score_topk_norm(Q[:4], (qm[:4], qs[:4]), G[cols], g2, k2)
        T64 = _statement(S64[:4, cols], (qm[:4], qs[:4]), g2)
        assert np.all(np.isnan(T64[:, 23])) and int(np.isnan(T64).sum()) == 4
        order, want = _reference(T64, k2)
        assert np.array_equal(ix2, order) and _same(sc2, want)
        if k2 < M2:
            assert 23 not in ix2
        else:
            assert np.all(ix2[:, -1] == 23) and np.all(np.isnan(sc2[:, -1]))


# ---- 7. bad arguments by name --------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_name(eng):
    Q = np.zeros((3, 192), np.float32)
    G = np.zeros((50, 192), np.float32)
    q_stats = (np.zeros(3, np.float32), np.ones(3, np.float32))
    g_stats = (np.zeros(50, np.float32), np.ones(50, np.float32))
    for k, text in ((0, "score_topk_norm: k = 0"), (129, "score_topk_norm: k = 129"), (51, "score_topk_norm: k = 51")):
        with pytest.raises(_lib.SvhipError, match=text):
            eng.score_topk_norm(Q, q_stats, G, g_stats, k)
    with pytest.raises(ValueError):
        eng.score_topk_norm(Q, q_stats, np.zeros((50, 256), np.float32), g_stats, 1)
    # a short statistic array, a missing one
    with pytest.raises(ValueError, match="g_stats"):
        eng.score_topk_norm(Q, q_stats, G, (g_stats[0][:49], g_stats[1]), 1)
    with pytest.raises(ValueError, match="q_stats"):
        eng.score_topk_norm(Q, (q_stats[0], q_stats[1][:2]), G, g_stats, 1)
    with pytest.raises(ValueError):
        eng.score_topk_norm(Q, (q_stats[0], None), G, g_stats, 1)
    # a NULL statistic pointer at the C ABI, each of the four
    out_s, out_i = np.zeros((3, 1), np.float32), np.zeros((3, 1), np.int32)
    ptrs = [q_stats[0].ctypes.data, q_stats[1].ctypes.data, g_stats[0].ctypes.data, g_stats[1].ctypes.data]
    for null in range(4):
        p = [None if i == null else v for i, v in enumerate(ptrs)]
        rc = eng.lib.svhip_score_topk_norm(eng.h, Q.ctypes.data, 3, p[0], p[1], G.ctypes.data, 50, p[2], p[3], 192, 1, out_s.ctypes.data,
                                           out_i.ctypes.data, 0)
        assert rc == -1                                  # SVHIP_ERR_INVALID
        with pytest.raises(_lib.SvhipError, match="score_topk_norm: NULL pointer"):
            eng._ck(rc)
    sc, ix = eng.score_topk_norm(Q[:0], (q_stats[0][:0], q_stats[1][:0]), G, g_stats, 5)
    assert sc.shape == ix.shape == (0, 5) and sc.dtype == np.float32 and ix.dtype == np.int32


# ---- 8. identify(scoring_mode="norm") on the committed speaker fixture ---------------------------------------------------------------------
def test_identify_norm_matches_the_numpy_statement(tmp_path):
    """enroll two speakers through prepare('embed'), identify every file against a seeded 64-row unit cohort; the stated rule in numpy
    on the same embeddings must give the same best class and scores within 1e-4"""
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
    cohort = np.random.default_rng(64).standard_normal((64, 192))
    cohort = (cohort / np.linalg.norm(cohort, axis=1, keepdims=True)).astype(np.float32)
    scores, index, names = mh.identify(probe, out, top=2, num_eval=4, scoring_mode="norm", cohorts=cohort, cohort_top=8)
    assert scores.shape == index.shape == (6, 2) and index.dtype == np.int32

    def unit(a):
        return a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-12)

    embeds = torch.load(os.path.join(out, "embeds.pt")).numpy().astype(np.float64)          # (num_eval, nOut, n_class)
    classes = np.load(os.path.join(out, "classes.npy"), allow_pickle=True).item()
    gal = unit(embeds.mean(axis=0).T)
    q = unit(np.stack([unit(mh.embed_utterance(f, num_eval=4, normalize=False).numpy().astype(np.float64)).mean(axis=0) for f in probe]))
    c64 = cohort.astype(np.float64)
    mq, sq = _stats64(q @ c64.T, 8)
    mg, sg = _stats64(gal @ c64.T, 8)
    s = q @ gal.T
    want = 0.5 * ((s - mq[:, None]) / sq[:, None] + (s - mg[None, :]) / sg[None, :])
    order = np.argsort(-want, axis=1, kind="stable")
    assert np.array_equal(index[:, 0], order[:, 0])
    err = float(np.abs(scores - np.take_along_axis(want, index.astype(np.int64), axis=1)).max())
    print(f"max |identify(norm) - numpy statement| = {err:.3e}")
    assert err <= 1e-4
    assert names == [[classes[int(i)] for i in row] for row in index]
    # the cohort as a file gives the same answer
    path = os.path.join(tmp, "cohorts.npy")
    np.save(path, cohort)
    s2, i2, _ = mh.identify(probe, out, top=2, num_eval=4, scoring_mode="norm", cohorts_path=path, cohort_top=8)
    assert np.array_equal(i2, index) and np.array_equal(s2, scores)
    # a threshold between the best and the second score of one probe: -1 / None there and below it, nothing at or above it
    r = int(np.argmax(scores[:, 0] - scores[:, 1]))
    thr = float(0.5 * (float(scores[r, 0]) + float(scores[r, 1])))
    s3, i3, n3 = mh.identify(probe, out, top=2, num_eval=4, scoring_mode="norm", cohorts=cohort, cohort_top=8, thresh_score=thr)
    assert np.array_equal(s3, scores)
    assert i3[r, 0] == index[r, 0] and i3[r, 1] == -1 and n3[r] == [classes[int(index[r, 0])], None]
    assert np.array_equal(i3, np.where(scores < thr, -1, index))
    assert n3 == [[classes[int(i)] if i >= 0 else None for i in row] for row in i3]
    # cosine mode is still the plain call, whatever cohort is handed in
    sc0, ic0, nc0 = mh.identify(probe, out, top=2, num_eval=4)
    sc1, ic1, nc1 = mh.identify(probe, out, top=2, num_eval=4, scoring_mode="cosine", cohorts=cohort)
    assert np.array_equal(ic1, ic0) and np.array_equal(sc1, sc0) and nc1 == nc0
    with pytest.raises(ValueError, match="cohort"):
        mh.identify(probe, out, top=2, num_eval=4, scoring_mode="norm")
