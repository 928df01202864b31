"""GPU: threshold search (svhip_score_above_count / _fill, Engine.score_above, ModelHandling.matches / duplicates) against its statement.

Statement (svhip.h): a pair (n, m) is a hit iff v(n, m) >= thr, v the inner product as score_topk computes it (or t as score_topk_norm
does); a NaN v is never a hit.  Result: CSR, a row's hits in ascending gallery index.  D in {192, 256} with aligned operands takes the
fused route (score_topk's MFMA loop, counted once and written once), everything else the slab route (score GEMM + a row kernel)."""
import os
import shutil

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
from tests.test_gpu_topk_norm import EPS, _chunk_data, _coef, _statement, _stats64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return Engine(model="none", max_batch=1)


def _csr(keep, V):
    """numpy's statement: np.nonzero per row in ascending index -> (row_ptr, index, score)"""
    row_ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    n, m = np.nonzero(keep)
    return row_ptr, m.astype(np.int32), np.asarray(V)[n, m].astype(np.float32)


def _equal(got, want):
    """row_ptr, index and score bits, exactly"""
    rp, ix, sc = (np.asarray(x.cpu() if torch.is_tensor(x) else x) for x in got)
    assert rp.dtype == np.int64 and ix.dtype == np.int32 and sc.dtype == np.float32
    return np.array_equal(rp, want[0]) and np.array_equal(ix, want[1]) and np.array_equal(sc.view(np.uint32), want[2].view(np.uint32))


def _rows(got, sl):
    """the CSR rows sl of a result, re-based"""
    rp, ix, sc = got
    a, b = int(rp[sl.start]), int(rp[sl.stop])
    return rp[sl.start:sl.stop + 1] - a, ix[a:b], sc[a:b]


# ---- integer data: every inner product is an exact fp32 integer, so the hit sets are exact -------------------------------------------------
_INT = {}


def _int_cols(D):
    """_int_data at width D; widths below 192 are the first D columns of the 192-wide set"""
    Q, G, q_stats, g_stats, _, _ = _int_data(max(D, 192))
    return np.ascontiguousarray(Q[:, :D]), np.ascontiguousarray(G[:, :D]), q_stats, g_stats


def _int_data(D):
    """Q (300, D), G (4100, D) uniform in {-2..2}; S = Q G^T in float64 (|s| <= 4 D: exact in fp32 at every D used here); statistics with
    power-of-two sigmas and integer means as tests/test_gpu_topk_norm.py builds them (every step of t is exact), and that t"""
    if D not in _INT:
        rng = np.random.default_rng(11 + D)
        G = rng.integers(-2, 3, (4100, D)).astype(np.float32)
        Q = rng.integers(-2, 3, (300, D)).astype(np.float32)
        sig = np.array([0.25, 0.5, 1.0, 2.0], np.float32)
        q_stats = (rng.integers(-8, 9, 300).astype(np.float32), sig[rng.integers(0, 4, 300)])
        g_stats = (rng.integers(-8, 9, 4100).astype(np.float32), sig[rng.integers(0, 4, 4100)])
        S = Q.astype(np.float64) @ G.astype(np.float64).T
        _INT[D] = (Q, G, q_stats, g_stats, S, _statement(S, q_stats, g_stats))
    return _INT[D]


def _occurring(V, quantile=0.9):
    """a value that occurs in V, with about a tenth of V at or above it"""
    return float(np.sort(V.ravel())[int(quantile * (V.size - 1))])


def _exact_sets(eng, D, N, sizes, dev=None):
    Q, G, _, _, S, _ = _int_data(D)
    hits = ties = 0
    for M in sizes:
        s = S[:N, :M]
        t0 = _occurring(s)
        for thr in (t0, t0 + 0.5):
            q, g = (Q[:N], G[:M]) if dev is None else dev(Q[:N], G[:M])
            got = eng.score_above(q, g, thr)
            assert _equal(got, _csr(s >= thr, s)), (D, N, M, thr)
            hits += int((s >= thr).sum())
        ties += int((s == t0).sum())
    return hits, ties


# ---- 1. exact sets on integer data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 33, 130])
@pytest.mark.parametrize("D", [192, 256])
def test_exact_sets_on_integer_data(eng, D, N):
    """N = 1: the FEW form; N = 33: one MANY tile with 95 empty query slots; N = 130: a full MANY tile and a FEW launch of 2.  M = 1, 31:
    a gallery shorter than a block; 33, 1000, 4100: a last block that runs past M; 4100 = 129 blocks: several gallery slices."""
    hits, ties = _exact_sets(eng, D, N, (1, 31, 33, 1000, 4100))
    assert hits > 0 and ties > 0                # pairs exactly AT the threshold were there: >= includes them


@pytest.mark.parametrize("norm", [False, True])
def test_more_than_one_query_chunk(eng, norm):
    """N = 16 384 + 148, M = 1 283, D = 192: three launches of the fused route (tests/test_gpu_topk_norm.py, _chunk_data), each with its
    own place in the list-count scratch, its own rows of row_ptr and of the coefficient table.  The threshold is a value that occurs,
    with about three hits a row at or above it."""
    d = _chunk_data()
    V = d["T"] if norm else d["S"]
    thr = _occurring(V[:512], 1.0 - 3.0 / V.shape[1])
    keep = V >= np.float32(thr)
    per_row = keep.sum(axis=1)
    assert (per_row == 0).any() and (per_row >= 3).any() and 1.0 <= per_row.mean() <= 6.0 and int((V == np.float32(thr)).sum()) > 0
    got = eng.score_above(d["Q"], d["G"], thr, *((d["q_stats"], d["g_stats"]) if norm else ()))
    assert _equal(got, _csr(keep, V))


# ---- 2. edge values -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 64])
def test_edge_values(eng, D):
    Q, G, _, _ = _int_cols(D)
    N, M = 40, 1000
    Q, G = Q[:N].copy(), G[:M].copy()
    S = Q.astype(np.float64) @ G.astype(np.float64).T
    thr = _occurring(S)
    clean = eng.score_above(Q, G, thr)
    assert _equal(clean, _csr(S >= thr, S))
    if D == 192:
        # an inf entry in one gallery row: +inf, -inf or NaN (0 * inf) scores in that column, by the sign of the query's entry.  (The
        # fused route's exact fp32 MFMA only: the slab route's GEMM splits an operand into half planes, and inf = inf + NaN there.)
        Gi = G.copy()
        Gi[5, 0] = np.inf
        Si = S.copy()
        Si[:, 5] = np.where(Q[:, 0] > 0, np.inf, np.where(Q[:, 0] < 0, -np.inf, np.nan))
        assert np.isnan(Si[:, 5]).any() and np.isposinf(Si[:, 5]).any() and np.isneginf(Si[:, 5]).any()
        n_nan = int(np.isnan(Si).sum())
        with np.errstate(invalid="ignore"):
            got = eng.score_above(Q, Gi, -np.inf)
            assert int(got[0][-1]) == N * M - n_nan and _equal(got, _csr(~np.isnan(Si), Si))          # everything but the NaN pairs
            got = eng.score_above(Q, Gi, np.inf)
            assert int(got[0][-1]) == int(np.isposinf(Si).sum()) > 0 and _equal(got, _csr(np.isposinf(Si), Si))      # only the +inf scores
    assert int(eng.score_above(Q, G, np.inf)[0][-1]) == 0
    # a NaN row of Q, a NaN row of G: no hits there - not even at thr = -inf - and every other row and column as before
    Qn, Gn = Q.copy(), G.copy()
    Qn[7, 3] = np.nan
    Gn[33, D - 1] = np.nan
    keep = S >= thr
    keep[7, :] = False
    keep[:, 33] = False
    assert _equal(eng.score_above(Qn, Gn, thr), _csr(keep, S))
    keep[:] = True
    keep[7, :] = False
    keep[:, 33] = False
    got = eng.score_above(Qn, Gn, -np.inf)
    assert int(got[0][-1]) == N * M - (N + M - 1) and _equal(got, _csr(keep, S))
    # no hit at all; no query at all
    rp, ix, sc = eng.score_above(Q, G, 4.0 * D + 1.0)
    assert rp.tolist() == [0] * (N + 1) and ix.shape == sc.shape == (0,) and ix.dtype == np.int32 and sc.dtype == np.float32
    rp, ix, sc = eng.score_above(Q[:0], G, thr)
    assert rp.tolist() == [0] and rp.dtype == np.int64 and ix.shape == sc.shape == (0,)
    cnt = np.zeros(1, np.int64)
    assert eng.lib.svhip_score_above_count(eng.h, None, 0, G.ctypes.data, M, D, thr, None, None, None, None, 0, 0, None, 0) == 0
    assert eng.lib.svhip_score_above_fill(eng.h, None, 0, G.ctypes.data, M, D, thr, None, None, None, None, 0, 0, cnt.ctypes.data, None, None, 0) == 0


def test_bad_arguments_are_refused_by_name(eng):
    Q, G = np.zeros((3, 192), np.float32), np.zeros((50, 192), np.float32)
    cnt = np.zeros(3, np.int64)
    st = [np.ones(3, np.float32), np.ones(3, np.float32), np.ones(50, np.float32), np.ones(50, np.float32)]
    call = lambda thr, p, mode=0, q_base=0: eng.lib.svhip_score_above_count(eng.h, Q.ctypes.data, 3, G.ctypes.data, 50, 192, thr, *p, q_base, mode,
                                                                            cnt.ctypes.data, 0)
    none = [None] * 4
    for args, text in (((float("nan"), none), "score_above: the threshold is NaN"),
                       ((0.5, [st[0].ctypes.data, None, st[2].ctypes.data, st[3].ctypes.data]), "score_above: 1 of the four statistic arrays"),
                       ((0.5, [None, None, None, st[3].ctypes.data]), "score_above: 3 of the four statistic arrays"),
                       ((0.5, none, 2), "score_above: unknown mode"),
                       ((0.5, none, _lib.ABOVE_UPPER, -1), "score_above: q_base = -1")):
        rc = call(*args)
        assert rc == -1                                 # SVHIP_ERR_INVALID
        with pytest.raises(_lib.SvhipError, match=text):
            eng._ck(rc)
    with pytest.raises(_lib.SvhipError, match="multiple of 32") as e:
        eng.score_above(np.zeros((3, 48), np.float32), np.zeros((50, 48), np.float32), 0.5)
    assert e.value.code == -5                           # SVHIP_ERR_UNSUPPORTED


# ---- 3. norm mode on exact data -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 130])
@pytest.mark.parametrize("D", [192, 256, 64])
def test_norm_mode_on_exact_data(eng, D, N):
    """the fp32 restatement of fmaf(s, aq + ag, -(bq + bg)) >= thr: on this data every coefficient, sum and product is exact, so one
    rounding of the float64 value IS the fp32 chain.  t moves in steps of 0.25: thr + 0.125 lies strictly between two values."""
    Q, G, (qm, qs), (gm, gs) = _int_cols(D)
    for M in (33, 1000, 4100):
        q, g = Q[:N], G[:M]
        q_stats, g_stats = (qm[:N], qs[:N]), (gm[:M], gs[:M])
        aq, bq = _coef(*q_stats)
        ag, bg = _coef(*g_stats)
        S32 = (q.astype(np.float64) @ g.astype(np.float64).T).astype(np.float32)
        A, B = aq[:, None] + ag[None, :], bq[:, None] + bg[None, :]                    # fp32 sums
        T = (S32.astype(np.float64) * A.astype(np.float64) - B.astype(np.float64)).astype(np.float32)      # one rounding: the fmaf
        assert np.array_equal(T.astype(np.float64), _statement(S32.astype(np.float64), q_stats, g_stats))  # (nothing was rounded)
        t0 = _occurring(T)
        for thr in (t0, t0 + 0.125):
            assert _equal(eng.score_above(q, g, thr, q_stats, g_stats), _csr(T >= np.float32(thr), T)), (D, N, M, thr)


# ---- 4. UPPER: the self-join of one set ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 64])
def test_upper_self_join(eng, D):
    E = _int_cols(D)[0]
    S = E.astype(np.float64) @ E.astype(np.float64).T
    thr = _occurring(S, 0.97)
    keep = (S >= thr) & (np.arange(300)[None, :] > np.arange(300)[:, None])           # numpy's upper triangle: m > n
    want = _csr(keep, S)
    assert 0 < want[0][-1] < keep.size // 20
    whole = eng.score_above(E, E, thr, upper=True)
    assert _equal(whole, want)
    assert not np.any(whole[1] == np.repeat(np.arange(300), np.diff(whole[0])))         # no row matches itself (it would: s(n, n) is the largest)
    a = eng.score_above(E[:150], E, thr, upper=True, q_base=0)
    b = eng.score_above(E[150:], E, thr, upper=True, q_base=150)
    both = (np.concatenate([a[0], a[0][-1] + b[0][1:]]), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]]))
    assert _equal(both, want)
    assert not _equal(eng.score_above(E, E, thr), want)                                 # (without the flag: the full square)


# ---- 5. bits and independence on unit-norm float rows -------------------------------------------------------------------------------------------
_UNIT = {}


def _unit_rows(D):
    if D not in _UNIT:
        rng = np.random.default_rng(2026 + D)
        Q = rng.standard_normal((130, D)).astype(np.float32)
        G = rng.standard_normal((4100, D)).astype(np.float32)
        for X in (Q, G):
            X /= np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
        q_stats = (rng.uniform(0.05, 0.15, 130).astype(np.float32), rng.uniform(0.02, 0.05, 130).astype(np.float32))
        g_stats = (rng.uniform(0.05, 0.15, 4100).astype(np.float32), rng.uniform(0.02, 0.05, 4100).astype(np.float32))
        _UNIT[D] = (Q, G, q_stats, g_stats)
    return _UNIT[D]


def _dense_from_topk(sc, ix):
    T = np.empty(sc.shape, np.float32)
    np.put_along_axis(T, ix.astype(np.int64), sc, axis=1)
    return T


@pytest.mark.parametrize("D", [192, 256, 320])
def test_score_bits_are_score_topks(eng, D):
    """M <= 128: score_topk(k = M) returns every pair's score, so it gives the dense matrix of the SAME route's bits"""
    Q, G, (qm, qs), (gm, gs) = _unit_rows(D)
    for M in (128, 97):
        g = G[:M]
        T = _dense_from_topk(*eng.score_topk(Q, g, M))
        assert _equal(eng.score_above(Q, g, 0.0), _csr(T >= 0.0, T)), (D, M)
        Tn = _dense_from_topk(*eng.score_topk_norm(Q, (qm, qs), g, (gm[:M], gs[:M]), M))
        thr = float(np.median(Tn))
        assert _equal(eng.score_above(Q, g, thr, (qm, qs), (gm[:M], gs[:M])), _csr(Tn >= np.float32(thr), Tn)), (D, M)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("D", [192, 256])
def test_rows_do_not_depend_on_the_launch(eng, D, norm):
    """The same 20 rows alone (N = 20: the FEW form) and at places 70 .. 89 of a 130-query call (the MANY form), on a long and on a short
    gallery.  More than one gallery slice: the launch rule (csrc/api_search.hip, above_fused, as score_topk's) cuts the gallery so that
    a workgroup walks at least 8 blocks of 32 rows (FEW: 16) while there are fewer workgroups than twice the CUs; M = 4100 is 129
    blocks: 9 slices for the FEW launch and 17 for the one-tile MANY launch on any chip with more than 16 CUs, while M = 250 is 8
    blocks: ONE slice in both.  The hits below index 250 of the long-gallery calls must be the short-gallery calls' hits."""
    Q, G, q_stats, g_stats = _unit_rows(D)
    assert eng.lib.svhip_abi_version() == 5 and torch.cuda.get_device_properties(0).multi_processor_count > 16
    thr = 1.0 if norm else 0.15
    sl = slice(70, 90)
    perm = np.concatenate([np.arange(50, 120), np.arange(0, 50), np.arange(120, 130)])       # rows 0 .. 19 of Q sit at 70 .. 89
    qs = lambda rows: (q_stats[0][rows], q_stats[1][rows]) if norm else None
    gs = lambda M: (g_stats[0][:M], g_stats[1][:M]) if norm else None
    few = eng.score_above(Q[:20], G, thr, qs(slice(0, 20)), gs(4100))
    many = eng.score_above(Q[perm], G, thr, qs(perm), gs(4100))
    assert few[0][-1] > 20
    assert _equal(_rows(many, sl), few)
    few_short = eng.score_above(Q[:20], G[:250], thr, qs(slice(0, 20)), gs(250))
    many_short = eng.score_above(Q[perm], G[:250], thr, qs(perm), gs(250))
    assert _equal(_rows(many_short, sl), few_short)
    below = few[1] < 250
    rows = np.repeat(np.arange(20), np.diff(few[0]))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[below], minlength=20))]).astype(np.int64)
    assert few_short[0][-1] > 0 and _equal(few_short, (rp, few[1][below], few[2][below]))


# ---- 6. the slab route --------------------------------------------------------------------------------------------------------------------------
def _labels(eng, fn):
    eng.profile(True)
    try:
        out = fn()
        return out, set(eng.profile_results())
    finally:
        eng.profile(False)


@pytest.mark.parametrize("N", [1, 33, 130])
@pytest.mark.parametrize("D", [64, 512])
def test_slab_route_exact_sets(eng, D, N):
    hits, ties = _exact_sets(eng, D, N, (1, 31, 33, 1000, 4100))
    assert hits > 0 and ties > 0


def test_routes_by_width_and_alignment(eng):
    """D = 192 from a device operand 4 bytes off a 16-byte boundary takes the slab route (host operands are staged on aligned scratch),
    the aligned one the fused route; both give numpy's sets"""
    def off4(*arrays):
        out = []
        for a in arrays:
            flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
            flat[1:] = torch.from_numpy(a.reshape(-1)).cuda()
            t = flat[1:].view(a.shape)
            assert t.data_ptr() % 16 == 4
            out.append(t)
        return out

    (hits, ties), labels = _labels(eng, lambda: _exact_sets(eng, 192, 130, (33, 1000, 4100), dev=off4))
    assert hits > 0 and ties > 0
    assert {"score_above_gemm", "score_above_rows"} <= labels and not {"score_above_count", "score_above_fill"} & labels
    _, labels = _labels(eng, lambda: _exact_sets(eng, 192, 130, (1000,), dev=lambda *a: [torch.from_numpy(x).cuda() for x in a]))
    assert {"score_above_count", "score_above_scan", "score_above_fill"} <= labels and not {"score_above_gemm", "score_above_rows"} & labels
    _, labels = _labels(eng, lambda: _exact_sets(eng, 64, 33, (1000,)))
    assert {"score_above_gemm", "score_above_rows"} <= labels and not {"score_above_count", "score_above_fill"} & labels


# ---- 7. float data against float64 --------------------------------------------------------------------------------------------------------------
THR = 0.2
_F64 = {}


def _float_data(norm):
    """Unit rows, N = 130, M = 4100, D = 192, and the float64 score of every pair with its accuracy bar: 1e-6 for the cosine (svhip.h:
    a score of L2-normalised rows lies within 1e-6 of the float64 inner product); for the normalised score the bar
    tests/test_gpu_topk_norm.py derives (_bound there: the cosine's 1e-6 scaled by A = aq + ag, plus 8 roundings of 2^-24 of a term
    no larger than |s| A + |bq| + |bg|).  Pairs whose float64 score lies within the bar of THR may fall either way.  The seed is the
    first from 20261020 on whose float64 data alone leaves at most 1 % of the float64 hit set undecided (the expected number of
    undecided pairs is below one for the cosine and a handful in 10^4 hits for the normalised score)."""
    if norm not in _F64:
        for seed in range(20261020, 20261030):
            rng = np.random.default_rng(seed)
            Q = rng.standard_normal((130, 192)).astype(np.float32)
            G = rng.standard_normal((4100, 192)).astype(np.float32)
            C = rng.standard_normal((600, 192)).astype(np.float32)
            for X in (Q, G, C):
                X /= np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
            V = Q.astype(np.float64) @ G.astype(np.float64).T
            bar = np.full(V.shape, 1e-6)
            stats = None
            if norm:
                C64 = C.astype(np.float64)
                q_stats = tuple(x.astype(np.float32) for x in _stats64(Q.astype(np.float64) @ C64.T, 100))
                g_stats = tuple(x.astype(np.float32) for x in _stats64(G.astype(np.float64) @ C64.T, 100))
                aq, bq = (x.astype(np.float64) for x in _coef(*q_stats))
                ag, bg = (x.astype(np.float64) for x in _coef(*g_stats))
                A = aq[:, None] + ag[None, :]
                bar = 1e-6 * A + 8 * EPS * (np.abs(V) * A + np.abs(bq)[:, None] + np.abs(bg)[None, :])
                V = _statement(V, q_stats, g_stats)
                stats = (q_stats, g_stats)
            undecided = np.abs(V - THR) <= bar
            if undecided.sum() <= 0.01 * (V >= THR).sum():
                _F64[norm] = (Q, G, stats, V, bar, undecided)
                break
    return _F64[norm]


@pytest.mark.parametrize("norm", [False, True])
def test_float_data_against_float64(eng, norm):
    Q, G, stats, V, bar, undecided = _float_data(norm)
    n_hits = int((V >= THR).sum())
    print(f"float64 hits {n_hits}, undecided pairs {int(undecided.sum())}, largest bar {float(bar.max()):.3e}")
    assert n_hits > 100 and int(undecided.sum()) <= 0.01 * n_hits                      # at most 1 % of the float64 hit set is excluded
    rp, ix, sc = eng.score_above(Q, G, THR, *(stats or ()))
    rows = np.repeat(np.arange(130), np.diff(rp))
    got = np.zeros(V.shape, bool)
    got[rows, ix] = True
    assert got.sum() == ix.size                                                          # no pair twice
    assert all(np.all(np.diff(ix[rp[n]:rp[n + 1]]) > 0) for n in range(130))            # ascending index
    decided = ~undecided
    assert np.array_equal(got[decided], (V >= THR)[decided])
    err = np.abs(sc.astype(np.float64) - V[rows, ix])
    print(f"max |score - float64| = {float(err.max()):.3e}, worst err / bar {float((err / bar[rows, ix]).max()):.3f}")
    assert np.all(err <= bar[rows, ix])
    assert np.all(sc >= np.float32(THR))


# ---- 8. the fill guard --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("D", [192, 64])
def test_fill_refuses_a_row_ptr_of_other_inputs(eng, D, space):
    """host: the library stages the outputs and copies row_ptr[N] entries back, so the caller's arrays show what the HOST side does.
    device: the kernels write straight into the caller's allocations - the outputs are the middle of two larger tensors with PAD canary
    entries before and behind, so a store outside [0, row_ptr[N]) by the fill or row kernel (D = 192: fused route, D = 64: slab route)
    lands on a canary."""
    Q, G, _, _ = _int_cols(D)
    N, M, PAD = 130, 1000, 64
    Q, G = Q[:N], G[:M]
    S = Q.astype(np.float64) @ G.astype(np.float64).T
    thr = _occurring(S, 0.95)
    lib, none = eng.lib, [None] * 4
    on_dev = space == "device"
    flags = (_lib.IN_DEVICE | _lib.OUT_DEVICE) if on_dev else 0
    hold = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda() if on_dev else np.ascontiguousarray(a)
    ptr = lambda x, skip=0: (x.data_ptr() if on_dev else x.ctypes.data) + skip * x.itemsize
    host = lambda x: x.cpu().numpy() if on_dev else x
    ready = torch.cuda.synchronize if on_dev else (lambda: None)
    q, g, cnt = hold(Q), hold(G), hold(np.zeros(N, np.int64))
    ready()
    assert lib.svhip_score_above_count(eng.h, ptr(q), N, ptr(g), M, D, thr, *none, 0, 0, ptr(cnt), flags) == 0
    count = host(cnt)
    assert np.array_equal(count, (S >= thr).sum(axis=1))
    rp, total = Engine._above_row_ptr(count, 2 ** 28)
    index, score = hold(np.full(total + 2 * PAD, -7, np.int32)), hold(np.full(total + 2 * PAD, -7.0, np.float32))
    row_ptr, shifted = hold(rp), hold(rp + 1)
    ready()
    fill = lambda t, r: lib.svhip_score_above_fill(eng.h, ptr(q), N, ptr(g), M, D, t, *none, 0, 0, ptr(r), ptr(index, PAD), ptr(score, PAD), flags)
    untouched = lambda: bool(np.all(host(index) == -7) and np.all(host(score) == -7.0))
    # the threshold moved between the calls: more hits than row_ptr has room for in most rows, fewer with the higher one
    for other in (thr - 3.0, thr + 3.0):
        first_bad = int(np.nonzero((S >= other).sum(axis=1) != count)[0][0])
        rc = fill(other, row_ptr)
        assert rc == -1                                 # SVHIP_ERR_INVALID
        with pytest.raises(_lib.SvhipError, match=rf"score_above: row {first_bad} .*changed between count and fill"):
            eng._ck(rc)
        assert untouched()                              # nothing was written, inside the outputs or around them
    # a row_ptr that does not start at 0 is refused as row 0
    rc = fill(thr, shifted)
    assert rc == -1 and untouched()
    with pytest.raises(_lib.SvhipError, match="score_above: row 0 "):
        eng._ck(rc)
    # the same inputs fill exactly [0, total): the canaries on both sides are intact
    assert fill(thr, row_ptr) == 0
    ix, sc = host(index), host(score)
    for x, c in ((ix, -7), (sc, -7.0)):
        assert np.all(x[:PAD] == c) and np.all(x[PAD + total:] == c)
    assert _equal((rp, ix[PAD:PAD + total], sc[PAD:PAD + total]), _csr(S >= thr, S))


def test_device_pointers(eng):
    Q, G, (qm, qs), (gm, gs), _, T = _int_data(192)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    thr = _occurring(T[:130, :1000])
    got = eng.score_above(dev(Q[:130]), dev(G[:1000]), thr, (dev(qm[:130]), dev(qs[:130])), (dev(gm[:1000]), dev(gs[:1000])))
    assert all(torch.is_tensor(x) and x.is_cuda for x in got)
    assert _equal(got, _csr(T[:130, :1000] >= thr, T[:130, :1000]))
    with pytest.raises(ValueError):
        eng.score_above(dev(Q[:130]), G[:1000], thr)                                    # one memory space per call
    with pytest.raises(ValueError, match="exceed max_hits = 10"):
        eng.score_above(dev(Q[:130]), dev(G[:1000]), -np.inf, max_hits=10)


# ---- 9. matches / duplicates on the committed speaker fixture -----------------------------------------------------------------------------------
def test_matches_and_duplicates_on_the_speaker_fixture(tmp_path):
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
    out = os.path.join(tmp, "prep")
    os.makedirs(out)
    assert mh.prepare(save_path=out, prepare_type="embed", num_eval=4, source=root) is True
    probe = list(files[:6])
    n_class = 3
    cohort = np.random.default_rng(64).standard_normal((64, 192))
    cohort = (cohort / np.linalg.norm(cohort, axis=1, keepdims=True)).astype(np.float32)
    for kw in ({}, dict(scoring_mode="norm", cohorts=cohort, cohort_top=8)):
        scores, index, names = mh.identify(probe, out, top=n_class, num_eval=4, **kw)
        flat = np.sort(scores.ravel())
        some = 0
        for thr in (float(flat[0]), float(flat[len(flat) // 2]), float(0.5 * (flat[-2] + flat[-1])), float(flat[-1]) + 1.0):
            ms, mi, mn = mh.matches(probe, out, thr, num_eval=4, **kw)
            for n in range(len(probe)):
                keep = scores[n] >= np.float32(thr)                                     # identify reports them best first: a prefix
                assert np.array_equal(mi[n], index[n][keep]) and np.array_equal(ms[n].view(np.uint32), scores[n][keep].view(np.uint32)), (kw, thr, n)
                assert mn[n] == [names[n][c] for c in np.nonzero(keep)[0]]
                some += int(keep.sum())
        assert some >= len(probe) * n_class                                            # (the lowest threshold returns everything)
    # duplicates: the six files' own embeddings as a gallery, rows 1 and 4 enrolled a second time
    rows = np.stack([mh.embed_utterance(f, num_eval=4, normalize=True).numpy().mean(axis=0) for f in probe]).astype(np.float32)
    gallery = np.concatenate([rows, rows[[1, 4]]])
    unit = gallery.astype(np.float64) / np.linalg.norm(gallery.astype(np.float64), axis=1, keepdims=True)
    C = unit @ unit.T
    # the threshold is picked here, from the float64 cosines alone: half way between the closest pair of DIFFERENT rows and the copies'
    # cosine of 1, so that the float64 data gives exactly the two copied pairs - with room for the fp32 score on either side
    iu, ju = np.triu_indices(8, 1)
    copies = [(1, 6), (4, 7)]
    others = max(C[a, b] for a, b in zip(iu, ju) if (int(a), int(b)) not in copies)
    assert 1.0 - others > 1e-5
    thr = 0.5 * (others + 1.0)
    want = [(int(a), int(b)) for a, b in zip(iu, ju) if C[a, b] >= thr]
    assert want == copies
    i, j, s, pairs = mh.duplicates(gallery, thr, classes=[f"e{c}" for c in range(8)])
    assert list(zip(i.tolist(), j.tolist())) == [(1, 6), (4, 7)]                        # exactly the copied pairs
    assert np.all(s >= np.float32(thr)) and pairs == [(f"e{a}", f"e{b}") for a, b in want]
    i2, j2, s2 = mh.duplicates(gallery, thr, chunk=3)                                   # in query chunks: the same pairs
    assert np.array_equal(i2, i) and np.array_equal(j2, j) and np.array_equal(s2.view(np.uint32), s.view(np.uint32))
