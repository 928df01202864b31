"""GPU: two-set clustering (svhip_cluster_join, Engine.cluster_join, scoring.cluster_join, ModelHandling.cluster_extend) against its
statement (svhip.h, "cluster_join"; tests/cluster_join_statement.py).

The joint rows are A's, then B's.  The links are the seed links of every seeded side, the pairs inside every unseeded side and every
pair of the rectangle A x B at or above thr; the clusters are the components in the canonical form, so every comparison is exact.  The
six routes are tests/test_gpu_cluster.py's: D in {192, 256} with aligned operands takes the fused route, everything else the slab
route.  tests/test_cluster_join_host.py proves without a GPU that none of the data has a pair within the accuracy bar of its threshold
and that every split's statement is the whole set's; it also runs the seed clamp's host check (svhip_selftest)."""
import os

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, engine as sv_engine, synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
from tests import cluster_join_statement as cj
from tests import cluster_statement as cs
from tests.test_gpu_cluster import ROUTE_IDS, ROUTES, _fused_parts, _off4, _same

pytestmark = pytest.mark.gpu
routes = pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def eng():
    return Engine(model="none", max_batch=1)


def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def _sides(E, NA, route, stats=None):
    """the two sides of a cut as the route wants them: host arrays (aligned scratch), or views of ONE device tensor 4 bytes off a 16-byte
    boundary (NA * D * 4 is a multiple of 16: both sides are off by 4) -> (A, B, a_stats, b_stats)"""
    cut = lambda lo, hi: None if stats is None else tuple(np.ascontiguousarray(x[lo:hi]) for x in stats)
    sa, sb = cut(0, NA), cut(NA, None)
    if not route[1]:
        return np.ascontiguousarray(E[:NA]), np.ascontiguousarray(E[NA:]), sa, sb
    t = _off4(E) if E.shape[0] else dev(E)
    to = lambda s: None if s is None else tuple(dev(x) for x in s)
    return t[:NA], t[NA:], to(sa), to(sb)


def _join(eng, E, NA, thr, route, mode="none", stats=None, roots=None):
    """the join of E cut at NA -> (root, cluster, C) as numpy / int.  mode: which sides are seeded with eng.cluster_above's roots of that
    side alone ("none", "a", "ab"); roots = (root_a, root_b): host seeds given outright"""
    A, B, sa, sb = _sides(E, NA, route, stats)
    if roots is not None:
        ra, rb = (None if r is None else (dev(np.asarray(r, np.int32)) if route[1] else np.asarray(r, np.int32)) for r in roots)
    else:
        ra = eng.cluster_above(A, thr, sa)[0] if mode in ("a", "ab") else None
        rb = eng.cluster_above(B, thr, sb)[0] if mode == "ab" else None
    root, cluster, C = eng.cluster_join(A, B, thr, ra, rb, sa, sb)
    return _host(root), _host(cluster), int(C)


def _whole(eng, E, thr, route, stats=None):
    if not route[1]:
        return eng.cluster_above(E, thr, stats)
    st = None if stats is None else tuple(dev(x) for x in stats)
    root, cluster, C = eng.cluster_above(_off4(E), thr, st)
    return _host(root), _host(cluster), int(C)


# ---- 1. splits of every graph shape -------------------------------------------------------------------------------------------------------
@routes
def test_splits_of_every_graph_shape(eng, route):
    """NA = 0 .. 33: the FEW form of the rectangle and its edge; 128: one MANY tile; 129, 161: a MANY tile and a FEW tail / a partial tile,
    and offsets that are no multiple of 32; 299: one gallery row; 300: no B at all.  Every seed mode must give the shape's own labelling,
    which is also cluster_above's of the concatenation.  The permuted and reversed paths make B rows bridge A clusters."""
    D = route[0]
    for name, (E, thr, lab) in cj.split_cases(D).items():
        want = cs.canonical(lab)
        assert _same(_whole(eng, E, thr, route), want), name
        for NA in sorted({min(c, E.shape[0]) for c in cj.CUTS}):
            for mode in cj.MODES:
                assert _same(_join(eng, E, NA, thr, route, mode), want), (name, NA, mode)


# ---- 2. seeds are trusted, not rescored ---------------------------------------------------------------------------------------------------
@routes
def test_seeds_are_trusted_not_rescored(eng, route):
    D = route[0]
    e = np.eye(64, D, dtype=np.float32)
    # 70 rows of A: rows 0 .. 39 are ONE value (e_0), seeded as singletons; rows 40 .. 69 are orthogonal (e_1 .. e_30), seeded as one
    # cluster under row 40; B: 35 rows near none of them (e_40 .. e_50 repeated)
    A = np.concatenate([e[np.zeros(40, int)], e[1 + np.arange(30)]])
    B = e[40 + np.arange(35) % 11]
    flat = np.concatenate([np.arange(40), np.full(30, 40)])
    got = _join(eng, np.concatenate([A, B]), 70, 0.5, route, roots=(flat, None))
    want = cj.join_statement(A, B, 0.5, flat, None)
    assert _same(got, want)
    assert got[0][:40].tolist() == list(range(40))                   # identical rows seeded apart stay apart: A x A is not walked
    assert np.all(got[0][40:70] == 40)                               # orthogonal rows seeded together stay together
    assert got[2] == 40 + 1 + 11                                     # B's own pairs ARE scored: 11 clusters of its repeated rows
    # a downward chain inside the group is its flat form
    chain = np.concatenate([np.arange(40), [40], 40 + np.arange(29)])
    assert _same(_join(eng, np.concatenate([A, B]), 70, 0.5, route, roots=(chain, None)), want)
    # one B row that scores above thr against two separate A clusters merges them under the smaller root
    bridge = ((e[0] + e[7]) / np.sqrt(2.0)).astype(np.float32)[None]
    got = _join(eng, np.concatenate([A, bridge]), 70, 0.5, route, roots=(flat, None))
    assert _same(got, cj.join_statement(A, bridge, 0.5, flat, None))
    assert np.all(got[0][:40] == 0) and np.all(got[0][40:] == 0) and got[2] == 1       # 40 singletons of e_0 and the group holding e_7


# ---- 3. the profile -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NA,NB", [(300, 20), (1044, 300), (1044, 1100), (16384 + 148, 161), (161, 16384 + 148), (16384 + 148, 16384 + 200)])
def test_profile_of_the_fused_route(eng, NA, NB):
    """One launch per part of the rectangle's plan, whose query side is the smaller side (A where they are equal)."""
    E, thr, lab = cs.shared_coordinate_rows(NA + NB, 192)
    ra, rb = eng.cluster_above(E[:NA], thr)[0], eng.cluster_above(E[NA:], thr)[0]
    queries = NB if NB < NA else NA
    assert [_fused_parts(min(a, b)) for a, b in ((300, 20), (1044, 300), (1044, 1100), (16384 + 148, 161), (161, 16384 + 148), (16384 + 148, 16384 + 200))] == [1, 1, 2, 1, 1, 3]

    def profiled(root_b):
        eng.profile(True)
        try:
            got = eng.cluster_join(E[:NA], E[NA:], thr, ra, root_b)
            return got, eng.profile_results()
        finally:
            eng.profile(False)

    got, labels = profiled(None)
    assert _same(got, cs.canonical(lab))
    assert labels["cluster_join_link"]["launches"] == _fused_parts(queries)       # one launch per part of the A x B plan
    assert labels["cluster_join_self"]["launches"] == _fused_parts(NB)            # B's self-join: its own launches
    assert labels["cluster_join_link"]["flops"] == 2.0 * NA * NB * 192
    assert {"cluster_seed", "cluster_flatten", "cluster_ids"} <= set(labels) and "cluster_init" not in labels
    bad = ("score_above", "cluster_gemm", "cluster_link", "cluster_join_gemm", "cluster_join_rows", "cluster_join_self_")
    assert not [k for k in labels if k.startswith(bad)]
    got, labels = profiled(rb)
    assert _same(got, cs.canonical(lab))
    assert labels["cluster_join_link"]["launches"] == _fused_parts(queries) and "cluster_join_self" not in labels  # both seeded: no self-join


@pytest.mark.parametrize("D", [192, 256])
def test_fused_score_is_symmetric_in_its_bits(eng, D):
    """What lets the fused rectangle take the smaller side as its queries: v(a, b) as the walk computes it for the query a and the gallery
    row b has the bits of v(b, a) - plain and normalised, in the FEW and in the MANY form (33 x 300: one form each way)."""
    E, _, _ = synth.synth_speaker_embeddings(333, n_speakers=40, dim=D, seed=9)
    rng = np.random.default_rng(D)
    stats = (rng.standard_normal(333).astype(np.float32), (0.5 + rng.random(333)).astype(np.float32))
    A, B = E[:33], E[33:]
    for sa, sb in ((None, None), (tuple(x[:33] for x in stats), tuple(x[33:] for x in stats))):
        rp, ix, ab = eng.score_above(A, B, -np.inf, sa, sb)
        rp2, ix2, ba = eng.score_above(B, A, -np.inf, sb, sa)
        assert ix.size == ix2.size == 33 * 300 and np.array_equal(np.diff(rp), np.full(33, 300))
        assert np.array_equal(ab.reshape(33, 300).view(np.uint32), ba.reshape(300, 33).T.view(np.uint32))


# ---- 4. second chunk and offsets ----------------------------------------------------------------------------------------------------------
@routes
def test_second_chunk_and_offsets(eng, route):
    """NA = 16 417: A is two plan chunks, the second a 33-row tail (the slab route walks it as the queries; the fused route takes the
    smaller side, B, as its queries and A as a gallery of 514 blocks behind them).  NA = 161: B's chunked self-join, with its diagonal
    skip, runs behind an offset of 161.  Exact data (scores 0, 1, 2; thr = 1)."""
    E, thr, lab = cs.shared_coordinate_rows(16384 + 33 + 161, route[0])
    want = cs.canonical(lab)
    for NA in (16417, 161):
        for mode in ("a", "ab"):
            assert _same(_join(eng, E, NA, thr, route, mode), want), (NA, mode)


@pytest.mark.parametrize("route", ROUTES[:2], ids=ROUTE_IDS[:2])
def test_second_chunk_of_the_fused_rectangles_query_side(eng, route):
    """Both sides 16 417 rows: the rectangle's query side (A: the sides are equal) runs two plan chunks, the second a 33-row tail whose
    links carry the chunk's row base, against a gallery behind an offset that is no multiple of 32; both sides seeded, so the rectangle
    alone joins what the cut separates."""
    E, thr, lab = cs.shared_coordinate_rows(2 * 16417, route[0])
    assert _same(_join(eng, E, 16417, thr, route, "ab"), cs.canonical(lab))


# ---- 5. exact integer data with ties at thr -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@routes
def test_exact_integer_data(eng, route, norm):
    E, stats = cs.int_rows(300, route[0])
    stats = stats if norm else None
    cut = lambda lo, hi: None if stats is None else tuple(x[lo:hi] for x in stats)
    V = cs.scores64(E, stats)
    ties = 0
    for q in (0.9995, 0.999, 0.99):
        t0 = cs.occurring(V, q)
        ties += int((V[:139, 139:] == t0).sum())
        for thr in (t0, t0 + (0.125 if norm else 0.5)):                    # a value that occurs, and one strictly between two values
            for mode in cj.MODES:
                ra, rb = cj.seeds(E, 139, thr, mode, stats)
                want = cj.join_statement(E[:139], E[139:], thr, ra, rb, cut(0, 139), cut(139, None))
                assert _same(_join(eng, E, 139, thr, route, stats=stats, roots=(ra, rb)), want), (q, thr, mode)
                assert _same(want, cs.statement(E, thr, stats))
    assert ties > 0                                                        # ties AT thr inside the rectangle


# ---- 6. contention ------------------------------------------------------------------------------------------------------------------------
@routes
def test_contention(eng, route):
    E = np.zeros((2048, route[0]), np.float32)
    E[:, 3] = 1.0                                           # 10^6 cross links onto one root
    roots = (np.arange(1024), np.arange(1024))              # both sides seeded as singletons: only the rectangle links
    root, cluster, C = _join(eng, E, 1024, 0.5, route, roots=roots)
    assert C == 1 and not root.any() and not cluster.any()


# ---- 7. edge values -----------------------------------------------------------------------------------------------------------------------
@routes
def test_edge_values(eng, route):
    D = route[0]
    E, _ = cs.int_rows(200, D)
    NA = 77
    one = (np.zeros(200, np.int32), np.zeros(200, np.int32), 1)
    ident = (np.arange(200, dtype=np.int32), np.arange(200, dtype=np.int32), 200)
    for mode in cj.MODES:
        assert _same(_join(eng, E, NA, -np.inf, route, mode), one)
        assert _same(_join(eng, E, NA, np.inf, route, mode), ident)
    # rows holding a NaN, one on either side, are singletons - even at thr = -inf - and break no other cluster
    En = E.copy()
    En[7, 3] = np.nan
    En[150, D - 1] = np.nan
    thr = cs.occurring(cs.scores64(E), 0.999)
    rest = np.delete(np.arange(200), [7, 150])
    with np.errstate(invalid="ignore"):
        want = cs.statement(En, thr)
        assert want[0][7] == 7 and want[0][150] == 150
        for mode in cj.MODES:
            ra, rb = cj.seeds(En, NA, thr, mode)
            assert _same(_join(eng, En, NA, thr, route, roots=(ra, rb)), want), mode
        got = _join(eng, En, NA, -np.inf, route)
    assert got[2] == 3 and got[0][7] == 7 and got[0][150] == 150 and not got[0][rest].any()
    # an all-zero row of B at thr = 0 links to every row of A: +0 >= 0, and the zeros of a product with -0.0
    N = 40
    Z = np.zeros((N, D), np.float32)
    Z[np.arange(N - 1), 1 + np.arange(N - 1)] = 1.0
    Z[:N - 1, 0] = np.where(np.arange(N - 1) % 2 == 0, 2.0, -2.0)          # even rows score +4 among themselves, -4 against odd rows
    assert _same(_join(eng, Z[:N - 1], 20, 0.0, route), cs.canonical(np.arange(N - 1) % 2))
    Z[N - 1, ::2] = -0.0
    assert _same(_join(eng, Z, N - 1, 0.0, route, "a"), (np.zeros(N, np.int32), np.zeros(N, np.int32), 1))
    # an empty side, and both: one side alone, seeded (no walk at all) or walked
    E3, thr3, lab3 = cs.graph_shapes(161, D)["path_permuted"]
    want = cs.canonical(lab3)
    for NA in (0, 161):
        for mode in cj.MODES:
            assert _same(_join(eng, E3, NA, thr3, route, mode), want), (NA, mode)
    # (a seeded side alone comes back as its seed says)
    assert _same(_join(eng, E3, 161, thr3, route, roots=(np.arange(161) // 2 * 2, None)), cs.canonical(np.arange(161) // 2))
    got = _join(eng, E3[:0], 0, thr3, route)
    assert got[0].shape == got[1].shape == (0,) and got[2] == 0


# ---- 8. seed checking ---------------------------------------------------------------------------------------------------------------------
def test_host_seeds_are_checked_on_the_host(eng):
    lib, h = eng.lib, eng.h
    E, thr, _ = cs.graph_shapes(40, 192)["two_paths"]
    A, B = np.ascontiguousarray(E[:25]), np.ascontiguousarray(E[25:])
    root, cluster, n = np.full(40, -7, np.int32), np.full(40, -7, np.int32), np.full(1, -7, np.int64)
    p = lambda a: None if a is None else a.ctypes.data
    good_a, good_b = np.arange(25, dtype=np.int32), np.arange(15, dtype=np.int32)
    for which, at, value, text in (("a", 2, 5, r"cluster_join: root_a\[2\] = 5 is outside \[0, 2\]"),
                                   ("a", 24, -1, r"cluster_join: root_a\[24\] = -1 is outside \[0, 24\]"),
                                   ("b", 0, 1, r"cluster_join: root_b\[0\] = 1 is outside \[0, 0\]"),
                                   ("b", 14, -2 ** 31, r"cluster_join: root_b\[14\] = -2147483648 is outside \[0, 14\]")):
        ra, rb = good_a.copy(), good_b.copy()
        (ra if which == "a" else rb)[at] = value
        eng.profile(True)
        try:
            rc = lib.svhip_cluster_join(h, p(A), 25, p(ra), p(B), 15, p(rb), 192, thr, None, None, None, None, p(root), p(cluster), p(n), 0)
            launched = eng.profile_results()
        finally:
            eng.profile(False)
        assert rc == -1 and not launched                     # SVHIP_ERR_INVALID, and nothing was launched
        with pytest.raises(_lib.SvhipError, match=text):
            eng._ck(rc)
        assert np.all(root == -7) and np.all(cluster == -7) and n[0] == -7
    with pytest.raises(_lib.SvhipError, match=r"root_a\[1\] = 2"):
        eng.cluster_join(A, B, thr, root_a=np.array([0, 2] + [0] * 23, np.int32))


def test_device_seeds_outside_their_range_are_read_as_the_row_itself(eng):
    """N = 40, once: device seeds cannot be checked on the host, so an entry above i or below 0 is read as i by the seed kernel - through
    the clamp function that svhip_selftest exercises on the CPU (tests/test_cluster_join_host.py), and which keeps parent[x] <= x."""
    assert eng.lib.svhip_selftest() == 0
    E, thr, _ = cs.graph_shapes(40, 192)["two_paths"]
    ra = np.arange(25) % 2                                  # A's even rows under row 0, its odd rows under row 1 ...
    ra[[4, 9, 24]] = [5, -1, 2 ** 31 - 1]                   # ... but three entries are no seeds at all
    rb = np.zeros(15, np.int64)
    rb[[0, 3]] = [-2 ** 31, 40]
    got = eng.cluster_join(dev(E[:25]), dev(E[25:]), 2.0, dev(ra.astype(np.int32)), dev(rb.astype(np.int32)))       # thr = 2: no score links
    want = cj.join_statement(E[:25], E[25:], 2.0, ra, rb)
    assert _same((_host(got[0]), _host(got[1]), int(got[2])), want)
    assert want[0][[4, 9, 24]].tolist() == [4, 9, 24] and want[0][25] == 25 and want[0][28] == 25 + 3 and want[0][26] == 25


# ---- 9. plumbing --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 64])
def test_device_tensors_stay_on_the_device(eng, D):
    E, stats = cs.int_rows(300, D)
    thr = cs.occurring(cs.scores64(E, stats), 0.999)
    Ed, st = dev(E), tuple(dev(x) for x in stats)
    ra = eng.cluster_above(Ed[:139], thr, tuple(x[:139] for x in st))[0]
    torch.cuda.synchronize()
    before = dict(sv_engine.TRANSFER_STATS)
    root, cluster, C = eng.cluster_join(Ed[:139], Ed[139:], thr, ra, None, tuple(x[:139] for x in st), tuple(x[139:] for x in st))
    assert dict(sv_engine.TRANSFER_STATS) == before                                        # nothing staged, nothing copied back
    assert all(torch.is_tensor(x) and x.is_cuda for x in (root, cluster, C)) and C.dtype == torch.int64 and C.dim() == 0
    want = cs.statement(E, thr, stats)
    assert _same((_host(root), _host(cluster), int(C)), want)
    again = eng.cluster_join(Ed[:139], Ed[139:], thr, ra, None, tuple(x[:139] for x in st), tuple(x[139:] for x in st))
    assert torch.equal(again[0], root) and torch.equal(again[1], cluster) and int(again[2]) == int(C)      # the same bits twice
    with pytest.raises(ValueError):
        eng.cluster_join(Ed[:139], E[139:], thr)                                           # one memory space per call


def test_raw_abi_null_cluster_async_and_refusals(eng):
    lib, h = eng.lib, eng.h
    E, stats = cs.int_rows(300, 192)
    thr = cs.occurring(cs.scores64(E), 0.999)
    want = cs.statement(E, thr)
    A, B = np.ascontiguousarray(E[:139]), np.ascontiguousarray(E[139:])
    root, n = np.full(300, -7, np.int32), np.full(1, -7, np.int64)
    p = lambda a: None if a is None else a.ctypes.data
    # out_cluster = NULL: roots and the count alone
    assert lib.svhip_cluster_join(h, p(A), 139, None, p(B), 161, None, 192, thr, None, None, None, None, p(root), None, p(n), 0) == 0
    assert np.array_equal(root, want[0]) and int(n[0]) == want[2]
    # the same through device pointers, asynchronously, with a device seed
    Ad, Bd = dev(A), dev(B)
    ra = eng.cluster_above(Ad, thr)[0]
    rd, nd = torch.full((300,), -7, dtype=torch.int32, device="cuda"), torch.full((1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    flags = _lib.IN_DEVICE | _lib.OUT_DEVICE | _lib.ASYNC
    assert lib.svhip_cluster_join(h, Ad.data_ptr(), 139, ra.data_ptr(), Bd.data_ptr(), 161, None, 192, thr, None, None, None, None,
                                  rd.data_ptr(), None, nd.data_ptr(), flags) == 0
    eng.synchronize()
    assert np.array_equal(rd.cpu().numpy(), want[0]) and int(nd[0]) == want[2]
    # refusals: by name, before any copy or launch - the outputs keep their canaries
    root[:], n[:] = -7, -7
    cluster = np.full(300, -7, np.int32)
    s = [np.ascontiguousarray(x) for x in (stats[0][:139], stats[1][:139], stats[0][139:], stats[1][139:])]
    call = lambda NA=139, NB=161, D=192, thr=thr, A=A, B=B, st=(None,) * 4, root=root, n=n: lib.svhip_cluster_join(
        h, p(A), NA, None, p(B), NB, None, D, thr, *[p(x) for x in st], p(root), p(cluster), p(n), 0)
    for kw, code, text in ((dict(thr=float("nan")), -1, "cluster_join: the threshold is NaN"),
                           (dict(D=0), -1, "cluster_join: D = 0 must be at least 1"),
                           (dict(D=48), -5, "cluster_join: embedding dim 48 must be a multiple of 32"),
                           (dict(NA=-1), -1, "cluster_join: NA = -1 is negative"),
                           (dict(NB=-3), -1, "cluster_join: NB = -3 is negative"),
                           (dict(NA=2 ** 31 - 100), -1, "cluster_join: NA \\+ NB = 2147483548 \\+ 161 is outside"),
                           (dict(NB=2 ** 31), -1, "cluster_join: NA \\+ NB = 139 \\+ 2147483648 is outside"),
                           (dict(A=None), -1, "cluster_join: NULL pointer"),
                           (dict(B=None), -1, "cluster_join: NULL pointer"),
                           (dict(root=None), -1, "cluster_join: NULL pointer"),
                           (dict(n=None), -1, "cluster_join: NULL pointer"),
                           (dict(st=(s[0], s[1], None, None)), -1, "cluster_join: 2 of the four statistic arrays are NULL"),
                           (dict(st=(s[0], s[1], s[2], None)), -1, "cluster_join: 1 of the four statistic arrays are NULL"),
                           (dict(st=(None, None, None, s[3])), -1, "cluster_join: 3 of the four statistic arrays are NULL")):
        rc = call(**kw)
        assert rc == code, kw                               # SVHIP_ERR_INVALID / SVHIP_ERR_UNSUPPORTED
        with pytest.raises(_lib.SvhipError, match=text):
            eng._ck(rc)
        assert np.all(root == -7) and np.all(cluster == -7) and n[0] == -7, kw
    # NA + NB = 0: OK, C = 0, nothing else touched; a NULL side is legal where it has no rows
    assert call(NA=0, NB=0, A=None, B=None, root=None) == 0 and n[0] == 0 and np.all(cluster == -7)
    assert call(NA=0, A=None) == 0 and int(n[0]) == cs.statement(B, thr)[2]
    assert int(eng.cluster_join(Ad[:0], Bd[:0], thr)[2]) == 0


# ---- 10. model level ----------------------------------------------------------------------------------------------------------------------
def test_model_cluster_extend_on_the_speaker_fixture(tmp_path, golden_dir):
    """The fixture and the threshold of test_model_cluster_on_the_speaker_fixture, with its margin check: cluster the first four files,
    extend with the other four, and get what clustering all eight gives."""
    from tests.e2e_data import E2E2_SEED_W, make_e2e_speaker_files
    from tests.test_gpu_e2e import ARGS
    tmp = str(tmp_path)
    g = np.load(os.path.join(golden_dir, "e2e_speakers.npz"))
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    rows = unit(unit(g["embeddings_ne2"].astype(np.float64)).mean(axis=1))
    S = rows @ rows.T
    v = np.sort(S[np.triu_indices(rows.shape[0], 1)])
    k = int(np.argmax(np.diff(v)))
    thr = float(0.5 * (v[k] + v[k + 1]))
    assert 0.5 * (v[k + 1] - v[k]) > 10 * (4e-4 + cs.BAR)

    args = dict(ARGS, save_folder=tmp)
    net = WrappedModel(SpeakerEncoder(**args))
    mh = ModelHandling(net, **args)
    sd = synth.synth_state_dict(synth.ecapa_param_spec(C=512), seed=E2E2_SEED_W)
    sd["asp_bn.norm.running_mean"] = g["asp_bn_running_mean"]
    sd["asp_bn.norm.running_var"] = g["asp_bn_running_var"]
    net.module.load_state_dict({"__S__." + k_: v_ for k_, v_ in sd.items()})
    files, _, _ = make_e2e_speaker_files(tmp)
    model_rows = np.stack([mh.embed_utterance(f, num_eval=2, normalize=True).numpy().mean(axis=0) for f in files]).astype(np.float32)
    base_labels, _ = mh.cluster(source=files[:4], thresh_score=thr, num_eval=2)
    all_labels, _ = mh.cluster(source=files, thresh_score=thr, num_eval=2)
    base_ids, new_ids, merged = mh.cluster_extend(model_rows[:4], base_labels, source=files[4:], thresh_score=thr, num_eval=2)
    assert base_ids.dtype == new_ids.dtype == np.int32
    assert np.concatenate([base_ids, new_ids]).tolist() == all_labels.tolist()
    want_merged = {}
    for c, lab in zip(base_ids.tolist(), base_labels.tolist()):
        want_merged.setdefault(c, set()).add(lab)
    assert merged == [sorted(x) for _, x in sorted(want_merged.items()) if len(x) > 1]
    # base_labels = None: every base row starts alone, against the statement over the fixture's own rows
    base_ids, new_ids, merged = mh.cluster_extend(model_rows[:4], None, source=files[4:], thresh_score=thr, num_eval=2)
    want = cj.join_statement(rows[:4], rows[4:], thr, np.arange(4), None)
    assert np.concatenate([base_ids, new_ids]).tolist() == want[1].tolist()
    assert merged == [sorted(np.nonzero(want[1][:4] == c)[0].tolist()) for c in range(want[2]) if (want[1][:4] == c).sum() > 1]
