"""GPU: speaker clustering (svhip_cluster_above, Engine.cluster_above, scoring.cluster, ModelHandling.cluster) against its statement.

Statement (svhip.h): rows i < j are linked iff v(i, j) >= thr, v as score_above computes it for Q = G = E; a cluster is a connected
component; root[i] = the smallest row of i's cluster, cluster[i] the dense id in order of the smallest member, C their number.  The
canonical form leaves no freedom, so every comparison is exact, on root, cluster and C.  D in {192, 256} with an aligned E takes the
fused route (one link launch per part of the plan), everything else the slab route; every test runs on both unless it says otherwise.
The data comes from tests/cluster_statement.py; tests/test_cluster_host.py proves without a GPU that none of it has a pair within the
accuracy bar of its threshold, so the float64 statement decides every pair."""
import os

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, engine as sv_engine, synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
from tests import cluster_statement as cs

pytestmark = pytest.mark.gpu

# (D, E handed over as a device tensor 4 bytes off a 16-byte boundary): two fused routes, four slab routes
ROUTES = [(192, False), (256, False), (64, False), (320, False), (512, False), (192, True)]
ROUTE_IDS = ["fused192", "fused256", "slab64", "slab320", "slab512", "slab192_unaligned"]
SIZES = (1, 2, 31, 32, 33, 128, 129, 160, 161, 300)
routes = pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)


@pytest.fixture(scope="module")
def eng():
    return Engine(model="none", max_batch=1)


def _off4(a):
    flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    t = flat[1:].view(a.shape)
    assert t.data_ptr() % 16 == 4
    return t


def _cluster(eng, E, thr, route, stats=None):
    """-> (root, cluster, C) as numpy / int, from host arrays (aligned scratch) or from the unaligned device view"""
    if not route[1]:
        return eng.cluster_above(E, thr, stats)
    st = None if stats is None else tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in stats)
    root, cluster, C = eng.cluster_above(_off4(E), thr, st)
    return root.cpu().numpy(), cluster.cpu().numpy(), int(C)


def _same(got, want):
    root, cluster, C = got
    assert root.dtype == np.int32 and cluster.dtype == np.int32 and isinstance(C, int)
    return np.array_equal(root, want[0]) and np.array_equal(cluster, want[1]) and C == want[2]


# ---- 1. graph shapes at every size ------------------------------------------------------------------------------------------------------
@routes
def test_graph_shapes_at_every_size(eng, route):
    """N = 1 .. 33: the FEW form and its edge; 128: one MANY tile; 129, 160: MANY + a FEW tail; 161, 300: a partial last tile.  Paths in
    index order, reversed and permuted (long climbs, hooks in every order), two interleaved paths, a perfect matching; a star whose
    centre is the last row."""
    D = route[0]
    for N in SIZES:
        for name, (E, thr, lab) in cs.graph_shapes(N, D).items():
            assert _same(_cluster(eng, E, thr, route), cs.canonical(lab)), (name, N)
    E, thr, lab = cs.star(D)
    got = _cluster(eng, E, thr, route)
    assert _same(got, cs.canonical(lab)) and got[2] == 1 and not got[0].any()


@routes
def test_second_query_chunk_and_a_few_part_behind_it(eng, route):
    """N = 16 384 + 33: the fused plan runs a full chunk of 128 MANY tiles and, from row 16 384 on, a second launch - 33 rows are one
    MANY tile, one row past the FEW form's 32 - whose every row must find its cluster's root in the first chunk.  N = 16 384 + 20 puts
    a FEW launch behind the full chunk.  Exact data (scores 0, 1, 2; thr = 1), millions of links among 1.3 10^8 pairs."""
    E, thr, lab = cs.shared_coordinate_rows(16384 + 33, route[0])
    assert _same(_cluster(eng, E, thr, route), cs.canonical(lab))
    # ... and 16 384 + 20: the part behind the full chunk is a FEW launch
    assert _same(_cluster(eng, E[:16384 + 20], thr, route), cs.canonical(lab[:16384 + 20]))


# ---- 2. contention ----------------------------------------------------------------------------------------------------------------------
@routes
def test_contention(eng, route):
    D = route[0]
    E = np.zeros((2048, D), np.float32)
    E[:, 3] = 1.0                                           # a complete graph: 2 10^6 links onto one root
    root, cluster, C = _cluster(eng, E, 0.5, route)
    assert C == 1 and not root.any() and not cluster.any()
    N = 40 * min(D, 16)
    E, lab = cs.blocks_of_identical_rows(N, D)              # runs of 40 straddle the 32-row gallery blocks
    got = _cluster(eng, E, 1.0, route)                      # (a score AT the threshold: >=)
    assert got[2] == N // 40 and _same(got, cs.canonical(lab))


# ---- 3. exact data: ties at thr and the >= ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@routes
def test_exact_integer_data(eng, route, norm):
    E, stats = cs.int_rows(300, route[0])
    stats = stats if norm else None
    V = cs.scores64(E, stats)
    ties = 0
    for q in (0.9995, 0.999, 0.99):
        t0 = cs.occurring(V, q)
        ties += int((V[np.triu_indices(300, 1)] == t0).sum())
        for thr in (t0, t0 + (0.125 if norm else 0.5)):                    # a value that occurs, and one strictly between two values
            want = cs.statement(E, thr, stats)
            assert _same(_cluster(eng, E, thr, route, stats), want), (q, thr)
    assert ties > 0
    assert 1 < cs.statement(E, cs.occurring(V, 0.999), stats)[2] < 300       # (neither one cluster nor all singletons)


# ---- 4. agreement with the project's own pairs ------------------------------------------------------------------------------------------
def _above_components(eng, E, thr, route, stats=None):
    if route[1]:
        Ed = _off4(E)
        st = None if stats is None else tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in stats)
        rp, ix, _ = eng.score_above(Ed, Ed, thr, st, st, upper=True)
        rp, ix = rp.cpu().numpy(), ix.cpu().numpy()
    else:
        rp, ix, _ = eng.score_above(E, E, thr, stats, stats, upper=True)
    return cs.components_of_csr(E.shape[0], rp, ix), int(ix.size)


@routes
def test_components_of_score_aboves_pair_set(eng, route):
    D = route[0]
    E, stats = cs.int_rows(300, D)
    for st in (None, stats):
        thr = cs.occurring(cs.scores64(E, st), 0.999)
        want, n_pairs = _above_components(eng, E, thr, route, st)
        assert n_pairs > 0 and _same(_cluster(eng, E, thr, route, st), want)
    # speaker-structured unit rows (tools/above_bench.py's generator), a few thousand: float scores, so the yardstick is the library's
    # own pair set - the same scores, bit for bit, on the same route
    E, _, _ = synth.synth_speaker_embeddings(3000, n_speakers=300, dim=D, seed=5)
    want, n_pairs = _above_components(eng, E, 0.45, route)
    got = _cluster(eng, E, 0.45, route)
    assert n_pairs > 3000 and 1 <= got[2] < 3000 and _same(got, want)


# ---- 5. edge values ---------------------------------------------------------------------------------------------------------------------
@routes
def test_edge_values(eng, route):
    D = route[0]
    E, _ = cs.int_rows(200, D)
    ident = (np.arange(200, dtype=np.int32), np.arange(200, dtype=np.int32), 200)
    assert _same(_cluster(eng, E, -np.inf, route), (np.zeros(200, np.int32), np.zeros(200, np.int32), 1))
    assert _same(_cluster(eng, E, np.inf, route), ident)
    # rows holding a NaN are singletons - even at thr = -inf - and break no other cluster
    En = E.copy()
    En[7, 3] = np.nan
    En[150, D - 1] = np.nan
    thr = cs.occurring(cs.scores64(E), 0.999)
    with np.errstate(invalid="ignore"):
        want = cs.statement(En, thr)
        assert want[0][7] == 7 and want[0][150] == 150
        assert _same(_cluster(eng, En, thr, route), want)
        rest = np.delete(np.arange(200), [7, 150])
        assert np.array_equal(cs.canonical(want[0][rest])[0], cs.statement(E[rest], thr)[0])      # the others: as without them
        got = _cluster(eng, En, -np.inf, route)
    assert got[2] == 3 and got[0][7] == 7 and got[0][150] == 150 and not got[0][rest].any()
    # an all-zero row at thr = 0 links to everything: +0 >= 0, and the zeros of a product with -0.0
    N = 40
    Z = np.zeros((N, D), np.float32)
    Z[np.arange(N - 1), 1 + np.arange(N - 1)] = 1.0
    Z[:N - 1, 0] = np.where(np.arange(N - 1) % 2 == 0, 2.0, -2.0)          # even rows score +4 among themselves, -4 against odd rows
    assert _same(_cluster(eng, Z[:N - 1], 0.0, route), cs.canonical(np.arange(N - 1) % 2))
    Z[N - 1, ::2] = -0.0
    assert _same(_cluster(eng, Z, 0.0, route), (np.zeros(N, np.int32), np.zeros(N, np.int32), 1))


# ---- 6. independence --------------------------------------------------------------------------------------------------------------------
@routes
def test_independence(eng, route):
    D = route[0]
    E, thr, lab = cs.shared_coordinate_rows(300, D)
    first = _cluster(eng, E, thr, route)
    again = _cluster(eng, E, thr, route)
    assert _same(first, cs.canonical(lab)) and _same(again, first)                        # the same bits on every run
    # a subset that is a union of whole clusters: the same partition of it
    keep = np.isin(first[1], np.arange(0, first[2], 2))
    assert 0 < keep.sum() < 300
    assert _same(_cluster(eng, E[keep], thr, route), cs.canonical(first[0][keep]))
    # unrelated rows behind: the first N roots do not move
    P, pthr, plab = cs.graph_shapes(161, D)["path_permuted"]
    far = cs.circle_rows(np.arange(40) * 3, np.full(40, 1), D)                            # another plane, and nobody linked there
    got = _cluster(eng, np.concatenate([P, far]), pthr, route)
    assert np.array_equal(got[0][:161], _cluster(eng, P, pthr, route)[0]) and np.array_equal(got[0][161:], 161 + np.arange(40)) and got[2] == 41


def test_fused_and_slab_agree_on_exact_data(eng):
    E, stats = cs.int_rows(300, 192)
    for st in (None, stats):
        thr = cs.occurring(cs.scores64(E, st), 0.999)
        assert _same(_cluster(eng, E, thr, (192, True), st), _cluster(eng, E, thr, (192, False), st))
    E, thr, _ = cs.shared_coordinate_rows(1000, 192)
    assert _same(_cluster(eng, E, thr, (192, True)), _cluster(eng, E, thr, (192, False)))


# ---- 7. plumbing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [192, 64])
def test_device_tensors_stay_on_the_device(eng, D):
    E, stats = cs.int_rows(300, D)
    thr = cs.occurring(cs.scores64(E, stats), 0.999)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Ed, st = dev(E), tuple(dev(x) for x in stats)
    torch.cuda.synchronize()
    before = dict(sv_engine.TRANSFER_STATS)
    root, cluster, C = eng.cluster_above(Ed, thr, st)
    assert dict(sv_engine.TRANSFER_STATS) == before                                        # nothing staged, nothing copied back
    assert all(torch.is_tensor(x) and x.is_cuda for x in (root, cluster, C)) and C.dtype == torch.int64 and C.dim() == 0
    assert _same((root.cpu().numpy(), cluster.cpu().numpy(), int(C)), cs.statement(E, thr, stats))
    with pytest.raises(ValueError):
        eng.cluster_above(Ed, thr, stats)                                                  # one memory space per call


def test_raw_abi_null_cluster_refusals_and_empty_input(eng):
    lib, h = eng.lib, eng.h
    E, stats = cs.int_rows(300, 192)
    thr = cs.occurring(cs.scores64(E), 0.999)
    want = cs.statement(E, thr)
    root, n = np.full(300, -7, np.int32), np.full(1, -7, np.int64)
    p = lambda a: a.ctypes.data
    # out_cluster = NULL: roots and the count alone
    assert lib.svhip_cluster_above(h, p(E), 300, 192, thr, None, None, p(root), None, p(n), 0) == 0
    assert np.array_equal(root, want[0]) and int(n[0]) == want[2]
    # the same through device pointers, asynchronously
    Ed = torch.from_numpy(E).cuda()
    rd, nd = torch.full((300,), -7, dtype=torch.int32, device="cuda"), torch.full((1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    flags = _lib.IN_DEVICE | _lib.OUT_DEVICE | _lib.ASYNC
    assert lib.svhip_cluster_above(h, Ed.data_ptr(), 300, 192, thr, None, None, rd.data_ptr(), None, nd.data_ptr(), flags) == 0
    eng.synchronize()
    assert np.array_equal(rd.cpu().numpy(), want[0]) and int(nd[0]) == want[2]
    # refusals: by name, before any copy or launch - the outputs keep their canaries
    root[:], n[:] = -7, -7
    cluster = np.full(300, -7, np.int32)
    mu, sigma = stats
    call = lambda N=300, D=192, thr=thr, E=E, mu=None, sigma=None, root=root, n=n: lib.svhip_cluster_above(
        h, None if E is None else p(E), N, D, thr, None if mu is None else p(mu), None if sigma is None else p(sigma),
        None if root is None else p(root), p(cluster), None if n is None else p(n), 0)
    for kw, code, text in ((dict(thr=float("nan")), -1, "cluster_above: the threshold is NaN"),
                           (dict(D=0), -1, "cluster_above: D = 0 must be at least 1"),
                           (dict(D=48), -5, "cluster_above: embedding dim 48 must be a multiple of 32"),
                           (dict(N=-1), -1, "cluster_above: N = -1 is negative"),
                           (dict(N=2 ** 31), -1, "cluster_above: N = 2147483648 is outside"),
                           (dict(E=None), -1, "cluster_above: NULL pointer"),
                           (dict(root=None), -1, "cluster_above: NULL pointer"),
                           (dict(n=None), -1, "cluster_above: NULL pointer"),
                           (dict(mu=mu), -1, "cluster_above: sigma is NULL"),
                           (dict(sigma=sigma), -1, "cluster_above: mu is NULL")):
        rc = call(**kw)
        assert rc == code, kw                               # SVHIP_ERR_INVALID / SVHIP_ERR_UNSUPPORTED
        with pytest.raises(_lib.SvhipError, match=text):
            eng._ck(rc)
        assert np.all(root == -7) and np.all(cluster == -7) and n[0] == -7, kw
    with pytest.raises(_lib.SvhipError, match="multiple of 32"):
        eng.cluster_above(np.zeros((3, 48), np.float32), 0.5)
    # N = 0: OK, C = 0, nothing else touched
    assert call(N=0, E=None, root=None) == 0 and n[0] == 0 and np.all(cluster == -7)
    r0, c0, C0 = eng.cluster_above(E[:0], thr)
    assert r0.shape == c0.shape == (0,) and r0.dtype == c0.dtype == np.int32 and C0 == 0
    assert int(eng.cluster_above(Ed[:0], thr)[2]) == 0


# ---- 8. one pass, no edge list ----------------------------------------------------------------------------------------------------------
def _fused_parts(N):
    """the launches of csrc/api_search.hip's fused_plan: per chunk of 16 384 rows its whole 128-row tiles (a tail above 32 rows counts
    as a tile) and, for a tail of 1 .. 32 rows, a FEW launch"""
    parts = 0
    for r0 in range(0, N, 16384):
        rows = min(16384, N - r0)
        few = rows % 128 if 1 <= rows % 128 <= 32 else 0
        parts += (rows - few > 0) + (few > 0)
    return parts


@pytest.mark.parametrize("N", [20, 300, 1044, 16384 + 148])
def test_one_link_launch_per_part_and_no_threshold_search(eng, N):
    assert [_fused_parts(n) for n in (20, 128, 300, 1044, 16384, 16384 + 148)] == [1, 1, 1, 2, 1, 3]
    E, thr, lab = cs.shared_coordinate_rows(N, 192)
    eng.profile(True)
    try:
        got = eng.cluster_above(E, thr)
        labels = eng.profile_results()
    finally:
        eng.profile(False)
    assert _same(got, cs.canonical(lab))
    assert labels["cluster_link"]["launches"] == _fused_parts(N)
    assert {"cluster_init", "cluster_flatten", "cluster_ids"} <= set(labels)
    assert not [k for k in labels if k.startswith("score_above") or k.startswith("cluster_gemm") or k.startswith("cluster_link_rows")]


# ---- 9. model level ---------------------------------------------------------------------------------------------------------------------
def test_model_cluster_on_the_speaker_fixture(tmp_path, golden_dir):
    """ModelHandling.cluster(source=...) on the eight files of tests/golden/e2e_speakers.npz.  The threshold is the midpoint of the widest
    gap in the sorted float64 scores of the fixture's OWN embeddings (the reference's, prepared by cluster's rule).  The model's
    embeddings lie within 1e-4 of those relative to their scale (tests/test_gpu_e2e.py's bar for this fixture), which moves a cosine
    of unit rows by a few 1e-4 at most; the fp32 score adds 1e-6.  Half the gap must exceed ten times that."""
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
    print(f"widest gap {v[k + 1] - v[k]:.4f} between {v[k]:.4f} and {v[k + 1]:.4f}")
    assert 0.5 * (v[k + 1] - v[k]) > 10 * (4e-4 + cs.BAR)
    want = cs.statement(rows, thr)
    assert 1 < want[2] < rows.shape[0]

    args = dict(ARGS, save_folder=tmp)
    net = WrappedModel(SpeakerEncoder(**args))
    mh = ModelHandling(net, **args)
    sd = synth.synth_state_dict(synth.ecapa_param_spec(C=512), seed=E2E2_SEED_W)
    sd["asp_bn.norm.running_mean"] = g["asp_bn_running_mean"]
    sd["asp_bn.norm.running_var"] = g["asp_bn_running_var"]
    net.module.load_state_dict({"__S__." + k_: v_ for k_, v_ in sd.items()})
    files, _, _ = make_e2e_speaker_files(tmp)
    labels, groups = mh.cluster(source=files, thresh_score=thr, num_eval=2)
    assert labels.dtype == np.int32 and labels.tolist() == want[1].tolist()
    assert groups == [[files[i] for i in np.nonzero(want[1] == c)[0]] for c in range(want[2])]
    # min_size = 2: singletons become -1, the rest is renumbered in order.  At the widest gap the fixture falls into its four speakers,
    # two files each, and nothing is dropped; the widest gap ABOVE it (held to the same margin) leaves pairs and singletons.
    hi = v[k + 1:]
    k2 = int(np.argmax(np.diff(hi)))
    thr2 = float(0.5 * (hi[k2] + hi[k2 + 1]))
    assert 0.5 * (hi[k2 + 1] - hi[k2]) > 10 * (4e-4 + cs.BAR)
    for t in (thr, thr2):
        w = cs.statement(rows, t)
        sizes = np.bincount(w[1])
        kept = np.nonzero(sizes >= 2)[0]
        labels2, groups2 = mh.cluster(source=files, thresh_score=t, num_eval=2, min_size=2)
        assert labels2.tolist() == [int(np.searchsorted(kept, c)) if sizes[c] >= 2 else -1 for c in w[1]]
        assert groups2 == [[files[i] for i in np.nonzero(w[1] == c)[0]] for c in kept]
    assert (sizes == 1).any() and (sizes >= 2).any() and -1 in labels2 and labels2.max() == len(kept) - 1
    # a gallery: cluster's groups are the components of duplicates' pairs
    model_rows = np.stack([mh.embed_utterance(f, num_eval=2, normalize=True).numpy().mean(axis=0) for f in files]).astype(np.float32)
    gallery = np.concatenate([model_rows, model_rows[[1, 4]]])
    i, j, _ = mh.duplicates(gallery, thr)
    want_g = cs.components(gallery.shape[0], i, j)
    labels3, groups3 = mh.cluster(embeds=gallery, thresh_score=thr)
    assert labels3.tolist() == want_g[1].tolist() and groups3 == [np.nonzero(want_g[1] == c)[0].tolist() for c in range(want_g[2])]
    assert labels3[8] == labels3[1] and labels3[9] == labels3[4]
