"""numpy's restatement of svhip_cluster_above (include/svhip.h, "cluster_above") and the data both the host and the GPU tests cluster.

Statement: rows i < j are linked iff v(i, j) >= thr, v the inner product (or, with statistics, t = s (a_i + a_j) - (b_i + b_j) from the
fp32 coefficients); a NaN v links nothing; a cluster is a connected component; root[i] = the smallest row of i's cluster, cluster[i] the
dense id in order of the smallest member, C the number of clusters.  Here v is taken in float64, so the statement decides a pair only
when |v - thr| exceeds the accuracy bar of the fp32 score: every builder below is made so that NO pair lies within the bar
(`undecided` counts them; tests/test_cluster_host.py asserts zero for every case, without a GPU)."""
import numpy as np

from tests.test_gpu_topk_norm import EPS, _coef, _statement

# The bar on a plain score of L2-normalised rows: svhip.h's contract for score_topk ("within 1e-6 of the float64 inner product"), the
# figure tests/test_gpu_topk.py asserts (_check_against_float64: err <= 1e-6) and tests/test_gpu_above.py uses for its float data.  That
# file holds it as a literal, so there is no name to import; EPS (the normalised score's) is tests/test_gpu_topk_norm.py's own.
BAR = 1e-6


# ---- components ---------------------------------------------------------------------------------------------------------------------------
def components(n, i, j):
    """plain union-find over the links (i[k], j[k]) of n rows -> (root int32, cluster int32, C): the canonical form"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)              # the smaller index stays root: the root of a set is its minimum
    root = np.array([find(x) for x in range(n)], np.int32).reshape(n)
    return canonical(root)


def canonical(label):
    """any labelling of the rows (equal label = same cluster) -> (root, cluster, C)"""
    label = np.asarray(label)
    n = label.size
    _, first, inv = np.unique(label, return_index=True, return_inverse=True)
    root = first[inv.reshape(-1)].astype(np.int32) if n else np.zeros(0, np.int32)      # the first (smallest) row that carries the label
    is_root = root == np.arange(n)
    rank = np.cumsum(is_root) - 1
    return root, rank[root].astype(np.int32), int(is_root.sum())


def scores64(E, stats=None):
    """v of every pair in float64 (the coefficients in fp32, as the library computes them)"""
    E64 = np.asarray(E, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        V = E64 @ E64.T
        if stats is not None:
            V = _statement(V, stats, stats)
    return V


def bar64(E, stats=None):
    """the accuracy bar of every pair's fp32 score: BAR for the plain score; for the normalised one the bar tests/test_gpu_topk_norm.py
    derives and tests/test_gpu_above.py uses (the plain bar scaled by A = a_i + a_j, plus 8 roundings of 2^-24 of a term no larger than
    |s| A + |b_i| + |b_j|)"""
    n = np.asarray(E).shape[0]
    if stats is None:
        return np.full((n, n), BAR)
    E64 = np.asarray(E, np.float64)
    a, b = (x.astype(np.float64) for x in _coef(*stats))
    A = a[:, None] + a[None, :]
    return BAR * A + 8 * EPS * (np.abs(E64 @ E64.T) * A + np.abs(b)[:, None] + np.abs(b)[None, :])


def links64(E, thr, stats=None):
    """the link matrix of the statement: the upper triangle of v >= thr (NaN compares false)"""
    V = scores64(E, stats)
    with np.errstate(invalid="ignore"):
        return np.triu(V >= thr, 1)


def undecided(E, thr, stats=None):
    """the pairs i < j whose float64 score lies within the bar of thr: the fp32 score may put them on either side"""
    V = scores64(E, stats)
    with np.errstate(invalid="ignore"):
        return int(np.triu(np.abs(V - thr) <= bar64(E, stats), 1).sum())


def statement(E, thr, stats=None):
    """-> (root, cluster, C) by the float64 statement"""
    i, j = np.nonzero(links64(E, thr, stats))
    return components(np.asarray(E).shape[0], i, j)


def components_of_csr(n, row_ptr, index):
    """the components of a score_above(upper=True) result"""
    row_ptr, index = np.asarray(row_ptr), np.asarray(index)
    return components(n, np.repeat(np.arange(n), np.diff(row_ptr)), index)


# ---- graph shapes: unit rows on circles ---------------------------------------------------------------------------------------------------
DELTA = 0.02


def circle_rows(slot, plane, D, delta=DELTA):
    """row i = (cos, sin)(slot[i] * delta) in the coordinates (2 plane[i], 2 plane[i] + 1), zero elsewhere: rows of one plane score
    cos((slot_i - slot_j) delta), rows of different planes 0.  With thr = cos(1.5 delta) two rows are linked iff they share a plane and
    their slots differ by at most 1; the nearest scores to thr are cos(delta) and cos(2 delta), about 0.6 delta^2 and 0.9 delta^2 away
    (delta = 0.02: 2.5e-4 and 3.5e-4 against a bar of 1e-6)."""
    slot, plane = np.asarray(slot, np.int64), np.asarray(plane, np.int64)
    assert 2 * (int(plane.max(initial=0)) + 1) <= D and (int(slot.max(initial=0)) + 2) * delta < 2 * np.pi      # no wrap round the circle
    E = np.zeros((slot.size, D), np.float32)
    ang = slot.astype(np.float64) * delta
    E[np.arange(slot.size), 2 * plane] = np.cos(ang)
    E[np.arange(slot.size), 2 * plane + 1] = np.sin(ang)
    return E


def circle_thr(delta=DELTA):
    return float(np.cos(1.5 * delta))


def graph_shapes(N, D, seed=0):
    """name -> (E, thr, the labelling the shape has by construction).  N <= 300: a path of N slots stays inside one turn."""
    rng = np.random.default_rng(1000 * N + D + seed)
    zero = np.zeros(N, np.int64)
    idx = np.arange(N)
    perm = rng.permutation(N)
    shapes = {
        "path": (circle_rows(idx, zero, D), zero),                                          # hooks in index order
        "path_reversed": (circle_rows(idx[::-1].copy(), zero, D), zero),                    # long climbs
        "path_permuted": (circle_rows(perm, zero, D), zero),                                # hooks that arrive in every order
        "two_paths": (circle_rows(idx // 2, idx % 2, D), idx % 2),                          # even rows and odd rows
    }
    pair = perm // 2                                                                        # a perfect matching (N odd: one row alone)
    shapes["matching"] = (circle_rows(3 * (pair // 2) + perm % 2, pair % 2, D), pair)
    return {k: (E, circle_thr(), lab) for k, (E, lab) in shapes.items()}


def star(D, leaves=None):
    """a star whose centre is the LAST row: leaf k = e_k, the centre = sum_k e_k / sqrt(L); leaf . leaf = 0, leaf . centre = 1 / sqrt(L),
    thr half of that (the nearest score is 0.5 / sqrt(L) >= 0.02 away)"""
    L = int(leaves or min(D - 1, 40))
    E = np.zeros((L + 1, D), np.float32)
    E[np.arange(L), np.arange(L)] = 1.0
    E[L, :L] = np.float32(1.0 / np.sqrt(L))
    return E, float(0.5 / np.sqrt(L)), np.zeros(L + 1, np.int64)


# ---- exact data ---------------------------------------------------------------------------------------------------------------------------
def shared_coordinate_rows(N, D, seed=0):
    """row i = e_p + e_q (p != q) with p, q inside one group of four coordinates: every score is 0, 1 or 2, exactly, on every route, and
    with thr = 1 two rows are linked iff they share a coordinate.  The rows of a group form ONE cluster as soon as its coordinate pairs
    connect the four coordinates, which the labelling checks by a union-find over the coordinates themselves.  -> (E, thr, labelling)"""
    rng = np.random.default_rng(77 + N + D + seed)
    group = rng.integers(0, D // 4, N)
    p = rng.integers(0, 4, N)
    q = (p + rng.integers(1, 4, N)) % 4
    E = np.zeros((N, D), np.float32)
    E[np.arange(N), 4 * group + p] = 1.0
    E[np.arange(N), 4 * group + q] = 1.0
    _, coord_cluster, _ = components(D, 4 * group + p, 4 * group + q)
    return E, 1.0, coord_cluster[4 * group + p]


def blocks_of_identical_rows(N, D, size=40):
    """runs of `size` identical unit rows (N a multiple of size; 40 straddles the 32-row gallery blocks): run k is the basis row
    e_(k mod D), so a score is exactly 1 (same coordinate) or 0 and any thr in (0, 1] links exactly the rows of one coordinate; with
    N / size <= D every run is a cluster of its own.  -> (E, labelling)"""
    assert N % size == 0
    run = np.arange(N) // size
    E = np.zeros((N, D), np.float32)
    E[np.arange(N), run % D] = 1.0
    return E, run % D


def int_rows(N, D, seed=0):
    """rows uniform in {-2..2} (tests/test_gpu_above.py's _int_data): every inner product is an exact fp32 integer; statistics with
    power-of-two sigmas and integer means (every step of t exact)"""
    rng = np.random.default_rng(11 + D + 7 * N + seed)
    E = rng.integers(-2, 3, (N, D)).astype(np.float32)
    sig = np.array([0.25, 0.5, 1.0, 2.0], np.float32)
    stats = (rng.integers(-8, 9, N).astype(np.float32), sig[rng.integers(0, 4, N)])
    return E, stats


def occurring(V, quantile):
    """a value that occurs among the pairs i < j of V, with about 1 - quantile of them at or above it"""
    v = np.sort(V[np.triu_indices(V.shape[0], 1)])
    return float(v[int(quantile * (v.size - 1))])
