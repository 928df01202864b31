"""numpy's restatement of svhip_cluster_join (include/svhip.h, "cluster_join"), built on tests/cluster_statement.py.

Statement: A's rows are 0 .. NA - 1 of the joint numbering, B's NA .. NA + NB - 1.  The links are (1) the seed links (i, root_x[i]) of
every side that brings a seed, an entry outside [0, i] being read as i; (2) the pairs i < j with v >= thr inside every side WITHOUT a
seed; (3) every pair (a in A, b in B) with v(a, b) >= thr.  v is the float64 score of cluster_statement (a NaN links nothing); the
clusters are the connected components, in the canonical form (root, cluster, C).  Like cluster_statement's, the statement decides a
pair only outside the fp32 score's accuracy bar: tests/test_cluster_join_host.py asserts that no pair of the data lies inside it."""
import numpy as np

from tests.cluster_statement import (bar64, canonical, components, graph_shapes, int_rows, occurring, scores64,  # noqa: F401
                                     shared_coordinate_rows, star)

# the cuts of the GPU test's split cases (tests/test_gpu_cluster_join.py)
CUTS = (0, 1, 31, 32, 33, 128, 129, 161, 299, 300)
MODES = ("none", "a", "ab")              # which sides are seeded with cluster_above's roots of that side


def clamp(seed):
    """a seed array as the library reads it: an entry outside [0, i] is i"""
    seed = np.asarray(seed, np.int64)
    i = np.arange(seed.size)
    return np.where((seed >= 0) & (seed <= i), seed, i)


def join_links(A, B, thr, root_a=None, root_b=None, a_stats=None, b_stats=None):
    """-> (i, j): the links of the statement in the joint numbering"""
    A, B = np.asarray(A), np.asarray(B)
    NA, NB = A.shape[0], B.shape[0]
    E = np.concatenate([A, B])
    stats = None if a_stats is None else tuple(np.concatenate([x, y]) for x, y in zip(a_stats, b_stats))
    V = scores64(E, stats)
    with np.errstate(invalid="ignore"):
        hit = np.triu(V >= thr, 1)
    keep = np.zeros_like(hit)
    keep[:NA, NA:] = True                                   # the rectangle: always walked
    ii, jj = [], []
    for seed, lo, n in ((root_a, 0, NA), (root_b, NA, NB)):
        if seed is None:
            keep[lo:lo + n, lo:lo + n] = True               # an unseeded side: its own pairs
        else:
            ii.append(lo + np.arange(n))
            jj.append(lo + clamp(seed))
    i, j = np.nonzero(hit & keep)
    return np.concatenate([i] + ii).astype(np.int64), np.concatenate([j] + jj).astype(np.int64)


def join_statement(A, B, thr, root_a=None, root_b=None, a_stats=None, b_stats=None):
    """-> (root, cluster, C) over the NA + NB joint rows"""
    i, j = join_links(A, B, thr, root_a, root_b, a_stats, b_stats)
    return components(np.asarray(A).shape[0] + np.asarray(B).shape[0], i, j)


def seeds(E, NA, thr, mode, stats=None, statement=None):
    """the seeds of a split of E at NA in one of MODES: cluster_above's roots of the seeded sides, by `statement` (default: the float64
    statement of cluster_statement)"""
    from tests import cluster_statement as cs
    st = statement or (lambda X, s: cs.statement(X, thr, s)[0])
    cut = lambda s, lo, hi: None if s is None else tuple(x[lo:hi] for x in s)
    root_a = st(E[:NA], cut(stats, 0, NA)) if mode in ("a", "ab") else None
    root_b = st(E[NA:], cut(stats, NA, None)) if mode == "ab" else None
    return root_a, root_b


def labels_to_roots(labels):
    """any labelling -> per row the first row that carries its label"""
    return canonical(labels)[0]


def split_cases(D):
    """name -> (E, thr, labelling): the data of the GPU test's split cases"""
    cases = dict(graph_shapes(300, D))
    cases["star"] = star(D)
    return cases
