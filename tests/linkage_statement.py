"""numpy's restatement of svhip_cluster_linkage (include/svhip.h, "cluster_linkage") and the data the host and the GPU tests cluster.

Statement: the COMPONENTS are cluster_above's (tests/cluster_statement.py).  Inside a component every row starts as its own cluster;
L(A, B) is the sum (average) or the minimum (complete) of v over the pairs between A and B, g = L / (|A| |B|) or L; the pair of current
clusters with the largest g - ties to the smallest (min A, min B) - is merged while g >= thr; a NaN v counts as -inf, a NaN g is never
taken.  A component of more than MAX_ROWS rows is not refined.  root / cluster / C are cluster_above's canonical form.

Here everything is float64, so a decision stands only when its margin exceeds what fp32 may move it by.  A DECISION is "best g against
thr" or "best g against the best candidate of another value"; `undecided` counts the decisions whose margin is within the bars of the
candidates involved.  The bar of a candidate (A, B): the bar of one score (cluster_statement.BAR, or the largest normalised bar of the
component's pairs with statistics), plus - average only - (|A| + |B|) 2^-24 max|v|: a leaf passes through at most |A| + |B| - 2 fp32
additions and one division.  Complete linkage adds nothing: a minimum is one of the scores.  Every builder below is made so that
`undecided` is 0 (tests/test_linkage_host.py asserts it without a GPU)."""
import numpy as np

from tests import cluster_statement as cs

MAX_ROWS = 1024
LINKAGES = ("average", "complete")


def agglomerate(V, thr, linkage, vbar=0.0, exact=False):
    """one component: V (m, m) float64 scores -> (label per slot = the smallest slot of its cluster, undecided, smallest margin / bar).
    `exact`: every v and every L is an exactly representable fp32 number (the builder says why), so fp32 and float64 hold the same
    L and the only rounding left is average linkage's one division: the bar of a candidate is 2^-24 |g| (average) or 0 (complete),
    and a margin of exactly 0 - g equal to thr, which both precisions see alike - is decided."""
    m = V.shape[0]
    L = np.where(np.isnan(V), -np.inf, V).astype(np.float64)
    finite = L[np.isfinite(L)]
    vmax = float(np.abs(finite).max()) if finite.size else 0.0
    n = np.ones(m)
    alive = np.ones(m, bool)
    label = np.arange(m)
    upper = np.triu(np.ones((m, m), bool), 1)
    undecided, closest = 0, np.inf
    while True:
        with np.errstate(invalid="ignore", divide="ignore"):
            G = L / np.outer(n, n) if linkage == "average" else L.copy()
        def bar(ii, jj):                                                     # of the candidates (ii[k], jj[k])
            if linkage != "average":
                return np.full(np.shape(ii), 0.0 if exact else vbar)
            return np.abs(G[ii, jj]) * 2.0 ** -24 if exact else vbar + (n[ii] + n[jj]) * 2.0 ** -24 * vmax

        valid = upper & alive[:, None] & alive[None, :] & ~np.isnan(G)
        if not valid.any():
            break
        best = G[valid].max()
        i, j = np.unravel_index(np.flatnonzero(valid & (G == best))[0], (m, m))          # row-major: the smallest (min A, min B)
        margins = [(abs(best - thr), float(bar(i, j)))] if np.isfinite(best) and np.isfinite(thr) else []
        other = valid & (G < best)
        if other.any() and np.isfinite(best):
            second = G[other].max()
            if np.isfinite(second):
                margins.append((best - second, float(bar(i, j)) + float(bar(*np.nonzero(other & (G == second))).max())))
        for margin, b in margins:
            if exact and margin == 0:
                continue
            undecided += int(margin <= b)
            closest = min(closest, margin / b if b > 0 else np.inf)
        if not best >= thr:
            break
        with np.errstate(invalid="ignore"):
            L[i, :] = L[i, :] + L[j, :] if linkage == "average" else np.minimum(L[i, :], L[j, :])
        L[:, i] = L[i, :]
        n[i] += n[j]
        alive[j] = False
        label[label == j] = i
    return label, undecided, closest


def statement(E, thr, stats=None, linkage="average", max_rows=MAX_ROWS, exact=False):
    """-> (root, cluster, C, undecided, n_unrefined, closest): the canonical labelling by the float64 statement, the decisions within
    their bar (the pairs within the bar of thr, which decide the components, included unless the data is `exact`) and the smallest
    margin / bar seen"""
    assert linkage in LINKAGES
    E = np.asarray(E)
    N = E.shape[0]
    comp_root, _, _ = cs.statement(E, thr, stats)
    undecided, closest, unrefined = (0 if exact else cs.undecided(E, thr, stats)), np.inf, 0
    label = comp_root.astype(np.int64).copy()
    E64 = E.astype(np.float64)
    for r in np.flatnonzero(np.bincount(comp_root, minlength=N) >= 2):
        rows = np.flatnonzero(comp_root == r)
        if rows.size > max_rows:
            unrefined += 1
            continue
        sub_stats = None if stats is None else tuple(np.asarray(x)[rows] for x in stats)
        V = cs.scores64(E64[rows], sub_stats)
        B = cs.bar64(E64[rows], sub_stats)
        lab, u, c = agglomerate(V, thr, linkage, float(B[np.triu_indices(rows.size, 1)].max()), exact)
        label[rows] = rows[lab]
        undecided += u
        closest = min(closest, c)
    return cs.canonical(label) + (undecided, unrefined, closest)


def refines(fine, coarse):
    """every cluster of `fine` lies inside one cluster of `coarse` (both: a root per row)"""
    fine, coarse = np.asarray(fine), np.asarray(coarse)
    return bool(np.all(coarse[fine] == coarse))


# ---- float data ---------------------------------------------------------------------------------------------------------------------------
def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def speaker_rows(D, seed, speakers=40):
    """40 speakers of 2 - 12 unit rows, shuffled: a speaker's rows are its centroid plus noise of squared length about 0.55, so rows of
    one speaker score about 0.65 and some of them less than thr = 0.5; components stay at a dozen rows.  -> (E, thr)"""
    rng = np.random.default_rng(7000 + 13 * D + seed)
    sizes = rng.integers(2, 13, speakers)
    cent = _unit(rng.standard_normal((speakers, D)))
    who = np.repeat(np.arange(speakers), sizes)
    rows = _unit(cent[who] + rng.standard_normal((who.size, D)) * np.sqrt(0.55 / D))
    return rows[rng.permutation(who.size)].astype(np.float32), 0.5


NORM_THR = 4.5          # the normalised score of s = 0.5 at the middle of speaker_stats' ranges


def speaker_stats(N, seed):
    """cohort statistics as asnorm_stats gives them for unit rows: mu in [0, 0.1), sigma in [0.08, 0.12).  -> (mu, sigma) float32"""
    rng = np.random.default_rng(900 + seed)
    return rng.uniform(0.0, 0.1, N).astype(np.float32), rng.uniform(0.08, 0.12, N).astype(np.float32)


def bridge_rows(D, seed, per=20, bridge=9):
    """two speakers of `per` rows and `bridge` rows interpolated between their centroids, the bridge LAST: thr = 0.6 links every bridge
    row to its neighbours, so single linkage returns one cluster; average and complete linkage keep the two speakers apart.
    -> (E, thr, speaker per row with -1 for the bridge)"""
    rng = np.random.default_rng(100 + seed)
    c = _unit(rng.standard_normal((2, D)))
    c[1] = _unit(c[1] - (c[1] @ c[0]) * c[0])                              # orthogonal centroids
    who = np.repeat([0, 1], per)
    rows = _unit(c[who] + rng.standard_normal((2 * per, D)) * np.sqrt(0.25 / D))
    t = (np.arange(bridge) + 1.0) / (bridge + 1.0)
    mid = _unit((1 - t)[:, None] * c[0] + t[:, None] * c[1] + rng.standard_normal((bridge, D)) * np.sqrt(0.02 / D))
    return np.concatenate([rows, mid]).astype(np.float32), 0.6, np.concatenate([who, np.full(bridge, -1)])


# ---- exact data ---------------------------------------------------------------------------------------------------------------------------
def identical_runs(sizes, D):
    """run k = `sizes[k]` copies of the basis row e_k: every score is 1 or 0, every g exactly 1 or 0.  -> (E, thr = 1, labelling)"""
    sizes = np.asarray(sizes)
    assert sizes.size <= D
    run = np.repeat(np.arange(sizes.size), sizes)
    E = np.zeros((run.size, D), np.float32)
    E[np.arange(run.size), run] = 1.0
    return E, 1.0, run


def two_level(run_sizes, runs_per_super, D, bridge=False, seed=0):
    """row = e_run + e_(D - 1 - super): 2 inside a run, 1 inside a super-group, 0 otherwise, and every L between whole runs is a sum of
    equal integers, so g is exact at any size.  thr = 1: a component is a super-group; both linkages merge the runs (g = 2), then the
    runs of a super-group (g = 1 = thr).  `bridge`: one more row, e_(run 0) + e_(last run), which scores 1 against the rows of two runs
    of DIFFERENT super-groups and joins their components into one; the rows are shuffled.  -> (E, thr)"""
    run_sizes = np.asarray(run_sizes)
    n_super = -(-run_sizes.size // runs_per_super)
    assert run_sizes.size + n_super <= D
    run = np.repeat(np.arange(run_sizes.size), run_sizes)
    E = np.zeros((run.size + bool(bridge), D), np.float32)
    E[np.arange(run.size), run] = 1.0
    E[np.arange(run.size), D - 1 - run // runs_per_super] = 1.0
    if bridge:
        E[-1, 0] = E[-1, run_sizes.size - 1] = 1.0
    return E[np.random.default_rng(31 + seed + run.size).permutation(E.shape[0])], 1.0


def int_case(N, D, norm, quantile=0.97, seed=0):
    """cluster_statement.int_rows, with its power-of-two statistics if `norm`, at a threshold that occurs among its scores: every v is
    an exact fp32 value and ties abound.  For COMPLETE linkage, whose minimum of exact values is exact at any size and whose ties the
    rule alone decides.  -> (E, thr, stats or None)"""
    E, stats = cs.int_rows(N, D, seed)
    stats = stats if norm else None
    return E, cs.occurring(cs.scores64(E, stats), quantile), stats


# ---- the cases both test files walk ---------------------------------------------------------------------------------------------------------
SPEAKER_SEED = {192: 0, 256: 1, 64: 0}          # chosen by the margin check of tests/test_linkage_host.py (closest margin >= 4 bars)
BRIDGE_SEED = 0
SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65)


def _double_stats(N):
    """mu = 0, sigma = 0.5: a = 1, b = 0, so t = 2 s exactly"""
    return np.zeros(N, np.float32), np.full(N, 0.5, np.float32)


def cases(D, lds_rows, norm):
    """name -> (E, thr, stats, linkages, exact): every case whose labels are compared exactly.  Component sizes 1 .. 65, the LDS cap and one
    more, a run of 300; `norm`: the same data under statistics (t = 2 s on the exact sets, so thr doubles)."""
    out = {}
    both = LINKAGES
    scale = 2.0 if norm else 1.0
    E, thr, _ = identical_runs(SIZES + (lds_rows, lds_rows + 1, 300), D)
    out["identical_runs"] = (E, scale * thr, _double_stats(E.shape[0]) if norm else None, both, True)
    sizes = [x for m in SIZES[2:] + (lds_rows, lds_rows + 1) for x in (1, (m - 1) // 2, m - 1 - (m - 1) // 2)]
    E, thr = two_level(sizes, 3, D)
    out["two_level"] = (E, scale * thr, _double_stats(E.shape[0]) if norm else None, both, True)
    E, thr = two_level([5, 7, 4, 6, 3, 8], 3, D, bridge=True)
    out["two_level_bridge"] = (E, scale * thr, _double_stats(E.shape[0]) if norm else None, both, True)
    E, thr = two_level([40, 30, 50, 45, 35, 25], 3, D, bridge=True)
    out["two_level_bridge_226"] = (E, scale * thr, _double_stats(E.shape[0]) if norm else None, both, True)
    E, thr, stats = int_case(300, D, norm)
    out["int_rows"] = (E, thr, stats, ("complete",), True)
    E, thr = speaker_rows(D, SPEAKER_SEED[D])
    out["speakers"] = (E, NORM_THR if norm else thr, speaker_stats(E.shape[0], SPEAKER_SEED[D]) if norm else None, both, False)
    if not norm:
        E, thr, _ = bridge_rows(D, BRIDGE_SEED)
        out["bridge_49"] = (E, thr, None, both, False)
    return out
