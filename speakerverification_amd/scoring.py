"""Scoring counterparts of the reference's ``src/utils.py:126-169``.

``similarity_measure(method, ref, com, **kw)`` keeps the per-trial signature for compatibility; the
batched entry points (``score_pairs``, ``score_matrix``, ``score_topk``, ``score_topk_norm``, ``score_above``, ``cluster``, ``cluster_join``, ``group_audit``, ``asnorm_stats``,
``asnorm_pairs``, ``score_trials``) are what ``ModelHandling.evaluateFromList`` uses: one kernel launch per trial LIST
instead of three host<->device crossings per trial.
"""
from __future__ import annotations

import numpy as np

from .engine import Engine, _is_torch

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

_engines = {}


def scoring_engine(device=0) -> Engine:
    """one fbank/scoring-only handle per device, created on first use"""
    if device not in _engines:
        _engines[device] = Engine(model="none", max_batch=1, device=device)
    return _engines[device]


_comms = {}


def lib_comm(device, rank, world):
    """the RCCL communicator of a device's scoring engine (svhip_comm_*): created once per process and device — svhip_comm_init
    refuses a second communicator on a handle — and reused by every ModelHandling; destroyed with the engine."""
    from . import distributed as sv_dist
    key = (device, rank, world)
    if key not in _comms:
        _comms[key] = sv_dist.LibComm(scoring_engine(device), rank, world)
    return _comms[key]


def _np(x):
    return x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x)


def _feature_block(feats):
    """crop embeddings as the engine takes them: contiguous float32 where they live, (n_files, n_crops, D) - 2-D is one crop per file"""
    on_dev = _is_torch(feats) and feats.is_cuda
    feats = feats.contiguous() if on_dev else np.ascontiguousarray(_np(feats), dtype=np.float32)
    return feats[:, None, :] if feats.ndim == 2 else feats


def _cohort_stats(eng, cohort, top, G, g_stats=None, Q=None):
    """AS-norm statistics against ``cohort`` -> ``(q_stats, g_stats)``: the gallery's first, unless given; then the queries' (None without Q)"""
    if g_stats is None:
        g_stats = eng.asnorm_stats(G, cohort, top)
    return (None if Q is None else eng.asnorm_stats(Q, cohort, top)), g_stats


# ---- batched API ---------------------------------------------------------------------------------------
def score_pairs(E, ia, ib, device=0):
    """|cos(E[ia], E[ib])| (utils.py:163-164 with one crop per row)."""
    return scoring_engine(device).score_pairs(E, ia, ib)


def score_matrix(A, B, device=0):
    return scoring_engine(device).score_matrix(A, B)


def score_topk(Q, G, k, device=0):
    """per row of Q the k best rows of the gallery G by inner product -> (scores (N, k), int32 index (N, k)), best first"""
    return scoring_engine(device).score_topk(Q, G, k)


def score_topk_norm(Q, G, k, cohort, top=200, g_stats=None, device=0):
    """``score_topk`` over adaptive-S-normalised scores (open-set identification: the best score can be held against one threshold).
    The cohort statistics of Q, and of G unless ``g_stats = (mu, sigma)`` is given, come from ``asnorm_stats(., cohort, top)``;
    the k best gallery rows per query are selected on the normalised score.  All arrays in one memory space.
    -> (scores (N, k), int32 index (N, k), g_stats): keep ``g_stats`` with the gallery to skip its statistics next time."""
    eng = scoring_engine(device)
    q_stats, g_stats = _cohort_stats(eng, cohort, top, G, g_stats, Q)
    scores, index = eng.score_topk_norm(Q, q_stats, G, g_stats, k)
    return scores, index, tuple(g_stats)


def score_above(Q, G, thr, cohort=None, top=200, g_stats=None, upper=False, q_base=0, max_hits=2 ** 28, device=0):
    """every (row of Q, row of G) pair whose score is at least ``thr`` -> CSR ``(row_ptr (N + 1,) int64, index int32, score float32)``,
    a row's hits in ascending gallery index (``Engine.score_above``).  With a ``cohort`` the score is the adaptive-S-normalised one of
    ``score_topk_norm``: the statistics of Q, and of G unless ``g_stats = (mu, sigma)`` is given, come from
    ``asnorm_stats(., cohort, top)``.  ``upper`` / ``q_base``: the self-join of one set, every unordered pair once."""
    if float(thr) != float(thr):
        raise ValueError("score_above: the threshold is NaN")
    eng = scoring_engine(device)
    if cohort is None:
        if g_stats is not None:
            raise ValueError("score_above: g_stats without a cohort (the queries' statistics need it)")
        return eng.score_above(Q, G, thr, upper=upper, q_base=q_base, max_hits=max_hits)
    q_stats, g_stats = _cohort_stats(eng, cohort, top, G, g_stats, Q)
    return eng.score_above(Q, G, thr, q_stats, g_stats, upper=upper, q_base=q_base, max_hits=max_hits)


LINKAGES = ("single", "average", "complete")


def cluster(E, thr, cohort=None, top=200, stats=None, device=0, linkage="single"):
    """which rows of E are the same speaker?  Rows ``i < j`` are linked iff their score is at least ``thr``; a cluster is a connected
    component -> ``(root (N,) int32, cluster (N,) int32, n_clusters)`` (``Engine.cluster_above``).  With a ``cohort`` the score is the
    adaptive-S-normalised one of ``score_topk_norm``: the rows' statistics come from ``asnorm_stats(E, cohort, top)``; ``stats =
    (mu, sigma)``, kept from an earlier call, is used as it is.  The clusters are the components of the pair set ``score_above(E, E, thr, ..., upper=True)``
    returns, found in one pass over the upper half plane and without that pair list.

    ``linkage``: ``"single"`` is the above.  ``"average"`` / ``"complete"`` agglomerate inside each of those components until no two
    clusters' mean / smallest score reaches ``thr`` (``Engine.cluster_linkage``) and return a fourth value, ``n_unrefined``: the
    components too large to refine, which stay one cluster each."""
    if float(thr) != float(thr):
        raise ValueError("cluster: the threshold is NaN")
    if linkage not in LINKAGES:
        raise ValueError(f"cluster: linkage = {linkage!r} is not one of {LINKAGES}")
    eng = scoring_engine(device)
    if cohort is not None:
        stats = _cohort_stats(eng, cohort, top, E, stats)[1]
    if linkage == "single":
        return eng.cluster_above(E, thr, stats)
    return eng.cluster_linkage(E, thr, stats, linkage)


def _first_rows_torch(lab):
    """``labels_to_roots`` for a 1-D integer tensor, where it lives (plumbing: unique, then the smallest row of each label)"""
    _, inv = torch.unique(lab, return_inverse=True)
    first = torch.full((int(inv.max()) + 1 if inv.numel() else 0,), lab.numel(), dtype=torch.int64, device=lab.device)
    first.scatter_reduce_(0, inv, torch.arange(lab.numel(), device=lab.device), "amin")
    return first[inv].to(torch.int32)


def labels_to_roots(labels, n=None, what="labels"):
    """any integer labelling (an equal label means the same cluster) -> the root form ``cluster_join`` takes as a seed: per row the
    FIRST row that carries its label (int32, ``root[i] <= i``); on the host, or on the device for a CUDA tensor.  ``n``: the length
    the labelling must have."""
    on_dev = _is_torch(labels) and labels.is_cuda
    lab = _np(labels).reshape(-1) if not on_dev else labels.reshape(-1)
    if n is not None and int(lab.shape[0]) != int(n):
        raise ValueError(f"cluster_join: {what} must hold {int(n)} values, not {int(lab.shape[0])}")
    if on_dev:
        if lab.dtype.is_floating_point or lab.dtype == torch.bool:
            raise ValueError(f"cluster_join: {what} must be integers, not {lab.dtype}")
        return _first_rows_torch(lab)
    if lab.dtype.kind not in "iu":
        raise ValueError(f"cluster_join: {what} must be integers, not {lab.dtype}")
    _, first, inv = np.unique(lab, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)].astype(np.int32) if lab.size else np.zeros(0, np.int32)


def cluster_join(A, B, thr, labels_a=None, labels_b=None, cohort=None, top=200, a_stats=None, b_stats=None, device=0):
    """which clusters do the new rows B belong to?  Joins B (NB, D) to a set A (NA, D) without scoring A against itself again ->
    ``(root (NA + NB,) int32, cluster (NA + NB,) int32, n_clusters)`` over the joint rows, A's first (``Engine.cluster_join``).
    ``labels_a`` / ``labels_b``: a known grouping of that side as ANY integer labelling - an equal label means the same cluster -
    which is trusted, not rescored; ``None``: the side's own pairs are scored as ``cluster`` scores them.  Every pair (row of A, row
    of B) whose score is at least ``thr`` is linked, so a new row may join an old cluster, start its own, or bridge two old ones.
    With ``labels_a = cluster(A, thr)[1]`` the result is exactly ``cluster`` of the concatenation (single linkage).  With a
    ``cohort`` the score is the adaptive-S-normalised one: the statistics of each side come from ``asnorm_stats(., cohort, top)``
    unless ``a_stats`` / ``b_stats = (mu, sigma)``, kept from an earlier call, are given.  All arrays in one memory space."""
    if float(thr) != float(thr):
        raise ValueError("cluster_join: the threshold is NaN")
    if cohort is None and (a_stats is None) != (b_stats is None):
        raise ValueError("cluster_join: a_stats and b_stats go together without a cohort: give both or neither")
    root_a = None if labels_a is None else labels_to_roots(labels_a, A.shape[0], "labels_a")
    root_b = None if labels_b is None else labels_to_roots(labels_b, B.shape[0], "labels_b")
    eng = scoring_engine(device)
    if cohort is not None:
        if a_stats is None:
            a_stats = eng.asnorm_stats(A, cohort, top)
        if b_stats is None:
            b_stats = eng.asnorm_stats(B, cohort, top)
    return eng.cluster_join(A, B, thr, root_a, root_b, a_stats, b_stats)


def audit_cut(threshold):
    """The largest float32 score the reference's audit rule (src/benchmark/benchmark_dataset.py:24-29) calls a MISMATCH: with
    ``ratio = threshold / 0.5`` a pair matches iff ``min(score / ratio, 1) > 0.5``, the float32 score divided in float64 (what numpy
    1.x made of a float32 scalar over a Python float).  ``group_audit`` counts ``score <= audit_cut(threshold)``."""
    threshold = float(threshold)
    if not (threshold > 0.0 and np.isfinite(threshold)):
        raise ValueError(f"audit_cut: the threshold must be a positive finite number, not {threshold}")
    ratio = threshold / 0.5

    def mismatch(s):
        return not (min(float(s) / ratio, 1.0) > 0.5)

    s = np.float32(threshold)
    inf = np.float32(np.inf)
    while not mismatch(s):
        s = np.nextafter(s, -inf)
    while mismatch(np.nextafter(s, inf)):
        s = np.nextafter(s, inf)
    return np.float32(s)


def group_audit(feats, group_ptr, threshold, scores=False, device=0):
    """The reference's label-noise audit (benchmark_dataset.py:32-84) over many folders at once.  ``feats``: (n_files, n_crops, D)
    float32 crop embeddings (numpy, or a CUDA tensor that stays where it is), the files sorted by folder; ``group_ptr``: the folders'
    boundaries (n_folders + 1).  Returns per file the number of files of its own folder it does not match under the reference's rule at
    ``threshold`` (``audit_cut``); with ``scores=True`` also the per-folder score blocks (``Engine.group_audit``)."""
    feats = _feature_block(feats)
    Engine._audit_group_ptr(group_ptr, int(feats.shape[0]))           # (refused here: before an engine is even created)
    return scoring_engine(device).group_audit(feats, group_ptr, audit_cut(threshold), scores=scores)


def asnorm_stats(E, cohort, top=200, device=0):
    return scoring_engine(device).asnorm_stats(E, cohort, top)


def asnorm_pairs(E, mu, sigma, ia, ib, device=0):
    return scoring_engine(device).asnorm_pairs(E, mu, sigma, ia, ib)


def score_trials(feats, ia, ib, mode="cosine", cohorts=None, top=200, device=0):
    """Score a whole trial list.  ``feats``: (n_files, n_crops, D) float32 (already L2-normalised when
    the loss sets test_normalize) — a numpy array, or a CUDA tensor, in which case everything stays on the device and a CUDA
    tensor of P scores comes back; ``ia``/``ib``: file indices per trial.
      cosine: mean_i |cos(R_i, C_i)| over aligned crops                          (utils.py:163-164)
      norm  : adaptive S-norm on crop means with the top-`top` cohort scores     (utils.py:135-160)
      pnorm : mean_i ||R_i - C_i + 1e-6||_2                                      (utils.py:167-169)
      pdist : -mean pairwise distance over the (n, D, n) broadcast               (model.py:425-431, cohorts_path=None)
    Every mode is a device kernel (svhip_score_trials / svhip_mean_crops + svhip_asnorm_*)."""
    from . import engine as _engine
    feats = _feature_block(feats)
    on_dev = _is_torch(feats)                 # (a CUDA tensor: anything else came back as a numpy array)
    ia = np.ascontiguousarray(ia, dtype=np.int32)
    ib = np.ascontiguousarray(ib, dtype=np.int32)
    eng = scoring_engine(device)
    if len(ia) == 0:
        if on_dev:
            import torch
            return torch.zeros((0,), dtype=torch.float32, device=feats.device)
        return np.zeros((0,), np.float32)
    # the C ABI range-checks host indices only; on the device-resident path they are uploaded first, so the check happens here (O(P))
    n_files = int(feats.shape[0])
    if int(ia.min()) < 0 or int(ib.min()) < 0 or int(ia.max()) >= n_files or int(ib.max()) >= n_files:
        raise ValueError(f"trial indexes outside [0, {n_files})")
    if on_dev:                                # indices follow the embeddings into HBM (8 P bytes over PCIe)
        ia, ib = _engine.to_device(ia, feats.device.index), _engine.to_device(ib, feats.device.index)
    if mode in ("cosine", "pnorm", "pdist"):
        return eng.score_trials(feats, ia, ib, mode)
    if mode in ("norm", "zt_norm"):
        if cohorts is None:
            raise ValueError("scoring_mode 'norm' needs a cohort matrix")
        Em = eng.mean_crops(feats)                                              # crop means
        if on_dev:
            cohorts = cohorts if (_is_torch(cohorts) and cohorts.is_cuda) else _engine.to_device(np.ascontiguousarray(_np(cohorts), np.float32), feats.device.index)
        else:
            cohorts = np.ascontiguousarray(_np(cohorts), dtype=np.float32)
        mu, sd = eng.asnorm_stats(Em, cohorts, top)
        return eng.asnorm_pairs(Em, mu, sd, ia, ib)
    raise ValueError(f"unknown scoring mode {mode}")


# ---- per-trial compatibility API (same names / arguments as the reference) ---------------------------------
def cosine_similarity(ref, com, **kwargs):
    r, c = np.ascontiguousarray(_np(ref), np.float32), np.ascontiguousarray(_np(com), np.float32)
    if r.ndim == 1:
        r, c = r[None], c[None]
    n = r.shape[0]
    E = np.concatenate([r, c])
    s = scoring_engine(kwargs.get("device", 0)).score_pairs(E, np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32))
    return np.mean(s)


def ZT_norm_similarity(ref, com, cohorts, top=-1, **kwargs):
    r, c = _np(ref).astype(np.float32), _np(com).astype(np.float32)
    if r.ndim == 1:
        r, c = r[None], c[None]
    E = np.ascontiguousarray(np.stack([r.mean(axis=0), c.mean(axis=0)]), dtype=np.float32)
    eng = scoring_engine(kwargs.get("device", 0))
    mu, sd = eng.asnorm_stats(E, np.ascontiguousarray(_np(cohorts), np.float32), top)
    return float(eng.asnorm_pairs(E, mu, sd, np.array([0], np.int32), np.array([1], np.int32))[0])


def pnorm_similarity(ref, com, p=2, **kwargs):
    r, c = np.ascontiguousarray(_np(ref), np.float32), np.ascontiguousarray(_np(com), np.float32)
    if r.ndim == 1:
        r, c = r[None], c[None]
    F = np.ascontiguousarray(np.stack([r, c]), dtype=np.float32)                 # (2 files, n crops, D)
    eng = scoring_engine(kwargs.get("device", 0))
    # (the reference only ever calls it with p = 2, model.py:446; any p of F.pairwise_distance is served: svhip_score_trials_pnorm)
    return float(eng.score_trials(F, np.array([0], np.int32), np.array([1], np.int32), "pnorm", p=p)[0])


def similarity_measure(method="cosine", ref=None, com=None, **kwargs):
    """src/utils.py:126-132"""
    if method == "cosine":
        return cosine_similarity(ref, com, **kwargs)
    elif method == "pnorm":
        return pnorm_similarity(ref, com, **kwargs)
    elif method == "zt_norm":
        return ZT_norm_similarity(ref, com, **kwargs)
