"""numpy's restatement of svhip_group_audit (include/svhip.h, "group_audit"): the per-group score blocks and the mismatch counts, in
float32 (the statement itself) and in float64 (the yardstick of the float-data test), and the exact test data both GPU and host
tests use."""
import numpy as np

CLAMP = np.float32(1e-5)


def group_scores(F, group_ptr, dtype=np.float32):
    """the dense score blocks, one (n_g, n_g) array per group: mean over the crops of | cos(F[i, c], F[j, c]) |, norms clamped at
    float32(1e-5), the crops added in index order, ONE final division by n_crops"""
    F = np.asarray(F)
    C = F.shape[1]
    blocks = []
    for g in range(len(group_ptr) - 1):
        X = F[int(group_ptr[g]):int(group_ptr[g + 1])].astype(dtype)
        n = X.shape[0]
        acc = np.zeros((n, n), dtype)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            nrm = np.maximum(np.sqrt(np.einsum("icd,icd->ic", X, X)), dtype(CLAMP))
            for c in range(C):
                dot = X[:, c] @ X[:, c].T
                acc += np.abs(dot / (nrm[:, c, None] * nrm[None, :, c]))
            blocks.append(acc / dtype(C))
    return blocks


def miss_counts(blocks, cut):
    """per file: the partners j != i of its group with s(i, j) <= cut (a NaN score compares false: never a mismatch)"""
    out = []
    for S in blocks:
        with np.errstate(invalid="ignore"):
            m = S <= cut
        np.fill_diagonal(m, False)
        out.append(m.sum(axis=1))
    return np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)


def flat_scores(blocks):
    return np.concatenate([b.ravel() for b in blocks]) if blocks else np.zeros(0, np.float32)


def numpy_group_audit(feats, group_ptr, threshold, scores=False, device=0):
    """scoring.group_audit by the statement (the host tests put it in the product's place)"""
    from speakerverification_amd import scoring
    F = np.asarray(feats, np.float32)
    if F.ndim == 2:
        F = F[:, None, :]
    blocks = group_scores(F, group_ptr)
    miss = miss_counts(blocks, scoring.audit_cut(threshold))
    if not scores:
        return miss
    sizes = np.diff(np.asarray(group_ptr, np.int64))
    return miss, flat_scores(blocks).astype(np.float32), np.concatenate([[0], np.cumsum(sizes * sizes)]).astype(np.int64)


def exact_data(sizes, n_crops, D, seed, flips=24):
    """Crop rows with exactly 64 entries of +-1 and zeros elsewhere (norm 8): every dot is an integer, every quotient a multiple of
    1 / 64, the sum over the crops exact in any order, so a score's bits are fixed: the exact sum after one correctly rounded division.
    A group's files are sign-flipped copies of the group's own pattern (up to `flips` of the 64 entries), so the scores spread over
    many values and many pairs share one."""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    F = np.zeros((n, n_crops, D), np.float32)
    at = 0
    for size in sizes:
        for c in range(n_crops):
            pos = rng.choice(D, 64, replace=False)
            sign = rng.choice(np.float32([-1.0, 1.0]), 64)
            for i in range(size):
                s = sign.copy()
                k = int(rng.integers(0, flips + 1))
                s[rng.choice(64, k, replace=False)] *= -1
                F[at + i, c, pos] = s
        at += size
    group_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return F, group_ptr
