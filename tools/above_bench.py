"""Threshold search on the MI355X: Engine.score_above next to what a user could do before it existed — Engine.score_matrix into a
device tensor followed by (S >= thr).nonzero() in torch — and next to Engine.score_topk (k = 10) on the same device-resident operands,
in ONE process ("Threshold search").

    python tools/above_bench.py [--out profiles/above_bench.json] [--only N,M,D]

Shapes: 16 384 x 16 384 x 192, 4 096 x 1 000 000 x 192, the UPPER self-join 65 536 x 65 536 x 192 (fused route) and 4 096 x 65 536 x 512
(slab route).  Operands: unit vectors with speaker structure (synth.synth_speaker_embeddings: 5 994 centroids + within-speaker noise, as
the AS-norm benchmark builds them), queries and gallery drawn from the same speakers.  The threshold is the score that one pair in 10^4
of a fixed sample (1 024 queries x 65 536 gallery rows, float32 in torch) reaches: about one hit per 10^4 pairs, mostly same-speaker
pairs.  The yardstick runs in slabs of query rows where the matrix would exceed 2 GiB, and masks the self-join with triu.  Per shape:
one warm-up of each version, then five timed passes in which the three versions alternate; a pass is bracketed by HIP events around work
that ends in a synchronise.  Recorded: the median, fastest and slowest pass of each, score_above's ratio to the yardstick and to
score_topk (what the second MFMA pass, the recount of the fill call and the placement cost), the per-label kernel times of one profiled
call of each, the hit counts of both versions and whether their pair sets agree (score_matrix runs another GEMM route: a pair within
rounding of the threshold may fall on the other side).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np       # noqa: E402
import torch             # noqa: E402

from speakerverification_amd import synth                 # noqa: E402
from speakerverification_amd.engine import Engine        # noqa: E402

K, RUNS = 10, 5
SHAPES = ((16384, 16384, 192, "fused", False), (4096, 1000000, 192, "fused", False), (65536, 65536, 192, "fused", True),
          (4096, 65536, 512, "slab", False))
SLAB_BYTES = 1 << 31
HIT_RATE = 1e-4


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    torch.cuda.synchronize()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _stats(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def _profile(eng, fn):
    eng.profile(True)
    fn()
    torch.cuda.synchronize()
    res = {k: {"ms": round(v["ms"], 4), "launches": v["launches"]} for k, v in eng.profile_results().items()}
    eng.profile(False)
    return res


def _operands(N, M, D, upper):
    """queries and gallery from the same 5 994 speakers; the self-join's queries ARE the gallery"""
    e, _, _ = synth.synth_speaker_embeddings(M if upper else N + M, dim=D, seed=2)
    G = torch.from_numpy(e[:M] if upper else e[N:]).cuda()
    return (G if upper else torch.from_numpy(e[:N]).cuda()), G


def _threshold(Q, G):
    s = (Q[:1024] @ G[:65536].T).reshape(-1)
    return float(torch.topk(s, max(1, int(HIT_RATE * s.numel())), sorted=True).values[-1].item())


def bench_shape(eng, N, M, D, route, upper):
    Q, G = _operands(N, M, D, upper)
    thr = _threshold(Q, G)
    out = (torch.empty((N, K), dtype=torch.float32, device="cuda"), torch.empty((N, K), dtype=torch.int32, device="cuda"))
    rows = max(1, min(N, SLAB_BYTES // (M * 4)))
    slab = torch.empty((rows, M), dtype=torch.float32, device="cuda")
    res = {}

    def above():
        res["above"] = eng.score_above(Q, G, thr, upper=upper)

    def yardstick():
        found = []
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            s = slab[:r1 - r0]
            eng.score_matrix(Q[r0:r1], G, out=s)
            if upper:
                s.triu_(r0 + 1)                                  # (thr > 0: a zeroed entry is no hit)
            nz = (s >= thr).nonzero()
            nz[:, 0] += r0
            found.append(nz)
        res["yardstick"] = torch.cat(found)

    def topk():
        eng.score_topk(Q, G, K, out=out)

    versions = (("score_above", above), ("score_matrix_plus_torch_nonzero", yardstick), ("score_topk", topk))
    for _, fn in versions:
        fn()
    ms = {name: [] for name, _ in versions}
    for _ in range(RUNS):
        for name, fn in versions:
            ms[name].append(_timed(fn))
    st = {name: _stats(v) for name, v in ms.items()}
    new = st["score_above"]["ms_median"]
    row_ptr, index, _ = res["above"]
    pairs = torch.stack([torch.repeat_interleave(torch.arange(N, device="cuda"), row_ptr[1:] - row_ptr[:-1]), index.long()], dim=1)
    yard = res["yardstick"]
    rec = {"N": N, "M": M, "D": D, "route": route, "upper": upper, "threshold": thr, "k_of_score_topk": K, "yardstick_slab_rows": rows, **st,
           "above_over_yardstick": round(new / st["score_matrix_plus_torch_nonzero"]["ms_median"], 3),
           "above_over_topk": round(new / st["score_topk"]["ms_median"], 3),
           "hits": int(index.numel()), "hits_yardstick": int(yard.shape[0]),
           "hits_per_1e4_pairs": round(index.numel() / (N * (M - 1) / 2 if upper else N * M) * 1e4, 3),
           "pair_sets_equal": bool(pairs.shape == yard.shape and torch.equal(pairs, yard))}
    rec["score_above_labels"] = _profile(eng, above)
    rec["yardstick_labels"] = _profile(eng, yardstick)
    rec["score_topk_labels"] = _profile(eng, topk)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="N,M,D of the one shape to run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "above_bench needs a GPU"
    eng = Engine(model="none", max_batch=1)
    rec = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "hit_rate_aimed_at": HIT_RATE, "shapes": []}
    for N, M, D, route, upper in SHAPES:
        if a.only and a.only != f"{N},{M},{D}":
            continue
        row = bench_shape(eng, N, M, D, route, upper)
        rec["shapes"].append(row)
        print(json.dumps(row), flush=True)
        eng.trim_scratch()
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
