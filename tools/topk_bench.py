"""1:N identification on the MI355X: Engine.score_topk next to what a user could do before it existed — Engine.score_matrix into a
device tensor followed by torch.topk — on the same device-resident inputs, in ONE process ("Top-k gallery search").

    python tools/topk_bench.py [--out profiles/topk_bench.json] [--only N,M,D]
    python tools/topk_bench.py --norm [--out profiles/topk_norm_bench.json] [--only N,M,D]

Shapes (k = 10): 16 384 x 16 384 x 192, 20 x 1 000 000 x 192, 4 096 x 1 000 000 x 192 (fused route) and 4 096 x 65 536 x 512 (slab route).
The yardstick runs in slabs of query rows where the matrix would exceed 2 GiB.  Per shape: one warm-up of each version, then five timed
passes in which the two versions alternate; a pass is bracketed by HIP events around work that ends in a synchronise.  Recorded: the
median, fastest and slowest pass of both, their ratio, the per-label kernel times of one profiled call of each (the library's event
profile, taken after the timed passes), the gallery bytes per second (M x D x 4 bytes, read once, over the pass) and the FLOP/s
(2 N M D over the pass) of score_topk, and how many of the two versions' index rows agree.

--norm: the AS-normalised search (Engine.score_topk_norm) on the same shapes in the same process, with the statistics of queries and
gallery taken once, outside the timed region, against a seeded cohort of 2 048 unit rows (top 200).  Three versions alternate in each of
the five passes: plain score_topk (the difference is what the normalising epilogue costs), score_topk_norm, and what a user could do
without it — score_matrix into a device tensor, the broadcast normalisation in torch (four elementwise passes over the slab), torch.topk.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np       # noqa: E402
import torch             # noqa: E402

from speakerverification_amd.engine import Engine        # noqa: E402

K, RUNS = 10, 5
SHAPES = ((16384, 16384, 192, "fused"), (20, 1000000, 192, "fused"), (4096, 1000000, 192, "fused"), (4096, 65536, 512, "slab"))
SLAB_BYTES = 1 << 31


def _unit_rows(n, d, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True)


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


def bench_shape(eng, N, M, D, route):
    Q, G = _unit_rows(N, D, 1), _unit_rows(M, D, 2)
    out = (torch.empty((N, K), dtype=torch.float32, device="cuda"), torch.empty((N, K), dtype=torch.int32, device="cuda"))
    rows = max(1, min(N, SLAB_BYTES // (M * 4)))
    slab = torch.empty((rows, M), dtype=torch.float32, device="cuda")
    ys, yi = torch.empty((N, K), dtype=torch.float32, device="cuda"), torch.empty((N, K), dtype=torch.int64, device="cuda")

    def topk():
        eng.score_topk(Q, G, K, out=out)

    def yardstick():
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            eng.score_matrix(Q[r0:r1], G, out=slab[:r1 - r0])
            torch.topk(slab[:r1 - r0], K, dim=1, out=(ys[r0:r1], yi[r0:r1]))

    topk()
    yardstick()
    t_new, t_old = [], []
    for _ in range(RUNS):
        t_new.append(_timed(topk))
        t_old.append(_timed(yardstick))
    new, old = _stats(t_new), _stats(t_old)
    sec = new["ms_median"] * 1e-3
    rec = {"N": N, "M": M, "D": D, "k": K, "route": route, "yardstick_slab_rows": rows,
           "score_topk": new, "score_matrix_plus_torch_topk": old,
           "speedup_over_yardstick": round(old["ms_median"] / new["ms_median"], 3),
           "score_topk_gallery_GBps": round(M * D * 4 / sec / 1e9, 1),
           "score_topk_TFLOPs": round(2.0 * N * M * D / sec / 1e12, 2),
           "index_rows_equal": int((out[1].long() == yi).all(dim=1).sum().item()),
           "max_abs_score_difference": float((out[0] - ys).abs().max().item())}
    rec["score_topk_labels"] = _profile(eng, topk)
    rec["yardstick_labels"] = _profile(eng, yardstick)
    return rec


def bench_shape_norm(eng, N, M, D, route):
    Q, G, cohort = _unit_rows(N, D, 1), _unit_rows(M, D, 2), _unit_rows(2048, D, 3)
    q_stats, g_stats = eng.asnorm_stats(Q, cohort, 200), eng.asnorm_stats(G, cohort, 200)
    out = (torch.empty((N, K), dtype=torch.float32, device="cuda"), torch.empty((N, K), dtype=torch.int32, device="cuda"))
    outp = (torch.empty_like(out[0]), torch.empty_like(out[1]))
    rows = max(1, min(N, SLAB_BYTES // (M * 4)))
    slab, tmp = torch.empty((rows, M), dtype=torch.float32, device="cuda"), torch.empty((rows, M), dtype=torch.float32, device="cuda")
    ys, yi = torch.empty((N, K), dtype=torch.float32, device="cuda"), torch.empty((N, K), dtype=torch.int64, device="cuda")
    aq, ag = 0.5 / q_stats[1], 0.5 / g_stats[1]
    bq, bg = q_stats[0] * aq, g_stats[0] * ag

    def plain():
        eng.score_topk(Q, G, K, out=outp)

    def norm():
        eng.score_topk_norm(Q, q_stats, G, g_stats, K, out=out)

    def yardstick():
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            s, t = slab[:r1 - r0], tmp[:r1 - r0]
            eng.score_matrix(Q[r0:r1], G, out=s)
            torch.mul(s, ag[None, :], out=t)                    # t = s (aq + ag) - (bq + bg), by broadcasting
            t.addcmul_(s, aq[r0:r1, None])
            t.sub_(bg[None, :])
            t.sub_(bq[r0:r1, None])
            torch.topk(t, K, dim=1, out=(ys[r0:r1], yi[r0:r1]))

    versions = (("score_topk", plain), ("score_topk_norm", norm), ("score_matrix_torch_norm_topk", yardstick))
    for _, fn in versions:
        fn()
    ms = {name: [] for name, _ in versions}
    for _ in range(RUNS):
        for name, fn in versions:
            ms[name].append(_timed(fn))
    st = {name: _stats(v) for name, v in ms.items()}
    new = st["score_topk_norm"]["ms_median"]
    rec = {"N": N, "M": M, "D": D, "k": K, "route": route, "cohort": 2048, "cohort_top": 200, "yardstick_slab_rows": rows, **st,
           "norm_over_plain": round(new / st["score_topk"]["ms_median"], 3),
           "speedup_over_yardstick": round(st["score_matrix_torch_norm_topk"]["ms_median"] / new, 3),
           "best_row_differs_from_plain": int((out[1][:, 0] != outp[1][:, 0]).sum().item()),
           "index_rows_equal_yardstick": int((out[1].long() == yi).all(dim=1).sum().item()),
           "max_abs_score_difference": float((out[0] - ys).abs().max().item())}
    rec["score_topk_labels"] = _profile(eng, plain)
    rec["score_topk_norm_labels"] = _profile(eng, norm)
    rec["yardstick_labels"] = _profile(eng, yardstick)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--norm", action="store_true", help="time score_topk_norm against score_topk and against score_matrix + torch")
    ap.add_argument("--only", default=None, help="N,M,D of the one shape to run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "topk_bench needs a GPU"
    eng = Engine(model="none", max_batch=1)
    rec = {"device": torch.cuda.get_device_name(0), "k": K, "runs": RUNS, "shapes": []}
    for N, M, D, route in SHAPES:
        if a.only and a.only != f"{N},{M},{D}":
            continue
        row = (bench_shape_norm if a.norm else bench_shape)(eng, N, M, D, route)
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
