"""Two-set clustering on the MI355X: Engine.cluster_join next to its only yardstick, Engine.cluster_above on the concatenation - what a
user had to run before the join existed - in ONE process on the same device-resident rows ("Two-set clustering").

    python tools/cluster_join_bench.py [--out profiles/cluster_join_bench.json] [--only NA,NB,D]

Shapes (NA x NB, D): 262 144 x 4 096, 262 144 x 16 384 and 1 048 576 x 64 at D = 192 with A seeded and B walked; 65 536 x 65 536 at
D = 192 with both sides seeded; 65 536 x 4 096 at D = 512 on the slab route, A seeded and B walked.  Rows and threshold: tools/cluster_bench.py's
(speaker-structured unit rows; the score one pair in 10^4 of a fixed sample reaches).  The seeds are cluster_above's roots of the seeded
sides, computed once outside the timed passes: they are what the user kept from yesterday's call.  Per shape: one warm-up of each
version, then five timed passes in which the versions alternate, each bracketed by HIP events around work that ends in a synchronise.
Recorded: the median, fastest and slowest pass of each; the join's time over the yardstick's and, beside it, the ratio of the pairs
walked ((NA NB + NB^2 / 2) / ((NA + NB)^2 / 2), or NA NB over the same where both sides are seeded); the per-label kernel times of one
profiled call of each; and cluster_join_link's rate over the pairs it walks (2 NA NB D flops).  The tool asserts that the two roots
are equal."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402

from speakerverification_amd import synth                       # noqa: E402
from speakerverification_amd.engine import Engine               # noqa: E402
from tools.cluster_bench import RUNS, _profile, _stats, _threshold, _timed      # noqa: E402

# NA, NB, D, route, both sides seeded
SHAPES = ((262144, 4096, 192, "fused", False), (262144, 16384, 192, "fused", False), (65536, 65536, 192, "fused", True),
          (1048576, 64, 192, "fused", False), (65536, 4096, 512, "slab", False))


def bench_shape(eng, NA, NB, D, route, both):
    e, _, _ = synth.synth_speaker_embeddings(NA + NB, dim=D, seed=2)
    E = torch.from_numpy(e).cuda()
    del e
    thr = _threshold(E)
    A, B = E[:NA], E[NA:]
    root_a = eng.cluster_above(A, thr)[0]
    root_b = eng.cluster_above(B, thr)[0] if both else None
    res = {}

    def join():
        res["join"] = eng.cluster_join(A, B, thr, root_a, root_b)

    def whole():
        res["whole"] = eng.cluster_above(E, thr)

    versions = [("cluster_join", join), ("cluster_above_of_the_concatenation", whole)]
    for _, fn in versions:
        fn()
    assert torch.equal(res["join"][0], res["whole"][0]) and int(res["join"][2]) == int(res["whole"][2])      # the same roots, exactly
    ms = {name: [] for name, _ in versions}
    for _ in range(RUNS):
        for name, fn in versions:
            ms[name].append(_timed(fn))
    st = {name: _stats(v) for name, v in ms.items()}
    assert torch.equal(res["join"][0], res["whole"][0])
    n = float(NA + NB)
    walked = float(NA) * NB + (0.0 if both else 0.5 * NB * NB)
    rec = {"NA": NA, "NB": NB, "D": D, "route": route, "seeded": "A and B" if both else "A", "threshold": thr, **st,
           "join_over_cluster_above": round(st["cluster_join"]["ms_median"] / st["cluster_above_of_the_concatenation"]["ms_median"], 4),
           "walked_pairs_ratio": round(walked / (0.5 * n * n), 4),
           "clusters": int(res["join"][2]), "clusters_of_A_alone": int((root_a == torch.arange(NA, device="cuda", dtype=torch.int32)).sum().item())}
    rec["cluster_join_labels"] = _profile(eng, join)
    rec["cluster_above_labels"] = _profile(eng, whole)
    link = rec["cluster_join_labels"].get("cluster_join_link")
    if link and link["ms"] > 0:
        rec["cluster_join_link_tflops_of_walked_pairs"] = round(2.0 * NA * NB * D / (link["ms"] * 1e-3) / 1e12, 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="NA,NB,D of the one shape to run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cluster_join_bench needs a GPU"
    eng = Engine(model="none", max_batch=1)
    rec = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "shapes": []}
    for NA, NB, D, route, both in SHAPES:
        if a.only and a.only != f"{NA},{NB},{D}":
            continue
        row = bench_shape(eng, NA, NB, D, route, both)
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
