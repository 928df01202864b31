"""Average / complete linkage on the MI355X: Engine.cluster_linkage next to cluster_above (the increment is the cost of the feature) and
next to what a user had before it existed, in ONE process on the same device-resident rows ("Average and complete linkage"):

  (i)  cluster_above, the labels and the rows copied to the host, scipy.cluster.hierarchy.linkage + fcluster per component of two
       rows or more (the containment argument applied by hand);
  (ii) score_matrix + scipy's linkage + fcluster on the WHOLE set, where the condensed float64 matrix fits (16 384 rows: 1 GiB) - one
       timed pass, it takes tens of seconds.

    python tools/linkage_bench.py [--out profiles/linkage_bench.json] [--only N,D] [--linkage average|complete]

Shapes: tools/cluster_bench.py's four at its thresholds (one pair in 10^4), and one CHAINED shape: 65 536 x 192 at the first of a
ladder of lower thresholds at which the largest component has at least 300 rows (and at most SVHIP_LINKAGE_MAX_ROWS, so it is refined;
a component beyond that is one cluster for the yardstick as it is for the call).
Then ONE component alone, of 256, 512 and SVHIP_LINKAGE_MAX_ROWS rows around one centroid (thr = 0.5: every pair is linked): the call,
the call with option "linkage_fill_only" (the matrix is built, nothing is merged) and cluster_above beside them - the fill / merge split
of the scratch home, and the figure the row cap was set by.
Per shape and linkage: one warm-up of each version, then five timed passes in which the versions alternate; the yardstick's host part
is inside the bracket.  The cluster count must equal yardstick (i)'s wherever the float64 statement (tests/linkage_statement.py) has no
decision within its accuracy bar on a 4 096-row sample of the shape; otherwise the difference is recorded.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402
from scipy.cluster.hierarchy import fcluster, linkage as scipy_linkage      # noqa: E402
from scipy.spatial.distance import squareform                   # noqa: E402

from speakerverification_amd import _lib, synth                 # noqa: E402
from speakerverification_amd.engine import Engine               # noqa: E402
from tests import linkage_statement as ls                       # noqa: E402
from tools.cluster_bench import RUNS, SHAPES, _profile, _stats, _threshold, _timed      # noqa: E402

CHAINED = (65536, 192)
# The ladder the chained shape walks.  Between 0.59 (every same-speaker pair is in, the largest component has 24 rows) and 0.30 (one
# component of 65 158 rows) the synthetic rows percolate within a few hundredths: 0.34 -> 129 rows, 0.33 -> 819, 0.32 -> 42 614.
CHAIN_THRESHOLDS = (0.34, 0.335, 0.33, 0.3275, 0.325)
MATRIX_ROWS_MAX = 16384
SAMPLE = 4096


def _scipy_count(V, thr, method):
    """clusters of one set from its float64 score matrix, as a scipy user would get them"""
    top = float(V.max()) + 1.0
    dist = top - V
    np.fill_diagonal(dist, 0.0)
    return int(fcluster(scipy_linkage(squareform(dist, checks=False), method), top - thr, "distance").max())


def bench_shape(eng, N, D, route, linkages, chained):
    e, _, _ = synth.synth_speaker_embeddings(N, dim=D, seed=2)
    E = torch.from_numpy(e).cuda()
    if chained:
        for thr in CHAIN_THRESHOLDS:
            largest = int(torch.bincount(eng.cluster_above(E, thr)[1].long()).max().item())
            if largest >= 300:
                break
        assert 300 <= largest <= _lib.LINKAGE_MAX_ROWS, (thr, largest)
    else:
        thr = _threshold(E)
    res = {}

    def single():
        res["single"] = eng.cluster_above(E, thr)

    def yardstick_components(method):
        def run():
            root, _, _ = eng.cluster_above(E, thr)
            r, rows = root.cpu().numpy(), E.cpu().numpy().astype(np.float64)
            order = np.argsort(r, kind="stable")
            cuts = np.flatnonzero(np.diff(r[order])) + 1
            count = 0
            for members in np.split(order, cuts):
                if members.size == 1 or members.size > _lib.LINKAGE_MAX_ROWS:      # (beyond the cap: one cluster, as the call leaves it)
                    count += 1
                else:
                    x = rows[members]
                    count += _scipy_count(x @ x.T, thr, method)
            res["c_components_" + method] = count
        return run

    rec = {"N": N, "D": D, "route": route, "chained": chained, "threshold": thr}
    sample = e[:SAMPLE]
    for method in linkages:
        def new():
            res[method] = eng.cluster_linkage(E, thr, None, method)

        versions = [("cluster_linkage", new), ("cluster_above", single), ("cluster_above_plus_scipy_per_component", yardstick_components(method))]
        for _, fn in versions:
            fn()
        ms = {name: [] for name, _ in versions}
        for _ in range(RUNS):
            for name, fn in versions:
                ms[name].append(_timed(fn))
        st = {name: _stats(v) for name, v in ms.items()}
        _, cluster_id, C, U = res[method]
        sizes = torch.bincount(cluster_id.long())
        comp = torch.bincount(res["single"][1].long())
        undecided = ls.statement(sample, thr, None, method)[3]
        row = {**st, "clusters": int(C), "unrefined": int(U), "clusters_yardstick_components": res["c_components_" + method],
               "components": int(res["single"][2]), "largest_component": int(comp.max().item()),
               "components_of_two_rows_or_more": int((comp >= 2).sum().item()), "largest_cluster": int(sizes.max().item()),
               "statement_undecided_on_sample": int(undecided),
               "linkage_minus_above_ms": round(st["cluster_linkage"]["ms_median"] - st["cluster_above"]["ms_median"], 4),
               "linkage_over_yardstick_components": round(st["cluster_linkage"]["ms_median"] / st["cluster_above_plus_scipy_per_component"]["ms_median"], 4)}
        if undecided == 0 and int(U) == 0:
            assert int(C) == row["clusters_yardstick_components"], (method, int(C), row["clusters_yardstick_components"])
        row["clusters_minus_yardstick"] = int(C) - row["clusters_yardstick_components"]
        if N <= MATRIX_ROWS_MAX:
            def matrix_path():
                S = eng.score_matrix(E, E).cpu().numpy().astype(np.float64)
                res["c_matrix"] = _scipy_count(S, thr, method)
            row["score_matrix_plus_scipy_whole_set_ms_one_pass"] = round(_timed(matrix_path), 1)
            row["clusters_matrix_path"] = res["c_matrix"]
        row["labels"] = _profile(eng, new)
        rec[method] = row
    return rec


def bench_single(eng, m, linkages):
    rng = np.random.default_rng(5)
    c = rng.standard_normal(192)
    c /= np.linalg.norm(c)
    rows = c + rng.standard_normal((m, 192)) * np.sqrt(0.55 / 192)
    E = torch.from_numpy((rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)).cuda()
    comp = eng.cluster_above(E, 0.5)
    rec = {"single_component_rows": m, "components": int(comp[2]), "cluster_above": _stats([_timed(lambda: eng.cluster_above(E, 0.5)) for _ in range(RUNS)])}
    for method in linkages:
        row = {}
        for name, fill_only in (("cluster_linkage", 0), ("cluster_linkage_fill_only", 1)):
            eng.set_option("linkage_fill_only", fill_only)
            try:
                res = eng.cluster_linkage(E, 0.5, None, method)
                row[name] = _stats([_timed(lambda: eng.cluster_linkage(E, 0.5, None, method)) for _ in range(RUNS)])
                row[name]["clusters"] = int(res[2])
                row[name]["labels"] = {k: v for k, v in _profile(eng, lambda: eng.cluster_linkage(E, 0.5, None, method)).items() if k.startswith("linkage")}
            finally:
                eng.set_option("linkage_fill_only", 0)
        rec[method] = row
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="N,D of the one shape to run ('chained': the chained shape; 'single': the single components)")
    ap.add_argument("--linkage", default=None, choices=ls.LINKAGES, help="one linkage instead of both")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "linkage_bench needs a GPU"
    eng = Engine(model="none", max_batch=1)
    linkages = (a.linkage,) if a.linkage else ls.LINKAGES
    rec = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "max_rows": _lib.LINKAGE_MAX_ROWS, "lds_rows": _lib.LINKAGE_LDS_ROWS, "shapes": []}
    for N, D, route, chained in [s + (False,) for s in SHAPES] + [CHAINED + ("fused", True)]:
        if a.only and a.only != ("chained" if chained else f"{N},{D}"):
            continue
        row = bench_shape(eng, N, D, route, linkages, chained)
        rec["shapes"].append(row)
        print(json.dumps(row), flush=True)
        eng.trim_scratch()
        torch.cuda.empty_cache()
    rec["single_components"] = []
    for m in (256, 512, _lib.LINKAGE_MAX_ROWS):
        if a.only and a.only != "single":
            continue
        row = bench_single(eng, m, linkages)
        rec["single_components"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
