"""Speaker clustering on the MI355X: Engine.cluster_above next to the two ways a user had before it existed, in ONE process on the same
device-resident rows ("Speaker clustering"):

  (i)  the `duplicates` path: score_above(upper=True) per chunk of 65 536 query rows, the pair list copied to the host,
       scipy.sparse.csgraph.connected_components there;
  (ii) score_matrix into a device tensor + (S >= thr).nonzero() in torch (slabs of query rows where the matrix would exceed 2 GiB, the
       self-join masked with triu) and the same host components - for the shapes up to 65 536 rows (at 262 144 the matrix is 256 GiB).

    python tools/cluster_bench.py [--out profiles/cluster_bench.json] [--only N,D]

Shapes: 16 384, 65 536 and 262 144 rows x 192 (fused route) and 65 536 x 512 (slab route).  Rows: unit vectors with speaker structure
(synth.synth_speaker_embeddings: 5 994 centroids + within-speaker noise, as tools/above_bench.py builds them).  The threshold is the
score one pair in 10^4 of a fixed sample reaches (tools/above_bench.py's rule): mostly same-speaker pairs.  Per shape: one warm-up of
each version, then five timed passes in which the versions alternate; a pass is bracketed by HIP events around work that ends in a
synchronise, and the yardsticks' host part (the copy and the components) is inside the bracket, since it is part of the answer.
Recorded: the median, fastest and slowest pass of each, cluster_above's ratio to each yardstick, the cluster counts (which must agree;
(ii) runs another GEMM route, so there a pair within rounding of the threshold may fall on the other side: its count is recorded, not
asserted), the per-label kernel times of one profiled call and the cluster_link kernel's rate over the flops of the pairs i < j it
must compute (N (N - 1) D) and over those of the gallery slices its workgroups walk (the profile's figure: whole slices from the diagonal
on, so more than the pairs).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402
from scipy.sparse import coo_matrix                             # noqa: E402
from scipy.sparse.csgraph import connected_components           # noqa: E402

from speakerverification_amd import synth                       # noqa: E402
from speakerverification_amd.engine import Engine               # noqa: E402

RUNS = 5
SHAPES = ((16384, 192, "fused"), (65536, 192, "fused"), (262144, 192, "fused"), (65536, 512, "slab"))
CHUNK = 65536                    # ModelHandling.duplicates' default
SLAB_BYTES = 1 << 31
MATRIX_ROWS_MAX = 65536          # yardstick (ii) runs up to here
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
    res = {k: {"ms": round(v["ms"], 4), "launches": v["launches"], "flops": v["flops"]} for k, v in eng.profile_results().items()}
    eng.profile(False)
    return res


def _threshold(E):
    s = (E[:1024] @ E[:65536].T).reshape(-1)
    return float(torch.topk(s, max(1, int(HIT_RATE * s.numel())), sorted=True).values[-1].item())


def _host_components(N, i, j):
    g = coo_matrix((np.ones(i.size, np.int8), (i, j)), shape=(N, N))
    return connected_components(g, directed=False)[0]


def bench_shape(eng, N, D, route):
    e, _, _ = synth.synth_speaker_embeddings(N, dim=D, seed=2)
    E = torch.from_numpy(e).cuda()
    thr = _threshold(E)
    res = {}

    def cluster():
        res["cluster"] = eng.cluster_above(E, thr)

    def duplicates_path():
        ii, jj = [], []
        for base in range(0, N, CHUNK):
            rows = E[base:base + CHUNK]
            row_ptr, index, _ = eng.score_above(rows, E, thr, upper=True, q_base=base)
            rp = row_ptr.cpu().numpy()
            ii.append(np.repeat(np.arange(base, base + rows.shape[0], dtype=np.int64), np.diff(rp)))
            jj.append(index.cpu().numpy())
        i, j = np.concatenate(ii), np.concatenate(jj)
        res["pairs"] = int(i.size)
        res["c_duplicates"] = _host_components(N, i, j)

    versions = [("cluster_above", cluster), ("duplicates_path_plus_host_components", duplicates_path)]
    if N <= MATRIX_ROWS_MAX:
        rows_per = max(1, min(N, SLAB_BYTES // (N * 4)))
        slab = torch.empty((rows_per, N), dtype=torch.float32, device="cuda")

        def matrix_path():
            found = []
            for r0 in range(0, N, rows_per):
                r1 = min(N, r0 + rows_per)
                s = slab[:r1 - r0]
                eng.score_matrix(E[r0:r1], E, out=s)
                s.triu_(r0 + 1)                                  # (thr > 0: a zeroed entry is no link)
                nz = (s >= thr).nonzero()
                nz[:, 0] += r0
                found.append(nz)
            nz = torch.cat(found).cpu().numpy()
            res["pairs_matrix"] = int(nz.shape[0])
            res["c_matrix"] = _host_components(N, nz[:, 0], nz[:, 1])

        versions.append(("score_matrix_plus_nonzero_plus_host_components", matrix_path))
    for _, fn in versions:
        fn()
    ms = {name: [] for name, _ in versions}
    for _ in range(RUNS):
        for name, fn in versions:
            ms[name].append(_timed(fn))
    st = {name: _stats(v) for name, v in ms.items()}
    new = st["cluster_above"]["ms_median"]
    root, cluster_id, C = res["cluster"]
    C = int(C)
    assert C == res["c_duplicates"], (C, res["c_duplicates"])       # the same scores, bit for bit: the same components
    sizes = torch.bincount(cluster_id.long())
    rec = {"N": N, "D": D, "route": route, "threshold": thr, **st,
           "cluster_over_duplicates_path": round(new / st["duplicates_path_plus_host_components"]["ms_median"], 3),
           "clusters": C, "clusters_duplicates_path": int(res["c_duplicates"]), "pairs_of_duplicates_path": res["pairs"],
           "largest_cluster": int(sizes.max().item()), "singletons": int((sizes == 1).sum().item())}
    if "c_matrix" in res:
        rec["cluster_over_matrix_path"] = round(new / st["score_matrix_plus_nonzero_plus_host_components"]["ms_median"], 3)
        rec["clusters_matrix_path"] = int(res["c_matrix"])
        rec["pairs_of_matrix_path"] = res["pairs_matrix"]
    rec["cluster_above_labels"] = _profile(eng, cluster)
    rec["duplicates_path_labels"] = _profile(eng, duplicates_path)
    link = rec["cluster_above_labels"].get("cluster_link")
    if link and link["ms"] > 0:
        rec["cluster_link_tflops_of_needed_pairs"] = round(float(N) * (N - 1) * D / (link["ms"] * 1e-3) / 1e12, 2)
        rec["cluster_link_tflops_of_walked_slices"] = round(link["flops"] / (link["ms"] * 1e-3) / 1e12, 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="N,D of the one shape to run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cluster_bench needs a GPU"
    eng = Engine(model="none", max_batch=1)
    rec = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "hit_rate_aimed_at": HIT_RATE, "duplicates_chunk": CHUNK, "shapes": []}
    for N, D, route in SHAPES:
        if a.only and a.only != f"{N},{D}":
            continue
        row = bench_shape(eng, N, D, route)
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
