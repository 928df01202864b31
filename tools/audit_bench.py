"""The dataset audit on the MI355X: Engine.group_audit next to the two ways a user could run the reference's label-noise audit
(src/benchmark/benchmark_dataset.py) before it existed, on the same device-resident embeddings, in ONE process ("Dataset
audit").

    python tools/audit_bench.py [--out profiles/audit_bench.json] [--only a,b,c,d]

Shapes (20 crops): (a) 2 000 folders of log-uniform 8 .. 512 files, D = 192; (b) one folder of 16 384 files, D = 192; (c) 20 000 folders
of 4 .. 32 files, D = 192; (d) shape (a) at D = 704, the width Raw_ECAPA_hype concatenates.  Operands: seeded unit rows around one
centroid per folder (noise 1.2: a same-folder cosine of about 0.41, so that the reference's default threshold 0.384 splits the pairs).
Yardsticks:
  (i)  what a user writes today: the host-made list of every within-folder pair, Engine.score_trials(mode="cosine") on device tensors,
       the comparison and two bincounts in torch.  The list's construction and its upload are timed once and reported separately;
  (ii) per folder torch.einsum('icd,jcd->ijc'), abs().mean(-1) and the comparison, on the device (in row slabs where the (n, n, crops)
       temporary would exceed 2 GiB).
Per shape: one warm-up of each version, then five timed passes in which the three alternate; a pass is bracketed by HIP events around
work that ends in a synchronise.  Recorded: the median, fastest and slowest pass of each, scores/s, group_audit's ratio to both
yardsticks, whether its counts equal yardstick (i)'s (and how many pairs lie within the accuracy bar of the cut: those may fall either
way), the per-label kernel times of one profiled call, and the MFMA kernel's achieved fp32 TFLOP/s against the 157 peak (work:
2 * n_crops * D per score COMPUTED: the kernel computes the upper triangle and the diagonal, each score once).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np       # noqa: E402
import torch             # noqa: E402

from speakerverification_amd import scoring              # noqa: E402
from speakerverification_amd.engine import Engine        # noqa: E402

RUNS, CROPS, NOISE, THRESHOLD, PEAK_TFLOPS = 5, 20, 1.2, 0.38405078649520874, 157.0
SLAB_BYTES = 1 << 31


def _sizes(shape):
    rng = np.random.default_rng(20261021)
    if shape in ("a", "d"):
        return np.exp(rng.uniform(np.log(8), np.log(512), 2000)).astype(np.int64).clip(8, 512), (704 if shape == "d" else 192)
    if shape == "b":
        return np.array([16384], np.int64), 192
    return rng.integers(4, 33, 20000).astype(np.int64), 192


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


def _operands(sizes, D):
    """(n_files, CROPS, D) unit rows on the device: folder centroid + NOISE * unit-variance noise / sqrt(D), normalised; 4 096 files at a time"""
    gen = torch.Generator(device="cuda").manual_seed(20261021)
    n = int(sizes.sum())
    cen = torch.randn((len(sizes), D), generator=gen, device="cuda")
    cen /= cen.norm(dim=1, keepdim=True)
    owner = torch.repeat_interleave(torch.arange(len(sizes), device="cuda"), torch.from_numpy(sizes).cuda())
    F = torch.empty((n, CROPS, D), dtype=torch.float32, device="cuda")
    for f0 in range(0, n, 4096):
        f1 = min(n, f0 + 4096)
        x = cen[owner[f0:f1]][:, None, :] + NOISE / D ** 0.5 * torch.randn((f1 - f0, CROPS, D), generator=gen, device="cuda")
        F[f0:f1] = x / x.norm(dim=-1, keepdim=True)
    return F


def _pair_list(gp):
    ia, ib = [], []
    for s, e in zip(gp[:-1], gp[1:]):
        a, b = np.triu_indices(int(e - s), 1)
        ia.append((a + s).astype(np.int32))
        ib.append((b + s).astype(np.int32))
    return np.concatenate(ia), np.concatenate(ib)


def bench_shape(eng, shape):
    sizes, D = _sizes(shape)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(gp[-1])
    F = _operands(sizes, D)
    cut = scoring.audit_cut(THRESHOLD)
    t0 = time.perf_counter()
    ia, ib = _pair_list(gp)
    t1 = time.perf_counter()
    dia, dib = torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    lia, lib = dia.long(), dib.long()
    res = {}

    def audit():
        res["audit"] = eng.group_audit(F, gp, cut)

    def pair_list():
        s = eng.score_trials(F, dia, dib, "cosine")
        m = s <= cut
        res["pairs"] = torch.bincount(lia[m], minlength=n) + torch.bincount(lib[m], minlength=n)
        res["pair_scores"] = s

    def einsum():
        out = torch.empty(n, dtype=torch.int64, device="cuda")
        for s, e in zip(gp[:-1].tolist(), gp[1:].tolist()):
            X = F[s:e]
            rows = max(1, min(e - s, SLAB_BYTES // ((e - s) * CROPS * 4)))
            for r0 in range(0, e - s, rows):
                S = torch.einsum("icd,jcd->ijc", X[r0:r0 + rows], X).abs().mean(-1)
                m = S <= cut
                idx = torch.arange(r0, min(e - s, r0 + rows), device="cuda")
                m[idx - r0, idx] = False
                out[s + r0:s + r0 + m.shape[0]] = m.sum(1)
        res["einsum"] = out

    versions = (("group_audit", audit), ("pair_list_score_trials_bincount", pair_list), ("per_folder_einsum", einsum))
    for _, fn in versions:
        fn()
    ms = {name: [] for name, _ in versions}
    for _ in range(RUNS):
        for name, fn in versions:
            ms[name].append(_timed(fn))
    st = {name: _stats(v) for name, v in ms.items()}
    new = st["group_audit"]["ms_median"]
    n_pairs = int(ia.size)
    bar = (2 * D + CROPS + 16) * 2.0 ** -24
    got, yard = res["audit"].long(), res["pairs"]
    eng.profile(True)
    audit()
    torch.cuda.synchronize()
    prof = eng.profile_results()
    eng.profile(False)
    k = prof.get("group_audit", {"ms": 0.0, "flops": 0.0})
    rec = {"shape": shape, "folders": int(len(sizes)), "n_files": n, "n_crops": CROPS, "D": D, "within_folder_pairs": n_pairs, "cut": float(cut),
           **st,
           "pair_list_build_s": round(t1 - t0, 4), "pair_list_upload_s": round(t2 - t1, 4), "pair_list_bytes": int(ia.nbytes + ib.nbytes),
           "audit_over_pair_list": round(new / st["pair_list_score_trials_bincount"]["ms_median"], 4),
           "audit_over_einsum": round(new / st["per_folder_einsum"]["ms_median"], 4),
           "pair_scores_per_s": {name: round(n_pairs / (v["ms_median"] * 1e-3), 1) for name, v in st.items()},
           "mismatching_pairs": int(got.sum().item()) // 2,
           "counts_equal_pair_list": bool(torch.equal(got, yard)), "files_whose_count_differs": int((got != yard).sum().item()),
           "counts_equal_einsum": bool(torch.equal(got, res["einsum"])),
           "pairs_within_bar_of_cut": int(((res["pair_scores"] - float(cut)).abs() <= bar).sum().item()), "bar": bar,
           "triangles": "upper triangle and diagonal: each score computed once",
           "labels": {name: {"ms": round(v["ms"], 4), "launches": v["launches"]} for name, v in prof.items()},
           "kernel_ms": round(k["ms"], 4), "kernel_scores_computed": int(n_pairs + n),
           "kernel_tflops": round(k["flops"] / (k["ms"] * 1e-3) / 1e12, 3) if k["ms"] else None,
           "kernel_fraction_of_fp32_mfma_peak": round(k["flops"] / (k["ms"] * 1e-3) / 1e12 / PEAK_TFLOPS, 4) if k["ms"] else None}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="the shapes to run, e.g. a,c")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "audit_bench needs a GPU"
    eng = Engine(model="none", max_batch=1)
    rec = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "threshold": THRESHOLD, "noise": NOISE, "shapes": []}
    for shape in "abcd":
        if a.only and shape not in a.only.split(","):
            continue
        row = bench_shape(eng, shape)
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
