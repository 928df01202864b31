"""Conformer on the MI355X: throughput, per-kernel breakdown, the attention kernel's bandwidth and the subsampling GEMM's fraction of
peak, in ONE process ("Conformer").

    python tools/conformer_bench.py [--steps N] [--out profiles/conformer_bench.json] [--only conformer_bf16]

Reports, at B = 256, L = 32000 (T = 401 frames, T' = 99):
  * embeddings/s of the Conformer (nOut 512) on bf16 and f32 handles (device-resident waveforms, asynchronous calls: mel front-end +
    net), with ECAPA C = 1024 bf16 in the same process as the yardstick;
  * the library's per-label event times (svhip_profile_*); cf_attn's bandwidth in algorithmic bytes (q, k, v read once, the context
    written once, over kernel time); the subsampling GEMM's (gemm_generic at M = B T' F2, N = 256, K = 2304) TFLOP/s and its fraction
    of the dense peak (2.5 PFLOP/s bf16, 157 TFLOP/s fp32 matrix).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch             # noqa: E402

from speakerverification_amd import synth                # noqa: E402
from speakerverification_amd.engine import Engine        # noqa: E402

B, L = 256, 32000
PEAK = {"bf16": 2.5e15, "f32": 157.3e12}


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def _run(model, compute, kw, sd, nOut, steps, wav, st):
    out = torch.empty((B, nOut), device="cuda")
    with torch.cuda.stream(st):
        eng = Engine(model=model, compute=compute, embed_dim=nOut, max_batch=B, samples=L, stream=st.cuda_stream, **kw)
        eng.load_state_dict(sd)
        eng.finalize()
        s = _time(lambda: eng.embed_wave(wav, out=out, async_=True), steps, 3)
        eng.profile(True)
        for _ in range(steps):
            eng.embed_wave(wav, out=out, async_=True)
        torch.cuda.synchronize()
        p = eng.profile_results()
        eng.profile(False)
        eng.close()
    tot = sum(v["ms"] for v in p.values()) / steps
    r = {"ms_per_batch": round(s * 1e3, 3), "emb_per_s": round(B / s, 1), "kernel_ms_per_batch": round(tot, 4),
         "labels": {k: {"ms_per_batch": round(v["ms"] / steps, 4), "share": round(v["ms"] / steps / tot, 4),
                        "launches_per_batch": v["launches"] // steps,
                        "TFLOPs": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["flops"] else None}
                    for k, v in sorted(p.items(), key=lambda kv: -kv[1]["ms"])}}
    return r, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one handle: 'conformer_bf16', 'conformer_f32' or 'ecapa_bf16' (a kernel trace of one model)")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    T = L // 80 + 1
    Tp = synth.conformer_frames(T)
    F2 = synth.conformer_f2(80)
    rec = {"B": B, "L": L, "T": T, "T_sub": Tp, "device": torch.cuda.get_device_name(0), "steps": a.steps, "throughput": {}}
    wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
    st = torch.cuda.Stream()
    cf_sd = synth.synth_state_dict(synth.conformer_param_spec(512, 80), seed=1)
    for compute in ("bf16", "f32"):
        name = f"conformer_{compute}"
        if a.only and a.only != name:
            continue
        r, p = _run("conformer", compute, dict(channels=256, log_input=True, input_norm=True), cf_sd, 512, a.steps, wav, st)
        esz = 2 if compute == "bf16" else 4
        at = p["cf_attn"]
        us = at["ms"] / at["launches"] * 1e3
        r["cf_attn_us_per_launch"] = round(us, 2)
        r["cf_attn_TBps"] = round(B * Tp * 4 * 256 * esz / (us * 1e-6) / 1e12, 3)        # q, k, v read + context written
        g = p["gemm_generic"]                        # (the subsampling GEMM is the only generic-kernel GEMM of the net)
        fl = 2.0 * B * Tp * F2 * 256 * 2304
        ms = g["ms"] / a.steps
        r["subsample_gemm_ms_per_batch"] = round(ms, 4)
        r["subsample_gemm_TFLOPs"] = round(fl / (ms * 1e-3) / 1e12, 1)
        r["subsample_gemm_fraction_of_peak"] = round(fl / (ms * 1e-3) / PEAK[compute], 4)
        rec["throughput"][name] = r
        print(name, json.dumps({k: v for k, v in r.items() if k != "labels"}), flush=True)
    if a.only in (None, "ecapa_bf16"):
        sd = synth.synth_state_dict(synth.ecapa_param_spec(C=1024, nOut=192), seed=1)
        r, _ = _run("ecapa", "bf16", dict(channels=1024), sd, 192, a.steps, wav, st)
        rec["throughput"]["ecapa_c1024_bf16"] = r
        print("ecapa_c1024_bf16", json.dumps({k: v for k, v in r.items() if k != "labels"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
