"""ResNetSE34V2 on the MI355X: throughput, per-kernel breakdown, the convolution's TFLOP/s per stage and rs_se_apply's bandwidth, in ONE
process ("ResNetSE34V2").

    python tools/resnetse_bench.py [--steps N] [--runs R] [--out profiles/resnetse_bench.json]

Reports, at B = 256, L = 32000 (T = 401 frames, 80 mels):
  * ms per batch and embeddings/s of ResNetSE34V2 on bf16 and f32 handles (device-resident waveforms, asynchronous calls: mel front-end +
    net), as the median of R timed runs of N steps after a warm-up, with the runs' minimum and maximum;
  * ECAPA-TDNN C = 1024 bf16 beside it in the same process (the same-box yardstick);
  * from the handle's per-label event times (svhip_profile_*): the achieved TFLOP/s of each stage's rs_conv3x3 (algorithmic FLOPs: 2 x
    MACs) and the GB/s of rs_se_apply in algorithmic bytes (conv2's output and the residual read once, the block output written once).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch             # noqa: E402

from speakerverification_amd import synth                # noqa: E402
from speakerverification_amd.engine import Engine        # noqa: E402

B, L, N_MELS, NOUT = 256, 32000, 80, 256


def _runs(fn, steps, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps)
    return out


def _rate(ts):
    med = statistics.median(ts)
    return {"ms_per_batch": round(med * 1e3, 3), "ms_min": round(min(ts) * 1e3, 3), "ms_max": round(max(ts) * 1e3, 3),
            "emb_per_s": round(B / med, 1)}


def se_apply_bytes(esz):
    """algorithmic bytes of the 16 rs_se_apply launches of one batch: two tensors read, one written, per block"""
    blocks, widths = synth.RESNETSE_BLOCKS["ResNetSE34V2"]
    T, Q = L // 80 + 1, N_MELS
    total = 0
    for s, (n, C) in enumerate(zip(blocks, widths)):
        if s:
            T, Q = (T - 1) // 2 + 1, (Q - 1) // 2 + 1
        total += n * 3 * B * T * Q * C * esz
    return total


def resnetse(steps, runs, only=None):
    res = {}
    wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
    st = torch.cuda.Stream()
    out = torch.empty((B, NOUT), device="cuda")
    sd = synth.synth_state_dict(synth.resnetse_param_spec(NOUT, N_MELS), seed=1)
    for compute in ("bf16", "f32"):
        if only and only != f"resnetse_{compute}":
            continue
        with torch.cuda.stream(st):
            eng = Engine(model="resnetse", compute=compute, channels=2, n_mels=N_MELS, embed_dim=NOUT, max_batch=B, samples=L, log_input=True,
                         input_norm=True, stream=st.cuda_stream)
            eng.load_state_dict(sd)
            eng.finalize()
            ts = _runs(lambda: eng.embed_wave(wav, out=out, async_=True), steps, runs)
            eng.profile(True)
            for _ in range(steps):
                eng.embed_wave(wav, out=out, async_=True)
            torch.cuda.synchronize()
            p = eng.profile_results()
            eng.profile(False)
            flops = eng.flops_per_utterance
            eng.close()
        tot = sum(v["ms"] for v in p.values()) / steps
        r = _rate(ts)
        r["kernel_ms_per_batch"] = round(tot, 4)
        r["model_TFLOPs"] = round(flops * B / (r["ms_per_batch"] * 1e-3) / 1e12, 1)
        esz = 2 if compute == "bf16" else 4
        sa = p["rs_se_apply"]
        r["rs_se_apply_GBps"] = round(se_apply_bytes(esz) * steps / (sa["ms"] * 1e-3) / 1e9, 1)
        r["rs_conv3x3_TFLOPs"] = {k: round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) for k, v in sorted(p.items()) if k.startswith("rs_conv3x3")}
        r["labels"] = {kk: {"ms_per_batch": round(v["ms"] / steps, 4), "share": round(v["ms"] / steps / tot, 4),
                            "launches_per_batch": v["launches"] // steps,
                            "TFLOPs": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["flops"] else None}
                       for kk, v in sorted(p.items(), key=lambda kv: -kv[1]["ms"])}
        res[f"resnetse_{compute}"] = r
        print("resnetse", compute, json.dumps({kk: v for kk, v in r.items() if kk != "labels"}), flush=True)
    return res


def ecapa(steps, runs):
    wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
    st = torch.cuda.Stream()
    out = torch.empty((B, 192), device="cuda")
    with torch.cuda.stream(st):
        eng = Engine(model="ecapa", compute="bf16", channels=1024, max_batch=B, samples=L, stream=st.cuda_stream)
        eng.load_state_dict(synth.synth_state_dict(synth.ecapa_param_spec(C=1024), seed=1))
        eng.finalize()
        ts = _runs(lambda: eng.embed_wave(wav, out=out, async_=True), steps, runs)
        eng.close()
    r = _rate(ts)
    print("ecapa_C1024_bf16", json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one handle, e.g. 'resnetse_bf16' (a kernel trace of one model)")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    rec = {"B": B, "L": L, "T": L // 80 + 1, "device": torch.cuda.get_device_name(0), "steps": a.steps, "runs": a.runs}
    rec["resnetse"] = resnetse(a.steps, a.runs, a.only)
    if not a.only:
        rec["ecapa_C1024_bf16"] = ecapa(a.steps, a.runs)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
