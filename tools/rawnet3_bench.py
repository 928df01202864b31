"""RawNet3 and Raw3_ECAPA on the MI355X: throughput and per-kernel times ("RawNet3").

    python tools/rawnet3_bench.py [--steps N] [--warmup W] [--batch B]

At B = 256, L = 32000, for compute f32 and bf16:
  * emb/s of RawNet3 (one handle, device-resident batch) and of Raw3_ECAPA (its two branches on two streams), timed with device
    events over N >= 20 steps after W warm-up steps;
  * RawNet3's per-label kernel times from the handle's profiler (svhip_profile_*: event pairs around every launch), one JSON line per
    label, and the GEMM rows' TFLOP/s against the matrix peaks of the MI355X (2.5 PFLOP/s dense bf16, 157 TFLOP/s fp32).
Prints one JSON summary line at the end.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch             # noqa: E402

from speakerverification_amd import synth                # noqa: E402
from speakerverification_amd.engine import Engine        # noqa: E402

L = 32000
PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.0}
AUDIO_SPEC = dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1)
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw", audio_spec=AUDIO_SPEC)


def _time(fn, steps, warmup):
    """ms per call on device events (the calls enqueue on their handles' streams, which the events bracket through torch's stream)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def rawnet3(compute, B, steps, warmup):
    st = torch.cuda.Stream()             # (a handle on torch's current stream: async calls and the events order on it)
    with torch.cuda.stream(st):
        return _rawnet3(compute, B, steps, warmup)


def _rawnet3(compute, B, steps, warmup):
    eng = Engine(model="rawnet3", compute=compute, embed_dim=320, channels=1024, max_batch=B, samples=L,
                 stream=torch.cuda.current_stream().cuda_stream)
    eng.load_state_dict(synth.synth_state_dict(synth.rawnet3_param_spec(nOut=320), seed=1))
    eng.finalize()
    wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
    out = torch.empty((B, 320), device="cuda")
    ms = _time(lambda: eng.embed_wave(wav, out=out, async_=True), steps, warmup)
    row = {"model": "RawNet3", "compute": compute, "B": B, "ms_per_batch": round(ms, 3), "emb_per_s": round(B / ms * 1e3, 1),
           "gflop_per_utt": round(eng.flops_per_utterance / 1e9, 2)}
    print(json.dumps(row), flush=True)
    eng.profile(True)
    for _ in range(steps):
        eng.embed_wave(wav, out=out, async_=True)
    torch.cuda.synchronize()
    prof = eng.profile_results()
    eng.profile(False)
    eng.close()
    total = sum(v["ms"] for v in prof.values()) / steps
    kernels = []
    for name, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
        k = {"label": name, "ms_per_step": round(v["ms"] / steps, 4), "share": round(v["ms"] / steps / total, 3),
             "launches_per_step": v["launches"] // steps}
        if v["flops"] > 0 and name.startswith("gemm"):
            tf = v["flops"] / (v["ms"] * 1e-3) / 1e12
            k["tflops"] = round(tf, 1)
            k["of_peak"] = round(tf / PEAK_TFLOPS[compute], 3)
        kernels.append(k)
        print(json.dumps(dict(k, compute=compute)), flush=True)
    gemm = [v for n, v in prof.items() if n.startswith("gemm")]
    g_ms, g_fl = sum(v["ms"] for v in gemm), sum(v["flops"] for v in gemm)
    row.update(kernel_ms_per_step=round(total, 3), gemm_ms_per_step=round(g_ms / steps, 3),
               gemm_tflops=round(g_fl / (g_ms * 1e-3) / 1e12, 1) if g_ms else None,
               gemm_of_peak=round(g_fl / (g_ms * 1e-3) / 1e12 / PEAK_TFLOPS[compute], 3) if g_ms else None, kernels=kernels)
    return row


def raw3_ecapa(compute, B, steps, warmup):
    from speakerverification_amd.models import Raw3_ECAPA
    m = Raw3_ECAPA.MainModel(nOut=512, hip_compute=compute, embed_batch=B, **KW)
    wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
    ms = _time(lambda: m(wav), steps, warmup)
    row = {"model": "Raw3_ECAPA", "compute": compute, "B": B, "ms_per_batch": round(ms, 3), "emb_per_s": round(B / ms * 1e3, 1)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    assert torch.cuda.is_available() and a.steps >= 1
    res = []
    for compute in ("bf16", "f32"):
        res.append(rawnet3(compute, a.batch, a.steps, a.warmup))
        res.append(raw3_ecapa(compute, a.batch, a.steps, a.warmup))
    print(json.dumps({"L": L, "B": a.batch, "steps": a.steps, "warmup": a.warmup,
                      "results": [{k: v for k, v in r.items() if k != "kernels"} for r in res]}))


if __name__ == "__main__":
    main()
