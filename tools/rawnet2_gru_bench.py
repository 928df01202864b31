"""RawNet2's GRU aggregation on the MI355X: throughput against the asp aggregation, the GRU kernels' share and latency, in ONE process
("RawNet2 GRU aggregation").

    python tools/rawnet2_gru_bench.py [--steps N] [--out profiles/rawnet2_gru_bench.json]

Reports, at L = 32000 (T = 14 frames reach the GRU):
  * embeddings/s at B = 256 for f16 and f32x3 handles, asp and gru side by side (device-resident batches, asynchronous calls);
  * the library's per-kernel event times (svhip_profile_*) of the gru handles and the share of rn_gru_proj / rn_gru_step / rn_gru_fc;
  * the B = 20 call latency (host waveform in, host embedding out) of both aggregations on f16;
  * Raw_ECAPA_sinc_gru against Raw_ECAPA_sinc_asp (hip_compute='half', B = 256).
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

from speakerverification_amd import synth                # noqa: E402
from speakerverification_amd.engine import Engine        # noqa: E402

B, L = 256, 32000
AUDIO_SPEC = dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1)
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw", audio_spec=AUDIO_SPEC)
GRU_LABELS = ("rn_gru_proj", "rn_gru_step", "rn_gru_fc")


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def _engine(kind, compute, batch, stream=None):
    eng = Engine(model=kind, compute=compute, embed_dim=320, max_batch=batch, samples=L, stream=stream)
    eng.load_state_dict(synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, aggregate="gru" if kind == "rawnet2_gru" else "asp"), seed=1))
    eng.finalize()
    return eng


def throughput(steps):
    res = {}
    wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
    out = torch.empty((B, 320), device="cuda")
    st = torch.cuda.Stream()
    for compute in ("f16", "f32x3"):
        row = {}
        for kind in ("rawnet2", "rawnet2_gru"):
            with torch.cuda.stream(st):
                eng = _engine(kind, compute, B, st.cuda_stream)
                s = _time(lambda: eng.embed_wave(wav, out=out, async_=True), steps, 3)
                eng.profile(True)
                for _ in range(steps):
                    eng.embed_wave(wav, out=out, async_=True)
                torch.cuda.synchronize()
                p = eng.profile_results()
                eng.profile(False)
                eng.close()
            tot = sum(v["ms"] for v in p.values()) / steps
            r = {"ms_per_batch": round(s * 1e3, 3), "emb_per_s": round(B / s, 1), "kernel_ms_per_batch": round(tot, 4)}
            if kind == "rawnet2_gru":
                for k in GRU_LABELS:
                    r[k + "_us_per_batch"] = round(p[k]["ms"] / steps * 1e3, 1)
                    r[k + "_us_per_launch"] = round(p[k]["ms"] / p[k]["launches"] * 1e3, 2)
                r["gru_share_of_kernel_time"] = round(sum(p[k]["ms"] for k in GRU_LABELS) / steps / tot, 4)
                r["rn_gru_step_TFLOPs"] = round(p["rn_gru_step"]["flops"] / (p["rn_gru_step"]["ms"] * 1e-3) / 1e12, 1)
                r["rn_gru_proj_TFLOPs"] = round(p["rn_gru_proj"]["flops"] / (p["rn_gru_proj"]["ms"] * 1e-3) / 1e12, 1)
            row[kind] = r
            print(compute, kind, json.dumps(r), flush=True)
        row["gru_over_asp_rate"] = round(row["rawnet2_gru"]["emb_per_s"] / row["rawnet2"]["emb_per_s"], 4)
        res[compute] = row
    return res


def latency(steps):
    res = {}
    x = synth.synth_waveforms(20, L, seed=6)
    for kind in ("rawnet2", "rawnet2_gru"):
        eng = _engine(kind, "f16", 20)
        for _ in range(3):
            eng.embed_wave(x)
        t = []
        for _ in range(steps):
            t0 = time.perf_counter()
            eng.embed_wave(x)
            t.append(time.perf_counter() - t0)
        eng.close()
        res[kind] = {"B": 20, "median_ms": round(float(np.median(t)) * 1e3, 3), "min_ms": round(float(np.min(t)) * 1e3, 3)}
        print("latency f16", kind, json.dumps(res[kind]), flush=True)
    return res


def fusion(steps):
    from speakerverification_amd.models import Raw_ECAPA_sinc_asp, Raw_ECAPA_sinc_gru
    wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
    res = {}
    for name, mod in (("Raw_ECAPA_sinc_asp", Raw_ECAPA_sinc_asp), ("Raw_ECAPA_sinc_gru", Raw_ECAPA_sinc_gru)):
        m = mod.MainModel(nOut=512, hip_compute="half", embed_batch=B, **KW)
        s = _time(lambda: m(wav), steps, 3)
        res[name] = {"ms_per_batch": round(s * 1e3, 3), "emb_per_s": round(B / s, 1)}
        print(name, json.dumps(res[name]), flush=True)
        del m
    res["gru_over_asp_rate"] = round(res["Raw_ECAPA_sinc_gru"]["emb_per_s"] / res["Raw_ECAPA_sinc_asp"]["emb_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available()
    rec = {"B": B, "L": L, "T": 14, "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "throughput": throughput(a.steps), "latency_B20": latency(a.steps), "fusion_half": fusion(a.steps)}
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
