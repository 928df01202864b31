"""Raw_ECAPA_hype on the MI355X: throughput next to Raw_ECAPA_sinc_gru, whose branches it shares, and the cost of its attention-head
kernel, in ONE process ("Raw_ECAPA_hype's attention head").

    python tools/hype_bench.py [--steps N] [--out profiles/hype_bench.json]

Reports, at B = 256 for hip_compute 'half' and 'f32x3', at L = 16000 (8 kHz x 2 s, the saved experiment's config) and L = 32000
(16 kHz x 2 s), on device-resident batches:
  * ms per batch and embeddings/s of both models: the median of five runs of `steps` forwards, with the fastest and the slowest run;
  * hype_head's time per launch from the library's event profile (svhip_profile_*) of the head's handle, and its share of the
    Raw_ECAPA_sinc_gru step measured beside it.
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

B, RUNS = 256, 5
CASES = ((8000, 16000), (16000, 32000))          # (sample rate, samples)


def _kw(sr, L):
    spec = dict(sample_rate=sr, sentence_len=L / float(sr), win_len=0.025, hop_len=0.01, channels=1)
    return dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw", audio_spec=spec)


def _runs(fn, steps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) / steps)
    return {"ms_per_batch": round(float(np.median(t)) * 1e3, 3), "ms_min": round(min(t) * 1e3, 3), "ms_max": round(max(t) * 1e3, 3),
            "emb_per_s": round(B / float(np.median(t)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available()
    from speakerverification_amd.models import Raw_ECAPA_hype, Raw_ECAPA_sinc_gru
    rec = {"B": B, "device": torch.cuda.get_device_name(0), "steps": a.steps, "runs": RUNS, "cases": {}}
    for sr, L in CASES:
        wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
        for compute in ("half", "f32x3"):
            row = {}
            for name, mod in (("Raw_ECAPA_sinc_gru", Raw_ECAPA_sinc_gru), ("Raw_ECAPA_hype", Raw_ECAPA_hype)):
                m = mod.MainModel(nOut=512, hip_compute=compute, embed_batch=B, **_kw(sr, L))
                row[name] = _runs(lambda: m(wav), a.steps)
                if name == "Raw_ECAPA_hype":
                    head = m._head_engine()
                    head.profile(True, only="hype_head")
                    for _ in range(a.steps):
                        m(wav)
                    torch.cuda.synchronize()
                    p = head.profile_results()["hype_head"]
                    head.profile(False)
                    row["hype_head_us_per_launch"] = round(p["ms"] / p["launches"] * 1e3, 2)
                    row["hype_head_launches_per_forward"] = p["launches"] / a.steps
                del m
            row["hype_over_sinc_gru_rate"] = round(row["Raw_ECAPA_hype"]["emb_per_s"] / row["Raw_ECAPA_sinc_gru"]["emb_per_s"], 4)
            row["hype_head_share_of_sinc_gru_step"] = round(row["hype_head_us_per_launch"] * 1e-3 / row["Raw_ECAPA_sinc_gru"]["ms_per_batch"], 5)
            rec["cases"][f"sr{sr}_L{L}_{compute}"] = row
            print(f"sr={sr} L={L} {compute}", json.dumps(row), flush=True)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
