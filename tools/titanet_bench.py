"""TitaNet on the MI355X: throughput, per-kernel breakdown and the depthwise kernel's bandwidth, in ONE process ("TitaNet").

    python tools/titanet_bench.py [--steps N] [--out profiles/titanet_bench.json]

Reports, at B = 256, L = 32000 (T = 401 frames):
  * embeddings/s of TitaNet-M (H = 512, k = 7, 10 blocks, nOut 320) and TitaNet-L (H = 1024, k = 11, 5 blocks, nOut 512) on bf16 and
    f32 handles (device-resident waveforms, asynchronous calls: mel front-end + net);
  * the library's per-label event times (svhip_profile_*) and the achieved bandwidth of tn_dw in algorithmic bytes (input read once +
    output written once, over kernel time);
  * Tita_ECAPA and Raw_tita (hip_compute='half') beside Raw_ECAPA in the same process as a yardstick.
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
AUDIO_SPEC = dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1)
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw", audio_spec=AUDIO_SPEC)
MODELS = {"titanet_m": ("m", 320), "titanet_l": ("l", 512)}


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def throughput(steps, only=None):
    res = {}
    wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
    st = torch.cuda.Stream()
    for name, (size, nOut) in MODELS.items():
        H, k = synth.TITANET_SIZES[size]
        out = torch.empty((B, nOut), device="cuda")
        for compute in ("bf16", "f32"):
            if only and only != f"{name}_{compute}":
                continue
            with torch.cuda.stream(st):
                eng = Engine(model="titanet", compute=compute, channels=H, embed_dim=nOut, max_batch=B, samples=L, log_input=False,
                             stream=st.cuda_stream)
                eng.load_state_dict(synth.synth_state_dict(synth.titanet_param_spec(size, nOut), seed=1))
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
            T = L // 80 + 1
            esz = 2 if compute == "bf16" else 4
            dw = p["tn_dw"]
            dw_bytes = 2.0 * B * T * H * esz                     # one input read + one output write per launch
            r = {"ms_per_batch": round(s * 1e3, 3), "emb_per_s": round(B / s, 1), "kernel_ms_per_batch": round(tot, 4),
                 "tn_dw_us_per_launch": round(dw["ms"] / dw["launches"] * 1e3, 2),
                 "tn_dw_TBps": round(dw_bytes / (dw["ms"] / dw["launches"] * 1e-3) / 1e12, 2),
                 "labels": {kk: {"ms_per_batch": round(v["ms"] / steps, 4), "share": round(v["ms"] / steps / tot, 4),
                                 "launches_per_batch": v["launches"] // steps,
                                 "TFLOPs": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["flops"] else None}
                            for kk, v in sorted(p.items(), key=lambda kv: -kv[1]["ms"])}}
            res[f"{name}_{compute}"] = r
            print(name, compute, json.dumps({kk: v for kk, v in r.items() if kk != "labels"}), flush=True)
    return res


def fusion(steps):
    from speakerverification_amd.models import Raw_ECAPA, Raw_tita, Tita_ECAPA
    wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
    res = {}
    for name, mod in (("Raw_ECAPA", Raw_ECAPA), ("Tita_ECAPA", Tita_ECAPA), ("Raw_tita", Raw_tita)):
        m = mod.MainModel(nOut=512, hip_compute="half", embed_batch=B, **KW)
        s = _time(lambda: m(wav), steps, 3)
        res[name] = {"ms_per_batch": round(s * 1e3, 3), "emb_per_s": round(B / s, 1)}
        print(name, json.dumps(res[name]), flush=True)
        del m
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="'throughput', 'fusion' or one handle, e.g. 'titanet_m_bf16' (a kernel trace of one model)")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    rec = {"B": B, "L": L, "T": L // 80 + 1, "device": torch.cuda.get_device_name(0), "steps": a.steps}
    if a.only != "fusion":
        rec["throughput"] = throughput(a.steps, None if a.only in (None, "throughput") else a.only)
    if a.only in (None, "fusion"):
        rec["fusion_half"] = fusion(a.steps)
    print(json.dumps({k: v for k, v in rec.items() if k != "throughput"}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
