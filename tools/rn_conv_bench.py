"""RawNet2 'conv' front-end on the MI355X: kernel times and throughput ("RawNet2 conv front-end").

    python tools/rn_conv_bench.py kernels [--steps N]    # B = 256 fp16 L = 32000: block 0 fused (rn_block128_conv), then option
                                                          # rn_conv_unfused (rn_conv3_front + rn_block128); run under
                                                          # rocprofv3 --kernel-trace --stats for the per-kernel table
    python tools/rn_conv_bench.py throughput [--steps N]  # utt/s at B = 256, hip_compute='half', one process: RawNet2 conv and sinc
                                                          # branches, Raw_ECAPA_conv_asp and Raw_ECAPA_sinc_asp (device-resident batches)

Both modes also print the library's own per-kernel event times (svhip_profile_*) and the achieved bytes per second of the
front-end: algorithmic bytes = waveform read (B L 4) + x written (B T1 128 2).
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
T1 = (L - 3) // 3 + 1
AUDIO_SPEC = dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1)
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw", audio_spec=AUDIO_SPEC)


def kernels(steps):
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        eng = Engine(model="rawnet2_conv", compute="f16", embed_dim=320, max_batch=B, samples=L, stream=st.cuda_stream)
        eng.load_state_dict(synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, front_proc="conv"), seed=1))
        eng.finalize()
        wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
        out = torch.empty((B, 320), device="cuda")
        res = {}
        outs = {}
        for mode in (0, 1):
            eng.set_option("rn_conv_unfused", mode)
            for _ in range(3):
                eng.embed_wave(wav, out=out, async_=True)
            torch.cuda.synchronize()
            eng.profile(True)
            for _ in range(steps):
                eng.embed_wave(wav, out=out, async_=True)
            torch.cuda.synchronize()
            p = eng.profile_results()
            eng.profile(False)
            outs[mode] = out.cpu().numpy().copy()
            per = {k: v["ms"] / v["launches"] * 1e3 for k, v in p.items()}
            tot = sum(v["ms"] for v in p.values()) / steps
            name = "unfused (rn_conv3_front + rn_block128)" if mode else "fused (rn_block128_conv)"
            row = {"all_kernels_ms_per_step": round(tot, 4)}
            for k in ("rn_conv3_front", "rn_block128_conv", "rn_block128"):
                if k in per:
                    row[k + "_us"] = round(per[k], 1)
            if "rn_conv3_front" in per:
                gb = (B * L * 4 + B * T1 * 128 * 2) / 1e9
                row["rn_conv3_front_TBps"] = round(gb / (per["rn_conv3_front"] * 1e-6) / 1e3, 2)
            res[name] = row
            print(name, json.dumps(row), flush=True)
        same = bool(np.array_equal(outs[0], outs[1]))
        print("fused == unfused bit for bit:", same, flush=True)
        eng.close()
    return res


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def throughput(steps):
    from speakerverification_amd.models import Raw_ECAPA_conv_asp, Raw_ECAPA_sinc_asp, RawNet2_custom
    wav = torch.from_numpy(synth.synth_waveforms(B, L, seed=5)).cuda()
    res = {}
    for name, make, front in (
            ("rawnet2_conv", lambda: RawNet2_custom.MainModel(nOut=320, front_proc="conv", aggregate="asp", audio_spec=AUDIO_SPEC,
                                                              hip_compute="half", embed_batch=B), "conv"),
            ("rawnet2_sinc", lambda: RawNet2_custom.MainModel(nOut=320, front_proc="sinc", aggregate="asp", audio_spec=AUDIO_SPEC,
                                                              hip_compute="half", embed_batch=B), "sinc"),
            ("Raw_ECAPA_conv_asp", lambda: Raw_ECAPA_conv_asp.MainModel(nOut=512, hip_compute="half", embed_batch=B, **KW), None),
            ("Raw_ECAPA_sinc_asp", lambda: Raw_ECAPA_sinc_asp.MainModel(nOut=512, hip_compute="half", embed_batch=B, **KW), None)):
        m = make()
        if front is not None:
            m.load_state_dict(synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, front_proc=front), seed=1))
        s = _time(lambda: m(wav), steps, 3)
        res[name] = {"ms_per_batch": round(s * 1e3, 3), "utt_per_s": round(B / s, 1)}
        print(name, json.dumps(res[name]), flush=True)
        del m
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "throughput"])
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available()
    res = kernels(a.steps) if a.mode == "kernels" else throughput(a.steps)
    print(json.dumps({"mode": a.mode, "B": B, "L": L, "results": res}))


if __name__ == "__main__":
    main()
