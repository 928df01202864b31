"""Whole-file evaluation (num_eval = 0) on the MI355X: files/s of `ModelHandling._embed_files` over seeded files of 2 - 20 s.

    python tools/ragged_bench.py [--model ECAPA_TDNN|RawNet3|Raw3_ECAPA|Conformer|TitaNet|Tita_ECAPA|RawNet2_conv|Raw_ECAPA_conv_asp|ResNetSE34V2] [--per-file] [--files 512] [--runs 5] [--compute bf16,f32]
                                 [--out profiles/ragged_bench.json]

Default mode: the ragged path of this tree (files of different lengths share calls of the model's primary handle), plus, without a
bar, the frames/s of the ragged call relative to the fixed-length B = 256 call of the same handle and the library's per-label event
times of the ragged forward (which ragged kernel to fuse first).
--per-file: one forward per file on a handle of that file's length — `ragged_eval=False` where the tree knows the keyword, and the
only path of a tree that does not: the mode uses nothing newer than `_embed_files` and is meant to be run against a checkout of the
parent commit (put that checkout first on PYTHONPATH), whose files/s are the yardstick.

Own process; every figure is the median of `--runs` timed passes over the whole file list (after one untimed pass), with the spread
(min, max); wall time and HIP-event time around the whole pass are both given.  ECAPA-TDNN C = 1024, nOut 192; with --model RawNet3
(nOut 320) or Raw3_ECAPA (nOut 512, the model of the reference's default configs: ECAPA-TDNN C = 512 + RawNet3), `features: raw`,
written to profiles/rawnet3_ragged_bench.json by convention; --model Conformer (nOut 512, the model of yaml/model_plot.yaml, mel features)
to profiles/conformer_ragged_bench.json; --model TitaNet (TitaNet-M, nOut 320, mel features) and --model Tita_ECAPA (nOut 512: ECAPA-TDNN
C = 512 + TitaNet-M, `features: raw`) to profiles/titanet_ragged_bench.json (one record per run: --out names the file).  The single-call
comparison and the kernel table are given for ECAPA-TDNN, the Conformer and TitaNet; for TitaNet also the packed depthwise kernels
(tn_dw, tn_mega_tail) beside the fixed ones over the same rows in the same process, in algorithmic bytes per second.  --model
RawNet2_conv (RawNet2 with front_proc='conv', nOut 320) and --model Raw_ECAPA_conv_asp (nOut 512: ECAPA-TDNN C = 512 + RawNet2 'conv',
`features: raw`; --compute f32,bf16,f16 or half) go to profiles/rawnet2_ragged_bench.json; for RawNet2_conv also the packed block tail
(rn_rag_tail_part + rn_rag_gate + rn_rag_tail_apply) per block beside the fixed sliced tail (rn_tail at B * 4 <= CUs) of the blocks where
the fixed forward takes it, from the library's per-label event times of both forwards in the same process, in algorithmic bytes per
second.  --model ResNetSE34V2 (nOut 256, mel features) goes to profiles/resnetse_ragged_bench.json; it has the single-call comparison and the
kernel table too, and the packed rs_conv beside the fixed one per stage, in TFLOP/s, over the same rows in the same process: as many
401-frame utterances as a pack of the handle holds (251 of max_batch = 256: a pack counts an utterance as 408 rows) against the
fixed-length call at that batch size, from the library's per-label event times."""
from __future__ import annotations

import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

if not os.environ.get("RAGGED_BENCH_NO_PATH"):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch             # noqa: E402

from speakerverification_amd import _lib, synth                                                # noqa: E402
from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel      # noqa: E402

SEED = 20220829
ARGS = dict(
    device="cuda", gpu=0, model={"name": "ECAPA_TDNN", "nOut": 192}, criterion={"name": "AAmSoftmaxAP"}, features="melspectrogram",
    include_top=False, n_mels=80, channels=[1024] * 4 + [3072],
    audio_spec={"sample_rate": 16000, "channels": 1, "sentence_len": 2.0, "win_len": 0.025, "hop_len": 0.01},
    augment=False, augment_options={"augment_chain": []},
)


def make_files(n):
    """n seeded waveforms of 2 - 20 s at 16 kHz (401 - 4001 frames), every length distinct from its neighbours"""
    rng = np.random.Generator(np.random.PCG64(SEED))
    lens = rng.integers(32000, 320001, size=n)
    return [np.clip(0.1 * rng.standard_normal(int(L), dtype=np.float32), -1.0, 1.0) for L in lens]


MODELS = {"ECAPA_TDNN": "ECAPA_TDNN C=1024 nOut=192", "RawNet3": "RawNet3 nOut=320", "Raw3_ECAPA": "Raw3_ECAPA nOut=512 (ECAPA-TDNN C=512 + RawNet3)",
          "Conformer": "Conformer nOut=512", "TitaNet": "TitaNet-M nOut=320",
          "Tita_ECAPA": "Tita_ECAPA nOut=512 (ECAPA-TDNN C=512 + TitaNet-M)", "RawNet2_conv": "RawNet2 front_proc='conv' nOut=320",
          "Raw_ECAPA_conv_asp": "Raw_ECAPA_conv_asp nOut=512 (ECAPA-TDNN C=512 + RawNet2 'conv')", "ResNetSE34V2": "ResNetSE34V2 nOut=256"}


def state_dict(model):
    if model == "ECAPA_TDNN":
        return synth.synth_state_dict(synth.ecapa_param_spec(C=1024), seed=5)
    if model == "Conformer":
        return synth.synth_state_dict(synth.conformer_param_spec(512, 80), seed=5)
    if model == "TitaNet":
        return synth.synth_state_dict(synth.titanet_param_spec("m", 320), seed=5)
    if model == "ResNetSE34V2":
        return synth.synth_state_dict(synth.resnetse_param_spec(256, 80, "ASP"), seed=5)
    if model == "Tita_ECAPA":
        sd = {"ECAPA_TDNN." + k: v for k, v in synth.synth_state_dict(synth.ecapa_param_spec(C=512, input_norm=True), seed=5).items()}
        sd.update({"titaNet." + k: v for k, v in synth.synth_state_dict(synth.titanet_param_spec("m", 320), seed=5).items()})
        return sd
    if model in ("RawNet2_conv", "Raw_ECAPA_conv_asp"):
        rn2 = synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, front_proc="conv"), seed=5)
        if model == "RawNet2_conv":
            return rn2
        sd = {"ECAPA_TDNN." + k: v for k, v in synth.synth_state_dict(synth.ecapa_param_spec(C=512, input_norm=True), seed=5).items()}
        sd.update({"rawnet2v2." + k: v for k, v in rn2.items()})
        return sd
    rn3 = synth.synth_state_dict(synth.rawnet3_param_spec(nOut=320), seed=5)
    if model == "RawNet3":
        return rn3
    sd = {"ECAPA_TDNN." + k: v for k, v in synth.synth_state_dict(synth.ecapa_param_spec(C=512, input_norm=True), seed=5).items()}
    sd.update({"rawnet." + k: v for k, v in rn3.items()})
    return sd


def handler(compute, per_file, model="ECAPA_TDNN"):
    kw = dict(ARGS, hip_compute=compute)
    if model == "Conformer":
        kw.update(model={"name": model, "nOut": 512})
        kw.pop("channels")
    elif model == "TitaNet":
        kw.update(model={"name": model, "nOut": 320}, model_size="m")
        kw.pop("channels")
    elif model == "ResNetSE34V2":
        kw.update(model={"name": model, "nOut": 256})
        kw.pop("channels")
    elif model == "RawNet2_conv":
        kw.update(model={"name": "RawNet2_custom", "nOut": 320}, features="raw", front_proc="conv", aggregate="asp", att_dim=128)
        kw.pop("channels")
    elif model != "ECAPA_TDNN":
        kw.update(model={"name": model, "nOut": 320 if model == "RawNet3" else 512}, features="raw")
        kw.pop("channels")
    net = WrappedModel(SpeakerEncoder(**kw))
    extra = {}
    if per_file and "ragged_eval" in inspect.getsource(ModelHandling.__init__):
        extra["ragged_eval"] = False
    mh = ModelHandling(net, **dict(kw, save_folder=".", device_feats=False, **extra))
    net.module.load_state_dict({"__S__." + k: v for k, v in state_dict(model).items()})
    return mh, getattr(net.module, "__S__")


def engines_alive(S):
    """handles the model keeps alive: of the module itself, or of each branch of a fusion model"""
    if hasattr(S, "_engines"):
        return len(S._engines)
    return {a: len(getattr(S, a)._engines) for a in (S.FIRST_ATTR, S.RAW_ATTR)}


def drop_engines(S):
    for m in ([S] if hasattr(S, "_drop_engine") else [getattr(S, S.FIRST_ATTR), getattr(S, S.RAW_ATTR)]):
        m._drop_engine()


def titanet_depthwise_rates(lens, H=512, k=7, compute="bf16", iters=20):
    """TitaNet's two depthwise kernels over the pack `lens` (mel frames per utterance) through svhip_titanet_depthwise_ragged, beside the
    fixed kernels (svhip_titanet_depthwise) over B x 401 frames with B = rows // 401 — the same rows but for the last < 401 — on the same
    buffers: microseconds per launch (HIP events around `iters` launches) and algorithmic bytes per second (tn_dw: the input read once
    and the output written once; tn_mega_tail with the next depthwise conv: skip and h3 read, y and d written)"""
    lib = _lib.load()
    dtype, code, esz = (torch.bfloat16, _lib.BF16, 2) if compute == "bf16" else (torch.float32, _lib.F32, 4)
    n, M = len(lens), int(sum(lens))
    B = M // 401
    row0 = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")
    x, skip, h3, y, d = (torch.randn((M, H), device="cuda").to(dtype) for _ in range(5))
    gate = torch.rand((max(n, B), H), device="cuda")
    w, bias = torch.randn((k, H), device="cuda"), torch.randn(H, device="cuda")
    P = lambda t: t.data_ptr()
    forms = {
        "tn_dw": (2, lambda rag: lib.svhip_titanet_depthwise_ragged(P(x), None, None, None, None, P(w), P(bias), P(d), code, k, P(row0), n, max(lens), H, None)
                  if rag else lib.svhip_titanet_depthwise(P(x), None, None, None, None, P(w), P(bias), P(d), code, k, B, 401, H, None)),
        "tn_mega_tail": (4, lambda rag: lib.svhip_titanet_depthwise_ragged(None, P(skip), P(h3), P(gate), P(y), P(w), P(bias), P(d), code, k, P(row0), n,
                                                                           max(lens), H, None)
                         if rag else lib.svhip_titanet_depthwise(None, P(skip), P(h3), P(gate), P(y), P(w), P(bias), P(d), code, k, B, 401, H, None)),
    }
    out = {"rows_packed": M, "rows_fixed": B * 401, "utterances": n, "H": H, "k": k, "compute": compute}
    for name, (tensors, call) in forms.items():
        for rag in (False, True):
            rows = M if rag else B * 401
            us = []
            for _ in range(5):
                assert call(rag) == 0
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    call(rag)
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / iters)
            med = float(np.median(us))
            out[name + ("_packed" if rag else "_fixed")] = {"us_per_launch": stats(us), "TBps": round(tensors * rows * H * esz / (med * 1e-6) / 1e12, 3)}
    return out


RN2_BLOCKS = ((128, True), (128, True), (256, True), (256, False), (256, True), (512, True), (512, False), (512, True))      # (cout, pooled)


def rawnet2_tail_rates(eng, pack, offs, lens, esz):
    """RawNet2's block tail per block over the pack `lens` (samples per utterance): the three packed launches of a block, summed, beside
    the fixed sliced tail (label rn_tail, a batch of B <= 64 primary-length utterances with about the pack's rows) where the fixed
    forward takes it — milliseconds from the library's per-label events (option layer_labels: one label per block) and algorithmic
    bytes per second: the block output read twice, the next pre-activation written once, and x where the next block reads it"""
    def prof(call):
        eng.set_option("layer_labels", 1)
        eng.profile(True)
        call()
        p = eng.profile_results()
        eng.profile(False)
        eng.set_option("layer_labels", 0)
        return p
    T1s = [n // 3 for n in lens]
    B = max(1, min(64, eng.max_batch, sum(T1s) // (eng.samples // 3)))
    x = torch.from_numpy(synth.synth_waveforms(B, eng.samples, seed=1)).cuda()
    p_rag = prof(lambda: eng.embed_wave_ragged(pack, offsets=offs, lengths=lens))
    p_fix = prof(lambda: eng.embed_wave(x))
    out = {"utterances": len(lens), "rows_packed": int(sum(T1s)), "fixed_B": B, "rows_fixed": B * (eng.samples // 3), "blocks": []}
    Tu, Tf = list(T1s), eng.samples // 3
    for i, (C, down) in enumerate(RN2_BLOCKS):
        m_in, f_in = sum(Tu), B * Tf
        if down:
            Tu, Tf = [t // 3 for t in Tu], Tf // 3
        writes = 1 if i == 7 or RN2_BLOCKS[i + 1][0] != C else 2
        ms_r = sum(v["ms"] for k, v in p_rag.items() if k.startswith("rn_rag_") and k.endswith(f" M{m_in} C{C}"))
        row = {"block": i, "C": C, "packed_ms": round(ms_r, 4),
               "packed_TBps": round((2 * m_in + writes * sum(Tu)) * C * esz / (ms_r * 1e-3) / 1e12, 3) if ms_r else None}
        fix = [v for k, v in p_fix.items() if k == f"rn_tail T{f_in // B} C{C}"]
        if fix:
            ms_f = sum(v["ms"] for v in fix)
            row.update(fixed_ms=round(ms_f, 4), fixed_TBps=round((2 * f_in + writes * B * Tf) * C * esz / (ms_f * 1e-3) / 1e12, 3))
        out["blocks"].append(row)
    return out


def resnetse_conv_rates(eng, runs=3):
    """rs_conv per stage, packed beside fixed, over the same rows in the same process: n utterances of the handle's own length (as many
    as one pack holds: an utterance counts as its frames rounded up to a multiple of 8) as a features pack against the fixed-length call
    at B = n.  Both forwards label their convolutions rs_conv3x3_s1 .. s4 and rs_down; ms and FLOP from the library's per-label events,
    the median of `runs` profiled forwards each"""
    T = eng.frames
    n = min(eng.max_batch, eng.row_capacity // (8 * -(-T // 8)))
    x = (torch.randn((n, eng.n_mels, T), device="cuda") ** 2 + 1e-3).contiguous()
    offs, lens = np.arange(n, dtype=np.int64) * T, np.full(n, T, np.int32)
    forms = {"fixed": lambda: eng.embed_features(x), "packed": lambda: eng.embed_features_ragged(x.reshape(-1), offsets=offs, lengths=lens)}
    out = {"utterances": n, "frames_each": T, "stages": {}}
    for form, call in forms.items():
        call()
        seen = []
        for _ in range(runs):
            eng.profile(True)
            call()
            seen.append(eng.profile_results())
            eng.profile(False)
        for label in ("rs_conv3x3_s1", "rs_conv3x3_s2", "rs_conv3x3_s3", "rs_conv3x3_s4", "rs_down"):
            ms = [p[label]["ms"] for p in seen]
            med = float(np.median(ms))
            out["stages"].setdefault(label, {})[form] = {"ms": stats(ms), "launches": seen[0][label]["launches"],
                                                        "TFLOPs": round(seen[0][label]["flops"] / (med * 1e-3) / 1e12, 2)}
    return out


def timed(fn, runs):
    fn()                                                        # untimed: handles, allocations, first launches
    wall, dev = [], []
    for _ in range(runs):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        dev.append(e0.elapsed_time(e1) * 1e-3)
    return wall, dev


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ECAPA_TDNN", choices=sorted(MODELS))
    ap.add_argument("--per-file", action="store_true")
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--compute", default="bf16,f32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    files = make_files(a.files)
    frames = int(sum(len(f) // 80 + 1 for f in files))
    res = {"mode": "per_file" if a.per_file else "ragged", "files": a.files, "frames": frames, "runs": a.runs, "model": MODELS[a.model],
           "device": torch.cuda.get_device_name(0), "tree_has_ragged_calls": hasattr(ModelHandling, "_ragged_ok")}
    for compute in a.compute.split(","):
        mh, S = handler(compute, a.per_file, a.model)
        wall, dev = timed(lambda: mh._embed_files(files, 0), a.runs)
        r = {"wall_s": stats(wall), "hip_event_s": stats(dev),
             "files_per_s": {"median": a.files / float(np.median(wall)), "min": a.files / max(wall), "max": a.files / min(wall)},
             "frames_per_s": frames / float(np.median(wall)), "engines_alive": engines_alive(S)}
        if not a.per_file and a.model == "RawNet2_conv":
            eng = S.ragged_engine()
            pack = [torch.from_numpy(f).cuda() for f in files[:40]]
            while sum(len(p) // 3 for p in pack) > eng.row_capacity or len(pack) > eng.max_batch:
                pack.pop()
            lens = [len(p) for p in pack]
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
            packed = torch.cat(pack)
            x = torch.from_numpy(synth.synth_waveforms(eng.max_batch, eng.samples, seed=1)).cuda()
            w_fix, _ = timed(lambda: eng.embed_wave(x), a.runs)
            w_rag, _ = timed(lambda: eng.embed_wave_ragged(packed, offsets=offs, lengths=lens), a.runs)
            r["fixed_B256_frames_per_s"] = eng.max_batch * (eng.samples // 3) / float(np.median(w_fix))
            r["ragged_call_frames_per_s"] = sum(n // 3 for n in lens) / float(np.median(w_rag))
            r["ragged_over_fixed"] = r["ragged_call_frames_per_s"] / r["fixed_B256_frames_per_s"]
            eng.profile(True)
            eng.embed_wave_ragged(packed, offsets=offs, lengths=lens)
            prof = eng.profile_results()
            eng.profile(False)
            r["ragged_forward_kernels_ms"] = {k: {"ms": round(v["ms"], 4), "launches": v["launches"]}
                                              for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])}
            r["block_tail"] = rawnet2_tail_rates(eng, packed, offs, lens, 4 if compute in ("f32", "fp32") else 2)
        if not a.per_file and a.model in ("ECAPA_TDNN", "Conformer", "TitaNet", "ResNetSE34V2"):
            eng = S.ragged_engine()
            # the ragged call against the fixed-length call of the same handle, device-resident input, frames/s of each
            x = torch.from_numpy(synth.synth_waveforms(eng.max_batch, eng.samples, seed=1)).cuda()
            pack = [torch.from_numpy(f).cuda() for f in files[:40]]
            rows_of = (lambda p: 8 * -(-(len(p) // 80 + 1) // 8)) if a.model == "ResNetSE34V2" else (lambda p: len(p) // 80 + 1)      # as a pack counts them
            while sum(rows_of(p) for p in pack) > eng.row_capacity:
                pack.pop()
            packed = torch.cat(pack)
            lens = [len(p) for p in pack]
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
            w_fix, _ = timed(lambda: eng.embed_wave(x), a.runs)
            w_rag, _ = timed(lambda: eng.embed_wave_ragged(packed, offsets=offs, lengths=lens), a.runs)
            f_fix = eng.max_batch * eng.frames / float(np.median(w_fix))
            f_rag = sum(n // 80 + 1 for n in lens) / float(np.median(w_rag))
            r["fixed_B256_frames_per_s"] = f_fix
            r["ragged_call_frames_per_s"] = f_rag
            r["ragged_over_fixed"] = f_rag / f_fix
            eng.profile(True)
            eng.embed_wave_ragged(packed, offsets=offs, lengths=lens)
            prof = eng.profile_results()
            eng.profile(False)
            r["ragged_forward_kernels_ms"] = {k: {"ms": round(v["ms"], 4), "launches": v["launches"]}
                                              for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])}
            r["ragged_forward_pack"] = {"utterances": len(lens), "frames": int(sum(n // 80 + 1 for n in lens))}
            if a.model == "TitaNet":
                r["depthwise_kernels"] = titanet_depthwise_rates([n // 80 + 1 for n in lens], compute=compute)
            if a.model == "ResNetSE34V2":
                r["rs_conv_packed_beside_fixed"] = resnetse_conv_rates(eng)
        res[compute] = r
        print(compute, json.dumps(r["files_per_s"]), flush=True)
        drop_engines(S)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
