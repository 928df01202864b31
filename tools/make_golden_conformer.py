"""Generate the Conformer fixture (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_conformer.py     (from the repository root)

Writes ONE new file, ``tests/golden/conformer.npz``, and touches no other fixture: the reference ``Conformer.MainModel(nOut=512,
n_mels=80, features='melspectrogram')`` with ``synth``'s seeded weights (``pe`` included, so the library and the fixture use the same
buffer by construction), fp32 and float64 outputs for B = 2 utterances of different content at L = 32000 (T' = 99), 512 (T' = 1, the
shortest input the mel front-end takes), 800 (T' = 2), 41440 (T' = 129: one key tile and one frame more) and 160000 (T' = 499), the key
list, per-stage checksums at 32000, and the float64 stage values of utterance 0 at 32000 rounded to float32 (input projection, block 0's
per-head attention context, block 0's output, the last block's output, the pooled vector after attention_norm).  Outputs and seeds only.
Asserts that the spec matches the reference's keys and shapes and that every block's output is finite and non-degenerate.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle._refimport import import_reference     # noqa: E402
from oracle import fbank as o_fbank                 # noqa: E402
from speakerverification_amd import synth           # noqa: E402
from make_golden_fusion_variants import checksum, spec_of, torch_sd  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED_W, SEED_X = 1, 20220829
LENGTHS = (32000, 512, 800, 41440, 160000)
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="melspectrogram")


def mel_of(L, B=2):
    x = torch.from_numpy(synth.synth_waveforms(B, L, seed=SEED_X))
    return o_fbank.melspectrogram(x)


def main():
    import_reference()
    torch.manual_seed(0)
    from models import Conformer                     # noqa: E402  (reference module)
    model = Conformer.MainModel(nOut=512, **KW).eval()
    spec = synth.conformer_param_spec(512, 80)
    assert spec_of(model) == [(k, tuple(s)) for k, s in spec], "conformer_param_spec diverges from the reference"
    model.load_state_dict(torch_sd(synth.synth_state_dict(spec, seed=SEED_W)), strict=True)
    m64 = Conformer.MainModel(nOut=512, **KW).eval()
    m64.load_state_dict(model.state_dict())
    m64 = m64.double()
    rec = {"seed_w": SEED_W, "seed_x": SEED_X, "B": 2, "lengths": np.array(LENGTHS), "keys": np.array([k for k, _ in spec])}
    enc = m64.conformer_block
    for L in LENGTHS:
        mel = mel_of(L)
        stages, handles = {}, []
        if L == 32000:
            handles.append(enc.input_projection.register_forward_hook(lambda m, i, o: stages.__setitem__("cf_in", o)))
            for bi, blk in enumerate(enc.layers):
                handles.append(blk.register_forward_hook(lambda m, i, o, bi=bi: stages.__setitem__(f"block{bi}", o)))
            att = enc.layers[0].sequential[1].module.attention
            handles.append(att.out_proj.register_forward_hook(lambda m, i, o: stages.__setitem__("cf_attn0", i[0])))
            handles.append(m64.attention_norm.register_forward_hook(lambda m, i, o: stages.__setitem__("cf_pool", o)))
        with torch.no_grad():
            out = model(mel)
            out64 = m64(mel.double())
        for hd in handles:
            hd.remove()
        rel = float((out.double() - out64).abs().max() / out64.abs().max())
        Tp = synth.conformer_frames(mel.shape[2])
        print(f"conformer L={L} T={mel.shape[2]} T'={Tp}: |max| {float(out64.abs().max()):.3f}, fp32 vs float64 {rel:.2e} of scale")
        assert torch.isfinite(out64).all()
        rec[f"out32_L{L}"] = out.numpy().astype(np.float32)
        rec[f"out64_L{L}"] = out64.numpy()
        rec[f"mel_L{L}"] = np.array(checksum(mel))
        for name, t in stages.items():
            if name.startswith("block"):
                sd = float(t.std())
                print(f"  {name}: finite {bool(torch.isfinite(t).all())}, std {sd:.3f}, |max| {float(t.abs().max()):.2f}")
                assert torch.isfinite(t).all() and 0.3 < sd < 3.0, f"{name}: dead or exploded (std {sd:.3f})"
            rec[f"stage_{name}"] = np.array(checksum(t))
        if L == 32000:
            for name in ("cf_in", "cf_attn0", "block0", "block5", "cf_pool"):
                rec[f"val_{name}"] = stages[name][0].numpy().astype(np.float32)
    np.savez_compressed(os.path.join(GOLD, "conformer.npz"), **rec)
    print(os.path.getsize(os.path.join(GOLD, "conformer.npz")), "bytes")


if __name__ == "__main__":
    main()
