"""Generate the TitaNet / Tita_ECAPA / Raw_tita fixtures (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_titanet.py     (from the repository root)

Writes three NEW files under ``tests/golden`` and touches no other fixture:
  * ``titanet.npz``            reference ``TitaNet.get_titanet`` for sizes s (nOut 192), m (nOut 320) and l (nOut 512) with
                               find_n_mega_blocks' count: fp32 and float64 outputs for B = 2 utterances of different content at
                               L = 32000, 640 (T = 9, below the largest kernel) and 512 (T = 7, the shortest input the mel front-end
                               takes), the key lists, the find_n_mega_blocks table over s / m / l x nOut {192, 256, 320, 512} x n_mels
                               {40, 64, 80}, and per-stage checksums (prolog, every mega-block, epilog, pooled) at L = 32000;
  * ``fusion_tita_ecapa.npz``  reference ``Tita_ECAPA`` (ECAPA C = 512 with input_norm + TitaNet-M 320-d): fp32 and float64 at 32000;
  * ``fusion_raw_tita.npz``    reference ``Raw_tita`` (TitaNet-M 192-d + RawNet2 sinc / asp 320-d): fp32 and float64 at 32000.
The fusion weights are drawn per branch (each branch's own spec and seed), as the tests rebuild them.
TitaNet's input is the mel POWER of the waveform (the oracle's restatement of the nnAudio front-end with pre-emphasis, as the fusion
models' compute_features forms it).  Weights come from ``synth``'s seeds; the tests regenerate the inputs from the seeds stored beside
the outputs.  The script asserts that every mega-block output of the synthetic weights is finite and has a non-trivial fraction of
non-zeros, so that the fixtures do not pin a dead or exploded net.
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
from make_golden_fusion_variants import AUDIO_SPEC, FUSION_KW, checksum, install_oracle_mel, spec_of, torch_sd  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED_W, SEED_X = 1, 20220829
LENGTHS = (32000, 640, 512)
SIZES = (("s", 192), ("m", 320), ("l", 512))


def mel_of(L, B=2):
    x = torch.from_numpy(synth.synth_waveforms(B, L, seed=SEED_X))
    return o_fbank.melspectrogram(x)


def golden_titanet(TitaNet):
    rec = {"seed_w": SEED_W, "seed_x": SEED_X, "B": 2, "lengths": np.array(LENGTHS)}
    table = []
    for size in "sml":
        for nOut in (192, 256, 320, 512):
            for n_mels in (40, 64, 80):
                n = TitaNet.TitaNet.find_n_mega_blocks(nOut, n_mels, size)
                assert n == synth.titanet_n_mega_blocks(size, nOut, n_mels), (size, nOut, n_mels, n)
                table.append(("sml".index(size), nOut, n_mels, n))
    rec["n_blocks_table"] = np.array(table, dtype=np.int64)
    for size, nOut in SIZES:
        model = TitaNet.MainModel(nOut=nOut, model_size=size, n_mega_blocks=None, n_mels=80, device="cpu").eval()
        spec = synth.titanet_param_spec(size, nOut)
        assert spec_of(model) == [(k, tuple(s)) for k, s in spec], f"titanet_param_spec({size}) diverges from the reference"
        model.load_state_dict(torch_sd(synth.synth_state_dict(spec, seed=SEED_W)), strict=True)
        rec[f"{size}_nOut"] = nOut
        rec[f"{size}_n_blocks"] = len(model.encoder.mega_blocks)
        rec[f"{size}_keys"] = np.array([k for k, _ in spec])
        m64 = TitaNet.MainModel(nOut=nOut, model_size=size, n_mega_blocks=None, n_mels=80, device="cpu").eval()
        m64.load_state_dict(model.state_dict())
        m64 = m64.double()
        for L in LENGTHS:
            mel = mel_of(L)
            stages, handles = {}, []
            if L == 32000:
                handles.append(m64.encoder.prolog.register_forward_hook(lambda m, i, o: stages.__setitem__("prolog", o)))
                for bi, blk in enumerate(m64.encoder.mega_blocks):
                    handles.append(blk.register_forward_hook(lambda m, i, o, bi=bi: stages.__setitem__(f"block{bi}", o)))
                handles.append(m64.encoder.epilog.register_forward_hook(lambda m, i, o: stages.__setitem__("epilog", o)))
                handles.append(m64.decoder.pool.register_forward_hook(lambda m, i, o: stages.__setitem__("pool", o)))
            with torch.no_grad():
                out = model(mel)
                out64 = m64(mel.double())
            for hd in handles:
                hd.remove()
            rel = float((out.double() - out64).abs().max() / out64.abs().max())
            print(f"titanet-{size} nOut {nOut} L={L} T={mel.shape[2]}: |max| {float(out64.abs().max()):.3f}, fp32 vs float64 {rel:.2e} of scale")
            assert torch.isfinite(out64).all()
            rec[f"{size}_out32_L{L}"] = out.numpy().astype(np.float32)
            rec[f"{size}_out64_L{L}"] = out64.numpy()
            rec[f"{size}_mel_L{L}"] = np.array(checksum(mel))
            for name, t in stages.items():
                if name.startswith("block"):
                    nz = float((t != 0).double().mean())
                    print(f"  {name}: finite {bool(torch.isfinite(t).all())}, non-zero {nz:.2f}, |max| {float(t.abs().max()):.2f}")
                    assert torch.isfinite(t).all() and 0.05 < nz < 0.98, f"{size} {name}: dead or exploded ({nz:.3f} non-zero)"
                rec[f"{size}_stage_{name}"] = np.array(checksum(t))
    np.savez_compressed(os.path.join(GOLD, "titanet.npz"), **rec)


FUSION_BRANCHES = {     # each branch draws its own synthetic weights (its own init rules: the RawNet2 residual stack's gain)
    "Tita_ECAPA": (("ECAPA_TDNN.", synth.ecapa_param_spec(C=512, input_norm=True)), ("titaNet.", synth.titanet_param_spec("m", 320))),
    "Raw_tita": (("titaNet.", synth.titanet_param_spec("m", 192)), ("RawNet.", synth.rawnet2_param_spec(nOut=320))),
}


def fusion_state_dict(name, seed):
    sd = {}
    for prefix, spec in FUSION_BRANCHES[name]:
        sd.update({prefix + k: v for k, v in synth.synth_state_dict(spec, seed=seed).items()})
    return sd


def golden_fusion(mod, name, fname):
    model = mod.MainModel(nOut=512, device="cpu", **FUSION_KW).eval()
    spec = spec_of(model)
    sd = fusion_state_dict(name, SEED_W)
    assert sorted(sd) == sorted(k for k, _ in spec if not k.startswith("compute_features."))
    full = model.state_dict()
    full.update(torch_sd(sd))
    model.load_state_dict(full, strict=True)
    x = torch.from_numpy(synth.synth_waveforms(2, 32000, seed=SEED_X))
    with torch.no_grad():
        out = model(x)
        model.double()
        for m in model.modules():          # plain tensor attributes (the sinc layer's n_ / window_) are not converted by .double()
            for k, v in list(vars(m).items()):
                if torch.is_tensor(v) and v.dtype == torch.float32:
                    setattr(m, k, v.double())
        out64 = model(x.double())
    rel = float((out.double() - out64).abs().max() / out64.abs().max())
    print(f"{name}: {len(spec)} tensors, out {tuple(out.shape)}, |max| {float(out64.abs().max()):.3f}, fp32 vs float64 {rel:.2e} of scale")
    np.savez_compressed(os.path.join(GOLD, fname), seed_w=SEED_W, seed_x=SEED_X, B=2, L=32000,
                        keys=np.array([k for k, _ in spec]), out32=out.numpy().astype(np.float32), out64=out64.numpy())


def main():
    import_reference()
    install_oracle_mel()
    torch.manual_seed(0)
    from models import TitaNet, Tita_ECAPA, Raw_tita          # noqa: E402  (reference modules)
    golden_titanet(TitaNet)
    golden_fusion(Tita_ECAPA, "Tita_ECAPA", "fusion_tita_ecapa.npz")
    golden_fusion(Raw_tita, "Raw_tita", "fusion_raw_tita.npz")


if __name__ == "__main__":
    main()
