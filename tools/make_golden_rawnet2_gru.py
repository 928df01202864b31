"""Generate the fixtures of RawNet2's GRU aggregation and the Raw_ECAPA_sinc_gru fusion model (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_rawnet2_gru.py     (from the repository root)

Writes two NEW files under ``tests/golden`` and touches no other fixture:
  * ``rawnet2_gru.npz``                 reference ``RawNet2_custom.MainModel(nOut=320, front_proc='sinc', aggregate='gru')``: outputs
                                        at L = 2438, 32000 and 96000 (T = 1, 14, 43 frames reach the GRU), the GRU input
                                        lrelu(bn_before_gru(x)) and the last state h_T at L = 32000, the key list;
  * ``fusion_raw_ecapa_sinc_gru.npz``   reference ``Raw_ECAPA_sinc_gru`` (ECAPA C = 512 without input_norm + RawNet2 sinc / gru).
The recipe is tools/make_golden_fusion_variants.py's: the reference runs on CPU in fp32 on ``synth``'s deterministic weights
(one state dict per length: LayerNorm(nb_samp) fixes it), the nnAudio mel front-end is stood in for by the oracle's
restatement, and the tests regenerate the inputs from the seeds stored beside the outputs.
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_golden_fusion_variants import AUDIO_SPEC, FUSION_KW, install_oracle_mel, spec_of, torch_sd  # noqa: E402
from oracle._refimport import import_reference  # noqa: E402
from speakerverification_amd import synth     # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED_W, SEED_X = 1, 20220829
LENGTHS = (2438, 32000, 96000)                 # the sinc minimum (T = 1), the 2 s crop (T = 14), a 6 s crop (T = 43)


def audio_spec(L):
    return dict(AUDIO_SPEC, sentence_len=L / 16000.0)


def golden_rawnet2_gru(ref):
    rec = {"seed_w": SEED_W, "seed_x": SEED_X, "B": 2, "lengths": np.array(LENGTHS)}
    for L in LENGTHS:
        model = ref.RawNet2_custom.MainModel(nOut=320, audio_spec=audio_spec(L)).eval()      # the defaults: front_proc='sinc', aggregate='gru'
        assert model.aggregate == "gru" and model.front_proc == "sinc"
        spec = synth.rawnet2_param_spec(nOut=320, nb_samp=L, aggregate="gru")
        ref_spec = spec_of(model)
        assert ref_spec == [(k, tuple(s)) for k, s in spec], "rawnet2_param_spec(aggregate='gru') diverges from the reference"
        model.load_state_dict(torch_sd(synth.synth_state_dict(spec, seed=SEED_W)), strict=True)
        if L == 32000:
            rec["keys"] = np.array([k for k, _ in ref_spec])
        seen = {}
        hk = model.gru.register_forward_hook(lambda m, i, o: seen.update(x=i[0].detach(), h=o[0][:, -1].detach()))
        x = torch.from_numpy(synth.synth_waveforms(2, L, seed=SEED_X))
        with torch.no_grad():
            out = model(x)
        hk.remove()
        rec[f"out_{L}"] = out.numpy()
        rec[f"T_{L}"] = int(seen["x"].shape[1])
        if L == 32000:
            rec["gru_in"] = seen["x"].numpy()            # (B, T, 512)
            rec["h_T"] = seen["h"].numpy()               # (B, 1024)
        print(f"rawnet2 gru L={L}: T={seen['x'].shape[1]} out {tuple(out.shape)} |max| {float(out.abs().max()):.3f}")
    np.savez_compressed(os.path.join(GOLD, "rawnet2_gru.npz"), **rec)


def golden_fusion_sinc_gru(ref):
    fus = importlib.import_module("models.Raw_ECAPA_sinc_gru")          # reference module
    model = fus.MainModel(nOut=512, **FUSION_KW).eval()
    spec_e = synth.ecapa_param_spec(C=512, input_norm=False)
    spec_r = synth.rawnet2_param_spec(nOut=320, aggregate="gru")
    assert spec_of(model.ECAPA_TDNN) == [(k, tuple(s)) for k, s in spec_e]
    assert spec_of(model.rawnet2v2) == [(k, tuple(s)) for k, s in spec_r]
    model.ECAPA_TDNN.load_state_dict(torch_sd(synth.synth_state_dict(spec_e, seed=1)), strict=True)
    model.rawnet2v2.load_state_dict(torch_sd(synth.synth_state_dict(spec_r, seed=SEED_W)), strict=True)
    keys = list(model.state_dict().keys())
    rec = {"seed_w_ecapa": 1, "seed_w_rawnet2": SEED_W, "seed_x": SEED_X, "B": 2, "lengths": np.array([32000]), "keys": np.array(keys)}
    x = torch.from_numpy(synth.synth_waveforms(2, 32000, seed=SEED_X))
    with torch.no_grad():
        out = model(x)
    rec["out_32000"] = out.numpy()
    print(f"Raw_ECAPA_sinc_gru L=32000: {len(keys)} keys, out {tuple(out.shape)} |max| {float(out.abs().max()):.3f}")
    np.savez_compressed(os.path.join(GOLD, "fusion_raw_ecapa_sinc_gru.npz"), **rec)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref = import_reference()
    install_oracle_mel()
    golden_rawnet2_gru(ref)
    golden_fusion_sinc_gru(ref)


if __name__ == "__main__":
    main()
