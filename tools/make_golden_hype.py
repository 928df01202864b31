"""Generate the fixtures of the 8 kHz sinc front-end and of the Raw_ECAPA_hype fusion model (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_hype.py     (from the repository root)

Writes two NEW files under ``tests/golden`` and touches no other fixture:
  * ``rawnet2_sr8000.npz``          reference ``RawNet2_custom.MainModel(front_proc='sinc', audio_spec sample_rate 8000)`` with
                                    ``aggregate='asp'`` (nOut 320) and ``'gru'`` (nOut 512): outputs at 8000 samples (1.0 s, 3 GRU
                                    steps), 16000 (2.0 s) and 2438 (one frame reaches the aggregation) on weights whose band edges
                                    start where the reference starts them at 8 kHz, and one more case ("clamp") on the 16 kHz
                                    band edges, several of which meet the clamp at sample_rate / 2;
  * ``fusion_raw_ecapa_hype.npz``   reference ``Raw_ECAPA_hype.MainModel(nOut=512, features='raw')`` at 8 kHz x 2.0 s (the saved
                                    config), 8 kHz x 1.0 s (yaml/verification.yaml) and 16 kHz x 2.0 s: the output, the two branch
                                    outputs (forward hooks), the key list.
The recipe is tools/make_golden_fusion_variants.py's: the reference runs on CPU in fp32 on ``synth``'s deterministic weights (one
state dict per length: LayerNorm(nb_samp) fixes it), the nnAudio mel front-end is stood in for by the oracle's restatement, and
the tests regenerate inputs and weights from the seeds stored beside the outputs.
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
SEED_W, SEED_HEAD, SEED_X = 1, 3, 20220829
SR8K_LENGTHS = (8000, 16000, 2438)
SR8K_MODELS = (("asp", 320), ("gru", 512))
HYPE_CASES = ((8000, 16000), (8000, 8000), (16000, 32000))        # (sample rate, samples)


def audio_spec(sr, L):
    return dict(AUDIO_SPEC, sample_rate=sr, sentence_len=L / float(sr))


def clamped_filters(sd, sr):
    """how many filters of a state dict meet the clamp high <= sr / 2 (RawNet_baseline.py:339-341), and how many start above it"""
    low = 50.0 + np.abs(sd["first_conv.low_hz_"][:, 0])
    high = low + 50.0 + np.abs(sd["first_conv.band_hz_"][:, 0])
    return int((high > sr / 2).sum()), int((low > sr / 2).sum())


def golden_rawnet2_sr8000(ref):
    rec = {"seed_w": SEED_W, "seed_x": SEED_X, "B": 2, "sample_rate": 8000, "lengths": np.array(SR8K_LENGTHS),
           "aggregates": np.array([a for a, _ in SR8K_MODELS]), "nOuts": np.array([n for _, n in SR8K_MODELS])}

    def run(agg, nOut, L, weights_sr):
        model = ref.RawNet2_custom.MainModel(nOut=nOut, front_proc="sinc", aggregate=agg, att_dim=128, audio_spec=audio_spec(8000, L)).eval()
        assert model.first_conv.sample_rate == 8000
        spec = synth.rawnet2_param_spec(nOut=nOut, nb_samp=L, aggregate=agg)
        assert spec_of(model) == [(k, tuple(s)) for k, s in spec], "rawnet2_param_spec diverges from the reference"
        sd = synth.synth_state_dict(spec, seed=SEED_W, sample_rate=weights_sr)
        model.load_state_dict(torch_sd(sd), strict=True)
        with torch.no_grad():
            out = model(torch.from_numpy(synth.synth_waveforms(2, L, seed=SEED_X)))
        return out.numpy(), sd

    for agg, nOut in SR8K_MODELS:
        for L in SR8K_LENGTHS:
            out, sd = run(agg, nOut, L, 8000)
            assert np.isfinite(out).all()
            rec[f"out_{agg}_{L}"] = out
            # (the reference starts the top filter's upper edge AT sample_rate / 2: with synth's jitter it may just meet the clamp)
            print(f"rawnet2 8 kHz {agg} L={L}: out {out.shape} |max| {np.abs(out).max():.3f}, filters (clamped, above) {clamped_filters(sd, 8000)}")
    # the 16 kHz band edges on the 8 kHz model: the upper edges of the top filters meet the clamp, some filters start above it
    out, sd = run("asp", 320, 16000, 16000)
    n_clamp, n_above = clamped_filters(sd, 8000)
    print(f"rawnet2 8 kHz clamp case: {n_clamp} filters clamp at 4000 Hz, {n_above} have low > 4000 Hz; finite: {bool(np.isfinite(out).all())}")
    assert n_clamp >= 8, n_clamp
    if np.isfinite(out).all():
        rec["out_clamp"] = out
        rec["clamp_filters"] = np.array([n_clamp, n_above])
    else:
        print("the reference's output is not finite: the clamp case is DROPPED")
    np.savez_compressed(os.path.join(GOLD, "rawnet2_sr8000.npz"), **rec)


def golden_hype(ref):
    fus = importlib.import_module("models.Raw_ECAPA_hype")            # reference module
    spec_e = synth.ecapa_param_spec(C=512, input_norm=True)
    spec_h = synth.hype_head_param_spec(512)
    rec = {"seed_w_ecapa": 1, "seed_w_rawnet2": SEED_W, "seed_w_head": SEED_HEAD, "seed_x": SEED_X, "B": 2,
           "sample_rates": np.array([sr for sr, _ in HYPE_CASES]), "lengths": np.array([L for _, L in HYPE_CASES])}
    for sr, L in HYPE_CASES:
        model = fus.MainModel(nOut=512, **dict(FUSION_KW, audio_spec=audio_spec(sr, L))).eval()
        spec_r = synth.rawnet2_param_spec(nOut=512, nb_samp=L, aggregate="gru")
        assert spec_of(model.ECAPA_TDNN) == [(k, tuple(s)) for k, s in spec_e]
        assert spec_of(model.rawnet2v2) == [(k, tuple(s)) for k, s in spec_r]
        top = [(k, s) for k, s in spec_of(model) if not k.startswith(("ECAPA_TDNN.", "rawnet2v2.", "compute_features."))]
        assert top == [(k, tuple(s)) for k, s in spec_h], "hype_head_param_spec diverges from the reference"
        model.ECAPA_TDNN.load_state_dict(torch_sd(synth.synth_state_dict(spec_e, seed=1)), strict=True)
        model.rawnet2v2.load_state_dict(torch_sd(synth.synth_state_dict(spec_r, seed=SEED_W, sample_rate=sr)), strict=True)
        res = model.load_state_dict(torch_sd(synth.synth_state_dict(spec_h, seed=SEED_HEAD)), strict=False)
        assert not res.unexpected_keys and all(k.startswith(("ECAPA_TDNN.", "rawnet2v2.", "compute_features.")) for k in res.missing_keys)
        seen = {}
        hooks = [model.ECAPA_TDNN.register_forward_hook(lambda m, i, o: seen.update(out1=o.detach())),
                 model.rawnet2v2.register_forward_hook(lambda m, i, o: seen.update(out2=o.detach()))]
        with torch.no_grad():
            out = model(torch.from_numpy(synth.synth_waveforms(2, L, seed=SEED_X)))
        for hk in hooks:
            hk.remove()
        assert tuple(seen["out1"].shape) == (2, 192) and tuple(seen["out2"].shape) == (2, 512) and bool(torch.isfinite(out).all())
        rec[f"out_{L}"], rec[f"out1_{L}"], rec[f"out2_{L}"] = out.numpy(), seen["out1"].numpy(), seen["out2"].numpy()
        if "keys" not in rec:
            rec["keys"] = np.array(list(model.state_dict().keys()))
        print(f"Raw_ECAPA_hype sr={sr} L={L}: {len(model.state_dict())} keys, out {tuple(out.shape)} |max| {float(out.abs().max()):.3f}, "
              f"|out1| {float(seen['out1'].abs().max()):.3f}, |out2| {float(seen['out2'].abs().max()):.3f}")
    np.savez_compressed(os.path.join(GOLD, "fusion_raw_ecapa_hype.npz"), **rec)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref = import_reference()
    install_oracle_mel()
    golden_rawnet2_sr8000(ref)
    golden_hype(ref)


if __name__ == "__main__":
    main()
