"""GPU parity of RawNet2's 'conv' front-end and the two fusion models the reference configs name (Raw_ECAPA_conv_asp,
Raw_ECAPA) against the outputs of the REFERENCE's own modules (tests/golden/rawnet2_conv.npz, fusion_raw_ecapa_conv.npz,
fusion_raw_ecapa_in.npz; tools/make_golden_fusion_variants.py), and the bit-identity of block 0 reading the waveform itself
(rn_block128's CONV form) against rn_conv3_front + the plain block (option rn_conv_unfused)."""
import os

import numpy as np
import pytest

from speakerverification_amd import synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.models import Raw_ECAPA, Raw_ECAPA_conv_asp, RawNet2_custom

pytestmark = pytest.mark.gpu

AUDIO_SPEC = dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1)
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw", audio_spec=AUDIO_SPEC)
BARS_16 = {"f16": (0.999, 0.03), "bf16": (0.99, 0.15)}          # the bars of tests/test_gpu_rawnet2.py: (min cosine, max error / scale)


def _cos(a, b):
    return np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def _check(out, ref, compute, tag):
    out = np.atleast_2d(out)
    assert out.shape == ref.shape and np.isfinite(out).all()
    scale = float(np.abs(ref).max())
    rel = float(np.abs(out - ref).max()) / scale
    cos = _cos(out, ref)
    print(f"{tag} {compute}: max|d| / scale {rel:.2e}, min cos {cos.min():.7f}")
    if compute in BARS_16:
        c_min, r_max = BARS_16[compute]
        assert rel <= r_max and float(cos.min()) >= c_min, (rel, cos)
    else:
        assert rel <= 1e-4, rel
        nrm = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
        assert float(np.abs(nrm(out) - nrm(ref)).max()) <= 1e-4


def _conv_sd(seed):
    return synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, front_proc="conv"), seed=seed)


def _fusion_sd(g, front):
    sd = {"ECAPA_TDNN." + k: v for k, v in
          synth.synth_state_dict(synth.ecapa_param_spec(C=512, input_norm=True), seed=int(g["seed_w_ecapa"])).items()}
    sd.update({"rawnet2v2." + k: v for k, v in
               synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, front_proc=front), seed=int(g["seed_w_rawnet2"])).items()})
    sd["compute_features.0.flipped_filter"] = np.array([[[-0.97, 1.0]]], np.float32)     # reference checkpoints carry it
    return sd


@pytest.mark.parametrize("compute", ["f32", "f32x3", "f16", "bf16"])
def test_rawnet2_conv_matches_reference_at_every_length(golden_dir, compute):
    g = np.load(os.path.join(golden_dir, "rawnet2_conv.npz"))
    m = RawNet2_custom.MainModel(nOut=320, front_proc="conv", aggregate="asp", att_dim=128, audio_spec=AUDIO_SPEC,
                                 hip_compute=compute, range_fallback=None, embed_batch=8)
    m.load_state_dict(_conv_sd(int(g["seed_w"])))
    for L in g["lengths"]:
        x = synth.synth_waveforms(int(g["B"]), int(L), seed=int(g["seed_x"]))
        _check(m(x), g[f"out_{int(L)}"], compute, f"rawnet2 conv L={int(L)}")
    assert len(m._engines) <= m.ENGINE_CACHE


@pytest.mark.parametrize("compute, L, B", [("f16", 32000, 3), ("f16", 32000, 40), ("f16", 24001, 5), ("f16", 2187, 1), ("f16", 50000, 2),
                                           ("bf16", 32000, 40), ("bf16", 24001, 5)])
def test_fused_block0_is_bit_identical_to_the_two_kernel_route(compute, L, B):
    """block 0 computing its input rows from the waveform (rn_block128's CONV form) == rn_conv3_front -> rn_block128, bit for bit;
    the (L, B) cases span L mod 3, floor(L / 3) mod 78 tile remainders, one item and more items than CUs"""
    eng = Engine(model="rawnet2_conv", compute=compute, embed_dim=320, max_batch=B, samples=L)
    eng.load_state_dict(_conv_sd(3))
    eng.finalize()
    x = synth.synth_waveforms(B, L, seed=11)
    eng.profile(True)
    fused = eng.embed_wave(x)
    labels_fused = set(eng.profile_results())
    eng.profile(False)
    eng.set_option("rn_conv_unfused", 1)
    eng.profile(True)
    two = eng.embed_wave(x)
    labels_two = set(eng.profile_results()) - labels_fused
    eng.close()
    assert "rn_block128_conv" in labels_fused and "rn_conv3_front" not in labels_fused
    assert "rn_conv3_front" in labels_two
    assert np.isfinite(fused).all()
    assert np.array_equal(fused, two), float(np.abs(fused - two).max())


def test_conv_blob_path_equals_state_dict_path(tmp_path):
    from speakerverification_amd import checkpoint
    sd = _conv_sd(5)
    p = tmp_path / "conv.svhip"
    checkpoint.write_blob(p, "rawnet2_conv", sd)
    x = synth.synth_waveforms(3, 24001, seed=9)
    outs = []
    for via_blob in (False, True):
        e = Engine(model="rawnet2_conv", compute="f16", embed_dim=320, max_batch=3, samples=24001)
        if via_blob:
            e.load_blob(p)
        else:
            e.load_state_dict(sd)
            e.finalize()
        outs.append(e.embed_wave(x))
        e.close()
    assert np.array_equal(outs[0], outs[1])
    # a sinc blob is refused by a conv handle
    checkpoint.write_blob(tmp_path / "sinc.svhip", "rawnet2", synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320), seed=5))
    e = Engine(model="rawnet2_conv", compute="f32", embed_dim=320, max_batch=1, samples=24001)
    with pytest.raises(Exception):
        e.load_blob(tmp_path / "sinc.svhip")
    e.close()


def test_conv_handle_refuses_short_utterances():
    from speakerverification_amd import _lib
    with pytest.raises(_lib.SvhipError, match="2187"):
        Engine(model="rawnet2_conv", compute="f32", embed_dim=320, max_batch=1, samples=2186)
    e = Engine(model="rawnet2_conv", compute="f32", embed_dim=320, max_batch=1, samples=2187)
    e.close()


@pytest.mark.parametrize("compute", ["f32", "half"])
def test_raw_ecapa_conv_asp_matches_reference(golden_dir, compute):
    g = np.load(os.path.join(golden_dir, "fusion_raw_ecapa_conv.npz"))
    m = Raw_ECAPA_conv_asp.MainModel(nOut=512, hip_compute=compute, embed_batch=4, **KW)
    m.load_state_dict(_fusion_sd(g, "conv"))
    for L in g["lengths"]:
        x = synth.synth_waveforms(int(g["B"]), int(L), seed=int(g["seed_x"]))
        ref = g[f"out_{int(L)}"]
        out = m(x)
        # the 16-bit bar that applies is the looser branch's: the ECAPA branch runs bf16 under 'half'
        _check(out, ref, "bf16" if compute == "half" else compute, f"Raw_ECAPA_conv_asp L={int(L)}")
        if compute == "half":
            _check(out[:, 192:], ref[:, 192:], "f16", f"Raw_ECAPA_conv_asp rawnet2 branch L={int(L)}")


@pytest.mark.parametrize("compute", ["f32", "half"])
def test_raw_ecapa_matches_reference(golden_dir, compute):
    g = np.load(os.path.join(golden_dir, "fusion_raw_ecapa_in.npz"))
    m = Raw_ECAPA.MainModel(nOut=512, hip_compute=compute, embed_batch=4, **KW)
    m.load_state_dict(_fusion_sd(g, "sinc"))
    x = synth.synth_waveforms(int(g["B"]), 32000, seed=int(g["seed_x"]))
    ref = g["out_32000"]
    out = m(x)
    _check(out, ref, "bf16" if compute == "half" else compute, "Raw_ECAPA L=32000")
    if compute == "half":
        _check(out[:, 192:], ref[:, 192:], "f16", "Raw_ECAPA rawnet2 branch")


def test_conv_fusion_blob_and_device_paths_are_bit_identical(tmp_path):
    """blob pair == state dict; the CUDA two-stream path == the host path, also at a length other than the configured crop"""
    import torch
    from speakerverification_amd import checkpoint
    g = {"seed_w_ecapa": 1, "seed_w_rawnet2": 2}
    sd = _fusion_sd(g, "conv")
    dst = tmp_path / "conv_fusion.svhip"
    checkpoint.convert_checkpoint({"__S__." + k: v for k, v in sd.items()}, dst, "Raw_ECAPA_conv_asp")
    a = Raw_ECAPA_conv_asp.MainModel(nOut=512, embed_batch=6, hip_compute="half", **KW)
    a.load_state_dict(sd)
    b = Raw_ECAPA_conv_asp.MainModel(nOut=512, embed_batch=6, hip_compute="half", **KW)
    b.load_blob(dst)
    for L, B in ((32000, 5), (24001, 3)):
        x = synth.synth_waveforms(B, L, seed=L)
        host = a(x)
        assert host.shape == (B, 512) and np.isfinite(host).all()
        assert np.array_equal(b(x), host)
        dev = a(torch.from_numpy(x).cuda())
        assert dev.is_cuda and tuple(dev.shape) == (B, 512)
        assert np.array_equal(dev.cpu().numpy(), host), L
    # a sinc pair is refused by the conv module
    sd_sinc = _fusion_sd(g, "sinc")
    checkpoint.convert_checkpoint({"__S__." + k: v for k, v in sd_sinc.items()}, tmp_path / "sinc.svhip", "Raw_ECAPA")
    with pytest.raises(ValueError):
        Raw_ECAPA_conv_asp.MainModel(nOut=512, **KW).load_blob(tmp_path / "sinc.svhip")


@pytest.mark.parametrize("name", ["Raw_ECAPA_conv_asp", "Raw_ECAPA"])
def test_speaker_encoder_serves_the_config_models(name):
    from speakerverification_amd.model import SpeakerEncoder
    enc = SpeakerEncoder(model={"name": name, "nOut": 512}, features="raw", n_mels=80, audio_spec=AUDIO_SPEC)
    x = synth.synth_waveforms(3, 32000, seed=21)
    out = enc(x)
    out = out.detach().cpu().numpy() if hasattr(out, "detach") else np.asarray(out)
    assert out.shape == (3, 512) and np.isfinite(out).all()
