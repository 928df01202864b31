"""GPU parity of RawNet3 and Raw3_ECAPA (the model of the reference's default configs) against the outputs of the REFERENCE's own
modules in fp32 and float64 (tests/golden/rawnet3.npz, fusion_raw3_ecapa.npz; tools/make_golden_rawnet3.py), per-layer checksums,
the blob and device-resident paths, the create-time refusals and ModelHandling serving Raw3_ECAPA from a config dict.

Bars of the f32 handle.  Its filterbank sums run in fp64, so it tracks the exact (float64) result: <= 1e-5 of scale.  The reference's
OWN fp32 output is farther than that from the exact result on these weights (1.2e-4 .. 5.2e-4 of scale, printed by the generator:
log(|s| + 1e-6) turns the fp32 rounding of the filterbank sums into O(1) errors where s is near zero), so no handle that tracks the
exact result can sit within 1e-4 of it: the fp32 bar is 1e-4 beyond the reference's own fp32-to-float64 distance."""
import os

import numpy as np
import pytest

from speakerverification_amd import synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.models import Raw3_ECAPA, RawNet3

pytestmark = pytest.mark.gpu

AUDIO_SPEC = dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1)
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw", audio_spec=AUDIO_SPEC)
BF16_BARS = (0.999, 3e-2)           # tests/test_gpu_ecapa.py's bf16 bars: (min cosine, max error / scale)


def _cos(a, b):
    return np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def _rel(out, ref):
    return float(np.abs(out - ref).max()) / float(np.abs(ref).max())


def _check(out, ref32, ref64, compute, tag):
    out = np.atleast_2d(out)
    assert out.shape == ref32.shape and np.isfinite(out).all()
    r64, r32, own = _rel(out, ref64), _rel(out, ref32), _rel(ref32, ref64)
    cos = _cos(out, ref64)
    print(f"{tag} {compute}: to float64 {r64:.2e}, to fp32 {r32:.2e} (reference fp32 to float64 {own:.2e}), min cos {cos.min():.7f}")
    if compute == "f32":
        assert r64 <= 1e-5, r64
        assert r32 <= 1e-4 + own, (r32, own)
    else:
        c_min, r_max = BF16_BARS
        assert r64 <= r_max and float(cos.min()) >= c_min, (r64, cos)


def _sd(seed):
    return synth.synth_state_dict(synth.rawnet3_param_spec(nOut=320), seed=seed)


def _fusion_sd(seed_e=1, seed_r=1):
    sd = {"ECAPA_TDNN." + k: v for k, v in synth.synth_state_dict(synth.ecapa_param_spec(C=512, input_norm=True), seed=seed_e).items()}
    sd.update({"rawnet." + k: v for k, v in _sd(seed_r).items()})
    sd["compute_features.0.flipped_filter"] = np.array([[[-0.97, 1.0]]], np.float32)     # reference checkpoints carry it
    return sd


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_rawnet3_matches_reference_at_every_length(golden_dir, compute):
    g = np.load(os.path.join(golden_dir, "rawnet3.npz"))
    m = RawNet3.MainModel(nOut=320, hip_compute=compute, embed_batch=4, audio_spec=AUDIO_SPEC)
    m.load_state_dict(_sd(int(g["seed_w"])))
    for L in g["lengths"]:
        L = int(L)
        x = synth.synth_waveforms(int(g["B"]), L, seed=int(g["seed_x"]))
        _check(m(x), g[f"out_{L}"], g[f"out64_{L}"], compute, f"rawnet3 L={L}")
    assert len(m._engines) <= m.ENGINE_CACHE


def test_rawnet3_layer_checksums(golden_dir):
    """every stage of the f32 handle at L = 32000 against the reference's forward hooks (frame-major, fp32).  The hooks ran in fp32,
    so their sums carry the reference's own rounding (the pooled statistics sit 1.1e-5 of their |sum| away): the usual 1e-4 bar."""
    g = np.load(os.path.join(golden_dir, "rawnet3.npz"))
    e = Engine(model="rawnet3", compute="f32", embed_dim=320, channels=1024, max_batch=2, samples=32000)
    e.load_state_dict(_sd(int(g["seed_w"])))
    e.finalize()
    e.embed_wave(synth.synth_waveforms(2, 32000, seed=int(g["seed_x"])))
    for stage, key in (("rn3_front", "front"), ("rn3_layer1", "layer1"), ("rn3_layer2", "layer2"), ("rn3_layer3", "layer3"),
                       ("rn3_layer4", "layer4"), ("rn3_pooled", "pooled")):
        t = e.get_stage(stage).astype(np.float64)
        cs = g["cs_" + key]
        d_sum, d_abs = abs(t.sum() - cs[0]) / cs[1], abs(np.abs(t).sum() - cs[1]) / cs[1]
        d_head = float(np.abs(t[:8] - cs[2:]).max()) / max(1.0, float(np.abs(cs[2:]).max()))
        print(f"{stage}: sum {d_sum:.2e}, |sum| {d_abs:.2e}, first values {d_head:.2e} (of the |sum|)")
        assert d_sum <= 1e-4 and d_abs <= 1e-4 and d_head <= 1e-3, (stage, d_sum, d_abs, d_head)
    e.close()


@pytest.mark.parametrize("compute", ["f32", "half"])
def test_raw3_ecapa_matches_reference(golden_dir, compute):
    g = np.load(os.path.join(golden_dir, "fusion_raw3_ecapa.npz"))
    m = Raw3_ECAPA.MainModel(nOut=512, hip_compute=compute, embed_batch=4, **KW)
    m.load_state_dict(_fusion_sd(int(g["seed_w_ecapa"]), int(g["seed_w_rawnet3"])))
    x = synth.synth_waveforms(int(g["B"]), 32000, seed=int(g["seed_x"]))
    out = m(x)
    ref32, ref64 = g["out_32000"], g["out64_32000"]
    if compute == "f32":
        _check(out[:, 192:], ref32[:, 192:], ref64[:, 192:], "f32", "Raw3_ECAPA rawnet3 branch")
        assert _rel(out[:, :192], ref32[:, :192]) <= 1e-4                    # the ECAPA branch's usual bar
    else:
        _check(out, ref32, ref64, "bf16", "Raw3_ECAPA")


def test_blob_path_is_bit_identical_to_the_state_dict_path(tmp_path):
    from speakerverification_amd import checkpoint
    sd = _sd(5)
    p = tmp_path / "rawnet3.svhip"
    checkpoint.write_blob(p, "RawNet3", sd)
    x = synth.synth_waveforms(3, 24001, seed=9)
    for compute in ("f32", "bf16"):
        outs = []
        for via_blob in (False, True):
            e = Engine(model="rawnet3", compute=compute, embed_dim=320, max_batch=3, samples=24001)
            if via_blob:
                e.load_blob(p)
            else:
                e.load_state_dict(sd)
                e.finalize()
            outs.append(e.embed_wave(x))
            e.close()
        assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1]), compute


def test_create_refuses_short_inputs_and_other_computes():
    from speakerverification_amd import _lib
    with pytest.raises(_lib.SvhipError, match="541"):
        Engine(model="rawnet3", compute="f32", embed_dim=320, max_batch=1, samples=540)
    for compute in ("f32x3", "f16"):
        with pytest.raises(_lib.SvhipError) as ei:
            Engine(model="rawnet3", compute=compute, embed_dim=320, max_batch=1, samples=32000)
        assert ei.value.code == -1                  # SVHIP_ERR_INVALID
    with pytest.raises(_lib.SvhipError, match="1024"):
        Engine(model="rawnet3", compute="f32", embed_dim=320, channels=512, max_batch=1, samples=32000)
    e = Engine(model="rawnet3", compute="f32", embed_dim=320, max_batch=1, samples=541)
    e.close()


def test_device_resident_fusion_path_equals_the_host_path():
    import torch
    m = Raw3_ECAPA.MainModel(nOut=512, embed_batch=4, hip_compute="half", **KW)
    m.load_state_dict(_fusion_sd(1, 2))
    for L, B in ((32000, 3), (16000, 2)):
        x = synth.synth_waveforms(B, L, seed=L)
        host = m(x)
        assert host.shape == (B, 512) and np.isfinite(host).all()
        dev = m(torch.from_numpy(x).cuda())
        assert dev.is_cuda and tuple(dev.shape) == (B, 512)
        assert np.array_equal(dev.cpu().numpy(), host), L


def test_model_handling_embeds_with_raw3_ecapa(golden_dir):
    """the reference's default config (model.name Raw3_ECAPA, features raw, nOut 512) served through SpeakerEncoder /
    ModelHandling; the embedding of the fixture's waveform matches the reference module's"""
    import torch
    from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
    from tests.test_gpu_e2e import ARGS
    g = np.load(os.path.join(golden_dir, "fusion_raw3_ecapa.npz"))
    args = dict(ARGS, model={"name": "Raw3_ECAPA", "nOut": 512}, features="raw", classifier={"input_size": 512, "out_neurons": 10})
    enc = SpeakerEncoder(**args)
    enc.load_state_dict({"__S__." + k: v for k, v in _fusion_sd(int(g["seed_w_ecapa"]), int(g["seed_w_rawnet3"])).items()})
    x = synth.synth_waveforms(int(g["B"]), 32000, seed=int(g["seed_x"]))
    out = enc(x)
    out = out.detach().cpu().numpy() if hasattr(out, "detach") else np.asarray(out)
    assert out.shape == (2, 512)
    assert _rel(out, g["out64_32000"]) <= 1e-4 + _rel(g["out_32000"], g["out64_32000"])
    mh = ModelHandling(WrappedModel(enc), **args)
    emb = mh.embed_utterance(x[0], num_eval=2, normalize=True)
    emb = emb.numpy() if hasattr(emb, "numpy") else np.asarray(emb)
    assert np.isfinite(emb).all() and emb.size % 512 == 0
