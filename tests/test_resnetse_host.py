"""Host-side ResNetSE34V2 checks (no GPU): the parameter spec against the reference's key list and shapes, a float64 restatement of the
network (ref64, which the GPU tests import) against the reference module's own float64 outputs and stage checksums on every case of
tests/golden/resnetse34v2.npz (tools/make_golden_resnetse.py) — and its visible difference when the first block's residual is taken from
x instead of relu(x) — the plug-in's refusals and the checkpoint blob round trip."""
import os

import numpy as np
import pytest
import torch

from oracle import fbank as o_fbank, resnetse as o_resnetse
from speakerverification_amd import _lib, checkpoint, synth
from speakerverification_amd.models import ResNetSE34V2

AUDIO_SPEC = dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1)
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="melspectrogram", audio_spec=AUDIO_SPEC)


def load_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "resnetse34v2.npz"))


def case_cfg(g, name):
    features, enc, n_mels = (str(v) for v in g[f"{name}_cfg"])
    return features, enc, int(n_mels)


def mel_of(L, n_mels, B=2, seed=20220829):
    """the fixture's input: the mel power of the synthetic waveforms, front-end in float64 and rounded once to fp32 (the same bits on every machine)"""
    return o_fbank.melspectrogram(torch.from_numpy(synth.synth_waveforms(B, L, seed=seed)).double(), n_mels=n_mels).float().numpy()


def checksum(t):
    t = np.asarray(t, np.float64)
    return np.array([t.sum(), np.abs(t).sum()] + list(t.ravel()[:8]))


def ref64(sd, mel, features="melspectrogram", encoder_type="ASP", residual_relu=True):
    """float64 restatement of ResNetSE.forward with SEBasicBlockV2 (ResNetBaseline.py:250-301, ResNetBlocks.py:229-246,303-307;
    oracle/resnetse.py, one utterance at a time): returns the stages in the reference's (B, C, n_mels', T') layout and the embedding.  residual_relu=False takes the identity residual from x, as
    the block would WITHOUT its in-place ReLU (only the first block's input has negative values)."""
    t = o_resnetse.to_torch_sd(sd)
    last = [i for i, p in enumerate(o_resnetse.block_names(t)) if p.endswith(".0.")][1:] + [len(o_resnetse.block_names(t))]
    names = dict([("rs_stem", "stem")] + [(f"rs_layer{s + 1}", f"b{i - 1}_out") for s, i in enumerate(last)])
    F_ = t["attention.3.weight"].shape[0]
    st, emb = {n: [] for n in list(names) + ["rs_pool"]}, []
    with torch.no_grad():
        for m in torch.from_numpy(np.asarray(mel)).double():
            s = {}
            emb.append(o_resnetse.forward(m, t, log_input=features == "melspectrogram", residual_relu=residual_relu, stages=s).numpy())
            for n, k in names.items():
                st[n].append(s[k].permute(2, 1, 0).numpy())          # (P, Q, C) -> (C, Q, P)
            st["rs_pool"].append(s["pool"].numpy()[:2 * F_ if encoder_type == "ASP" else F_])
    return {k: np.stack(v) for k, v in st.items()}, np.stack(emb)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max()) / float(np.abs(np.asarray(b)).max())


def test_param_spec_equals_reference_keys_and_shapes(golden_dir):
    g = load_golden(golden_dir)
    for name in (str(c) for c in g["cases"]):
        _, enc, n_mels = case_cfg(g, name)
        spec = synth.resnetse_param_spec(int(g["nOut"]), n_mels, enc)
        assert [k for k, _ in spec] == [str(k) for k in g[f"{name}_keys"]]
        assert [",".join(str(d) for d in s) for _, s in spec] == [str(s) for s in g[f"{name}_shapes"]]
        m = ResNetSE34V2.MainModel(nOut=int(g["nOut"]), encoder_type=enc, device="cpu", **dict(KW, n_mels=n_mels))
        assert list(m.state_dict()) == [str(k) for k in g[f"{name}_keys"]]
    assert len(synth.resnetse_param_spec(256)) == 292


def test_float64_restatement_reproduces_the_reference(golden_dir):
    g = load_golden(golden_dir)
    for name in (str(c) for c in g["cases"]):
        features, enc, n_mels = case_cfg(g, name)
        sd = synth.synth_state_dict(synth.resnetse_param_spec(int(g["nOut"]), n_mels, enc), seed=int(g["seed_w"]))
        for L in (int(v) for v in g[f"{name}_lengths"]):
            mel = mel_of(L, n_mels, int(g["B"]), int(g["seed_x"]))
            assert np.allclose(checksum(mel)[:2], g[f"{name}_mel_L{L}"][:2], rtol=1e-5)
            st, emb = ref64(sd, mel, features, enc)
            r = _rel(emb, g[f"{name}_out64_L{L}"])
            print(f"{name} L={L}: restatement to the reference's float64 {r:.2e} of scale")
            assert r <= 1e-9, (name, L, r)
            if L == 32000:
                for sn, key in [("rs_stem", "stem")] + [(f"rs_layer{s}", f"layer{s}") for s in range(1, 5)] + [("rs_pool", "pool")]:
                    want = g[f"{name}_stage_{key}"]
                    got = checksum(st[sn])
                    assert np.abs(got - want).max() <= 1e-9 * np.abs(want[1]), (name, sn, got[:2], want[:2])


def test_residual_is_taken_after_the_in_place_relu(golden_dir):
    """the identity residual of the first block is relu(x), not x: without the in-place ReLU the embedding moves visibly"""
    g = load_golden(golden_dir)
    name, L = "mel_asp_80", 32000
    sd = synth.synth_state_dict(synth.resnetse_param_spec(int(g["nOut"])), seed=int(g["seed_w"]))
    mel = mel_of(L, 80, int(g["B"]), int(g["seed_x"]))
    st, emb = ref64(sd, mel, residual_relu=False)
    r = _rel(emb, g[f"{name}_out64_L{L}"])
    print(f"residual from x instead of relu(x): embedding moves by {r:.2e} of scale")
    assert r >= 1e-3
    assert (st["rs_stem"] < 0).mean() >= 0.1


def test_plugin_refusals():
    with pytest.raises(NotImplementedError):
        ResNetSE34V2.MainModel(nOut=256, device="cpu", **dict(KW, n_mels=30))
    with pytest.raises(NotImplementedError):
        ResNetSE34V2.MainModel(nOut=256, att_dim=64, device="cpu", **KW)
    for compute in ("f16", "f32x3"):
        with pytest.raises(NotImplementedError):
            ResNetSE34V2.MainModel(nOut=256, hip_compute=compute, device="cpu", **KW)
    with pytest.raises(ValueError):
        ResNetSE34V2.MainModel(nOut=256, encoder_type="TAP", device="cpu", **KW)
    m = ResNetSE34V2.MainModel(nOut=256, device="cpu", **KW)
    with pytest.raises(ValueError):
        m(np.ones((2, 80, 1), np.float32))                   # T = 1: InstanceNorm1d over one frame, a ValueError in the reference
    with pytest.raises(ValueError):
        m(np.ones((2, 32000), np.float32))                   # forward takes (B, n_mels, T) features
    with pytest.raises(ValueError):
        m.embed_wave(np.zeros((2, 400), np.float32))
    assert m.accepts_length(512) and not m.accepts_length(511)
    sap = ResNetSE34V2.MainModel(nOut=256, encoder_type="SAP", device="cpu", **KW)
    assert tuple(sap.state_dict()["fc.weight"].shape) == (256, 2560) and tuple(m.state_dict()["fc.weight"].shape) == (256, 5120)


def test_checkpoint_blob_round_trip(tmp_path):
    sd = synth.synth_state_dict(synth.resnetse_param_spec(192, 80), seed=4)
    path = str(tmp_path / "resnetse.svhip")
    n = checkpoint.convert_checkpoint({"__S__." + k: v for k, v in sd.items()}, path, "ResNetSE34V2")
    assert n == len(sd) == 292
    mid, back = checkpoint.read_blob(path)
    assert mid == _lib.MODEL_RESNETSE == 8
    assert list(back) == list(sd)
    for k, v in sd.items():
        assert np.array_equal(np.asarray(back[k]), np.asarray(v)), k
    m = ResNetSE34V2.MainModel(nOut=192, device="cpu", **KW)
    m.load_blob(path)
    assert np.array_equal(np.asarray(m.state_dict()["layer4.2.conv2.weight"]), sd["layer4.2.conv2.weight"])
    other = tmp_path / "titanet.svhip"
    checkpoint.write_blob(other, "TitaNet", {})
    with pytest.raises(ValueError):
        m.load_blob(str(other))
