"""Host-side checks of RawNet2's GRU aggregation (aggregate='gru', the reference's default) and of Raw_ECAPA_sinc_gru: the parameter
spec against the reference's key list (tests/golden/rawnet2_gru.npz, fusion_raw_ecapa_sinc_gru.npz; tools/make_golden_rawnet2_gru.py),
the C header's model id, the plug-ins' constructors, the checkpoint conversion, and a float64 restatement of the GRU that pins the
fixture's last state — the oracle tests/test_gpu_rawnet2_gru.py compares the library's recurrence with.  No GPU."""
import os
import re

import numpy as np
import pytest

from speakerverification_amd import _lib, checkpoint, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIO_SPEC = dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1)
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw", audio_spec=AUDIO_SPEC)
GRU_SHAPES = {"bn_before_gru.weight": (512,), "gru.weight_ih_l0": (3072, 512), "gru.weight_hh_l0": (3072, 1024), "gru.bias_ih_l0": (3072,),
              "gru.bias_hh_l0": (3072,), "fc_after_gru.weight": (320, 1024), "fc_after_gru.bias": (320,), "fc.weight": (320, 1024),
              "fc.bias": (320,)}


def gru_f64(x, sd):
    """torch.nn.GRU (one layer, batch_first, h0 = 0, gate order r, z, n) in float64: x (B, T, 512) -> h_T (B, 1024)"""
    W_ih, W_hh = (np.asarray(sd[k], np.float64) for k in ("gru.weight_ih_l0", "gru.weight_hh_l0"))
    b_ih, b_hh = (np.asarray(sd[k], np.float64) for k in ("gru.bias_ih_l0", "gru.bias_hh_l0"))
    H = W_hh.shape[1]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    x = np.asarray(x, np.float64)
    h = np.zeros((x.shape[0], H))
    for t in range(x.shape[1]):
        gi = x[:, t] @ W_ih.T + b_ih
        gh = h @ W_hh.T + b_hh
        r = sig(gi[:, :H] + gh[:, :H])
        z = sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1.0 - z) * n + z * h
    return h


def _gru_sd(g, L=32000):
    return synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, nb_samp=L, aggregate="gru"), seed=int(g["seed_w"]))


def test_gru_spec_matches_the_reference_key_list(golden_dir):
    g = np.load(os.path.join(golden_dir, "rawnet2_gru.npz"))
    spec = synth.rawnet2_param_spec(nOut=320, aggregate="gru")
    assert [k for k, _ in spec] == list(g["keys"])
    assert len(spec) == 144
    d = dict(spec)
    for k, s in GRU_SHAPES.items():
        assert d[k] == s, k
    assert not any(k.startswith(("bn_before_agg.", "attention.")) for k in d)
    # the asp and conv specs are unchanged
    assert synth.rawnet2_param_spec(nOut=320) == synth.rawnet2_param_spec(nOut=320, aggregate="asp")
    assert len(synth.rawnet2_param_spec(nOut=320)) == 147 and len(synth.rawnet2_param_spec(nOut=320, front_proc="conv")) == 140
    with pytest.raises(ValueError):
        synth.rawnet2_param_spec(front_proc="gru")
    with pytest.raises(ValueError):
        synth.rawnet2_param_spec(aggregate="sap")


def test_gru_weights_follow_torch_init_and_leave_other_specs_alone():
    sd = synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, aggregate="gru"), seed=1)
    k = 1.0 / np.sqrt(1024)
    for name in ("gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0"):
        a = sd[name]
        assert a.dtype == np.float32 and np.abs(a).max() <= k and np.abs(a).max() > 0.9 * k, name
    # no existing spec holds a GRU name: their synthetic state dicts draw exactly what they drew before
    for spec in (synth.rawnet2_param_spec(nOut=320), synth.rawnet2_param_spec(nOut=320, front_proc="conv"), synth.ecapa_param_spec(C=512),
                 synth.rawnet3_param_spec()):
        assert not any("_l0" in n for n, _ in spec)


def test_fusion_key_list(golden_dir):
    keys = list(np.load(os.path.join(golden_dir, "fusion_raw_ecapa_sinc_gru.npz"))["keys"])
    want = ["ECAPA_TDNN." + k for k, _ in synth.ecapa_param_spec(C=512, input_norm=False)]
    want += ["rawnet2v2." + k for k, _ in synth.rawnet2_param_spec(nOut=320, aggregate="gru")]
    assert sorted(k for k in keys if not k.startswith("compute_features.")) == sorted(want)
    assert len(want) == 231 + 144


def test_header_model_id_matches_the_binding():
    text = open(os.path.join(ROOT, "include", "svhip.h")).read()
    m = re.search(r"SVHIP_MODEL_RAWNET2_GRU\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == _lib.MODEL_RAWNET2_GRU == 5
    assert re.search(r"#define SVHIP_ABI_VERSION 5\b", text)


def test_constructors_and_unbuilt_variants():
    from speakerverification_amd.models import RawNet2_custom, Raw_ECAPA_sinc_gru
    m = RawNet2_custom.MainModel(nOut=320)                       # the reference's defaults: front_proc='sinc', aggregate='gru'
    assert m.model_kind == "rawnet2_gru" and m.aggregate == "gru" and m.nb_samp == 32000
    assert len(m.state_dict()) == 144
    assert RawNet2_custom.MainModel(nOut=320, aggregate="asp").model_kind == "rawnet2"
    assert RawNet2_custom.MainModel(nOut=320, hip_compute="half")._is_f16_handle()
    for kw in (dict(front_proc="conv", aggregate="gru"), dict(aggregate="sap"), dict(gru_node=512), dict(nb_gru_layers=2)):
        with pytest.raises(NotImplementedError):
            RawNet2_custom.MainModel(nOut=320, **kw)
    f = Raw_ECAPA_sinc_gru.MainModel(nOut=512, **KW)
    assert not f.ECAPA_TDNN.input_norm and f.rawnet2v2.model_kind == "rawnet2_gru"
    assert len(f.state_dict()) == 231 + 144
    sd = {"ECAPA_TDNN." + k: v for k, v in synth.synth_state_dict(synth.ecapa_param_spec(C=512), seed=1).items()}
    sd.update({"rawnet2v2." + k: v for k, v in synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, aggregate="gru"), seed=1).items()})
    sd["compute_features.0.flipped_filter"] = np.array([[[-0.97, 1.0]]], np.float32)
    f.load_state_dict(sd, strict=True)


def _fusion_state(aggregate):
    e = synth.synth_state_dict(synth.ecapa_param_spec(C=512), seed=1)
    r = synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, aggregate=aggregate), seed=1)
    sd = {"__S__.ECAPA_TDNN." + k: v for k, v in e.items()}
    sd.update({"__S__.rawnet2v2." + k: v for k, v in r.items()})
    return sd, e, r


def test_checkpoint_round_trip_and_aggregate_mismatches(tmp_path):
    from speakerverification_amd.models import RawNet2_custom, Raw_ECAPA_sinc_asp, Raw_ECAPA_sinc_gru
    sd, e, r = _fusion_state("gru")
    dst = tmp_path / "gru.svhip"
    assert checkpoint.convert_checkpoint(sd, dst, "Raw_ECAPA_sinc_gru") == 231 + 144
    p_e, p_r = checkpoint.fusion_blob_paths(dst, "Raw_ECAPA_sinc_gru")
    mid_r, back = checkpoint.read_blob(p_r)
    assert mid_r == _lib.MODEL_RAWNET2_GRU and checkpoint.read_blob(p_e)[0] == _lib.MODEL_ECAPA
    assert list(back) == list(r) and all(np.array_equal(back[k], np.asarray(v)) for k, v in r.items())
    m = Raw_ECAPA_sinc_gru.MainModel(nOut=512, **KW)
    missing, _ = m.load_blob(dst)[1]
    assert not missing
    # a gru blob pair into the asp module, and the reverse, raise
    with pytest.raises(ValueError):
        Raw_ECAPA_sinc_asp.MainModel(nOut=512, **KW).load_blob(dst)
    sd_asp, _, _ = _fusion_state("asp")
    checkpoint.convert_checkpoint(sd_asp, tmp_path / "asp.svhip", "Raw_ECAPA_sinc_asp")
    with pytest.raises(ValueError):
        Raw_ECAPA_sinc_gru.MainModel(nOut=512, **KW).load_blob(tmp_path / "asp.svhip")
    # a checkpoint converted as the other aggregate is refused with a clear message
    with pytest.raises(ValueError, match="gru"):
        checkpoint.convert_checkpoint(sd, tmp_path / "x.svhip", "Raw_ECAPA_sinc_asp")
    with pytest.raises(ValueError, match="attention"):
        checkpoint.convert_checkpoint(sd_asp, tmp_path / "y.svhip", "Raw_ECAPA_sinc_gru")
    # a bare RawNet2 checkpoint: its own blob id, and the same guards
    checkpoint.convert_checkpoint(r, tmp_path / "rn.svhip", "RawNet2_custom_gru")
    assert checkpoint.read_blob(tmp_path / "rn.svhip")[0] == _lib.MODEL_RAWNET2_GRU
    assert not RawNet2_custom.MainModel(nOut=320).load_blob(tmp_path / "rn.svhip")[0]
    with pytest.raises(ValueError):
        RawNet2_custom.MainModel(nOut=320, aggregate="asp").load_blob(tmp_path / "rn.svhip")
    with pytest.raises(ValueError, match="gru"):
        checkpoint.convert_checkpoint(r, tmp_path / "z.svhip", "RawNet2_custom")


def test_checkpoint_help_lists_the_gru_models(capsys):
    with pytest.raises(SystemExit):
        checkpoint.main(["--help"])
    out = capsys.readouterr().out
    assert "Raw_ECAPA_sinc_gru" in out and "RawNet2_custom_gru" in out
    assert "Raw_ECAPA_sinc_gru" in checkpoint.FUSION_MODELS


def test_float64_gru_reproduces_the_fixture_state(golden_dir):
    """the float64 restatement, fed the reference's GRU input, gives the reference's fp32 h_T within fp32 round-off"""
    g = np.load(os.path.join(golden_dir, "rawnet2_gru.npz"))
    x, h_ref = g["gru_in"], g["h_T"]
    assert x.shape == (2, int(g["T_32000"]), 512) and x.shape[1] == 14 and h_ref.shape == (2, 1024)
    assert [int(g[f"T_{L}"]) for L in g["lengths"]] == [1, 14, 43]
    h = gru_f64(x, _gru_sd(g))
    scale = float(np.abs(h).max())
    err = float(np.abs(h - h_ref).max())
    print(f"float64 GRU against the reference's fp32 h_T: {err / scale:.2e} of scale {scale:.3f}")
    assert err <= 1e-5 * scale
    # the recurrence matters: the last frame alone from h = 0 is far from h_T
    h1 = gru_f64(x[:, -1:], _gru_sd(g))
    assert float(np.abs(h1 - h_ref).max()) >= 0.1 * scale
    # and fc_after_gru (not fc) maps h_T to the output
    sd = _gru_sd(g)
    out = h.astype(np.float64) @ sd["fc_after_gru.weight"].astype(np.float64).T + sd["fc_after_gru.bias"]
    assert float(np.abs(out - g["out_32000"]).max()) <= 1e-4 * float(np.abs(g["out_32000"]).max())
    wrong = h @ sd["fc.weight"].astype(np.float64).T + sd["fc.bias"]
    assert float(np.abs(wrong - g["out_32000"]).max()) > 0.1 * float(np.abs(g["out_32000"]).max())
