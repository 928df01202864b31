"""Host-side checks of Raw_ECAPA_hype and of the sinc front-end's sample rate: the head's parameter spec and the model's keys against the
reference's key list (tests/golden/fusion_raw_ecapa_hype.npz; tools/make_golden_hype.py), the float64 restatement of the head
(tests/hype_head_oracle.py) against the reference's own output, the ABI's new field, checkpoint naming and the constructors.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from speakerverification_amd import _lib, checkpoint, synth
from tests import hype_head_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE = ("ECAPA_TDNN.", "rawnet2v2.", "compute_features.")


def _kw(sr=8000, sentence_len=2.0):
    spec = dict(sample_rate=sr, sentence_len=sentence_len, win_len=0.025, hop_len=0.01, channels=1)
    return dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw", audio_spec=spec)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "fusion_raw_ecapa_hype.npz"))


def test_head_spec_and_model_keys_are_the_references(gold):
    from speakerverification_amd.models import Raw_ECAPA_hype
    keys = list(gold["keys"])
    spec = synth.hype_head_param_spec(512)
    assert len(spec) == 21 and [k for k in keys if not k.startswith(PRE)] == [k for k, _ in spec]
    m = Raw_ECAPA_hype.MainModel(nOut=512, **_kw())
    assert list(m.state_dict()) == [k for k in keys if not k.startswith("compute_features.")]
    assert len(m.state_dict()) == 233 + 144 + 21
    assert m.ECAPA_TDNN.input_norm and m.rawnet2v2.model_kind == "rawnet2_gru" and m.rawnet2v2.nb_samp == 16000
    assert m.rawnet2v2._engine_kwargs == dict(embed_dim=512, sinc_sr=8000)
    assert not hasattr(m, "embed_ragged")                       # LayerNorm(nb_samp) fixes the length
    n_par = sum(1 for _ in m.parameters())
    assert n_par == sum(1 for k in m.state_dict() if "running_" not in k and "num_batches" not in k)
    assert synth.hype_head_param_spec(200)[-2:] == [("fc.weight", (200, 1408)), ("fc.bias", (200,))]


def test_load_state_dict_covers_the_three_parts(gold):
    from speakerverification_amd.models import Raw_ECAPA_hype
    m = Raw_ECAPA_hype.MainModel(nOut=512, **_kw())
    sd = dict(m.state_dict())
    head = synth.synth_state_dict(synth.hype_head_param_spec(512), seed=int(gold["seed_w_head"]))
    sd.update(head)
    sd["compute_features.0.flipped_filter"] = np.array([[[-0.97, 1.0]]], np.float32)
    m.load_state_dict(sd, strict=True)                          # compute_features.* is accepted
    assert np.array_equal(np.asarray(m.state_dict()["fc.weight"]), head["fc.weight"])
    with pytest.raises(KeyError):
        m.load_state_dict(dict(sd, stray=np.zeros(3, np.float32)), strict=True)
    with pytest.raises(KeyError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "bn_final.weight"}, strict=True)
    m.load_state_dict(dict(sd, stray=np.zeros(3, np.float32)), strict=False)


def test_float64_head_reproduces_the_reference(gold):
    """the restatement, fed the reference's branch outputs, gives the reference's fp32 output within fp32 round-off"""
    head = synth.synth_state_dict(synth.hype_head_param_spec(512), seed=int(gold["seed_w_head"]))
    for L in gold["lengths"]:
        ref = gold[f"out_{int(L)}"]
        out = hype_head_oracle.head_forward(head, gold[f"out1_{int(L)}"], gold[f"out2_{int(L)}"])
        scale = float(np.abs(ref).max())
        err = float(np.abs(out - ref).max())
        print(f"L={int(L)}: max|d| / scale {err / scale:.2e}")
        assert out.shape == ref.shape == (2, 512) and err <= 1e-5 * scale


def test_abi_config_field():
    text = open(os.path.join(ROOT, "include", "svhip.h")).read()
    assert re.search(r"#define SVHIP_ABI_VERSION 5\b", text)
    m = re.search(r"SVHIP_MODEL_FUSION_HEAD\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == _lib.MODEL_FUSION_HEAD == 9
    cfg = _lib.default_config()
    assert cfg.struct_size == ctypes.sizeof(_lib.Config)
    assert _lib.Config._fields_[-1][0] == "sinc_sr" and cfg.sinc_sr == 16000
    assert _lib.load().svhip_abi_version() == 5


def test_checkpoint_knows_the_model(tmp_path, capsys):
    assert checkpoint._MODEL_IDS["fusion_head"] == checkpoint._MODEL_IDS["Raw_ECAPA_hype_head"] == 9
    assert checkpoint.fusion_blob_paths("x.svhip", "Raw_ECAPA_hype") == ("x.svhip.ecapa", "x.svhip.rawnet2", "x.svhip.head")
    e = synth.synth_state_dict(synth.ecapa_param_spec(C=512, input_norm=True), seed=1)
    r = synth.synth_state_dict(synth.rawnet2_param_spec(nOut=512, nb_samp=16000, aggregate="gru"), seed=1, sample_rate=8000)
    hd = synth.synth_state_dict(synth.hype_head_param_spec(512), seed=3)
    sd = {"__S__.ECAPA_TDNN." + k: v for k, v in e.items()}
    sd.update({"__S__.rawnet2v2." + k: v for k, v in r.items()})
    sd.update({"__S__." + k: v for k, v in hd.items()})
    sd["__S__.compute_features.0.flipped_filter"] = np.array([[[-0.97, 1.0]]], np.float32)
    dst = tmp_path / "hype.svhip"
    assert checkpoint.convert_checkpoint(sd, dst, "Raw_ECAPA_hype") == 233 + 144 + 21
    mid, back = checkpoint.read_blob(str(dst) + ".head")
    assert mid == 9 and list(back) == list(hd) and all(np.array_equal(back[k], v) for k, v in hd.items())
    assert checkpoint.read_blob(str(dst) + ".rawnet2")[0] == _lib.MODEL_RAWNET2_GRU
    from speakerverification_amd.models import Raw_ECAPA_hype
    m = Raw_ECAPA_hype.MainModel(nOut=512, **_kw())
    done = m.load_blob(dst)
    assert len(done) == 3 and not any(missing for missing, _ in done)
    assert np.array_equal(np.asarray(m.state_dict()["attention.3.bias"]), hd["attention.3.bias"])
    # the pair converted as Raw_ECAPA_sinc_gru has no head blob
    sd_gru = {k: v for k, v in sd.items() if k.startswith(("__S__.ECAPA_TDNN.", "__S__.rawnet2v2."))}
    checkpoint.convert_checkpoint(sd_gru, tmp_path / "gru.svhip", "Raw_ECAPA_sinc_gru")
    with pytest.raises(ValueError, match="Raw_ECAPA_sinc_gru"):
        Raw_ECAPA_hype.MainModel(nOut=512, **_kw()).load_blob(tmp_path / "gru.svhip")
    # a head blob that lacks a tensor
    checkpoint.write_blob(str(dst) + ".head", "fusion_head", {k: v for k, v in hd.items() if k != "fc.bias"})
    with pytest.raises(_lib.SvhipError) as ei:
        Raw_ECAPA_hype.MainModel(nOut=512, **_kw()).load_blob(dst)
    assert ei.value.code == _lib.ERR_MISSING
    with pytest.raises(SystemExit):
        checkpoint.main(["--help"])
    assert "Raw_ECAPA_hype" in capsys.readouterr().out


def test_sinc_models_take_their_configured_rate():
    from speakerverification_amd.models import RawNet2_custom, Raw_ECAPA, Raw_ECAPA_sinc_asp
    spec8 = dict(sample_rate=8000, sentence_len=1.0, win_len=0.025, hop_len=0.01, channels=1)
    m = RawNet2_custom.MainModel(nOut=320, front_proc="sinc", aggregate="asp", audio_spec=spec8)
    assert m.nb_samp == 8000 and m._engine_kwargs["sinc_sr"] == 8000
    lo, band = synth._sinc_init(128, 8000)
    assert float(np.abs(np.asarray(m.state_dict()["first_conv.low_hz_"])[:, 0] - lo).max()) <= 3.0       # the 8 kHz start, plus jitter
    assert RawNet2_custom.MainModel(nOut=320)._engine_kwargs["sinc_sr"] == 16000
    assert RawNet2_custom.MainModel(nOut=320, front_proc="conv", aggregate="asp", audio_spec=spec8)._engine_kwargs["sinc_sr"] == 16000
    assert Raw_ECAPA.MainModel(nOut=512, **_kw(8000, 1.0)).rawnet2v2.nb_samp == 8000                     # yaml/verification.yaml
    assert Raw_ECAPA_sinc_asp.MainModel(nOut=512, **_kw(8000, 2.0)).rawnet2v2._engine_kwargs["sinc_sr"] == 8000


def test_synth_sample_rate_default_is_unchanged():
    spec = synth.rawnet2_param_spec(nOut=320, nb_samp=4000)
    a, b = synth.synth_state_dict(spec, seed=4), synth.synth_state_dict(spec, seed=4, sample_rate=16000)
    assert list(a) == list(b) and all(x.tobytes() == y.tobytes() and x.dtype == y.dtype for x, y in zip(a.values(), b.values()))
    c = synth.synth_state_dict(spec, seed=4, sample_rate=8000)
    assert not np.array_equal(a["first_conv.low_hz_"], c["first_conv.low_hz_"])
    assert all(np.array_equal(a[k], c[k]) for k in a if not k.startswith("first_conv."))     # only the band edges move
