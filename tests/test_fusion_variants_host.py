"""Host-side checks of the two fusion models the reference configs name (Raw_ECAPA, Raw_ECAPA_conv_asp) and of RawNet2's
'conv' front-end: parameter specs against the reference's key lists (tests/golden/rawnet2_conv.npz, fusion_raw_ecapa_*.npz),
the C header's model id, the plug-ins' input checks and the checkpoint conversion.  No GPU."""
import os
import re

import numpy as np
import pytest

from speakerverification_amd import _lib, checkpoint, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw",
          audio_spec=dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1))


def test_conv_spec_matches_the_reference_key_list(golden_dir):
    g = np.load(os.path.join(golden_dir, "rawnet2_conv.npz"))
    spec = synth.rawnet2_param_spec(nOut=320, front_proc="conv")
    assert [k for k, _ in spec] == list(g["keys"])
    assert len(spec) == 140
    assert dict(spec)["conv1.weight"] == (128, 1, 3) and dict(spec)["conv1.bias"] == (128,)
    assert not any(k.startswith(("ln.", "first_conv.", "first_bn.")) for k, _ in spec)
    # the default output is the sinc form, unchanged
    assert synth.rawnet2_param_spec(nOut=320) == synth.rawnet2_param_spec(nOut=320, front_proc="sinc")
    assert len(synth.rawnet2_param_spec(nOut=320)) == 147
    with pytest.raises(ValueError):
        synth.rawnet2_param_spec(front_proc="gru")


@pytest.mark.parametrize("fname, front, n_keys", [("fusion_raw_ecapa_conv.npz", "conv", 374), ("fusion_raw_ecapa_in.npz", "sinc", 381)])
def test_fusion_key_lists(golden_dir, fname, front, n_keys):
    keys = list(np.load(os.path.join(golden_dir, fname))["keys"])
    assert len(keys) == n_keys
    want = ["ECAPA_TDNN." + k for k, _ in synth.ecapa_param_spec(C=512, input_norm=True)]
    want += ["rawnet2v2." + k for k, _ in synth.rawnet2_param_spec(nOut=320, front_proc=front)]
    assert sorted(k for k in keys if not k.startswith("compute_features.")) == sorted(want)
    assert [k for k in keys if k.startswith("compute_features.")] == ["compute_features.0.flipped_filter"]


def test_header_model_id_matches_the_binding():
    text = open(os.path.join(ROOT, "include", "svhip.h")).read()
    m = re.search(r"SVHIP_MODEL_RAWNET2_CONV\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == _lib.MODEL_RAWNET2_CONV == 3
    assert re.search(r"#define SVHIP_ABI_VERSION 5\b", text)


def test_plugins_import_and_hold_the_reference_keys():
    from speakerverification_amd.models import Raw_ECAPA, Raw_ECAPA_conv_asp, Raw_ECAPA_sinc_asp
    conv = Raw_ECAPA_conv_asp.MainModel(nOut=512, **KW)
    inn = Raw_ECAPA.MainModel(nOut=512, **KW)
    sinc = Raw_ECAPA_sinc_asp.MainModel(nOut=512, **KW)
    assert len(conv.state_dict()) == 233 + 140
    assert len(inn.state_dict()) == 233 + 147
    assert len(sinc.state_dict()) == 231 + 147
    assert conv.ECAPA_TDNN.input_norm and inn.ECAPA_TDNN.input_norm and not sinc.ECAPA_TDNN.input_norm
    assert conv.rawnet2v2.model_kind == "rawnet2_conv" and inn.rawnet2v2.model_kind == "rawnet2"
    # a reference checkpoint's state dict (with the nnAudio buffer) loads strictly
    sd = {"ECAPA_TDNN." + k: v for k, v in synth.synth_state_dict(synth.ecapa_param_spec(C=512, input_norm=True), seed=1).items()}
    sd.update({"rawnet2v2." + k: v for k, v in synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, front_proc="conv"), seed=1).items()})
    sd["compute_features.0.flipped_filter"] = np.array([[[-0.97, 1.0]]], np.float32)
    conv.load_state_dict(sd)


def test_conv_front_end_input_checks_need_no_gpu():
    from speakerverification_amd.models import RawNet2_custom
    with pytest.raises(NotImplementedError):
        RawNet2_custom.MainModel(nOut=320, front_proc="gru", aggregate="asp")
    with pytest.raises(NotImplementedError):
        RawNet2_custom.MainModel(nOut=320, front_proc="conv", aggregate="sap")
    with pytest.raises(NotImplementedError):
        RawNet2_custom.MainModel(nOut=320, front_proc="conv", aggregate="asp", att_dim=64)
    m = RawNet2_custom.MainModel(nOut=320, front_proc="conv", aggregate="asp", att_dim=128)
    assert len(m.state_dict()) == 140
    assert m.accepts_length(2187) and m.accepts_length(24001) and not m.accepts_length(2186)
    with pytest.raises(ValueError, match="2187"):
        m(np.zeros((2, 2186), np.float32))
    assert not m._engines                           # refused before any handle was made
    # the sinc form keeps its fixed length
    s = RawNet2_custom.MainModel(nOut=320, front_proc="sinc", aggregate="asp", att_dim=128)
    assert s.accepts_length(32000) and not s.accepts_length(24001)
    with pytest.raises(ValueError):
        s(np.zeros((2, 24001), np.float32))


def _fusion_state(front, input_norm=True, prefix="__S__."):
    e = synth.synth_state_dict(synth.ecapa_param_spec(C=512, input_norm=input_norm), seed=1)
    r = synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, front_proc=front), seed=1)
    sd = {prefix + "ECAPA_TDNN." + k: v for k, v in e.items()}
    sd.update({prefix + "rawnet2v2." + k: v for k, v in r.items()})
    sd["compute_features.0.flipped_filter"] = np.array([[[-0.97, 1.0]]], np.float32)
    return sd, e, r


def test_conv_fusion_checkpoint_converts_to_ecapa_and_rawnet2_conv_blobs(tmp_path):
    sd, e, r = _fusion_state("conv")
    dst = tmp_path / "conv.svhip"
    n = checkpoint.convert_checkpoint(sd, dst, "Raw_ECAPA_conv_asp")
    assert n == len(e) + len(r) == 233 + 140
    p_e, p_r = checkpoint.fusion_blob_paths(dst, "Raw_ECAPA_conv_asp")
    mid_e, back_e = checkpoint.read_blob(p_e)
    mid_r, back_r = checkpoint.read_blob(p_r)
    assert (mid_e, mid_r) == (_lib.MODEL_ECAPA, _lib.MODEL_RAWNET2_CONV)
    assert list(back_r) == list(r) and all(np.array_equal(back_r[k], np.asarray(v)) for k, v in r.items())
    # Raw_ECAPA: a sinc RawNet2 blob
    sd_in, _, _ = _fusion_state("sinc")
    checkpoint.convert_checkpoint(sd_in, tmp_path / "in.svhip", "Raw_ECAPA")
    assert checkpoint.read_blob(str(tmp_path / "in.svhip") + ".rawnet2")[0] == _lib.MODEL_RAWNET2
    # a sinc checkpoint is not a conv one
    with pytest.raises(ValueError, match="sinc"):
        checkpoint.convert_checkpoint(sd_in, tmp_path / "x.svhip", "Raw_ECAPA_conv_asp")


def test_conv_module_refuses_a_sinc_blob_pair(tmp_path):
    from speakerverification_amd.models import Raw_ECAPA_conv_asp
    sd, _, _ = _fusion_state("sinc", input_norm=True)
    dst = tmp_path / "sinc.svhip"
    checkpoint.convert_checkpoint(sd, dst, "Raw_ECAPA")
    m = Raw_ECAPA_conv_asp.MainModel(nOut=512, **KW)
    with pytest.raises(ValueError):
        m.load_blob(dst)


def test_input_norm_module_refuses_an_ecapa_blob_without_instance_norm(tmp_path):
    """Raw_ECAPA given the ECAPA branch of a Raw_ECAPA_sinc_asp checkpoint (no instance_norm.*): the library's MISSING error,
    not a forward on the module's initial values"""
    from speakerverification_amd.models import Raw_ECAPA
    sd, _, _ = _fusion_state("sinc", input_norm=False)
    dst = tmp_path / "noin.svhip"
    checkpoint.convert_checkpoint(sd, dst, "Raw_ECAPA_sinc_asp")
    m = Raw_ECAPA.MainModel(nOut=512, **KW)
    with pytest.raises(_lib.SvhipError, match="instance_norm") as ei:
        m.load_blob(dst)
    assert ei.value.code == _lib.ERR_MISSING


def test_checkpoint_help_lists_the_fusion_models(capsys):
    with pytest.raises(SystemExit):
        checkpoint.main(["--help"])
    out = capsys.readouterr().out
    for name in ("Raw_ECAPA_sinc_asp", "Raw_ECAPA", "Raw_ECAPA_conv_asp"):
        assert name in out
        assert name in checkpoint.FUSION_MODELS
