"""Host-side checks of RawNet3 and Raw3_ECAPA (the model of the reference's default configs): the parameter spec against the
reference's key list (tests/golden/rawnet3.npz, fusion_raw3_ecapa.npz; tools/make_golden_rawnet3.py), the restated sinc
filterbank against the reference's own cos formula, the C header's model id, the plug-ins' option and input checks, and the
checkpoint conversion with its cross-model refusals.  No GPU."""
import os
import re

import numpy as np
import pytest

from speakerverification_amd import _lib, checkpoint, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw",
          audio_spec=dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1))


def test_spec_matches_the_reference_key_list(golden_dir):
    g = np.load(os.path.join(golden_dir, "rawnet3.npz"))
    spec = synth.rawnet3_param_spec(nOut=320)
    assert [k for k, _ in spec] == list(g["keys"])
    assert len(spec) == 234
    f = np.load(os.path.join(golden_dir, "fusion_raw3_ecapa.npz"))
    want = ["ECAPA_TDNN." + k for k, _ in synth.ecapa_param_spec(C=512, input_norm=True)] + ["rawnet." + k for k, _ in spec]
    assert [k for k in f["keys"] if not k.startswith("compute_features.")] == want


def test_restated_filterbank_matches_the_reference_cos_formula(golden_dir):
    """the cos half of ParamSincFB as restated here == SincConv_fast (RawNet_baseline.py:339-357) on the same band edges; the whole
    bank == the fixture generator's stand-in module"""
    g = np.load(os.path.join(golden_dir, "rawnet3.npz"))
    sd = synth.synth_state_dict(synth.rawnet3_param_spec(nOut=320), seed=int(g["seed_w"]))
    p = "conv1.filterbank."
    f = synth.rawnet3_sinc_filters(sd[p + "low_hz_"], sd[p + "band_hz_"], sd[p + "window_"], sd[p + "n_"])
    assert f.shape == (256, 251)
    # both references run in fp32: sin / cos of arguments up to 2 pi 8000 125 / 16000 = 393 rad carry ~2e-5 absolute error
    assert np.abs(f[:128] - g["sincconv_fast_cos"]).max() <= 3e-5
    assert np.abs(f - g["filters"]).max() <= 3e-5
    assert np.array_equal(f[:, 125], np.r_[np.ones(128), np.zeros(128)])        # centre taps: 2 band / 2 band, and 0
    assert np.allclose(f[:128, :125], f[:128, 250:125:-1])                      # cos filters even, sin filters odd
    assert np.allclose(f[128:, :125], -f[128:, 250:125:-1])


def test_header_model_id_matches_the_binding():
    text = open(os.path.join(ROOT, "include", "svhip.h")).read()
    m = re.search(r"SVHIP_MODEL_RAWNET3\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == _lib.MODEL_RAWNET3 == 4
    assert re.search(r"#define SVHIP_ABI_VERSION 5\b", text)
    assert checkpoint.model_id("RawNet3") == checkpoint.model_id("rawnet3") == 4


def test_unsupported_options_raise():
    from speakerverification_amd.models import RawNet3
    for kw in (dict(encoder_type="ECA"), dict(context=False), dict(summed=False), dict(norm_sinc="mean_std"), dict(model_scale=4),
               dict(out_bn=True), dict(log_sinc=False), dict(sinc_stride=5)):
        with pytest.raises(NotImplementedError):
            RawNet3.MainModel(nOut=320, **kw)
    with pytest.raises(NotImplementedError):
        RawNet3.MainModel(nOut=320, hip_compute="f32x3")
    with pytest.raises(NotImplementedError):
        RawNet3.MainModel(nOut=320, hip_compute="f16")
    m = RawNet3.MainModel(nOut=320, unrelated_option=3, **KW)       # other kwargs are ignored, as in the reference
    assert len(m.state_dict()) == 234 and m.model_kind == "rawnet3"
    assert m.accepts_length(541) and not m.accepts_length(540)
    with pytest.raises(ValueError, match="541"):
        m(np.zeros((2, 540), np.float32))
    assert not m._engines


def test_raw3_ecapa_plugin_holds_the_reference_keys():
    from speakerverification_amd.models import Raw3_ECAPA
    m = Raw3_ECAPA.MainModel(nOut=512, **KW)
    assert m.ECAPA_TDNN.input_norm and m.rawnet.model_kind == "rawnet3" and not hasattr(m, "rawnet2v2")
    sd = m.state_dict()
    assert len(sd) == 233 + 234 and all(k.startswith(("ECAPA_TDNN.", "rawnet.")) for k in sd)
    full = dict(sd)
    full["compute_features.0.flipped_filter"] = np.array([[[-0.97, 1.0]]], np.float32)
    m.load_state_dict(full)
    with pytest.raises(KeyError):
        m.load_state_dict({**full, "rawnet2v2.fc.weight": np.zeros((320, 1024), np.float32)})


def _raw3_state(prefix="__S__."):
    e = synth.synth_state_dict(synth.ecapa_param_spec(C=512, input_norm=True), seed=1)
    r = synth.synth_state_dict(synth.rawnet3_param_spec(nOut=320), seed=1)
    sd = {prefix + "ECAPA_TDNN." + k: v for k, v in e.items()}
    sd.update({prefix + "rawnet." + k: v for k, v in r.items()})
    sd["compute_features.0.flipped_filter"] = np.array([[[-0.97, 1.0]]], np.float32)
    return sd, e, r


def _raw2_state(prefix="__S__."):
    e = synth.synth_state_dict(synth.ecapa_param_spec(C=512, input_norm=True), seed=1)
    r = synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320), seed=1)
    sd = {prefix + "ECAPA_TDNN." + k: v for k, v in e.items()}
    sd.update({prefix + "rawnet2v2." + k: v for k, v in r.items()})
    return sd


def test_raw3_ecapa_checkpoint_converts_to_ecapa_and_rawnet3_blobs(tmp_path):
    sd, e, r = _raw3_state()
    dst = tmp_path / "raw3.svhip"
    n = checkpoint.convert_checkpoint(sd, dst, "Raw3_ECAPA")
    assert n == len(e) + len(r) == 233 + 234
    p_e, p_r = checkpoint.fusion_blob_paths(dst, "Raw3_ECAPA")
    assert p_r.endswith(".rawnet3")
    mid_e, back_e = checkpoint.read_blob(p_e)
    mid_r, back_r = checkpoint.read_blob(p_r)
    assert (mid_e, mid_r) == (_lib.MODEL_ECAPA, _lib.MODEL_RAWNET3)
    assert list(back_r) == list(r) and all(np.array_equal(back_r[k], np.asarray(v)) for k, v in r.items())


def test_cross_model_checkpoints_and_blob_pairs_are_refused(tmp_path):
    from speakerverification_amd.models import Raw3_ECAPA, Raw_ECAPA
    sd3, _, _ = _raw3_state()
    sd2 = _raw2_state()
    with pytest.raises(ValueError, match="rawnet2v2"):
        checkpoint.convert_checkpoint(sd2, tmp_path / "a.svhip", "Raw3_ECAPA")
    with pytest.raises(ValueError, match="rawnet"):
        checkpoint.convert_checkpoint(sd3, tmp_path / "b.svhip", "Raw_ECAPA")
    with pytest.raises(ValueError, match="fusion"):
        checkpoint.convert_checkpoint(sd3, tmp_path / "c.svhip", "RawNet3")
    # blob pairs: a Raw_ECAPA pair into Raw3_ECAPA and the other way round
    checkpoint.convert_checkpoint(sd2, tmp_path / "r2.svhip", "Raw_ECAPA")
    checkpoint.convert_checkpoint(sd3, tmp_path / "r3.svhip", "Raw3_ECAPA")
    with pytest.raises(ValueError):
        Raw3_ECAPA.MainModel(nOut=512, **KW).load_blob(tmp_path / "r2.svhip")
    with pytest.raises(ValueError):
        Raw_ECAPA.MainModel(nOut=512, **KW).load_blob(tmp_path / "r3.svhip")
    # a RawNet3 blob is not a RawNet2 one, nor the other way round
    from speakerverification_amd.models import RawNet2_custom, RawNet3
    with pytest.raises(ValueError):
        RawNet2_custom.MainModel(nOut=320, front_proc="sinc", aggregate="asp", att_dim=128).load_blob(str(tmp_path / "r3.svhip") + ".rawnet3")
    with pytest.raises(ValueError):
        RawNet3.MainModel(nOut=320).load_blob(str(tmp_path / "r2.svhip") + ".rawnet2")


def test_checkpoint_help_lists_raw3_ecapa(capsys):
    with pytest.raises(SystemExit):
        checkpoint.main(["--help"])
    out = capsys.readouterr().out
    assert "Raw3_ECAPA" in out and "RawNet3" in out
