"""GPU parity of the sinc front-end at 8 kHz (tests/golden/rawnet2_sr8000.npz), of the attention-head kernel of Raw_ECAPA_hype on its own
against the float64 restatement (tests/hype_head_oracle.py), and of the whole model against the outputs of the REFERENCE's own module
(tests/golden/fusion_raw_ecapa_hype.npz; tools/make_golden_hype.py)."""
import os

import numpy as np
import pytest

from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.models import Raw_ECAPA_hype, RawNet2_custom
from tests import hype_head_oracle
from tests.test_gpu_fusion_variants import _check, _cos

pytestmark = pytest.mark.gpu

MODELS_8K = {"asp": 320, "gru": 512}


def _spec(sr, L):
    return dict(sample_rate=sr, sentence_len=L / float(sr), win_len=0.025, hop_len=0.01, channels=1)


def _kw(sr, L):
    return dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw", audio_spec=_spec(sr, L))


@pytest.fixture(scope="module")
def g8k(golden_dir):
    return np.load(os.path.join(golden_dir, "rawnet2_sr8000.npz"))


@pytest.fixture(scope="module")
def ghype(golden_dir):
    return np.load(os.path.join(golden_dir, "fusion_raw_ecapa_hype.npz"))


# ---- the sinc front-end at 8 kHz ------------------------------------------------------------------------------------------------------
def _rawnet2(agg, L, compute, sr=8000, weights_sr=8000, seed=1):
    nOut = MODELS_8K[agg]
    m = RawNet2_custom.MainModel(nOut=nOut, front_proc="sinc", aggregate=agg, att_dim=128, audio_spec=_spec(sr, L), hip_compute=compute,
                                 range_fallback=None, embed_batch=4)
    m.load_state_dict(synth.synth_state_dict(synth.rawnet2_param_spec(nOut=nOut, nb_samp=L, aggregate=agg), seed=seed, sample_rate=weights_sr))
    return m


@pytest.mark.parametrize("L", [8000, 16000, 2438])
@pytest.mark.parametrize("compute", ["f32", "f32x3", "f16", "bf16"])
@pytest.mark.parametrize("agg", ["asp", "gru"])
def test_rawnet2_sinc_at_8khz_matches_reference(g8k, agg, compute, L):
    m = _rawnet2(agg, L, compute, seed=int(g8k["seed_w"]))
    x = synth.synth_waveforms(int(g8k["B"]), L, seed=int(g8k["seed_x"]))
    _check(m(x), g8k[f"out_{agg}_{L}"], compute, f"rawnet2 8 kHz {agg} L={L}")


def test_rawnet2_sinc_clamps_band_edges_at_half_the_rate(g8k):
    """the 16 kHz band edges on the 8 kHz model: 33 filters meet the clamp at 4000 Hz, 31 of them start above it"""
    assert int(g8k["clamp_filters"][0]) >= 8
    m = _rawnet2("asp", 16000, "f32", weights_sr=16000, seed=int(g8k["seed_w"]))
    x = synth.synth_waveforms(int(g8k["B"]), 16000, seed=int(g8k["seed_x"]))
    _check(m(x), g8k["out_clamp"], "f32", "rawnet2 8 kHz, 16 kHz band edges")


def test_a_16khz_handle_on_the_same_weights_differs(g8k):
    """a rate that were still hard-coded would make these two equal"""
    x = synth.synth_waveforms(2, 8000, seed=int(g8k["seed_x"]))
    at8 = _rawnet2("asp", 8000, "f32", sr=8000)(x)
    at16 = _rawnet2("asp", 8000, "f32", sr=16000)(x)
    ref = g8k["out_asp_8000"]
    scale = float(np.abs(ref).max())
    assert float(np.abs(at8 - ref).max()) <= 1e-4 * scale
    assert float(np.abs(at16 - at8).max()) > 1e-3 * scale


def test_create_refuses_a_rate_below_the_band_minimum():
    for sr in (-1, 200, 201):
        with pytest.raises(_lib.SvhipError, match="sinc_sr"):
            Engine(model="rawnet2", embed_dim=320, max_batch=1, samples=8000, sinc_sr=sr)
    Engine(model="rawnet2", embed_dim=320, max_batch=1, samples=8000, sinc_sr=0).close()        # 0 means 16000


# ---- the head kernel alone ---------------------------------------------------------------------------------------------------------------
def _head_sd(nOut, seed=3, att3_gain=1.0):
    sd = synth.synth_state_dict(synth.hype_head_param_spec(nOut), seed=seed)
    sd["attention.3.weight"] = (sd["attention.3.weight"] * np.float32(att3_gain)).astype(np.float32)
    return sd


def _head_engine(sd, nOut, max_batch=32):
    eng = Engine(model="fusion_head", channels=704, embed_dim=nOut, max_batch=max_batch, samples=512)
    eng.load_state_dict(sd)
    eng.finalize()
    return eng


@pytest.fixture(scope="module")
def branch_rows(ghype):
    """32 rows of branch outputs: the reference's own (3 cases x 2 utterances), then those rows again plus seeded normal data of 5 % of
    each branch's standard deviation.
    Why not white rows of the branches' scale: the head's logits have magnitude ~55, so fp32 leaves ~2e-5 absolute in them, and the
    output moves by w (1 - w) |x| per unit of logit.  On the reference's own branch outputs one channel holds >= 0.99 of the softmax
    weight and that factor is small: the reference's fp32 head (torch, CPU) is within 1.6e-7 of the float64 restatement there and within
    1.1e-6 on these 32 rows.  On white rows, or perturbations of 20 %, the weight spreads over several channels (1 - max w up to 0.6),
    w (1 - w) |x| reaches ~14 and the reference's own fp32 is 1.04e-5 of the scale away from float64: no fp32 head can carry a 1e-5 bar
    there."""
    o1 = np.concatenate([ghype[f"out1_{int(L)}"] for L in ghype["lengths"]])
    o2 = np.concatenate([ghype[f"out2_{int(L)}"] for L in ghype["lengths"]])
    rng = np.random.Generator(np.random.PCG64(7))
    n = 32 - o1.shape[0]
    base = np.arange(n) % o1.shape[0]
    e1 = np.concatenate([o1, o1[base] + 0.05 * o1.std() * rng.standard_normal((n, 192))]).astype(np.float32)
    e2 = np.concatenate([o2, o2[base] + 0.05 * o2.std() * rng.standard_normal((n, 512))]).astype(np.float32)
    return e1, e2


@pytest.fixture(scope="module", params=[512, 200])
def head(request):
    nOut = request.param
    sd = _head_sd(nOut)
    eng = _head_engine(sd, nOut)
    yield eng, sd, nOut
    eng.close()


@pytest.mark.parametrize("B", [1, 2, 5, 17, 32])
def test_head_kernel_matches_the_float64_oracle(head, branch_rows, B):
    eng, sd, nOut = head
    e1, e2 = branch_rows[0][:B], branch_rows[1][:B]
    eng.profile(True)
    out = eng.fusion_head(e1, e2)
    prof = eng.profile_results()
    eng.profile(False)
    assert prof["hype_head"]["launches"] == 1 and set(prof) == {"hype_head"}          # one launch, nothing else
    ref = hype_head_oracle.head_forward(sd, e1, e2)
    scale = float(np.abs(ref).max())
    err = float(np.abs(out - ref).max())
    print(f"head nOut={nOut} B={B}: max|d| / scale {err / scale:.2e}")
    assert out.shape == (B, nOut) and np.isfinite(out).all() and err <= 1e-5 * scale
    assert eng.numeric_status() == 0


def test_head_device_and_host_pointers_give_the_same_bits(head, branch_rows):
    import torch
    eng, _, nOut = head
    e1, e2 = branch_rows[0][:17], branch_rows[1][:17]
    host = eng.fusion_head(e1, e2)
    dev = eng.fusion_head(torch.from_numpy(e1).cuda(), torch.from_numpy(e2).cuda())
    assert dev.is_cuda and tuple(dev.shape) == (17, nOut)
    assert np.array_equal(dev.cpu().numpy(), host)


def test_head_is_batch_invariant(head, branch_rows):
    """row u of a B = 17 call == the B = 1 call on that row, bit for bit: the first, a middle and the last row (17 = four full tiles
    of utterances and one with a single live row)"""
    eng, _, _ = head
    e1, e2 = branch_rows[0][:17], branch_rows[1][:17]
    full = eng.fusion_head(e1, e2)
    for u in (0, 9, 16):
        alone = eng.fusion_head(e1[u:u + 1], e2[u:u + 1])
        assert np.array_equal(alone[0], full[u]), u
    assert np.array_equal(eng.fusion_head(e1[3:12], e2[3:12]), full[3:12])


def test_head_saturated_softmax_stays_finite(branch_rows):
    """attention.3 scaled by 1e3: one channel takes all the softmax weight.  No tolerance is claimed: under that cancellation the
    reference's own fp32 is only as good as its clamp."""
    sd = _head_sd(512, att3_gain=1e3)
    e1, e2 = branch_rows[0][:5], branch_rows[1][:5]
    _, w = hype_head_oracle.head_forward(sd, e1, e2, return_weights=True)
    assert float(w.max(axis=1).min()) > 0.99                           # (the case is what it says)
    eng = _head_engine(sd, 512)
    out = eng.fusion_head(e1, e2)
    status = eng.numeric_status()
    eng.close()
    assert np.isfinite(out).all() and status == 0


def test_head_reports_a_nan_input_and_keeps_the_other_rows(branch_rows):
    eng = _head_engine(_head_sd(512), 512)
    e1, e2 = branch_rows[0][:6].copy(), branch_rows[1][:6].copy()
    clean = eng.fusion_head(e1, e2)
    e2[2, 100] = np.nan
    out = np.zeros((6, 512), np.float32)
    with pytest.raises(_lib.SvhipNumericError) as ei:                  # the call completes and writes its outputs, then reports
        eng.fusion_head(e1, e2, out=out)
    assert ei.value.code == _lib.ERR_NONFINITE
    assert eng.numeric_status() == 0                                   # reported once, then cleared
    assert np.isnan(out[2]).all()
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(out[keep], clean[keep])
    assert np.array_equal(eng.fusion_head(e1[keep], e2[keep]), clean[keep])
    eng.close()


def test_head_handle_has_no_waveform_forward_and_checks_its_arguments(branch_rows):
    with pytest.raises(_lib.SvhipError, match="704"):
        Engine(model="fusion_head", channels=512, embed_dim=512, max_batch=2, samples=512)
    eng = _head_engine(_head_sd(8), 8, max_batch=2)
    e1, e2 = branch_rows[0], branch_rows[1]
    for call in (lambda: eng.embed_wave(np.zeros((1, 512), np.float32)), lambda: eng.embed_features(np.zeros((1, 80, eng.frames), np.float32))):
        with pytest.raises(_lib.SvhipError) as ei:
            call()
        assert ei.value.code == -5                                     # SVHIP_ERR_UNSUPPORTED
    with pytest.raises(_lib.SvhipError, match="max_batch"):
        eng.fusion_head(e1[:3], e2[:3])
    with pytest.raises(_lib.SvhipError, match="704"):
        eng.fusion_head(e1[:2], e2[:2, :500])
    assert eng.fusion_head(e1[:2], e2[:2]).shape == (2, 8)
    eng.close()
    other = Engine(model="none")
    with pytest.raises(_lib.SvhipError) as ei:
        other.fusion_head(e1[:1], e2[:1])
    assert ei.value.code == -5
    other.close()


# ---- the whole model -------------------------------------------------------------------------------------------------------------------------
def _hype_sd(g, sr, L):
    sd = {"ECAPA_TDNN." + k: v for k, v in
          synth.synth_state_dict(synth.ecapa_param_spec(C=512, input_norm=True), seed=int(g["seed_w_ecapa"])).items()}
    sd.update({"rawnet2v2." + k: v for k, v in
               synth.synth_state_dict(synth.rawnet2_param_spec(nOut=512, nb_samp=L, aggregate="gru"), seed=int(g["seed_w_rawnet2"]),
                                      sample_rate=sr).items()})
    sd.update(synth.synth_state_dict(synth.hype_head_param_spec(512), seed=int(g["seed_w_head"])))
    sd["compute_features.0.flipped_filter"] = np.array([[[-0.97, 1.0]]], np.float32)     # reference checkpoints carry it
    return sd


# 'half' (the ECAPA branch in bf16, the RawNet2 branch in fp16; the head in fp32): the distance to the reference as measured on the first
# GPU run, per case (sample rate, samples): (max error / scale, min cosine).  The bars are three times the error and three times the
# cosine's distance from 1; the outputs are deterministic, the margin covers other seeds.  All three cosines are far above the 0.99
# bf16 bar of the concatenating fusion models: on these weights the softmax over channels is nearly saturated (one channel holds
# >= 0.99 of the weight), so it does not amplify the branches' 16-bit error.
HALF_MEASURED = {(8000, 16000): (8.518e-04, 0.9999996), (8000, 8000): (2.927e-03, 0.9999959), (16000, 32000): (1.621e-03, 0.9999989)}


@pytest.mark.parametrize("sr, L", [(8000, 16000), (8000, 8000), (16000, 32000)])
@pytest.mark.parametrize("compute", ["f32", "f32x3", "half"])
def test_raw_ecapa_hype_matches_reference(ghype, compute, sr, L):
    m = Raw_ECAPA_hype.MainModel(nOut=512, hip_compute=compute, embed_batch=4, **_kw(sr, L))
    sd = _hype_sd(ghype, sr, L)
    m.load_state_dict(sd)
    x = synth.synth_waveforms(int(ghype["B"]), L, seed=int(ghype["seed_x"]))
    ref = ghype[f"out_{L}"]
    out = m(x)
    assert out.shape == ref.shape and np.isfinite(out).all()
    # the head is pinned in every mode: the device's output against the float64 head on the device's OWN branch outputs
    o1, o2 = m.ECAPA_TDNN.embed_wave(x), m.rawnet2v2(x)
    own = hype_head_oracle.head_forward({k: v for k, v in sd.items() if k in dict(synth.hype_head_param_spec(512))}, o1, o2)
    scale = float(np.abs(ref).max())
    err_head = float(np.abs(out - own).max())
    rel = float(np.abs(out - ref).max()) / scale
    cos = float(_cos(out, ref).min())
    print(f"Raw_ECAPA_hype {compute} sr={sr} L={L}: head against its oracle {err_head / scale:.2e}; to the reference max|d| / scale {rel:.3e}, min cos {cos:.7f}")
    assert err_head <= 1e-5 * scale
    if compute != "half":
        _check(out, ref, compute, f"Raw_ECAPA_hype sr={sr} L={L}")
    else:
        rel_m, cos_m = HALF_MEASURED[(sr, L)]
        assert rel <= 3.0 * rel_m and 1.0 - cos <= 3.0 * (1.0 - cos_m), (rel, cos)


def test_hype_blob_and_device_paths_are_bit_identical(ghype, tmp_path):
    """blob triple == state dict; the CUDA two-stream path == the host path; B = 1 gives (512,); more rows than embed_batch run as the
    branches' chunks; a pair converted as Raw_ECAPA_sinc_gru is refused.  (Rows are compared between calls of the same batch size: the
    branches choose kernels by batch size, only the head is batch-invariant.)"""
    import torch
    from speakerverification_amd import checkpoint
    sr, L = 8000, 16000
    sd = _hype_sd(ghype, sr, L)
    dst = tmp_path / "hype.svhip"
    checkpoint.convert_checkpoint({"__S__." + k: v for k, v in sd.items()}, dst, "Raw_ECAPA_hype")
    a = Raw_ECAPA_hype.MainModel(nOut=512, embed_batch=6, hip_compute="half", **_kw(sr, L))
    a.load_state_dict(sd)
    b = Raw_ECAPA_hype.MainModel(nOut=512, embed_batch=6, hip_compute="half", **_kw(sr, L))
    b.load_blob(dst)
    x = synth.synth_waveforms(5, L, seed=L)
    host = a(x)
    assert host.shape == (5, 512) and np.isfinite(host).all()
    assert np.array_equal(b(x), host)
    dev = a(torch.from_numpy(x).cuda())
    assert dev.is_cuda and tuple(dev.shape) == (5, 512)
    assert np.array_equal(dev.cpu().numpy(), host)
    one = a(x[:1])
    assert one.shape == (512,) and np.isfinite(one).all()
    one_dev = a(torch.from_numpy(x[:1]).cuda())
    assert tuple(one_dev.shape) == (512,) and np.array_equal(one_dev.cpu().numpy(), one)
    x13 = np.concatenate([x, x, x[:3]])                                  # more rows than embed_batch = 6: chunks of 6, 6 and 1
    big = a(x13)
    assert big.shape == (13, 512) and np.array_equal(big, np.concatenate([a(x13[:6]), a(x13[6:12]), a(x13[12:])[None]]))
    gru_only = {"__S__." + k: v for k, v in sd.items() if k.startswith(("ECAPA_TDNN.", "rawnet2v2."))}
    checkpoint.convert_checkpoint(gru_only, tmp_path / "gru.svhip", "Raw_ECAPA_sinc_gru")
    with pytest.raises(ValueError, match="Raw_ECAPA_sinc_gru"):
        Raw_ECAPA_hype.MainModel(nOut=512, **_kw(sr, L)).load_blob(tmp_path / "gru.svhip")


def test_speaker_encoder_serves_raw_ecapa_hype():
    from speakerverification_amd.model import SpeakerEncoder
    enc = SpeakerEncoder(model={"name": "Raw_ECAPA_hype", "nOut": 512}, features="raw", n_mels=80, audio_spec=_spec(8000, 16000))
    x = synth.synth_waveforms(3, 16000, seed=21)
    out = enc(x)
    out = out.detach().cpu().numpy() if hasattr(out, "detach") else np.asarray(out)
    assert out.shape == (3, 512) and np.isfinite(out).all()
