"""GPU parity of ResNetSE34V2 against the outputs of the REFERENCE's own module in fp32 and float64 (tests/golden/resnetse34v2.npz;
tools/make_golden_resnetse.py) at every fixture length, option and compute, the named stages against the float64 restatement of
tests/test_resnetse_host.py (checked against the fixture there), the 3 x 3 convolution kernel alone against torch's conv2d in float64
(every (Cin, Cout, stride) of the net, odd and even image sizes down to one output column, no bleed across utterances or rows, a NaN
utterance), batch-order invariance bit for bit, B = 1, and ModelHandling.

Bars are test_gpu_titanet.py's: f32 <= 1e-5 of scale to float64 and <= 1e-4 + (reference fp32 to float64) to the reference's fp32; bf16
cosine >= 0.999 and <= 3e-2 of scale."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.models import ResNetSE34V2
from tests.test_resnetse_host import KW, case_cfg, checksum, load_golden, mel_of, ref64

pytestmark = pytest.mark.gpu

BF16_BARS = (0.999, 3e-2)
ERR_INVALID, ERR_UNSUPPORTED = -1, -5         # include/svhip.h


def _cos(a, b):
    return np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def _rel(out, ref):
    return float(np.abs(out - ref).max()) / float(np.abs(ref).max())


def _check(out, ref32, ref64_, compute, tag):
    out = np.atleast_2d(out)
    assert out.shape == ref32.shape and np.isfinite(out).all()
    r64, r32, own = _rel(out, ref64_), _rel(out, ref32), _rel(ref32, ref64_)
    cos = _cos(out, ref64_)
    print(f"{tag} {compute}: to float64 {r64:.2e}, to fp32 {r32:.2e} (reference fp32 to float64 {own:.2e}), min cos {cos.min():.7f}")
    if compute == "f32":
        assert r64 <= 1e-5, r64
        assert r32 <= 1e-4 + own, (r32, own)
    else:
        c_min, r_max = BF16_BARS
        assert r64 <= r_max and float(cos.min()) >= c_min, (r64, cos)


def _sd(nOut=256, n_mels=80, enc="ASP", seed=1):
    return synth.synth_state_dict(synth.resnetse_param_spec(nOut, n_mels, enc), seed=seed)


def _engine(compute, B, L, sd, features="melspectrogram", enc="ASP", n_mels=80, nOut=256):
    eng = Engine(model="resnetse", compute=compute, channels=1 if enc == "SAP" else 2, n_mels=n_mels, embed_dim=nOut, max_batch=B, samples=L,
                 log_input=features == "melspectrogram", input_norm=True)
    eng.load_state_dict(sd)
    eng.finalize()
    return eng


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["mel_asp_80", "raw_asp_80", "mel_sap_80", "mel_asp_64"])
def test_matches_reference_at_every_length(golden_dir, name, compute):
    g = load_golden(golden_dir)
    features, enc, n_mels = case_cfg(g, name)
    B = int(g["B"])
    sd = _sd(int(g["nOut"]), n_mels, enc, int(g["seed_w"]))
    for L in (int(v) for v in g[f"{name}_lengths"]):
        mel = mel_of(L, n_mels, B, int(g["seed_x"]))
        assert np.allclose(checksum(mel)[:2], g[f"{name}_mel_L{L}"][:2], rtol=1e-5)
        eng = _engine(compute, B, L, sd, features, enc, n_mels)
        out = eng.embed_features(mel)
        _check(out, g[f"{name}_out32_L{L}"], g[f"{name}_out64_L{L}"], compute, f"{name} L={L}")
        if n_mels == 80:              # forward(mel) and embed_wave(wav) agree (the mel front-end + net path)
            wav = synth.synth_waveforms(B, L, seed=int(g["seed_x"]))
            outw = eng.embed_wave(wav)
            _check(outw, g[f"{name}_out32_L{L}"], g[f"{name}_out64_L{L}"], compute, f"{name} wave L={L}")
            assert _rel(outw, out) <= (1e-4 if compute == "f32" else BF16_BARS[1])
        eng.close()


def _nchw(stage, B, P, Q):            # (B P Q, C) channels-last rows -> the reference's (B, C, Q, P)
    return stage.reshape(B, P, Q, -1).transpose(0, 3, 2, 1)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("L", [32000, 640, 512])
def test_stages_against_float64(golden_dir, L, compute):
    g = load_golden(golden_dir)
    B = 2
    sd = _sd(seed=int(g["seed_w"]))
    mel = mel_of(L, 80, B, int(g["seed_x"]))
    st, emb = ref64(sd, mel)
    assert _rel(emb, g[f"mel_asp_80_out64_L{L}"]) <= 1e-9                 # the restatement is the reference's arithmetic
    eng = _engine(compute, B, L, sd)
    eng.embed_features(mel)
    for name in ("rs_stem", "rs_layer1", "rs_layer2", "rs_layer3", "rs_layer4", "rs_pool"):
        got = eng.get_stage(name)
        want = st[name]
        if name == "rs_pool":         # [mean | std] with feature q C + c here, c Q + q in the reference
            C, Q = 256, want.shape[1] // 512
            got = got.reshape(B, 2, Q, C).transpose(0, 1, 3, 2).reshape(B, -1)
        else:
            got = _nchw(got, B, want.shape[3], want.shape[2])
        r = _rel(got, want)
        print(f"L={L} {compute} {name} {want.shape}: {r:.2e} of scale")
        assert got.shape == want.shape and r <= (1e-5 if compute == "f32" else 3e-2), (name, r)
    eng.close()


CONV_SHAPES = [(32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1)]
IMAGES = [(5, 7), (8, 6), (3, 2), (2, 3), (1, 1), (17, 33), (2, 1)]          # (H, W): odd and even; W = 2 / 1 (one output column at stride 2)


def _conv(x_nchw, w, scale, shift, compute, stride, relu_in, relu_out):
    """x (B, C, H, W) float32 host -> y (B, Cout, Ho, Wo) float32 host through svhip_resnetse_conv3x3 (P = W, Q = H)"""
    lib = _lib.load()
    B, Cin, H, W = x_nchw.shape
    Cout = w.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dtype = torch.float32 if compute == "f32" else torch.bfloat16
    xd = torch.from_numpy(np.ascontiguousarray(x_nchw.transpose(0, 3, 2, 1))).cuda().to(dtype).contiguous()
    yd = torch.full((B, Wo, Ho, Cout), 12345.0, device="cuda", dtype=dtype)
    sc, sh = torch.from_numpy(scale).cuda(), torch.from_numpy(shift).cuda()
    wc = np.ascontiguousarray(w, dtype=np.float32)
    torch.cuda.synchronize()
    rc = lib.svhip_resnetse_conv3x3(xd.data_ptr(), wc.ctypes.data, sc.data_ptr(), sh.data_ptr(), yd.data_ptr(), _lib.F32 if compute == "f32" else _lib.BF16,
                                    B, W, H, Cin, Cout, stride, int(relu_in), int(relu_out), None)
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return yd.float().cpu().numpy().transpose(0, 3, 2, 1), xd.float().cpu().numpy().transpose(0, 3, 2, 1)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("cin,cout,stride", CONV_SHAPES)
def test_rs_conv3x3_alone_against_conv2d(cin, cout, stride, compute):
    """every (Cin, Cout, stride) of the net at odd and even image sizes; the neighbours of utterance 1 are filled with large values and
    utterance 1 alone must give the same values (no bleed across utterances or rows); both ReLU switches"""
    rng = np.random.default_rng(cin * 7 + cout + stride)
    w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    for (H, W) in IMAGES:
        for relu_in, relu_out in ((True, True), (False, False)):
            x = rng.standard_normal((3, cin, H, W)).astype(np.float32)
            x[0] *= 1e4
            x[2] *= 1e4
            got, xq = _conv(x, w, scale, shift, compute, stride, relu_in, relu_out)
            wq = torch.from_numpy(w).to(torch.bfloat16).float().numpy() if compute == "bf16" else w     # the operands the kernel reads
            xin = torch.from_numpy(xq).double()
            if relu_in:
                xin = F.relu(xin)
            ref = F.conv2d(xin, torch.from_numpy(wq).double(), stride=stride, padding=1)
            ref = ref * torch.from_numpy(scale).double()[None, :, None, None] + torch.from_numpy(shift).double()[None, :, None, None]
            if relu_out:
                ref = F.relu(ref)
            ref = ref.numpy()
            assert got.shape == ref.shape
            # per utterance: its own scale (the neighbours are 1e4 times larger); bf16: the output's own rounding
            tol = 1e-5 if compute == "f32" else 2 ** -7
            for b in range(3):
                r = float(np.abs(got[b] - ref[b]).max()) / max(float(np.abs(ref[b]).max()), 1e-30)
                assert r <= tol, (H, W, relu_in, b, r)
            one, _ = _conv(x[1:2], w, scale, shift, compute, stride, relu_in, relu_out)
            assert np.array_equal(one[0], got[1]), (H, W)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_rs_conv3x3_nan_stays_in_its_utterance(compute):
    rng = np.random.default_rng(3)
    cin, cout = 64, 64
    w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    scale, shift = np.ones(cout, np.float32), np.zeros(cout, np.float32)
    x = rng.standard_normal((3, cin, 9, 12)).astype(np.float32)
    clean, _ = _conv(x, w, scale, shift, compute, 1, True, True)
    bad = x.copy()
    bad[1, 5, 4, 6] = np.nan
    got, _ = _conv(bad, w, scale, shift, compute, 1, True, True)
    assert np.array_equal(got[[0, 2]], clean[[0, 2]])
    assert np.isnan(got[1, :, 3:6, 5:8]).all()               # the 3 x 3 neighbourhood of the NaN, every output channel
    mask = np.ones(got[1].shape, bool)
    mask[:, 3:6, 5:8] = False
    assert np.array_equal(got[1][mask], clean[1][mask])


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_batch_order_invariance_and_single_utterance(compute):
    """permuting the batch permutes the embeddings and the stage outputs bit for bit; B = 1 returns (1, nOut)"""
    L, B = 32000, 3
    sd = _sd()
    mel = mel_of(L, 80, B, seed=77)
    mel[1] *= 3.0
    eng = _engine(compute, B, L, sd)
    out = eng.embed_features(mel).copy()
    l4 = eng.get_stage("rs_layer4").reshape(B, -1).copy()
    perm = [2, 0, 1]
    outp = eng.embed_features(np.ascontiguousarray(mel[perm]))
    assert np.array_equal(outp, out[perm])
    assert np.array_equal(eng.get_stage("rs_layer4").reshape(B, -1), l4[perm])
    eng.close()
    m = ResNetSE34V2.MainModel(nOut=256, hip_compute=compute, device="cuda", **KW)
    m.load_state_dict(sd)
    one = m(mel[1:2])
    assert tuple(one.shape) == (1, 256)
    assert _rel(np.asarray(one), out[1:2]) <= (1e-5 if compute == "f32" else BF16_BARS[1])


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_nan_utterance_stays_in_its_row(compute):
    L, B = 32000, 3
    sd = _sd()
    mel = mel_of(L, 80, B, seed=9)
    eng = _engine(compute, B, L, sd)
    clean = eng.embed_features(mel).copy()
    bad = mel.copy()
    bad[1, 3, 100] = np.nan
    eng.on_numeric = "ignore"
    out = eng.embed_features(bad)
    assert np.isnan(out[1]).all()
    assert np.array_equal(out[[0, 2]], clean[[0, 2]])
    eng.on_numeric = "raise"
    with pytest.raises(_lib.SvhipError) as ei:
        eng.embed_features(bad)
    assert ei.value.code == _lib.ERR_NONFINITE
    eng.close()


def test_refusals_at_create():
    def make(**kw):
        a = dict(model="resnetse", compute="f32", channels=2, embed_dim=256, max_batch=2, samples=32000, log_input=True, input_norm=True)
        a.update(kw)
        return Engine(**a)
    for compute in ("f32x3", "f16"):
        with pytest.raises(_lib.SvhipError) as ei:
            make(compute=compute)
        assert ei.value.code == ERR_UNSUPPORTED
    for kw in (dict(channels=3), dict(input_norm=False), dict(n_mels=30)):
        with pytest.raises(_lib.SvhipError) as ei:
            make(**kw)
        assert ei.value.code == ERR_INVALID
    eng = make()
    sd = _sd()
    eng.load_state_dict({k: v for k, v in sd.items() if k != "layer3.0.downsample.0.weight"})
    with pytest.raises(_lib.SvhipError) as ei:
        eng.finalize()
    assert ei.value.code == _lib.ERR_MISSING
    eng.close()


def test_device_tensor_blob_and_model_handling(golden_dir, tmp_path):
    """the plug-in takes CUDA tensors and .svhip blobs; ModelHandling serves ResNetSE34V2 from a config dict"""
    from speakerverification_amd import checkpoint
    from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
    from tests.test_gpu_e2e import ARGS
    g = load_golden(golden_dir)
    sd = _sd(seed=int(g["seed_w"]))
    m = ResNetSE34V2.MainModel(nOut=256, device="cuda", **KW)
    path = str(tmp_path / "r.svhip")
    checkpoint.convert_checkpoint({"__S__." + k: v for k, v in sd.items()}, path, "ResNetSE34V2")
    m.load_blob(path)
    mel = mel_of(32000, 80, 2, int(g["seed_x"]))
    out = m(torch.from_numpy(mel).cuda())
    assert out.is_cuda
    assert _rel(out.cpu().numpy(), g["mel_asp_80_out64_L32000"]) <= 1e-5
    args = dict(ARGS, model={"name": "ResNetSE34V2", "nOut": 256}, features="melspectrogram", classifier={"input_size": 256, "out_neurons": 10},
                augment=False, augment_options={"augment_chain": []})
    enc = SpeakerEncoder(**args)
    enc.load_state_dict({"__S__." + k: v for k, v in sd.items()})
    x = synth.synth_waveforms(2, 32000, seed=int(g["seed_x"]))
    o = enc(x)
    o = o.detach().cpu().numpy() if hasattr(o, "detach") else np.asarray(o)
    assert o.shape == (2, 256)
    assert _rel(o, g["mel_asp_80_out64_L32000"]) <= 1e-4 + _rel(g["mel_asp_80_out32_L32000"], g["mel_asp_80_out64_L32000"])
    mh = ModelHandling(WrappedModel(enc), **args)
    emb = mh.embed_utterance(x[0], num_eval=2, normalize=True)
    emb = emb.numpy() if hasattr(emb, "numpy") else np.asarray(emb)
    assert emb.shape[-1] == 256 and np.isfinite(emb).all()
