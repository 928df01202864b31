"""GPU parity of TitaNet (s / m / l), Tita_ECAPA and Raw_tita against the outputs of the REFERENCE's own modules in fp32 and float64
(tests/golden/titanet.npz, fusion_tita_ecapa.npz, fusion_raw_tita.npz; tools/make_golden_titanet.py), the stages against a float64
restatement of the network (checked against the fixture first), the depthwise kernel against numpy (no bleed between utterances,
batch-order invariance), the pointwise GEMMs on every route, a NaN utterance, the refusals, the device-tensor path and ModelHandling.

Bars follow test_gpu_rawnet3.py: f32 <= 1e-5 of scale to float64 and <= 1e-4 + (reference fp32 to float64) to the reference's fp32;
bf16 at the shared 16-bit bars (cosine >= 0.999, <= 3e-2 of scale)."""
import os

import numpy as np
import pytest
import torch

from oracle import fbank as o_fbank, titanet as o_titanet
from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.models import Raw_tita, Tita_ECAPA, TitaNet

pytestmark = pytest.mark.gpu

AUDIO_SPEC = dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1)
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="raw", audio_spec=AUDIO_SPEC)
BF16_BARS = (0.999, 3e-2)
SIZES = {"s": 192, "m": 320, "l": 512}
ERR_INVALID, ERR_UNSUPPORTED = -1, -5         # include/svhip.h


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


def _sd(size, seed=1):
    return synth.synth_state_dict(synth.titanet_param_spec(size, SIZES[size]), seed=seed)


def _mel(L, B=2, seed=20220829):
    return o_fbank.melspectrogram(torch.from_numpy(synth.synth_waveforms(B, L, seed=seed))).numpy()


def _engine(size, compute, B, L, sd=None):
    H = synth.TITANET_SIZES[size][0]
    eng = Engine(model="titanet", compute=compute, channels=H, embed_dim=SIZES[size], max_batch=B, samples=L, log_input=False)
    eng.load_state_dict(sd if sd is not None else _sd(size))
    eng.finalize()
    return eng


def _frames(stage, B, T):           # (B T, C) -> (B, C, T)
    return stage.reshape(B, T, -1).transpose(0, 2, 1)


def ref64(sd, mel, size):
    """float64 restatement of TitaNet.forward (TitaNet.py:159-431; oracle/titanet.py, one utterance at a time): returns the stages
    (B, C, T) and the embedding"""
    assert sd["encoder.prolog.conv_block.0.weight"].shape[0] == synth.TITANET_SIZES[size][0]
    t = o_titanet.to_torch_sd(sd)
    last = f"b{o_titanet.n_blocks(t) - 1}_out"
    names = {"tn_prolog": "prolog", "tn_dw0": "b0_dw0", "tn_mega_last": last, "tn_enc": "enc"}
    st, emb = {n: [] for n in list(names) + ["tn_pool"]}, []
    with torch.no_grad():
        for m in torch.from_numpy(mel).double():
            s = {}
            emb.append(o_titanet.forward(m, t, stages=s).numpy())
            for n, k in names.items():
                st[n].append(s[k].numpy().T)                 # (T, C) -> (C, T)
            st["tn_pool"].append(s["pool"].numpy())
    return {n: np.stack(v) for n, v in st.items()}, np.stack(emb)


@pytest.mark.parametrize("size,compute", [("s", "f32"), ("m", "f32"), ("l", "f32"), ("m", "bf16"), ("l", "bf16")])
def test_titanet_matches_reference_at_every_length(golden_dir, size, compute):
    g = np.load(os.path.join(golden_dir, "titanet.npz"))
    B = int(g["B"])
    for L in (int(v) for v in g["lengths"]):
        mel = _mel(L, B, int(g["seed_x"]))
        assert np.allclose(np.array([mel.astype(np.float64).sum(), np.abs(mel).astype(np.float64).sum()]), g[f"{size}_mel_L{L}"][:2], rtol=1e-5)
        eng = _engine(size, compute, B, L, _sd(size, int(g["seed_w"])))
        _check(eng.embed_features(mel), g[f"{size}_out32_L{L}"], g[f"{size}_out64_L{L}"], compute, f"titanet-{size} L={L}")
        if compute == "f32" and L == 512:       # the mel front-end + net path (svhip_embed_wave) at the shortest length
            wav = synth.synth_waveforms(B, L, seed=int(g["seed_x"]))
            _check(eng.embed_wave(wav), g[f"{size}_out32_L{L}"], g[f"{size}_out64_L{L}"], compute, f"titanet-{size} wave L={L}")
        eng.close()


@pytest.mark.parametrize("size,compute", [("m", "f32"), ("l", "f32"), ("m", "bf16")])
def test_titanet_stages_against_float64(golden_dir, size, compute):
    g = np.load(os.path.join(golden_dir, "titanet.npz"))
    B, L = 2, 32000
    sd = _sd(size, int(g["seed_w"]))
    mel = _mel(L, B, int(g["seed_x"]))
    st, emb = ref64(sd, mel, size)
    assert _rel(emb, g[f"{size}_out64_L{L}"]) <= 1e-9                 # the restatement is the reference's arithmetic
    eng = _engine(size, compute, B, L, sd)
    eng.embed_features(mel)
    T = mel.shape[2]
    for name in ("tn_prolog", "tn_dw0", "tn_mega_last", "tn_enc", "tn_pool"):
        got = eng.get_stage(name)
        got = got.reshape(B, -1) if name == "tn_pool" else _frames(got, B, T)
        r = _rel(got, st[name])
        print(f"titanet-{size} {compute} {name}: {r:.2e} of scale")
        assert r <= (2e-5 if compute == "f32" else 3e-2), (name, r)
    eng.close()


def _np_dw(x, w, b):
    """numpy depthwise conv over (B, C, T) with zero 'same' padding per utterance, float64"""
    B, C, T = x.shape
    k = w.shape[-1]
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (k // 2, k // 2)))
    out = np.zeros((B, C, T)) + b[None, :, None]
    for j in range(k):
        out += w[None, :, 0, j, None].astype(np.float64) * xp[:, :, j:j + T]
    return out


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("size", ["s", "m", "l"])
def test_tn_dw_against_numpy_no_bleed(size, compute):
    """tn_dw0 = dw(tn_prolog) + b for B = 3 utterances of different content at L = 32000, an L whose T is below 11 and the shortest L;
    permuting the batch permutes the rows bit-identically; B = 1 agrees with row b of the batch"""
    sd = _sd(size)
    w = sd["encoder.mega_blocks.0.sub_blocks.0.conv_block.0.conv.0.weight"]
    bias = sd["encoder.mega_blocks.0.sub_blocks.0.conv_block.0.conv.0.bias"]
    B = 3
    for L in (32000, 640, 512):
        mel = _mel(L, B, seed=77)
        mel[1] *= 3.0                                          # utterances of different content and scale
        T = mel.shape[2]
        eng = _engine(size, compute, B, L, sd)
        eng.embed_features(mel)
        pro = _frames(eng.get_stage("tn_prolog"), B, T)
        dw = _frames(eng.get_stage("tn_dw0"), B, T)
        want = _np_dw(pro, w, bias)
        terms = _np_dw(np.abs(pro), np.abs(w), np.abs(bias)) + 1e-30       # sum of |w x| + |b|: the scale of the fp32 rounding
        tol = 1e-6 if compute == "f32" else 2 ** -8                         # (bf16: the output's own rounding)
        err = np.abs(dw - want) / terms
        print(f"tn_dw {size} {compute} L={L} T={T}: max rel {err.max():.2e}")
        assert err.max() <= tol
        perm = [2, 0, 1]
        eng.embed_features(np.ascontiguousarray(mel[perm]))
        dwp = _frames(eng.get_stage("tn_dw0"), B, T)
        assert np.array_equal(dwp, dw[perm])
        e1 = _engine(size, compute, 1, L, sd)
        e1.embed_features(np.ascontiguousarray(mel[1:2]))
        d1 = _frames(e1.get_stage("tn_dw0"), 1, T)
        assert _rel(d1[0], dw[1]) <= (1e-5 if compute == "f32" else 3e-2)
        e1.close()
        eng.close()


@pytest.mark.parametrize("compute", ["bf16", "f32"])
def test_pointwise_gemms_on_every_route(compute):
    """TitaNet-M's pointwise GEMMs (N = K = 512) at batch sizes that put M = B T on each route conv_plan picks (bf16: the 256 x 256
    per-tile kernel while the tiles do not outnumber the CUs, the persistent one beyond), plus a capped persistent grid (pw3_cus); the
    first four utterances (the same waveforms at every B) against the float64 restatement; the profile labels name the routes taken"""
    size, L = "m", 32000
    sd = _sd(size)
    _, want = ref64(sd, _mel(L, 4, seed=5), size)
    seen = set()
    for B, cus in [(4, None), (64, None), (160, None), (8, 16)]:
        mel = _mel(L, B, seed=5)
        eng = _engine(size, compute, B, L, sd)
        if cus is not None:
            eng.set_option("pw3_cus", cus)
        eng.profile(True)
        out = np.atleast_2d(eng.embed_features(mel))[:4]
        labels = {k for k in eng.profile_results() if k.startswith("gemm")}
        seen |= labels
        r, cos = _rel(out, want[:len(out)]), float(_cos(out, want[:len(out)]).min())
        print(f"B={B} pw3_cus={cus} {compute}: {sorted(labels)} to float64 {r:.2e}, min cos {cos:.6f}")
        if compute == "f32":
            assert r <= 1e-5
        else:
            assert r <= BF16_BARS[1] and cos >= BF16_BARS[0]
        eng.close()
    print("routes:", sorted(seen))
    if compute == "bf16":
        assert {"gemm_pw3", "gemm_pw2"} <= seen, seen


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_nan_utterance_stays_in_its_row(compute):
    """a NaN in one utterance's mel gives that utterance a NaN embedding (the ReLU epilogues would drop it; tn_in_check restores the
    reference's propagation) and SVHIP_ERR_NONFINITE; the other rows keep their values"""
    size, L, B = "m", 32000, 3
    sd = _sd(size)
    mel = _mel(L, B, seed=9)
    eng = _engine(size, compute, B, L, sd)
    clean = eng.embed_features(mel)
    bad = mel.copy()
    bad[1, 3, 100] = np.nan
    eng.on_numeric = "ignore"
    out = eng.embed_features(bad)
    assert np.isnan(out[1]).all()
    assert np.isfinite(out[[0, 2]]).all()
    # (as on ECAPA handles, a bf16 row moves by round-off with its neighbours' column sums; the fp32 rows do not)
    assert _rel(out[[0, 2]], clean[[0, 2]]) <= (1e-6 if compute == "f32" else BF16_BARS[1])
    eng.on_numeric = "raise"
    with pytest.raises(_lib.SvhipError) as ei:
        eng.embed_features(bad)
    assert ei.value.code == _lib.ERR_NONFINITE
    eng.close()


def test_refusals_at_create_and_finalize():
    def make(**kw):
        a = dict(model="titanet", compute="f32", channels=512, embed_dim=320, max_batch=2, samples=32000, log_input=False)
        a.update(kw)
        return Engine(**a)
    for compute, code in (("f32x3", ERR_UNSUPPORTED), ("f16", ERR_UNSUPPORTED)):
        with pytest.raises(_lib.SvhipError) as ei:
            make(compute=compute)
        assert ei.value.code == code
    for kw in (dict(channels=384), dict(log_input=True), dict(input_norm=True)):
        with pytest.raises(_lib.SvhipError) as ei:
            make(**kw)
        assert ei.value.code == ERR_INVALID
    sd = _sd("m")
    # a depthwise weight of another size's kernel
    eng = make()
    with pytest.raises(_lib.SvhipError) as ei:
        eng.load_state_dict({"encoder.mega_blocks.0.sub_blocks.0.conv_block.0.conv.0.weight": np.zeros((512, 1, 11), np.float32)})
    assert ei.value.code == ERR_INVALID
    eng.close()
    # a gap in the block indices; a missing tensor of a present block; no block at all
    for drop in (lambda k: k.startswith("encoder.mega_blocks.4."), lambda k: k == "encoder.mega_blocks.2.sub_blocks.3.excitation.2.weight",
                 lambda k: k.startswith("encoder.mega_blocks.")):
        eng = make()
        eng.load_state_dict({k: v for k, v in sd.items() if not drop(k)})
        with pytest.raises(_lib.SvhipError) as ei:
            eng.finalize()
        assert ei.value.code == _lib.ERR_MISSING
        eng.close()
    # a user-given block count (the first 3 of 10) is served: the forward runs on 3 blocks
    g3 = {k: v for k, v in sd.items() if not any(k.startswith(f"encoder.mega_blocks.{i}.") for i in range(3, 10))}
    eng = make()
    eng.load_state_dict(g3)
    eng.finalize()
    mel = _mel(32000, 2, seed=3)
    _, want = ref64(g3, mel, "m")
    assert _rel(eng.embed_features(mel), want) <= 1e-5
    eng.close()


FUSION_BRANCHES = {     # tools/make_golden_titanet.py: each branch's own synthetic weights
    Tita_ECAPA: (("ECAPA_TDNN.", lambda: synth.ecapa_param_spec(C=512, input_norm=True)), ("titaNet.", lambda: synth.titanet_param_spec("m", 320))),
    Raw_tita: (("titaNet.", lambda: synth.titanet_param_spec("m", 192)), ("RawNet.", lambda: synth.rawnet2_param_spec(nOut=320))),
}


def _fusion_sd(mod, g):
    sd = {}
    for prefix, spec in FUSION_BRANCHES[mod]:
        sd.update({prefix + k: v for k, v in synth.synth_state_dict(spec(), seed=int(g["seed_w"])).items()})
    return sd


@pytest.mark.parametrize("compute", ["f32", "half"])
@pytest.mark.parametrize("name,mod,fname", [("Tita_ECAPA", Tita_ECAPA, "fusion_tita_ecapa.npz"), ("Raw_tita", Raw_tita, "fusion_raw_tita.npz")])
def test_fusion_matches_reference(golden_dir, name, mod, fname, compute):
    g = np.load(os.path.join(golden_dir, fname))
    model = mod.MainModel(nOut=512, hip_compute=compute, **KW)
    assert sorted(model.state_dict()) == sorted(k for k in g["keys"] if not k.startswith("compute_features."))
    model.load_state_dict(_fusion_sd(mod, g))
    x = synth.synth_waveforms(int(g["B"]), 32000, seed=int(g["seed_x"]))
    out = np.atleast_2d(np.asarray(model(x)))
    ref32, ref64_ = g["out32"], g["out64"]
    r64, r32, own = _rel(out, ref64_), _rel(out, ref32), _rel(ref32, ref64_)
    cos = float(_cos(out, ref64_).min())
    print(f"{name} {compute}: to float64 {r64:.2e}, to fp32 {r32:.2e} (reference fp32 to float64 {own:.2e}), min cos {cos:.7f}")
    assert out.shape == (2, 512)
    if compute == "f32":
        assert r64 <= 1e-4 + own and r32 <= 1e-4 + own
    else:
        assert r64 <= BF16_BARS[1] and cos >= BF16_BARS[0]
    # device-resident batch: both branches concurrently, each on its handle's stream
    xd = torch.from_numpy(x).cuda()
    outd = model(xd).cpu().numpy()
    assert _rel(outd, out) <= 1e-6


def test_titanet_device_tensor_and_model_handling(golden_dir):
    """TitaNet takes CUDA tensors; ModelHandling serves Tita_ECAPA and Raw_tita from a config dict"""
    from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
    from tests.test_gpu_e2e import ARGS
    g = np.load(os.path.join(golden_dir, "titanet.npz"))
    m = TitaNet.MainModel(nOut=320, model_size="m", n_mels=80, device="cuda")
    m.load_state_dict(_sd("m", int(g["seed_w"])))
    mel = _mel(32000, 2, int(g["seed_x"]))
    out = m(torch.from_numpy(mel).cuda())
    assert out.is_cuda
    assert _rel(out.cpu().numpy(), g["m_out64_L32000"]) <= 1e-5
    for name, fname, mod in (("Tita_ECAPA", "fusion_tita_ecapa.npz", Tita_ECAPA), ("Raw_tita", "fusion_raw_tita.npz", Raw_tita)):
        gf = np.load(os.path.join(golden_dir, fname))
        args = dict(ARGS, model={"name": name, "nOut": 512}, features="raw", classifier={"input_size": 512, "out_neurons": 10})
        enc = SpeakerEncoder(**args)
        enc.load_state_dict({"__S__." + k: v for k, v in _fusion_sd(mod, gf).items()})
        x = synth.synth_waveforms(2, 32000, seed=int(gf["seed_x"]))
        o = enc(x)
        o = o.detach().cpu().numpy() if hasattr(o, "detach") else np.asarray(o)
        assert o.shape == (2, 512)
        assert _rel(o, gf["out64"]) <= 1e-4 + _rel(gf["out32"], gf["out64"])
        mh = ModelHandling(WrappedModel(enc), **args)
        emb = mh.embed_utterance(x[0], num_eval=2, normalize=True)
        emb = emb.numpy() if hasattr(emb, "numpy") else np.asarray(emb)
        assert np.isfinite(emb).all()
