"""GPU: ragged ResNetSE34V2 packs (svhip_resnetse_embed_ragged) — utterances of different lengths in one call of one handle.

The packed 3 x 3 convolution alone against the fixed kernel per utterance, bit for bit, with a sentinel around the pack's rows; the
lengths of tests/golden/resnetse34v2.npz and more in ONE features call and ONE wave call against the reference's fp32 and float64
embeddings and the stages against the float64 restatement, at the bars of tests/test_gpu_resnetse.py (imported, not restated); batch
invariance bit for bit, and the stages bit for bit against the fixed-length handle of the utterance's own length at B = 1; a NaN
utterance; six asynchronous calls; refusals on a real handle; the fixed-length call of a handle before and after a ragged one; the
plug-in and whole-file evaluation.

Where the ragged EMBEDDING is compared with the fixed-length one (the attention convolutions take different GEMM kernels, so not bit for
bit) the f32 bar is 2e-5 of scale: each forward is held to 1e-5 of scale against float64 (test_gpu_resnetse.py for the fixed one, test 2
here for the ragged one), so two passing forwards differ by at most the sum.  bf16 keeps its own bar (cosine >= 0.999, <= 3e-2 of scale).

All handles are small (max_batch <= 8 at 3200 samples, T = 41 frames) but the plug-in ones, which take the 2 s primary geometry."""
import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, synth
from speakerverification_amd.models import ResNetSE34V2
from tests.ragged_ring_check import check_async_ring
from tests.test_gpu_resnetse import BF16_BARS, ERR_INVALID, ERR_UNSUPPORTED, _check, _cos, _engine, _rel, _sd
from tests.test_resnetse_host import KW, case_cfg, load_golden, mel_of, ref64

pytestmark = pytest.mark.gpu

STAGES = ("rs_stem", "rs_layer1", "rs_layer2", "rs_layer3", "rs_layer4")
SMALL_L = 3200                                  # T = 41
_REF = {}


def _ref(key, sd_args, mel, **kw):
    """ref64 of one (n_mels, T) mel block alone, computed once per key and shared (never written to): (stages, embedding (nOut,))"""
    if key not in _REF:
        st, emb = ref64(_sd(*sd_args), mel[None], **kw)
        _REF[key] = ({k: v[0] for k, v in st.items()}, emb[0])
    return _REF[key]


def _close(a, b, compute, tag):
    """the ragged forward against the fixed-length one (module docstring)"""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    r, c = _rel(a, b), float(_cos(a.astype(np.float64), b.astype(np.float64)).min())
    print(f"{tag} {compute}: {r:.2e} of scale, min cos {c:.7f}")
    if compute == "f32":
        assert r <= 2e-5, (tag, r)
    else:
        assert c >= BF16_BARS[0] and r <= BF16_BARS[1], (tag, r, c)


def _levels(T):
    out = [T]
    for _ in range(3):
        out.append((out[-1] - 1) // 2 + 1)
    return out


def _stages(e, Ts, n_mels=80):
    """the packed stages of the handle's last (ragged) forward, one {stage: (P, Q, C) array} dict per utterance, rs_pool (2 F,)"""
    lv = np.array([_levels(T) for T in Ts])                     # (n, 4)
    row0 = np.concatenate([np.zeros((1, 4), int), np.cumsum(lv, 0)])
    pool = e.get_stage("rs_pool")
    pool = pool.reshape(len(Ts), -1)
    out = [dict(rs_pool=pool[u].copy()) for u in range(len(Ts))]
    for k, name in enumerate(STAGES):
        l = max(k - 1, 0)
        Q, C = n_mels >> l, (32, 32, 64, 128, 256)[k]
        a = e.get_stage(name)
        assert a.size == row0[-1, l] * Q * C, (name, a.size, row0[-1, l], Q, C)
        a = a.reshape(row0[-1, l], Q, C)
        for u in range(len(Ts)):
            out[u][name] = a[row0[u, l]:row0[u + 1, l]].copy()
    return out


def _stage_as_reference(name, got, sap=False):
    """(P, Q, C) -> the reference's (C, Q, P); rs_pool [mean | std] with feature q C + c here -> c Q + q"""
    if name != "rs_pool":
        return got.transpose(2, 1, 0)
    C = 256
    Q = got.size // (2 * C)
    got = got.reshape(2, Q, C).transpose(0, 2, 1)
    return got[0].reshape(-1) if sap else got.reshape(-1)


def _features(T, seed, n_mels=80):
    """a seeded (n_mels, T) mel-power block"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_mels, T)) ** 2 + 1e-3).astype(np.float32)


def _samples(T):
    """a waveform length with T mel frames (any L with L // 80 + 1 == T and L >= 512)"""
    return (T - 1) * 80 if (T - 1) * 80 >= 512 else T * 80 - 1


# ---- 1. the packed convolution alone -------------------------------------------------------------------------------------------------
CONV_P = (1, 2, 3, 8, 17, 41)          # one output column at stride 2, odd and even, more than one tile along P
SENTINEL = 12288.0                              # (exact in bf16)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("Q", [5, 10])
@pytest.mark.parametrize("cin,cout,stride", [(32, 32, 1), (32, 64, 2), (128, 256, 2), (256, 256, 1)])
def test_packed_conv_is_the_fixed_kernel_per_utterance(cin, cout, stride, Q, compute):
    lib = _lib.load()
    dtype = torch.float32 if compute == "f32" else torch.bfloat16
    code = _lib.F32 if compute == "f32" else _lib.BF16
    rng = np.random.default_rng(cin * 7 + cout + stride + Q)
    w = np.ascontiguousarray((rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32))
    sc = torch.from_numpy(rng.uniform(0.5, 1.5, cout).astype(np.float32)).cuda()
    sh = torch.from_numpy((0.1 * rng.standard_normal(cout)).astype(np.float32)).cuda()
    Po = [(P - 1) // stride + 1 for P in CONV_P]
    Qo = (Q - 1) // stride + 1
    rin, rout = np.concatenate([[0], np.cumsum(CONV_P)]), np.concatenate([[0], np.cumsum(Po)])
    x = torch.from_numpy(rng.standard_normal((rin[-1], Q, cin)).astype(np.float32)).cuda().to(dtype).contiguous()
    P_host = np.array(CONV_P, np.int32)
    for relu_in, relu_out in ((1, 1), (0, 0)):
        guard = 3                                                        # sentinel rows past the pack's last row
        y = torch.full((rout[-1] + guard, Qo, cout), SENTINEL, device="cuda", dtype=dtype)
        torch.cuda.synchronize()
        rc = lib.svhip_resnetse_conv3x3_ragged(x.data_ptr(), w.ctypes.data, sc.data_ptr(), sh.data_ptr(), y.data_ptr(), code, P_host.ctypes.data,
                                               len(CONV_P), Q, cin, cout, stride, relu_in, relu_out, None)
        assert rc == _lib.OK, rc
        got = y.float().cpu().numpy()
        assert np.all(got[rout[-1]:] == SENTINEL)                        # nothing past the pack's rows
        assert np.isfinite(got[:rout[-1]]).all() and not np.any(got[:rout[-1]] == SENTINEL)
        for u, P in enumerate(CONV_P):
            xu = x[rin[u]:rin[u + 1]].contiguous()
            yu = torch.full((Po[u], Qo, cout), SENTINEL, device="cuda", dtype=dtype)
            torch.cuda.synchronize()
            rc = lib.svhip_resnetse_conv3x3(xu.data_ptr(), w.ctypes.data, sc.data_ptr(), sh.data_ptr(), yu.data_ptr(), code, 1, P, Q, cin, cout, stride,
                                            relu_in, relu_out, None)
            assert rc == _lib.OK, rc
            want = yu.float().cpu().numpy()
            assert np.array_equal(got[rout[u]:rout[u + 1]], want), (compute, cin, cout, stride, Q, P, relu_in,
                                                                    float(np.abs(got[rout[u]:rout[u + 1]] - want).max()))


# ---- 2. the golden lengths in one call, and the stages ------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_golden_lengths_in_one_call(golden_dir, compute):
    """features: the fixture's 640- and 512-sample utterances (T = 9, 7), T = 41 and 23, and T = 2 and 3 (P_4 = 1) in one call of a
    max_batch = 8 handle; waves: 640, 512, 3200 and 1760 samples in one call.  Every utterance against ref64 on its own mel; the fixture's
    lengths also against its out32 / out64; every stage of every utterance of the features call at the bars of test_stages_against_float64"""
    g = load_golden(golden_dir)
    B, seed_x, seed_w, nOut = int(g["B"]), int(g["seed_x"]), int(g["seed_w"]), int(g["nOut"])
    sd_args = (nOut, 80, "ASP", seed_w)
    mels = {L: mel_of(L, 80, B, seed_x) for L in (640, 512, 3200, 1760)}
    assert [mels[L].shape[2] for L in (640, 512, 3200, 1760)] == [9, 7, 41, 23] and B == 2
    feats = [mels[640][0], mels[640][1], mels[512][0], mels[512][1], mels[3200][0], mels[1760][1],
             np.ascontiguousarray(mels[3200][1][:, :2]), np.ascontiguousarray(mels[1760][0][:, 5:8])]
    keys = [("g", 640, 0), ("g", 640, 1), ("g", 512, 0), ("g", 512, 1), ("g", 3200, 0), ("g", 1760, 1), ("g", "T2"), ("g", "T3")]
    Ts = [f.shape[1] for f in feats]
    assert Ts == [9, 9, 7, 7, 41, 23, 2, 3]
    eng = _engine(compute, 8, SMALL_L, _sd(*sd_args))
    assert eng.ragged_check(Ts, is_wave=False) is None
    emb = eng.embed_features_ragged(feats)
    S = _stages(eng, Ts)
    assert np.array_equal(eng.get_stage("mel").reshape(-1)[:feats[0].size], feats[0].reshape(-1))      # the packed blocks
    for i, L in enumerate((640, 512)):
        _check(emb[2 * i:2 * i + 2], g[f"mel_asp_80_out32_L{L}"], g[f"mel_asp_80_out64_L{L}"], compute, f"ragged features L={L}")
    for u, (key, f) in enumerate(zip(keys, feats)):
        st, e64 = _ref(key, sd_args, f)
        if key[1] in (640, 512):
            assert _rel(e64, g[f"mel_asp_80_out64_L{key[1]}"][key[2]]) <= 1e-9        # the restatement is the reference's arithmetic
        _check(emb[u], e64[None], e64[None], compute, f"ragged features T={Ts[u]} alone in float64")
        for name in STAGES + ("rs_pool",):
            got = _stage_as_reference(name, S[u][name])
            r = _rel(got, st[name])
            print(f"ragged T={Ts[u]} {compute} {name} {st[name].shape}: {r:.2e} of scale")
            assert got.shape == st[name].shape and r <= (1e-5 if compute == "f32" else 3e-2), (Ts[u], name, r)
    # one wave call: the mel front-end of every utterance, then the same forward
    wavs = [w for L in (640, 512, 3200, 1760) for w in synth.synth_waveforms(B, L, seed=seed_x)]
    assert eng.ragged_check([len(w) for w in wavs]) is None
    emb_w = eng.embed_wave_ragged(wavs)
    for i, L in enumerate((640, 512, 3200, 1760)):
        if L in (640, 512):
            _check(emb_w[2 * i:2 * i + 2], g[f"mel_asp_80_out32_L{L}"], g[f"mel_asp_80_out64_L{L}"], compute, f"ragged wave L={L}")
        for b in range(B):
            _, e64 = _ref(("g", L, b), sd_args, mels[L][b])
            _check(emb_w[2 * i + b], e64[None], e64[None], compute, f"ragged wave L={L} utterance {b} in float64")
    eng.close()


@pytest.mark.parametrize("name", ["mel_sap_80", "mel_asp_64"])
def test_sap_and_64_mels_once_each(golden_dir, name):
    g = load_golden(golden_dir)
    features, enc, n_mels = case_cfg(g, name)
    B, seed_x, seed_w, nOut = int(g["B"]), int(g["seed_x"]), int(g["seed_w"]), int(g["nOut"])
    L = 640 if name == "mel_sap_80" else 512
    mel = mel_of(L, n_mels, B, seed_x)
    other = np.ascontiguousarray(mel_of(1760, n_mels, 1, seed_x)[0][:, :19])
    feats = [mel[0], other, mel[1], np.ascontiguousarray(other[:, :2])]
    eng = _engine("f32", 4, SMALL_L, _sd(nOut, n_mels, enc, seed_w), features, enc, n_mels)
    emb = eng.embed_features_ragged(feats)
    _check(emb[[0, 2]], g[f"{name}_out32_L{L}"], g[f"{name}_out64_L{L}"], "f32", f"ragged {name} L={L}")
    S = _stages(eng, [f.shape[1] for f in feats], n_mels)
    for u in (1, 3):
        st, e64 = _ref((name, u), (nOut, n_mels, enc, seed_w), feats[u], features=features, encoder_type=enc)
        _check(emb[u], e64[None], e64[None], "f32", f"ragged {name} T={feats[u].shape[1]} in float64")
        got = _stage_as_reference("rs_pool", S[u]["rs_pool"], sap=enc == "SAP")
        assert got.shape == st["rs_pool"].shape and _rel(got, st["rs_pool"]) <= 1e-5
    eng.close()


# ---- 3. batch invariance, and the fixed-length handle of the utterance's own length ---------------------------------------------------
INV_T = (2, 7, 18, 41)                         # counted 8 + 8 + 24 + 48 = 88 of 164 rows


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_batch_invariance_bit_for_bit_and_the_fixed_length_handle(compute):
    feats = [_features(T, 100 + T) for T in INV_T]
    n = len(INV_T)
    sd = _sd()
    eng = _engine(compute, 4, SMALL_L, sd)

    def run(e, idx):
        emb = e.embed_features_ragged([feats[i] for i in idx])
        assert np.isfinite(emb).all()
        S = _stages(e, [INV_T[i] for i in idx])
        return {i: dict(S[k], emb=emb[k].copy()) for k, i in enumerate(idx)}

    ref = run(eng, range(n))
    arrangements = {"reversed": [run(eng, range(n)[::-1])], "alone": [run(eng, [i]) for i in range(n)], "permuted": [run(eng, [2, 0, 3, 1])],
                    "two calls": [run(eng, [3, 0]), run(eng, [1, 2])]}
    eng.close()
    other = _engine(compute, 6, 4000, sd)                                 # another max_batch and another primary length
    arrangements["another handle"] = [run(other, [1, 3, 0, 2])]
    other.close()
    for name, parts in arrangements.items():
        got = {i: s for part in parts for i, s in part.items()}
        assert sorted(got) == list(range(n))
        for i in got:
            for st in ref[i]:
                assert np.array_equal(got[i][st], ref[i][st]), (compute, name, INV_T[i], st, float(np.abs(got[i][st] - ref[i][st]).max()))
    for i, T in enumerate(INV_T):
        if T < 7:
            continue                                                      # (a fixed-length handle takes at least one FFT window)
        one = _engine(compute, 1, _samples(T), sd)
        emb1 = one.embed_features(feats[i][None])
        for k, name in enumerate(STAGES):
            fixed = one.get_stage(name).reshape(ref[i][name].shape)
            assert np.array_equal(fixed, ref[i][name]), (compute, T, name, float(np.abs(fixed - ref[i][name]).max()))
        _close(ref[i]["emb"], emb1, compute, f"ragged vs fixed T={T}")
        one.close()


# ---- 4. a non-finite input -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_a_nonfinite_input_stays_in_its_utterance(compute):
    eng = _engine(compute, 3, SMALL_L, _sd())
    wavs = [synth.synth_waveforms(1, L, seed=60 + L)[0] for L in (3200, 800, 2000)]
    feats = [_features(T, 70 + T) for T in (26, 9, 41)]
    for name, items, fn, is_wave in (("wave", wavs, eng.embed_wave_ragged, 1), ("features", feats, eng.embed_features_ragged, 0)):
        eng.on_numeric = "raise"
        clean = fn(items).copy()
        assert eng.numeric_status() == 0 and np.isfinite(clean).all()
        bad = [a.copy() for a in items]
        bad[1][..., 5] = np.nan
        packed, offs, lens = eng._pack(bad, None, None, bool(is_wave))
        got = np.empty_like(clean)
        rc = eng.lib.svhip_resnetse_embed_ragged(eng.h, packed.ctypes.data, offs.ctypes.data, lens.ctypes.data, 3, got.ctypes.data, 0, is_wave)
        assert rc == _lib.ERR_NONFINITE, (name, rc, eng.lib.svhip_last_error(eng.h))
        assert np.isnan(got[1]).all(), name
        assert np.array_equal(got[[0, 2]], clean[[0, 2]]), name
        with pytest.raises(_lib.SvhipError) as ei:
            fn(bad)
        assert ei.value.code == _lib.ERR_NONFINITE
        eng.on_numeric = "ignore"
        out = fn(bad)
        assert np.isnan(out[1]).all() and np.array_equal(out[[0, 2]], clean[[0, 2]]), name
        eng.on_numeric = "raise"
        assert np.array_equal(fn(items), clean), name
    eng.close()


# ---- 5. more asynchronous calls in flight than table slots ---------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_six_async_calls_wrap_the_table_slot_ring(compute):
    """six SVHIP_ASYNC calls in flight over the four pinned table slots of the handle (tests/ragged_ring_check.py)"""
    eng = _engine(compute, 3, SMALL_L, _sd())                            # 123 rows
    Ls = [(600, 1500), (2000, 512, 900), (1200, 1000), (800, 700, 1600), (2000, 1700), (900, 1500, 640)]
    check_async_ring(eng, [[synth.synth_waveforms(1, L, seed=300 + 10 * k + i)[0] for i, L in enumerate(ls)] for k, ls in enumerate(Ls)])
    eng.close()


# ---- 6. refusals on a real handle ----------------------------------------------------------------------------------------------------
def test_gpu_handle_refuses_bad_packs_and_keeps_working():
    """the capacity rules on a real handle (the host checks of svhip_resnetse_ragged_check: nothing is enqueued); the good call
    afterwards returns the same bits; the other models' calls keep refusing a ResNetSE handle"""
    eng = _engine("f32", 3, SMALL_L, _sd())                               # 123 rows
    good = [_features(T, 500 + T) for T in (41, 2, 57)]                   # counted 48 + 8 + 64 = 120
    first = eng.embed_features_ragged(good).copy()
    assert np.isfinite(first).all()
    wav = synth.synth_waveforms(1, SMALL_L, seed=8)[0]
    cases = [("too many utterances", lambda: eng.embed_features_ragged([_features(5, i) for i in range(4)]), "4 utterances"),
             ("too many frames as counted", lambda: eng.embed_features_ragged([_features(T, 600 + T) for T in (41, 2, 65)]), "123"),
             ("one frame", lambda: eng.embed_features_ragged([_features(41, 1), _features(1, 2)]), "fewer than 2"),
             ("a too-short wave", lambda: eng.embed_wave_ragged([wav, wav[:511]]), "n_fft=512")]
    for name, call, text in cases:
        with pytest.raises(_lib.SvhipError) as ei:
            call()
        assert ei.value.code == ERR_INVALID and text in str(ei.value), (name, str(ei.value))
    packed, offs, lens = eng._pack([wav], None, None, True)
    out = np.empty((1, eng.embed_dim), np.float32)
    neg = np.array([-1], np.int64)
    rc = eng.lib.svhip_resnetse_embed_ragged(eng.h, packed.ctypes.data, neg.ctypes.data, lens.ctypes.data, 1, out.ctypes.data, 0, 1)
    assert rc == ERR_INVALID and "negative offset" in eng.lib.svhip_last_error(eng.h).decode()
    for export, tail in (("svhip_embed_wave_ragged", ()), ("svhip_rawnet3_embed_ragged", ()), ("svhip_rawnet2_embed_ragged", ()),
                         ("svhip_conformer_embed_ragged", (1,)), ("svhip_titanet_embed_ragged", (1,))):
        rc = getattr(eng.lib, export)(eng.h, packed.ctypes.data, offs.ctypes.data, lens.ctypes.data, 1, out.ctypes.data, 0, *tail)
        assert rc == ERR_UNSUPPORTED, export
    assert np.array_equal(eng.embed_features_ragged(good), first)
    eng.close()


# ---- 7. the fixed-length call of the same handle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_fixed_length_call_unchanged_by_a_ragged_call(compute):
    eng = _engine(compute, 3, SMALL_L, _sd())
    mel = mel_of(SMALL_L, 80, 3, seed=13)
    before = eng.embed_features(mel).copy()
    st_before = {n: eng.get_stage(n).copy() for n in STAGES + ("rs_pool",)}
    eng.embed_features_ragged([_features(T, T) for T in (50, 2, 33)])
    assert eng.get_stage("rs_layer1").size == (50 + 2 + 33) * 80 * 32 and eng.get_stage("rs_layer4").size == (7 + 1 + 5) * 10 * 256
    after = eng.embed_features(mel)
    assert np.array_equal(before, after)
    for n in st_before:
        assert np.array_equal(st_before[n], eng.get_stage(n)), n
    assert eng.get_stage("rs_layer4").size == 3 * 6 * 10 * 256
    eng.close()


# ---- 8. the plug-in and whole-file evaluation ----------------------------------------------------------------------------------------
PLUG_L = (32000, 600, 48000, 20000, 41000)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_plugin_embed_ragged_numpy_and_cuda(compute):
    m = ResNetSE34V2.MainModel(nOut=256, device="cuda", compute=compute, max_batch=4, **KW)
    m.load_state_dict(_sd())
    wavs = [synth.synth_waveforms(1, L, seed=40 + i)[0] for i, L in enumerate(PLUG_L)]
    host = m.embed_ragged(wavs)
    dev = m.embed_ragged([torch.from_numpy(w).cuda() for w in wavs])
    assert host.shape == (5, 256) and np.isfinite(host).all() and dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
    assert len(m._engines) == 1
    for i in (1, 3):
        _close(host[i], np.atleast_2d(m.embed_wave(wavs[i][None]))[0], compute, f"embed_ragged vs embed_wave L={len(wavs[i])}")
    with pytest.raises(ValueError):
        m.embed_ragged([wavs[0], np.zeros(80 * 1700, np.float32)])          # 1701 frames: over the 1604 of the handle
    with pytest.raises(ValueError):
        m.embed_ragged([wavs[0], np.zeros(511, np.float32)])


def _handler(tmp, compute, **kw):
    from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
    from tests.test_gpu_e2e import ARGS
    args = dict(ARGS, model={"name": "ResNetSE34V2", "nOut": 256}, features="melspectrogram", classifier={"input_size": 256, "out_neurons": 10},
                augment=False, augment_options={"augment_chain": []}, embed_batch=4, hip_compute=compute)
    net = WrappedModel(SpeakerEncoder(**args))
    mh = ModelHandling(net, **dict(args, save_folder=tmp, device_feats=False, **kw))
    net.module.load_state_dict({"__S__." + k: v for k, v in _sd().items()})
    return mh, getattr(net.module, "__S__")


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_whole_file_evaluation_rides_on_ragged_calls(tmp_path, compute):
    """num_eval = 0 over eight seeded WAV files of 0.5 to 2.5 s on a max_batch = 4 handle (1604 rows a call): the files share a few
    calls of the primary handle; the embeddings are the per-file path's to the compute type's bar"""
    import scipy.io.wavfile as wavfile
    rng = np.random.default_rng(20220829)
    files = []
    for i, n in enumerate(rng.integers(8000, 40001, size=8)):
        x = 0.1 * rng.standard_normal(int(n)) + 0.05 * np.sin(2 * np.pi * (200 + 50 * i) * np.arange(int(n)) / 16000.0)
        files.append(str(tmp_path / f"utt{i}.wav"))
        wavfile.write(files[-1], 16000, np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16))
    rag, S_rag = _handler(str(tmp_path), compute)
    per, S_per = _handler(str(tmp_path), compute, ragged_eval=False)
    assert rag._ragged_ok(0) and not per._ragged_ok(0)
    calls = []
    eng = S_rag.ragged_engine()
    inner = eng.embed_wave_ragged
    eng.embed_wave_ragged = lambda wavs, *a, **k: (calls.append(len(wavs)), inner(wavs, *a, **k))[1]
    got = np.asarray(rag._embed_files(files, 0))
    want = np.asarray(per._embed_files(files, 0))
    print(f"{compute}: {len(files)} files in ragged calls of {calls} utterances")
    assert sum(calls) == 8 and 2 <= len(calls) < 8
    assert got.shape == want.shape == (8, 1, 256) and np.isfinite(got).all()
    _close(got[:, 0], want[:, 0], compute, "whole-file evaluation, ragged vs per file")
    assert len(S_rag._engines) == 1 and len(S_per._engines) > 1
