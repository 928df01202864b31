"""GPU: ragged TitaNet packs (svhip_titanet_embed_ragged) — utterances of different lengths in one call of one handle.

The packed depthwise kernels alone against the fixed kernels bit for bit (utterances shorter than the kernel radius and than a tile,
tile edges, NaN neighbours); the lengths of tests/golden/titanet.npz in ONE call against the reference's fp32 and float64 embeddings
and the stages against the float64 restatement, at the bars of tests/test_gpu_titanet.py (imported, not restated); batch invariance
bit for bit; agreement with the fixed-length forward; a NaN utterance; six asynchronous calls; refusals on a real handle; the plug-ins
and whole-file evaluation; and the fixed-length call of a handle before and after a ragged one.

Where the ragged forward is compared with the fixed-length one (different GEMM kernels, so not bit for bit) the f32 bar is 2e-5 of
scale: each forward is held to 1e-5 of scale against float64 (test_gpu_titanet.py for the fixed one, test 3 here for the ragged one),
so two passing forwards differ by at most the sum.  bf16 keeps its own bar (cosine >= 0.999, <= 3e-2 of scale)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, synth
from speakerverification_amd.models import Tita_ECAPA, TitaNet
from tests import ecapa_oracle_check as chk
from tests.ragged_ring_check import check_async_ring
from tests.test_gpu_titanet import BF16_BARS, ERR_INVALID, ERR_UNSUPPORTED, KW, _check, _cos, _engine, _mel, _rel, _sd, ref64

pytestmark = pytest.mark.gpu

STAGES = ("tn_prolog", "tn_dw0", "tn_mega_last", "tn_enc")
_REF = {}


def _ref(size, seed_w, key, mel):
    """ref64 of a (B, 80, T) mel block, computed once per (size, weights, key) and shared (never written to)"""
    k = (size, seed_w, key)
    if k not in _REF:
        _REF[k] = ref64(_sd(size, seed_w), mel, size)
    return _REF[k]


def _close(a, b, compute, tag):
    """the ragged forward against the fixed-length one (module docstring)"""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    r, c = _rel(a, b), float(_cos(a.astype(np.float64), b.astype(np.float64)).min())
    print(f"{tag} {compute}: {r:.2e} of scale, min cos {c:.7f}")
    if compute == "f32":
        assert r <= 2e-5, (tag, r)
    else:
        assert c >= BF16_BARS[0] and r <= BF16_BARS[1], (tag, r, c)


def _stages(e, Ts):
    """the packed stages of the handle's last (ragged) forward, one {stage: (T_u, C) array} dict per utterance"""
    row0 = np.concatenate([[0], np.cumsum(Ts)])
    pool = e.get_stage("tn_pool").reshape(-1, 3072)
    assert pool.shape[0] == len(Ts)
    packed = {}
    for n in STAGES:
        a = e.get_stage(n)
        assert a.size % row0[-1] == 0, (n, a.size, row0[-1])
        packed[n] = a.reshape(row0[-1], -1)
        assert packed[n].shape[1] == (1536 if n == "tn_enc" else e.cfg.channels), (n, packed[n].shape)
    return [dict({n: packed[n][row0[u]:row0[u + 1]].copy() for n in STAGES}, tn_pool=pool[u].copy()) for u in range(len(Ts))]


def _features(T, seed):
    """a seeded (80, T) mel-power block"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((80, T)) ** 2 + 1e-3).astype(np.float32)


def _samples(T):
    """a waveform length with T mel frames (any L with L // 80 + 1 == T and L >= 512)"""
    return (T - 1) * 80 if (T - 1) * 80 >= 512 else T * 80 - 1


# ---- 1. the depthwise kernels alone --------------------------------------------------------------------------------------------------
DW_T = (1, 2, 5, 6, 7, 8, 9, 15, 16, 17, 33)          # below the radius (1, 3, 5), below / at / over a tile of 8 and of 16, three tiles


def _dw_case(compute, k, C, forms):
    lib = _lib.load()
    dtype = torch.float32 if compute == "f32" else torch.bfloat16
    code = _lib.F32 if compute == "f32" else _lib.BF16
    rng = np.random.default_rng(1000 * k + C)
    n, M = len(DW_T), sum(DW_T)
    row0_h = np.concatenate([[0], np.cumsum(DW_T)])
    row0 = torch.tensor(row0_h, dtype=torch.int32, device="cuda")
    x, skip, h3 = (torch.from_numpy(rng.standard_normal((M, C)).astype(np.float32)).cuda().to(dtype) for _ in range(3))
    gate = torch.from_numpy(rng.uniform(0.1, 1.0, (n, C)).astype(np.float32)).cuda()
    w = torch.from_numpy((rng.standard_normal((k, C)) / k).astype(np.float32)).cuda()
    bias = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).cuda()
    nan = float("nan")

    def outputs(rows):
        return torch.full((rows, C), nan, device="cuda", dtype=dtype), torch.full((rows, C), nan, device="cuda", dtype=dtype)

    def ptr(t, on):
        return t.data_ptr() if on else None

    def run(form, fixed_u=None, keep=None):
        """form: "dw" | "tail" | "tail_dw".  fixed_u: utterance fixed_u alone through the fixed kernel; else the pack, with every
        utterance but `keep` filled with NaN when keep is given.  -> (y, d) as float32 numpy (a tensor the form does not write: None)"""
        is_dw, with_d = form == "dw", form != "tail"
        if fixed_u is not None:
            r = slice(row0_h[fixed_u], row0_h[fixed_u + 1])
            xs, ss, hs, gs = x[r].contiguous(), skip[r].contiguous(), h3[r].contiguous(), gate[fixed_u:fixed_u + 1].contiguous()
            y, d = outputs(DW_T[fixed_u])
            torch.cuda.synchronize()
            rc = lib.svhip_titanet_depthwise(ptr(xs, is_dw), ptr(ss, not is_dw), ptr(hs, not is_dw), ptr(gs, not is_dw), ptr(y, not is_dw),
                                             ptr(w, with_d), ptr(bias, with_d), ptr(d, with_d), code, k, 1, DW_T[fixed_u], C, None)
        else:
            xs, ss, hs, gs = x, skip, h3, gate
            if keep is not None:
                xs, ss, hs, gs = (torch.full_like(t, nan) for t in (x, skip, h3, gate))
                r = slice(row0_h[keep], row0_h[keep + 1])
                xs[r], ss[r], hs[r], gs[keep] = x[r], skip[r], h3[r], gate[keep]
            y, d = outputs(M)
            torch.cuda.synchronize()
            rc = lib.svhip_titanet_depthwise_ragged(ptr(xs, is_dw), ptr(ss, not is_dw), ptr(hs, not is_dw), ptr(gs, not is_dw), ptr(y, not is_dw),
                                                    ptr(w, with_d), ptr(bias, with_d), ptr(d, with_d), code, k, row0.data_ptr(), n, max(DW_T), C, None)
        assert rc == _lib.OK, (form, fixed_u, rc)
        torch.cuda.synchronize()
        return (None if is_dw else y.float().cpu().numpy()), (d.float().cpu().numpy() if with_d else None)

    for form in forms:
        alone = [run(form, fixed_u=u) for u in range(n)]
        for out in alone:
            assert all(np.isfinite(a).all() for a in out if a is not None), form
        pack = run(form)
        for u in range(n):
            r = slice(row0_h[u], row0_h[u + 1])
            for name, got, want in zip("yd", pack, alone[u]):
                if want is not None:
                    assert np.array_equal(got[r], want), (compute, k, C, form, name, DW_T[u], float(np.abs(got[r] - want).max()))
        # every other utterance NaN: no tap of the clean one reads a neighbour's row, not even to discard it
        for u in range(n):
            r = slice(row0_h[u], row0_h[u + 1])
            poisoned = run(form, keep=u)
            for name, got, want in zip("yd", poisoned, alone[u]):
                if want is not None:
                    assert np.array_equal(got[r], want), (compute, k, C, form, name, "NaN neighbours", DW_T[u])


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("k", [3, 7, 11])
def test_packed_depthwise_is_the_fixed_kernel_per_utterance(compute, k):
    assert sum(DW_T) == 119
    _dw_case(compute, k, 64, ("dw", "tail", "tail_dw"))


def test_packed_depthwise_at_the_widest_row():
    """C = 1024, k = 11, bf16: 128 channel vectors per row, so a 256-thread group spans two tiles of different utterances"""
    _dw_case("bf16", 11, 1024, ("dw", "tail_dw"))


# ---- 2. the golden lengths in one call, and the stages ------------------------------------------------------------------------------
def _smallest_max_batch(size, lengths, compute, is_wave):
    lib = _lib.load()
    a = np.ascontiguousarray(lengths, dtype=np.int32)
    for mb in range(1, 4096):
        cfg = _lib.default_config()
        cfg.model, cfg.channels, cfg.embed_dim, cfg.log_input = _lib.MODEL_TITANET, synth.TITANET_SIZES[size][0], 320, 0
        cfg.samples, cfg.max_batch = 32000, mb
        cfg.compute = _lib.BF16 if compute == "bf16" else _lib.F32
        if lib.svhip_titanet_ragged_check(ctypes.byref(cfg), a.ctypes.data, len(a), 1 if is_wave else 0) == _lib.OK:
            return mb
    raise AssertionError("no max_batch holds the pack")


@pytest.mark.parametrize("size,compute", [("m", "f32"), ("m", "bf16"), ("s", "f32"), ("l", "bf16")])
def test_golden_lengths_in_one_call(golden_dir, size, compute):
    """The stages are held on size m, both computes: the cases of these four for which test_titanet_stages_against_float64 has set a
    bar (it covers (m, f32), (l, f32), (m, bf16))."""
    g = np.load(os.path.join(golden_dir, "titanet.npz"))
    B, seed_x, seed_w = int(g["B"]), int(g["seed_x"]), int(g["seed_w"])
    Ls = [int(v) for v in g["lengths"]]
    mels = {L: _mel(L, B, seed_x) for L in Ls}
    assert sorted(m.shape[2] for m in mels.values()) == [7, 9, 401] and B == 2
    feats = [mels[L][b] for L in Ls for b in range(B)]
    Ts = [f.shape[1] for f in feats]
    mb = _smallest_max_batch(size, Ts, compute, False)
    assert mb == 6                                                       # six utterances, 834 frames
    eng = _engine(size, compute, mb, 32000, _sd(size, seed_w))
    assert eng.ragged_check(Ts, is_wave=False) is None
    emb = eng.embed_features_ragged(feats)
    for i, L in enumerate(Ls):
        _check(emb[i * B:(i + 1) * B], g[f"{size}_out32_L{L}"], g[f"{size}_out64_L{L}"], compute, f"ragged titanet-{size} features L={L}")
    if size == "m":
        # the stages of utterance 1 of L = 32000 (T = 401), cut out of the pack by row0
        u = Ls.index(32000) * B + 1
        S = _stages(eng, Ts)[u]
        st, e64 = _ref(size, seed_w, "golden", mels[32000])
        assert _rel(e64, g[f"{size}_out64_L32000"]) <= 1e-9              # the restatement is the reference's arithmetic
        assert np.array_equal(eng.get_stage("mel").reshape(-1)[:feats[0].size], feats[0].reshape(-1))      # the packed blocks
        for name in STAGES + ("tn_pool",):
            want = st[name][1] if name == "tn_pool" else st[name][1].T
            r = _rel(S[name], want)
            print(f"ragged titanet-{size} {compute} {name}: {r:.2e} of scale")
            assert S[name].shape == want.shape and r <= (2e-5 if compute == "f32" else 3e-2), (name, r)
    if (size, compute) == ("m", "f32"):
        # the two waveform lengths through the mel front-end of the same call
        wavs = [w for L in (512, 32000) for w in synth.synth_waveforms(B, L, seed=seed_x)]
        assert eng.ragged_check([len(w) for w in wavs]) is None
        emb_w = eng.embed_wave_ragged(wavs)
        for i, L in enumerate((512, 32000)):
            _check(emb_w[i * B:(i + 1) * B], g[f"{size}_out32_L{L}"], g[f"{size}_out64_L{L}"], compute, f"ragged titanet-{size} wave L={L}")
    eng.close()


# ---- 3. batch invariance, the float64 restatement per utterance, and the fixed-length forward ---------------------------------------
INV_T = (1, 2, 7, 11, 70, 263, 401)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_batch_invariance_bit_for_bit_and_the_fixed_length_forward(compute):
    size = "m"
    feats = [_features(T, 100 + T) for T in INV_T]
    n = len(INV_T)
    eng = _engine(size, compute, n, 32000)

    def run(idx):
        emb = eng.embed_features_ragged([feats[i] for i in idx])
        assert np.isfinite(emb).all()
        S = _stages(eng, [INV_T[i] for i in idx])
        return {i: dict(S[k], emb=emb[k].copy()) for k, i in enumerate(idx)}

    ref = run(range(n))
    arrangements = {"reversed": [run(range(n)[::-1])], "alone": [run([i]) for i in range(n)], "two calls": [run([0, 1, 2, 3]), run([4, 5, 6])]}
    for name, parts in arrangements.items():
        got = {i: s for part in parts for i, s in part.items()}
        assert sorted(got) == list(range(n))
        for i in got:
            for st in ref[i]:
                assert np.array_equal(got[i][st], ref[i][st]), (compute, name, INV_T[i], st, float(np.abs(got[i][st] - ref[i][st]).max()))
    eng.close()
    for i, T in enumerate(INV_T):
        _, e64 = _ref(size, 1, ("inv", T), feats[i][None])
        _check(ref[i]["emb"], e64, e64, compute, f"ragged titanet-{size} T={T} alone in float64")
        if T >= 7:
            one = _engine(size, compute, 1, _samples(T))
            _close(ref[i]["emb"], one.embed_features(feats[i][None]), compute, f"ragged vs fixed T={T}")
            one.close()


# ---- 4. a non-finite input -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_a_nonfinite_input_stays_in_its_utterance(compute):
    eng = _engine("m", compute, 3, 32000)
    wavs = [synth.synth_waveforms(1, L, seed=60 + L)[0] for L in (32000, 8000, 20000)]
    feats = [_features(T, 70 + T) for T in (263, 70, 401)]
    for name, items, fn, is_wave in (("wave", wavs, eng.embed_wave_ragged, 1), ("features", feats, eng.embed_features_ragged, 0)):
        eng.on_numeric = "raise"
        clean = fn(items).copy()
        assert eng.numeric_status() == 0 and np.isfinite(clean).all()
        bad = [a.copy() for a in items]
        bad[1][..., 33] = np.nan
        packed, offs, lens = eng._pack(bad, None, None, bool(is_wave))
        got = np.empty_like(clean)
        rc = eng.lib.svhip_titanet_embed_ragged(eng.h, packed.ctypes.data, offs.ctypes.data, lens.ctypes.data, 3, got.ctypes.data, 0, is_wave)
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
    eng = _engine("m", compute, 3, 32000)
    Ls = [(600, 4000), (8000, 512, 2500), (1200, 5000), (3000, 700, 6100), (2000, 7000), (900, 4500, 1700)]
    check_async_ring(eng, [[synth.synth_waveforms(1, L, seed=300 + 10 * k + i)[0] for i, L in enumerate(ls)] for k, ls in enumerate(Ls)])
    eng.close()


# ---- 6. refusals on a real handle ----------------------------------------------------------------------------------------------------
def test_gpu_handle_refuses_bad_packs_and_keeps_working():
    """the capacity rules on a real handle (the host checks of svhip_titanet_ragged_check: nothing is enqueued); the good call
    afterwards returns the same bits; the other models' calls keep refusing a TitaNet handle"""
    eng = _engine("m", "f32", 3, 32000)                                   # 1203 rows
    good = [_features(T, 500 + T) for T in (401, 1, 801)]
    first = eng.embed_features_ragged(good).copy()
    assert np.isfinite(first).all()
    wav = synth.synth_waveforms(1, 32000, seed=8)[0]
    cases = [("too many utterances", lambda: eng.embed_features_ragged([_features(5, i) for i in range(4)]), "4 utterances"),
             ("too many frames", lambda: eng.embed_features_ragged([_features(T, 600 + T) for T in (401, 2, 801)]), "1204"),
             ("a too-short wave", lambda: eng.embed_wave_ragged([wav, wav[:511]]), "n_fft=512")]
    for name, call, text in cases:
        with pytest.raises(_lib.SvhipError) as ei:
            call()
        assert ei.value.code == ERR_INVALID and text in str(ei.value), (name, str(ei.value))
    packed, offs, lens = eng._pack([wav], None, None, True)
    out = np.empty((1, eng.embed_dim), np.float32)
    for export, tail in (("svhip_embed_wave_ragged", ()), ("svhip_rawnet3_embed_ragged", ()), ("svhip_conformer_embed_ragged", (1,))):
        rc = getattr(eng.lib, export)(eng.h, packed.ctypes.data, offs.ctypes.data, lens.ctypes.data, 1, out.ctypes.data, 0, *tail)
        assert rc == ERR_UNSUPPORTED, export
    assert np.array_equal(eng.embed_features_ragged(good), first)
    eng.close()


# ---- 7. the plug-ins and whole-file evaluation ---------------------------------------------------------------------------------------
PLUG_L = (32000, 600, 48000, 20000, 41000, 56000)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_plugin_embed_ragged_numpy_and_cuda(compute):
    m = TitaNet.MainModel(nOut=320, model_size="m", device="cuda", compute=compute, max_batch=4, **KW)
    m.load_state_dict(_sd("m"))
    wavs = [synth.synth_waveforms(1, L, seed=40 + i)[0] for i, L in enumerate(PLUG_L)]
    host = m.embed_ragged(wavs)
    dev = m.embed_ragged([torch.from_numpy(w).cuda() for w in wavs])
    assert host.shape == (6, 320) and np.isfinite(host).all() and dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
    assert len(m._engines) == 1
    for i in (1, 3):
        _close(host[i], np.atleast_2d(m.embed_wave(wavs[i][None]))[0], compute, f"embed_ragged vs embed_wave L={len(wavs[i])}")
    with pytest.raises(ValueError):
        m.embed_ragged([wavs[0], np.zeros(80 * 1700, np.float32)])          # 1701 frames: over the 1604 of the handle
    with pytest.raises(ValueError):
        m.embed_ragged([wavs[0], np.zeros(511, np.float32)])


@pytest.mark.parametrize("compute", ["f32", "half"])
def test_tita_ecapa_embed_ragged_agrees_with_forward_per_file(compute):
    """Tita_ECAPA picks the ragged path up from its two branches: [ECAPA | TitaNet] per file against model(wav) at that file's own
    length.  The TitaNet columns at the bars of _close; the ECAPA columns at the end-to-end bar of tests/ecapa_oracle_check.py, which
    tests/test_gpu_ragged.py holds the ragged ECAPA forward to against the fixed-length one."""
    kind = "bf16" if compute == "half" else "f32"
    spec_e, spec_t = synth.ecapa_param_spec(C=512, input_norm=True), synth.titanet_param_spec("m", 320)
    sd = {"ECAPA_TDNN." + k: v for k, v in synth.synth_state_dict(spec_e, seed=1).items()}
    sd.update({"titaNet." + k: v for k, v in synth.synth_state_dict(spec_t, seed=1).items()})
    model = Tita_ECAPA.MainModel(nOut=512, hip_compute=compute, max_batch=4, **KW)
    model.load_state_dict(sd)
    wavs = [synth.synth_waveforms(1, L, seed=40 + i)[0] for i, L in enumerate(PLUG_L)]
    host = np.asarray(model.embed_ragged(wavs))
    dev = model.embed_ragged([torch.from_numpy(w).cuda() for w in wavs])
    assert host.shape == (6, 512) and np.isfinite(host).all() and dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
    bar = chk.bars(kind)["end_to_end"]
    for i in (0, 1, 3):
        alone = np.asarray(model(wavs[i][None])).reshape(-1)
        err = chk.rel_err(host[i, :192], alone[:192])[0]
        print(f"Tita_ECAPA {kind} L={len(wavs[i])}: ECAPA columns {err:.2e} (bar {bar})")
        assert err <= bar, (i, err)
        _close(host[i, 192:], alone[192:], kind, f"Tita_ECAPA TitaNet columns L={len(wavs[i])}")


def _handler(tmp, compute, **kw):
    from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
    from tests.test_gpu_e2e import ARGS
    args = dict(ARGS, model={"name": "TitaNet", "nOut": 320}, model_size="m", features="melspectrogram",
                classifier={"input_size": 320, "out_neurons": 10}, embed_batch=4, hip_compute=compute)
    net = WrappedModel(SpeakerEncoder(**args))
    mh = ModelHandling(net, **dict(args, save_folder=tmp, device_feats=False, **kw))
    net.module.load_state_dict({"__S__." + k: v for k, v in _sd("m").items()})
    return mh, getattr(net.module, "__S__")


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_whole_file_evaluation_rides_on_ragged_calls(tmp_path, compute):
    """num_eval = 0 over ten seeded WAV files of 0.5 to 3 s on a max_batch = 4 handle (1604 frames a call): the files share a few calls
    of the primary handle; the embeddings are the per-file path's to the compute type's bar"""
    import scipy.io.wavfile as wavfile
    rng = np.random.default_rng(20220829)
    files = []
    for i, n in enumerate(rng.integers(8000, 48001, size=10)):
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
    assert sum(calls) == 10 and 2 <= len(calls) < 10
    assert got.shape == want.shape == (10, 1, 320) and np.isfinite(got).all()
    _close(got[:, 0], want[:, 0], compute, "whole-file evaluation, ragged vs per file")
    assert len(S_rag._engines) == 1 and len(S_per._engines) > 1


# ---- 8. the fixed-length call of the same handle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_fixed_length_call_unchanged_by_a_ragged_call(compute):
    eng = _engine("m", compute, 3, 32000)
    mel = _mel(32000, 3, seed=13)
    before = eng.embed_features(mel).copy()
    st_before = {n: eng.get_stage(n).copy() for n in STAGES + ("tn_pool",)}
    eng.embed_features_ragged([_features(T, T) for T in (521, 1, 263)])
    assert eng.get_stage("tn_mega_last").size == (521 + 1 + 263) * 512
    after = eng.embed_features(mel)
    assert np.array_equal(before, after)
    for n in st_before:
        assert np.array_equal(st_before[n], eng.get_stage(n)), n
    assert eng.get_stage("tn_mega_last").size == 3 * 401 * 512
    eng.close()
