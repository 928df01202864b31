"""GPU: ragged Conformer packs (svhip_conformer_embed_ragged) — utterances of different lengths in one call of one handle.

The packed attention kernel alone against the fixed kernel bit for bit (tile and wave edges, a NaN neighbour); the lengths of
tests/golden/conformer.npz in ONE call against the reference's fp32 and float64 embeddings and stages at the bars of
tests/test_gpu_conformer.py (imported, not restated); batch invariance bit for bit; agreement with the fixed-length forward; a NaN
utterance; a pack that needs two subsampling slices; the plug-in and whole-file evaluation; and the fixed-length call of a handle
before and after a ragged one.

Where the ragged forward is compared with the fixed-length one (different GEMM kernels, so not bit for bit) the f32 bar is 2e-5 of
scale: each forward is held to 1e-5 of scale against float64 by test_gpu_conformer.py, so two passing forwards differ by at most the
sum.  bf16 keeps its own bar (cosine >= 0.999, <= 3e-2 of scale)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, synth
from speakerverification_amd.models import Conformer
from tests.ragged_ring_check import check_async_ring
from tests.test_gpu_conformer import BF16_BARS, KW, _check, _cos, _engine, _mel, _rel, _sd

pytestmark = pytest.mark.gpu

STAGES = ("cf_in", "cf_attn0", "cf_block0", "cf_last")


def _tp(T):
    return synth.conformer_frames(T)


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
    """the packed stages of the handle's last (ragged) forward, one {stage: array} dict per utterance"""
    tps = [_tp(T) for T in Ts]
    row0 = np.concatenate([[0], np.cumsum(tps)])
    packed = {n: e.get_stage(n).reshape(-1, 256) for n in STAGES}
    pool = e.get_stage("cf_pool").reshape(-1, 512)
    assert pool.shape[0] == len(Ts) and all(packed[n].shape[0] == row0[-1] for n in STAGES)
    return [dict({n: packed[n][row0[u]:row0[u + 1]].copy() for n in STAGES}, cf_pool=pool[u].copy()) for u in range(len(Ts))]


def _features(T, seed):
    """a seeded (80, T) mel-power block"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((80, T)) ** 2 + 1e-3).astype(np.float32)


# ---- 1. the attention kernel alone -----------------------------------------------------------------------------------------------
ATT_T = (1, 2, 15, 16, 17, 63, 64, 65, 129)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_packed_attention_is_the_fixed_kernel_per_utterance(compute):
    lib = _lib.load()
    assert sum(ATT_T) == 372
    dtype = torch.float32 if compute == "f32" else torch.bfloat16
    code = _lib.F32 if compute == "f32" else _lib.BF16
    rng = np.random.default_rng(372)
    qkv = {T: torch.from_numpy(rng.standard_normal((T, 768)).astype(np.float32)).cuda().to(dtype) for T in ATT_T}
    P, u, v = (torch.from_numpy(a.astype(np.float32)).cuda() for a in
               (rng.standard_normal((max(ATT_T), 256)), 0.5 * rng.standard_normal((4, 64)), 0.5 * rng.standard_normal((4, 64))))

    def alone(T):
        out = torch.full((T, 256), float("nan"), device="cuda", dtype=dtype)
        assert lib.svhip_conformer_attention(qkv[T].data_ptr(), P.data_ptr(), u.data_ptr(), v.data_ptr(), out.data_ptr(), code, 1, T, None) == _lib.OK
        torch.cuda.synchronize()
        return out.float().cpu().numpy()

    def packed(order, poison=None):
        x = torch.cat([torch.full_like(qkv[T], float("nan")) if T == poison else qkv[T] for T in order]).contiguous()
        row0 = torch.tensor(np.concatenate([[0], np.cumsum(order)]), dtype=torch.int32, device="cuda")
        out = torch.full((sum(order), 256), float("nan"), device="cuda", dtype=dtype)
        torch.cuda.synchronize()
        rc = lib.svhip_conformer_attention_ragged(x.data_ptr(), P.data_ptr(), u.data_ptr(), v.data_ptr(), out.data_ptr(), code, row0.data_ptr(),
                                                  len(order), max(order), None)
        assert rc == _lib.OK
        torch.cuda.synchronize()
        got, r = out.float().cpu().numpy(), row0.cpu().numpy()
        return {T: got[r[i]:r[i + 1]] for i, T in enumerate(order)}

    ref = {T: alone(T) for T in ATT_T}
    assert all(np.isfinite(ref[T]).all() for T in ATT_T)
    for order in (ATT_T, ATT_T[::-1]):
        got = packed(order)
        for T in ATT_T:
            assert np.array_equal(got[T], ref[T]), (compute, order[0], T, float(np.abs(got[T] - ref[T]).max()))
        # the T' = 17 utterance all NaN: its neighbours on both sides (16 | 63 in order, 63 | 16 reversed) must not see it through the
        # Q''_{i+1} row, the key tile or the value tile
        got = packed(order, poison=17)
        assert np.isnan(got[17]).all()
        for T in ATT_T:
            if T != 17:
                assert np.array_equal(got[T], ref[T]), (compute, "NaN neighbour", order[0], T)


# ---- 2 / 3. the golden lengths in one call, and the stages --------------------------------------------------------------------------
def _smallest_max_batch(lengths, compute, is_wave):
    lib = _lib.load()
    a = np.ascontiguousarray(lengths, dtype=np.int32)
    for mb in range(1, 4096):
        cfg = _lib.default_config()
        cfg.model, cfg.channels, cfg.embed_dim, cfg.input_norm, cfg.samples, cfg.max_batch = _lib.MODEL_CONFORMER, 256, 512, 1, 32000, mb
        cfg.compute = _lib.BF16 if compute == "bf16" else _lib.F32
        if lib.svhip_conformer_ragged_check(ctypes.byref(cfg), a.ctypes.data, len(a), 1 if is_wave else 0) == _lib.OK:
            return mb
    raise AssertionError("no max_batch holds the pack")


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_golden_lengths_in_one_call(golden_dir, compute):
    g = np.load(os.path.join(golden_dir, "conformer.npz"))
    B, seed_x = int(g["B"]), int(g["seed_x"])
    Ls = [int(v) for v in g["lengths"]]
    mels = {L: _mel(L, B, seed_x) for L in Ls}
    assert sorted(_tp(m.shape[2]) for m in mels.values()) == [1, 2, 99, 129, 499]
    feats = [mels[L][b] for L in Ls for b in range(B)]
    Ts = [f.shape[1] for f in feats]
    mb = _smallest_max_batch(Ts, compute, False)
    print(f"{compute}: {len(feats)} utterances, {sum(Ts)} frames, max_batch = {mb}")
    eng = _engine(compute, mb, 32000, _sd(int(g["seed_w"])))
    assert eng.ragged_check(Ts, is_wave=False) is None
    emb = eng.embed_features_ragged(feats)
    for i, L in enumerate(Ls):
        _check(emb[i * B:(i + 1) * B], g[f"out32_L{L}"], g[f"out64_L{L}"], compute, f"ragged features L={L} T'={_tp(mels[L].shape[2])}")
    # the stages of utterance 0 of L = 32000, cut out of the pack by row0
    S = _stages(eng, Ts)[Ls.index(32000) * B]
    for stage, key in (("cf_in", "cf_in"), ("cf_attn0", "cf_attn0"), ("cf_block0", "block0"), ("cf_last", "block5"), ("cf_pool", "cf_pool")):
        want = g[f"val_{key}"]
        r = _rel(S[stage], want)
        print(f"ragged {compute} {stage}: {r:.2e} of scale")
        assert S[stage].shape == want.shape and r <= (1e-5 if compute == "f32" else 3e-2), (stage, r)
    # the two waveform lengths through the mel front-end of the same call
    wavs = [w for L in (512, 32000) for w in synth.synth_waveforms(B, L, seed=seed_x)]
    assert eng.ragged_check([len(w) for w in wavs]) is None
    emb_w = eng.embed_wave_ragged(wavs)
    for i, L in enumerate((512, 32000)):
        _check(emb_w[i * B:(i + 1) * B], g[f"out32_L{L}"], g[f"out64_L{L}"], compute, f"ragged wave L={L}")
    eng.close()


# ---- 4 / 5. batch invariance, and the fixed-length forward -----------------------------------------------------------------------------
INV_T = (7, 11, 70, 263, 401, 521)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_batch_invariance_bit_for_bit_and_the_fixed_length_forward(compute):
    feats = [_features(T, 100 + T) for T in INV_T]
    eng = _engine(compute, len(INV_T), 32000)

    def run(idx):
        emb = eng.embed_features_ragged([feats[i] for i in idx])
        assert np.isfinite(emb).all()
        S = _stages(eng, [INV_T[i] for i in idx])
        return {i: dict(S[k], emb=emb[k].copy()) for k, i in enumerate(idx)}

    ref = run(range(len(INV_T)))
    arrangements = {"reversed": [run(range(len(INV_T))[::-1])], "alone": [run([i]) for i in range(len(INV_T))],
                    "two calls": [run([0, 1, 2]), run([3, 4, 5])]}
    for name, parts in arrangements.items():
        got = {i: s for part in parts for i, s in part.items()}
        assert sorted(got) == list(range(len(INV_T)))
        for i in got:
            for n in ref[i]:
                assert np.array_equal(got[i][n], ref[i][n]), (compute, name, INV_T[i], n, float(np.abs(got[i][n] - ref[i][n]).max()))
    eng.close()
    for i, T in enumerate(INV_T):
        samples = (T - 1) * 80 if (T - 1) * 80 >= 512 else T * 80 - 1
        one = _engine(compute, 1, samples)
        _close(ref[i]["emb"], one.embed_features(feats[i][None])[0], compute, f"ragged vs fixed T={T}")
        one.close()


# ---- 6. a non-finite input -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_a_nonfinite_input_stays_in_its_utterance(compute):
    eng = _engine(compute, 3, 32000)
    eng.on_numeric = "ignore"
    wavs = [synth.synth_waveforms(1, L, seed=60 + L)[0] for L in (32000, 8000, 20000)]
    feats = [_features(T, 70 + T) for T in (263, 70, 401)]
    for name, items, fn, is_wave in (("wave", wavs, eng.embed_wave_ragged, 1), ("features", feats, eng.embed_features_ragged, 0)):
        clean = fn(items).copy()
        assert eng.numeric_status() == 0 and np.isfinite(clean).all()
        bad = [a.copy() for a in items]
        bad[1][..., 33] = np.nan
        packed, offs, lens = eng._pack(bad, None, None, bool(is_wave))
        got = np.empty_like(clean)
        rc = eng.lib.svhip_conformer_embed_ragged(eng.h, packed.ctypes.data, offs.ctypes.data, lens.ctypes.data, 3, got.ctypes.data, 0, is_wave)
        assert rc == _lib.ERR_NONFINITE, (name, rc, eng.lib.svhip_last_error(eng.h))
        assert np.isnan(got[1]).all(), name
        assert np.array_equal(got[[0, 2]], clean[[0, 2]]), name
        assert np.array_equal(fn(items), clean), name
    eng.close()


# ---- 6b. more asynchronous calls in flight than table slots ---------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_six_async_calls_wrap_the_table_slot_ring(compute):
    """six SVHIP_ASYNC calls in flight over the four pinned table slots of the handle (tests/ragged_ring_check.py)"""
    eng = _engine(compute, 3, 32000)
    Ls = [(600, 4000), (8000, 512, 2500), (1200, 5000), (3000, 700, 6100), (2000, 7000), (900, 4500, 1700)]
    check_async_ring(eng, [[synth.synth_waveforms(1, L, seed=300 + 10 * k + i)[0] for i, L in enumerate(ls)] for k, ls in enumerate(Ls)])
    eng.close()


# ---- 7. more than one subsampling slice ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_a_pack_over_two_subsampling_slices(compute):
    """four 20 s utterances (T = 4001, T' = 999) on a max_batch = 40 handle of 2 s: one slice holds min(40, 33 | 67) x 99 = 3267 | 3960
    subsampled frames, the pack has 3996, so the subsampling runs as slices of three utterances and one; the same utterances in calls of
    three and one (a single slice each) give the same bits"""
    feats = [_features(4001, 900 + i) for i in range(4)]
    eng = _engine(compute, 40, 32000)
    slice_rows = Conformer.slice_frames(40, 401, 80, compute)
    assert 3 * 999 <= slice_rows < 4 * 999
    whole = eng.embed_features_ragged(feats)
    assert np.isfinite(whole).all()
    parts = np.concatenate([eng.embed_features_ragged(feats[:3]), eng.embed_features_ragged(feats[3:])])
    assert np.array_equal(whole, parts)
    eng.close()


# ---- 8. the plug-in and whole-file evaluation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_plugin_embed_ragged_numpy_and_cuda(compute):
    m = Conformer.MainModel(nOut=512, device="cuda", compute=compute, max_batch=4, **KW)
    m.load_state_dict(_sd())
    wavs = [synth.synth_waveforms(1, L, seed=40 + i)[0] for i, L in enumerate((32000, 600, 48000, 20000, 41000, 56000))]
    host = m.embed_ragged(wavs)
    dev = m.embed_ragged([torch.from_numpy(w).cuda() for w in wavs])
    assert host.shape == (6, 512) and np.isfinite(host).all() and dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
    assert len(m._engines) == 1
    for i in (1, 3):
        _close(host[i], np.atleast_2d(m.embed_wave(wavs[i][None]))[0], compute, f"embed_ragged vs embed_wave L={len(wavs[i])}")
    with pytest.raises(ValueError):
        m.embed_ragged([wavs[0], np.zeros(80 * 1700, np.float32)])          # 1701 frames: over the 1604 of the handle


def _handler(tmp, compute, **kw):
    from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
    from tests.test_gpu_e2e import ARGS
    args = dict(ARGS, model={"name": "Conformer", "nOut": 512}, features="melspectrogram", classifier={"input_size": 512, "out_neurons": 10},
                embed_batch=4, hip_compute=compute)
    net = WrappedModel(SpeakerEncoder(**args))
    mh = ModelHandling(net, **dict(args, save_folder=tmp, device_feats=False, **kw))
    net.module.load_state_dict({"__S__." + k: v for k, v in _sd().items()})
    return mh, getattr(net.module, "__S__")


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_whole_file_evaluation_rides_on_ragged_calls(tmp_path, compute):
    """num_eval = 0 over nine WAV files: eight share three calls of the primary handle (1604 frames each), the ninth (1751 frames) fits
    no call and comes back through the per-file path; the embeddings are the per-file path's to the compute type's bar"""
    import scipy.io.wavfile as wavfile
    from tests.e2e_data import make_e2e_files
    files, _, _ = make_e2e_files(str(tmp_path))
    rng = np.random.default_rng(3)
    long_file = str(tmp_path / "long.wav")
    wavfile.write(long_file, 16000, np.round(3000 * rng.standard_normal(140000)).astype(np.int16))
    files = files + [long_file]
    rag, S_rag = _handler(str(tmp_path), compute)
    per, S_per = _handler(str(tmp_path), compute, ragged_eval=False)
    assert rag._ragged_ok(0) and not per._ragged_ok(0)
    assert S_rag.ragged_frames(140000) == 0 and not S_rag.ragged_packer().fits_alone(1751)      # T' = 437: over the slice, and over the rows
    calls = []
    eng = S_rag.ragged_engine()
    inner = eng.embed_wave_ragged
    eng.embed_wave_ragged = lambda wavs, *a, **k: (calls.append(len(wavs)), inner(wavs, *a, **k))[1]
    got = np.asarray(rag._embed_files(files, 0))
    want = np.asarray(per._embed_files(files, 0))
    print(f"{compute}: {len(files)} files in ragged calls of {calls} utterances")
    assert sum(calls) == 8 and len(calls) < 8
    assert got.shape == want.shape == (9, 1, 512) and np.isfinite(got).all()
    _close(got[:, 0], want[:, 0], compute, "whole-file evaluation, ragged vs per file")
    assert len(S_per._engines) > 1


# ---- 9. the fixed-length call of the same handle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_fixed_length_call_unchanged_by_a_ragged_call(compute):
    eng = _engine(compute, 3, 32000)
    mel = _mel(32000, 3, seed=13)
    before = eng.embed_features(mel).copy()
    st_before = eng.get_stage("cf_last").copy()
    eng.embed_features_ragged([_features(T, T) for T in (521, 7, 263)])
    after = eng.embed_features(mel)
    assert np.array_equal(before, after) and np.array_equal(st_before, eng.get_stage("cf_last"))
    assert eng.get_stage("cf_last").size == 3 * 99 * 256
    eng.close()
