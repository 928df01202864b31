"""GPU: ragged RawNet3 packs (svhip_rawnet3_embed_ragged) — utterances of different lengths in one call of one handle — against the
float64 oracle stage by stage, against the library's own fixed-length forward, for batch invariance bit for bit, for the refusals
of a real handle, and through the reference API with Raw3_ECAPA (whole-file evaluation, num_eval = 0).

The oracle check is tests/test_gpu_rawnet3_oracle.py's: every utterance's rows are sliced out of the packed stages and each stage is
compared with the oracle's block on the handle's previous stage, max |diff| / max |ref| over the utterance, against that file's
F32_BARS / BF16_BARS (imported, not restated).

Pack A (T0 = 30, 45, 33, 2992 on a samples = 8000, max_batch = 4 handle: 3100 rows): fewer frames than one 32-frame sinc tile, one
frame into a second tile, T2 = 2 (the minimum), utterance starts at rows 30 / 75 / 108 (off every tile grid), pooling left-overs
of 2 and 1 frames, n = max_batch and the level-0 capacity filled exactly — with 206 level-2 rows against max_batch * T2 = 204.
Pack B: one utterance of T0 = 2376 (T0 % 5 = 1, T1 % 3 = 1)."""
import numpy as np
import pytest
import torch

from oracle import rawnet3 as o_rn3
from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from tests.e2e_data import make_e2e_files
from tests.ragged_ring_check import check_async_ring
from tests.test_gpu_rawnet3_oracle import BF16_BARS, F32_BARS, SEED_W, STAGES, _layer_local, _rel, _sd_np

pytestmark = pytest.mark.gpu

MAXB, PRIMARY = 4, 8000
CAP = MAXB * o_rn3.frames(PRIMARY)[0]                  # 3100 level-0 rows
PACK_A, PACK_B = (30, 45, 33, 2992), (2376,)
HANDLE_STAGES = ("rn3_front", "rn3_layer1", "rn3_layer2", "rn3_layer3", "rn3_layer4", "rn3_pooled")
LEVEL = {"rn3_front": 0, "rn3_layer1": 1, "rn3_layer2": 2, "rn3_layer3": 2, "rn3_layer4": 2}
WIDTH = {"rn3_front": 256, "rn3_layer1": 1024, "rn3_layer2": 1024, "rn3_layer3": 1024, "rn3_layer4": 1536}


def _len(T0, extra=3):
    return 251 + 10 * (T0 - 1) + extra


def _waves(T0s, first=0):
    """one seeded waveform per utterance, each from its own stream position"""
    return [synth.synth_waveforms(1, _len(T), seed=20220829 + 7 * (first + u))[0] for u, T in enumerate(T0s)]


def _engine(compute, max_batch=MAXB, samples=PRIMARY, **kw):
    e = Engine(model="rawnet3", compute=compute, embed_dim=320, channels=1024, max_batch=max_batch, samples=samples, **kw)
    e.load_state_dict(_sd_np())
    e.finalize()
    return e


def _bars(compute):
    return F32_BARS if compute == "f32" else BF16_BARS


def _utterance_stages(e, lens):
    """the packed stages of the handle's last (ragged) forward, cut into one {stage: (1, T, C) or (1, 3072)} dict per utterance"""
    fr = [o_rn3.frames(L) for L in lens]
    packed = {n: e.get_stage(n) for n in HANDLE_STAGES}
    for n, lv in LEVEL.items():
        assert packed[n].size == sum(f[lv] for f in fr) * WIDTH[n], (n, packed[n].size)
    assert packed["rn3_pooled"].size == len(lens) * 3072
    out = []
    for u in range(len(lens)):
        S = {}
        for n, lv in LEVEL.items():
            r0 = sum(f[lv] for f in fr[:u])
            S[n] = packed[n].reshape(-1, WIDTH[n])[r0:r0 + fr[u][lv]].astype(np.float64)[None]
        S["rn3_pooled"] = packed["rn3_pooled"].reshape(len(lens), 3072)[u].astype(np.float64)[None]
        out.append(S)
    return out


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("pack", [PACK_A, PACK_B], ids=["A", "B"])
def test_packed_stages_against_the_oracle(compute, pack):
    wavs = _waves(pack, first=100 * len(pack))
    assert sum(pack) <= CAP and (pack is not PACK_A or sum(pack) == CAP)
    e = _engine(compute)
    emb = e.embed_wave_ragged(wavs)
    assert e.numeric_status() == 0 and emb.shape == (len(pack), 320) and np.isfinite(emb).all()
    for u, S in enumerate(_utterance_stages(e, [len(w) for w in wavs])):
        err = _layer_local(S, emb[u:u + 1], wavs[u][None], 0)
        print(f"ragged {compute} u={u} T0={pack[u]}: " + ", ".join(f"{n[4:] if n.startswith('rn3_') else n} {err[n]:.2e}" for n in STAGES))
        for n in STAGES:
            assert err[n] <= _bars(compute)[n], (compute, u, pack[u], n, err[n], _bars(compute)[n])
    e.close()


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_ragged_against_the_library_itself(compute):
    """every utterance of pack A alone through svhip_embed_wave on a handle of its own length, and a pack of four primary-length
    utterances against the ordinary batched call: within the end-to-end bar of the compute type (the two forwards take different GEMM
    kernels); device pointers in and out give the bits of the host call"""
    bar = _bars(compute)["end_to_end"]
    wavs = _waves(PACK_A, first=500)
    e = _engine(compute)
    emb = e.embed_wave_ragged(wavs)
    for u, w in enumerate(wavs):
        one = _engine(compute, max_batch=1, samples=len(w))
        alone = one.embed_wave(w[None])
        one.close()
        err = _rel(emb[u], alone[0])
        print(f"{compute} u={u} T0={PACK_A[u]}: ragged vs alone {err:.3g} (bar {bar})")
        assert err <= bar, (u, PACK_A[u], err)
    x = synth.synth_waveforms(MAXB, PRIMARY, seed=77)
    batched = e.embed_wave(x)
    ragged = e.embed_wave_ragged([x[b] for b in range(MAXB)])
    for b in range(MAXB):
        err = _rel(ragged[b], batched[b])
        print(f"{compute} b={b}: ragged vs batched at the primary length {err:.3g} (bar {bar})")
        assert err <= bar, (b, err)
    packed = torch.from_numpy(np.concatenate(wavs)).cuda()
    lens = [len(w) for w in wavs]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    dev = e.embed_wave_ragged(packed, offsets=offs, lengths=lens)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), emb)
    e.close()


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_batch_invariance_bit_for_bit(compute):
    """the same utterance alone / first / last / between different neighbours / in a pack of max_batch: its embedding and all six
    stages are bit for bit the same"""
    T0 = 173                                       # T1 = 34 (3 frames left over), T2 = 11 (1 left over)
    probe = _waves([T0], first=900)[0]
    others = _waves((401, 31, 260, 33, 1280, 77, 47), first=901)
    packs = {
        "alone": ([probe], 0),
        "first": ([probe, others[0], others[1]], 0),
        "last": ([others[2], others[3], probe], 2),
        "between": ([others[4], probe, others[5]], 1),
        "between2": ([others[6], probe, others[0]], 1),
        "max_batch": ([others[1], others[4], probe, others[3]], 2),
    }
    assert len(packs["max_batch"][0]) == MAXB
    e = _engine(compute)
    ref = None
    for name, (wavs, pos) in packs.items():
        emb = e.embed_wave_ragged(wavs)
        got = dict(_utterance_stages(e, [len(w) for w in wavs])[pos], emb=emb[pos].copy())
        if ref is None:
            ref = got
            assert np.isfinite(emb).all()
            continue
        for n in ref:
            assert np.array_equal(got[n], ref[n]), (compute, name, n, float(np.abs(got[n] - ref[n]).max()))
    e.close()


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_six_async_calls_wrap_the_table_slot_ring(compute):
    """six SVHIP_ASYNC calls in flight over the four pinned table slots of the handle (tests/ragged_ring_check.py)"""
    e = _engine(compute)
    T0s = [(30, 45), (33, 61, 38), (52, 31), (40, 35, 47), (36, 70), (44, 32, 55)]
    check_async_ring(e, [_waves(ts, first=700 + 10 * k) for k, ts in enumerate(T0s)])
    e.close()


def test_gpu_handle_refuses_bad_packs_and_keeps_working():
    """the capacity rules on a real handle (the host checks of svhip_rawnet3_ragged_check: nothing is enqueued); the good call
    afterwards returns the same bits; the ECAPA calls keep refusing a RawNet3 handle and this call refuses a handle of another model"""
    e = _engine("f32")
    w = _waves((401, 30), first=40)
    good = e.embed_wave_ragged(w)
    for wavs, word in (([w[1]] * (MAXB + 1), "max_batch"), ([np.zeros(540, np.float32)], "541"),
                       ([np.zeros(_len(CAP + 1), np.float32)], "capacity"), ([w[0], np.zeros(_len(CAP - 400), np.float32)], "utterance 1")):
        with pytest.raises(_lib.SvhipError) as ei:
            e.embed_wave_ragged(wavs)
        assert ei.value.code == -1 and word in str(ei.value), (word, str(ei.value))
    offs, lens = np.array([0, -1], np.int64), np.array([len(w[0]), len(w[1])], np.int32)
    with pytest.raises(_lib.SvhipError) as ei:
        e.embed_wave_ragged(np.concatenate(w), offsets=offs, lengths=lens)
    assert ei.value.code == -1 and "utterance 1" in str(ei.value)
    assert np.array_equal(e.embed_wave_ragged(w), good)
    out = np.empty((2, 320), np.float32)
    packed = np.concatenate(w)
    offs[1] = len(w[0])
    rc = e.lib.svhip_embed_wave_ragged(e.h, packed.ctypes.data, offs.ctypes.data, lens.ctypes.data, 2, out.ctypes.data, 0)
    assert rc not in (0, -1) and "ECAPA" in e.lib.svhip_last_error(e.h).decode()
    e.close()
    none = Engine(model="none")
    rc = none.lib.svhip_rawnet3_embed_ragged(none.h, packed.ctypes.data, offs.ctypes.data, lens.ctypes.data, 2, out.ctypes.data, 0)
    assert rc not in (0, -1) and "RAWNET3" in none.lib.svhip_last_error(none.h).decode()
    none.close()


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_a_nonfinite_waveform_stays_in_its_utterance(compute):
    """a NaN in slot 1 of a pack: SVHIP_ERR_NONFINITE, NaN for that utterance only, the others the bits of the clean call, and a
    clean next call"""
    e = _engine(compute, on_numeric="ignore")
    w = _waves((260, 77, 401), first=60)
    clean = e.embed_wave_ragged(w).copy()
    assert e.numeric_status() == 0
    bad = [a.copy() for a in w]
    bad[1][555] = np.nan
    packed = np.concatenate(bad)
    lens = np.array([len(a) for a in bad], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    got = np.empty_like(clean)
    rc = e.lib.svhip_rawnet3_embed_ragged(e.h, packed.ctypes.data, offs.ctypes.data, lens.ctypes.data, 3, got.ctypes.data, 0)
    assert rc == _lib.ERR_NONFINITE, (rc, e.lib.svhip_last_error(e.h))
    assert np.isnan(got[1]).all()
    assert np.array_equal(got[[0, 2]], clean[[0, 2]])
    assert np.array_equal(e.embed_wave_ragged(w), clean)
    e.close()


def _handler(tmp, **kw):
    from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
    from tests.test_gpu_e2e import ARGS
    from tests.test_gpu_rawnet3 import _fusion_sd
    args = dict(ARGS, model={"name": "Raw3_ECAPA", "nOut": 512}, features="raw", classifier={"input_size": 512, "out_neurons": 10},
                embed_batch=16)
    net = WrappedModel(SpeakerEncoder(**args))
    mh = ModelHandling(net, **dict(args, save_folder=tmp, **kw))
    net.module.load_state_dict({"__S__." + k: v for k, v in _fusion_sd(1, SEED_W).items()})
    return mh, getattr(net.module, "__S__"), args


def test_whole_file_evaluation_with_raw3_ecapa_rides_on_ragged_calls(tmp_path):
    """evaluateFromList / testFromList with num_eval = 0 and features = "raw" over WAV files of distinct lengths: the f32 scores equal
    the ragged_eval=False run within 1e-4 (the bar of the ECAPA test), and each branch ends with ONE engine where the per-file path
    cycles through its cache"""
    tmp = str(tmp_path)
    files, trial_path, lines = make_e2e_files(tmp)
    rag, S_rag, args = _handler(tmp)
    per, S_per, _ = _handler(tmp, ragged_eval=False)
    assert rag._ragged_ok(0) and not per._ragged_ok(0)
    kw = dict(listfilename=trial_path, distributed=False, dataloader_options=args["dataloader_options"], cohorts_path="unused", num_eval=0,
              scoring_mode="cosine")
    sc_r, lab_r, tr_r = rag.evaluateFromList(**kw)
    sc_p, lab_p, tr_p = per.evaluateFromList(**kw)
    assert lab_r == lab_p and tr_r == tr_p and len(sc_r) == len(lines)
    err = float(np.abs(np.array(sc_r) - np.array(sc_p)).max())
    print("Raw3_ECAPA evaluateFromList(num_eval=0): ragged vs per-file max score difference", err)
    assert err <= 1e-4
    for branch in (S_rag.ECAPA_TDNN, S_rag.rawnet):
        assert len(branch._engines) == 1 and branch._engine.max_batch == 16
    assert len(S_per.ECAPA_TDNN._engines) > 1 and len(S_per.rawnet._engines) > 1
    csv_path = tmp_path / "pairs.txt"
    csv_path.write_text("audio_1,audio_2\n" + "".join(f"{files[i]},{files[i + 1]}\n" for i in range(4)))
    res_r = rag.testFromList(test_list=str(csv_path), thresh_score=0.5, cohorts_path=None, num_eval=0, scoring_mode="cosine",
                             output_file=str(tmp_path / "out_r.txt"))
    res_p = per.testFromList(test_list=str(csv_path), thresh_score=0.5, cohorts_path=None, num_eval=0, scoring_mode="cosine",
                             output_file=str(tmp_path / "out_p.txt"))
    s_r = np.array([float(r.split(",")[-1]) for r in res_r])
    s_p = np.array([float(r.split(",")[-1]) for r in res_p])
    assert len(s_r) == 4 and float(np.abs(s_r - s_p).max()) <= 1e-4
    assert len(S_rag.ECAPA_TDNN._engines) == 1 and len(S_rag.rawnet._engines) == 1
    # a CUDA pack keeps forward's two-stream overlap and gives the bits of the host pack
    wavs = _waves((401, 60, 173), first=7)
    host = S_rag.embed_ragged(wavs)
    dev = S_rag.embed_ragged([torch.from_numpy(w).cuda() for w in wavs])
    assert host.shape == (3, 512) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
