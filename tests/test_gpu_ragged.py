"""GPU: ragged ECAPA-TDNN batches — utterances of different lengths embedded by one call on one handle.

1. against the float64 oracle, per utterance and stage by stage: the rows of every utterance are sliced out of the packed stages and
   held against tests/ecapa_oracle_check.py at ITS bars (`bars(compute)`, measured on fixed-length calls; none is loosened here);
   the mel front-end against oracle/fbank.py at the bars of tests/test_gpu_fbank.py;
2. against the library itself: every utterance alone through svhip_embed_wave on a handle of its own length, and a pack of
   primary-length utterances against the ordinary batched call;
3. batch invariance: the same utterance first / last / between different neighbours / alone / in a pack of max_batch — embeddings
   and every stage bit for bit;
4. the API: evaluateFromList / testFromList with num_eval = 0 over files of distinct lengths against the ragged_eval=False run.

The ragged forward has ONE kernel per GEMM (the generic one, whatever the row count: that is what keeps (3)), so "every GEMM route"
of the fixed-length oracle test is a single route here; the developer options that steer the routed kernels are set in one case to
show that they do not reach the ragged forward.

Length sets: T_u = 5 .. 12 (the reflect pads of 2 / 3 / 4 / 8 frames all wrap), the primary length (401), a long utterance
(3001 frames), n = 1, n = max_batch, a pack that fills the row capacity exactly (3001 + 200 + 7 = 8 * 401), utterance starts that are
no multiples of 128 / 256 rows."""
import os

import numpy as np
import pytest
import torch

from oracle import ecapa as o_ecapa, fbank as o_fbank, synthwave
from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
from tests import ecapa_oracle_check as chk
from tests.e2e_data import make_e2e_files
from tests.ragged_ring_check import check_async_ring

pytestmark = pytest.mark.gpu

SEED_W, SEED_X = 5, 20220829
HOP, NMEL, PRIMARY, MAXB = 80, 80, 32000, 8
ROWS = MAXB * (PRIMARY // HOP + 1)                          # 3208: the row capacity of the test handles
_SD = {}


def _sd(C, input_norm=False):
    if (C, input_norm) not in _SD:
        sd = synth.synth_state_dict(synth.ecapa_param_spec(C=C, n_mels=NMEL, input_norm=input_norm), seed=SEED_W)
        sd64 = chk.torch_sd(sd)
        _SD[(C, input_norm)] = (sd, sd64, chk.rounded_sd(sd64, C))
    return _SD[(C, input_norm)]


def _engine(compute, C, input_norm=False, max_batch=MAXB, samples=PRIMARY, log_input=True):
    e = Engine(model="ecapa", compute=compute, channels=C, max_batch=max_batch, samples=samples, input_norm=input_norm, log_input=log_input)
    e.load_state_dict(_sd(C, input_norm)[0])
    e.finalize()
    return e


def _waves(lengths, first=0):
    """seeded waveforms from the counter-based stream of oracle/synthwave.py, utterance u = stream utterance first + u"""
    return [np.ascontiguousarray(synthwave.synth_waveforms(SEED_X, first + u, 1, L + (-L) % 4)[0, :L], dtype=np.float32) for u, L in enumerate(lengths)]


def _frames(L):
    return L // HOP + 1


def _len(T):
    return (T - 1) * HOP + 37                                # T frames, not a multiple of the hop


def _packed_stages(e, Ts):
    """{stage: per-utterance list of float64 arrays (T_u, channels) or (n,)} of the handle's last (ragged) forward"""
    M, row0 = sum(Ts), np.concatenate([[0], np.cumsum(Ts)])
    S = {}
    for n in chk.HANDLE_STAGES:
        a = e.get_stage(n).astype(np.float64)
        if n in chk.VECTOR_STAGES:
            a = a.reshape(len(Ts), -1)
            S[n] = [a[u] for u in range(len(Ts))]
        else:
            a = a.reshape(M, -1)
            S[n] = [a[row0[u]:row0[u + 1]] for u in range(len(Ts))]
    return S


def _oracle_check(tag, e, compute, C, Ts, emb, feats64, input_norm=False):
    """every utterance of the last ragged call against the oracle at the bars of ecapa_oracle_check; feats64[u]: the oracle's
    (1, n_mels, T_u) network input of utterance u"""
    sd, sd64, sdq = _sd(C, input_norm)
    S = _packed_stages(e, Ts)
    bad = []
    for u, T in enumerate(Ts):
        Su = {n: v[u][None] for n, v in S.items()}
        with torch.no_grad():
            e2e = o_ecapa.ecapa_forward(feats64[u], sd64, features="none").reshape(-1).numpy()
        err = chk.layer_local(Su, 0, sdq if compute == "bf16" else sd64, ref_input=feats64[u], emb=emb[u].astype(np.float64), e2e_ref=e2e,
                              bf16=compute == "bf16")
        print(f"{tag} {compute} C={C} u={u} T={T}: {chk.describe(err)}")
        bad += [(u, T) + f for f in chk.failures(err, compute)]
    assert not bad, (tag, compute, C, bad)


def _wave_feats64(wavs, input_norm, C):
    sd64 = _sd(C, input_norm)[1]
    out = []
    with torch.no_grad():
        for w in wavs:
            mel = o_fbank.melspectrogram(torch.from_numpy(w).double()[None], n_fft=512, n_mels=NMEL)
            out.append(chk.features(mel, sd64, input_norm))
    return out


# the wave packs: T_u of every utterance.  A: the short lengths, the primary one and starts off the tile grid, n = max_batch;
# B: the long utterance, filling the row capacity exactly; C1: n = 1
PACK_A = [7, 8, 9, 10, 11, 12, 401, 300]
PACK_B = [3001, 200, 7]
PACK_1 = [137]
assert sum(PACK_B) == ROWS and len(PACK_A) == MAXB


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("pack", ["A", "B", "1"])
def test_wave_packs_meet_the_oracle_stage_by_stage(compute, pack):
    Ts = {"A": PACK_A, "B": PACK_B, "1": PACK_1}[pack]
    C = 64
    wavs = _waves([_len(T) for T in Ts], first=10 * ord(pack))
    assert [_frames(len(w)) for w in wavs] == Ts
    e = _engine(compute, C)
    emb = e.embed_wave_ragged(wavs)
    assert emb.shape == (len(Ts), 192) and e.numeric_status() == 0 and np.isfinite(emb).all()
    # the mel front-end per utterance (f32 handles: the exact DFT; bars of tests/test_gpu_fbank.py)
    mel = e.get_stage("mel").astype(np.float64)
    pos = 0
    for u, T in enumerate(Ts):
        got = mel[pos:pos + NMEL * T].reshape(NMEL, T)
        pos += NMEL * T
        with torch.no_grad():
            ref = o_fbank.melspectrogram(torch.from_numpy(wavs[u]).double()[None], n_fft=512, n_mels=NMEL)[0].numpy()
        peak = float(np.abs(ref).max())
        e_mel = float(np.abs(got - ref).max()) / peak
        lg = lambda m: np.log(m + 1e-6) - np.log(m + 1e-6).mean(axis=1, keepdims=True)
        e_log = float(np.abs(lg(got) - lg(ref)).max())
        print(f"pack {pack} {compute} u={u} T={T}: mel rel-to-peak {e_mel:.3g}, log-mel abs {e_log:.3g}")
        if compute == "f32":
            assert e_mel <= 2e-6 and e_log <= 1e-4, (u, T, e_mel, e_log)
        else:
            assert e_log <= 5e-3, (u, T, e_log)
    assert pos == mel.size
    _oracle_check(f"pack {pack}", e, compute, C, Ts, emb, _wave_feats64(wavs, False, C))
    e.close()


@pytest.mark.parametrize("compute,C,input_norm,log_input", [("f32", 64, False, True), ("bf16", 64, True, True), ("f32", 512, True, True),
                                                            ("bf16", 1024, False, True)])
def test_feature_packs_from_five_frames_meet_the_oracle(compute, C, input_norm, log_input):
    """svhip_embed_features_ragged: T_u = 5 and 6 are only reachable from features (a waveform has at least n_fft samples: 7 frames);
    blocks separated by gaps in the feature array; C = 512 / 1024 and input_norm here.  The developer options that steer the routed
    GEMMs are set: the ragged forward does not read them."""
    Ts = [5, 6, 7, 8, 9, 12, 401, 150] if C == 64 else [5, 401, 9, 150]
    e = _engine(compute, C, input_norm)
    for k, v in (("pw3_cus", 8), ("n128_off", 1), ("cv_off", 1), ("pw3_tail_off", 1)):
        e.set_option(k, v)
    feats = [synth.synth_mel(1, NMEL, T, seed=SEED_X + 31 * u + T)[0] for u, T in enumerate(Ts)]
    # one packed array with a gap of 3 frames' worth of blocks between the utterances
    offs, pos = [], 0
    for T in Ts:
        offs.append(pos)
        pos += T + 3
    packed = np.full(pos * NMEL, np.nan, np.float32)
    for f, o in zip(feats, offs):
        packed[o * NMEL:(o + f.shape[1]) * NMEL] = f.reshape(-1)
    emb = e.embed_features_ragged(packed, offsets=offs, lengths=Ts)
    assert e.numeric_status() == 0 and np.isfinite(emb).all()
    emb_list = e.embed_features_ragged(feats)
    assert np.array_equal(emb, emb_list)                                  # list form == packed form, bit for bit
    sd64 = _sd(C, input_norm)[1]
    f64 = [chk.features(torch.from_numpy(f).double()[None], sd64, input_norm) for f in feats]
    _oracle_check("features", e, compute, C, Ts, emb, f64, input_norm)
    e.close()


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_ragged_against_the_library_itself(compute):
    """each utterance alone through svhip_embed_wave on a handle of its own length, and a pack of primary-length utterances against
    the ordinary batched call: within the end-to-end bar of the oracle check (the two forwards run different kernels)."""
    C = 64
    bar = chk.bars(compute)["end_to_end"]
    Ts = PACK_A
    wavs = _waves([_len(T) for T in Ts], first=500)
    e = _engine(compute, C)
    emb = e.embed_wave_ragged(wavs)
    for u, w in enumerate(wavs):
        one = _engine(compute, C, max_batch=1, samples=len(w))
        alone = one.embed_wave(w[None])
        one.close()
        err = chk.rel_err(emb[u], alone[0])[0]
        print(f"{compute} u={u} T={Ts[u]}: ragged vs alone {err:.3g} (bar {bar})")
        assert err <= bar, (u, Ts[u], err)
    x = synth.synth_waveforms(MAXB, PRIMARY, seed=SEED_X)
    batched = e.embed_wave(x)
    ragged = e.embed_wave_ragged([x[b] for b in range(MAXB)])
    err = chk.rel_err(ragged, batched)[0]
    print(f"{compute}: ragged vs batched at the primary length {err:.3g} (bar {bar})")
    assert err <= bar
    # device pointers in and out
    packed = torch.from_numpy(np.concatenate(wavs)).cuda()
    lens = [len(w) for w in wavs]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    dev = e.embed_wave_ragged(packed, offsets=offs, lengths=lens)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), emb)
    e.close()


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_ragged_pack_on_another_front_end(compute):
    """the ragged waveform path at another window and hop (16 kHz, win 400, hop 160: per utterance the 64-frame fbank kernel at 76.9 KB
    of LDS, on a bf16 handle the separate fbank + prologue kernels): three waveforms of different lengths in one call, each utterance's
    mel rows and embedding against a fixed-length handle of its own length"""
    C = 64
    fe = dict(sr=16000, n_fft=512, win_length=400, hop_length=160)
    Ts = [9, 65, 130]
    wavs = _waves([(T - 1) * 160 + 37 for T in Ts], first=700)
    e = Engine(model="ecapa", compute=compute, channels=C, max_batch=3, samples=32000, **fe)
    e.load_state_dict(_sd(C)[0])
    e.finalize()
    emb = e.embed_wave_ragged(wavs)
    assert emb.shape == (3, 192) and e.numeric_status() == 0 and np.isfinite(emb).all()
    mel = e.get_stage("mel")
    e.close()
    assert mel.size == NMEL * sum(Ts)
    pos = 0
    for u, (w, T) in enumerate(zip(wavs, Ts)):
        one = Engine(model="ecapa", compute=compute, channels=C, max_batch=1, samples=len(w), **fe)
        one.load_state_dict(_sd(C)[0])
        one.finalize()
        alone = one.embed_wave(w[None])
        mel1 = one.get_stage("mel")
        one.close()
        got = mel[pos:pos + NMEL * T]
        pos += NMEL * T
        with torch.no_grad():
            ref = o_fbank.melspectrogram(torch.from_numpy(w).double()[None], n_mels=NMEL, **fe)[0].numpy()
        e_mel = float(np.abs(got.reshape(NMEL, T) - ref).max() / np.abs(ref).max())
        d_emb = chk.rel_err(emb[u], alone[0])[0]
        print(f"{compute} u={u} T={T}: mel bit for bit {np.array_equal(got, mel1.reshape(-1))}, against the oracle {e_mel:.3g}; "
              f"embedding bit for bit {np.array_equal(emb[u], alone[0])}, ragged vs alone {d_emb:.3g}")
        assert mel1.size == NMEL * T and np.array_equal(got, mel1.reshape(-1)), (compute, u, T)
        assert np.array_equal(emb[u], alone[0]), (compute, u, T, d_emb)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_batch_invariance_bit_for_bit(compute):
    """the same utterance first / last / between different neighbours / alone / in a pack of max_batch: its embedding and every stage
    are bit-for-bit the same"""
    C = 64
    T0 = 173
    probe = _waves([_len(T0)], first=900)[0]
    others = _waves([_len(T) for T in (401, 9, 260, 33, 128, 77, 12, 500, 7)], first=901)
    packs = {
        "alone": ([probe], 0),
        "first": ([probe, others[0], others[1]], 0),
        "last": ([others[2], others[3], probe], 2),
        "between": ([others[4], probe, others[5]], 1),
        "between2": ([others[7], others[8], probe, others[6], others[1]], 2),
        "max_batch": (others[:5] + [probe] + others[5:7], 5),
    }
    assert len(packs["max_batch"][0]) == MAXB
    e = _engine(compute, C)
    ref = None
    for name, (wavs, pos) in packs.items():
        emb = e.embed_wave_ragged(wavs)
        Ts = [_frames(len(w)) for w in wavs]
        r0 = sum(Ts[:pos])
        got = {"emb": emb[pos].copy()}
        for n in chk.HANDLE_STAGES:
            a = e.get_stage(n)
            got[n] = a.reshape(len(Ts), -1)[pos].copy() if n in chk.VECTOR_STAGES else a.reshape(sum(Ts), -1)[r0:r0 + T0].copy()
        if ref is None:
            ref = got
            continue
        for n in ref:
            assert np.array_equal(got[n], ref[n]), (compute, name, n, float(np.abs(got[n] - ref[n]).max()))
    e.close()


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_six_async_calls_wrap_the_table_slot_ring(compute):
    """six SVHIP_ASYNC calls in flight over the four pinned table slots of the handle (tests/ragged_ring_check.py)"""
    e = _engine(compute, 64)
    Ts = [(7, 33), (60, 9, 21), (12, 45), (30, 8, 17), (25, 50), (11, 40, 19)]
    check_async_ring(e, [_waves([_len(T) for T in ts], first=700 + 10 * k) for k, ts in enumerate(Ts)])
    e.close()


def test_gpu_handles_refuse_bad_packs_and_keep_working():
    """the capacity rules on a real handle (the same host checks as svhip_ragged_check: nothing is enqueued), the scope rule on an
    F32X3 and a non-ECAPA handle; a good call afterwards is unaffected"""
    e = _engine("f32", 64)
    w = _waves([_len(401), _len(9)], first=40)
    good = e.embed_wave_ragged(w)
    for wavs, word in (([w[1]] * (MAXB + 1), "max_batch"), ([np.zeros(511, np.float32)], "n_fft"), ([np.zeros(ROWS * HOP, np.float32)], "capacity")):
        with pytest.raises(_lib.SvhipError) as ei:
            e.embed_wave_ragged(wavs)
        assert ei.value.code == -1 and word in str(ei.value)
    with pytest.raises(_lib.SvhipError) as ei:
        e.embed_features_ragged([synth.synth_mel(1, NMEL, 4)[0]])
    assert ei.value.code == -1 and "fewer than 5" in str(ei.value)
    assert np.array_equal(e.embed_wave_ragged(w), good)
    e.close()
    x3 = _engine("f32x3", 64)
    with pytest.raises(_lib.SvhipError) as ei:
        x3.embed_wave_ragged(w)
    assert ei.value.code not in (0, -1) and "SVHIP_F32" in str(ei.value)
    x3.close()
    none = Engine(model="none")
    with pytest.raises(_lib.SvhipError) as ei:
        none.embed_wave_ragged(w)
    assert ei.value.code not in (0, -1) and "ECAPA" in str(ei.value)
    none.close()


ARGS = dict(
    device="cuda", gpu=0, model={"name": "ECAPA_TDNN", "nOut": 192}, criterion={"name": "AAmSoftmaxAP", "margin": 0.25, "scale": 30},
    classifier={"input_size": 192, "out_neurons": 10}, optimizer={"name": "adam"}, callbacks={"name": "steplr"},
    features="melspectrogram", include_top=False, n_mels=80, nClasses=10, channels=[64] * 4 + [192],
    dataloader_options={"nPerSpeaker": 2, "num_workers": 0, "batch_size": 2},
    audio_spec={"sample_rate": 16000, "channels": 1, "sentence_len": 2.0, "win_len": 0.025, "hop_len": 0.01},
    augment=False, augment_options={"augment_chain": []},
)


def _handler(tmp, **kw):
    net = WrappedModel(SpeakerEncoder(**ARGS))
    mh = ModelHandling(net, **dict(ARGS, save_folder=tmp, **kw))
    net.module.load_state_dict({"__S__." + k: v for k, v in synth.synth_state_dict(synth.ecapa_param_spec(C=64), seed=3).items()})
    return mh, getattr(net.module, "__S__")


def test_whole_file_evaluation_rides_on_ragged_calls(tmp_path):
    """evaluateFromList / testFromList with num_eval = 0 over WAV files of distinct lengths: the scores equal the ragged_eval=False run
    within 1e-4 (the project's cosine-score bar for f32), and the module ends with ONE engine where the per-file path cycles through
    its cache"""
    tmp = str(tmp_path)
    files, trial_path, lines = make_e2e_files(tmp)
    rag, S_rag = _handler(tmp)
    per, S_per = _handler(tmp, ragged_eval=False)
    kw = dict(listfilename=trial_path, distributed=False, dataloader_options=ARGS["dataloader_options"], cohorts_path="unused", num_eval=0,
              scoring_mode="cosine")
    sc_r, lab_r, tr_r = rag.evaluateFromList(**kw)
    sc_p, lab_p, tr_p = per.evaluateFromList(**kw)
    assert lab_r == lab_p and tr_r == tr_p and len(sc_r) == len(lines)
    err = float(np.abs(np.array(sc_r) - np.array(sc_p)).max())
    print("evaluateFromList(num_eval=0): ragged vs per-file max score difference", err)
    assert err <= 1e-4
    assert len(S_rag._engines) == 1 and S_rag._engine.max_batch == 256
    assert len(S_per._engines) > 1
    csv_path = tmp_path / "pairs.txt"
    csv_path.write_text("audio_1,audio_2\n" + "".join(f"{files[i]},{files[i + 1]}\n" for i in range(4)))
    res_r = rag.testFromList(test_list=str(csv_path), thresh_score=0.5, cohorts_path=None, num_eval=0, scoring_mode="cosine",
                             output_file=str(tmp_path / "out_r.txt"))
    res_p = per.testFromList(test_list=str(csv_path), thresh_score=0.5, cohorts_path=None, num_eval=0, scoring_mode="cosine",
                             output_file=str(tmp_path / "out_p.txt"))
    s_r = np.array([float(r.split(",")[-1]) for r in res_r])
    s_p = np.array([float(r.split(",")[-1]) for r in res_p])
    assert len(s_r) == 4 and float(np.abs(s_r - s_p).max()) <= 1e-4
    assert len(S_rag._engines) == 1
