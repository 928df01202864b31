"""GPU: ragged RawNet2 'conv' packs (svhip_rawnet2_embed_ragged) — utterances of different lengths in one call of one handle — against
the float64 oracle block by block, against the library's own fixed-length forward, for batch invariance bit for bit, for option
rn_keep, the table ring, the refusals of a real handle, a non-finite input, and through the reference API with Raw_ECAPA_conv_asp
(whole-file evaluation, num_eval = 0).

The oracle check is tests/rawnet2_oracle_check.py's: every utterance's rows are cut out of the packed stages (option rn_keep) and
layer_local compares each with the oracle's step on the handle's own stored input, against that file's BARS (imported, not restated).

Handle: samples = 8000, max_batch = 4 (T1 = 2666, 10 664 level-0 rows).  An utterance of T1 front-end frames is 3 T1 + extra samples.
Pack A (T1 = 729, 2188, 730, 7017): fills the capacity exactly; utterances start at rows 729 / 2917 / 3647, off every tile grid; 729 is
the minimum (one frame at the aggregation), 730 one frame over it; 2188 has the levels 729 / 243 / 81 / 27 / 9 / 3, 7017 has 2339 / 779 /
259 / 86 / 28 / 9 with pooling left-overs of 0, 2, 2, 1, 2, 1; the last level has 1 + 3 + 1 + 9 = 14 rows against max_batch * tf = 12 (the
ragged-only buffers).  Pack B: one utterance of the whole capacity.  The probes of the batch-invariance test sit on both sides of the
tail's 48-frame slice: T1 = 1297 (432 / 144 / 48 / 16 / 5 / 1: whole slices at three levels) and 1325 (441 / 147 / 49: one frame into a
new slice); tests/test_rawnet2_ragged_host.py asserts that they sit there."""
import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from tests import rawnet2_oracle_check as chk
from tests.e2e_data import E2E_LENGTHS, make_e2e_files
from tests.ecapa_oracle_check import BF16_BARS as ECAPA_BF16_BARS
from tests.ragged_ring_check import check_async_ring
from tests.test_gpu_rawnet2_oracle import ERR_STATE, NOUT, SEED_W, _e2e, _sd
from tests.test_rawnet2_ragged_host import PROBES, levels

pytestmark = pytest.mark.gpu

MODEL = "rawnet2_conv"
MAXB, PRIMARY = 4, 8000
CAP = MAXB * (PRIMARY // 3)                                  # 10 664 level-0 rows
PACK_A, PACK_B = ((729, 0), (2188, 1), (730, 2), (7017, 1)), ((10664, 2),)      # (T1, extra samples)
COMPUTES = ("f32", "bf16", "f16")
IN_LEVEL = (0, 1, 2, 3, 3, 4, 5, 5)                          # the frame level each block reads
X_STORED = (1, 3, 4, 6, 7)                                   # blocks with an identity shortcut behind another block: their x is stored


def _stage_table():
    """{stage name without rn_: (level or None for one row per utterance, columns)}"""
    t = {"front": (0, 128), "agg_in": (6, 512), "logits": (6, 512), "pooled": (None, 1024)}
    for i, (_, cin, cout, down) in enumerate(chk.BLOCKS):
        t[f"b{i}_pre"] = (IN_LEVEL[i], cin)
        t[f"b{i}_o"] = (IN_LEVEL[i], cout)
        t[f"b{i}_gate"] = (None, cout)
        if i in X_STORED:
            t[f"b{i}_x"] = (IN_LEVEL[i], cin)
    return t


STAGE_TABLE = _stage_table()


def _len(T1, extra=0):
    return 3 * T1 + extra


def _waves(pack, first=0):
    """one seeded waveform per (T1, extra), each from its own stream position"""
    return [synth.synth_waveforms(1, _len(T, x), seed=20220829 + 7 * (first + u))[0] for u, (T, x) in enumerate(pack)]


def _engine(compute, max_batch=MAXB, samples=PRIMARY, keep=False, **kw):
    e = Engine(model=MODEL, compute=compute, embed_dim=NOUT, max_batch=max_batch, samples=samples, **kw)
    e.load_state_dict(_sd(MODEL, PRIMARY, compute)[0])
    e.finalize()
    if keep:
        e.set_option("rn_keep", 1)
    return e


def _utterance_stages(e, lens):
    """the kept stages of the handle's last (ragged) forward, cut into one {stage: (1, T, C) or (1, C)} float64 dict per utterance"""
    lv = [levels(L // 3) for L in lens]
    out = [{} for _ in lens]
    for name, (level, cols) in STAGE_TABLE.items():
        a = e.get_stage("rn_" + name).astype(np.float64)
        if level is None:
            assert a.size == len(lens) * cols, (name, a.size)
            for u in range(len(lens)):
                out[u][name] = a.reshape(len(lens), cols)[u][None]
            continue
        assert a.size == sum(f[level] for f in lv) * cols, (name, a.size)
        a = a.reshape(-1, cols)
        for u in range(len(lens)):
            r0 = sum(f[level] for f in lv[:u])
            out[u][name] = a[r0:r0 + lv[u][level]][None]
    return out


def _rel(got, ref):
    return chk.rel_err(got, ref)[0]


# An fp32-accumulated K = 512 product is known to about the f32 handle's own `logits` bar (the same generic kernel in fp32): a hidden
# attention value that close to the midpoint of two 16-bit numbers has no decided rounding.
TIE_REL = chk.BARS["f32"]["logits"]


def logits_with_ties(S, sdq, compute):
    """layer_local's `logits` checks of one utterance with the reference's 16-bit rounding of the hidden attention layer decided
    either way where it is a tie.  layer_local rounds attention.2's float64 output to the handle's type; the kernel rounds its fp32
    value of the same element, and where that element lies within TIE_REL of the midpoint of two 16-bit numbers the two roundings can
    differ by one unit, which moves a frame's logits by about 1e-3 of their scale against bars of 3e-6 (bf16).  Per frame, every
    combination of its tied elements (at most four) is a reference; the one nearest the stored logits is held to the imported bars.
    Returns ({check: (error, index)}, the tied (frame, hidden unit) pairs)."""
    import itertools
    import torch.nn.functional as F
    from oracle import rawnet2 as o_rn
    rnd = chk.rounder(compute)
    agg = torch.from_numpy(np.ascontiguousarray(S["agg_in"][0].T))[None]
    with torch.no_grad():
        a = o_rn.bn(F.leaky_relu(F.conv1d(agg, sdq["attention.0.weight"], sdq["attention.0.bias"]), 0.01), sdq, "attention.2")
        ar = rnd(a)
        ref = F.conv1d(ar, sdq["attention.3.weight"], sdq["attention.3.bias"])[0].numpy().T.copy()
    got, w3 = S["logits"][0], sdq["attention.3.weight"][:, :, 0].numpy()              # (T, 512), (512, 128)
    v, r = a[0].numpy().T, ar[0].numpy().T                                               # (T, 128)
    bits = 8 if compute == "bf16" else 11
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 1e-300))) - (bits - 1))
    tied = (0.5 * ulp - np.abs(v - r) <= TIE_REL * np.abs(v)) & (np.abs(v) > 0)
    pairs = [(int(t), int(k)) for t, k in zip(*np.nonzero(tied))]
    for t in sorted({t for t, _ in pairs}):
        ks = [k for tt, k in pairs if tt == t]
        assert len(ks) <= 4, (t, ks)
        best = ref[t]
        for flip in itertools.product((0, 1), repeat=len(ks)):
            alt = ref[t] + sum(f * np.sign(v[t, k] - r[t, k]) * ulp[t, k] * w3[:, k] for f, k in zip(flip, ks))
            if np.abs(got[t] - alt).max() < np.abs(got[t] - best).max():
                best = alt
        ref[t] = best
    return {"logits": chk.rel_err(got, ref), "logits/local": chk.local_err(got, ref), "logits/bias": chk.bias_err(got, ref)}, pairs


@pytest.mark.parametrize("compute", COMPUTES)
@pytest.mark.parametrize("pack", [PACK_A, PACK_B], ids=["A", "B"])
def test_packed_stages_against_the_oracle(compute, pack):
    """every utterance's stages, cut out of the pack, against the oracle's steps on the handle's own stored inputs and the imported
    bars.  (`b<i>.pre` is the pre-activation block i's tail writes: it is formed from the gated value before its 16-bit store, so it
    carries the rounding of one store, not of two.)  The `logits` checks of a 16-bit handle decide a rounding tie of the hidden
    attention layer either way (logits_with_ties): pack A in bf16 has one, utterance 3, frame 6, unit 78 — 3.97656278 against the
    midpoint 3.9765625, 7e-8 away in relative terms — where layer_local alone reports 8.9e-4 against the bar 3e-6 and the other
    rounding gives 1.1e-7."""
    wavs = _waves(pack, first=100 * len(pack))
    assert sum(T for T, _ in pack) == CAP and {x for _, x in PACK_A} == {0, 1, 2}
    assert sum(levels(T)[6] for T, _ in PACK_A) == 14 > MAXB * levels(PRIMARY // 3)[6]
    sdq = _sd(MODEL, PRIMARY, compute)[2]
    e = _engine(compute, keep=True)
    emb = e.embed_wave_ragged(wavs).astype(np.float64)
    assert e.numeric_status() == 0 and emb.shape == (len(pack), NOUT) and np.isfinite(emb).all()
    stages = _utterance_stages(e, [len(w) for w in wavs])
    with pytest.raises(_lib.SvhipError) as ei:             # the fixed forward's other stages are not a pack's
        e.get_stage("rn_b0_pool")
    assert ei.value.code == ERR_STATE
    e.close()
    worst, bad = {}, []
    for u, S in enumerate(stages):
        err = chk.layer_local(S, 0, sdq, wavs[u], MODEL, compute, emb=emb[u], e2e_ref=_e2e(wavs[u], MODEL, PRIMARY))
        print(f"ragged {compute} u={u} T1={pack[u][0]}: {chk.describe(err)}")
        if compute != "f32" and any(f[0].startswith("logits") for f in chk.failures(err, compute)):
            tie_err, pairs = logits_with_ties(S, sdq, compute)
            print(f"ragged {compute} u={u}: rounding ties of the hidden attention layer at (frame, unit) {pairs}: {chk.describe(tie_err)}")
            if pairs:
                err.update(tie_err)
        chk.by_kind(err, worst)
        bad += [(u,) + f for f in chk.failures(err, compute)]
    print(f"WORST ragged {compute} " + " ".join(f"{k}={v:.3e}" for k, v in sorted(worst.items())))
    assert not bad, (compute, bad)


@pytest.mark.parametrize("compute", COMPUTES)
def test_ragged_against_the_library_itself(compute):
    """every utterance of pack A alone through svhip_embed_wave on a handle of its own length, and a pack of four primary-length
    utterances against the ordinary batched call: within the end-to-end bar of the compute type (the two forwards take different
    kernels); device pointers in and out give the bits of the host call"""
    bar = chk.bar(compute, "end_to_end")
    wavs = _waves(PACK_A, first=500)
    e = _engine(compute)
    emb = e.embed_wave_ragged(wavs)
    for u, w in enumerate(wavs):
        one = _engine(compute, max_batch=1, samples=len(w))
        alone = one.embed_wave(w[None])
        one.close()
        err = _rel(emb[u], alone[0])
        print(f"{compute} u={u} T1={PACK_A[u][0]}: ragged vs alone {err:.3g} (bar {bar})")
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


@pytest.mark.parametrize("compute", COMPUTES)
@pytest.mark.parametrize("T1", PROBES)
def test_batch_invariance_bit_for_bit(compute, T1):
    """the same utterance alone / first / last / between two different pairs of neighbours / in a pack of max_batch: its embedding and
    every kept stage are bit for bit the same"""
    probe = _waves([(T1, 1)], first=900 + T1)[0]
    others = _waves(((3001, 0), (729, 2), (1460, 1), (735, 0), (4100, 2), (977, 1), (801, 0)), first=901)
    packs = {
        "alone": ([probe], 0),
        "first": ([probe, others[0], others[1]], 0),
        "last": ([others[2], others[3], probe], 2),
        "between": ([others[4], probe, others[5]], 1),
        "between2": ([others[6], probe, others[0]], 1),
        "max_batch": ([others[1], others[4], probe, others[3]], 2),
    }
    assert len(packs["max_batch"][0]) == MAXB
    e = _engine(compute, keep=True)
    ref = None
    for name, (wavs, pos) in packs.items():
        assert sum(len(w) // 3 for w in wavs) <= CAP
        emb = e.embed_wave_ragged(wavs)
        got = dict(_utterance_stages(e, [len(w) for w in wavs])[pos], emb=emb[pos].copy())
        if ref is None:
            ref = got
            assert np.isfinite(emb).all() and set(ref) == set(STAGE_TABLE) | {"emb"}
            continue
        for n in ref:
            assert np.array_equal(got[n], ref[n]), (compute, T1, name, n, float(np.abs(got[n] - ref[n]).max()))
    e.close()


@pytest.mark.parametrize("compute", COMPUTES)
def test_keeping_the_stages_leaves_the_ragged_forward_alone(compute):
    """option rn_keep on and off on a pack: equal profile labels, launch counts and embedding bits; with it off only rn_pooled is served"""
    wavs = _waves(((1297, 2), (729, 0), (2188, 1)), first=300)
    e = _engine(compute)
    e.set_option("layer_labels", 1)
    got = {}
    for keep in (0, 1, 0):
        e.set_option("rn_keep", keep)
        e.profile(True)
        emb = e.embed_wave_ragged(wavs).copy()
        prof = {n: r["launches"] for n, r in e.profile_results().items()}
        e.profile(False)
        if keep:
            stages = _utterance_stages(e, [len(w) for w in wavs])
            assert all(np.isfinite(a).all() for S in stages for a in S.values())
        else:
            assert e.get_stage("rn_pooled").size == len(wavs) * 1024
            for n in STAGE_TABLE:
                if n != "pooled":
                    with pytest.raises(_lib.SvhipError) as ei:
                        e.get_stage("rn_" + n)
                    assert ei.value.code == ERR_STATE, n
        if "emb" in got:
            assert prof == got["prof"], (keep, prof, got["prof"])
            assert np.array_equal(emb, got["emb"])
        got["emb"], got["prof"] = emb, prof
    labels = {n.split()[0] for n in got["prof"]}
    assert labels == {"rag_rows", "rn_rag_slices", "rn_rag_front", "gemm_conv", "gemm_pw", "rn_rag_tail_part", "rn_rag_gate", "rn_rag_tail_apply",
                      "rn_rag_attn_pool", "rn_fc", "emb_out"}, sorted(labels)
    e.close()


@pytest.mark.parametrize("compute", COMPUTES)
def test_six_async_calls_wrap_the_table_slot_ring(compute):
    """six SVHIP_ASYNC calls in flight over the four pinned table slots of the handle (tests/ragged_ring_check.py)"""
    e = _engine(compute)
    T1s = [(729, 1045), (733, 1161, 838), (952, 731), (1040, 735, 747), (736, 1170), (844, 732, 955)]
    check_async_ring(e, [_waves([(T, (T + k) % 3) for T in ts], first=700 + 10 * k) for k, ts in enumerate(T1s)])
    e.close()


def test_gpu_handle_refuses_bad_packs_and_keeps_working():
    """the capacity rules on a real handle (the host checks of svhip_rawnet2_ragged_check: nothing is enqueued); the good call afterwards
    returns the same bits; the ECAPA call keeps refusing a RawNet2 handle, and this call refuses a handle of another model and a sinc
    RawNet2 handle"""
    e = _engine("f32")
    w = _waves(((1401, 1), (729, 0)), first=40)
    good = e.embed_wave_ragged(w)
    for wavs, word in (([w[1]] * (MAXB + 1), "max_batch"), ([np.zeros(2186, np.float32)], "2187"),
                       ([np.zeros(_len(CAP + 1), np.float32)], "capacity"), ([w[0], np.zeros(_len(CAP - 1400), np.float32)], "utterance 1")):
        with pytest.raises(_lib.SvhipError) as ei:
            e.embed_wave_ragged(wavs)
        assert ei.value.code == -1 and word in str(ei.value), (word, str(ei.value))
    offs, lens = np.array([0, -1], np.int64), np.array([len(w[0]), len(w[1])], np.int32)
    with pytest.raises(_lib.SvhipError) as ei:
        e.embed_wave_ragged(np.concatenate(w), offsets=offs, lengths=lens)
    assert ei.value.code == -1 and "utterance 1" in str(ei.value)
    assert np.array_equal(e.embed_wave_ragged(w), good)
    out = np.empty((2, NOUT), np.float32)
    packed = np.concatenate(w)
    offs[1] = len(w[0])
    rc = e.lib.svhip_embed_wave_ragged(e.h, packed.ctypes.data, offs.ctypes.data, lens.ctypes.data, 2, out.ctypes.data, 0)
    assert rc not in (0, -1) and "ECAPA" in e.lib.svhip_last_error(e.h).decode()
    e.close()
    none = Engine(model="none")
    rc = none.lib.svhip_rawnet2_embed_ragged(none.h, packed.ctypes.data, offs.ctypes.data, lens.ctypes.data, 2, out.ctypes.data, 0)
    assert rc not in (0, -1) and "RAWNET2_CONV" in none.lib.svhip_last_error(none.h).decode()
    none.close()
    L = 2438
    sinc = Engine(model="rawnet2", compute="f32", embed_dim=NOUT, max_batch=2, samples=L)
    sinc.load_state_dict(_sd("rawnet2", L, "f32")[0])
    sinc.finalize()
    x = synth.synth_waveforms(2, L, seed=5).reshape(-1)
    o2, l2 = np.array([0, L], np.int64), np.array([L, L], np.int32)
    rc = sinc.lib.svhip_rawnet2_embed_ragged(sinc.h, x.ctypes.data, o2.ctypes.data, l2.ctypes.data, 2, out.ctypes.data, 0)
    msg = sinc.lib.svhip_last_error(sinc.h).decode()
    assert rc not in (0, -1) and "RAWNET2_CONV" in msg and "LayerNorm(nb_samp)" in msg, msg
    sinc.close()


@pytest.mark.parametrize("compute", COMPUTES)
def test_a_nonfinite_waveform_stays_in_its_utterance(compute):
    """a NaN sample in slot 1 of a pack: SVHIP_ERR_NONFINITE, NaN for that utterance only, the others the bits of the clean call, and a
    clean next call"""
    e = _engine(compute, on_numeric="ignore")
    w = _waves(((1260, 1), (977, 0), (1401, 2)), first=60)
    clean = e.embed_wave_ragged(w).copy()
    assert e.numeric_status() == 0 and np.isfinite(clean).all()
    bad = [a.copy() for a in w]
    bad[1][1555] = np.nan
    packed = np.concatenate(bad)
    lens = np.array([len(a) for a in bad], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    got = np.empty_like(clean)
    rc = e.lib.svhip_rawnet2_embed_ragged(e.h, packed.ctypes.data, offs.ctypes.data, lens.ctypes.data, 3, got.ctypes.data, 0)
    assert rc == _lib.ERR_NONFINITE, (rc, e.lib.svhip_last_error(e.h))
    assert not np.isfinite(got[1]).any()
    assert np.array_equal(got[[0, 2]], clean[[0, 2]])
    assert np.array_equal(e.embed_wave_ragged(w), clean)
    e.close()


def _handler(tmp, compute="f32", **kw):
    from speakerverification_amd.model import ModelHandling, SpeakerEncoder, WrappedModel
    from tests.test_gpu_e2e import ARGS
    from tests.test_gpu_fusion_variants import _fusion_sd
    args = dict(ARGS, model={"name": "Raw_ECAPA_conv_asp", "nOut": 512}, features="raw", classifier={"input_size": 512, "out_neurons": 10},
                embed_batch=16, hip_compute=compute)
    net = WrappedModel(SpeakerEncoder(**args))
    mh = ModelHandling(net, **dict(args, save_folder=tmp, **kw))
    net.module.load_state_dict({"__S__." + k: v for k, v in _fusion_sd({"seed_w_ecapa": 1, "seed_w_rawnet2": SEED_W}, "conv").items()})
    return mh, getattr(net.module, "__S__"), args


def test_whole_file_evaluation_with_raw_ecapa_conv_asp_rides_on_ragged_calls(tmp_path):
    """evaluateFromList / testFromList with num_eval = 0 and features = "raw" over WAV files of distinct lengths: the f32 scores equal
    the ragged_eval=False run within 1e-4 (the bar of the ECAPA and RawNet3 tests), and each branch ends with ONE engine where the
    per-file path cycles through its cache"""
    tmp = str(tmp_path)
    assert min(E2E_LENGTHS) >= 2187
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
    print("Raw_ECAPA_conv_asp evaluateFromList(num_eval=0): ragged vs per-file max score difference", err)
    assert err <= 1e-4
    for branch in (S_rag.ECAPA_TDNN, S_rag.rawnet2v2):
        assert len(branch._engines) == 1 and branch._engine.max_batch == 16
    assert len(S_per.ECAPA_TDNN._engines) > 1 and len(S_per.rawnet2v2._engines) > 1
    csv_path = tmp_path / "pairs.txt"
    csv_path.write_text("audio_1,audio_2\n" + "".join(f"{files[i]},{files[i + 1]}\n" for i in range(4)))
    res_r = rag.testFromList(test_list=str(csv_path), thresh_score=0.5, cohorts_path=None, num_eval=0, scoring_mode="cosine",
                             output_file=str(tmp_path / "out_r.txt"))
    res_p = per.testFromList(test_list=str(csv_path), thresh_score=0.5, cohorts_path=None, num_eval=0, scoring_mode="cosine",
                             output_file=str(tmp_path / "out_p.txt"))
    s_r = np.array([float(r.split(",")[-1]) for r in res_r])
    s_p = np.array([float(r.split(",")[-1]) for r in res_p])
    assert len(s_r) == 4 and float(np.abs(s_r - s_p).max()) <= 1e-4
    assert len(S_rag.ECAPA_TDNN._engines) == 1 and len(S_rag.rawnet2v2._engines) == 1
    # a CUDA pack keeps forward's two-stream overlap and gives the bits of the host pack
    wavs = _waves(((1401, 0), (760, 1), (1297, 2)), first=7)
    host = S_rag.embed_ragged(wavs)
    dev = S_rag.embed_ragged([torch.from_numpy(w).cuda() for w in wavs])
    assert host.shape == (3, 512) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)


def test_whole_file_evaluation_in_the_half_mode(tmp_path):
    """hip_compute = 'half' (ECAPA bf16 + RawNet2 fp16, the configured fast mode) rides on ragged calls too.  Both runs hold each
    branch's embedding to that branch's end-to-end bar of the oracle (rawnet2_oracle_check f16, ecapa_oracle_check bf16), and a cosine
    score of the concatenated embeddings moves by no more than the relative change of its two vectors: the scores of the two runs
    lie within the sum of the two branches' bars of each other."""
    tmp = str(tmp_path)
    files, trial_path, lines = make_e2e_files(tmp)
    rag, S_rag, args = _handler(tmp, compute="half")
    per, _, _ = _handler(tmp, compute="half", ragged_eval=False)
    kw = dict(listfilename=trial_path, distributed=False, dataloader_options=args["dataloader_options"], cohorts_path="unused", num_eval=0,
              scoring_mode="cosine")
    sc_r = np.array(rag.evaluateFromList(**kw)[0])
    sc_p = np.array(per.evaluateFromList(**kw)[0])
    bar = chk.bar("f16", "end_to_end") + ECAPA_BF16_BARS["end_to_end"]
    err = float(np.abs(sc_r - sc_p).max())
    print(f"Raw_ECAPA_conv_asp half: ragged vs per-file max score difference {err:.3g} (bar {bar})")
    assert np.isfinite(sc_r).all() and len(sc_r) == len(lines) and err <= bar
    assert S_rag.rawnet2v2._engine.compute == "f16" and S_rag.ECAPA_TDNN._engine.compute == "bf16"
    assert len(S_rag.ECAPA_TDNN._engines) == 1 and len(S_rag.rawnet2v2._engines) == 1
