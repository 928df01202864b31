"""GPU: RawNet2 against the float64 oracle (oracle/rawnet2.py), block by block, on every kernel route of the forward.

Each case runs one forward with option rn_keep, layer labels and profiling on, reads every tensor the route stored and compares, for
the checked utterances, each with the oracle's step applied to the handle's own stored input (tests/rawnet2_oracle_check.py: the
checks, the bars and the measured values beside them).  The shapes are the smallest that reach each kernel form: the shortest
utterance (2438 samples: every T a power of 3, one frame at the end, a short last tile in rn_block128), lengths where every pool
drops a remainder, lengths on both sides of each limit of the kernels (derived below from the limits restated here), one
L = 32000 case per compute, the batches at which kernels switch, two lanes, every developer option that forces a kernel form and
all three model ids.  The census test asserts the exact set of kernels each compute reached."""
import hashlib

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from tests import rawnet2_oracle_check as chk

pytestmark = pytest.mark.gpu

SEED_W, SEED_X = 7, 20220829
ERR_STATE = -3                               # include/svhip.h
NOUT = 320
_SD, _REF = {}, {}
_CENSUS = {c: {} for c in chk.COMPUTES}
_INFO = {}


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the kernels' limits, restated (rawnet2.hip: rn_tail_supported, rn_tail_slices, SINC_PT; r2_step.hip: mode 3's tile) ----
def tail_supported(es, Tn, C):
    """the one-launch block tail holds an utterance's pooled activation in the registers of 1024 threads, 16 chunks of 16 bytes each"""
    return Tn * (C // (8 if es == 2 else 4)) <= 16 * 1024


def tail_slices(es, B, Tn, C, num_cu):
    """slices per utterance of the tail's sliced form (0: one workgroup per utterance, the gate stays on chip)"""
    cpr = C // (8 if es == 2 else 4)
    if cpr < 32 or 256 % cpr:
        return 0
    if B * 4 > num_cu:
        return 0 if C < 256 or Tn > 48 else (Tn + 15) // 16
    S = min((Tn + 47) // 48, 16)
    return S if S >= 2 else 0


def _sinc_L(T1):
    return 250 + 3 * T1


def _first_block(C):
    return next(i for i, blk in enumerate(chk.BLOCKS) if blk[2] == C)


def _L_for(C, Tn):
    """the shortest sinc utterance whose first block with C output channels leaves Tn frames"""
    div = 3 ** sum(blk[3] for blk in chk.BLOCKS[:_first_block(C) + 1])
    return _sinc_L(max(Tn * div, 729))


def limit_lengths():
    """[(tag, computes, L)]: lengths on both sides of each limit.  Not reachable: the tail's limit and the slice rule at C = 128 on
    16-bit handles (their 128-channel blocks run fused, rn_block128; with rn_unfused no tail runs), and 48 | 49 frames at C = 128 (the
    shortest utterance leaves block 1 81 frames)."""
    out = [("SINC_PT 768", chk.COMPUTES, _sinc_L(768)), ("SINC_PT 769", chk.COMPUTES, _sinc_L(769))]
    for C in (256, 512):
        out += [(f"slices C={C} Tn={Tn}", chk.COMPUTES, _L_for(C, Tn)) for Tn in (48, 49)]
    for es, computes in ((4, ("f32", "f32x3")), (2, ("f16", "bf16"))):
        for C in ((128, 256, 512) if es == 4 else (256, 512)):
            lim = max(Tn for Tn in range(1, 2000) if tail_supported(es, Tn, C))
            assert tail_supported(es, lim, C) and not tail_supported(es, lim + 1, C)
            out += [(f"tail C={C} Tn={Tn}", computes, _L_for(C, Tn)) for Tn in (lim, lim + 1)]
    # r2_step mode 3 (F32X3, conv2 pools on its way out where the tail does not take the block): tiles of 126 frames of one utterance
    out += [(f"r2_step T1={T1}", ("f32x3",), _sinc_L(T1)) for T1 in (126 * 13, 126 * 13 + 2, 126 * 13 + 3)]
    return out


def _rows(B, lanes=1):
    if B <= 3:
        return list(range(B))
    rows = {0, B // 2, B - 1}
    if lanes > 1:
        per = ((B + lanes - 1) // lanes + 3) & ~3
        rows |= {per - 1, per}
    return sorted(rows)


def _sd(model, L, compute):
    key = (model, L)
    if key not in _SD:
        spec = synth.rawnet2_param_spec(nOut=NOUT, nb_samp=L, front_proc="conv" if model == "rawnet2_conv" else "sinc",
                                        aggregate="gru" if model == "rawnet2_gru" else "asp")
        sd = synth.synth_state_dict(spec, seed=SEED_W)
        _SD[key] = (sd, chk.torch_sd(sd), {})
    sd, sd64, q = _SD[key]
    if compute not in q:
        q[compute] = chk.rounded_sd(sd64, compute)
    return sd, sd64, q[compute]


def _e2e(wav, model, L):
    key = hashlib.sha1(wav.tobytes() + model.encode()).hexdigest()
    if key not in _REF:
        _REF[key] = chk.end_to_end(wav, _sd(model, L, "f32")[1], model)
    return _REF[key]


def _cols(name):
    if name in ("front",):
        return 128
    if name in ("agg_in", "logits"):
        return 512
    if name in ("pooled", "gru_h"):
        return 1024
    i, what = int(name[1]), name.split("_", 1)[1]
    return chk.BLOCKS[i][1] if what in ("pre", "x") else chk.BLOCKS[i][2]


def stage_names(model):
    names = ["front", "agg_in"] + [f"b{i}_{w}" for i in range(8) for w in ("pool", "gate", "pre", "x", "o", "c2")]
    return names + (["gru_h"] if model == "rawnet2_gru" else ["logits", "pooled"])


def _stages(e, B, model):
    """every kept stage of the last forward as float64 (B, rows, channels) / (B, n); a stage the route did not store is refused with
    SVHIP_ERR_STATE and left out"""
    S = {}
    for n in stage_names(model):
        try:
            a = e.get_stage("rn_" + n).astype(np.float64)
        except _lib.SvhipError as err:
            assert err.code == ERR_STATE, (n, err.code, str(err))
            continue
        a = a.reshape(B, -1, _cols(n))
        S[n] = a[:, 0] if a.shape[1] == 1 and n.endswith(("gate", "pooled", "gru_h")) else a
    return S


def run_case(compute, L, B, model="rawnet2", options=None, lanes=1, tag="", monkeypatch=None):
    """one forward, its kept stages against the oracle at _rows; returns (embeddings, kernel labels, the stages kept)"""
    if lanes > 1:
        monkeypatch.setenv("SVHIP_LANES", str(lanes))
    sd, sd64, sdq = _sd(model, L, compute)
    e = Engine(model=model, compute=compute, embed_dim=NOUT, max_batch=B, samples=L)
    if lanes > 1:
        monkeypatch.delenv("SVHIP_LANES")
    e.load_state_dict(sd)
    e.finalize()
    for k, v in (options or {}).items():
        e.set_option(k, v)
    e.set_option("rn_keep", 1)
    e.set_option("layer_labels", 1)
    e.profile(True)
    x = synth.synth_waveforms(B, L, seed=SEED_X + L)
    emb = e.embed_wave(x).reshape(B, -1).astype(np.float64)
    labels = sorted({n.split()[0] for n in e.profile_results()})
    e.profile(False)
    assert e.numeric_status() == 0 and np.isfinite(emb).all()
    S = _stages(e, B, model)
    e.close()
    worst, bad = {}, []
    for b in _rows(B, lanes):
        err = chk.layer_local(S, b, sdq, x[b], model, compute, emb=emb[b], e2e_ref=_e2e(x[b], model, L))
        print(f"{tag} {compute} {model} L={L} B={B} b={b}: {chk.describe(err)}")
        chk.by_kind(err, worst)
        bad += [(b,) + f for f in chk.failures(err, compute)]
    print(f"WORST {compute} " + " ".join(f"{k}={v:.3e}" for k, v in sorted(worst.items())))
    _CENSUS[compute][tag] = labels
    _INFO[(compute, tag)] = sorted(S)
    assert not bad, (tag, compute, model, L, B, bad)
    return emb, labels, sorted(S)


# ---- the cases: (tag, compute, L, B, keyword arguments of run_case) ----------------------------------------------------------
def _length_cases():
    out = []
    for c in chk.COMPUTES:
        out += [("L=2438", c, 2438, 2, {}), ("L=2441", c, 2441, 3, {}), ("L=4003", c, 4003, 1, {}), ("L=32000", c, 32000, 2, {}),
                ("L=96000", c, 96000, 1, {})]
    return out


def _limit_cases():
    out = [(tag, c, L, 1, {}) for tag, computes, L in limit_lengths() for c in computes]
    # the slice rule of full batches (B * 4 > CUs: 16-frame slices up to 48 frames at C >= 256, one workgroup per utterance beyond)
    return out + [(tag + " full batch", c, L, "CUs/4+1", {}) for tag, computes, L in limit_lengths() if tag.startswith("slices C=256") for c in computes]


def _batch_cases():
    """64 | 65: rn_afms_gate and rowvec_linear switch kernels; B * 4 > CUs: the tail's full-batch form; B = 32 on two lanes"""
    out = []
    for c in chk.COMPUTES:
        out += [(f"B={B}", c, 2438, B, {}) for B in (64, 65, "CUs/4+1")]          # (the last one from the device, in _case)
        out.append(("two lanes B=32", c, 2438, 32, dict(lanes=2)))
    return out


MODEL_CASES = tuple((f"{m} L={L}", c, L, B, dict(model=m)) for c in chk.COMPUTES
                    for m, L, B in (("rawnet2_conv", 2187, 2), ("rawnet2_conv", 2192, 3), ("rawnet2_gru", 2438, 2), ("rawnet2_gru", 4003, 3)))
# (tag, computes, L, B, options, model)
FORCED = (
    ("rn_unfused", chk.COMPUTES, 2441, 2, dict(rn_unfused=1), "rawnet2"),
    # (bf16: the lengths at which the recovered gate is too coarse for one dropped frame, on the route that stores every gate —
    #  tests/test_rawnet2_oracle_host.py: GATE_REC_TOO_COARSE)
    ("rn_unfused L=4003", ("bf16",), 4003, 1, dict(rn_unfused=1), "rawnet2"),
    ("rn_unfused L=4219", ("bf16",), 4219, "CUs/4+1", dict(rn_unfused=1), "rawnet2"),
    ("rn_unfused L=32000", ("bf16",), 32000, 2, dict(rn_unfused=1), "rawnet2"),
    ("rn_unfused L=35242", ("bf16",), 35242, 1, dict(rn_unfused=1), "rawnet2"),
    ("rn_unfused L=96000", ("bf16",), 96000, 1, dict(rn_unfused=1), "rawnet2"),
    ("rn_conv_unfused", ("f16", "bf16"), 2192, 2, dict(rn_conv_unfused=1), "rawnet2_conv"),
    ("rn_tail_big", chk.COMPUTES, 4219, 2, dict(rn_tail_big=1), "rawnet2"),
    ("rn_step_off", ("f32x3",), 2441, 2, dict(rn_step_off=1), "rawnet2"),
    ("rn_pool_off", ("f32x3",), 5170, 1, dict(rn_pool_off=1), "rawnet2"),
    ("rn_sinc_f32", ("f32x3",), 2441, 2, dict(rn_sinc_f32=1), "rawnet2"),
    ("rn_sinc_full", ("f16",), 2441, 2, dict(rn_sinc_full=1), "rawnet2"),
    # the persistent conv-gather GEMM takes a k = 3 layer of a 16-bit handle when it has more 256 x 256 tiles than the grid cap: with the
    # cap at 1 - 3 workgroups, 8002 samples at B = 3 (287 and 95 frames in the 256-channel blocks: 4 and 2 row tiles) put block 2's conv1
    # on it (cap 2, 3) and, at cap 1, both convolutions of blocks 3 and 4, whose tails then add the identity shortcut (stage rn_b<i>_c2)
    ("cv_off", ("f16", "bf16"), 8002, 3, dict(cv_off=1, pw3_cus=1), "rawnet2"),
    ("n128_off", ("f16", "bf16"), 2441, 2, dict(n128_off=1), "rawnet2"),            # (gemm_n128 is ECAPA's: no RawNet2 layer has its epilogue)
    ("pw3_cus=1", ("f16", "bf16", "f32x3"), 8002, 3, dict(pw3_cus=1), "rawnet2"),
    ("pw3_cus=2", ("f16", "bf16", "f32x3"), 8002, 3, dict(pw3_cus=2), "rawnet2"),
    ("pw3_cus=3", ("f16", "bf16", "f32x3"), 8002, 3, dict(pw3_cus=3), "rawnet2"),
    ("pw3_cus=0", ("f16", "bf16", "f32x3"), 8002, 3, dict(pw3_cus=0), "rawnet2"),
)


def _forced_cases():
    return [(f"forced {t}", c, L, B, dict(options=o, model=m)) for t, computes, L, B, o, m in FORCED for c in computes]


def _all_cases():
    return _length_cases() + _limit_cases() + _batch_cases() + list(MODEL_CASES) + _forced_cases()


def _case(case, monkeypatch):
    tag, compute, L, B, kw = case
    if tag not in _CENSUS[compute]:
        B = _num_cu() // 4 + 1 if B == "CUs/4+1" else B
        run_case(compute, L, B, tag=tag, monkeypatch=monkeypatch, **kw)
    return _CENSUS[compute][tag], _INFO[(compute, tag)]


_ids = lambda c: f"{c[0]}-{c[1]}"


@pytest.mark.parametrize("case", _length_cases(), ids=_ids)
def test_blocks_at_base_lengths(case, monkeypatch):
    """`pooled` on fp32-grade handles exposed a kernel error: rn_attn_pool took the variance as sum(w x^2) - m^2, whose fp32 difference
    keeps the rounding of x^2 (up to 2^-24 x^2: past the 1e-5 clamp from |x| = 13 on), so that with one frame at the aggregation
    (utterances of up to 4 624 samples) a std came out up to 1.5 times the reference's sqrt(1e-5) (1.2e-4 of the pooled vector's scale,
    8.4e-5 of the embedding's); the kernel now sums w (x - m)^2 (2.5e-7, and 2.0e-5 end to end).

    2438 samples (T1 = 729, every later T a power of 3, one frame reaches the aggregation), 2441 and 4003 (L % 8 != 0, pools that drop
    a remainder: 730 -> 243 and 1251 -> 417 -> 139 -> 46 -> 15 -> 5 -> 1), the reference configs' 32000 at B = 2, and 96000 (43 frames reach
    the aggregation)"""
    _case(case, monkeypatch)


@pytest.mark.parametrize("case", _limit_cases(), ids=_ids)
def test_blocks_on_both_sides_of_the_kernels_limits(case, monkeypatch):
    """the sinc kernel's 64-frame tile, the tail's 48-frame slice rule, the longest utterance the one-launch tail takes at each width and
    element size, r2_step's 126-frame pooled tile"""
    tag, compute, L, B, _ = case
    _, kept = _case(case, monkeypatch)
    if tag.startswith("slices"):
        C, Tn = int(tag.split("C=")[1].split()[0]), int(tag.split("Tn=")[1].split()[0])
        i = chk.BLOCKS.index(next(b for b in chk.BLOCKS if b[2] == C))
        es = 2 if compute in ("f16", "bf16") else 4
        B = _num_cu() // 4 + 1 if B == "CUs/4+1" else B
        assert (f"b{i}_gate" in kept) == (tail_slices(es, B, Tn, C, _num_cu()) > 0), (tag, compute, kept)


def test_limit_lengths_sit_on_the_limits():
    """the derived lengths: the block meant has exactly the frames asked for, and the two sides differ in what they reach"""
    for tag, computes, L in limit_lengths():
        fr = chk.frames_after(chk.front_frames(L, "rawnet2"))
        if "Tn=" in tag:
            C, Tn = int(tag.split("C=")[1].split()[0]), int(tag.split("Tn=")[1])
            assert fr[_first_block(C)][1] == Tn, (tag, L, fr)
    es4 = {C: max(Tn for Tn in range(1, 2000) if tail_supported(4, Tn, C)) for C in (128, 256, 512)}
    es2 = {C: max(Tn for Tn in range(1, 2000) if tail_supported(2, Tn, C)) for C in (128, 256, 512)}
    assert es4 == {128: 512, 256: 256, 512: 128} and es2 == {128: 1024, 256: 512, 512: 256}


@pytest.mark.parametrize("case", _batch_cases(), ids=_ids)
def test_blocks_at_the_batch_size_switches(case, monkeypatch):
    _case(case, monkeypatch)


@pytest.mark.parametrize("case", MODEL_CASES, ids=_ids)
def test_blocks_of_the_conv_and_gru_models(case, monkeypatch):
    """front_proc='conv' at its own minimum length (2187 samples) and at one where its stride drops samples; aggregate='gru' with one
    and with five frames reaching the GRU"""
    tag, compute, L, B, kw = case
    labels, kept = _case(case, monkeypatch)
    if kw["model"] == "rawnet2_conv":
        fused = compute in ("f16", "bf16")       # block 0 reads the waveform: no front-end tensor
        assert ("front" not in kept) == fused and ("rn_block128_conv" in labels) == fused, (labels, kept)


@pytest.mark.parametrize("case", _forced_cases(), ids=_ids)
def test_forced_kernel_forms_meet_the_oracle(case, monkeypatch):
    """each developer option that forces a kernel form: the forced kernels meet the oracle bars themselves"""
    tag, compute, L, B, kw = case
    labels, kept = _case(case, monkeypatch)
    opts = kw["options"]
    half = compute in ("f16", "bf16")
    if "rn_unfused" in opts:
        assert not {"rn_tail", "rn_block128"} & set(labels) and "rn_afms_mean" in labels, labels
        assert ("rn_maxpool3" in labels) == (compute != "f32x3"), labels          # (F32X3: conv2 pools on its way out, r2_step mode 3)
        assert all(f"b{i}_gate" in kept for i in range(8)), kept
    if "rn_conv_unfused" in opts:
        assert "rn_conv3_front" in labels and "rn_block128_conv" not in labels and "front" in kept, (labels, kept)
    if "rn_tail_big" in opts:
        assert not [n for n in kept if n.endswith("_gate") and f"{n[:2]}_pool" not in kept], kept
    if "rn_step_off" in opts:
        assert "rn_step" not in labels, labels
    if "rn_pool_off" in opts:
        assert "rn_maxpool3" in labels, labels
    if "cv_off" in opts:
        assert "gemm_pw3cv16" not in labels and not [n for n in kept if n.endswith("_c2")], (labels, kept)
    elif half and opts.get("pw3_cus", 0) > 0:
        assert "gemm_pw3cv16" in labels, labels
        assert ({"b3_c2", "b4_c2"} <= set(kept)) == (opts["pw3_cus"] == 1), kept
    if "n128_off" in opts:
        assert "gemm_n128" not in labels, labels
    if opts.get("pw3_cus") == 0:
        assert not [n for n in labels if n.startswith("gemm_pw3")], labels
    assert ("rn_block128" in labels) == (half and "rn_unfused" not in opts), labels


# every kernel each compute reached over the cases of this file (profile labels; the GEMMs by kernel).  Not reached by any RawNet2
# geometry: gemm_n128 (its ReLU + tanh epilogue is ECAPA's asp.tdnn) and the persistent 1 x 1 kernel gemm_pw3 (no RawNet2 1 x 1 layer
# has both a bias and a BN epilogue on a 256-column output).  gemm_pw3cv16 takes a k = 3 layer with more tiles than the grid: here
# through option pw3_cus, at full batches (tests/test_gpu_fullsize.py) on its own.
_F32 = {"emb_out", "gemm_conv", "gemm_pw", "rn_afms_apply", "rn_afms_gate", "rn_afms_mean", "rn_attn_pool", "rn_bn_act", "rn_conv3_front",
        "rn_fc", "rn_gru_fc", "rn_gru_proj", "rn_gru_step", "rn_ln_stats", "rn_maxpool3", "rn_sinc", "rn_tail"}
_H16 = _F32 | {"gemm_pw2_conv", "gemm_pw3cv16", "rn_block128", "rn_block128_conv"}
CENSUS_WANT = {"f32": _F32, "f32x3": _F32 | {"rn_step"}, "f16": _H16, "bf16": _H16}


@pytest.mark.parametrize("compute", chk.COMPUTES)
def test_route_census(compute, monkeypatch):
    """every kernel a RawNet2 forward of this compute reaches ran in a case checked against the oracle, and nothing else ran"""
    for case in _all_cases():
        if case[1] == compute:
            _case(case, monkeypatch)
    seen = set()
    for tag, labels in sorted(_CENSUS[compute].items()):
        print(f"census {compute} {tag}: {' '.join(labels)}")
        seen |= set(labels)
    print(f"census {compute}: {sorted(seen)}")
    assert seen == CENSUS_WANT[compute], (sorted(seen - CENSUS_WANT[compute]), sorted(CENSUS_WANT[compute] - seen))


@pytest.mark.parametrize("compute", chk.COMPUTES)
@pytest.mark.parametrize("model,L,B,lanes", [("rawnet2", 4219, 3, 1), ("rawnet2_gru", 2441, 32, 2), ("rawnet2_conv", 2192, 2, 1)])
def test_keeping_the_stages_leaves_the_forward_alone(compute, model, L, B, lanes, monkeypatch):
    """option rn_keep on and off: the same profile labels with the same launch counts, bit-identical embeddings; with the option off
    every kept stage is refused with SVHIP_ERR_STATE.  (Two lanes: each stage's slices land side by side; rn_gru_in stays refused.)"""
    if lanes > 1:
        monkeypatch.setenv("SVHIP_LANES", str(lanes))
    e = Engine(model=model, compute=compute, embed_dim=NOUT, max_batch=B, samples=L)
    monkeypatch.delenv("SVHIP_LANES", raising=False)
    e.load_state_dict(_sd(model, L, compute)[0])
    e.finalize()
    e.set_option("layer_labels", 1)
    x = synth.synth_waveforms(B, L, seed=77)
    got = {}
    for keep in (0, 1, 0):
        e.set_option("rn_keep", keep)
        e.profile(True)
        emb = e.embed_wave(x).copy()
        prof = {n: r["launches"] for n, r in e.profile_results().items()}
        e.profile(False)
        kept = _stages(e, B, model)
        if keep:
            assert {"agg_in", "b7_pre"} <= set(kept) and all(np.isfinite(a).all() for a in kept.values()), sorted(kept)
            got["kept"] = kept
        else:
            assert not set(kept) - {"pooled", "gru_h"}, sorted(kept)       # (rn_pooled / rn_gru_h are the forward's own buffers)
        if "emb" in got:
            assert prof == got["prof"], (keep, prof, got["prof"])
            assert np.array_equal(emb, got["emb"])
        got["emb"], got["prof"] = emb, prof
    if model == "rawnet2_gru" and lanes > 1:
        with pytest.raises(_lib.SvhipError):
            e.get_stage("rn_gru_in")
    e.close()
