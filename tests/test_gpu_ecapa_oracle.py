"""GPU: ECAPA-TDNN against the float64 oracle (oracle/ecapa.py), stage by stage, on every kernel route of the forward.

Each case runs one forward with layer labels and profiling on, reads every stage the handle exposes and compares, for the checked
utterances, each stage with the oracle's block applied to the handle's own previous stage (tests/ecapa_oracle_check.py: the checks,
the bars and the measured values beside them).  The cases put each GEMM on each of its kernels (the batches derived from the CU
count), run the Res2Net chain whole and in time slices and the per-layer fallback, take the SE squeeze and the ASP statistics from
the GEMMs' column sums and from their own kernels, reach every ASP kernel and both front-ends, run two lanes, the lengths at the
edges of the kernels' limits, C = 1024 and 512 (and C = 128 for the ASP kernels only it reaches), every developer option that forces
a kernel form, and the headline configuration (C = 1024, bf16, B = 256, L = 32000).  The census test asserts the exact set of
kernels each compute reached."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import ecapa as o_ecapa, fbank as o_fbank
from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from tests import ecapa_oracle_check as chk

pytestmark = pytest.mark.gpu

SEED_W, SEED_X = 5, 20220829
ERR_STATE = -3                               # include/svhip.h
_SD = {}
_REF = {}
_CENSUS = {"f32": {}, "f32x3": {}, "bf16": {}}


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _frames(L, hop=80):
    return L // hop + 1


def _pw3_regime(M, N, num_cu):
    """gemm_route (gemm.hip) of a bf16 1 x 1 GEMM with the pw3 epilogue at the default options (grid cap = CUs, tail split on)"""
    tiles = -(-M // 256) * (N // 256)
    return "gemm_pw3" if tiles > num_cu else ("gemm_pw3/halves" if 2 * tiles <= num_cu else "gemm_pw2")


def _route_batches(C, L, num_cu, b_max=96):
    """the smallest batch at which tdnn1 / tdnn2 (N = C) and mfa (N = 3C) reach each of their kernels"""
    T = _frames(L)
    picks = {}
    for name, N in (("tdnn", C), ("mfa", 3 * C)):
        for B in range(1, b_max + 1):
            picks.setdefault((name, _pw3_regime(B * T, N, num_cu)), B)
    return picks


def _rows(B, T, lanes=1):
    """every row for B <= 3; else the first, the last, the utterance over the middle 256-row tile boundary and, with two lanes, both
    rows beside the lane split"""
    if B <= 3:
        return list(range(B))
    rows = {0, B - 1, min(B - 2, max(1, (256 * ((B * T // 2) // 256)) // T))}
    if lanes == 2 and B >= 64:
        per = (B // 2 + 3) & ~3
        rows |= {per - 1, per}
    return sorted(rows)


def _sd(C, input_norm=False, n_mels=80):
    key = (C, input_norm, n_mels)
    if key not in _SD:
        sd = synth.synth_state_dict(synth.ecapa_param_spec(C=C, n_mels=n_mels, input_norm=input_norm), seed=SEED_W)
        sd64 = chk.torch_sd(sd)
        _SD[key] = (sd, sd64, chk.rounded_sd(sd64, C))
    return _SD[key]


def _oracle(x_row, C, wave, input_norm, fe, n_mels):
    """(the oracle's input features (1, n_mels, T), its embedding end to end) of one utterance, cached by input hash"""
    key = hashlib.sha1(x_row.tobytes() + repr((C, wave, input_norm, sorted(fe.items()), n_mels)).encode()).hexdigest()
    if key not in _REF:
        _, sd64, _ = _sd(C, input_norm, n_mels)
        with torch.no_grad():
            x = torch.from_numpy(x_row).double()[None]
            mel = o_fbank.melspectrogram(x, n_mels=n_mels, **fe) if wave else x
            feat = chk.features(mel, sd64, input_norm)
            _REF[key] = (feat, o_ecapa.ecapa_forward(feat, sd64, features="none").reshape(-1).numpy())
    return _REF[key]


def _stages(e, B, T, C):
    """every stage of the handle's last forward as float64, (B, T, channels) or (B, n); None where the route does not produce it"""
    S = {}
    for n in chk.HANDLE_STAGES:
        try:
            a = e.get_stage(n).astype(np.float64)
        except _lib.SvhipError as err:
            assert err.code == ERR_STATE and n == "blocks.3.tdnn1" and e.compute == "f32x3", (n, err.code, str(err))
            S[n] = None
            continue
        S[n] = a.reshape(B, -1) if n in chk.VECTOR_STAGES else a.reshape(B, T, -1)
    return S


def run_case(compute, C, L, B, rows=None, wave=True, options=None, lanes=1, input_norm=False, n_fft=512, n_mels=80, tag="",
             monkeypatch=None, front=None):
    """one forward, its stages against the oracle at `rows` (default _rows); returns (embeddings, kernel labels, the worst error of
    every check).  Every error is printed; the bars are asserted after the whole case.  front: the front-end keywords of the handle
    and of the oracle (sr, n_fft, win_length, hop_length, fmin, fmax) where they are not the defaults."""
    fe = dict(dict(n_fft=n_fft), **(front or {}))
    T = _frames(L, fe.get("hop_length", 80))
    if lanes > 1:
        monkeypatch.setenv("SVHIP_LANES", str(lanes))
    sd, sd64, sdq = _sd(C, input_norm, n_mels)
    e = Engine(model="ecapa", compute=compute, channels=C, max_batch=B, samples=L, input_norm=input_norm, n_mels=n_mels, **fe)
    if lanes > 1:
        monkeypatch.delenv("SVHIP_LANES")
    e.load_state_dict(sd)
    e.finalize()
    for k, v in (options or {}).items():
        e.set_option(k, v)
    e.set_option("layer_labels", 1)
    e.profile(True)
    x = synth.synth_waveforms(B, L, seed=SEED_X + L) if wave else synth.synth_mel(B, n_mels, T, seed=SEED_X + T)
    emb = (e.embed_wave(x) if wave else e.embed_features(x)).reshape(B, -1).astype(np.float64)
    labels = sorted({n.split()[0] for n in e.profile_results()})
    e.profile(False)
    assert e.numeric_status() == 0 and np.isfinite(emb).all()
    S = _stages(e, B, T, C)
    e.close()
    worst, bad = {}, []
    for b in (_rows(B, T, lanes) if rows is None else rows):
        feat, e2e = _oracle(x[b], C, wave, input_norm, fe, n_mels)
        err = chk.layer_local(S, b, sdq if compute == "bf16" else sd64, ref_input=feat, emb=emb[b], e2e_ref=e2e,
                              bf16=compute == "bf16")
        print(f"{tag} {compute} C={C} T={T} B={B} b={b}: {chk.describe(err)}")
        for n, (v, _) in err.items():
            worst[n] = max(worst.get(n, 0.0), v)
        bad += [(b,) + f for f in chk.failures(err, compute)]
    _CENSUS[compute][tag or f"C={C} L={L} B={B} {options}"] = labels
    assert not bad, (tag, compute, C, T, B, bad)
    return emb, labels, worst


# (tag, compute, C, L, B, keyword arguments of run_case)
LENGTHS = (("T=5", 320, dict(wave=False, n_fft=256)), ("T=9", 640, {}), ("T=33", 2560, {}), ("T=201", 16000, {}),
           ("T=255", 20320, {}), ("T=256", 20400, {}), ("T=401", 32000, {}), ("T=416", 33200, {}), ("T=417", 33280, {}),
           ("T=1001", 80000, {}), ("L=32037", 32037, {}))


def _length_cases():
    out = []
    for tag, L, kw in LENGTHS:
        out.append((tag, "bf16", 1024, L, 2, kw))
        if tag in ("T=5", "T=9", "T=256", "T=417"):
            out += [(tag, "f32", 1024, L, 2, kw), (tag, "f32x3", 1024, L, 2, kw)]
    return out


FRONT_16K = dict(sr=16000, n_fft=512, win_length=400, hop_length=160)      # T = 201: the 64-frame fbank kernel at 76.9 KB of LDS
OTHER_CASES = (
    ("C=512", "bf16", 512, 32000, 2, {}),
    ("C=512", "f32", 512, 32000, 2, {}),
    ("C=512 pw3r2", "f32x3", 512, 32000, 2, {}),
    ("C=128 asp_fused", "bf16", 128, 32000, 2, {}),
    ("C=128 asp_pool", "bf16", 128, 33280, 2, {}),
    ("features", "bf16", 1024, 32000, 3, dict(wave=False)),
    ("features input_norm", "bf16", 1024, 32000, 2, dict(wave=False, input_norm=True)),
    ("n_mels=128", "f32x3", 1024, 32000, 2, dict(n_mels=128)),
    ("per-file crops B=10", "bf16", 1024, 32000, 10, {}),
    ("per-file crops B=20", "bf16", 1024, 32000, 20, {}),
    ("two lanes B=64", "bf16", 1024, 32000, 64, dict(lanes=2)),
    ("16 kHz front-end", "bf16", 512, 32000, 2, dict(front=FRONT_16K)),
    ("16 kHz front-end", "f32", 512, 32000, 2, dict(front=FRONT_16K)),
)
FORCED = (
    ("pw3_cus=2", "bf16", dict(pw3_cus=2)),
    ("pw3_cus=3 tail_off", "bf16", dict(pw3_cus=3, pw3_tail_off=1)),
    ("pw3_tail_off", "bf16", dict(pw3_tail_off=1)),
    ("pw3_cus=0", "bf16", dict(pw3_cus=0)),
    ("r2_slices=3", "bf16", dict(r2_slices=3)),
    ("r2_slices=0", "bf16", dict(r2_slices=0)),
    ("asp_v1", "bf16", dict(asp_v1=1)),
    ("n128_off", "bf16", dict(n128_off=1)),
    ("cv_off", "bf16", dict(cv_off=1)),
    ("fbank_unfused", "bf16", dict(fbank_unfused=1)),
    ("r2_big", "f32x3", dict(r2_big=1)),
    ("x3_keep_f32", "f32x3", dict(x3_keep_f32=1)),
    ("pw3_cus=2", "f32x3", dict(pw3_cus=2)),
)


def _route_cases():
    picks = _route_batches(1024, 32000, _num_cu())
    return [(f"route B={B}", "bf16", 1024, 32000, B, {}) for B in sorted(set(picks.values()))]


def _cv16_case():
    """bf16 blocks.0 on gemm_pw3cv16: its conv-gather form takes input channels in multiples of 64 (128 mels) and runs when the grid
    has more tiles than CUs.  (fbank_fused_supported admitted banks of up to 128 mels that its launcher refuses — more than 80 outputs
    per thread and pass — so embed_wave failed with "invalid argument"; such banks now take the separate kernels.)"""
    B = _route_batches(1024, 32000, _num_cu())[("tdnn", "gemm_pw3")]
    return ("n_mels=128 pw3cv16", "bf16", 1024, 32000, B, dict(n_mels=128))


def _all_cases():
    out = _length_cases() + list(OTHER_CASES) + _route_cases() + [_cv16_case()]
    out += [(f"forced {t}", c, 1024, 32000, 2, dict(options=o)) for t, c, o in FORCED]
    out += [("forced asp_v1 T=417", "bf16", 1024, 33280, 2, dict(options=dict(asp_v1=1)))]
    return out


def _case(case, monkeypatch):
    tag, compute, C, L, B, kw = case
    if tag not in _CENSUS[compute]:
        run_case(compute, C, L, B, tag=tag, monkeypatch=monkeypatch, **kw)
    return _CENSUS[compute][tag]


@pytest.mark.parametrize("case", _length_cases(), ids=lambda c: f"{c[0]}-{c[1]}")
def test_stages_at_edge_lengths(case, monkeypatch):
    """T = 5 (the shortest the reference takes: block 3 reflects 4 frames), 9 (the fused chain's first length at dilation 4), 33,
    201, 255 / 256 (column sums from the GEMM epilogues from T = 256 on), 401, 416 / 417 (R2_TMAX / AF_TMAX: the chain and asp_fused
    up to 416 frames), 1001, and a sample count that is not a multiple of the hop"""
    _case(case, monkeypatch)


@pytest.mark.parametrize("case", OTHER_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_stages_on_other_geometries(case, monkeypatch):
    _case(case, monkeypatch)


def test_another_front_end_takes_the_separate_kernels(monkeypatch):
    """fbank_fused_supported takes the default window, FFT size and hop only: a bf16 handle at any other geometry runs fbank and the
    prologue, and meets the same bars"""
    labels = _case(next(c for c in OTHER_CASES if c[0] == "16 kHz front-end" and c[1] == "bf16"), monkeypatch)
    assert "fbank" in labels and "prologue" in labels and "fbank_fused" not in labels, labels


def test_stages_on_every_gemm_route(monkeypatch):
    """bf16, C = 1024, L = 32000 at the smallest batch that puts tdnn1 / tdnn2 and mfa on each of their kernels (derived from the CU
    count: the persistent gemm_pw3 as column halves, gemm_pw2, the whole-tile gemm_pw3)"""
    picks = _route_batches(1024, 32000, _num_cu())
    print("route batches:", {f"{n} {r}": B for (n, r), B in sorted(picks.items(), key=lambda kv: kv[1])})
    assert len({r for (n, r) in picks if n == "tdnn"}) == 3 and len({r for (n, r) in picks if n == "mfa"}) == 3, picks
    for case in _route_cases():
        _case(case, monkeypatch)


def test_stages_with_blocks0_on_the_conv_gather_kernel(monkeypatch):
    assert "gemm_pw3cv16" in _case(_cv16_case(), monkeypatch)


@pytest.mark.parametrize("forced", FORCED + (("asp_v1 T=417", "bf16", None),), ids=lambda f: f"{f[0]}-{f[1]}")
def test_forced_kernel_forms_meet_the_oracle(forced, monkeypatch):
    """each developer option that forces a kernel form: the forced kernels meet the oracle bars themselves"""
    tag, compute, _ = forced
    case = next(c for c in _all_cases() if c[0] == f"forced {tag}" and c[1] == compute)
    labels = _case(case, monkeypatch)
    opts = case[5]["options"]
    if opts.get("pw3_cus") == 0:
        assert "gemm_pw3" not in labels, labels
    if "asp_v1" in opts:
        assert ("asp_pool" if case[3] == 33280 else "asp_fused") in labels and "asp_bf16" not in labels, labels
    if "n128_off" in opts:
        assert "gemm_n128" not in labels, labels
    if "cv_off" in opts:
        assert "gemm_pw3cv16" not in labels, labels
    if "fbank_unfused" in opts:
        assert "fbank_fused" not in labels and "fbank" in labels, labels
    if opts.get("r2_slices") == 3:
        assert "res2net_slices" in labels, labels
    if "r2_big" in opts:
        assert "gemm_pw3r2" in labels and "r2_step" not in labels, labels


# every kernel each compute reached over the cases of this file (profile labels; the GEMMs by kernel).  Not reached by any valid ECAPA
# geometry: gemm_generic (every ECAPA GEMM has whole K tiles and unsegmented rows).  gemm_pw3cv16 takes blocks.0 only with a bank of
# a multiple of 64 mels (_cv16_case); the reference configs' 80 mels go to gemm_conv / gemm_pw2_conv.  f32 handles run the exact-fp32
# kernels only (gemm_pw, gemm_conv / gemm_conv_add, the per-layer Res2Net, se_mean, asp_gstats, asp_pool).
CENSUS_WANT = {
    "bf16": {"asp_bf16", "asp_ctx", "asp_fused", "asp_gstats", "asp_pool", "colsum_finalize", "copy_cols", "emb_out", "fbank", "fbank_fused",
             "fc", "gemm_conv", "gemm_conv_add", "gemm_n128", "gemm_pw", "gemm_pw2", "gemm_pw2_conv", "gemm_pw3", "gemm_pw3cv16", "prologue",
             "res2net_chain", "res2net_slices", "se_apply", "se_mean", "se_mlp"},
    "f32": {"asp_ctx", "asp_gstats", "asp_pool", "copy_cols", "emb_out", "fbank", "fc", "gemm_conv", "gemm_conv_add", "gemm_pw", "prologue",
            "se_apply", "se_mean", "se_mlp"},
    "f32x3": {"asp_ctx", "asp_gstats", "asp_x3", "colsum_finalize", "copy_cols", "emb_out", "fbank", "fc", "gemm_conv", "gemm_conv_add",
              "gemm_pw", "gemm_pw3cv", "gemm_pw3r2", "gemm_pw3x3", "in_scale", "prologue", "r2_step", "se_apply", "se_mean", "se_mlp",
              "split_s32"},
}


@pytest.mark.parametrize("compute", ["f32", "f32x3", "bf16"])
def test_route_census(compute, monkeypatch):
    """every kernel an ECAPA forward of this compute reaches ran in a case checked against the oracle, and nothing else ran"""
    for case in _all_cases():
        if case[1] == compute:
            _case(case, monkeypatch)
    seen = set()
    for tag, labels in sorted(_CENSUS[compute].items()):
        print(f"census {compute} {tag}: {' '.join(labels)}")
        seen |= set(labels)
    print(f"census {compute}: {sorted(seen)}")
    assert seen == CENSUS_WANT[compute], (sorted(seen - CENSUS_WANT[compute]), sorted(CENSUS_WANT[compute] - seen))


@pytest.mark.parametrize("lanes", [1, 2])
def test_headline(lanes, monkeypatch):
    """the bench.py headline: C = 1024, bf16, B = 256, L = 32000 from the waveform — the first and last rows, the utterance over the
    middle tile boundary and, with two lanes, both rows beside the lane split"""
    run_case("bf16", 1024, 32000, 256, lanes=lanes, tag=f"headline lanes={lanes}", monkeypatch=monkeypatch)


@pytest.mark.parametrize("compute,C,B", [("bf16", 1024, 64), ("f32x3", 1024, 2), ("f32", 512, 2)])
def test_reading_the_stages_leaves_the_forward_alone(compute, C, B, monkeypatch):
    """embed, read every stage, embed again: bit-identical embeddings (two lanes on the bf16 handle).  A stage the route does not
    produce is refused with SVHIP_ERR_STATE: blocks.3.tdnn1 of an F32X3 handle whose tdnn1 wrote its first two chunks in the split
    layout only, and the mel power after the fused front-end."""
    if compute == "bf16":
        monkeypatch.setenv("SVHIP_LANES", "2")
    e = Engine(model="ecapa", compute=compute, channels=C, max_batch=B, samples=32000)
    monkeypatch.delenv("SVHIP_LANES", raising=False)
    e.load_state_dict(_sd(C)[0])
    e.finalize()
    x = synth.synth_waveforms(B, 32000, seed=77)
    first = e.embed_wave(x).copy()
    refused = []
    for n in chk.HANDLE_STAGES + ("mel",):
        try:
            assert np.isfinite(e.get_stage(n)).all(), n
        except _lib.SvhipError as err:
            assert err.code == ERR_STATE, (n, err.code)
            refused.append(n)
    assert np.array_equal(e.embed_wave(x), first)
    e.close()
    want = {"bf16": ["mel"], "f32x3": ["blocks.3.tdnn1"], "f32": []}[compute]
    assert refused == want, refused


def test_create_refuses_fewer_than_five_frames():
    """T = L / hop + 1 <= 4: block 3's reflect padding (4 frames) is undefined; refused at create, T = 5 is served"""
    for L in (256, 319):
        with pytest.raises(_lib.SvhipError, match="5 frames") as ei:
            Engine(model="ecapa", compute="bf16", channels=512, max_batch=1, samples=L, n_fft=256)
        assert ei.value.code == -1                   # SVHIP_ERR_INVALID
    with pytest.raises(_lib.SvhipError, match="5 frames"):
        Engine(model="ecapa", compute="f32", channels=512, max_batch=1, samples=1023, n_fft=512, hop_length=400)
    Engine(model="ecapa", compute="bf16", channels=512, max_batch=1, samples=320, n_fft=256).close()
