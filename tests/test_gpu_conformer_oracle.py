"""GPU: the Conformer against the float64 oracle (oracle/conformer.py), step by step, on every GEMM route of the forward.

Each case runs one forward with option cf_keep, layer labels and profiling on, reads what the walk stored — per block ff1, qkv, ctx,
att, pw1, dw, conv, ff2, out; cf_in, the pooling logits, the pooled vector before and after attention_norm — and compares, for the
checked utterances, every tensor with the oracle's step applied in float64 to the handle's own stored input of that step
(tests/conformer_oracle_check.py: the checks, the bars — 3 x a clean CPU emulation, never the GPU's own numbers — and the measured
values beside them).  The cases:

  edge lengths   f32 and bf16, B = 3 (utterances scaled x1, x3, x0.3), all rows, T' = 1, 2, 7, 8, 15, 16, 17, 33, 63, 64, 65, 99, 129,
                 499 (cf_glu_dw's 16-frame tiles and 7-frame halo, cf_attn's 64-query / 64-key tiles, cf_ln's four rows per workgroup:
                 3 T' is odd for most), T = 4 T' + 3; at T' = 16 and 64 also T = 4 T' + 6 (T1 even, trailing frames dropped).  T' = 7
                 goes through embed_features.
  GEMM routes    bf16, the smallest batches that put qkv, then pw1 (T' = 99), then the N = 256 residual layers ff2 / out / pw2
                 (T' = 499) on gemm_pw2, from the routing rule restated here on the device's CU count; several subsampling slices.
                 f32: B = cf_chunk + 1, a partial last slice.  Rows: the first, the last, the utterance over the middle 256-row tile
                 boundary, the first of the second slice (and so the only one of a one-utterance last slice).
  a ragged pack  per compute, T' = 1, 17, 64, 65, 99 in one call: the *_rag kernels and the generic GEMM, every utterance.
  the benchmark  bf16, B = 256, L = 32000.

input_projection never reaches gemm_pw2: its rows are those of ONE subsampling slice, which the 256 MiB conv1 buffer holds to
about 6 700 (cf_chunk T'), 27 row tiles; the narrow gemm_pw tile takes it while 2 x tiles <= CUs, that is on every device with 54
CUs or more.  The route test asserts what the rule predicts, for proj too.

The census asserts the exact set of profile labels each compute reached over the file.  gemm_pw3 and gemm_n128 are NOT in it: the
Conformer's layers are built without a BatchNorm affine (make_conv with an empty BN name: scale is null), which gemm_pw3_supported
refuses, ff2's scale comes with a residual, which it refuses too, and gemm_n128 wants the tanh epilogue of ECAPA's attention.  An
observation for a later performance issue, not changed here."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import conformer as oc
from speakerverification_amd import _lib
from speakerverification_amd.engine import Engine
from tests import conformer_oracle_check as chk

pytestmark = pytest.mark.gpu

ERR_STATE = -3                               # include/svhip.h
D, F1, F2 = 256, 39, 19                      # d_model; the mel axis after each 3 x 3 stride-2 convolution (80 mels)
_W = {}
_REF = {}
_CENSUS = {"f32": {}, "bf16": {}}
_WORST = {"f32": {}, "bf16": {}}


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sub(n):
    return (n - 3) // 2 + 1


def _chunk(compute, T, max_batch):
    """cf_chunk (api_conformer.hip): utterances per subsampling slice, what keeps a slice's conv1 output within 256 MiB"""
    per_utt = _sub(T) * F1 * D * (2 if compute == "bf16" else 4)
    return max(1, min(max_batch, (256 << 20) // per_utt))


def _on_pw2(M, N, num_cu):
    """gemm_route (gemm.hip) of a bf16 pointwise GEMM that gemm_pw2 supports and gemm_pw3 refuses: the narrow gemm_pw tile while
    2 x tiles <= CUs, else gemm_pw2"""
    return 2 * (-(-M // 256) * -(-N // 256)) > num_cu


def _smallest_batch(Tp, N, num_cu):
    return next(B for B in range(1, 4096) if _on_pw2(B * Tp, N, num_cu))


def _gemm_labels(compute, B, Tp, T, num_cu):
    """the GEMM profile labels (layer_labels = 1) a fixed-length forward must show"""
    M = B * Tp
    k = lambda N: "gemm_pw2" if compute == "bf16" and _on_pw2(M, N, num_cu) else "gemm_pw"
    want = {f"gemm_pw M{M} N1024 K256", f"{k(768)} M{M} N768 K256", f"{k(512)} M{M} N512 K256", f"{k(256)} M{M} N256 K1024",
            f"{k(256)} M{M} N256 K256", f"gemm_pw M{M} N128 K256", f"gemm_pw M{M} N256 K128"}
    chunk = _chunk(compute, T, B)
    for n in {min(chunk, B - s0) for s0 in range(0, B, chunk)}:
        kp = "gemm_pw2" if compute == "bf16" and _on_pw2(n * Tp, 256, num_cu) else "gemm_pw"
        want |= {f"gemm_generic M{n * Tp * F2} N256 K2304", f"{kp} M{n * Tp} N256 K{D * F2}"}
    return want


def _weights():
    if not _W:
        sd, sd64 = chk.weights()
        _W.update(sd=sd, f32=sd64, bf16=oc.rounded_sd(sd64))
    return _W


def _oracle(x_row, wave):
    """(the oracle's mel power of one utterance, its embedding end to end on the full weights), cached by input hash"""
    key = hashlib.sha1(x_row.tobytes() + bytes([wave])).hexdigest()
    if key not in _REF:
        with torch.no_grad():
            mel = chk.mel_of(x_row) if wave else torch.from_numpy(x_row).double()
            _REF[key] = (mel, oc.forward(mel, _weights()["f32"]).numpy())
    return _REF[key]


STAGES = [("cf_in", D)] + [(f"cf_b{i}_{s}", {"qkv": 3 * D, "pw1": 2 * D}.get(s, D)) for i in range(oc.LAYERS) for s in oc.BLOCK_STEPS] + \
         [("cf_logits", D), ("cf_pool_raw", 2 * D), ("cf_pool", 2 * D)]


def _read_stages(e, row0, rows):
    """the kept stages of the last forward for the utterances `rows`: one {oracle stage name: float64 array} per utterance.
    row0: the first packed row of every utterance, and the end"""
    out = {b: {} for b in rows}
    for name, cols in STAGES:
        a = e.get_stage(name).reshape(-1, cols)
        key = name[3:] if name.startswith("cf_b") else {"cf_in": "cf_in", "cf_logits": "logits", "cf_pool_raw": "pool_raw", "cf_pool": "pool"}[name]
        per_utt = name in ("cf_pool_raw", "cf_pool")
        assert a.shape[0] == (len(row0) - 1 if per_utt else row0[-1]), (name, a.shape)
        for b in rows:
            out[b][key] = a[b].astype(np.float64) if per_utt else a[row0[b]:row0[b + 1]].astype(np.float64)
    # the stages that were there before cf_keep hold the same values
    for name, key in (("cf_attn0", "b0_ctx"), ("cf_block0", "b0_out"), ("cf_last", f"b{oc.LAYERS - 1}_out")):
        a = e.get_stage(name).reshape(-1, D)
        for b in rows:
            assert np.array_equal(a[row0[b]:row0[b + 1]], out[b][key]), name
    return out


def _check_rows(tag, compute, S, emb, inputs, wave):
    """layer_local on every read utterance; every error printed, the bars asserted after the whole case"""
    sd = _weights()[compute]
    bad = []
    for b in sorted(S):
        mel, e2e = _oracle(inputs[b], wave)
        with torch.no_grad():
            feat = oc.features(mel, sd)
        err = chk.layer_local(S[b], sd, ref_input=feat, emb=emb[b], e2e_ref=e2e)
        assert set(err) == set(chk.CHECKS)
        print(f"{tag} {compute} b={b} T'={S[b]['cf_in'].shape[0]}: {chk.describe(err)}")
        for n, (v, _) in err.items():
            _WORST[compute][n] = max(_WORST[compute].get(n, 0.0), v)
        bad += [(b,) + f for f in chk.failures(err, compute)]
    assert not bad, (tag, compute, bad)


def _engine(compute, B, L, options=None):
    e = Engine(model="conformer", compute=compute, channels=256, embed_dim=512, max_batch=B, samples=L, log_input=True, input_norm=True)
    e.load_state_dict(_weights()["sd"])
    e.finalize()
    for k, v in dict(options or {}, cf_keep=1, layer_labels=1).items():
        e.set_option(k, v)
    return e


def _route_rows(B, Tp, chunk):
    """every row for B <= 3; else the first, the last, the utterance over the middle 256-row tile boundary and the first utterance of
    the second subsampling slice (the only one of the last slice where B = k chunk + 1)"""
    if B <= 3:
        return list(range(B))
    rows = {0, B - 1, min(B - 2, max(1, (256 * ((B * Tp // 2) // 256)) // Tp))}
    if chunk < B:
        rows.add(chunk)
    return sorted(rows)


def run_case(compute, L, B, rows=None, options=None, ragged=None, wave=True, tag=""):
    """one forward with cf_keep, layer labels and profiling on; the kept stages of `rows` (default _route_rows) against the oracle.
    ragged: the sample counts of a pack (L: the handle's samples).  Returns the profile labels of the forward."""
    e = _engine(compute, B, L, options)
    e.profile(True)
    if ragged:
        x = [chk.waveforms(len(ragged), n)[u] for u, n in enumerate(ragged)]
        assert e.ragged_check([len(w) for w in x]) is None
        emb = e.embed_wave_ragged(x)
        tps = [oc.frames(len(w) // 80 + 1) for w in x]
    elif wave:
        x = chk.waveforms(B, L)
        emb = e.embed_wave(x)
        tps = [oc.frames(L // 80 + 1)] * B
    else:
        x = np.stack([chk.mel_of(w, torch.float32).numpy() for w in chk.waveforms(B, L)])
        emb = e.embed_features(x)
        tps = [oc.frames(x.shape[2])] * B
    emb = emb.reshape(len(tps), -1).astype(np.float64)
    labels = sorted(e.profile_results())
    e.profile(False)
    assert e.numeric_status() == 0 and np.isfinite(emb).all()
    row0 = [0] + list(np.cumsum(tps))
    chunk = _chunk(compute, L // 80 + 1, B)
    S = _read_stages(e, row0, _route_rows(len(tps), tps[0], chunk) if rows is None else rows)
    e.close()
    _CENSUS[compute][tag] = sorted({n.split()[0] for n in labels})
    _check_rows(tag, compute, S, emb, x, wave)
    return labels


# ---- edge lengths ------------------------------------------------------------------------------------------------------------------------
def _edge_cases():
    out = []
    for compute in ("f32", "bf16"):
        out += [(f"T'={t}", compute, chk.samples_of(t), t != 7) for t in chk.EDGE_TP]
        out += [(f"T'={t} T1 even", compute, chk.samples_of(t, 3), True) for t in (16, 64)]
    return out


def test_the_edge_cases_are_the_lengths_the_bars_were_built_on():
    assert sorted({c[2] for c in _edge_cases()}) == sorted(chk.LENGTHS)
    assert [oc.frames(L // 80 + 1) for L in chk.LENGTHS] == list(chk.EDGE_TP) + [16, 64]
    assert [_sub(L // 80 + 1) % 2 for L in chk.LENGTHS[-2:]] == [0, 0]


@pytest.mark.parametrize("case", _edge_cases(), ids=lambda c: f"{c[0]}-{c[1]}")
def test_steps_at_edge_lengths(case):
    tag, compute, L, wave = case
    labels = run_case(compute, L, 3, wave=wave, tag=tag)
    T = L // 80 + 1
    assert _gemm_labels(compute, 3, oc.frames(T), T, _num_cu()) <= set(labels), labels


# ---- every GEMM route --------------------------------------------------------------------------------------------------------------------
def test_steps_on_every_gemm_route():
    """bf16: qkv (N = 768), pw1 (N = 512) and the N = 256 residual layers each on gemm_pw2 at the smallest batch that puts them there,
    the layers below their thresholds on the narrow gemm_pw tile in the same forwards; every predicted label ran"""
    cu = _num_cu()
    picks = {"qkv": (99, _smallest_batch(99, 768, cu)), "pw1": (99, _smallest_batch(99, 512, cu)), "n256": (499, _smallest_batch(499, 256, cu))}
    print(f"{cu} CUs, route batches: {picks}")
    seen = set()
    for name, (Tp, B) in picks.items():
        L = chk.samples_of(Tp)
        T = L // 80 + 1
        labels = set(run_case("bf16", L, B, tag=f"route {name} B={B}"))
        want = _gemm_labels("bf16", B, Tp, T, cu)
        assert want <= labels, (name, sorted(want - labels), sorted(labels))
        assert B > _chunk("bf16", T, B), "the case was meant to take several subsampling slices"
        seen |= {(n.split()[0], n.split()[2], n.split()[3]) for n in want}
    for N, K in (("N768", "K256"), ("N512", "K256"), ("N256", "K1024"), ("N256", "K256")):
        assert ("gemm_pw2", N, K) in seen, (N, K, sorted(seen))
        # (below their thresholds in the smaller of these batches; qkv, the first to leave, is on the narrow tile in every edge case)
        assert ("gemm_pw", N, K) in seen or N == "N768", (N, K, sorted(seen))
    # input_projection: one slice's rows only (module docstring)
    assert ("gemm_pw", "N256", f"K{D * F2}") in seen
    assert ("gemm_pw2", "N256", f"K{D * F2}") in seen or cu >= 54


def test_steps_with_a_partial_last_slice_in_f32():
    L, T = 32000, 401
    chunk = _chunk("f32", T, 4096)
    labels = run_case("f32", L, chunk + 1, tag=f"f32 B={chunk + 1}")
    launches = [n for n in labels if n.startswith("gemm_generic")]
    assert sorted(launches) == sorted({f"gemm_generic M{chunk * 99 * F2} N256 K2304", f"gemm_generic M{99 * F2} N256 K2304"}), launches


def test_steps_at_the_benchmark_shape():
    labels = set(run_case("bf16", 32000, 256, tag="benchmark"))
    want = _gemm_labels("bf16", 256, 99, 401, _num_cu())
    assert want <= labels, (sorted(want - labels), sorted(labels))


# ---- a ragged pack -------------------------------------------------------------------------------------------------------------------------
RAGGED_TP = (1, 17, 64, 65, 99)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_steps_of_a_ragged_pack(compute):
    labels = run_case(compute, 32000, len(RAGGED_TP), rows=list(range(len(RAGGED_TP))), ragged=[chk.samples_of(t) for t in RAGGED_TP], tag="ragged")
    heads = {n.split()[0] for n in labels}
    assert {"cf_conv1_rag", "cf_attn_rag", "cf_glu_dw_rag", "rag_asp_pool", "rag_gemm", "rag_fc"} <= heads, heads
    assert not heads & {"cf_conv1", "cf_attn", "cf_glu_dw", "cf_asp_pool", "gemm_pw", "gemm_pw2", "gemm_generic"}, heads


# ---- the census ----------------------------------------------------------------------------------------------------------------------------
FIXED = {"fbank", "prologue", "cf_conv1", "gemm_generic", "gemm_pw", "cf_ln", "cf_attn", "cf_glu_dw", "cf_asp_pool", "cf_in_check", "cf_fc", "emb_out"}
PACKED = {"fbank", "rag_rows", "rag_prologue", "cf_conv1_rag", "rag_gemm", "cf_ln", "cf_attn_rag", "cf_glu_dw_rag", "rag_asp_pool", "cf_in_check",
          "rag_fc", "emb_out"}
CENSUS_WANT = {"f32": FIXED | PACKED, "bf16": FIXED | PACKED | {"gemm_pw2"}}


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_route_census(compute):
    """every kernel a Conformer forward of this compute reaches ran in a case checked against the oracle, and nothing else ran; the
    worst GPU value of every check over the file (the third column of the bars' tables)"""
    if not any(t.startswith("T'=499") for t in _CENSUS[compute]):
        run_case(compute, chk.samples_of(499), 3, tag="T'=499")
    if "ragged" not in _CENSUS[compute]:
        test_steps_of_a_ragged_pack(compute)
    if compute == "bf16" and not any(t.startswith("route") for t in _CENSUS[compute]):
        test_steps_on_every_gemm_route()
    seen = set()
    for tag, heads in sorted(_CENSUS[compute].items()):
        print(f"census {compute} {tag}: {' '.join(heads)}")
        seen |= set(heads)
    print(f"census {compute}: {sorted(seen)}")
    for n in chk.CHECKS:
        print(f"worst {compute} {n}: {_WORST[compute][n]:.1e} (bar {chk.bars(compute)[n]:.1e})")
    assert not seen & {"gemm_pw3", "gemm_n128"}, seen
    assert seen == CENSUS_WANT[compute], (sorted(seen - CENSUS_WANT[compute]), sorted(CENSUS_WANT[compute] - seen))


# ---- cf_keep leaves the forward alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_cf_keep_leaves_the_forward_alone(compute, ragged):
    """embed; embed with cf_keep on and read every stage; embed with it off: bit-identical embeddings, the same profile labels and
    launch counts.  Without the option a kept stage is refused with SVHIP_ERR_STATE, the five older stages are served"""
    e = Engine(model="conformer", compute=compute, channels=256, embed_dim=512, max_batch=5, samples=32000, log_input=True, input_norm=True)
    e.load_state_dict(_weights()["sd"])
    e.finalize()
    x = [chk.waveforms(5, chk.samples_of(t))[u] for u, t in enumerate(RAGGED_TP)] if ragged else chk.waveforms(5, 32000)
    embed = e.embed_wave_ragged if ragged else e.embed_wave
    runs = []
    for keep in (0, 1, 0):
        e.set_option("cf_keep", keep)
        e.profile(True)
        emb = embed(x).copy()
        prof = {n: r["launches"] for n, r in e.profile_results().items()}
        e.profile(False)
        runs.append((emb, prof))
        for name, _ in STAGES:
            if keep or name in ("cf_in", "cf_pool"):
                assert np.isfinite(e.get_stage(name)).all(), name
            else:
                with pytest.raises(_lib.SvhipError, match="option cf_keep was not set") as ei:
                    e.get_stage(name)
                assert ei.value.code == ERR_STATE, name
    e.close()
    for emb, prof in runs[1:]:
        assert np.array_equal(emb, runs[0][0]) and prof == runs[0][1]
    print(f"{compute} {'ragged' if ragged else 'fixed'}: sha1 {hashlib.sha1(runs[0][0].tobytes()).hexdigest()}")
