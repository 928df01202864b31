"""GPU: TitaNet against the float64 oracle (oracle/titanet.py), step by step, on every GEMM route of the forward.

Each case runs one forward with option tn_keep, layer labels and profiling on, reads what the walk stored — tn_prolog; per block skip,
dw0, pw0, dw1, pw1, dw2, pw2, the SE squeeze (where its kernel ran) and gate, out; tn_enc, the attention layer, the fp32 logits, the
pooled vector before and after its BatchNorm — and compares, for the checked utterances, every tensor with the oracle's step applied
in float64 to the handle's own stored input of that step (tests/titanet_oracle_check.py: the checks, the bars — 3 x a clean CPU
emulation, never the GPU's own numbers — and the measured values beside them).  Handles are built with the first three mega-blocks of
the checkpoint (titanet_finalize serves a user-given block count), which cover every form: block 0 tn_dw then tail + dw, block 1 its
first depthwise conv from the tail, block 2 the tail without a depthwise conv.  The cases:

  edge lengths   sizes s / m / l, f32 and bf16, B = 3 (utterances scaled x1, x3, x0.3), all rows, through embed_features, T = 7, 8, 9, 15,
                 16, 17, 31, 33, 255, 256, 257, 401: the tail's 8-frame and tn_dw's 16-frame tiles, radii 1 / 3 / 5, a 256-thread group
                 over several tiles and utterances, the GEMMs' and the column-sum partials' 256-row tiles with an utterance border inside
                 a tile (T = 255, 257, 401), on it (256) and the squeeze kernel below T = 256.
  full depth     per size and compute, the checkpoint's own block count at T = 401 from WAVEFORMS: prolog against the oracle's front-end
                 (the same check and bar as from features.  Its gain form reaches 3.0e-8 on an f32 handle, against 9.5e-9 in the
                 emulated waveform case and 2.2e-8 in the worst emulated feature case: measured beside the oracle's float64 front-end,
                 the handle's mel power is low by 2.4 - 3.2e-8 on every utterance and in nearly every mel bin — half an fp32 step,
                 which the CPU emulation of the same sums does not show (+-5e-9).  A rounding inside the fp32 MFMA chain of the DFT
                 is suspected, not established.)
  a ragged pack  per size and compute, T = 1, 2, 3, 5, 6 (below each radius), 8, 16, 17, 257 in one call: the *_rag kernels and rag_gemm.
  GEMM routes    size l, T = 401; gemm_route (gemm.hip) and the predicates it calls restated here (_route) on the device's CU count; the
                 smallest batches that move each layer to each kernel it can reach, a capped persistent grid (pw3_cus = 16) and the
                 persistent kernels off (pw3_cus = 0).  Rows at B > 3: the first and the last utterance (the last M tile with the
                 last N tile is the persistent kernel's last item, in its tail round), the one before it and the utterance over the
                 middle 256-row tile boundary.

Routes a bf16 TitaNet layer can take (256-row x 256-column tiles, `tiles` of them; cap = the persistent grid's, the CU count or pw3_cus):
  prolog (k = 3 gather, N = H, K = 240)      gemm_conv (the narrow gemm_pw tile) while 2 tiles <= CUs, gemm_pw2_conv above.
                                             gemm_pw3cv16 is UNREACHABLE: gemm_pw3cv16_supported takes GELU / BN + LeakyReLU / no
                                             activation and cin % 64 == 0; the prolog has a ReLU and cin = 80.
  skip, pw 0 / 1, epilog (N % 256 == 0)      gemm_pw3 as column halves while 2 tiles <= cap, gemm_pw2 while tiles <= cap, gemm_pw3
                                             (persistent) above.  The narrow gemm_pw tile is reached only with the persistent kernels
                                             off (pw3_cus = 0) or the tail split off: by default gemm_pw3_supported takes every grid the
                                             narrow tile would.
  pw 2                                       the same kernels with column sums for T >= 256 (never the narrow tile: it writes none);
                                             below T = 256 gemm_pw2_supported refuses the sums and tn_se_mean runs.
  att_in (N = 128, tanh), logits (fp32 out)  gemm_pw always.  gemm_n128 is UNREACHABLE: gemm_n128_supported wants act1 = ReLU with a
                                             BatchNorm affine (ECAPA's asp.tdnn); in_linear has neither.  gemm_pw2_supported refuses
                                             a tanh epilogue, N < 256 and fp32 output.
An f32 handle: gemm_conv (prolog) and gemm_pw (everything else).  gemm_generic is UNREACHABLE on a fixed-length forward:
gemm_pw_supported takes every layer (K a multiple of 32 = Kp, N a multiple of 4, 16-byte aligned buffers); it runs as rag_gemm.

The census asserts the exact set of profile labels each compute reached over the file."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import titanet as ot
from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine
from tests import titanet_oracle_check as chk

pytestmark = pytest.mark.gpu

ERR_STATE = -3                               # include/svhip.h
E, A = ot.ENC, ot.ATT
_REF = {}
_CENSUS = {"f32": {}, "bf16": {}}
_WORST = {"f32": {}, "bf16": {}}
_ROUTES = set()


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _H(size):
    return synth.TITANET_SIZES[size][0]


# ---- gemm_route restated for TitaNet's layers ------------------------------------------------------------------------------------------
def _layers(H, T):
    """(name, N, K, taps, column sums asked for) of the GEMMs of a fixed-length forward, in the order of one block"""
    return [("prolog", H, 240, 3, False), ("skip", H, H, 1, False), ("pw", H, H, 1, False), ("pw_cs", H, H, 1, True), ("epilog", E, H, 1, False),
            ("att_in", A, E, 1, False), ("logits", E, A, 1, False)]


def _route(compute, layer, M, N, T, cu, pw3_cus=-1):
    """(kernel label, form) of one layer: gemm_route (gemm.hip) with gemm_pw_supported, gemm_pw2_supported, gemm_pw3_supported,
    gemm_pw3cv16_supported, gemm_n128_supported and pw3_grid_cap evaluated for TitaNet's operands (module docstring), and conv_plan's
    label (api_gemm.hip).  form: "" | "halves" | "persistent" for gemm_pw3, "sums" where the kernel writes column sums"""
    conv = layer == "prolog"
    if compute == "f32":
        return ("gemm_conv" if conv else "gemm_pw"), ""                         # gemm_pw2_supported: bf16 only; gemm_pw_supported: every layer
    if layer in ("att_in", "logits"):                                           # n128: act1 != ReLU; pw2: tanh / N < 256 / fp32 out
        return "gemm_pw", ""
    sums = layer == "pw_cs" and T >= chk.COLSUM_T                               # (conv_plan drops the sums where pw2 refuses them)
    tiles = -(-M // 256) * -(-N // 256)
    cap = (1 << 30) if pw3_cus == 0 else min(pw3_cus, cu) if pw3_cus > 0 else cu
    pw3 = not conv and (tiles > cap or (2 * tiles <= cap and cap <= cu))        # gemm_pw3_supported (tail_split = 1); taps > 1 refused
    if not sums and 2 * tiles <= cu and not pw3:                                # ROUTE_PW_NARROW (pw3 && tail_split keeps it off)
        return ("gemm_conv" if conv else "gemm_pw"), ""
    if pw3:
        return "gemm_pw3", ("persistent" if tiles > cap else "halves") + (" sums" if sums else "")
    return ("gemm_pw2_conv" if conv else "gemm_pw2"), ("sums" if sums else "")


def _gemm_labels(compute, size, B, T, cu, pw3_cus=-1):
    """{profile label (layer_labels = 1): (layer, form)} a fixed-length forward must show"""
    M, H = B * T, _H(size)
    out = {}
    for layer, N, K, _, _ in _layers(H, T):
        k, form = _route(compute, layer, M, N, T, cu, pw3_cus)
        out.setdefault(f"{k} M{M} N{N} K{K}", []).append((layer, k, form))
    return out


def _smallest_batch(size, T, cu, layer, want):
    """the smallest B that puts `layer` on (kernel, form) `want`"""
    N = {n: v for n, v, _, _, _ in _layers(_H(size), T)}[layer]
    return next(B for B in range(1, 4096) if _route("bf16", layer, B * T, N, T, cu) == want)


# ---- one case --------------------------------------------------------------------------------------------------------------------------
def _oracle(key, mel64, full):
    """the oracle's embedding end to end on the checkpoint's weights, cached"""
    if key not in _REF:
        with torch.no_grad():
            _REF[key] = ot.forward(mel64, full).numpy()
    return _REF[key]


def _stage_names(H, nb):
    out = [("tn_prolog", H, "prolog")]
    for i in range(nb):
        out += [(f"tn_b{i}_{s}", H, f"b{i}_{s}") for s in ot.BLOCK_STEPS]
    return out + [("tn_enc", E, "enc"), ("tn_att", A, "att"), ("tn_logits", E, "logits"), ("tn_pool_raw", 2 * E, "pool_raw"), ("tn_pool", 2 * E, "pool")]


def _read_stages(e, H, nb, row0, rows, with_mean):
    """the kept stages of the last forward for the utterances `rows`: one {oracle stage name: float64 array} per utterance.
    row0: the first packed row of every utterance, and the end"""
    out = {b: {} for b in rows}
    means = [(f"tn_b{i}_mean", H, f"b{i}_mean") for i in range(nb)]
    names = _stage_names(H, nb) + (means if with_mean else [])
    for name, cols, key in names:
        a = e.get_stage(name).reshape(-1, cols)
        per_utt = key in ("pool_raw", "pool") or key.endswith("_gate") or key.endswith("_mean")
        assert a.shape[0] == (len(row0) - 1 if per_utt else row0[-1]), (name, a.shape)
        for b in rows:
            out[b][key] = a[b].astype(np.float64) if per_utt else a[row0[b]:row0[b + 1]].astype(np.float64)
    if not with_mean:                   # the gate came from column-sum partials: no squeeze vector exists, and get_stage says so
        with pytest.raises(_lib.SvhipError, match="never stored it") as ei:
            e.get_stage("tn_b0_mean")
        assert ei.value.code == ERR_STATE
    # the stages that were there before tn_keep hold the same values
    for name, key in (("tn_dw0", "b0_dw0"), ("tn_mega_last", f"b{nb - 1}_out")):
        a = e.get_stage(name).reshape(-1, H)
        for b in rows:
            assert np.array_equal(a[row0[b]:row0[b + 1]], out[b][key]), name
    return out


def _route_rows(B, T):
    """every row for B <= 3; else the first, the last two and the utterance over the middle 256-row tile boundary"""
    if B <= 3:
        return list(range(B))
    return sorted({0, B - 2, B - 1, min(B - 2, max(1, (256 * ((B * T // 2) // 256)) // T))})


def run_case(compute, size, kind, T, B=3, rows=None, options=None, tag=""):
    """one forward with tn_keep, layer labels and profiling on; the kept stages of `rows` (default _route_rows) against the oracle.
    kind: "edge" (features, chk.BLOCKS blocks), "ragged" (the pack of chk.ragged_features), "full" (waveforms, every block).
    Returns the profile labels of the forward."""
    H = _H(size)
    w = chk.weights(size, None if kind == "full" else chk.BLOCKS)
    nb = ot.n_blocks(w["full"])
    L = 32000 if kind == "ragged" else chk.samples_of(T)
    e = Engine(model="titanet", compute=compute, channels=H, embed_dim=chk.NOUT[size], max_batch=B, samples=L, log_input=False)
    e.load_state_dict(w["sd"])
    e.finalize()
    for k, v in dict(options or {}, tn_keep=1, layer_labels=1).items():
        e.set_option(k, v)
    e.profile(True)
    if kind == "ragged":
        x = chk.ragged_features()
        assert e.ragged_check([f.shape[1] for f in x], is_wave=False) is None
        emb = e.embed_features_ragged(x)
        mels = [torch.from_numpy(f).double() for f in x]
    elif kind == "full":
        x = chk.waveforms(B, L)
        emb = e.embed_wave(x)
        mels = [chk.mel_of(v) for v in x]
    else:
        x = chk.features(B, T)
        emb = e.embed_features(x)
        mels = [torch.from_numpy(f).double() for f in x]
    emb = np.asarray(emb).reshape(len(mels), -1).astype(np.float64)
    labels = sorted(e.profile_results())
    e.profile(False)
    assert e.numeric_status() == 0 and np.isfinite(emb).all()
    tps = [m.shape[1] for m in mels]
    row0 = [0] + list(np.cumsum(tps))
    rows = _route_rows(len(tps), tps[0]) if rows is None else rows
    with_mean = not chk.from_partials(compute, kind, tps[0])
    S = _read_stages(e, H, nb, row0, rows, with_mean)
    e.close()
    _CENSUS[compute][tag] = sorted({n.split()[0] for n in labels})
    sd = w[compute][1]
    bad = []
    for b in rows:
        e2e = _oracle((size, kind, T, B, b), mels[b], w["full"])
        err = chk.layer_local(S[b], sd, mel=mels[b], emb=emb[b], e2e_ref=e2e)
        assert set(err) == chk.checks_of(with_mean), set(err) ^ chk.checks_of(with_mean)
        print(f"{tag} {compute} b={b} T={tps[b]}: {chk.describe(err)}")
        for n, (v, _) in err.items():
            _WORST[compute][n] = max(_WORST[compute].get(n, 0.0), v)
        bad += [(b,) + f for f in chk.failures(err, compute)]
    assert not bad, (tag, compute, bad)
    return labels


# ---- edge lengths ----------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_ones_the_bars_were_built_on():
    edge = {("edge", s, T) for s in "sml" for T in chk.EDGE_T}
    assert set(chk.CASES) == edge | {("ragged", s, 0) for s in "sml"} | {("full", s, 401) for s in "sml"}
    assert chk.EDGE_T == (7, 8, 9, 15, 16, 17, 31, 33, 255, 256, 257, 401) and chk.RAGGED_T == (1, 2, 3, 5, 6, 8, 16, 17, 257)
    assert [chk.samples_of(T) // 80 + 1 for T in chk.EDGE_T] == list(chk.EDGE_T) and chk.samples_of(7) == 512


@pytest.mark.parametrize("T", chk.EDGE_T)
@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("size", ["s", "m", "l"])
def test_steps_at_edge_lengths(size, compute, T):
    labels = set(run_case(compute, size, "edge", T, tag=f"{size} T={T}"))
    want = _gemm_labels(compute, size, 3, T, _num_cu())
    assert set(want) <= labels, (sorted(set(want) - labels), sorted(labels))
    heads = {n.split()[0] for n in labels}
    assert ("tn_se_mean" in heads) == (compute == "f32" or T < chk.COLSUM_T), heads
    if compute == "bf16":
        _ROUTES.update(r for v in want.values() for r in v)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("size", ["s", "m", "l"])
def test_steps_at_full_depth_from_waveforms(size, compute):
    labels = set(run_case(compute, size, "full", 401, tag=f"{size} full depth"))
    assert set(_gemm_labels(compute, size, 3, 401, _num_cu())) <= labels, sorted(labels)
    assert "fbank" in labels


# ---- a ragged pack ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("size", ["s", "m", "l"])
def test_steps_of_a_ragged_pack(size, compute):
    n = len(chk.RAGGED_T)
    labels = run_case(compute, size, "ragged", 0, B=n, rows=list(range(n)), tag=f"{size} ragged")
    heads = {x.split()[0] for x in labels}
    assert {"tn_dw_rag", "tn_mega_tail_rag", "rag_gemm", "rag_se_mean", "rag_asp_pool", "rag_fc"} <= heads, heads
    assert not heads & (FIXED - PACKED), heads


# ---- every GEMM route ------------------------------------------------------------------------------------------------------------------
ROUTES_WANT = {
    ("prolog", "gemm_conv", ""), ("prolog", "gemm_pw2_conv", ""),
    ("skip", "gemm_pw3", "halves"), ("skip", "gemm_pw2", ""), ("skip", "gemm_pw3", "persistent"), ("skip", "gemm_pw", ""),
    ("pw", "gemm_pw3", "halves"), ("pw", "gemm_pw2", ""), ("pw", "gemm_pw3", "persistent"), ("pw", "gemm_pw", ""),
    ("pw_cs", "gemm_pw3", "halves"), ("pw_cs", "gemm_pw", ""),                                                # T < 256: no column sums
    ("pw_cs", "gemm_pw3", "halves sums"), ("pw_cs", "gemm_pw2", "sums"), ("pw_cs", "gemm_pw3", "persistent sums"),
    ("epilog", "gemm_pw3", "halves"), ("epilog", "gemm_pw2", ""), ("epilog", "gemm_pw3", "persistent"), ("epilog", "gemm_pw", ""),
    ("att_in", "gemm_pw", ""), ("logits", "gemm_pw", ""),
}


def test_steps_on_every_gemm_route():
    """bf16, size l, T = 401: the smallest batches that move the epilog, then the N = K = H layers and the prolog, to gemm_pw2 and to
    the persistent gemm_pw3; a capped persistent grid; the persistent kernels off.  Every predicted label ran"""
    cu, size, T = _num_cu(), "l", 401
    picks = [(f"{layer} on {k} {form}".strip(), _smallest_batch(size, T, cu, layer, (k, form)), None)
             for layer, k, form in (("epilog", "gemm_pw2", ""), ("pw", "gemm_pw2", ""), ("epilog", "gemm_pw3", "persistent"),
                                    ("pw", "gemm_pw3", "persistent"))]
    picks += [("pw3_cus=16", 8, {"pw3_cus": 16}), ("pw3_cus=0", 3, {"pw3_cus": 0}), ("pw3_cus=0 T=33", 3, {"pw3_cus": 0})]
    print(f"{cu} CUs, route cases: {picks}")
    for name, B, options in picks:
        t = 33 if name.endswith("T=33") else T
        labels = set(run_case("bf16", size, "edge", t, B=B, options=options, tag=f"route {name} B={B}"))
        want = _gemm_labels("bf16", size, B, t, cu, (options or {}).get("pw3_cus", -1))
        assert set(want) <= labels, (name, sorted(set(want) - labels), sorted(labels))
        _ROUTES.update(r for v in want.values() for r in v)


# ---- the census ------------------------------------------------------------------------------------------------------------------------
FIXED = {"fbank", "prologue", "gemm_conv", "gemm_pw", "tn_dw", "tn_se_mean", "tn_se_mlp", "tn_mega_tail", "tn_asp_pool", "tn_in_check", "tn_fc",
         "emb_out"}
PACKED = {"rag_rows", "rag_prologue", "rag_gemm", "tn_dw_rag", "rag_se_mean", "tn_se_mlp", "tn_mega_tail_rag", "rag_asp_pool", "tn_in_check",
          "rag_fc", "emb_out"}
CENSUS_WANT = {"f32": FIXED | PACKED, "bf16": FIXED | PACKED | {"gemm_pw2", "gemm_pw2_conv", "gemm_pw3"}}


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_route_census(compute):
    """every kernel a TitaNet forward of this compute reaches ran in a case checked against the oracle, and nothing else ran; every
    route of ROUTES_WANT was predicted and observed; the worst GPU value of every check over the file (the third column of the bars'
    tables)"""
    have = _CENSUS[compute]
    for T in (33, 401):
        if f"l T={T}" not in have:
            test_steps_at_edge_lengths("l", compute, T)
    if "l full depth" not in have:
        test_steps_at_full_depth_from_waveforms("l", compute)
    if "l ragged" not in have:
        test_steps_of_a_ragged_pack("l", compute)
    if compute == "bf16" and not any(t.startswith("route") for t in have):
        test_steps_on_every_gemm_route()
    seen = set()
    for tag, heads in sorted(have.items()):
        print(f"census {compute} {tag}: {' '.join(heads)}")
        seen |= set(heads)
    print(f"census {compute}: {sorted(seen)}")
    for n in chk.CHECKS:
        print(f"worst {compute} {n}: {_WORST[compute][n]:.1e} (bar {chk.bars(compute)[n]:.1e})")
    assert not seen & {"gemm_pw3cv16", "gemm_n128", "gemm_generic"}, seen
    assert seen == CENSUS_WANT[compute], (sorted(seen - CENSUS_WANT[compute]), sorted(CENSUS_WANT[compute] - seen))
    if compute == "bf16":
        print(f"routes: {sorted(_ROUTES)}")
        assert _ROUTES == ROUTES_WANT, (sorted(_ROUTES - ROUTES_WANT), sorted(ROUTES_WANT - _ROUTES))


# ---- tn_keep leaves the forward alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_tn_keep_leaves_the_forward_alone(compute, ragged):
    """embed; embed with tn_keep on and read every stage; embed with it off: bit-identical embeddings, the same profile labels and
    launch counts.  Without the option a kept stage is refused with SVHIP_ERR_STATE; the five older stages are served either way, and
    tn_dw0 / tn_mega_last are bit-equal to their kept counterparts"""
    size, T = "m", 257
    H, nb = _H(size), chk.BLOCKS
    e = Engine(model="titanet", compute=compute, channels=H, embed_dim=chk.NOUT[size], max_batch=len(chk.RAGGED_T), samples=chk.samples_of(T),
               log_input=False)
    e.load_state_dict(chk.weights(size, nb)["sd"])
    e.finalize()
    x = chk.ragged_features() if ragged else chk.features(len(chk.RAGGED_T), T)
    embed = e.embed_features_ragged if ragged else e.embed_features
    old = ("tn_prolog", "tn_dw0", "tn_mega_last", "tn_enc", "tn_pool")
    with_mean = not chk.from_partials(compute, "ragged" if ragged else "edge", T)
    names = [n for n, _, _ in _stage_names(H, nb)] + ([f"tn_b{i}_mean" for i in range(nb)] if with_mean else [])
    runs = []
    for keep in (0, 1, 0):
        e.set_option("tn_keep", keep)
        e.profile(True)
        emb = np.asarray(embed(x)).copy()
        prof = {n: r["launches"] for n, r in e.profile_results().items()}
        e.profile(False)
        runs.append((emb, prof))
        for name in names:
            if keep or name in old:
                assert np.isfinite(e.get_stage(name)).all(), name
            else:
                with pytest.raises(_lib.SvhipError, match="option tn_keep was not set") as ei:
                    e.get_stage(name)
                assert ei.value.code == ERR_STATE, name
        if keep:
            assert np.array_equal(e.get_stage("tn_dw0"), e.get_stage("tn_b0_dw0"))
            assert np.array_equal(e.get_stage("tn_mega_last"), e.get_stage(f"tn_b{nb - 1}_out"))
    e.close()
    for emb, prof in runs[1:]:
        assert np.array_equal(emb, runs[0][0]) and prof == runs[0][1]
    print(f"{compute} {'ragged' if ragged else 'fixed'}: sha1 {hashlib.sha1(runs[0][0].tobytes()).hexdigest()}")
