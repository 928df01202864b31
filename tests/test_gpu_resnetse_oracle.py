"""GPU: ResNetSE34V2 against the float64 oracle (oracle/resnetse.py), step by step, on fixed-length and ragged forwards.

Each case runs one forward with option rs_keep, layer labels and profiling on, reads what the walk stored — rs_xin, rs_stem; per block
conv1, conv2, the SE tile sums and gate, the downsample (first block of stages 2 - 4) and out; the attention layer, the fp32 logits, the
pooled vector — and compares, for the checked utterances, every tensor with the oracle's step applied in float64 to the handle's own
stored input of that step (tests/resnetse_oracle_check.py: the checks, the bars — 3 x a clean CPU emulation, never the GPU's own
numbers — and the measured values beside them).  n_mels = 80, 'ASP', f32 and bf16 unless said otherwise.  The cases:

  edge lengths   B = 3 (utterances scaled x1, x3, x0.3), all rows, through embed_features, T = 2, 3, 5, 8, 9, 16, 17, 33, 65, 129 (a handle takes
                 at least one FFT window of 512 samples: below seven frames its hop is 512 / (T - 1), which the network never sees).
                 test_the_edge_lengths_reach_every_tile_condition asserts from oracle.resnetse.tile_of (rs_tile_of restated) what they
                 cover: 1 x 10 deepest images with three idle waves (T <= 8), odd and even P into every stride-2 convolution and
                 downsample, one and several tiles along P, partial last tiles along P and along Q, the 121-position (11 x 11) and
                 126-position (6 x 21) tiles, whose rows m >= mt recompute position 0.
  configurations n_mels = 64 at T = 33 (Q = 64 / 32 / 16 / 8), 'SAP' at T = 33, features without the log at T = 17.
  full size      B = 3 WAVEFORMS of 32000 samples (T = 401 at the front-end's hop of 80), the last utterance checked, `fbank` among the
                 labels, xin against the oracle's own front-end.
  ragged packs   T = 2, 3, 5, 8, 9, 17, 33, 65 in one embed_features_ragged call on a max_batch = 8, T = 65 handle (sum 8 ceil(T_u / 8)
                 = 184 <= 520; ragged_check admits it), every utterance checked: the *_rag kernels, rs_rag_tiles, rag_gemm, rag_asp_pool,
                 rag_fc and none of the fixed-only labels; and a pack of one utterance (T = 33).
  GEMM routes    the two attention convolutions, gemm_route (gemm.hip) restated in _route: att0 (N = 128, K = F, ReLU + BN affine) and
                 att3 (N = F, K = 128, fp32 out) run gemm_pw at every M, on both computes; the predicted `gemm_pw M<m> N<n> K<k>`
                 labels are asserted in every fixed-length case.  No batch moves either layer: none of the predicates below reads M.
                 UNREACHABLE for both layers: gemm_n128 (gemm_n128_supported wants act2 = tanh: att0 has act1 = ReLU, a BN affine and
                 no second activation; att3 has N = F and fp32 output), gemm_pw2 / gemm_pw3 (gemm_pw2_supported refuses N < 256 for att0
                 and out_f32 for att3, and is bf16 only), gemm_pw3cv16 (taps = 1), gemm_generic on a fixed-length forward
                 (gemm_pw_supported takes both layers: K = 2560 / 2048 / 128 are multiples of 32, N a multiple of 4); a pack runs the
                 generic kernel as rag_gemm.

The census asserts the exact set of profile labels each compute reached over the file and prints the worst GPU value of every check
beside its bar."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import resnetse as orr
from speakerverification_amd import _lib
from speakerverification_amd.engine import Engine
from tests import resnetse_oracle_check as chk

pytestmark = pytest.mark.gpu

ERR_STATE = -3                               # include/svhip.h
A = orr.ATT
WIDTHS = (32, 64, 128, 256)
STAGE_OF = tuple(s for s, n in enumerate((3, 4, 6, 3)) for _ in range(n))
DOWN_BLOCKS = (3, 7, 13)
_REF = {}
_CENSUS = {"f32": {}, "bf16": {}}
_WORST = {"f32": {}, "bf16": {}}


def _levels(T, n_mels):
    """[(P, Q)] of the four frame levels of an utterance of T frames"""
    out = [(T, n_mels)]
    for _ in range(3):
        out.append((orr.out_size(out[-1][0], 2), orr.out_size(out[-1][1], 2)))
    return out


def _route(compute, N, out_f32, act2_tanh=False):
    """the kernel of a pointwise (taps = 1) convolution on a fixed-length forward: gemm_route (gemm.hip) with gemm_n128_supported,
    gemm_pw2_supported and gemm_pw_supported evaluated for the attention convolutions' operands (module docstring) — none reads M"""
    bf = compute == "bf16"
    if bf and N == 128 and not out_f32 and act2_tanh:             # gemm_n128_supported: ReLU -> BN affine -> tanh
        return "gemm_n128"
    if bf and not out_f32 and N >= 256:                           # gemm_pw2_supported (then gemm_pw3 / gemm_pw2 / the narrow tile by M)
        return "gemm_pw2"
    return "gemm_pw"                                              # gemm_pw_supported: K a multiple of 32, N of 4


def _gemm_labels(compute, B, T, n_mels):
    """the two attention convolutions' profile labels (layer_labels = 1): att0 N = 128, K = F, ReLU + BN affine; att3 N = F, K = 128, fp32"""
    P4, Q4 = _levels(T, n_mels)[3]
    M, F_ = B * P4, 256 * Q4
    return {f"{_route(compute, A, False)} M{M} N{A} K{F_}", f"{_route(compute, F_, True)} M{M} N{F_} K{A}"}


def _oracle(key, mel64, full, log_input):
    """the oracle's embedding end to end on the checkpoint's weights, cached"""
    if key not in _REF:
        with torch.no_grad():
            _REF[key] = orr.forward(mel64, full, log_input).numpy()
    return _REF[key]


def _stage_list():
    """[(stage name, oracle key, kind, level or -1, columns or None)]: kind "img" | "part" | "utt" | "att" | "logits" | "xin" | "pool\""""
    out = [("rs_xin", "xin", "xin", 0), ("rs_stem", "stem", "img", 0)]
    for i, s in enumerate(STAGE_OF):
        for step in orr.BLOCK_STEPS:
            if step == "down" and i not in DOWN_BLOCKS:
                continue
            out.append((f"rs_b{i}_{step}", f"b{i}_{step}", {"part": "part", "gate": "utt"}.get(step, "img"), s))
    return out + [("rs_att", "att", "att", 3), ("rs_logits", "logits", "logits", 3), ("rs_pool_raw", "pool_raw", "pool", 3), ("rs_pool", "pool", "pool", 3)]


def _read_stages(e, Ts, n_mels, rows):
    """the kept stages of the last forward for the utterances `rows`: one {oracle stage name: float64 array in the oracle's layout} per
    utterance"""
    lv = [_levels(T, n_mels) for T in Ts]
    n = len(Ts)
    out = {b: {} for b in rows}
    for name, key, kind, l in _stage_list():
        C = 32 if key == "stem" else WIDTHS[l]
        a = e.get_stage(name)
        if kind in ("utt", "pool"):
            a = a.reshape(n, -1)
            for b in rows:
                v = a[b].astype(np.float64)
                out[b][key] = orr.ref_cols(v.reshape(2, -1), 256).reshape(-1) if kind == "pool" else v
            continue
        if kind == "part":
            cnt = [(lambda g: g[2] * g[3])(orr.tile_grid(*lv[u][l])) for u in range(n)]
        elif kind in ("att", "logits", "xin"):
            cnt = [lv[u][l][0] for u in range(n)]
        else:
            cnt = [lv[u][l][0] * lv[u][l][1] for u in range(n)]
        r0 = [0] + list(np.cumsum(cnt))
        cols = {"att": A, "logits": 256 * lv[0][3][1], "xin": n_mels}.get(kind, C)
        assert a.size == r0[-1] * cols, (name, a.size, r0[-1], cols)
        a = a.reshape(r0[-1], cols)
        for b in rows:
            v = a[r0[b]:r0[b + 1]].astype(np.float64)
            if kind == "img":
                v = v.reshape(lv[b][l][0], lv[b][l][1], cols)
            elif kind == "logits":
                v = orr.ref_cols(v, 256)
            out[b][key] = v
    # the stages that were there before rs_keep hold the same values: a stage's output is its last block's out, bit for bit
    for s, last in enumerate((2, 6, 12, 15)):
        assert np.array_equal(e.get_stage(f"rs_layer{s + 1}"), e.get_stage(f"rs_b{last}_out")), s
    return out


def run_case(compute, case, B=3, rows=None, tag="", engine=None):
    """one forward with rs_keep, layer labels and profiling on; the kept stages of `rows` (default: all) against the oracle.  case: one of
    chk.CASES.  Returns the profile labels of the forward."""
    kind, n_mels, enc, log_input, T = case
    w = chk.weights(n_mels, enc)
    ragged = kind.startswith("ragged")
    e = engine
    if e is None:
        e = Engine(model="resnetse", compute=compute, channels=1 if enc == "SAP" else 2, n_mels=n_mels, embed_dim=chk.NOUT, max_batch=8 if ragged else B,
                   log_input=log_input, input_norm=True, **chk.engine_kw(65 if ragged else T))
        e.load_state_dict(w["sd"])
        e.finalize()
    for k, v in dict(rs_keep=1, layer_labels=1).items():
        e.set_option(k, v)
    e.profile(True)
    if ragged:
        x = chk.case_features(case)
        assert e.ragged_check([f.shape[1] for f in x], is_wave=False) is None
        assert sum(8 * -(-f.shape[1] // 8) for f in x) <= 8 * 65
        emb = e.embed_features_ragged(x)
        mels = [torch.tensor(f, dtype=torch.float64) for f in x]
    elif kind == "full":
        x = chk.waveforms(B, chk.engine_samples(T))
        emb = e.embed_wave(x)
        mels = [chk.mel_of(v) if b in (rows or range(B)) else None for b, v in enumerate(x)]
    else:
        x = chk.features(B, T, n_mels)
        emb = e.embed_features(x)
        mels = [torch.tensor(f, dtype=torch.float64) for f in x]
    emb = np.asarray(emb).reshape(len(mels), -1).astype(np.float64)
    labels = sorted(e.profile_results())
    e.profile(False)
    assert e.numeric_status() == 0 and np.isfinite(emb).all()
    Ts = [T] * B if kind == "full" else [m.shape[1] for m in mels]
    rows = list(range(len(Ts))) if rows is None else list(rows)
    S = _read_stages(e, Ts, n_mels, rows)
    if engine is None:
        e.close()
    _CENSUS[compute][tag] = sorted({n.split()[0] for n in labels})
    sd = w[compute][1]
    bad = []
    for b in rows:
        e2e = _oracle((case, B, b), mels[b], w["full"], log_input)
        err = chk.layer_local(S[b], sd, log_input, mel=mels[b], emb=emb[b], e2e_ref=e2e)
        assert set(err) == set(chk.CHECKS), set(err) ^ set(chk.CHECKS)
        print(f"{tag} {compute} b={b} T={Ts[b]}: {chk.describe(err)}")
        for n, (v, _) in err.items():
            _WORST[compute][n] = max(_WORST[compute].get(n, 0.0), v)
        bad += [(b,) + f for f in chk.failures(err, compute)]
    assert not bad, (tag, compute, bad)
    return labels


# ---- edge lengths ----------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_ones_the_bars_were_built_on():
    edge = {("edge", 80, "ASP", True, T) for T in chk.EDGE_T}
    other = {("edge", 64, "ASP", True, 33), ("edge", 80, "SAP", True, 33), ("edge", 80, "ASP", False, 17), ("full", 80, "ASP", True, 401),
             ("ragged", 80, "ASP", True, 0), ("ragged1", 80, "ASP", True, 0)}
    assert set(chk.CASES) == edge | other
    assert chk.EDGE_T == (2, 3, 5, 8, 9, 16, 17, 33, 65, 129) and chk.RAGGED_T == (2, 3, 5, 8, 9, 17, 33, 65) and chk.RAGGED_ONE_T == (33,)
    assert [chk.engine_kw(T)["samples"] // chk.engine_kw(T)["hop_length"] + 1 for T in chk.EDGE_T] == list(chk.EDGE_T)
    assert chk.engine_kw(401) == dict(samples=32000, hop_length=80) and all(chk.engine_kw(T)["samples"] >= 512 for T in chk.EDGE_T)


def test_the_edge_lengths_reach_every_tile_condition():
    """what the edge lengths are there for, from rs_tile_of restated (oracle.resnetse.tile_of): a later change of the plan that empties a
    condition fails here"""
    plans = {}                                # (T, level) -> (P, Q, TP, TQ, ntp, ntq) of the 3 x 3 stride-1 convolutions (conv2: the SE tiles)
    for T in chk.EDGE_T:
        for l, (P, Q) in enumerate(_levels(T, 80)):
            plans[T, l] = (P, Q) + orr.tile_grid(P, Q)
    deep = {T: plans[T, 3] for T in chk.EDGE_T}
    assert all(deep[T][:2] == (1, 10) and deep[T][2] * deep[T][3] <= 32 for T in chk.EDGE_T if T <= 8), deep          # three of four waves idle
    for l in range(3):                        # the inputs of the stride-2 convolution and downsample into level l + 1
        assert {plans[T, l][0] % 2 for T in chk.EDGE_T} == {0, 1}, l
    ntp = {v[4] for v in plans.values()}
    assert 1 in ntp and max(ntp) > 1
    assert any(v[4] > 1 and v[0] % v[2] for v in plans.values()) and any(v[1] % v[3] for v in plans.values())
    mt = {v[2] * v[3]: v[2:4] for v in plans.values()}
    assert mt.get(121) == (11, 11) and mt.get(126) == (6, 21), sorted(mt)
    # the table of the module that asked for these lengths, level 0 (L0) and level 1 (L1)
    assert plans[9, 0][2:4] == (9, 14) and plans[16, 0][2:] == (16, 8, 1, 10) and plans[17, 0][2:] == (9, 14, 2, 6)
    assert plans[33, 0][2:4] == (11, 11) and plans[65, 0][2:4] == (6, 21) and plans[65, 1][2:] == (11, 11, 3, 4)
    assert plans[129, 0][4:] == (17, 5)
    assert plans[129, 1][2:] == (6, 21, 11, 2)


@pytest.mark.parametrize("T", chk.EDGE_T)
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_steps_at_edge_lengths(compute, T):
    labels = set(run_case(compute, ("edge", 80, "ASP", True, T), tag=f"T={T}"))
    assert _gemm_labels(compute, 3, T, 80) <= labels, sorted(labels)


@pytest.mark.parametrize("case", [("edge", 64, "ASP", True, 33), ("edge", 80, "SAP", True, 33), ("edge", 80, "ASP", False, 17)],
                         ids=["n_mels64", "sap", "nolog"])
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_steps_of_other_configurations(compute, case):
    labels = set(run_case(compute, case, tag=f"{case[1]} {case[2]} log={case[3]} T={case[4]}"))
    assert _gemm_labels(compute, 3, case[4], case[1]) <= labels, sorted(labels)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_steps_at_full_size_from_waveforms(compute):
    """xin from waveforms: the TitaNet work left an f32 gain offset of 3.0e-8 of its prolog open; here xin/gain from waveforms is printed
    beside its bar (tests/resnetse_oracle_check.py records the value)"""
    labels = set(run_case(compute, ("full", 80, "ASP", True, chk.FULL_T), rows=chk.FULL_ROWS, tag="full size"))
    assert _gemm_labels(compute, 3, chk.FULL_T, 80) <= labels, sorted(labels)
    assert "fbank" in labels


# ---- ragged packs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_steps_of_ragged_packs(compute):
    w = chk.weights()
    e = Engine(model="resnetse", compute=compute, channels=2, n_mels=80, embed_dim=chk.NOUT, max_batch=8, samples=chk.engine_samples(65), log_input=True,
               input_norm=True)
    e.load_state_dict(w["sd"])
    e.finalize()
    for case, tag in ((("ragged", 80, "ASP", True, 0), "ragged"), (("ragged1", 80, "ASP", True, 0), "ragged n=1")):
        labels = run_case(compute, case, tag=tag, engine=e)
        heads = {x.split()[0] for x in labels}
        assert {"rs_rag_tiles", "rs_stem_rag", "rs_se_gate_rag", "rs_se_apply_rag", "rag_gemm", "rag_asp_pool", "rag_fc"} <= heads, heads
        assert not heads & (FIXED - PACKED), heads
    e.close()


# ---- the census ------------------------------------------------------------------------------------------------------------------------
CONVS = {"rs_conv3x3_s1", "rs_conv3x3_s2", "rs_conv3x3_s3", "rs_conv3x3_s4", "rs_down"}
FIXED = CONVS | {"fbank", "prologue", "rs_stem", "rs_se_gate", "rs_se_apply", "gemm_pw", "rs_asp_pool", "rs_in_check", "rs_fc", "emb_out"}
PACKED = CONVS | {"rag_rows", "rs_rag_tiles", "rag_prologue", "rs_stem_rag", "rs_se_gate_rag", "rs_se_apply_rag", "rag_gemm", "rag_asp_pool",
                  "rs_in_check", "rag_fc", "emb_out"}


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_route_census(compute):
    """every kernel a ResNetSE forward of this compute reaches ran in a case checked against the oracle, and nothing else ran; the worst
    GPU value of every check over the file (the third column of the bars' tables)"""
    have = _CENSUS[compute]
    if "T=33" not in have:
        test_steps_at_edge_lengths(compute, 33)
    if "full size" not in have:
        test_steps_at_full_size_from_waveforms(compute)
    if "ragged" not in have:
        test_steps_of_ragged_packs(compute)
    seen = set()
    for tag, heads in sorted(have.items()):
        print(f"census {compute} {tag}: {' '.join(heads)}")
        seen |= set(heads)
    for n in chk.CHECKS:
        print(f"worst {compute} {n}: {_WORST[compute][n]:.1e} (bar {chk.bars(compute)[n]:.1e})")
    assert not seen & {"gemm_n128", "gemm_pw2", "gemm_pw3", "gemm_pw3cv16", "gemm_generic"}, seen
    assert seen == FIXED | PACKED, (sorted(seen - (FIXED | PACKED)), sorted((FIXED | PACKED) - seen))


# ---- rs_keep leaves the forward alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_rs_keep_leaves_the_forward_alone(compute, ragged):
    """embed; embed with rs_keep on and read every stage; embed with it off: bit-identical embeddings, the same profile labels and
    launch counts.  Without the option a kept stage is refused with SVHIP_ERR_STATE; the six older stages are served either way, and
    rs_layer<s> is bit-equal to the kept out of the stage's last block"""
    T = 65
    e = Engine(model="resnetse", compute=compute, channels=2, n_mels=80, embed_dim=chk.NOUT, max_batch=8, samples=chk.engine_samples(T), log_input=True,
               input_norm=True)
    e.load_state_dict(chk.weights()["sd"])
    e.finalize()
    x = chk.ragged_features() if ragged else chk.features(3, T)
    embed = e.embed_features_ragged if ragged else e.embed_features
    old = ("rs_stem", "rs_layer1", "rs_layer2", "rs_layer3", "rs_layer4", "rs_pool")
    names = [n for n, _, _, _ in _stage_list()] + list(old[1:5])
    runs = []
    for keep in (0, 1, 0):
        e.set_option("rs_keep", keep)
        e.profile(True)
        emb = np.asarray(embed(x)).copy()
        prof = {n: r["launches"] for n, r in e.profile_results().items()}
        e.profile(False)
        stages = {}
        for name in names:
            if keep or name in old:
                stages[name] = e.get_stage(name)
                assert np.isfinite(stages[name]).all(), name
            else:
                with pytest.raises(_lib.SvhipError, match="option rs_keep was not set") as ei:
                    e.get_stage(name)
                assert ei.value.code == ERR_STATE, name
        if keep:
            for s, last in enumerate((2, 6, 12, 15)):
                assert np.array_equal(stages[f"rs_layer{s + 1}"], stages[f"rs_b{last}_out"])
        runs.append((emb, prof, {n: stages[n] for n in old}))
    e.close()
    for emb, prof, st in runs[1:]:
        assert np.array_equal(emb, runs[0][0]) and prof == runs[0][1]
        for n in old:
            assert np.array_equal(st[n], runs[0][2][n]), n
    print(f"{compute} {'ragged' if ragged else 'fixed'}: sha1 {hashlib.sha1(runs[0][0].tobytes()).hexdigest()}")
