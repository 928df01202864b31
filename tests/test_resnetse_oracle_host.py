"""CPU: the ResNetSE34V2 oracle (oracle/resnetse.py) is the reference's arithmetic, and the bars of tests/resnetse_oracle_check.py can fail.

1. The oracle's steps compose to the reference: forward against tests/golden/resnetse34v2.npz (the reference module's own float64
   outputs) to 1e-9 of scale — every case and length through tests/test_resnetse_host.py::ref64, which wraps it; here the short lengths
   again, with the steps called one by one on each other's outputs.
2. A handle is emulated on the CPU (resnetse_oracle_check.emulate).  Its layer-local errors are what the bars are: 3 x the worst over
   the cases the GPU file runs.  (fp32 sums differ between CPU builds and thread counts, so the test holds bar / emulation within
   [2, 4.5], not at 3.)
3. Each fault of FAULTS — a mistake rs_conv_kernel, the stem, the SE gate, the block tail, the pooling or the host's weight packing
   could make — is injected into one step of the emulation, at every edge length and in both computes ('SAP' faults on the 'SAP' case).
   The step's check family must exceed a bar by at least 2 x at every length where the fault changes the exact result (float64), and
   every fault must be exercised at one length at least.

THE FAULT TABLE (fault: the check that sees it, the smallest and largest ratio to its bar over the lengths, f32 | bf16):
    taps_transposed                conv1     3.3e6 - 4.9e6 x      | 3.9e3 - 6.9e3 x
    pad_missing_last_frame         conv1     1.1e5 - 3.4e5 x      | 1.4e3 - 2.3e3 x
    pad_missing_last_mel_row       conv1     5.3e4 - 2.0e5 x      | 6.8e2 - 2.6e3 x
    stride_two_odd                 conv1     2.9e6 - 5.3e6 x      | 3.0e3 - 8.9e3 x
    down_pad_offset                down      1.5e7 - 3.2e7 x      | 2.0e3 - 3.4e3 x
    relu_in_missing                conv1     8.5e4 - 3.7e5 x      | 1.4e2 - 2.3e2 x
    residual_from_x                out       4.2e6 - 4.9e6 x      | 64 - 75 x
    relu_on_down_residual          out       5.7e7 - 1.4e8 x      | 8.8e2 - 2.1e3 x
    stem_bn_before_relu            stem      5.4e6 - 2.3e7 x      | 68 - 1.5e2 x
    shift_after_relu               conv1     3.2e5 - 1.2e6 x      | 2.6e2 - 5.2e2 x
    part_beyond_image              part      1.0e5 - 3.2e5 x      | 1.4e5 - 4.5e5 x
    gate_last_tile_dropped         gate      2.0e2 - 5.3e4 x      | 1.6e2 - 4.5e4 x
    mean_over_covered_positions    gate      1.2e4 - 5.2e4 x      | 1.0e4 - 4.3e4 x
    gate_of_neighbour              out       1.9e5 - 1.6e6 x      | 2.7 - 24 x
    rows_beyond_tile_stored        conv2     1.4e5 - 3.4e5 x      | 1.5e3 - 1.9e3 x
    chunk_skipped                  conv1     4.5e6 - 5.2e6 x      | 1.4e3 - 1.8e3 x
    conv1_not_rounded              conv2     (nothing to skip)    | 5.3 - 10 x
    attention_columns_unpermuted   att       3.8e5 - 5.2e5 x      | 2.2e3 - 4.2e3 x
    variance_clamp_missing         pool_raw  1.9e2 - 5.9e2 x      | 2.2e2 - 6.8e2 x
    sap_reads_the_std_half         emb       4.1e5 x              | 3.2e5 x
    fc_columns_unpermuted          emb       5.1e5 - 9.1e5 x      | 4.0e5 - 7.2e5 x
(part_beyond_image and mean_over_covered_positions change nothing where the tiles cover the image exactly, T = 8 and 16;
rows_beyond_tile_stored applies to the 126- and 121-position tiles of T = 17, 33, 65; sap_reads_the_std_half runs on the 'SAP' case.)

BLIND — faults not caught at 2 x at every length where they apply — is empty: the weakest are, on bf16, the neighbour's gate at T = 129
(out/local at 2.7 x: two utterances' gates differ little in most channels) and conv1 left unrounded (conv2/local at 5.3 - 10 x).  The
test asserts for a fault listed in BLIND that it stays below 2 x somewhere, so the list cannot go stale."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import resnetse as orr
from speakerverification_amd import synth
from tests import resnetse_oracle_check as chk
from tests.test_resnetse_host import load_golden, mel_of

P0, P3 = "layer1.0.", "layer2.0."            # block 0 (identity residual, the stem's signed output) and block 3 (stride 2, downsample)


def _rel(a, b):
    return float(np.abs(a - b).max()) / float(np.abs(b).max())


# ---- 1. the oracle is the reference's arithmetic ------------------------------------------------------------------------------------
def test_the_steps_compose_to_the_reference(golden_dir):
    g = load_golden(golden_dir)
    sd = orr.to_torch_sd(synth.synth_state_dict(synth.resnetse_param_spec(int(g["nOut"])), seed=int(g["seed_w"])))
    for L in (640, 512):
        mel = torch.from_numpy(mel_of(L, 80, int(g["B"]), int(g["seed_x"]))).double()
        out = []
        with torch.no_grad():
            for m in mel:
                x = orr.stem(orr.prologue(m), sd)
                for p in orr.block_names(sd):
                    u = orr.conv1(x, sd, p)
                    v = orr.conv2(u, sd, p)
                    gt = orr.gate(orr.squeeze_tiles(orr.tile_sums(v), v.shape[0] * v.shape[1]), sd, p)
                    x = orr.out(v, gt, orr.down(x, sd, p), res_relu=False) if orr.has_down(sd, p) else orr.out(v, gt, x)
                xf = orr.flat(x)
                out.append(orr.fc(orr.pool_stats(orr.logits(orr.att(xf, sd), sd), xf), sd).numpy())
                assert _rel(out[-1], orr.forward(m, sd).numpy()) <= 1e-12
        r = _rel(np.stack(out), g[f"mel_asp_80_out64_L{L}"])
        print(f"L={L}: the steps to the reference's float64 {r:.2e} of scale")
        assert r <= 1e-9, (L, r)


def test_rounded_weights_are_what_a_bf16_handle_reads():
    """folded_sd: no BatchNorm key left, every scale / shift an fp32 number folded in double; rounded_sd rounds exactly the block
    convolutions, the downsamples and the two attention convolutions to bf16"""
    w = chk.weights()
    f, r, full = w["f32"][1], w["bf16"][1], w["full"]
    assert set(f) == set(r) and not [k for k in f if "running" in k or "num_batches" in k]
    mfma = [k for k in f if orr.is_mfma_weight(k)]
    assert len(mfma) == 2 * 16 + 3 + 2, mfma
    for k, v in f.items():
        assert torch.equal(r[k], orr.bf16_round(v) if k in mfma else v), k
        if k.endswith(".scale") or k.endswith(".shift"):
            assert torch.equal(v, v.float().double()), k
        else:
            assert torch.equal(v, full[k]), k
    s = full["layer2.0.bn1.weight"] / torch.sqrt(full["layer2.0.bn1.running_var"] + 1e-5)
    assert torch.equal(f["layer2.0.bn1.scale"], s.float().double())


# ---- 2. the bars are the emulation's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_bars_are_three_times_the_clean_emulation(compute):
    worst = chk.emulation_worst(compute)
    bar = chk.bars(compute)
    assert set(worst) == set(chk.CHECKS) == set(bar)
    for n in chk.CHECKS:
        print(f"{compute} {n}: emulation {worst[n]:.2e}, bar {bar[n]:.2e}")
    assert worst["pool"] == 0.0 and bar["pool"] == 0.0                      # (the pooling's affine is the identity: pool is pool_raw)
    off = {n: bar[n] / worst[n] for n in chk.CHECKS if n != "pool" and not 2.0 <= bar[n] / worst[n] <= 4.5}
    assert not off, off


def test_every_emulated_utterance_shows_every_check():
    for compute in ("f32", "bf16"):
        for case in chk.CASES:
            emu = chk.emulated_case(compute, case)
            assert len(emu) == {"full": len(chk.FULL_ROWS), "ragged": len(chk.RAGGED_T), "ragged1": 1}.get(case[0], 3)
            for _, _, err in emu:
                assert set(err) == set(chk.CHECKS), (compute, case)
                assert not chk.failures(err, compute), (compute, case, chk.failures(err, compute))


def test_the_cases_are_the_ones_the_bars_were_built_on():
    edge = {("edge", 80, "ASP", True, T) for T in chk.EDGE_T}
    other = {("edge", 64, "ASP", True, 33), ("edge", 80, "SAP", True, 33), ("edge", 80, "ASP", False, 17), ("full", 80, "ASP", True, 401),
             ("ragged", 80, "ASP", True, 0), ("ragged1", 80, "ASP", True, 0)}
    assert set(chk.CASES) == edge | other
    assert chk.EDGE_T == (2, 3, 5, 8, 9, 16, 17, 33, 65, 129) and chk.RAGGED_T == (2, 3, 5, 8, 9, 17, 33, 65) and chk.RAGGED_ONE_T == (33,)
    assert [chk.engine_kw(T)["samples"] // chk.engine_kw(T)["hop_length"] + 1 for T in chk.EDGE_T] == list(chk.EDGE_T)


# ---- 3. every bar fails on a subtly wrong kernel ------------------------------------------------------------------------------------
def _affine(sd, bn, acc):
    s, t = orr._bn_affine(sd, bn)
    return s.expand_as(acc), t.expand_as(acc)


def _store_rows_beyond_the_tile(y, stride=1):
    """rs_conv_kernel without `m < mt` in its store: rows mt .. 127 of a tile hold position 0 of the tile again and land at (p0 + m / TQ,
    q0 + m % TQ) wherever that lies inside the image (the next tile's first rows)"""
    P, Q, _ = y.shape
    TP, TQ, ntp, ntq = orr.tile_grid(P, Q, stride, 3)
    y = y.clone()
    src = y.clone()
    for tp in range(ntp):
        for tq in range(ntq):
            for m in range(TP * TQ, 128):
                po, qo = tp * TP + m // TQ, tq * TQ + m % TQ
                if po < P and qo < Q:
                    y[po, qo] = src[tp * TP, tq * TQ]
    return y


def conv_direct(x, xn, sd, conv, bn, stride, relu_out, store, fault=None, ck=16):
    """conv + BN (+ ReLU) of the block input x as rs_conv_kernel runs it (the ReLU on the operand, zero padding, the epilogue as one
    multiply-add); xn: the neighbouring utterance's input"""
    a = x if fault == "relu_in_missing" else torch.relu(x)
    w = sd[conv + ".weight"]
    P, Q, _ = a.shape
    if fault == "taps_transposed":
        w = w.transpose(2, 3)
    if fault == "chunk_skipped":                            # the last K chunk of input channels never added
        a = a.clone()
        a[..., -ck:] = 0
    if fault == "pad_missing_last_frame":                   # the row behind the last frame is the next utterance's first frame
        a = torch.cat([a, torch.relu(xn[:1])])
    if fault == "pad_missing_last_mel_row":                 # the column behind the last mel row is the next frame's first (flat memory)
        a = torch.cat([a, torch.cat([a[1:, :1], torch.relu(xn[:1, :1])])], dim=1)
    if fault == "stride_two_odd":                           # positions 2 p + 1 where 2 p are meant
        full = F.pad(orr._conv(a, w, 1), (0, 0, 0, 1, 0, 1))
        acc = full[1::2, 1::2][:orr.out_size(P, 2), :orr.out_size(Q, 2)]
    elif fault == "down_pad_offset":                        # the 1 x 1 convolution read with the 3 x 3 one's pad of one position
        acc = orr._conv(F.pad(a, (0, 0, 1, 0, 1, 0))[:-1, :-1], w, stride)
    else:
        acc = orr._conv(a, w, stride)[:orr.out_size(P, stride), :orr.out_size(Q, stride)]
    s, t = _affine(sd, bn, acc)
    if fault == "shift_after_relu":
        y = torch.relu(acc * s) + t
    else:
        y = orr._fma(acc, s, t)
        y = torch.relu(y) if relu_out else y
    if fault == "rows_beyond_tile_stored":
        y = _store_rows_beyond_the_tile(y)
    return store(y)


def part_direct(S, sd, store, fault=None):
    """block 0's tile sums from the stored conv1: conv2's unrounded values summed per tile in the kernel's order"""
    v = conv_direct(S["b0_conv1"], None, sd, P0 + "conv2", P0 + "bn2", 1, False, orr.ident)
    if fault != "part_beyond_image":
        return orr.tile_sums(v, True)
    # `ok` dropped: the positions of a partial tile beyond the image are added too — what the convolution gives there, its halo zero
    P, Q, _ = v.shape
    TP, TQ, ntp, ntq = orr.tile_grid(P, Q)
    u = F.pad(S["b0_conv1"], (0, 0, 0, ntq * TQ - Q, 0, ntp * TP - P))
    ve = conv_direct(u, None, sd, P0 + "conv2", P0 + "bn2", 1, False, orr.ident)
    t = ve.reshape(ntp, TP, ntq, TQ, -1).permute(0, 2, 1, 3, 4).reshape(ntp * ntq, TP * TQ, -1)
    return t.sum(dim=1)


def gate_direct(S, sd, fault=None):
    part = S["b0_part"]
    P, Q, _ = S["b0_conv2"].shape
    TP, TQ, ntp, ntq = orr.tile_grid(P, Q)
    n = ntp * TP * ntq * TQ if fault == "mean_over_covered_positions" else P * Q
    if fault == "gate_last_tile_dropped":
        part = torch.cat([part[:-1], torch.zeros_like(part[:1])])
    return orr.gate(orr.squeeze_tiles(part, n), sd, P0)


def pool_direct(S, fault=None):
    xf = orr.flat(S["b15_out"])
    return orr.pool_stats(S["logits"], xf, centred=True, clamp=None if fault == "variance_clamp_missing" else 1e-5)


def handle_cols(v, C=256):
    """the reference's columns c Q + q -> a handle's q C + c"""
    return v.reshape(v.shape[0], C, -1).swapaxes(1, 2).reshape(v.shape[0], -1)


# fault: (the check family that guards it, f(S, Sn, W, store, fault, compute) -> that stage of the faulty handle; fault None: the clean
# step).  S / Sn: the clean emulation's stages of the utterance and of its neighbour in the batch, as tensors of the dtype of the weights W
def _c1(S, Sn, W, store, fault, compute):
    return conv_direct(S["stem"], Sn["stem"], W, P0 + "conv1", P0 + "bn1", 1, True, store, fault, chk.CK[compute])


def _c1s2(S, Sn, W, store, fault, compute):
    return conv_direct(S["b2_out"], Sn["b2_out"], W, P3 + "conv1", P3 + "bn1", 2, True, store, fault)


def _c2(S, Sn, W, store, fault, compute):
    u = S["b0_conv1"]
    if fault == "conv1_not_rounded":                        # conv2 reads conv1's fp32 values, not what was stored in bf16
        u = conv_direct(S["stem"], None, W, P0 + "conv1", P0 + "bn1", 1, True, orr.ident)
    return conv_direct(u, None, W, P0 + "conv2", P0 + "bn2", 1, False, store, fault)


def _down(S, Sn, W, store, fault, compute):
    return conv_direct(S["b2_out"], Sn["b2_out"], W, P3 + "downsample.0", P3 + "downsample.1", 2, False, store, fault)


def _stem(S, Sn, W, store, fault, compute):
    return orr.stem(S["xin"], W, store, "bn_relu" if fault == "stem_bn_before_relu" else "relu_bn")


def _out0(S, Sn, W, store, fault, compute):
    g = Sn["b0_gate"] if fault == "gate_of_neighbour" else S["b0_gate"]
    return orr.out(S["b0_conv2"], g, S["stem"], store, res_relu=fault != "residual_from_x")


def _out3(S, Sn, W, store, fault, compute):
    return orr.out(S["b3_conv2"], S["b3_gate"], S["b3_down"], store, res_relu=fault == "relu_on_down_residual")


def _part(S, Sn, W, store, fault, compute):
    return part_direct(S, W, store, fault)


def _gate(S, Sn, W, store, fault, compute):
    return gate_direct(S, W, fault)


def _att(S, Sn, W, store, fault, compute):
    xf = orr.flat(S["b15_out"])
    return orr.att(handle_cols(xf) if fault == "attention_columns_unpermuted" else xf, W, store)


def _pool_raw(S, Sn, W, store, fault, compute):
    return pool_direct(S, fault)


def _emb(S, Sn, W, store, fault, compute):
    pool = S["pool"]
    F_ = pool.shape[0] // 2
    if fault == "sap_reads_the_std_half":
        pool = torch.cat([pool[F_:], pool[:F_]])
    if fault == "fc_columns_unpermuted":
        pool = handle_cols(pool.reshape(2, -1)).reshape(-1)
    return orr.fc(pool, W)


FAULTS = {
    "taps_transposed": ("conv1", _c1), "pad_missing_last_frame": ("conv1", _c1), "pad_missing_last_mel_row": ("conv1", _c1),
    "stride_two_odd": ("conv1", _c1s2), "down_pad_offset": ("down", _down), "relu_in_missing": ("conv1", _c1),
    "residual_from_x": ("out", _out0), "relu_on_down_residual": ("out", _out3), "stem_bn_before_relu": ("stem", _stem),
    "shift_after_relu": ("conv1", _c1), "part_beyond_image": ("part", _part), "gate_last_tile_dropped": ("gate", _gate),
    "mean_over_covered_positions": ("gate", _gate), "gate_of_neighbour": ("out", _out0), "rows_beyond_tile_stored": ("conv2", _c2),
    "chunk_skipped": ("conv1", _c1), "conv1_not_rounded": ("conv2", _c2), "attention_columns_unpermuted": ("att", _att),
    "variance_clamp_missing": ("pool_raw", _pool_raw), "sap_reads_the_std_half": ("emb", _emb), "fc_columns_unpermuted": ("emb", _emb),
}
# layer_local's reference of each direct step: the oracle's step on the stored input
ORACLE_OF = {
    _c1: lambda S, sd: orr.conv1(S["stem"], sd, P0), _c1s2: lambda S, sd: orr.conv1(S["b2_out"], sd, P3),
    _c2: lambda S, sd: orr.conv2(S["b0_conv1"], sd, P0), _down: lambda S, sd: orr.down(S["b2_out"], sd, P3),
    _stem: lambda S, sd: orr.stem(S["xin"], sd), _out0: lambda S, sd: orr.out(S["b0_conv2"], S["b0_gate"], S["stem"]),
    _out3: lambda S, sd: orr.out(S["b3_conv2"], S["b3_gate"], S["b3_down"], res_relu=False),
    _part: lambda S, sd: orr.tile_sums(orr.conv2(S["b0_conv1"], sd, P0)),
    _gate: lambda S, sd: orr.gate(orr.squeeze(S["b0_conv2"]), sd, P0), _att: lambda S, sd: orr.att(orr.flat(S["b15_out"]), sd),
    _pool_raw: lambda S, sd: orr.pool_stats(S["logits"], orr.flat(S["b15_out"])), _emb: lambda S, sd: orr.fc(S["pool"], sd),
}
SAP_CASE = ("edge", 80, "SAP", True, 33)
EDGE_CASES = tuple(c for c in chk.CASES if c[0] == "edge" and c[1:4] == (80, "ASP", True))
ROUNDING_FAULTS = ("conv1_not_rounded",)          # (an f32 handle stores conv1 unrounded: nothing to skip)


def _cases_of(fault):
    return (SAP_CASE,) if fault == "sap_reads_the_std_half" else EDGE_CASES


def _tensors(compute, case, dtype):
    """(S, Sn, W) of utterance 0 and its neighbour 1 of an edge case, in dtype"""
    emu = chk.emulated_case(compute, case)
    out = [{k: torch.from_numpy(v).to(dtype) for k, v in emu[b][0].items()} for b in (0, 1)]
    return out[0], out[1], chk.weights(case[1], case[2])[compute][0 if dtype == torch.float32 else 1]


def _fault_ratio(compute, case, fault):
    """(applies to this case, the largest error / bar over the guarding family, the check that gave it) for utterance 0 of the case"""
    stage, f = FAULTS[fault]
    q = orr.bf16_round if compute == "bf16" else orr.ident
    with torch.no_grad():
        S64, Sn64, W64 = _tensors(compute, case, torch.float64)
        # (a fault in WHAT is rounded changes nothing in exact arithmetic: it is looked for with the handle's rounding on)
        q64 = q if fault in ROUNDING_FAULTS else orr.ident
        clean = f(S64, Sn64, W64, q64, None, compute)
        exact = f(S64, Sn64, W64, q64, fault, compute)
        if not float((exact - clean).abs().max()) > 1e-9 * float(clean.abs().max()):
            return False, 0.0, ""
        ref = ORACLE_OF[f](S64, W64)
        with orr.matmul_as(orr.chained_matmul(chk.KSTEP[compute])), orr.conv_as(orr.chained_conv(chk.CK[compute], chk.KSTEP[compute])):
            got = f(*_tensors(compute, case, torch.float32), q, fault, compute).double().numpy()
        bar = chk.bars(compute)
        if stage == "gate":
            return True, chk.gate_err(got, S64["b0_conv2"], orr.conv2(S64["b0_conv1"], W64, P0), W64, P0)[0] / bar["gate"], "gate"
        if stage == "part":
            (e, _), (et, _) = chk.part_errs(got, orr.conv2(S64["b0_conv1"], W64, P0))
            return (True,) + max((e / bar["part"], "part"), (et / bar["part_total"], "part_total"))
    if stage in chk.VECTOR_STAGES:
        return True, chk.rel_err(got, ref.numpy())[0] / bar[stage], stage
    r = {stage + form: e / bar[stage + form] for form, (e, _) in chk.frame_errs(got.reshape(-1, got.shape[-1]), ref.numpy().reshape(-1, got.shape[-1])).items()}
    name = max(r, key=r.get)
    return True, r[name], name


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_the_direct_steps_are_the_oracles(compute):
    """the fault-free forms of the kernels' restatements above against the oracle's steps, on the emulation's stored inputs"""
    for case in (EDGE_CASES[1], EDGE_CASES[6], EDGE_CASES[7], SAP_CASE):
        S, Sn, W = _tensors(compute, case, torch.float64)
        with torch.no_grad():
            for fault, (stage, f) in FAULTS.items():
                want = ORACLE_OF[f](S, W)
                got = f(S, Sn, W, orr.ident, None, compute)
                if f is _gate:                              # (from the emulation's own tile sums: those of its unrounded conv2)
                    assert chk.gate_err(got.numpy(), S["b0_conv2"], orr.conv2(S["b0_conv1"], W, P0), W, P0)[0] <= chk.bars(compute)["gate"]
                elif f is _pool_raw:                        # (the centred variance: the same number to rounding)
                    assert _rel(got.numpy(), want.numpy()) <= 1e-9, (fault, case)
                else:
                    assert _rel(got.numpy(), want.numpy()) <= 1e-12, (fault, case)


# Not caught at 2 x at every length (module docstring): {(fault, compute)}
BLIND = set()

FAULT_CASES = [(f, c) for f in sorted(FAULTS) for c in ("f32", "bf16") if not (f in ROUNDING_FAULTS and c == "f32")]


@pytest.mark.parametrize("fault,compute", FAULT_CASES)
def test_every_bar_is_at_most_half_the_fault_it_guards(fault, compute):
    hit, low = [], []
    for case in _cases_of(fault):
        applies, ratio, name = _fault_ratio(compute, case, fault)
        if applies:
            hit.append(case)
            print(f"{compute} {fault} T={case[4]}: {name} at {ratio:.1f} x its bar")
            if ratio < 2.0:
                low.append((case[4], name, round(ratio, 2)))
    assert hit, "the fault changes nothing in any tested case"
    if (fault, compute) in BLIND:
        assert low, "the fault is caught after all: take it out of BLIND"
    else:
        assert not low, (fault, compute, low)
