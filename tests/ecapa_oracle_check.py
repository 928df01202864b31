"""ECAPA-TDNN stages against the float64 oracle (oracle/ecapa.py), one utterance at a time: the comparisons and bars of
tests/test_gpu_ecapa_oracle.py.  They need no GPU, so tests/test_ecapa_oracle_host.py can show on CPU emulations of a bf16 handle
that every bar fails when the value it guards is subtly wrong.

Layer-local checks.  Each stage of the handle (svhip_get_stage) is compared with the oracle's block applied in float64 to the
handle's OWN previous stage: blocks.0 from the handle's input features, blocks.i from blocks.(i - 1), inside block 3 tdnn1 ->
Res2Net chain -> tdnn2 -> SE gate, mfa from blocks.1 .. 3, the ASP statistics from mfa, the attention from mfa and those
statistics, the pooled vector from the attention and mfa, asp_bn, the embedding (fc) and, last, the embedding end to end.  The
error of a stage is max |got - ref| / max |ref| over ONE utterance, so one wrong row, frame or 256-row tile fails; a failure names
the frame and channel of the worst element.

bf16 handles read bf16 weights (upload_h16: round to nearest even; BN folded into the fp32 epilogue, not into the weights), and
the layer-local references read the same rounded weights (rounded_sd): what remains is the rounding of the stored activations and
the kernels' fp32 sums, far below the errors the checks look for.  The end-to-end reference reads the full-precision weights.

The reductions over time (the SE squeeze, the ASP statistics, the attention softmax) change by about 1/T when one frame is dropped
or doubled — less than a block output's bf16 noise — so each has a check of its own against the handle's stored input:
blocks.3.se_gate (squeeze + SE MLP) from blocks.3.tdnn2, asp_gstats from mfa, asp from asp_att and mfa.  Their bf16 bars sit at
least 4x below the effect of one frame at every length the tests run (REDUCTIONS; tests/test_ecapa_oracle_host.py checks it)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ecapa as o_ecapa

STAGES = ("input", "blocks.0", "blocks.1", "blocks.2", "blocks.3.tdnn1", "blocks.3.res2net", "blocks.3.tdnn2", "blocks.3.se_gate",
          "blocks.3", "mfa", "asp_gstats", "asp_att", "asp", "asp_bn", "emb", "end_to_end")
HANDLE_STAGES = STAGES[:-2]                        # what svhip_get_stage returns ("emb" is the forward's output)
VECTOR_STAGES = ("blocks.3.se_gate", "asp_gstats", "asp", "asp_bn")     # (B, n) f32 per utterance; the others (B * T, channels)
REDUCTIONS = ("blocks.3.se_gate", "asp_gstats", "asp")

# The bars: the largest error measured over every case of tests/test_gpu_ecapa_oracle.py (beside each bar; for bf16 also the clean
# emulation of tests/test_ecapa_oracle_host.py where it is larger), times about 1.5.  Keys: the stage (max |diff| / max |ref|), and for
# (T, channels) stages also `stage/local` (local_err) and `stage/bias` (bias_err).  On f32 / f32x3 handles asp_att is the loosest
# stage: the ASP statistics come from one pass (E[x^2] - mean^2 in fp32), whose std carries the cancellation of channels that barely
# vary over time into the attention's per-utterance bias.  bf16 whole-block checks (blocks.1 / blocks.2: their chains' internal
# roundings) have loose local / bias bars; the stages inside block 3 are each checked on their own input at the bf16 rounding floor.
def _checks():
    out = []
    for s in STAGES:
        out.append(s)
        if s not in VECTOR_STAGES and s not in ("emb", "end_to_end"):
            out += [s + "/local", s + "/bias"]
    return tuple(out)


CHECKS = _checks()
F32_BARS = {
    "input": 8e-06,                  # 4.4e-06
    "input/local": 8e-05,            # 4.6e-05
    "input/bias": 6e-06,             # 3.9e-06
    "blocks.0": 1.5e-06,             # 9.5e-07
    "blocks.0/local": 2.5e-05,       # 1.5e-05
    "blocks.0/bias": 6e-07,          # 3.7e-07
    "blocks.1": 2e-06,               # 1.1e-06
    "blocks.1/local": 8e-05,         # 4.0e-05
    "blocks.1/bias": 6e-06,          # 3.7e-06
    "blocks.2": 4e-06,               # 2.0e-06
    "blocks.2/local": 5e-05,         # 3.2e-05
    "blocks.2/bias": 1.5e-05,        # 9.7e-06
    "blocks.3.tdnn1": 3e-06,         # 1.8e-06
    "blocks.3.tdnn1/local": 4e-05,   # 2.5e-05
    "blocks.3.tdnn1/bias": 2e-06,    # 1.2e-06
    "blocks.3.res2net": 1.5e-06,     # 8.4e-07
    "blocks.3.res2net/local": 3e-05, # 1.9e-05
    "blocks.3.res2net/bias": 5e-06,  # 2.7e-06
    "blocks.3.tdnn2": 1.5e-06,       # 9.9e-07
    "blocks.3.tdnn2/local": 3e-05,   # 1.8e-05
    "blocks.3.tdnn2/bias": 8e-06,    # 4.7e-06
    "blocks.3.se_gate": 1e-05,       # 5.7e-06
    "blocks.3": 1e-07,               # 4.5e-08
    "blocks.3/local": 1e-07,         # 5.8e-08
    "blocks.3/bias": 1.5e-07,        # 8.9e-08
    "mfa": 2.5e-06,                  # 1.6e-06
    "mfa/local": 6e-05,              # 3.9e-05
    "mfa/bias": 2e-06,               # 1.3e-06
    "asp_gstats": 2.5e-07,           # 1.5e-07
    "asp_att": 0.00015,              # 8.2e-05
    "asp_att/local": 0.002,          # 1.2e-03
    "asp_att/bias": 8e-05,           # 4.2e-05
    "asp": 3e-07,                    # 1.8e-07
    "asp_bn": 1.2e-07,               # 7.1e-08
    "emb": 3e-07,                    # 2.0e-07
    "end_to_end": 5e-06,             # 2.9e-06
}
F32X3_BARS = {
    "input": 8e-06,                  # 4.2e-06
    "input/local": 0.0001,           # 6.0e-05
    "input/bias": 8e-06,             # 4.3e-06
    "blocks.0": 1.5e-06,             # 8.2e-07
    "blocks.0/local": 2e-05,         # 1.1e-05
    "blocks.0/bias": 5e-07,          # 2.8e-07
    "blocks.1": 2.5e-06,             # 1.4e-06
    "blocks.1/local": 5e-05,         # 3.1e-05
    "blocks.1/bias": 1.5e-05,        # 8.5e-06
    "blocks.2": 4e-06,               # 2.2e-06
    "blocks.2/local": 8e-05,         # 4.9e-05
    "blocks.2/bias": 4e-05,          # 2.3e-05
    "blocks.3.tdnn1": 1.2e-06,       # 6.7e-07
    "blocks.3.tdnn1/local": 2.5e-05, # 1.6e-05
    "blocks.3.tdnn1/bias": 1.2e-06,  # 7.9e-07
    "blocks.3.res2net": 1e-06,       # 6.4e-07
    "blocks.3.res2net/local": 3e-05, # 1.8e-05
    "blocks.3.res2net/bias": 6e-06,  # 3.8e-06
    "blocks.3.tdnn2": 1.5e-06,       # 8.4e-07
    "blocks.3.tdnn2/local": 4e-05,   # 2.0e-05
    "blocks.3.tdnn2/bias": 1.2e-05,  # 7.3e-06
    "blocks.3.se_gate": 8e-06,       # 4.3e-06
    "blocks.3": 2.5e-07,             # 1.6e-07
    "blocks.3/local": 3e-07,         # 1.7e-07
    "blocks.3/bias": 2e-07,          # 1.2e-07
    "mfa": 2e-06,                    # 1.3e-06
    "mfa/local": 6e-05,              # 3.6e-05
    "mfa/bias": 2e-05,               # 1.3e-05
    "asp_gstats": 5e-06,             # 3.0e-06
    "asp_att": 0.00015,              # 8.6e-05
    "asp_att/local": 0.006,          # 3.4e-03
    "asp_att/bias": 0.00012,         # 7.9e-05
    "asp": 1e-07,                    # 5.0e-08
    "asp_bn": 1.2e-07,               # 7.5e-08
    "emb": 4e-07,                    # 2.2e-07
    "end_to_end": 6e-06,             # 3.8e-06
}
BF16_BARS = {
    "input": 0.005,                  # 3.2e-03
    "input/local": 0.015,            # 9.7e-03
    "input/bias": 0.0025,            # 1.6e-03
    "blocks.0": 0.006,               # 3.5e-03
    "blocks.0/local": 0.006,         # 3.8e-03
    "blocks.0/bias": 0.0025,         # 1.4e-03
    "blocks.1": 0.015,               # 8.4e-03
    "blocks.1/local": 0.3,           # 1.8e-01
    "blocks.1/bias": 0.02,           # 1.2e-02
    "blocks.2": 0.015,               # 9.5e-03
    "blocks.2/local": 0.5,           # 2.9e-01
    "blocks.2/bias": 0.1,            # 3.0e-02 (bf16 emulation 5.7e-02)
    "blocks.3.tdnn1": 0.006,         # 3.8e-03
    "blocks.3.tdnn1/local": 0.006,   # 3.8e-03
    "blocks.3.tdnn1/bias": 0.006,    # 3.4e-03
    "blocks.3.res2net": 0.006,       # 3.4e-03 (bf16 emulation 3.4e-03)
    "blocks.3.res2net/local": 0.006, # 3.8e-03
    "blocks.3.res2net/bias": 0.006,  # 3.7e-03
    "blocks.3.tdnn2": 0.006,         # 3.5e-03
    "blocks.3.tdnn2/local": 0.006,   # 3.8e-03
    "blocks.3.tdnn2/bias": 0.006,    # 3.5e-03
    "blocks.3.se_gate": 1.2e-05,     # 7.0e-06
    "blocks.3": 0.006,               # 3.7e-03
    "blocks.3/local": 0.006,         # 3.8e-03
    "blocks.3/bias": 0.02,           # 1.3e-02
    "mfa": 0.005,                    # 3.3e-03
    "mfa/local": 0.006,              # 3.8e-03 (bf16 emulation 3.8e-03)
    "mfa/bias": 0.006,               # 3.8e-03
    "asp_gstats": 6e-06,             # 3.5e-06
    "asp_att": 0.003,                # 2.0e-03
    "asp_att/local": 0.006,          # 3.8e-03
    "asp_att/bias": 0.05,            # 2.9e-02
    "asp": 6e-06,                    # 3.4e-06
    "asp_bn": 1.2e-07,               # 7.9e-08
    "emb": 4e-07,                    # 2.6e-07
    "end_to_end": 0.05,              # 2.1e-02 (bf16 emulation 3.1e-02)
}


def bars(compute):
    return {"f32": F32_BARS, "f32x3": F32X3_BARS, "bf16": BF16_BARS}[compute]


def torch_sd(sd_np):
    """the synthetic state dict in float64"""
    return o_ecapa.to_torch_sd(sd_np, torch.float64)


def bf16_round(a):
    """round to bf16 (nearest even) from fp32, as upload_h16 does and the bf16 stores of the kernels do; float64 out"""
    t = torch.as_tensor(a)
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def rounded_sd(sd64, C):
    """the weights a bf16 handle reads: every convolution's weight tensor in bf16 (the SE MLP's two included); the linears kept in
    fp32 (fc, and asp.tdnn's time-constant mean | std columns, which become a per-utterance bias); biases and BN statistics in fp32"""
    out = dict(sd64)
    for k, v in sd64.items():
        if k == "asp.tdnn.conv.conv.weight":
            w = v.clone()
            w[:, :3 * C] = bf16_round(v[:, :3 * C].float())
            out[k] = w
        elif k.endswith("conv.weight") and k != "fc.conv.weight":
            out[k] = bf16_round(v.float())
    return out


def features(mel, sd64, input_norm=False):
    """the network's input (the handle's stage 'input') from the mel power: log, mean over time off, optional instance norm"""
    x = torch.as_tensor(mel).double()
    x = (x + 1e-6).log()
    x = x - x.mean(dim=-1, keepdim=True)
    if input_norm:
        x = F.instance_norm(x, weight=sd64["instance_norm.weight"], bias=sd64["instance_norm.bias"], eps=1e-5)
    return x


def gstats(x, eps=1e-12):
    """(1, C, T) -> (1, 2C): the ASP's global [mean | std] over time (the handle's asp_gstats)"""
    mean = x.mean(dim=2)
    std = torch.sqrt(((x - mean.unsqueeze(2)) ** 2).mean(dim=2).clamp(eps))
    return torch.cat([mean, std], dim=1)


def se_gate(x, sd, p):
    """SEBlock's gate sigmoid(W2 relu(W1 mean_t(x) + b1) + b2), (1, C, T) -> (1, C)"""
    s = x.mean(dim=2, keepdim=True)
    s = F.relu(o_ecapa.conv_same(s, sd, p + ".conv1.conv"))
    return torch.sigmoid(o_ecapa.conv_same(s, sd, p + ".conv2.conv"))[:, :, 0]


def asp_att(x, gs, sd, p="asp"):
    """the attention of AttentiveStatisticsPooling before its last convolution: tanh(BN(relu(conv([x, mean, std])))), given the
    global statistics gs (1, 2C)"""
    C, T = x.shape[1], x.shape[2]
    ctx = gs.unsqueeze(2).expand(1, 2 * C, T)
    return torch.tanh(o_ecapa.tdnn(torch.cat([x, ctx], dim=1), sd, p + ".tdnn", 1, F.relu))


def asp_pool(att, x, sd, p="asp", eps=1e-12):
    """the pooled [mean | std] of x (1, C, T) under softmax_t(conv(att)) (1, 2C)"""
    w = F.softmax(o_ecapa.conv_same(att, sd, p + ".conv.conv"), dim=2)
    mean = (w * x).sum(2)
    std = torch.sqrt((w * (x - mean.unsqueeze(2)) ** 2).sum(2).clamp(eps))
    return torch.cat([mean, std], dim=1)


def rel_err(got, ref):
    """(max |got - ref| / max |ref|, index of the worst element)"""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    i = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d.max()) / max(float(np.abs(ref).max()), 1e-30), tuple(int(v) for v in i)


def nearer_err(got, ref_a, ref_b):
    """rel_err of each element against the nearer of two references"""
    got = np.asarray(got, np.float64)
    d = np.minimum(np.abs(got - ref_a), np.abs(got - ref_b))
    i = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d.max()) / max(float(np.abs(ref_a).max()), 1e-30), tuple(int(v) for v in i)


def local_err(got, ref):
    """(max |got - ref| / (|ref| + max |ref| / 64), worst index): each element against its own size, so that one element wrong
    by a few percent of its value shows above the bf16 rounding of the stored values (<= 2^-8 of each value)"""
    ref = np.asarray(ref, np.float64)
    d = np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + float(np.abs(ref).max()) / 64 + 1e-30)
    i = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d.max()), tuple(int(v) for v in i)


def bias_err(got, ref):
    """(max over channels of |sum_t (got - ref)| / sqrt(T) / max |ref|, (0, channel)) of a (T, channels) stage: an error common to every
    frame of a channel (a bias, a BN shift) that hides under the rounding of the single elements.  Independent roundings add up to
    sqrt(T) of one; a common error to T of it."""
    ref = np.asarray(ref, np.float64)
    m = np.abs((np.asarray(got, np.float64) - ref).sum(axis=0)) / np.sqrt(ref.shape[0])
    c = int(np.argmax(m))
    return float(m[c]) / max(float(np.abs(ref).max()), 1e-30), (0, c)


def where(check, idx):
    """the worst element of a check in words: frame and channel of a (T, channels) stage, channel of a per-utterance vector or bias"""
    if check.split("/")[0] in VECTOR_STAGES + ("emb", "end_to_end"):
        return f"channel {idx[0]}"
    return f"channel {idx[1]}" if check.endswith("/bias") else f"frame {idx[0]} channel {idx[1]}"


def res2net_steps(t1, r2, sd, p, dil, bf16):
    """the Res2Net chain step by step: chunk i from tdnn1's chunk i and the handle's own chunk i - 1 (its operand rounded to bf16 on
    bf16 handles, as the MFMA reads it), so that each step is checked on its own input"""
    xs, ys = torch.chunk(t1, o_ecapa.SCALE, dim=1), torch.chunk(r2, o_ecapa.SCALE, dim=1)
    out = [xs[0]]
    for i in range(1, o_ecapa.SCALE):
        u = xs[i] if i == 1 else xs[i] + ys[i - 1]
        if bf16:
            u = bf16_round(u.float())
        out.append(o_ecapa.tdnn(u, sd, f"{p}.blocks.{i - 1}", dil, F.relu))
    return torch.cat(out, dim=1)


def layer_local(S, b, sd, ref_input=None, emb=None, e2e_ref=None, bf16=False):
    """{check: (error, worst index)} of utterance b.  S: the handle's stages as float64 arrays, (B, T, channels) or (B, n); a stage
    the handle does not produce is None (its successor then starts from the oracle's own value).  sd: the float64 weights the
    handle reads (rounded_sd for bf16 handles).  ref_input: the oracle's features of the utterance (1, n_mels, T); emb, e2e_ref: the
    handle's embedding of the utterance and the oracle's end to end.  A (T, channels) stage has three checks: `name` (max |diff| /
    max |ref|), `name/local` (local_err) and `name/bias` (bias_err).

    The SE squeeze and the ASP statistics are sums over time of tdnn2's / mfa's output.  Some kernels take them from the GEMM
    epilogue's fp32 values before the bf16 store (gemm_pw3's accumulators), others from the stored bf16 values (gemm_pw2's LDS image,
    se_mean, asp_gstats); where a channel barely varies over time, the rounding biases its mean by up to half a unit in the last
    place — as much as one dropped frame.  So each element of se_gate / asp_gstats is held against the nearer of two references:
    from the handle's stored tdnn2 / mfa, and from the oracle's tdnn2 / mfa of the handle's own inputs (the same bf16 operands and
    weights: the epilogue's values but for its fp32 sums).  The two differ by far less than one frame's weight."""
    cm = lambda name: torch.from_numpy(np.ascontiguousarray(S[name][b].T))[None]       # frame-major row b -> (1, channels, T)
    err = {}

    def frame(name, ref):
        got, ref = S[name][b], ref[0].numpy().T if torch.is_tensor(ref) else ref
        err[name], err[name + "/local"], err[name + "/bias"] = rel_err(got, ref), local_err(got, ref), bias_err(got, ref)

    with torch.no_grad():
        if ref_input is not None:
            frame("input", ref_input)
        frame("blocks.0", o_ecapa.tdnn(cm("input"), sd, "blocks.0", 1, o_ecapa.gelu))
        for i in (1, 2):
            frame(f"blocks.{i}", o_ecapa.se_res2net_block(cm(f"blocks.{i - 1}"), sd, f"blocks.{i}", i + 1))
        p = "blocks.3"
        t1 = o_ecapa.tdnn(cm("blocks.2"), sd, p + ".tdnn1", 1, o_ecapa.gelu)
        if S.get(p + ".tdnn1") is not None:
            frame(p + ".tdnn1", t1)
            t1 = cm(p + ".tdnn1")
        frame(p + ".res2net", res2net_steps(t1, cm(p + ".res2net"), sd, p + ".res2net_block", 4, bf16))
        t2 = o_ecapa.tdnn(cm(p + ".res2net"), sd, p + ".tdnn2", 1, o_ecapa.gelu)
        frame(p + ".tdnn2", t2)
        err[p + ".se_gate"] = nearer_err(S[p + ".se_gate"][b], se_gate(cm(p + ".tdnn2"), sd, p + ".se_block")[0].numpy(),
                                         se_gate(t2, sd, p + ".se_block")[0].numpy())
        frame(p, S[p + ".se_gate"][b][None, :] * S[p + ".tdnn2"][b] + S["blocks.2"][b])
        cat = torch.cat([cm("blocks.1"), cm("blocks.2"), cm("blocks.3")], dim=1)
        mfa_ref = o_ecapa.tdnn(cat, sd, "mfa", 1, o_ecapa.gelu)
        frame("mfa", mfa_ref)
        mfa = cm("mfa")
        err["asp_gstats"] = nearer_err(S["asp_gstats"][b], gstats(mfa)[0].numpy(), gstats(mfa_ref)[0].numpy())
        gs = torch.from_numpy(S["asp_gstats"][b])[None]
        frame("asp_att", asp_att(mfa, gs, sd))
        err["asp"] = rel_err(S["asp"][b], asp_pool(cm("asp_att"), mfa, sd)[0].numpy())
        pooled = torch.from_numpy(S["asp"][b])[None, :, None]
        err["asp_bn"] = rel_err(S["asp_bn"][b], o_ecapa.bn(pooled, sd, "asp_bn.norm")[0, :, 0].numpy())
        if emb is not None:
            bn = torch.from_numpy(S["asp_bn"][b])[None, :, None]
            err["emb"] = rel_err(emb, o_ecapa.conv_same(bn, sd, "fc.conv")[0, :, 0].numpy())
    if emb is not None and e2e_ref is not None:
        err["end_to_end"] = rel_err(emb, e2e_ref)
    return err


def failures(err, compute):
    """the checks over their bars: [(check, error, bar, where the worst element sits)]"""
    bar = bars(compute)
    return [(n, e, bar[n], where(n, i)) for n, (e, i) in err.items() if not e <= bar[n]]


def describe(err):
    """one line: every check's error in stage order"""
    return ", ".join(f"{n} {err[n][0]:.2e}" for n in CHECKS if n in err)
