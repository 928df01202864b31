"""RawNet2 against the float64 oracle (oracle/rawnet2.py), block by block and one utterance at a time: the comparisons and bars of
tests/test_gpu_rawnet2_oracle.py.  They need no GPU, so tests/test_rawnet2_oracle_host.py can show on CPU emulations of a 16-bit
handle that every bar fails when the value it guards is subtly wrong.

Layer-local checks.  Option rn_keep makes a forward copy what it stores anyway (svhip_get_stage): the front-end output, per fused
128-channel block its pooled output and its gate, per block of the generic path the pre-activation it reads, its input x where an
identity shortcut reads it, the conv2 + shortcut output o (or conv2 alone, c2, where the tail adds the identity shortcut), the gate
where a kernel stores one, and the next block's x and pre-activation; then the aggregation's input, the attention logits and the
pooled vector (GRU: the last state).  Each is compared with the oracle's step applied in float64 to the handle's OWN stored input.
The error of a check is max |got - ref| / max |ref| over ONE utterance, for (T, channels) tensors also the `/local` form (each
element against its own size) and the `/bias` form (an error common to a channel's frames); a failure names frame and channel.

16-bit handles read 16-bit convolution weights and sinc filters (to_h16: round to nearest even) and keep the folded BN, the
biases, AFMS's fc, the conv front-end's constants and the final linears in fp32: the references read the same (rounded_sd), round
the intermediate tensors the kernels hold in 16 bits (conv1's output; inside a fused block also y and its pre-activation), and take
every reduction before the rounding of its result.  What remains is the rounding of the stored outputs and the fp32 sums.

Reductions over time (AFMS's mean, the attention's softmax and statistics) move by about 1 / T when one frame is dropped — less
than a 16-bit store rounds — so each has a check of its own: `gate` against the stored gate (held to the nearer of two references,
as in tests/ecapa_oracle_check.py: the mean of the stored o, and of the oracle's o before its rounding, which the fused kernels
sum), `pooled` against the stored logits and aggregation input.  Where the one-workgroup tail keeps its gate on chip, `gate_rec`
recovers it per channel by least squares over the frames from the stored o and the stored block output (or, where the block output
is not stored either, from the next pre-activation with LeakyReLU and BN undone).  tests/test_rawnet2_oracle_host.py asserts that
these bars sit 4x below the effect of one dropped frame at every length the GPU file runs."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import rawnet2 as o_rn
from tests.ecapa_oracle_check import bias_err, local_err, nearer_err, rel_err

# (prefix, cin, cout, downsample) of the eight residual blocks (RawNet2_custom.py:230-243)
BLOCKS = (("layer1.0", 128, 128, True), ("layer2.0", 128, 128, True), ("layer3.0", 128, 256, True), ("layer4.0", 256, 256, False),
          ("layer4.1", 256, 256, True), ("layer5.0", 256, 512, True), ("layer6.0", 512, 512, False), ("layer6.1", 512, 512, True))
COMPUTES = ("f32", "f32x3", "f16", "bf16")
FRAME_KINDS = ("front", "pool", "o", "x", "pre", "logits")            # (T, channels) checks: also /local and /bias
VECTOR_KINDS = ("gate", "gate_rec", "pooled", "gru_h", "emb", "end_to_end")
REDUCTIONS = ("gate", "gate_rec", "pooled")


def frames_after(T1):
    """(frames entering, frames leaving) each block, from the front-end's T1"""
    out, T = [], T1
    for _, _, _, down in BLOCKS:
        out.append((T, T // 3 if down else T))
        T = out[-1][1]
    return out


def front_frames(L, model):
    return (L - 3) // 3 + 1 if model == "rawnet2_conv" else (L - 250) // 3


# The bars, by compute and kind of check (a block check `b<i>.<kind>` takes the bar of its kind): the largest error measured over every
# case of tests/test_gpu_rawnet2_oracle.py (beside each bar; for the 16-bit computes also the clean emulation of
# tests/test_rawnet2_oracle_host.py where it is larger), times about 1.5.
BARS = {
    "f32": {
        "front":         5e-06   ,      # 3.1e-06
        "front/local":   0.00012 ,      # 7.9e-05
        "front/bias":    6e-05   ,      # 3.6e-05
        "o":             2.5e-06 ,      # 1.4e-06
        "o/local":       8e-05   ,      # 4.9e-05
        "o/bias":        1e-05   ,      # 5.7e-06
        "gate":          5e-06   ,      # 2.7e-06
        "gate_rec":      3e-06   ,      # 1.8e-06
        "x":             2.5e-06 ,      # 1.4e-06
        "x/local":       8e-06   ,      # 4.4e-06
        "x/bias":        1.5e-05 ,      # 8.4e-06
        "pre":           2.5e-06 ,      # 1.4e-06
        "pre/local":     6.5e-06 ,      # 4.0e-06
        "pre/bias":      1e-05   ,      # 6.4e-06
        "logits":        1.5e-06 ,      # 9.3e-07
        "logits/local":  5e-05   ,      # 3.3e-05
        "logits/bias":   1.5e-06 ,      # 9.3e-07
        "pooled":        4e-07   ,      # 2.5e-07
        "gru_h":         2.5e-06 ,      # 1.6e-06
        "emb":           2.5e-07 ,      # 1.6e-07
        "end_to_end":    3e-05   ,      # 2.0e-05
    },
    "f32x3": {
        "front":         5e-06   ,      # 2.7e-06
        "front/local":   0.00012 ,      # 7.8e-05
        "front/bias":    6e-05   ,      # 3.5e-05
        "o":             2e-06   ,      # 1.0e-06
        "o/local":       8e-05   ,      # 4.6e-05
        "o/bias":        2e-05   ,      # 1.3e-05
        "gate":          3.5e-06 ,      # 2.3e-06
        "gate_rec":      4e-06   ,      # 2.4e-06
        "x":             2.5e-06 ,      # 1.7e-06
        "x/local":       8e-06   ,      # 5.0e-06
        "x/bias":        1e-05   ,      # 6.4e-06
        "pre":           2e-06   ,      # 1.3e-06
        "pre/local":     8e-06   ,      # 4.8e-06
        "pre/bias":      1.5e-05 ,      # 8.9e-06
        "logits":        1e-06   ,      # 6.4e-07
        "logits/local":  5e-05   ,      # 2.7e-05
        "logits/bias":   3e-06   ,      # 1.8e-06
        "pooled":        3e-07   ,      # 1.9e-07
        "gru_h":         8e-06   ,      # 4.9e-06
        "emb":           3e-07   ,      # 2.0e-07
        "end_to_end":    6e-05   ,      # 3.8e-05
    },
    "f16": {
        "front":         0.001   ,      # 5.6e-04
        "front/local":   0.02    ,      # 1.1e-02
        "front/bias":    0.002   ,      # 1.2e-03
        "pool":          0.001   ,      # 6.5e-04
        "pool/local":    0.0065  ,      # 4.1e-03
        "pool/bias":     0.001   ,      # 5.8e-04
        "o":             0.001   ,      # 5.9e-04
        "o/local":       0.012   ,      # 7.7e-03
        "o/bias":        0.001   ,      # 5.5e-04
        "gate":          8e-06   ,      # 4.4e-06
        "gate_rec":      0.0012  ,      # 6.7e-04
        "x":             0.0008  ,      # 4.6e-04
        "x/local":       0.0008  ,      # 4.8e-04
        "x/bias":        0.012   ,      # 7.3e-03
        "pre":           0.0012  ,      # 7.6e-04
        "pre/local":     0.003   ,      # 1.8e-03
        "pre/bias":      0.012   ,      # 6.7e-03
        "logits":        0.00025 ,      # 1.4e-04
        "logits/local":  0.01    ,      # 6.2e-03
        "logits/bias":   2.5e-05 ,      # 1.5e-05
        "pooled":        4e-07   ,      # 2.5e-07
        "gru_h":         1.2e-06 ,      # 7.9e-07
        "emb":           3.5e-07 ,      # 2.3e-07
        "end_to_end":    0.065   ,      # 4.2e-02
    },
    "bf16": {
        "front":         0.006   ,      # 3.6e-03
        "front/local":   0.035   ,      # 2.3e-02
        "front/bias":    0.006   ,      # 3.6e-03
        "pool":          0.006   ,      # 3.6e-03
        "pool/local":    0.025   ,      # 1.4e-02
        "pool/bias":     0.005   ,      # 3.0e-03
        "o":             0.008   ,      # 5.1e-03
        "o/local":       0.15    ,      # 8.3e-02
        "o/bias":        0.008   ,      # 4.6e-03
        "gate":          6e-06   ,      # 3.5e-06
        "gate_rec":      0.009   ,      # 5.8e-03
        "x":             0.006   ,      # 3.5e-03
        "x/local":       0.006   ,      # 3.8e-03
        "x/bias":        0.08    ,      # 5.2e-02
        "pre":           0.01    ,      # 5.9e-03
        "pre/local":     0.025   ,      # 1.4e-02
        "pre/bias":      0.1     ,      # 6.3e-02
        "logits":        3e-06   ,      # 1.8e-06
        "logits/local":  0.0001  ,      # 6.0e-05
        "logits/bias":   5e-07   ,      # 3.2e-07
        "pooled":        6.5e-07 ,      # 4.1e-07
        "gru_h":         1e-06   ,      # 5.5e-07
        "emb":           3e-07   ,      # 2.0e-07
        "end_to_end":    0.3     ,      # 1.9e-01
    },
}



def kind_of(check):
    return check.split(".", 1)[1] if check[0] == "b" and check[1].isdigit() else check


def bar(compute, check):
    return BARS[compute][kind_of(check)]


def rounder(compute):
    """what a store in the handle's activation type does to a float64 tensor"""
    if compute in ("f32", "f32x3"):
        return lambda t: t
    dt = torch.bfloat16 if compute == "bf16" else torch.float16
    return lambda t: t.to(torch.float32).to(dt).to(torch.float64)


def torch_sd(sd_np):
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd_np.items()}


def rounded_sd(sd64, compute):
    """the weights a handle of this compute reads: on 16-bit handles every convolution weight (the blocks' conv1 / conv2 / shortcut, the
    attention's two 1 x 1 layers, the GRU's W_ih and W_hh) in the 16-bit type; the folded BN, biases, AFMS's fc and alpha, the conv
    front-end's constants, fc and fc_after_gru in fp32.  (The sinc filters are rounded where they are built: front().)"""
    rnd = rounder(compute)
    out = dict(sd64)
    for k, v in sd64.items():
        if (k.startswith("layer") and k.endswith(("conv1.weight", "conv2.weight", "shortcut.0.weight"))) or \
                k in ("attention.0.weight", "attention.3.weight", "gru.weight_ih_l0", "gru.weight_hh_l0"):
            out[k] = rnd(v)
    return out


def lrelu(x):
    return F.leaky_relu(x, 0.3)


# ---- the oracle's steps, (1, C, T) float64 tensors.  `mut`: the deliberate errors of tests/test_rawnet2_oracle_host.py (the references
# of the checks never pass one) ----------------------------------------------------------------------------------------------------
def front(wav, sd, model, rnd, mut=()):
    """waveform (1, L) -> the front-end output (1, 128, T1)"""
    if model == "rawnet2_conv":
        return o_rn.front_conv(wav, sd)
    xn = rnd(o_rn.layer_norm(wav, sd))
    filt = rnd(o_rn.sinc_filters(sd["first_conv.low_hz_"], sd["first_conv.band_hz_"]))
    return o_rn.front_sinc(xn, sd, filt)


def conv3(x, w, mut=(), other=None):
    """k = 3, padding 1.  halo_zero: the frame in front of the seam at frame 78 read as zero by the frame behind it; halo_neighbour: the
    last frame's right halo read from `other`'s first frame"""
    y = F.conv1d(x, w, padding=1)
    if "halo_zero" in mut and x.shape[2] > 80:
        xz = x.clone()
        xz[:, :, 77] = 0
        y[:, :, 78] = F.conv1d(xz, w, padding=1)[:, :, 78]
    if "halo_neighbour" in mut:
        xx = torch.cat([x, other[:, :, :1]], dim=2)
        y[:, :, -1] = F.conv1d(xx, w, padding=1)[:, :, -2]
    return y


def block_convs(pre, x, sd, p, rnd, mut=(), other=None):
    """(conv2's output, the shortcut) of a block from its pre-activation and its input: conv1 -> bn2 -> LeakyReLU (stored in the
    activation type) -> conv2; the shortcut is x, or the 1 x 1 projection of the pre-activation"""
    h = o_rn.bn(conv3(pre, sd[p + ".conv1.weight"], mut, other), sd, p + ".bn2")
    if "bn_slab" in mut:          # channels 32 .. 63 without bn2's shift
        scale = sd[p + ".bn2.weight"] / torch.sqrt(sd[p + ".bn2.running_var"] + 1e-5)
        h[:, 32:64] -= (sd[p + ".bn2.bias"] - sd[p + ".bn2.running_mean"] * scale)[None, 32:64, None]
    c2 = F.conv1d(rnd(lrelu(h)), sd[p + ".conv2.weight"], padding=1)
    if (p + ".shortcut.0.weight") in sd:
        return c2, F.conv1d(pre, sd[p + ".shortcut.0.weight"])
    return c2, (pre if "shortcut_pre" in mut else x)


def pool3(o, mut=()):
    """max_pool1d(3); pool_shift: every window one frame late (the same count when T % 3 != 0)"""
    if "pool_shift" in mut and o.shape[2] % 3:
        return F.max_pool1d(o[:, :, 1:], 3)
    return F.max_pool1d(o, 3)


def gate_of(y, sd, p, mut=(), T_unpooled=None):
    """AFMS's gate sigmoid(fc(mean_t y)), (1, C, Tn) -> (1, C).  mean_short: the mean over Tn - 1 frames; mean_T: the sum over the pooled
    frames divided by the un-pooled length"""
    m = y.mean(dim=2)
    if "mean_short" in mut:
        m = y[:, :, :-1].sum(dim=2) / max(y.shape[2] - 1, 1)
    if "mean_T" in mut and T_unpooled:
        m = y.sum(dim=2) / T_unpooled
    return torch.sigmoid(F.linear(m, sd[p + ".afms.fc.weight"], sd[p + ".afms.fc.bias"]))


def afms_apply(y, g, sd, p):
    return (y + sd[p + ".afms.alpha"]) * g[:, :, None]


def next_bn(i):
    return f"{BLOCKS[i + 1][0]}.bn1" if i < 7 else None       # (None: the aggregation's BN, whose name follows the model)


def agg_bn(model):
    return "bn_before_gru" if model == "rawnet2_gru" else "bn_before_agg"


def logits_of(x, sd, rnd):
    a = F.conv1d(x, sd["attention.0.weight"], sd["attention.0.bias"])
    a = rnd(o_rn.bn(F.leaky_relu(a, 0.01), sd, "attention.2"))
    return F.conv1d(a, sd["attention.3.weight"], sd["attention.3.bias"])


def pooled_of(a, x, mut=()):
    """(1, 512, T) logits and aggregation input -> (1, 1024) [mean | std].  softmax_short: the softmax over T - 1 frames; no_clamp: the
    variance not clamped at 1e-5"""
    if "softmax_short" in mut and a.shape[2] > 1:
        a, x = a[:, :, :-1], x[:, :, :-1]
    w = F.softmax(a, dim=-1)
    m = torch.sum(x * w, dim=-1)
    v = torch.sum((x ** 2) * w, dim=-1) - m ** 2
    s = torch.sqrt(v.clamp(min=0.0) if "no_clamp" in mut else v.clamp(min=1e-5))
    return torch.cat([m, s], dim=1)


def gru_h_of(x, sd):
    """the float64 GRU of tests/test_rawnet2_gru_host.py on (1, 512, T) -> (1, 1024)"""
    from tests.test_rawnet2_gru_host import gru_f64
    return torch.from_numpy(gru_f64(x[0].numpy().T[None], {k: sd[k].numpy() for k in sd if k.startswith("gru.")}))


def recovered_gate(y, sd, p, x_next=None, pre_next=None, bn_next=None):
    """the gate a tail applied, per channel by least squares over the frames: x = (y + alpha) g, read from the stored block output, or
    from the stored next pre-activation lrelu(scale x + shift) with the LeakyReLU and the BN undone.  (1, C)"""
    pa = y + sd[p + ".afms.alpha"]
    if x_next is None:
        scale = sd[bn_next + ".weight"] / torch.sqrt(sd[bn_next + ".running_var"] + 1e-5)
        shift = sd[bn_next + ".bias"] - sd[bn_next + ".running_mean"] * scale
        z = torch.where(pre_next >= 0, pre_next, pre_next / 0.3)
        x_next = (z - shift[None, :, None]) / scale[None, :, None]
    return (x_next * pa).sum(dim=2) / (pa * pa).sum(dim=2).clamp(min=1e-30)


# ---- the checks --------------------------------------------------------------------------------------------------------------
def layer_local(S, b, sd, wav, model, compute, emb=None, e2e_ref=None):
    """{check: (error, worst index)} of utterance b.  S: the handle's kept stages as float64 arrays (B, T, channels) or (B, n), without
    the `rn_` prefix; a stage the route did not store is absent.  sd: the float64 weights the handle reads (rounded_sd).  wav: the
    utterance's waveform (L,); emb / e2e_ref: the handle's embedding and the oracle's, end to end."""
    rnd = rounder(compute)
    cm = lambda name: torch.from_numpy(np.ascontiguousarray(S[name][b].T))[None]      # frame-major row b -> (1, channels, T)
    vec = lambda name: torch.from_numpy(np.ascontiguousarray(S[name][b]))[None]
    err = {}

    def frame(check, got_name, ref):
        got, ref = S[got_name][b], ref[0].numpy().T
        assert got.shape == ref.shape, (check, got.shape, ref.shape)
        err[check], err[check + "/local"], err[check + "/bias"] = rel_err(got, ref), local_err(got, ref), bias_err(got, ref)

    with torch.no_grad():
        x0 = front(torch.from_numpy(np.asarray(wav, np.float64))[None], sd, model, rnd)
        if "front" in S:
            frame("front", "front", x0)
            x0 = cm("front")
        else:
            x0 = rnd(x0)           # (block 0 of the conv-fused chain forms it on chip, in the activation type)
        xin, gprev = x0, None      # a fused block's input and the gate (with its alpha) still to be applied to it
        for i, (p, cin, cout, down) in enumerate(BLOCKS):
            nbn = next_bn(i) or agg_bn(model)
            nx, npre = f"b{i + 1}_x", (f"b{i + 1}_pre" if i < 7 else "agg_in")
            if f"b{i}_pool" in S:                                                     # one fused kernel: the pooled output and its gate
                y = xin if gprev is None else rnd(afms_apply(xin, gprev[0], sd, gprev[1]))
                c2, sc = block_convs(rnd(lrelu(o_rn.bn(y, sd, p + ".bn1"))), y, sd, p, rnd)
                ref = pool3(c2 + sc)
                frame(f"b{i}.pool", f"b{i}_pool", ref)
                yp = cm(f"b{i}_pool")
                err[f"b{i}.gate"] = nearer_err(S[f"b{i}_gate"][b], gate_of(yp, sd, p)[0].numpy(), gate_of(ref, sd, p)[0].numpy())
                xin, gprev = yp, (vec(f"b{i}_gate"), p)
                if npre not in S:
                    continue           # the next block is fused too and applies this gate on its way in
                xr = afms_apply(yp, gprev[0], sd, p)
            else:
                if i == 0:
                    frame("b0.pre", "b0_pre", lrelu(o_rn.bn(x0, sd, p + ".bn1")))
                pre = cm(f"b{i}_pre")
                xi = None if cin != cout else (x0 if i == 0 else cm(f"b{i}_x"))
                c2, sc = block_convs(pre, xi, sd, p, rnd)
                in_tail = f"b{i}_c2" in S                                              # conv2 alone: the tail adds the identity shortcut
                name = f"b{i}_c2" if in_tail else f"b{i}_o"
                T_in = pre.shape[2]
                by_conv = down and S[name].shape[1] == T_in // 3 and T_in >= 3         # conv2 pooled on its way out
                ref_o = c2 if in_tail else c2 + sc
                frame(f"b{i}.o", name, pool3(ref_o) if by_conv else ref_o)
                o_st = rnd(cm(name) + xi) if in_tail else cm(name)                     # (the tail holds the sum in the activation type)
                yp = pool3(o_st) if down and not by_conv else o_st
                yr = pool3(c2 + sc) if down else c2 + sc
                g_ref = gate_of(yp, sd, p)
                if f"b{i}_gate" in S:
                    err[f"b{i}.gate"] = nearer_err(S[f"b{i}_gate"][b], g_ref[0].numpy(), gate_of(yr, sd, p)[0].numpy())
                    g = vec(f"b{i}_gate")
                else:
                    if yp.shape[2] >= 2:       # (one frame: one equation per channel, which returns that element's own rounding)
                        rec = recovered_gate(yp, sd, p, cm(nx) if nx in S else None, cm(npre) if nx not in S else None, nbn)
                        err[f"b{i}.gate_rec"] = rel_err(rec[0].numpy(), g_ref[0].numpy())
                    g = g_ref
                xr = afms_apply(yp, g, sd, p)
            if nx in S:
                frame(f"b{i}.x", nx, xr)
            frame(f"b{i}.pre", npre, lrelu(o_rn.bn(xr, sd, nbn)))
        agg = cm("agg_in")
        if model == "rawnet2_gru":
            err["gru_h"] = rel_err(S["gru_h"][b], gru_h_of(agg, sd)[0].numpy())
            if emb is not None:
                err["emb"] = rel_err(emb, F.linear(vec("gru_h"), sd["fc_after_gru.weight"], sd["fc_after_gru.bias"])[0].numpy())
        else:
            frame("logits", "logits", logits_of(agg, sd, rnd))
            err["pooled"] = rel_err(S["pooled"][b], pooled_of(cm("logits"), agg)[0].numpy())
            if emb is not None:
                err["emb"] = rel_err(emb, F.linear(vec("pooled"), sd["fc.weight"], sd["fc.bias"])[0].numpy())
    if emb is not None and e2e_ref is not None:
        err["end_to_end"] = rel_err(emb, e2e_ref)
    return err


def where(check, idx):
    """the worst element of a check in words"""
    k = kind_of(check)
    if k in VECTOR_KINDS:
        return f"channel {idx[0]}"
    return f"channel {idx[1]}" if k.endswith("/bias") else f"frame {idx[0]} channel {idx[1]}"


def failures(err, compute):
    """the checks over their bars: [(check, error, bar, where the worst element sits)]"""
    return [(n, e, bar(compute, n), where(n, i)) for n, (e, i) in err.items() if not e <= bar(compute, n)]


def describe(err):
    return ", ".join(f"{n} {e:.2e}" for n, (e, _) in err.items())


def by_kind(err, into=None):
    """the largest error of each kind of check"""
    into = {} if into is None else into
    for n, (e, _) in err.items():
        into[kind_of(n)] = max(into.get(kind_of(n), 0.0), e)
    return into


def end_to_end(wav, sd64, model):
    """the oracle's embedding of one utterance from the full-precision weights"""
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(wav, np.float64))[None]
        if model != "rawnet2_gru":
            return o_rn.rawnet2_forward(x, sd64, front_proc="conv" if model == "rawnet2_conv" else "sinc").reshape(-1).numpy()
        h = lrelu(o_rn.bn(_trunk(x, sd64), sd64, "bn_before_gru"))
        return F.linear(gru_h_of(h, sd64), sd64["fc_after_gru.weight"], sd64["fc_after_gru.bias"]).reshape(-1).numpy()


def _trunk(x, sd):
    x = o_rn.front_sinc(o_rn.layer_norm(x, sd), sd)
    for li, nblk in enumerate(o_rn.LAYERS, start=1):
        for b in range(nblk):
            x = o_rn.basic_block(x, sd, f"layer{li}.{b}", downsample=(b == nblk - 1))
    return x
