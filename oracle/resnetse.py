"""Oracle (TEST INFRASTRUCTURE) — functional restatement of the reference ResNetSE34V2, as steps.

Follows reference ``src/models/ResNetSE34V2.py``, ``ResNetBaseline.py:141-301`` and ``ResNetBlocks.py:211-246,292-307``: the input
normalisation (log, mean over time off, InstanceNorm1d without affine), the stem (Conv2d(1, 32, 3) with bias -> ReLU -> BatchNorm, in
that order), sixteen SEBasicBlockV2 in four stages (the block's opening ReLU is in place, so the identity residual is relu(x);
conv3x3 + BN + ReLU, conv3x3 + BN, the SE gate with biases, a 1 x 1 stride-2 downsample + BN on the first block of stages 2 - 4,
relu(residual + gate * v)), the attention over frames on the flattened (C Q) rows (Conv1d -> ReLU -> BN -> Conv1d -> softmax), the
weighted mean and sqrt(clamp(weighted variance, 1e-5)) ('SAP': the mean alone) and fc.  Plain torch; pinned against the reference's
float64 outputs and stage checksums through ``tests/test_resnetse_host.py::ref64``, which wraps ``forward``.

Every step works on ONE utterance in the layout the library stores: an image is (P, Q, C) — P frames, Q mel rows, channels last — and a
reference weight (Cout, Cin, kh, kw) has kh over mel rows and kw over frames.  The attention rows are taken in the REFERENCE's column
order c Q + q (``flat``); the library keeps q C + c and permutes its weights instead, so a check brings a handle's att input, logits
and pooled vector into this order first (``ref_cols``).  A step takes its input tensor and the state dict and computes in the dtype
of both (float64 for the oracle; float32 for a CPU emulation of a handle).  ``store`` is applied to every tensor a handle keeps in its
storage type: the identity for the oracle, a rounding to bf16 for the emulation of a bf16 handle.

The state dict comes in two forms.  The checkpoint's own, where a step takes each BatchNorm as scale / shift in the dtype of the dict;
and the form of ``folded_sd`` / ``rounded_sd``, which holds the numbers a handle reads: every BatchNorm as an fp32 ``.scale`` /
``.shift`` pair folded in double, on a bf16 handle the weights of the MFMA convolutions and of the two attention convolutions rounded to
bf16 (the stem, the SE layers, every bias and fc stay fp32).

Multiply-adds the kernels do in one rounding (the stem's taps, every BatchNorm epilogue, the block tail) go through oracle.titanet's
``_fma``; the convolutions through ``_conv``, which ``conv_as(chained_conv(ck, kstep))`` replaces by the kernel's order of sums; the
two attention GEMMs through oracle.conformer's ``_mm``.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from oracle.conformer import _mm, bf16_round, chained_matmul, ident, matmul_as, to_torch_sd  # noqa: F401  (shared, unchanged)
from oracle.titanet import _bn_affine, _fma

BLOCK_STEPS = ("conv1", "conv2", "part", "gate", "down", "out")        # the handle's stages rs_b<i>_<step> (option rs_keep)
ATT = 128
HALO_MAX, ROWB = 56 * 1024, 64                                         # resnetse.hip: RS_HALO_MAX, RS_ROWB


def block_names(sd):
    """the prefixes "layer<s>.<j>." of the blocks in forward order"""
    out = []
    for s in range(1, 5):
        j = 0
        while f"layer{s}.{j}.conv1.weight" in sd:
            out.append(f"layer{s}.{j}.")
            j += 1
    return out


def has_down(sd, p):
    return p + "downsample.0.weight" in sd


def bn_names(sd):
    out = ["bn1"]
    for p in block_names(sd):
        out += [p + "bn1", p + "bn2"] + ([p + "downsample.1"] if has_down(sd, p) else [])
    return out + ["attention.2"]


def is_mfma_weight(k):
    """the tensors a bf16 handle reads in bf16: the block convolutions, the downsamples and the two attention convolutions"""
    return k.startswith("layer") and (k.endswith("conv1.weight") or k.endswith("conv2.weight") or k.endswith("downsample.0.weight")) or \
        k in ("attention.0.weight", "attention.3.weight")


def folded_sd(sd, bf16=False):
    """the numbers a handle reads, in the dtype of sd: every BatchNorm folded in double to scale / shift and cast to fp32 (make_bn), every
    other tensor as it is; bf16: the MFMA weights (is_mfma_weight) rounded to bf16"""
    some = next(v for v in sd.values() if torch.is_floating_point(v))
    d64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}
    bns = bn_names(d64)
    out = {}
    for p in bns:
        s, t = _bn_affine(d64, p)
        out[p + ".scale"], out[p + ".shift"] = s.float().double(), t.float().double()
    for k, v in d64.items():
        if torch.is_floating_point(v) and k.rsplit(".", 1)[0] not in bns:
            out[k] = bf16_round(v) if bf16 and is_mfma_weight(k) else v
    return {k: v.to(some.dtype) for k, v in out.items()}


def rounded_sd(sd):
    """the weights a bf16 handle reads (folded_sd, bf16), in the dtype of sd"""
    return folded_sd(sd, bf16=True)


# ---- the convolution -------------------------------------------------------------------------------------------------------------------
def out_size(n, stride):
    return (n - 1) // stride + 1


def taps_of(x, ks, stride):
    """[(tap = ks dp + dq, the (Po, Qo, Cin) operand of that tap)] of a ks x ks convolution with zero padding ks // 2 on the (P, Q, Cin)
    image x: tap (dp, dq) reads position (stride p + dp - pad, stride q + dq - pad)"""
    pad = ks // 2
    P, Q, _ = x.shape
    Po, Qo = out_size(P, stride), out_size(Q, stride)
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    return [(ks * dp + dq, xp[dp:dp + stride * (Po - 1) + 1:stride, dq:dq + stride * (Qo - 1) + 1:stride]) for dp in range(ks) for dq in range(ks)]


def conv_direct(x, w, stride):
    """(P, Q, Cin) x (Cout, Cin, ks, ks) -> (Po, Qo, Cout): torch's conv2d on the image as the reference holds it, (1, Cin, Q, P)"""
    return F.conv2d(x.permute(2, 1, 0)[None], w, stride=stride, padding=w.shape[-1] // 2)[0].permute(2, 1, 0)


def chained_conv(ck, kstep):
    """the same numbers as rs_conv_kernel adds them up: one accumulator per output in the dtype of the operands, the input channels in
    chunks of ck outermost, then the taps in the order ks dp + dq, the products of a tap `kstep` at a time (one MFMA)"""
    def conv(x, w, stride):
        ks = w.shape[-1]
        taps = taps_of(x, ks, stride)
        Po, Qo = taps[0][1].shape[:2]
        ops = [t.reshape(Po * Qo, -1).contiguous() for _, t in taps]
        wt = [w[:, :, t % ks, t // ks].T.contiguous() for t, _ in taps]          # (Cin, Cout): tap (dp, dq) is the element [dq][dp]
        acc = x.new_zeros(Po * Qo, w.shape[0])
        for c0 in range(0, x.shape[2], ck):
            for a, b in zip(ops, wt):
                for k in range(c0, c0 + ck, kstep):
                    acc.addmm_(a[:, k:k + kstep], b[k:k + kstep])
        return acc.reshape(Po, Qo, -1)
    return conv


_CONV = [conv_direct]


def _conv(x, w, stride):
    return _CONV[0](x, w, stride)


@contextlib.contextmanager
def conv_as(fn):
    old, _CONV[0] = _CONV[0], fn
    try:
        yield
    finally:
        _CONV[0] = old


def _conv_bn(x, sd, conv, bn, stride, relu_out):
    s, t = _bn_affine(sd, bn)
    acc = _conv(torch.relu(x), sd[conv + ".weight"], stride)
    y = _fma(acc, s.expand_as(acc), t.expand_as(acc))
    return torch.relu(y) if relu_out else y


# ---- the tiles of the SE sums ----------------------------------------------------------------------------------------------------------
def tile_of(Po, Qo, stride=1, ks=3):
    """(TP, TQ): rs_tile_of (resnetse.hip) restated — the tile of at most 128 positions with the most MFMA rows that carry an output,
    then the fewest halo positions per output; IEEE doubles in the same order, so the choice is the kernel's on every image"""
    best, TP, TQ = -1.0, 1, 1
    for tq in range(1, min(32, Qo) + 1):
        tp = min(128 // tq, Po)
        halo = ((tp - 1) * stride + ks) * ((tq - 1) * stride + ks)
        if halo * ROWB > HALO_MAX:
            continue
        cover = float(-(-Po // tp) * tp) * float(-(-Qo // tq) * tq)
        score = ((float(Po) * Qo) / cover) * (tp * tq / 128.0) - 0.01 * float(halo) / (float(tp) * tq * stride * stride)
        if score > best:
            best, TP, TQ = score, tp, tq
    return TP, TQ


def tile_grid(Po, Qo, stride=1, ks=3):
    """(TP, TQ, ntp, ntq)"""
    TP, TQ = tile_of(Po, Qo, stride, ks)
    return TP, TQ, -(-Po // TP), -(-Qo // TQ)


def tile_sums(v, kernel_order=False):
    """(ntp ntq, C): the sum of v (P, Q, C) over each tile's positions inside the image, tiles in the order tp_i ntq + tq_i.
    kernel_order: added as rs_conv_kernel's epilogue does — tile row m = tp TQ + tq belongs to wave m // 32; a lane adds its sixteen rows
    (r & 3) + 8 (r >> 2) + 4 fh in the order of r, the two half-waves fh are added, then the four waves ((w0 + w1) + w2) + w3"""
    P, Q, C = v.shape
    TP, TQ, ntp, ntq = tile_grid(P, Q)
    vp = F.pad(v, (0, 0, 0, ntq * TQ - Q, 0, ntp * TP - P))
    t = vp.reshape(ntp, TP, ntq, TQ, C).permute(0, 2, 1, 3, 4).reshape(ntp * ntq, TP * TQ, C)
    if not kernel_order:
        return t.sum(dim=1)
    t = F.pad(t, (0, 0, 0, 128 - TP * TQ)).reshape(-1, 4, 4, 2, 4, C)          # m = 32 wave + 8 a + 4 fh + b, r = 4 a + b
    lane = t.new_zeros(t.shape[0], 4, 2, C)
    for a in range(4):
        for b in range(4):
            lane = lane + t[:, :, a, :, b]
    w = lane[:, :, 0] + lane[:, :, 1]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def squeeze(v):
    """the SE squeeze: the mean of v (P, Q, C) over the image"""
    return v.mean(dim=(0, 1))


def squeeze_tiles(part, positions):
    """the squeeze as rs_se_gate takes it from the tile sums: added in tile order, times the fp32 reciprocal of the positions"""
    s = torch.zeros_like(part[0])
    for t in range(part.shape[0]):
        s = s + part[t]
    if part.dtype == torch.float32:
        return s * (torch.ones((), dtype=torch.float32) / torch.tensor(float(positions), dtype=torch.float32))
    return s / positions


# ---- the steps -------------------------------------------------------------------------------------------------------------------------
def _lane_sum(v):
    """the sum over the last axis as prologue_stats_row takes it: lane l of a wave adds t = l, l + 64, ... in order, then the 64 lanes
    are added pairwise"""
    T = v.shape[-1]
    lanes = torch.zeros(*v.shape[:-1], 64, dtype=v.dtype)
    for t0 in range(0, T, 64):
        n = min(64, T - t0)
        lanes[..., :n] = lanes[..., :n] + v[..., t0:t0 + n]
    w = 32
    while w:
        lanes = lanes[..., :w] + lanes[..., w:2 * w]
        w //= 2
    return lanes[..., 0]


def prologue(mel, log_input=True, kernel_form=False):
    """(n_mels, T) mel power -> (T, n_mels): log(x + 1e-6) and its mean over time off (features 'melspectrogram'), then InstanceNorm1d
    without affine (biased variance, eps 1e-5): the handle's rs_xin.  kernel_form: as prologue_stats_row / prologue_apply_tile
    (fbank.hip) compute it — ONE centring (the mean of the centred row is taken as zero, where the reference subtracts it once more),
    the variance about that mean, then (v - mean) * (1 / sqrt(var + eps)); the same numbers in exact arithmetic"""
    x = mel
    if kernel_form:
        v = torch.log(x + 1e-6) if log_input else x
        T = v.shape[-1]
        mean = _lane_sum(v) / T
        d = v - mean[:, None]
        scale = 1.0 / torch.sqrt(_lane_sum(d * d) / T + 1e-5)
        return (d * scale[:, None]).T.contiguous()
    if log_input:
        x = torch.log(x + 1e-6)
        x = x - x.mean(dim=-1, keepdim=True)
    x = (x - x.mean(dim=-1, keepdim=True)) / torch.sqrt(x.var(dim=-1, unbiased=False, keepdim=True) + 1e-5)
    return x.T.contiguous()


def stem(xin, sd, store=ident, order="relu_bn"):
    """(P, Q) -> (P, Q, 32): conv1 + bias as a chain of multiply-adds from the bias over the taps 3 dp + dq, ReLU, then bn1
    (ResNetBaseline.py:260-262).  order "bn_relu": the other order, a fault the host test injects"""
    w, b = sd["conv1.weight"], sd["conv1.bias"]
    s, t = _bn_affine(sd, "bn1")
    taps = taps_of(xin[:, :, None], 3, 1)
    a = b.expand(*xin.shape, -1)
    for tap, op in taps:
        a = _fma(w[:, 0, tap % 3, tap // 3].expand_as(a), op.expand_as(a), a)
    if order == "bn_relu":
        return store(torch.relu(_fma(a, s.expand_as(a), t.expand_as(a))))
    a = torch.relu(a)
    return store(_fma(a, s.expand_as(a), t.expand_as(a)))


def stride_of(sd, p):
    return 2 if has_down(sd, p) else 1


def conv1(x, sd, p, store=ident):
    """relu(bn1(conv3x3(relu(x)))), stride 2 in the first block of stages 2 - 4"""
    return store(_conv_bn(x, sd, p + "conv1", p + "bn1", stride_of(sd, p), True))


def conv2(u, sd, p, store=ident):
    """bn2(conv3x3(u)) (u is non-negative: the kernel applies no ReLU to it, and none changes it)"""
    return store(_conv_bn(u, sd, p + "conv2", p + "bn2", 1, False))


def gate(m, sd, p):
    """sigmoid(W2 relu(W1 m + b1) + b2): the SE excitation (ResNetBlocks.py:303-307)"""
    hid = torch.relu(m @ sd[p + "se.fc.0.weight"].T + sd[p + "se.fc.0.bias"])
    return torch.sigmoid(hid @ sd[p + "se.fc.2.weight"].T + sd[p + "se.fc.2.bias"])


def down(x, sd, p, store=ident):
    """bn(conv1x1 stride 2 (relu(x))): the downsample of the block's input, which the in-place ReLU has already overwritten"""
    return store(_conv_bn(x, sd, p + "downsample.0", p + "downsample.1", 2, False))


def out(v, g, res, store=ident, res_relu=True):
    """relu(res + g v); res_relu: res is the block's input x and the residual relu(x) (the identity residual)"""
    r = torch.relu(res) if res_relu else res
    return store(torch.relu(_fma(v, g.expand_as(v), r)))


def flat(x):
    """(P, Q, C) -> (P, C Q): the rows of the attention in the reference's column order c Q + q"""
    return x.permute(0, 2, 1).reshape(x.shape[0], -1)


def ref_cols(a, C=256):
    """a handle's (rows, Q C) columns q C + c -> the reference's c Q + q (numpy or torch)"""
    return a.reshape(a.shape[0], -1, C).swapaxes(1, 2).reshape(a.shape[0], -1)


def att(xf, sd, store=ident):
    """bn(relu(attention.0(xf))) (P, 128)"""
    s, t = _bn_affine(sd, "attention.2")
    a = torch.relu(_mm(xf, sd["attention.0.weight"][:, :, 0].T) + sd["attention.0.bias"])
    return store(_fma(a, s.expand_as(a), t.expand_as(a)))


def logits(a, sd):
    """attention.3 (P, C Q): the attention energies, fp32 on every handle"""
    return _mm(a, sd["attention.3.weight"][:, :, 0].T) + sd["attention.3.bias"]


def pool_stats(lg, xf, centred=False, clamp=1e-5):
    """softmax over the frames, [mu | sqrt(clamp(var, 1e-5))] (2 C Q,): the handle's rs_pool_raw and, its affine being the identity,
    rs_pool.  The reference takes var = sum w x^2 - mu^2; centred: sum w (x - mu)^2, the form the pooling kernel sums"""
    w = torch.softmax(lg, dim=0)
    mu = (w * xf).sum(dim=0)
    var = (w * (xf - mu) ** 2).sum(dim=0) if centred else (w * xf ** 2).sum(dim=0) - mu ** 2
    if clamp is not None:
        var = var.clamp(min=clamp)
    return torch.cat([mu, torch.sqrt(var)])


def fc(pool, sd):
    """fc on [mu | sg], or on mu alone where fc.weight has C Q columns ('SAP')"""
    w = sd["fc.weight"]
    return pool[:w.shape[1]] @ w.T + sd["fc.bias"]


def block(x, sd, p, store=ident, squeeze_acc=False, kernel_sums=False, residual_relu=True, steps=None):
    """one block on x (P, Q, Cin).  squeeze_acc: the tile sums are taken from conv2's values before they are rounded for storage (every
    handle: the epilogue adds the fp32 value it is about to store).  kernel_sums: tile_sums' and squeeze_tiles' orders.
    residual_relu False: the identity residual from x itself (only ref64's variant asks for it).  steps: filled with BLOCK_STEPS"""
    s = {"conv1": conv1(x, sd, p, store)}
    raw = conv2(s["conv1"], sd, p, ident)
    s["conv2"] = store(raw)
    v = raw if squeeze_acc else s["conv2"]
    s["part"] = tile_sums(v, kernel_sums)
    n = v.shape[0] * v.shape[1]
    s["gate"] = gate(squeeze_tiles(s["part"], n) if kernel_sums else s["part"].sum(dim=0) / n, sd, p)
    if has_down(sd, p):
        s["down"] = down(x, sd, p, store)
        s["out"] = out(s["conv2"], s["gate"], s["down"], store, False)
    else:
        s["out"] = out(s["conv2"], s["gate"], x, store, residual_relu)
    if steps is not None:
        steps.update(s)
    return s["out"]


def forward(mel, sd, log_input=True, store=ident, squeeze_acc=False, kernel_sums=False, residual_relu=True, stages=None, xin=None):
    """one utterance's embedding from its mel power (n_mels, T) (or from xin, a normalised input).  stages: optional dict filled with
    xin, stem, b<i>_<step> of every block, att, logits, pool_raw (= pool)"""
    st = {}
    st["xin"] = prologue(mel, log_input, kernel_sums) if xin is None else xin
    x = st["stem"] = stem(st["xin"], sd, store)
    for i, p in enumerate(block_names(sd)):
        steps = {}
        x = block(x, sd, p, store, squeeze_acc, kernel_sums, residual_relu, steps)
        st.update({f"b{i}_{k}": v for k, v in steps.items()})
    xf = flat(x)
    st["att"] = att(xf, sd, store)
    st["logits"] = logits(st["att"], sd)
    st["pool_raw"] = st["pool"] = pool_stats(st["logits"], xf, kernel_sums)
    if stages is not None:
        stages.update(st)
    return fc(st["pool"], sd)
