"""Oracle (TEST INFRASTRUCTURE) — functional restatement of the reference TitaNet, as steps.

Follows reference ``src/models/TitaNet.py:159-431`` and ``src/models/blocks/titanet_blocks.py``: the prolog (Conv1dSamePadding k = 3 +
BatchNorm + ReLU, TitaNet.py:226-227, titanet_blocks.py:123-139), n mega-blocks (TitaNet.py:293-318: three sub-blocks of a depthwise
conv with 'same' zero padding, a pointwise conv, BatchNorm and ReLU, titanet_blocks.py:47-97; squeeze-excitation without biases,
titanet_blocks.py:162-192; a 1 x 1 skip + BatchNorm; ReLU of the sum), the epilog (TitaNet.py:244-245), attentive statistics pooling
(TitaNet.py:389-431: tanh(in_linear), out_linear, softmax over time, mean and sqrt(clamp(E[x^2] - mu^2, 1e-6)), BatchNorm1d(3072))
and the last linear layer with its BatchNorm (TitaNet.py:355-358).  Plain torch; pinned against the reference's float64 outputs and
stage checksums by ``tests/test_titanet_oracle_host.py`` (``tests/golden/titanet.npz``).

Every step works on ONE utterance, frame-major as the library stores it — (T, channels) — takes its input tensor and the state dict,
and computes in the dtype of both (float64 for the oracle; float32 for a CPU emulation of a handle).  ``store`` is applied to every
tensor a handle keeps in its storage type: the identity for the oracle, a rounding to bf16 for the emulation of a bf16 handle.

The state dict comes in two forms, and every step takes both.  The checkpoint's own: each conv is followed by its BatchNorm, which the
step folds into the conv in the dtype of the dict (W' = s W, b' = s b + t; s = gamma / sqrt(var + eps), t = beta - mean s).  And the
FOLDED form of ``folded_sd`` / ``rounded_sd``, which holds exactly the numbers a handle reads (make_conv_bn, api_titanet.hip): no
BatchNorm keys, the folded conv weights and biases, ``decoder.pool.1.scale`` / ``.shift`` and the folded last linear layer.

Multiply-adds that the kernels do in one rounding (the depthwise taps, the block tail, the pooling's BatchNorm) go through ``_fma``:
the product and the sum in float64, rounded once to the dtype of the operands — plain arithmetic for the float64 oracle.  GEMMs go
through oracle.conformer's ``_mm``, which ``matmul_as(chained_matmul(k))`` replaces by the kernels' order of sums.
"""
from __future__ import annotations

import torch

from oracle.conformer import _mm, bf16_round, chained_matmul, ident, matmul_as, to_torch_sd  # noqa: F401  (shared, unchanged)

ENC, ATT = 1536, 128
KERNEL = {256: 3, 512: 7, 1024: 11}                 # depthwise kernel size by hidden size (TitaNet.py:152-157)
BLOCK_STEPS = ("skip", "dw0", "pw0", "dw1", "pw1", "dw2", "pw2", "gate", "out")      # the handle's stages tn_b<i>_<step> (option tn_keep)
PROLOG, EPILOG = "encoder.prolog.conv_block.", "encoder.epilog.conv_block."
POOL, LINEAR = "decoder.pool.", "decoder.linear."


def _blk(i):
    return f"encoder.mega_blocks.{i}."


def n_blocks(sd):
    n = 0
    while _blk(n) + "skip_connection.0.weight" in sd:
        n += 1
    return n


def conv_bn_names(sd):
    """[(conv, its BatchNorm)] of every conv the handle folds its BatchNorm into, in forward order"""
    out = [(PROLOG + "0", PROLOG + "1")]
    for i in range(n_blocks(sd)):
        out += [(_blk(i) + f"sub_blocks.{j}.conv_block.0.conv.1", _blk(i) + f"sub_blocks.{j}.conv_block.1") for j in range(3)]
        out.append((_blk(i) + "skip_connection.0", _blk(i) + "skip_connection.1"))
    return out + [(EPILOG + "0", EPILOG + "1")]


def _fma(a, b, c):
    """a b + c in one rounding to the dtype of c (fmaf of the kernels; plain float64 arithmetic for the oracle)"""
    return (a.double() * b.double() + c.double()).to(c.dtype)


def _bn_affine(sd, p, eps=1e-5):
    """BatchNorm1d (eval) `p` as (scale, shift); the folded form of a dict holds them as p.scale / p.shift"""
    if p + ".scale" in sd:
        return sd[p + ".scale"], sd[p + ".shift"]
    s = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + eps)
    return s, sd[p + ".bias"] - sd[p + ".running_mean"] * s


def _conv_bn(sd, conv, bn, eps=1e-5):
    """(weight, bias) of conv followed by BatchNorm bn, the BatchNorm folded in; a folded dict holds them as the conv's own"""
    w, b = sd[conv + ".weight"], sd[conv + ".bias"]
    if bn + ".weight" not in sd:
        return w, b
    s, t = _bn_affine(sd, bn, eps)
    return w * s.reshape(-1, *([1] * (w.dim() - 1))), b * s + t


def folded_sd(sd, bf16=False):
    """the numbers a handle reads, in the dtype of sd (float64 for a reference, float32 for an emulation): every BatchNorm folded into
    its conv in double and cast to fp32 (make_conv_bn), decoder.pool.1 as fp32 scale / shift (make_bn), decoder.linear.1 folded into
    decoder.linear.0 in double and cast to fp32; depthwise weights, SE matrices and biases as they are.  bf16: what a bf16 handle
    reads — the GEMM weights (the folded convs, in_linear, out_linear) rounded to bf16 AFTER the fold, and the bf16 copies of the two
    SE matrices; the depthwise weights, every bias, decoder.pool.1 and the last linear layer stay fp32."""
    some = next(v for v in sd.values() if torch.is_floating_point(v))
    d64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}
    f32 = lambda t: t.float().double()
    out = {}
    for conv, bn in conv_bn_names(d64):
        w, b = _conv_bn(d64, conv, bn)
        out[conv + ".weight"], out[conv + ".bias"] = f32(w), f32(b)
    s, t = _bn_affine(d64, POOL + "1")
    out[POOL + "1.scale"], out[POOL + "1.shift"] = f32(s), f32(t)
    w, b = _conv_bn(d64, LINEAR + "0", LINEAR + "1")
    out[LINEAR + "0.weight"], out[LINEAR + "0.bias"] = f32(w), f32(b)
    for k, v in d64.items():
        if k not in out and torch.is_floating_point(v) and ".conv_block.1." not in k and "skip_connection.1." not in k and \
                not k.startswith(POOL + "1.") and not k.startswith(LINEAR + "1."):
            out[k] = v
    if bf16:
        for k in out:
            if is_gemm_weight(k) or ".excitation." in k:
                out[k] = bf16_round(out[k])
    return {k: v.to(some.dtype) for k, v in out.items()}


def is_gemm_weight(k):
    """the tensors a bf16 handle's GEMMs read in bf16: the prolog, pointwise, skip and epilog convs and the two attention layers"""
    if not k.endswith(".weight"):
        return False
    return k in (PROLOG + "0.weight", EPILOG + "0.weight", POOL + "0.in_linear.weight", POOL + "0.out_linear.weight") or \
        k.endswith(".conv.1.weight") or k.endswith("skip_connection.0.weight")


def rounded_sd(sd):
    """the weights a bf16 handle reads (folded_sd, bf16), in the dtype of sd"""
    return folded_sd(sd, bf16=True)


# ---- the steps ------------------------------------------------------------------------------------------------------------------------
def prolog(mel, sd, store=ident, eps=1e-5):
    """(n_mels, T) mel power as it is -> (T, H): the k = 3 conv with zero padding at the utterance's own ends as the GEMM the library runs
    (k = tap * n_mels + c over the rows t - 1, t, t + 1), BatchNorm, ReLU.  The handle keeps its input rows in its storage type."""
    x = store(mel.T)
    z = x.new_zeros(1, x.shape[1])
    cols = torch.cat([torch.cat([z, x[:-1]]), x, torch.cat([x[1:], z])], dim=1)
    w, b = _conv_bn(sd, PROLOG + "0", PROLOG + "1", eps)
    return store(torch.relu(_mm(cols, w.permute(0, 2, 1).reshape(w.shape[0], -1).T) + b))


def skip(x, sd, i, store=ident, eps=1e-5):
    """BN(conv1x1(x)): the block's skip connection (TitaNet.py:306-308), no activation"""
    w, b = _conv_bn(sd, _blk(i) + "skip_connection.0", _blk(i) + "skip_connection.1", eps)
    return store(_mm(x, w[:, :, 0].T) + b)


def dw(x, sd, i, j, store=ident):
    """depthwise conv j of block i with 'same' zero padding, its bias included: ((b + w_0 x_{t-R}) + w_1 x_{t-R+1}) + ..., the order of
    tn_dw / tn_mega_tail (titanet.hip)"""
    q = _blk(i) + f"sub_blocks.{j}.conv_block.0.conv.0."
    w = sd[q + "weight"][:, 0, :]                      # (H, k)
    k = w.shape[1]
    T = x.shape[0]
    z = x.new_zeros(k // 2, x.shape[1])
    xp = torch.cat([z, x, z])
    a = sd[q + "bias"].expand(T, -1)
    for t in range(k):
        a = _fma(w[:, t], xp[t:t + T], a)
    return store(a)


def pw(d, sd, i, j, store=ident, eps=1e-5):
    """relu(BN(pointwise conv j of block i))"""
    q = _blk(i) + f"sub_blocks.{j}.conv_block."
    w, b = _conv_bn(sd, q + "0.conv.1", q + "1", eps)
    return store(torch.relu(_mm(d, w[:, :, 0].T) + b))


def squeeze(h, kernel_sums=False):
    """the SE squeeze: the mean over the utterance's own frames.  kernel_sums: added up as colstats_kernel does (elementwise.hip) — four
    chains over the frames t = w, w + 4, ..., then ((s0 + s1) + s2) + s3, divided by T"""
    if not kernel_sums:
        return h.mean(dim=0)
    s = [h.new_zeros(h.shape[1]) for _ in range(4)]
    for t in range(h.shape[0]):
        s[t & 3] = s[t & 3] + h[t]
    return (((s[0] + s[1]) + s[2]) + s[3]) / h.shape[0]


def gate(m, sd, i):
    """sigmoid(W2 relu(W1 m)): the SE excitation (no biases)"""
    e = _blk(i) + "sub_blocks.3.excitation."
    return torch.sigmoid(torch.relu(m @ sd[e + "0.weight"].T) @ sd[e + "2.weight"].T)


def out(sk, h3, g, store=ident):
    """relu(skip + g h3): the mega-block's output"""
    return store(torch.relu(_fma(g.expand_as(h3), h3, sk)))


def epilog(x, sd, store=ident, eps=1e-5):
    w, b = _conv_bn(sd, EPILOG + "0", EPILOG + "1", eps)
    return store(torch.relu(_mm(x, w[:, :, 0].T) + b))


def att(enc, sd, store=ident):
    """tanh(in_linear(enc)) (T, 128)"""
    return store(torch.tanh(_mm(enc, sd[POOL + "0.in_linear.weight"].T) + sd[POOL + "0.in_linear.bias"]))


def logits(a, sd):
    """out_linear (T, 1536): the attention energies, fp32 on every handle"""
    return _mm(a, sd[POOL + "0.out_linear.weight"].T) + sd[POOL + "0.out_linear.bias"]


def pool_stats(lg, enc, centred=False):
    """softmax over time, [mu | sqrt(clamp(var, 1e-6))] (3072,): the handle's tn_pool_raw.  The reference takes var = sum a x^2 - mu^2
    (TitaNet.py:420-424); centred: sum a (x - mu)^2, the same number in exact arithmetic and the form the pooling kernel sums"""
    a = torch.softmax(lg, dim=0)
    mu = (a * enc).sum(dim=0)
    var = (a * (enc - mu) ** 2).sum(dim=0) if centred else (a * enc ** 2).sum(dim=0) - mu ** 2
    return torch.cat([mu, torch.sqrt(var.clamp(min=1e-6))])


def pool_norm(raw, sd):
    """decoder.pool.1 (BatchNorm1d(3072), eval): the handle's tn_pool"""
    s, t = _bn_affine(sd, POOL + "1")
    return _fma(raw, s, t)


def fc(pool, sd):
    """decoder.linear: Linear(3072, nOut) + BatchNorm1d(nOut)"""
    w, b = _conv_bn(sd, LINEAR + "0", LINEAR + "1")
    return pool @ w.T + b


def block(x, sd, i, d0=None, store=ident, squeeze_acc=False, kernel_sums=False, steps=None):
    """one mega-block on x (T, H).  d0: its first depthwise output when the previous block's tail has made it (None: computed here, the
    same numbers).  squeeze_acc: the squeeze reads the third pointwise conv's values before they are rounded for storage (the column
    sums of a bf16 handle's GEMM epilogue).  kernel_sums: squeeze's.  steps: optional dict filled with BLOCK_STEPS and mean"""
    s = {"skip": skip(x, sd, i, store)}
    s["dw0"] = d = dw(x, sd, i, 0, store) if d0 is None else d0
    for j in range(3):
        if j:
            s[f"dw{j}"] = d = dw(s[f"pw{j - 1}"], sd, i, j, store)
        s[f"pw{j}"] = pw(d, sd, i, j, store)
    s["mean"] = squeeze(pw(d, sd, i, 2, ident) if squeeze_acc else s["pw2"], kernel_sums)
    s["gate"] = gate(s["mean"], sd, i)
    s["out"] = out(s["skip"], s["pw2"], s["gate"], store)
    if steps is not None:
        steps.update(s)
    return s["out"]


def forward(mel, sd, store=ident, squeeze_acc=False, kernel_sums=False, stages=None):
    """one utterance's embedding from its mel power (n_mels, T).  kernel_sums: the reductions over time in the kernels' forms (squeeze,
    pool_stats' centred variance) — for an emulation; the same numbers in exact arithmetic.
    stages: optional dict filled with prolog, b<i>_<step> and b<i>_mean of
    every block, enc, att, logits, pool_raw, pool"""
    st = {}
    x = st["prolog"] = prolog(mel, sd, store)
    for i in range(n_blocks(sd)):
        steps = {}
        x = block(x, sd, i, None, store, squeeze_acc, kernel_sums, steps)
        st.update({f"b{i}_{k}": v for k, v in steps.items()})
    st["enc"] = epilog(x, sd, store)
    st["att"] = att(st["enc"], sd, store)
    st["logits"] = logits(st["att"], sd)
    st["pool_raw"] = pool_stats(st["logits"], st["enc"], kernel_sums)
    st["pool"] = pool_norm(st["pool_raw"], sd)
    if stages is not None:
        stages.update(st)
    return fc(st["pool"], sd)
