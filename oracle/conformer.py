"""Oracle (TEST INFRASTRUCTURE) — functional restatement of the reference Conformer speaker encoder, as steps.

Follows reference ``src/models/Conformer.py:80-124`` and ``src/models/conformer/conformer/{encoder,feed_forward,attention,convolution,
embedding}.py``: log + InstanceNorm front-end, Conv2dSubampling + input projection, six Conformer blocks (half-step feed-forward,
relative multi-head self-attention with the reference's cat / view shift, convolution module, half-step feed-forward, LayerNorm),
attentive statistics pooling with ``clamp(1e-4, 1e4)``, ``attention_norm`` and ``fc``.  Plain torch; pinned against the reference's
float64 outputs and stage values by ``tests/test_conformer_oracle_host.py`` (``tests/golden/conformer.npz``).

Every step works on ONE utterance, frame-major as the library stores it — (T', channels) — takes its input tensor and the state dict,
and computes in the dtype of both (float64 for the oracle; float32 for a CPU emulation of a handle).  ``store`` is applied to every
tensor a handle keeps in its storage type on the way (LayerNorm outputs, the feed-forward hidden layer, the step's own output): the
identity for the oracle, a rounding to bf16 for the emulation of a bf16 handle.  ``stage`` of ``attn_context`` is applied to what the
attention kernel stages as MFMA operands (q + u, q + v, k, v, P, the softmax weights).
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

D, HEADS, DH, LAYERS, DW_K = 256, 4, 64, 6, 15
SUB = "conformer_block.conv_subsample.sequential."
PROJ = "conformer_block.input_projection.0.linear."
BLOCK_STEPS = ("ff1", "qkv", "ctx", "att", "pw1", "dw", "conv", "ff2", "out")      # the handle's stages cf_b<i>_<step> (option cf_keep)


def ident(x):
    return x


# Every GEMM of the steps below (the Linears, the pointwise convolutions, conv2 of the subsampling as the GEMM the library runs) goes
# through _mm, which matmul_as replaces for the length of a with-block: an emulation of a handle sums its products in the kernels'
# order (chained_matmul), the oracle leaves torch's own.
_MATMUL = [torch.matmul]


def _mm(a, b):
    return _MATMUL[0](a, b)


@contextlib.contextmanager
def matmul_as(fn):
    old, _MATMUL[0] = _MATMUL[0], fn
    try:
        yield
    finally:
        _MATMUL[0] = old


def chained_matmul(kstep):
    """(M, K) @ (K, N) as the library's GEMM kernels add it up: one accumulator per output in the dtype of the operands, the products
    added `kstep` at a time in the order of k (the depth of one MFMA: 2 for v_mfma_f32_32x32x2f32, 16 for the bf16 forms).  A chain
    of K / kstep fp32 additions loses about sqrt(K / kstep) roundings, where a CPU GEMM's blocked sums lose far fewer."""
    def mm(a, b):
        if a.dim() != 2:                       # (fc on the pooled vector: the library's row-vector kernel, not a GEMM)
            return torch.matmul(a, b)
        a, b = a.contiguous(), b.contiguous()
        acc = a[:, :kstep] @ b[:kstep]
        for k in range(kstep, a.shape[1], kstep):
            acc.addmm_(a[:, k:k + kstep], b[k:k + kstep])
        return acc
    return mm


def to_torch_sd(sd, dtype=torch.float64):
    out = {}
    for k, v in sd.items():
        t = torch.as_tensor(v)
        out[k] = t.to(dtype) if t.is_floating_point() else t
    return out


def bf16_round(t):
    """round to bf16 (nearest even) from fp32, as the 16-bit weight upload and the kernels' bf16 stores do; the dtype is kept"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def is_gemm_weight(k):
    """the tensors a bf16 handle reads in bf16: every GEMM's weight matrix (conv2 of the subsampling, the input projection, the linears
    and pointwise convolutions of the blocks, the two pooling convolutions).  conv1's taps, the depthwise taps, LayerNorm, biases, BN,
    u / v, pos_proj (P is formed on the host in double and kept in fp32) and fc stay fp32."""
    if k in (SUB + "2.weight", PROJ + "weight", "attention.0.weight", "attention.3.weight"):
        return True
    if not k.startswith("conformer_block.layers."):
        return False
    if k.endswith("pos_proj.linear.weight"):
        return False
    return k.endswith(".linear.weight") or k.endswith("sequential.2.conv.weight") or k.endswith("sequential.7.conv.weight")


def rounded_sd(sd):
    """the weights a bf16 handle reads (is_gemm_weight), in the dtype of sd"""
    return {k: (bf16_round(v) if is_gemm_weight(k) else v) for k, v in sd.items()}


def frames(T):
    """T' of T mel frames: two 3 x 3 stride-2 convolutions"""
    return ((T - 3) // 2 + 1 - 3) // 2 + 1


def _bn(x, sd, p, eps=1e-5):
    """BatchNorm1d (eval) over the last axis of x"""
    s = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + eps)
    return (x - sd[p + ".running_mean"]) * s + sd[p + ".bias"]


def _ln(x, sd, p):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], 1e-5)


def _lin(x, sd, p):
    w = sd[p + ".weight"]
    return _mm(x, w.reshape(w.shape[0], -1).T) + sd[p + ".bias"]


def swish(x):
    return x * torch.sigmoid(x)


# ---- front-end ----------------------------------------------------------------------------------------------------------------------
def features(mel, sd, store=ident):
    """(n_mels, T) mel power -> (T, n_mels): log(x + 1e-6), the mean over time off, InstanceNorm1d(affine, eps 1e-5) (Conformer.py:92-98)"""
    x = (mel + 1e-6).log()
    x = x - x.mean(dim=-1, keepdim=True)
    x = F.instance_norm(x[None], weight=sd["instance_norm.weight"], bias=sd["instance_norm.bias"], eps=1e-5)[0]
    return store(x.T)


def conv1(x, sd, store=ident):
    """(T, n_mels) -> (256, T1, F1): Conv2d(1, 256, 3, stride 2) + ReLU on the (T, F) image"""
    return store(F.relu(F.conv2d(x[None, None], sd[SUB + "0.weight"], sd[SUB + "0.bias"], stride=2))[0])


def conv2(y, sd, store=ident):
    """(256, T1, F1) -> (256, T', F2): Conv2d(256, 256, 3, stride 2) + ReLU, as a GEMM over the unfolded 3 x 3 windows"""
    w = sd[SUB + "2.weight"]
    Tp, F2 = (y.shape[1] - 3) // 2 + 1, (y.shape[2] - 3) // 2 + 1
    cols = F.unfold(y[None], kernel_size=3, stride=2)[0]                 # (256 * 9, T' F2), k = (c, dt, df) as the weight's own layout
    z = _mm(cols.T, w.reshape(w.shape[0], -1).T) + sd[SUB + "2.bias"]
    return store(F.relu(z).T.reshape(w.shape[0], Tp, F2))


def input_projection(z, sd, store=ident):
    """(256, T', F2) -> (T', 256): permute to (T', 256 F2), column c F2 + f (convolution.py:180-181), then the Linear"""
    return store(_lin(z.permute(1, 0, 2).reshape(z.shape[1], -1), sd, PROJ[:-1]))


def subsample(x, sd, store=ident):
    """features (T, n_mels) -> the encoder's input (T', 256): the handle's stage cf_in"""
    return input_projection(conv2(conv1(x, sd, store), sd, store), sd, store)


# ---- one block ----------------------------------------------------------------------------------------------------------------------
def _blk(i):
    return f"conformer_block.layers.{i}."


def ff_half(x, sd, i, which, store=ident):
    """x + 0.5 FF(x): LayerNorm, Linear + Swish, Linear (feed_forward.py); which: 0 the block's first feed-forward module, 1 its second"""
    p = _blk(i) + ("sequential.0." if which == 0 else "sequential.3.") + "module.sequential."
    h = store(swish(_lin(store(_ln(x, sd, p + "0")), sd, p + "1.linear")))
    return store(0.5 * _lin(h, sd, p + "4.linear") + x)


def qkv(x, sd, i, store=ident):
    """(T', 256) -> (T', 768): LayerNorm, then the query | key | value projections side by side"""
    a = _blk(i) + "sequential.1.module."
    ln = store(_ln(x, sd, a + "layer_norm"))
    return store(torch.cat([_lin(ln, sd, a + f"attention.{n}.linear") for n in ("query_proj", "key_proj", "value_proj")], dim=-1))


def pos_table(sd, i, T, f32=True):
    """P = pe[:T'] W_pos^T (T', 256), summed in float64; f32: rounded to fp32 as the handle keeps it; in the dtype of sd"""
    a = _blk(i) + "sequential.1.module."
    w = sd[a + "attention.pos_proj.linear.weight"]
    P = sd[a + "positional_encoding.pe"][0, :T].double() @ w.double().T
    return (P.float() if f32 else P).to(w.dtype)


def relative_shift(pos):
    """RelativeMultiHeadAttention._relative_shift (attention.py:105-113) on (heads, T', T'): a zero column in front, the (T', T' + 1)
    matrix read as (T' + 1, T'), its first row dropped"""
    h, t1, t2 = pos.shape
    padded = torch.cat([pos.new_zeros(h, t1, 1), pos], dim=-1).view(h, t2 + 1, t1)
    return padded[:, 1:].reshape(h, t1, t2)


def attn_context(x, P, sd, i, store=ident, stage=ident):
    """q | k | v (T', 768) and P (T', 256) -> the attention context (T', 256) before out_proj (attention.py:80-101); scores / 16"""
    a = _blk(i) + "sequential.1.module.attention."
    T = x.shape[0]
    q, k, v = (x[:, c * D:(c + 1) * D].reshape(T, HEADS, DH).transpose(0, 1) for c in range(3))      # (4, T', 64)
    p = stage(P).reshape(T, HEADS, DH).transpose(0, 1)
    content = stage(q + sd[a + "u_bias"][:, None]) @ stage(k).transpose(1, 2)
    pos = relative_shift(stage(q + sd[a + "v_bias"][:, None]) @ p.transpose(1, 2))
    score = (content + pos) / 16.0
    w = torch.exp(score - score.max(dim=-1, keepdim=True).values)
    out = (stage(w) @ stage(v)) / w.sum(dim=-1, keepdim=True)          # (the kernel normalises by the sum of the unrounded weights)
    return store(out.transpose(0, 1).reshape(T, D))


def out_proj(ctx, r, sd, i, store=ident):
    """r + out_proj(ctx): the MHSA module's residual step"""
    return store(_lin(ctx, sd, _blk(i) + "sequential.1.module.attention.out_proj.linear") + r)


def pw1(x, sd, i, store=ident):
    """(T', 256) -> (T', 512): LayerNorm, the first pointwise convolution"""
    cv = _blk(i) + "sequential.2.module.sequential."
    return store(_lin(store(_ln(x, sd, cv + "0")), sd, cv + "2.conv"))


def glu_dw(u, sd, i, store=ident):
    """(T', 512) -> (T', 256): GLU over the channels, depthwise conv k = 15 with zero padding 7, BatchNorm (eval), Swish"""
    cv = _blk(i) + "sequential.2.module.sequential."
    g = u[:, :D] * torch.sigmoid(u[:, D:])
    y = F.conv1d(g.T[None], sd[cv + "4.conv.weight"], None, padding=(DW_K - 1) // 2, groups=D)[0].T
    return store(swish(_bn(y, sd, cv + "5")))


def pw2(dw, xo, sd, i, store=ident):
    """xo + pw2(dw): the convolution module's residual step"""
    return store(_lin(dw, sd, _blk(i) + "sequential.2.module.sequential.7.conv") + xo)


def final_ln(x, sd, i, store=ident):
    return store(_ln(x, sd, _blk(i) + "sequential.4"))


def mhsa(r, sd, i, store=ident, stage=ident, f32_P=False):
    """r + MHSA(r)"""
    x = qkv(r, sd, i, store)
    return out_proj(attn_context(x, pos_table(sd, i, r.shape[0], f32_P), sd, i, store, stage), r, sd, i, store)


def conv_module(xo, sd, i, store=ident):
    """xo + Conv(xo)"""
    return pw2(glu_dw(pw1(xo, sd, i, store), sd, i, store), xo, sd, i, store)


def block(x, sd, i, store=ident, stage=ident, f32_P=False, steps=None):
    """one Conformer block (encoder.py ConformerBlock); steps: optional dict filled with the block's nine stored tensors (BLOCK_STEPS)"""
    s = {}
    s["ff1"] = ff_half(x, sd, i, 0, store)
    s["qkv"] = qkv(s["ff1"], sd, i, store)
    s["ctx"] = attn_context(s["qkv"], pos_table(sd, i, x.shape[0], f32_P), sd, i, store, stage)
    s["att"] = out_proj(s["ctx"], s["ff1"], sd, i, store)
    s["pw1"] = pw1(s["att"], sd, i, store)
    s["dw"] = glu_dw(s["pw1"], sd, i, store)
    s["conv"] = pw2(s["dw"], s["att"], sd, i, store)
    s["ff2"] = ff_half(s["conv"], sd, i, 1, store)
    s["out"] = final_ln(s["ff2"], sd, i, store)
    if steps is not None:
        steps.update(s)
    return s["out"]


# ---- pooling and fc -----------------------------------------------------------------------------------------------------------------
def pool_logits(x, sd, store=ident):
    """(T', 256) -> (T', 256) fp32 logits: attention.0, ReLU, attention.2 (BatchNorm), attention.3 (Conformer.py:64-70)"""
    h = store(_bn(F.relu(_lin(x, sd, "attention.0")), sd, "attention.2"))
    return _lin(h, sd, "attention.3")


def pool_stats(logits, x):
    """softmax over time, [mu | sqrt(clamp(sum w x^2 - mu^2, 1e-4, 1e4))] (Conformer.py:106-111): (512,), the handle's cf_pool_raw"""
    w = torch.softmax(logits, dim=0)
    mu = (x * w).sum(dim=0)
    sg = torch.sqrt(((x ** 2) * w).sum(dim=0).sub(mu ** 2).clamp(min=1e-4, max=1e4))
    return torch.cat([mu, sg])


def pool_norm(raw, sd):
    """attention_norm (BatchNorm1d(512), eval): the handle's cf_pool"""
    return _bn(raw, sd, "attention_norm")


def fc(pool, sd):
    return _lin(pool, sd, "fc.conv")


def forward(mel, sd, store=ident, stage=ident, f32_P=False, stages=None):
    """one utterance's embedding from its mel power (n_mels, T).  stages: optional dict filled with input, cf_in, b<i>_<step> of every
    block, logits, pool_raw, pool"""
    st = {}
    st["input"] = features(mel, sd, store)
    x = st["cf_in"] = subsample(st["input"], sd, store)
    for i in range(LAYERS):
        steps = {}
        x = block(x, sd, i, store, stage, f32_P, steps)
        st.update({f"b{i}_{k}": v for k, v in steps.items()})
    st["logits"] = pool_logits(x, sd, store)
    st["pool_raw"] = pool_stats(st["logits"], x)
    st["pool"] = pool_norm(st["pool_raw"], sd)
    if stages is not None:
        stages.update(st)
    return fc(st["pool"], sd)
