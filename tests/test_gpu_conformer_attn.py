"""Conformer's relative-position attention kernel on its own (svhip_conformer_attention) against a float64 restatement that uses the
reference's own cat / view shift (attention.py:75-118), on random q / k / v / P / biases at T' = 1, 2, 3, 17, 99, 128, 129, 1000 (below,
at and past one 64-query / 64-key tile; many online-softmax rescales), f32 and bf16; the standard Transformer-XL shift must not match,
and nothing may cross utterances."""
import numpy as np
import pytest
import torch

from speakerverification_amd import _lib

pytestmark = pytest.mark.gpu


def _rel(out, ref):
    return float(np.abs(out - ref).max()) / float(np.abs(ref).max())


def _attn_ref64(qkv, P, u, v, B, Tp, shift="reference"):
    """float64 restatement of the attention kernel's contract (attention.py:75-118): (B T', 768) q | k | v -> (B T', 256)"""
    x = torch.from_numpy(qkv).double().view(B, Tp, 3, 4, 64)
    q, k, vv = (x[:, :, c].transpose(1, 2) for c in range(3))              # (B, 4, T', 64)
    p = torch.from_numpy(P).double().view(Tp, 4, 64).transpose(0, 1)         # (4, T', 64)
    ub, vb = torch.from_numpy(u).double()[None, :, None], torch.from_numpy(v).double()[None, :, None]
    content = (q + ub) @ k.transpose(2, 3)
    pos = (q + vb) @ p.transpose(1, 2)[None]
    if shift == "reference":
        z = pos.new_zeros(B, 4, Tp, 1)
        pos = torch.cat([z, pos], dim=-1).view(B, 4, Tp + 1, Tp)[:, :, 1:].reshape(B, 4, Tp, Tp)
    else:                   # the standard Transformer-XL shift: row i only, zero above the diagonal
        idx = torch.arange(Tp)
        rel = (Tp - 1 - (idx[:, None] - idx[None, :])).clamp(0, Tp - 1)
        pos = torch.gather(pos, 3, rel.expand(B, 4, Tp, Tp)) * (idx[None, :] <= idx[:, None])
    att = torch.softmax((content + pos) / 16.0, -1)
    return (att @ vv).transpose(1, 2).reshape(B * Tp, 256).numpy()


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("Tp", [1, 2, 3, 17, 99, 128, 129, 1000])
def test_cf_attn_alone_against_float64(Tp, compute):
    """the attention kernel by itself (svhip_conformer_attention) on random q / k / v / P / biases, B = 2, at T' below, at and past one
    64-query / 64-key tile and over many online-softmax rescales; the standard Transformer-XL shift must NOT match (T' >= 3)"""
    lib = _lib.load()
    B = 2
    rng = np.random.default_rng(Tp)
    qkv = rng.standard_normal((B * Tp, 768)).astype(np.float32)
    P = rng.standard_normal((Tp, 256)).astype(np.float32)
    u = (0.5 * rng.standard_normal((4, 64))).astype(np.float32)
    v = (0.5 * rng.standard_normal((4, 64))).astype(np.float32)
    dtype = torch.float32 if compute == "f32" else torch.bfloat16
    qkv_d = torch.from_numpy(qkv).cuda().to(dtype)
    if compute == "bf16":         # the reference sees exactly the operands the kernel reads
        qkv = qkv_d.float().cpu().numpy()
    P_d, u_d, v_d = (torch.from_numpy(a).cuda() for a in (P, u, v))
    out_d = torch.full((B * Tp, 256), float("nan"), device="cuda", dtype=dtype)
    torch.cuda.synchronize()
    rc = lib.svhip_conformer_attention(qkv_d.data_ptr(), P_d.data_ptr(), u_d.data_ptr(), v_d.data_ptr(), out_d.data_ptr(),
                                       _lib.F32 if compute == "f32" else _lib.BF16, B, Tp, None)
    assert rc == _lib.OK
    torch.cuda.synchronize()
    got = out_d.float().cpu().numpy()
    want = _attn_ref64(qkv, P, u, v, B, Tp)
    r = _rel(got, want)
    print(f"T'={Tp} {compute}: {r:.2e} of scale")
    assert np.isfinite(got).all() and r <= (1e-5 if compute == "f32" else 2e-2), r
    if Tp >= 3:
        assert _rel(got, _attn_ref64(qkv, P, u, v, B, Tp, shift="standard")) > 2e-2
    # nothing crosses utterances: utterance 1 alone gives its rows of the B = 2 call
    one = torch.full((Tp, 256), float("nan"), device="cuda", dtype=dtype)
    assert lib.svhip_conformer_attention(qkv_d[Tp:].contiguous().data_ptr(), P_d.data_ptr(), u_d.data_ptr(), v_d.data_ptr(), one.data_ptr(),
                                         _lib.F32 if compute == "f32" else _lib.BF16, 1, Tp, None) == _lib.OK
    torch.cuda.synchronize()
    assert np.array_equal(one.float().cpu().numpy(), got[Tp:])
