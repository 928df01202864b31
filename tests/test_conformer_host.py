"""Host-side Conformer checks (no GPU): the spec against the reference's key list (stored by tools/make_golden_conformer.py), the
positional-encoding buffer against torch's own formula, the reference's relative shift as an index map, the input projection's column
permutation, checkpoint conversion, and the plug-in's refusals."""
import math
import os

import numpy as np
import pytest
import torch

from speakerverification_amd import _lib, checkpoint, synth
from speakerverification_amd.models import Conformer

KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="melspectrogram")


def test_conformer_keys_equal_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "conformer.npz"))
    spec = synth.conformer_param_spec(512, 80)
    assert [k for k, _ in spec] == list(g["keys"])
    assert len(spec) == 278 and sum(int(np.prod(s)) for _, s in spec) == 27_174_314
    m = Conformer.MainModel(nOut=512, device="cpu", **KW)
    assert list(m.state_dict()) == list(g["keys"])


def test_pe_matches_torch_formula():
    """embedding.py:30-38 evaluated by torch itself"""
    d, n = 256, 10000
    pe = torch.zeros(n, d)
    position = torch.arange(0, n, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2).float() * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    ours = synth.conformer_pe()
    assert ours.shape == (1, n, d) and ours.dtype == np.float32
    assert np.array_equal(ours[0], pe.numpy())
    sd = synth.synth_state_dict(synth.conformer_param_spec(), seed=3)
    assert np.array_equal(sd["conformer_block.layers.4.sequential.1.module.positional_encoding.pe"], ours)


def _shift_ref(pos):
    """RelativeMultiHeadAttention._relative_shift (attention.py:110-118), the cat / view form"""
    b, h, t1, t2 = pos.shape
    padded = torch.cat([pos.new_zeros(b, h, t1, 1), pos], dim=-1).view(b, h, t2 + 1, t1)
    return padded[:, :, 1:].reshape(b, h, t1, t2)


def _shift_map(pos):
    """the index map the kernel uses: j <= i: pos[i, T-1-(i-j)]; j == i+1: 0; j >= i+2: pos[i+1, j-i-2]"""
    T = pos.shape[-1]
    out = np.zeros_like(pos)
    for i in range(T):
        for j in range(T):
            if j <= i:
                out[..., i, j] = pos[..., i, T - 1 - (i - j)]
            elif j >= i + 2:
                out[..., i, j] = pos[..., i + 1, j - i - 2]
    return out


@pytest.mark.parametrize("T", list(range(1, 21)))
def test_relative_shift_index_map(T):
    rng = np.random.default_rng(T)
    pos = rng.standard_normal((2, 3, T, T))
    want = _shift_ref(torch.from_numpy(pos)).numpy()
    assert np.array_equal(_shift_map(pos), want)
    if T >= 3:          # the standard Transformer-XL shift (row i only) is a different map
        std = np.zeros_like(pos)
        for i in range(T):
            for j in range(T):
                std[..., i, j] = pos[..., i, T - 1 - (i - j)] if j <= i else 0.0
        assert not np.array_equal(std, want)


def test_input_projection_column_permutation():
    """Conv2dSubampling's permute(0, 2, 1, 3).view(B, T', 256 F2) puts feature c F2 + f in column c F2 + f; the library's GEMM writes
    (b, t, f) rows of 256 channels, i.e. column f 256 + c of the (B T', 256 F2) view, so finalize permutes the projection's columns"""
    rng = np.random.default_rng(0)
    C, F2, T, N = 8, 5, 3, 4
    y = rng.standard_normal((C, T, F2))                      # conv2 output of one utterance (channels, T', F2)
    W = rng.standard_normal((N, C * F2))
    ref = torch.from_numpy(y)[None].permute(0, 2, 1, 3).reshape(1, T, C * F2).numpy()[0] @ W.T
    rows = y.transpose(1, 2, 0).reshape(T, F2 * C)           # the GEMM's layout: (t, f, c)
    Wp = np.empty_like(W)
    for c in range(C):
        for f in range(F2):
            Wp[:, f * C + c] = W[:, c * F2 + f]
    assert np.allclose(rows @ Wp.T, ref, rtol=0, atol=1e-12)


def test_conformer_checkpoint_round_trip(tmp_path):
    sd = synth.synth_state_dict(synth.conformer_param_spec(192, 80), seed=4)
    n = checkpoint.convert_checkpoint({"__S__." + k: v for k, v in sd.items()}, str(tmp_path / "conformer.svw"), "Conformer")
    assert n == len(sd)
    mid, back = checkpoint.read_blob(str(tmp_path / "conformer.svw"))
    assert mid == _lib.MODEL_CONFORMER == 7
    for k, v in sd.items():
        if np.asarray(v).dtype != np.int64:
            assert np.array_equal(np.asarray(back[k]), v), k
    m = Conformer.MainModel(nOut=192, device="cpu", **KW)
    m.load_blob(str(tmp_path / "conformer.svw"))
    assert np.array_equal(np.asarray(m.state_dict()["fc.conv.weight"]), sd["fc.conv.weight"])


def test_conformer_plugin_refusals():
    m = Conformer.MainModel(nOut=512, device="cuda:0", **KW)
    assert m.accepts_length(512) and not m.accepts_length(511)
    assert m.accepts_length(40005 * 80) and not m.accepts_length(40006 * 80)          # T' = 10000 / 10001
    with pytest.raises(ValueError):
        m.embed_wave(np.zeros((2, 400), np.float32))
    with pytest.raises(ValueError):
        m(np.zeros((1, 80, 6), np.float32))
    for kw in (dict(hip_compute="f16"), dict(hip_compute="f32x3"), dict(attention_dim=64),
               dict(augment=True, augment_options={"augment_chain": ["env_corrupt", "spec_domain"]})):
        a = dict(KW)
        a.update(kw)
        with pytest.raises(NotImplementedError):
            Conformer.MainModel(nOut=512, device="cpu", **a)
    # env_corrupt / time_domain augmentation happens before the model: accepted
    a = dict(KW, augment=True, augment_options={"augment_chain": ["env_corrupt"]})
    Conformer.MainModel(nOut=512, device="cpu", **a)
    assert synth.conformer_frames(401) == 99 and synth.conformer_frames(7) == 1 and synth.conformer_frames(6) == 0
