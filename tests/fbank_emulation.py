"""The mel front-end (csrc/fbank.hip) on the CPU, its sums in its kernels' order, at any geometry the front-end takes.  Shared by the
oracle checks of the models that read mel power from a waveform (tests/titanet_oracle_check.py, tests/resnetse_oracle_check.py: the
default geometry) and by tests/fbank_geometry_check.py (every other one).  The keywords are oracle.fbank.FBANK_DEFAULTS' and
`pre_emphasis` (True: 0.97, False / None: none, a number: that coefficient, rounded to float32 as the reference's filter tensor is)."""
import numpy as np
import torch

from oracle import fbank as o_fbank
from oracle.conformer import bf16_round, chained_matmul
from oracle.titanet import _fma

KSTEP_F32 = 2                                 # products per v_mfma_f32_32x32x2f32


def geometry(**kw):
    """FBANK_DEFAULTS with the given keywords put over them; an unknown keyword is an error"""
    p = dict(o_fbank.FBANK_DEFAULTS)
    unknown = set(kw) - set(p)
    assert not unknown, unknown
    p.update(kw)
    return p


def emphasised(x, pre_emphasis=True):
    """(B, L) samples -> the pre-emphasised samples in the dtype of x"""
    if pre_emphasis is False or pre_emphasis is None:
        return x
    return o_fbank.pre_emphasis(x, 0.97 if pre_emphasis is True else float(pre_emphasis))


def _frames(wave, p, pre_emphasis):
    """(L,) samples -> (T, win_length) fp32: the non-zero window's samples of every frame, and the window's first tap in the frame"""
    n_fft, win, hop = p["n_fft"], p["win_length"], p["hop_length"]
    lo = (n_fft - win) // 2
    y = emphasised(torch.tensor(np.asarray(wave), dtype=torch.float32)[None], pre_emphasis)
    yp = torch.nn.functional.pad(y.unsqueeze(1), (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
    return yp.unfold(0, n_fft, hop)[:, lo:lo + win].contiguous(), lo


def _basis(p, lo):
    """the windowed cos and sin taps (win_length, n_bins) fp32"""
    win = p["win_length"]
    wsin, wcos = o_fbank.fourier_kernels(p["n_fft"], win, p["window"])
    return tuple(torch.from_numpy(np.ascontiguousarray(k[:, lo:lo + win].T)) for k in (wcos, wsin))


def _mel(power, p):
    """(T, n_bins) power -> (n_mels, T): each mel filter as a chain of fused multiply-adds over its bins"""
    mb = torch.from_numpy(o_fbank.mel_basis(p["sr"], p["n_fft"], p["n_mels"], p["fmin"], p["fmax"]))
    acc = power.new_zeros(power.shape[0], mb.shape[0])
    for k in range(mb.shape[1]):
        acc = _fma(mb[:, k], power[:, k:k + 1], acc)
    return acc.T.contiguous()


def mel_emulated(wave, kstep=KSTEP_F32, pre_emphasis=True, **kw):
    """(L,) samples -> (n_mels, T) mel power in fp32 as the exact-fp32 form adds it up: the windowed DFT over the non-zero taps as one
    accumulator per bin along the taps, `kstep` products at a time (chained_matmul: the MFMA's k-order; torch's blocked conv1d sums sat
    2 x below the chain's error at TitaNet's prolog), sqrt(re^2 + im^2) squared, then the mel filters"""
    p = geometry(**kw)
    fr, lo = _frames(wave, p, pre_emphasis)
    wcos, wsin = _basis(p, lo)
    mm = chained_matmul(kstep)
    re, im = mm(fr, wcos), mm(fr, wsin)
    return _mel(torch.sqrt(re * re + im * im) ** 2.0, p)


def mel_emulated_split(wave, pre_emphasis=True, **kw):
    """(L,) samples -> (n_mels, T) mel power in fp32 as the bf16x3 form adds it up (a BF16 handle whose hop is a multiple of 8): the
    pre-emphasised samples and the windowed DFT basis split into bf16 hi + lo parts, per k step of 16 taps the products lo hi, hi lo and
    hi hi added to one fp32 accumulator per bin, |X|^2 as re^2 + im^2, then the mel filters.  The dropped lo lo term is 2^-16 of a
    product: after the log, 1e-4 in a mel bin with little energy, where the exact form keeps 1e-6"""
    p = geometry(**kw)
    win = p["win_length"]
    fr, lo = _frames(wave, p, pre_emphasis)
    fh = bf16_round(fr)
    fl = bf16_round(fr - fh)
    out = []
    for b in _basis(p, lo):
        bh = bf16_round(b)
        bl = bf16_round(b - bh)
        acc = torch.zeros(fr.shape[0], b.shape[1])
        for k0 in range(0, win, 16):
            sl = slice(k0, k0 + 16)
            acc.addmm_(fl[:, sl], bh[sl])
            acc.addmm_(fh[:, sl], bl[sl])
            acc.addmm_(fh[:, sl], bh[sl])
        out.append(acc)
    return _mel(out[0] * out[0] + out[1] * out[1], p)
