"""The mel front-end (csrc/fbank.hip) against the float64 oracle (oracle/fbank.py) at every geometry a handle accepts: the case table,
the inputs, the comparison and the bars of tests/test_gpu_fbank_geometry.py.  They need no GPU, so tests/test_fbank_geometry_host.py
runs the same comparison on the CPU emulations (tests/fbank_emulation.py) and checks the oracle itself away from the default geometry.

A case is a row of ROWS, a compute, a pre-emphasis and a waveform length.  What a handle runs for it (launch_fbank, restated in `route`):
the 64-frame kernel where the bank has at least 8 bin pairs, stops below bin 256 and its tile fits 80 KiB of LDS, the 32-frame kernel
otherwise (and with option fbank32); on a bf16 handle the bf16x3 form and on an f32x3 handle the six-product form where the hop is a
multiple of 8, the exact-fp32 form otherwise.

THE BARS are not taken from the GPU.  Compared are the two quantities of tests/test_gpu_fbank.py, per utterance: mel power relative to
the utterance's peak, and log(mel + 1e-6) minus its time mean.
  exact forms (f32, f32x3, and bf16 where hop % 8 != 0)
      power    max(2e-6, 3 x the float32 ORACLE's own error against the float64 oracle on the same input): both sides are fp32 sums of
               win_length products taken in different orders.  That error is 1.6e-7 .. 1.04e-6 over the table, largest at win 400 / 512.
      log-mel  1e-4, on the condition (asserted, so that an input is not blamed on the kernel) that the float32 oracle stays under 2.5e-5.
  bf16x3 form  3 x the CPU emulation's error (fbank_emulation.mel_emulated_split) on the same input; for the log-mel never above the
               5e-3 of test_fbank_bf16x3_split_path; for the power (impulses and tones are compared on power only, and
               tests/test_gpu_fbank.py states no bf16 power bar) never below the exact forms' 2e-6.
Impulse and tone inputs are compared on mel power only: after the log their empty bins compare log(1e-6) noise.

The values measured on the MI355X stand in MEASURED below; the GPU test prints every figure."""
import numpy as np
import torch

from oracle import fbank as o_fbank
from speakerverification_amd import synth
from tests import fbank_emulation as emu

COMPUTES = ("f32", "bf16", "f32x3")
POWER_FLOOR, LOG_BAR, LOG_ORACLE32_MAX, BF16_LOG_CAP = 2e-6, 1e-4, 2.5e-5, 5e-3
FRAME_COUNTS = (32, 33, 64, 65, 129)          # the last tile of both kernels full, one frame into the next, a second partial tile
F2_LDS_MAX = 80 * 1024                        # fbank.hip


def _row(name, sr, n_fft, win, hop, n_mels, fmin=0.0, fmax=None, pre=(True, 0.5)):
    return dict(name=name, pre=pre, kw=dict(sr=sr, n_fft=n_fft, win_length=win, hop_length=hop, n_mels=n_mels, fmin=fmin, fmax=fmax))


# what each row reaches is said in its name's comment; `pre`: the pre-emphases it runs with (every row also runs one with 0.5)
ROWS = (
    _row("default", 8000, 512, 200, 80, 80),                            # control: the geometry of tests/test_gpu_fbank.py
    _row("16k_512_400_160", 16000, 512, 400, 160, 80),                  # 64-frame kernel at 76.9 KB of LDS, a full last k step of 16
    _row("16k_400_400_160", 16000, 400, 400, 160, 80, 20.0, 7600.0, pre=(True, False, 0.5)),      # 7 pairs, lpad = 0, pre-emphasis off
    _row("16k_480_400_160_m64", 16000, 480, 400, 160, 64),              # 241 bins: 8 pairs, the last holds 17 bins, weight up to bin 239
    _row("8k_256_200_80_m40", 8000, 256, 200, 80, 40),                  # 5 pairs
    _row("8k_256_256_100", 8000, 256, 256, 100, 80),                    # hop % 8 != 0: bf16 / f32x3 handles on the exact-fp32 form
    _row("8k_512_8_4", 8000, 512, 8, 4, 80),                            # n_q = n_k16 = 1
    _row("8k_band_300_3400", 8000, 512, 200, 80, 80, 300.0, 3400.0),    # band-limited bank: top bin 217, the first filters start above bin 0
    _row("8k_64_64_16_m8", 8000, 64, 64, 16, 8),                        # 2 pairs, n_mels = 8
    _row("8k_574_400_84", 8000, 574, 400, 84, 80),                      # 288 bins, the largest n_fft: the 32-frame kernel at 9 full pairs
    _row("16k_256_200_80_m128", 16000, 256, 200, 80, 128),              # 13 empty mel filters
    _row("8k_128_128_32", 8000, 128, 128, 32, 80),                      # 3 empty mel filters
    _row("8k_512_512_400", 8000, 512, 512, 400, 80),                    # the 32-frame kernel at 90.7 KB of LDS
)
# refused when the handle is created (tests/test_gpu_fbank_geometry.py::test_create_refuses): a row with an odd n_fft.  The
# kernels' alignment would take it (the sample buffer's origin lpad - n_fft / 2 is any integer: the waveform is read sample by sample,
# the 16-byte LDS reads start at multiples of the hop); the frame count does not: the reference pads n_fft / 2 on both sides, n_fft - 1
# samples in all, and has (L - 1) / hop + 1 frames where every buffer of the library holds L / hop + 1.
ODD_ROW = _row("16k_401_400_160", 16000, 401, 400, 160, 80)
ROW = {r["name"]: r for r in ROWS}

# MEASURED[row, compute]: on the MI355X, the case of the row that came closest to its bar (the bars are per input), as (error, error / bar):
# power and log-mel of the noise inputs, `edges` the power of the impulses and the tone; option fbank32 included where it applies.
# A record, not a bar: nothing reads it.  (f32x3 rows equal the f32 rows where their worst case is the exact-fp32 form both run.)
MEASURED = {
    ("default", "f32"): dict(power=(7.31e-07, 0.37), edges=(5.04e-07, 0.25), logmel=(1.02e-05, 0.10)),
    ("default", "bf16"): dict(power=(1.59e-06, 0.44), edges=(1.12e-06, 0.36), logmel=(7.52e-05, 0.34)),
    ("default", "f32x3"): dict(power=(7.31e-07, 0.37), edges=(5.04e-07, 0.25), logmel=(1.02e-05, 0.10)),
    ("16k_512_400_160", "f32"): dict(power=(8.08e-07, 0.38), edges=(4.60e-07, 0.23), logmel=(1.95e-05, 0.20)),
    ("16k_512_400_160", "bf16"): dict(power=(3.97e-06, 0.36), edges=(9.13e-07, 0.40), logmel=(5.34e-05, 0.34)),
    ("16k_512_400_160", "f32x3"): dict(power=(8.08e-07, 0.38), edges=(4.60e-07, 0.23), logmel=(1.95e-05, 0.20)),
    ("16k_400_400_160", "f32"): dict(power=(9.87e-07, 0.38), edges=(7.55e-07, 0.38), logmel=(1.56e-05, 0.16)),
    ("16k_400_400_160", "bf16"): dict(power=(3.11e-06, 0.39), edges=(8.58e-07, 0.41), logmel=(1.87e-03, 0.37)),
    ("16k_400_400_160", "f32x3"): dict(power=(9.87e-07, 0.38), edges=(7.55e-07, 0.38), logmel=(1.56e-05, 0.16)),
    ("16k_480_400_160_m64", "f32"): dict(power=(7.90e-07, 0.38), edges=(6.31e-07, 0.31), logmel=(1.05e-05, 0.10)),
    ("16k_480_400_160_m64", "bf16"): dict(power=(1.49e-06, 0.52), edges=(9.04e-07, 0.43), logmel=(5.31e-05, 0.34)),
    ("16k_480_400_160_m64", "f32x3"): dict(power=(7.90e-07, 0.38), edges=(6.31e-07, 0.31), logmel=(1.05e-05, 0.10)),
    ("8k_256_200_80_m40", "f32"): dict(power=(9.53e-07, 0.38), edges=(5.43e-07, 0.27), logmel=(5.95e-06, 0.06)),
    ("8k_256_200_80_m40", "bf16"): dict(power=(3.73e-06, 0.38), edges=(9.54e-07, 0.43), logmel=(4.97e-05, 0.34)),
    ("8k_256_200_80_m40", "f32x3"): dict(power=(9.53e-07, 0.38), edges=(5.43e-07, 0.27), logmel=(5.95e-06, 0.06)),
    ("8k_256_256_100", "f32"): dict(power=(1.15e-06, 0.44), edges=(8.95e-07, 0.45), logmel=(2.07e-05, 0.21)),
    ("8k_256_256_100", "bf16"): dict(power=(1.15e-06, 0.44), edges=(8.95e-07, 0.45), logmel=(2.07e-05, 0.21)),
    ("8k_256_256_100", "f32x3"): dict(power=(1.15e-06, 0.44), edges=(8.95e-07, 0.45), logmel=(2.07e-05, 0.21)),
    ("8k_512_8_4", "f32"): dict(power=(2.34e-07, 0.12), edges=(1.99e-07, 0.10), logmel=(6.65e-06, 0.07)),
    ("8k_512_8_4", "bf16"): dict(power=(2.34e-07, 0.12), edges=(1.99e-07, 0.10), logmel=(6.65e-06, 0.07)),
    ("8k_512_8_4", "f32x3"): dict(power=(2.34e-07, 0.12), edges=(1.99e-07, 0.10), logmel=(6.65e-06, 0.07)),
    ("8k_band_300_3400", "f32"): dict(power=(7.81e-07, 0.39), edges=(2.49e-07, 0.12), logmel=(5.08e-06, 0.05)),
    ("8k_band_300_3400", "bf16"): dict(power=(3.21e-06, 0.35), edges=(1.01e-06, 0.37), logmel=(3.27e-05, 0.34)),
    ("8k_band_300_3400", "f32x3"): dict(power=(7.81e-07, 0.39), edges=(3.60e-07, 0.18), logmel=(5.08e-06, 0.05)),
    ("8k_64_64_16_m8", "f32"): dict(power=(4.23e-07, 0.21), edges=(5.48e-07, 0.27), logmel=(2.01e-06, 0.02)),
    ("8k_64_64_16_m8", "bf16"): dict(power=(3.05e-06, 0.36), edges=(2.09e-06, 0.36), logmel=(9.93e-06, 0.34)),
    ("8k_64_64_16_m8", "f32x3"): dict(power=(4.23e-07, 0.21), edges=(5.48e-07, 0.27), logmel=(2.01e-06, 0.02)),
    ("8k_574_400_84", "f32"): dict(power=(7.67e-07, 0.38), edges=(8.81e-07, 0.44), logmel=(1.08e-05, 0.11)),
    ("8k_574_400_84", "bf16"): dict(power=(7.67e-07, 0.38), edges=(8.81e-07, 0.44), logmel=(1.08e-05, 0.11)),
    ("8k_574_400_84", "f32x3"): dict(power=(7.67e-07, 0.38), edges=(8.81e-07, 0.44), logmel=(1.08e-05, 0.11)),
    ("16k_256_200_80_m128", "f32"): dict(power=(8.40e-07, 0.42), edges=(5.45e-07, 0.27), logmel=(1.72e-05, 0.17)),
    ("16k_256_200_80_m128", "bf16"): dict(power=(1.81e-06, 0.39), edges=(9.86e-07, 0.42), logmel=(2.54e-03, 0.51)),
    ("16k_256_200_80_m128", "f32x3"): dict(power=(8.40e-07, 0.42), edges=(5.45e-07, 0.27), logmel=(1.72e-05, 0.17)),
    ("8k_128_128_32", "f32"): dict(power=(8.28e-07, 0.33), edges=(5.89e-07, 0.29), logmel=(1.37e-05, 0.14)),
    ("8k_128_128_32", "bf16"): dict(power=(1.37e-06, 0.43), edges=(3.19e-06, 0.36), logmel=(1.79e-04, 0.34)),
    ("8k_128_128_32", "f32x3"): dict(power=(8.28e-07, 0.33), edges=(5.89e-07, 0.29), logmel=(1.37e-05, 0.14)),
    ("8k_512_512_400", "f32"): dict(power=(8.77e-07, 0.39), edges=(9.27e-07, 0.37), logmel=(1.00e-05, 0.10)),
    ("8k_512_512_400", "bf16"): dict(power=(8.78e-07, 0.43), edges=(1.13e-06, 0.55), logmel=(2.45e-05, 0.34)),
    ("8k_512_512_400", "f32x3"): dict(power=(8.77e-07, 0.39), edges=(9.27e-07, 0.37), logmel=(1.00e-05, 0.10)),
}


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def mel_table(kw):
    """(first bin, bin count) of every filter as build_fbank_tables packs them, from the oracle's bank"""
    mb = o_fbank.mel_basis(kw["sr"], kw["n_fft"], kw["n_mels"], kw["fmin"], kw["fmax"])
    out = []
    for w in mb:
        nz = np.flatnonzero(w)
        out.append((int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0))
    return out


def top_bin(kw):
    """the highest bin with mel weight (mel_max_bin)"""
    return max(s + n - 1 for s, n in mel_table(kw))


def empty_filters(kw):
    return sum(1 for _, n in mel_table(kw) if n == 0)


def split_form(kw, compute):
    """the bf16x3 / six-product forms need 16-byte aligned bf16 frame starts"""
    return compute in ("bf16", "f32x3") and kw["hop_length"] % 8 == 0


def route(kw, compute):
    """(frames per workgroup, dynamic LDS bytes) of launch_fbank's default choice, restated from fbank.hip"""
    n_melw = max(1, sum(n for _, n in mel_table(kw)))
    n_pairs = (kw["n_fft"] // 2 + 1 + 31) // 32
    pad = lambda ns: ((ns + 15) & ~15) + 16
    lds64 = (32 * 257 + n_melw) * 4 + pad(63 * kw["hop_length"] + kw["win_length"]) * (6 if compute == "f32x3" and split_form(kw, compute) else 4)
    if n_pairs >= 8 and top_bin(kw) < 256 and lds64 <= F2_LDS_MAX:
        return 64, lds64
    return 32, (pad(31 * kw["hop_length"] + kw["win_length"]) + 32 * 289 + n_melw) * 4


def lengths(kw):
    """the sample counts of a row: one FFT window (the fewest frames a handle takes), FRAME_COUNTS where they are no shorter than that,
    and one length that is no multiple of the hop"""
    n_fft, hop = kw["n_fft"], kw["hop_length"]
    ls = [n_fft] + [(T - 1) * hop for T in FRAME_COUNTS if (T - 1) * hop > n_fft]
    ragged = max(40 * hop, n_fft) + hop // 2 + 1
    assert ragged % hop
    return tuple(ls + [ragged])


def cases(row):
    """(pre-emphasis, L) of a row: every length with the row's first pre-emphasis, the others at the shortest length of more than 32
    frames and at the one that is no multiple of the hop"""
    kw = row["kw"]
    ls = lengths(kw)
    few = sorted({next((L for L in ls if L // kw["hop_length"] + 1 > 32), ls[-1]), ls[-1]})
    return tuple((row["pre"][0], L) for L in ls) + tuple((p, L) for p in row["pre"][1:] for L in few)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def noise(L):
    """(4, L): two white and two speech-like utterances (compared on power and on log-mel)"""
    return np.concatenate([synth.synth_waveforms(2, L, seed=20220829 + L), synth.synth_speechlike(2, L, seed=7 + L)])


def edges(L, kw):
    """(4, L): the three border impulses of test_fbank_edges_and_device (the reflect padding of n_fft / 2 and of the pre-emphasis) and
    a sine at the centre of the highest bin with mel weight: its energy lands in the last non-empty filter, which a kernel that drops
    or misplaces the last bin pair leaves at zero (compared on power only)"""
    w = np.zeros((4, L), np.float32)
    w[0, 0] = 1.0
    w[1, -1] = 1.0
    w[2, 1] = -0.5
    w[3] = 0.5 * np.sin(2.0 * np.pi * top_bin(kw) * np.arange(L) / kw["n_fft"])
    return w


_REF = {}


def reference(row, pre, L, kind):
    """{"wav", "ref64", "ref32", "peak", "lr", "pow32", "log32"} of a case's input, cached and never written to: the float64 and float32
    oracle, each utterance's peak mel power, the float64 log-mel and the float32 oracle's own errors per utterance"""
    key = (row["name"], pre, L, kind)
    if key not in _REF:
        kw = row["kw"]
        wav = noise(L) if kind == "noise" else edges(L, kw)
        x = torch.from_numpy(wav)
        ref64 = o_fbank.melspectrogram(emu.emphasised(x.double(), pre), pre_emph=False, **kw).numpy()
        ref32 = o_fbank.melspectrogram(emu.emphasised(x, pre), pre_emph=False, **kw).numpy()
        peak = np.abs(ref64).max(axis=(1, 2))
        peak[peak == 0.0] = 1.0               # (an impulse that no window reaches, where the hop is longer than the window: absolute)
        r = dict(wav=wav, ref64=ref64, ref32=ref32, peak=peak, lr=_logmel(ref64))
        r["pow32"], r["log32"] = _errs(ref32, r)
        for v in r.values():
            v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _logmel(mel):
    return o_fbank.log_mean_norm(torch.from_numpy(np.asarray(mel, np.float64))).numpy()


def _errs(got, r):
    """per utterance: (max |got - ref64| / peak, max |log-mel difference|)"""
    return (np.abs(got - r["ref64"]).max(axis=(1, 2)) / r["peak"], np.abs(_logmel(got) - r["lr"]).max(axis=(1, 2)))


_EMU = {}


def emulated(row, pre, L, kind):
    """the bf16x3 emulation's (power, log-mel) errors per utterance of a case's input, cached"""
    key = (row["name"], pre, L, kind)
    if key not in _EMU:
        r = reference(row, pre, L, kind)
        mel = np.stack([emu.mel_emulated_split(w, pre_emphasis=pre, **row["kw"]).numpy() for w in r["wav"]])
        assert np.isfinite(mel).all()
        _EMU[key] = _errs(mel, r)
    return _EMU[key]


def compare(got, row, compute, pre, L, kind):
    """[(what, utterance, error, bar)] of one result (4, n_mels, T) against the oracle, every entry to be printed and then held to
    error <= bar; the condition on the float32 oracle is an entry of its own"""
    kw = row["kw"]
    r = reference(row, pre, L, kind)
    assert got.shape == r["ref64"].shape, (got.shape, r["ref64"].shape)
    assert np.isfinite(got).all()
    e_pow, e_log = _errs(got, r)
    out = []
    if split_form(kw, compute) and compute == "bf16":
        m_pow, m_log = emulated(row, pre, L, kind)
        bar_pow = np.maximum(POWER_FLOOR, 3.0 * m_pow)
        bar_log = np.minimum(BF16_LOG_CAP, 3.0 * m_log)
    else:
        bar_pow = np.maximum(POWER_FLOOR, 3.0 * r["pow32"])
        bar_log = np.full(len(e_log), LOG_BAR)
    for b in range(got.shape[0]):
        out.append(("power", b, float(e_pow[b]), float(bar_pow[b])))
        if kind == "noise":
            out.append(("oracle32 log-mel", b, float(r["log32"][b]), LOG_ORACLE32_MAX))
            out.append(("log-mel", b, float(e_log[b]), float(bar_log[b])))
    return out


def top_filter_energy(row, pre, L):
    """the tone's share of its utterance's peak in the last non-empty filter of the float64 oracle, over the frames (the premise of the
    tone input: close to 1)"""
    r = reference(row, pre, L, "edges")
    last = max(m for m, (_, n) in enumerate(mel_table(row["kw"])) if n)
    return float(r["ref64"][3, last].max() / r["peak"][3])
