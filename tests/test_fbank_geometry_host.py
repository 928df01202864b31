"""CPU: the float64 oracle of the mel front-end (oracle/fbank.py) away from the default geometry, which is the only one frozen in
tests/golden/fbank.npz, and the premises of tests/fbank_geometry_check.py: its case table, and its bars on the CPU emulations of the
front-end's two forms at every row."""
import numpy as np
import pytest
import torch

from oracle import fbank as o_fbank
from tests import fbank_emulation as emu, fbank_geometry_check as chk

ALL_ROWS = chk.ROWS + (chk.ODD_ROW,)          # (the oracle takes an odd n_fft; a handle does not)


def _independent(wav, kw, pre):
    """(L,) samples -> (n_mels, T) mel power in float64, stated without the oracle's convolutions: pre-emphasis with the float32-rounded
    coefficient, np.pad(reflect) by n_fft // 2, frames at the hop, the float32-cast periodic Hamming window centred at
    (n_fft - win) // 2, np.fft.rfft, |.|^2, the oracle's mel_basis"""
    n_fft, win, hop = kw["n_fft"], kw["win_length"], kw["hop_length"]
    x = wav.astype(np.float64)
    if pre is not False and pre is not None:
        c = float(np.float32(0.97 if pre is True else pre))
        x = x - c * np.concatenate([x[1:2], x[:-1]])
    xp = np.pad(x, n_fft // 2, mode="reflect")
    T = (len(xp) - n_fft) // hop + 1
    w = np.zeros(n_fft)
    lo = (n_fft - win) // 2
    w[lo:lo + win] = (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(win) / win)).astype(np.float32)
    fr = np.stack([xp[t * hop:t * hop + n_fft] for t in range(T)]) * w
    power = np.abs(np.fft.rfft(fr, axis=1)) ** 2
    mb = o_fbank.mel_basis(kw["sr"], n_fft, kw["n_mels"], kw["fmin"], kw["fmax"]).astype(np.float64)
    return mb @ power.T


@pytest.mark.parametrize("row", ALL_ROWS, ids=lambda r: r["name"])
def test_oracle_matches_an_independent_float64_statement(row):
    """bar 2e-7 of the utterance's peak: the oracle, as nnAudio, casts its sin / cos kernels to float32, at most 2^-24 per tap on the
    amplitude and twice that on the power (measured 1.4e-8 .. 3.4e-8)"""
    kw = row["kw"]
    worst = 0.0
    for pre in row["pre"]:
        for L in (chk.lengths(kw)[0], chk.lengths(kw)[-1], 33 * kw["hop_length"] + kw["n_fft"]):
            for kind in ("noise", "edges"):
                wav = chk.noise(L) if kind == "noise" else chk.edges(L, kw)
                got = o_fbank.melspectrogram(emu.emphasised(torch.from_numpy(wav).double(), pre), pre_emph=False, **kw).numpy()
                for b in range(len(wav)):
                    ref = _independent(wav[b], kw, pre)
                    assert got[b].shape == ref.shape
                    worst = max(worst, float(np.abs(got[b] - ref).max() / np.abs(ref).max()))
    print(row["name"], "oracle against the independent statement, rel. to peak:", worst)
    assert worst <= 2e-7


def test_melspectrogram_pre_emphasis_keyword_is_the_emphasised_input():
    """the oracle's own pre-emphasis (0.97) and fbank_emulation.emphasised followed by pre_emph=False are the same numbers"""
    x = torch.from_numpy(chk.noise(2000)).double()
    a = o_fbank.melspectrogram(x)
    b = o_fbank.melspectrogram(emu.emphasised(x, True), pre_emph=False)
    assert torch.equal(a, b)


def test_case_table_reaches_what_it_says():
    """what the comments of chk.ROWS say of the rows, from the restated launcher (chk.route) and the oracle's bank"""
    top = {n: chk.top_bin(chk.ROW[n]["kw"]) for n in chk.ROW}
    assert top["16k_400_400_160"] == 189 and top["16k_480_400_160_m64"] == 239 and top["8k_band_300_3400"] == 217 and top["8k_574_400_84"] == 286
    assert top["default"] == 255 and chk.mel_table(chk.ROW["8k_band_300_3400"]["kw"])[0][0] > 0
    assert chk.empty_filters(chk.ROW["16k_256_200_80_m128"]["kw"]) == 13 and chk.empty_filters(chk.ROW["8k_128_128_32"]["kw"]) == 3
    assert all(chk.empty_filters(r["kw"]) == 0 for r in chk.ROWS if r["name"] not in ("16k_256_200_80_m128", "8k_128_128_32"))
    frames, lds = chk.route(chk.ROW["16k_512_400_160"]["kw"], "f32")
    assert frames == 64 and 64 * 1024 < lds <= 80 * 1024 and abs(lds - 76.9e3) < 500          # above the default limit of a launch
    assert chk.route(chk.ROW["16k_512_400_160"]["kw"], "f32x3")[0] == 32                       # six-product tile: 98 KB, over the 64-frame cap
    frames, lds = chk.route(chk.ROW["8k_512_512_400"]["kw"], "f32")
    assert frames == 32 and abs(lds - 90.7e3) < 500
    assert chk.route(chk.ROW["default"]["kw"], "f32")[0] == 64 and chk.route(chk.ROW["16k_480_400_160_m64"]["kw"], "bf16")[0] == 64
    for n in ("16k_400_400_160", "8k_256_200_80_m40", "8k_64_64_16_m8", "8k_574_400_84", "8k_128_128_32"):
        assert chk.route(chk.ROW[n]["kw"], "f32")[0] == 32, n                                   # fewer than 8 pairs, or weight at bin >= 256
    for r in chk.ROWS:
        kw = r["kw"]
        Ts = {L // kw["hop_length"] + 1 for L in chk.lengths(kw)}
        assert kw["n_fft"] // kw["hop_length"] + 1 in Ts and all(L >= kw["n_fft"] for L in chk.lengths(kw))
        assert {T for T in chk.FRAME_COUNTS if (T - 1) * kw["hop_length"] >= kw["n_fft"]} <= Ts
        assert any(L % kw["hop_length"] for L in chk.lengths(kw))
        assert 0.5 in r["pre"] and max(Ts) <= 129 + 1
        # the tone's energy lands in the last non-empty filter
        assert chk.top_filter_energy(r, r["pre"][0], chk.lengths(kw)[-1]) >= 0.5, r["name"]


@pytest.mark.parametrize("row", chk.ROWS, ids=lambda r: r["name"])
def test_emulations_meet_the_bars(row):
    """the exact-fp32 form's emulation under the bars of the exact forms, the float32 oracle under its condition, and the bf16x3 form's
    emulation finite and under the 5e-3 its bar never exceeds, at one length of more than 32 frames per pre-emphasis"""
    kw = row["kw"]
    for pre, L in chk.cases(row)[len(chk.lengths(kw)) - 1:]:
        for kind in ("noise", "edges"):
            r = chk.reference(row, pre, L, kind)
            mel = np.stack([emu.mel_emulated(w, pre_emphasis=pre, **kw).numpy() for w in r["wav"]])
            res = chk.compare(mel, row, "f32", pre, L, kind)
            for what, b, e, bar in res:
                print(row["name"], pre, L, kind, "fp32 emulation:", what, b, f"{e:.2e} (bar {bar:.2e})")
            assert all(e <= bar for _, _, e, bar in res), [x for x in res if not x[2] <= x[3]]
            if chk.split_form(kw, "bf16"):
                m_pow, m_log = chk.emulated(row, pre, L, kind)
                print(row["name"], pre, L, kind, "bf16x3 emulation: power", m_pow, "log-mel", m_log)
                assert np.isfinite(m_pow).all() and (kind != "noise" or (m_log <= chk.BF16_LOG_CAP).all())
