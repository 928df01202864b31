"""GPU: the mel front-end against the float64 oracle at every geometry a handle accepts (tests/fbank_geometry_check.py: the rows, the
inputs, the comparison, the bars and the measured values).  tests/test_gpu_fbank.py runs one geometry, 8 kHz / 512 / 200 / 80; here
are the 32-frame kernel as the kernel of record (fewer than 8 bin pairs, or mel weight at bin 256 and above), a partial last pair that
carries mel weight, window lengths from 8 to 512 taps (n_q and n_k16 from 1, a half and a full last k step), lpad = 0, a hop that is
a multiple of 4 only (bf16 and f32x3 handles on the exact-fp32 form), banks with fmin > 0, fmax < sr / 2 and empty filters,
pre-emphasis off and at 0.5, and the two geometries whose tiles need more than the 64 KiB of LDS a launch gets by default.

The rule: a geometry that create accepts is served within the bars; anything else is refused at create with a message that names it.

Per row and compute, every length of the row (one FFT window, 32 / 33 / 64 / 65 / 129 frames, one length that is no multiple of the
hop): two white and two speech-like utterances on mel power and log-mel, three border impulses and a tone in the highest weighted bin
on mel power; where the 64-frame kernel is the default also with option fbank32, bit for bit on the exact-fp32 form."""
import numpy as np
import pytest

from speakerverification_amd import _lib
from speakerverification_amd.engine import Engine
from tests import fbank_geometry_check as chk

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5        # include/svhip.h


def _engine(row, compute, L, pre=True, **over):
    kw = dict(row["kw"], **over)
    return Engine(model="none", compute=compute, max_batch=4, samples=L, pre_emphasis=pre, **kw)


@pytest.mark.parametrize("compute", chk.COMPUTES)
@pytest.mark.parametrize("row", chk.ROWS, ids=lambda r: r["name"])
def test_front_end_meets_the_oracle(row, compute):
    kw = row["kw"]
    frames, lds = chk.route(kw, compute)
    print(f"{row['name']} {compute}: {frames}-frame kernel, {lds} bytes of LDS, {'split' if chk.split_form(kw, compute) else 'exact-fp32'} form")
    bad, worst = [], {}
    for pre, L in chk.cases(row):
        eng = _engine(row, compute, L, pre)
        try:
            for kind in ("noise", "edges"):
                wav = np.array(chk.reference(row, pre, L, kind)["wav"])
                outs = [("", eng.fbank(wav))]
                if frames == 64:
                    eng.set_option("fbank32", 1)
                    outs.append(("fbank32", eng.fbank(wav)))
                    eng.set_option("fbank32", 0)
                    if not chk.split_form(kw, compute):           # the same taps in the same order: bit for bit
                        np.testing.assert_array_equal(outs[0][1], outs[1][1], err_msg=f"{row['name']} {compute} pre={pre} L={L} {kind}")
                for tag, got in outs:
                    for what, b, e, bar in chk.compare(got, row, compute, pre, L, kind):
                        print(f"{row['name']} {compute} pre={pre} L={L} T={L // kw['hop_length'] + 1} {kind}[{b}] {tag} {what}: {e:.3e} (bar {bar:.3e})")
                        if not what.startswith("oracle32"):
                            k = what + (" (edges)" if kind == "edges" else "")
                            worst[k] = max(worst.get(k, (0.0, 0.0)), (e / bar, e))
                        if not e <= bar:
                            bad.append((pre, L, kind, b, tag, what, e, bar))
        finally:
            eng.close()
    print(f"WORST {row['name']} {compute}: " + ", ".join(f"{k} {e:.2e} ({r:.2f} of its bar)" for k, (r, e) in sorted(worst.items())))
    assert not bad, bad


REFUSED = (
    ("win % 8 != 0", dict(win_length=204), ERR_UNSUPPORTED, "n_fft=512 win=204 hop=80"),
    ("hop % 4 != 0", dict(hop_length=82), ERR_UNSUPPORTED, "n_fft=512 win=200 hop=82"),
    ("win > n_fft", dict(n_fft=256, win_length=264), ERR_UNSUPPORTED, "n_fft=256 win=264 hop=80"),
    ("10 bin pairs", dict(n_fft=576), ERR_UNSUPPORTED, "n_fft=576 win=200 hop=80"),
    ("odd n_fft", dict(chk.ODD_ROW["kw"]), ERR_UNSUPPORTED, "n_fft=401 win=400 hop=160 not supported: n_fft must be even"),
    ("a tile beyond a workgroup's LDS", dict(hop_length=1400), ERR_UNSUPPORTED, "n_fft=512 win=200 hop=1400 n_mels=80 not supported: its tile needs"),
    ("samples < n_fft", dict(samples=511), ERR_INVALID, "samples"),
    ("n_mels % 8 != 0", dict(n_mels=60), ERR_INVALID, "n_mels"),
)


@pytest.mark.parametrize("compute", chk.COMPUTES)
@pytest.mark.parametrize("what,over,code,msg", REFUSED, ids=[r[0] for r in REFUSED])
def test_create_refuses(what, over, code, msg, compute):
    """what build_fbank_tables and svhip_create do not take is refused when the handle is created, by code and by a message that names
    the geometry; the same handle without the offending keyword is created"""
    over = dict(over)
    L = over.pop("samples", 4096)
    with pytest.raises(_lib.SvhipError, match=msg) as ei:
        _engine(chk.ROW["default"], compute, L, **over)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    _engine(chk.ROW["default"], compute, 4096).close()


@pytest.mark.parametrize("compute", chk.COMPUTES)
def test_a_long_hop_below_the_lds_limit_is_served(compute):
    """hop 800: the 32-frame kernel's tile is about 138 KB, the largest of this file and under a workgroup's 160 KiB (hop 1400 is refused
    above): served, one frame per 800 samples, within the bars"""
    row = dict(name="8k_512_200_800", pre=(True,), kw=dict(chk.ROW["default"]["kw"], hop_length=800))
    frames, lds = chk.route(row["kw"], compute)
    assert frames == 32 and 128 * 1024 < lds < 160 * 1024
    bad = []
    for L in (512, 32 * 800, 33 * 800 + 401):
        eng = _engine(row, compute, L)
        for kind in ("noise", "edges"):
            got = eng.fbank(np.array(chk.reference(row, True, L, kind)["wav"]))
            for what, b, e, bar in chk.compare(got, row, compute, True, L, kind):
                print(f"hop 800 {compute} L={L} {kind}[{b}] {what}: {e:.3e} (bar {bar:.3e})")
                if not e <= bar:
                    bad.append((L, kind, b, what, e, bar))
        eng.close()
    assert not bad, bad
