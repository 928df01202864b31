"""CPU: the host side of ragged RawNet2 'conv' / Raw_ECAPA_conv_asp packs — the capacity and scope rules of svhip_rawnet2_embed_ragged
(svhip_rawnet2_ragged_check is that test without a handle), which models offer the ragged path, the plan both branches of the
fusion model share, and the fp16 range fallback on the ragged path, alone and driven by the fusion model."""
import ctypes
import warnings

import numpy as np
import pytest

from speakerverification_amd import _lib
from speakerverification_amd.models import (Raw_ECAPA, Raw_ECAPA_conv_asp, Raw_ECAPA_sinc_asp, Raw_ECAPA_sinc_gru, Raw_tita,
                                            RawNet2_custom)
from speakerverification_amd.ragged import FusionPacker, plan_packed
from tests.test_rawnet3_ragged_host import _FakeBranch, _FakeEngine, _FakeFusion, _handling, _mel

INVALID = -1
PACK_A = (729, 2188, 730, 7017)         # T1 per utterance: 10 664 rows, the capacity of a samples = 8000, max_batch = 4 handle
PROBES = (1297, 1325)                   # T1 of the batch-invariance probes of tests/test_gpu_rawnet2_ragged.py
SLICE = 48                              # RN_RAG_SLICE (kernels.h): the pooled frames of one slice of the ragged block tail
KW = dict(n_mels=80, features="raw", audio_spec=dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1))


def _cfg(**kw):
    cfg = _lib.default_config()
    cfg.model, cfg.max_batch, cfg.samples = _lib.MODEL_RAWNET2_CONV, 4, 8000       # T1 = 2666: 10 664 rows
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _check(cfg, lengths, n=None, export="svhip_rawnet2_ragged_check", extra=()):
    lib = _lib.load()
    a = np.ascontiguousarray(lengths, dtype=np.int32)
    rc = getattr(lib, export)(ctypes.byref(cfg), a.ctypes.data, len(a) if n is None else n, *extra)
    return rc, (lib.svhip_last_error(None) or b"").decode()


def levels(T1):
    """frames of an utterance at the seven levels"""
    out = [T1]
    for _ in range(6):
        out.append(out[-1] // 3)
    return out


def test_probe_lengths_sit_on_the_slice_limit():
    """the first probe has whole slices at the levels the tails of blocks 0 - 2 write, the second is one frame into a new slice at the
    same levels; both leave one frame at the aggregation, and pack A's levels are the ones its test names"""
    a, b = (levels(T) for T in PROBES)
    assert a == [1297, 432, 144, 48, 16, 5, 1] and b == [1325, 441, 147, 49, 16, 5, 1]
    assert [n % SLICE for n in a[1:4]] == [0, 0, 0] and a[3] == SLICE and b[3] == SLICE + 1 and all(n % SLICE for n in b[1:4])
    assert levels(2188)[1:] == [729, 243, 81, 27, 9, 3] and levels(7017)[1:] == [2339, 779, 259, 86, 28, 9]
    assert [n % 3 for n in levels(7017)[:6]] == [0, 2, 2, 1, 2, 1]


def test_rawnet2_ragged_check_capacity_and_scope():
    cfg = _cfg()
    assert sum(PACK_A) == 4 * (8000 // 3) == 10664
    assert _check(cfg, [3 * T + x for T, x in zip(PACK_A, (0, 1, 2, 1))])[0] == 0       # fills the capacity exactly
    assert sum(T // 729 for T in PACK_A) == 14 > 4 * (2666 // 729)                       # ... with more last-level rows than max_batch * tf
    rc, msg = _check(cfg, [3 * T for T in (729, 2188, 731, 7017)])                       # one row over
    assert rc == INVALID and "utterance 3" in msg and "10664" in msg, msg
    rc, msg = _check(cfg, [3 * 10665])
    assert rc == INVALID and "utterance 0" in msg and "10664" in msg
    assert _check(cfg, [2187])[0] == 0
    rc, msg = _check(cfg, [8000, 2186])
    assert rc == INVALID and "utterance 1" in msg and "2187" in msg
    rc, msg = _check(cfg, [8000], n=0)
    assert rc == INVALID and "max_batch=4" in msg
    rc, msg = _check(cfg, [8000] * 5)
    assert rc == INVALID and "5 utterances" in msg and "max_batch=4" in msg
    rc, msg = _check(_cfg(samples=2186), [2187])
    assert rc == INVALID and "2187" in msg
    unsupported, msg = _check(_cfg(compute=_lib.F32X3), [8000])
    assert unsupported not in (0, INVALID) and "SVHIP_F16" in msg and "RAWNET2_CONV" in msg
    for compute in (_lib.F32, _lib.BF16, _lib.F16):
        assert _check(_cfg(compute=compute), [8000])[0] == 0
    for m in (_lib.MODEL_ECAPA, _lib.MODEL_RAWNET2, _lib.MODEL_RAWNET2_GRU, _lib.MODEL_RAWNET3, _lib.MODEL_TITANET, _lib.MODEL_CONFORMER,
              _lib.MODEL_RESNETSE, _lib.MODEL_NONE):
        rc, msg = _check(_cfg(model=m), [8000])
        assert rc == unsupported and "RAWNET2_CONV" in msg, (m, rc, msg)
        assert ("LayerNorm(nb_samp)" in msg) == (m in (_lib.MODEL_RAWNET2, _lib.MODEL_RAWNET2_GRU)), (m, msg)
    # the four older exports refuse a RawNet2 'conv' configuration by their own names, and F16 as before
    for export, extra, name in (("svhip_ragged_check", (1,), "ECAPA"), ("svhip_rawnet3_ragged_check", (), "RAWNET3"),
                                ("svhip_conformer_ragged_check", (1,), "CONFORMER"), ("svhip_titanet_ragged_check", (1,), "TITANET")):
        rc, msg = _check(cfg, [8000], export=export, extra=extra)
        assert rc == unsupported and name in msg, (export, rc, msg)
    rc, msg = _check(_cfg(model=_lib.MODEL_RAWNET3, compute=_lib.F16), [8000], export="svhip_rawnet3_ragged_check")
    assert rc == unsupported and "SVHIP_F32 or SVHIP_BF16 only" in msg
    lib = _lib.load()
    assert lib.svhip_rawnet2_embed_ragged(None, None, None, None, 1, None, 0) == INVALID
    bad = _cfg()
    bad.struct_size = 4
    assert _check(bad, [8000])[0] == INVALID
    assert lib.svhip_abi_version() == 5


def test_only_the_conv_front_end_offers_the_ragged_path():
    conv = RawNet2_custom.MainModel(nOut=320, front_proc="conv", aggregate="asp", att_dim=128)
    assert all(hasattr(conv, a) for a in ("embed_ragged", "ragged_packer", "ragged_frames"))
    assert conv.MIN_FRAMES == 729
    assert [conv.ragged_frames(n) for n in (0, 2186, 2187, 2189, 2190, 32000)] == [0, 0, 729, 729, 730, 10666]
    assert len(conv._engines) == 0                                           # (the frame count needs no handle)
    for kw in (dict(front_proc="sinc", aggregate="asp", att_dim=128), dict(front_proc="sinc", aggregate="gru"), dict()):
        m = RawNet2_custom.MainModel(nOut=320, **kw)
        assert not hasattr(m, "embed_ragged") and not hasattr(m, "ragged_packer") and not hasattr(m, "ragged_frames"), kw
    fus = Raw_ECAPA_conv_asp.MainModel(nOut=512, **KW)
    assert all(hasattr(fus, a) for a in ("embed_ragged", "ragged_packer", "ragged_frames"))
    assert _handling(fus, "raw", True)._ragged_ok(0) and not _handling(fus, "raw", True)._ragged_ok(2)
    assert _handling(conv, "raw", True)._ragged_ok(0)
    for mod in (Raw_ECAPA, Raw_ECAPA_sinc_asp, Raw_ECAPA_sinc_gru, Raw_tita):
        m = mod.MainModel(nOut=512, **KW)
        assert not hasattr(m, "embed_ragged") and not hasattr(m, "ragged_packer") and not hasattr(m, "ragged_frames"), mod.__name__
        assert not _handling(m, "raw", True)._ragged_ok(0), mod.__name__


def _rn2(n): return n // 3 if n >= 2187 else 0


@pytest.mark.parametrize("caps,closes_on", [((4, 300, 8, 10 ** 6), "ecapa rows"), ((8, 10 ** 5, 8, 9000), "rawnet2 rows"),
                                            ((2, 10 ** 5, 8, 10 ** 6), "ecapa count"), ((8, 10 ** 5, 3, 10 ** 6), "rawnet2 count")])
def test_one_plan_for_both_branches_closes_on_either(caps, closes_on):
    mb1, cap1, mb2, cap2 = caps
    lens = [8000, 4000, 2200, 9000, 2186, 7000, 3000, 12000, 2500, 20000, 8000]
    first, raw = _FakeBranch(mb1, cap1, 2, _mel, 5), _FakeBranch(mb2, cap2, 3, _rn2, 729)
    fus = _FakeFusion(first, raw)
    units = [fus.ragged_frames(n) for n in lens]
    assert units[0] == (101, 2666) and units[4] == (28, 0)
    assert isinstance(fus.ragged_packer(), FusionPacker)
    calls, alone = plan_packed(units, fus.ragged_packer())
    assert sorted(alone + [i for c in calls for i in c]) == list(range(len(lens))) and 4 in alone
    for c in calls:
        assert len(c) <= min(mb1, mb2) and sum(units[i][0] for i in c) <= cap1 and sum(units[i][1] for i in c) <= cap2
    for c, nxt in zip(calls[:-1], calls[1:]):          # greedy: a group closed because its next utterance overflowed one branch
        i = nxt[0]
        over1 = len(c) + 1 > mb1 or sum(units[j][0] for j in c) + units[i][0] > cap1
        over2 = len(c) + 1 > mb2 or sum(units[j][1] for j in c) + units[i][1] > cap2
        assert over1 or over2
    wavs = [np.full(n, 1.0, np.float32) for i, n in enumerate(lens) if i not in alone]
    out = fus.embed_ragged(wavs)
    assert out.shape == (len(wavs), 5) and np.array_equal(out[:, 0], [len(w) for w in wavs]) and np.array_equal(out[:, 0], out[:, 4])
    assert first.eng.calls == raw.eng.calls and [len(c) for c in first.eng.calls] == [len(c) for c in calls]


class _RangeEngine(_FakeEngine):
    """a fake handle of one compute; `fail_on`: the index of the ragged call that reports an fp16 overflow (once)"""

    def __init__(self, compute, fail_on=None):
        super().__init__(4, 4 * 2666, 3)
        self.compute, self.fail_on, self.synced = compute, fail_on, 0

    def embed_wave_ragged(self, packed, offsets=None, lengths=None, out=None, **kw):
        if offsets is None:
            packed, offsets, lengths = self._pack(packed, None, None, True)
        k = len(self.calls)
        res = super().embed_wave_ragged(packed, offsets, lengths)
        if k == self.fail_on:
            raise _lib.SvhipNumericError(_lib.ERR_NONFINITE, "3 embedding value(s) are not finite")
        return res

    def synchronize(self):
        self.synced += 1

    def close(self):
        pass


def _conv_with_fake_handles(fail_on, **kw):
    m = RawNet2_custom.MainModel(nOut=3, front_proc="conv", aggregate="asp", att_dim=128, hip_compute="half", embed_batch=4, **kw)
    built = []

    def get_engine(samples, stream=None, batch=None):
        if not built or built[-1].compute != m._compute:
            built.append(_RangeEngine(m._compute, fail_on if not built else None))
        return built[-1]
    m._get_engine = get_engine
    return m, built


def test_the_fp16_fallback_covers_the_ragged_calls():
    lens = [8000, 9000, 6000, 12000, 5000, 30000, 2187]           # four calls of a 10 664-row handle: [0 1 2] [3 4] [5] [6]
    wavs = [np.full(n, float(i + 1), np.float32) for i, n in enumerate(lens)]
    m, built = _conv_with_fake_handles(fail_on=1)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        out = m.embed_ragged(wavs)
    seen = [w for w in seen if issubclass(w.category, RuntimeWarning)]
    assert len(seen) == 1 and "'f32'" in str(seen[0].message)
    assert [e.compute for e in built] == ["f16", "f32"] and m._compute == "f32"
    assert len(built[0].calls) == 2 and built[1].calls[0] == built[0].calls[1]          # the failed call, redone on the fallback handle
    assert sum(len(c) for c in built[0].calls[:1] + built[1].calls) == len(lens)
    assert np.array_equal(out[:, 0], [float(i + 1) * n for i, n in enumerate(lens)])      # file order
    # without a fallback compute the report is the caller's
    m2, built2 = _conv_with_fake_handles(fail_on=0, range_fallback=None)
    with pytest.raises(_lib.SvhipNumericError):
        m2.embed_ragged(wavs[:2])
    assert [e.compute for e in built2] == ["f16"]


def test_the_fusion_drives_the_raw_branch_through_its_fallback():
    lens = [8000, 9000, 6000, 12000, 5000]
    wavs = [np.full(n, float(i + 1), np.float32) for i, n in enumerate(lens)]
    raw, built = _conv_with_fake_handles(fail_on=1)
    first = _FakeBranch(4, 10 ** 6, 2, _mel, 5)
    fus = _FakeFusion(first, raw)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        out = fus.embed_ragged(wavs)
    assert len([w for w in seen if issubclass(w.category, RuntimeWarning)]) == 1
    assert [e.compute for e in built] == ["f16", "f32"]
    assert first.eng.calls == built[0].calls and built[1].calls == built[0].calls[1:2]
    assert out.shape == (5, 5) and np.array_equal(out[:, 0], [float(i + 1) * n for i, n in enumerate(lens)])
    assert np.array_equal(out[:, 0], out[:, 4])
