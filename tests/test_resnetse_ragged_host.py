"""CPU: the host side of ragged ResNetSE34V2 packs — the capacity rule of svhip_resnetse_embed_ragged (an utterance counts as its
frames rounded up to a multiple of 8; svhip_resnetse_ragged_check is that test without a handle) with the brute-force check that the
rule keeps every subsampled level within the handle's rows, the scope and argument refusals, the plug-in's planning
(ResNetSE.ragged_frames / ragged_packer / plan_ragged) against the library's own check, and whole-file evaluation's choice of path."""
import ctypes

import numpy as np
import pytest

from speakerverification_amd import _lib
from speakerverification_amd.models import ResNetSE34V2
from speakerverification_amd.ragged import plan_ragged
from tests.test_rawnet3_ragged_host import _handling
from tests.test_resnetse_host import KW
from tests.test_titanet_ragged_host import _cfg as _titanet_cfg

INVALID, UNSUPPORTED = -1, -5


def _cfg(**kw):
    cfg = _lib.default_config()
    cfg.model, cfg.channels, cfg.embed_dim, cfg.log_input, cfg.input_norm = _lib.MODEL_RESNETSE, 2, 256, 1, 1
    cfg.max_batch, cfg.samples = 4, 3120                    # T = 3120 / 80 + 1 = 40: 160 rows
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _check(cfg, lengths, is_wave=False, n=None):
    lib = _lib.load()
    a = np.ascontiguousarray(lengths, dtype=np.int32)
    rc = lib.svhip_resnetse_ragged_check(ctypes.byref(cfg), a.ctypes.data, len(a) if n is None else n, 1 if is_wave else 0)
    return rc, (lib.svhip_last_error(None) or b"").decode()


def _levels(T):
    """frames of an utterance at the four levels: Conv2d(3, stride 2, padding 1) and Conv2d(1, stride 2) leave ceil(P / 2)"""
    out = [T]
    for _ in range(3):
        out.append((out[-1] - 1) // 2 + 1)
    return out


def test_capacity_counts_an_utterance_in_groups_of_eight():
    cfg = _cfg()
    # 37 + 41 + 41 + 41 = 160 = max_batch * T frames, but 19 + 21 + 21 + 21 = 82 rows at level 1, over 4 * 20
    assert sum((37, 41, 41, 41)) == 160 and sum(_levels(T)[1] for T in (37, 41, 41, 41)) == 82 > 4 * _levels(40)[1]
    rc, msg = _check(cfg, [37, 41, 41, 41])
    assert rc == INVALID and "utterance 3" in msg and "160" in msg and "184" in msg, msg       # 40 + 48 + 48 + 48
    assert _check(cfg, [40, 40, 40, 40])[0] == 0
    assert _check(cfg, [33, 33, 33, 33])[0] == 0                          # 4 * 40 rows as counted
    rc, msg = _check(cfg, [40, 40, 40, 41])
    assert rc == INVALID and "utterance 3" in msg and "160" in msg and "168" in msg, msg
    assert _check(cfg, [160])[0] == 0
    rc, msg = _check(cfg, [161])
    assert rc == INVALID and "utterance 0" in msg and "160" in msg


@pytest.mark.parametrize("max_batch,T", [(4, 40), (4, 41), (3, 7), (16, 401), (5, 33)])
def test_admitted_packs_fit_every_level(max_batch, T):
    """brute force: random packs the rule admits never pass max_batch * P_l rows at any of the four levels; the library and the rule
    restated here agree on every pack drawn"""
    cfg = _cfg(max_batch=max_batch, samples=(T - 1) * 80 if (T - 1) * 80 >= 512 else T * 80 - 1)      # samples // 80 + 1 == T
    cap = [max_batch * p for p in _levels(T)]
    rng = np.random.default_rng(1000 * max_batch + T)
    admitted = 0
    for _ in range(400):
        n = int(rng.integers(1, max_batch + 1))
        hi = max(3, 2 * cap[0] // n)
        Ts = [int(v) for v in rng.integers(2, hi, size=n)]
        fits = sum(8 * -(-t // 8) for t in Ts) <= cap[0]
        assert (_check(cfg, Ts)[0] == 0) == fits, Ts
        if fits:
            admitted += 1
            for lv in range(4):
                assert sum(_levels(t)[lv] for t in Ts) <= cap[lv], (Ts, lv)
    assert admitted >= 40


def test_refusals_without_a_gpu():
    cfg = _cfg()
    rc, msg = _check(cfg, [40], n=0)
    assert rc == INVALID and "0 utterances" in msg and "max_batch=4" in msg
    rc, msg = _check(cfg, [8] * 5)                                        # n = max_batch + 1
    assert rc == INVALID and "5 utterances" in msg and "max_batch=4" in msg
    rc, msg = _check(cfg, [40, 1])                                        # InstanceNorm1d over one frame
    assert rc == INVALID and "utterance 1" in msg and "fewer than 2" in msg and "InstanceNorm1d" in msg
    assert _check(cfg, [2, 3])[0] == 0
    rc, msg = _check(cfg, [3120, 511], is_wave=True)                      # a waveform shorter than one FFT window
    assert rc == INVALID and "utterance 1" in msg and "511" in msg and "n_fft=512" in msg
    assert _check(cfg, [3120, 512], is_wave=True)[0] == 0                 # 512 samples: T = 7
    rc, msg = _check(cfg, [40, -3])
    assert rc == INVALID and "utterance 1" in msg and "-3" in msg
    for compute in (_lib.F32X3, _lib.F16):                                # an f32x3 handle's configuration
        rc, msg = _check(_cfg(compute=compute), [40])
        assert rc == UNSUPPORTED and "SVHIP_F32" in msg
    assert _check(_cfg(compute=_lib.BF16), [40])[0] == 0
    bad = _cfg()
    bad.struct_size = 4
    assert _check(bad, [40])[0] == INVALID
    lib = _lib.load()
    assert lib.svhip_resnetse_ragged_check(ctypes.byref(_cfg()), None, 1, 0) == INVALID
    # a NULL handle, and NULL pointers to the packed-convolution test export: refused before any HIP call
    assert lib.svhip_resnetse_embed_ragged(None, None, None, None, 1, None, 0, 1) == INVALID
    assert lib.svhip_resnetse_conv3x3_ragged(None, None, None, None, None, _lib.F32, None, 1, 5, 32, 32, 1, 0, 0, None) == INVALID
    assert lib.svhip_abi_version() == 5


def test_scope_both_ways():
    lib = _lib.load()
    for m in (_lib.MODEL_ECAPA, _lib.MODEL_RAWNET2, _lib.MODEL_RAWNET2_CONV, _lib.MODEL_RAWNET2_GRU, _lib.MODEL_RAWNET3, _lib.MODEL_CONFORMER,
              _lib.MODEL_TITANET, _lib.MODEL_NONE):
        rc, msg = _check(_cfg(model=m), [40])
        assert rc == UNSUPPORTED and "RESNETSE" in msg, (m, rc, msg)
    rc, msg = _check(_titanet_cfg(), [401])                               # a TitaNet configuration
    assert rc == UNSUPPORTED and "RESNETSE" in msg
    a = np.array([3120], np.int32)
    rs = _cfg()
    assert lib.svhip_titanet_ragged_check(ctypes.byref(rs), a.ctypes.data, 1, 1) == UNSUPPORTED
    assert "TITANET" in (lib.svhip_last_error(None) or b"").decode()
    assert lib.svhip_ragged_check(ctypes.byref(rs), a.ctypes.data, 1, 1) == UNSUPPORTED
    assert lib.svhip_rawnet3_ragged_check(ctypes.byref(rs), a.ctypes.data, 1) == UNSUPPORTED
    assert lib.svhip_rawnet2_ragged_check(ctypes.byref(rs), a.ctypes.data, 1) == UNSUPPORTED
    assert lib.svhip_conformer_ragged_check(ctypes.byref(rs), a.ctypes.data, 1, 1) == UNSUPPORTED


@pytest.mark.parametrize("compute,max_batch,enc", [("f32", 4, "ASP"), ("bf16", 3, "SAP"), ("f32", 32, "ASP")])
def test_plugin_planning_agrees_with_the_library(compute, max_batch, enc):
    """ragged_frames is 8 ceil(T / 8), and 0 exactly for the waveforms the library refuses alone for their length; every call
    plan_ragged forms for a seeded list of lengths passes the library's check, and a call was closed only where one more utterance would
    not have passed"""
    m = ResNetSE34V2.MainModel(nOut=256, encoder_type=enc, device="cpu", compute=compute, max_batch=max_batch, **KW)
    cfg = _cfg(max_batch=max_batch, samples=32000, compute=_lib.BF16 if compute == "bf16" else _lib.F32, channels=1 if enc == "SAP" else 2)
    mb, cap = m._ragged_geometry()[:2]
    assert (mb, cap) == (max_batch, max_batch * 401)
    assert len(m._engines) == 0                                            # (no handle was built for the geometry)
    assert hasattr(m, "embed_ragged") and m.MIN_FRAMES == 2
    assert [m.ragged_frames(L) for L in (0, 511, 512, 559, 560, 639, 640, 32000)] == [0, 0, 8, 8, 8, 8, 16, 408]
    rng = np.random.default_rng(7 + max_batch)
    edge = [0, 1, 511, 512, 80 * (cap - 8), 80 * (cap - 8) + 79, 80 * (cap - 1), 80 * cap, 80 * cap + 79]
    lens = edge + [int(v) for v in rng.integers(300, 80 * 900, size=120)] + [int(v) for v in rng.integers(300, 80 * (cap + 50), size=40)]
    packer = m.ragged_packer()
    assert packer.min_frames == 2 and packer.max_batch == max_batch and packer.row_capacity == cap
    frames = [m.ragged_frames(L) for L in lens]
    for L, f in zip(lens, frames):
        assert (f == 0) == (L < 512), (L, f)
        assert f in (0, 8 * -(-(L // 80 + 1) // 8))
        assert (f > 0 and packer.fits_alone(f)) == (_check(cfg, [L], is_wave=True)[0] == 0), (L, f)
    order = rng.permutation(len(lens))
    calls, alone = plan_ragged([frames[i] for i in order], mb, cap, min_frames=2)
    assert sorted(alone + [i for c in calls for i in c]) == list(range(len(lens)))
    assert all(_check(cfg, [lens[order[i]]], is_wave=True)[0] != 0 for i in alone) and len(calls) >= 3
    for c, nxt in zip(calls, calls[1:] + [None]):
        assert _check(cfg, [lens[order[i]] for i in c], is_wave=True)[0] == 0, c
        if nxt is not None:
            assert _check(cfg, [lens[order[i]] for i in c + nxt[:1]], is_wave=True)[0] == INVALID
    with pytest.raises(ValueError):
        m.embed_ragged([np.zeros(511, np.float32)])


def test_whole_file_evaluation_takes_the_ragged_path():
    m = ResNetSE34V2.MainModel(nOut=256, **KW)
    assert _handling(m, "melspectrogram", True)._ragged_ok(0)
    assert not _handling(m, "melspectrogram", True)._ragged_ok(2)          # crops of one length: the fixed-length call
    assert not _handling(m, "melspectrogram", False)._ragged_ok(0)         # a front-end the handle does not bake in
