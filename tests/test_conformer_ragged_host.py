"""CPU: the host side of ragged Conformer packs — the capacity and scope rules of svhip_conformer_embed_ragged
(svhip_conformer_ragged_check is that test without a handle), the bound the one sum rule puts on the subsampled level, and the
plug-in's planning (Conformer.ragged_frames / ragged_packer / plan_ragged) against the library's own check."""
import ctypes

import numpy as np
import pytest

from speakerverification_amd import _lib, synth
from speakerverification_amd.models import Conformer
from speakerverification_amd.ragged import plan_ragged

INVALID, UNSUPPORTED = -1, -5
KW = dict(n_mels=80, augment=False, augment_options={"augment_chain": []}, features="melspectrogram")


def _cfg(**kw):
    cfg = _lib.default_config()
    cfg.model, cfg.channels, cfg.embed_dim, cfg.input_norm = _lib.MODEL_CONFORMER, 256, 512, 1
    cfg.max_batch, cfg.samples = 4, 32000                   # T = 401: 1604 mel rows; one slice holds 4 x 99 = 396 subsampled frames
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _check(cfg, lengths, is_wave=False, n=None):
    lib = _lib.load()
    a = np.ascontiguousarray(lengths, dtype=np.int32)
    rc = lib.svhip_conformer_ragged_check(ctypes.byref(cfg), a.ctypes.data, len(a) if n is None else n, 1 if is_wave else 0)
    return rc, (lib.svhip_last_error(None) or b"").decode()


def test_conformer_ragged_check_capacity():
    cfg = _cfg()
    assert _check(cfg, [7, 11, 586, 1000])[0] == 0                       # sum T_i = max_batch * T = 1604 exactly
    assert _check(cfg, [401] * 4)[0] == 0
    rc, msg = _check(cfg, [7, 11, 587, 1000])                            # one frame more
    assert rc == INVALID and "utterance 3" in msg and "1604" in msg and "1605" in msg
    rc, msg = _check(cfg, [401], n=0)
    assert rc == INVALID and "0 utterances" in msg and "max_batch=4" in msg
    rc, msg = _check(cfg, [100] * 5)
    assert rc == INVALID and "5 utterances" in msg and "max_batch=4" in msg
    rc, msg = _check(cfg, [401, 6])
    assert rc == INVALID and "utterance 1" in msg and "fewer than 7" in msg
    assert _check(cfg, [7])[0] == 0
    rc, msg = _check(cfg, [32000, 511], is_wave=True)
    assert rc == INVALID and "utterance 1" in msg and "n_fft=512" in msg
    assert _check(cfg, [32000, 512], is_wave=True)[0] == 0               # T = 512 / 80 + 1 = 7, the shortest utterance a pack takes


def test_wave_lengths_count_frames_as_the_front_end_does():
    """T = L / hop + 1: the capacity is reached by the last sample that still gives max_batch * T frames"""
    cfg = _cfg()
    assert _check(cfg, [80 * 1603 + 79], is_wave=True)[0] == INVALID      # 1604 frames, T' = 400: over the slice's 396
    assert _check(cfg, [80 * 1202 + 79, 32000], is_wave=True)[0] == 0     # 1203 + 401 = 1604 frames
    rc, msg = _check(cfg, [80 * 1203, 32000], is_wave=True)               # one sample more: 1204 + 401
    assert rc == INVALID and "utterance 1" in msg and "1605" in msg


def test_conformer_ragged_check_position_and_slice_limits():
    big = _cfg(max_batch=128)                                            # 51328 mel rows; f32: 33 utterances per slice, 3267 frames
    assert _check(big, [4 * 3267 + 3])[0] == 0
    rc, msg = _check(big, [401, 4 * 3268 + 3])
    assert rc == INVALID and "utterance 1" in msg and "3268" in msg and "3267" in msg and "slice" in msg
    rc, msg = _check(big, [4 * 10001 + 3])                               # T' = 10001: the positional encoding's limit is named first
    assert rc == INVALID and "utterance 0" in msg and "10001" in msg and "10000" in msg
    small = _cfg()                                                       # 4 x 99 = 396 < (1604 - 3) / 4 = 400
    assert _check(small, [4 * 396 + 3])[0] == 0
    rc, msg = _check(small, [4 * 397 + 3])
    assert rc == INVALID and "397" in msg and "396" in msg and "slice" in msg
    bf = _cfg(max_batch=128, compute=_lib.BF16)                          # half the bytes per conv1 row: 67 utterances per slice
    assert _check(bf, [4 * 3268 + 3])[0] == 0


def test_conformer_ragged_check_scope():
    for compute in (_lib.F32X3, _lib.F16):
        rc, msg = _check(_cfg(compute=compute), [401])
        assert rc == UNSUPPORTED and "SVHIP_F32" in msg
    assert _check(_cfg(compute=_lib.BF16), [401])[0] == 0
    for m in (_lib.MODEL_ECAPA, _lib.MODEL_RAWNET2, _lib.MODEL_RAWNET2_CONV, _lib.MODEL_RAWNET2_GRU, _lib.MODEL_RAWNET3, _lib.MODEL_TITANET,
              _lib.MODEL_RESNETSE, _lib.MODEL_NONE):
        rc, msg = _check(_cfg(model=m), [401])
        assert rc == UNSUPPORTED and "CONFORMER" in msg, (m, rc, msg)
    # the call itself and a bad config: no handle, nothing runs
    lib = _lib.load()
    assert lib.svhip_conformer_embed_ragged(None, None, None, None, 1, None, 0, 1) == INVALID
    assert lib.svhip_conformer_attention_ragged(None, None, None, None, None, _lib.F32, None, 1, 8, None) == INVALID
    bad = _cfg()
    bad.struct_size = 4
    assert _check(bad, [401])[0] == INVALID
    assert lib.svhip_abi_version() == 5
    # the ECAPA and RawNet3 checks keep refusing a Conformer configuration
    a = np.array([32000], np.int32)
    assert lib.svhip_ragged_check(ctypes.byref(_cfg()), a.ctypes.data, 1, 1) == UNSUPPORTED
    assert lib.svhip_rawnet3_ragged_check(ctypes.byref(_cfg()), a.ctypes.data, 1) == UNSUPPORTED


def test_the_sum_rule_bounds_the_subsampled_rows():
    """over seeded random packs that pass the check: sum T'_i <= floor((max_batch * T - 3) / 4), the rows the block buffers hold —
    and some packs do pass max_batch * T'"""
    rng = np.random.default_rng(20220829)
    passed, over = 0, 0
    for trial in range(6000):
        B = int(rng.integers(1, 9))
        samples = int(rng.integers(8, 200)) * 80
        cfg = _cfg(max_batch=B, samples=samples)
        T = samples // 80 + 1
        n = int(rng.integers(1, B + 1))
        lens = rng.integers(7, max(8, 2 * (B * T) // n), size=n)
        if _check(cfg, lens)[0] != 0:
            continue
        passed += 1
        rows = int(sum(synth.conformer_frames(int(t)) for t in lens))
        assert rows <= (B * T - 3) // 4, (B, samples, lens)
        over += rows > B * synth.conformer_frames(T)
    print(f"{passed} packs passed the check, {over} of them hold more than max_batch * T' subsampled rows")
    assert passed >= 2000 and over >= 1


@pytest.mark.parametrize("compute,max_batch", [("f32", 4), ("bf16", 4), ("f32", 64)])
def test_plugin_planning_agrees_with_the_library(compute, max_batch):
    """ragged_frames says 0 exactly for the waveforms the library refuses alone; every call plan_ragged forms passes the library's
    check, and a call was closed only where one more utterance would not have passed"""
    m = Conformer.MainModel(nOut=512, device="cpu", compute=compute, max_batch=max_batch, **KW)
    cfg = _cfg(max_batch=max_batch, compute=_lib.BF16 if compute == "bf16" else _lib.F32)
    mb, cap, slice_limit = m._ragged_geometry()
    assert (mb, cap) == (max_batch, max_batch * 401)
    rng = np.random.default_rng(7 + max_batch)
    edge = [511, 512, 559, 560, 80 * (4 * slice_limit + 2), 80 * (4 * slice_limit + 3), 80 * (4 * slice_limit + 6), 80 * (4 * slice_limit + 7) - 1,
            80 * (cap - 1), 80 * (cap - 1) + 79, 80 * cap, 80 * (4 * 10000 + 6), 80 * (4 * 10001 + 2)]
    lens = edge + [int(v) for v in rng.integers(300, 80 * 900, size=120)] + [int(v) for v in rng.integers(300, 80 * (cap + 50), size=40)]
    packer = m.ragged_packer()
    assert packer.min_frames == 7 and packer.max_batch == max_batch and packer.row_capacity == cap
    frames = [m.ragged_frames(L) for L in lens]
    for L, f in zip(lens, frames):
        alone_ok = _check(cfg, [L], is_wave=True)[0] == 0
        assert (f > 0 and packer.fits_alone(f)) == alone_ok, (L, f)
        assert f in (0, L // 80 + 1)
    order = rng.permutation(len(lens))
    calls, alone = plan_ragged([frames[i] for i in order], mb, cap, min_frames=7)
    assert sorted(alone + [i for c in calls for i in c]) == list(range(len(lens)))
    assert all(_check(cfg, [lens[order[i]]], is_wave=True)[0] != 0 for i in alone) and len(calls) >= 3
    for c, nxt in zip(calls, calls[1:] + [None]):
        assert _check(cfg, [lens[order[i]] for i in c], is_wave=True)[0] == 0, c
        if nxt is not None:
            assert _check(cfg, [lens[order[i]] for i in c + nxt[:1]], is_wave=True)[0] == INVALID
    with pytest.raises(ValueError):
        m.embed_ragged([np.zeros(511, np.float32)])
