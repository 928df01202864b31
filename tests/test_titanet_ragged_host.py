"""CPU: the host side of ragged TitaNet / Tita_ECAPA packs — the capacity and scope rules of svhip_titanet_embed_ragged
(svhip_titanet_ragged_check is that test without a handle), the argument refusals of the two depthwise test exports, the plug-in's
planning (TitaNet.ragged_frames / ragged_packer / plan_ragged) against the library's own check, and which fusion models whole-file
evaluation sends down the ragged path."""
import ctypes

import numpy as np
import pytest

from speakerverification_amd import _lib
from speakerverification_amd.models import Raw_tita, Tita_ECAPA, TitaNet
from speakerverification_amd.ragged import FusionPacker, plan_ragged
from tests.test_rawnet3_ragged_host import _handling

INVALID, UNSUPPORTED = -1, -5
AUDIO_SPEC = dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1)
KW = dict(n_mels=80, features="raw", audio_spec=AUDIO_SPEC)


def _cfg(**kw):
    cfg = _lib.default_config()
    cfg.model, cfg.channels, cfg.embed_dim, cfg.log_input = _lib.MODEL_TITANET, 512, 320, 0
    cfg.max_batch, cfg.samples = 4, 32000                   # T = 401: 1604 rows
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _check(cfg, lengths, is_wave=False, n=None):
    lib = _lib.load()
    a = np.ascontiguousarray(lengths, dtype=np.int32)
    rc = lib.svhip_titanet_ragged_check(ctypes.byref(cfg), a.ctypes.data, len(a) if n is None else n, 1 if is_wave else 0)
    return rc, (lib.svhip_last_error(None) or b"").decode()


def test_titanet_ragged_check_capacity():
    cfg = _cfg()
    rc, msg = _check(cfg, [401], n=0)
    assert rc == INVALID and "0 utterances" in msg and "max_batch=4" in msg
    assert _check(cfg, [401] * 4)[0] == 0                                # n = max_batch
    rc, msg = _check(cfg, [100] * 5)                                     # n = max_batch + 1
    assert rc == INVALID and "5 utterances" in msg and "max_batch=4" in msg
    assert _check(cfg, [1, 2, 601, 1000])[0] == 0                        # sum T_i = max_batch * T = 1604 exactly
    rc, msg = _check(cfg, [1, 2, 602, 1000])                             # one frame more
    assert rc == INVALID and "utterance 3" in msg and "1604" in msg and "1605" in msg
    rc, msg = _check(cfg, [1605])
    assert rc == INVALID and "utterance 0" in msg and "1604" in msg
    assert _check(cfg, [1])[0] == 0                                      # T_i = 1 from features
    assert _check(cfg, [1, 1, 1, 1])[0] == 0
    rc, msg = _check(cfg, [401, 0])
    assert rc == INVALID and "utterance 1" in msg and "fewer than 1" in msg
    rc, msg = _check(cfg, [32000, 511], is_wave=True)                    # a wave shorter than one FFT window
    assert rc == INVALID and "utterance 1" in msg and "511" in msg and "n_fft=512" in msg
    assert _check(cfg, [32000, 512], is_wave=True)[0] == 0
    for is_wave in (False, True):                                        # a negative length
        rc, msg = _check(cfg, [401 if not is_wave else 32000, -3], is_wave=is_wave)
        assert rc == INVALID and "utterance 1" in msg and "-3" in msg, (is_wave, msg)
    # T = L / hop + 1, as the front-end counts: the last sample that still gives 1604 frames, and one more
    assert _check(cfg, [80 * 1202 + 79, 32000], is_wave=True)[0] == 0
    rc, msg = _check(cfg, [80 * 1203, 32000], is_wave=True)
    assert rc == INVALID and "utterance 1" in msg and "1605" in msg


def test_titanet_ragged_check_scope_both_ways():
    lib = _lib.load()
    for compute in (_lib.F32X3, _lib.F16):
        rc, msg = _check(_cfg(compute=compute), [401])
        assert rc == UNSUPPORTED and "SVHIP_F32" in msg
    assert _check(_cfg(compute=_lib.BF16), [401])[0] == 0
    for channels in (256, 1024):
        assert _check(_cfg(channels=channels), [401, 3])[0] == 0
    for m in (_lib.MODEL_ECAPA, _lib.MODEL_RAWNET2, _lib.MODEL_RAWNET2_CONV, _lib.MODEL_RAWNET2_GRU, _lib.MODEL_RAWNET3, _lib.MODEL_CONFORMER,
              _lib.MODEL_RESNETSE, _lib.MODEL_NONE):
        rc, msg = _check(_cfg(model=m), [401])
        assert rc == UNSUPPORTED and "TITANET" in msg, (m, rc, msg)
    # the three existing checks keep refusing a TitaNet configuration
    a = np.array([32000], np.int32)
    assert lib.svhip_ragged_check(ctypes.byref(_cfg()), a.ctypes.data, 1, 1) == UNSUPPORTED
    assert lib.svhip_rawnet3_ragged_check(ctypes.byref(_cfg()), a.ctypes.data, 1) == UNSUPPORTED
    assert lib.svhip_conformer_ragged_check(ctypes.byref(_cfg()), a.ctypes.data, 1, 1) == UNSUPPORTED
    bad = _cfg()
    bad.struct_size = 4
    assert _check(bad, [401])[0] == INVALID
    assert lib.svhip_titanet_ragged_check(ctypes.byref(_cfg()), None, 1, 0) == INVALID
    assert lib.svhip_abi_version() == 5


def test_null_arguments_launch_nothing():
    """a NULL handle, and NULL pointers to the two depthwise exports: SVHIP_ERR_INVALID before any HIP call (this test has no GPU)"""
    lib = _lib.load()
    assert lib.svhip_titanet_embed_ragged(None, None, None, None, 1, None, 0, 1) == INVALID
    assert lib.svhip_titanet_embed_ragged(None, None, None, None, 1, None, 0, 0) == INVALID
    for compute in (_lib.F32, _lib.BF16):
        for k in (3, 7, 11):
            assert lib.svhip_titanet_depthwise(None, None, None, None, None, None, None, None, compute, k, 1, 8, 64, None) == INVALID
            assert lib.svhip_titanet_depthwise_ragged(None, None, None, None, None, None, None, None, compute, k, None, 1, 8, 64, None) == INVALID
    # a non-NULL x with everything else NULL, and a non-NULL table with NULL activations
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.svhip_titanet_depthwise(p, None, None, None, None, None, None, None, _lib.F32, 3, 1, 1, 8, None) == INVALID
    assert lib.svhip_titanet_depthwise_ragged(p, None, None, None, None, None, None, None, _lib.F32, 3, p, 1, 1, 8, None) == INVALID
    assert lib.svhip_titanet_depthwise_ragged(None, None, None, None, None, None, None, None, _lib.F32, 3, p, 1, 1, 8, None) == INVALID
    # bad k / compute / C with NULL pointers
    assert lib.svhip_titanet_depthwise(None, None, None, None, None, None, None, None, _lib.F32, 5, 1, 8, 64, None) == INVALID
    assert lib.svhip_titanet_depthwise(None, None, None, None, None, None, None, None, _lib.F16, 3, 1, 8, 64, None) == INVALID
    assert lib.svhip_titanet_depthwise_ragged(None, None, None, None, None, None, None, None, _lib.F32X3, 3, p, 1, 8, 64, None) == INVALID


@pytest.mark.parametrize("compute,max_batch,size", [("f32", 4, "m"), ("bf16", 4, "l"), ("f32", 64, "s")])
def test_plugin_planning_agrees_with_the_library(compute, max_batch, size):
    """ragged_frames says 0 exactly for the waveforms the library refuses alone; every call plan_ragged forms for a seeded list of
    lengths passes the library's check, and a call was closed only where one more utterance would not have passed"""
    m = TitaNet.MainModel(nOut=320, model_size=size, device="cpu", compute=compute, max_batch=max_batch, **KW)
    cfg = _cfg(max_batch=max_batch, compute=_lib.BF16 if compute == "bf16" else _lib.F32, channels={"s": 256, "m": 512, "l": 1024}[size])
    mb, cap = m._ragged_geometry()[:2]
    assert (mb, cap) == (max_batch, max_batch * 401)
    assert len(m._engines) == 0                                                          # (no handle was built for the geometry)
    rng = np.random.default_rng(11 + max_batch)
    edge = [0, 1, 511, 512, 559, 560, 80 * (cap - 1), 80 * (cap - 1) + 79, 80 * cap, 80 * cap + 79]
    lens = edge + [int(v) for v in rng.integers(300, 80 * 900, size=120)] + [int(v) for v in rng.integers(300, 80 * (cap + 50), size=40)]
    packer = m.ragged_packer()
    assert packer.min_frames == 1 and packer.max_batch == max_batch and packer.row_capacity == cap
    frames = [m.ragged_frames(L) for L in lens]
    for L, f in zip(lens, frames):
        alone_ok = _check(cfg, [L], is_wave=True)[0] == 0
        assert (f == 0) == (L < 512), (L, f)
        assert (f > 0 and packer.fits_alone(f)) == alone_ok, (L, f)
        assert f in (0, L // 80 + 1)
    order = rng.permutation(len(lens))
    calls, alone = plan_ragged([frames[i] for i in order], mb, cap, min_frames=1)
    assert sorted(alone + [i for c in calls for i in c]) == list(range(len(lens)))
    assert all(_check(cfg, [lens[order[i]]], is_wave=True)[0] != 0 for i in alone) and len(calls) >= 3
    for c, nxt in zip(calls, calls[1:] + [None]):
        assert _check(cfg, [lens[order[i]] for i in c], is_wave=True)[0] == 0, c
        if nxt is not None:
            assert _check(cfg, [lens[order[i]] for i in c + nxt[:1]], is_wave=True)[0] == INVALID
    with pytest.raises(ValueError):
        m.embed_ragged([np.zeros(511, np.float32)])


class _PrimaryHandle:
    """stands in for the ECAPA branch's primary handle, which its ragged_packer / ragged_frames read (there is no GPU to create one
    on): max_batch x 401 rows, the mel front-end's frame count"""
    max_batch, row_capacity, cfg = 256, 256 * 401, type("cfg", (), {"n_fft": 512})

    def frames_of(self, n):
        return n // 80 + 1


def test_fusions_offer_the_ragged_path_only_with_two_ragged_branches():
    te = Tita_ECAPA.MainModel(nOut=512, **KW)
    assert hasattr(te, "embed_ragged") and hasattr(te, "ragged_frames") and hasattr(te, "ragged_packer")
    te.ECAPA_TDNN.ragged_engine = lambda: _PrimaryHandle()
    packer = te.ragged_packer()
    assert isinstance(packer, FusionPacker)
    assert te.ragged_frames(32000) == (401, 401) and te.ragged_frames(511) == (0, 0) and te.ragged_frames(512) == (7, 7)
    assert len(te.titaNet._engines) == 0                                  # (TitaNet's own geometry needs no handle)
    rt = Raw_tita.MainModel(nOut=512, **KW)
    assert not hasattr(rt, "embed_ragged") and not hasattr(rt, "ragged_packer") and not hasattr(rt, "ragged_frames")
    assert hasattr(rt.titaNet, "embed_ragged")                            # (its TitaNet branch alone has one: RawNet2 does not)
    # whole-file evaluation: ModelHandling._ragged_ok
    assert _handling(TitaNet.MainModel(nOut=320, model_size="m", **KW), "raw", True)._ragged_ok(0)
    assert _handling(te, "raw", True)._ragged_ok(0)
    assert not _handling(te, "raw", True)._ragged_ok(2)
    assert not _handling(rt, "raw", True)._ragged_ok(0)
