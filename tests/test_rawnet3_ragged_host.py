"""CPU: the host side of ragged RawNet3 / Raw3_ECAPA packs — the capacity and scope rules of svhip_rawnet3_embed_ragged
(svhip_rawnet3_ragged_check is that test without a handle), the frame formula against the oracle, the packer that plans both
branches of a fusion model at once, and which models whole-file evaluation sends down the ragged path."""
import ctypes

import numpy as np
import pytest

from oracle import rawnet3 as o_rn3
from speakerverification_amd import _lib, model as sv_model
from speakerverification_amd.models._fusion import RawECAPAFusion
from speakerverification_amd.ragged import FusionPacker, RaggedPacker, plan_packed, plan_ragged

INVALID = -1


def _len(T0, extra=3):
    """a waveform length with T0 frames after the sinc filterbank"""
    return 251 + 10 * (T0 - 1) + extra


def _cfg(**kw):
    cfg = _lib.default_config()
    cfg.model, cfg.max_batch, cfg.samples = _lib.MODEL_RAWNET3, 4, 8000       # T0 = 775: 3100 rows
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _check(cfg, lengths, n=None):
    lib = _lib.load()
    a = np.ascontiguousarray(lengths, dtype=np.int32)
    rc = lib.svhip_rawnet3_ragged_check(ctypes.byref(cfg), a.ctypes.data, len(a) if n is None else n)
    return rc, (lib.svhip_last_error(None) or b"").decode()


def test_rawnet3_ragged_check_capacity_and_scope():
    cfg = _cfg()
    assert o_rn3.frames(8000)[0] == 775
    assert _check(cfg, [_len(T) for T in (30, 45, 33, 2992)])[0] == 0            # fills the 3100 rows exactly
    assert sum(T // 15 for T in (30, 45, 33, 2992)) == 206 > 4 * (775 // 15)      # ... with more level-2 rows than max_batch * T2
    assert _check(cfg, [544])[0] == 0
    rc, msg = _check(cfg, [8000] * 5)
    assert rc == INVALID and "5 utterances" in msg and "max_batch=4" in msg
    rc, msg = _check(cfg, [8000], n=0)
    assert rc == INVALID and "max_batch=4" in msg
    rc, msg = _check(cfg, [8000, 540])
    assert rc == INVALID and "utterance 1" in msg and "541" in msg
    rc, msg = _check(cfg, [_len(T) for T in (30, 45, 34, 2992)])                  # 3101 frames
    assert rc == INVALID and "utterance 3" in msg and "3100" in msg
    rc, msg = _check(cfg, [_len(3101)])
    assert rc == INVALID and "utterance 0" in msg and "3100" in msg
    unsupported = _check(_cfg(compute=_lib.F32X3), [8000])[0]
    assert unsupported not in (0, INVALID)
    assert "SVHIP_F32" in _check(_cfg(compute=_lib.F32X3), [8000])[1]
    assert _check(_cfg(compute=_lib.F16), [8000])[0] == unsupported
    assert _check(_cfg(compute=_lib.BF16), [8000])[0] == 0
    for m in (_lib.MODEL_ECAPA, _lib.MODEL_RAWNET2, _lib.MODEL_RAWNET2_CONV, _lib.MODEL_RAWNET2_GRU, _lib.MODEL_TITANET,
              _lib.MODEL_CONFORMER, _lib.MODEL_RESNETSE, _lib.MODEL_NONE):
        rc, msg = _check(_cfg(model=m), [8000])
        assert rc == unsupported and "RAWNET3" in msg, (m, rc, msg)
    # the call itself and a bad config: no handle, nothing runs
    lib = _lib.load()
    assert lib.svhip_rawnet3_embed_ragged(None, None, None, None, 1, None, 0) == INVALID
    bad = _cfg()
    bad.struct_size = 4
    assert _check(bad, [8000])[0] == INVALID
    assert lib.svhip_abi_version() == 5


def test_frame_formula_matches_the_oracle():
    """the check counts an utterance's frames as the oracle does: for every L in 541 .. 600 a pack of that one utterance is accepted
    on a handle whose capacity is exactly its frames, and refused on one with a frame less"""
    for L in range(541, 601):
        T0 = o_rn3.frames(L)[0]
        assert _check(_cfg(max_batch=1, samples=_len(T0, 0)), [L])[0] == 0, L
        if T0 > 30:
            rc, msg = _check(_cfg(max_batch=1, samples=_len(T0 - 1, 9)), [L])
            assert rc == INVALID and f"= {T0 - 1} rows" in msg, (L, msg)


# ---- the fusion packer ----------------------------------------------------------------------------------------------------
class _FakeEngine:
    def __init__(self, max_batch, cap, dim):
        self.max_batch, self.row_capacity, self.embed_dim, self.calls = max_batch, cap, dim, []

    def _pack(self, items, offsets, lengths, is_wave):
        lens = np.asarray([len(a) for a in items], np.int32)
        return np.concatenate(items), np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), lens

    def embed_wave_ragged(self, packed, offsets=None, lengths=None, **kw):
        self.calls.append([int(n) for n in lengths])
        return np.stack([np.full(self.embed_dim, packed[o:o + n].sum(), np.float32) for o, n in zip(offsets, lengths)])


class _FakeBranch:
    """a branch with ECAPA's / RawNet3's ragged surface over a fake engine; `frames` maps samples to the branch's frames"""

    def __init__(self, max_batch, cap, dim, frames, min_frames):
        self.eng, self.frames, self.min_frames = _FakeEngine(max_batch, cap, dim), frames, min_frames

    def ragged_engine(self): return self.eng
    def ragged_packer(self): return RaggedPacker(self.eng.max_batch, self.eng.row_capacity, self.min_frames)
    def ragged_frames(self, n): return self.frames(n)
    def embed_ragged(self, wavs): raise AssertionError("the fusion plans its branches itself")


class _FakeFusion(RawECAPAFusion):
    def __init__(self, first, raw):
        self.ECAPA_TDNN, self.rawnet2v2 = first, raw


def _mel(n): return n // 80 + 1 if n >= 512 else 0
def _rn3(n): return (n - 251) // 10 + 1 if n >= 541 else 0


@pytest.mark.parametrize("caps,closes_on", [((4, 300, 8, 100000), "ecapa rows"), ((8, 100000, 8, 2000), "rawnet3 rows"),
                                            ((2, 100000, 8, 100000), "ecapa count"), ((8, 100000, 3, 100000), "rawnet3 count")])
def test_fusion_packer_closes_a_group_on_either_branch(caps, closes_on):
    mb1, cap1, mb2, cap2 = caps
    lens = [8000, 4000, 600, 9000, 540, 7000, 3000, 12000, 700, 50000, 8000]
    first, raw = _FakeBranch(mb1, cap1, 2, _mel, 5), _FakeBranch(mb2, cap2, 3, _rn3, 30)
    fus = _FakeFusion(first, raw)
    units = [fus.ragged_frames(n) for n in lens]
    assert units[0] == (101, 775) and units[4] == (7, 0)
    calls, alone = plan_packed(units, fus.ragged_packer())
    assert sorted(alone + [i for c in calls for i in c]) == list(range(len(lens)))      # every index exactly once
    assert 4 in alone                                                    # 540 samples: too short for RawNet3, so for the pair
    for c in calls:
        assert c == sorted(c)
        assert len(c) <= min(mb1, mb2)
        assert sum(units[i][0] for i in c) <= cap1 and sum(units[i][1] for i in c) <= cap2
    # greedy: a group was closed because its next utterance would have overflowed one of the branches
    for c, nxt in zip(calls[:-1], calls[1:]):
        i = nxt[0]
        over1 = len(c) + 1 > mb1 or sum(units[j][0] for j in c) + units[i][0] > cap1
        over2 = len(c) + 1 > mb2 or sum(units[j][1] for j in c) + units[i][1] > cap2
        assert over1 or over2
    # the limit named by the case is the one that binds somewhere, and the other branch alone would have packed differently
    other = plan_ragged([u[1] for u in units], mb2, cap2, 30) if "ecapa" in closes_on else plan_ragged([u[0] for u in units], mb1, cap1, 5)
    assert other[0] != calls
    # embed_ragged runs the same groups on both engines and concatenates first | raw
    wavs = [np.full(n, 1.0, np.float32) for i, n in enumerate(lens) if i not in alone]
    out = fus.embed_ragged(wavs)
    assert out.shape == (len(wavs), 5)
    assert np.array_equal(out[:, 0], [len(w) for w in wavs]) and np.array_equal(out[:, 0], out[:, 4])
    assert first.eng.calls == raw.eng.calls and [len(c) for c in first.eng.calls] == [len(c) for c in calls]
    with pytest.raises(ValueError):
        fus.embed_ragged([np.zeros(540, np.float32)])


def test_fusion_offers_the_ragged_path_only_when_both_branches_do():
    class _Plain:
        pass
    both = _FakeFusion(_FakeBranch(4, 100, 2, _mel, 5), _FakeBranch(4, 100, 3, _rn3, 30))
    assert hasattr(both, "embed_ragged") and hasattr(both, "ragged_packer") and hasattr(both, "ragged_frames")
    for fus in (_FakeFusion(_FakeBranch(4, 100, 2, _mel, 5), _Plain()), _FakeFusion(_Plain(), _FakeBranch(4, 100, 3, _rn3, 30))):
        assert not hasattr(fus, "embed_ragged") and not hasattr(fus, "ragged_packer") and not hasattr(fus, "ragged_frames")
    assert isinstance(both.ragged_packer(), FusionPacker)


# ---- ModelHandling._ragged_ok ----------------------------------------------------------------------------------------------
def _handling(S, features, fusable):
    enc = sv_model.SpeakerEncoder.__new__(sv_model.SpeakerEncoder)
    enc.model = {"name": "x", "nOut": 16}
    enc.criterion = {"name": "AAmSoftmaxAP"}
    enc.features = features
    enc.__S__ = S
    enc._fusable = lambda: fusable
    spec = {"sample_rate": 16000, "channels": 1, "sentence_len": 2.0, "win_len": 0.025, "hop_len": 0.01}
    return sv_model.ModelHandling(sv_model.WrappedModel(enc), audio_spec=spec, save_folder=".")


def test_ragged_ok_admits_raw_models_that_offer_embed_ragged():
    class _WithRagged:
        def embed_ragged(self, wavs): return None

    class _Without:
        pass
    # a `features: raw` model bakes its own front-end: the mel extractor's settings (_fusable) do not apply to it
    assert _handling(_WithRagged(), "raw", False)._ragged_ok(0)
    assert not _handling(_WithRagged(), "raw", False)._ragged_ok(2)
    assert not _handling(_Without(), "raw", True)._ragged_ok(0)
    assert _handling(_WithRagged(), "melspectrogram", True)._ragged_ok(0)
    assert not _handling(_WithRagged(), "melspectrogram", False)._ragged_ok(0)


def test_ragged_ok_by_model():
    """Raw3_ECAPA (ECAPA-TDNN + RawNet3) claims the ragged path; Raw_ECAPA_sinc_asp (RawNet2 branch) keeps the per-file one.  The
    modules are built without a device: only their attributes are read."""
    from speakerverification_amd.models import Raw3_ECAPA, Raw_ECAPA_sinc_asp
    kw = dict(n_mels=80, features="raw", audio_spec=dict(sample_rate=16000, sentence_len=2.0, win_len=0.025, hop_len=0.01, channels=1))
    assert _handling(Raw3_ECAPA.MainModel(nOut=512, **kw), "raw", True)._ragged_ok(0)
    assert not _handling(Raw_ECAPA_sinc_asp.MainModel(nOut=512, **kw), "raw", True)._ragged_ok(0)
