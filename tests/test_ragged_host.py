"""CPU: the host side of ragged batches — the planner that cuts a list of utterances into library calls, whole-file evaluation
(`_embed_files(num_eval=0)`) riding on it, and the argument / capacity checks of the two C calls, which happen on the host before
any GPU work (svhip_ragged_check is that test without a handle)."""
import ctypes

import numpy as np
import pytest

from speakerverification_amd import _lib, audio
from speakerverification_amd import model as sv_model
from speakerverification_amd.ragged import MIN_FRAMES, RaggedPacker, plan_ragged
from tests import fakes
from tests.e2e_data import make_e2e_files


# ---- the planner -------------------------------------------------------------------------------------------------------------
def _check_plan(frames, max_batch, cap):
    calls, alone = plan_ragged(frames, max_batch, cap)
    flat = [i for c in calls for i in c]
    assert sorted(flat + alone) == list(range(len(frames)))              # every file exactly once: none dropped, none twice
    assert flat == sorted(flat) and alone == sorted(alone)                # in order, within and across calls
    for c in calls:
        assert 1 <= len(c) <= max_batch
        assert sum(frames[i] for i in c) <= cap
    for i in alone:                                                       # handed back only when it fits NO call
        assert frames[i] > cap or frames[i] < MIN_FRAMES
    for i in flat:
        assert MIN_FRAMES <= frames[i] <= cap
    # greedy: a call was closed only because the next utterance did not fit it
    for a, b in zip(calls, calls[1:]):
        assert len(a) == max_batch or sum(frames[i] for i in a) + frames[b[0]] > cap
    return calls, alone


@pytest.mark.parametrize("seed", range(20))
def test_planner_properties_over_random_length_lists(seed):
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    max_batch = int(rng.integers(1, 40))
    T = int(rng.integers(5, 500))
    cap = max_batch * T
    n = int(rng.integers(0, 200))
    frames = [int(x) for x in rng.integers(1, int(2.2 * cap / max(1, max_batch // 2)) + 2, size=n)]
    _check_plan(frames, max_batch, cap)


def test_planner_named_cases():
    assert plan_ragged([], 4, 100) == ([], [])
    assert plan_ragged([50, 50, 50], 4, 100) == ([[0, 1], [2]], [])       # fills the row capacity exactly, then a new call
    assert plan_ragged([10] * 9, 4, 1000) == ([[0, 1, 2, 3], [4, 5, 6, 7], [8]], [])      # max_batch utterances per call
    assert plan_ragged([100, 101, 4, 5], 4, 100) == ([[0], [3]], [1, 2])  # too long and too short are handed back, not dropped
    calls, alone = _check_plan([401] * 256 + [4001, 12001], 256, 256 * 401)
    assert calls == [list(range(256)), [256, 257]] and alone == []
    with pytest.raises(ValueError):
        RaggedPacker(0, 10)


# ---- _embed_files(num_eval=0) ------------------------------------------------------------------------------------------------
class _RaggedS:
    """stand-in for the model module: embeds every utterance on its own with the fake embedder and records the ragged calls"""
    HOP, NFFT = 80, 512

    def __init__(self, emb, max_batch, frames):
        self.emb, self.max_batch, self.cap = emb, max_batch, max_batch * frames
        self.calls = []

    def eval(self): return self
    def state_dict(self): return {}
    def ragged_packer(self): return RaggedPacker(self.max_batch, self.cap)
    def ragged_frames(self, n): return n // self.HOP + 1 if n >= self.NFFT else 0

    def embed_ragged(self, wavs):
        self.calls.append([w.shape[0] for w in wavs])
        assert all(w.ndim == 1 and w.dtype == np.float32 for w in wavs)
        assert len(wavs) <= self.max_batch and sum(self.ragged_frames(w.shape[0]) for w in wavs) <= self.cap
        return np.concatenate([self.emb(w[None]) for w in wavs], 0)


class _PlainS:
    def eval(self): return self
    def state_dict(self): return {}


def _handler(tmp_path, S, dim=16, **kw):
    enc = sv_model.SpeakerEncoder.__new__(sv_model.SpeakerEncoder)
    enc.model = {"name": "ECAPA_TDNN", "nOut": dim}
    enc.criterion = {"name": "AAmSoftmaxAP"}
    enc.test_normalize = True
    enc.features = "melspectrogram"
    enc.__S__ = S
    enc._fusable = lambda: True
    emb = fakes.fake_embedder(dim)
    per_file = []
    def forward(data, label=None):
        per_file.append(data.shape)
        return emb(data.reshape(-1, data.shape[-1]))
    enc.forward = forward
    net = sv_model.WrappedModel(enc)
    net.forward = lambda x, label=None: enc.forward(x)
    spec = {"sample_rate": 16000, "channels": 1, "sentence_len": 2.0, "win_len": 0.025, "hop_len": 0.01}
    mh = sv_model.ModelHandling(net, audio_spec=spec, save_folder=str(tmp_path), embed_batch=5, device_feats=False, **kw)
    mh.test_encoder = enc
    return mh, per_file


def test_embed_files_whole_file_goes_through_planned_ragged_calls(tmp_path):
    files, _, _ = make_e2e_files(str(tmp_path))
    emb = fakes.fake_embedder(16)
    lens = [audio.loadWAV(f, {"sample_rate": 16000, "channels": 1, "sentence_len": 2.0}, evalmode=True, num_eval=0).reshape(-1).shape[0]
            for f in files]
    assert len(set(lens)) > 1                                            # the files have distinct lengths
    base_mh, base_calls = _handler(tmp_path, _PlainS())                  # no embed_ragged: today's per-file path
    want = base_mh._embed_files(files, 0)
    assert len(base_calls) == len(files) and want.shape == (len(files), 1, 16)
    for max_batch, frames in ((256, 401), (3, 700), (1, 420)):
        S = _RaggedS(emb, max_batch, frames)
        mh, per_file = _handler(tmp_path, S)
        got = mh._embed_files(files, 0)
        fr = [S.ragged_frames(n) for n in lens]
        calls, alone = plan_ragged(fr, max_batch, S.cap)
        assert S.calls == [[lens[i] for i in c] for c in calls]          # one ragged call per planned group, files in order
        assert len(per_file) == len(alone)                               # what fits no call keeps the per-file path
        assert np.array_equal(got, want)                                 # the same block as the per-file path
    # (1, 420): one file per call, and the longer files of the set exceed the 420 rows on their own
    assert alone and calls
    # ragged_eval=False, a model without embed_ragged, a non-default front-end, num_eval > 0: exactly today's path
    S = _RaggedS(emb, 256, 401)
    mh, per_file = _handler(tmp_path, S, ragged_eval=False)
    assert np.array_equal(mh._embed_files(files, 0), want) and S.calls == [] and len(per_file) == len(files)
    mh, per_file = _handler(tmp_path, S)
    enc = mh.test_encoder
    enc._fusable = lambda: False
    assert np.array_equal(mh._embed_files(files, 0), want) and S.calls == [] and len(per_file) == len(files)
    enc._fusable = lambda: True
    mh._embed_files(files, 2)
    assert S.calls == []


# ---- the C calls' argument checks: on the host, before any GPU work -------------------------------------------------------------
def _cfg(**kw):
    cfg = _lib.default_config()
    cfg.max_batch, cfg.samples = 4, 32000                                # T = 401: 1604 rows
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _check(cfg, lengths, is_wave, n=None):
    lib = _lib.load()
    a = np.ascontiguousarray(lengths, dtype=np.int32)
    rc = lib.svhip_ragged_check(ctypes.byref(cfg), a.ctypes.data, len(a) if n is None else n, 1 if is_wave else 0)
    return rc, (lib.svhip_last_error(None) or b"").decode()


def test_ragged_calls_refuse_bad_arguments_without_touching_a_gpu():
    INVALID, UNSUPPORTED = -1, _check(_cfg(model=_lib.MODEL_RAWNET2), [32000], True)[0]
    assert UNSUPPORTED not in (0, INVALID)
    cfg = _cfg()
    assert _check(cfg, [32000, 16000, 512, 70000], True)[0] == 0         # 401 + 201 + 7 + 876 frames
    assert _check(cfg, [401] * 4, False)[0] == 0                         # fills the row capacity exactly
    assert _check(cfg, [5, 6, 7, 1586], False)[0] == 0
    rc, msg = _check(cfg, [32000], True, n=0)
    assert rc == INVALID and "max_batch=4" in msg
    rc, msg = _check(cfg, [32000] * 5, True)
    assert rc == INVALID and "5 utterances" in msg and "max_batch=4" in msg
    rc, msg = _check(cfg, [401, 4, 401], False)
    assert rc == INVALID and "utterance 1" in msg and "fewer than 5" in msg
    rc, msg = _check(cfg, [32000, 511], True)
    assert rc == INVALID and "utterance 1" in msg and "n_fft=512" in msg
    rc, msg = _check(cfg, [401, 401, 401, 402], False)
    assert rc == INVALID and "utterance 3" in msg and "1604" in msg      # one row over the capacity
    rc, msg = _check(cfg, [1604 * 80], True)                            # 1605 frames
    assert rc == INVALID and "utterance 0" in msg and "1604" in msg
    for model in (_lib.MODEL_RAWNET2, _lib.MODEL_RAWNET3, _lib.MODEL_TITANET, _lib.MODEL_CONFORMER, _lib.MODEL_RESNETSE, _lib.MODEL_NONE):
        rc, msg = _check(_cfg(model=model), [32000], True)
        assert rc == UNSUPPORTED and "ECAPA" in msg
    rc, msg = _check(_cfg(compute=_lib.F32X3), [32000], True)
    assert rc == UNSUPPORTED and "SVHIP_F32" in msg
    assert _check(_cfg(compute=_lib.BF16), [32000], True)[0] == 0
    # the calls themselves: no handle, nothing runs
    lib = _lib.load()
    assert lib.svhip_embed_wave_ragged(None, None, None, None, 1, None, 0) == INVALID
    assert lib.svhip_embed_features_ragged(None, None, None, None, 1, None, 0) == INVALID
    bad = _cfg()
    bad.struct_size = 4
    assert _check(bad, [32000], True)[0] == INVALID
