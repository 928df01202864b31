"""CPU: what every array-passing wrapper of the Engine hands to the library — the export, its arguments in order (a pointer shown
as "ptr"), the flags word and the bytes it adds to TRANSFER_STATS — over a recording stand-in for libsvhip, once with numpy arrays
and once with CPU torch tensors (a non-CUDA tensor is a host buffer).  The expected values are written out by hand from the shapes:
N = 3 queries, M = 5 gallery rows, D = 192, k = 2, three trials."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from speakerverification_amd import engine as sv_engine
from speakerverification_amd.engine import Engine

P = "ptr"
N, M, D, K = 3, 5, 192, 2
HITS = (1, 0, 2)                        # what the stand-in's score_above_count reports per query: 3 hits in all


class _RecordingLib:
    """every export answers 0 and is written down; svhip_score_above_count also fills its counts so that the fill call follows"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def export(*args):
            self.calls.append((name, tuple(P if isinstance(a, int) and a > 1 << 20 else a for a in args)))
            if name == "svhip_score_above_count":
                np.ctypeslib.as_array((C.c_int64 * N).from_address(args[-2]))[:] = HITS
            return 0
        return export


def _engine(model="ecapa"):
    eng = Engine.__new__(Engine)
    eng.lib, eng.h, eng.on_numeric, eng.device, eng._stream = _RecordingLib(), None, "raise", 0, None
    eng.model, eng.n_mels, eng.frames, eng.embed_dim, eng.samples, eng.comm_world = model, 80, 11, D, 800, 2
    return eng


def _arrays(kind):
    rng = np.random.default_rng(0)
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    a = dict(E=f32(N, D), G=f32(M, D), F=f32(N, 2, D), ia=np.array([0, 1, 2], np.int32), ib=np.array([1, 2, 0], np.int32),
             q_stats=(f32(N), f32(N)), g_stats=(f32(M), f32(M)), wav=f32(N, 800), feat=f32(N, 80, 11), e1=f32(N, 512),
             utts=[f32(500), f32(300)], mels=[f32(80, 7), f32(80, 4)], pcm=rng.integers(-9, 9, 1000).astype(np.int16))
    if kind == "torch":
        t = torch.from_numpy
        a = {k: tuple(map(t, v)) if isinstance(v, tuple) else list(map(t, v)) if isinstance(v, list) else t(v) for k, v in a.items()}
    return SimpleNamespace(**a)


# label, engine model, the call, the library calls it makes, h2d bytes, d2h bytes.  Sizes: E 3*192*4 = 2304, G 5*192*4 = 3840,
# F 3*2*192*4 = 4608, an index list 3*4 = 12, q_stats 2*12 = 24, g_stats 2*20 = 40, wav 3*800*4 = 9600, feat 3*80*11*4 = 10560.
CASES = [
    ("l2norm_", "ecapa", lambda e, a: e.l2norm_(a.E),
     [("svhip_l2norm", (None, P, 3, 192, 0))], 2304, 2304),
    ("score_pairs", "ecapa", lambda e, a: e.score_pairs(a.E, a.ia, a.ib),
     [("svhip_score_pairs", (None, P, 3, 192, P, P, 3, P, 0))], 2304 + 12 + 12, 12),
    ("score_trials", "ecapa", lambda e, a: e.score_trials(a.F, a.ia, a.ib, "pdist"),
     [("svhip_score_trials", (None, 2, P, 3, 2, 192, P, P, 3, P, 0))], 4608 + 12 + 12, 12),
    ("score_trials_pnorm", "ecapa", lambda e, a: e.score_trials(a.F, a.ia, a.ib, "pnorm", p=3),
     [("svhip_score_trials_pnorm", (None, 3.0, P, 3, 2, 192, P, P, 3, P, 0))], 4608 + 12 + 12, 12),
    ("mean_crops", "ecapa", lambda e, a: e.mean_crops(a.F),
     [("svhip_mean_crops", (None, P, 3, 2, 192, P, 0))], 4608, 2304),
    # (until the wrappers shared one staging helper score_matrix counted nothing: 0, 0; now its host arrays count like every other call's)
    ("score_matrix", "ecapa", lambda e, a: e.score_matrix(a.E, a.G),
     [("svhip_score_matrix", (None, P, 3, P, 5, 192, P, 0))], 2304 + 3840, 3 * 5 * 4),
    ("score_topk", "ecapa", lambda e, a: e.score_topk(a.E, a.G, K),
     [("svhip_score_topk", (None, P, 3, P, 5, 192, 2, P, P, 0))], 2304 + 3840, 3 * 2 * 4 + 3 * 2 * 4),
    ("score_topk_norm", "ecapa", lambda e, a: e.score_topk_norm(a.E, a.q_stats, a.G, a.g_stats, K),
     [("svhip_score_topk_norm", (None, P, 3, P, P, P, 5, P, P, 192, 2, P, P, 0))], 2304 + 3840 + 24 + 40, 48),
    # two calls: the count (N int64 counts back), then the fill (the 4 int64 of row_ptr up; 3 hits: 3 int32 and 3 float32 back)
    ("score_above", "ecapa", lambda e, a: e.score_above(a.E, a.G, 0.25),
     [("svhip_score_above_count", (None, P, 3, P, 5, 192, 0.25, None, None, None, None, 0, 0, P, 0)),
      ("svhip_score_above_fill", (None, P, 3, P, 5, 192, 0.25, None, None, None, None, 0, 0, P, P, P, 0))],
     6144 + 6144 + 32, 24 + 12 + 12),
    ("score_above_norm_upper", "ecapa", lambda e, a: e.score_above(a.E, a.G, 0.25, a.q_stats, a.g_stats, upper=True, q_base=1),
     [("svhip_score_above_count", (None, P, 3, P, 5, 192, 0.25, P, P, P, P, 1, 1, P, 0)),
      ("svhip_score_above_fill", (None, P, 3, P, 5, 192, 0.25, P, P, P, P, 1, 1, P, P, P, 0))],
     6208 + 6208 + 32, 24 + 12 + 12),
    ("cluster_above", "ecapa", lambda e, a: e.cluster_above(a.E, 0.25, a.q_stats),
     [("svhip_cluster_above", (None, P, 3, 192, 0.25, P, P, P, P, P, 0))], 2304 + 24, 12 + 12 + 8),
    ("cluster_above_plain", "ecapa", lambda e, a: e.cluster_above(a.E, 0.25),
     [("svhip_cluster_above", (None, P, 3, 192, 0.25, None, None, P, P, P, 0))], 2304, 12 + 12 + 8),
    # group_ptr [0, 2, 3] (3 int64 = 24 bytes up, a host table whatever F is); the score blocks hold 2*2 + 1*1 = 5 float32
    ("group_audit", "ecapa", lambda e, a: e.group_audit(a.F, [0, 2, 3], 0.5, scores=True),
     [("svhip_group_audit", (None, P, 3, 2, 192, P, 2, 0.5, P, P, 0))], 4608 + 24, 12 + 20),
    ("group_audit_counts", "ecapa", lambda e, a: e.group_audit(a.F, [0, 2, 3], 0.5),
     [("svhip_group_audit", (None, P, 3, 2, 192, P, 2, 0.5, P, None, 0))], 4608 + 24, 12),
    ("asnorm_stats", "ecapa", lambda e, a: e.asnorm_stats(a.E, a.G, top=4),
     [("svhip_asnorm_stats", (None, P, 3, 192, P, 5, 4, P, P, 0))], 2304 + 3840, 12 + 12),
    ("asnorm_pairs", "ecapa", lambda e, a: e.asnorm_pairs(a.E, a.q_stats[0], a.q_stats[1], a.ia, a.ib),
     [("svhip_asnorm_pairs", (None, P, 3, 192, P, P, P, P, 3, P, 0))], 2304 + 12 + 12 + 12 + 12, 12),
    # ---- the forward half ----
    ("fbank", "ecapa", lambda e, a: e.fbank(a.wav),
     [("svhip_fbank", (None, P, 3, 800, P, 0))], 9600, 10560),
    ("fbank_async", "ecapa", lambda e, a: e.fbank(a.wav, async_=True),
     [("svhip_fbank", (None, P, 3, 800, P, 4))], 9600, 10560),
    ("embed_features", "ecapa", lambda e, a: e.embed_features(a.feat),
     [("svhip_embed_features", (None, P, 3, 11, P, 0))], 10560, 2304),
    ("embed_wave", "ecapa", lambda e, a: e.embed_wave(a.wav),
     [("svhip_embed_wave", (None, P, 3, 800, P, 0))], 9600, 2304),
    ("embed_wave_async_ordered", "ecapa", lambda e, a: e.embed_wave(a.wav, async_=True, ordered=True),
     [("svhip_embed_wave", (None, P, 3, 800, P, 4))], 9600, 2304),
    ("fusion_head", "fusion_head", lambda e, a: e.fusion_head(a.e1, a.E),
     [("svhip_fusion_head", (None, P, 512, P, 192, 3, P, 0))], 3 * 512 * 4 + 2304, 2304),
    # ragged packs: 500 + 300 samples / 7 + 4 frames of 80 mels in one float32 array; the offsets and lengths are not counted
    ("embed_wave_ragged", "ecapa", lambda e, a: e.embed_wave_ragged(a.utts),
     [("svhip_embed_wave_ragged", (None, P, P, P, 2, P, 0))], 800 * 4, 2 * 192 * 4),
    ("embed_features_ragged", "conformer", lambda e, a: e.embed_features_ragged(a.mels, async_=True),
     [("svhip_conformer_embed_ragged", (None, P, P, P, 2, P, 4, 0))], 11 * 80 * 4, 2 * 192 * 4),
    ("allgather_rows", "ecapa", lambda e, a: e.allgather_rows(a.E),
     [("svhip_allgather_rows", (None, P, 3, 192, P, 0))], 2304, 2 * 2304),
    # 1000 int16 samples, two files: the PCM, 2 int64 offsets and 2 int32 lengths go up; 2 files * 2 crops of 100 float32 come back
    ("crop_pcm16_packed", "ecapa", lambda e, a: e.crop_pcm16_packed(a.pcm, [0, 600], [600, 400], 2, L=100),
     [("svhip_crop_pcm16", (None, P, 1000, P, P, 2, 2, 100, P, 0))], 2000 + 16 + 8, 4 * 100 * 4),
    ("synth_waveforms", "ecapa", lambda e, a: e.synth_waveforms(7, 5, 3, L=100),
     [("svhip_synth_waveforms", (None, 7, 5, 3, 100, P, 0))], 0, 3 * 100 * 4),
    ("synth_waveforms_async", "ecapa", lambda e, a: e.synth_waveforms(7, 5, 3, out=np.empty((3, 800), np.float32), async_=True),
     [("svhip_synth_waveforms", (None, 7, 5, 3, 800, P, 4))], 0, 3 * 800 * 4),
]


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("label,model,call,want,h2d,d2h", CASES, ids=[c[0] for c in CASES])
def test_wrapper_reaches_the_library_as_written_down(kind, label, model, call, want, h2d, d2h):
    eng, a = _engine(model), _arrays(kind)
    before = dict(sv_engine.TRANSFER_STATS)
    call(eng, a)
    assert eng.lib.calls == want
    assert sv_engine.TRANSFER_STATS["h2d_bytes"] - before["h2d_bytes"] == h2d
    assert sv_engine.TRANSFER_STATS["d2h_bytes"] - before["d2h_bytes"] == d2h


def test_results_come_back_in_the_inputs_space_and_type():
    eng, a = _engine(), _arrays("torch")
    scores, index = eng.score_topk(a.E, a.G, K)                 # a CPU tensor is a host buffer: numpy comes back
    assert isinstance(scores, np.ndarray) and scores.shape == (N, K) and scores.dtype == np.float32 and index.dtype == np.int32
    row_ptr, index, score = eng.score_above(a.E, a.G, 0.25)
    assert row_ptr.tolist() == [0, 1, 1, 3] and row_ptr.dtype == np.int64 and index.shape == score.shape == (3,)
    root, cluster, n = eng.cluster_above(a.E, 0.25)
    assert root.shape == cluster.shape == (N,) and isinstance(n, int)
    miss, score, score_ptr = eng.group_audit(a.F, [0, 2, 3], 0.5, scores=True)
    assert miss.shape == (N,) and miss.dtype == np.int32 and score.shape == (5,) and score_ptr.tolist() == [0, 4, 5]
    out = np.empty(N, np.float32)
    assert eng.score_pairs(a.E, a.ia, a.ib, out=out) is out and eng.l2norm_(a.E) is a.E


def test_a_wrong_output_is_refused_before_the_library_is_touched():
    eng, a = Engine.__new__(Engine), _arrays("numpy")           # no library at all: a call that got past the check fails on `self.lib`
    with pytest.raises(ValueError, match="output arrays must be C-contiguous and of the right dtype"):
        eng.score_pairs(a.E, a.ia, a.ib, out=np.empty(N, np.float64))
    with pytest.raises(ValueError, match="output arrays must be C-contiguous and of the right dtype"):
        eng.score_matrix(a.E, a.G, out=np.empty((M, N), np.float32).T)
    with pytest.raises(ValueError, match="output tensors must be contiguous and of the right dtype"):
        eng.mean_crops(a.F, out=torch.empty((N, D), dtype=torch.float64))
    with pytest.raises(ValueError, match="output tensors must be contiguous and of the right dtype"):
        eng.l2norm_(torch.zeros((D, N)).T)
    with pytest.raises(ValueError, match=r"out must be a \(3, 2\) float32 and a \(3, 2\) int32 array"):
        eng.score_topk(a.E, a.G, K, out=(np.empty((N, 1), np.float32), np.empty((N, 1), np.int32)))
    with pytest.raises(ValueError, match=r"out must be a \(3, 2\) float32 and a \(3, 2\) int32 array"):
        eng.score_topk_norm(a.E, a.q_stats, a.G, a.g_stats, K, out=(np.empty((N, K), np.float32), np.empty((N, 1), np.int32)))
    with pytest.raises(ValueError, match="output arrays"):
        eng.synth_waveforms(7, 5, 3, L=100, out=np.empty((3, 100), np.int16))
    with pytest.raises(ValueError, match="async_ needs a device output tensor"):
        eng.crop_pcm16_packed(a.pcm, [0, 600], [600, 400], 2, L=100, async_=True)
    with pytest.raises(AttributeError):                         # (the control: good arguments do reach the library)
        eng.score_pairs(a.E, a.ia, a.ib)


def test_an_input_of_another_type_is_converted():
    seen = {}

    class _Lib:
        def svhip_score_pairs(self, h, e, n, d, ia, ib, p, out, flags):
            seen["E"] = np.ctypeslib.as_array((C.c_float * (n * d)).from_address(e)).reshape(n, d).copy()
            seen["ia"] = np.ctypeslib.as_array((C.c_int32 * p).from_address(ia)).tolist()
            seen["ib"] = np.ctypeslib.as_array((C.c_int32 * p).from_address(ib)).tolist()
            return 0

    eng = _engine()
    eng.lib = _Lib()
    E = np.arange(N * D, dtype=np.float64).reshape(N, D)
    before = dict(sv_engine.TRANSFER_STATS)
    eng.score_pairs(E[:, ::-1], torch.tensor([0, 1, 2]), np.array([1, 2, 0], np.int64))     # float64 and a view; int64 indices
    assert seen["E"].dtype == np.float32 and np.array_equal(seen["E"], E[:, ::-1].astype(np.float32))
    assert seen["ia"] == [0, 1, 2] and seen["ib"] == [1, 2, 0]
    assert sv_engine.TRANSFER_STATS["h2d_bytes"] - before["h2d_bytes"] == 2304 + 12 + 12        # what travels is the converted copy
