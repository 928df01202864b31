"""Engine — thin Python owner of one svhip handle (one HIP device, one stream, one model).

Host-side plumbing only: every array that crosses into the library is passed as a raw pointer
(numpy -> host pointer, torch CUDA tensor -> device pointer).  No computation happens here.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Dict, Optional

import numpy as np

from . import _lib

try:  # torch is plumbing (device memory / streams / torch.distributed); numpy-only use works without it
    import torch
except Exception:  # pragma: no cover
    torch = None


def _is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


# bytes that crossed PCIe through this module since import (host buffers handed to / filled by the library); tests use it
# to assert WHAT travels (e.g. int16 PCM instead of fp32 crops), bench.py to report PCIe-inclusive rates
TRANSFER_STATS = {"h2d_bytes": 0, "d2h_bytes": 0}


def to_device(a, device=0):
    """host array -> CUDA tensor (torch owns the memory: plumbing), counted as PCIe traffic"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{device}")
    TRANSFER_STATS["h2d_bytes"] += t.numel() * t.element_size()
    return t


def to_host(t):
    """CUDA tensor -> numpy, counted as PCIe traffic (numpy arrays pass through)"""
    if _is_torch(t):
        if t.is_cuda:
            TRANSFER_STATS["d2h_bytes"] += t.numel() * t.element_size()
        return t.detach().cpu().numpy()
    return np.asarray(t)


class _Buf:
    """Pointer view of a numpy array (host) or a torch tensor (host or device)."""

    def __init__(self, x, dtype, writable=False):
        self.keep = x
        if _is_torch(x):
            tdt = {np.float32: torch.float32, np.int32: torch.int32, np.int16: torch.int16, np.int64: torch.int64}[dtype]
            if x.dtype != tdt or not x.is_contiguous():
                if writable:
                    raise ValueError("output tensors must be contiguous and of the right dtype")
                x = x.to(tdt).contiguous()
                self.keep = x
            self.device = x.is_cuda
            self.ptr = x.data_ptr()
            self.nbytes = x.numel() * x.element_size()
        else:
            a = np.asarray(x)
            if a.dtype != dtype or not a.flags["C_CONTIGUOUS"]:
                if writable:
                    raise ValueError("output arrays must be C-contiguous and of the right dtype")
                a = np.ascontiguousarray(a, dtype=dtype)
            self.keep = a
            self.device = False
            self.ptr = a.ctypes.data
            self.nbytes = a.nbytes


class _Call:
    """The arrays of ONE library call: ``inp`` / ``out`` / ``inout`` register an array and return its pointer, ``host`` a host table
    that travels beside the arrays.  ``run(export, *args)`` works the flags word out from what was registered and appends it to the
    arguments (where every C signature has it), orders the call after torch, makes it, checks the return code and counts the host
    buffers into TRANSFER_STATS (once, after the call returned).
    ``same_space`` (scoring calls): all arrays live in one memory space, or ``run`` refuses.  Otherwise (forward calls) the first
    input and the output say where the data lives, each for itself; a call without an input array has no input on the device.
    ``ins``: the registered inputs of an earlier call that this one takes again."""
    __slots__ = ("eng", "same_space", "async_", "ordered", "ins", "outs", "h2d")

    def __init__(self, eng, same_space=False, async_=False, ordered=False, ins=()):
        self.eng = eng
        self.same_space = same_space
        self.async_ = async_
        self.ordered = ordered
        self.ins = list(ins)
        self.outs = []
        self.h2d = 0

    def inp(self, x, dtype=np.float32):
        b = _Buf(x, dtype)
        self.ins.append(b)
        return b.ptr

    def out(self, x, dtype=np.float32):
        b = _Buf(x, dtype, writable=True)
        self.outs.append(b)
        return b.ptr

    def inout(self, x, dtype=np.float32):
        """an array the call rewrites in place: it travels both ways"""
        b = _Buf(x, dtype, writable=True)
        self.ins.append(b)
        self.outs.append(b)
        return b.ptr

    def host(self, a):
        """a contiguous host numpy table (offsets, lengths, group boundaries) that is copied up whatever space the arrays live in"""
        self.h2d += a.nbytes
        return a.ctypes.data

    def run(self, export, *args, tail=()):
        """export(*args, flags, *tail): ``tail`` is what a ragged export takes after the flags"""
        ins, outs = self.ins, self.outs
        h2d, d2h, n_dev = self.h2d, 0, 0
        for b in ins:
            if b.device:
                n_dev += 1
            else:
                h2d += b.nbytes
        for b in outs:
            if b.device:
                n_dev += 1
            else:
                d2h += b.nbytes
        if n_dev:
            if self.same_space and n_dev != len(ins) + len(outs):
                raise ValueError("all arrays of one scoring call must live in the same memory space")
            if not self.ordered:                            # (ordered: the caller has already waited for torch's stream)
                self.eng._order_after_torch(self.async_)
            flags = (_lib.IN_DEVICE if ins and ins[0].device else 0) | (_lib.OUT_DEVICE if outs[0].device else 0)
        else:
            flags = 0
        self.eng._ck(export(*args, (flags | _lib.ASYNC) if self.async_ else flags, *tail))
        TRANSFER_STATS["h2d_bytes"] += h2d
        TRANSFER_STATS["d2h_bytes"] += d2h


# The ragged exports of the library per model kind, as data: the waveform export and the feature export (None: a waveform model), each a
# name with the arguments that follow the common ones (svhip_embed_wave_ragged's); the host-only check export and whether it takes is_wave
# after (cfg, lengths, n); and the frames of an utterance of n samples at the handle's hop, in the unit of row_capacity.  A model kind
# without a row goes to ECAPA's exports, which refuse its handle by name.
_RaggedCalls = namedtuple("_RaggedCalls", "wave features check check_takes_is_wave frames")
_MEL_FRAMES = lambda n, hop: n // hop + 1
_RAGGED = {
    "ecapa": _RaggedCalls(("svhip_embed_wave_ragged",), ("svhip_embed_features_ragged",), "svhip_ragged_check", True, _MEL_FRAMES),
    "rawnet3": _RaggedCalls(("svhip_rawnet3_embed_ragged",), None, "svhip_rawnet3_ragged_check", False,
                            lambda n, hop: (n - 251) // 10 + 1),       # the frames after its sinc filterbank (251 taps, stride 10)
    "rawnet2_conv": _RaggedCalls(("svhip_rawnet2_embed_ragged",), None, "svhip_rawnet2_ragged_check", False,
                                 lambda n, hop: n // 3),                # the frames after its conv front-end (kernel 3, stride 3)
    "conformer": _RaggedCalls(("svhip_conformer_embed_ragged", 1), ("svhip_conformer_embed_ragged", 0), "svhip_conformer_ragged_check", True,
                              _MEL_FRAMES),
    "titanet": _RaggedCalls(("svhip_titanet_embed_ragged", 1), ("svhip_titanet_embed_ragged", 0), "svhip_titanet_ragged_check", True, _MEL_FRAMES),
    # (row_capacity counts mel frames; an utterance of a pack takes its frames rounded up to a multiple of 8: ResNetSE.ragged_frames)
    "resnetse": _RaggedCalls(("svhip_resnetse_embed_ragged", 1), ("svhip_resnetse_embed_ragged", 0), "svhip_resnetse_ragged_check", True, _MEL_FRAMES),
}


class Engine:
    def __init__(self, model="ecapa", compute="f32", channels=1024, n_mels=80, embed_dim=192, max_batch=8,
                 samples=32000, log_input=True, input_norm=False, device=0, stream=None,
                 sr=8000, n_fft=512, win_length=200, hop_length=80, fmin=0.0, fmax=None, pre_emphasis=True, on_numeric="raise",
                 sinc_sr=16000):
        """``sinc_sr``: the sample rate of RawNet2's sinc front-end (the reference's ``audio_spec['sample_rate']``, RawNet2_custom.py:55-67).
        ``model="fusion_head"``: the attention head of Raw_ECAPA_hype (``channels=704``, ``embed_dim=nOut``; ``fusion_head`` is its forward).
        ``on_numeric``: what a forward does when the library reports SVHIP_ERR_NONFINITE / SVHIP_ERR_RANGE (the outputs were written,
        but an fp16 activation overflowed / the input left an f32x3 handle's range / the input was not finite): "raise"
        (_lib.SvhipNumericError, default), "warn" (RuntimeWarning; the outputs are returned as computed, as the reference would) or "ignore"."""
        if on_numeric not in ("raise", "warn", "ignore"):
            raise ValueError("on_numeric must be 'raise', 'warn' or 'ignore'")
        self.on_numeric = on_numeric
        self.lib = _lib.load()
        cfg = _lib.default_config()
        cfg.model = {"ecapa": _lib.MODEL_ECAPA, "rawnet2": _lib.MODEL_RAWNET2, "rawnet2_conv": _lib.MODEL_RAWNET2_CONV,
                     "rawnet2_gru": _lib.MODEL_RAWNET2_GRU, "rawnet3": _lib.MODEL_RAWNET3, "titanet": _lib.MODEL_TITANET,
                     "conformer": _lib.MODEL_CONFORMER, "resnetse": _lib.MODEL_RESNETSE, "none": _lib.MODEL_NONE,
                     "fusion_head": _lib.MODEL_FUSION_HEAD}[model]
        cfg.compute = {"f32": _lib.F32, "fp32": _lib.F32, "bf16": _lib.BF16, "f32x3": _lib.F32X3, "bf16x3": _lib.F32X3,
                       "f16": _lib.F16, "fp16": _lib.F16}[compute]
        cfg.device = int(device)
        cfg.channels = int(channels)
        cfg.n_mels = int(n_mels)
        cfg.embed_dim = int(embed_dim)
        cfg.max_batch = int(max_batch)
        cfg.samples = int(samples)
        cfg.log_input = int(bool(log_input))
        cfg.input_norm = int(bool(input_norm))
        cfg.fb_sr, cfg.n_fft, cfg.win_length, cfg.hop_length = int(sr), int(n_fft), int(win_length), int(hop_length)
        cfg.fmin = float(fmin)
        cfg.fmax = -1.0 if fmax is None else float(fmax)
        cfg.preemph = 0.97 if pre_emphasis is True else (-1.0 if pre_emphasis in (False, None) else float(pre_emphasis))
        cfg.stream = C.c_void_p(int(stream)) if stream else None
        cfg.sinc_sr = int(sinc_sr)
        self.cfg = cfg
        self.model = model
        self.compute = {_lib.BF16: "bf16", _lib.F32X3: "f32x3", _lib.F16: "f16"}.get(cfg.compute, "f32")
        self.max_batch = cfg.max_batch
        self.samples = cfg.samples
        self.frames = cfg.samples // cfg.hop_length + 1
        self.n_mels = cfg.n_mels
        self.embed_dim = cfg.embed_dim
        self.device = cfg.device
        h = C.c_void_p()
        rc = self.lib.svhip_create(C.byref(cfg), C.byref(h))
        if rc != _lib.OK:
            msg = self.lib.svhip_last_error(None)
            raise _lib.SvhipError(rc, msg.decode() if msg else "?")
        self.h = h
        self._stream = int(stream) if stream else None

    def _order_after_torch(self, async_):
        """Device tensors handed in by torch may still be in flight on torch's current stream.  When the
        handle runs on that same stream the order is already right; otherwise wait for torch's stream
        on the host before the library touches the data (and refuse async calls, which would race)."""
        cur = torch.cuda.current_stream(self.device)
        if self._stream is not None and cur.cuda_stream == self._stream:
            return
        if async_:
            raise ValueError("async_ calls need the Engine to be created on torch's current stream")
        cur.synchronize()

    # ---- lifetime ------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.svhip_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        _lib.check(self.h, rc, self.on_numeric)

    def synchronize(self):
        """waits for the handle's stream; reports (per on_numeric) and clears the numeric status of the async calls it waited for"""
        self._ck(self.lib.svhip_synchronize(self.h))

    def numeric_status(self, reset=True):
        """0, _lib.ERR_NONFINITE or _lib.ERR_RANGE for the forwards since the last reset (waits for the stream; never raises)"""
        return int(self.lib.svhip_numeric_status(self.h, 1 if reset else 0))

    # ---- weights ---------------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, object], strict=True, show_error=False):
        """Name-matched copy of a reference ``__S__`` state dict (src/model.py:718-746 semantics:
        with strict=False unknown / mis-shaped tensors are skipped, optionally printed)."""
        skipped = []
        for name, v in sd.items():
            if _is_torch(v):
                v = v.detach().cpu().numpy()
            a = np.asarray(v)
            shp = a.shape                       # (ascontiguousarray would promote 0-d to 1-d)
            if a.dtype == np.int64:
                dt = _lib.I64
                a = np.ascontiguousarray(a)
            else:
                a = np.ascontiguousarray(a, dtype=np.float32)
                dt = _lib.F32
            shape = (C.c_int64 * max(1, len(shp)))(*shp)
            rc = self.lib.svhip_load_tensor(self.h, name.encode(), a.ctypes.data, shape, len(shp), dt)
            if rc != _lib.OK:
                if strict:
                    self._ck(rc)
                msg = self.lib.svhip_last_error(self.h).decode()
                skipped.append(name)
                if show_error:
                    print(msg)
        return skipped

    def finalize(self):
        self._ck(self.lib.svhip_finalize_weights(self.h))

    def load_blob(self, path):
        """mmap a packed checkpoint blob (speakerverification_amd.checkpoint) and finalize: svhip_load_blob."""
        self._ck(self.lib.svhip_load_blob(self.h, str(path).encode()))

    # ---- forward ------------------------------------------------------------------------------------------
    def _out(self, like, shape, dtype=np.float32):
        """an uninitialised output where ``like`` lives: a CUDA tensor beside a CUDA tensor, else a numpy array"""
        if torch is not None and isinstance(like, torch.Tensor) and like.is_cuda:
            return torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=like.device)
        return np.empty(shape, dtype)

    def fbank(self, wav, out=None, async_=False):
        """(B, L) fp32 waveforms -> (B, n_mels, T) mel power (numpy in -> numpy out, CUDA tensor in -> CUDA tensor out)."""
        B, L = wav.shape
        if out is None:
            out = self._out(wav, (B, self.n_mels, self.frames))
        c = _Call(self, async_=async_)
        i, o = c.inp(wav), c.out(out)
        c.run(self.lib.svhip_fbank, self.h, i, B, L, o)
        return out

    def embed_features(self, feat, out=None, async_=False):
        B, nm, T = feat.shape
        if nm != self.n_mels:
            raise ValueError(f"expected {self.n_mels} feature channels, got {nm}")
        if out is None:
            out = self._out(feat, (B, self.embed_dim))
        c = _Call(self, async_=async_)
        i, o = c.inp(feat), c.out(out)
        c.run(self.lib.svhip_embed_features, self.h, i, B, T, o)
        return out

    def embed_wave(self, wav, out=None, async_=False, ordered=False):
        """``ordered=True``: the caller guarantees that the device buffers are complete and stay alive (it has synchronised
        torch's stream and will call synchronize() on this handle): lets an async call run on the handle's OWN stream."""
        B, L = wav.shape
        if out is None:
            out = self._out(wav, (B, self.embed_dim))
        c = _Call(self, async_=async_, ordered=ordered)
        i, o = c.inp(wav), c.out(out)
        c.run(self.lib.svhip_embed_wave, self.h, i, B, L, o)
        return out

    def fusion_head(self, e1, e2, out=None, async_=False, ordered=False):
        """``model="fusion_head"`` handles: the two branch embeddings (B, d1) and (B, d2), d1 + d2 == 704, as separate arrays -> (B, embed_dim)
        (svhip_fusion_head; numpy in -> numpy out, CUDA tensors in -> CUDA tensor out).  ``ordered``: as in embed_wave."""
        B, d1 = e1.shape
        B2, d2 = e2.shape
        if B2 != B:
            raise ValueError(f"the branch embeddings have {B} and {B2} rows")
        if out is None:
            out = self._out(e1, (B, self.embed_dim))
        c = _Call(self, async_=async_, ordered=ordered)
        i1, i2, o = c.inp(e1), c.inp(e2), c.out(out)
        if c.ins[0].device != c.ins[1].device:
            raise ValueError("both branch embeddings must live in the same memory space")
        c.run(self.lib.svhip_fusion_head, self.h, i1, d1, i2, d2, B, o)
        return out

    # ---- ragged batches: utterances of different lengths in one call (_RAGGED names the model's exports) ----
    @property
    def _ragged(self):
        return _RAGGED.get(self.model, _RAGGED["ecapa"])

    @property
    def row_capacity(self):
        """frames one ragged call can hold: the rows of the handle's workspace, max_batch frames_of(samples)"""
        return self.max_batch * self.frames_of(self.samples)

    def frames_of(self, n_samples):
        """frames of an utterance of n_samples in the unit of row_capacity (_RAGGED: mel frames, or the model's own first frame level)"""
        return self._ragged.frames(int(n_samples), int(self.cfg.hop_length))

    def _pack(self, items, offsets, lengths, is_wave):
        """a list of arrays -> (packed array, int64 offsets, int32 lengths); a packed array with its tables passes through.
        Offsets and lengths count samples (waveforms) or frames (features: each item (n_mels, T_i), packed as blocks back to back)."""
        if offsets is not None:
            if lengths is None:
                raise ValueError("a packed array needs offsets and lengths")
            return items, np.ascontiguousarray(offsets, dtype=np.int64), np.ascontiguousarray(lengths, dtype=np.int32)
        items = list(items)
        if not items:
            raise ValueError("empty batch")
        if not is_wave:
            for a in items:
                if a.ndim != 2 or a.shape[0] != self.n_mels:
                    raise ValueError(f"expected ({self.n_mels}, T) features, got {tuple(a.shape)}")
        lens = np.asarray([a.shape[-1] for a in items], dtype=np.int32)
        offs = np.zeros(len(items), dtype=np.int64)
        offs[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        if _is_torch(items[0]):
            packed = torch.cat([a.to(torch.float32).reshape(-1) for a in items])
        else:
            packed = np.concatenate([np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in items])
        return packed, offs, lens

    def _embed_ragged(self, export, items, offsets, lengths, out, async_, is_wave, ordered=False):
        """export: a wave / features entry of _RAGGED, (name, trailing arguments ..)"""
        packed, offs, lens = self._pack(items, offsets, lengths, is_wave)
        n = int(lens.shape[0])
        if out is None:
            out = self._out(packed, (n, self.embed_dim))
        c = _Call(self, async_=async_, ordered=ordered)
        i, o = c.inp(packed), c.out(out)
        c.run(getattr(self.lib, export[0]), self.h, i, offs.ctypes.data, lens.ctypes.data, n, o, tail=export[1:])   # (the tables are not counted)
        return out

    def embed_wave_ragged(self, wavs, offsets=None, lengths=None, out=None, async_=False, ordered=False):
        """utterances of different lengths -> (n, embed_dim), each as if forwarded alone at its own length.  ``wavs``: a list of 1-D
        arrays, or ONE packed array with ``offsets`` / ``lengths`` in samples; numpy or CUDA tensors, like embed_wave."""
        return self._embed_ragged(self._ragged.wave, wavs, offsets, lengths, out, async_, True, ordered)

    def embed_features_ragged(self, feats, offsets=None, lengths=None, out=None, async_=False):
        """``feats``: a list of (n_mels, T_i) mel-power arrays, or one packed array of such blocks with frame ``offsets`` / ``lengths``."""
        return self._embed_ragged(self._ragged.features or _RAGGED["ecapa"].features, feats, offsets, lengths, out, async_, False)

    def ragged_check(self, lengths, is_wave=True):
        """the library's own capacity test for a pack (host only): None, or the refusal's text"""
        lens = np.ascontiguousarray(lengths, dtype=np.int32)
        r = self._ragged
        rc = getattr(self.lib, r.check)(C.byref(self.cfg), lens.ctypes.data, int(lens.shape[0]), *([1 if is_wave else 0] if r.check_takes_is_wave else []))
        return None if rc == _lib.OK else (self.lib.svhip_last_error(None) or b"?").decode()

    def crop_pcm16(self, pcm_list, num_eval, L=32000, out=None, async_=False):
        """list of 1-D int16 arrays (decoded files) -> (len(list) * num_eval, L) fp32 eval-mode crops, cropped on
        the device (int16 travels over PCIe; reference semantics of loadWAV for 16-bit files).  With ``out`` a CUDA
        tensor the crops stay in HBM (the embed call then takes them as a device pointer: no fp32 crop crosses PCIe)."""
        lens = np.asarray([len(a) for a in pcm_list], dtype=np.int32)
        offs = np.zeros(len(pcm_list), dtype=np.int64)
        offs[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        if len(pcm_list) == 1 and _is_torch(pcm_list[0]):          # one packed (pinned) int16 tensor holding the files back to back
            raise ValueError("pass packed PCM through crop_pcm16_packed")
        pcm = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int16) for a in pcm_list]))
        return self.crop_pcm16_packed(pcm, offs, lens, num_eval, L, out=out, async_=async_)

    def crop_pcm16_packed(self, pcm, offs, lens, num_eval, L=32000, out=None, async_=False):
        """the files back to back in ONE int16 array (numpy, or a pinned torch tensor for truly asynchronous copies) with their
        offsets / lengths; async_=True (device `out` only) returns once the copy and the crop kernel are enqueued."""
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        c = _Call(self, async_=async_)
        p = c.inp(pcm, np.int16)
        if c.ins[0].device:
            raise ValueError("packed PCM lives on the host (device PCM: call the C ABI with SVHIP_IN_DEVICE)")
        n_files = int(lens.shape[0])
        n = n_files * num_eval
        if out is None:
            out = np.empty((n, L), dtype=np.float32)
        elif tuple(out.shape) != (n, L):
            raise ValueError(f"out must be ({n}, {L})")
        o = c.out(out)
        if async_ and not c.outs[0].device:
            raise ValueError("async_ needs a device output tensor")
        c.run(self.lib.svhip_crop_pcm16, self.h, p, c.ins[0].nbytes // 2, c.host(offs), c.host(lens), n_files, int(num_eval), int(L), o)
        return out

    def synth_waveforms(self, seed, first_utt, B, L=None, out=None, async_=False):
        """utterances [first_utt, first_utt + B) of the counter-based synthetic stream ``seed`` (svhip_synth_waveforms)."""
        L = int(L or self.samples)
        if out is None:
            out = np.empty((B, L), dtype=np.float32)
        c = _Call(self, async_=async_)                       # (no input array: only the output says where the data lives)
        o = c.out(out)
        c.run(self.lib.svhip_synth_waveforms, self.h, int(seed), int(first_utt), int(B), L, o)
        return out

    # ---- multi-GPU exchange (RCCL under the C ABI) -------------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        lib = _lib.load()
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        rc = lib.svhip_comm_unique_id(buf)
        if rc != _lib.OK:
            raise _lib.SvhipError(rc, (lib.svhip_comm_last_error() or b"?").decode())
        return buf.raw

    def comm_init(self, id_bytes: bytes, rank: int, world: int):
        if len(id_bytes) != _lib.COMM_ID_BYTES:
            raise ValueError("the RCCL unique id is %d bytes" % _lib.COMM_ID_BYTES)
        self._ck(self.lib.svhip_comm_init(self.h, C.create_string_buffer(id_bytes, _lib.COMM_ID_BYTES), int(rank), int(world)))
        self.comm_rank, self.comm_world = int(rank), int(world)

    def comm_rank_world(self):
        """(rank, world) as the library's RCCL communicator reports them (svhip_comm_rank)"""
        r, w = C.c_int32(), C.c_int32()
        self._ck(self.lib.svhip_comm_rank(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def allgather_rows(self, local, out=None, async_=False):
        """(rows, D) fp32 block of every rank -> (world * rows, D) on every rank: ONE RCCL all-gather on the handle's stream."""
        rows, D = local.shape
        world = getattr(self, "comm_world", None)
        if world is None:
            raise RuntimeError("comm_init has not been called on this Engine")
        if out is None:
            out = self._out(local, (world * rows, D))
        c = _Call(self, async_=async_)
        i, o = c.inp(local), c.out(out)
        if tuple(out.shape) != (world * rows, D):
            raise ValueError(f"out must be ({world * rows}, {D})")
        c.run(self.lib.svhip_allgather_rows, self.h, i, rows, D, o)
        return out

    # ---- scoring ---------------------------------------------------------------------------------------------
    def l2norm_(self, E):
        N, D = E.shape
        c = _Call(self, same_space=True)
        e = c.inout(E)
        c.run(self.lib.svhip_l2norm, self.h, e, N, D)
        return E

    def score_pairs(self, E, ia, ib, out=None):
        N, D = E.shape
        P = int(ia.shape[0])
        if out is None:
            out = self._out(E, (P,))
        c = _Call(self, same_space=True)
        e, a, b, o = c.inp(E), c.inp(ia, np.int32), c.inp(ib, np.int32), c.out(out)
        c.run(self.lib.svhip_score_pairs, self.h, e, N, D, a, b, P, o)
        return out

    TRIAL_MODES = {"cosine": _lib.TRIAL_COSINE, "pnorm": _lib.TRIAL_PNORM, "pdist": _lib.TRIAL_PDIST}

    def score_trials(self, F, ia, ib, mode="cosine", out=None, p=2):
        """whole-trial scores over the crops of two files: F (n_files, n_crops, D), ia / ib file indices (svhip_score_trials);
        mode "pnorm" takes the reference's `p` (utils.py:167: any float, +-inf, 0)"""
        n_files, n_crops, D = F.shape
        P = int(ia.shape[0])
        if out is None:
            out = self._out(F, (P,))
        c = _Call(self, same_space=True)
        f, a, b, o = c.inp(F), c.inp(ia, np.int32), c.inp(ib, np.int32), c.out(out)
        if mode == "pnorm" and float(p) != 2.0:
            c.run(self.lib.svhip_score_trials_pnorm, self.h, float(p), f, n_files, n_crops, D, a, b, P, o)
        else:
            c.run(self.lib.svhip_score_trials, self.h, self.TRIAL_MODES[mode], f, n_files, n_crops, D, a, b, P, o)
        return out

    def mean_crops(self, F, out=None):
        """(n_files, n_crops, D) -> (n_files, D) crop means"""
        n_files, n_crops, D = F.shape
        if out is None:
            out = self._out(F, (n_files, D))
        c = _Call(self, same_space=True)
        f, o = c.inp(F), c.out(out)
        c.run(self.lib.svhip_mean_crops, self.h, f, n_files, n_crops, D, o)
        return out

    def score_matrix(self, A, B, out=None):
        Na, D = A.shape
        Nb = B.shape[0]
        if out is None:
            out = self._out(A, (Na, Nb))
        c = _Call(self, same_space=True)
        a, b, o = c.inp(A), c.inp(B), c.out(out)
        c.run(self.lib.svhip_score_matrix, self.h, a, Na, b, Nb, D, o)
        return out

    @staticmethod
    def _stat_pair(what, pair, n):
        """``what``'s ``(mu, sigma)`` pair of ``asnorm_stats`` for n rows, checked -> the pair"""
        if pair is None or len(pair) != 2:
            raise ValueError("stats must be a (mu, sigma) pair" if what == "stats" else "q_stats and g_stats must be (mu, sigma) pairs")
        for name, x in zip(("mu", "sigma"), pair):
            if x is None or tuple(x.shape) != (n,):
                raise ValueError(f"{what}: {name} must hold {n} values, not {None if x is None else tuple(x.shape)}")
        return tuple(pair)

    def _topk_out(self, c, like, N, k, out):
        """the ``(scores, index)`` pair of a top-k call: allocated where ``like`` lives, or ``out`` checked; registered as c's outputs
        -> ``(scores, index, their pointers)``"""
        shape = (N, max(k, 0))
        scores, index = out if out is not None else (self._out(like, shape), self._out(like, shape, np.int32))
        s, i = c.out(scores), c.out(index, np.int32)
        if c.outs[0].nbytes != N * max(k, 0) * 4 or c.outs[1].nbytes != c.outs[0].nbytes:
            raise ValueError(f"out must be a ({N}, {k}) float32 and a ({N}, {k}) int32 array")
        return scores, index, s, i

    def score_topk(self, Q, G, k, out=None):
        """1:N identification (``svhip_score_topk``): per row of Q (N, D) the k best rows of the gallery G (M, D) by inner product ->
        ``(scores (N, k) float32, index (N, k) int32)``, best first; equal scores go to the lower gallery index, NaN scores last.
        ``out``: a preallocated ``(scores, index)`` pair in the inputs' memory space."""
        N, D = Q.shape
        M = G.shape[0]
        if G.shape[1] != D:
            raise ValueError(f"queries are {D} wide, the gallery {G.shape[1]}")
        k = int(k)
        c = _Call(self, same_space=True)
        scores, index, s, i = self._topk_out(c, Q, N, k, out)
        q, g = c.inp(Q), c.inp(G)
        c.run(self.lib.svhip_score_topk, self.h, q, N, g, M, D, k, s, i)
        return scores, index

    def score_topk_norm(self, Q, q_stats, G, g_stats, k, out=None):
        """Open-set 1:N identification (``svhip_score_topk_norm``): ``score_topk`` over adaptive-S-normalised scores.  ``q_stats`` /
        ``g_stats``: the ``(mu, sigma)`` pairs ``asnorm_stats`` returns for Q and for G, in the inputs' memory space.  The score of
        query n against gallery row m is ``t = fmaf(s, aq + ag, -(bq + bg))`` with ``a = 0.5 / sigma``, ``b = mu * a`` in float32 —
        ``asnorm_pairs``' ``0.5*((s-mu_q)/sd_q + (s-mu_g)/sd_g)`` — and the k best rows are selected ON t (every gallery row has its own
        statistics, so the order differs from the cosine order).  Returns ``(t (N, k) float32, index (N, k) int32)``, best first,
        in ``score_topk``'s order; ``out`` as there."""
        N, D = Q.shape
        M = G.shape[0]
        if G.shape[1] != D:
            raise ValueError(f"queries are {D} wide, the gallery {G.shape[1]}")
        stats = self._stat_pair("q_stats", q_stats, N) + self._stat_pair("g_stats", g_stats, M)
        k = int(k)
        c = _Call(self, same_space=True)
        scores, index, s, i = self._topk_out(c, Q, N, k, out)
        q, g = c.inp(Q), c.inp(G)
        mq, sq, mg, sg = (c.inp(x) for x in stats)
        c.run(self.lib.svhip_score_topk_norm, self.h, q, N, mq, sq, g, M, mg, sg, D, k, s, i)
        return scores, index

    @staticmethod
    def _above_row_ptr(count, max_hits):
        """``score_above``'s step between its two calls: the per-row hit counts -> ``(row_ptr, total)``, the exclusive prefix sum
        (int64, N + 1 entries, in the counts' memory space) and its last entry.  A total above ``max_hits`` is a ``ValueError`` that
        names it, raised before anything is allocated for the hits."""
        if _is_torch(count):
            row_ptr = torch.zeros(count.numel() + 1, dtype=torch.int64, device=count.device)
            torch.cumsum(count, 0, out=row_ptr[1:])
        else:
            row_ptr = np.zeros(count.size + 1, np.int64)
            np.cumsum(count, out=row_ptr[1:])
        total = int(row_ptr[-1])
        if total > max_hits:
            raise ValueError(f"score_above: {total} hits exceed max_hits = {max_hits}; raise the threshold, query fewer rows per call or raise max_hits")
        return row_ptr, total

    def score_above(self, Q, G, thr, q_stats=None, g_stats=None, upper=False, q_base=0, max_hits=2 ** 28):
        """Threshold search (``svhip_score_above_count`` / ``_fill``): EVERY pair of a row of Q (N, D) and a row of the gallery G (M, D)
        whose score is at least ``thr``, as CSR -> ``(row_ptr (N + 1,) int64, index (total,) int32, score (total,) float32)``: the hits
        of query n are ``index[row_ptr[n]:row_ptr[n + 1]]``, in ascending gallery index.  The score is the inner product as
        ``score_topk`` computes it, or - with ``q_stats`` and ``g_stats``, the ``(mu, sigma)`` pairs of ``asnorm_stats`` - the
        normalised score of ``score_topk_norm``; a NaN score is never a hit.  ``upper``: the self-join of one set - Q is the rows
        ``q_base ..`` of G, and only the pairs with ``m > q_base + n`` are kept (every unordered pair once, no row with itself).
        All arrays in one memory space; the results come back in it.  Runs the count, takes the prefix sum, allocates, fills;
        more than ``max_hits`` hits in all are refused by a ``ValueError`` that names the total, before the allocation."""
        N, D = Q.shape
        M = G.shape[0]
        if G.shape[1] != D:
            raise ValueError(f"queries are {D} wide, the gallery {G.shape[1]}")
        thr = float(thr)
        if thr != thr:
            raise ValueError("score_above: the threshold is NaN")
        if (q_stats is None) != (g_stats is None):
            raise ValueError("score_above: q_stats and g_stats go together: give both (normalised scores) or neither")
        stats = () if q_stats is None else self._stat_pair("q_stats", q_stats, N) + self._stat_pair("g_stats", g_stats, M)
        c = _Call(self, same_space=True)
        q, g = c.inp(Q), c.inp(G)
        sp = [c.inp(x) for x in stats] or [None] * 4
        count = self._out(Q, N, np.int64)
        search = (self.h, q, N, g, M, D, thr, *sp, int(q_base), _lib.ABOVE_UPPER if upper else 0)
        c.run(self.lib.svhip_score_above_count, *search, c.out(count, np.int64))
        row_ptr, total = self._above_row_ptr(count, max_hits)
        index, score = self._out(Q, total, np.int32), self._out(Q, total)
        if total:
            c = _Call(self, same_space=True, ins=c.ins)                  # (the same operands again, and row_ptr)
            c.run(self.lib.svhip_score_above_fill, *search, c.inp(row_ptr, np.int64), c.out(index, np.int32), c.out(score))
        return row_ptr, index, score

    def cluster_above(self, E, thr, stats=None):
        """Speaker clustering (``svhip_cluster_above``): rows ``i < j`` of E (N, D) are linked iff their score is at least ``thr``, and
        a cluster is a connected component of that graph - by definition the components of the pair set
        ``score_above(E, E, thr, upper=True)`` returns, found in one pass and without the pair list.  The score is the inner product
        as ``score_above`` computes it, or - with ``stats``, the ``(mu, sigma)`` pair of ``asnorm_stats`` for E - the normalised score
        of ``score_topk_norm``; a NaN score links nothing.  Returns ``(root (N,) int32, cluster (N,) int32, n_clusters)``: the smallest
        row of each row's cluster, the dense id (clusters numbered in order of their smallest member) and the number of clusters.
        numpy in, numpy out (``n_clusters`` an int); a CUDA tensor in, CUDA tensors out (``n_clusters`` a 0-d int64 tensor)."""
        N, D = (int(x) for x in E.shape)
        thr = float(thr)
        if thr != thr:
            raise ValueError("cluster_above: the threshold is NaN")
        stats = () if stats is None else self._stat_pair("stats", stats, N)
        root, cluster, count = self._out(E, N, np.int32), self._out(E, N, np.int32), self._out(E, 1, np.int64)
        c = _Call(self, same_space=True)
        e = c.inp(E)
        sp = [c.inp(x) for x in stats] or [None] * 2
        r, cl, n = c.out(root, np.int32), c.out(cluster, np.int32), c.out(count, np.int64)
        c.run(self.lib.svhip_cluster_above, self.h, e, N, D, thr, *sp, r, cl, n)
        return root, cluster, (count[0] if _is_torch(count) else int(count[0]))

    def cluster_join(self, A, B, thr, root_a=None, root_b=None, a_stats=None, b_stats=None):
        """Two-set clustering (``svhip_cluster_join``): joins the rows B (NB, D) to a set A (NA, D) that may already be clustered,
        without scoring A against itself again.  The rows are numbered jointly - A's are ``0 .. NA - 1``, B's ``NA .. NA + NB - 1`` -
        and the clusters are the connected components of: the seed links of a side whose ``root_x`` is given (row i is linked to row
        ``root_x[i]`` of its side, ``0 <= root_x[i] <= i``: ``cluster_above``'s ``root``, or any downward parent-pointer forest; the
        side's own pairs are then NOT scored); the pairs ``i < j`` of a side without a seed, scored as ``cluster_above`` scores them;
        and every pair (row of A, row of B) whose score is at least ``thr``.  The score is ``score_above``'s for the query row of A
        and the gallery row of B, or - with ``a_stats`` and ``b_stats``, the ``(mu, sigma)`` pairs of ``asnorm_stats``, both or
        neither - the normalised score.  With seeds that are ``cluster_above``'s roots of their sides (or none) the result is exactly
        ``cluster_above`` of the concatenation.  A host seed with an entry outside ``[0, i]`` is refused by index; on the device such
        an entry is read as ``i``.  Returns ``(root (NA + NB,) int32, cluster (NA + NB,) int32, n_clusters)`` as ``cluster_above``
        does, in the inputs' memory space (all arrays in one)."""
        NA, D = (int(x) for x in A.shape)
        NB = int(B.shape[0])
        if int(B.shape[1]) != D:
            raise ValueError(f"cluster_join: A is {D} wide, B {int(B.shape[1])}")
        thr = float(thr)
        if thr != thr:
            raise ValueError("cluster_join: the threshold is NaN")
        if (a_stats is None) != (b_stats is None):
            raise ValueError("cluster_join: a_stats and b_stats go together: give both (normalised scores) or neither")
        stats = () if a_stats is None else self._stat_pair("a_stats", a_stats, NA) + self._stat_pair("b_stats", b_stats, NB)
        for name, seed, n in (("root_a", root_a, NA), ("root_b", root_b, NB)):
            if seed is not None and tuple(seed.shape) != (n,):
                raise ValueError(f"cluster_join: {name} must hold {n} values, not {tuple(seed.shape)}")
        N = NA + NB
        root, cluster, count = self._out(A, N, np.int32), self._out(A, N, np.int32), self._out(A, 1, np.int64)
        c = _Call(self, same_space=True)
        a, b = c.inp(A), c.inp(B)
        ra, rb = (None if x is None else c.inp(x, np.int32) for x in (root_a, root_b))
        sp = [c.inp(x) for x in stats] or [None] * 4
        r, cl, n = c.out(root, np.int32), c.out(cluster, np.int32), c.out(count, np.int64)
        c.run(self.lib.svhip_cluster_join, self.h, a, NA, ra, b, NB, rb, D, thr, *sp, r, cl, n)
        return root, cluster, (count[0] if _is_torch(count) else int(count[0]))

    _LINKAGES = {"average": _lib.LINKAGE_AVERAGE, "complete": _lib.LINKAGE_COMPLETE}

    def cluster_linkage(self, E, thr, stats=None, linkage="average"):
        """Speaker clustering that does not chain (``svhip_cluster_linkage``): average or complete linkage cut at ``thr``, run inside
        each component of ``cluster_above(E, thr, stats)`` - every merge of either linkage at a level of at least ``thr`` needs one pair
        that scores at least ``thr``, so no cluster leaves its component, and no N x N matrix is built.  Inside a component every row
        starts alone; the two clusters with the largest link value - the mean (``"average"``) or the minimum (``"complete"``) of the
        scores between them - are merged while that value is at least ``thr``, ties going to the pair with the smallest rows.  Returns
        ``(root, cluster, n_clusters, n_unrefined)``: the first three as ``cluster_above``; ``n_unrefined`` counts the components of
        more than ``_lib.LINKAGE_MAX_ROWS`` rows, which one workgroup cannot own and which stay one cluster each.  numpy in, numpy out
        (the counts ints); a CUDA tensor in, CUDA tensors out (the counts 0-d int64 tensors)."""
        N, D = (int(x) for x in E.shape)
        thr = float(thr)
        if thr != thr:
            raise ValueError("cluster_linkage: the threshold is NaN")
        if linkage not in self._LINKAGES:
            raise ValueError(f"cluster_linkage: linkage = {linkage!r} is neither 'average' nor 'complete'")
        stats = () if stats is None else self._stat_pair("stats", stats, N)
        root, cluster = self._out(E, N, np.int32), self._out(E, N, np.int32)
        count, unrefined = self._out(E, 1, np.int64), self._out(E, 1, np.int64)
        c = _Call(self, same_space=True)
        e = c.inp(E)
        sp = [c.inp(x) for x in stats] or [None] * 2
        r, cl, n, u = c.out(root, np.int32), c.out(cluster, np.int32), c.out(count, np.int64), c.out(unrefined, np.int64)
        c.run(self.lib.svhip_cluster_linkage, self.h, e, N, D, thr, *sp, self._LINKAGES[linkage], r, cl, n, u)
        if _is_torch(count):
            return root, cluster, count[0], unrefined[0]
        return root, cluster, int(count[0]), int(unrefined[0])

    @staticmethod
    def _audit_group_ptr(group_ptr, n_files):
        """``group_audit``'s group table as a contiguous host int64 array, checked by the C ABI's rules (a bad one is a
        ``ValueError`` that names the entry, raised before anything is allocated or launched)"""
        if _is_torch(group_ptr):
            group_ptr = group_ptr.detach().cpu().numpy()
        gp = np.ascontiguousarray(np.asarray(group_ptr).ravel(), dtype=np.int64)
        if gp.size < 1:
            raise ValueError("group_audit: group_ptr needs at least one entry (n_groups + 1)")
        if gp[0] != 0:
            raise ValueError(f"group_audit: group_ptr[0] = {int(gp[0])} is not 0")
        down = np.nonzero(np.diff(gp) < 0)[0]
        if down.size:
            g = int(down[0]) + 1
            raise ValueError(f"group_audit: group_ptr decreases at entry {g} ({int(gp[g])} after {int(gp[g - 1])})")
        if gp[-1] != n_files:
            raise ValueError(f"group_audit: group_ptr[n_groups] = {int(gp[-1])} is not n_files = {n_files}")
        return gp

    def group_audit(self, F, group_ptr, cut, scores=False):
        """Dataset audit (``svhip_group_audit``): F (n_files, n_crops, D) crop embeddings, the files sorted by group; ``group_ptr``
        (n_groups + 1, a host array whatever F is): group g is the files ``group_ptr[g]:group_ptr[g + 1]``.  The score of two files of
        one group is ``score_trials(mode="cosine")``'s mean |cos| over the aligned crops; they MISMATCH iff it is ``<= cut`` (a NaN
        score never is).  Returns ``miss`` (n_files,) int32: per file the number of OTHER files of its group it mismatches.  With
        ``scores=True``: ``(miss, score, score_ptr)``, ``score[score_ptr[g]:score_ptr[g + 1]]`` being the row-major n_g x n_g score
        block of group g (symmetric bit for bit; the diagonal is written and never counted).  numpy in, numpy out; a CUDA tensor in,
        CUDA tensors out (``score_ptr`` is always a host int64 array)."""
        if F.ndim != 3:
            raise ValueError(f"group_audit: F must be (n_files, n_crops, D), not {tuple(F.shape)}")
        n_files, n_crops, D = (int(x) for x in F.shape)
        gp = self._audit_group_ptr(group_ptr, n_files)
        if n_crops < 1 or D < 1:
            raise ValueError(f"group_audit: n_crops = {n_crops} and D = {D} must be at least 1")
        n_groups = gp.size - 1
        sizes = np.diff(gp)
        score_ptr = np.zeros(n_groups + 1, np.int64)
        np.cumsum(sizes * sizes, out=score_ptr[1:])
        miss = self._out(F, n_files, np.int32)
        score = self._out(F, int(score_ptr[-1])) if scores else None
        if n_files and n_groups:
            c = _Call(self, same_space=True)
            f, m = c.inp(F), c.out(miss, np.int32)
            s = c.out(score) if scores and score_ptr[-1] else None
            c.run(self.lib.svhip_group_audit, self.h, f, n_files, n_crops, D, c.host(gp), n_groups, float(cut), m, s)
        return (miss, score, score_ptr) if scores else miss

    # ---- verification metrics (host arrays in / out; the trial list is small next to the embeddings) --------------------
    def _scores_labels(self, scores, labels):
        if _is_torch(scores):
            scores = scores.detach().cpu().numpy()
        if _is_torch(labels):
            labels = labels.detach().cpu().numpy()
        s = np.ascontiguousarray(np.asarray(scores, dtype=np.float32).ravel())
        l = np.ascontiguousarray(np.asarray(labels).ravel().astype(np.int32))
        if s.shape != l.shape or s.size == 0:
            raise ValueError("scores and labels must be non-empty and of equal length")
        return s, l

    def roc_points(self, scores, labels):
        """-> (fps, tps, thresholds) of sklearn's _binary_clf_curve (float64 counts, highest threshold first)."""
        s, l = self._scores_labels(scores, labels)
        P = s.size
        thr = np.empty(P, np.float32)
        fps, tps = np.empty(P, np.int64), np.empty(P, np.int64)
        n = C.c_int64()
        self._ck(self.lib.svhip_roc_points(self.h, s.ctypes.data, l.ctypes.data, P, C.byref(n), thr.ctypes.data,
                                           fps.ctypes.data, tps.ctypes.data, 0))
        k = n.value
        return fps[:k].astype(np.float64), tps[:k].astype(np.float64), thr[:k].copy()

    def error_rates(self, scores, labels):
        """ComputeErrorRates (utils.py:221-256) -> (fnrs, fprs float64, thresholds float32), ascending thresholds."""
        s, l = self._scores_labels(scores, labels)
        P = s.size
        fnrs, fprs, thr = np.empty(P, np.float64), np.empty(P, np.float64), np.empty(P, np.float32)
        self._ck(self.lib.svhip_error_rates(self.h, s.ctypes.data, l.ctypes.data, P, fnrs.ctypes.data, fprs.ctypes.data,
                                            thr.ctypes.data, 0))
        return fnrs, fprs, thr

    def min_dcf(self, scores, labels, p_target, c_miss, c_fa):
        """ComputeErrorRates + ComputeMinDcf (utils.py:221-275) -> (min_dcf, threshold)."""
        s, l = self._scores_labels(scores, labels)
        d, t = C.c_double(), C.c_float()
        self._ck(self.lib.svhip_min_dcf(self.h, s.ctypes.data, l.ctypes.data, s.size, float(p_target), float(c_miss),
                                        float(c_fa), C.byref(d), C.byref(t), 0))
        return d.value, t.value

    def asnorm_stats(self, E, cohort, top=200):
        N, D = E.shape
        K = cohort.shape[0]
        mu, sd = self._out(E, (N,)), self._out(E, (N,))
        c = _Call(self, same_space=True)
        e, co, m, s = c.inp(E), c.inp(cohort), c.out(mu), c.out(sd)
        c.run(self.lib.svhip_asnorm_stats, self.h, e, N, D, co, K, int(top), m, s)
        return mu, sd

    @property
    def asnorm_last_fallback(self) -> int:
        """embeddings of the last asnorm_stats call that took the slab path after the fused kernel (-1: the whole call did)"""
        return int(self.lib.svhip_asnorm_last_fallback(self.h))

    @property
    def asnorm_last_refit(self):
        """(rows, passes): embeddings of the last asnorm_stats call that the fused kernel decided with a threshold re-derived from its own
        counts (non-Gaussian cohort scores), and the extra passes over them that took"""
        n = C.c_int32(0)
        rows = int(self.lib.svhip_asnorm_last_refit(self.h, C.byref(n)))
        return rows, int(n.value)

    def asnorm_pairs(self, E, mu, sigma, ia, ib, out=None):
        N, D = E.shape
        P = int(ia.shape[0])
        if out is None:
            out = self._out(E, (P,))
        c = _Call(self, same_space=True)
        e, m, s, a, b, o = c.inp(E), c.inp(mu), c.inp(sigma), c.inp(ia, np.int32), c.inp(ib, np.int32), c.out(out)
        c.run(self.lib.svhip_asnorm_pairs, self.h, e, N, D, m, s, a, b, P, o)
        return out

    # ---- introspection ------------------------------------------------------------------------------------------
    def get_stage(self, name: str) -> np.ndarray:
        n = C.c_int64()
        self._ck(self.lib.svhip_get_stage(self.h, name.encode(), None, C.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        self._ck(self.lib.svhip_get_stage(self.h, name.encode(), out.ctypes.data, C.byref(n)))
        return out

    def set_option(self, name: str, value: int):
        """Developer / test switch of this handle (``svhip_set_option``; the SVHIP_<NAME> environment variables are only the
        defaults a handle is created with)."""
        self._ck(self.lib.svhip_set_option(self.h, name.encode(), int(value)))

    def trim_scratch(self):
        """Free the scoring / metrics scratch the handle has grown (``svhip_trim_scratch``)."""
        self._ck(self.lib.svhip_trim_scratch(self.h))

    def profile(self, on=True, only=None):
        """HIP events around every kernel launch (``only``: just the launches with that label — fewer events in the stream)."""
        self._ck(self.lib.svhip_profile_filter(self.h, only.encode() if only else None))
        self._ck(self.lib.svhip_profile_enable(self.h, int(on)))
        if on:
            self._ck(self.lib.svhip_profile_reset(self.h))

    def profile_results(self):
        res = {}
        idx = 0
        name = C.create_string_buffer(64)
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        while self.lib.svhip_profile_get(self.h, idx, name, 64, C.byref(ms), C.byref(n), C.byref(fl)) == _lib.OK:
            res[name.value.decode()] = {"ms": ms.value, "launches": n.value, "flops": fl.value}
            idx += 1
        return res

    @property
    def flops_per_utterance(self) -> float:
        return float(self.lib.svhip_workload_flops(self.h))
