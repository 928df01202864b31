"""Shared body of the raw-waveform + ECAPA fusion plug-ins (reference ``models/Raw_ECAPA.py``, ``Raw_ECAPA_sinc_asp.py``,
``Raw_ECAPA_conv_asp.py``, each :22-52, and ``Raw3_ECAPA.py``): ECAPA-TDNN (C = 512, 192-d) on the mel spectrogram of the
waveform, concatenated with a raw-waveform network (nOut - 192 dims).  They differ in four switches:

    model                 ECAPA input_norm   raw branch (attribute)
    Raw_ECAPA             True               RawNet2 'sinc' / asp (rawnet2v2)
    Raw_ECAPA_sinc_asp    False              RawNet2 'sinc' / asp (rawnet2v2)
    Raw_ECAPA_sinc_gru    False              RawNet2 'sinc' / gru (rawnet2v2)
    Raw_ECAPA_hype        True               RawNet2 'sinc' / gru, 512-d (rawnet2v2); an attention head instead of the concatenation
    Raw_ECAPA_conv_asp    True               RawNet2 'conv' / asp (rawnet2v2)
    Raw3_ECAPA            True               RawNet3 (rawnet)
    Tita_ECAPA            True               TitaNet-M on the same mel spectrogram (titaNet)

``Raw_tita`` uses the same body with TitaNet-M (``titaNet``, 192-d) in place of the ECAPA branch and RawNet2 'sinc' / asp
(``RawNet``) as the second: FIRST_ATTR names the first branch and ``_make_first_branch`` builds it.

As in the reference the ECAPA branch inherits ``features`` from the config: with ``features: raw`` (what every fusion YAML
sets) it consumes the mel POWER without log / mean normalisation (ECAPA_TDNN.py:473).  Both branches read the same waveform;
the mel front-end and the ECAPA body run as one fused library call.  State-dict keys: ``ECAPA_TDNN.*`` and the raw branch's
attribute (``rawnet2v2.*`` or ``rawnet.*``); ``compute_features.*`` buffers of nnAudio are accepted and ignored (the front-end
tables are rebuilt from the config).
"""
from __future__ import annotations

import os

import numpy as np

from ..engine import _is_torch
from . import ECAPA_TDNN as _ecapa
from . import RawNet2_custom as _rawnet2

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


class RawECAPAFusion:
    accepts_device_wave = True      # both branches take CUDA tensors as raw device pointers
    INPUT_NORM = False              # ECAPA branch: InstanceNorm1d on its input (ECAPA_TDNN.py:406-409,477-478)
    FRONT_PROC = "sinc"             # RawNet2 branch front-end (RawNet2_custom.py:45-63)
    AGGREGATE = "asp"               # RawNet2 branch aggregation (RawNet2_custom.py:84-111)
    MODEL_NAME = "Raw_ECAPA_sinc_asp"
    RAW_ATTR = "rawnet2v2"          # the raw branch's attribute: the prefix of its state-dict keys
    FIRST_ATTR = "ECAPA_TDNN"       # the first (mel-spectrogram) branch's attribute

    def __init__(self, nOut=512, **kwargs):
        kw = dict(kwargs)
        kw.pop("channels", None)
        kw.pop("input_norm", None)
        setattr(self, self.FIRST_ATTR, self._make_first_branch(kw))
        setattr(self, self.RAW_ATTR, self._make_raw_branch(nOut, kw))
        self.training = False

    def _make_first_branch(self, kw):
        return _ecapa.MainModel(nOut=192, channels=[512, 512, 512, 512, 1536], input_norm=self.INPUT_NORM, **kw)

    def _make_raw_branch(self, nOut, kw):
        return _rawnet2.MainModel(nOut=nOut - 192, front_proc=self.FRONT_PROC, aggregate=self.AGGREGATE, att_dim=128, **kw)

    @property
    def _first(self):
        return getattr(self, self.FIRST_ATTR)

    @property
    def _raw(self):
        return getattr(self, self.RAW_ATTR)

    def _raw_forward(self, x):
        """the second branch on the waveform batch"""
        return self._raw(x)

    # nn.Module look-alikes --------------------------------------------------------------------------
    def to(self, device=None, *a, **k):
        self._first.to(device)
        self._raw.to(device)
        return self

    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("training is outside the scope of the MI355X inference path")
        return self

    def parameters(self):
        yield from self._first.parameters()
        yield from self._raw.parameters()

    def state_dict(self):
        sd = {self.FIRST_ATTR + "." + k: v for k, v in self._first.state_dict().items()}
        sd.update({self.RAW_ATTR + "." + k: v for k, v in self._raw.state_dict().items()})
        return sd

    def load_state_dict(self, sd, strict=True):
        pre1 = self.FIRST_ATTR + "."
        e = {k[len(pre1):]: v for k, v in sd.items() if k.startswith(pre1)}
        pre = self.RAW_ATTR + "."
        r = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        other = [k for k in sd if not k.startswith((pre1, pre, "compute_features."))]
        if strict and other:
            raise KeyError(f"unexpected keys {other[:4]}")
        m1 = self._first.load_state_dict(e, strict=strict)
        m2 = self._raw.load_state_dict(r, strict=strict)
        return m1, m2

    def load_blob(self, path):
        """the pair of branch blobs checkpoint.convert_checkpoint(..., model=MODEL_NAME) wrote for `path`.  A blob of another
        raw-waveform network (the other RawNet2 front-end, RawNet2 for RawNet3 or the other way round) raises ValueError; a blob that
        lacks a tensor this module needs (an ECAPA blob without instance_norm.* for a model with input_norm) raises the library's
        SVHIP_ERR_MISSING instead of running on the initial values."""
        from .. import checkpoint, _lib
        p_ecapa, p_raw = checkpoint.fusion_blob_paths(path, self.MODEL_NAME)[:2]
        if not os.path.exists(p_raw):
            raise ValueError(f"{self.MODEL_NAME}: no {p_raw} beside {path}: the pair was converted for another fusion model "
                             "(RawNet2 and RawNet3 branches are written as .rawnet2 / .rawnet3)")
        done = self._first.load_blob(p_ecapa), self._raw.load_blob(p_raw)
        for branch, (missing, _) in zip((self.FIRST_ATTR, self.RAW_ATTR), done):
            if missing:
                raise _lib.SvhipError(_lib.ERR_MISSING, f"{self.MODEL_NAME}: the {branch} blob lacks {missing[:4]} ({len(missing)} tensors)")
        return done

    def forward(self, x):
        if _is_torch(x) and x.is_cuda and x.ndim == 2 and self._raw.accepts_length(x.shape[1]):
            # device-resident batch: the two branches run CONCURRENTLY, each on its handle's own stream (RawNet2's small late
            # kernels beside ECAPA's GEMMs: 61 k instead of 55 k utt/s at B = 256)
            e1 = self._first._get_engine(x.shape[1], batch=x.shape[0])
            e2 = self._raw._engine_for(x)
            if x.shape[0] <= min(e1.max_batch, e2.max_batch) and x.dtype == torch.float32 and x.is_contiguous():
                torch.cuda.current_stream(x.device).synchronize()          # x is complete before either handle reads it
                o1 = torch.empty((x.shape[0], e1.embed_dim), device=x.device, dtype=torch.float32)
                o2 = torch.empty((x.shape[0], e2.embed_dim), device=x.device, dtype=torch.float32)
                e1.embed_wave(x, out=o1, async_=True, ordered=True)       # compute_features + ECAPA_TDNN (Raw_ECAPA_sinc_asp.py:41-44)
                e2.embed_wave(x, out=o2, async_=True, ordered=True)       # :48
                e1.synchronize()
                e2.synchronize()
                return self._combine(o1, o2).squeeze()
        out1 = self._first.embed_wave(x)              # compute_features + ECAPA_TDNN (Raw_ECAPA_sinc_asp.py:41-44)
        out2 = self._raw_forward(x)                   # :48
        return self._combine(out1, out2)

    def _combine(self, o1, o2):
        """what the model makes of its two branch outputs (CUDA tensors, complete, or numpy arrays; (B, d) or, squeezed, (d,)): the
        concatenation, torch.cat([out1, out2], dim=-1) (Raw_ECAPA_sinc_asp.py:50).  Raw_ECAPA_hype puts its attention head here."""
        if _is_torch(o1):
            return torch.cat([o1, o2], dim=-1)
        return np.concatenate([o1, o2], axis=-1)

    __call__ = forward

    # ---- ragged batches: whole files of different lengths in shared calls of BOTH branches' primary handles ---------------
    # Offered only when both branches have embed_ragged (ECAPA-TDNN + RawNet3: Raw3_ECAPA; ECAPA-TDNN + TitaNet: Tita_ECAPA; ECAPA-TDNN +
    # RawNet2 'conv': Raw_ECAPA_conv_asp); on the fusions with a RawNet2 'sinc' branch (Raw_ECAPA, Raw_ECAPA_sinc_asp, Raw_ECAPA_sinc_gru,
    # Raw_tita: LayerNorm(nb_samp) fixes that branch's length) these attributes do not exist (__getattr__), so whole-file evaluation
    # keeps the per-file path there.
    _RAGGED = ("ragged_packer", "ragged_frames", "embed_ragged")

    def __getattr__(self, name):
        if name in RawECAPAFusion._RAGGED:
            d = self.__dict__
            if all(hasattr(d.get(a), "embed_ragged") for a in (self.FIRST_ATTR, self.RAW_ATTR)):
                return getattr(self, "_fusion_" + name)
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def _fusion_ragged_packer(self):
        from ..ragged import FusionPacker
        return FusionPacker(self._first.ragged_packer(), self._raw.ragged_packer())

    def _fusion_ragged_frames(self, n_samples):
        """the packer's unit: (frames of the first branch, frames of the raw branch); a 0 fits no ragged call"""
        return self._first.ragged_frames(n_samples), self._raw.ragged_frames(n_samples)

    def _fusion_embed_ragged(self, wavs):
        """list of 1-D waveforms of any lengths -> (n, nOut): one plan for both branches, [first | raw] per utterance.  CUDA
        waveforms keep forward's two-stream overlap (each branch on its handle's own stream); otherwise the branches run one
        after the other.  Raises ValueError for utterances that fit no call of either branch."""
        from ..ragged import plan_packed
        calls, alone = plan_packed([self._fusion_ragged_frames(w.shape[-1]) for w in wavs], self._fusion_ragged_packer())
        if alone:
            raise ValueError(f"utterances {alone[:8]} fit no ragged call of both branches")
        e1, e2 = self._first.ragged_engine(), self._raw.ragged_engine()
        # a raw branch that owns a fallback (RawNet2 'conv': an fp16 handle that overflows is rebuilt in another compute) makes its own
        # call on the shared pack, so that the fallback works here as in its embed_ragged
        raw_call = getattr(self._raw, "ragged_call", None)
        outs = []
        for call in calls:
            group = [wavs[i].reshape(-1) for i in call]
            if _is_torch(group[0]) and group[0].is_cuda:
                lens = np.asarray([g.shape[0] for g in group], dtype=np.int32)
                offs = np.zeros(len(group), dtype=np.int64)
                offs[1:] = np.cumsum(lens[:-1], dtype=np.int64)
                packed = torch.cat([g.to(torch.float32) for g in group])
                torch.cuda.current_stream(packed.device).synchronize()     # the pack is complete before either handle reads it
                o1 = torch.empty((len(group), e1.embed_dim), device=packed.device, dtype=torch.float32)
                o2 = torch.empty((len(group), e2.embed_dim), device=packed.device, dtype=torch.float32)
                e1.embed_wave_ragged(packed, offs, lens, out=o1, async_=True, ordered=True)
                if raw_call:
                    raw_call(packed, offs, lens, out=o2, ordered=True)      # on its handle's own stream, beside e1's; waited for inside
                else:
                    e2.embed_wave_ragged(packed, offs, lens, out=o2, async_=True, ordered=True)
                e1.synchronize()
                if not raw_call:
                    e2.synchronize()
                outs.append(torch.cat([o1, o2], dim=-1))
            else:
                packed, offs, lens = e1._pack(group, None, None, True)      # packed once, read by both branches
                o1 = e1.embed_wave_ragged(packed, offs, lens)
                o2 = raw_call(packed, offs, lens) if raw_call else e2.embed_wave_ragged(packed, offs, lens)
                outs.append(torch.cat([o1, o2], dim=-1) if _is_torch(o1) else np.concatenate([o1, o2], axis=-1))
        if len(outs) == 1:
            return outs[0]
        return torch.cat(outs, 0) if _is_torch(outs[0]) else np.concatenate(outs, 0)
