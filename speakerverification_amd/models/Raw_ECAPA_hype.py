"""Drop-in for the reference fusion plug-in ``models/Raw_ECAPA_hype.py`` (:18-87), the model of the saved experiment
``backup/20220709/save/Raw_ECAPA_hype``: ECAPA-TDNN (C = 512, 192-d, input norm) on the mel spectrogram of the waveform and RawNet2
(``front_proc='sinc'``, ``aggregate='gru'``, 512-d) on the raw waveform, mixed by a small attention head instead of concatenated:

    x   = lrelu_0.3(bn_before_agg([out1 | out2]))                  704 channels
    w   = softmax over the channels of attention(x)                Conv1d(704, 128, 1) -> SiLU -> BatchNorm1d -> Conv1d(128, 704, 1)
    out = fc(bn_final([x w | sqrt(clamp(x^2 w - (x w)^2, 1e-9))]))  (B, nOut)

    model = MainModel(nOut=512, features='raw', n_mels=80, audio_spec={...})
    emb = model(wav)            # (B, 16000) at 8 kHz x 2 s -> (B, 512); (512,) for B == 1

The head is one kernel of the library (csrc/fusion_head.hip) on a handle of its own (``Engine(model="fusion_head")``), fp32 whatever
``hip_compute`` says; ``hip_compute`` means for the branches what it means for Raw_ECAPA_sinc_gru.  State-dict keys: ``ECAPA_TDNN.*``
(233), ``rawnet2v2.*`` (144) and the head's 21 tensors at the top level; ``compute_features.*`` is accepted and ignored.  The shared
body is models/_fusion.py; the head is its ``_combine`` hook.
"""
from __future__ import annotations

import os
from collections import OrderedDict

import numpy as np

from .. import synth
from ..engine import Engine, _is_torch
from . import RawNet2_custom as _rawnet2
from ._fusion import RawECAPAFusion

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

RAW_DIM = 512          # the RawNet2 branch's nOut (Raw_ECAPA_hype.py:25): fixed, the model's nOut is the head's


class Raw_ECAPA(RawECAPAFusion):
    INPUT_NORM = True
    FRONT_PROC = "sinc"
    AGGREGATE = "gru"
    MODEL_NAME = "Raw_ECAPA_hype"

    def __init__(self, nOut=512, **kwargs):
        super().__init__(nOut=nOut, **kwargs)
        self.nOut = int(nOut)
        self._head_spec = OrderedDict((n, tuple(s)) for n, s in synth.hype_head_param_spec(self.nOut))
        self._head_sd = synth.synth_state_dict(list(self._head_spec.items()), seed=0)       # random init, like a fresh nn.Module
        self._head = None               # the head's handle, built on the first forward

    def _make_raw_branch(self, nOut, kw):
        return _rawnet2.MainModel(nOut=RAW_DIM, front_proc=self.FRONT_PROC, aggregate=self.AGGREGATE, att_dim=128, **kw)

    # ---- the head's handle: on the branches' device, with their max_batch; closed whenever theirs are ----------------------
    def _drop_head(self):
        if self._head is not None:
            self._head.close()
            self._head = None

    def _head_engine(self):
        dev, mb = self._raw._device, self._raw._max_batch
        if self._head is not None and (self._head.device, self._head.max_batch) != (dev, mb):
            self._drop_head()
        if self._head is None:
            # (samples: the smallest the library takes; the handle has no waveform model.  on_numeric: as the branches' fp32 handles)
            eng = Engine(model="fusion_head", compute="f32", channels=synth.HYPE_CONTEXT, embed_dim=self.nOut, max_batch=mb, samples=512,
                         device=dev, on_numeric="warn")
            eng.load_state_dict(self._head_sd)
            eng.finalize()
            self._head = eng
        return self._head

    def to(self, device=None, *a, **k):
        super().to(device, *a, **k)
        if self._head is not None and self._head.device != self._raw._device:
            self._drop_head()
        return self

    def _combine(self, o1, o2):
        """the attention head on the two branch outputs: CUDA tensors (complete: both branch handles have been waited for) stay on
        the device, numpy arrays go in and come out as numpy arrays; (B, nOut), (nOut,) for one utterance"""
        head = self._head_engine()
        if _is_torch(o1):
            o1, o2 = o1.reshape(-1, o1.shape[-1]).contiguous(), o2.reshape(-1, o2.shape[-1]).contiguous()
        else:
            o1, o2 = np.atleast_2d(o1), np.atleast_2d(o2)
        B, mb = o1.shape[0], head.max_batch
        parts = [head.fusion_head(o1[i:i + mb], o2[i:i + mb], ordered=True) for i in range(0, B, mb)]
        out = parts[0] if len(parts) == 1 else (torch.cat(parts, 0) if _is_torch(parts[0]) else np.concatenate(parts, 0))
        return out.squeeze() if _is_torch(out) else np.squeeze(out)        # out.squeeze(), Raw_ECAPA_hype.py:86

    # ---- nn.Module look-alikes: the branches' and the head's -----------------------------------------------------------------
    def parameters(self):
        yield from super().parameters()
        for k, v in self._head_sd.items():
            if v.dtype != np.int64 and "running_" not in k:
                yield (torch.from_numpy(v) if torch is not None else v)

    def state_dict(self):
        sd = super().state_dict()
        sd.update((k, torch.from_numpy(np.asarray(v)) if torch is not None else v) for k, v in self._head_sd.items())
        return sd

    def load_state_dict(self, sd, strict=True):
        head = {k: v for k, v in sd.items() if k in self._head_spec}
        rest = {k: v for k, v in sd.items() if k not in self._head_spec}
        missing = [k for k in self._head_spec if k not in head and "num_batches_tracked" not in k]
        if strict and missing:
            raise KeyError(f"state dict mismatch: missing {missing[:4]}...")
        done = super().load_state_dict(rest, strict=strict)        # (a stray key at the top level is the shared body's KeyError)
        unexpected = []
        for k, v in head.items():
            a = v.detach().cpu().numpy() if _is_torch(v) else np.asarray(v)
            if tuple(a.shape) != self._head_spec[k]:
                if strict:
                    raise ValueError(f"Wrong parameter length: {k}, model: {self._head_spec[k]}, loaded: {tuple(a.shape)}")
                unexpected.append(k)
                continue
            self._head_sd[k] = a.astype(np.int64) if a.dtype == np.int64 else np.ascontiguousarray(a, dtype=np.float32)
        self._drop_head()
        return done + ((missing, unexpected),)

    def load_blob(self, path):
        """the three blobs checkpoint.convert_checkpoint(..., model='Raw_ECAPA_hype') wrote for `path`: the branch pair and `.head`.
        ValueError when the head blob is absent (the likely cause: the pair was converted as Raw_ECAPA_sinc_gru, which has the same
        branches' names and no head) or is another model's; SVHIP_ERR_MISSING when it lacks a tensor of the head."""
        from .. import checkpoint, _lib
        p_head = checkpoint.fusion_blob_paths(path, self.MODEL_NAME)[2]
        if not os.path.exists(p_head):
            raise ValueError(f"{self.MODEL_NAME}: no {p_head} beside {path}: the pair was probably converted as Raw_ECAPA_sinc_gru, "
                             "which shares the branches' blob names and has no attention head; convert the checkpoint with "
                             "model='Raw_ECAPA_hype'")
        mid, head = checkpoint.read_blob(p_head)
        if mid != _lib.MODEL_FUSION_HEAD:
            raise ValueError(f"{p_head} holds weights of model {mid}, not the fusion head's ({_lib.MODEL_FUSION_HEAD})")
        done = super().load_blob(path)
        lacking = [k for k in self._head_spec if k not in head and "num_batches_tracked" not in k]
        if lacking:
            raise _lib.SvhipError(_lib.ERR_MISSING, f"{self.MODEL_NAME}: the head blob lacks {lacking[:4]} ({len(lacking)} tensors)")
        for k, v in head.items():
            if k in self._head_spec and tuple(v.shape) == self._head_spec[k]:
                self._head_sd[k] = v
        self._drop_head()
        return done + ((lacking, [k for k in head if k not in self._head_spec]),)


def MainModel(nOut=512, **kwargs):
    return Raw_ECAPA(nOut=nOut, **kwargs)
