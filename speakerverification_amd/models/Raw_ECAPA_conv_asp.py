"""Drop-in for the reference fusion plug-in ``models/Raw_ECAPA_conv_asp.py`` (:22-52), the model the
reference's training configs name (yaml/configuration-voxceleb.yaml, yaml/configuration-vlsp.yaml):
ECAPA-TDNN (C = 512, 192-d) with ``input_norm=True`` on the mel spectrogram of the waveform, concatenated
with RawNet2 (``front_proc='conv'``, asp, nOut - 192 dims) on the raw waveform.

    model = MainModel(nOut=512, features='raw', n_mels=80, audio_spec={...})
    emb = model(wav)            # (B, L) -> (B, 512), any L >= 2187

The conv front-end has no LayerNorm(nb_samp), so any length of at least 2187 samples runs (one library
handle per length; the configured crop length keeps the full batch workspace).  374 state-dict tensors
(233 ECAPA with instance_norm.*, 140 RawNet2, compute_features.*, which is ignored).  The shared body is
models/_fusion.py.
"""
from __future__ import annotations

from ._fusion import RawECAPAFusion


class Raw_ECAPA(RawECAPAFusion):
    INPUT_NORM = True
    FRONT_PROC = "conv"
    MODEL_NAME = "Raw_ECAPA_conv_asp"


def MainModel(nOut=512, **kwargs):
    return Raw_ECAPA(nOut=nOut, **kwargs)
