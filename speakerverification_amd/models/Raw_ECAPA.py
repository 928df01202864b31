"""Drop-in for the reference fusion plug-in ``models/Raw_ECAPA.py`` (:22-52), the model the reference's
inference configs name (yaml/verification.yaml, yaml/verification_config.yaml): ECAPA-TDNN (C = 512,
192-d) with ``input_norm=True`` on the mel spectrogram of the waveform, concatenated with RawNet2
(sinc / asp, nOut - 192 dims) on the raw waveform.

    model = MainModel(nOut=512, features='raw', n_mels=80, audio_spec={...})
    emb = model(wav)            # (B, 32000) -> (B, 512)

381 state-dict tensors (233 ECAPA with instance_norm.*, 147 RawNet2, compute_features.*, which is ignored).
The shared body is models/_fusion.py.
"""
from __future__ import annotations

from ._fusion import RawECAPAFusion


class Raw_ECAPA(RawECAPAFusion):
    INPUT_NORM = True
    FRONT_PROC = "sinc"
    MODEL_NAME = "Raw_ECAPA"


def MainModel(nOut=512, **kwargs):
    return Raw_ECAPA(nOut=nOut, **kwargs)
