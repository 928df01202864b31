"""Drop-in for the reference fusion plug-in ``models/Raw_ECAPA_sinc_asp.py`` (:22-52): the repo's
production model — ECAPA-TDNN (C = 512, 192-d, no input norm) on the mel spectrogram of the waveform,
concatenated with RawNet2 (sinc / asp, nOut - 192 dims) on the raw waveform.

    model = MainModel(nOut=512, features='raw', n_mels=80, audio_spec={...})
    emb = model(wav)            # (B, 32000) -> (B, 512)

The shared body (forward, state dict, blob pair, the two-stream CUDA path) is models/_fusion.py.
"""
from __future__ import annotations

from ._fusion import RawECAPAFusion


class Raw_ECAPA(RawECAPAFusion):
    INPUT_NORM = False
    FRONT_PROC = "sinc"
    MODEL_NAME = "Raw_ECAPA_sinc_asp"


def MainModel(nOut=512, **kwargs):
    return Raw_ECAPA(nOut=nOut, **kwargs)
