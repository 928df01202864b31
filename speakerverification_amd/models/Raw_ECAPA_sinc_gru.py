"""Drop-in for the reference fusion plug-in ``models/Raw_ECAPA_sinc_gru.py`` (:22-52), the model ``yaml/dataprep.yaml``
names: ECAPA-TDNN (C = 512, 192-d, no input norm) on the mel spectrogram of the waveform, concatenated with RawNet2
(``front_proc='sinc'``, ``aggregate='gru'``, nOut - 192 dims) on the raw waveform.

    model = MainModel(nOut=512, features='raw', n_mels=80, audio_spec={...})
    emb = model(wav)            # (B, 32000) -> (B, 512)

375 state-dict tensors (231 ECAPA, 144 RawNet2 with bn_before_gru, gru.*, fc_after_gru and the unused fc; compute_features.*
is ignored).  The shared body is models/_fusion.py.
"""
from __future__ import annotations

from ._fusion import RawECAPAFusion


class Raw_ECAPA(RawECAPAFusion):
    INPUT_NORM = False
    FRONT_PROC = "sinc"
    AGGREGATE = "gru"
    MODEL_NAME = "Raw_ECAPA_sinc_gru"


def MainModel(nOut=512, **kwargs):
    return Raw_ECAPA(nOut=nOut, **kwargs)
