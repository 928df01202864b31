"""Drop-in for the reference fusion plug-in ``models/Raw3_ECAPA.py``, the model of the reference's default configs
(yaml/configuration.yaml, yaml/verification-voxceleb.yaml): ECAPA-TDNN (C = 512, 192-d, ``input_norm=True``) on the mel
spectrogram of the waveform, concatenated with RawNet3 (MainModel's defaults, nOut - 192 dims) on the raw waveform.

    model = MainModel(nOut=512, features='raw', n_mels=80, audio_spec={...})
    emb = model(wav)            # (B, 32000) -> (B, 512)

State-dict keys: ``ECAPA_TDNN.*`` (233 tensors with instance_norm.*) and ``rawnet.*`` (234); ``compute_features.*`` is ignored.
The shared body is models/_fusion.py.
"""
from __future__ import annotations

from . import RawNet3 as _rawnet3
from ._fusion import RawECAPAFusion


class Raw3_ECAPA(RawECAPAFusion):
    INPUT_NORM = True
    MODEL_NAME = "Raw3_ECAPA"
    RAW_ATTR = "rawnet"

    def _make_raw_branch(self, nOut, kw):
        # (Raw3_ECAPA.py passes RawNet3.MainModel's defaults explicitly; 'half' is bf16 on this branch)
        return _rawnet3.MainModel(nOut=nOut - 192, **kw)


def MainModel(nOut=512, **kwargs):
    return Raw3_ECAPA(nOut=nOut, **kwargs)
