"""Drop-in for the reference fusion plug-in ``models/Raw_tita.py`` (:10-52): TitaNet-M (192-d) on the mel spectrogram of the
waveform, concatenated with RawNet2 (``front_proc='sinc'``, ``aggregate='asp'``, nOut - 192 dims) on the raw waveform.

    model = MainModel(nOut=512, n_mels=80, audio_spec={...})
    emb = model(wav)            # (B, 32000) -> (B, 512) = [titaNet | RawNet]

State-dict keys: ``titaNet.*`` and ``RawNet.*``; ``compute_features.*`` is ignored.  The shared body is models/_fusion.py (with TitaNet
as its first branch).  Under 'half' TitaNet runs bf16 and RawNet2 its own 16-bit mode (f16).
"""
from __future__ import annotations

from . import TitaNet as _titanet
from ._fusion import RawECAPAFusion


class Raw_tita(RawECAPAFusion):
    MODEL_NAME = "Raw_tita"
    FIRST_ATTR = "titaNet"
    RAW_ATTR = "RawNet"
    FRONT_PROC = "sinc"
    AGGREGATE = "asp"

    def _make_first_branch(self, kw):
        kw = {k: v for k, v in kw.items() if k not in ("model_size", "n_mega_blocks")}
        return _titanet.MainModel(nOut=192, model_size="m", n_mega_blocks=None, **kw)


def MainModel(nOut=512, **kwargs):
    return Raw_tita(nOut=nOut, **kwargs)
