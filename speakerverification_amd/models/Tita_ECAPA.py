"""Drop-in for the reference fusion plug-in ``models/Tita_ECAPA.py`` (class Raw_ECAPA there, :10-57): ECAPA-TDNN (C = 512, GELU,
192-d, ``input_norm=True``) and TitaNet-M (nOut - 192 dims), both on the mel spectrogram of the waveform, concatenated.

    model = MainModel(nOut=512, features='raw', n_mels=80, audio_spec={...})
    emb = model(wav)            # (B, 32000) -> (B, 512)

State-dict keys: ``ECAPA_TDNN.*`` and ``titaNet.*``; ``compute_features.*`` is ignored.  Each branch runs its own mel front-end on its
own handle (and, for device-resident batches, its own stream).  The shared body is models/_fusion.py.  Both branches have a ragged
forward, so ``embed_ragged`` / ``ragged_packer`` / ``ragged_frames`` are offered: whole files of different lengths share calls of the two
primary handles, one plan for both (ragged.FusionPacker).
"""
from __future__ import annotations

from . import TitaNet as _titanet
from ._fusion import RawECAPAFusion


class Tita_ECAPA(RawECAPAFusion):
    INPUT_NORM = True
    MODEL_NAME = "Tita_ECAPA"
    RAW_ATTR = "titaNet"

    def _make_raw_branch(self, nOut, kw):
        kw = {k: v for k, v in kw.items() if k not in ("model_size", "n_mega_blocks")}
        return _titanet.MainModel(nOut=nOut - 192, model_size="m", n_mega_blocks=None, **kw)

    def _raw_forward(self, x):
        return self._raw.embed_wave(x)           # compute_features, then titaNet (Tita_ECAPA.py:43-51)


def MainModel(nOut=512, **kwargs):
    return Tita_ECAPA(nOut=nOut, **kwargs)
