"""Drop-in for the reference plug-in ``models/RawNet3.py`` (MainModel :172-186) with its defaults, the raw-waveform
branch of ``Raw3_ECAPA`` (the model of the reference's default configs):

    model = MainModel(nOut=320)
    emb = model(wav)          # (B, L) waveform -> (B, nOut); (nOut,) for B == 1

234 state-dict tensors under the reference's names (``bn1.*`` and ``bn6.*`` are accepted and unused, as in the reference's
forward).  The sinc filterbank ``ParamSincFB(256, 251, stride=10)`` is rebuilt from ``conv1.filterbank.{low_hz_, band_hz_,
window_, n_}`` once per weight load.  Any length L >= 541 runs (``forward``: one library handle per length; the reference's own
output is non-finite below that, where one frame reaches the unbiased variance of the context pooling).  ``embed_ragged`` embeds
utterances of different lengths in shared calls of the primary handle (whole-file evaluation).  Computes: "f32" (the filterbank
sums in fp64) and "bf16" ("half" means bf16 here).
"""
from __future__ import annotations

from .. import synth
from ._base import HipModule

MIN_SAMPLES = 541

# the options MainModel takes and the only values this build runs (RawNet3.py:172-175)
_BUILT = dict(model_scale=8, context=True, summed=True, out_bn=False, log_sinc=True, norm_sinc="mean", grad_mult=1,
              encoder_type="ASP", sinc_stride=10)


class RawNet3(HipModule):
    model_kind = "rawnet3"

    def __init__(self, nOut=512, device=None, compute=None, max_batch=None, audio_spec=None, **kwargs):
        compute = compute or kwargs.get("hip_compute", "f32")
        compute = {"half": "bf16", "fp32": "f32"}.get(compute, compute)
        if compute not in ("f32", "bf16"):
            raise NotImplementedError(f"RawNet3 runs in 'f32' or 'bf16' (got {compute!r})")
        spec_samples = int(audio_spec["sentence_len"] * audio_spec["sample_rate"]) if audio_spec else None
        if spec_samples is not None and spec_samples < MIN_SAMPLES:
            raise ValueError(f"audio_spec gives {spec_samples} samples; RawNet3 needs at least {MIN_SAMPLES}")
        max_batch = int(max_batch or kwargs.get("embed_batch", 256))
        super().__init__(synth.rawnet3_param_spec(nOut=nOut), dict(embed_dim=nOut, channels=1024),
                         device=device if device is not None else kwargs.get("device"),
                         compute=compute, max_batch=max_batch, primary_samples=spec_samples)

    def _check_input(self, x):
        if x.ndim != 2 or x.shape[1] < MIN_SAMPLES:
            raise ValueError(f"RawNet3 takes (batch, L >= {MIN_SAMPLES}) waveforms, got {tuple(x.shape)}")
        return int(x.shape[1])

    def accepts_length(self, L):
        return L >= MIN_SAMPLES

    def _engine_for(self, x):
        return self._get_engine(self._check_input(x), batch=x.shape[0])

    def forward(self, x):
        eng = self._engine_for(x)
        return self._squeeze(self._batched(eng.embed_wave, x, eng.max_batch))

    # ---- ragged batches: utterances of different lengths on the PRIMARY handle (whole-file evaluation) ----------------
    DEFAULT_PRIMARY = 32000         # the primary geometry when no audio_spec names one: the reference's 2 s crop at 16 kHz

    def ragged_engine(self):
        """the handle with the full max_batch workspace: its level-0 rows are the capacity of a ragged call"""
        return self._get_engine(self._primary or self.DEFAULT_PRIMARY)

    def ragged_packer(self):
        from ..ragged import RaggedPacker
        eng = self.ragged_engine()
        return RaggedPacker(eng.max_batch, eng.row_capacity, min_frames=eng.frames_of(MIN_SAMPLES))

    def ragged_frames(self, n_samples):
        """frames of an utterance of n_samples after the sinc filterbank; 0 below 541 samples (it fits no ragged call)"""
        return self.ragged_engine().frames_of(n_samples) if n_samples >= MIN_SAMPLES else 0

    def embed_ragged(self, wavs):
        """list of 1-D waveforms of any lengths -> (n, nOut), each embedded as if alone at its own length, in as few library calls
        as the primary handle's capacity allows (ragged.plan_ragged).  Raises ValueError for utterances that fit no call: the
        caller embeds those through forward, which builds a handle for their length."""
        from ..ragged import plan_ragged
        eng = self.ragged_engine()
        calls, alone = plan_ragged([self.ragged_frames(w.shape[-1]) for w in wavs], eng.max_batch, eng.row_capacity,
                                   min_frames=eng.frames_of(MIN_SAMPLES))
        if alone:
            raise ValueError(f"utterances {alone[:8]} fit no ragged call of this handle ({eng.row_capacity} frames, "
                             f"at least {MIN_SAMPLES} samples each)")
        outs = [eng.embed_wave_ragged([wavs[i].reshape(-1) for i in call]) for call in calls]
        if len(outs) == 1:
            return outs[0]
        import numpy as np
        from ..engine import _is_torch
        import torch
        return torch.cat(outs, 0) if _is_torch(outs[0]) else np.concatenate(outs, 0)


def MainModel(nOut=512, model_scale=8, context=True, summed=True, out_bn=False, log_sinc=True, norm_sinc="mean", grad_mult=1,
              encoder_type="ASP", sinc_stride=10, **kwargs):
    got = dict(model_scale=model_scale, context=context, summed=summed, out_bn=out_bn, log_sinc=log_sinc, norm_sinc=norm_sinc,
               grad_mult=grad_mult, encoder_type=encoder_type, sinc_stride=sinc_stride)
    other = {k: v for k, v in got.items() if v != _BUILT[k]}
    if other:
        raise NotImplementedError(f"RawNet3 is built for MainModel's defaults {_BUILT}; got {other}")
    return RawNet3(nOut=nOut, **kwargs)
