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
from ._base import HipModule, RaggedMixin

MIN_SAMPLES = 541

# the options MainModel takes and the only values this build runs (RawNet3.py:172-175)
_BUILT = dict(model_scale=8, context=True, summed=True, out_bn=False, log_sinc=True, norm_sinc="mean", grad_mult=1,
              encoder_type="ASP", sinc_stride=10)


class RawNet3(RaggedMixin, HipModule):
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

    # ---- ragged batches (RaggedMixin): the rows are the frames after the sinc filterbank -------------------------------------
    MIN_FRAMES = (MIN_SAMPLES - 251) // 10 + 1

    def ragged_frames(self, n_samples):
        """frames of an utterance of n_samples after the sinc filterbank; 0 below 541 samples (it fits no ragged call)"""
        return self.ragged_engine().frames_of(n_samples) if n_samples >= MIN_SAMPLES else 0

    def _ragged_limits(self):
        return f", at least {MIN_SAMPLES} samples each"


def MainModel(nOut=512, model_scale=8, context=True, summed=True, out_bn=False, log_sinc=True, norm_sinc="mean", grad_mult=1,
              encoder_type="ASP", sinc_stride=10, **kwargs):
    got = dict(model_scale=model_scale, context=context, summed=summed, out_bn=out_bn, log_sinc=log_sinc, norm_sinc=norm_sinc,
               grad_mult=grad_mult, encoder_type=encoder_type, sinc_stride=sinc_stride)
    other = {k: v for k, v in got.items() if v != _BUILT[k]}
    if other:
        raise NotImplementedError(f"RawNet3 is built for MainModel's defaults {_BUILT}; got {other}")
    return RawNet3(nOut=nOut, **kwargs)
