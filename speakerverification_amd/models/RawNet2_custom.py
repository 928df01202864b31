"""Drop-in for the reference plug-in ``models/RawNet2_custom.py`` (MainModel :230-243) in the variants
the fusion models and configs instantiate: ``aggregate='asp'``, ``att_dim=128`` with ``front_proc='sinc'``
(Raw_ECAPA_sinc_asp.py / Raw_ECAPA.py:26-28) or ``front_proc='conv'`` (Raw_ECAPA_conv_asp.py:26-28), and
``aggregate='gru'`` with ``front_proc='sinc'`` — the reference's defaults (RawNet2_custom.py:18-31; Raw_ECAPA_sinc_gru.py).

    model = MainModel(nOut=320, front_proc='sinc', aggregate='asp', att_dim=128, audio_spec={...})
    emb = model(wav)          # (B, 32000) waveform -> (B, nOut); (nOut,) for B == 1

State-dict keys are the reference's: 147 tensors for 'sinc' (the band-pass filters are rebuilt from
``first_conv.low_hz_`` / ``band_hz_`` once per weight load instead of once per forward), 140 for 'conv'
(``conv1.weight`` / ``conv1.bias``), 144 for 'sinc' + 'gru' (``bn_before_gru``, ``gru.*``, ``fc_after_gru``;
``fc`` is built and never used, as in the reference).  The sinc filters are baked at ``audio_spec['sample_rate']``, as the
reference's SincConv_fast builds them (RawNet2_custom.py:55-67; 8000 in every saved experiment).  The sinc form's LayerNorm(nb_samp) fixes the input length; the conv
form takes any length L >= 2187 (one library handle per length, the configured crop length with the
full batch workspace) and, alone of the three, offers ``embed_ragged``: utterances of different lengths in shared calls of the
primary handle (whole-file evaluation; ``RawNet2Conv``).
"""
from __future__ import annotations

from .. import synth
from ..engine import _RAGGED
from ._base import HipModule, RaggedMixin


# the conv front-end's shortest input: floor(L / 3) frames must survive six max_pool1d(3) stages (the reference raises below it)
CONV_MIN_SAMPLES = 3 * 3 ** 6


class RawNet2(HipModule):
    model_kind = "rawnet2"

    def __init__(self, nOut=512, front_proc="sinc", aggregate="gru", att_dim=128, audio_spec=None, device=None,
                 compute=None, max_batch=None, nb_gru_layers=1, gru_node=1024, **kwargs):
        if front_proc not in ("sinc", "conv") or aggregate not in ("asp", "gru") or (aggregate == "asp" and att_dim != 128):
            raise NotImplementedError("only front_proc='sinc' | 'conv' with aggregate='asp', att_dim=128, and front_proc='sinc' with "
                                      "aggregate='gru' are built (Raw_ECAPA_sinc_asp.py / Raw_ECAPA_conv_asp.py / Raw_ECAPA_sinc_gru.py)")
        if aggregate == "gru" and (front_proc != "sinc" or gru_node != 1024 or nb_gru_layers != 1):
            raise NotImplementedError("aggregate='gru' is built with front_proc='sinc', gru_node=1024 and nb_gru_layers=1 "
                                      "(RawNet2_custom.py:18-31 defaults)")
        self.front_proc = front_proc
        self.aggregate = aggregate
        if aggregate == "gru":
            self.model_kind = "rawnet2_gru"
        if front_proc == "conv":
            self.model_kind = "rawnet2_conv"
            # no LayerNorm(nb_samp): any length; the configured crop length (if the config gives one) gets the full workspace
            spec_samples = int(audio_spec["sentence_len"] * audio_spec["sample_rate"]) if audio_spec else None
            if spec_samples is not None and spec_samples < CONV_MIN_SAMPLES:
                raise ValueError(f"audio_spec gives {spec_samples} samples; RawNet2 (front_proc='conv') needs at least {CONV_MIN_SAMPLES}")
            self.nb_samp = spec_samples
        else:
            audio_spec = audio_spec or {"sample_rate": 16000, "sentence_len": 2.0}
            self.nb_samp = int(audio_spec["sentence_len"] * audio_spec["sample_rate"])      # LayerNorm(nb_samp), :58-60
        # hip_compute: "f32" (exact fp32 MFMA) | "f32x3" | "f16" (fp16 storage + fp16 MFMA: RawNet2's fast mode) | "bf16" (the same
        # kernels on bf16: range-safe, but RawNet2 loses two digits to bf16 weight rounding) | "half" = this model's 16-bit mode (f16)
        compute = compute or kwargs.get("hip_compute", "f32")
        compute = {"half": "f16", "fp16": "f16"}.get(compute, compute)
        # range_fallback (round 6): what an fp16 handle that reports an overflow (SVHIP_ERR_NONFINITE: this checkpoint's activations pass
        # 65504) is replaced by — a NEW handle in that mode, with a warning; None re-raises.  "f32" is the exact mode; "bf16" is range-safe and
        # fast but loses accuracy on RawNet2 (bf16 weight rounding: cosine 0.995 to fp32 on a well-scaled checkpoint, 0.7 - 0.97 on the
        # ill-scaled one of tests/test_gpu_rawnet2.py), so it is not the default
        self._range_fallback = kwargs.get("range_fallback", "f32")
        max_batch = int(max_batch or kwargs.get("embed_batch", 256))
        # SincConv_fast takes audio_spec['sample_rate'] (RawNet2_custom.py:55-67): the handle bakes its filters at that rate
        sinc_sr = int(audio_spec["sample_rate"]) if front_proc == "sinc" else 16000
        super().__init__(synth.rawnet2_param_spec(nOut=nOut, nb_samp=self.nb_samp or 0, att_dim=att_dim, front_proc=front_proc,
                                                  aggregate=aggregate),
                         dict(embed_dim=nOut, sinc_sr=sinc_sr), device=device if device is not None else kwargs.get("device"),
                         compute=compute, max_batch=max_batch, primary_samples=self.nb_samp, sample_rate=sinc_sr)

    def _check_input(self, x):
        """-> the input length; raises ValueError (before any handle is made) for a shape this module cannot run"""
        if self.front_proc == "conv":
            if x.ndim != 2 or x.shape[1] < CONV_MIN_SAMPLES:
                raise ValueError(f"RawNet2 (front_proc='conv') takes (batch, L >= {CONV_MIN_SAMPLES}) waveforms, got {tuple(x.shape)} "
                                 "(floor(L / 3) frames pass six max_pool1d(3) stages)")
            return int(x.shape[1])
        if x.ndim != 2 or x.shape[1] != self.nb_samp:
            raise ValueError(f"RawNet2 was built for (batch, {self.nb_samp}) waveforms, got {tuple(x.shape)} "
                             "(LayerNorm gamma/beta fix the length, RawNet_baseline.py:16-18)")
        return self.nb_samp

    def accepts_length(self, L):
        """can a (batch, L) waveform run (the sinc form: L == nb_samp; the conv form: L >= 2187)"""
        return L >= CONV_MIN_SAMPLES if self.front_proc == "conv" else L == self.nb_samp

    def _engine_for(self, x):
        L = self._check_input(x)
        return self._get_engine(L) if self.front_proc == "sinc" else self._get_engine(L, batch=x.shape[0])

    def _with_range_fallback(self, call):
        """call() — which looks its handle up itself — and, when an fp16 handle reports an overflow (SVHIP_ERR_NONFINITE) and
        range_fallback is set: a warning, this module's handles rebuilt in the fallback compute, and that call once more"""
        from .._lib import SvhipNumericError, ERR_NONFINITE
        try:
            return call()
        except SvhipNumericError as e:
            if e.code != ERR_NONFINITE or self._compute != "f16" or not self._range_fallback:
                raise
            import warnings
            warnings.warn(f"RawNet2 fp16 handle: {e}; rebuilding this module's handle with compute = {self._range_fallback!r} "
                          "(every later forward runs in that mode)", RuntimeWarning, stacklevel=3)
            self._compute = self._range_fallback
            self._drop_engine()
            return call()

    def forward(self, x):
        def call():
            eng = self._engine_for(x)
            return self._squeeze(self._batched(eng.embed_wave, x, eng.max_batch))
        return self._with_range_fallback(call)


class RawNet2Conv(RaggedMixin, RawNet2):
    """front_proc='conv': no LayerNorm(nb_samp) in front, so any length runs and files of different lengths ride in shared calls of
    the primary handle (RaggedMixin).  The rows of a call are the frames after the conv front-end, floor(L / 3); the fp16 range
    fallback of ``forward`` covers the ragged calls too, also when a fusion model drives this branch (``ragged_call``)."""

    MIN_FRAMES = 3 ** 6             # 729 front-end frames: one frame reaches the aggregation

    def ragged_frames(self, n_samples):
        """frames of an utterance of n_samples after the conv front-end; 0 below 2187 samples (it fits no ragged call)"""
        return _RAGGED["rawnet2_conv"].frames(int(n_samples), 0) if n_samples >= CONV_MIN_SAMPLES else 0

    def _ragged_limits(self):
        return f", at least {CONV_MIN_SAMPLES} samples each"

    def _embed_ragged_call(self, group):
        return self._with_range_fallback(lambda: self.ragged_engine().embed_wave_ragged(group))

    def ragged_call(self, packed, offsets, lengths, out=None, ordered=False):
        """one ragged call of the primary handle on a pack somebody else made (a fusion model's, shared with its other branch).
        ``ordered``: the device buffers are complete (Engine.embed_wave_ragged) — the call is enqueued on the handle's own stream and
        waited for here, so that an overflow is reported, and the call redone, before the caller reads ``out``."""
        def call():
            eng = self.ragged_engine()
            if not ordered:
                return eng.embed_wave_ragged(packed, offsets, lengths, out=out)
            res = eng.embed_wave_ragged(packed, offsets, lengths, out=out, async_=True, ordered=True)
            eng.synchronize()
            return res
        return self._with_range_fallback(call)


def MainModel(nOut=512, front_proc="sinc", **kwargs):
    """only the conv form has the ragged surface: hasattr(model, "embed_ragged") is how model.py and _fusion.py ask"""
    cls = RawNet2Conv if front_proc == "conv" else RawNet2
    return cls(nOut=nOut, front_proc=front_proc, **kwargs)
