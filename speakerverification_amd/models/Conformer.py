"""Drop-in for the reference plug-in ``models/Conformer.py`` (MainModel :100-102, Conformer_ :13-97), the model of
``yaml/model_plot.yaml``:

    model = MainModel(nOut=512, n_mels=80, features='melspectrogram', device='cuda')
    emb = model(mel)            # (B, n_mels, T) mel POWER -> (B, nOut); (nOut,) for B == 1
    emb = model.embed_wave(wav) # (B, L) waveform -> mel front-end + the net in one library call

The front-end takes log(x + 1e-6) and the time mean off only for ``features='melspectrogram'``, then InstanceNorm1d(n_mels, affine), as
the reference.  Six Conformer blocks (d_model 256, 4 heads, relative positions with the reference's own shift), attentive statistics
pooling with the variance clamped to [1e-4, 1e4], attention_norm and fc.  State-dict keys are the reference's (asp.* / asp_bn.* are
loaded and ignored, as the reference never calls them).  Computes: "f32" and "bf16" ("half" means bf16 here).  Lengths: L >= 512
samples (the library's front-end; the reference needs T >= 7 frames) and T' <= 10000 (the positional-encoding buffer).
``embed_ragged`` embeds utterances of different lengths in shared calls of the primary handle (whole-file evaluation).
SpecAugment (``augment=True`` with 'spec_domain') is not built.
"""
from __future__ import annotations

from .. import synth
from ._base import HipModule, RaggedMixin

MIN_SAMPLES = 512           # the mel front-end's n_fft (one frame of the library's front-end)


def slice_frames(max_batch, frames, n_mels, compute):
    """subsampled frames one subsampling slice of a handle of `frames` mel frames holds (csrc/api_conformer.hip: cf_chunk utterances
    of the handle's own T'): the longest utterance a ragged call of that handle takes"""
    sub = lambda n: (n - 3) // 2 + 1
    per_utt = sub(frames) * sub(n_mels) * synth.CONFORMER_D * (2 if compute == "bf16" else 4)      # conv1 output bytes of one utterance
    return max(1, min(int(max_batch), (256 << 20) // per_utt)) * synth.conformer_frames(frames)


def ragged_frames_of(n_samples, hop, n_fft, slice_limit):
    """mel frames of an utterance of n_samples, or 0 when it fits no ragged call: shorter than one FFT window or 7 frames, more than
    10000 subsampled frames, or more of them than one subsampling slice holds"""
    if n_samples < n_fft:
        return 0
    T = int(n_samples) // int(hop) + 1
    return T if 1 <= synth.conformer_frames(T) <= min(synth.CONFORMER_MAX_T, slice_limit) else 0


def _crop_samples(audio_spec):
    try:
        return int(audio_spec["sentence_len"] * audio_spec["sample_rate"])
    except Exception:
        return None


class Conformer(RaggedMixin, HipModule):
    model_kind = "conformer"

    def __init__(self, nOut=512, input_size=80, attention_dim=128, device=None, compute=None, max_batch=None, **kwargs):
        if int(attention_dim) != 128:
            raise NotImplementedError(f"Conformer is built for attention_dim = 128 (got {attention_dim})")
        chain = (kwargs.get("augment_options") or {}).get("augment_chain") or []
        if kwargs.get("augment") and "spec_domain" in chain:
            raise NotImplementedError("SpecAugment ('spec_domain' in augment_chain) is outside the inference hot path")
        n_mels = int(input_size)
        if n_mels < 7 or n_mels % 8 != 0:
            raise ValueError(f"Conformer takes n_mels >= 7, a multiple of 8 (got {n_mels})")
        self.n_mels = n_mels
        compute = compute or kwargs.get("hip_compute", "f32")
        compute = {"half": "bf16", "fp32": "f32"}.get(compute, compute)
        if compute not in ("f32", "bf16"):
            raise NotImplementedError(f"Conformer runs in 'f32' or 'bf16' (got {compute!r})")
        self.features = str(kwargs.get("features", "melspectrogram")).lower()
        hop = kwargs.get("hop_length", 80)
        self._hop = hop
        fe = {k: kwargs[k] for k in ("sr", "n_fft", "win_length", "fmin", "fmax", "pre_emphasis") if k in kwargs}
        if kwargs.get("window", "hamming") != "hamming":
            raise NotImplementedError("only the hamming window of feature.py:68 is built")
        self._min_samples = int(fe.get("n_fft", MIN_SAMPLES))
        max_batch = int(max_batch or kwargs.get("embed_batch", 256))
        super().__init__(synth.conformer_param_spec(nOut, n_mels),
                         dict(channels=synth.CONFORMER_D, n_mels=n_mels, embed_dim=nOut, log_input=self.features == "melspectrogram",
                              input_norm=True, hop_length=hop, **fe),
                         device=device if device is not None else kwargs.get("device"), compute=compute,
                         max_batch=max_batch, primary_samples=_crop_samples(kwargs.get("audio_spec")))

    def _frames_ok(self, T):
        return 1 <= synth.conformer_frames(T) <= synth.CONFORMER_MAX_T

    def accepts_length(self, L):
        return L >= self._min_samples and self._frames_ok(L // self._hop + 1)

    def _engine_for(self, x):
        """the handle for a (B, L) waveform batch"""
        if x.ndim != 2 or not self.accepts_length(x.shape[1]):
            raise ValueError(f"Conformer takes (batch, L) waveforms with L >= {self._min_samples} and at most 10000 subsampled frames, "
                             f"got {tuple(x.shape)}")
        return self._get_engine(int(x.shape[1]), batch=x.shape[0])

    def forward(self, x, lengths=None):
        """x: (B, n_mels, T) mel power, torch tensor (CPU / CUDA) or numpy (Conformer_.forward, Conformer.py:100-154)"""
        if x.ndim != 3:
            raise ValueError(f"expected (batch, n_mels, frames), got {tuple(x.shape)}")
        if not self._frames_ok(x.shape[2]):
            raise ValueError(f"Conformer takes 7 <= T frames with at most 10000 subsampled frames, got T = {x.shape[2]}")
        T = int(x.shape[2])
        samples = (T - 1) * self._hop if (T - 1) * self._hop >= self._min_samples else T * self._hop - 1      # (any L with T frames)
        eng = self._get_engine(samples, batch=x.shape[0])
        return self._squeeze(self._batched(eng.embed_features, x, eng.max_batch))

    def embed_wave(self, wav):
        """fused waveform -> embedding (mel front-end + forward in one library call)"""
        eng = self._engine_for(wav)
        return self._squeeze(self._batched(eng.embed_wave, wav, eng.max_batch))

    # ---- ragged batches (RaggedMixin): the rows are mel frames ----------------------------------------------------------------
    MIN_FRAMES = 7                  # T' = (T - 3) // 4 >= 1

    def _ragged_geometry(self):
        """(max_batch, row capacity, slice limit) of the primary handle, from the module's own settings (no handle is built)"""
        frames = (self._primary or self.DEFAULT_PRIMARY) // self._hop + 1
        return self._max_batch, self._max_batch * frames, slice_frames(self._max_batch, frames, self.n_mels, self._compute)

    def ragged_frames(self, n_samples):
        """mel frames of an utterance of n_samples; 0 for one that fits no ragged call (ragged_frames_of)"""
        return ragged_frames_of(n_samples, self._hop, self._min_samples, self._ragged_geometry()[2])

    def _ragged_limits(self):
        return f"; at least {self._min_samples} samples and 7 frames each, at most {self._ragged_geometry()[2]} subsampled frames"


def MainModel(nOut=512, **kwargs):
    kwargs.setdefault("input_size", kwargs.get("n_mels", 80))
    return Conformer(nOut=nOut, **kwargs)
