"""Drop-in for the reference plug-in ``models/ResNetSE34V2.py`` (MainModel :5-9 -> ``ResNetSE`` of ResNetBaseline.py:141-301 with
``SEBasicBlockV2`` of ResNetBlocks.py:211-246), the 2-D "Fast ResNet" baseline:

    model = MainModel(nOut=256, n_mels=80, features='melspectrogram', augment=False, augment_options={...}, device='cuda')
    emb = model(mel)            # (B, n_mels, T) mel POWER -> (B, nOut); B == 1 returns (1, nOut): the reference has no squeeze
    emb = model.embed_wave(wav) # (B, L) waveform -> mel front-end + the net in one library call

The front-end takes log(x + 1e-6) and the time mean off only for ``features='melspectrogram'``, then InstanceNorm1d(n_mels) without
affine, as the reference.  ``encoder_type`` 'ASP' (weighted mean | std) or 'SAP' (weighted mean); ``att_dim`` 128 only.  State-dict keys
are the reference's (292 at nOut = 256; ``num_batches_tracked`` is kept and ignored).  Computes: "f32" and "bf16" ("half" means bf16
here).  Lengths: T = 1 is a ``ValueError`` as in the reference (InstanceNorm1d over one frame); a handle is made for L >= 512 samples, one
frame of the library's front-end, so ``forward`` takes T >= 7 frames and ``embed_wave`` L >= 512 (T = 2 .. 6 raise ``ValueError`` here).  ``n_mels`` must be a multiple of 8: the reference's ``outmap_size = int(n_mels / 8)``
agrees with its own convolution arithmetic only then.  SpecAugment (``augment=True`` with 'spec_domain') is training only and not built.
``embed_ragged`` embeds utterances of different lengths in shared calls of the primary handle (whole-file evaluation).
"""
from __future__ import annotations

from .. import synth
from ._base import HipModule, RaggedMixin

MIN_SAMPLES = 512           # the mel front-end's n_fft (one frame of the library's front-end)


def _crop_samples(audio_spec):
    try:
        return int(audio_spec["sentence_len"] * audio_spec["sample_rate"])
    except Exception:
        return None


class ResNetSE(RaggedMixin, HipModule):
    model_kind = "resnetse"

    def __init__(self, nOut=256, encoder_type="ASP", att_dim=128, device=None, compute=None, max_batch=None, **kwargs):
        if encoder_type not in ("ASP", "SAP"):
            raise ValueError("Undefined encoder")                              # ResNetBaseline.py:200-201
        if int(att_dim) != 128:
            raise NotImplementedError(f"ResNetSE34V2 is built for att_dim = 128 (got {att_dim})")
        n_mels = int(kwargs.get("n_mels", 80))
        if n_mels <= 0 or n_mels % 8 != 0:
            raise NotImplementedError(f"ResNetSE34V2 takes n_mels that are a multiple of 8 (got {n_mels}): the reference's outmap_size = "
                                      "int(n_mels / 8) disagrees with its convolutions otherwise")
        self.n_mels, self.encoder_type = n_mels, encoder_type
        compute = compute or kwargs.get("hip_compute", "f32")
        compute = {"half": "bf16", "fp32": "f32"}.get(compute, compute)
        if compute not in ("f32", "bf16"):
            raise NotImplementedError(f"ResNetSE34V2 runs in 'f32' or 'bf16' (got {compute!r})")
        self.features = str(kwargs.get("features", "melspectrogram")).lower()
        hop = kwargs.get("hop_length", 80)
        self._hop = hop
        fe = {k: kwargs[k] for k in ("sr", "n_fft", "win_length", "fmin", "fmax", "pre_emphasis") if k in kwargs}
        if kwargs.get("window", "hamming") != "hamming":
            raise NotImplementedError("only the hamming window of feature.py:68 is built")
        self._min_samples = int(fe.get("n_fft", MIN_SAMPLES))
        max_batch = int(max_batch or kwargs.get("embed_batch", 256))
        super().__init__(synth.resnetse_param_spec(nOut, n_mels, encoder_type),
                         dict(channels=1 if encoder_type == "SAP" else 2, n_mels=n_mels, embed_dim=nOut,
                              log_input=self.features == "melspectrogram", input_norm=True, hop_length=hop, **fe),
                         device=device if device is not None else kwargs.get("device"), compute=compute,
                         max_batch=max_batch, primary_samples=_crop_samples(kwargs.get("audio_spec")))

    def accepts_length(self, L):
        return L >= self._min_samples

    def _engine_for(self, x):
        """the handle for a (B, L) waveform batch"""
        if x.ndim != 2 or not self.accepts_length(x.shape[1]):
            raise ValueError(f"ResNetSE34V2 takes (batch, L >= {self._min_samples}) waveforms, got {tuple(x.shape)}")
        return self._get_engine(int(x.shape[1]), batch=x.shape[0])

    def forward(self, x):
        """x: (B, n_mels, T) mel power, torch tensor (CPU / CUDA) or numpy (ResNetSE.forward, ResNetBaseline.py:250-301)"""
        if x.ndim != 3:
            raise ValueError(f"expected (batch, n_mels, frames), got {tuple(x.shape)}")
        T = int(x.shape[2])
        if T < 2:
            raise ValueError(f"Expected more than 1 spatial element when training, got input size {tuple(x.shape)}")     # InstanceNorm1d's own message
        samples = (T - 1) * self._hop if (T - 1) * self._hop >= self._min_samples else max(T * self._hop - 1, self._min_samples)
        if samples // self._hop + 1 != T:
            raise ValueError(f"ResNetSE34V2: T = {T} frames is below one frame of the library's front-end geometry (n_fft {self._min_samples}, "
                             f"hop {self._hop}: T >= {self._min_samples // self._hop + 1})")
        eng = self._get_engine(samples, batch=x.shape[0])
        return self._batched(eng.embed_features, x, eng.max_batch)              # (no squeeze: B = 1 stays (1, nOut))

    def embed_wave(self, wav):
        """fused waveform -> embedding (mel front-end + forward in one library call)"""
        eng = self._engine_for(wav)
        return self._batched(eng.embed_wave, wav, eng.max_batch)

    # ---- ragged batches (RaggedMixin): the rows are mel frames, an utterance counted in whole groups of 8 ---------------------------
    MIN_FRAMES = 2                  # InstanceNorm1d over one frame is the reference's own ValueError

    def _ragged_geometry(self):
        """(max_batch, row capacity) of the primary handle, from the module's own settings (no handle is built)"""
        frames = (self._primary or self.DEFAULT_PRIMARY) // self._hop + 1
        return self._max_batch, self._max_batch * frames

    def ragged_frames(self, n_samples):
        """rows an utterance of n_samples takes in a ragged call: its T mel frames rounded up to a multiple of 8 (the network halves the
        frame axis three times, rounding up, so the library counts an utterance this way to keep every level within the handle's rows);
        0 for one shorter than the front-end's FFT window, which fits no ragged call"""
        if n_samples < self._min_samples:
            return 0
        return 8 * -(-(int(n_samples) // int(self._hop) + 1) // 8)

    def _ragged_limits(self):
        return f", an utterance counted as its frames rounded up to a multiple of 8; at least {self._min_samples} samples each"


def MainModel(nOut=256, **kwargs):
    return ResNetSE(nOut=nOut, **kwargs)
