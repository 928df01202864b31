"""Drop-in for the reference plug-in ``models/TitaNet.py`` (MainModel :434-443, TitaNet :10-181), the spectral branch of
``Tita_ECAPA`` and ``Raw_tita``:

    model = MainModel(nOut=512, model_size='l', n_mels=80, device='cuda')
    emb = model(mel)            # (B, n_mels, T) mel POWER -> (B, nOut); (nOut,) for B == 1
    emb = model.embed_wave(wav) # (B, L) waveform -> mel front-end + the net in one library call

TitaNet reads its input as it is (no log, no normalisation).  Sizes s / m / l are H = 256 / 512 / 1024 with depthwise kernels 3 / 7 /
11; ``n_mega_blocks=None`` takes ``find_n_mega_blocks``' choice, restated in closed form (synth.titanet_n_mega_blocks).  State-dict keys
are the reference's.  Computes: "f32" and "bf16" ("half" means bf16 here).  ``device`` is accepted as the reference requires it.
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


class TitaNet(RaggedMixin, HipModule):
    model_kind = "titanet"

    def __init__(self, nOut=512, model_size="l", n_mega_blocks=None, device=None, compute=None, max_batch=None, **kwargs):
        size = str(model_size).lower()
        if size not in synth.TITANET_SIZES:
            raise AssertionError("Unsupported model size")                    # TitaNet.py:134-138
        n_mels = int(kwargs.get("n_mels", 80))
        if n_mega_blocks is None:
            n_mega_blocks = synth.titanet_n_mega_blocks(size, nOut, n_mels)
        self.model_size, self.n_mega_blocks, self.n_mels = size, int(n_mega_blocks), n_mels
        compute = compute or kwargs.get("hip_compute", "f32")
        compute = {"half": "bf16", "fp32": "f32"}.get(compute, compute)
        if compute not in ("f32", "bf16"):
            raise NotImplementedError(f"TitaNet runs in 'f32' or 'bf16' (got {compute!r})")
        H, _ = synth.TITANET_SIZES[size]
        hop = kwargs.get("hop_length", 80)
        self._hop = hop
        fe = {k: kwargs[k] for k in ("sr", "n_fft", "win_length", "fmin", "fmax", "pre_emphasis") if k in kwargs}
        if kwargs.get("window", "hamming") != "hamming":
            raise NotImplementedError("only the hamming window of feature.py:68 is built")
        self._min_samples = int(fe.get("n_fft", MIN_SAMPLES))
        max_batch = int(max_batch or kwargs.get("embed_batch", 256))
        super().__init__(synth.titanet_param_spec(size, nOut, self.n_mega_blocks, n_mels),
                         dict(channels=H, n_mels=n_mels, embed_dim=nOut, log_input=False, input_norm=False, hop_length=hop, **fe),
                         device=device if device is not None else kwargs.get("device"), compute=compute,
                         max_batch=max_batch, primary_samples=_crop_samples(kwargs.get("audio_spec")))

    def accepts_length(self, L):
        return L >= self._min_samples

    def _engine_for(self, x):
        """the handle for a (B, L) waveform batch"""
        if x.ndim != 2 or not self.accepts_length(x.shape[1]):
            raise ValueError(f"TitaNet takes (batch, L >= {self._min_samples}) waveforms, got {tuple(x.shape)}")
        return self._get_engine(int(x.shape[1]), batch=x.shape[0])

    def forward(self, x, speakers=None):
        """x: (B, n_mels, T) mel power, torch tensor (CPU / CUDA) or numpy (TitaNet.forward, TitaNet.py:159-173)"""
        if x.ndim != 3:
            raise ValueError(f"expected (batch, n_mels, frames), got {tuple(x.shape)}")
        eng = self._get_engine((x.shape[2] - 1) * self._hop, batch=x.shape[0])
        return self._squeeze(self._batched(eng.embed_features, x, eng.max_batch))

    def embed_wave(self, wav):
        """fused waveform -> embedding (mel front-end + forward in one library call)"""
        eng = self._engine_for(wav)
        return self._squeeze(self._batched(eng.embed_wave, wav, eng.max_batch))

    # ---- ragged batches (RaggedMixin): the rows are mel frames ----------------------------------------------------------------
    MIN_FRAMES = 1                  # no subsampling and zero padding: one frame is an utterance

    def _ragged_geometry(self):
        """(max_batch, row capacity) of the primary handle, from the module's own settings (no handle is built)"""
        frames = (self._primary or self.DEFAULT_PRIMARY) // self._hop + 1
        return self._max_batch, self._max_batch * frames

    def ragged_frames(self, n_samples):
        """mel frames of an utterance of n_samples; 0 for one shorter than the front-end's FFT window, which fits no ragged call"""
        return 0 if n_samples < self._min_samples else int(n_samples) // int(self._hop) + 1

    def _ragged_limits(self):
        return f"; at least {self._min_samples} samples each"


def MainModel(nOut=512, model_size="l", n_mega_blocks=None, **kwargs):
    return TitaNet(nOut=nOut, model_size=model_size, n_mega_blocks=n_mega_blocks, **kwargs)
