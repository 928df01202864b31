"""Counterparts of the reference's ``src/model.py`` for the inference hot path.

Same class / method names, arguments and return shapes as the reference so that
``inference.py``-style drivers keep working:

    net = WrappedModel(SpeakerEncoder(**vars(args)))
    speaker_model = ModelHandling(net, **vars(args))
    speaker_model.loadParameters(path)
    scores, labels, trials = speaker_model.evaluateFromList(listfilename=..., distributed=False,
                                                           dataloader_options=..., cohorts_path=...,
                                                           num_eval=10, scoring_mode='cosine')

What changed underneath: crops of MANY files are batched into one device call
(reference: batch = one file), embeddings stay in one dense matrix, and the whole trial list is
scored by one kernel launch per mode (reference: three host<->device crossings per trial).
Training (``fit``), ONNX export and report writing are out of scope and raise NotImplementedError.
"""
from __future__ import annotations

import csv
import importlib
import itertools
import os
import warnings
from pathlib import Path

import numpy as np

from . import _lib
from . import distributed as sv_dist
from . import scoring
from .audio import loadWAV, read_pcm16
from .engine import _is_torch, to_device, to_host

try:
    import torch
    import torch.nn.functional as F
except Exception:  # pragma: no cover
    torch = None

# losses whose test_normalize is False in the reference (src/losses/Prototypical.py:21); every other
# loss sets it True (src/losses/*.py), which is what reaches the hot path (src/model.py:90-94,421-423)
_NO_TEST_NORMALIZE = {"Prototypical"}


def _host(x):
    return x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x)


class WrappedModel:
    """src/model.py:24-33 — the DataParallel-compatibility wrapper: forward delegates to .module"""

    def __init__(self, model):
        self.module = model

    def forward(self, x, label=None):
        return self.module(x, label)

    __call__ = forward

    def eval(self):
        self.module.eval()
        return self

    def train(self, mode=True):
        self.module.train(mode)
        return self

    def state_dict(self):
        return self.module.state_dict()

    def parameters(self):
        return self.module.parameters()


class SpeakerEncoder:
    """src/model.py:36-135: feature extractor + __S__ (+ the loss's test_normalize flag)."""

    def __init__(self, model, criterion=None, classifier=None, optimizer=None, features="melspectrogram",
                 device="cuda", gpu=0, include_top=False, **kwargs):
        self.model = model
        self.criterion = criterion or {"name": "AAmSoftmaxAP"}
        self.classifier = classifier
        self.optimizer = optimizer
        self.gpu = gpu
        self.device = f"{device}:{gpu}"
        self.n_mels = kwargs.get("n_mels", 80)
        self.features = features.lower()
        if include_top:
            raise NotImplementedError("include_top (classification head) is outside the inference hot path")
        kw = dict(kwargs)
        kw.setdefault("n_mels", self.n_mels)
        kw.setdefault("augment", False)
        kw.setdefault("augment_options", {"augment_chain": []})
        if self.features in ("mfcc", "melspectrogram"):
            fx = importlib.import_module("speakerverification_amd.models.FeatureExtraction.feature")
            self.compute_features = getattr(fx, self.features)(**kw).to(self.device)
        else:
            self.compute_features = None
        if not isinstance(self.model["name"], str):
            raise NotImplementedError("Mixed_model lists are outside the hot path")
        mod = importlib.import_module("speakerverification_amd.models." + self.model["name"])
        self.__S__ = mod.MainModel(nOut=self.model["nOut"], features=self.features, device=self.device, **kw).to(self.device)
        self.test_normalize = self.criterion.get("name") not in _NO_TEST_NORMALIZE
        self.training = False

    # nn.Module look-alikes ------------------------------------------------------------------------------
    def eval(self):
        self.__S__.eval()
        return self

    def train(self, mode=True):
        self.__S__.train(mode)
        return self

    def parameters(self):
        return self.__S__.parameters()

    def state_dict(self):
        """reference checkpoint layout: keys prefixed with __S__. (src/model.py:710-716)"""
        return {"__S__." + k: v for k, v in self.__S__.state_dict().items()}

    def load_state_dict(self, sd, strict=True):
        sub = {k[len("__S__."):]: v for k, v in sd.items() if k.startswith("__S__.")}
        return self.__S__.load_state_dict(sub, strict=strict)

    def forward(self, data, label=None):
        """src/model.py:104-125 with label=None: (..., L) waveforms -> (N, nOut) embeddings
        ((nOut,) for a single row, as the reference's stack(dim=1).squeeze())."""
        if label is not None:
            raise NotImplementedError("loss evaluation (training) is outside the inference hot path")
        L = data.shape[-1]
        data = data.reshape(-1, L)
        if self.features != "raw" and hasattr(self.__S__, "embed_wave") and self._fusable():
            out = self.__S__.embed_wave(data)                   # fbank + forward in one library call
        else:
            inp = self.compute_features(data) if self.features != "raw" else data
            out = self.__S__.forward(inp)
        return out

    __call__ = forward

    def _fusable(self):
        """the fused path bakes the front-end defaults into the model handle; only use it when the
        feature extractor has exactly those defaults"""
        p = getattr(self.compute_features, "p", None)
        return p == dict(sr=8000, n_fft=512, win_length=200, n_mels=self.n_mels, hop_length=80,
                         fmin=0.0, fmax=None, pre_emphasis=True)


class ModelHandling:
    """src/model.py:138-792, inference methods only."""

    def __init__(self, encoder_model, optimizer=None, callbacks=None, device="cuda", gpu=0, mixedprec=False, **kwargs):
        self.kwargs = kwargs
        self.save_path = kwargs.get("save_folder", ".")
        self.audio_spec = kwargs["audio_spec"]
        self.__model__ = encoder_model
        self.model_name = self.__model__.module.model["name"]
        self.criterion = self.__model__.module.criterion["name"]
        self.gpu = gpu
        self.device = f"{device}:{gpu}"
        self.embed_batch = int(kwargs.get("embed_batch", 256))     # crops per device call (cross-file batching)
        self.device_crop = bool(kwargs.get("device_crop", True))   # 16-bit PCM files: crop on the device (svhip_crop_pcm16)
        self.device_feats = bool(kwargs.get("device_feats", True)) # keep enrol -> score on the device when a GPU is there
        self.ragged_eval = bool(kwargs.get("ragged_eval", True))   # num_eval == 0: whole files of different lengths share library calls

    # ---- training-only surface ---------------------------------------------------------------------------
    def fit(self, *a, **k):
        raise NotImplementedError("training is outside the scope of the MI355X inference path")

    def export_onnx(self, *a, **k):
        raise NotImplementedError("ONNX export is outside the scope of the MI355X inference path")

    # ---- embedding -------------------------------------------------------------------------------------------
    def _embed_crops(self, crops: np.ndarray) -> np.ndarray:
        """(n, L) float32 crops -> (n, nOut) float32, in device batches of embed_batch rows."""
        outs = []
        for i in range(0, crops.shape[0], self.embed_batch):
            o = self.__model__.forward(np.ascontiguousarray(crops[i:i + self.embed_batch], dtype=np.float32))
            o = o.detach().cpu().numpy() if _is_torch(o) else np.asarray(o)
            outs.append(o.reshape(-1, o.shape[-1]))
        return np.concatenate(outs, 0)

    def _device_path_ok(self, num_eval):
        """the device crop -> embed path needs fixed-length crops, a GPU, and a model that takes raw waveforms on the device"""
        if not self.device_crop or num_eval <= 0 or torch is None or not torch.cuda.is_available():
            return False
        enc = self.__model__.module
        S = getattr(enc, "__S__", None)
        if S is None:
            return False
        if enc.features == "raw":
            return callable(getattr(S, "forward", None)) and getattr(S, "accepts_device_wave", False)
        return hasattr(S, "embed_wave") and enc._fusable()

    def _ragged_ok(self, num_eval):
        """whole-file evaluation as ragged batches: the model offers embed_ragged and the front-end is the one its handle bakes in
        (a ``features: raw`` model reads the waveform and bakes its own front-end: the mel extractor's settings do not apply)"""
        if num_eval != 0 or not self.ragged_eval:
            return False
        enc = self.__model__.module
        S = getattr(enc, "__S__", None)
        if S is None or not hasattr(S, "embed_ragged"):
            return False
        return enc.features == "raw" or enc._fusable()

    def _feats_on_device(self):
        """evaluateFromList / testFromList keep the (n_files, num_eval, nOut) block in HBM from the embed calls to the scoring
        kernels when there is a GPU to hold it (only the P scores come back); CPU test doubles keep numpy."""
        return self.device_feats and torch is not None and torch.cuda.is_available()

    def _embed_files(self, files, num_eval, on_device=False):
        """crops of several files travel in one batch (the reference runs one file per forward,
        src/model.py:386-394).  Returns a dense (n_files, num_eval, nOut) float32 block: a numpy array, or with
        on_device=True a CUDA tensor that never visits the host.

        16-bit PCM files take the device path: the int16 samples are uploaded once, `svhip_crop_pcm16` cuts the eval-mode
        crops (audio_loader.py:110-150) straight into an HBM buffer, and the embed call consumes that buffer as a device
        pointer in batches of `embed_batch` crops across files — no fp32 crop crosses PCIe.
        Other sources (float / 24-bit files, ndarrays, num_eval == 0) keep the host path (loadWAV)."""
        feats = None
        max_audio = int(self.audio_spec["sentence_len"] * self.audio_spec["sample_rate"])
        use_dev = self._device_path_ok(num_eval)
        pending, owners = [], []            # host path: fp32 crops
        pcm_pending, pcm_owners = [], []    # device path: int16 files
        ncrop = max(1, num_eval)

        def store(idx_n, emb):
            nonlocal feats
            D = emb.shape[-1]
            if feats is None:
                feats = (torch.zeros((len(files), ncrop, D), dtype=torch.float32, device=f"cuda:{self.gpu}") if on_device
                         else np.zeros((len(files), ncrop, D), np.float32))
            if on_device and not (_is_torch(emb) and emb.is_cuda):
                emb = to_device(np.ascontiguousarray(_host(emb), np.float32), self.gpu)      # host-path files: only their embeddings go up
            elif not on_device:
                emb = to_host(emb) if _is_torch(emb) else np.asarray(emb)
            # files of one flush are consecutive and (almost always) full: one block copy; otherwise file by file
            idx0 = idx_n[0][0]
            if all(n == ncrop for _, n in idx_n) and [i for i, _ in idx_n] == list(range(idx0, idx0 + len(idx_n))):
                feats[idx0:idx0 + len(idx_n)] = emb.reshape(len(idx_n), ncrop, D)
                return
            pos = 0
            for idx, n in idx_n:
                feats[idx, :n] = emb[pos:pos + n]
                pos += n

        def flush():
            if pending:
                store(owners, self._embed_crops(np.concatenate(pending, 0)))
                pending.clear()
                owners.clear()

        def flush_pcm():
            if not pcm_pending:
                return
            eng = scoring.scoring_engine(self.gpu)
            n = len(pcm_pending) * num_eval
            crops = torch.empty((n, max_audio), dtype=torch.float32, device=f"cuda:{self.gpu}")
            eng.crop_pcm16(pcm_pending, num_eval, max_audio, out=crops)
            outs = []
            for i in range(0, n, self.embed_batch):
                o = self.__model__.forward(crops[i:i + self.embed_batch])
                outs.append(o.reshape(-1, o.shape[-1]))
            store(pcm_owners, torch.cat(outs, 0) if len(outs) > 1 else outs[0])
            pcm_pending.clear()
            pcm_owners.clear()

        # num_eval == 0 on a model with embed_ragged: whole files of different lengths are collected up to the capacity of the model's
        # primary handle and embedded in ONE call per group; a file that fits no call keeps the per-file path below
        S = getattr(self.__model__.module, "__S__", None) if self._ragged_ok(num_eval) else None
        packer = S.ragged_packer() if S is not None else None
        rag_pending, rag_owners = [], []

        def flush_ragged():
            if rag_pending:
                store(list(rag_owners), S.embed_ragged(list(rag_pending)))
                rag_pending.clear()
                rag_owners.clear()
                packer.reset()

        for idx, f in enumerate(files):
            pcm = read_pcm16(f, self.audio_spec["sample_rate"]) if (use_dev and isinstance(f, (str, Path))) else None
            if pcm is not None:
                pcm_pending.append(pcm)
                pcm_owners.append((idx, num_eval))
                if len(pcm_pending) * num_eval >= self.embed_batch:
                    flush_pcm()
                continue
            audio = loadWAV(f, self.audio_spec, evalmode=True, augment=False, augment_options=[], num_eval=num_eval,
                            random_chunk=False)
            if packer is not None:
                wav = np.ascontiguousarray(np.asarray(audio, np.float32).reshape(-1))
                frames = S.ragged_frames(wav.shape[0])
                if packer.fits_alone(frames):
                    if not packer.add(frames):
                        flush_ragged()
                        packer.add(frames)
                    rag_pending.append(wav)
                    rag_owners.append((idx, 1))
                    continue
            if num_eval == 0:                       # whole file: variable length, one forward per file
                flush()
                store([(idx, 1)], self._embed_crops(audio))
                continue
            pending.append(audio)
            owners.append((idx, audio.shape[0]))
            if sum(n for _, n in owners) >= self.embed_batch:
                flush()
        flush()
        flush_pcm()
        flush_ragged()
        return feats

    def embed_utterance(self, source, num_eval=20, normalize=False):
        """src/model.py:675-704: path or ndarray -> (num_eval, nOut) CPU tensor (L2-normalised on request)."""
        audio = loadWAV(source, self.audio_spec, evalmode=True, augment=False, augment_options=[], num_eval=num_eval,
                        random_chunk=False)
        emb = self._embed_crops(audio)
        if normalize:
            eng = scoring.scoring_engine(self.gpu)
            emb = np.ascontiguousarray(emb)
            eng.l2norm_(emb)
        return torch.from_numpy(emb) if torch is not None else emb

    # ---- evaluation ----------------------------------------------------------------------------------------------
    def _l2norm_crops(self, feats):
        """L2-normalise every crop row of an (n_files, n_crops, D) block where it lives (F.normalize(p=2, dim=1), model.py:421-423;
        embed_utterance(normalize=True)): a CUDA tensor in place through a view, a host array in a contiguous float32 copy"""
        eng = scoring.scoring_engine(self.gpu)
        if _is_torch(feats) and feats.is_cuda:
            feats = feats.contiguous()
            eng.l2norm_(feats.view(-1, feats.shape[-1]))
            return feats
        flat = np.ascontiguousarray(np.asarray(_host(feats), np.float32).reshape(-1, feats.shape[-1]))
        eng.l2norm_(flat)
        return flat.reshape(feats.shape)

    def _crop_mean_rows(self, files, num_eval):
        """identify's preparation of its queries, up to the last step: the files' crop embeddings, L2-normalised when the loss sets
        ``test_normalize``, averaged -> (n_files, nOut) host rows (the caller normalises the means)"""
        feats = np.ascontiguousarray(_host(self._embed_files(files, num_eval)), dtype=np.float32)       # (n_files, n_crops, nOut)
        if self.__model__.module.test_normalize:
            feats = self._l2norm_crops(feats)
        return np.ascontiguousarray(feats.mean(axis=1))

    def _score(self, feats, ia, ib, scoring_mode, cohorts, cohorts_path):
        """(n_files, n_crops, D) embeddings (numpy, or a CUDA tensor that stays where it is) + trial indices -> P float32 scores
        on the host.  Normalisation and every scoring mode are library kernels; with device embeddings the PCIe traffic is the
        index lists up, the P scores down (and the cohort up, for 'norm')."""
        if self.__model__.module.test_normalize:
            feats = self._l2norm_crops(feats)
        if cohorts_path is None:
            # model.py:425-431: F.pairwise_distance(ref (n,D,1), com (1,D,n)) takes the 2-norm over the LAST axis of the
            # broadcast (n, D, n) difference, i.e. over the crops j of `com`; score = -mean.  One kernel over the trial list
            # (svhip_score_trials, SVHIP_TRIAL_PDIST): O(P n^2 D) work, no (P, n, D, n) temporary.
            mode = "pdist"
        elif scoring_mode in ("norm", "cosine", "pnorm"):
            mode = scoring_mode
        else:
            raise ValueError(f"unknown scoring_mode {scoring_mode}")
        s = scoring.score_trials(feats, ia, ib, mode, cohorts=cohorts, top=200, device=self.gpu)
        return np.asarray(to_host(s), np.float32)

    def evaluateFromList(self, listfilename, distributed=False, dataloader_options=None,
                         cohorts_path="checkpoint/dump_cohorts.npy", num_eval=10, scoring_mode="cosine", **kwargs):
        """src/model.py:306-450.  Trial lines ``label file1 file2`` (or CSV with a header line).
        Returns (all_scores, all_labels, all_trials); empty lists on ranks != 0 when distributed."""
        self.__model__.eval()
        cohorts = np.load(cohorts_path) if (cohorts_path is not None and scoring_mode == "norm") else None
        with open(listfilename) as fh:
            lines = fh.readlines()
        determinator = "," if len(lines[0].split(",")) > 1 else " "
        start_index = 1 if determinator == "," else 0
        files = list(itertools.chain(*[x.strip().split(determinator)[-2:] for x in lines[start_index:]]))
        setfiles = sorted(set(files))
        rank, world = sv_dist.rank_world() if distributed else (0, 1)
        lo, hi, _ = sv_dist.shard_bounds(len(setfiles), rank, world)
        on_dev = self._feats_on_device()
        local = self._embed_files(setfiles[lo:hi], num_eval, on_device=on_dev)
        if distributed and sv_dist.is_distributed():
            nOut = self.__model__.module.model["nOut"]
            if local is None:
                local = (torch.zeros((0, max(1, num_eval), nOut), dtype=torch.float32, device=f"cuda:{self.gpu}") if on_dev
                         else np.zeros((0, max(1, num_eval), nOut), np.float32))
            feats = self._gather_rows(local, len(setfiles))            # ONE collective (reference: all_gather_object)
        else:
            feats = local
        all_scores, all_labels, all_trials = [], [], []
        index = {str(Path(f)): i for i, f in enumerate(setfiles)}
        index.update({f: i for i, f in enumerate(setfiles)})
        ia, ib = [], []
        for line in lines[start_index:]:
            data = line.strip().split(determinator) if determinator == "," else line.split()
            if len(data) < 3:
                continue
            data = data[-3:]
            ia.append(index[data[1]])
            ib.append(index[data[2]])
            all_labels.append(int(data[0]))
            all_trials.append(data[1] + " " + data[2])
        ia, ib = np.asarray(ia, np.int32), np.asarray(ib, np.int32)
        if kwargs.get("shard_scoring") and world > 1:
            # row-sharded scoring: every rank scores the trials whose enrol file sits in its block; the
            # P floats are then assembled with a second, small all-gather
            mine = sv_dist.trial_rows_of_rank(ia, len(setfiles), rank, world)
            s_loc = self._score(feats, ia[mine], ib[mine], scoring_mode, cohorts, cohorts_path)
            counts = [len(sv_dist.trial_rows_of_rank(ia, len(setfiles), r, world)) for r in range(world)]
            per = max(1, max(counts))
            pad = np.zeros((per, 1), np.float32)
            pad[:len(s_loc), 0] = s_loc
            allp = np.asarray(to_host(self._gather_rows(pad, per * world, exact=True))).reshape(world, per)
            if rank == 0:
                s = np.empty(len(ia), np.float32)
                for r in range(world):
                    s[sv_dist.trial_rows_of_rank(ia, len(setfiles), r, world)] = allp[r, :counts[r]]
                all_scores = [float(v) for v in s]
        elif rank == 0:
            s = self._score(feats, ia, ib, scoring_mode, cohorts, cohorts_path)
            all_scores = [float(v) for v in s]
        if rank != 0:
            return [], [], []
        return all_scores, all_labels, all_trials

    def _gather_rows(self, local, n_total: int, exact=False):
        """the path's exchange step.  With an Engine that owns RCCL (a real one on a GPU): svhip_allgather_rows on the scoring
        engine's stream, host or device rows alike; torch.distributed only ships the RCCL id once, and the communicator is cached
        next to the engine (scoring.lib_comm), not per ModelHandling.  Otherwise (gloo CPU tests with a stand-in engine):
        torch.distributed all_gather_into_tensor.  exact=True: every rank passes exactly n_total / world rows."""
        rank, world = sv_dist.rank_world()
        eng = scoring.scoring_engine(self.gpu)
        # (an engine without comm_init is a CPU stand-in; more ranks than GPUs means ranks share a device, which RCCL refuses)
        if hasattr(eng, "comm_init") and torch is not None and torch.cuda.is_available() and world <= torch.cuda.device_count():
            comm = scoring.lib_comm(self.gpu, rank, world)
            if not _is_torch(local):
                local = np.ascontiguousarray(local, np.float32)
            return comm.all_gather_rows(local, n_total)
        return sv_dist.all_gather_rows(torch.from_numpy(np.ascontiguousarray(_host(local))), n_total).numpy()

    def testFromList(self, test_list="evaluation_test.txt", thresh_score=0.5, distributed=False, dataloader_options=None,
                     cohorts_path=None, num_eval=10, scoring_mode="norm", output_file=None):
        """src/model.py:455-554: CSV ``audio_1,audio_2`` -> writes audio_1,audio_2,pred_label,score."""
        self.__model__.eval()
        cohorts = np.load(cohorts_path) if (cohorts_path is not None and scoring_mode == "norm") else None
        save_root = os.path.join(self.save_path, f"{self.model_name}/{self.criterion}/result")
        if output_file is None:
            output_file = test_list.replace(".txt", "_result.txt")
        write_file = Path(save_root, output_file) if os.path.split(output_file)[0] == "" else output_file
        files, lines = [], []
        with open(Path(test_list), newline="") as rf:
            reader = csv.reader(rf, delimiter=",")
            next(reader, None)
            for row in reader:
                files += [row[0], row[1]]
                lines.append(row)
        setfiles = sorted(set(files))
        feats = self._embed_files(setfiles, num_eval, on_device=self._feats_on_device())
        index = {f: i for i, f in enumerate(setfiles)}
        ia = np.asarray([index[r[0]] for r in lines], np.int32)
        ib = np.asarray([index[r[1]] for r in lines], np.int32)
        # the reference routes every mode through similarity_measure here (cohorts_path may be None for cosine)
        s = self._score(feats, ia, ib, scoring_mode, cohorts, cohorts_path if scoring_mode == "norm" else "")
        results = []
        os.makedirs(os.path.dirname(str(write_file)) or ".", exist_ok=True)
        with open(write_file, "w", newline="") as wf:
            w = csv.writer(wf, delimiter=",")
            w.writerow(["audio_1", "audio_2", "pred_label", "score"])
            for row, score in zip(lines, s):
                score = float(score)
                w.writerow([row[0], row[1], "1" if score >= thresh_score else "0", score])
                results.append(f"{Path(row[0]).name},{Path(row[1]).name},{score}")
        return results

    # ---- cohort / enrolment preparation ------------------------------------------------------------------------------
    def prepare(self, save_path=None, prepare_type="cohorts", num_eval=10, source=None, **kwargs):
        """src/model.py:559-670."""
        self.__model__.eval()
        if not source:
            raise ValueError("Please provide appropriate source!")
        if prepare_type == "cohorts":
            n_emb_per_spk = 3
            assert isinstance(source, str), "Please provide path to train metadata files"
            spk_files = {}
            with open(Path(source)) as fh:
                for line in fh.read().splitlines():
                    data = line.split()
                    if len(data) >= 2:
                        spk_files.setdefault(data[0], []).append(data[1])
            files, owner = [], []
            for si, (spk, paths) in enumerate(spk_files.items()):
                for pth in paths[:n_emb_per_spk]:
                    files.append(pth)
                    owner.append(si)
            feats = self._l2norm_crops(self._embed_files(files, num_eval))          # (n_files, n_crops, D), as embed_utterance(normalize=True)
            owner = np.asarray(owner)
            cohort = np.vstack([feats[owner == si].reshape(-1, feats.shape[-1]).mean(axis=0, keepdims=True)
                                for si in range(len(spk_files))])
            if save_path:
                np.save(save_path, np.array(cohort))
            return True
        if prepare_type == "embed":
            norm = self.__model__.module.test_normalize
            if isinstance(source, str):
                speaker_dirs = [x for x in Path(source).iterdir() if x.is_dir()]
                embeds, classes = [], {}
                for idx, d in enumerate(speaker_dirs):
                    classes[idx] = d.stem
                    fl = [str(f) for f in d.glob("*.wav")]
                    e = np.stack([self.embed_utterance(f, num_eval=num_eval, normalize=norm).numpy() for f in fl], 0)
                    embeds.append(e.mean(axis=0))
                embeds = torch.from_numpy(np.stack(embeds, -1))                     # (num_eval, nOut, n_class)
                if save_path:
                    torch.save(embeds, Path(save_path, "embeds.pt"))
                    np.save(str(Path(save_path, "classes.npy")), classes)
                return True
            if isinstance(source, list):
                e = np.stack([self.embed_utterance(a, num_eval=num_eval, normalize=norm).numpy() for a in source], 0)
                mean_embed = torch.from_numpy(e.mean(axis=0))
                if save_path:
                    torch.save(mean_embed, Path(save_path, "embeds.pt"))
                return mean_embed
        raise NotImplementedError

    # ---- 1:N identification -------------------------------------------------------------------------------------------------
    @staticmethod
    def _gallery(embeds, classes):
        """the three forms of an enrolled gallery -> ((n_class, nOut) float32 crop-mean rows, {index: name} or None)"""
        if isinstance(embeds, (str, Path)):
            d = Path(embeds)
            if classes is None and (d / "classes.npy").exists():
                classes = np.load(str(d / "classes.npy"), allow_pickle=True).item()
            embeds = torch.load(d / "embeds.pt")
        g = np.array(_host(embeds), dtype=np.float32)      # (a copy: the rows are normalised in place later)
        if g.ndim == 3:                                  # prepare('embed'): (num_eval, nOut, n_class)
            g = g.mean(axis=0).T
        elif g.ndim != 2:
            raise ValueError(f"embeds must be (num_eval, nOut, n_class) or (n_class, nOut), not {g.shape}")
        if classes is not None and not isinstance(classes, dict):
            classes = dict(enumerate(np.asarray(classes).tolist()))
        if classes is not None and len(classes) != g.shape[0]:
            raise ValueError(f"{len(classes)} class names for {g.shape[0]} enrolled classes")
        return np.ascontiguousarray(g), classes

    def _cohort(self, scoring_mode, cohorts, cohorts_path, width):
        """the cohort of ``scoring_mode="norm"`` as a (K, nOut) float32 array (None for "cosine"); a missing or mis-shaped one is refused"""
        if scoring_mode not in ("cosine", "norm"):
            raise ValueError(f"unknown scoring_mode {scoring_mode}")
        if scoring_mode != "norm":
            return None
        if cohorts is None and cohorts_path is not None:
            cohorts = np.load(str(cohorts_path))
        if cohorts is None:
            raise ValueError("scoring_mode 'norm' needs a cohort: cohorts (an array) or cohorts_path (an .npy file)")
        cohorts = np.ascontiguousarray(_host(cohorts), dtype=np.float32)
        if cohorts.ndim != 2 or cohorts.shape[1] != width:
            raise ValueError(f"the cohort must be (K, {width}), not {cohorts.shape}")
        return cohorts

    def _search_operands(self, source, embeds, classes, num_eval, scoring_mode, cohorts, cohorts_path, check_gallery=None):
        """What ``identify`` and ``matches`` search with, by ``identify``'s rule: the files' crop-mean embeddings and the gallery's class
        rows, both L2-normalised -> ``(q (n_files, nOut), gal (n_class, nOut), classes or None, cohort or None)``.
        ``check_gallery(gal)`` runs before any file is embedded."""
        self.__model__.eval()
        files = list(source) if isinstance(source, (list, tuple)) else [source]
        if not files:
            raise ValueError("Please provide appropriate source!")
        gal, classes = self._gallery(embeds, classes)
        if check_gallery is not None:
            check_gallery(gal)
        cohorts = self._cohort(scoring_mode, cohorts, cohorts_path, gal.shape[1])
        eng = scoring.scoring_engine(self.gpu)
        q = self._crop_mean_rows(files, num_eval)
        if q.shape[1] != gal.shape[1]:
            raise ValueError(f"the model embeds to {q.shape[1]} values, the gallery holds {gal.shape[1]}")
        eng.l2norm_(q)
        eng.l2norm_(gal)
        return q, gal, classes, cohorts

    def identify(self, source, embeds, classes=None, top=1, num_eval=10, scoring_mode="cosine", cohorts=None, cohorts_path=None,
                 cohort_top=200, thresh_score=None):
        """Whose voice is this?  The ``top`` best enrolled classes of every file of ``source`` (what ``_embed_files`` takes: a list of
        paths / arrays, or one of them) against a gallery: the directory ``prepare('embed')`` wrote (``embeds.pt``, ``classes.npy``),
        a ``(num_eval, nOut, n_class)`` tensor in that layout, or an ``(n_class, nOut)`` array.

        Rule: each crop embedding is L2-normalised when the loss sets ``test_normalize``; the crops are averaged; the mean is
        L2-normalised.  The gallery is treated the same way (mean over its crop axis, then L2-normalised), and the score is the cosine
        of the two.  (The reference's ``predict`` loop, src/inference.py:254-327, averages per-crop L2 distances d and reports
        1 - d^2 / 2: the same cosine for one crop of unit vectors; for several crops this project averages embeddings, as its AS-norm
        path does.)  Files are embedded in batches (whole files through the ragged path with ``num_eval=0``) and searched in ONE
        ``score_topk`` call.

        ``scoring_mode="norm"`` (open-set identification): queries and gallery are prepared as above, the adaptive-S-norm statistics of
        both are taken against a cohort — ``cohorts``, a ``(K, nOut)`` array, or ``cohorts_path``, the ``.npy`` file
        ``prepare('cohorts')`` wrote, as ``evaluateFromList`` takes it — over each row's ``cohort_top`` largest cohort scores, and the
        score of a file against a class is ``0.5 * ((s - mu_q) / sd_q + (s - mu_g) / sd_g)`` with s their cosine.  The ``top`` classes
        are the best by THAT score (every class has its own statistics: the order differs from the cosine order), found in one
        ``score_topk_norm`` call.  A missing cohort is refused.

        ``thresh_score`` (either mode): an entry whose score is below it is not an identification — its index becomes -1 and its name
        ``None``; the scores are returned as computed, and the entries stay in place (best first).  What the reference's ``predict``
        does with ``args.test_threshold``; a threshold on ``"norm"`` scores carries across speakers and channels, one on cosines does not.

        Returns ``(scores (n_files, top) float32, index (n_files, top) int32)``, best first, and as a third item the class names
        (a list of ``top`` names per file) when ``classes`` is given ({index: name} or a sequence) or the directory holds ``classes.npy``."""
        top = int(top)

        def check_top(gal):
            if top < 1 or top > gal.shape[0]:
                raise ValueError(f"top = {top} must lie in [1, n_class = {gal.shape[0]}]")

        q, gal, classes, cohorts = self._search_operands(source, embeds, classes, num_eval, scoring_mode, cohorts, cohorts_path, check_top)
        if scoring_mode == "norm":
            scores, index, _ = scoring.score_topk_norm(q, gal, top, cohorts, top=int(cohort_top), device=self.gpu)
        else:
            scores, index = scoring.score_topk(q, gal, top, device=self.gpu)
        if thresh_score is not None:
            index = np.where(np.asarray(_host(scores)) < thresh_score, np.int32(-1), np.asarray(_host(index))).astype(np.int32)
        if classes is None:
            return scores, index
        return scores, index, [[classes[int(i)] if i >= 0 else None for i in row] for row in np.asarray(_host(index))]

    def matches(self, source, embeds, thresh_score, classes=None, num_eval=10, scoring_mode="cosine", cohorts=None, cohorts_path=None,
                cohort_top=200):
        """Which enrolled classes match at all?  For every file of ``source`` ALL classes of the gallery whose score is at least
        ``thresh_score``, however many or few - where ``identify(top=k, thresh_score=...)`` stops at its k best.  Sources, gallery forms,
        the preparation of both sides, ``scoring_mode`` and the cohort arguments are ``identify``'s, and so is every score (bit for bit);
        the search is ONE ``score_above`` call, which writes no score below the threshold anywhere.

        Returns ``(scores, index)``: per file a float32 array and an int32 array of its matches, best first (score descending, equal
        scores by the lower class index: ``identify``'s order), empty for a file without a match; and as a third item the class names
        (a list per file) when ``classes`` is given or the directory holds ``classes.npy``."""
        q, gal, classes, cohorts = self._search_operands(source, embeds, classes, num_eval, scoring_mode, cohorts, cohorts_path)
        row_ptr, index, score = scoring.score_above(q, gal, thresh_score, cohort=cohorts, top=int(cohort_top), device=self.gpu)
        row_ptr, index, score = np.asarray(_host(row_ptr)), np.asarray(_host(index)), np.asarray(_host(score))
        scores, found = [], []
        for n in range(q.shape[0]):
            seg = slice(int(row_ptr[n]), int(row_ptr[n + 1]))
            order = np.argsort(-score[seg], kind="stable")              # (the segment is in ascending class index: ties keep it)
            scores.append(score[seg][order])
            found.append(index[seg][order])
        if classes is None:
            return scores, found
        return scores, found, [[classes[int(i)] for i in row] for row in found]

    def duplicates(self, embeds, thresh_score, classes=None, scoring_mode="cosine", cohorts=None, cohorts_path=None, cohort_top=200,
                   chunk=65536):
        """Who was enrolled twice?  The self-join of a gallery (``identify``'s three forms, prepared the same way): every pair of
        classes ``i < j`` whose score is at least ``thresh_score``, each once, no class with itself.  The gallery is joined ``chunk``
        query rows at a time (``score_above`` with ``upper=True``), so no N x N matrix exists.

        Returns ``(i, j, score)``: int32, int32 and float32 arrays of equal length, ordered by i, then j; and as a fourth item the
        pairs of class names when ``classes`` is given or the directory holds ``classes.npy``."""
        gal, classes = self._gallery(embeds, classes)
        cohorts = self._cohort(scoring_mode, cohorts, cohorts_path, gal.shape[1])
        eng = scoring.scoring_engine(self.gpu)
        eng.l2norm_(gal)
        g_stats = None if cohorts is None else eng.asnorm_stats(gal, cohorts, int(cohort_top))
        ii, jj, ss = [], [], []
        for base in range(0, gal.shape[0], int(chunk)):
            rows = gal[base:base + int(chunk)]
            row_ptr, index, score = scoring.score_above(rows, gal, thresh_score, cohort=cohorts, top=int(cohort_top), g_stats=g_stats, upper=True,
                                                        q_base=base, device=self.gpu)
            ii.append(np.repeat(np.arange(base, base + rows.shape[0], dtype=np.int32), np.diff(np.asarray(_host(row_ptr)))))
            jj.append(np.asarray(_host(index)))
            ss.append(np.asarray(_host(score)))
        i, j, s = (np.concatenate(x) for x in (ii, jj, ss))
        if classes is None:
            return i, j, s
        return i, j, s, [(classes[int(a)], classes[int(b)]) for a, b in zip(i, j)]

    def cluster(self, source=None, embeds=None, thresh_score=None, classes=None, num_eval=10, scoring_mode="cosine", cohorts=None,
                cohorts_path=None, cohort_top=200, min_size=1, linkage="single"):
        """Which of these are the same speaker?  Groups unlabelled files, or the classes of a carelessly enrolled gallery: two rows are
        linked when their score is at least ``thresh_score``, and a cluster is a connected component of those links - by definition
        the components of the pair set ``duplicates`` returns on the same rows, found by ONE ``cluster_above`` call per set: one pass
        over the upper half of the self-join, no pair list, one int per row.

        Exactly one of ``source`` and ``embeds`` is given.  ``source``: files (what ``_embed_files`` takes), embedded and prepared as
        ``identify`` prepares its queries (crops L2-normalised when the loss sets ``test_normalize``, averaged, the mean L2-normalised).
        ``embeds``: a gallery in ``identify``'s three forms, prepared as ``duplicates`` prepares it.  ``scoring_mode`` and the cohort
        arguments are ``identify``'s: with ``"norm"`` a row's statistics are taken against the cohort and the link score is the
        adaptive-S-normalised one.

        ``linkage``: ``"single"`` (the default) is exactly the above, and single linkage chains: one borderline pair joins two
        speakers, and a string of them joins many.  ``"average"`` and ``"complete"`` do not: inside each of those components every row
        starts alone, and the two clusters whose mean (average) or smallest (complete) score is largest are merged while that value
        is at least ``thresh_score`` - two speakers that one bridge file has joined come apart again.  Both run on the device,
        component by component, without the n x n matrix (``Engine.cluster_linkage``).  A component of more than
        ``_lib.LINKAGE_MAX_ROWS`` rows is left as one cluster, and a ``RuntimeWarning`` names how many there were.
        ``scoring_mode="norm"``, whose threshold carries across speakers and channels, and ``min_size``, which drops the clusters too
        small to trust, help with every linkage.

        Returns ``(labels, groups)``.  ``labels`` (n,) int32: the dense cluster id of every row, clusters numbered in order of their
        smallest member; rows of clusters with fewer than ``min_size`` members get -1 and the remaining clusters are renumbered in the
        same order.  ``groups``: per kept cluster the list of its members in index order - the files of ``source``, the class names
        when ``classes`` is given or the directory holds ``classes.npy``, else the row indices."""
        if (source is None) == (embeds is None):
            raise ValueError("cluster: give exactly one of source (files) and embeds (a gallery)")
        if thresh_score is None:
            raise ValueError("cluster: thresh_score is required")
        if linkage not in scoring.LINKAGES:
            raise ValueError(f"cluster: linkage = {linkage!r} is not one of {scoring.LINKAGES}")
        min_size = int(min_size)
        if min_size < 1:
            raise ValueError(f"cluster: min_size = {min_size} must be at least 1")
        eng = scoring.scoring_engine(self.gpu)
        if source is not None:
            self.__model__.eval()
            names = list(source) if isinstance(source, (list, tuple)) else [source]
            if not names:
                raise ValueError("Please provide appropriate source!")
            rows = self._crop_mean_rows(names, num_eval)
        else:
            rows, classes = self._gallery(embeds, classes)
            names = [classes[i] for i in range(rows.shape[0])] if classes is not None else list(range(rows.shape[0]))
        cohorts = self._cohort(scoring_mode, cohorts, cohorts_path, rows.shape[1])
        eng.l2norm_(rows)
        if linkage == "single":
            _, ids, _ = scoring.cluster(rows, thresh_score, cohort=cohorts, top=int(cohort_top), device=self.gpu)
        else:
            _, ids, _, unrefined = scoring.cluster(rows, thresh_score, cohort=cohorts, top=int(cohort_top), device=self.gpu, linkage=linkage)
            if int(unrefined) > 0:
                warnings.warn(f"cluster: {int(unrefined)} component(s) of more than {_lib.LINKAGE_MAX_ROWS} rows were not refined by "
                              f"{linkage} linkage and stay one cluster each; raise thresh_score", RuntimeWarning, stacklevel=2)
        ids = np.asarray(_host(ids))
        sizes = np.bincount(ids, minlength=0)
        keep = sizes >= min_size
        renumber = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        labels = renumber[ids] if ids.size else np.zeros(0, np.int32)
        groups = [[] for _ in range(int(keep.sum()))]
        for i, c in enumerate(labels):
            if c >= 0:
                groups[c].append(names[i])
        return labels, groups

    def cluster_extend(self, base_embeds, base_labels=None, source=None, embeds=None, thresh_score=None, num_eval=10, scoring_mode="cosine",
                       cohorts=None, cohorts_path=None, cohort_top=200):
        """Which of the clusters I already have do these NEW files belong to?  Joins new rows to a base set that was clustered before
        (by ``cluster``, by a person, or not at all) in ONE ``cluster_join`` call: the base rows are not scored against each other
        again, so the cost grows with (base x new + new^2 / 2) pairs, not with the square of everything ever ingested.

        ``base_embeds``: the base set in ``identify``'s three gallery forms, prepared as ``cluster(embeds=)`` prepares it.
        ``base_labels``: its known grouping as any integer labelling (an equal label means the same cluster; ``cluster``'s ``labels``
        with ``min_size=1``, or labels a person has corrected) - it is trusted, not rescored; ``None``: every base row is a cluster of
        its own (an enrolled gallery).  The new rows: exactly one of ``source`` (files) and ``embeds`` (a gallery), prepared as
        ``cluster`` prepares them; their own pairs are scored.  ``scoring_mode`` and the cohort arguments are ``identify``'s.

        Only SINGLE linkage is served: a cluster is a connected component of the links, and with ``base_labels = cluster(base)``'s
        labels the result is exactly ``cluster`` of base and new rows together.  A new row may join a base cluster, start a new one,
        or bridge two base clusters, which then come back as one.

        Returns ``(base_ids (NA,) int32, new_ids (NB,) int32, merged)``: the dense ids of the joint clustering, numbered in order of
        each cluster's smallest member (base rows first), and ``merged``: the groups of DISTINCT input base labels that ended in one
        cluster, each a sorted list, in order of the cluster's id - empty when no new row bridged anything."""
        if (source is None) == (embeds is None):
            raise ValueError("cluster_extend: give exactly one of source (files) and embeds (a gallery)")
        if thresh_score is None:
            raise ValueError("cluster_extend: thresh_score is required")
        base, _ = self._gallery(base_embeds, None)
        if base_labels is None:
            base_labels = np.arange(base.shape[0], dtype=np.int64)
        base_labels = np.asarray(_host(base_labels)).reshape(-1)
        if base_labels.shape[0] != base.shape[0]:
            raise ValueError(f"cluster_extend: {base_labels.shape[0]} base labels for {base.shape[0]} base rows")
        cohorts = self._cohort(scoring_mode, cohorts, cohorts_path, base.shape[1])
        eng = scoring.scoring_engine(self.gpu)
        if source is not None:
            self.__model__.eval()
            names = list(source) if isinstance(source, (list, tuple)) else [source]
            if not names:
                raise ValueError("Please provide appropriate source!")
            rows = self._crop_mean_rows(names, num_eval)
        else:
            rows, _ = self._gallery(embeds, None)
        if rows.shape[1] != base.shape[1]:
            raise ValueError(f"the new rows are {rows.shape[1]} wide, the base set {base.shape[1]}")
        eng.l2norm_(base)
        eng.l2norm_(rows)
        _, ids, _ = scoring.cluster_join(base, rows, thresh_score, labels_a=base_labels, cohort=cohorts, top=int(cohort_top), device=self.gpu)
        ids = np.asarray(_host(ids)).astype(np.int32, copy=False)
        base_ids, new_ids = ids[:base.shape[0]], ids[base.shape[0]:]
        seen = {}
        for c, lab in zip(base_ids.tolist(), base_labels.tolist()):
            seen.setdefault(c, set()).add(lab)
        merged = [sorted(labs) for c, labs in sorted(seen.items()) if len(labs) > 1]
        return base_ids, new_ids, merged

    # ---- dataset audit ----------------------------------------------------------------------------------------------------
    def audit(self, source, thresh_score, num_eval=20, save_file=None, max_files=65536):
        """Which files of a speaker folder do not sound like the rest of it?  The reference's label-noise audit
        (src/benchmark/benchmark_dataset.py:32-84): every file is embedded as ``embed_utterance(num_eval, normalize=True)`` does, ALL
        pairs of files of a folder are scored with ``similarity_measure('cosine')`` (the mean over the crops of |cos|, crop c against
        crop c) and a file's count is the number of partners it does not match under the reference's rule at ``thresh_score``
        (``scoring.audit_cut``).

        ``source``: a directory whose sub-directories are speakers (found as ``prepare('embed')`` finds them, ``*.wav`` inside), or
        ``{name: [files]}``.  Whole folders are collected up to ``max_files`` files (a larger folder goes alone); each collection is
        embedded in one ``_embed_files`` call (``num_eval=0``: whole files through the ragged path, one crop), every crop row is
        L2-normalised, and ONE ``group_audit`` call counts - no pair list, no score leaves the device.

        Returns, per folder in order, ``(folder, n_files, [(file, count), ...])`` with the files whose count is > 0, sorted by path.
        ``save_file``: the reference's report text is appended to it, for the folders with at least one such file."""
        self.__model__.eval()
        if isinstance(source, dict):
            folders = [(str(k), [str(f) for f in v]) for k, v in source.items()]
        elif isinstance(source, (str, Path)):
            folders = [(str(d), [str(f) for f in d.glob("*.wav")]) for d in Path(source).iterdir() if d.is_dir()]
        else:
            raise ValueError("Please provide appropriate source!")
        max_files = int(max_files)
        if max_files < 1:
            raise ValueError(f"max_files = {max_files} must be at least 1")
        on_dev = self._feats_on_device()
        counts = [None] * len(folders)

        def run(batch):
            files = [f for g in batch for f in folders[g][1]]
            if not files:
                for g in batch:
                    counts[g] = np.zeros(0, np.int32)
                return
            feats = self._l2norm_crops(self._embed_files(files, num_eval, on_device=on_dev))     # embed_utterance(normalize=True)
            group_ptr = np.zeros(len(batch) + 1, np.int64)
            np.cumsum([len(folders[g][1]) for g in batch], out=group_ptr[1:])
            miss = np.asarray(_host(scoring.group_audit(feats, group_ptr, thresh_score, device=self.gpu)))
            for k, g in enumerate(batch):
                counts[g] = miss[group_ptr[k]:group_ptr[k + 1]]

        batch, held = [], 0
        for g, (_, fl) in enumerate(folders):
            if batch and held + len(fl) > max_files:
                run(batch)
                batch, held = [], 0
            batch.append(g)
            held += len(fl)
        if batch:
            run(batch)

        result = []
        for (folder, fl), c in zip(folders, counts):
            result.append((folder, len(fl), sorted((f, int(n)) for f, n in zip(fl, c) if n > 0)))
        if save_file:
            with open(save_file, "a+") as fh:
                for folder, n, found in result:
                    if found:
                        fh.write(f"Folder:{folder}\n")
                        for f, cnt in found:
                            fh.write(f"[{cnt}/{n}] - {f}\n")
                        fh.write("//================//\n")
        return result

    # ---- checkpoints ------------------------------------------------------------------------------------------------------
    def saveParameters(self, path):
        torch.save(self.__model__.module.state_dict(), path)

    def loadParameters(self, path, show_error=True):
        """src/model.py:718-746: name-matched copy; 'module.' prefixes stripped; unknown or mis-shaped
        tensors are reported and skipped.  (map_location is 'cpu': weights are repacked for the device.)"""
        if not os.path.exists(path):
            raise FileNotFoundError("Model's path is not exists")
        from . import checkpoint
        if checkpoint.is_blob(path):                     # packed blob (checkpoint.convert_checkpoint): bare __S__ names
            _, sd = checkpoint.read_blob(path)
            loaded = {"__S__." + k: torch.from_numpy(v) for k, v in sd.items()}
        else:
            loaded = torch.load(path, map_location="cpu")
        own = self.__model__.module.state_dict()
        keep = {}
        for name, param in loaded.items():
            orig = name
            if name not in own:
                name = name.replace("module.", "")
                if name not in own:
                    if show_error and name.startswith("__S__."):
                        print("{} is not in the model.".format(orig))
                    continue
            if tuple(own[name].shape) != tuple(param.shape):
                if show_error:
                    print("Wrong parameter length: {}, model: {}, loaded: {}".format(orig, tuple(own[name].shape), tuple(param.shape)))
                continue
            keep[name] = param
        self.__model__.module.load_state_dict(keep, strict=False)
