"""ResNetSE34V2's stages against the float64 oracle (oracle/resnetse.py), one utterance at a time: the comparisons and bars of
tests/test_gpu_resnetse_oracle.py.  They need no GPU, so tests/test_resnetse_oracle_host.py runs them on a CPU emulation of a handle,
takes the bars from it and shows that every bar fails when the kernel it guards is subtly wrong.

Layer-local checks.  Option rs_keep makes a forward copy what it stores anyway; each stored tensor is compared with the oracle's step
applied in float64 to the handle's OWN stored input of that step:

    xin        from the mel power the handle was given; in a waveform case from the oracle's own front-end of the waveform
    stem       from xin
    per block  conv1 and down from the block's stored input (the stem's output, then the previous out), conv2 from the stored conv1,
               part (the SE tile sums, ntp ntq x C) and part_total (their sum over the tiles against the sum over the image), gate,
               out from the stored conv2, gate and down or the block's input
    att        from the last out (the handle's columns q C + c brought into the reference's c Q + q: oracle.resnetse.ref_cols);
    logits     from att;  pool_raw from the stored logits and the last out;  pool from pool_raw (the affine of the pooling kernel is the
               identity here: pool is pool_raw bit for bit, on the emulation and on the GPU, and its bar is 0);
    emb        from pool;  end_to_end: the embedding against the oracle on the checkpoint's own weights

part and gate.  rs_conv_kernel adds the fp32 value it is ABOUT to store, so on a bf16 handle the tile sums are those of the unrounded
conv2 and differ from the sums of the stored tensor by the bf16 roundings of a tile.  part and part_total are therefore compared with
the sums of the oracle's own unrounded conv2, recomputed from the stored conv1 (on an f32 handle that is the stored conv2 to an fp32
sum, and the same reference serves); the tile grid is oracle.resnetse.tile_of, rs_tile_of restated, and the number of stored rows must
equal its ntp ntq.  gate is ecapa_oracle_check.nearer_err: each element against the nearer of the SE MLP of the mean of the stored
conv2 and of the mean of the unrounded recomputation.  The emulation takes the sums where the kernel does.

The error of a check is taken over ONE utterance; an image (P, Q, C) is read as (P Q, C) and has four forms — `name` (max |diff| / max
|ref|), `name/local` (each element against its own size), `name/bias` (an error common to every position of a channel) and `name/gain`
(the regression slope of got on ref, minus one).  A block check's value is the worst over the sixteen blocks; a failure names block,
position (p, q) and channel.  rel_err, local_err, bias_err and nearer_err are tests/ecapa_oracle_check.py's, gain_err and frame_errs
tests/conformer_oracle_check.py's.

The layer-local references read the numbers the handle reads (oracle.resnetse.folded_sd / rounded_sd); end_to_end reads the
checkpoint's weights in float64.

THE BARS are not taken from the GPU.  Each is 3 x the worst error of the clean CPU emulation (emulate: the oracle's own steps in fp32,
every convolution's products added in rs_conv_kernel's order — channel chunks of 16 / 32 outermost, then the nine taps, one MFMA's
products at a time — the epilogue, the stem's taps and the tail as fused multiply-adds, the tile sums per half-wave, wave and tile in
the kernel's order, the gate's tile loop in index order, the two attention GEMMs in their k-order, the pooling's variance in the
centred form its kernel sums; for bf16 with rounded weights and every stored tensor rounded to bf16), over every case of CASES.  Beside
each bar: the emulation's value, then the GPU's worst over the whole GPU file.

xin.  The emulation follows the shared front-end's own arithmetic in two places, both read from its code after the first GPU run sat
above an emulation that did not (the bars were then rebuilt from the emulation, not from that run):
  * prologue_stats_row (fbank.hip) centres a row ONCE: it takes the mean of the centred row as zero, where the reference's
    InstanceNorm1d subtracts it again.  The residual, half an fp32 step of the row's sum, is multiplied by 1 / sqrt(var + eps), which
    is large where a mel row barely moves over the frames: xin 1.9e-5 and xin/bias 2.5e-5 at T = 2 against 3.0e-6 and 0 with the
    second centring (oracle.resnetse.prologue, kernel_form), 1.0 - 1.8e-6 of bias at T = 129.  One pass that also sums the centred
    values would remove it; the kernel is shared with every model and is left as it is here.
  * on a BF16 handle `fbank` runs its bf16x3 form (samples and basis split into bf16 hi + lo, the lo lo products dropped: 2^-16 of a
    product), which is documented in fbank.hip for handles that round their features to bf16 right after.  ResNetSE keeps xin in fp32,
    so it shows: from waveforms xin 1.1e-4 and xin/local 6.6e-3, in mel bin 0, which the pre-emphasis leaves with little energy
    (mel_emulated_split gives the GPU's figures to two digits; an f32 handle stays at 1.6e-6 / 4.3e-5).  The bf16 xin and xin/local
    bars are therefore those of the waveform case; from features the GPU's worst is 2.0e-5 / 6.8e-5 on both computes.
From waveforms on an f32 handle xin/gain is 1.8e-8 (7.2e-9 in that case's emulation, bar 6.5e-8): the log and the mean over time remove a
common gain of the mel power, so the offset TitaNet's prolog showed (3.0e-8) cannot be seen in xin."""
import numpy as np
import torch

from oracle import fbank as o_fbank, resnetse as orr
from speakerverification_amd import synth
from tests import fbank_emulation
from tests.conformer_oracle_check import KSTEP, frame_errs, gain_err  # noqa: F401
from tests.ecapa_oracle_check import bias_err, local_err, nearer_err, rel_err  # noqa: F401
from tests.titanet_oracle_check import mel_emulated

SEED_W, SEED_X = 1, 20220829
GAINS = (1.0, 3.0, 0.3)                       # the utterances of a case are scaled differently
NOUT = 256
HOP = 80
EDGE_T = (2, 3, 5, 8, 9, 16, 17, 33, 65, 129)
RAGGED_T = (2, 3, 5, 8, 9, 17, 33, 65)
RAGGED_ONE_T = (33,)
FULL_T = 401                                  # 32000 samples
CK = {"f32": 16, "bf16": 32}                  # input channels of one K chunk of rs_conv_kernel
FRAME_STAGES = ("xin", "stem", "conv1", "conv2", "down", "out", "att", "logits")
VECTOR_STAGES = ("part", "part_total", "gate", "pool_raw", "pool", "emb", "end_to_end")
FORMS = ("", "/local", "/bias", "/gain")
CHECKS = tuple(s + f for s in FRAME_STAGES for f in FORMS) + VECTOR_STAGES

# (kind, n_mels, encoder, log_input, T).  "edge": B = 3 of features at T; "full": B = 3 waveforms, the last utterance checked; "ragged" /
# "ragged1": the packs of RAGGED_T / RAGGED_ONE_T (T ignored)
CASES = tuple(("edge", 80, "ASP", True, T) for T in EDGE_T) + (("edge", 64, "ASP", True, 33), ("edge", 80, "SAP", True, 33),
                                                               ("edge", 80, "ASP", False, 17), ("full", 80, "ASP", True, FULL_T),
                                                               ("ragged", 80, "ASP", True, 0), ("ragged1", 80, "ASP", True, 0))
FULL_ROWS = (2,)

# check: bar,   # emulation, GPU
F32_BARS = {
    "xin": 5.7e-05,                 # 1.9e-05, 2.0e-05
    "xin/local": 1.4e-04,           # 4.7e-05, 6.8e-05
    "xin/bias": 7.4e-05,            # 2.5e-05, 2.4e-05
    "xin/gain": 6.5e-08,            # 2.2e-08, 2.4e-08
    "stem": 4.8e-07,                # 1.6e-07, 1.6e-07
    "stem/local": 6.1e-06,          # 2.0e-06, 1.8e-06
    "stem/bias": 8.6e-08,           # 2.9e-08, 3.8e-08
    "stem/gain": 5.5e-09,           # 1.8e-09, 2.8e-09
    "conv1": 6.6e-06,               # 2.2e-06, 2.2e-06
    "conv1/local": 1.4e-04,         # 4.6e-05, 4.5e-05
    "conv1/bias": 2.4e-06,          # 8.0e-07, 1.4e-06
    "conv1/gain": 1.1e-07,          # 3.7e-08, 5.4e-08
    "conv2": 4.3e-06,               # 1.4e-06, 1.7e-06
    "conv2/local": 1.4e-04,         # 4.8e-05, 4.4e-05
    "conv2/bias": 2.5e-06,          # 8.3e-07, 8.5e-07
    "conv2/gain": 8.4e-08,          # 2.8e-08, 3.9e-08
    "down": 1.1e-06,                # 3.8e-07, 5.4e-07
    "down/local": 3.6e-05,          # 1.2e-05, 1.0e-05
    "down/bias": 6.5e-07,           # 2.2e-07, 3.1e-07
    "down/gain": 3.1e-08,           # 1.0e-08, 1.5e-08
    "out": 1.7e-07,                 # 5.8e-08, 5.7e-08
    "out/local": 1.7e-07,           # 5.8e-08, 5.8e-08
    "out/bias": 1.7e-07,            # 5.6e-08, 5.1e-08
    "out/gain": 1.6e-08,            # 5.5e-09, 4.6e-09
    "att": 7.6e-06,                 # 2.5e-06, 2.1e-06
    "att/local": 8.9e-05,           # 3.0e-05, 3.4e-05
    "att/bias": 7.6e-06,            # 2.5e-06, 2.0e-06
    "att/gain": 9.9e-07,            # 3.3e-07, 3.2e-07
    "logits": 1.7e-06,              # 5.8e-07, 6.0e-07
    "logits/local": 2.4e-05,        # 7.8e-06, 8.3e-06
    "logits/bias": 1.7e-06,         # 5.8e-07, 1.2e-06
    "logits/gain": 2.9e-08,         # 9.8e-09, 9.7e-09
    "part": 8.3e-07,                # 2.8e-07, 3.6e-07
    "part_total": 8.3e-07,          # 2.8e-07, 3.6e-07
    "gate": 1.0e-06,                # 3.4e-07, 2.6e-07
    "pool_raw": 9.0e-07,            # 3.0e-07, 2.9e-07
    "pool": 0.0e+00,                # 0.0e+00, 0.0e+00
    "emb": 1.9e-06,                 # 6.4e-07, 2.0e-07
    "end_to_end": 9.1e-06,          # 3.0e-06, 1.5e-06
}
BF16_BARS = {
    "xin": 3.2e-04,                 # 1.1e-04, 1.1e-04
    "xin/local": 2.0e-02,           # 6.6e-03, 6.6e-03
    "xin/bias": 7.4e-05,            # 2.5e-05, 2.4e-05
    "xin/gain": 6.5e-08,            # 2.2e-08, 2.4e-08
    "stem": 1.0e-02,                # 3.4e-03, 3.4e-03
    "stem/local": 1.1e-02,          # 3.8e-03, 3.8e-03
    "stem/bias": 1.3e-02,           # 4.2e-03, 4.2e-03
    "stem/gain": 1.5e-03,           # 4.9e-04, 4.9e-04
    "conv1": 1.1e-02,               # 3.8e-03, 3.6e-03
    "conv1/local": 1.1e-02,         # 3.8e-03, 3.8e-03
    "conv1/bias": 9.6e-03,          # 3.2e-03, 3.2e-03
    "conv1/gain": 6.6e-04,          # 2.2e-04, 2.4e-04
    "conv2": 1.1e-02,               # 3.7e-03, 3.7e-03
    "conv2/local": 1.1e-02,         # 3.8e-03, 3.8e-03
    "conv2/bias": 9.6e-03,          # 3.2e-03, 3.5e-03
    "conv2/gain": 5.0e-04,          # 1.7e-04, 1.7e-04
    "down": 1.0e-02,                # 3.4e-03, 3.8e-03
    "down/local": 1.1e-02,          # 3.8e-03, 3.8e-03
    "down/bias": 7.2e-03,           # 2.4e-03, 3.1e-03
    "down/gain": 5.1e-04,           # 1.7e-04, 1.4e-04
    "out": 1.1e-02,                 # 3.8e-03, 3.8e-03
    "out/local": 1.1e-02,           # 3.8e-03, 3.8e-03
    "out/bias": 2.6e-02,            # 8.7e-03, 8.8e-03
    "out/gain": 1.4e-03,            # 4.7e-04, 4.7e-04
    "att": 1.1e-02,                 # 3.7e-03, 3.8e-03
    "att/local": 1.1e-02,           # 3.7e-03, 3.7e-03
    "att/bias": 1.1e-02,            # 3.7e-03, 3.2e-03
    "att/gain": 2.2e-03,            # 7.3e-04, 9.3e-04
    "logits": 7.7e-07,              # 2.6e-07, 1.9e-07
    "logits/local": 1.2e-05,        # 3.9e-06, 3.2e-06
    "logits/bias": 9.2e-07,         # 3.1e-07, 4.3e-07
    "logits/gain": 1.3e-08,         # 4.5e-09, 5.9e-09
    "part": 6.0e-07,                # 2.0e-07, 2.5e-07
    "part_total": 6.0e-07,          # 2.0e-07, 2.5e-07
    "gate": 1.2e-06,                # 4.1e-07, 2.9e-07
    "pool_raw": 7.7e-07,            # 2.6e-07, 2.7e-07
    "pool": 0.0e+00,                # 0.0e+00, 0.0e+00
    "emb": 2.4e-06,                 # 8.0e-07, 2.3e-07
    "end_to_end": 3.6e-02,          # 1.2e-02, 1.2e-02
}


def bars(compute):
    return {"f32": F32_BARS, "bf16": BF16_BARS}[compute]


def samples_of(T):
    """a sample count that gives at least T mel frames (hop 80), at least the 512 samples of one FFT window"""
    return max(512, HOP * (T - 1))


def mel_emulated_split(wave):
    """(L,) samples -> (80, T) mel power in fp32 as the front-end of a BF16 handle adds it up (fbank.hip, the bf16x3 form) at the default
    geometry: tests/fbank_emulation.py states the sums and takes any geometry.  The dropped lo lo term is 2^-16 of a product: after the
    log, 1e-4 of xin in a mel bin with little energy, where an f32 handle (titanet_oracle_check.mel_emulated) keeps 1e-6"""
    return fbank_emulation.mel_emulated_split(wave)


def engine_kw(T):
    """samples / hop_length of a fixed-length handle of T frames (T = samples // hop + 1).  A handle takes at least the 512 samples of one
    FFT window, seven frames at the front-end's hop of 80; a shorter image, which only a features call can bring, gets a handle with a
    longer hop (the network never sees the hop)"""
    if HOP * (T - 1) >= 512:
        return dict(samples=HOP * (T - 1), hop_length=HOP)
    assert 512 % (T - 1) == 0 and 512 // (T - 1) % 4 == 0, T
    return dict(samples=512, hop_length=512 // (T - 1))


def engine_samples(T):
    return engine_kw(T)["samples"]


def waveforms(B, L):
    """the inputs of a case: synth's waveforms, utterance b scaled by GAINS[b % 3]"""
    x = synth.synth_waveforms(B, L, seed=SEED_X + L)
    return np.ascontiguousarray(x * np.asarray([GAINS[b % 3] for b in range(B)], np.float32)[:, None])


def mel_of(wave, dtype=torch.float64, n_mels=80):
    """(L,) samples -> (n_mels, T) mel power"""
    return o_fbank.melspectrogram(torch.as_tensor(wave).to(dtype)[None], n_mels=n_mels)[0]


_FEATS = {}


def features(B, T, n_mels=80):
    """(B, n_mels, T) float32 mel power: the oracle's front-end on waveforms(B, samples_of(T)), its first T frames; cached, never written"""
    if (B, T, n_mels) not in _FEATS:
        _FEATS[B, T, n_mels] = np.stack([mel_of(w, torch.float32, n_mels).numpy()[:, :T] for w in waveforms(B, samples_of(T))])
        _FEATS[B, T, n_mels].setflags(write=False)
    return _FEATS[B, T, n_mels]


def ragged_features(lengths=RAGGED_T):
    """a pack's utterances: utterance u is features(u + 1, T_u)[u], so that every one has its own content and gain"""
    return [np.ascontiguousarray(features(u + 1, T)[u]) for u, T in enumerate(lengths)]


def case_features(case):
    kind, n_mels, _, _, T = case
    if kind == "ragged":
        return ragged_features(RAGGED_T)
    if kind == "ragged1":
        return ragged_features(RAGGED_ONE_T)
    return list(features(3, T, n_mels))


_W = {}


def weights(n_mels=80, enc="ASP"):
    """{"sd": numpy checkpoint, "full": float64 tensors, "f32" / "bf16": (what an emulation reads in fp32, what a handle of that compute
    reads as float64 reference)}"""
    key = (n_mels, enc)
    if key not in _W:
        sd = synth.synth_state_dict(synth.resnetse_param_spec(NOUT, n_mels, enc), seed=SEED_W)
        full = orr.to_torch_sd(sd)
        _W[key] = {"sd": sd, "full": full}
        for compute in ("f32", "bf16"):
            ref = orr.folded_sd(full, bf16=compute == "bf16")
            _W[key][compute] = (orr.to_torch_sd(ref, torch.float32), ref)
    return _W[key]


def emulate(mel, sd32, compute, log_input=True):
    """the stages of a handle on the CPU for one utterance: ({stage: float64 array}, the embedding).  mel (n_mels, T) and sd32 in float32
    (the folded weights of the handle: weights()[compute][0])"""
    q = orr.bf16_round if compute == "bf16" else orr.ident
    st = {}
    with torch.no_grad(), orr.matmul_as(orr.chained_matmul(KSTEP[compute])), orr.conv_as(orr.chained_conv(CK[compute], KSTEP[compute])):
        emb = orr.forward(mel, sd32, log_input, store=q, squeeze_acc=True, kernel_sums=True, stages=st)
    return {k: v.double().numpy() for k, v in st.items()}, emb.double().numpy()


_EMU = {}


def emulated_case(compute, case):
    """the clean emulation of a case, cached: [(stages, embedding, layer_local's errors)] per checked utterance"""
    if (compute, case) not in _EMU:
        kind, n_mels, enc, log_input, T = case
        w = weights(n_mels, enc)
        sd32, sdref = w[compute]
        if kind == "full":
            x = waveforms(3, engine_samples(T))
            inputs = [(mel_emulated_split(x[b]) if compute == "bf16" else mel_emulated(x[b], compute), mel_of(x[b])) for b in FULL_ROWS]
        else:
            inputs = [(torch.tensor(f), torch.tensor(f).double()) for f in case_features(case)]
        out = []
        for m32, m64 in inputs:
            S, emb = emulate(m32, sd32, compute, log_input)
            with torch.no_grad():
                e2e = orr.forward(m64, w["full"], log_input).numpy()
            out.append((S, emb, layer_local(S, sdref, log_input, mel=m64, emb=emb, e2e_ref=e2e)))
        _EMU[(compute, case)] = out
    return _EMU[(compute, case)]


def emulation_worst(compute):
    """{check: the clean emulation's worst error over CASES and the utterances of each}"""
    worst = {}
    for case in CASES:
        for _, _, err in emulated_case(compute, case):
            for n, (e, _) in err.items():
                worst[n] = max(worst.get(n, 0.0), e)
    return worst


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def gate_err(got, conv2_stored, conv2_exact, sd, p):
    """a block's gate against the nearer of its two references, element by element (module docstring)"""
    with torch.no_grad():
        a, b = (orr.gate(orr.squeeze(v), sd, p).numpy() for v in (conv2_stored, conv2_exact))
    return nearer_err(got, a, b)


def part_errs(got, conv2_exact):
    """(part's (error, index), part_total's) of a block's stored tile sums (ntiles, C) against the oracle's unrounded conv2 (P, Q, C); the
    stored rows must be the ntp ntq tiles of rs_tile_of on this image"""
    P, Q, _ = conv2_exact.shape
    TP, TQ, ntp, ntq = orr.tile_grid(P, Q)
    assert got.shape[0] == ntp * ntq, (got.shape, (P, Q), (TP, TQ, ntp, ntq))
    ref = orr.tile_sums(conv2_exact).numpy()
    tot = conv2_exact.sum(dim=(0, 1)).numpy()
    # (the total is judged on the scale of the tile sums: it is their sum, and channels cancel over an image)
    d = np.abs(np.asarray(got, np.float64).sum(axis=0) - tot)
    c = int(np.argmax(d))
    return rel_err(got, ref), (float(d[c]) / max(float(np.abs(ref).sum(axis=0).max()), 1e-30), (c,))


def layer_local(S, sd, log_input=True, mel=None, emb=None, e2e_ref=None):
    """{check: (error, worst index)} of one utterance.  S: the handle's stages of the utterance as float64 arrays in the oracle's layouts —
    xin (T, Q), stem and b<i>_conv1 | _conv2 | _down | _out (P, Q, C), b<i>_part (tiles, C), b<i>_gate (C,), att (P4, 128), logits
    (P4, C Q) and pool_raw, pool (2 C Q,) in the reference's column order.  sd: the float64 weights the handle reads.  mel: the
    reference's mel power (n_mels, T); emb / e2e_ref: the handle's embedding and the oracle's end to end.  A block check's index is
    (block, p, q, channel)."""
    err = {}

    def worse(name, e, idx):
        if name not in err or e > err[name][0] or e != e:
            err[name] = (e, idx)

    def image(name, got, ref, blk=None):
        ref = ref.numpy()
        assert got.shape == ref.shape, (name, blk, got.shape, ref.shape)
        Q = ref.shape[1] if ref.ndim == 3 else None
        for form, (e, idx) in frame_errs(got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])).items():
            if Q is not None:
                idx = (idx[0] // Q, idx[0] % Q, idx[1])
            worse(name + form, e, idx if blk is None else (blk,) + tuple(idx))

    def vector(name, got, ref, blk=None):
        e, idx = rel_err(got, ref.numpy() if torch.is_tensor(ref) else ref)
        worse(name, e, idx if blk is None else (blk,) + tuple(idx))

    with torch.no_grad():
        if mel is not None:
            image("xin", S["xin"], orr.prologue(mel, log_input))
        image("stem", S["stem"], orr.stem(_t(S["xin"]), sd))
        x = _t(S["stem"])
        for i, p in enumerate(orr.block_names(sd)):
            g = {k: _t(S[f"b{i}_{k}"]) for k in orr.BLOCK_STEPS if f"b{i}_{k}" in S}
            assert ("down" in g) == orr.has_down(sd, p), (i, sorted(g))
            image("conv1", S[f"b{i}_conv1"], orr.conv1(x, sd, p), i)
            exact = orr.conv2(g["conv1"], sd, p)
            image("conv2", S[f"b{i}_conv2"], exact, i)
            (e, idx), (et, it) = part_errs(S[f"b{i}_part"], exact)
            worse("part", e, (i,) + idx)
            worse("part_total", et, (i,) + it)
            e, idx = gate_err(S[f"b{i}_gate"], g["conv2"], exact, sd, p)
            worse("gate", e, (i,) + idx)
            if "down" in g:
                image("down", S[f"b{i}_down"], orr.down(x, sd, p), i)
                image("out", S[f"b{i}_out"], orr.out(g["conv2"], g["gate"], g["down"], res_relu=False), i)
            else:
                image("out", S[f"b{i}_out"], orr.out(g["conv2"], g["gate"], x), i)
            x = g["out"]
        xf, a, lg = orr.flat(x), _t(S["att"]), _t(S["logits"])
        image("att", S["att"], orr.att(xf, sd))
        image("logits", S["logits"], orr.logits(a, sd))
        vector("pool_raw", S["pool_raw"], orr.pool_stats(lg, xf))
        vector("pool", S["pool"], S["pool_raw"])
        if emb is not None:
            vector("emb", emb, orr.fc(_t(S["pool"]), sd))
    if emb is not None and e2e_ref is not None:
        err["end_to_end"] = rel_err(emb, e2e_ref)
    return err


def where(check, idx):
    """the worst element of a check in words"""
    if check in VECTOR_STAGES:
        return (f"block {idx[0]} " if check in ("part", "part_total", "gate") else "") + (f"tile {idx[1]} " if check == "part" else "") + f"channel {idx[-1]}"
    blk = f"block {idx[0]} " if len(idx) == 4 else ""
    if check.endswith("/gain"):
        return blk + "(whole tensor)"
    if check.endswith("/bias"):
        return blk + f"channel {idx[-1]}"
    return blk + (f"position ({idx[-3]}, {idx[-2]}) channel {idx[-1]}" if len(idx) >= 3 else f"frame {idx[0]} column {idx[1]}")


def failures(err, compute):
    """the checks over their bars: [(check, error, bar, where the worst element sits)]"""
    bar = bars(compute)
    return [(n, e, bar[n], where(n, i)) for n, (e, i) in err.items() if not e <= bar[n]]


def describe(err):
    """one line: every check's error in stage order"""
    return ", ".join(f"{n} {err[n][0]:.2e}" for n in CHECKS if n in err)
