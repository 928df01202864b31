"""TitaNet's stages against the float64 oracle (oracle/titanet.py), one utterance at a time: the comparisons and bars of
tests/test_gpu_titanet_oracle.py.  They need no GPU, so tests/test_titanet_oracle_host.py runs them on a CPU emulation of a handle,
takes the bars from it and shows that every bar fails when the kernel it guards is subtly wrong.

Layer-local checks.  Option tn_keep makes a forward copy what it stores anyway; each stored tensor is compared with the oracle's step
applied in float64 to the handle's OWN stored input of that step:

    prolog     from the mel power the handle was given; in a waveform case from the oracle's own front-end of the waveform
    per block  skip and dw0 from the block's input (block 0: tn_prolog — tn_dw; later blocks: the previous out — there dw0 comes from the
               previous block's tn_mega_tail, which recomputes y on its halo rows: this is the check that sees that recomputation),
               pw0 from dw0, dw1 from pw0, pw1 from dw1, dw2 from pw1, pw2 from dw2 (the GEMMs and tn_dw, one launch each),
               mean (where the squeeze kernel ran) and gate from the stored pw2, out from the stored skip, pw2 and gate
    enc        from the last out;  att from enc;  logits from att;  pool_raw from the stored logits and enc;  pool from pool_raw;
    emb        from pool;  end_to_end: the embedding against the oracle on the checkpoint's own weights

gate has two producers of its squeeze.  tn_se_mean / rag_se_mean read the STORED pw2; where the third pointwise GEMM writes column sums
(bf16, fixed-length, T >= 256) the squeeze is taken from the GEMM's UNROUNDED accumulators and no mean vector exists.  The two differ by
the mean of T bf16 roundings — 2e-4 of the gate's scale at T = 256, as much as a dropped frame at T = 401 moves it — so a bar that
covered the rounding could not see one frame.  The check is ecapa_oracle_check.nearer_err, which exists for this case: each element
against the nearer of two float64 references, the SE MLP of the squeeze of the stored pw2 and of the oracle's own unrounded pw2
recomputed from the stored dw2 (what the accumulators hold, to an fp32 sum).  The emulation takes the squeeze from the unrounded values
exactly where the handle does; the bar sits 4 x below one dropped frame (tests/test_titanet_oracle_host.py).

The error of a check is taken over ONE utterance; a frame tensor (T, channels) has four forms — `name` (max |diff| / max |ref|),
`name/local` (each element against its own size), `name/bias` (an error common to every frame of a channel) and `name/gain` (the
regression slope of got on ref, minus one).  A block check's value is the worst over the blocks; the failure names block, frame and
channel.  rel_err, local_err and bias_err are tests/ecapa_oracle_check.py's, gain_err and frame_errs tests/conformer_oracle_check.py's.

The layer-local references read the numbers the handle reads (oracle.titanet.folded_sd / rounded_sd: every BatchNorm folded into its
conv in double and cast to fp32, on a bf16 handle then rounded to bf16); end_to_end reads the checkpoint's weights in float64.

THE BARS are not taken from the GPU.  Each is 3 x the worst error of the clean CPU emulation (emulate: the oracle's own steps in fp32,
every GEMM's products added in the kernels' k-order, the depthwise taps and the tail as fused multiply-adds in the kernels' order, the
squeeze in colstats_kernel's four chains, the pooling's variance in the centred form its kernel sums; for bf16 with rounded weights and
every stored tensor rounded to bf16 — the tail's y BEFORE the next depthwise conv reads it, as titanet.hip says), over every case of
CASES: sizes s / m / l, the edge lengths EDGE_T with three blocks, the ragged pack's lengths, and the checkpoint's own depth at T = 401
from a waveform (mel_emulated: the front-end's sums in its kernel's order).  Beside each bar: the emulation's value, then the GPU's
worst over the whole GPU file."""
import numpy as np
import torch

from oracle import fbank as o_fbank, titanet as ot
from speakerverification_amd import synth
from tests import fbank_emulation
from tests.conformer_oracle_check import KSTEP, frame_errs, gain_err  # noqa: F401
from tests.ecapa_oracle_check import bias_err, local_err, nearer_err, rel_err  # noqa: F401

SEED_W, SEED_X = 1, 20220829
GAINS = (1.0, 3.0, 0.3)                       # the utterances of a case are scaled differently
NOUT = {"s": 192, "m": 320, "l": 512}         # the sizes of tests/golden/titanet.npz
EDGE_T = (7, 8, 9, 15, 16, 17, 31, 33, 255, 256, 257, 401)
RAGGED_T = (1, 2, 3, 5, 6, 8, 16, 17, 257)
BLOCKS = 3                                    # tn_dw then tail + dw; first depthwise conv from the tail, tail + dw; tail without dw
COLSUM_T = 256                                # gemm_pw2_supported: column sums need T >= 256
FRAME_STAGES = ("prolog", "skip", "dw0", "pw0", "dw1", "pw1", "dw2", "pw2", "out", "enc", "att", "logits")
VECTOR_STAGES = ("mean", "gate", "pool_raw", "pool", "emb", "end_to_end")
REDUCTIONS = ("gate", "pool_raw")
FORMS = ("", "/local", "/bias", "/gain")
CHECKS = tuple(s + f for s in FRAME_STAGES for f in FORMS) + VECTOR_STAGES                   # (mean: only where the squeeze kernel ran)

# check: bar,   # emulation, GPU
F32_BARS = {
    "prolog": 1.8e-06,              # 5.9e-07, 7.7e-07
    "prolog/local": 4.1e-05,        # 1.4e-05, 1.4e-05
    "prolog/bias": 1.2e-06,         # 4.2e-07, 5.5e-07
    "prolog/gain": 6.6e-08,         # 2.2e-08, 3.0e-08
    "skip": 4.5e-06,                # 1.5e-06, 1.7e-06
    "skip/local": 7.8e-05,          # 2.6e-05, 3.4e-05
    "skip/bias": 4.2e-06,           # 1.4e-06, 1.2e-06
    "skip/gain": 5.7e-08,           # 1.9e-08, 3.7e-08
    "dw0": 8.6e-07,                 # 2.9e-07, 2.4e-07
    "dw0/local": 1.9e-05,           # 6.2e-06, 6.1e-06
    "dw0/bias": 3.6e-07,            # 1.2e-07, 1.3e-07
    "dw0/gain": 2.0e-08,            # 6.7e-09, 8.6e-09
    "pw0": 4.9e-06,                 # 1.6e-06, 2.0e-06
    "pw0/local": 1.0e-04,           # 3.4e-05, 5.0e-05
    "pw0/bias": 1.9e-05,            # 6.4e-06, 1.5e-05
    "pw0/gain": 1.7e-07,            # 5.5e-08, 5.2e-08
    "dw1": 7.1e-07,                 # 2.4e-07, 2.4e-07
    "dw1/local": 1.4e-05,           # 4.8e-06, 4.7e-06
    "dw1/bias": 3.4e-07,            # 1.1e-07, 1.2e-07
    "dw1/gain": 2.3e-08,            # 7.7e-09, 1.1e-08
    "pw1": 4.7e-06,                 # 1.6e-06, 1.8e-06
    "pw1/local": 9.4e-05,           # 3.1e-05, 6.4e-05
    "pw1/bias": 2.2e-05,            # 7.5e-06, 1.3e-05
    "pw1/gain": 1.6e-07,            # 5.5e-08, 7.2e-08
    "dw2": 7.2e-07,                 # 2.4e-07, 2.3e-07
    "dw2/local": 1.8e-05,           # 6.1e-06, 3.4e-06
    "dw2/bias": 6.0e-07,            # 2.0e-07, 2.4e-07
    "dw2/gain": 3.1e-08,            # 1.0e-08, 8.3e-09
    "pw2": 4.2e-06,                 # 1.4e-06, 1.9e-06
    "pw2/local": 9.1e-05,           # 3.0e-05, 5.9e-05
    "pw2/bias": 2.1e-05,            # 7.0e-06, 1.4e-05
    "pw2/gain": 1.3e-07,            # 4.2e-08, 7.5e-08
    "out": 1.7e-07,                 # 5.8e-08, 5.8e-08
    "out/local": 1.8e-07,           # 5.8e-08, 5.8e-08
    "out/bias": 3.2e-07,            # 1.1e-07, 9.6e-08
    "out/gain": 2.1e-08,            # 7.0e-09, 4.8e-09
    "enc": 4.9e-06,                 # 1.6e-06, 2.0e-06
    "enc/local": 8.3e-05,           # 2.8e-05, 3.0e-05
    "enc/bias": 3.2e-06,            # 1.1e-06, 1.5e-06
    "enc/gain": 6.5e-08,            # 2.2e-08, 2.7e-08
    "att": 1.1e-05,                 # 3.5e-06, 3.4e-06
    "att/local": 3.6e-04,           # 1.2e-04, 1.5e-04
    "att/bias": 5.3e-06,            # 1.8e-06, 1.6e-06
    "att/gain": 2.1e-07,            # 7.0e-08, 5.7e-08
    "logits": 1.7e-06,              # 5.7e-07, 7.3e-07
    "logits/local": 4.2e-05,        # 1.4e-05, 1.5e-05
    "logits/bias": 2.9e-06,         # 9.8e-07, 1.0e-06
    "logits/gain": 1.4e-08,         # 4.7e-09, 1.1e-08
    "mean": 9.5e-07,                # 3.2e-07, 2.5e-07
    "gate": 1.1e-06,                # 3.6e-07, 3.1e-07
    "pool_raw": 1.9e-06,            # 6.5e-07, 1.9e-07
    "pool": 1.6e-07,                # 5.3e-08, 5.0e-08
    "emb": 1.2e-06,                 # 4.0e-07, 2.6e-07
    "end_to_end": 2.1e-06,          # 7.0e-07, 1.1e-06
}
BF16_BARS = {
    "prolog": 1.3e-02,              # 4.4e-03, 4.4e-03
    "prolog/local": 3.3e-01,        # 1.1e-01, 1.1e-01
    "prolog/bias": 1.5e-02,         # 4.9e-03, 4.9e-03
    "prolog/gain": 1.8e-03,         # 5.9e-04, 5.9e-04
    "skip": 1.1e-02,                # 3.7e-03, 3.7e-03
    "skip/local": 1.1e-02,          # 3.8e-03, 3.8e-03
    "skip/bias": 3.8e-02,           # 1.3e-02, 9.5e-03
    "skip/gain": 1.3e-03,           # 4.2e-04, 4.2e-04
    "dw0": 1.2e-02,                 # 3.8e-03, 3.8e-03
    "dw0/local": 1.1e-02,           # 3.8e-03, 3.8e-03
    "dw0/bias": 6.0e-02,            # 2.0e-02, 1.8e-02
    "dw0/gain": 1.5e-03,            # 4.9e-04, 4.9e-04
    "pw0": 1.1e-02,                 # 3.7e-03, 3.8e-03
    "pw0/local": 1.1e-02,           # 3.8e-03, 3.8e-03
    "pw0/bias": 1.5e-02,            # 5.2e-03, 7.1e-03
    "pw0/gain": 1.6e-03,            # 5.4e-04, 5.4e-04
    "dw1": 1.1e-02,                 # 3.6e-03, 3.8e-03
    "dw1/local": 1.1e-02,           # 3.8e-03, 3.8e-03
    "dw1/bias": 8.4e-02,            # 2.8e-02, 2.8e-02
    "dw1/gain": 1.2e-03,            # 4.2e-04, 4.2e-04
    "pw1": 1.1e-02,                 # 3.7e-03, 3.7e-03
    "pw1/local": 1.1e-02,           # 3.8e-03, 3.8e-03
    "pw1/bias": 1.8e-02,            # 6.0e-03, 5.1e-03
    "pw1/gain": 1.9e-03,            # 6.4e-04, 6.4e-04
    "dw2": 1.1e-02,                 # 3.8e-03, 3.8e-03
    "dw2/local": 1.1e-02,           # 3.8e-03, 3.8e-03
    "dw2/bias": 3.6e-02,            # 1.2e-02, 1.2e-02
    "dw2/gain": 2.1e-03,            # 6.9e-04, 6.9e-04
    "pw2": 1.1e-02,                 # 3.8e-03, 3.8e-03
    "pw2/local": 1.1e-02,           # 3.8e-03, 3.8e-03
    "pw2/bias": 2.5e-02,            # 8.2e-03, 6.0e-03
    "pw2/gain": 1.2e-03,            # 4.1e-04, 4.1e-04
    "out": 1.1e-02,                 # 3.8e-03, 3.8e-03
    "out/local": 1.1e-02,           # 3.8e-03, 3.8e-03
    "out/bias": 6.6e-02,            # 2.2e-02, 2.2e-02
    "out/gain": 1.2e-03,            # 4.0e-04, 4.0e-04
    "enc": 1.1e-02,                 # 3.6e-03, 3.6e-03
    "enc/local": 1.1e-02,           # 3.8e-03, 3.8e-03
    "enc/bias": 2.7e-02,            # 8.9e-03, 7.6e-03
    "enc/gain": 3.7e-04,            # 1.2e-04, 1.1e-04
    "att": 7.6e-03,                 # 2.5e-03, 2.5e-03
    "att/local": 1.1e-02,           # 3.8e-03, 3.8e-03
    "att/bias": 5.7e-02,            # 1.9e-02, 1.9e-02
    "att/gain": 9.3e-04,            # 3.1e-04, 3.1e-04
    "logits": 6.8e-07,              # 2.3e-07, 2.8e-07
    "logits/local": 1.2e-05,        # 4.0e-06, 4.8e-06
    "logits/bias": 3.3e-06,         # 1.1e-06, 9.7e-07
    "logits/gain": 1.2e-08,         # 4.1e-09, 3.9e-09
    "mean": 1.7e-07,                # 5.7e-08, 5.7e-08
    "gate": 1.1e-06,                # 3.7e-07, 3.1e-07
    "pool_raw": 2.1e-06,            # 7.1e-07, 2.0e-07
    "pool": 1.7e-07,                # 5.8e-08, 5.9e-08
    "emb": 1.5e-06,                 # 5.0e-07, 3.1e-07
    "end_to_end": 1.5e-02,          # 5.1e-03, 5.6e-03
}


def bars(compute):
    return {"f32": F32_BARS, "bf16": BF16_BARS}[compute]


def checks_of(with_mean):
    """the checks one utterance must show: every one of CHECKS, mean exactly where the squeeze kernel ran"""
    return set(CHECKS) - ({"mean"} if not with_mean else set())


def samples_of(T):
    """a sample count that gives T mel frames (hop 80), at least the 512 samples of one FFT window"""
    return max(512, 80 * (T - 1))


def waveforms(B, L):
    """the inputs of a case: synth's waveforms, utterance b scaled by GAINS[b % 3]"""
    x = synth.synth_waveforms(B, L, seed=SEED_X + L)
    return np.ascontiguousarray(x * np.asarray([GAINS[b % 3] for b in range(B)], np.float32)[:, None])


def mel_of(wave, dtype=torch.float64):
    """(L,) samples -> (80, T) mel power"""
    return o_fbank.melspectrogram(torch.as_tensor(wave).to(dtype)[None])[0]


def mel_emulated(wave, compute):
    """(L,) samples -> (80, T) mel power in fp32 as the handle's front-end adds it up (fbank.hip) at the default geometry: the DFT's
    products added KSTEP[compute] at a time (tests/fbank_emulation.py states the sums and takes any geometry)"""
    return fbank_emulation.mel_emulated(wave, kstep=KSTEP[compute])


_FEATS = {}


def features(B, T):
    """(B, 80, T) float32 mel power: the oracle's front-end on waveforms(B, samples_of(T)), its first T frames (T < 7: cut short); cached,
    never written to"""
    if (B, T) not in _FEATS:
        _FEATS[B, T] = np.stack([mel_of(w, torch.float32).numpy()[:, :T] for w in waveforms(B, samples_of(T))])
        _FEATS[B, T].setflags(write=False)
    return _FEATS[B, T]


def ragged_features():
    """the pack's utterances: utterance u is features(u + 1, T_u)[u], so that every one has its own content and gain"""
    return [np.ascontiguousarray(features(u + 1, T)[u]) for u, T in enumerate(RAGGED_T)]


def state_dict(size, blocks=None):
    """the synthetic checkpoint of tests/golden/titanet.npz (numpy); blocks: its first n mega-blocks only"""
    sd = synth.synth_state_dict(synth.titanet_param_spec(size, NOUT[size]), seed=SEED_W)
    if blocks is None:
        return sd
    return {k: v for k, v in sd.items() if not k.startswith("encoder.mega_blocks.") or int(k.split(".")[2]) < blocks}


_W = {}


def weights(size, blocks=None, eps=1e-5):
    """{"sd": numpy checkpoint, "full": float64 tensors, "f32" / "bf16": (what an emulation reads in fp32, what a handle of that compute
    reads as float64 reference)}; eps: of the BatchNorm fold (a fault of the host test)"""
    key = (size, blocks, eps)
    if key not in _W:
        sd = state_dict(size, blocks)
        full = ot.to_torch_sd(sd)
        if eps != 1e-5:
            folded = lambda k: k.endswith("running_var") and ("conv_block.1." in k or "skip_connection.1." in k)
            full = {k: (v - 1e-5 + eps if folded(k) else v) for k, v in full.items()}          # (var + eps is all the fold reads)
        _W[key] = {"sd": sd, "full": full}
        for compute in ("f32", "bf16"):
            ref = ot.folded_sd(full, bf16=compute == "bf16")
            _W[key][compute] = (ot.to_torch_sd(ref, torch.float32), ref)
    return _W[key]


def emulate(mel, sd32, compute, squeeze_acc=False):
    """the stages of a handle on the CPU for one utterance: ({stage: float64 array}, the embedding).  mel (80, T) and sd32 in float32
    (the folded weights of the handle: weights()[compute][0]); squeeze_acc: a bf16 handle's fixed-length forward at T >= COLSUM_T"""
    q = ot.bf16_round if compute == "bf16" else ot.ident
    st = {}
    with torch.no_grad(), ot.matmul_as(ot.chained_matmul(KSTEP[compute])):
        emb = ot.forward(mel, sd32, store=q, squeeze_acc=squeeze_acc, kernel_sums=True, stages=st)
    return {k: v.double().numpy() for k, v in st.items()}, emb.double().numpy()


def from_partials(compute, kind, T):
    """the SE squeeze comes from the third pointwise GEMM's column sums: bf16, fixed-length, T >= COLSUM_T (then no mean vector exists)"""
    return compute == "bf16" and kind != "ragged" and T >= COLSUM_T


# (kind, size, T): "edge": B = 3 of features at T, BLOCKS blocks; "ragged": the pack (T ignored), BLOCKS blocks; "full": B = 3 waveforms
# at T = 401, the checkpoint's own depth
CASES = tuple(("edge", s, T) for s in "sml" for T in EDGE_T) + tuple(("ragged", s, 0) for s in "sml") + tuple(("full", s, 401) for s in "sml")

_EMU = {}


def emulated_case(compute, case):
    """the clean emulation of a case, cached: [(stages, embedding, layer_local's errors)] per utterance"""
    if (compute, case) not in _EMU:
        kind, size, T = case
        w = weights(size, None if kind == "full" else BLOCKS)
        sd32, sdref = w[compute]
        out = []
        if kind == "full":
            inputs = [(mel_emulated(x, compute), mel_of(x), True) for x in waveforms(3, samples_of(T))]
        else:
            feats = ragged_features() if kind == "ragged" else features(3, T)
            inputs = [(torch.tensor(f), torch.tensor(f).double(), False) for f in feats]
        for m32, m64, wave in inputs:
            acc = from_partials(compute, kind, m32.shape[1])
            S, emb = emulate(m32, sd32, compute, acc)
            if acc:
                S = {k: v for k, v in S.items() if not k.endswith("_mean")}
            with torch.no_grad():
                e2e = ot.forward(m64, w["full"]).numpy()
            out.append((S, emb, layer_local(S, sdref, mel=m64, emb=emb, e2e_ref=e2e)))
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


def gate_err(got, pw2_stored, pw2_exact, sd, i):
    """block i's gate against the nearer of its two references, element by element (module docstring): the SE MLP of the squeeze of the
    stored pw2, and of the oracle's unrounded pw2 of the stored dw2"""
    with torch.no_grad():
        a, b = (ot.gate(ot.squeeze(h), sd, i).numpy() for h in (pw2_stored, pw2_exact))
    return nearer_err(got, a, b)


def layer_local(S, sd, mel=None, emb=None, e2e_ref=None):
    """{check: (error, worst index)} of one utterance.  S: the handle's stages of the utterance as float64 arrays — prolog, b<i>_<step>
    (oracle.titanet.BLOCK_STEPS), b<i>_mean where the squeeze kernel ran, enc, att, logits, pool_raw, pool.  sd: the float64 weights
    the handle reads.  mel: the reference's mel power (80, T);
    emb / e2e_ref: the handle's embedding and the oracle's end to end.  A block check's index is (block, frame, channel)."""
    err = {}

    def worse(name, e, idx):
        if name not in err or e > err[name][0] or e != e:
            err[name] = (e, idx)

    def frame(name, got, ref, blk=None):
        for form, (e, idx) in frame_errs(got, ref.numpy()).items():
            worse(name + form, e, idx if blk is None else (blk,) + idx)

    def vector(name, got, ref, blk=None):
        e, idx = rel_err(got, ref.numpy())
        worse(name, e, idx if blk is None else (blk,) + idx)

    with torch.no_grad():
        if mel is not None:
            frame("prolog", S["prolog"], ot.prolog(mel, sd))
        x = _t(S["prolog"])
        for i in range(ot.n_blocks(sd)):
            g = {k: _t(S[f"b{i}_{k}"]) for k in ot.BLOCK_STEPS}
            frame("skip", S[f"b{i}_skip"], ot.skip(x, sd, i), i)
            frame("dw0", S[f"b{i}_dw0"], ot.dw(x, sd, i, 0), i)
            for j in range(3):
                if j:
                    frame(f"dw{j}", S[f"b{i}_dw{j}"], ot.dw(g[f"pw{j - 1}"], sd, i, j), i)
                acc = ot.pw(g[f"dw{j}"], sd, i, j)
                frame(f"pw{j}", S[f"b{i}_pw{j}"], acc, i)
            m = ot.squeeze(g["pw2"])
            if f"b{i}_mean" in S:
                vector("mean", S[f"b{i}_mean"], m, i)
            e, idx = gate_err(S[f"b{i}_gate"], g["pw2"], acc, sd, i)
            worse("gate", e, (i,) + idx)
            frame("out", S[f"b{i}_out"], ot.out(g["skip"], g["pw2"], g["gate"]), i)
            x = g["out"]
        enc, a, lg = _t(S["enc"]), _t(S["att"]), _t(S["logits"])
        frame("enc", S["enc"], ot.epilog(x, sd))
        frame("att", S["att"], ot.att(enc, sd))
        frame("logits", S["logits"], ot.logits(a, sd))
        vector("pool_raw", S["pool_raw"], ot.pool_stats(lg, enc))
        vector("pool", S["pool"], ot.pool_norm(_t(S["pool_raw"]), sd))
        if emb is not None:
            vector("emb", emb, ot.fc(_t(S["pool"]), sd))
    if emb is not None and e2e_ref is not None:
        err["end_to_end"] = rel_err(emb, e2e_ref)
    return err


def where(check, idx):
    """the worst element of a check in words"""
    if check in VECTOR_STAGES:
        return (f"block {idx[0]} " if len(idx) == 2 else "") + f"channel {idx[-1]}"
    blk = f"block {idx[0]} " if len(idx) == 3 else ""
    if check.endswith("/gain"):
        return blk + "(whole tensor)"
    return blk + (f"channel {idx[-1]}" if check.endswith("/bias") else f"frame {idx[-2]} channel {idx[-1]}")


def failures(err, compute):
    """the checks over their bars: [(check, error, bar, where the worst element sits)]"""
    bar = bars(compute)
    return [(n, e, bar[n], where(n, i)) for n, (e, i) in err.items() if not e <= bar[n]]


def describe(err):
    """one line: every check's error in stage order"""
    return ", ".join(f"{n} {err[n][0]:.2e}" for n in CHECKS if n in err)
