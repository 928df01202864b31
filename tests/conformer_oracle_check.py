"""The Conformer's stages against the float64 oracle (oracle/conformer.py), one utterance at a time: the comparisons and bars of
tests/test_gpu_conformer_oracle.py.  They need no GPU, so tests/test_conformer_oracle_host.py runs them on a CPU emulation of a
handle, takes the bars from it and shows that every bar fails when the kernel it guards is subtly wrong.

Layer-local checks.  Option cf_keep makes a forward copy what it stores anyway; each stored tensor is compared with the oracle's step
applied in float64 to the handle's OWN stored input of that step:

    cf_in      from the oracle's own features of the utterance (front-end, both convolutions, input projection)
    per block  ff1 from the block's input, qkv from ff1 (GEMM), ctx from qkv (cf_attn), att from ff1 (the MHSA module), pw1 from att
               (GEMM), dw from pw1 (cf_glu_dw), conv from att (the convolution module), ff2 from conv, out from ff2 (cf_ln)
    logits     from cf_last;  pool_raw from cf_last and the handle's logits;  pool from pool_raw;  emb from pool
    end_to_end the embedding against the oracle on full-precision weights

The module-level checks (att, conv) look at a step's output through everything between its input and itself, the kernel-level ones
(ctx, dw) and the GEMM ones (qkv, pw1) at one launch.  The error of a check is taken over ONE utterance; a frame tensor (T', channels)
has four forms — `name` (max |diff| / max |ref|), `name/local` (each element against its own size), `name/bias` (an error common to
every frame of a channel) and `name/gain` (the regression slope of got on ref, minus one: a common factor, as a LayerNorm variance
over 255 instead of 256 channels gives, that hides under the rounding of the single elements).  A block check's value is the worst
over the six blocks; the failure names block, frame and channel.  (rel_err, local_err and bias_err are tests/ecapa_oracle_check.py's;
its nearer_err has no use here: the pooling reads the stored cf_last and logits only, never a GEMM epilogue's unrounded values.)

A bf16 handle reads bf16 GEMM weights (oracle.conformer.rounded_sd) and the layer-local references read the same rounded weights and
P in fp32; what remains is the rounding of the stored activations and the kernels' fp32 sums.  end_to_end reads the full weights.

THE BARS are not taken from the GPU.  Each is 3 x the worst error of the clean CPU emulation (emulate: the oracle's own steps in fp32,
for bf16 with rounded weights, every stored tensor rounded to bf16 and cf_attn's staged operands — q + u, q + v, k, v, P and the
softmax weights — rounded as conformer.hip says), over every length, utterance and block tests/test_gpu_conformer_oracle.py's edge
cases run (LENGTHS).  The emulation adds every GEMM's products as the MFMA kernels do, in one fp32 accumulator along k (KSTEP): with
torch's blocked CPU sums the first version of it sat 3 - 4 x below the f32 handle at the long sums (K = 4864 and 2304 in front of
cf_in, K = 1024 in ff2) and at the handle's level at K = 256 — the growth with sqrt(K) of a chain of fp32 additions.  The factor 3
covers what is left: the order inside one MFMA, expf / logf against torch's, the attention's online softmax.  Beside each
bar: the emulation's value, then the GPU's worst over the whole GPU file.  tests/test_conformer_oracle_host.py asserts that the
emulation's values are these, that every bar is at most half the effect of each fault it guards, and that the reduction's bar
(pool_raw) sits at least 4 x below one dropped frame."""
import numpy as np
import torch

from oracle import conformer as oc, fbank as o_fbank
from speakerverification_amd import synth
from tests.ecapa_oracle_check import bias_err, local_err, rel_err

SEED_W, SEED_X = 1, 20220829
GAINS = (1.0, 3.0, 0.3)                       # the utterances of a case are scaled differently
EDGE_TP = (1, 2, 7, 8, 15, 16, 17, 33, 63, 64, 65, 99, 129, 499)
FRAME_STAGES = ("cf_in",) + oc.BLOCK_STEPS + ("logits",)
VECTOR_STAGES = ("pool_raw", "pool", "emb", "end_to_end")
REDUCTIONS = ("pool_raw",)
FORMS = ("", "/local", "/bias", "/gain")
CHECKS = tuple(s + f for s in FRAME_STAGES for f in FORMS) + VECTOR_STAGES


def samples_of(Tp, extra=0):
    """the sample count that gives T = 4 T' + 3 + extra mel frames (hop 80; at least the 512 samples of one FFT window)"""
    return max(512, 80 * (4 * Tp + 2 + extra))


LENGTHS = tuple(samples_of(t) for t in EDGE_TP) + (samples_of(16, 3), samples_of(64, 3))       # ... and T1 even, trailing frames dropped

# check: bar,   # emulation, GPU
F32_BARS = {
    "cf_in": 5.7e-06,           # 1.9e-06, 2.8e-06
    "cf_in/local": 1.4e-04,     # 4.5e-05, 5.7e-05
    "cf_in/bias": 4.5e-06,      # 1.5e-06, 2.4e-06
    "cf_in/gain": 3.3e-07,      # 1.1e-07, 1.3e-07
    "ff1": 2.8e-06,             # 9.3e-07, 1.7e-06
    "ff1/local": 9.0e-05,       # 3.0e-05, 4.5e-05
    "ff1/bias": 2.9e-06,        # 9.5e-07, 1.2e-06
    "ff1/gain": 2.5e-07,        # 8.1e-08, 7.2e-08
    "qkv": 2.2e-06,             # 7.3e-07, 1.1e-06
    "qkv/local": 4.2e-05,       # 1.4e-05, 2.4e-05
    "qkv/bias": 2.2e-06,        # 7.2e-07, 9.1e-07
    "qkv/gain": 2.8e-07,        # 9.1e-08, 1.1e-07
    "ctx": 2.2e-06,             # 7.3e-07, 1.5e-06
    "ctx/local": 2.2e-05,       # 7.1e-06, 5.3e-06
    "ctx/bias": 1.5e-06,        # 5.0e-07, 8.1e-07
    "ctx/gain": 5.7e-08,        # 1.9e-08, 4.2e-08
    "att": 2.2e-06,             # 7.1e-07, 1.1e-06
    "att/local": 6.3e-05,       # 2.1e-05, 3.5e-05
    "att/bias": 3.0e-06,        # 1.0e-06, 1.1e-06
    "att/gain": 2.0e-07,        # 6.6e-08, 9.7e-08
    "pw1": 2.6e-06,             # 8.5e-07, 1.2e-06
    "pw1/local": 5.4e-05,       # 1.8e-05, 2.6e-05
    "pw1/bias": 3.6e-06,        # 1.2e-06, 1.3e-06
    "pw1/gain": 2.6e-07,        # 8.5e-08, 1.1e-07
    "dw": 1.1e-06,              # 3.5e-07, 3.3e-07
    "dw/local": 1.4e-05,        # 4.4e-06, 5.2e-06
    "dw/bias": 5.4e-06,         # 1.8e-06, 9.7e-07
    "dw/gain": 3.6e-07,         # 1.2e-07, 4.4e-08
    "conv": 1.2e-06,            # 4.0e-07, 5.2e-07
    "conv/local": 4.8e-05,      # 1.6e-05, 1.9e-05
    "conv/bias": 2.7e-06,       # 9.0e-07, 5.5e-07
    "conv/gain": 4.2e-08,       # 1.4e-08, 1.8e-08
    "ff2": 1.3e-06,             # 4.1e-07, 7.8e-07
    "ff2/local": 4.5e-05,       # 1.5e-05, 2.2e-05
    "ff2/bias": 1.2e-06,        # 3.8e-07, 4.4e-07
    "ff2/gain": 6.0e-08,        # 2.0e-08, 2.5e-08
    "out": 6.6e-07,             # 2.2e-07, 2.3e-07
    "out/local": 3.0e-06,       # 9.9e-07, 7.4e-07
    "out/bias": 1.8e-06,        # 5.7e-07, 5.9e-07
    "out/gain": 2.2e-07,        # 7.3e-08, 7.9e-08
    "logits": 2.1e-06,          # 7.0e-07, 7.4e-07
    "logits/local": 6.3e-05,    # 2.1e-05, 2.5e-05
    "logits/bias": 1.2e-05,     # 3.7e-06, 5.2e-06
    "logits/gain": 3.0e-07,     # 1.0e-07, 1.1e-07
    "pool_raw": 7.8e-05,        # 2.6e-05, 1.7e-07
    "pool": 3.3e-07,            # 1.1e-07, 8.0e-08
    "emb": 9.3e-07,             # 3.1e-07, 1.5e-07
    "end_to_end": 2.5e-05,      # 8.1e-06, 1.8e-06
}
BF16_BARS = {
    "cf_in": 1.4e-02,           # 4.5e-03, 4.5e-03
    "cf_in/local": 4.8e-01,     # 1.6e-01, 1.6e-01
    "cf_in/bias": 1.3e-02,      # 4.1e-03, 3.8e-03
    "cf_in/gain": 1.4e-03,      # 4.6e-04, 5.6e-04
    "ff1": 1.5e-02,             # 4.7e-03, 5.0e-03
    "ff1/local": 3.0e-01,       # 1.0e-01, 1.2e-01
    "ff1/bias": 1.7e-02,        # 5.4e-03, 6.4e-03
    "ff1/gain": 1.4e-03,        # 4.4e-04, 3.0e-04
    "qkv": 1.4e-02,             # 4.5e-03, 4.5e-03
    "qkv/local": 3.6e-01,       # 1.2e-01, 1.2e-01
    "qkv/bias": 1.5e-02,        # 5.0e-03, 5.7e-03
    "qkv/gain": 1.5e-03,        # 4.7e-04, 5.1e-04
    "ctx": 1.4e-02,             # 4.6e-03, 4.4e-03
    "ctx/local": 1.7e-01,       # 5.5e-02, 6.6e-02
    "ctx/bias": 9.6e-02,        # 3.2e-02, 4.8e-02
    "ctx/gain": 2.1e-03,        # 6.8e-04, 4.3e-04
    "att": 1.4e-02,             # 4.5e-03, 5.8e-03
    "att/local": 4.2e-01,       # 1.4e-01, 1.3e-01
    "att/bias": 5.1e-02,        # 1.7e-02, 2.9e-02
    "att/gain": 2.0e-03,        # 6.6e-04, 6.9e-04
    "pw1": 1.6e-02,             # 5.2e-03, 5.0e-03
    "pw1/local": 4.5e-01,       # 1.5e-01, 1.4e-01
    "pw1/bias": 2.0e-02,        # 6.6e-03, 6.3e-03
    "pw1/gain": 9.6e-04,        # 3.2e-04, 8.0e-04
    "dw": 1.2e-02,              # 3.7e-03, 3.7e-03
    "dw/local": 1.2e-02,        # 3.8e-03, 3.8e-03
    "dw/bias": 1.4e-02,         # 4.5e-03, 5.1e-03
    "dw/gain": 2.7e-03,         # 9.0e-04, 1.2e-03
    "conv": 1.4e-02,            # 4.5e-03, 4.8e-03
    "conv/local": 3.3e-01,      # 1.1e-01, 1.3e-01
    "conv/bias": 1.5e-02,       # 4.7e-03, 4.9e-03
    "conv/gain": 1.1e-03,       # 3.5e-04, 3.6e-04
    "ff2": 1.3e-02,             # 4.1e-03, 4.2e-03
    "ff2/local": 1.7e-01,       # 5.4e-02, 6.4e-02
    "ff2/bias": 2.0e-02,        # 6.6e-03, 6.6e-03
    "ff2/gain": 1.1e-03,        # 3.5e-04, 5.1e-04
    "out": 1.2e-02,             # 3.8e-03, 3.9e-03
    "out/local": 1.2e-02,       # 3.8e-03, 3.8e-03
    "out/bias": 4.2e-02,        # 1.4e-02, 1.4e-02
    "out/gain": 9.6e-04,        # 3.2e-04, 5.3e-04
    "logits": 8.1e-03,          # 2.7e-03, 3.0e-03
    "logits/local": 3.6e-01,    # 1.2e-01, 1.5e-01
    "logits/bias": 1.2e-02,     # 3.7e-03, 4.6e-03
    "logits/gain": 2.0e-03,     # 6.4e-04, 5.2e-04
    "pool_raw": 7.8e-05,        # 2.6e-05, 2.8e-07
    "pool": 3.3e-07,            # 1.1e-07, 7.8e-08
    "emb": 7.8e-07,             # 2.6e-07, 1.4e-07
    "end_to_end": 5.1e-02,      # 1.7e-02, 1.5e-02
}


def bars(compute):
    return {"f32": F32_BARS, "bf16": BF16_BARS}[compute]


def waveforms(B, L):
    """the inputs of a case: synth's waveforms, utterance b scaled by GAINS[b % 3]"""
    x = synth.synth_waveforms(B, L, seed=SEED_X + L)
    return np.ascontiguousarray(x * np.asarray([GAINS[b % 3] for b in range(B)], np.float32)[:, None])


def weights(dtype=torch.float64, nOut=512):
    """the synthetic state dict (numpy) and the same as torch tensors"""
    sd = synth.synth_state_dict(synth.conformer_param_spec(nOut, 80), seed=SEED_W)
    return sd, oc.to_torch_sd(sd, dtype)


def mel_of(wave, dtype=torch.float64):
    """(L,) samples -> (80, T) mel power"""
    return o_fbank.melspectrogram(torch.as_tensor(wave).to(dtype)[None])[0]


def gain_err(got, ref):
    """(|sum got ref / sum ref^2 - 1|, (0, 0)) of a (T, channels) stage"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return abs(float((got * ref).sum()) / max(float((ref * ref).sum()), 1e-300) - 1.0), (0, 0)


def frame_errs(got, ref):
    """{form: (error, worst index)} of one (T, channels) tensor"""
    return {"": rel_err(got, ref), "/local": local_err(got, ref), "/bias": bias_err(got, ref), "/gain": gain_err(got, ref)}


KSTEP = {"f32": 2, "bf16": 16}             # products per MFMA of the GEMM kernels: v_mfma_f32_32x32x2f32, v_mfma_f32_32x32x16_bf16


def emulate(mel, sd32, compute):
    """the stages of a handle on the CPU for one utterance: ({stage: float64 array}, the embedding).  mel (80, T) and sd32 in
    float32 (for bf16: oracle.conformer.rounded_sd of it); the oracle's steps in fp32 with every GEMM's products added in the
    kernels' order (oracle.conformer.chained_matmul), on a bf16 handle with every stored tensor and the attention's staged operands
    rounded to bf16"""
    q = oc.bf16_round if compute == "bf16" else oc.ident
    st = {}
    with torch.no_grad(), oc.matmul_as(oc.chained_matmul(KSTEP[compute])):
        emb = oc.forward(mel, sd32, store=q, stage=q, f32_P=True, stages=st)
    return {k: v.double().numpy() for k, v in st.items()}, emb.double().numpy()


_EMU = {}


def emulated_case(compute, L, B=3):
    """the clean emulation of a B-utterance case of L samples, cached: [(stages, embedding, layer_local's errors)] per utterance"""
    if (compute, L, B) not in _EMU:
        if "sd" not in _EMU:
            _, sd64 = weights()
            sd32 = oc.to_torch_sd(sd64, torch.float32)
            _EMU["sd"] = {"f32": (sd32, sd64), "bf16": (oc.rounded_sd(sd32), oc.rounded_sd(sd64)), "full": sd64}
        sd32, sdref = _EMU["sd"][compute]
        out = []
        for w in waveforms(B, L):
            S, emb = emulate(mel_of(w, torch.float32), sd32, compute)
            with torch.no_grad():
                m64 = mel_of(w)
                e2e = oc.forward(m64, _EMU["sd"]["full"]).numpy()
                feat = oc.features(m64, sdref)
            out.append((S, emb, layer_local(S, sdref, ref_input=feat, emb=emb, e2e_ref=e2e)))
        _EMU[(compute, L, B)] = out
    return _EMU[(compute, L, B)]


def emulation_worst(compute):
    """{check: the clean emulation's worst error over LENGTHS and the three utterances of each}"""
    worst = {}
    for L in LENGTHS:
        for _, _, err in emulated_case(compute, L):
            for n, (e, _) in err.items():
                worst[n] = max(worst.get(n, 0.0), e)
    return worst


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def layer_local(S, sd, ref_input=None, emb=None, e2e_ref=None):
    """{check: (error, worst index)} of one utterance.  S: the handle's stages of the utterance as float64 arrays — cf_in, b<i>_<step>
    (oracle.conformer.BLOCK_STEPS), logits, pool_raw, pool.  sd: the float64 weights the handle reads.  ref_input: the oracle's
    features (T, 80); emb / e2e_ref: the handle's embedding and the oracle's end to end.  A block check's index is (block, frame,
    channel)."""
    err = {}

    def frame(name, got, ref, blk=None):
        for form, (e, idx) in frame_errs(got, ref.numpy() if torch.is_tensor(ref) else ref).items():
            if blk is not None:
                idx = (blk,) + idx
            if name + form not in err or e > err[name + form][0]:
                err[name + form] = (e, idx)

    with torch.no_grad():
        if ref_input is not None:
            frame("cf_in", S["cf_in"], oc.subsample(ref_input, sd))
        x = _t(S["cf_in"])
        for i in range(oc.LAYERS):
            if f"b{i}_ff1" not in S:
                break
            g = {k: _t(S[f"b{i}_{k}"]) for k in oc.BLOCK_STEPS}
            P = oc.pos_table(sd, i, x.shape[0], f32=True)
            frame("ff1", S[f"b{i}_ff1"], oc.ff_half(x, sd, i, 0), i)
            frame("qkv", S[f"b{i}_qkv"], oc.qkv(g["ff1"], sd, i), i)
            frame("ctx", S[f"b{i}_ctx"], oc.attn_context(g["qkv"], P, sd, i), i)
            frame("att", S[f"b{i}_att"], oc.mhsa(g["ff1"], sd, i, f32_P=True), i)
            frame("pw1", S[f"b{i}_pw1"], oc.pw1(g["att"], sd, i), i)
            frame("dw", S[f"b{i}_dw"], oc.glu_dw(g["pw1"], sd, i), i)
            frame("conv", S[f"b{i}_conv"], oc.conv_module(g["att"], sd, i), i)
            frame("ff2", S[f"b{i}_ff2"], oc.ff_half(g["conv"], sd, i, 1), i)
            frame("out", S[f"b{i}_out"], oc.final_ln(g["ff2"], sd, i), i)
            x = g["out"]
        if "logits" in S:
            frame("logits", S["logits"], oc.pool_logits(x, sd))
            err["pool_raw"] = rel_err(S["pool_raw"], oc.pool_stats(_t(S["logits"]), x).numpy())
            err["pool"] = rel_err(S["pool"], oc.pool_norm(_t(S["pool_raw"]), sd).numpy())
            if emb is not None:
                err["emb"] = rel_err(emb, oc.fc(_t(S["pool"]), sd).numpy())
    if emb is not None and e2e_ref is not None:
        err["end_to_end"] = rel_err(emb, e2e_ref)
    return err


def where(check, idx):
    """the worst element of a check in words"""
    if check in VECTOR_STAGES:
        return f"channel {idx[0]}"
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
