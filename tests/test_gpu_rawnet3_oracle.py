"""GPU: RawNet3 against the float64 oracle (oracle/rawnet3.py), stage by stage, at the batches that put each GEMM on each of its
kernels.

Layer-local checks.  Every stage the handle exposes (svhip_get_stage) is fed to the oracle's NEXT block in float64 and compared
element by element with the handle's own next stage: the front-end from the waveform, layer1 .. layer3 (layer3 on mp3(x1) + x2 of
the handle's own x1 and x2), layer4 on the three stage outputs, the context pooling + bn5 (rn3_pooled) on layer4, fc6 on rn3_pooled,
and the embeddings end to end from the waveform.  The error of a stage is max |diff| / max |ref| over ONE utterance, so one wrong
row, frame or 256-row tile fails the test.

Bars: the largest value measured over every case of this file, with a margin (F32_BARS, BF16_BARS; the measured values beside
them).  The bf16 front-end is the loosest: its filterbank sums run in fp32, and log(|y| + 1e-6) turns their rounding into large errors
at the few outputs that sit near a zero crossing.

The batches are derived from the device's CU count: the 1 x 1 GEMMs of layer1 / layer2 (pw3-able: bias + BN + ReLU epilogue) take
the persistent gemm_pw3 as column halves while 2 tiles <= CUs, gemm_pw2 up to one tile per CU and the whole-tile gemm_pw3 beyond;
layer4 (no BN) and the residual-carrying conv3 take the narrow gemm_pw or gemm_pw2 (gemm_route, gemm.hip).  The route census
checks that the cases exercised every kernel RawNet3 reaches."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import rawnet3 as o_rn3
from speakerverification_amd import _lib, synth
from speakerverification_amd.engine import Engine

pytestmark = pytest.mark.gpu

SEED_W, SEED_X = 1, 20220829
STAGES = ("rn3_front", "rn3_layer1", "rn3_layer2", "rn3_layer3", "rn3_layer4", "rn3_pooled", "fc6", "end_to_end")
F32_BARS = {"rn3_front": 1e-6,          # 1.5e-7
            "rn3_layer1": 5e-6,         # 9.2e-7
            "rn3_layer2": 5e-6,         # 1.4e-6
            "rn3_layer3": 5e-6,         # 2.0e-6
            "rn3_layer4": 1e-5,         # 2.3e-6
            "rn3_pooled": 1e-5,         # 8.5e-6 at L = 541 (T2 = 2), 3.1e-6 at 700, <= 1.3e-6 beyond (1.4e-5 before rn3_pool summed in fp64)
            "fc6": 1e-6,                # 2.1e-7
            "end_to_end": 1e-5}         # 3.8e-6 (1.8e-6 with rn3_pool in fp64)
BF16_BARS = {"rn3_front": 6e-2,         # 4.0e-2
             "rn3_layer1": 1.2e-2,      # 8.0e-3
             "rn3_layer2": 1.2e-2,      # 8.0e-3
             "rn3_layer3": 1.5e-2,      # 9.9e-3
             "rn3_layer4": 6e-3,        # 3.7e-3
             "rn3_pooled": 3e-3,        # 1.6e-3
             "fc6": 1e-6,               # 2.1e-7
             "end_to_end": 8e-3}        # 5.7e-3 (test_gpu_rawnet3.py's end-to-end bf16 bar: 3e-2)
# every GEMM kernel a RawNet3 forward reaches (conv_plan's labels): the 1 x 1 convolutions on the persistent 256 x 256 kernel, the
# per-tile 256 x 256 kernel and the narrow gemm_pw (also the attention GEMM with its per-utterance bias), the Res2Net step 0 on
# gemm_pw's conv-gather form, the steps i > 0 (A + A2) on the generic conv kernel
CENSUS_WANT = {"bf16": {"gemm_pw3", "gemm_pw2", "gemm_pw", "gemm_conv", "gemm_conv_add"},
               "f32": {"gemm_pw", "gemm_conv", "gemm_conv_add"}}
LENGTH_CASES = ((541, 3), (700, 3), (24001, 3), (48000, 2))      # T0 = 30, 45 (< one / not a multiple of the 32-frame sinc tile),
#                                                                  2376 (T0 % 5, T1 % 3 != 0), 4775;  T2 = 2 (the minimum), 3, 158, 318

_SD = {}
_E2E = {}
_CENSUS = {"bf16": {}, "f32": {}}


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sd_np():
    if "np" not in _SD:
        _SD["np"] = synth.synth_state_dict(synth.rawnet3_param_spec(nOut=320), seed=SEED_W)
        _SD["t64"] = o_rn3.torch_sd(_SD["np"])
    return _SD["np"]


def _sd64():
    _sd_np()
    return _SD["t64"]


def _regime(M, N, num_cu, pw3_able):
    """gemm_route (gemm.hip) of a bf16 1 x 1 GEMM at the default options (grid cap = CUs, tail split on)"""
    tiles = -(-M // 256) * (N // 256)
    if pw3_able:
        return "gemm_pw3" if tiles > num_cu else ("gemm_pw3/halves" if 2 * tiles <= num_cu else "gemm_pw2")
    return "gemm_pw" if 2 * tiles <= num_cu else "gemm_pw2"


def _gemms(L):
    """(name, rows per utterance, N, K, pw3-able) of the 1 x 1 GEMM of each layer whose route moves with the batch"""
    T0, T1, T2 = o_rn3.frames(L)
    return (("layer1.conv1", T0, 1024, 256, True), ("layer2.conv1", T1, 1024, 1024, True), ("layer4", T2, 1536, 3072, False))


def _route_batches(L, num_cu, b_max=64):
    """the smallest batch at which each of those GEMMs reaches each of its kernels"""
    picks = {}
    for name, T, N, _, pw3 in _gemms(L):
        for B in range(1, b_max + 1):
            picks.setdefault((name, _regime(B * T, N, num_cu, pw3)), B)
    return picks


def _route_cases():
    return sorted(set(_route_batches(32000, _num_cu()).values()))


def _rows(B, L):
    """every row for B <= 3; else the first, the last and the utterance over the middle 256-row tile boundary of layer2"""
    if B <= 3:
        return list(range(B))
    T1 = o_rn3.frames(L)[1]
    mid = min(B - 2, max(1, (256 * ((B * T1 // 2) // 256)) // T1))
    return sorted({0, mid, B - 1})


def _engine(compute, B, L, **kw):
    e = Engine(model="rawnet3", compute=compute, embed_dim=320, channels=1024, max_batch=B, samples=L, **kw)
    e.load_state_dict(_sd_np())
    e.finalize()
    return e


def _stages(e, B, L):
    T0, T1, T2 = o_rn3.frames(L)
    shapes = {"rn3_front": (B, T0, 256), "rn3_layer1": (B, T1, 1024), "rn3_layer2": (B, T2, 1024), "rn3_layer3": (B, T2, 1024),
              "rn3_layer4": (B, T2, 1536), "rn3_pooled": (B, 3072)}
    return {n: e.get_stage(n).astype(np.float64).reshape(s) for n, s in shapes.items()}


def _oracle_e2e(x_row):
    key = hashlib.sha1(x_row.tobytes()).hexdigest()
    if key not in _E2E:
        with torch.no_grad():
            _E2E[key] = o_rn3.rawnet3_forward(torch.from_numpy(x_row).double()[None], _sd64())[0].numpy()
    return _E2E[key]


def _rel(got, ref):
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def _layer_local(S, emb, x, b):
    """{stage: max |diff| / max |ref|} of utterance b: each stage against the oracle's block on the handle's previous stage"""
    sd = _sd64()
    cm = lambda a: torch.from_numpy(np.ascontiguousarray(a[b].T))[None]        # frame-major row b -> (1, C, T)
    fm = lambda t: o_rn3.frame_major(t)[0].numpy()
    err = {}
    with torch.no_grad():
        err["rn3_front"] = _rel(S["rn3_front"][b], fm(o_rn3.front(torch.from_numpy(x[b]).double()[None], sd)))
        err["rn3_layer1"] = _rel(S["rn3_layer1"][b], fm(o_rn3.bottle2neck(cm(S["rn3_front"]), sd, 1)))
        err["rn3_layer2"] = _rel(S["rn3_layer2"][b], fm(o_rn3.bottle2neck(cm(S["rn3_layer1"]), sd, 2)))
        x3_in = o_rn3.layer3_input(cm(S["rn3_layer1"]), cm(S["rn3_layer2"]))
        err["rn3_layer3"] = _rel(S["rn3_layer3"][b], fm(o_rn3.bottle2neck(x3_in, sd, 3)))
        err["rn3_layer4"] = _rel(S["rn3_layer4"][b], fm(o_rn3.head(cm(S["rn3_layer1"]), cm(S["rn3_layer2"]), cm(S["rn3_layer3"]), sd)))
        err["rn3_pooled"] = _rel(S["rn3_pooled"][b], o_rn3.context_pool(cm(S["rn3_layer4"]), sd)[0].numpy())
        err["fc6"] = _rel(emb[b].astype(np.float64), o_rn3.fc6(torch.from_numpy(S["rn3_pooled"][b])[None], sd)[0].numpy())
    err["end_to_end"] = _rel(emb[b].astype(np.float64), _oracle_e2e(x[b]))
    return err


def _check_rows(e, x, emb, rows, compute, tag):
    """layer-local errors of the given rows of the handle's last forward, printed, against the bars; returns the worst per stage"""
    B, L = x.shape
    S = _stages(e, B, L)
    assert np.isfinite(emb).all()
    worst = {}
    for b in rows:
        err = _layer_local(S, emb, x, b)
        print(f"{tag} {compute} b={b}: " + ", ".join(f"{n[4:] if n.startswith('rn3_') else n} {err[n]:.2e}" for n in STAGES))
        for n in STAGES:
            worst[n] = max(worst.get(n, 0.0), err[n])
            bar = (F32_BARS if compute == "f32" else BF16_BARS)[n]
            assert err[n] <= bar, (tag, compute, b, n, err[n], bar)
    return worst


def _run_case(compute, B, L, rows=None, options=None, tag=None):
    """one forward with layer labels and profiling on; checks `rows` against the oracle; returns (embeddings, GEMM labels)"""
    x = synth.synth_waveforms(B, L, seed=SEED_X + L)
    e = _engine(compute, B, L)
    for k, v in (options or {}).items():
        e.set_option(k, v)
    e.set_option("layer_labels", 1)
    e.profile(True)
    emb = e.embed_wave(x).reshape(B, -1).copy()
    labels = sorted(n for n in e.profile_results() if n.startswith("gemm_"))
    e.profile(False)
    assert e.numeric_status() == 0
    _check_rows(e, x, emb, _rows(B, L) if rows is None else rows, compute, tag or f"L={L} B={B}")
    e.close()
    return emb, labels


def _kernels(labels, M=None, N=None, K=None):
    """kernel names of the GEMM labels ('<kernel> M<m> N<n> K<k>'), optionally of one shape"""
    out = set()
    for lab in labels:
        f = lab.split()
        if M is None or f[1:4] == [f"M{M}", f"N{N}", f"K{K}"]:
            out.add(f[0])
    return out


def _census_case(compute, B, L):
    key = (L, B)
    if key not in _CENSUS[compute]:
        _CENSUS[compute][key] = _run_case(compute, B, L)[1]
    return _CENSUS[compute][key]


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("L,B", LENGTH_CASES)
def test_stages_against_the_oracle_at_edge_lengths(compute, L, B):
    _census_case(compute, B, L)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_stages_against_the_oracle_on_every_gemm_route(compute):
    """L = 32000 at the smallest batch that puts layer1's, layer2's and layer4's 1 x 1 GEMMs on each of their kernels (derived from
    the CU count); on bf16 handles the label of each such GEMM names the kernel the derivation expects"""
    picks = _route_batches(32000, _num_cu())
    print("route batches:", {f"{n} {r}": B for (n, r), B in sorted(picks.items(), key=lambda kv: kv[1])})
    assert len({r for (n, r) in picks if n == "layer1.conv1"}) == 3 and len({r for (n, r) in picks if n == "layer4"}) == 2, picks
    for B in _route_cases():
        labels = _census_case(compute, B, 32000)
        if compute != "bf16":
            continue
        for name, T, N, K, pw3 in _gemms(32000):
            want = _regime(B * T, N, _num_cu(), pw3).split("/")[0]
            assert want in _kernels(labels, B * T, N, K), (name, B, want, labels)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_route_census(compute):
    """every GEMM kernel RawNet3 reaches ran in a case checked against the oracle (and no kernel outside the list ran)"""
    num_cu = _num_cu()
    for L, B in LENGTH_CASES:
        _census_case(compute, B, L)
    for B in _route_cases():
        _census_case(compute, B, 32000)
    seen = set()
    for (L, B), labels in sorted(_CENSUS[compute].items()):
        print(f"census {compute} L={L} B={B} ({num_cu} CUs): " + "; ".join(labels))
        seen |= _kernels(labels)
    print(f"census {compute}: {sorted(seen)}")
    assert seen == CENSUS_WANT[compute], (sorted(seen), sorted(CENSUS_WANT[compute]))


@pytest.mark.parametrize("options", [{"pw3_cus": 2}, {"pw3_cus": 3}, {"pw3_cus": 3, "pw3_tail_off": 1}, {"pw3_tail_off": 1},
                                     {"pw3_cus": 0}], ids=["cus2", "cus3", "cus3-tail_off", "tail_off", "persistent_off"])
def test_forced_persistent_forms(options):
    """bf16 at B = 2: a grid capped at 2 or 3 workgroups makes gemm_pw3 walk many tiles per workgroup (whole tiles with tail_off);
    pw3_cus = 0 turns the persistent kernel off.  Every variant stays within the layer-local bars."""
    _, labels = _run_case("bf16", 2, 16000, options=options, tag=f"L=16000 B=2 {options}")
    kernels = _kernels(labels)
    if options.get("pw3_cus", -1) > 0:
        assert "gemm_pw3" in kernels, labels
    if options.get("pw3_cus", -1) == 0 or options == {"pw3_tail_off": 1}:
        assert "gemm_pw3" not in kernels, labels


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_full_batch(compute):
    """the tools/rawnet3_bench.py configuration (B = 256, L = 32000): finite, repeatable bit for bit, rows 0 / 127 / 255 within the
    layer-local bars, rows of B = 1 and B = 8 runs within the bars of the full batch's, and a permuted batch gives the permuted rows BIT
    FOR BIT (no RawNet3 kernel sums across utterances: AFMS means, time statistics and softmax are per utterance)"""
    B, L = 256, 32000
    x = synth.synth_waveforms(B, L, seed=SEED_X + 1)
    e = _engine(compute, B, L)
    out = e.embed_wave(x).reshape(B, -1).copy()
    assert np.isfinite(out).all()
    _check_rows(e, x, out, [0, 127, 255], compute, "full batch")
    assert np.array_equal(e.embed_wave(x).reshape(B, -1), out)
    perm = np.random.default_rng(7).permutation(B)
    assert np.array_equal(e.embed_wave(np.ascontiguousarray(x[perm])).reshape(B, -1), out[perm])
    e.close()
    bar = (F32_BARS if compute == "f32" else BF16_BARS)["end_to_end"]
    for b in (1, 8):
        e = _engine(compute, b, L)
        small = e.embed_wave(np.ascontiguousarray(x[:b])).reshape(b, -1)
        e.close()
        for r in range(b):
            d = _rel(small[r], out[r])
            assert d <= bar, (b, r, d)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_partial_batch_is_bit_identical_to_a_handle_of_that_size(compute):
    """B = 3 on a max_batch = 8 handle == a max_batch = 3 handle, bit for bit (layer3's scratch sits at a B-dependent offset in P2)"""
    L = 24001
    x = synth.synth_waveforms(3, L, seed=31)
    outs = []
    for mb in (8, 3):
        e = _engine(compute, mb, L)
        outs.append(e.embed_wave(x).reshape(3, -1).copy())
        e.close()
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_a_nonfinite_input_stays_in_its_utterance(compute):
    """a NaN in one waveform of B = 3: SVHIP_ERR_NONFINITE, a non-finite embedding for that row, the other rows the bits of the clean
    call (the dilated convolutions' zero padding at utterance boundaries never reads a neighbour's frames), and a clean next call"""
    B, L = 3, 24001
    e = _engine(compute, B, L, on_numeric="ignore")
    x = synth.synth_waveforms(B, L, seed=41)
    clean = e.embed_wave(x).reshape(B, -1).copy()
    assert e.numeric_status() == 0
    bad = x.copy()
    bad[1, 12345] = np.nan
    got = np.empty_like(clean)
    rc = e.lib.svhip_embed_wave(e.h, bad.ctypes.data, B, L, got.ctypes.data, 0)
    assert rc == _lib.ERR_NONFINITE, (rc, e.lib.svhip_last_error(e.h))
    assert not np.isfinite(got[1]).any()
    assert np.array_equal(got[[0, 2]], clean[[0, 2]])
    assert e.lib.svhip_embed_wave(e.h, x.ctypes.data, B, L, got.ctypes.data, 0) == 0
    assert np.array_equal(got, clean)
    e.close()


@pytest.mark.parametrize("compute", ["f32", "half"])
def test_raw3_ecapa_with_more_utterances_than_embed_batch(compute):
    """B = 9 through embed_batch = 4 (slices 4, 4, 1): the RawNet3 columns 192: of every row against the oracle end to end, and the
    device-resident path equal to the host path"""
    from speakerverification_amd.models import Raw3_ECAPA
    from tests.test_gpu_rawnet3 import KW, _fusion_sd
    m = Raw3_ECAPA.MainModel(nOut=512, hip_compute=compute, embed_batch=4, **KW)
    m.load_state_dict(_fusion_sd(1, SEED_W))
    x = synth.synth_waveforms(9, 32000, seed=53)
    host = m(x)
    assert host.shape == (9, 512) and np.isfinite(host).all()
    bar = (F32_BARS if compute == "f32" else BF16_BARS)["end_to_end"]
    for b in range(9):
        d = _rel(host[b, 192:].astype(np.float64), _oracle_e2e(x[b]))
        print(f"Raw3_ECAPA {compute} b={b}: rawnet3 columns to the oracle {d:.2e}")
        assert d <= bar, (b, d)
    dev = m(torch.from_numpy(x).cuda())
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
