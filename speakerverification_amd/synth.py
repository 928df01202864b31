"""Parameter specs and deterministic synthetic weights for the hot-path models.

The reference ships no checkpoints and there is no network, so tests, smoke() and bench.py
run on random-initialised weights of the reference architectures.  This module is the single
source of truth for the *names and shapes* of the reference state dicts

  * ECAPA-TDNN  — reference ``src/models/ECAPA_TDNN.py:339-458`` (231 tensors),
  * RawNet2     — reference ``src/models/RawNet2_custom.py:18-135`` + ``RawNet_baseline.py``
                  (``aggregate='asp'``: 147 tensors with ``front_proc='sinc'``, 140 with ``'conv'``),
  * RawNet3     — reference ``src/models/RawNet3.py`` + ``RawNet_baseline.py`` (the defaults of its
                  ``MainModel``: 234 tensors),
  * TitaNet     — reference ``src/models/TitaNet.py`` + ``blocks/titanet_blocks.py`` (sizes s / m / l, any block count),
  * Conformer   — reference ``src/models/Conformer.py`` + ``models/conformer/conformer/*`` (278 tensors at n_mels 80),
  * ResNetSE34V2 — reference ``src/models/ResNetSE34V2.py`` + ``ResNetBaseline.py`` + ``ResNetBlocks.py`` (292 tensors),

and generates values from a ``numpy`` PCG64 stream in state-dict order, so the CPU oracle and the
HIP path see bit-identical weights on any machine.  ``tests/test_oracle_golden.py`` checks the
specs against key/shape lists captured from the imported reference (``tests/golden/*.json``).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np

ECAPA_KERNEL_SIZES = (5, 3, 3, 3, 1)      # ECAPA_TDNN.py:379
ECAPA_DILATIONS = (1, 2, 3, 4, 1)         # ECAPA_TDNN.py:380
RES2NET_SCALE = 8                         # ECAPA_TDNN.py:382
SE_CHANNELS = 128                         # ECAPA_TDNN.py:383
ATT_CHANNELS = 128                        # ECAPA_TDNN.py:381

RAWNET2_LAYERS = (1, 1, 1, 2, 1, 2)                    # RawNet2_custom.py:231
RAWNET2_FILTERS = (128, 128, 256, 256, 512, 512)       # RawNet2_custom.py:232
RAWNET2_SINC_K = 251                                   # RawNet2_custom.py:36
RAWNET2_GRU_NODE = 1024                                # gru_node (RawNet2_custom.py:31)

HYPE_CONTEXT = 512 + 192                               # Raw_ECAPA_hype.py:20: the RawNet2 and ECAPA-TDNN embeddings side by side

RAWNET3_C = 1024                                       # RawNet3.py:10 (C; no config sets it)
RAWNET3_SCALE = 8                                      # model_scale (RawNet3.py:178)
RAWNET3_DILATIONS = (2, 3, 4)                          # RawNet3.py:46-52
RAWNET3_CONTEXT = 1536                                 # RawNet3.py:31
RAWNET3_SINC_HALF = 125                                # ParamSincFB(256, 251): taps on each side of the centre


def _bn(prefix, c):
    return [(prefix + ".weight", (c,)), (prefix + ".bias", (c,)),
            (prefix + ".running_mean", (c,)), (prefix + ".running_var", (c,)),
            (prefix + ".num_batches_tracked", ())]


def _tdnn(prefix, cin, cout, k):
    return ([(prefix + ".conv.conv.weight", (cout, cin, k)), (prefix + ".conv.conv.bias", (cout,))]
            + _bn(prefix + ".norm.norm", cout))


def ecapa_param_spec(C=1024, n_mels=80, nOut=192, input_norm=False):
    """Ordered (name, shape) list == ``ECAPA_TDNN(...).state_dict()`` of the reference."""
    C3 = 3 * C
    spec = []
    spec += _tdnn("blocks.0", n_mels, C, ECAPA_KERNEL_SIZES[0])
    for i in (1, 2, 3):
        p = f"blocks.{i}"
        spec += _tdnn(p + ".tdnn1", C, C, 1)
        for j in range(RES2NET_SCALE - 1):
            spec += _tdnn(p + f".res2net_block.blocks.{j}", C // RES2NET_SCALE, C // RES2NET_SCALE,
                          ECAPA_KERNEL_SIZES[i])
        spec += _tdnn(p + ".tdnn2", C, C, 1)
        spec += [(p + ".se_block.conv1.conv.weight", (SE_CHANNELS, C, 1)),
                 (p + ".se_block.conv1.conv.bias", (SE_CHANNELS,)),
                 (p + ".se_block.conv2.conv.weight", (C, SE_CHANNELS, 1)),
                 (p + ".se_block.conv2.conv.bias", (C,))]
    if input_norm:  # nn.InstanceNorm1d(affine=True, track_running_stats=False), ECAPA_TDNN.py:406-409;
        # registered after the (still empty) blocks ModuleList, so it follows blocks.* in state_dict order
        spec += [("instance_norm.weight", (n_mels,)), ("instance_norm.bias", (n_mels,))]
    spec += _tdnn("mfa", C3, C3, 1)
    spec += _tdnn("asp.tdnn", 3 * C3, ATT_CHANNELS, 1)
    spec += [("asp.conv.conv.weight", (C3, ATT_CHANNELS, 1)), ("asp.conv.conv.bias", (C3,))]
    spec += _bn("asp_bn.norm", 2 * C3)
    spec += [("fc.conv.weight", (nOut, 2 * C3, 1)), ("fc.conv.bias", (nOut,))]
    return spec


def rawnet2_param_spec(nOut=320, nb_samp=32000, att_dim=128, front_proc="sinc", aggregate="asp"):
    """Ordered (name, shape) list == ``RawNet2_custom.MainModel(front_proc=front_proc,
    aggregate=aggregate).state_dict()`` of the reference: 147 tensors for ``'sinc'`` (LayerNorm, sinc filters,
    first_bn), 140 for ``'conv'`` (``conv1 = Conv1d(1, 128, 3, stride=3)`` with bias, RawNet2_custom.py:45-52);
    ``aggregate='gru'`` (RawNet2_custom.py:84-95) replaces bn_before_agg / attention with bn_before_gru, the GRU
    (512 -> 1024, one layer) and fc_after_gru, and keeps the unused fc: 144 tensors with 'sinc'."""
    if aggregate not in ("asp", "gru"):
        raise ValueError(f"aggregate {aggregate!r}: 'asp' or 'gru'")
    f = RAWNET2_FILTERS
    if front_proc == "sinc":
        spec = [("ln.gamma", (nb_samp,)), ("ln.beta", (nb_samp,)),
                ("first_conv.low_hz_", (f[0], 1)), ("first_conv.band_hz_", (f[0], 1))]
        spec += _bn("first_bn", f[0])
    elif front_proc == "conv":
        spec = [("conv1.weight", (f[0], 1, 3)), ("conv1.bias", (f[0],))]
    else:
        raise ValueError(f"front_proc {front_proc!r}: 'sinc' or 'conv'")
    inpl = f[0]
    for li, (nblk, planes) in enumerate(zip(RAWNET2_LAYERS, f), start=1):
        for b in range(nblk):
            p = f"layer{li}.{b}"
            spec += _bn(p + ".bn1", inpl)
            spec += [(p + ".conv1.weight", (planes, inpl, 3))]
            spec += _bn(p + ".bn2", planes)
            spec += [(p + ".conv2.weight", (planes, planes, 3)),
                     (p + ".afms.alpha", (planes, 1)),
                     (p + ".afms.fc.weight", (planes, planes)), (p + ".afms.fc.bias", (planes,))]
            if inpl != planes:
                spec += [(p + ".shortcut.0.weight", (planes, inpl, 1))]
            inpl = planes
    if aggregate == "gru":
        G, H = 3 * RAWNET2_GRU_NODE, RAWNET2_GRU_NODE
        spec += _bn("bn_before_gru", f[5])
        spec += [("gru.weight_ih_l0", (G, f[5])), ("gru.weight_hh_l0", (G, H)), ("gru.bias_ih_l0", (G,)), ("gru.bias_hh_l0", (G,)),
                 ("fc_after_gru.weight", (nOut, H)), ("fc_after_gru.bias", (nOut,)),
                 ("fc.weight", (nOut, 2 * f[5])), ("fc.bias", (nOut,))]
        return spec
    spec += _bn("bn_before_agg", f[5])
    spec += [("attention.0.weight", (att_dim, f[5], 1)), ("attention.0.bias", (att_dim,))]
    spec += _bn("attention.2", att_dim)
    spec += [("attention.3.weight", (f[5], att_dim, 1)), ("attention.3.bias", (f[5],)),
             ("fc.weight", (nOut, 2 * f[5])), ("fc.bias", (nOut,))]
    return spec


def hype_head_param_spec(nOut=512):
    """Ordered (name, shape) list of the attention head of the reference's ``Raw_ECAPA_hype`` (Raw_ECAPA_hype.py:34-44): the 21 tensors
    its state dict holds beside ``ECAPA_TDNN.*``, ``rawnet2v2.*`` and ``compute_features.*``, in its key order"""
    C, A = HYPE_CONTEXT, ATT_CHANNELS
    spec = _bn("bn_before_agg", C)
    spec += [("attention.0.weight", (A, C, 1)), ("attention.0.bias", (A,))]
    spec += _bn("attention.2", A)
    spec += [("attention.3.weight", (C, A, 1)), ("attention.3.bias", (C,))]
    spec += _bn("bn_final", 2 * C)
    spec += [("fc.weight", (nOut, 2 * C)), ("fc.bias", (nOut,))]
    return spec


def rawnet3_param_spec(nOut=512):
    """Ordered (name, shape) list == ``RawNet3.MainModel(nOut=nOut).state_dict()`` of the reference (defaults: model_scale=8,
    context=True, summed=True, encoder_type='ASP', C = 1024): 234 tensors.  ``bn1.*`` and ``bn6.*`` exist but the forward never
    uses them (RawNet3.py:88-99, out_bn=False); ``conv1.filterbank.*`` are the parameters and persistent buffers of the sinc
    filterbank ``ParamSincFB(256, 251, stride=10)``."""
    C, W = RAWNET3_C, RAWNET3_C // RAWNET3_SCALE
    spec = [("preprocess.0.flipped_filter", (1, 1, 2)), ("preprocess.1.weight", (1,)), ("preprocess.1.bias", (1,)),
            ("conv1.filterbank.low_hz_", (C // 8, 1)), ("conv1.filterbank.band_hz_", (C // 8, 1)),
            ("conv1.filterbank.window_", (RAWNET3_SINC_HALF,)), ("conv1.filterbank.n_", (1, RAWNET3_SINC_HALF))]
    spec += _bn("bn1", C // 4)
    for li, cin in enumerate((C // 4, C, C), start=1):
        p = f"layer{li}"
        spec += [(p + ".conv1.weight", (C, cin, 1)), (p + ".conv1.bias", (C,))]
        spec += _bn(p + ".bn1", C)
        for i in range(RAWNET3_SCALE - 1):
            spec += [(p + f".convs.{i}.weight", (W, W, 3)), (p + f".convs.{i}.bias", (W,))]
        for i in range(RAWNET3_SCALE - 1):
            spec += _bn(p + f".bns.{i}", W)
        spec += [(p + ".conv3.weight", (C, C, 1)), (p + ".conv3.bias", (C,))]
        spec += _bn(p + ".bn3", C)
        spec += [(p + ".afms.alpha", (C, 1)), (p + ".afms.fc.weight", (C, C)), (p + ".afms.fc.bias", (C,))]
        if cin != C:
            spec += [(p + ".residual.0.weight", (C, cin, 1))]
    D = RAWNET3_CONTEXT
    spec += [("layer4.weight", (D, 3 * C, 1)), ("layer4.bias", (D,)),
             ("attention.0.weight", (128, 3 * D, 1)), ("attention.0.bias", (128,))]
    spec += _bn("attention.2", 128)
    spec += [("attention.3.weight", (1, 128, 1)), ("attention.3.bias", (1,))]
    spec += _bn("bn5", 2 * D)
    spec += [("fc6.weight", (nOut, 2 * D)), ("fc6.bias", (nOut,))]
    spec += _bn("bn6", nOut)
    return spec


TITANET_SIZES = {"s": (256, 3), "m": (512, 7), "l": (1024, 11)}      # hidden size H, depthwise kernel (TitaNet.py:152-157)
TITANET_TARGET_PARAMS = {"s": 6.4, "m": 13.4, "l": 25.3}             # TitaNet.TARGET_PARAMS (millions)
TITANET_ENC = 1536                                                   # encoder_output_size (TitaNet.py:145)
TITANET_ATT = 128                                                    # attention_hidden_size
TITANET_SE_REDUCTION = 16


def titanet_n_params(size, nOut, n_blocks, n_mels=80):
    """trainable parameters of ``TitaNet.get_titanet(nOut, n_mels, n_blocks, size)`` (get_n_params: BatchNorm running statistics are
    buffers, not parameters), in closed form"""
    H, k = TITANET_SIZES[size]
    D, A = TITANET_ENC, TITANET_ATT
    prolog = H * n_mels * 3 + H + 2 * H
    block = 3 * (H * k + H + H * H + H + 2 * H) + 2 * H * (H // TITANET_SE_REDUCTION) + H * H + H + 2 * H
    epilog = D * H + D + 2 * D
    decoder = D * A + A + A * D + D + 2 * 2 * D + 2 * D * nOut + nOut + 2 * nOut
    return prolog + n_blocks * block + epilog + decoder


def titanet_n_mega_blocks(size, nOut, n_mels=80):
    """``TitaNet.find_n_mega_blocks`` (TitaNet.py:82-109): the count in 1 .. 19 whose parameter total (in millions) is closest to
    TARGET_PARAMS[size], the first one on a tie"""
    target = TITANET_TARGET_PARAMS[size]
    best, dist = None, math.inf
    for n in range(1, 20):
        d = abs(target - titanet_n_params(size, nOut, n, n_mels) / 1e6)
        if d < dist:
            best, dist = n, d
    return best


def titanet_param_spec(size="l", nOut=512, n_blocks=None, n_mels=80):
    """Ordered (name, shape) list == ``TitaNet.MainModel(nOut, model_size=size, n_mega_blocks=n_blocks).state_dict()`` of the reference
    (TitaNet.py:202-431, blocks/titanet_blocks.py); n_blocks None: find_n_mega_blocks' choice"""
    H, k = TITANET_SIZES[size]
    D = TITANET_ENC
    if n_blocks is None:
        n_blocks = titanet_n_mega_blocks(size, nOut, n_mels)
    spec = [("encoder.prolog.conv_block.0.weight", (H, n_mels, 3)), ("encoder.prolog.conv_block.0.bias", (H,))]
    spec += _bn("encoder.prolog.conv_block.1", H)
    for i in range(n_blocks):
        p = f"encoder.mega_blocks.{i}."
        for j in range(3):
            q = p + f"sub_blocks.{j}.conv_block."
            spec += [(q + "0.conv.0.weight", (H, 1, k)), (q + "0.conv.0.bias", (H,)),
                     (q + "0.conv.1.weight", (H, H, 1)), (q + "0.conv.1.bias", (H,))]
            spec += _bn(q + "1", H)
        Hh = H // TITANET_SE_REDUCTION
        spec += [(p + "sub_blocks.3.excitation.0.weight", (Hh, H)), (p + "sub_blocks.3.excitation.2.weight", (H, Hh)),
                 (p + "skip_connection.0.weight", (H, H, 1)), (p + "skip_connection.0.bias", (H,))]
        spec += _bn(p + "skip_connection.1", H)
    spec += [("encoder.epilog.conv_block.0.weight", (D, H, 1)), ("encoder.epilog.conv_block.0.bias", (D,))]
    spec += _bn("encoder.epilog.conv_block.1", D)
    spec += [("decoder.pool.0.in_linear.weight", (TITANET_ATT, D)), ("decoder.pool.0.in_linear.bias", (TITANET_ATT,)),
             ("decoder.pool.0.out_linear.weight", (D, TITANET_ATT)), ("decoder.pool.0.out_linear.bias", (D,))]
    spec += _bn("decoder.pool.1", 2 * D)
    spec += [("decoder.linear.0.weight", (nOut, 2 * D)), ("decoder.linear.0.bias", (nOut,))]
    spec += _bn("decoder.linear.1", nOut)
    return spec


CONFORMER_D = 256                                    # encoder_dim (Conformer.py:43)
CONFORMER_LAYERS = 6                                 # num_layers (Conformer.py:48)
CONFORMER_HEADS = 4
CONFORMER_MAX_T = 10000                              # PositionalEncoding's max_len (embedding.py:31)


def conformer_f2(n_mels):
    """frequency bins after Conv2dSubampling's two 3 x 3 stride-2 convolutions"""
    f1 = (n_mels - 3) // 2 + 1
    return (f1 - 3) // 2 + 1


def conformer_frames(T):
    """T' of Conv2dSubampling for T input frames (0 when T < 7: the reference refuses such inputs)"""
    if T < 7:
        return 0
    return ((T - 3) // 2 + 1 - 3) // 2 + 1


def conformer_pe(d_model=CONFORMER_D, max_len=CONFORMER_MAX_T):
    """PositionalEncoding.pe (embedding.py:30-38) in torch's float32 arithmetic: div_term = exp(float32), position * div_term rounded to
    float32, then sin / cos.  torch evaluates it when it is importable (its float32 exp is not correctly rounded: three of the 128
    div_term values differ by an ulp from the rounded exact value, which moves the arguments near position 10^4 by 1e-3); otherwise the
    same steps in numpy with correctly rounded exp / sin / cos"""
    try:
        import torch
    except Exception:  # pragma: no cover
        torch = None
    if torch is not None:
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * -(math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        return pe.numpy().reshape(1, max_len, d_model)
    div = np.exp((np.arange(0, d_model, 2, dtype=np.float32) * np.float32(-(math.log(10000.0) / d_model))).astype(np.float64)).astype(np.float32)
    arg = (np.arange(max_len, dtype=np.float32)[:, None] * div[None, :]).astype(np.float32)
    pe = np.zeros((max_len, d_model), np.float32)
    pe[:, 0::2] = np.sin(arg.astype(np.float64)).astype(np.float32)
    pe[:, 1::2] = np.cos(arg.astype(np.float64)).astype(np.float32)
    return pe.reshape(1, max_len, d_model)


def conformer_param_spec(nOut=512, n_mels=80, attention_dim=128):
    """Ordered (name, shape) list == ``Conformer.MainModel(nOut, n_mels=n_mels).state_dict()`` of the reference (Conformer.py:13-97,
    conformer/encoder.py, attention.py, convolution.py, feed_forward.py)"""
    D, F2 = CONFORMER_D, conformer_f2(n_mels)
    ln = lambda p: [(p + ".weight", (D,)), (p + ".bias", (D,))]
    spec = [("instance_norm.weight", (n_mels,)), ("instance_norm.bias", (n_mels,))]
    s = "conformer_block.conv_subsample.sequential."
    spec += [(s + "0.weight", (D, 1, 3, 3)), (s + "0.bias", (D,)), (s + "2.weight", (D, D, 3, 3)), (s + "2.bias", (D,))]
    spec += [("conformer_block.input_projection.0.linear.weight", (D, D * F2)), ("conformer_block.input_projection.0.linear.bias", (D,))]

    def ff(q):
        return ln(q + "module.sequential.0") + [
            (q + "module.sequential.1.linear.weight", (4 * D, D)), (q + "module.sequential.1.linear.bias", (4 * D,)),
            (q + "module.sequential.4.linear.weight", (D, 4 * D)), (q + "module.sequential.4.linear.bias", (D,))]
    for i in range(CONFORMER_LAYERS):
        p = f"conformer_block.layers.{i}."
        spec += ff(p + "sequential.0.")
        a = p + "sequential.1.module."
        spec += [(a + "positional_encoding.pe", (1, CONFORMER_MAX_T, D))] + ln(a + "layer_norm")
        dh = D // CONFORMER_HEADS
        spec += [(a + "attention.u_bias", (CONFORMER_HEADS, dh)), (a + "attention.v_bias", (CONFORMER_HEADS, dh))]
        for q in ("query_proj", "key_proj", "value_proj"):
            spec += [(a + f"attention.{q}.linear.weight", (D, D)), (a + f"attention.{q}.linear.bias", (D,))]
        spec += [(a + "attention.pos_proj.linear.weight", (D, D)),
                 (a + "attention.out_proj.linear.weight", (D, D)), (a + "attention.out_proj.linear.bias", (D,))]
        c = p + "sequential.2.module.sequential."
        spec += ln(c + "0") + [(c + "2.conv.weight", (2 * D, D, 1)), (c + "2.conv.bias", (2 * D,)), (c + "4.conv.weight", (D, 1, 15))]
        spec += _bn(c + "5", D) + [(c + "7.conv.weight", (D, D, 1)), (c + "7.conv.bias", (D,))]
        spec += ff(p + "sequential.3.") + ln(p + "sequential.4")
    spec += [("asp.tdnn.conv.conv.weight", (attention_dim, 3 * D, 1)), ("asp.tdnn.conv.conv.bias", (attention_dim,))]
    spec += _bn("asp.tdnn.norm.norm", attention_dim)
    spec += [("asp.conv.weight", (D, attention_dim, 1)), ("asp.conv.bias", (D,))] + _bn("asp_bn.norm", 2 * D)
    spec += [("attention.0.weight", (attention_dim, D, 1)), ("attention.0.bias", (attention_dim,))] + _bn("attention.2", attention_dim)
    spec += [("attention.3.weight", (D, attention_dim, 1)), ("attention.3.bias", (D,))] + _bn("attention_norm", 2 * D)
    spec += [("fc.conv.weight", (nOut, 2 * D, 1)), ("fc.conv.bias", (nOut,))]
    return spec


RESNETSE_BLOCKS = {"ResNetSE34V2": ((3, 4, 6, 3), (32, 64, 128, 256))}     # blocks per stage, widths (ResNetSE34V2.py:5-9)
RESNETSE_SE_HIDDEN = 16                              # SEBasicBlockV2's `reduction`, which SELayer takes as its hidden width
RESNETSE_ATT = 128                                   # att_dim


def resnetse_frames(T, n_mels=80):
    """(frames, mel rows) that reach the pooling: three Conv2d(3, stride 2, padding 1)"""
    for _ in range(3):
        T, n_mels = (T - 1) // 2 + 1, (n_mels - 1) // 2 + 1
    return T, n_mels


def resnetse_param_spec(nOut=256, n_mels=80, encoder_type="ASP", arch="ResNetSE34V2"):
    """Ordered (name, shape) list == ``ResNetSE34V2.MainModel(nOut, n_mels=n_mels, encoder_type=...).state_dict()`` of the reference
    (ResNetBaseline.py:141-243, ResNetBlocks.py:211-246,292-307): 292 tensors"""
    blocks, widths = RESNETSE_BLOCKS[arch]
    spec = [("conv1.weight", (widths[0], 1, 3, 3)), ("conv1.bias", (widths[0],))] + _bn("bn1", widths[0])
    inpl = widths[0]
    for s, (n, C) in enumerate(zip(blocks, widths)):
        for j in range(n):
            p = f"layer{s + 1}.{j}."
            spec += [(p + "conv1.weight", (C, inpl, 3, 3))] + _bn(p + "bn1", C)
            spec += [(p + "conv2.weight", (C, C, 3, 3))] + _bn(p + "bn2", C)
            spec += [(p + "se.fc.0.weight", (RESNETSE_SE_HIDDEN, C)), (p + "se.fc.0.bias", (RESNETSE_SE_HIDDEN,)),
                     (p + "se.fc.2.weight", (C, RESNETSE_SE_HIDDEN)), (p + "se.fc.2.bias", (C,))]
            if j == 0 and s > 0:
                spec += [(p + "downsample.0.weight", (C, inpl, 1, 1))] + _bn(p + "downsample.1", C)
            inpl = C
    F = widths[3] * (n_mels // 8)
    spec += [("attention.0.weight", (RESNETSE_ATT, F, 1)), ("attention.0.bias", (RESNETSE_ATT,))] + _bn("attention.2", RESNETSE_ATT)
    spec += [("attention.3.weight", (F, RESNETSE_ATT, 1)), ("attention.3.bias", (F,))]
    spec += [("fc.weight", (nOut, F if encoder_type == "SAP" else 2 * F)), ("fc.bias", (nOut,))]
    return spec


def rawnet3_sinc_buffers():
    """the persistent buffers of ParamSincFB(256, 251) at sample_rate 16000: window_ (125,), n_ (1, 125)"""
    n_lin = np.linspace(0.0, 251 / 2 - 1, RAWNET3_SINC_HALF)
    window = (0.54 - 0.46 * np.cos(2 * math.pi * n_lin / 251)).astype(np.float32)
    n = (2 * math.pi * np.arange(-RAWNET3_SINC_HALF, 0) / 16000.0).reshape(1, -1).astype(np.float32)
    return window, n


def rawnet3_sinc_filters(low_hz_, band_hz_, window_, n_, sample_rate=16000.0, min_low_hz=50.0, min_band_hz=50.0):
    """ParamSincFB.filters() (asteroid-filterbanks 0.4.x, the filterbank RawNet3.py:35-41 instantiates) in float64 numpy: the
    (256, 251) band-pass bank, 128 cos filters then 128 sin filters.  The cos half is RawNet_baseline.py:339-357's formula; the
    library bakes the same arithmetic at finalize (api_rawnet2.hip)."""
    low = min_low_hz + np.abs(np.asarray(low_hz_, np.float64).reshape(-1, 1))
    high = np.clip(low + min_band_hz + np.abs(np.asarray(band_hz_, np.float64).reshape(-1, 1)), min_low_hz, sample_rate / 2)
    band = (high - low)[:, 0]
    n = np.asarray(n_, np.float64).reshape(1, -1)
    w = np.asarray(window_, np.float64).reshape(1, -1)
    ft_low, ft_high = low @ n, high @ n
    cos_left = (np.sin(ft_high) - np.sin(ft_low)) / (n / 2) * w
    sin_left = (np.cos(ft_low) - np.cos(ft_high)) / (n / 2) * w
    cos = np.concatenate([cos_left, 2 * band[:, None], cos_left[:, ::-1]], axis=1)
    sin = np.concatenate([sin_left, np.zeros((len(band), 1)), -sin_left[:, ::-1]], axis=1)
    return np.concatenate([cos / (2 * band[:, None]), sin / (2 * band[:, None])], axis=0)


def _sinc_init(n_filt, sample_rate=16000, min_low_hz=50, min_band_hz=50):
    # same initial values as RawNet_baseline.py:296-310 (mel-spaced band edges)
    to_mel = lambda hz: 2595 * np.log10(1 + hz / 700)
    to_hz = lambda mel: 700 * (10 ** (mel / 2595) - 1)
    high_hz = sample_rate / 2 - (min_low_hz + min_band_hz)
    hz = to_hz(np.linspace(to_mel(10), to_mel(high_hz), n_filt + 1))
    return hz[:-1].astype(np.float32), np.diff(hz).astype(np.float32)


def synth_state_dict(spec, seed=1, sample_rate=16000):
    """Deterministic non-trivial weights (numpy float32 / int64) in ``spec`` order.

    Conv / linear weights are He-scaled so activations stay O(1) through the stack; BatchNorm
    running statistics and affine terms are randomised so that BN cannot be mistaken for the
    identity; sinc band edges start from the reference initialisation at ``sample_rate`` (SincConv_fast's argument,
    RawNet_baseline.py:296-310) plus jitter.
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for name, shape in spec:
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            sd[name] = np.array(1000, dtype=np.int64)
        elif leaf == "running_var":
            sd[name] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif leaf == "running_mean":
            sd[name] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif leaf == "gamma":                                  # RawNet2 LayerNorm
            sd[name] = (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif leaf == "beta":
            sd[name] = (0.01 * rng.standard_normal(shape)).astype(np.float32)
        elif leaf == "alpha":                                  # AFMS
            sd[name] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif leaf == "flipped_filter":                        # PreEmphasis(0.97), RawNet_baseline.py:27-38
            sd[name] = np.array([-0.97, 1.0], dtype=np.float32).reshape(shape)
        elif leaf == "pe":                                     # Conformer's PositionalEncoding buffer: the formula, not random
            sd[name] = conformer_pe(shape[2], shape[1])
        elif leaf in ("u_bias", "v_bias"):                     # Conformer's per-head position biases
            sd[name] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif leaf in ("window_", "n_"):                        # ParamSincFB's persistent buffers
            sd[name] = rawnet3_sinc_buffers()[0 if leaf == "window_" else 1].reshape(shape)
        elif leaf in ("low_hz_", "band_hz_"):
            lo, band = _sinc_init(shape[0], sample_rate)
            base = lo if leaf == "low_hz_" else band
            jitter = rng.uniform(-3.0, 3.0, shape[0]).astype(np.float32)
            sd[name] = (base + jitter).reshape(shape).astype(np.float32)
        elif leaf in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):      # nn.GRU's own init: U(+-1 / sqrt(hidden))
            k = 1.0 / math.sqrt(RAWNET2_GRU_NODE)
            sd[name] = rng.uniform(-k, k, shape).astype(np.float32)
        elif leaf == "weight" and len(shape) == 1:             # BN / InstanceNorm affine weight
            sd[name] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif leaf == "bias":
            sd[name] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif leaf == "weight":
            fan_in = int(np.prod(shape[1:]))
            std = math.sqrt(2.0 / fan_in)
            # RawNet2's residual stack has no normalisation on the skip path: with full He gain the
            # activations grow to O(500) and the reference's own fp32 arithmetic is only good to ~1e-3
            # (fp32 vs fp64 oracle).  Gain 0.7 keeps outputs at the O(20) the reference shows with its
            # default init and the fp32 noise floor at ~1e-5, so that a 1e-4 parity bar means something.
            if name.startswith("layer") and (".conv" in name or "shortcut" in name):
                std *= 0.7
            # TitaNet's mega-blocks add the BN'd skip to the gated sub-block path without a normalisation after the sum: with full He
            # gain the block outputs grow ~2x per block (TitaNet-S: 1e7 after 18 blocks).  Gains 0.5 (skip) and 0.7 (pointwise convs)
            # keep every block output O(1) for s / m / l.
            if "mega_blocks." in name and ".skip_connection.0." in name:
                std *= 0.5
            elif "mega_blocks." in name and ".conv.1." in name:
                std *= 0.7
            sd[name] = (std * rng.standard_normal(shape)).astype(np.float32)
        else:  # pragma: no cover
            raise KeyError(name)
    return sd


def synth_waveforms(batch, length=32000, seed=20220829):
    """``0.1·N(0,1)`` clipped to [-1,1]; seed = yaml/configuration-voxceleb.yaml:15."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = 0.1 * rng.standard_normal((batch, length), dtype=np.float32)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def synth_speechlike(batch, length=32000, seed=7):
    """Coloured, amplitude-modulated noise: a less flat spectrum than white noise, used by the
    fbank parity tests so that mel powers span several decades as they do on speech."""
    rng = np.random.Generator(np.random.PCG64(seed))
    from scipy.signal import lfilter
    x = rng.standard_normal((batch, length)).astype(np.float64)
    y = lfilter([1.0], [1.0, -0.95], x, axis=1)
    env = 0.3 + 0.7 * np.abs(np.sin(2 * np.pi * np.arange(length) / 4000.0 + rng.uniform(0, 6, (batch, 1))))
    y = y * env
    y = 0.5 * y / np.abs(y).max(axis=1, keepdims=True)
    return y.astype(np.float32)


def synth_mel(batch, n_mels=80, frames=401, seed=11):
    """Positive mel-power-like features spanning several decades, (B, n_mels, T) float32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = rng.normal(-4.0, 1.5, (batch, n_mels, 1))
    x = np.exp(base + 1.2 * rng.standard_normal((batch, n_mels, frames)))
    return x.astype(np.float32)


def synth_speaker_embeddings(n, n_speakers=5994, dim=192, seed=2, same_cos=(0.5, 0.8), n_groups=1, group_cos=0.35):
    """Embeddings with the structure trained speaker embeddings have: `n_speakers` unit centroids, embedding i =
    a c_s(i) + sqrt(1 - a^2) v_i with v_i a random unit direction and a^2 ~ U(same_cos), so that two embeddings of one speaker have cosine
    a a' in same_cos (the regime of tests/golden/e2e_speakers.npz) and an embedding scores ~a against its own centroid.  n_groups > 1 puts
    the centroids themselves into groups (gender / language): c_s = sqrt(group_cos) g_k(s) + sqrt(1 - group_cos) u_s, so centroids of one group
    have cosine ~group_cos and the cohort scores of an embedding are BIMODAL — what the normal-quantile threshold of the fused AS-norm
    kernel does not fit.  Returns (embeddings (n, dim), centroids (n_speakers, dim), speaker of each embedding), all fp32 / int32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    def unit(shape):
        x = rng.standard_normal(shape, dtype=np.float32)
        return x / np.linalg.norm(x, axis=-1, keepdims=True)
    cent = unit((n_speakers, dim))
    if n_groups > 1:
        g = unit((n_groups, dim))
        grp = np.arange(n_speakers) % n_groups
        cent = np.float32(np.sqrt(group_cos)) * g[grp] + np.float32(np.sqrt(1.0 - group_cos)) * cent
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    spk = rng.integers(0, n_speakers, n).astype(np.int32)
    a = np.sqrt(rng.uniform(same_cos[0], same_cos[1], n)).astype(np.float32)[:, None]
    e = a * cent[spk] + np.sqrt(1.0 - a * a) * unit((n, dim))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    return e.astype(np.float32), cent.astype(np.float32), spk


def synth_embeddings(n, dim=192, seed=2, normalize=True):
    """l2norm(standard_normal((n, dim)))."""
    rng = np.random.Generator(np.random.PCG64(seed))
    e = rng.standard_normal((n, dim), dtype=np.float32)
    if normalize:
        e /= np.linalg.norm(e, axis=1, keepdims=True)
    return e.astype(np.float32)
