"""Packed checkpoint blobs: reference checkpoints -> the archive libsvhip.so mmaps.

The reference keeps weights as torch pickles written by ``trainer.py:145-205`` (``<save_path>/model/*.model``, the
``state_dict()`` of ``WrappedModel(SpeakerEncoder)``: keys ``module.__S__.*`` for the embedding network, ``module.__L__.*``
for the loss head, ``module.compute_features.*`` for the front-end buffers) and reads them back with ``torch.load`` in
``ModelHandling.loadParameters`` (``model.py:718-746``).  ``convert_checkpoint`` does that read once, on the host, keeps
the ``__S__`` tensors under their bare reference names and writes a blob (``csrc/blob.hip`` documents the layout);
``Engine.load_blob`` / ``svhip_load_blob`` then need neither Python pickles nor torch.

    python -m speakerverification_amd.checkpoint SRC.model DST.svhip --model ECAPA_TDNN

The blob reader / writer is the C one (ctypes), so there is a single implementation of the format.
"""
from __future__ import annotations

import argparse
import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib

MAGIC = b"SVHIPWB1"
_MODEL_IDS = {"ECAPA_TDNN": _lib.MODEL_ECAPA, "ecapa": _lib.MODEL_ECAPA, "RawNet2_custom": _lib.MODEL_RAWNET2,
              "rawnet2": _lib.MODEL_RAWNET2, "RawNet2_custom_conv": _lib.MODEL_RAWNET2_CONV, "rawnet2_conv": _lib.MODEL_RAWNET2_CONV,
              "RawNet2_custom_gru": _lib.MODEL_RAWNET2_GRU, "rawnet2_gru": _lib.MODEL_RAWNET2_GRU,
              "RawNet3": _lib.MODEL_RAWNET3, "rawnet3": _lib.MODEL_RAWNET3, "TitaNet": _lib.MODEL_TITANET, "titanet": _lib.MODEL_TITANET,
              "Conformer": _lib.MODEL_CONFORMER, "conformer": _lib.MODEL_CONFORMER,
              "ResNetSE34V2": _lib.MODEL_RESNETSE, "resnetse": _lib.MODEL_RESNETSE,
              "Raw_ECAPA_hype_head": _lib.MODEL_FUSION_HEAD, "fusion_head": _lib.MODEL_FUSION_HEAD}


def model_id(model) -> int:
    if isinstance(model, int):
        return model
    try:
        return _MODEL_IDS[model]
    except KeyError:
        raise ValueError(f"unknown model {model!r}; expected one of {sorted(_MODEL_IDS)}") from None


def is_blob(path) -> bool:
    try:
        with open(path, "rb") as f:
            return f.read(8) == MAGIC
    except OSError:
        return False


def _blob_error(rc):
    msg = _lib.load().svhip_blob_last_error()
    return _lib.SvhipError(rc, msg.decode() if msg else "?")


def embedding_state_dict(state) -> "OrderedDict[str, np.ndarray]":
    """The ``__S__`` part of a reference checkpoint under bare parameter names (what ``__S__.state_dict()`` would give).

    Accepts a ``WrappedModel`` / ``SpeakerEncoder`` state dict (``module.__S__.x`` / ``__S__.x`` keys; everything else
    — loss head, front-end buffers — is dropped, as the eval path never reads it) or an already bare state dict.
    """
    out = OrderedDict()
    keys = list(state.keys())
    has_s = any("__S__." in k for k in keys)
    for k in keys:
        v = state[k]
        if has_s:
            i = k.find("__S__.")
            if i < 0:
                continue
            name = k[i + len("__S__."):]
        else:
            name = k[len("module."):] if k.startswith("module.") else k
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        out[name] = a
    return out


def write_blob(path, model, state) -> None:
    """Write ``state`` (name -> array; fp32 or int64 tensors of rank <= 4) as a weight blob for ``model``."""
    lib = _lib.load()
    names, arrays = [], []
    for k, v in state.items():
        shape = tuple(np.shape(v))
        a = np.asarray(v)
        if a.dtype == np.int64 or a.dtype == np.int32:
            a = np.ascontiguousarray(a, dtype=np.int64)
        else:
            a = np.ascontiguousarray(a, dtype=np.float32)
        if len(shape) > 4:
            raise ValueError(f"{k}: rank {len(shape)} tensors are not supported")
        names.append(k.encode())
        arrays.append((a, shape))
    n = len(names)
    c_names = (C.c_char_p * max(n, 1))(*names)
    c_data = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a, _ in arrays])
    c_shapes = (C.c_int64 * (4 * max(n, 1)))()
    c_ndims = (C.c_int32 * max(n, 1))()
    c_dtypes = (C.c_int32 * max(n, 1))()
    for i, (a, shape) in enumerate(arrays):
        for d, s in enumerate(shape):
            c_shapes[4 * i + d] = s
        c_ndims[i] = len(shape)
        c_dtypes[i] = _lib.I64 if a.dtype == np.int64 else _lib.F32
    rc = lib.svhip_blob_write(str(path).encode(), model_id(model), n, c_names, c_data, c_shapes, c_ndims, c_dtypes)
    if rc != _lib.OK:
        raise _blob_error(rc)


def read_blob(path):
    """-> (model id, OrderedDict name -> array copy).  Validates magic, version, size and checksum (C reader)."""
    lib = _lib.load()
    b = C.c_void_p()
    rc = lib.svhip_blob_open(str(path).encode(), C.byref(b))
    if rc != _lib.OK:
        raise _blob_error(rc)
    try:
        out = OrderedDict()
        for i in range(lib.svhip_blob_count(b)):
            name, data = C.c_char_p(), C.c_void_p()
            shape = (C.c_int64 * 4)()
            ndim, dtype = C.c_int32(), C.c_int32()
            rc = lib.svhip_blob_tensor(b, i, C.byref(name), C.byref(data), shape, C.byref(ndim), C.byref(dtype))
            if rc != _lib.OK:
                raise _blob_error(rc)
            shp = tuple(shape[d] for d in range(ndim.value))
            np_dt = np.int64 if dtype.value == _lib.I64 else np.float32
            count = int(np.prod(shp, dtype=np.int64)) if shp else 1
            if count:
                buf = (C.c_char * (count * np.dtype(np_dt).itemsize)).from_address(data.value)
                a = np.frombuffer(buf, dtype=np_dt, count=count).reshape(shp).copy()
            else:
                a = np.zeros(shp, np_dt)
            out[name.value.decode()] = a
        return lib.svhip_blob_model(b), out
    finally:
        lib.svhip_blob_close(b)


# fusion model -> its branches: (state-dict prefix, blob model, blob suffix).  The RawNet2 blob's model id records the front-end
# and the aggregation (SVHIP_MODEL_RAWNET2: 'sinc' / asp, SVHIP_MODEL_RAWNET2_CONV: 'conv' / asp, SVHIP_MODEL_RAWNET2_GRU: 'sinc' / gru),
# so a pair cannot be loaded into the other model's module.
FUSION_MODELS = {
    "Raw_ECAPA_sinc_asp": (("ECAPA_TDNN.", "ECAPA_TDNN", ".ecapa"), ("rawnet2v2.", "RawNet2_custom", ".rawnet2")),
    "Raw_ECAPA_sinc_gru": (("ECAPA_TDNN.", "ECAPA_TDNN", ".ecapa"), ("rawnet2v2.", "RawNet2_custom_gru", ".rawnet2")),
    "Raw_ECAPA": (("ECAPA_TDNN.", "ECAPA_TDNN", ".ecapa"), ("rawnet2v2.", "RawNet2_custom", ".rawnet2")),
    "Raw_ECAPA_conv_asp": (("ECAPA_TDNN.", "ECAPA_TDNN", ".ecapa"), ("rawnet2v2.", "RawNet2_custom_conv", ".rawnet2")),
    # Raw3_ECAPA.py: the raw-waveform branch is RawNet3, attribute `rawnet`; its blob's model id is SVHIP_MODEL_RAWNET3
    "Raw3_ECAPA": (("ECAPA_TDNN.", "ECAPA_TDNN", ".ecapa"), ("rawnet.", "RawNet3", ".rawnet3")),
    # Tita_ECAPA.py: ECAPA + TitaNet-M (attribute `titaNet`); Raw_tita.py: TitaNet-M, then RawNet2 'sinc' / asp (attribute `RawNet`)
    "Tita_ECAPA": (("ECAPA_TDNN.", "ECAPA_TDNN", ".ecapa"), ("titaNet.", "TitaNet", ".titanet")),
    "Raw_tita": (("titaNet.", "TitaNet", ".titanet"), ("RawNet.", "RawNet2_custom", ".rawnet2")),
    # Raw_ECAPA_hype.py: ECAPA + RawNet2 'sinc' / gru (nOut 512), then the attention head whose 21 tensors sit at the top level of the
    # state dict (prefix ""): a third blob, model id SVHIP_MODEL_FUSION_HEAD
    "Raw_ECAPA_hype": (("ECAPA_TDNN.", "ECAPA_TDNN", ".ecapa"), ("rawnet2v2.", "RawNet2_custom_gru", ".rawnet2"),
                       ("", "Raw_ECAPA_hype_head", ".head")),
}
_BRANCH_PREFIXES = ("ECAPA_TDNN.", "rawnet2v2.", "rawnet.", "titaNet.", "RawNet.")


def fusion_blob_paths(dst, model="Raw_ECAPA_sinc_asp"):
    """the branch blobs a fusion checkpoint converts to: (ECAPA path, RawNet2 path), and for Raw_ECAPA_hype the head's as a third"""
    return tuple(str(dst) + suffix for _, _, suffix in FUSION_MODELS[model])


def convert_checkpoint(src, dst, model) -> int:
    """Reference checkpoint file (torch pickle) or state dict -> blob at ``dst``.  Returns the number of tensors written.

    A fusion checkpoint (``model`` one of FUSION_MODELS — ``Raw_ECAPA_sinc_asp``, ``Raw_ECAPA``, ``Raw_ECAPA_conv_asp``: keys
    ``__S__.ECAPA_TDNN.*`` / ``__S__.rawnet2v2.*``, Raw_ECAPA*.py:22-28) becomes one blob per branch, ``dst + '.ecapa'`` and ``dst + '.rawnet2'`` — a handle is one
    network, and ``Raw_ECAPA.load_blob(dst)`` reads the pair back.  ``Raw3_ECAPA`` (keys ``__S__.ECAPA_TDNN.*`` / ``__S__.rawnet.*``)
    writes ``dst + '.ecapa'`` and ``dst + '.rawnet3'``; ``Raw_ECAPA_hype`` writes ``dst + '.ecapa'``, ``dst + '.rawnet2'`` and, for the 21
    tensors of its attention head, ``dst + '.head'``."""
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        import torch  # host-side only: the one place a pickle is read
        state = torch.load(src, map_location="cpu")     # the reference's 'cpu:0' is rejected by current torch
        if isinstance(state, dict) and "model" in state and "optimizer" in state:   # trainer.py:170-180 full-state files
            state = state["model"]
    else:
        state = src
    sd = embedding_state_dict(state)
    if model in FUSION_MODELS:
        mine = tuple(prefix for prefix, _, _ in FUSION_MODELS[model] if prefix)
        foreign = sorted({p for p in _BRANCH_PREFIXES if p not in mine and any(k.startswith(p) for k in sd)})
        if foreign and ("titaNet." in mine or "titaNet." in foreign):    # a TitaNet fusion checkpoint as another fusion model, or the other way round
            raise ValueError(f"{model}: the checkpoint holds {foreign[0]}* tensors, a branch this model does not have (its branches: {list(mine)})")
        if any(k.startswith(("RawNet.conv1.", "RawNet.gru.")) for k in sd):         # Raw_tita's RawNet2 is 'sinc' / asp (Raw_tita.py:22-24)
            raise ValueError(f"{model}: the checkpoint's RawNet2 branch is not front_proc='sinc', aggregate='asp'")
        raw_prefix = FUSION_MODELS[model][1][0]
        other = "rawnet2v2." if raw_prefix == "rawnet." else "rawnet."
        if any(k.startswith(other) for k in sd):          # a RawNet2 fusion checkpoint as Raw3_ECAPA, or the other way round
            raise ValueError(f"{model}: the checkpoint's raw-waveform branch is '{other}*' ("
                             f"{'RawNet2' if other == 'rawnet2v2.' else 'RawNet3'}), not this model's '{raw_prefix}*'")
        front = "conv" if FUSION_MODELS[model][1][1] == "RawNet2_custom_conv" else "sinc"
        if front == "conv" and any(k.startswith("rawnet2v2.first_conv.") for k in sd):
            raise ValueError(f"{model}: the checkpoint's RawNet2 branch has a sinc front-end (rawnet2v2.first_conv.*)")
        if front == "sinc" and any(k.startswith("rawnet2v2.conv1.") for k in sd):
            raise ValueError(f"{model}: the checkpoint's RawNet2 branch has a conv front-end (rawnet2v2.conv1.*)")
        if raw_prefix == "rawnet2v2.":
            agg = "gru" if FUSION_MODELS[model][1][1] == "RawNet2_custom_gru" else "asp"
            if agg == "asp" and any(k.startswith("rawnet2v2.gru.") for k in sd):
                raise ValueError(f"{model}: the checkpoint's RawNet2 branch aggregates with a GRU (rawnet2v2.gru.*), not attentive "
                                 "statistics pooling: convert it as Raw_ECAPA_sinc_gru")
            if agg == "gru" and any(k.startswith("rawnet2v2.attention.") for k in sd):
                raise ValueError(f"{model}: the checkpoint's RawNet2 branch aggregates with attentive statistics pooling "
                                 "(rawnet2v2.attention.*), not a GRU")
        total = 0
        for prefix, branch, suffix in FUSION_MODELS[model]:
            if prefix:
                sub = OrderedDict((k[len(prefix):], v) for k, v in sd.items() if k.startswith(prefix))
            else:       # the head: what sits at the top level, beside the branches and the front-end's buffers
                sub = OrderedDict((k, v) for k, v in sd.items() if not k.startswith(_BRANCH_PREFIXES + ("compute_features.",)))
            if not sub:
                raise ValueError(f"{model}: the checkpoint holds no '{prefix}*' tensors" if prefix else
                                 f"{model}: the checkpoint holds no head tensors (bn_before_agg.*, attention.*, bn_final.*, fc.*)")
            write_blob(str(dst) + suffix, branch, sub)
            total += len(sub)
        return total
    if any(k.startswith(_BRANCH_PREFIXES) for k in sd):
        raise ValueError("this is a fusion checkpoint (ECAPA_TDNN.* / rawnet2v2.* / rawnet.* / titaNet.* / RawNet.* keys): convert it with "
                         f"model= one of {sorted(FUSION_MODELS)} (one blob per branch)")
    mid = model_id(model)
    if mid in (_lib.MODEL_RAWNET2, _lib.MODEL_RAWNET2_CONV) and any(k.startswith("gru.") for k in sd):
        raise ValueError(f"{model}: the checkpoint aggregates with a GRU (gru.*): convert it as RawNet2_custom_gru")
    if mid == _lib.MODEL_RAWNET2_GRU and any(k.startswith("attention.") for k in sd):
        raise ValueError(f"{model}: the checkpoint aggregates with attentive statistics pooling (attention.*), not a GRU")
    write_blob(dst, model, sd)
    return len(sd)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--model", default="ECAPA_TDNN", help="reference model name (ECAPA_TDNN, RawNet2_custom, RawNet2_custom_conv, RawNet2_custom_gru, "
                    "RawNet3, TitaNet, Conformer, ResNetSE34V2, Raw_ECAPA_sinc_asp, Raw_ECAPA_sinc_gru, Raw_ECAPA, Raw_ECAPA_conv_asp, Raw_ECAPA_hype, Raw3_ECAPA, Tita_ECAPA, Raw_tita)")
    a = ap.parse_args(argv)
    n = convert_checkpoint(a.src, a.dst, a.model)
    print(f"{a.dst}: {n} tensors")


if __name__ == "__main__":
    main()
