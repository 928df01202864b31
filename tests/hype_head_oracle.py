"""float64 numpy restatement of the attention head of the reference's Raw_ECAPA_hype (models/Raw_ECAPA_hype.py:65-85, eval mode): what
the GPU tests of the head kernel compare against, itself checked against the reference's own fp32 output (tests/test_hype_host.py)."""
import numpy as np


def _bn(x, sd, p, eps=1e-5):
    f = lambda k: np.asarray(sd[p + "." + k], np.float64)
    return (x - f("running_mean")) / np.sqrt(f("running_var") + eps) * f("weight") + f("bias")


def head_forward(sd, e1, e2, return_weights=False):
    """sd: the 21 head tensors (numpy); e1 (B, 192), e2 (B, 512) -> (B, nOut) float64; return_weights: and the softmax weights (B, 704)"""
    f = lambda k: np.asarray(sd[k], np.float64)
    x = _bn(np.concatenate([np.asarray(e1, np.float64), np.asarray(e2, np.float64)], axis=-1), sd, "bn_before_agg")
    x = np.where(x > 0, x, 0.3 * x)                                               # LeakyReLU(0.3)
    a = x @ f("attention.0.weight")[:, :, 0].T + f("attention.0.bias")           # Conv1d(704, 128, 1) on a time axis of length 1
    with np.errstate(over="ignore"):
        a = a / (1.0 + np.exp(-a))                                                # SiLU
    a = _bn(a, sd, "attention.2")
    z = a @ f("attention.3.weight")[:, :, 0].T + f("attention.3.bias")
    z = z - z.max(axis=1, keepdims=True)                                          # Softmax(dim=1): over the 704 channels
    w = np.exp(z)
    w /= w.sum(axis=1, keepdims=True)
    m = x * w
    s = np.sqrt(np.maximum(x * x * w - m * m, 1e-9))
    p = _bn(np.concatenate([m, s], axis=1), sd, "bn_final")
    out = p @ f("fc.weight").T + f("fc.bias")
    return (out, w) if return_weights else out
