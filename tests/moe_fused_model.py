"""Numpy model of the fused MoE decode entries (gq_mmq_id_glu, gq_moe_combine): what they are
defined to return from fp16 inputs, and the fp16 ulp distance the tests measure with."""
import numpy as np


def glu(g16, u16):
    """fp16(silu(g) * u) from fp16 g, u, evaluated in float64 and rounded once (the ideal the
    entry's fp32 evaluation is held to within 1 ulp16)."""
    g = np.asarray(g16, dtype=np.float16).astype(np.float64)
    u = np.asarray(u16, dtype=np.float16).astype(np.float64)
    with np.errstate(over="ignore"):
        h = g / (1.0 + np.exp(-g)) * u
    with np.errstate(over="ignore"):
        return h.astype(np.float16)


def combine(D16, W):
    """gq_moe_combine's defined order exactly: acc = 0.f; for s in order acc = fl32(acc + fl32(w*d)),
    then one rounding to fp16.  D16 (N, S, M) fp16, W (N, S) fp16 or fp32 -> (N, M) fp16."""
    D = np.asarray(D16, dtype=np.float16).astype(np.float32)
    W = np.asarray(W)
    assert W.dtype in (np.float16, np.float32)
    W = W.astype(np.float32)
    N, S, M = D.shape
    acc = np.zeros((N, M), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(S):
            prod = (W[:, s, None] * D[:, s, :]).astype(np.float32)
            acc = (acc + prod).astype(np.float32)
        return acc.astype(np.float16)


def _ordered(a):
    """fp16 bit patterns mapped to integers that ascend with the value (-0 and +0 coincide)."""
    b = np.ascontiguousarray(np.asarray(a, dtype=np.float16)).view(np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7fff), b)


def ulp16(a, b):
    """Distance between a and b in steps of the ordered fp16 bit patterns (elementwise)."""
    return np.abs(_ordered(a) - _ordered(b))
