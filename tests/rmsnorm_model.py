"""The numpy model of gq_rmsnorm (tests/test_rmsnorm_host.py, test_gpu_rmsnorm.py).

h is the kernel's own definition and exact: fp16(float(x) + float(r)) -- fp32 holds the sum of two
fp16 values closely enough that the one rounding to fp16 is the sum's correct rounding.  y_ideal is
what the kernel approximates in fp32: float64(h) / sqrt(mean(h^2) + float64(float32(eps))) *
float64(w), rounded once to fp16.  ulp_dist counts fp16 values between two results."""
import numpy as np


def h_of(x, r=None):
    """fp16 (N, K): x itself without a residual, else the correctly rounded sum."""
    x = np.asarray(x)
    assert x.dtype == np.float16
    if r is None:
        return x.copy()
    r = np.asarray(r)
    assert r.dtype == np.float16 and r.shape == x.shape
    return (x.astype(np.float32) + r.astype(np.float32)).astype(np.float16)


def y_ideal(h, w, eps):
    """fp16 (N, K) from fp16 h (N, K), fp32 w (K,) and eps, evaluated in fp64."""
    h, w = np.asarray(h), np.asarray(w)
    assert h.dtype == np.float16 and w.dtype == np.float32
    h64 = h.astype(np.float64)
    ms = np.mean(h64 * h64, axis=1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return (h64 / np.sqrt(ms + np.float64(np.float32(eps))) * w.astype(np.float64)[None, :]).astype(np.float16)


def _ordered(a):
    """fp16 bit patterns as integers that order like the values (sign-magnitude -> two's complement;
    -0 and +0 both map to 0)."""
    b = np.asarray(a).view(np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def ulp_dist(a, b):
    """Element-wise count of fp16 steps between a and b (int64; 0 where the bits agree or both are
    zeros of either sign)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float16 and b.dtype == np.float16 and a.shape == b.shape
    return np.abs(_ordered(a) - _ordered(b))
