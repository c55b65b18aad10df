"""Synthetic packed GGUF weights for benchmarks and size-independent parity tests.

Random bytes are valid blocks for every format except where a byte pair is an fp16 scale,
so those fields are overwritten with fp16(U(0.5, 1.5) * 2^-7); Q6_K's
int8 sub-block scales and Q3_K's 6-bit ones stay uniformly random (including negative ones), as do
Q2_K's 4-bit scales and mins (d at bytes 80..81, dmin at 82..83).  Q4_0 (d at bytes 0..1, as
Q8_0) keeps its random nibbles: uniform over 0..15, so the codes -8 and +7 occur.  The kernels have
no data-dependent control flow, so timings do not depend on the values.
"""
from __future__ import annotations

import numpy as np

from gguf.blocks import BLOCK  # noqa: F401  (re-exported: utils.synth.BLOCK)


def _scales(rng, n):
    return (rng.uniform(0.5, 1.5, size=n) * 2.0 ** -7).astype(np.float16).view(np.uint16)


def random_blocks(fmt: str, M: int, K: int, seed: int = 0) -> np.ndarray:
    """uint8 array of M rows of packed `fmt` blocks covering K elements each."""
    qk, nbytes = BLOCK[fmt]
    assert K % qk == 0
    nb = M * (K // qk)
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(nb, nbytes), dtype=np.uint8)
    u16 = raw.view(np.uint8)
    if fmt in ("q8_0", "q4_0"):
        d = _scales(rng, nb)
        u16[:, 0] = d & 0xFF
        u16[:, 1] = d >> 8
    elif fmt in ("q4_k", "q5_k"):
        d, dm = _scales(rng, nb), _scales(rng, nb)
        u16[:, 0], u16[:, 1] = d & 0xFF, d >> 8
        u16[:, 2], u16[:, 3] = dm & 0xFF, dm >> 8
    elif fmt == "q3_k":
        d = _scales(rng, nb)
        u16[:, 108], u16[:, 109] = d & 0xFF, d >> 8
    elif fmt == "q2_k":
        d, dm = _scales(rng, nb), _scales(rng, nb)
        u16[:, 80], u16[:, 81] = d & 0xFF, d >> 8
        u16[:, 82], u16[:, 83] = dm & 0xFF, dm >> 8
    else:
        d = _scales(rng, nb)
        u16[:, 208], u16[:, 209] = d & 0xFF, d >> 8
    return raw.reshape(-1)


def random_activations(N: int, K: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed + 12345)
    return rng.standard_normal((N, K), dtype=np.float32).astype(np.float16)
