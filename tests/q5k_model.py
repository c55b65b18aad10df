"""An independent numpy model of GGUF Q5_K (GGML type 13), shared by the Q5_K tests.

The reference project has no Q5_K, so the format is pinned here, from its definition
(include/gguf_mmq.h): a super-block is 256 weights in 176 bytes, little endian --
[0:2] d fp16 | [2:4] dmin fp16 | [4:16] 12 scale bytes (Q4_K's get_scale_min_k4) | [16:48] qh[32] |
[48:176] qs[128]; for element e, j = e / 32, l = e % 32:
    q = ((qs[32*(j/2) + l] >> 4*(j&1)) & 15) + 16*((qh[l] >> j) & 1)      (0..31)
    w = d*sc_j*q - dmin*m_j
"""
import numpy as np

import type_models as TM
from type_models import (BLAS_SHAPES, GEMM_SHAPES, LONG_SHAPES, SPLITK_SHAPES, TIGHT_GEMM, TIGHT_GEMV,  # noqa: F401
                         make_case, q81, rel_err, tight)

BYTES = 176


def unpack(raw, M, K):
    """(d, dmin) fp32 (M, nsb); (sc, m) int (M, nsb, 8); q int (M, nsb, 8, 32)."""
    blk = np.ascontiguousarray(np.asarray(raw).view(np.uint8).reshape(M, K // 256, BYTES))
    hdr = np.ascontiguousarray(blk[..., 0:4]).view(np.float16).astype(np.float32)
    d, dmin = hdr[..., 0], hdr[..., 1]
    s = blk[..., 4:16].astype(np.int64)
    sc = np.empty(blk.shape[:2] + (8,), np.int64)
    mn = np.empty_like(sc)
    for j in range(8):
        if j < 4:
            sc[..., j] = s[..., j] & 63
            mn[..., j] = s[..., j + 4] & 63
        else:
            sc[..., j] = (s[..., j + 4] & 15) | ((s[..., j - 4] >> 6) << 4)
            mn[..., j] = (s[..., j + 4] >> 4) | ((s[..., j] >> 6) << 4)
    qh = blk[..., 16:48].astype(np.int64)
    qs = blk[..., 48:176].astype(np.int64)
    q = np.empty(blk.shape[:2] + (8, 32), np.int64)
    for j in range(8):
        q[..., j, :] = ((qs[..., 32 * (j // 2):32 * (j // 2) + 32] >> (4 * (j & 1))) & 15) + 16 * ((qh >> j) & 1)
    return d, dmin, sc, mn, q


def dequant_f32(raw, M, K):
    """(M, K) fp32: (d*sc)*q - (dmin*m), every operation rounded to fp32 on its own."""
    d, dmin, sc, mn, q = unpack(raw, M, K)
    ds = (d[..., None] * sc.astype(np.float32)).astype(np.float32)
    dm = (dmin[..., None] * mn.astype(np.float32)).astype(np.float32)
    w = (ds[..., None] * q.astype(np.float32)).astype(np.float32) - dm[..., None]
    return w.astype(np.float32).reshape(M, K)


def ideal(raw, B, M, N, K):
    """x~ @ W^T in fp64, x~ = d*q of the q8_1 blocks; (N, M) float64."""
    d, _, q = q81(B)
    xt = (d.astype(np.float64)[..., None] * q).reshape(N, K)
    return xt @ dequant_exact(raw, M, K).T


def dequant_exact(raw, M, K):
    d, dmin, sc, mn, q = unpack(raw, M, K)
    d, dmin = d.astype(np.float64), dmin.astype(np.float64)
    return ((d[..., None] * sc)[..., None] * q - (dmin[..., None] * mn)[..., None]).reshape(M, K)


def model_mfma(raw, B, M, N, K):
    """The MFMA path's roundings: fp16 d*sc, fp16 -(dmin*m), one fp16 fma per weight, fp16 x~, fp32
    sums, fp16 output."""
    d, dmin, sc, mn, q = unpack(raw, M, K)
    ds = (d[..., None] * sc.astype(np.float32)).astype(np.float16).astype(np.float64)
    ndm = (-(dmin[..., None] * mn.astype(np.float32))).astype(np.float16).astype(np.float64)
    w = (q * ds[..., None] + ndm[..., None]).astype(np.float16).astype(np.float32).reshape(M, K)  # exact, then once
    xd, _, xq = q81(B)
    xt = (xd[..., None] * xq.astype(np.float32)).astype(np.float16).astype(np.float32).reshape(N, K)
    return (xt @ w.T).astype(np.float32).astype(np.float16)


def model_decode(raw, B, M, N, K):
    """The decode / GEMV path: per 32-block d*sc*dB*idot - dmin*m*sB in fp32, fp32 sums, fp16 output."""
    d, dmin, sc, mn, q = unpack(raw, M, K)
    nb = K // 32
    ds = (d[..., None] * sc.astype(np.float32)).astype(np.float32).reshape(M, nb)
    dm = (dmin[..., None] * mn.astype(np.float32)).astype(np.float32).reshape(M, nb)
    xd, xs, xq = q81(B)
    idot = np.einsum("mbl,nbl->nmb", q.reshape(M, nb, 32), xq).astype(np.float32)
    t = ds[None] * xd[:, None, :] * idot - dm[None] * xs[:, None, :]
    return t.astype(np.float32).sum(axis=2, dtype=np.float32).astype(np.float16)


# ---- the GPU tests' inputs (the CPU model test checks the same ones): the shared K % 256 lists
# without the two shapes at Q3_K's four-token limit (tests/type_models.py) ----
DECODE_SHAPES = [s for s in TM.DECODE_SHAPES if s != (16, 4, 8704)]
GEMV_SHAPES = [s for s in TM.GEMV_SHAPES if s != (16, 4, 8960)]
ALL_SHAPES = DECODE_SHAPES + LONG_SHAPES + GEMV_SHAPES + GEMM_SHAPES + SPLITK_SHAPES + BLAS_SHAPES


case = make_case("q5_k", ideal)  # (the fp64 ideal)
