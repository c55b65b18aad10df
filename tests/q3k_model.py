"""An independent numpy model of GGUF Q3_K (GGML type 11), shared by the Q3_K tests.

The reference project has no Q3_K, so the format is pinned here, from its definition
(include/gguf_mmq.h): a super-block is 256 weights in 110 bytes, little endian --
[0:32] hmask[32] | [32:96] qs[64] | [96:108] scales[12] | [108:110] d fp16; for element e,
h = e / 128, j = (e % 128) / 32, l = e % 32, s = e / 16:
    q  = ((qs[32*h + l] >> 2*j) & 3) + 4*((hmask[l] >> (4*h + j)) & 1) - 4           (-4..3)
    sc = ((s < 8 ? scales[s] & 15 : scales[s-8] >> 4) | ((scales[8 + s%4] >> 2*(s/4)) & 3) << 4) - 32
    w  = d*sc*q
Q3_K has Q6_K's arithmetic (sixteen signed scales, one d, no mins), so a Q3_K super-block
re-encodes as a Q6_K super-block without loss (to_q6_k) and the reference's Q6_K oracle judges it.
"""
import numpy as np

import oracle as O
from type_models import (ALL_SHAPES, BLAS_SHAPES, DECODE_SHAPES, GEMM_SHAPES, GEMV_SHAPES, LONG_SHAPES,  # noqa: F401
                         SPLITK_SHAPES, TIGHT_GEMM, TIGHT_GEMV, make_case, pack_q6_k, q81, rel_err, tight)

BYTES = 110


def unpack(raw, M, K):
    """d fp32 (M, nsb); sc int (M, nsb, 16) in -32..31; q int (M, nsb, 256) in -4..3."""
    blk = np.ascontiguousarray(np.asarray(raw).view(np.uint8).reshape(M, K // 256, BYTES))
    d = np.ascontiguousarray(blk[..., 108:110]).view(np.float16).astype(np.float32)[..., 0]
    hm = blk[..., 0:32].astype(np.int64)
    qs = blk[..., 32:96].astype(np.int64)
    s = blk[..., 96:108].astype(np.int64)
    sc = np.empty(blk.shape[:2] + (16,), np.int64)
    for i in range(16):
        lo4 = (s[..., i] & 15) if i < 8 else (s[..., i - 8] >> 4)
        hi2 = (s[..., 8 + i % 4] >> (2 * (i // 4))) & 3
        sc[..., i] = (lo4 | (hi2 << 4)) - 32
    q = np.empty(blk.shape[:2] + (256,), np.int64)
    for h in range(2):
        for j in range(4):
            e0 = 128 * h + 32 * j
            q[..., e0:e0 + 32] = ((qs[..., 32 * h:32 * h + 32] >> (2 * j)) & 3) + 4 * ((hm >> (4 * h + j)) & 1) - 4
    return d, sc, q


def dequant_f32(raw, M, K):
    """(M, K) fp32: (d*sc)*q, every operation rounded to fp32 on its own."""
    d, sc, q = unpack(raw, M, K)
    ds = (d[..., None] * sc.astype(np.float32)).astype(np.float32)
    w = np.repeat(ds, 16, axis=-1) * q.astype(np.float32)
    return w.astype(np.float32).reshape(M, K)


def dequant_exact(raw, M, K):
    d, sc, q = unpack(raw, M, K)
    return (np.repeat(d.astype(np.float64)[..., None] * sc, 16, axis=-1) * q).reshape(M, K)


def to_q6_k(raw):
    """The same weights as Q6_K super-blocks (210 B): the same d, int8 scales = sc, 6-bit codes
    q + 32 at Q6_K's positions for the same element (type_models.pack_q6_k)."""
    raw = np.asarray(raw).view(np.uint8)
    nblk = raw.size // BYTES
    d, sc, q = unpack(raw, 1, 256 * nblk)
    return pack_q6_k(raw.reshape(nblk, BYTES)[:, 108:110], sc[0], q[0] + 32)  # (codes 28..35)


def ideal(raw, B, M, N, K):
    """x~ @ W^T in fp64, x~ = d*q of the q8_1 blocks; (N, M) float64."""
    d, _, q = q81(B)
    xt = (d.astype(np.float64)[..., None] * q).reshape(N, K)
    return xt @ dequant_exact(raw, M, K).T


def oracle_ideal(raw, B, M, N, K):
    """The judge of the GPU tests: the reference's Q6_K arithmetic on the transcoded blocks."""
    return O.mmq_from_fp16("q6_k", to_q6_k(raw), B, M, N, K, O.IDEAL)


def model_mfma(raw, B, M, N, K):
    """The MFMA path's roundings: fp16 d*sc, times the code in fp16, fp16 x~, fp32 sums, fp16 output."""
    d, sc, q = unpack(raw, M, K)
    ds = (d[..., None] * sc.astype(np.float32)).astype(np.float16).astype(np.float32)
    w = (np.repeat(ds, 16, axis=-1) * q.astype(np.float32)).astype(np.float16).astype(np.float32).reshape(M, K)
    xd, _, xq = q81(B)
    xt = (xd[..., None] * xq.astype(np.float32)).astype(np.float16).astype(np.float32).reshape(N, K)
    return (xt @ w.T).astype(np.float32).astype(np.float16)


def model_decode(raw, B, M, N, K):
    """The decode / GEMV path: per 32-block dB*((d*sc_lo)*idot_lo + (d*sc_hi)*idot_hi) in fp32, fp32
    sums, fp16 output."""
    d, sc, q = unpack(raw, M, K)
    nh = K // 16
    ds = (d[..., None] * sc.astype(np.float32)).astype(np.float32).reshape(M, nh)
    xd, _, xq = q81(B)
    idot = np.einsum("mbl,nbl->nmb", q.reshape(M, nh, 16), xq.reshape(N, nh, 16)).astype(np.float32)
    t = (ds[None] * idot).astype(np.float32).reshape(N, M, K // 32, 2)
    t = (t[..., 0] + t[..., 1]).astype(np.float32) * xd[:, None, :]
    return t.astype(np.float32).sum(axis=2, dtype=np.float32).astype(np.float16)


def naive_quantize(x):
    """The yardstick quantizer, (nblk, 256) fp32 -> packed bytes: per 16 elements the scale
    -peak/4 (peak = the element of largest magnitude, so it takes code -4), the sixteen scales to
    6 bits against the one of largest magnitude (which takes -32), then the nearest code."""
    x = np.asarray(x, np.float32).reshape(-1, 16, 16)
    nblk = x.shape[0]
    idx = np.argmax(np.abs(x), axis=-1)
    peak = np.take_along_axis(x, idx[..., None], axis=-1)[..., 0]
    sub = -peak / 4
    big = np.take_along_axis(sub, np.argmax(np.abs(sub), axis=-1)[:, None], axis=-1)[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(big != 0, -32.0 / big, 0.0)
        d = np.where(big != 0, 1.0 / inv, 0.0).astype(np.float16)
        sc = np.clip(np.rint(inv[:, None] * sub), -32, 31).astype(np.int64)
        eff = d.astype(np.float32)[:, None] * sc
        q = np.where(eff[..., None] != 0, np.rint(x / np.where(eff == 0, 1, eff)[..., None]), 0)
    q = np.clip(q, -4, 3).astype(np.int64).reshape(nblk, 256) + 4
    out = np.zeros((nblk, BYTES), np.uint8)
    v = (sc + 32).astype(np.uint8)
    for s in range(16):
        if s < 8:
            out[:, 96 + s] |= v[:, s] & 15
        else:
            out[:, 96 + s - 8] |= (v[:, s] & 15) << 4
        out[:, 96 + 8 + s % 4] |= (v[:, s] >> 4) << (2 * (s // 4))
    for h in range(2):
        for j in range(4):
            c = q[:, 128 * h + 32 * j:128 * h + 32 * j + 32].astype(np.uint8)
            out[:, 32 + 32 * h:64 + 32 * h] |= (c & 3) << (2 * j)
            out[:, 0:32] |= (c >> 2) << (4 * h + j)
    out[:, 108:110] = d.view(np.uint8).reshape(nblk, 2)
    return out.reshape(-1)


# ---- the GPU tests' inputs: the shared K % 256 lists (tests/type_models.py) ----


# the ideal as fp64: the reference's Q6_K arithmetic on the transcoded blocks (one final fp16
# rounding), not code of this project
case = make_case("q3_k", lambda *a: oracle_ideal(*a).astype(np.float64))
