"""An independent numpy model of GGUF Q2_K (GGML type 10), shared by the Q2_K tests.

The reference project has no Q2_K, so the format is pinned here, from its definition
(include/gguf_mmq.h): a super-block is 256 weights in 84 bytes, little endian --
[0:16] scales[16] | [16:80] qs[64] | [80:82] d fp16 | [82:84] dmin fp16; for element e,
h = e / 128, j = (e % 128) / 32, l = e % 32, s = e / 16:
    q  = (qs[32*h + l] >> 2*j) & 3          (0..3)
    sc = scales[s] & 15,  m = scales[s] >> 4 (0..15)
    w  = d*sc*q - dmin*m
d*sc*q and dmin*m are exact in fp32 (an 11-bit significand times at most 4 + 2 bits), so the fp32
weight is the difference rounded once.  A Q2_K super-block is the difference of two Q6_K
super-blocks, both exact (split_q6_k): W1 carries d, the scales and the codes, W2 carries dmin and
the mins under the constant code 1.  That ties the format to the reference's Q6_K oracle with no
code of this project in between.
"""
import numpy as np

from type_models import (ALL_SHAPES, BLAS_SHAPES, DECODE_SHAPES, GEMM_SHAPES, GEMV_SHAPES, LONG_SHAPES,  # noqa: F401
                         SPLITK_SHAPES, TIGHT_GEMM, TIGHT_GEMV, make_case, pack_q6_k, q81, rel_err, tight)

BYTES = 84


def unpack(raw, M, K):
    """d, dmin fp32 (M, nsb); sc, m int (M, nsb, 16) in 0..15; q int (M, nsb, 256) in 0..3."""
    blk = np.ascontiguousarray(np.asarray(raw).view(np.uint8).reshape(M, K // 256, BYTES))
    dd = np.ascontiguousarray(blk[..., 80:84]).view(np.float16).astype(np.float32)
    s = blk[..., 0:16].astype(np.int64)
    qs = blk[..., 16:80].astype(np.int64)
    q = np.empty(blk.shape[:2] + (256,), np.int64)
    for h in range(2):
        for j in range(4):
            e0 = 128 * h + 32 * j
            q[..., e0:e0 + 32] = (qs[..., 32 * h:32 * h + 32] >> (2 * j)) & 3
    return dd[..., 0], dd[..., 1], s & 15, s >> 4, q


def dequant_exact(raw, M, K):
    """(M, K) fp64: d*sc*q - dmin*m, exact (multiples of 2^-24 below 2^46)."""
    d, dmin, sc, m, q = unpack(raw, M, K)
    ds = np.repeat(d.astype(np.float64)[..., None] * sc, 16, axis=-1)
    dm = np.repeat(dmin.astype(np.float64)[..., None] * m, 16, axis=-1)
    return (ds * q - dm).reshape(M, K)


def dequant_f32(raw, M, K):
    """(M, K) fp32: the exact weight rounded once."""
    return dequant_exact(raw, M, K).astype(np.float32)


def split_q6_k(raw):
    """(W1, W2), two Q6_K tensors with W = W1 - W2, both parts exact: W1 has d6 = d, int8
    sc6 = sc and codes q + 32 (so d*sc*q); W2 has d6 = dmin, sc6 = m and every code 33 (dmin*m)."""
    raw = np.asarray(raw).view(np.uint8)
    nblk = raw.size // BYTES
    blk = raw.reshape(nblk, BYTES)
    _, _, sc, m, q = unpack(raw, 1, 256 * nblk)
    w1 = pack_q6_k(blk[:, 80:82], sc[0], q[0] + 32)
    w2 = pack_q6_k(blk[:, 82:84], m[0], np.full((nblk, 256), 33, np.int64))
    return w1, w2


def ideal(raw, B, M, N, K):
    """x~ @ W^T in fp64, x~ = d*q of the oracle's q8_1 blocks; (N, M) float64."""
    d, _, q = q81(B)
    xt = (d.astype(np.float64)[..., None] * q).reshape(N, K)
    return xt @ dequant_exact(raw, M, K).T


def model_mfma(raw, B, M, N, K):
    """The MFMA path's roundings: fp16 d*sc, fp16 -(dmin*m), one fp16 fma per weight on the exact
    code, fp16 x~, fp32 sums, fp16 output."""
    d, dmin, sc, m, q = unpack(raw, M, K)
    ds = (d[..., None] * sc.astype(np.float32)).astype(np.float16).astype(np.float64)
    dm = (dmin[..., None] * m.astype(np.float32)).astype(np.float16).astype(np.float64)
    w = (np.repeat(ds, 16, axis=-1) * q - np.repeat(dm, 16, axis=-1)).astype(np.float16)  # (exact in fp64, one rounding)
    w = w.astype(np.float32).reshape(M, K)
    xd, _, xq = q81(B)
    xt = (xd[..., None] * xq.astype(np.float32)).astype(np.float16).astype(np.float32).reshape(N, K)
    return (xt @ w.T).astype(np.float32).astype(np.float16)


def _sums(raw, B, M, N, K):
    """d*sc, dmin*m as fp32 (M, K/16); dB fp32 (N, K/32); i, sigma as fp32 (N, M, K/16), (N, K/16)."""
    d, dmin, sc, m, q = unpack(raw, M, K)
    nh = K // 16
    ds = (d[..., None] * sc.astype(np.float32)).astype(np.float32).reshape(M, nh)
    dm = (dmin[..., None] * m.astype(np.float32)).astype(np.float32).reshape(M, nh)
    xd, _, xq = q81(B)
    xq = xq.reshape(N, nh, 16)
    idot = np.einsum("mbl,nbl->nmb", q.reshape(M, nh, 16), xq).astype(np.float32)
    return ds, dm, xd, idot, xq.sum(axis=-1).astype(np.float32)


def model_decode(raw, B, M, N, K):
    """The decode / GEMV path: per 16 elements (d*sc)*i - (dmin*m)*sigma in fp32, the block's two
    halves added, times dB, fp32 sums over the blocks, fp16 output."""
    ds, dm, xd, idot, sig = _sums(raw, B, M, N, K)
    t = ((ds[None] * idot).astype(np.float32) - (dm[None] * sig[:, None]).astype(np.float32)).astype(np.float32)
    t = t.reshape(N, M, K // 32, 2)
    t = (t[..., 0] + t[..., 1]).astype(np.float32) * xd[:, None, :]
    return t.astype(np.float32).sum(axis=2, dtype=np.float32).astype(np.float16)


def model_cpu(raw, B, M, N, K):
    """gq_cpu_mmq type 5, operation for operation (csrc/quant/gguf_cpu_mmq.cpp): per q8_1 block
    p = (d*sc_lo)*i_lo + (d*sc_hi)*i_hi, s = (dmin*m_lo)*sig_lo + (dmin*m_hi)*sig_hi,
    term = dB*p - dB*s, every operation one fp32 rounding; C = fp16(fp32(C) + fp32(fp16(term)))
    in block order.  (N, M) fp16."""
    f = np.float32
    ds, dm, xd, idot, sig = _sums(raw, B, M, N, K)
    nb = K // 32
    ds, dm = ds.reshape(M, nb, 2), dm.reshape(M, nb, 2)
    idot, sig = idot.reshape(N, M, nb, 2), sig.reshape(N, nb, 2)
    c = np.zeros((N, M), np.float16)
    for j in range(nb):
        p = ((ds[None, :, j, 0] * idot[:, :, j, 0]).astype(f) + (ds[None, :, j, 1] * idot[:, :, j, 1]).astype(f)).astype(f)
        s = ((dm[None, :, j, 0] * sig[:, None, j, 0]).astype(f) + (dm[None, :, j, 1] * sig[:, None, j, 1]).astype(f)).astype(f)
        dB = xd[:, j][:, None]
        t = ((dB * p).astype(f) - (dB * s).astype(f)).astype(f)
        c = (c.astype(f) + t.astype(np.float16).astype(f)).astype(f).astype(np.float16)
    return c


def naive_quantize(x):
    """The yardstick quantizer, (nblk, 256) fp32 -> packed bytes: per 16 elements m = max(0, -min x)
    and scale = (max x + m) / 3; the sixteen scales and the sixteen mins to 4 bits against the
    largest of each (d = max scale / 15, dmin = max min / 15); then the nearest code."""
    x = np.asarray(x, np.float32).reshape(-1, 16, 16)
    nblk = x.shape[0]
    mn = np.maximum(0, -x.min(axis=-1))
    scale = (x.max(axis=-1) + mn) / 3
    smax, mmax = scale.max(axis=-1), mn.max(axis=-1)
    d, dmin = (smax / 15).astype(np.float16), (mmax / 15).astype(np.float16)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.where(smax[:, None] > 0, np.rint(15 * scale / smax[:, None]), 0)
        m = np.where(mmax[:, None] > 0, np.rint(15 * mn / mmax[:, None]), 0)
        sc, m = np.clip(sc, 0, 15).astype(np.int64), np.clip(m, 0, 15).astype(np.int64)
        es, em = d.astype(np.float32)[:, None] * sc, dmin.astype(np.float32)[:, None] * m
        q = np.where(es[..., None] != 0, np.rint((x + em[..., None]) / np.where(es == 0, 1, es)[..., None]), 0)
    q = np.clip(q, 0, 3).astype(np.uint8).reshape(nblk, 256)
    out = np.zeros((nblk, BYTES), np.uint8)
    out[:, 0:16] = (sc | (m << 4)).astype(np.uint8)
    for h in range(2):
        for j in range(4):
            out[:, 16 + 32 * h:48 + 32 * h] |= q[:, 128 * h + 32 * j:128 * h + 32 * j + 32] << (2 * j)
    out[:, 80:82] = d.view(np.uint8).reshape(nblk, 2)
    out[:, 82:84] = dmin.view(np.uint8).reshape(nblk, 2)
    return out.reshape(-1)


# ---- the GPU tests' inputs: the shared K % 256 lists, which are Q3_K's (tests/type_models.py) ----


case = make_case("q2_k", ideal)  # (the fp64 ideal)
