"""A numpy model of GGUF Q4_0 (GGML type 2), shared by the Q4_0 tests.

The reference project has no Q4_0, so the format is pinned here, from its definition
(include/gguf_mmq.h): a block is 32 weights in 18 bytes, little endian -- [0:2] d fp16 | [2:18] qs[16];
element j (0..15) has q = qs[j] & 15, element 16 + j has q = qs[j] >> 4, and w = d*(q - 8), exact in
fp32.  A Q4_0 block is a Q8_0 block with the same two d bytes and the int8 codes q - 8 in element
order (widen): that ties the format, the CPU product and the GPU tests' judge to the reference's
Q8_0 oracle bit for bit, with no code of this project in between.
"""
import numpy as np

import oracle as O
from type_models import BLAS_SHAPES, SPLITK_SHAPES, TIGHT_GEMM, TIGHT_GEMV, make_case, q81, rel_err, tight  # noqa: F401
from utils.synth import random_blocks

BYTES = 18


def _blocks(raw):
    raw = np.ascontiguousarray(np.asarray(raw).view(np.uint8)).reshape(-1)
    assert raw.size % BYTES == 0
    return raw.reshape(-1, BYTES)


def codes(raw):
    """(nblk, 32) int64 in -8..7, element order: the low nibbles of qs[0..15], then the high ones."""
    qs = _blocks(raw)[:, 2:].astype(np.int64)
    return np.concatenate([qs & 15, qs >> 4], axis=1) - 8


def widen(raw):
    """The Q8_0 image: per block the same two d bytes, then int8 q - 8 in element order (34 bytes).
    Exact: d*(q - 8) is the Q8_0 weight d*q8 of the image."""
    blk = _blocks(raw)
    out = np.empty((blk.shape[0], 34), np.uint8)
    out[:, 0:2] = blk[:, 0:2]
    out[:, 2:] = codes(raw).astype(np.int8).view(np.uint8)
    return out.reshape(-1)


def unpack(raw, M, K):
    """d fp32 (M, K/32); q int64 (M, K/32, 32) in -8..7."""
    blk = _blocks(raw)
    d = np.ascontiguousarray(blk[:, 0:2]).view(np.float16).astype(np.float32)
    return d.reshape(M, K // 32), codes(raw).reshape(M, K // 32, 32)


def dequant_f32(raw, M, K):
    """(M, K) fp32: d*(q - 8), exact."""
    d, q = unpack(raw, M, K)
    return (d[..., None].astype(np.float64) * q).astype(np.float32).reshape(M, K)


def ideal(raw, B, M, N, K):
    """The judge: the reference's Q8_0 oracle on the widened blocks, exact products of the oracle's
    q8_1 blocks, one rounding to fp16; (N, M) fp16."""
    return O.mmq_from_fp16("q8_0", widen(raw), np.ascontiguousarray(B), M, N, K, O.IDEAL)


def model_decode(raw, B, M, N, K):
    """The decode / GEMV order: per block (d*dB)*i in fp32 with i the exact integer dot product, the
    blocks added in fp32, one rounding to fp16.  (The lanes' summation tree is not modelled: fp32
    sums of at most K/32 terms differ from it by a few fp32 ulps.)"""
    d, q = unpack(raw, M, K)
    xd, _, xq = q81(B)
    i = np.einsum("mbl,nbl->nmb", q, xq).astype(np.float32)
    t = ((d[None] * xd[:, None]).astype(np.float32) * i).astype(np.float32)
    return t.sum(axis=2, dtype=np.float32).astype(np.float16)


def model_mfma(raw, B, M, N, K):
    """The MFMA paths' roundings: fp16 d times the exact code rounded once to fp16 per weight, fp16
    x~ = dB*qB, fp32 sums, fp16 output."""
    d, q = unpack(raw, M, K)
    w = (d[..., None].astype(np.float64) * q).astype(np.float16).astype(np.float32).reshape(M, K)
    xd, _, xq = q81(B)
    xt = (xd[..., None] * xq.astype(np.float32)).astype(np.float16).astype(np.float32).reshape(N, K)
    return (xt @ w.T).astype(np.float32).astype(np.float16)


def pack(d16, q):
    """fp16 d (nblk,) and codes 0..15 (nblk, 32) in element order -> packed bytes."""
    q = np.asarray(q).astype(np.uint8)
    out = np.empty((q.shape[0], BYTES), np.uint8)
    out[:, 0:2] = np.asarray(d16, np.float16).reshape(-1, 1).view(np.uint8)
    out[:, 2:] = q[:, :16] | (q[:, 16:] << 4)
    return out.reshape(-1)


def naive_quantize(x):
    """The yardstick quantizer, (nblk, 32) fp32 -> packed bytes: d = amax / 7, the nearest code,
    clamped to -7..7 (code -8 unused); d stored as fp16."""
    x = np.asarray(x, np.float32).reshape(-1, 32)
    d = np.abs(x).max(axis=1) / np.float32(7)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d[:, None] > 0, np.rint(x / d[:, None]), 0)
    return pack(d.astype(np.float16), np.clip(q, -7, 7).astype(np.int64) + 8)


def new_rule_quantize(x):
    """The rule of gq_quantize_q4_0 (include/gguf_quant.h) restated in numpy, fp32 throughout:
    d = m / -8 with m the block's element of largest magnitude (the first of equals), sign kept;
    id = d ? 1/d : 0; code min(15, trunc(x*id + 8.5)); d stored as fp16."""
    x = np.asarray(x, np.float32).reshape(-1, 32)
    m = x[np.arange(x.shape[0]), np.abs(x).argmax(axis=1)]
    d = (m / np.float32(-8)).astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, np.float32(1) / d, np.float32(0)).astype(np.float32)
    v = ((x * inv[:, None]).astype(np.float32) + np.float32(8.5)).astype(np.float32)
    return pack(d.astype(np.float16), np.minimum(15, np.trunc(v).astype(np.int64)))


# ---- the GPU tests' inputs (the CPU model test checks the same ones) ----
# Routes: 1..4 tokens the streaming decode at any K % 32 == 0 while the tokens' q8_1 image (Q8_0's:
# the codes over K rounded up to 64, and a d per block) fits the 48 KiB of LDS beside the ring, else
# act_quant + gemv_kernel; from 5 tokens the GEMV where K % 256 != 0 (Q8_0's rule: the GEMMs work on
# whole 256-element groups; 5..8 such tokens still fit the decode kernel's two token groups), the
# streaming GEMM otherwise.  At four tokens the image is 4*(ceil(K/64)*64 + K/8) bytes: K = 10880 is
# 48960 bytes, the last K on the decode, K = 10912 (49232) the first on the GEMV
# (test_gpu_q4_0.py asserts both routes).  K = 28672 at one token: seven cached chunks per lane.
DECODE_SHAPES = [(1, 1, 32), (5, 3, 96), (63, 2, 160), (65, 4, 1024), (96, 1, 2848), (16, 4, 10880), (8, 1, 28672)]
GEMV_SHAPES = [(32, 4, 11008), (16, 4, 10912), (70, 16, 160), (33, 130, 1120)]
GEMM_SHAPES = [(130, 5, 256), (7, 8, 512), (70, 16, 512), (129, 17, 768), (64, 64, 1024), (200, 130, 512)]
ALL_SHAPES = DECODE_SHAPES + GEMV_SHAPES + GEMM_SHAPES + SPLITK_SHAPES + BLAS_SHAPES


case = make_case("q4_0", ideal)  # (the oracle's ideal, fp16)


def edge_blocks(M, K, seed=0):
    """M rows of K weights with edge-valued codes: the first third of the rows every nibble 0 (code
    -8), the second third every nibble 15 (+7), the rest blocks of 0 and of 15 in turn; d as
    random_blocks gives it."""
    blk = _blocks(random_blocks("q4_0", M, K, seed=seed)).copy().reshape(M, K // 32, BYTES)
    a, b = M // 3, 2 * (M // 3)
    blk[:a, :, 2:] = 0x00
    blk[a:b, :, 2:] = 0xFF
    blk[b:, 0::2, 2:] = 0x00
    blk[b:, 1::2, 2:] = 0xFF
    return blk.reshape(-1)
