"""What the numpy models of the added block types (tests/q5k_model.py, q3k_model.py, q2k_model.py,
q4_0_model.py) share: the gates, the q8_1 activation blocks, the Q6_K re-packer, the K % 256 shape
lists, the builder of a shape's inputs, and the one table of which function judges which type.
Each model re-exports these names, so `Q.tight`, `Q.case`, `Q.ALL_SHAPES` read as before."""
import functools
import importlib

import numpy as np

import oracle as O
from utils.synth import random_activations, random_blocks

TIGHT_GEMV = 1.5e-3
TIGHT_GEMM = 4e-3


def tight(N):
    return TIGHT_GEMV if N <= 4 else TIGHT_GEMM


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def q81(B):
    """The oracle's q8_1 quantizer on fp16 (N, K): d, s as fp32 (N, K/32); codes int (N, K/32, 32)."""
    N, K = B.shape
    blk = O.quantize_q8_1(np.ascontiguousarray(B)).reshape(N, K // 32, 36)
    ds = np.ascontiguousarray(blk[..., 0:4]).view(np.float16).astype(np.float32)
    return ds[..., 0], ds[..., 1], blk[..., 4:].view(np.int8).astype(np.int64)


def pack_q6_k(d_bytes, sc, codes):
    """Q6_K super-blocks (210 B) with fp16 d bytes (nblk, 2), int8 scales (nblk, 16) and 6-bit
    codes (nblk, 256) at Q6_K's positions: ql nibble (e%128)/64 of byte 64*(e/128) + e%64, qh bits
    2*((e%128)/32) of byte 32*(e/128) + e%32."""
    nblk = codes.shape[0]
    out = np.zeros((nblk, 210), np.uint8)
    c = codes.astype(np.uint8)
    for h in range(2):
        for j in range(4):
            e0 = 128 * h + 32 * j
            ce = c[:, e0:e0 + 32]
            lo = 64 * h + 32 * (j & 1)
            out[:, lo:lo + 32] |= (ce & 15) << (4 * (j >> 1))
            out[:, 128 + 32 * h:128 + 32 * h + 32] |= (ce >> 4) << (2 * j)
    out[:, 192:208] = sc.astype(np.int8).view(np.uint8)
    out[:, 208:210] = d_bytes
    return out.reshape(-1)


# ---- the GPU tests' inputs of the K % 256 types (the CPU model tests check the same ones) ----
# These are Q3_K's and Q2_K's lists.  Their streaming decode keeps codes, d and the two per-16 code
# sums of every token in LDS beside the 112 KiB ring: 1.375 K bytes per token in the 48 KiB left.
# Four tokens fit up to K = 8936: (16, 4, 8704) is the last multiple of 256 on the decode,
# (16, 4, 8960) the first on the GEMV.  One token of K = 16640 fits (five cached units per lane);
# 3 tokens of 16384 and 2 of 28672 do not (they would run as two token groups) and take the GEMV,
# as do 4 tokens of 11008.  Q5_K's image is 1.25 K bytes per token, so its own threshold (K = 9830)
# lies above both of those shapes: its lists are these without them (tests/q5k_model.py).  Q4_0
# (K % 32) has its own decode, GEMV and GEMM lists and shares the last two.
DECODE_SHAPES = [(1, 1, 256), (5, 3, 512), (63, 2, 768), (65, 4, 1024), (96, 1, 2816), (16, 4, 8704)]
LONG_SHAPES = [(4, 1, 16640), (4, 3, 16384), (8, 2, 28672)]
GEMV_SHAPES = [(32, 4, 11008), (16, 4, 8960)]
GEMM_SHAPES = [(130, 5, 256), (7, 8, 512), (33, 9, 256), (70, 16, 512), (129, 17, 768), (64, 64, 1024),
               (200, 130, 512)]
SPLITK_SHAPES = [(256, 32, 4096), (300, 128, 2048)]
BLAS_SHAPES = [(65, 24, 1024), (130, 33, 256)]
ALL_SHAPES = DECODE_SHAPES + LONG_SHAPES + GEMV_SHAPES + GEMM_SHAPES + SPLITK_SHAPES + BLAS_SHAPES


def make_case(fmt, judge):
    """case(M, N, K) -> (packed `fmt` weights, fp16 activations, judge(raw, B, M, N, K)) of a shape:
    computed once, never written to."""
    @functools.lru_cache(maxsize=None)
    def case(M, N, K):
        raw = random_blocks(fmt, M, K, seed=M * 7 + N)
        B = random_activations(N, K, seed=K + N)
        want = judge(raw, B, M, N, K)
        for a in (raw, B, want):
            a.setflags(write=False)
        return raw, B, want
    return case


# type name -> (model module, its function): the fp64 model where the type has no exact image in a
# reference type, the reference's oracle on that image where it has one
_JUDGES = {"q5_k": ("q5k_model", "ideal"), "q3_k": ("q3k_model", "oracle_ideal"), "q2_k": ("q2k_model", "ideal"),
           "q4_0": ("q4_0_model", "ideal")}


def judge(fmt, raw, B, M, N, K):
    """The ideal (N, M) that the GPU tests hold `fmt` weights to: the table above for the added
    types, the oracle's IDEAL for the reference's own."""
    if fmt not in _JUDGES:
        return O.mmq_from_fp16(fmt, raw, B, M, N, K, O.IDEAL)
    module, name = _JUDGES[fmt]  # (by name: the models import this module)
    return getattr(importlib.import_module(module), name)(raw, B, M, N, K)
