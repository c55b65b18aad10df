"""Q4_0-Q8_1 CPU MMQ (no counterpart in the reference).

C = (A @ B.T).T with A packed Q4_0 (18 B per 32 weights, M rows), B packed q8_1 (N rows); returns
the (N, M) transposed view of an (M, N) fp16 tensor.  A Q4_0 block is a Q8_0 block with the same d
and the int8 codes nibble - 8, and the product is mmq_q8_0_q8_1_cpu's on that image, bit for bit:
per block fp16(fp16(dA*dB) * i) with i the exact integer dot product, added to the fp16 running sum
in block order (csrc/quant/gguf_cpu_mmq.cpp).
"""
import torch

from ._cpu import cpu_mmq


def mmq_q4_0_q8_1_cpu(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int, threads: int = 0):
    assert K % 32 == 0
    assert A.dtype == torch.int8
    assert B.dtype == torch.int8
    assert A.numel() == M * K / 32 * 18
    assert B.numel() == N * K / 32 * 36
    return cpu_mmq(6, A, B, M, N, K, threads)
