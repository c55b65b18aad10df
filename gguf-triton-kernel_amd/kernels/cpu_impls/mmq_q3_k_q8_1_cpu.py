"""Q3_K-Q8_1 CPU MMQ (no counterpart in the reference).

C = (A @ B.T).T with A packed Q3_K (110 B per 256 weights, M rows), B packed q8_1 (N rows);
returns the (N, M) transposed view of an (M, N) fp16 tensor: mmq_q6_k_q8_1_cpu's terms and fp16
running sum in block order over the codes -4..3 and 6-bit scales.
"""
import torch

from ._cpu import cpu_mmq


def mmq_q3_k_q8_1_cpu(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int, threads: int = 0):
    assert K % 256 == 0
    assert A.dtype == torch.int8
    assert B.dtype == torch.int8
    assert A.numel() == M * K / 256 * 110
    assert B.numel() == N * K / 32 * 36
    return cpu_mmq(4, A, B, M, N, K, threads)
