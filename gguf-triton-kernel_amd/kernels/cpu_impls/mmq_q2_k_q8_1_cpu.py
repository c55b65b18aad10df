"""Q2_K-Q8_1 CPU MMQ (no counterpart in the reference).

C = (A @ B.T).T with A packed Q2_K (84 B per 256 weights, M rows), B packed q8_1 (N rows);
returns the (N, M) transposed view of an (M, N) fp16 tensor.  Per q8_1 block, from exact integer
sums over its two 16-element halves, dB*((d*sc_lo)*i_lo + (d*sc_hi)*i_hi) -
dB*((dmin*m_lo)*sigma_lo + (dmin*m_hi)*sigma_hi), added to the others' fp16 running sum in block
order (csrc/quant/gguf_cpu_mmq.cpp gives the order of the fp32 operations).
"""
import torch

from ._cpu import cpu_mmq


def mmq_q2_k_q8_1_cpu(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int, threads: int = 0):
    assert K % 256 == 0
    assert A.dtype == torch.int8
    assert B.dtype == torch.int8
    assert A.numel() == M * K / 256 * 84
    assert B.numel() == N * K / 32 * 36
    return cpu_mmq(5, A, B, M, N, K, threads)
