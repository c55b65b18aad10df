"""Q4_0 x fp16 MMQ (no counterpart in the reference: GGML type 2, include/gguf_mmq.h).

A: packed Q4_0 blocks (18 B per 32 weights: fp16 d, then sixteen bytes of 4-bit codes -- element j
in the low nibble of byte j, element 16 + j in the high one; w = d*(code - 8)) as a flat int8 device
tensor of M*K/32*18 bytes; B: fp16 (N, K); returns fp16 (N, M) = (A @ B^T)^T.  K is any multiple of
32.  Runs in libgguf_mmq.so.
"""
import torch

from ._lib import GQ_Q4_0, mmq

Q4_0_BLOCK_SIZE = 18  # bytes
Q8_1_BLOCK_SIZE = 36  # bytes
QK4_0 = 32
QK8_1 = 32


def mmq_q4_0(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int) -> torch.Tensor:
    """out = (A @ B.T).T with A in Q4_0 (M rows), B fp16 (N, K); fp16 (N, M)."""
    assert (K % 32 == 0)
    return mmq(GQ_Q4_0, A, B, M, N, K)
