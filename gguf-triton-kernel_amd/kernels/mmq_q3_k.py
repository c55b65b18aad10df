"""Q3_K x fp16 MMQ (no counterpart in the reference: GGML type 11, include/gguf_mmq.h).

A: packed Q3_K super-blocks (110 B per 256 weights: 32 bytes of high bits, 64 bytes of 2-bit
codes, 12 bytes of sixteen 6-bit scales, fp16 d) as a flat int8 device tensor of M*K/256*110
bytes; B: fp16 (N, K); returns fp16 (N, M) = (A @ B^T)^T.  Runs in libgguf_mmq.so.
"""
import torch

from ._lib import GQ_Q3_K, mmq

Q3_K_BLOCK_SIZE = 110  # bytes
Q8_1_BLOCK_SIZE = 36  # bytes
Q3_K_SUBBLK_NUM = 16
QK_K = 256
QK8_1 = 32


def mmq_q3_k(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int) -> torch.Tensor:
    """out = (A @ B.T).T with A in Q3_K (M rows), B fp16 (N, K); fp16 (N, M)."""
    assert (K % 256 == 0)
    return mmq(GQ_Q3_K, A, B, M, N, K)
