"""Q2_K x fp16 MMQ (no counterpart in the reference: GGML type 10, include/gguf_mmq.h).

A: packed Q2_K super-blocks (84 B per 256 weights: sixteen scale bytes -- a 4-bit scale and a 4-bit
min per 16 weights -- 64 bytes of 2-bit codes, fp16 d and dmin) as a flat int8 device tensor of
M*K/256*84 bytes; B: fp16 (N, K); returns fp16 (N, M) = (A @ B^T)^T.  Runs in libgguf_mmq.so.
"""
import torch

from ._lib import GQ_Q2_K, mmq

Q2_K_BLOCK_SIZE = 84  # bytes
Q8_1_BLOCK_SIZE = 36  # bytes
Q2_K_SUBBLK_NUM = 16
QK_K = 256
QK8_1 = 32


def mmq_q2_k(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int) -> torch.Tensor:
    """out = (A @ B.T).T with A in Q2_K (M rows), B fp16 (N, K); fp16 (N, M)."""
    assert (K % 256 == 0)
    return mmq(GQ_Q2_K, A, B, M, N, K)
