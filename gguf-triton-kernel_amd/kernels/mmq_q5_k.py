"""Q5_K x fp16 MMQ (no counterpart in the reference: GGML type 13, include/gguf_mmq.h).

A: packed Q5_K super-blocks (176 B per 256 weights: fp16 d, fp16 dmin, 12 bytes of 6-bit
scales/mins as Q4_K's, 32 bytes of high bits, 128 bytes of nibbles) as a flat int8 device
tensor of M*K/256*176 bytes; B: fp16 (N, K); returns fp16 (N, M) = (A @ B^T)^T.  Runs in
libgguf_mmq.so.
"""
import torch

from ._lib import GQ_Q5_K, mmq

Q5_K_BLOCK_SIZE = 176  # bytes
Q8_1_BLOCK_SIZE = 36  # bytes
Q5_K_SUBBLK_NUM = 8
QK_K = 256
QK8_1 = 32


def mmq_q5_k(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int) -> torch.Tensor:
    """out = (A @ B.T).T with A in Q5_K (M rows), B fp16 (N, K); fp16 (N, M)."""
    assert (K % 256 == 0)
    return mmq(GQ_Q5_K, A, B, M, N, K)
