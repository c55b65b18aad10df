"""Q5_K producer (no counterpart in the reference: GGML type 13).

Super-block (176 B per 256 weights): fp16 d, fp16 dmin, 12 bytes of 6-bit (scale, min) pairs
for 8 sub-blocks (Q4_K's packing), 32 bytes qh (bit j of qh[l] = bit 4 of sub-block j's element
l), 128 bytes of low nibbles; w = d*sc*q - dmin*m with q = 0..31.  Produced by the Q4_K
producer's scale / min search with 31 levels (csrc/quant/gguf_quant_blocks.hpp q5k_block).
"""
import torch

from ._qlib import dequantize, quantize

QK_K = 256
K_SCALE_SIZE = 12


def quantize_to_q5_k(input_tensor: torch.Tensor) -> torch.Tensor:
    """Any-shape tensor (numel % 256 == 0) -> flat int8 CPU tensor of numel/256*176 bytes."""
    return quantize("q5_k", input_tensor)


def dequantize_q5_k(quantized_tensor: torch.Tensor, original_shape) -> torch.Tensor:
    """Packed Q5_K bytes -> fp16 tensor of original_shape."""
    return dequantize("q5_k", quantized_tensor).to(torch.float16).reshape(original_shape)
