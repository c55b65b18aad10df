"""Q2_K producer (no counterpart in the reference: GGML type 10).

Super-block (84 B per 256 weights): sixteen scale bytes (low nibble = 4-bit scale, high nibble =
4-bit min of 16 weights), 64 bytes of 2-bit codes, fp16 d, fp16 dmin; w = d*sc*code - dmin*m.
Produced by the Q4_K producer's scale / min fit per 16 weights over codes 0..3, the scales and mins
quantized to 4 bits against the largest of each (csrc/quant/gguf_quant_blocks.hpp q2k_block).
"""
import torch

from ._qlib import dequantize, quantize

QK_K = 256


def quantize_to_q2_k(input_tensor: torch.Tensor) -> torch.Tensor:
    """Any-shape tensor (numel % 256 == 0) -> flat int8 CPU tensor of numel/256*84 bytes."""
    return quantize("q2_k", input_tensor)


def dequantize_q2_k(quantized_tensor: torch.Tensor, original_shape) -> torch.Tensor:
    """Packed Q2_K bytes -> fp16 tensor of original_shape."""
    return dequantize("q2_k", quantized_tensor).to(torch.float16).reshape(original_shape)
