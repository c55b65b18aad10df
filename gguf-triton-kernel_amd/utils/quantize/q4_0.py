"""Q4_0 producer (no counterpart in the reference: GGML type 2).

Block (18 B per 32 weights): fp16 d, then sixteen bytes of 4-bit codes (element j in the low nibble
of byte j, element 16 + j in the high one); w = d*(code - 8).  d = m / -8 with m the block's element
of largest magnitude, sign kept, so that m itself gets code 0; the other codes by truncation of
x/d + 8.5, clamped to 15 (csrc/quant/gguf_quant_blocks.hpp q4_0_block).  This is llama.cpp's rule
written from memory; nothing here can check it against llama.cpp.
"""
import torch

from ._qlib import dequantize, quantize

QK4_0 = 32


def quantize_to_q4_0(input_tensor: torch.Tensor) -> torch.Tensor:
    """Any-shape tensor (numel % 32 == 0) -> flat int8 CPU tensor of numel/32*18 bytes."""
    return quantize("q4_0", input_tensor)


def dequantize_q4_0(quantized_tensor: torch.Tensor, original_shape) -> torch.Tensor:
    """Packed Q4_0 bytes -> fp16 tensor of original_shape."""
    return dequantize("q4_0", quantized_tensor).to(torch.float16).reshape(original_shape)
