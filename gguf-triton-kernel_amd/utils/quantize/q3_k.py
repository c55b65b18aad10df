"""Q3_K producer (no counterpart in the reference: GGML type 11).

Super-block (110 B per 256 weights): 32 bytes hmask (bit 4*(e/128) + (e%128)/32 of hmask[e%32] =
bit 2 of element e's code), 64 bytes of 2-bit codes, 12 bytes of sixteen 6-bit scales, fp16 d;
w = d*(sc - 32)*(code - 4).  Produced by the Q6_K producer's per-16 scale search over codes -4..3,
the scales quantized to 6 bits against the largest (csrc/quant/gguf_quant_blocks.hpp q3k_block).
"""
import torch

from ._qlib import dequantize, quantize

QK_K = 256
K_SCALE_SIZE = 12


def quantize_to_q3_k(input_tensor: torch.Tensor) -> torch.Tensor:
    """Any-shape tensor (numel % 256 == 0) -> flat int8 CPU tensor of numel/256*110 bytes."""
    return quantize("q3_k", input_tensor)


def dequantize_q3_k(quantized_tensor: torch.Tensor, original_shape) -> torch.Tensor:
    """Packed Q3_K bytes -> fp16 tensor of original_shape."""
    return dequantize("q3_k", quantized_tensor).to(torch.float16).reshape(original_shape)
