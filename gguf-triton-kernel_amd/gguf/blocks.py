"""The GGUF block types' sizes: the one Python table (its native counterpart is kFmt in
csrc/gguf_blocks.hpp; tests/test_fmt_table.py holds the two together).

Pure Python, so that kernels/ (libgguf_mmq.so), utils/quantize/ (libgguf_quant.so), utils/synth.py
and gguf/file.py can all read it without loading each other's native library.
"""

# weight type name -> (elements per block, bytes per block), in gq_type order (include/gguf_mmq.h)
BLOCK = {"q8_0": (32, 34), "q4_k": (256, 144), "q6_k": (256, 210), "q5_k": (256, 176), "q3_k": (256, 110),
         "q2_k": (256, 84), "q4_0": (32, 18)}
Q8_1 = (32, 36)  # the activation block (not a weight type)
