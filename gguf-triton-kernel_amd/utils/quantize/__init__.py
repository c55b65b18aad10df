"""GGUF block producers: quantize_to_{q8_0,q8_1,q4_k,q6_k,q5_k,q3_k,q2_k,q4_0} and dequantize_* (host side).

Byte-identical to the reference's utils/quantize/*.py (tests/golden/golden_quant.npz);
the work is done by libgguf_quant.so (csrc/quant/gguf_quant.cpp).  q5_k, q3_k, q2_k and q4_0 have no
reference counterpart (no byte contract): utils/quantize/q5_k.py, q3_k.py, q2_k.py, q4_0.py.
"""
