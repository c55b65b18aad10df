"""GGUF container I/O (reader + writer) and the Q4_K_M layer-type map."""
from .file import GGML_TYPES, GGUFTensor, read_gguf, write_gguf  # noqa: F401
from .mix import (LLAMA_LAYER_SHAPES, q2_k_layer_types, q3_k_m_layer_types, q4_0_layer_types,  # noqa: F401
                  q4_k_m_layer_types, q5_k_m_layer_types)
