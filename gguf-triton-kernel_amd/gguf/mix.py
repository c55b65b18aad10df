"""The Q4_K_M (and Q5_K_M, Q3_K_M, Q2_K, Q4_0) layer-type mix of a Llama block (BASELINE.json configs[4]).

llama.cpp's Q4_K_M recipe (not in the reference): every weight Q4_K except attn_v and
ffn_down, which are Q6_K on a subset of layers -- the first eighth, the last eighth and every
third layer in between (use_more_bits(i, n) = i < n/8 || i >= 7n/8 || (i - n/8) % 3 == 2).
"""

# Llama-7B projection shapes (rows M = out features, K = in features)
LLAMA_LAYER_SHAPES = {
    "attn_q": (4096, 4096), "attn_k": (4096, 4096), "attn_v": (4096, 4096), "attn_output": (4096, 4096),
    "ffn_gate": (11008, 4096), "ffn_up": (11008, 4096), "ffn_down": (4096, 11008),
}


def _more_bits(i, n):
    return i < n // 8 or i >= 7 * n // 8 or (i - n // 8) % 3 == 2


def q4_k_m_layer_types(layer: int, n_layers: int = 32):
    """{projection: gguf type} of layer `layer` of an n_layers model under Q4_K_M."""
    hi = "q6_k" if _more_bits(layer, n_layers) else "q4_k"
    return {name: (hi if name in ("attn_v", "ffn_down") else "q4_k") for name in LLAMA_LAYER_SHAPES}


def q5_k_m_layer_types(layer: int, n_layers: int = 32):
    """{projection: gguf type} of layer `layer` under Q5_K_M: Q4_K_M's rule with q5_k as the base type."""
    hi = "q6_k" if _more_bits(layer, n_layers) else "q5_k"
    return {name: (hi if name in ("attn_v", "ffn_down") else "q5_k") for name in LLAMA_LAYER_SHAPES}


def q3_k_m_layer_types(layer: int, n_layers: int = 32):
    """{projection: gguf type} of layer `layer` under Q3_K_M.

    llama.cpp's rule for Llama models, written here from memory (nothing here can check it against
    llama.cpp): attn_v q5_k on layers 0-1 and q4_k after, attn_output q4_k, ffn_down q5_k on the
    first sixteenth of the layers and q4_k after, everything else q3_k."""
    def one(name):
        if name == "attn_v":
            return "q5_k" if layer < 2 else "q4_k"
        if name == "attn_output":
            return "q4_k"
        if name == "ffn_down":
            return "q5_k" if layer < n_layers // 16 else "q4_k"
        return "q3_k"
    return {name: one(name) for name in LLAMA_LAYER_SHAPES}


def q2_k_layer_types(layer: int, n_layers: int = 32, n_gqa: int = 1):
    """{projection: gguf type} of layer `layer` under llama.cpp's Q2_K file type.

    llama.cpp's rule for Llama models, written here from memory (nothing here can check it against
    llama.cpp): attn_v q3_k, or q4_k when the model groups its query heads (n_gqa >= 4);
    attn_output q3_k; ffn_down q3_k; everything else q2_k.  The rule does not depend on the layer."""
    def one(name):
        if name == "attn_v":
            return "q4_k" if n_gqa >= 4 else "q3_k"
        if name in ("attn_output", "ffn_down"):
            return "q3_k"
        return "q2_k"
    return {name: one(name) for name in LLAMA_LAYER_SHAPES}


def q4_0_layer_types(layer: int, n_layers: int = 32):
    """{projection: gguf type} of layer `layer` under llama.cpp's Q4_0 file type: every projection
    q4_0, whatever the layer.

    llama.cpp's rule for Llama models, written here from memory (nothing here can check it against
    llama.cpp; the token embedding and output tensors, which it may store in another type, are not
    projections of a block)."""
    return {name: "q4_0" for name in LLAMA_LAYER_SHAPES}
