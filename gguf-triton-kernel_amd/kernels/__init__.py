"""Drop-in replacement for the reference's `kernels` package (MI355X / gfx950, HIP).

    from kernels.mmq_q8_0 import mmq_q8_0
    from kernels.mmq_q4_k import mmq_q4_k
    from kernels.mmq_q6_k import mmq_q6_k
    from kernels.mmq_q5_k import mmq_q5_k   (beyond the reference: GGML type 13)
    from kernels.mmq_q3_k import mmq_q3_k   (beyond the reference: GGML type 11)
    from kernels.mmq_q2_k import mmq_q2_k   (beyond the reference: GGML type 10)
    from kernels.mmq_q4_0 import mmq_q4_0   (beyond the reference: GGML type 2)

Each computes C = (A @ B^T)^T with A a packed GGUF weight tensor (int8, flat) and B fp16
activations (N, K), returning fp16 (N, M) -- the reference's signature and layout.

Beyond the reference, decode and prefill attention over an fp16 or Q8_0 KV cache (kernels/attention.py):

    from kernels import KVCache, attn_decode, attn_prefill, kv_append

with a sliding window and a logit soft-cap per layer, at head dims 64, 128 and 256 (Gemma):

    from kernels import attn_options           # cache.attend(q, **attn_options(meta, layer))

and the rotary embedding (with the per-head q/k norm) fused into the append:

    from kernels import RoPE, rope_append

and DeepSeek's multi-head latent attention over a latent cache, at decode and over a prompt (gq_mla_decode,
gq_mla_prefill, gq_mla_append):

    from kernels import MLACache, MLAttention, mla_decode, mla_prefill, mla_append

with the per-head W_UK / W_UV products around it in HIP (gq_mla_proj; MLAttention(..., fused=True)):

    from kernels import mla_proj

and the un-absorbed prompt pass (gq_mla_kv_expand, gq_mla_prefill_mha; MLAttention(..., unabsorbed_from=n)):

    from kernels import mla_kv_expand, mla_prefill_mha
"""
_LAZY = {"KVCache": "attention", "attn_decode": "_lib", "attn_prefill": "_lib", "kv_append": "_lib", "RoPE": "attention",
         "rope_append": "_lib", "attn_options": "attention", "MLACache": "attention", "MLAttention": "attention",
         "mla_decode": "_lib", "mla_prefill": "_lib", "mla_append": "_lib", "mla_proj": "_lib",
         "mla_kv_expand": "_lib", "mla_prefill_mha": "_lib"}
__all__ = list(_LAZY)


def __getattr__(name):  # (on first use: importing the package loads neither torch nor the library)
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module(f"{__name__}.{_LAZY[name]}"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
