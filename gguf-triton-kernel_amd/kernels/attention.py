"""Attention over a KV cache that lives on the device: the step between a block's q/k/v
projections and its attn_output (kernels/layer_mix.py LayerMix.forward takes the result as `attn`).

    cache = KVCache(B, capacity, n_kv_head, D, kind="q8_0")     # or "f16"
    cache.append(k, v)                # the N new tokens' rows, RoPE already applied to k
    a = cache.attend(q)               # (B*N, n_head*D) fp16

or, from the projections as they come, with the rotary embedding (and the per-head q/k norm of Qwen3,
Gemma-3 and OLMo-2) applied on the way -- one launch instead of append, no position tensor:

    rope = RoPE.from_gguf(meta, tensors, layer)                 # the file's rope.* metadata and norm weights
    q = cache.append_rope(q, k, v, rope)                        # gq_rope_append; q, k, v may be slices of one qkv buffer
    a = cache.attend(q)

Gemma-2/3, Mistral, Cohere2 and Phi-3 layers with a sliding window, and Gemma-2's soft-capped scores:

    opts = attn_options(meta, layer)                            # {"window": 4096, "softcap": 50.0} from the file's metadata
    a = cache.attend(q, **opts)                                 # gq_attn_decode_ex / gq_attn_prefill_ex; D = 256 is served

append advances the lengths on the device and writes the rows there (gq_kv_append; Q8_0 blocks with
the weight producer's bytes); attend is gq_attn_decode up to 32 query rows per kv head and
gq_attn_prefill (a prompt, or a chunk of one after a prefix) beyond.  Neither syncs the host or
allocates, the lengths are read by the kernels, so one captured graph of a step serves every length up to
the capacity.  No fallback: a shape the library refuses raises.  No reference counterpart.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

# the pairing of a rotation's two elements by architecture (llama.cpp's rope types)
ROPE_MODE = {a: "norm" for a in ("llama", "llama4", "deepseek", "deepseek2")}
ROPE_MODE.update({a: "neox" for a in ("qwen2", "qwen2moe", "qwen3", "qwen3moe", "gemma", "gemma2", "gemma3", "phi3", "falcon",
                                      "stablelm", "olmo2", "gptneox")})


def _f32_values(t) -> np.ndarray:
    """A GGUF f32 / f16 tensor (gguf.file.GGUFTensor) or any array as flat float64."""
    if hasattr(t, "type_name"):
        t = np.frombuffer(np.ascontiguousarray(t.data), dtype={"f32": np.float32, "f16": np.float16}[t.type_name])
    return np.asarray(t, dtype=np.float64).reshape(-1)


class RoPE:
    """What gq_rope_append needs beside the rows: the frequency table inv_freq (float32 (n_rot/2), on
    the device), n_rot, the mode ("norm": pairs (2j, 2j+1); "neox": (j, j + n_rot/2)), the factor mscale
    on cos and sin, and the optional per-head norm weights (float32 (D), both or neither) with their eps.
    Every frequency scaling is linear in the position, so it lives in the table."""

    def __init__(self, inv_freq: torch.Tensor, n_rot: int, mode: str, mscale: float = 1.0, q_norm: torch.Tensor | None = None,
                 k_norm: torch.Tensor | None = None, eps: float = 1e-6):
        if mode not in _lib.ROPE_MODES:
            raise ValueError(f"mode={mode!r} is neither 'norm' nor 'neox'")
        if n_rot < 2 or n_rot % 2 or inv_freq.numel() != n_rot // 2:
            raise ValueError(f"n_rot={n_rot} must be even and inv_freq hold n_rot/2 values (it holds {inv_freq.numel()})")
        if (q_norm is None) != (k_norm is None):
            raise ValueError("q_norm and k_norm come together or not at all")
        self.inv_freq, self.n_rot, self.mode, self.mscale = inv_freq.to(torch.float32).contiguous(), int(n_rot), mode, float(mscale)
        self.q_norm, self.k_norm = (None if w is None else w.to(torch.float32).contiguous() for w in (q_norm, k_norm))
        self.eps = float(eps)

    @staticmethod
    def table(n_rot: int, base: float = 10000.0, scaling: str = "none", factor: float = 1.0, n_ctx_orig: int = 0,
              freq_factors=None):
        """(inv_freq float64 (n_rot/2), mscale): f_j = base^(-2j/n_rot) / freq_factors[j]; "linear" multiplies
        by 1/factor; "yarn" (beta_fast 32, beta_slow 1) blends f_j / factor and f_j over the ramp between the
        pairs that turn 32 times and once in n_ctx_orig positions, with mscale = 1 + 0.1 ln(factor)."""
        j = np.arange(n_rot // 2, dtype=np.float64)
        f = float(base) ** (-2.0 * j / n_rot)
        if freq_factors is not None:
            f = f / _f32_values(freq_factors)[:n_rot // 2]
        mscale = 1.0
        if scaling == "linear":
            f = f / factor
        elif scaling == "yarn":
            corr = lambda beta: n_rot * math.log(n_ctx_orig / (2 * math.pi * beta)) / (2 * math.log(base))  # noqa: E731
            lo, hi = max(0, math.floor(corr(32.0))), min(n_rot - 1, math.ceil(corr(1.0)))
            ramp = 1.0 - np.clip((j - lo) / max(0.001, hi - lo), 0.0, 1.0)
            f = f * ((1.0 - ramp) / factor + ramp)
            mscale = 1.0 + 0.1 * math.log(factor)
        elif scaling != "none":
            raise ValueError(f"rope scaling type {scaling!r} is none of 'none', 'linear', 'yarn'")
        return f, mscale

    @classmethod
    def from_gguf(cls, meta: dict, tensors: dict, layer: int, device="cuda", mode: str | None = None) -> "RoPE":
        """From a GGUF file's metadata and tensors (gguf.file.read_gguf): {arch}.rope.freq_base,
        .dimension_count, .scaling.{type, factor, original_context_length}, the optional rope_freqs.weight
        (Llama-3.1) and blk.<layer>.attn_{q,k}_norm.weight; the mode from the architecture unless given.
        The table is computed in float64 and rounded to float32 once."""
        arch = meta["general.architecture"]
        if mode is None:
            if arch not in ROPE_MODE:
                raise ValueError(f"no rope mode known for architecture {arch!r}: pass mode='norm' or 'neox'")
            mode = ROPE_MODE[arch]
        get = lambda key, default=None: meta.get(f"{arch}.{key}", default)  # noqa: E731
        D = get("attention.key_length") or get("embedding_length") // get("attention.head_count")
        n_rot = int(get("rope.dimension_count", D))
        ff = tensors.get("rope_freqs.weight")
        f, mscale = cls.table(n_rot, float(get("rope.freq_base", 10000.0)), get("rope.scaling.type", "none"),
                              float(get("rope.scaling.factor", 1.0)), int(get("rope.scaling.original_context_length", 0)), ff)
        norms = [tensors.get(f"blk.{layer}.attn_{n}_norm.weight") for n in "qk"]
        qn, kn = (None if w is None else torch.from_numpy(_f32_values(w).astype(np.float32)).to(device) for w in norms)
        return cls(torch.from_numpy(f.astype(np.float32)).to(device), n_rot, mode, mscale, qn, kn,
                   float(get("attention.layer_norm_rms_epsilon", 1e-6)))


# local layers per global one where the file has no {arch}.attention.sliding_window_pattern (llama.cpp's defaults)
SWA_PATTERN = {"gemma2": 2, "gemma3": 6}


def attn_options(meta: dict, layer: int) -> dict:
    """KVCache.attend's window and softcap for one layer from a GGUF file's metadata:
    {arch}.attention.sliding_window and {arch}.attn_logit_softcapping (0 where the file has none).  With
    a pattern n -- {arch}.attention.sliding_window_pattern, else 2 for gemma2 and 6 for gemma3 -- layer il
    is windowed unless il % n == n - 1; any other architecture with a window has it on every layer."""
    arch = meta["general.architecture"]
    window = int(meta.get(f"{arch}.attention.sliding_window", 0) or 0)
    n = meta.get(f"{arch}.attention.sliding_window_pattern", SWA_PATTERN.get(arch))
    if window and n is not None and layer % int(n) == int(n) - 1:
        window = 0
    return {"window": window, "softcap": float(meta.get(f"{arch}.attn_logit_softcapping", 0.0) or 0.0)}


class KVCache:
    """The K and V caches of one layer, token-major as llama.cpp keeps them: row (b, t, h) at byte
    ((b*capacity + t)*n_kv_head + h) * row_bytes.  kv_len: int32 (B) on the device, the tokens cached
    per sequence."""

    def __init__(self, B: int, capacity: int, n_kv_head: int, D: int, kind: str = "f16", device="cuda"):
        if kind not in _lib.KV_KINDS:
            raise ValueError(f"kind={kind!r} is neither 'f16' nor 'q8_0'")
        if D not in (64, 128, 256):
            raise ValueError(f"D={D} is none of 64, 128, 256")
        if min(B, capacity, n_kv_head) < 1:
            raise ValueError("B, capacity and n_kv_head must be positive")
        self.B, self.capacity, self.n_kv_head, self.D, self.kind = B, capacity, n_kv_head, D, kind
        rb = _lib.kv_row_bytes(kind, D)
        self.strides = (n_kv_head * rb, rb, capacity * n_kv_head * rb)  # (tok, head, seq) bytes
        self.k = torch.zeros(B * capacity * n_kv_head * rb, dtype=torch.uint8, device=device)
        self.v = torch.zeros_like(self.k)
        self.kv_len = torch.zeros(B, dtype=torch.int32, device=device)
        self._ws = {}  # (N, n_head, window, softcap) -> workspace
        self._n = 0    # the last append's token count: attend's N

    def reset(self):
        self.kv_len.zero_()
        self._n = 0

    def append(self, k: torch.Tensor, v: torch.Tensor):
        """k, v: fp16 (B*N, n_kv_head*D), the N new tokens of every sequence.  The caller keeps
        kv_len + N <= capacity (a row past the capacity is not written)."""
        N = k.shape[0] // self.B
        if N * self.B != k.shape[0] or N < 1:
            raise ValueError(f"k has {k.shape[0]} rows, not a positive multiple of B = {self.B}")
        self.kv_len += N
        _lib.kv_append(self.kind, k, v, self.k, self.v, self.strides, self.kv_len, self.capacity, self.B, N,
                       self.n_kv_head, self.D)
        self._n = N

    def append_rope(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, rope: RoPE, out: torch.Tensor | None = None):
        """append with the rotary embedding on the way (gq_rope_append): q fp16 (B*N, n_head*D), k and v
        (B*N, n_kv_head*D) as the projections wrote them, possibly column slices of one buffer.  The
        per-head norm (where rope has one) and the rotation by each token's position are applied to q and
        k, k and v go into the caches, and the rotated q is returned (in `out`; out=q rotates in place)."""
        N = q.shape[0] // self.B
        if N * self.B != q.shape[0] or N < 1:
            raise ValueError(f"q has {q.shape[0]} rows, not a positive multiple of B = {self.B}")
        if q.shape[1] % self.D:
            raise ValueError(f"q has {q.shape[1]} columns, not a multiple of D = {self.D}")
        self.kv_len += N
        out = _lib.rope_append(self.kind, rope.mode, q, k, v, self.k, self.v, self.strides, self.kv_len, self.capacity,
                               rope.inv_freq, rope.n_rot, self.B, N, q.shape[1] // self.D, self.n_kv_head, self.D, rope.mscale,
                               rope.q_norm, rope.k_norm, rope.eps, out)
        self._n = N
        return out

    def attend(self, q: torch.Tensor, scale: float | None = None, out: torch.Tensor | None = None, window: int = 0,
               softcap: float = 0.0) -> torch.Tensor:
        """q: fp16 (B*N, n_head*D), the queries of the N tokens last appended -> (B*N, n_head*D) fp16.
        window > 0: each token attends its last `window` positions only; softcap > 0: softcap * tanh(s /
        softcap) on the scaled scores (attn_options reads both from a file's metadata)."""
        N = q.shape[0] // self.B
        if N < 1 or N * self.B != q.shape[0] or N != self._n:
            raise ValueError(f"q has {q.shape[0]} rows; the last append wrote {self._n} tokens for each of {self.B} sequences")
        if q.shape[1] % self.D:
            raise ValueError(f"q has {q.shape[1]} columns, not a multiple of D = {self.D}")
        n_head = q.shape[1] // self.D
        if N * (n_head // self.n_kv_head) > 32:  # beyond decode's rows per kv head: the prefill kernel, no workspace
            return _lib.attn_prefill(self.kind, q, self.k, self.v, self.strides, self.kv_len, self.capacity, self.B, N, n_head,
                                     self.n_kv_head, self.D, scale, out, window=window, softcap=softcap)
        key = (N, n_head, window, softcap)
        ws = self._ws.get(key)
        if ws is None:
            need = _lib.attn_workspace_size(self.B, N, n_head, self.n_kv_head, self.D, window, softcap)
            ws = self._ws[key] = torch.empty(max(need, 16), dtype=torch.uint8, device=self.k.device)
        return _lib.attn_decode(self.kind, q, self.k, self.v, self.strides, self.kv_len, self.capacity, self.B, N, n_head,
                                self.n_kv_head, self.D, ws, scale, out, window=window, softcap=softcap)


MLA_DECODE_MAX_N = 4  # gq_mla_decode's limit on the new tokens of a step; more go to gq_mla_prefill


class MLACache:
    """The latent cache of one DeepSeek-V2/V3 (multi-head latent attention) layer: ONE fp16 row of rank +
    rope_dim values [c_kv | k_pe] per (sequence, position), at byte (b*capacity + t) * 2 * (rank + rope_dim),
    shared by every query head as key and value.  kv_len: int32 (B) on the device.  append and attend are
    gq_mla_append and, up to 4 new tokens, gq_mla_decode; beyond -- a prompt, a chunk of one, a speculative
    verification -- gq_mla_prefill; up to 128 heads.  None syncs the host, and none allocates after the first
    call at a given (N, n_head), so one captured graph of a step serves every length up to the capacity.  No
    fallback: a shape the library refuses raises.  expand and attend_mha are the un-absorbed prompt pass
    (gq_mla_kv_expand, gq_mla_prefill_mha) over a second, per-head buffer of the first kv_capacity positions."""

    def __init__(self, B: int, capacity: int, rank: int = _lib.MLA_RANK, rope_dim: int = _lib.MLA_ROPE, device="cuda",
                 kv_capacity: int | None = None):
        if (rank, rope_dim) != (_lib.MLA_RANK, _lib.MLA_ROPE):
            raise ValueError(f"(rank, rope_dim) = ({rank}, {rope_dim}) is not ({_lib.MLA_RANK}, {_lib.MLA_ROPE})")
        if min(B, capacity) < 1:
            raise ValueError("B and capacity must be positive")
        self.B, self.capacity, self.rank, self.rope_dim = B, capacity, rank, rope_dim
        rb = 2 * (rank + rope_dim)
        self.strides = (rb, capacity * rb)  # (tok, seq) bytes
        self.c = torch.zeros(B * capacity * rb, dtype=torch.uint8, device=device)
        self.kv_len = torch.zeros(B, dtype=torch.int32, device=device)
        self._bufs = {}  # (N, n_head) -> (q [q_abs | q_pe] rows, decode's workspace or None, output)
        self._n = 0      # the last append's token count: attend's N
        # the un-absorbed prompt pass (expand, attend_mha): per-head [k_nope | v] of the first kv_capacity positions,
        # allocated at the first expand; host counts of the positions appended per sequence and of those expanded
        self.kv_capacity = capacity if kv_capacity is None else min(int(kv_capacity), capacity)
        self.kv, self._mha_out, self.appended, self.expanded = None, {}, 0, 0

    def reset(self):
        self.kv_len.zero_()
        self._n = self.appended = self.expanded = 0

    def _for(self, N: int, n_head: int):
        bufs = self._bufs.get((N, n_head))
        if bufs is None:
            dev, T = self.c.device, self.B * N
            ws = None  # (the prefill route has no workspace)
            if N <= MLA_DECODE_MAX_N:
                need = _lib.mla_workspace_size(self.B, N, n_head, self.rank, self.rope_dim)
                ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            bufs = self._bufs[(N, n_head)] = (torch.zeros(T, n_head * (self.rank + self.rope_dim), dtype=torch.float16, device=dev),
                                              ws,
                                              torch.empty(T, n_head * self.rank, dtype=torch.float16, device=dev))
        return bufs

    def append(self, ckv: torch.Tensor, kpe: torch.Tensor, q: torch.Tensor, rope: RoPE, norm_w: torch.Tensor, eps: float = 1e-6,
               q_head_dim: int = 192):
        """ckv fp16 (B*N, rank) and kpe (B*N, rope_dim): the N new tokens' halves of the attn_kv_a_mqa output
        (column slices of it will do).  q fp16 (B*N, n_head*q_head_dim): the rope_dim values to rotate are the
        LAST rope_dim columns of every head (192: [q_nope (128) | q_pe (64)]; rope_dim: q_pe alone).
        The cache rows are written, kv_len advances by N, and the returned fp16 (B*N, n_head*(rank + rope_dim))
        buffer -- this cache's own, reused every step -- has every head's rotated q_pe in its last rope_dim
        columns; the caller writes the absorbed q into the first rank columns of each head and calls attend."""
        N, n_head, Dq = q.shape[0] // self.B, q.shape[1] // q_head_dim, q_head_dim
        if N * self.B != q.shape[0] or N < 1:
            raise ValueError(f"q has {q.shape[0]} rows, not a positive multiple of B = {self.B}")
        if n_head < 1 or Dq * n_head != q.shape[1] or Dq < self.rope_dim:
            raise ValueError(f"q has {q.shape[1]} columns, not heads of q_head_dim = {Dq} >= rope_dim = {self.rope_dim}")
        qbuf = self._for(N, n_head)[0]
        self.kv_len += N
        _lib.mla_append(rope.mode, ckv, kpe, q[:, Dq - self.rope_dim:], Dq, qbuf, self.c, self.strides, self.kv_len, self.capacity,
                        rope.inv_freq, rope.mscale, norm_w, eps, self.B, N, n_head, self.rank, self.rope_dim)
        self._n = N
        self.appended += N
        return qbuf

    def attend(self, q: torch.Tensor, scale: float) -> torch.Tensor:
        """q: fp16 (B*N, n_head*(rank + rope_dim)), [q_abs | q_pe] per head, of the N tokens last appended
        (append's buffer, completed) -> fp16 (B*N, n_head*rank), the cache's own output buffer."""
        N = q.shape[0] // self.B
        if N < 1 or N * self.B != q.shape[0] or N != self._n:
            raise ValueError(f"q has {q.shape[0]} rows; the last append wrote {self._n} tokens for each of {self.B} sequences")
        n_head = q.shape[1] // (self.rank + self.rope_dim)
        _, ws, out = self._for(N, n_head)
        if N > MLA_DECODE_MAX_N:
            return _lib.mla_prefill(q, self.c, self.strides, self.kv_len, self.capacity, self.B, N, n_head, scale, out,
                                    self.rank, self.rope_dim)
        return _lib.mla_decode(q, self.c, self.strides, self.kv_len, self.capacity, self.B, N, n_head, ws, scale, out,
                               self.rank, self.rope_dim)

    def expand(self, W: torch.Tensor, N: int) -> torch.Tensor:
        """Decompress the N newest positions of every sequence into the expanded buffer (gq_mla_kv_expand): W fp16
        (n_head, 256, 512), head h's rows [k_b^T (128) | v_b (128)].  The buffer -- fp16 (B, kv_capacity, n_head*256),
        [k_nope | v] per head -- is allocated at the first call and kept; positions at or beyond kv_capacity are
        skipped.  The host count of expanded positions (`expanded`) becomes the host count of appended ones."""
        n_head = int(W.shape[0])
        if self.kv is None or self.kv.shape[2] != n_head * _lib.MLA_KV_WIDTH:
            if self.kv_capacity * n_head * 2 * _lib.MLA_KV_WIDTH > 1 << 30:
                raise ValueError(f"kv_capacity = {self.kv_capacity} positions of {n_head} heads span more than 1 GiB a sequence")
            self.kv = torch.zeros(self.B, self.kv_capacity, n_head * _lib.MLA_KV_WIDTH, dtype=torch.float16, device=self.c.device)
        _lib.mla_kv_expand(W, self.c, self.strides, self.kv_len, self.capacity, self.kv, self.B, N, n_head)
        self.expanded = self.appended
        return self.kv

    def attend_mha(self, qn: torch.Tensor, qp: torch.Tensor, scale: float, qn_head_stride: int = 192,
                   qp_head_stride: int | None = None) -> torch.Tensor:
        """Un-absorbed attention of the N tokens last appended over the expanded buffer (gq_mla_prefill_mha): qn the
        q projection's output (head h's q_nope at column h*qn_head_stride), qp the rotated q_pe (append's buffer from
        column rank on: head stride rank + rope_dim) -> fp16 (B*N, n_head*128), the cache's own buffer for (N, n_head)."""
        N = qn.shape[0] // self.B
        if N < 1 or N * self.B != qn.shape[0] or N != self._n:
            raise ValueError(f"qn has {qn.shape[0]} rows; the last append wrote {self._n} tokens for each of {self.B} sequences")
        if self.kv is None:
            raise ValueError("nothing is expanded: call expand(W, N) first")
        n_head = self.kv.shape[2] // _lib.MLA_KV_WIDTH
        out = self._mha_out.get((N, n_head))
        if out is None:
            out = self._mha_out[(N, n_head)] = torch.empty(self.B * N, n_head * _lib.MLA_PROJ_DIM, dtype=torch.float16, device=self.c.device)
        return _lib.mla_prefill_mha(qn, qn_head_stride, qp, qp_head_stride or self.rank + self.rope_dim, self.kv, self.c, self.strides,
                                    self.kv_len, self.capacity, self.B, N, n_head, scale, out)


class MLAttention:
    """A DeepSeek-V2/V3 layer's attention core, at decode and over a prompt alike, between the q / attn_kv_a_mqa
    projections and attn_output: the absorption of W_UK into q (a torch bmm on dequantized weights), MLACache.append,
    MLACache.attend, and the product with W_UV (a second bmm).  fused=True: the two products are gq_mla_proj
    launches that write straight into the cache's q buffer and an output buffer kept per token count -- four
    launches at decode (five with the combine), no torch op, no allocation after the first call at a given T, the
    whole step capturable in one graph; (rank, nope, v_dim) must be (512, 128, 128), anything else raises.  The
    default keeps the bmm form and its bits.  k_b: fp16 (n_head, rank, nope), v_b: fp16 (n_head, v_dim, rank)."""

    def __init__(self, k_b: torch.Tensor, v_b: torch.Tensor, norm_w: torch.Tensor, rope: RoPE, eps: float = 1e-6,
                 scale: float | None = None, fused: bool = False, unabsorbed_from: int = 0):
        self.k_b, self.v_b = k_b.to(torch.float16).contiguous(), v_b.to(torch.float16).contiguous()
        self.n_head, self.rank, self.nope = self.k_b.shape
        self.v_dim = self.v_b.shape[1]
        if self.v_b.shape[0] != self.n_head or self.v_b.shape[2] != self.rank:
            raise ValueError(f"v_b is {tuple(self.v_b.shape)}, expected ({self.n_head}, v_dim, {self.rank})")
        self.norm_w, self.rope, self.eps = norm_w.to(torch.float32).contiguous(), rope, float(eps)
        # llama.cpp's deepseek2 scale: mscale^2 / sqrt(the un-absorbed key length)
        self.scale = rope.mscale ** 2 / math.sqrt(self.nope + rope.n_rot) if scale is None else float(scale)
        self.cache = None
        self.fused, self._out = bool(fused), {}  # T -> the fused form's output buffer
        # unabsorbed_from = n > 0: a forward of n or more new tokens takes the un-absorbed pass (append, expand, MHA)
        self.unabsorbed_from, self.w_kv = int(unabsorbed_from), None
        if self.unabsorbed_from > 0:
            if (self.rank, self.nope, self.v_dim) != (_lib.MLA_RANK, _lib.MLA_PROJ_DIM, _lib.MLA_PROJ_DIM):
                raise ValueError(f"(rank, nope, v_dim) = ({self.rank}, {self.nope}, {self.v_dim}) is not (512, 128, 128)")
            self.w_kv = torch.cat([self.k_b.transpose(1, 2), self.v_b], dim=1).contiguous()  # (n_head, 256, 512)

    @classmethod
    def from_gguf(cls, meta: dict, tensors: dict, layer: int, device="cuda", scale: float | None = None,
                  fused: bool = False, unabsorbed_from: int = 0) -> "MLAttention":
        """From read_gguf()'s metadata and tensors: {arch}.attention.kv_lora_rank, {arch}.rope.dimension_count
        and the rope.scaling.* keys (through RoPE.from_gguf), {arch}.attention.layer_norm_rms_epsilon,
        blk.<layer>.attn_kv_a_norm.weight, and blk.<layer>.attn_k_b.weight (GGUF dims (nope, rank, n_head)) with
        attn_v_b.weight (dims (rank, v_dim, n_head)) -- or the older fused blk.<layer>.attn_kv_b.weight (dims
        (rank, n_head * (nope + v_dim)): per head nope rows of W_UK, then v_dim rows of W_UV), split here with
        {arch}.attention.key_length - rope dimension as nope.  These key and tensor names, their dims and the
        default scale are written from memory of llama.cpp's deepseek2 graph; nothing here can check them
        against it.  Quantized weights are dequantized once (gq_dequantize) and kept as fp16."""
        arch = meta["general.architecture"]
        rank, n_rot = int(meta[f"{arch}.attention.kv_lora_rank"]), int(meta[f"{arch}.rope.dimension_count"])
        n_head = int(meta[f"{arch}.attention.head_count"])
        rope = RoPE.from_gguf(meta, tensors, layer, device, mode=ROPE_MODE.get(arch, "norm"))
        rope = RoPE(rope.inv_freq, n_rot, rope.mode, rope.mscale)  # (attn_q_norm / attn_k_norm are no MLA tensors)

        def dense(t):
            if t.type_name in ("f16", "f32"):
                return torch.from_numpy(_f32_values(t).astype(np.float16)).to(device).reshape(t.shape)
            rows = int(np.prod(t.shape[:-1]))
            return _lib.dequantize_device(_lib.TYPES[t.type_name], t.to_device(device), rows, t.shape[-1]).reshape(t.shape)

        kb, vb = tensors.get(f"blk.{layer}.attn_k_b.weight"), tensors.get(f"blk.{layer}.attn_v_b.weight")
        if kb is not None and vb is not None:
            k_b, v_b = dense(kb), dense(vb)
        else:
            kv = dense(tensors[f"blk.{layer}.attn_kv_b.weight"])  # (n_head * (nope + v_dim), rank)
            nope = int(meta[f"{arch}.attention.key_length"]) - n_rot
            kv = kv.view(n_head, -1, rank)
            k_b, v_b = kv[:, :nope].transpose(1, 2), kv[:, nope:]
        norm_w = torch.from_numpy(_f32_values(tensors[f"blk.{layer}.attn_kv_a_norm.weight"]).astype(np.float32)).to(device)
        return cls(k_b, v_b, norm_w, rope, float(meta.get(f"{arch}.attention.layer_norm_rms_epsilon", 1e-6)), scale, fused,
                   unabsorbed_from)

    def new_cache(self, B: int, capacity: int, device="cuda", kv_capacity: int | None = None) -> MLACache:
        """The layer's latent cache, empty: forward appends to it and attends over it.  kv_capacity: the positions the
        un-absorbed pass may expand (default: the capacity, at most what 1 GiB a sequence holds -- 16384 at 128 heads)."""
        if kv_capacity is None:
            kv_capacity = min(capacity, (1 << 30) // (self.n_head * 2 * _lib.MLA_KV_WIDTH))
        self.cache = MLACache(B, capacity, self.rank, self.rope.n_rot, device, kv_capacity)
        return self.cache

    def forward(self, q: torch.Tensor, kv_a_out: torch.Tensor, cache: MLACache | None = None) -> torch.Tensor:
        """q fp16 (B*N, n_head*(nope + rope_dim)) and the attn_kv_a_mqa output (B*N, rank + rope_dim) of the N
        new tokens -> fp16 (B*N, n_head*v_dim), attn_output's input, over `cache` (new_cache's when None).
        Four steps: q_nope absorbed by bmm, append, attend, bmm with W_UV; fused: append, gq_mla_proj into the
        cache's q buffer, attend, gq_mla_proj into this layer's output buffer for T (returned: reused every step).
        unabsorbed_from = n > 0 and n or more new tokens per sequence that the expanded buffer still holds: append,
        gq_mla_kv_expand of every position not yet expanded, gq_mla_prefill_mha -- three launches, no torch op, no
        allocation after the first call at a given shape; the cache's own output buffer for (N, n_head) is returned."""
        cache = self.cache if cache is None else cache
        if cache is None:
            raise ValueError("no cache: call new_cache(B, capacity) first, or pass one")
        T, H, rank = q.shape[0], self.n_head, self.rank
        N = T // cache.B
        if 0 < self.unabsorbed_from <= N and cache.appended + N <= cache.kv_capacity:
            # (positions decode steps appended since the last expansion are expanded in the same launch)
            qbuf = cache.append(kv_a_out[:, :rank], kv_a_out[:, rank:], q, self.rope, self.norm_w, self.eps)
            cache.expand(self.w_kv, cache.appended - cache.expanded)
            return cache.attend_mha(q, qbuf[:, rank:], self.scale, q.shape[1] // H, qbuf.shape[1] // H)
        if self.fused:
            qbuf = cache.append(kv_a_out[:, :rank], kv_a_out[:, rank:], q, self.rope, self.norm_w, self.eps)
            _lib.mla_proj(0, self.k_b, q, q.shape[1] // H, qbuf, qbuf.shape[1] // H, T, H)
            o = cache.attend(qbuf, self.scale)
            out = self._out.get(T)
            if out is None or out.device != q.device:
                out = self._out[T] = torch.empty(T, H * self.v_dim, dtype=torch.float16, device=q.device)
            return _lib.mla_proj(1, self.v_b, o, rank, out, self.v_dim, T, H)
        q_abs = torch.bmm(q.view(T, H, -1)[:, :, :self.nope].transpose(0, 1), self.k_b.transpose(1, 2))  # (H, T, rank)
        qbuf = cache.append(kv_a_out[:, :rank], kv_a_out[:, rank:], q, self.rope, self.norm_w, self.eps)
        qbuf.view(T, H, -1)[:, :, :rank].copy_(q_abs.transpose(0, 1))
        o = cache.attend(qbuf, self.scale)                                                               # (T, H*rank)
        return torch.bmm(o.view(T, H, rank).transpose(0, 1), self.v_b.transpose(1, 2)).transpose(0, 1).reshape(T, H * self.v_dim)
