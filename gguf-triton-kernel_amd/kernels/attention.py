"""Attention over a KV cache that lives on the device: the step between a block's q/k/v
projections and its attn_output (kernels/layer_mix.py LayerMix.forward takes the result as `attn`).

    cache = KVCache(B, capacity, n_kv_head, D, kind="q8_0")     # or "f16"
    cache.append(k, v)                # the N new tokens' rows, RoPE already applied to k
    a = cache.attend(q)               # (B*N, n_head*D) fp16

append advances the lengths on the device and writes the rows there (gq_kv_append; Q8_0 blocks with
the weight producer's bytes); attend is gq_attn_decode up to 32 query rows per kv head and
gq_attn_prefill (a prompt, or a chunk of one after a prefix) beyond.  Neither syncs the host or
allocates, the lengths are read by the kernels, so one captured graph of a step serves every length up to
the capacity.  No fallback: a shape the library refuses raises.  No reference counterpart.
"""
from __future__ import annotations

import torch

from . import _lib


class KVCache:
    """The K and V caches of one layer, token-major as llama.cpp keeps them: row (b, t, h) at byte
    ((b*capacity + t)*n_kv_head + h) * row_bytes.  kv_len: int32 (B) on the device, the tokens cached
    per sequence."""

    def __init__(self, B: int, capacity: int, n_kv_head: int, D: int, kind: str = "f16", device="cuda"):
        if kind not in _lib.KV_KINDS:
            raise ValueError(f"kind={kind!r} is neither 'f16' nor 'q8_0'")
        if D not in (64, 128):
            raise ValueError(f"D={D} is neither 64 nor 128")
        if min(B, capacity, n_kv_head) < 1:
            raise ValueError("B, capacity and n_kv_head must be positive")
        self.B, self.capacity, self.n_kv_head, self.D, self.kind = B, capacity, n_kv_head, D, kind
        rb = _lib.kv_row_bytes(kind, D)
        self.strides = (n_kv_head * rb, rb, capacity * n_kv_head * rb)  # (tok, head, seq) bytes
        self.k = torch.zeros(B * capacity * n_kv_head * rb, dtype=torch.uint8, device=device)
        self.v = torch.zeros_like(self.k)
        self.kv_len = torch.zeros(B, dtype=torch.int32, device=device)
        self._ws = {}  # (N, n_head) -> workspace
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

    def attend(self, q: torch.Tensor, scale: float | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """q: fp16 (B*N, n_head*D), the queries of the N tokens last appended -> (B*N, n_head*D) fp16."""
        N = q.shape[0] // self.B
        if N < 1 or N * self.B != q.shape[0] or N != self._n:
            raise ValueError(f"q has {q.shape[0]} rows; the last append wrote {self._n} tokens for each of {self.B} sequences")
        if q.shape[1] % self.D:
            raise ValueError(f"q has {q.shape[1]} columns, not a multiple of D = {self.D}")
        n_head = q.shape[1] // self.D
        if N * (n_head // self.n_kv_head) > 32:  # beyond decode's rows per kv head: the prefill kernel, no workspace
            return _lib.attn_prefill(self.kind, q, self.k, self.v, self.strides, self.kv_len, self.capacity, self.B, N, n_head,
                                     self.n_kv_head, self.D, scale, out)
        ws = self._ws.get((N, n_head))
        if ws is None:
            need = _lib.attn_workspace_size(self.B, N, n_head, self.n_kv_head, self.D)
            ws = self._ws[(N, n_head)] = torch.empty(max(need, 16), dtype=torch.uint8, device=self.k.device)
        return _lib.attn_decode(self.kind, q, self.k, self.v, self.strides, self.kv_len, self.capacity, self.B, N, n_head,
                                self.n_kv_head, self.D, ws, scale, out)
