"""Mixture-of-experts FFN block (Mixtral, Qwen-MoE, DeepSeek GGUF checkpoints), decode and prefill.

A MoE model stores each FFN projection as ONE 3-D tensor of E expert matrices,
blk.<L>.ffn_{gate,up,down}_exps.weight with GGUF dims (K, M, E): E packed M x K matrices back
to back.  The router picks S experts per token and leaves the choices in device memory; the
expert-indexed MMQ (kernels._lib.mmq_id) reads them there: up to 64 (token, slot) pairs one
launch per projection (gq_mmq_id), beyond that the device-sorted expert GEMM (gq_mmq_id_sorted:
sort, gather-quantize, GEMM -- three launches per projection).  Either way a block is a fixed
sequence of launches and a little torch glue with no host sync: graph-capturable at any pair
count the sorted entry admits (K % 256 == 0, E <= 1024, up to 65536 pairs); only a shape both
entries refuse takes mmq_id's host-sorted path, which synchronises.  No reference counterpart:
the reference multiplies one dense matrix per call.

MoEFFN(..., fused=True) runs the decode block as three launches instead of seven: gate, up and
SwiGLU in one (gq_mmq_id_glu, the token's row quantized once for both weight streams), down
(gq_mmq_id), and the router-weighted sum over the slots (gq_moe_combine).  Opt-in: the default
keeps the unfused lines and their bits.
"""
from __future__ import annotations

import torch

from . import _lib


class GGUFExperts:
    """E packed GGUF weights (M rows of K elements each) on the device, multiplied by index:
    y[n, s] = x_row(n, s) @ W[ids[n, s]]^T, at any number of (token, slot) pairs (mmq_id: the
    one-launch decode up to 64 pairs, the sorted expert GEMM beyond), the ids read on the device."""

    def __init__(self, type_name: str, A: torch.Tensor, E: int, M: int, K: int):
        self.type_name, self.gtype = type_name, _lib.TYPES[type_name]
        self.A, self.E, self.M, self.K = A, E, M, K

    def __call__(self, x: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
        """x (N, K): every slot of token n reads row n; x (N, S, K): one row per slot.
        ids (N, S) int32 on the device.  Returns (N, S, M) fp16."""
        return _lib.mmq_id(self.gtype, self.A, ids, x, self.E, self.M, self.K)


class MoEFFN:
    """y[n] = sum_s weights[n, s] * down_e(silu(gate_e(x[n])) * up_e(x[n])), e = ids[n, s].
    No host sync at decode or prefill: forward can be captured in a graph, and a replay follows
    whatever ids and weights hold then."""

    NAMES = ("ffn_gate_exps", "ffn_up_exps", "ffn_down_exps")

    def __init__(self, gate: GGUFExperts, up: GGUFExperts, down: GGUFExperts, fused: bool = False):
        if not (gate.E == up.E == down.E and gate.M == up.M == down.K and gate.K == up.K == down.M):
            raise ValueError("gate / up are E x (ffn, hidden) and down E x (hidden, ffn) of one block")
        self.gate, self.up, self.down, self.fused = gate, up, down, bool(fused)

    @classmethod
    def from_gguf(cls, tensors: dict, layer: int, device="cuda", fused: bool = False):
        """From read_gguf() tensors named blk.<layer>.ffn_{gate,up,down}_exps.weight (3-D)."""
        parts = []
        for name in cls.NAMES:
            t = tensors[f"blk.{layer}.{name}.weight"]
            if len(t.dims) != 3:
                raise ValueError(f"{t.name}: expected a 3-D expert tensor, dims {t.dims}")
            E, M, K = t.shape
            parts.append(GGUFExperts(t.type_name, t.to_device(device), E, M, K))
        return cls(*parts, fused=fused)

    def forward(self, x: torch.Tensor, ids: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
        """x (N, hidden) fp16, ids (N, S) int32 and weights (N, S) on the device -> (N, hidden).
        fused=True: gate, up and SwiGLU in one launch (mmq_id_glu: h = fp16(silu(g) * u) in fp32,
        one rounding fewer than the torch ops below), down, and the weighted sum over the slots in
        one launch (moe_combine: fp32 in slot order) -- three launches up to 64 pairs, fp16 out.
        A gate / up pair of different types has no fused kernel: the same h from two mmq_id calls."""
        if self.fused:
            if self.gate.gtype == self.up.gtype:
                h = _lib.mmq_id_glu(self.gate.gtype, self.gate.A, self.up.A, ids, x, self.gate.E, self.gate.M, self.gate.K)
            else:
                h = _lib.glu_torch(self.gate(x, ids), self.up(x, ids))
            return _lib.moe_combine(self.down(h, ids), weights)
        g, u = self.gate(x, ids), self.up(x, ids)
        h = torch.nn.functional.silu(g) * u
        d = self.down(h, ids)
        return (weights[..., None] * d).sum(1)

    __call__ = forward
