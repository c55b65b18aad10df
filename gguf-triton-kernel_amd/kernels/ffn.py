"""Dense SwiGLU FFN over packed GGUF weights: the FFN of a dense (Llama-style) layer and the shared
expert of a mixture-of-experts block (kernels/moe.py MoEBlock(shared=...)).

DenseFFN(..., fused=True) runs gate, up and SwiGLU as one launch at decode (gq_mmq_glu, 1..4 tokens:
the tokens quantized once for both weight streams, h = fp16(silu(g) * u) in fp32) and down as one
more; the default keeps the three products and the torch lines between them.  No reference
counterpart: the reference multiplies one matrix per call.
"""
from __future__ import annotations

import torch

from . import _lib
from .layer_mix import GGUFLinear


class DenseFFN:
    """y = down(silu(gate(x)) * up(x)), x (N, hidden) fp16 -> (N, hidden) fp16.  No host sync:
    forward can be captured in a graph."""

    NAMES = ("ffn_gate", "ffn_up", "ffn_down")

    def __init__(self, gate: GGUFLinear, up: GGUFLinear, down: GGUFLinear, fused: bool = False):
        if not (gate.M == up.M == down.K and gate.K == up.K == down.M):
            raise ValueError("gate / up are (ffn, hidden) and down (hidden, ffn) of one block")
        self.gate, self.up, self.down, self.fused = gate, up, down, bool(fused)

    @classmethod
    def from_gguf(cls, tensors: dict, layer: int, names=NAMES, device="cuda", fused: bool = False):
        """From read_gguf() tensors named blk.<layer>.<name>.weight for the three names (gate, up,
        down): the default is a dense layer's FFN, kernels.moe.SHARED_EXPERT_NAMES a shared expert."""
        parts = []
        for name in names:
            key = f"blk.{layer}.{name}.weight"
            if key not in tensors:
                raise ValueError(f"{key}: the file has no such tensor")
            t = tensors[key]
            if len(t.dims) != 2:
                raise ValueError(f"{t.name}: expected a 2-D weight, dims {t.dims}")
            M, K = t.shape
            parts.append(GGUFLinear(t.type_name, t.to_device(device), M, K))
        return cls(*parts, fused=fused)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """fused=True: gate, up and SwiGLU in one launch (mmq_glu; its own fallback beyond 4 tokens),
        then down -- two launches at decode.  A gate / up pair of different types has no fused
        kernel: the same h from two mmq calls and torch ops."""
        if self.fused:
            if self.gate.gtype == self.up.gtype:
                h = _lib.mmq_glu(self.gate.gtype, self.gate.A, self.up.A, x, self.gate.M, x.shape[0], self.gate.K)
            else:
                h = _lib.glu_torch(self.gate(x), self.up(x))
            return self.down(h)
        return self.down(torch.nn.functional.silu(self.gate(x)) * self.up(x))

    __call__ = forward
