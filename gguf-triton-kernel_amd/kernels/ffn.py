"""Dense SwiGLU FFN over packed GGUF weights: the FFN of a dense (Llama-style) layer and the shared
expert of a mixture-of-experts block (kernels/moe.py MoEBlock(shared=...)).

DenseFFN(..., fused=True) runs gate, up and SwiGLU as one launch at decode (gq_mmq_glu, 1..4 tokens:
the tokens quantized once for both weight streams, h = fp16(silu(g) * u) in fp32) and down as one
more; the default keeps the three products and the torch lines between them.  No reference
counterpart: the reference multiplies one matrix per call.

DenseFFN(..., norm=RMSNorm) adds forward_normed(x, residual): the block's residual add and FFN norm
in front (kernels/norm.py), from 5 tokens on written straight into the prepared activations gate
and up both read -- one launch where forward's input costs an add, a norm and two quantizations.
"""
from __future__ import annotations

import torch

from . import _lib
from .layer_mix import PREPARED_MIN_TOKENS, GGUFLinear
from .norm import RMSNorm


class DenseFFN:
    """y = down(silu(gate(x)) * up(x)), x (N, hidden) fp16 -> (N, hidden) fp16.  No host sync:
    forward can be captured in a graph."""

    NAMES = ("ffn_gate", "ffn_up", "ffn_down")

    def __init__(self, gate: GGUFLinear, up: GGUFLinear, down: GGUFLinear, fused: bool = False,
                 norm: RMSNorm | None = None):
        if not (gate.M == up.M == down.K and gate.K == up.K == down.M):
            raise ValueError("gate / up are (ffn, hidden) and down (hidden, ffn) of one block")
        if norm is not None and norm.K != gate.K:
            raise ValueError(f"the norm has {norm.K} weights, the block's hidden size is {gate.K}")
        self.gate, self.up, self.down, self.fused, self.norm = gate, up, down, bool(fused), norm

    @classmethod
    def from_gguf(cls, tensors: dict, layer: int, names=NAMES, device="cuda", fused: bool = False, norm: bool = False,
                  meta: dict | None = None):
        """From read_gguf() tensors named blk.<layer>.<name>.weight for the three names (gate, up,
        down): the default is a dense layer's FFN, kernels.moe.SHARED_EXPERT_NAMES a shared expert.
        norm=True: blk.<layer>.ffn_norm.weight too (RMSNorm.from_gguf; it reads eps from `meta`,
        read_gguf()'s metadata, which is then required)."""
        rms = None
        if norm:
            if meta is None:
                raise ValueError("norm=True needs the file's metadata (meta=) for the norm's eps")
            rms = RMSNorm.from_gguf(meta, tensors, f"blk.{layer}.ffn_norm", device)
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
        return cls(*parts, fused=fused, norm=rms)

    def forward_normed(self, x: torch.Tensor, residual: torch.Tensor | None = None):
        """(out, h): h = fp16(x + residual) (x itself without a residual), out = forward(norm(h)).
        From PREPARED_MIN_TOKENS["q8_1"] tokens: one rmsnorm_prepare launch into a workspace sized
        for the larger of gate and up, both as mmq_prepared on it -- one quantization of the normed
        row where forward makes two, and no fp16 copy of it -- then forward's SwiGLU and down.
        Below that: rmsnorm, then forward on y (forward's bits).  No host sync."""
        if self.norm is None:
            raise RuntimeError("forward_normed needs DenseFFN(..., norm=RMSNorm(...))")
        N = x.shape[0]
        if N < PREPARED_MIN_TOKENS["q8_1"]:
            if residual is None:
                return self.forward(self.norm(x)), x
            y, h = self.norm(x, residual)
            return self.forward(y), h
        ws = torch.empty(max(self.gate.workspace_bytes(N), self.up.workspace_bytes(N)), dtype=torch.uint8, device=x.device)
        h = self.norm.prepare(x, ws, residual)
        g = _lib.mmq_prepared(self.gate.gtype, self.gate.A, ws, self.gate.M, N, self.gate.K)
        u = _lib.mmq_prepared(self.up.gtype, self.up.A, ws, self.up.M, N, self.up.K)
        return self.down(self.glu(g, u)), h

    def glu(self, g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
        """forward's SwiGLU of separate gate and up outputs: fused, mmq_glu's definition in torch ops
        (what it runs beyond 4 tokens); else the torch line."""
        return _lib.glu_torch(g, u) if self.fused else torch.nn.functional.silu(g) * u

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
