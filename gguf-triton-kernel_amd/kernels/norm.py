"""Residual add + RMSNorm of a transformer block's hidden state, fused with the activation
quantization of the products that read it.

Every projection group of a block reads y = RMSNorm(x + residual) * w.  RMSNorm(weight, eps)(x,
residual) is that in one launch (gq_rmsnorm: h = fp16(x + residual), y = fp16((h / sqrt(mean(h^2) +
eps)) * w), the sum of squares and the scale in fp32); .prepare(x, workspace, residual) leaves y in a
workspace exactly as act_prepare would (gq_rmsnorm_prepare), so that mmq_prepared calls follow with
no fp16 round trip of y and no act_quant launch.  DenseFFN.forward_normed and
MoEBlock.forward_normed (kernels/ffn.py, kernels/moe.py) are a block's FFN on it.  No reference
counterpart: the reference multiplies one matrix per call.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


class RMSNorm:
    """y = x_or_h / sqrt(mean(.^2) + eps) * weight over the last dimension, fp16 in and out.
    weight: K fp32 values on the device (GGUF stores *_norm.weight as F32).  No host sync: every
    call can be captured in a graph."""

    def __init__(self, weight: torch.Tensor, eps: float):
        if weight.dim() != 1 or weight.dtype != torch.float32:
            raise ValueError("weight must be a 1-D fp32 tensor")
        eps = float(eps)
        if not (0.0 <= eps < float("inf")):
            raise ValueError(f"eps={eps} is not a finite value >= 0")
        self.weight, self.eps, self.K = weight.contiguous(), eps, weight.numel()

    @classmethod
    def from_gguf(cls, meta: dict, tensors: dict, name: str, device="cuda"):
        """From read_gguf()'s metadata and tensors: the tensor <name>.weight -- name e.g.
        "blk.3.ffn_norm", "blk.3.attn_norm" or "output_norm" -- which must be F32 and 1-D, and, with
        arch = meta["general.architecture"], eps = {arch}.attention.layer_norm_rms_epsilon (required).
        That key name is written from memory of llama.cpp; nothing here can check it against it.
        Build RMSNorm(weight, eps) by hand when a file spells it differently."""
        key = f"{name}.weight"
        if key not in tensors:
            raise ValueError(f"{key}: the file has no such tensor")
        t = tensors[key]
        if t.type_name != "f32" or len(t.dims) != 1:
            raise ValueError(f"{t.name}: expected a 1-D f32 norm weight, got {t.type_name} dims {t.dims}")
        arch = meta.get("general.architecture")
        if not isinstance(arch, str):
            raise ValueError("the file's metadata has no general.architecture")
        ek = f"{arch}.attention.layer_norm_rms_epsilon"
        if ek not in meta:
            raise ValueError(f"the file's metadata has no {ek}")
        w = torch.from_numpy(np.array(t.data, dtype=np.uint8).view(np.float32).reshape(t.dims[0])).to(device)
        return cls(w, float(meta[ek]))

    def __call__(self, x: torch.Tensor, residual: torch.Tensor | None = None):
        """y, or with a residual (y, h): h = fp16(x + residual), the new residual stream."""
        if residual is None:
            return _lib.rmsnorm(x, self.weight, self.eps)
        h = torch.empty((x.shape[0], self.K), dtype=torch.float16, device=x.device)
        y = _lib.rmsnorm(x, self.weight, self.eps, residual, h_out=h)
        return y, h

    def prepare(self, x: torch.Tensor, workspace: torch.Tensor, residual: torch.Tensor | None = None):
        """y into `workspace` as act_prepare(y, N, K, workspace) would leave it, in one launch.
        Returns h (x itself without a residual)."""
        h = None
        if residual is not None:
            h = torch.empty((x.shape[0], self.K), dtype=torch.float16, device=x.device)
        _lib.rmsnorm_prepare(x, self.weight, self.eps, workspace, residual, h_out=h)
        return x if h is None else h
