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

MoERouter makes ids and weights on the device from the token's hidden state (gq_moe_route: the
router product and the top-S selection, two launches), reading the gating function, the
renormalisation, the scale and the selection bias from the file's metadata; MoEBlock is a router
and its MoEFFN: MoEBlock.from_gguf(meta, tensors, layer).forward(x) is the FFN of a MoE layer.

Shared experts (DeepSeek-V2/V3, Qwen-MoE, Llama-4: blk.<L>.ffn_{gate,up,down}_shexp.weight) are a
dense SwiGLU FFN (kernels/ffn.py DenseFFN) whose output is added to the routed sum:
MoEBlock(router, ffn, shared=..., shared_gate=...), or MoEBlock.from_gguf(..., shared_experts=True).
With everything fused the decode block is seven launches: router 2, gq_mmq_id_glu, gq_mmq_id (down),
gq_mmq_glu and gq_mmq (the shared expert), gq_moe_combine_shared; Qwen-MoE's per-token sigmoid gate
of the shared term adds two.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .ffn import DenseFFN
from .norm import RMSNorm


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
        d = self.slots(x, ids)
        if self.fused:
            return _lib.moe_combine(d, weights)
        return (weights[..., None] * d).sum(1)

    def slots(self, x: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
        """The (N, S, hidden) down outputs of the chosen experts, before the weighted sum (forward's
        own first part in either mode)."""
        if self.fused:
            if self.gate.gtype == self.up.gtype:
                h = _lib.mmq_id_glu(self.gate.gtype, self.gate.A, self.up.A, ids, x, self.gate.E, self.gate.M, self.gate.K)
            else:
                h = _lib.glu_torch(self.gate(x, ids), self.up(x, ids))
            return self.down(h, ids)
        g, u = self.gate(x, ids), self.up(x, ids)
        h = torch.nn.functional.silu(g) * u
        return self.down(h, ids)

    __call__ = forward


SHARED_EXPERT_NAMES = ("ffn_gate_shexp", "ffn_up_shexp", "ffn_down_shexp")
SHARED_GATE_NAME = "ffn_gate_inp_shexp"


def _refuse_shared_experts(tensors: dict, layer: int):
    found = [f"blk.{layer}.{n}.weight" for n in SHARED_EXPERT_NAMES if f"blk.{layer}.{n}.weight" in tensors]
    if found:
        raise NotImplementedError("layer %d has shared-expert tensors (%s): their output is added to the routed "
                                  "experts' and this block does not compute it" % (layer, ", ".join(found)))


class MoERouter:
    """The router of a MoE block on the device: x (N, hidden) fp16 -> (ids (N, S) int32, weights
    (N, S) fp32), the arguments MoEFFN.forward takes.  Wr is the (E, hidden) router matrix, fp32 or
    fp16; func "softmax" or "sigmoid"; norm renormalises the S weights to sum 1; scale multiplies
    them; bias (E fp32, sigmoid gating only) moves the selection and never the weights.  The
    definition is gq_moe_topk's (include/gguf_mmq.h).  Two launches up to 64 tokens
    (kernels._lib.moe_route), no host sync: graph-capturable, a replay follows x."""

    def __init__(self, Wr: torch.Tensor, S: int, bias: torch.Tensor | None = None, func: str = "softmax",
                 norm: bool = True, scale: float = 1.0):
        if Wr.dim() != 2 or Wr.dtype not in (torch.float32, torch.float16):
            raise ValueError("Wr must be an fp32 or fp16 (E, hidden) tensor")
        if func not in _lib.GATING:
            raise ValueError(f"func is {func!r}, expected 'softmax' or 'sigmoid'")
        self.Wr, self.E, self.H = Wr.contiguous(), Wr.shape[0], Wr.shape[1]
        if not 1 <= S <= self.E:
            raise ValueError(f"S={S} outside 1..E={self.E}")
        if bias is not None:
            if func != "sigmoid":
                raise ValueError("a selection bias goes with sigmoid gating only")
            if bias.numel() != self.E:
                raise ValueError(f"bias has {bias.numel()} elements, expected E={self.E}")
            bias = bias.to(torch.float32).contiguous()
        self.S, self.bias, self.func, self.norm, self.scale = int(S), bias, func, bool(norm), float(scale)

    @classmethod
    def from_gguf(cls, meta: dict, tensors: dict, layer: int, device="cuda", shared_experts: bool = False):
        """From read_gguf()'s metadata and tensors: blk.<layer>.ffn_gate_inp.weight (f32 or f16,
        GGUF dims (hidden, E)), the optional blk.<layer>.exp_probs_b.bias (f32, E) and, with arch =
        meta["general.architecture"],
            {arch}.expert_count          E; required, must equal the tensor's
            {arch}.expert_used_count     S; required
            {arch}.expert_gating_func    1 softmax, 2 sigmoid; absent or 0: softmax
            {arch}.expert_weights_norm   renormalise the S weights; absent: True with softmax gating
                                         (what Mixtral's graph does), False with sigmoid gating
            {arch}.expert_weights_scale  absent or 0: 1.0
        These key names, values and defaults are written from memory of llama.cpp; nothing here
        can check them against it.  In particular a Qwen-MoE file written without
        expert_weights_norm may want norm=False: build MoERouter(...) by hand when in doubt.
        A layer that also holds shared-expert tensors raises NotImplementedError unless
        shared_experts=True says that the caller computes their term (MoEBlock.from_gguf does)."""
        if not shared_experts:
            _refuse_shared_experts(tensors, layer)
        arch = meta.get("general.architecture")
        if not isinstance(arch, str):
            raise ValueError("the file's metadata has no general.architecture")
        t = tensors[f"blk.{layer}.ffn_gate_inp.weight"]
        if t.type_name not in ("f32", "f16") or len(t.dims) != 2:
            raise ValueError(f"{t.name}: expected a 2-D f32 or f16 router matrix, got {t.type_name} dims {t.dims}")
        E, H = t.shape
        for key in ("expert_count", "expert_used_count"):
            if f"{arch}.{key}" not in meta:
                raise ValueError(f"the file's metadata has no {arch}.{key}")
        if int(meta[f"{arch}.expert_count"]) != E:
            raise ValueError(f"{arch}.expert_count is {meta[f'{arch}.expert_count']} but {t.name} has {E} rows")
        S = int(meta[f"{arch}.expert_used_count"])
        gating = int(meta.get(f"{arch}.expert_gating_func", 0))
        if gating not in (0, 1, 2):
            raise ValueError(f"{arch}.expert_gating_func is {gating}: neither 1 (softmax) nor 2 (sigmoid)")
        func = "sigmoid" if gating == 2 else "softmax"
        norm = bool(meta.get(f"{arch}.expert_weights_norm", func == "softmax"))
        scale = float(meta.get(f"{arch}.expert_weights_scale", 0.0)) or 1.0
        np_dtype = np.float32 if t.type_name == "f32" else np.float16
        Wr = torch.from_numpy(np.array(t.data, dtype=np.uint8).view(np_dtype).reshape(E, H)).to(device)
        bias = None
        b = tensors.get(f"blk.{layer}.exp_probs_b.bias")
        if b is not None:
            if b.type_name != "f32" or int(np.prod(b.dims)) != E:
                raise ValueError(f"{b.name}: expected {E} f32 values, got {b.type_name} dims {b.dims}")
            if func != "sigmoid":
                raise ValueError(f"{b.name}: a selection bias in a file whose gating is softmax")
            bias = torch.from_numpy(np.array(b.data, dtype=np.uint8).view(np.float32).reshape(E)).to(device)
        return cls(Wr, S, bias, func, norm, scale)

    def __call__(self, x: torch.Tensor):
        ids, weights, _ = _lib.moe_route(self.Wr, x, self.S, self.bias, self.func, self.norm, self.scale)
        return ids, weights


class MoEBlock:
    """The whole FFN of a MoE layer: forward(x) = ffn(x, *router(x)), x (N, hidden) fp16 ->
    (N, hidden).  With MoEFFN(fused=True) five launches at decode (two for the router, three for
    the experts), no host sync: graph-capturable, a replay routes the x it finds.
    shared: a DenseFFN over the same hidden size, the layer's shared expert(s); its output is added
    to the routed sum.  shared_gate: an (H,) or (1, H) vector v, Qwen-MoE's gate of the shared term:
    token n's shared output is multiplied by sigmoid(x[n] . v), made in fp32 by the router entry
    (kernels._lib.moe_route with one "expert", sigmoid gating, no renormalisation: its weights are
    exactly that, and it falls back to torch by itself beyond 64 tokens or H % 32 != 0).
    With a fused ffn the routed slots, the shared term and the gate meet in one launch
    (moe_combine_shared: fp32, the slots in order, the shared term last, fp16 out); an unfused ffn
    keeps torch lines: ffn(x, ids, w) + shared(x), the latter times the gate where there is one."""

    def __init__(self, router: MoERouter, ffn: MoEFFN, shared: DenseFFN | None = None,
                 shared_gate: torch.Tensor | None = None, norm: RMSNorm | None = None):
        if norm is not None and norm.K != router.H:
            raise ValueError(f"the norm has {norm.K} weights, the block's hidden size is {router.H}")
        self.norm = norm
        if router.E != ffn.gate.E or router.H != ffn.gate.K:
            raise ValueError(f"router is {router.E} x {router.H} but the experts are {ffn.gate.E} x (ffn, {ffn.gate.K})")
        if shared is not None and (shared.gate.K != router.H or shared.down.M != router.H):
            raise ValueError(f"the shared expert maps {shared.gate.K} -> {shared.down.M}, the block's hidden size is {router.H}")
        if shared_gate is not None:
            if shared is None:
                raise ValueError("a shared_gate without a shared expert")
            if shared_gate.numel() != router.H or shared_gate.dtype not in (torch.float32, torch.float16):
                raise ValueError(f"shared_gate must hold hidden = {router.H} fp32 or fp16 values")
            shared_gate = shared_gate.reshape(1, router.H).contiguous()
        self.router, self.ffn, self.shared, self.shared_gate = router, ffn, shared, shared_gate

    @classmethod
    def from_gguf(cls, meta: dict, tensors: dict, layer: int, device="cuda", fused: bool = True,
                  shared_experts: bool = False, norm: bool = False):
        """From read_gguf()'s metadata and tensors: MoERouter.from_gguf and MoEFFN.from_gguf of the
        layer.  A layer with shared-expert tensors (blk.<layer>.ffn_*_shexp.weight) raises
        NotImplementedError: their output belongs in the sum and nothing here computes it --
        unless shared_experts=True: then blk.<layer>.ffn_{gate,up,down}_shexp.weight (all three once
        any is present; a layer without any has no shared expert) become the block's DenseFFN
        (fused as the block), and the optional blk.<layer>.ffn_gate_inp_shexp.weight (f32 or f16,
        hidden values) its shared_gate.  That last tensor name is written from memory of llama.cpp's
        qwen2moe graph; nothing here can check it against it.
        norm=True: blk.<layer>.ffn_norm.weight becomes the block's RMSNorm (RMSNorm.from_gguf)."""
        if not shared_experts:
            _refuse_shared_experts(tensors, layer)
        router = MoERouter.from_gguf(meta, tensors, layer, device, shared_experts=shared_experts)
        ffn = MoEFFN.from_gguf(tensors, layer, device, fused=fused)
        shared = gate = None
        if shared_experts and any(f"blk.{layer}.{n}.weight" in tensors for n in SHARED_EXPERT_NAMES):
            for n in SHARED_EXPERT_NAMES:
                if f"blk.{layer}.{n}.weight" not in tensors:
                    raise ValueError(f"blk.{layer}.{n}.weight is missing: a shared expert needs its gate, up and down")
            shared = DenseFFN.from_gguf(tensors, layer, SHARED_EXPERT_NAMES, device, fused=fused)
            g = tensors.get(f"blk.{layer}.{SHARED_GATE_NAME}.weight")
            if g is not None:
                if g.type_name not in ("f32", "f16") or int(np.prod(g.dims)) != router.H:
                    raise ValueError(f"{g.name}: expected {router.H} f32 or f16 values, got {g.type_name} dims {g.dims}")
                np_dtype = np.float32 if g.type_name == "f32" else np.float16
                gate = torch.from_numpy(np.array(g.data, dtype=np.uint8).view(np_dtype).reshape(1, router.H)).to(device)
        rms = RMSNorm.from_gguf(meta, tensors, f"blk.{layer}.ffn_norm", device) if norm else None
        return cls(router, ffn, shared, gate, norm=rms)

    def token_gate(self, x: torch.Tensor) -> torch.Tensor | None:
        """The (N,) fp32 gate of the shared term, sigmoid(x . shared_gate), or None without one."""
        if self.shared_gate is None:
            return None
        _, g, _ = _lib.moe_route(self.shared_gate, x, 1, func="sigmoid", norm=False)
        return g.reshape(-1)

    def forward_normed(self, x: torch.Tensor, residual: torch.Tensor | None = None):
        """(out, h): h = fp16(x + residual) (x itself without a residual), out = forward(norm(h)) --
        rmsnorm, one launch, then forward on y at every token count: the router and the expert
        kernels read fp16."""
        if self.norm is None:
            raise RuntimeError("forward_normed needs MoEBlock(..., norm=RMSNorm(...))")
        if residual is None:
            return self.forward(self.norm(x)), x
        y, h = self.norm(x, residual)
        return self.forward(y), h

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        ids, w = self.router(x)
        if self.shared is None:
            return self.ffn(x, ids, w)
        gate = self.token_gate(x)
        if self.ffn.fused:
            return _lib.moe_combine_shared(self.ffn.slots(x, ids), w, self.shared(x), gate)
        sh = self.shared(x)
        if gate is not None:
            sh = gate[:, None] * sh
        return self.ffn(x, ids, w) + sh

    __call__ = forward
