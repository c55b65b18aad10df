#!/usr/bin/env python3
"""The MoE router on the device (kernels/moe.py MoERouter, MoEBlock: gq_moe_route -- the router
product and the top-S selection, two launches) beside the router a user writes in torch today
(cast, matmul, softmax, topk, sum, divide, int cast: seven launches), alone and in front of the
fused expert block (MoEFFN(fused=True)).  Graph-replayed step times (tools/moe_fused_bench.py's
method, bench.py's helpers; bench.py itself does not know the block).

    python tools/moe_route_bench.py [--steps 20] [--repeats 3] [--only mixtral] [--out moe_route.json]

Forms, per row:
    torch_block   the torch router, then MoEFFN(fused=True).forward(x, ids, w)
    block         MoEBlock.forward(x)
    torch_router  the torch router alone
    router        MoERouter(x) alone
Step = one call over N tokens.  The expert tensors rotate over copies holding >= 1 GiB together as
in moe_fused_bench, and every copy has a router matrix of its own (so the routing differs from step
to step); the router-alone rows rotate over router matrices holding 1 GiB together, at most
MAX_ROUTERS of them.  Every replay is timed alone by device events (bench.timed_rotation); the forms
are measured interleaved in one process, `repeats` passes, and each cell is the median over the
passes with their spread (max - min).  "X_slower" is true when X - torch's form exceeds the larger
of the two spreads.  Needs the GPU.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gguf-triton-kernel_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
import moe_fused_bench as FB  # noqa: E402

MAX_ROUTERS = 256

# (name, type or None for the router alone, E, hidden, ffn, S, N)
CASES = [
    ("mixtral", "q4_k", 8, 4096, 14336, 2, 1),
    ("mixtral", "q4_k", 8, 4096, 14336, 2, 4),
    ("qwen-moe-like", "q4_k", 60, 2048, 1536, 4, 1),
    ("qwen-moe-like", "q4_k", 60, 2048, 1536, 4, 8),
    ("router-256x7168", None, 256, 7168, 0, 8, 1),
    ("router-256x7168", None, 256, 7168, 0, 8, 4),
]


def torch_router(Wr, x, S):
    """What a caller writes without the entry: seven launches."""
    logits = torch.matmul(x.float(), Wr.T)
    w, ids = torch.topk(torch.softmax(logits, dim=1), S, dim=1)
    return ids.to(torch.int32), w / w.sum(1, keepdim=True)


class Case:
    def __init__(self, fmt, E, H, F, S, N, dev, steps):
        from kernels.moe import GGUFExperts, MoEBlock, MoEFFN, MoERouter
        self.dev, self.S = dev, S
        gen = torch.Generator(device=dev).manual_seed(5)
        rbytes = E * H * 4
        if fmt is None:
            ncopies = min(MAX_ROUTERS, max(2, math.ceil(bench.ROTATE_BYTES / rbytes)))
            self.plans = [[(g * steps + i) % ncopies for i in range(steps)] for g in range(max(1, math.ceil(ncopies / steps)))]
            self.rotated = bench.rotated_bytes(rbytes, self.plans)
        else:
            ebytes = F * (H // 256) * FB.BLOCK[fmt][1]
            ncopies, self.plans = bench.rotation_plan(3 * E * ebytes, steps)
            self.rotated = bench.rotated_bytes(3 * E * ebytes + rbytes, self.plans)
        # (x as moe_fused_bench scales it, keeping g*u and d in fp16 range; the router matrices are
        # scaled up instead so that the logits are of order 1)
        self.x = (torch.randn((N, H), device=dev, generator=gen) / 1024).to(torch.float16)
        self.routers = [MoERouter(torch.randn((E, H), device=dev, generator=gen) * (1024.0 / math.sqrt(H)), S)
                        for _ in range(ncopies)]
        self.blocks = None
        if fmt is not None:
            base = [FB.random_blocks(fmt, E * F, H, dev, 1), FB.random_blocks(fmt, E * F, H, dev, 2),
                    FB.random_blocks(fmt, E * H, F, dev, 3)]
            self.blocks = []
            for c in range(ncopies):
                g, u, d = (t if c == 0 else t.clone() for t in base)
                ffn = MoEFFN(GGUFExperts(fmt, g, E, F, H), GGUFExperts(fmt, u, E, F, H), GGUFExperts(fmt, d, E, H, F), fused=True)
                self.blocks.append(MoEBlock(self.routers[c], ffn))

    def forms(self):
        return ("torch_block", "block", "torch_router", "router") if self.blocks else ("torch_router", "router")

    def step(self, form, c):
        r = self.routers[c]
        if form == "router":
            return r(self.x)
        if form == "torch_router":
            return torch_router(r.Wr, self.x, self.S)
        if form == "block":
            return self.blocks[c].forward(self.x)
        return self.blocks[c].ffn.forward(self.x, *torch_router(r.Wr, self.x, self.S))

    def check(self):
        """Both routers pick the same experts with the same weights (random logits: no ties), and
        the two block forms agree up to the weights' last bits."""
        ia, wa = self.step("torch_router", 0)
        ib, wb = self.step("router", 0)
        torch.cuda.synchronize(self.dev)
        assert torch.equal(ia, ib), (ia, ib)
        d = float(((wa - wb).abs() / wb).max())
        assert d <= 1e-4, d
        if self.blocks:
            a, b = self.step("torch_block", 0).float(), self.step("block", 0).float()
            torch.cuda.synchronize(self.dev)
            assert torch.isfinite(a).all() and float(a.abs().max()) > 0
            assert float((a - b).abs().max() / a.abs().max()) <= 2e-3
        return d

    def graphs(self, form):
        grs = []
        for plan in self.plans:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for c in plan:
                    self.step(form, c)
            grs.append(gr)
        return grs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, help="substring of the case names to run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_route_bench needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda:0")
    rows = []
    for name, fmt, E, H, F, S, N in CASES:
        if a.only and a.only not in name:
            continue
        case = Case(fmt, E, H, F, S, N, dev, a.steps)
        diff = case.check()
        forms = case.forms()
        graphs = {f: case.graphs(f) for f in forms}
        ts = {f: [] for f in forms}
        for _ in range(a.repeats):  # interleaved: one pass over the forms per repeat
            for f in forms:
                ts[f].append(bench.timed_rotation(graphs[f], dev) / a.steps * 1e6)
        row = {"case": name, "type": fmt, "E": E, "hidden": H, "ffn": F, "S": S, "N_tok": N, "rotated_bytes": case.rotated,
               "router_weights_max_rel_diff": float(f"{diff:.3g}")}
        for f in forms:
            row[f] = {"us": round(float(np.median(ts[f])), 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2)}
        for mine, theirs in (("router", "torch_router"), ("block", "torch_block")):
            if mine in row:
                row[mine + "_slower"] = bool(row[mine]["us"] - row[theirs]["us"] >
                                             max(row[mine]["spread_us"], row[theirs]["spread_us"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del graphs, case
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"steps": a.steps, "repeats": a.repeats, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
