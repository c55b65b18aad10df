#!/usr/bin/env python3
"""The fused MoE decode block (kernels/moe.py MoEFFN(fused=True): gq_mmq_id_glu, gq_mmq_id,
gq_moe_combine) beside the unfused one (fused=False: three gq_mmq_id and four torch kernels), and
the GLU launch alone beside the two gq_mmq_id launches it replaces.  Graph-replayed step times
(bench.py's method and helpers; bench.py itself does not know the block).

    python tools/moe_fused_bench.py [--steps 20] [--repeats 3] [--only mixtral] [--out moe_fused.json]

Step = one MoEFFN.forward over N tokens x S slots.  A step reads only the chosen experts, so the
three expert tensors rotate over copies holding >= 1 GiB together and every step of every graph
has ids of its own, drawn once (distinct experts per token).  Every replay is timed alone by
device events (bench.timed_rotation); the forms are measured interleaved in one process, `repeats`
passes, and each cell is the median over the passes with their spread (max - min).  A row's
"fused_slower" is true when fused - unfused exceeds the larger of the two spreads.  Needs the GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gguf-triton-kernel_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402

BLOCK = {"q4_k": (256, 144), "q2_k": (256, 84)}
_HALVES = {"q4_k": (0, 2), "q2_k": (80, 82)}  # the blocks' fp16 fields

# (name, type, E, hidden, ffn, S, N)
CASES = [
    ("mixtral", "q4_k", 8, 4096, 14336, 2, 1),
    ("mixtral", "q4_k", 8, 4096, 14336, 2, 4),
    ("mixtral", "q2_k", 8, 4096, 14336, 2, 1),
    ("mixtral", "q2_k", 8, 4096, 14336, 2, 4),
    # (Qwen1.5-MoE's ffn is 1408, no multiple of a 256-weight super-block: its Q4_K files keep the
    # down experts in another type; 1536 is the nearest size all three projections take as Q4_K)
    ("qwen-moe-like", "q4_k", 60, 2048, 1536, 4, 1),
    ("qwen-moe-like", "q4_k", 60, 2048, 1536, 4, 8),
]


def random_blocks(fmt, rows, K, dev, seed):
    """Random packed blocks made on the device; fp16 fields = U(0.5, 1.5) * 2^-7."""
    nb, nbytes = rows * (K // BLOCK[fmt][0]), BLOCK[fmt][1]
    g = torch.Generator(device=dev).manual_seed(seed)
    raw = torch.randint(0, 256, (nb, nbytes), dtype=torch.uint8, device=dev, generator=g)
    for off in _HALVES[fmt]:
        raw[:, off:off + 2] = ((torch.rand(nb, device=dev, generator=g) + 0.5) * 2.0 ** -7).to(torch.float16).view(
            torch.uint8).view(nb, 2)
    return raw.view(-1).view(torch.int8)


class Case:
    def __init__(self, fmt, E, H, F, S, N, dev, steps):
        import kernels._lib as kl
        from kernels.moe import GGUFExperts, MoEFFN
        self.kl, self.dev, self.fmt, self.E, self.H, self.F, self.S, self.N = kl, dev, fmt, E, H, F, S, N
        self.gtype = kl.TYPES[fmt]
        ebytes = F * (H // 256) * BLOCK[fmt][1]  # (gate, up and down experts: the same size)
        self.step_bytes = 3 * min(E, N * S) * ebytes
        ncopies, self.plans = bench.rotation_plan(3 * E * ebytes, steps)
        self.rotated = bench.rotated_bytes(3 * E * ebytes, self.plans)
        base = [random_blocks(fmt, E * F, H, dev, 1), random_blocks(fmt, E * F, H, dev, 2),
                random_blocks(fmt, E * H, F, dev, 3)]
        self.blocks = []
        for c in range(ncopies):
            g, u, d = (t if c == 0 else t.clone() for t in base)
            parts = (GGUFExperts(fmt, g, E, F, H), GGUFExperts(fmt, u, E, F, H), GGUFExperts(fmt, d, E, H, F))
            self.blocks.append({False: MoEFFN(*parts), True: MoEFFN(*parts, fused=True)})
        rng = np.random.default_rng(4)
        self.ids = [[torch.from_numpy(np.stack([rng.permutation(E)[:S] for _ in range(N)]).astype(np.int32)).to(dev)
                     for _ in plan] for plan in self.plans]
        gen = torch.Generator(device=dev).manual_seed(5)
        # (random block bits make weights of a few units: small activations keep g*u and d in fp16 range)
        self.x = (torch.randn((N, H), device=dev, generator=gen) / 1024).to(torch.float16)
        self.w = torch.softmax(torch.randn((N, S), device=dev, generator=gen), dim=1).to(torch.float16)
        self.h = torch.empty((N, S, F), dtype=torch.float16, device=dev)
        self.g = torch.empty((N, S, F), dtype=torch.float16, device=dev)

    def step(self, form, c, ids):
        b, kl = self.blocks[c], self.kl
        if form in ("unfused", "fused"):
            return b[form == "fused"].forward(self.x, ids, self.w)
        gate, up = b[False].gate, b[False].up
        if form == "glu":
            return kl.mmq_id_glu(self.gtype, gate.A, up.A, ids, self.x, self.E, self.F, self.H, out=self.h)
        kl.mmq_id(self.gtype, gate.A, ids, self.x, self.E, self.F, self.H, out=self.g)
        return kl.mmq_id(self.gtype, up.A, ids, self.x, self.E, self.F, self.H, out=self.h)

    def check(self):
        """The fused block against the unfused one: the same g, u and d up to the roundings the
        fused form leaves out (compared loosely; tests/test_gpu_moe_fused.py is the judge)."""
        a = self.step("unfused", 0, self.ids[0][0]).float()
        b = self.step("fused", 0, self.ids[0][0]).float()
        torch.cuda.synchronize(self.dev)
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        d = float((a - b).abs().max() / a.abs().max())
        assert d <= 2e-2, d
        return d

    def graphs(self, form):
        grs = []
        for plan, ids in zip(self.plans, self.ids):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for c, it in zip(plan, ids):
                    self.step(form, c, it)
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
        raise SystemExit("moe_fused_bench needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda:0")
    forms = ("unfused", "fused", "two_id", "glu")
    rows = []
    for name, fmt, E, H, F, S, N in CASES:
        if a.only and a.only not in name and a.only != fmt:
            continue
        case = Case(fmt, E, H, F, S, N, dev, a.steps)
        diff = case.check()
        graphs = {f: case.graphs(f) for f in forms}
        ts = {f: [] for f in forms}
        for _ in range(a.repeats):  # interleaved: one pass over the forms per repeat
            for f in forms:
                ts[f].append(bench.timed_rotation(graphs[f], dev) / a.steps * 1e6)
        row = {"case": name, "type": fmt, "E": E, "hidden": H, "ffn": F, "S": S, "N_tok": N, "pairs": N * S,
               "rotated_bytes": case.rotated, "fused_vs_unfused_max_rel_diff": round(diff, 5)}
        for f in forms:
            row[f] = {"us": round(float(np.median(ts[f])), 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2)}
        row["fused_slower"] = bool(row["fused"]["us"] - row["unfused"]["us"] >
                                   max(row["fused"]["spread_us"], row["unfused"]["spread_us"]))
        row["glu_slower_than_two_id"] = bool(row["glu"]["us"] - row["two_id"]["us"] >
                                             max(row["glu"]["spread_us"], row["two_id"]["spread_us"]))
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
