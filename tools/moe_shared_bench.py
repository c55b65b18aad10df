#!/usr/bin/env python3
"""The dense GLU decode launch (kernels._lib.mmq_glu: gq_mmq_glu) beside the two gq_mmq launches and
the torch GLU it replaces, and a MoE block with a shared expert (kernels/moe.py MoEBlock(shared=...))
fused beside its unfused composition.  Graph-replayed step times (bench.py's method and helpers;
bench.py itself does not know either).

    python tools/moe_shared_bench.py [--steps 20] [--repeats 3] [--only glu|block] [--out shared.json]

glu rows: Q4_K 11008 x 4096 (a 7B FFN's gate and up) at N = 1, 2, 4 -- "glu" is one mmq_glu call,
"two_mmq" two mmq calls and torch's silu(g) * u.  block rows: a Qwen-MoE-like block (E = 60, hidden
2048, routed ffn 1536, S = 4, shared ffn 5632, Q4_K, with the per-token gate of the shared term) --
"fused" is MoEBlock over MoEFFN(fused=True) and DenseFFN(fused=True) (nine launches), "unfused" the
same block over fused=False parts (its torch lines).  The weights rotate over copies holding
>= 1 GiB together, every step of a graph has an x of its own, every replay is timed alone by device
events (bench.timed_rotation); the forms are measured interleaved in one process, `repeats` passes,
and each cell is the median over the passes with their spread (max - min).  "slower" is true when
the fused form exceeds the other by more than the larger of the two spreads.  Needs the GPU.
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

Q4K_BYTES = 144  # per 256 weights

GLU_CASES = [("q4_k", 11008, 4096, N) for N in (1, 2, 4)]
# (name, E, hidden, routed ffn, S, shared ffn, N)
BLOCK_CASES = [("qwen-moe-like", 60, 2048, 1536, 4, 5632, 1), ("qwen-moe-like", 60, 2048, 1536, 4, 5632, 4)]


def _xs(n, N, K, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    # (random block bits make weights of a few units: small activations keep silu(g) * u in fp16 range)
    return [(torch.randn((N, K), device=dev, generator=gen) / 1024).to(torch.float16) for _ in range(n)]


class GluCase:
    def __init__(self, fmt, M, K, N, dev, steps):
        import kernels._lib as kl
        self.kl, self.dev, self.M, self.K, self.N = kl, dev, M, K, N
        self.gtype = kl.TYPES[fmt]
        wbytes = 2 * M * (K // 256) * Q4K_BYTES
        ncopies, self.plans = bench.rotation_plan(wbytes, steps)
        self.rotated = bench.rotated_bytes(wbytes, self.plans)
        self.w = [(bench.device_random_blocks(fmt, M, K, dev, 2 * c), bench.device_random_blocks(fmt, M, K, dev, 2 * c + 1))
                  for c in range(ncopies)]
        self.x = _xs(steps, N, K, dev, 5)
        self.h = torch.empty((N, M), dtype=torch.float16, device=dev)

    def step(self, form, c, i):
        kl, (Ag, Au), x = self.kl, self.w[c], self.x[i]
        if form == "glu":
            return kl.mmq_glu(self.gtype, Ag, Au, x, self.M, self.N, self.K, out=self.h)
        g, u = kl.mmq(self.gtype, Ag, x, self.M, self.N, self.K), kl.mmq(self.gtype, Au, x, self.M, self.N, self.K)
        return torch.nn.functional.silu(g) * u

    def check(self):
        """The entry must take the shape (no fallback is being timed), and the two forms agree up
        to the rounding the fused one leaves out."""
        Ag, Au = self.w[0]
        rc = self.kl.lib().gq_mmq_glu(self.gtype, Ag.data_ptr(), Au.data_ptr(), self.x[0].data_ptr(), self.h.data_ptr(),
                                      self.M, self.N, self.K, self.K, self.M, None)
        assert rc == self.kl.GQ_OK, self.kl.lib().gq_last_error()
        a, b = self.step("two_mmq", 0, 0).float(), self.step("glu", 0, 0).float()
        torch.cuda.synchronize(self.dev)
        assert torch.isfinite(a).all() and torch.isfinite(b).all() and float(a.abs().max()) > 0
        d = float((a - b).abs().max() / a.abs().max())
        assert d <= 2e-3, d
        return d


class BlockCase:
    def __init__(self, E, H, F, S, Fs, N, dev, steps):
        from kernels.ffn import DenseFFN
        from kernels.layer_mix import GGUFLinear
        from kernels.moe import GGUFExperts, MoEBlock, MoEFFN, MoERouter
        self.dev, self.N = dev, N
        fmt = "q4_k"
        wbytes = (3 * E * F * (H // 256) + 3 * Fs * (H // 256)) * Q4K_BYTES
        ncopies, self.plans = bench.rotation_plan(wbytes, steps)
        self.rotated = bench.rotated_bytes(wbytes, self.plans)
        gen = torch.Generator(device=dev).manual_seed(3)
        Wr = torch.randn((E, H), device=dev, generator=gen)
        v = torch.randn((H,), device=dev, generator=gen)
        router = MoERouter(Wr, S)
        self.blocks = []
        for c in range(ncopies):
            rb = lambda rows, K, s: bench.device_random_blocks(fmt, rows, K, dev, 100 * c + s)  # noqa: E731
            ex = (GGUFExperts(fmt, rb(E * F, H, 1), E, F, H), GGUFExperts(fmt, rb(E * F, H, 2), E, F, H),
                  GGUFExperts(fmt, rb(E * H, F, 3), E, H, F))
            sh = (GGUFLinear(fmt, rb(Fs, H, 4), Fs, H), GGUFLinear(fmt, rb(Fs, H, 5), Fs, H), GGUFLinear(fmt, rb(H, Fs, 6), H, Fs))
            self.blocks.append({f: MoEBlock(router, MoEFFN(*ex, fused=f), DenseFFN(*sh, fused=f), v) for f in (False, True)})
        self.x = _xs(steps, N, H, dev, 7)

    def step(self, form, c, i):
        return self.blocks[c][form == "fused"].forward(self.x[i])

    def check(self):
        a, b = self.step("unfused", 0, 0).float(), self.step("fused", 0, 0).float()
        torch.cuda.synchronize(self.dev)
        assert torch.isfinite(a).all() and torch.isfinite(b).all() and float(a.abs().max()) > 0
        d = float((a - b).abs().max() / a.abs().max())
        assert d <= 2e-2, d
        return d


def graphs(case, form):
    grs = []
    for plan in case.plans:
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for i, c in enumerate(plan):
                case.step(form, c, i)
        grs.append(gr)
    return grs


def measure(case, forms, steps, repeats, dev):
    diff = case.check()
    gs = {f: graphs(case, f) for f in forms}
    ts = {f: [] for f in forms}
    for _ in range(repeats):  # interleaved: one pass over the forms per repeat
        for f in forms:
            ts[f].append(bench.timed_rotation(gs[f], dev) / steps * 1e6)
    row = {"rotated_bytes": case.rotated, "max_rel_diff": round(diff, 5)}
    for f in forms:
        row[f] = {"us": round(float(np.median(ts[f])), 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2)}
    a, b = forms
    row["slower"] = bool(row[a]["us"] - row[b]["us"] > max(row[a]["spread_us"], row[b]["spread_us"]))
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("glu", "block"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_shared_bench needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda:0")
    rows = []
    if a.only in (None, "glu"):
        for fmt, M, K, N in GLU_CASES:
            case = GluCase(fmt, M, K, N, dev, a.steps)
            row = {"what": "glu", "type": fmt, "M": M, "K": K, "N_tok": N, **measure(case, ("glu", "two_mmq"), a.steps, a.repeats, dev)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del case
            torch.cuda.empty_cache()
    if a.only in (None, "block"):
        for name, E, H, F, S, Fs, N in BLOCK_CASES:
            case = BlockCase(E, H, F, S, Fs, N, dev, a.steps)
            row = {"what": "block", "case": name, "type": "q4_k", "E": E, "hidden": H, "ffn": F, "S": S, "shared_ffn": Fs,
                   "N_tok": N, **measure(case, ("fused", "unfused"), a.steps, a.repeats, dev)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del case
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"steps": a.steps, "repeats": a.repeats, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
