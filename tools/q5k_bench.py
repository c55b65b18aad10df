#!/usr/bin/env python3
"""Q5_K beside Q4_K and Q6_K: graph-replayed step times (bench.py's method and helpers; bench.py
itself does not know the type).

    python tools/q5k_bench.py [--steps 50] [--repeats 3] [--out q5k_bench.json]

Step = one gq_mmq_ex call (activation quantization included), weights rotating over >= 1 GiB
(bench.rotation_plan), every replay timed alone by device events (bench.timed_rotation).  The
formats are measured interleaved, `repeats` passes over the whole table in one process, and each
cell reports the median over the passes and their spread (max - min): a difference within the
spread is not one.  Then the Llama-7B layer under Q5_K_M beside Q4_K_M (kernels.layer_mix.LayerMix,
layer 0: attn_v and ffn_down in Q6_K).  Needs the GPU: no fallback.
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

BLOCK = {"q4_k": (256, 144), "q5_k": (256, 176), "q6_k": (256, 210)}
SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))
TOKENS = (1, 16, 128)


def random_blocks(fmt, M, K, dev, seed):
    """bench.device_random_blocks with a q5_k branch (d and dmin as for q4_k)."""
    if fmt != "q5_k":
        return bench.device_random_blocks(fmt, M, K, dev, seed)
    nb = M * (K // 256)
    g = torch.Generator(device=dev).manual_seed(seed)
    raw = torch.randint(0, 256, (nb, 176), dtype=torch.uint8, device=dev, generator=g)
    for o in (0, 2):
        raw[:, o:o + 2] = ((torch.rand(nb, device=dev, generator=g) + 0.5) * 2.0 ** -7).to(torch.float16).view(
            torch.uint8).view(nb, 2)
    return raw.view(-1).view(torch.int8)


class Runner(bench.Runner):
    """bench.Runner over this script's block table (step / capture / timed are bench's)."""

    def __init__(self, fmt, M, K, N, dev, steps, seed=0):
        import kernels._lib as kl
        self.kl, self.L = kl, kl.lib()
        self.fmt, self.M, self.K, self.N, self.dev = fmt, M, K, N, dev
        self.act = kl.ACTS["q8_1"]
        self.gtype = kl.TYPES[fmt]
        self.wbytes = M * (K // 256) * BLOCK[fmt][1]
        self.ncopies, self.plans = bench.rotation_plan(self.wbytes, steps)
        self.rotated = bench.rotated_bytes(self.wbytes, self.plans)
        base = random_blocks(fmt, M, K, dev, seed)
        self.weights = [base] + [base.clone() for _ in range(self.ncopies - 1)]
        g = torch.Generator(device=dev).manual_seed(seed + 1)
        self.B = torch.randn(N, K, device=dev, generator=g).to(torch.float16)
        self.C = [torch.empty(N, M, dtype=torch.float16, device=dev) for _ in range(2)]
        self.ws_bytes = kl.workspace_size(self.gtype, M, N, K)
        self.ws = torch.empty(max(self.ws_bytes, 1), dtype=torch.uint8, device=dev)


def matrices(dev, steps, repeats):
    import kernels._lib as kl
    rows = []
    for M, K in SHAPES:
        for N in TOKENS:
            runs = {f: Runner(f, M, K, N, dev, steps) for f in BLOCK}
            graphs = {f: r.graphs(r.step) for f, r in runs.items()}
            ts = {f: [] for f in BLOCK}
            for _ in range(repeats):  # interleaved: one pass over the formats per repeat
                for f in BLOCK:
                    ts[f].append(bench.timed_rotation(graphs[f], dev) / steps * 1e6)
            row = {"M": M, "K": K, "N_tok": N}
            for f in BLOCK:
                row[f] = {"us": round(float(np.median(ts[f])), 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2),
                          "route": kl.route_name(kl.TYPES[f], M, N, K),
                          "weight_GBps": round(runs[f].wbytes / np.median(ts[f]) / 1e3, 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del graphs, runs
            torch.cuda.empty_cache()
    return rows


def layer(dev, steps, repeats, Ns=(1, 8, 128)):
    from gguf import LLAMA_LAYER_SHAPES, q4_k_m_layer_types, q5_k_m_layer_types
    from kernels.layer_mix import GGUFLinear, LayerMix
    out = []
    for mix, types in (("q4_k_m", q4_k_m_layer_types(0, 32)), ("q5_k_m", q5_k_m_layer_types(0, 32))):
        one = {n: random_blocks(types[n], M, K, dev, seed=i) for i, (n, (M, K)) in enumerate(LLAMA_LAYER_SHAPES.items())}
        layer_bytes = sum(t.numel() for t in one.values())
        ncopies, plans = bench.rotation_plan(layer_bytes, steps)
        layers = [LayerMix({n: GGUFLinear(types[n], one[n] if c == 0 else one[n].clone(), *LLAMA_LAYER_SHAPES[n])
                            for n in LLAMA_LAYER_SHAPES}) for c in range(ncopies)]
        for N in Ns:
            g = torch.Generator(device=dev).manual_seed(7)
            x = torch.randn(N, 4096, device=dev, generator=g).to(torch.float16)
            h = torch.randn(N, 11008, device=dev, generator=g).to(torch.float16)
            outs = {n: torch.empty(N, M, dtype=torch.float16, device=dev) for n, (M, K) in LLAMA_LAYER_SHAPES.items()
                    if n not in layers[0].parts}
            for i in range(ncopies):  # library handles, every copy's buffers: outside capture
                layers[i].forward(x, h, out=outs)
            torch.cuda.synchronize(dev)
            grs = []
            for p in plans:
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for c in p:
                        layers[c].forward(x, h, out=outs)
                grs.append(gr)
            ts = [bench.timed_rotation(grs, dev) / steps * 1e6 for _ in range(repeats)]
            rec = {"mix": mix, "N_tok": N, "us": round(float(np.median(ts)), 2), "spread_us": round(max(ts) - min(ts), 2),
                   "weight_bytes": layer_bytes}
            out.append(rec)
            print(json.dumps(rec), flush=True)
            del grs
        del layers, one
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-layer", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("q5k_bench needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda:0")
    res = {"steps": a.steps, "repeats": a.repeats, "matrices": matrices(dev, a.steps, a.repeats)}
    if not a.no_layer:
        res["layer"] = layer(dev, a.steps, a.repeats)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
