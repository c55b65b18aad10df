#!/usr/bin/env python3
"""An added block type beside its yardstick formats: graph-replayed step times (bench.py's method
and helpers; bench.py itself does not know these types).

    python tools/type_bench.py --type {q5_k,q3_k,q2_k,q4_0} [--steps 50] [--repeats 3] [--out FILE]
                               [--lib PATH] [--tokens 1,16,128] [--no-moe]

Step = one gq_mmq_ex call (activation quantization included), weights rotating over >= 1 GiB
(bench.rotation_plan), every replay timed alone by device events (bench.timed_rotation).  The
formats are measured interleaved, `repeats` passes over the whole table in one process, and each
cell reports the median over the passes and their spread (max - min): a difference within the
spread is not one.  Nine points: 4096^2, 11008 x 4096 and 4096 x 11008 at 1, 16 and 128 tokens.

    type   beside       the yardsticks
    q5_k   Q4_K, Q6_K   the K-quants on either side of its 176 bytes
    q3_k   Q4_K, Q6_K   Q6_K has its arithmetic, Q4_K the next size up
    q2_k   Q3_K, Q4_K   Q3_K shares its activation image
    q4_0   Q8_0, Q4_K   53% of Q8_0's bytes through the same unit partition at one token, and Q4_K's
                        bytes through the same 80-byte half image on the streaming GEMM

Then the type's extra row (TYPES below; --no-moe leaves it out): for q5_k the Llama-7B layer under
Q5_K_M beside Q4_K_M (kernels.layer_mix.LayerMix, layer 0: attn_v and ffn_down in Q6_K), for the
others one MoE row, the Mixtral gate experts (E = 8, 14336 x 4096, one token, two slots) through
gq_mmq_id (tools/moe_bench.py's case and rotation).
--lib loads another build of the library (an A/B variant, `make variant VFLAGS=...`).  Needs the
GPU: no fallback.
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
import moe_bench  # noqa: E402
from gguf.blocks import BLOCK  # noqa: E402

# type -> the formats of a row, in column order; the extra row's JSON key and its formats
TYPES = {"q5_k": dict(formats=("q4_k", "q5_k", "q6_k"), extra="layer"),
         "q3_k": dict(formats=("q3_k", "q4_k", "q6_k"), extra="moe", moe=("q3_k", "q4_k")),
         "q2_k": dict(formats=("q2_k", "q3_k", "q4_k"), extra="moe", moe=("q2_k", "q3_k", "q4_k")),
         "q4_0": dict(formats=("q4_0", "q8_0", "q4_k"), extra="moe", moe=("q4_0", "q8_0", "q4_k"))}
# byte offsets of the fp16 fields set to U(0.5, 1.5) * 2^-7 where bench.device_random_blocks does
# not know the type (q5_k, q2_k: d and dmin; q3_k, q4_0: d); every other byte stays random
_HALVES = {"q5_k": (0, 2), "q3_k": (108,), "q2_k": (80, 82), "q4_0": (0,)}
SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))
TOKENS = (1, 16, 128)


def nbytes(fmt, M, K):
    return M * (K // BLOCK[fmt][0]) * BLOCK[fmt][1]


def random_blocks(fmt, M, K, dev, seed):
    """bench.device_random_blocks with a branch for the added types."""
    if fmt not in _HALVES:
        return bench.device_random_blocks(fmt, M, K, dev, seed)
    nb = M * (K // BLOCK[fmt][0])
    g = torch.Generator(device=dev).manual_seed(seed)
    raw = torch.randint(0, 256, (nb, BLOCK[fmt][1]), dtype=torch.uint8, device=dev, generator=g)
    for off in _HALVES[fmt]:
        raw[:, off:off + 2] = ((torch.rand(nb, device=dev, generator=g) + 0.5) * 2.0 ** -7).to(torch.float16).view(
            torch.uint8).view(nb, 2)
    return raw.view(-1).view(torch.int8)


class Runner(bench.Runner):
    """bench.Runner over the library's block table (step / capture / timed are bench's)."""

    def __init__(self, fmt, M, K, N, dev, steps, seed=0):
        import kernels._lib as kl
        self.kl, self.L = kl, kl.lib()
        self.fmt, self.M, self.K, self.N, self.dev = fmt, M, K, N, dev
        self.act = kl.ACTS["q8_1"]
        self.gtype = kl.TYPES[fmt]
        self.wbytes = nbytes(fmt, M, K)
        self.ncopies, self.plans = bench.rotation_plan(self.wbytes, steps)
        self.rotated = bench.rotated_bytes(self.wbytes, self.plans)
        base = random_blocks(fmt, M, K, dev, seed)
        self.weights = [base] + [base.clone() for _ in range(self.ncopies - 1)]
        g = torch.Generator(device=dev).manual_seed(seed + 1)
        self.B = torch.randn(N, K, device=dev, generator=g).to(torch.float16)
        self.C = [torch.empty(N, M, dtype=torch.float16, device=dev) for _ in range(2)]
        self.ws_bytes = kl.workspace_size(self.gtype, M, N, K)
        self.ws = torch.empty(max(self.ws_bytes, 1), dtype=torch.uint8, device=dev)


def matrices(formats, dev, steps, repeats, shapes=SHAPES, tokens=TOKENS):
    import kernels._lib as kl
    rows = []
    for M, K in shapes:
        for N in tokens:
            runs = {f: Runner(f, M, K, N, dev, steps) for f in formats}
            graphs = {f: r.graphs(r.step) for f, r in runs.items()}
            ts = {f: [] for f in formats}
            for _ in range(repeats):  # interleaved: one pass over the formats per repeat
                for f in formats:
                    ts[f].append(bench.timed_rotation(graphs[f], dev) / steps * 1e6)
            row = {"M": M, "K": K, "N_tok": N}
            for f in formats:
                row[f] = {"us": round(float(np.median(ts[f])), 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2),
                          "route": kl.route_name(kl.TYPES[f], M, N, K),
                          "weight_GBps": round(runs[f].wbytes / np.median(ts[f]) / 1e3, 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del graphs, runs
            torch.cuda.empty_cache()
    return rows


class IdCase(moe_bench.Case):
    """moe_bench.Case over the library's block table."""

    def __init__(self, fmt, E, M, K, N, S, dev, steps):
        import kernels._lib as kl
        self.kl, self.L, self.dev = kl, kl.lib(), dev
        self.gtype, self.E, self.M, self.K, self.N, self.S = kl.TYPES[fmt], E, M, K, N, S
        self.ebytes = nbytes(fmt, M, K)
        ncopies = max(2, math.ceil(bench.ROTATE_BYTES / (E * self.ebytes)))
        base = random_blocks(fmt, E * M, K, dev, 1)
        self.A = [base] + [base.clone() for _ in range(ncopies - 1)]
        self.sets = moe_bench.tiles(E, N, S, 1)
        self.ids = [torch.from_numpy(s).to(dev) for s in self.sets]
        g = torch.Generator(device=dev).manual_seed(2)
        self.B = torch.randn((N, K), device=dev, generator=g).to(torch.float16)
        self.ldb, self.ldb_slot = K, 0
        self.C = torch.empty((N, S, M), dtype=torch.float16, device=dev)
        self.share = 1
        self.step_bytes = len(np.unique(self.sets[0])) * self.ebytes
        combos = [(c, j) for c in range(ncopies) for j in range(len(self.sets))]
        G = max(1, math.ceil(len(combos) / steps))
        self.plans = [[combos[(g_ * steps + i) % len(combos)] for i in range(steps)] for g_ in range(G)]
        self.rotated = ncopies * E * self.ebytes
        self.items = {}


def moe_row(formats, dev, steps, repeats):
    E, M, K, N, S = 8, 14336, 4096, 1, 2
    cases = {f: IdCase(f, E, M, K, N, S, dev, steps) for f in formats}
    graphs = {}
    for f, c in cases.items():
        c.step("id", 0, 0)  # (first use outside the capture)
        torch.cuda.synchronize(dev)
        graphs[f] = c.graphs("id")
    ts = {f: [] for f in cases}
    for _ in range(repeats):
        for f in cases:
            ts[f].append(bench.timed_rotation(graphs[f], dev) / steps * 1e6)
    row = {"case": "mixtral gate, gq_mmq_id", "E": E, "M": M, "K": K, "N_tok": N, "S": S}
    for f, c in cases.items():
        row[f] = {"us": round(float(np.median(ts[f])), 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2),
                  "weight_GBps": round(c.step_bytes / np.median(ts[f]) / 1e3, 1)}
    print(json.dumps(row), flush=True)
    return row


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
    ap.add_argument("--type", required=True, choices=sorted(TYPES))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libgguf_mmq.so (A/B variants)")
    ap.add_argument("--tokens", default=None, help="comma-separated token counts (default 1,16,128)")
    ap.add_argument("--no-moe", dest="no_extra", action="store_true", help="leave the type's extra row out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("type_bench needs a ROCm GPU (no CPU timing)")
    if a.lib:
        import kernels._lib as kl
        kl.LIB_PATH = os.path.abspath(a.lib)
    dev = torch.device("cuda:0")
    t = TYPES[a.type]
    tokens = tuple(int(n) for n in a.tokens.split(",")) if a.tokens else TOKENS
    res = {"steps": a.steps, "repeats": a.repeats, "lib": a.lib,
           "matrices": matrices(t["formats"], dev, a.steps, a.repeats, tokens=tokens)}
    if not a.no_extra:
        res[t["extra"]] = layer(dev, a.steps, a.repeats) if t["extra"] == "layer" else moe_row(t["moe"], dev, a.steps, a.repeats)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
