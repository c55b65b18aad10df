#!/usr/bin/env python3
"""Decode attention (kernels._lib.attn_decode: gq_attn_decode) over an fp16 and a Q8_0 KV cache beside
the base a caller has today, torch.nn.functional.scaled_dot_product_attention over the same fp16 cache
sliced to the length.  The base has no Q8_0 form: torch has no kernel that reads Q8_0 blocks.
Graph-replayed step times (bench.py's method and helpers; bench.py itself does not know the entry).

    python tools/attn_bench.py [--steps 20] [--repeats 3] [--out profiles/attn_bench.json] [--max-len 32768]

Cases: Llama-3-8B heads (32 query / 8 kv, D 128) and Llama-2-7B heads (32 / 32, D 128), N in {1, 4} new
tokens, B in {1, 4} sequences, kv_len in {512, 4096, 32768}; token-major caches exactly kv_len long.
Every step of a graph reads another copy of the caches, the copies together holding >= 1 GiB
(bench.rotation_plan), so no step finds its cache in the Infinity Cache; q and the workspace do not
rotate.  Every replay is timed alone by device events (bench.timed_rotation), the three forms are
measured interleaved in one process, `repeats` passes; a cell is the median over the passes, their
spread (max - min), and the live cache bytes (K and V rows below kv_len) per second against the HBM
figure bench.py uses.  Needs the GPU.
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

HEADS = {"llama3_8b": (32, 8, 128), "llama2_7b": (32, 32, 128)}
FORMS = ("torch", "f16", "q8_0")


class Case:
    def __init__(self, nh, kvh, D, N, B, L, dev, steps):
        import kernels._lib as kl
        self.kl, self.dev, self.dims = kl, dev, (nh, kvh, D, N, B, L)
        self.live = {k: 2 * B * L * kvh * kl.kv_row_bytes(k, D) for k in ("f16", "q8_0")}
        ncopies, self.plans = bench.rotation_plan(self.live["q8_0"], steps)
        gen = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(torch.float16)  # noqa: E731
        self.f16 = [(rnd(B, L, kvh, D), rnd(B, L, kvh, D)) for _ in range(ncopies)]
        self.q8 = [tuple(bench.device_random_blocks("q8_0", B * L * kvh, D, dev, 10 * c + s) for s in (0, 1))
                   for c in range(ncopies)]
        self.q = rnd(B * N, nh * D)
        self.kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
        self.ws = torch.empty(kl.attn_workspace_size(B, N, nh, kvh, D), dtype=torch.uint8, device=dev)
        self.out = torch.empty(B * N, nh * D, dtype=torch.float16, device=dev)
        # the N new tokens sit at the cache's end: query i sees positions 0 .. L - N + i
        self.mask = None if N == 1 else torch.ones(N, L, dtype=torch.bool, device=dev).tril(L - N)

    def step(self, form, c, i):
        nh, kvh, D, N, B, L = self.dims
        if form == "torch":
            k, v = (t.permute(0, 2, 1, 3) for t in self.f16[c])
            q = self.q.view(B, N, nh, D).permute(0, 2, 1, 3)
            o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=self.mask, enable_gqa=nh != kvh)
            return o.permute(0, 2, 1, 3).reshape(B * N, nh * D)
        k, v = self.f16[c] if form == "f16" else self.q8[c]
        rb = self.kl.kv_row_bytes(form, D)
        return self.kl.attn_decode(form, self.q, k, v, (kvh * rb, rb, L * kvh * rb), self.kv_len, L, B, N, nh, kvh, D,
                                   self.ws, out=self.out)

    def check(self):
        a, b = self.step("torch", 0, 0).float(), self.step("f16", 0, 0).float()
        torch.cuda.synchronize(self.dev)
        d = float((a - b).abs().max() / a.abs().max())
        assert d <= 1e-2, d
        assert torch.isfinite(self.step("q8_0", 0, 0)).all()
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


def measure(case, steps, repeats, dev):
    diff = case.check()
    gs = {f: graphs(case, f) for f in FORMS}
    ts = {f: [] for f in FORMS}
    for _ in range(repeats):  # interleaved: one pass over the forms per repeat
        for f in FORMS:
            ts[f].append(bench.timed_rotation(gs[f], dev) / steps * 1e6)
    row = {"f16_vs_torch_max_rel_diff": round(diff, 5)}
    for f in FORMS:
        us = float(np.median(ts[f]))
        gbs = case.live["q8_0" if f == "q8_0" else "f16"] / us / 1e3
        row[f] = {"us": round(us, 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2), "cache_GBs": round(gbs, 1),
                  "hbm_frac": round(gbs / bench.HBM_PEAK_GBS, 4)}
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-len", type=int, default=32768)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_bench.py needs a ROCm device: there is no CPU timing path")
    dev = torch.device("cuda:0")
    rows = []
    for name, (nh, kvh, D) in HEADS.items():
        for L in (512, 4096, 32768):
            for B in (1, 4):
                for N in (1, 4):
                    if L > a.max_len:
                        continue
                    case = Case(nh, kvh, D, N, B, L, dev, a.steps)
                    row = {"heads": name, "N": N, "B": B, "kv_len": L, **measure(case, a.steps, a.repeats, dev)}
                    row["f16_slower_than_torch"] = bool(row["f16"]["us"] - row["torch"]["us"] >
                                                        max(row["f16"]["spread_us"], row["torch"]["spread_us"]))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del case
                    torch.cuda.empty_cache()
                    if a.out:  # (after every cell: a run cut short keeps what it measured)
                        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                        with open(a.out, "w") as f:
                            json.dump({"steps": a.steps, "repeats": a.repeats, "hbm_peak_GBs": bench.HBM_PEAK_GBS,
                                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
