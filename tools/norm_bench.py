#!/usr/bin/env python3
"""The fused residual add + RMSNorm (kernels._lib.rmsnorm / rmsnorm_prepare: gq_rmsnorm,
gq_rmsnorm_prepare) beside the torch lines it replaces, and DenseFFN.forward_normed beside torch's
norm + DenseFFN.forward.  Graph-replayed step times (bench.py's method and helpers; bench.py itself
does not know either).

    python tools/norm_bench.py [--steps 50] [--repeats 5] [--only norm|ffn] [--out norm.json]

norm rows, (N, K) = (1, 4096), (4, 4096), (16, 4096), (128, 4096), (512, 4096), (128, 11008): the
input of a projection group from x and the residual to prepared q8_1 activations, three ways --
  "torch"   h = x + r, y = (h.float() * rsqrt(mean(h.float()^2) + eps) * w).half() in torch ops, then
            act_prepare(y): what a caller did before these entries (the comparison base);
  "norm"    rmsnorm(x, w, eps, r, h_out) then act_prepare(y): two launches;
  "fused"   rmsnorm_prepare(x, w, eps, ws, r, h_out): one launch.
All three leave h and the workspace; y itself is stored by the first two only.  Every step of a
graph has an x and an r of its own (nothing else rotates: a layer's hidden state is as cache-warm in
a model); every replay is timed alone by device events (bench.timed_rotation), the forms are
measured interleaved in one process, `repeats` passes, and each cell is the median over the passes
with their spread (max - min).
ffn rows: Q4_K gate / up 11008 x 4096 and down 4096 x 11008 at N = 16 and 128 -- "normed" is
DenseFFN.forward_normed(x, r), "torch" the torch lines above and DenseFFN.forward(y); the weights
rotate over copies holding >= 1 GiB together.  Needs the GPU.
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

EPS = 1e-5
NORM_CASES = [(1, 4096), (4, 4096), (16, 4096), (128, 4096), (512, 4096), (128, 11008)]
FFN_CASES = [("q4_k", 4096, 11008, N) for N in (16, 128)]
Q4K_BYTES = 144  # per 256 weights


def torch_norm(x, r, w, eps=EPS):
    """(y, h) in torch ops: the path before gq_rmsnorm."""
    h = x + r
    f = h.float()
    return (f * torch.rsqrt(f.pow(2).mean(-1, keepdim=True) + eps) * w).half(), h


def _xs(n, N, K, dev, seed, scale=1.0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return [(torch.randn((N, K), device=dev, generator=gen) * scale).to(torch.float16) for _ in range(n)]


class NormCase:
    forms = ("torch", "norm", "fused")

    def __init__(self, N, K, dev, steps):
        import kernels._lib as kl
        self.kl, self.dev, self.N, self.K = kl, dev, N, K
        self.x, self.r = _xs(steps, N, K, dev, 1), _xs(steps, N, K, dev, 2)
        gen = torch.Generator(device=dev).manual_seed(3)
        self.w = 1 + 0.3 * torch.randn((K,), device=dev, generator=gen)
        self.ws = torch.empty(kl.workspace_size(kl.GQ_Q4_K, 4096, N, K), dtype=torch.uint8, device=dev)
        self.h = torch.empty((N, K), dtype=torch.float16, device=dev)
        self.y = torch.empty((N, K), dtype=torch.float16, device=dev)
        self.plans = [list(range(steps))]

    def step(self, form, c, i):
        kl, x, r = self.kl, self.x[i], self.r[i]
        if form == "fused":
            kl.rmsnorm_prepare(x, self.w, EPS, self.ws, r, h_out=self.h)
        elif form == "norm":
            kl.act_prepare(kl.rmsnorm(x, self.w, EPS, r, out=self.y, h_out=self.h), self.N, self.K, self.ws)
        else:
            y, _ = torch_norm(x, r, self.w)
            kl.act_prepare(y, self.N, self.K, self.ws)

    def check(self):
        """"norm" and "fused" leave the same workspace bytes; torch's y is within 1 fp16 ulp-ish."""
        self.step("norm", 0, 0)
        a = self.ws.clone()
        self.step("fused", 0, 0)
        torch.cuda.synchronize(self.dev)
        need = int(self.kl.lib().gq_mmq_workspace_size_ex(self.kl.GQ_Q4_K, 0, 4096, self.N, self.K))
        assert need == self.ws.numel()
        y, _ = torch_norm(self.x[0], self.r[0], self.w)
        d = float((y.float() - self.y.float()).abs().max() / self.y.float().abs().max())
        assert d <= 2e-3, d
        # (the bytes behind the activation part are never written by either: equal garbage)
        assert torch.equal(a, self.ws), "rmsnorm + act_prepare and rmsnorm_prepare disagree"
        return d


class FFNCase:
    forms = ("torch", "normed")

    def __init__(self, fmt, H, F, N, dev, steps):
        from kernels.ffn import DenseFFN
        from kernels.layer_mix import GGUFLinear
        from kernels.norm import RMSNorm
        self.dev, self.N = dev, N
        wbytes = 3 * F * (H // 256) * Q4K_BYTES
        ncopies, self.plans = bench.rotation_plan(wbytes, steps)
        self.rotated = bench.rotated_bytes(wbytes, self.plans)
        gen = torch.Generator(device=dev).manual_seed(3)
        # (random block bits make weights of a few units: a small norm weight keeps silu(g) * u in fp16 range)
        self.norm = RMSNorm((1 + 0.3 * torch.randn((H,), device=dev, generator=gen)) / 1024, EPS)
        rb = lambda rows, K, s: bench.device_random_blocks(fmt, rows, K, dev, s)  # noqa: E731
        self.ffn = [DenseFFN(GGUFLinear(fmt, rb(F, H, 10 * c + 1), F, H), GGUFLinear(fmt, rb(F, H, 10 * c + 2), F, H),
                             GGUFLinear(fmt, rb(H, F, 10 * c + 3), H, F), norm=self.norm) for c in range(ncopies)]
        self.x, self.r = _xs(steps, N, H, dev, 5), _xs(steps, N, H, dev, 6)

    def step(self, form, c, i):
        if form == "normed":
            return self.ffn[c].forward_normed(self.x[i], self.r[i])[0]
        y, _ = torch_norm(self.x[i], self.r[i], self.norm.weight)
        return self.ffn[c].forward(y)

    def check(self):
        a, b = self.step("torch", 0, 0).float(), self.step("normed", 0, 0).float()
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


def measure(case, steps, repeats, dev):
    diff = case.check()
    gs = {f: graphs(case, f) for f in case.forms}
    ts = {f: [] for f in case.forms}
    for _ in range(repeats):  # interleaved: one pass over the forms per repeat
        for f in case.forms:
            ts[f].append(bench.timed_rotation(gs[f], dev) / steps * 1e6)
    row = {"max_rel_diff": round(diff, 5)}
    for f in case.forms:
        row[f] = {"us": round(float(np.median(ts[f])), 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2)}
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, choices=("norm", "ffn"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("norm_bench.py needs a ROCm device: there is no CPU timing path")
    dev = torch.device("cuda:0")
    rows = []
    if a.only in (None, "norm"):
        for N, K in NORM_CASES:
            row = {"case": "norm", "N": N, "K": K, **measure(NormCase(N, K, dev, a.steps), a.steps, a.repeats, dev)}
            row["fused_slower_than_norm"] = bool(row["fused"]["us"] - row["norm"]["us"] >
                                                 max(row["fused"]["spread_us"], row["norm"]["spread_us"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.only in (None, "ffn"):
        for fmt, H, F, N in FFN_CASES:
            case = FFNCase(fmt, H, F, N, dev, a.steps)
            row = {"case": "ffn", "fmt": fmt, "hidden": H, "ffn": F, "N": N, "rotated_bytes": case.rotated,
                   **measure(case, a.steps, a.repeats, dev)}
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
