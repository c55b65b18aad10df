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

    python tools/attn_bench.py --prefill [--steps 10] [--out profiles/attn_prefill_bench.json]

Prefill attention (kernels._lib.attn_prefill: gq_attn_prefill) by the same method: the same heads, B = 1,
N in {128, 512, 2048, 8192} new tokens without a prefix and 512 after a prefix of 4096, and one B = 4
cell; a cell is the median time, its spread, the causal TFLOP/s (4 D flops per attended (row, key) pair)
and that as a share of bench.py's MFMA_F16_PEAK_TF (PrefillCase).

    python tools/attn_bench.py --rope [--steps 20] [--out profiles/rope_bench.json]

The fused per-head norm + RoPE + KV append (kernels._lib.rope_append: gq_rope_append) beside the path a
caller had before it: torch RoPE from a position tensor (arange + kv_len - N, outer product, cos, sin,
rotate, cast), the torch per-head RMSNorm where the model has one, then kv_append (RopeCase).  Llama-3-8B
heads (32 / 8, D 128, NORM pairs) and Qwen3-8B heads (32 / 8, D 128, NEOX pairs, q/k norm), fp16 and Q8_0
caches, B = 1 with N in {1, 4, 512, 8192} new tokens into an empty cache of that capacity.  Every step uses
another copy of the packed qkv rows, the q output and the caches; the copies hold >= 1 GiB together, but
never more than 256 of them, so the cells at N <= 4 (KiB per step) measure launches on cached data.  A cell
is the median time of both forms, their spread, and for N >= 512 the bytes a step must move (qkv read, q and
cache rows written) per second against bench.py's HBM figure.

    python tools/attn_bench.py --gemma [--out profiles/attn_gemma_bench.json]

Head dim 256 and the sliding window (gq_attn_decode_ex, gq_attn_prefill at D = 256): Gemma-2-9B heads (16 / 8,
D 256) at decode over 32768 cached tokens and at a prefill of 8192; then, at Llama-3-8B heads (D 128) and
Gemma-2-9B heads (D 256), decode with window 1024 over 2048, 8192 and 32768 cached tokens beside the
yardstick, the plain call over a cache of 1024 tokens.  torch SDPA is the base everywhere (the window as a
boolean mask).  A windowed cell's bytes are the window's rows; its copies rotate like any other cell's.

    python tools/attn_bench.py --mla [--out profiles/attn_mla_bench.json]

DeepSeek's absorbed latent attention (kernels._lib.mla_decode: gq_mla_decode) over an fp16 latent cache of
[c_kv (512) | k_pe (64)] rows, 128 heads (V3, R1) and 16 (V2-Lite), B in {1, 4}, N in {1, 4}, kv_len in {512,
4096, 32768}, beside torch over the same cache sliced to the length: softmax(q C^T) C[:, :512] in fp16 (two
matmuls and a masked softmax; MlaCase).  A cell is the median time of both forms, their spread, and the live
cache bytes (read ONCE: 1152 per position) per second against the HBM figure; every 128-head cell also
carries its time over the 16-head cell's: what the repeated stream of its row groups costs.

    python tools/attn_bench.py --mla-prefill [--out profiles/attn_mla_prefill_bench.json]

The same attention over a prompt or a chunk of one (kernels._lib.mla_prefill: gq_mla_prefill), 16 and 128 heads,
N in {16, 512, 4096} without a prefix and N = 512 after a prefix of 4096, B in {1, 4}, beside two bases: torch
fp16 softmax(mask(q C^T)) C[:, :512] over the same cache, and what the library offered before -- a loop of
mla_decode at four tokens a step, each step at its own length -- all three as captured graphs (MlaPrefillCase).
A cell is the median time of each form and the causal TFLOP/s at 2 * (576 + 512) flops per attended (row, key).

    python tools/attn_bench.py --mla-proj [--out profiles/attn_mla_proj_bench.json]

The per-head W_UK / W_UV products around that attention (kernels._lib.mla_proj: gq_mla_proj), 16 and 128 heads, T in
{1, 4, 64, 4096} token rows of one sequence: each direction beside the lines MLAttention.forward runs without
fused=True (a strided-batch torch.bmm, and for the absorb the copy into the q buffer), and the fused forward beside
the unfused one over a cache of 4096 positions (MlaProjCase).  The weights rotate.  A few-row cell carries the weight
bytes over the time against the HBM figure, a tiled cell the TFLOP/s of 2 * T * heads * 512 * 128 flops.

    python tools/attn_bench.py --mla-mha [--out profiles/attn_mla_mha_bench.json]

The un-absorbed prompt pass (kernels._lib.mla_kv_expand, mla_prefill_mha), 16 and 128 heads, one sequence: a fresh
prompt of 512 and of 4096 and a chunk of 512 after a prefix of 4096 (MlaMhaCase).  Per cell the expansion of the new
rows alone, the attention alone (causal TFLOP/s at 2 * (192 + 128) flops per attended (row, key)) and the layer step
MLAttention(unabsorbed_from=1) beside the absorbed fused step MLAttention(fused=True), all as captured graphs.
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
GEMMA_HEADS = {"llama3_8b": (32, 8, 128), "gemma2_9b": (16, 8, 256)}
FORMS = ("torch", "f16", "q8_0")


class Case:
    def __init__(self, nh, kvh, D, N, B, L, dev, steps, window=0):
        import kernels._lib as kl
        self.kl, self.dev, self.dims, self.window = kl, dev, (nh, kvh, D, N, B, L), window
        rows = min(L, window + N - 1) if window else L  # the positions some query attends
        self.live = {k: 2 * B * rows * kvh * kl.kv_row_bytes(k, D) for k in ("f16", "q8_0")}
        ncopies, self.plans = bench.rotation_plan(self.live["q8_0"], steps)
        gen = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(torch.float16)  # noqa: E731
        self.f16 = [(rnd(B, L, kvh, D), rnd(B, L, kvh, D)) for _ in range(ncopies)]
        self.q8 = [tuple(bench.device_random_blocks("q8_0", B * L * kvh, D, dev, 10 * c + s) for s in (0, 1))
                   for c in range(ncopies)]
        self.q = rnd(B * N, nh * D)
        self.kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
        self.ws = torch.empty(kl.attn_workspace_size(B, N, nh, kvh, D, window), dtype=torch.uint8, device=dev)
        self.out = torch.empty(B * N, nh * D, dtype=torch.float16, device=dev)
        # the N new tokens sit at the cache's end: query i sees positions 0 .. L - N + i
        self.mask = None if N == 1 and not window else torch.ones(N, L, dtype=torch.bool, device=dev).tril(L - N)
        if window:  # ... and L - N + i - window + 1 at the least
            self.mask &= ~torch.ones(N, L, dtype=torch.bool, device=dev).tril(L - N - window)

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
                                   self.ws, out=self.out, window=self.window)

    def check(self):
        a, b = self.step("torch", 0, 0).float(), self.step("f16", 0, 0).float()
        torch.cuda.synchronize(self.dev)
        d = float((a - b).abs().max() / a.abs().max())
        assert d <= 1e-2, d
        assert torch.isfinite(self.step("q8_0", 0, 0)).all()
        return d


class PrefillCase:
    """N new tokens after a prefix of P per sequence: kernels._lib.attn_prefill over an fp16 and a Q8_0
    cache exactly P + N long, beside torch SDPA on the same fp16 cache (is_causal=True without a prefix,
    an explicit (N, P + N) boolean mask with one; grouped heads by enable_gqa=True, i.e. K and V are
    not repeated by the caller).  The caches rotate as in Case; q does not."""

    def __init__(self, nh, kvh, D, N, B, P, dev, steps):
        import kernels._lib as kl
        L = P + N
        self.kl, self.dev, self.dims = kl, dev, (nh, kvh, D, N, B, L)
        ncopies, self.plans = bench.rotation_plan(2 * B * L * kvh * kl.kv_row_bytes("q8_0", D), steps)
        gen = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(torch.float16)  # noqa: E731
        # (every copy holds the same values: a copy per step is about where the bytes come from)
        self.f16 = [tuple(t.expand(ncopies, B, L, kvh, D).contiguous().unbind(0)) for t in (rnd(B, L, kvh, D), rnd(B, L, kvh, D))]
        self.q8 = [tuple(bench.device_random_blocks("q8_0", B * L * kvh, D, dev, s).expand(ncopies, -1).contiguous().unbind(0))
                   for s in (0, 1)]
        self.q = rnd(B * N, nh * D)
        self.kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
        self.out = torch.empty(B * N, nh * D, dtype=torch.float16, device=dev)
        self.mask = None if P == 0 else torch.ones(N, L, dtype=torch.bool, device=dev).tril(P)
        self.flops = 4.0 * D * B * nh * (N * P + N * (N + 1) // 2)  # 4 D per attended (row, key) pair

    def step(self, form, c, i):
        nh, kvh, D, N, B, L = self.dims
        if form == "torch":
            k, v = (t[c].permute(0, 2, 1, 3) for t in self.f16)
            q = self.q.view(B, N, nh, D).permute(0, 2, 1, 3)
            o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=self.mask, is_causal=self.mask is None,
                                                                 enable_gqa=nh != kvh)
            return o.permute(0, 2, 1, 3).reshape(B * N, nh * D)
        kind = "q8_0" if form == "q8_0" else "f16"
        k, v = (t[c] for t in (self.q8 if form == "q8_0" else self.f16))
        rb = self.kl.kv_row_bytes(kind, D)
        self.kl.set_tuning("GQ_ATTN_TRV", int(form != "f16_gather"))  # (read at the launch, so at the capture)
        o = self.kl.attn_prefill(kind, self.q, k, v, (kvh * rb, rb, L * kvh * rb), self.kv_len, L, B, N, nh, kvh, D,
                                 out=self.out)
        self.kl.reset_tuning()
        return o

    check = Case.check


class MlaCase:
    def __init__(self, nh, N, B, L, dev, steps):
        import kernels._lib as kl
        self.kl, self.dev, self.dims = kl, dev, (nh, N, B, L)
        self.live = {"f16": B * L * 1152}
        ncopies, self.plans = bench.rotation_plan(self.live["f16"], steps)
        gen = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(torch.float16)  # noqa: E731
        self.c = [rnd(B, L, 576) for _ in range(ncopies)]
        self.q = rnd(B * N, nh * 576)
        self.kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
        self.ws = torch.empty(kl.mla_workspace_size(B, N, nh), dtype=torch.uint8, device=dev)
        self.out = torch.empty(B * N, nh * 512, dtype=torch.float16, device=dev)
        self.mask = None if N == 1 else ~torch.ones(N, L, dtype=torch.bool, device=dev).tril(L - N)
        self.scale = 192 ** -0.5

    def step(self, form, c, i):
        nh, N, B, L = self.dims
        if form == "torch":
            C = self.c[c]                                                       # (B, L, 576)
            s = torch.matmul(self.q.view(B, N * nh, 576), C.transpose(1, 2)) * self.scale
            if self.mask is not None:
                s = s.view(B, N, nh, L).masked_fill(self.mask[None, :, None, :], float("-inf")).view(B, N * nh, L)
            return torch.matmul(torch.softmax(s, dim=-1), C[:, :, :512]).reshape(B * N, nh * 512)
        return self.kl.mla_decode(self.q, self.c[c], (1152, L * 1152), self.kv_len, L, B, N, nh, self.ws, self.scale, out=self.out)

    def check(self):
        a, b = self.step("torch", 0, 0).float(), self.step("f16", 0, 0).float()
        torch.cuda.synchronize(self.dev)
        d = float((a - b).abs().max() / a.abs().max())
        assert d <= 1e-2, d
        return d


def main_mla(a, dev):
    rows, forms, base = [], ("torch", "f16"), {}
    for nh in (16, 128):
        for L in (512, 4096, 32768):
            for B in (1, 4):
                for N in (1, 4):
                    if L > a.max_len:
                        continue
                    case = MlaCase(nh, N, B, L, dev, a.steps)
                    diff = case.check()
                    gs = {f: graphs(case, f) for f in forms}
                    ts = {f: [] for f in forms}
                    for _ in range(a.repeats):  # interleaved: one pass over the forms per repeat
                        for f in forms:
                            ts[f].append(bench.timed_rotation(gs[f], dev) / a.steps * 1e6)
                    tile, grows, W = case.kl.mla_plan(B, N, nh)
                    row = {"heads": nh, "N": N, "B": B, "kv_len": L, "W": W, "row_groups": -(-N * nh // grows),
                           "f16_vs_torch_max_rel_diff": round(diff, 5)}
                    for f in forms:
                        us = float(np.median(ts[f]))
                        gbs = case.live["f16"] / us / 1e3
                        row[f] = {"us": round(us, 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2), "cache_GBs": round(gbs, 1),
                                  "hbm_frac": round(gbs / bench.HBM_PEAK_GBS, 4)}
                    if nh == 16:
                        base[(N, B, L)] = row["f16"]["us"]
                    else:
                        row["f16_us_over_16_heads"] = round(row["f16"]["us"] / base[(N, B, L)], 2)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del case, gs
                    torch.cuda.empty_cache()
                    if a.out:  # (after every cell: a run cut short keeps what it measured)
                        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                        with open(a.out, "w") as f:
                            json.dump({"steps": a.steps, "repeats": a.repeats, "hbm_peak_GBs": bench.HBM_PEAK_GBS,
                                       "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count,
                                       "not_measured": "two ring slots against three, blockIdx in plain order against the "
                                                       "die-aware one, any profile (no counters were collected)",
                                       "rows": rows}, f, indent=1)


class MlaPrefillCase:
    """N new tokens after a prefix of P per sequence over a latent cache exactly P + N long.  The caches rotate as
    in PrefillCase (every copy the same values), over at most 256 copies: a cache below 4 MiB is not the cost."""
    forms = ("torch", "f16", "decode_x4")

    def __init__(self, nh, N, B, P, dev, steps):
        import kernels._lib as kl
        L = P + N
        self.kl, self.dev, self.dims, self.scale = kl, dev, (nh, N, B, L), 192 ** -0.5
        ncopies, self.plans = bench.rotation_plan(max(B * L * 1152, bench.ROTATE_BYTES // 256), steps)
        gen = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(torch.float16)  # noqa: E731
        self.c = rnd(B, L, 576).expand(ncopies, B, L, 576).contiguous().unbind(0)
        self.q = rnd(B * N, nh * 576)
        self.kv_len = torch.full((B,), L, dtype=torch.int32, device=dev)
        self.out = torch.empty(B * N, nh * 512, dtype=torch.float16, device=dev)
        self.mask = ~torch.ones(N, L, dtype=torch.bool, device=dev).tril(P)
        self.flops = 2.0 * (576 + 512) * B * nh * (N * P + N * (N + 1) // 2)
        # the loop of decode steps: step j's tokens 4j .. as rows of their own, at the length that ends with them
        self.steps4 = [(self.q.view(B, N, -1)[:, j:j + 4].reshape(-1, nh * 576).contiguous(),
                        torch.full((B,), P + min(j + 4, N), dtype=torch.int32, device=dev)) for j in range(0, N, 4)]
        self.ws = torch.empty(kl.mla_workspace_size(B, 4, nh), dtype=torch.uint8, device=dev)
        self.out4 = torch.empty(B * 4, nh * 512, dtype=torch.float16, device=dev)

    def step(self, form, c, i):
        nh, N, B, L = self.dims
        C = self.c[c]
        if form == "torch":
            s = torch.matmul(self.q.view(B, N * nh, 576), C.transpose(1, 2)) * self.scale
            s = s.view(B, N, nh, L).masked_fill_(self.mask[None, :, None, :], float("-inf")).view(B, N * nh, L)
            return torch.matmul(torch.softmax(s, dim=-1), C[:, :, :512]).view(B, N, nh * 512).reshape(B * N, nh * 512)
        if form == "f16":
            return self.kl.mla_prefill(self.q, C, (1152, L * 1152), self.kv_len, L, B, N, nh, self.scale, out=self.out)
        for q4, len4 in self.steps4:
            n = q4.shape[0] // B
            self.kl.mla_decode(q4, C, (1152, L * 1152), len4, L, B, n, nh, self.ws, self.scale, out=self.out4[:B * n])
        return self.out4

    check = MlaCase.check


# (N, prefix)
MLA_PREFILL_CELLS = [(16, 0), (512, 0), (4096, 0), (512, 4096)]


def main_mla_prefill(a, dev):
    rows, skipped = [], []
    for nh in (16, 128):
        for N, P in MLA_PREFILL_CELLS:
            for B in (1, 4):
                if P + N > a.max_len:
                    continue
                # torch's scores, their masked copy and the probabilities, fp16, beside q and its decode-step copy
                need = 3 * 2 * B * N * nh * (P + N) + 2 * 2 * B * N * nh * 576
                if need > 0.5 * torch.cuda.get_device_properties(dev).total_memory:
                    skipped.append({"heads": nh, "N": N, "prefix": P, "B": B, "why": f"{need >> 30} GiB of torch scores and q"})
                    continue
                steps = a.steps if N <= 512 else max(2, a.steps // 5)  # (a 4096-token step is 1024 decode steps)
                case = MlaPrefillCase(nh, N, B, P, dev, steps)
                diff = case.check()
                # (one pool a form: torch's 4 GiB of scores at 128 heads x 4096 tokens, not once per graph)
                gs = {f: graphs(case, f, torch.cuda.graph_pool_handle()) for f in case.forms}
                ts = {f: [] for f in case.forms}
                for _ in range(a.repeats):  # interleaved: one pass over the forms per repeat
                    for f in case.forms:
                        ts[f].append(bench.timed_rotation(gs[f], dev) / steps * 1e6)
                _, rows_wg, grid = case.kl.mla_prefill_plan(B, N, nh)
                row = {"heads": nh, "B": B, "N": N, "prefix": P, "rows_per_workgroup": rows_wg, "workgroups": grid,
                       "f16_vs_torch_max_rel_diff": round(diff, 5), "causal_gflop": round(case.flops / 1e9, 2)}
                for f in case.forms:
                    us = float(np.median(ts[f]))
                    tf = case.flops / us / 1e6
                    row[f] = {"us": round(us, 1), "spread_us": round(max(ts[f]) - min(ts[f]), 1), "causal_TFLOPs": round(tf, 1),
                              "mfma_frac": round(tf / bench.MFMA_F16_PEAK_TF, 4)}
                for base in ("torch", "decode_x4"):
                    row[f"f16_slower_than_{base}"] = bool(row["f16"]["us"] - row[base]["us"] >
                                                          max(row["f16"]["spread_us"], row[base]["spread_us"]))
                rows.append(row)
                print(json.dumps(row), flush=True)
                del case, gs
                torch.cuda.empty_cache()
                if a.out:  # (after every cell: a run cut short keeps what it measured)
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        json.dump({"steps": a.steps, "repeats": a.repeats, "mfma_f16_peak_TF": bench.MFMA_F16_PEAK_TF,
                                   "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count,
                                   "not_measured": "the die-aware workgroup order, two ring slots against three, a 32-row "
                                                   "form (it spills), any profile (no counters were collected)",
                                   "skipped": skipped, "rows": rows}, f, indent=1)


class MlaProjCase:
    """T token rows of one sequence through a layer's two latent projections and through MLAttention.forward over a
    latent cache of 4096 positions (the T new tokens its last).  The weights rotate (every copy the same values,
    at most 256 copies); q, the q buffer, the attention output and the cache do not."""
    forms = ("absorb_torch", "absorb_hip", "expand_torch", "expand_hip", "layer_torch", "layer_fused")
    L = 4096

    def __init__(self, nh, T, dev, steps):
        import kernels._lib as kl
        from kernels import MLAttention, RoPE
        self.kl, self.dev, self.dims = kl, dev, (nh, T)
        self.wbytes = 2 * nh * 512 * 128  # one direction's weights
        ncopies, self.plans = bench.rotation_plan(max(2 * self.wbytes, bench.ROTATE_BYTES // 256), steps)
        gen = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(torch.float16)  # noqa: E731
        self.kb = (rnd(nh, 512, 128) * 128 ** -0.5).expand(ncopies, nh, 512, 128).contiguous().unbind(0)
        self.vb = (rnd(nh, 128, 512) * 512 ** -0.5).expand(ncopies, nh, 128, 512).contiguous().unbind(0)
        self.q, self.kv, self.o = rnd(T, nh * 192), rnd(T, 576), rnd(T, nh * 512)
        self.qbuf = torch.zeros(T, nh * 576, dtype=torch.float16, device=dev)
        self.out = torch.empty(T, nh * 128, dtype=torch.float16, device=dev)
        f, m = RoPE.table(64)
        rope, w = RoPE(torch.from_numpy(f).float().to(dev), 64, "norm", m), torch.ones(512, device=dev)
        self.layers = {fused: [MLAttention(k, v, w, rope, fused=fused) for k, v in zip(self.kb, self.vb)] for fused in (False, True)}
        self.cache = self.layers[False][0].new_cache(1, self.L, dev)
        self.cache.c.view(torch.float16).copy_(rnd(self.L * 576))
        self.len0 = torch.full((1,), self.L - T, dtype=torch.int32, device=dev)
        self.flops = 2.0 * T * nh * 512 * 128  # one direction

    def step(self, form, c, i):
        nh, T = self.dims
        if form == "absorb_torch":  # MLAttention.forward's lines: a strided-batch bmm and the copy into the q buffer
            q_abs = torch.bmm(self.q.view(T, nh, -1)[:, :, :128].transpose(0, 1), self.kb[c].transpose(1, 2))
            return self.qbuf.view(T, nh, -1)[:, :, :512].copy_(q_abs.transpose(0, 1))
        if form == "absorb_hip":
            return self.kl.mla_proj(0, self.kb[c], self.q, 192, self.qbuf, 576, T, nh).view(T, nh, -1)[:, :, :512]
        if form == "expand_torch":
            return torch.bmm(self.o.view(T, nh, 512).transpose(0, 1), self.vb[c].transpose(1, 2)).transpose(0, 1).reshape(T, nh * 128)
        if form == "expand_hip":
            return self.kl.mla_proj(1, self.vb[c], self.o, 512, self.out, 128, T, nh)
        self.cache.kv_len.copy_(self.len0)  # (both layer forms: every step appends the same T tokens at the cache's end)
        return self.layers[form == "layer_fused"][c].forward(self.q, self.kv, self.cache)

    def check(self):
        d = {}
        for what in ("absorb", "expand", "layer"):
            a = self.step(f"{what}_torch", 0, 0).float().clone()
            b = self.step(f"{what}_{'fused' if what == 'layer' else 'hip'}", 0, 0).float()
            torch.cuda.synchronize(self.dev)
            d[what] = float((a - b).abs().max() / a.abs().max())
            assert d[what] <= 1e-2, d
        return d


def main_mla_proj(a, dev):
    rows = []
    for nh in (16, 128):
        for T in (1, 4, 64, 4096):
            steps = a.steps if T <= 4 else max(2, a.steps // 5)
            case = MlaProjCase(nh, T, dev, steps)
            diff = case.check()
            gs = {f: graphs(case, f, torch.cuda.graph_pool_handle()) for f in case.forms}
            ts = {f: [] for f in case.forms}
            for _ in range(a.repeats):  # interleaved: one pass over the forms per repeat
                for f in case.forms:
                    ts[f].append(bench.timed_rotation(gs[f], dev) / steps * 1e6)
            form, rows_wg, _ = case.kl.mla_proj_plan(0, T, nh)
            row = {"heads": nh, "T": T, "form": "tiled" if form else "few-row", "rows_per_workgroup": rows_wg,
                   "workgroups": {d: case.kl.mla_proj_plan(i, T, nh)[2] for i, d in enumerate(("absorb", "expand"))},
                   "hip_vs_torch_max_rel_diff": {k: round(v, 5) for k, v in diff.items()}}
            for f in case.forms:
                us = float(np.median(ts[f]))
                row[f] = {"us": round(us, 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2)}
                if not f.startswith("layer"):
                    if form == 0:  # the weights, read once, over the time against the HBM figure
                        row[f]["weight_GBs"] = round(case.wbytes / us / 1e3, 1)
                        row[f]["hbm_frac"] = round(case.wbytes / us / 1e3 / bench.HBM_PEAK_GBS, 4)
                    else:
                        row[f]["TFLOPs"] = round(case.flops / us / 1e6, 1)
                        row[f]["mfma_frac"] = round(case.flops / us / 1e6 / bench.MFMA_F16_PEAK_TF, 4)
            for new, old in (("absorb_hip", "absorb_torch"), ("expand_hip", "expand_torch"), ("layer_fused", "layer_torch")):
                row[f"{new}_slower"] = bool(row[new]["us"] - row[old]["us"] > max(row[new]["spread_us"], row[old]["spread_us"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del case, gs
            torch.cuda.empty_cache()
            if a.out:  # (after every cell: a run cut short keeps what it measured)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump({"steps": a.steps, "repeats": a.repeats, "hbm_peak_GBs": bench.HBM_PEAK_GBS,
                               "mfma_f16_peak_TF": bench.MFMA_F16_PEAK_TF, "layer_kv_len": MlaProjCase.L,
                               "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count,
                               "not_measured": "the LDS-DMA ring for the few-row weight stream, other tiles-per-workgroup "
                                               "counts, two token tiles per wave in the tiled form, any profile (no "
                                               "counters were collected)",
                               "rows": rows}, f, indent=1)


class MlaMhaCase:
    """N new tokens of one sequence after a prefix of P through the un-absorbed prompt pass: the expansion of the N
    new rows alone, the attention alone, and the layer step (append + expand + attention: MLAttention(unabsorbed_from=1))
    beside the absorbed fused step (append + gq_mla_proj + gq_mla_prefill + gq_mla_proj: MLAttention(fused=True)).
    The weights rotate (every copy the same values); q, the caches and the outputs do not."""
    forms = ("expand", "mha", "layer_unabsorbed", "layer_absorbed")

    def __init__(self, nh, N, P, dev, steps):
        import kernels._lib as kl
        from kernels import MLAttention, RoPE
        self.kl, self.dev, self.dims, L = kl, dev, (nh, N, P), P + N
        ncopies, self.plans = bench.rotation_plan(max(2 * nh * 256 * 512, bench.ROTATE_BYTES // 256), steps)
        gen = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen).to(torch.float16)  # noqa: E731
        kb = (rnd(nh, 512, 128) * 128 ** -0.5).expand(ncopies, nh, 512, 128).contiguous().unbind(0)
        vb = (rnd(nh, 128, 512) * 512 ** -0.5).expand(ncopies, nh, 128, 512).contiguous().unbind(0)
        self.q, self.kv = rnd(N, nh * 192), rnd(N, 576)
        f, m = RoPE.table(64)
        rope, w = RoPE(torch.from_numpy(f).float().to(dev), 64, "norm", m), torch.ones(512, device=dev)
        self.layers = {u: [MLAttention(k, v, w, rope, fused=True, unabsorbed_from=u) for k, v in zip(kb, vb)] for u in (0, 1)}
        self.cache = c = self.layers[1][0].new_cache(1, L, dev)
        c.c.view(torch.float16).copy_(rnd(L * 576))
        self.len0, self.len1 = (torch.full((1,), n, dtype=torch.int32, device=dev) for n in (P, L))
        c.kv_len.copy_(self.len1)  # the prefix (and the rest) expanded once: every copy of the weights has the same values
        c.expand(self.layers[1][0].w_kv, L)
        self.qbuf, self.out = c._for(N, nh)[0], torch.empty(N, nh * 128, dtype=torch.float16, device=dev)
        self.pairs = N * P + N * (N + 1) // 2  # attended (row, key) pairs per head

    def step(self, form, c, i):
        nh, N, P = self.dims
        ch = self.cache
        if form == "expand":
            return self.kl.mla_kv_expand(self.layers[1][c].w_kv, ch.c, ch.strides, self.len1, ch.capacity, ch.kv, 1, N, nh)
        if form == "mha":
            return self.kl.mla_prefill_mha(self.q, 192, self.qbuf[:, 512:], 576, ch.kv, ch.c, ch.strides, self.len1, ch.capacity, 1, N, nh,
                                           self.layers[1][c].scale, self.out)
        ch.kv_len.copy_(self.len0)  # (both layer forms: every step appends the same N tokens after the prefix)
        ch.appended = ch.expanded = P
        return self.layers[form == "layer_unabsorbed"][c].forward(self.q, self.kv, ch)

    def check(self):
        a = self.step("layer_absorbed", 0, 0).float().clone()
        b = self.step("layer_unabsorbed", 0, 0).float()
        torch.cuda.synchronize(self.dev)
        d = float((a - b).abs().max() / a.abs().max())
        assert d <= 2e-2, d
        return d


def main_mla_mha(a, dev):
    rows = []
    for nh in (16, 128):
        for N, P in ((512, 0), (4096, 0), (512, 4096)):
            steps = max(2, a.steps // 5)
            case = MlaMhaCase(nh, N, P, dev, steps)
            diff = case.check()
            gs = {f: graphs(case, f, torch.cuda.graph_pool_handle()) for f in case.forms}
            ts = {f: [] for f in case.forms}
            for _ in range(a.repeats):  # interleaved: one pass over the forms per repeat
                for f in case.forms:
                    ts[f].append(bench.timed_rotation(gs[f], dev) / steps * 1e6)
            rows_wg, tile, grid = case.kl.mla_prefill_mha_plan(1, N, nh)
            row = {"heads": nh, "N": N, "prefix": P, "rows_per_workgroup": rows_wg, "tile": tile, "workgroups": grid,
                   "layers_max_rel_diff": round(diff, 5)}
            for f in case.forms:
                us = float(np.median(ts[f]))
                row[f] = {"us": round(us, 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2)}
            tf = 640.0 * case.pairs * nh / row["mha"]["us"] / 1e6  # causal: the attended pairs at 2 (192 + 128) flops
            row["mha"].update(TFLOPs=round(tf, 1), mfma_frac=round(tf / bench.MFMA_F16_PEAK_TF, 4))
            tf = 2.0 * N * nh * 256 * 512 / row["expand"]["us"] / 1e6
            row["expand"].update(TFLOPs=round(tf, 1), mfma_frac=round(tf / bench.MFMA_F16_PEAK_TF, 4))
            row["unabsorbed_speedup"] = round(row["layer_absorbed"]["us"] / row["layer_unabsorbed"]["us"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del case, gs
            torch.cuda.empty_cache()
            if a.out:  # (after every cell: a run cut short keeps what it measured)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump({"steps": steps, "repeats": a.repeats, "mfma_f16_peak_TF": bench.MFMA_F16_PEAK_TF,
                               "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count,
                               "not_measured": "another workgroup id order, a third ring slot, other tile lengths, any profile "
                                               "(no counters were collected)",
                               "rows": rows}, f, indent=1)


ROPE_HEADS = {"llama3_8b": (32, 8, 128, "norm", False), "qwen3_8b": (32, 8, 128, "neox", True)}


class RopeCase:
    def __init__(self, nh, kvh, D, mode, norm, kind, T, dev, steps):
        import kernels._lib as kl
        from kernels import RoPE
        self.kl, self.dev, self.dims, self.kind = kl, dev, (nh, kvh, D, T), kind
        rb, J = kl.kv_row_bytes(kind, D), nh + 2 * kvh
        self.bytes = 2 * T * J * D + 2 * T * nh * D + 2 * T * kvh * rb
        ncopies, self.plans = bench.rotation_plan(max(self.bytes, bench.ROTATE_BYTES // 256), steps)
        gen = torch.Generator(device=dev).manual_seed(1)
        self.qkv = torch.randn(ncopies, T, J * D, device=dev, generator=gen).to(torch.float16)
        self.qo = torch.empty(ncopies, T, nh * D, dtype=torch.float16, device=dev)
        # (kv_append wants k and v rows one stride apart: the base gets its v rows contiguous, made here, not in the step)
        self.v = self.qkv[:, :, (nh + kvh) * D:].contiguous()
        self.caches = torch.zeros(ncopies, 2, T * kvh * rb, dtype=torch.uint8, device=dev)
        self.strides = (kvh * rb, rb, T * kvh * rb)
        self.kv_len = torch.full((1,), T, dtype=torch.int32, device=dev)
        f, m = RoPE.table(D, 500000.0 if mode == "norm" else 1e6)
        w = [1 + 0.1 * torch.randn(D, device=dev, generator=gen) for _ in range(2)] if norm else [None, None]
        self.rope = RoPE(torch.from_numpy(f).float().to(dev), D, mode, m, w[0], w[1], 1e-6)

    def _torch_rope(self, x, heads, w, cos, sin):
        nh, kvh, D, T = self.dims
        y = x.float().view(T, heads, D)
        if w is not None:
            y = y * torch.rsqrt(y.pow(2).mean(-1, keepdim=True) + self.rope.eps) * w
        if self.rope.mode == "norm":
            y0, y1 = y[..., 0::2], y[..., 1::2]
            o = torch.stack((y0 * cos - y1 * sin, y0 * sin + y1 * cos), dim=-1)
        else:
            y0, y1 = y[..., :D // 2], y[..., D // 2:]
            o = torch.cat((y0 * cos - y1 * sin, y0 * sin + y1 * cos), dim=-1)
        return o.reshape(T, heads * D).to(torch.float16)

    def step(self, form, c, i):
        nh, kvh, D, T = self.dims
        q, k, v = self.qkv[c, :, :nh * D], self.qkv[c, :, nh * D:(nh + kvh) * D], self.qkv[c, :, (nh + kvh) * D:]
        Kc, Vc = self.caches[c, 0], self.caches[c, 1]
        r = self.rope
        if form == "fused":
            return self.kl.rope_append(self.kind, r.mode, q, k, v, Kc, Vc, self.strides, self.kv_len, T, r.inv_freq, D, 1, T, nh, kvh,
                                       D, r.mscale, r.q_norm, r.k_norm, r.eps, out=self.qo[c])
        pos = torch.arange(T, device=self.dev, dtype=torch.int32) + (self.kv_len - T)  # the caller's position tensor
        ang = torch.outer(pos.float(), r.inv_freq)[:, None, :]
        cos, sin = ang.cos() * r.mscale, ang.sin() * r.mscale
        self.qo[c].copy_(self._torch_rope(q, nh, r.q_norm, cos, sin))
        self.kl.kv_append(self.kind, self._torch_rope(k, kvh, r.k_norm, cos, sin), self.v[c], Kc, Vc, self.strides, self.kv_len, T, 1, T, kvh, D)
        return self.qo[c]

    def check(self):
        a = self.step("torch", 0, 0).float().clone()
        b = self.step("fused", 0, 0).float()
        torch.cuda.synchronize(self.dev)
        d = float((a - b).abs().max() / a.abs().max())
        assert d <= 2e-3, d  # (the base forms its angles in fp32)
        return d


def main_rope(a, dev):
    rows, forms = [], ("torch", "fused")
    for name, (nh, kvh, D, mode, norm) in ROPE_HEADS.items():
        for kind in ("f16", "q8_0"):
            for T in (1, 4, 512, 8192):
                case = RopeCase(nh, kvh, D, mode, norm, kind, T, dev, a.steps)
                diff = case.check()
                gs = {f: graphs(case, f) for f in forms}
                ts = {f: [] for f in forms}
                for _ in range(a.repeats):  # interleaved: one pass over the forms per repeat
                    for f in forms:
                        ts[f].append(bench.timed_rotation(gs[f], dev) / a.steps * 1e6)
                row = {"heads": name, "mode": mode, "qk_norm": norm, "kv": kind, "tokens": T, "step_bytes": case.bytes,
                       "copies": int(case.qkv.shape[0]), "fused_vs_torch_max_rel_diff": round(diff, 6)}
                for f in forms:
                    us = float(np.median(ts[f]))
                    row[f] = {"us": round(us, 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2)}
                    if T >= 512:
                        row[f]["GBs"] = round(case.bytes / us / 1e3, 1)
                        row[f]["hbm_frac"] = round(case.bytes / us / 1e3 / bench.HBM_PEAK_GBS, 4)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del case, gs
                torch.cuda.empty_cache()
                if a.out:  # (after every cell: a run cut short keeps what it measured)
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        json.dump({"steps": a.steps, "repeats": a.repeats, "hbm_peak_GBs": bench.HBM_PEAK_GBS,
                                   "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "rows": rows}, f, indent=1)


# "f16_gather": the fp16 form with V^T gathered element by element (GQ_ATTN_TRV=0), the alternative
# the transposing LDS read was measured against
PREFILL_FORMS = ("torch", "f16", "f16_gather", "q8_0")


def measure_prefill(case, steps, repeats, dev):
    diff = case.check()
    gs = {f: graphs(case, f) for f in PREFILL_FORMS}
    ts = {f: [] for f in PREFILL_FORMS}
    for _ in range(repeats):  # interleaved: one pass over the forms per repeat
        for f in PREFILL_FORMS:
            ts[f].append(bench.timed_rotation(gs[f], dev) / steps * 1e6)
    row = {"f16_vs_torch_max_rel_diff": round(diff, 5), "causal_gflop": round(case.flops / 1e9, 2)}
    for f in PREFILL_FORMS:
        us = float(np.median(ts[f]))
        tf = case.flops / us / 1e6
        row[f] = {"us": round(us, 1), "spread_us": round(max(ts[f]) - min(ts[f]), 1), "causal_TFLOPs": round(tf, 1),
                  "mfma_frac": round(tf / bench.MFMA_F16_PEAK_TF, 4)}
    return row


# (heads, B, N, prefix)
PREFILL_CELLS = [(h, 1, N, 0) for h in HEADS for N in (128, 512, 2048, 8192)] + [(h, 1, 512, 4096) for h in HEADS] + \
    [("llama3_8b", 4, 2048, 0)]


def main_prefill(a, dev):
    rows = []
    for name, B, N, P in PREFILL_CELLS:
        if P + N > a.max_len:
            continue
        nh, kvh, D = HEADS[name]
        case = PrefillCase(nh, kvh, D, N, B, P, dev, a.steps)
        rows_wg, tile = case.kl.attn_prefill_plan(B, N, nh, kvh, D)
        grid = B * kvh * -(-N * (nh // kvh) // rows_wg)
        row = {"heads": name, "B": B, "N": N, "prefix": P, "rows_per_workgroup": rows_wg, "workgroups": grid,
               **measure_prefill(case, a.steps, a.repeats, dev)}
        row["f16_slower_than_torch"] = bool(row["f16"]["us"] - row["torch"]["us"] >
                                            max(row["f16"]["spread_us"], row["torch"]["spread_us"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del case
        torch.cuda.empty_cache()
        if a.out:  # (after every cell: a run cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump({"steps": a.steps, "repeats": a.repeats, "mfma_f16_peak_TF": bench.MFMA_F16_PEAK_TF,
                           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "rows": rows}, f, indent=1)


def main_gemma(a, dev):
    out = {"steps": a.steps, "repeats": a.repeats, "hbm_peak_GBs": bench.HBM_PEAK_GBS, "decode": [], "prefill": [], "window": []}

    def decode(name, L, window=0):
        nh, kvh, D = GEMMA_HEADS[name]
        case = Case(nh, kvh, D, 1, 1, L, dev, a.steps, window)
        row = {"heads": name, "D": D, "N": 1, "B": 1, "kv_len": L, "window": window,
               "W": case.kl.attn_plan(1, 1, nh, kvh, D, window)[1], **measure(case, a.steps, a.repeats, dev)}
        print(json.dumps(row), flush=True)
        del case
        torch.cuda.empty_cache()
        return row

    def save():
        if a.out:  # (after every cell: a run cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    for name in GEMMA_HEADS:  # the yardstick (a cache of `window` tokens, the plain call), then the window over longer caches
        for L, window in ((1024, 0), (2048, 1024), (8192, 1024), (32768, 1024)):
            if L <= a.max_len:
                out["window"].append(decode(name, L, window))
                save()
    if 32768 <= a.max_len:
        out["decode"].append(decode("gemma2_9b", 32768))
        save()
    if 8192 <= a.max_len:
        nh, kvh, D = GEMMA_HEADS["gemma2_9b"]
        case = PrefillCase(nh, kvh, D, 8192, 1, 0, dev, a.steps)
        out["prefill"].append({"heads": "gemma2_9b", "D": D, "B": 1, "N": 8192, "prefix": 0,
                               "rows_per_workgroup": case.kl.attn_prefill_plan(1, 8192, nh, kvh, D)[0],
                               **measure_prefill(case, a.steps, a.repeats, dev)})
        print(json.dumps(out["prefill"][-1]), flush=True)
        save()


def graphs(case, form, pool=None):
    """pool: one memory pool for all the graphs of a form (they replay one after another), or a pool per graph."""
    grs = []
    for plan in case.plans:
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, pool=pool):
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
    ap.add_argument("--prefill", action="store_true", help="prefill attention (attn_prefill) instead of decode")
    ap.add_argument("--gemma", action="store_true", help="head dim 256 and windowed decode (Gemma-2-9B heads; window 1024)")
    ap.add_argument("--mla", action="store_true", help="DeepSeek's latent attention at decode (mla_decode) beside torch matmuls")
    ap.add_argument("--mla-prefill", action="store_true", help="the latent attention over a prompt (mla_prefill) beside torch and a decode loop")
    ap.add_argument("--rope", action="store_true", help="the fused norm + RoPE + append (rope_append) beside torch RoPE + kv_append")
    ap.add_argument("--mla-proj", action="store_true", help="the latent projections (mla_proj) and the fused MLAttention beside torch bmm")
    ap.add_argument("--mla-mha", action="store_true", help="the un-absorbed MLA prompt pass (mla_kv_expand, mla_prefill_mha) beside the absorbed fused step")
    a = ap.parse_args()
    if a.mla_mha and not a.out:
        a.out = "profiles/attn_mla_mha_bench.json"
    if not torch.cuda.is_available():
        sys.exit("attn_bench.py needs a ROCm device: there is no CPU timing path")
    dev = torch.device("cuda:0")
    if a.mla:
        return main_mla(a, dev)
    if a.mla_prefill:
        return main_mla_prefill(a, dev)
    if a.mla_proj:
        return main_mla_proj(a, dev)
    if a.mla_mha:
        return main_mla_mha(a, dev)
    if a.prefill:
        return main_prefill(a, dev)
    if a.rope:
        return main_rope(a, dev)
    if a.gemma:
        return main_gemma(a, dev)
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
