#!/usr/bin/env python3
"""The expert-indexed MMQ (gq_mmq_id) beside what the library offered for the same work before it:
gq_mmq_grouped over the same (expert, row) items with the ids already on the host.  Graph-replayed
step times (bench.py's method and helpers; bench.py itself does not know the call).

    python tools/moe_bench.py [--steps 20] [--repeats 3] [--out moe_bench.json]

Step = one call over the N x S (token, slot) pairs of one expert tensor.  A step reads only the
chosen experts, so both the tensor copies AND the choices rotate: the id sets of a case tile the
E experts, and the steps walk every (copy, id set) -- >= 1 GiB of distinct weight bytes between
two reads of one expert's copy.  Every replay is timed alone by device events
(bench.timed_rotation); the forms are measured interleaved, `repeats` passes in one process, and
each cell reports the median over the passes and their spread (max - min): a difference within the
sum of two spreads is not one.

Forms: "id" = gq_mmq_id (ids in device memory); "grouped" = gq_mmq_grouped, one 1-token item per
pair (at most 16 items per launch: 64 pairs would be four launches); "merged" (the cases whose
pairs share experts) = gq_mmq_grouped with the two pairs of an expert as one 2-token item -- the
weights streamed once per expert, which needs the ids on the host AND a choice pattern that leaves
the two rows a constant stride apart.  Needs the GPU: no fallback.
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gguf-triton-kernel_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402

BLOCK = {"q4_k": (256, 144), "q6_k": (256, 210)}


def tiles(E, N, S, share):
    """Id sets (N, S) that together visit every expert once (share = 1) or twice (share = 2: tokens
    2i and 2i+1 make the same choices, so an expert's two rows are adjacent tokens)."""
    per = (N // share) * S
    assert E % per == 0 and N % share == 0
    sets = []
    for j in range(E // per):
        a = (np.arange(per, dtype=np.int32) + j * per).reshape(N // share, S)
        sets.append(np.repeat(a, share, axis=0))
    return sets


# (name, type, E, M, K, N, S, per-slot rows, share)
CASES = [
    ("mixtral gate", "q4_k", 8, 14336, 4096, 1, 2, False, 1),
    ("mixtral gate", "q4_k", 8, 14336, 4096, 4, 2, False, 1),
    ("mixtral gate, experts shared by 2 tokens", "q4_k", 8, 14336, 4096, 4, 2, False, 2),
    ("mixtral down", "q6_k", 8, 4096, 14336, 1, 2, True, 1),
    ("mixtral down", "q6_k", 8, 4096, 14336, 4, 2, True, 1),
    ("mixtral down, experts shared by 2 tokens", "q6_k", 8, 4096, 14336, 4, 2, True, 2),
    ("qwen-moe gate", "q4_k", 128, 768, 2048, 1, 8, False, 1),
]


class Case:
    def __init__(self, fmt, E, M, K, N, S, per_slot, share, dev, steps):
        import kernels._lib as kl
        self.kl, self.L, self.dev = kl, kl.lib(), dev
        self.gtype, self.E, self.M, self.K, self.N, self.S = kl.TYPES[fmt], E, M, K, N, S
        self.ebytes = M * (K // 256) * BLOCK[fmt][1]
        ncopies = max(2, math.ceil(bench.ROTATE_BYTES / (E * self.ebytes)))
        base = bench.device_random_blocks(fmt, E * M, K, dev, 1)
        self.A = [base] + [base.clone() for _ in range(ncopies - 1)]
        self.sets = tiles(E, N, S, share)
        self.ids = [torch.from_numpy(s).to(dev) for s in self.sets]
        g = torch.Generator(device=dev).manual_seed(2)
        self.B = torch.randn((N, S, K) if per_slot else (N, K), device=dev, generator=g).to(torch.float16)
        self.ldb, self.ldb_slot = (S * K, K) if per_slot else (K, 0)
        self.C = torch.empty((N, S, M), dtype=torch.float16, device=dev)
        self.share = share
        self.step_bytes = len(np.unique(self.sets[0])) * self.ebytes
        combos = [(c, j) for c in range(ncopies) for j in range(len(self.sets))]
        G = max(1, math.ceil(len(combos) / steps))
        self.plans = [[combos[(g_ * steps + i) % len(combos)] for i in range(steps)] for g_ in range(G)]
        self.rotated = ncopies * E * self.ebytes
        self.items = {}  # (form, copy, set) -> [(ctypes item array, n, N_tok), ...], built once

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _row(self, n, s):
        return self.B.data_ptr() + 2 * (n * self.ldb + s * self.ldb_slot)

    def _grouped_items(self, form, c, j):
        key = (form, c, j)
        if key not in self.items:
            ids, kl = self.sets[j], self.kl
            out = []
            if form == "grouped":  # one 1-token item per pair
                its = [kl.GroupItem(self.gtype, self.A[c].data_ptr() + int(ids[n, s]) * self.ebytes, self._row(n, s),
                                    self.K, self.C[n, s].data_ptr(), self.M, self.M, self.K)
                       for n in range(self.N) for s in range(self.S)]
                ntok = 1
            else:  # merged: tokens 2i, 2i+1 chose the same experts -- one 2-token item per (pair of tokens, slot)
                its = [kl.GroupItem(self.gtype, self.A[c].data_ptr() + int(ids[n, s]) * self.ebytes, self._row(n, s),
                                    self.ldb, self.C[n, s].data_ptr(), self.S * self.M, self.M, self.K)
                       for n in range(0, self.N, 2) for s in range(self.S)]
                ntok = 2
            for o in range(0, len(its), 16):
                part = its[o:o + 16]
                out.append(((kl.GroupItem * len(part))(*part), len(part), ntok))
            self.items[key] = out
        return self.items[key]

    def step(self, form, c, j):
        if form == "id":
            rc = self.L.gq_mmq_id(self.gtype, self.A[c].data_ptr(), self.ids[j].data_ptr(), self.B.data_ptr(),
                                  self.C.data_ptr(), self.E, self.M, self.N, self.S, self.K, self.ldb, self.ldb_slot,
                                  self.M, self._stream())
            if rc:
                raise RuntimeError(self.L.gq_last_error().decode())
            return
        for arr, n, ntok in self._grouped_items(form, c, j):
            rc = self.L.gq_mmq_grouped(arr, n, ntok, self._stream())
            if rc:
                raise RuntimeError(self.L.gq_last_error().decode())

    def check(self, forms):
        """Every form gives the id form's bits (the same decode body; the merged 2-token items run
        the 2-token tile: compared within the decode tolerance instead)."""
        self.C.zero_()
        self.step("id", 0, 0)
        torch.cuda.synchronize(self.dev)
        want = self.C.clone()
        for f in forms:
            if f == "id":
                continue
            self.C.zero_()
            self.step(f, 0, 0)
            torch.cuda.synchronize(self.dev)
            if f == "grouped":
                assert torch.equal(self.C.view(torch.int16), want.view(torch.int16)), f
            else:
                d = (self.C.float() - want.float()).abs().max() / want.float().abs().max()
                assert float(d) <= 3e-3, (f, float(d))

    def graphs(self, form):
        grs = []
        for plan in self.plans:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for c, j in plan:
                    self.step(form, c, j)
            grs.append(gr)
        return grs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="substring of the case names to run")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda:0")
    rows = []
    for name, fmt, E, M, K, N, S, per_slot, share in CASES:
        if a.only and a.only not in name:
            continue
        case = Case(fmt, E, M, K, N, S, per_slot, share, dev, a.steps)
        forms = ["id", "grouped"] + (["merged"] if share == 2 else [])
        case.check(forms)
        graphs = {f: case.graphs(f) for f in forms}
        ts = {f: [] for f in forms}
        for _ in range(a.repeats):  # interleaved: one pass over the forms per repeat
            for f in forms:
                ts[f].append(bench.timed_rotation(graphs[f], dev) / a.steps * 1e6)
        row = {"case": name, "type": fmt, "E": E, "M": M, "K": K, "N_tok": N, "S": S, "pairs": N * S,
               "experts_read": int(len(np.unique(case.sets[0]))), "step_weight_bytes": case.step_bytes,
               "rotated_bytes": case.rotated}
        for f in forms:
            med = float(np.median(ts[f]))
            reads = 1 if f == "merged" else share  # times each chosen expert is streamed
            row[f] = {"us": round(med, 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2),
                      "weight_GBps": round(case.step_bytes * reads / med / 1e3, 1)}
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
