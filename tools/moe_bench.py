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

    python tools/moe_bench.py --prefill [--steps 20] [--repeats 3] [--out moe_prefill.json]

The prefill cases instead (64..1024 pairs): the sorted expert GEMM (gq_mmq_id_sorted) beside
(i) gq_act_prepare_grouped + gq_mmq_grouped_prepared over per-expert items whose rows were gathered
beforehand with the ids on the host, and (ii) the host-sorted loop mmq_id ran beyond 64 pairs before
the sorted entry existed (eager, wall time with its sync); the same interleaved median +- spread,
the sorted / baseline ratios, and the device time of each of the sorted entry's three launches.
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


# ---- prefill (--prefill): the sorted expert GEMM (gq_mmq_id_sorted) beside two baselines ----
# Every step reads all E experts, so only the tensor copies rotate (>= 1 GiB between two reads of a
# copy).  The ids are balanced (every expert P / E pairs, shuffled): baseline (i) needs one token
# count for all its items.
#   "sorted"      gq_mmq_id_sorted, graph-replayed, device-event times
#   "grouped"     (i) gq_act_prepare_grouped + gq_mmq_grouped_prepared over per-expert items, the
#                 ids on the host and every expert's rows ALREADY gathered (neither the gather nor
#                 the scatter of its outputs is in the step): the best the library offers when it
#                 is told the grouping; at most 16 items, so Mixtral only; graph-replayed
#   "host_sorted" (ii) the parent commit's mmq_id beyond 64 pairs: ids.cpu(), then index_select /
#                 mmq / index_copy_ per expert; eager, WALL time per call including its sync
# (name, type, E, M, K, N, S, per-slot rows)
PREFILL_CASES = [
    ("mixtral gate", "q4_k", 8, 14336, 4096, 64, 2, False),
    ("mixtral gate", "q4_k", 8, 14336, 4096, 512, 2, False),
    ("mixtral down", "q6_k", 8, 4096, 14336, 64, 2, True),
    ("mixtral down", "q6_k", 8, 4096, 14336, 512, 2, True),
    ("qwen-moe gate", "q4_k", 128, 768, 2048, 16, 8, False),
    ("qwen-moe gate", "q4_k", 128, 768, 2048, 128, 8, False),
]


class PrefillCase:
    def __init__(self, fmt, E, M, K, N, S, per_slot, dev, steps):
        import kernels._lib as kl
        self.kl, self.L, self.dev = kl, kl.lib(), dev
        self.fmt, self.gtype, self.E, self.M, self.K, self.N, self.S = fmt, kl.TYPES[fmt], E, M, K, N, S
        self.ebytes = M * (K // 256) * BLOCK[fmt][1]
        ncopies, self.plans = bench.rotation_plan(E * self.ebytes, steps)
        base = bench.device_random_blocks(fmt, E * M, K, dev, 1)
        self.A = [base] + [base.clone() for _ in range(ncopies - 1)]
        self.rotated = bench.rotated_bytes(E * self.ebytes, self.plans)
        P = N * S
        assert P % E == 0
        self.ids_np = np.random.default_rng(3).permutation(np.arange(P, dtype=np.int32) % E).reshape(N, S)
        self.ids = torch.from_numpy(self.ids_np).to(dev)
        g = torch.Generator(device=dev).manual_seed(2)
        self.B = torch.randn((N, S, K) if per_slot else (N, K), device=dev, generator=g).to(torch.float16)
        self.ldb, self.ldb_slot = (S * K, K) if per_slot else (K, 0)
        self.C = torch.empty((N, S, M), dtype=torch.float16, device=dev)
        need = int(self.L.gq_mmq_id_sorted_workspace_size(self.gtype, E, M, N, S, K))
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self.grouped = None

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _ok(self, rc):
        if rc:
            raise RuntimeError(self.L.gq_last_error().decode())

    def sorted_step(self, c):
        self._ok(self.L.gq_mmq_id_sorted(self.gtype, self.A[c].data_ptr(), self.ids.data_ptr(), self.B.data_ptr(),
                                         self.C.data_ptr(), self.E, self.M, self.N, self.S, self.K, self.ldb,
                                         self.ldb_slot, self.M, self.ws.data_ptr(), self.ws.numel(), self._stream()))

    def build_grouped(self):
        """Baseline (i): per-expert gathered rows, workspaces and outputs, made once."""
        kl, E, M, K = self.kl, self.E, self.M, self.K
        ne = self.N * self.S // E
        flat = self.B.reshape(-1, K)
        groups = kl.pairs_by_expert(self.ids_np, E)
        self.g_idx = [torch.tensor(groups[e], dtype=torch.int64, device=self.dev) for e in range(E)]
        self.g_x = [flat.index_select(0, i if self.ldb_slot else i // self.S).contiguous() for i in self.g_idx]
        self.g_ws = [torch.empty(kl.workspace_size(self.gtype, M, ne, K), dtype=torch.uint8, device=self.dev)
                     for _ in range(E)]
        self.g_c = [torch.empty((ne, M), dtype=torch.float16, device=self.dev) for _ in range(E)]
        self.g_prep = (kl.PrepItem * E)(*[kl.PrepItem(self.g_x[e].data_ptr(), ne, K, K, self.g_ws[e].data_ptr(),
                                                      self.g_ws[e].numel()) for e in range(E)])
        self.g_items = []
        for c in range(len(self.A)):
            arr = (kl.GemmItem * E)(*[kl.GemmItem(self.gtype, self.A[c].data_ptr() + e * self.ebytes,
                                                  self.g_ws[e].data_ptr(), self.g_c[e].data_ptr(), M, M, K)
                                      for e in range(E)])
            self.g_items.append(arr)
        pn = int(self.L.gq_mmq_grouped_prepared_workspace_size(0, self.g_items[0], E, ne))
        self.g_part = torch.empty(max(pn, 16), dtype=torch.uint8, device=self.dev)
        self.g_pn, self.g_ne = pn, ne
        self.grouped = True
        # more row tiles than the chip holds (Mixtral gate at 128 rows per expert): the grouped
        # GEMM refuses, and its header says what to do -- gq_mmq_prepared per item
        self._ok(self.L.gq_act_prepare_grouped(0, self.g_prep, E, self._stream()))
        rc = self.L.gq_mmq_grouped_prepared(0, self.g_items[0], E, ne, self.g_part.data_ptr() if pn else None, pn,
                                            self._stream())
        self.g_per_item = rc == kl.GQ_EUNSUPPORTED
        if not self.g_per_item:
            self._ok(rc)

    def grouped_step(self, c):
        self._ok(self.L.gq_act_prepare_grouped(0, self.g_prep, self.E, self._stream()))
        if self.g_per_item:
            for e in range(self.E):
                self._ok(self.L.gq_mmq_prepared(self.gtype, self.A[c].data_ptr() + e * self.ebytes,
                                                self.g_ws[e].data_ptr(), self.g_ws[e].numel(), self.g_c[e].data_ptr(),
                                                self.M, self.g_ne, self.K, self.M, self._stream()))
            return
        self._ok(self.L.gq_mmq_grouped_prepared(0, self.g_items[c], self.E, self.g_ne,
                                                self.g_part.data_ptr() if self.g_pn else None, self.g_pn, self._stream()))

    def host_sorted_step(self, c):
        """Baseline (ii): the parent commit's mmq_id fallback, line for line."""
        kl, E, M, K, N, S = self.kl, self.E, self.M, self.K, self.N, self.S
        experts = self.A[c].reshape(E, self.ebytes)
        rows = self.B.reshape(N * S, K) if self.ldb_slot else None
        res = self.C.view(N * S, M)
        res.zero_()
        for e, pairs in kl.pairs_by_expert(self.ids.cpu().numpy(), E).items():
            idx = torch.tensor(pairs, dtype=torch.int64, device=self.dev)
            x = rows.index_select(0, idx) if rows is not None else self.B.index_select(0, idx // S)
            res.index_copy_(0, idx, kl.mmq(self.gtype, experts[e], x, M, len(pairs), K))

    def check(self):
        """The three forms agree within the GEMM paths' tolerance (other kernels, other K splits)."""
        self.sorted_step(0)
        torch.cuda.synchronize(self.dev)
        want = self.C.clone().view(-1, self.M)
        scale = float(want.float().abs().max())
        self.C.zero_()
        self.host_sorted_step(0)
        torch.cuda.synchronize(self.dev)
        d = float((self.C.view(-1, self.M).float() - want.float()).abs().max()) / scale
        assert d <= 8e-3, ("host_sorted", d)
        if self.grouped:
            self.grouped_step(0)
            torch.cuda.synchronize(self.dev)
            for e in range(self.E):
                d = float((self.g_c[e].float() - want.index_select(0, self.g_idx[e]).float()).abs().max()) / scale
                assert d <= 8e-3, ("grouped", e, d)

    def graphs(self, step):
        grs = []
        for plan in self.plans:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for c in plan:
                    step(c)
            grs.append(gr)
        return grs

    def wall_us(self, steps):
        """Median wall time of one eager host-sorted call, its sync included."""
        import time
        ts = []
        for i in range(steps + 2):
            torch.cuda.synchronize(self.dev)
            t0 = time.perf_counter()
            self.host_sorted_step(i % len(self.A))
            torch.cuda.synchronize(self.dev)
            ts.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(ts[2:]))

    def launch_times(self, calls=8):
        """Mean device time of each of the sorted entry's three launches (torch profiler, eager
        calls rotating the copies); {} when the profiler gives no kernel records."""
        from torch.profiler import ProfilerActivity, profile
        self.sorted_step(0)
        torch.cuda.synchronize(self.dev)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for i in range(calls):
                self.sorted_step(i % len(self.A))
            torch.cuda.synchronize(self.dev)
        out = {}
        for ev in prof.key_averages():
            for short in ("id_sort_kernel", "act_quant_gather_kernel", "sgemm_id_kernel"):
                if short in ev.key:
                    total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
                    out[short] = round(total / max(1, ev.count), 2)
        return out


def prefill_main(a, dev):
    rows = []
    for name, fmt, E, M, K, N, S, per_slot in PREFILL_CASES:
        if a.only and a.only not in name:
            continue
        case = PrefillCase(fmt, E, M, K, N, S, per_slot, dev, a.steps)
        forms = {"sorted": case.sorted_step}
        if E <= 16:
            case.build_grouped()
            forms["grouped"] = case.grouped_step
        case.check()
        graphs = {f: case.graphs(fn) for f, fn in forms.items()}
        ts = {f: [] for f in list(forms) + ["host_sorted"]}
        for _ in range(a.repeats):  # interleaved: one pass over the forms per repeat
            for f in forms:
                ts[f].append(bench.timed_rotation(graphs[f], dev) / a.steps * 1e6)
            ts["host_sorted"].append(case.wall_us(min(a.steps, 10)))
        row = {"case": name, "type": fmt, "E": E, "M": M, "K": K, "N_tok": N, "S": S, "pairs": N * S,
               "step_weight_bytes": E * case.ebytes, "rotated_bytes": case.rotated}
        for f in ts:
            med = float(np.median(ts[f]))
            row[f] = {"us": round(med, 2), "spread_us": round(max(ts[f]) - min(ts[f]), 2),
                      "weight_GBps": round(E * case.ebytes / med / 1e3, 1)}
        if "grouped" in row:
            row["grouped"]["per_item_gemms"] = bool(case.g_per_item)
        for f in ("grouped", "host_sorted"):
            if f in row:
                row["sorted_over_" + f] = round(row["sorted"]["us"] / row[f]["us"], 3)
        slower = row["sorted"]["us"] - row["host_sorted"]["us"] > row["sorted"]["spread_us"] + row["host_sorted"]["spread_us"]
        row["slower_than_host_sorted"] = bool(slower)
        row["launch_us"] = case.launch_times()
        rows.append(row)
        print(json.dumps(row), flush=True)
        del graphs, case, forms
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="substring of the case names to run")
    ap.add_argument("--prefill", action="store_true",
                    help="the prefill cases instead: gq_mmq_id_sorted beside the grouped and host-sorted baselines")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench needs a ROCm GPU (no CPU timing)")
    dev = torch.device("cuda:0")
    if a.prefill:
        rows = prefill_main(a, dev)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump({"steps": a.steps, "repeats": a.repeats, "prefill": True, "rows": rows}, f, indent=1)
        return
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
