"""tests/golden/make_route_golden.py -- record the library's routing and workspace sizes.

    make -C gguf-triton-kernel_amd
    python tests/golden/make_route_golden.py

Every function asked here is host-only once GQ_CUS is set (the device's CU count never enters),
so this runs without a GPU.  For each (tuning set, type, act, M, N, K) of the grid it records
gq_debug_route for the raw and the prepared call, gq_mmq_workspace_size_ex and
gq_mmq_call_workspace_size into tests/golden/golden_routes.npz; tests/test_route_golden.py
replays the rows and requires every column equal.  Re-record only when a route or a size is
MEANT to change (the sizes are ABI-visible: gq_version).

Keys of the .npz (all rows in one order):
  routes   the route strings; raw / prep index into it
  knobs    the tuning sets as "GQ_X=v" ("" = the defaults); knob indexes into it
  type, act, M, N, K, knob, raw, prep, ws, call_ws    int64[rows]

The file may not grow past golden_q8_0.npz.  Stored column by column the full grid below fits
(about 170 KB), so THIN_M / THIN_N are the full lists; should they ever be thinned, the kept rows
may lose no route string and no tuning set's effect, which main() asserts against the full grid.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "gguf-triton-kernel_amd"))
OUT = os.path.join(REPO, "tests", "golden", "golden_routes.npz")
MAX_BYTES = os.path.getsize(os.path.join(REPO, "tests", "golden", "golden_q8_0.npz"))

TYPES = (0, 1, 2, 3, 4)  # Q8_0, Q4_K, Q6_K, Q5_K, Q3_K
ACTS = (0, 1)            # q8_1, fp8
FULL_M = (16, 64, 100, 512, 4096, 8192, 11008, 28672)
FULL_N = (1, 2, 3, 4, 5, 8, 16, 17, 32, 33, 64, 65, 128, 200, 767, 768)
KS = (96, 256, 2816, 4096, 8192, 11008, 28672)  # 96: Q8_0 only (32-element blocks)
# the recorded M / N (see the module docstring)
THIN_M = FULL_M
THIN_N = FULL_N
BASE = ("GQ_CUS", 256)
KNOBS = ((), ("GQ_SKINNY", 0), ("GQ_SKINNY", 1), ("GQ_RGEMM", 0), ("GQ_RGEMM", 1), ("GQ_SGEMM", 0), ("GQ_SGEMM", 1),
         ("GQ_KSTREAM", 0), ("GQ_KSTREAM", 1), ("GQ_GEMM_SPLITS", 4), ("GQ_GEMM_I8", 1), ("GQ_BLAS_MIN_TOKENS", 0),
         ("GQ_NO_FUSED_DECODE", 1), ("GQ_GEMM_MAX_BYTES", 1 << 20), ("GQ_SGEMM_STREAMK", 1), ("GQ_SGEMM_SPLITS", 2),
         ("GQ_CUS", 96))


def knob_name(k):
    return f"{k[0]}={k[1]}" if k else ""


def apply_knob(kl, name):
    """The tuning set `name` ("GQ_X=v" or ""), over GQ_CUS=256."""
    kl.reset_tuning()
    kl.set_tuning(*BASE)
    if name:
        key, v = name.split("=")
        kl.set_tuning(key, int(v))


def query(kl, t, act, M, N, K):
    """(raw route, prepared route, gq_mmq_workspace_size_ex, gq_mmq_call_workspace_size)."""
    L = kl.lib()
    return (L.gq_debug_route(t, act, M, N, K, 0).decode(), L.gq_debug_route(t, act, M, N, K, 1).decode(),
            int(L.gq_mmq_workspace_size_ex(t, act, M, N, K)), int(L.gq_mmq_call_workspace_size(t, act, M, N, K)))


def record(kl, Ms, Ns):
    rows = []
    for ki, knob in enumerate(KNOBS):
        apply_knob(kl, knob_name(knob))
        for t in TYPES:
            for act in ACTS:
                for K in KS:
                    if K % (32 if t == 0 else 256):
                        continue
                    for M in Ms:
                        for N in Ns:
                            rows.append((t, act, M, N, K, ki) + query(kl, t, act, M, N, K))
    kl.reset_tuning()
    return rows


def main():
    import kernels._lib as kl
    full = record(kl, FULL_M, FULL_N)
    keep_m, keep_n = set(THIN_M), set(THIN_N)
    thin = [r for r in full if r[2] in keep_m and r[3] in keep_n]
    # the thinned grid keeps every route string, raw and prepared
    names = sorted({r[6] for r in full} | {r[7] for r in full})
    for col in (6, 7):
        lost = {r[col] for r in full} - {r[col] for r in thin}
        assert not lost, f"thinning loses route strings {lost} (column {col})"
    # ... and every tuning set still differs from the defaults somewhere
    base = {r[:5]: r[6:] for r in thin if r[5] == 0}
    for ki in range(1, len(KNOBS)):
        assert any(base[r[:5]] != r[6:] for r in thin if r[5] == ki), f"{knob_name(KNOBS[ki])} changes no kept row"
    idx = {n: i for i, n in enumerate(names)}
    cols = {name: np.array([r[i] for r in thin], np.int64)
            for i, name in enumerate(("type", "act", "M", "N", "K", "knob"))}
    cols["raw"] = np.array([idx[r[6]] for r in thin], np.int64)
    cols["prep"] = np.array([idx[r[7]] for r in thin], np.int64)
    cols["ws"] = np.array([r[8] for r in thin], np.int64)
    cols["call_ws"] = np.array([r[9] for r in thin], np.int64)
    np.savez_compressed(OUT, routes=np.array(names), knobs=np.array([knob_name(k) for k in KNOBS]), **cols)
    size = os.path.getsize(OUT)
    print(f"{len(full)} rows in the full grid, {len(thin)} recorded, {len(names)} route strings, {size} bytes")
    assert size <= MAX_BYTES, f"{size} bytes > {MAX_BYTES}: thin THIN_M / THIN_N further"


if __name__ == "__main__":
    main()
