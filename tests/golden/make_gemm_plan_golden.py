"""tests/golden/make_gemm_plan_golden.py -- record the 256-row tile family's workspace sizes.

    make -C gguf-triton-kernel_amd
    python tests/golden/make_gemm_plan_golden.py

The two size queries asked here -- gq_mmq_grouped_prepared_workspace_size (plan_sgemm_grouped, both
its stream-K and its whole-tile branch) and gq_mmq_id_sorted_workspace_size (plan_sgemm_id) -- are
host-only once GQ_CUS is set, and the grouped query reads its items' pointers as numbers only (null
checks, the output's alignment): it dereferences nothing, so the items carry fixed fake addresses
and this runs without a GPU.  The dense sizes (plan_rgemm, plan_sgemm, plan_gemm) are held by
golden_routes.npz.  tests/test_gemm_plan_golden.py replays the rows and requires every size equal.
Re-record only when a size is MEANT to change (the sizes are ABI-visible: gq_version).

Keys of the .npz:
  knobs     the tuning sets as "GQ_X=v,..." (each over a reset; knobs[0] is the default)
  lists     the grouped item lists' names
  g_knob, g_list, g_N, g_size    int64[rows]: the grouped query (q8_1 activations)
  s_type, s_E, s_M, s_pairs, s_K, s_size    int64[rows]: the sorted query (N = pairs, S = 1) at knobs[0]
"""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "gguf-triton-kernel_amd"))
OUT = os.path.join(REPO, "tests", "golden", "golden_gemm_plans.npz")

TOKENS = (5, 16, 17, 32, 33, 64, 65, 128, 200)
TYPES = ("q8_0", "q4_k", "q6_k", "q5_k", "q3_k", "q2_k", "q4_0")
SINGLE_MK = ((256, 256), (300, 512), (4096, 4096), (11008, 4096), (4096, 11008))
KNOBS = ("GQ_CUS=256", "GQ_CUS=256,GQ_SGEMM_STREAMK=0", "GQ_CUS=256,GQ_SGEMM_SPLITS=2", "GQ_CUS=256,GQ_RGEMM_ILC=1",
         "GQ_CUS=64")
SIZE_NEUTRAL = ("GQ_CUS=256,GQ_RGEMM_ILC=1",)  # recorded all the same: main() asserts it moves no row
SORTED_E = (4, 64, 1024)
SORTED_M = (70, 4096)
SORTED_PAIRS = (65, 80, 4096, 65536)
SORTED_K = (256, 4096)


def item_lists():
    """[(name, [(type name, M, K), ...])]: the grouped query's item lists."""
    from gguf.mix import LLAMA_LAYER_SHAPES, q2_k_layer_types, q4_k_m_layer_types
    out = [(f"{t}_{M}x{K}", [(t, M, K)]) for t in TYPES for M, K in SINGLE_MK]
    for name, types in (("q4_k_m_layer", q4_k_m_layer_types(0, 32)), ("q2_k_layer", q2_k_layer_types(0, 32))):
        out.append((name, [(types[p], M, K) for p, (M, K) in LLAMA_LAYER_SHAPES.items()]))
    out.append(("q4_0+q3_k", [("q4_0", 4096, 4096), ("q3_k", 4096, 4096)]))  # refused: no kernel holds both
    return out


def apply_knobs(kl, name):
    kl.reset_tuning()
    for kv in name.split(","):
        key, v = kv.split("=")
        kl.set_tuning(key, int(v))


def grouped_size(kl, items, N):
    """gq_mmq_grouped_prepared_workspace_size of the (type name, M, K) items at N tokens; item i's
    three pointers are the fake, 4096-aligned addresses (3i + 1..3) << 32 (never dereferenced)."""
    arr = (kl.GemmItem * len(items))()
    for i, (t, M, K) in enumerate(items):
        arr[i] = kl.GemmItem(kl.TYPES[t], (3 * i + 1) << 32, (3 * i + 2) << 32, (3 * i + 3) << 32, M, M, K)
    return int(kl.lib().gq_mmq_grouped_prepared_workspace_size(kl.GQ_ACT_Q8_1, arr, len(items), N))


def sorted_size(kl, t, E, M, pairs, K):
    return int(kl.lib().gq_mmq_id_sorted_workspace_size(kl.TYPES[t], E, M, pairs, 1, K))


def main():
    import kernels._lib as kl
    lists = item_lists()
    g_rows = []
    for ki, knob in enumerate(KNOBS):
        apply_knobs(kl, knob)
        for li, (_, items) in enumerate(lists):
            for N in TOKENS:
                g_rows.append((ki, li, N, grouped_size(kl, items, N)))
    apply_knobs(kl, KNOBS[0])
    s_rows = [(kl.TYPES[t], E, M, P, K, sorted_size(kl, t, E, M, P, K))
              for t in TYPES for E in SORTED_E for M in SORTED_M for P in SORTED_PAIRS for K in SORTED_K]
    kl.reset_tuning()
    # both answers occur, the refused pair stays refused, and every tuning set moves some row
    assert any(r[3] > 0 for r in g_rows) and any(r[3] == 0 for r in g_rows)
    assert all(r[5] > 0 for r in s_rows), "every sorted shape of the grid has a plan"
    refused = len(lists) - 1
    assert all(r[3] == 0 for r in g_rows if r[1] == refused), "the Q4_0 + Q3_K pair got a plan"
    base = {r[1:3]: r[3] for r in g_rows if r[0] == 0}
    for ki in range(1, len(KNOBS)):
        moved = any(base[r[1:3]] != r[3] for r in g_rows if r[0] == ki)
        # GQ_RGEMM_ILC is decided at the launch (by the kernel's occupancy): every split plan holds the
        # combine's flags and nonces whatever the knob says, so its rows must equal the default's
        assert moved != (KNOBS[ki] in SIZE_NEUTRAL), f"{KNOBS[ki]}: rows moved = {moved}"
    g = np.array(g_rows, np.int64)
    s = np.array(s_rows, np.int64)
    np.savez_compressed(OUT, knobs=np.array(KNOBS), lists=np.array([n for n, _ in lists]),
                        g_knob=g[:, 0], g_list=g[:, 1], g_N=g[:, 2], g_size=g[:, 3],
                        s_type=s[:, 0], s_E=s[:, 1], s_M=s[:, 2], s_pairs=s[:, 3], s_K=s[:, 4], s_size=s[:, 5])
    print(f"{len(g_rows)} grouped rows ({sum(r[3] > 0 for r in g_rows)} non-zero), {len(s_rows)} sorted rows "
          f"({sum(r[5] > 0 for r in s_rows)} non-zero), {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
