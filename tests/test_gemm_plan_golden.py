"""The 256-row tile family's workspace sizes against the recorded grid (CPU: both queries are
host-only once GQ_CUS is set, and the grouped one never dereferences its items' pointers).
tests/golden/make_gemm_plan_golden.py recorded golden_gemm_plans.npz; a size that moves fails here,
row by row, with no tolerance."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gen():
    """The generator module: the test asks through its item lists and query functions."""
    spec = importlib.util.spec_from_file_location("make_gemm_plan_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_gemm_plan_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def grid():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_gemm_plans.npz"))


def test_grouped_sizes_match_the_recorded_grid(gen, grid):
    import kernels._lib as kl
    knobs = [str(s) for s in grid["knobs"]]
    lists = gen.item_lists()
    assert [n for n, _ in lists] == [str(s) for s in grid["lists"]] and knobs == list(gen.KNOBS)
    rows = list(zip(*(grid[k].tolist() for k in ("g_knob", "g_list", "g_N", "g_size"))))
    assert len(rows) == len(knobs) * len(lists) * len(gen.TOKENS)
    current, bad = None, []
    try:
        for knob, li, N, size in rows:
            if knob != current:
                gen.apply_knobs(kl, knobs[knob])
                current = knob
            got = gen.grouped_size(kl, lists[li][1], N)
            if got != size:
                bad.append((knobs[knob], lists[li][0], N, got, size))
    finally:
        kl.reset_tuning()
    assert not bad, f"{len(bad)} rows differ (tuning, items, N, got, recorded), the first: {bad[:5]}"


def test_sorted_sizes_match_the_recorded_grid(gen, grid):
    import kernels._lib as kl
    names = {v: k for k, v in kl.TYPES.items()}
    rows = list(zip(*(grid[k].tolist() for k in ("s_type", "s_E", "s_M", "s_pairs", "s_K", "s_size"))))
    assert len(rows) == len(gen.TYPES) * len(gen.SORTED_E) * len(gen.SORTED_M) * len(gen.SORTED_PAIRS) * len(gen.SORTED_K)
    bad = []
    try:
        gen.apply_knobs(kl, str(grid["knobs"][0]))
        for t, E, M, P, K, size in rows:
            got = gen.sorted_size(kl, names[t], E, M, P, K)
            if got != size:
                bad.append((names[t], E, M, P, K, got, size))
    finally:
        kl.reset_tuning()
    assert not bad, f"{len(bad)} rows differ (type, E, M, pairs, K, got, recorded), the first: {bad[:5]}"


def test_grid_holds_both_answers_and_every_knob_acts(gen, grid):
    """What the generator asserted, on the file itself."""
    size, knob = grid["g_size"], grid["g_knob"]
    assert (size > 0).any() and (size == 0).any() and (grid["s_size"] > 0).all()
    refused = len(grid["lists"]) - 1
    assert str(grid["lists"][refused]) == "q4_0+q3_k" and (size[grid["g_list"] == refused] == 0).all()
    base = size[knob == 0]
    for ki in range(1, len(grid["knobs"])):
        moved = bool((size[knob == ki] != base).any())
        assert moved != (str(grid["knobs"][ki]) in gen.SIZE_NEUTRAL), grid["knobs"][ki]
