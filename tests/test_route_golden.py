"""The library's routing and workspace sizes against the recorded grid (CPU: every function asked
here is host-only once GQ_CUS is set).  tests/golden/make_route_golden.py recorded
golden_routes.npz; a route or a size that moves fails here, row by row, with no tolerance."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def grid():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_routes.npz"))


def test_routes_and_sizes_match_the_recorded_grid(grid):
    import kernels._lib as kl
    L = kl.lib()
    routes = [str(s) for s in grid["routes"]]
    knobs = [str(s) for s in grid["knobs"]]
    cols = [grid[k].tolist() for k in ("type", "act", "M", "N", "K", "knob", "raw", "prep", "ws", "call_ws")]
    assert len(cols[0]) > 0
    current, bad = None, []
    try:
        for t, act, M, N, K, knob, raw, prep, ws, call_ws in zip(*cols):
            if knob != current:
                kl.reset_tuning()
                kl.set_tuning("GQ_CUS", 256)
                if knobs[knob]:
                    key, v = knobs[knob].split("=")
                    kl.set_tuning(key, int(v))
                current = knob
            got = (L.gq_debug_route(t, act, M, N, K, 0).decode(), L.gq_debug_route(t, act, M, N, K, 1).decode(),
                   int(L.gq_mmq_workspace_size_ex(t, act, M, N, K)), int(L.gq_mmq_call_workspace_size(t, act, M, N, K)))
            want = (routes[raw], routes[prep], ws, call_ws)
            if got != want:
                bad.append((knobs[knob], t, act, M, N, K, got, want))
    finally:
        kl.reset_tuning()
    assert not bad, f"{len(bad)} rows differ (tuning, type, act, M, N, K, got, recorded), the first: {bad[:5]}"
    # the q8_1-only grid through the plain entry
    assert int(L.gq_mmq_workspace_size(1, 4096, 16, 4096)) == int(L.gq_mmq_workspace_size_ex(1, 0, 4096, 16, 4096))


def test_grid_covers_every_route_and_knob(grid):
    """What the generator asserted when it thinned the grid, on the file itself."""
    n = len(grid["routes"])
    assert set(grid["raw"].tolist()) == set(range(n)) and set(grid["prep"].tolist()) == set(range(n))
    key = np.stack([grid[k] for k in ("type", "act", "M", "N", "K")], 1)
    val = np.stack([grid[k] for k in ("raw", "prep", "ws", "call_ws")], 1)
    base = {tuple(k): tuple(v) for k, v in zip(key[grid["knob"] == 0].tolist(), val[grid["knob"] == 0].tolist())}
    for ki in range(1, len(grid["knobs"])):
        sel = grid["knob"] == ki
        assert any(base[tuple(k)] != tuple(v) for k, v in zip(key[sel].tolist(), val[sel].tolist())), grid["knobs"][ki]


def test_size_queries_refuse_what_the_launch_refuses():
    """A K that is not whole blocks, or an unknown type: 0 from every size function (K = 96 with a
    256-element block once divided by K / 256 = 0 on the host)."""
    import kernels._lib as kl
    L = kl.lib()
    for t, act, M, N, K in ((kl.GQ_Q4_K, kl.GQ_ACT_Q8_1, 16, 1, 96), (7, kl.GQ_ACT_Q8_1, 16, 1, 256)):
        assert L.gq_mmq_call_workspace_size(t, act, M, N, K) == 0
        assert L.gq_mmq_workspace_size_ex(t, act, M, N, K) == 0
        assert L.gq_mmq_workspace_size(t, M, N, K) == 0
        assert L.gq_mmq_sharded_workspace_size(t, M, N, K, 2) == 0
