"""Guarded buffers for the stride tests (tests/test_strides_host.py, test_gpu_strides.py): an output
wider than the result, an input wider than the activations, a workspace with a band behind it.
Each comes with a checker that fails when anything outside the part a call may touch was changed,
naming the first changed position.  Plain functions on torch tensors; device=None is cuda:0, the
host tests pass "cpu".

Positions are counted from the view: element e of the allocation is (row, column) =
divmod(e - start, ld), start the view's first element -- so the first pad column of row n is
(n, M), the element after the last row's M is (N - 1, M), and the one before the view (-1, ld - 1)."""
import numpy as np
import torch

GUARD = 64             # elements before the view and at least as many behind it; keeps 16-byte alignment
SENTINEL = 0x7D5B      # an fp16 NaN with a payload no kernel produces
WS_TAIL, WS_FILL = 4096, 0xA5
INF, FMAX = float("inf"), 65504.0  # the poisons of wide_in


def _dev(device):
    return torch.device("cuda:0" if device is None else device)


def wide_out(N, M, ldc, lead, device=None):
    """(flat, view, check): a flat fp16 allocation filled with SENTINEL, its (N, M) view with rows
    ldc apart starting `lead` elements behind a 16-byte aligned address (GUARD elements into the
    allocation), and check(), which asserts that every element outside the view's N runs of M still
    holds SENTINEL."""
    assert ldc >= M and lead >= 0
    start = GUARD + lead
    total = start + (N - 1) * ldc + M + GUARD + 8
    flat = torch.full((total,), SENTINEL, dtype=torch.int16, device=_dev(device)).view(torch.float16)
    assert flat.data_ptr() % 16 == 0
    view = flat.as_strided((N, M), (ldc, 1), start)
    e = torch.arange(total, device=flat.device) - start
    inside = (e >= 0) & (e < (N - 1) * ldc + M) & (e % ldc < M)

    def check():
        bad = (flat.view(torch.int16) != SENTINEL) & ~inside
        if bool(bad.any()):
            first = int(torch.nonzero(bad)[0]) - start
            row, col = first // ldc, first % ldc
            raise AssertionError(f"wrote outside the (N={N}, M={M}) result, ldc={ldc} lead={lead}: first at "
                                 f"(row {row}, column {col}), {int(bad.sum())} elements in all")

    return flat, view, check


def wide_in(B, ldb, lead, poison, device=None):
    """The (N, K) device view, rows ldb apart and `lead` elements behind a 16-byte aligned address,
    of a flat allocation that holds the fp16 array B in the view and `poison` everywhere else: the
    GUARD elements and the lead in front, the ldb - K pad columns of every row, and 16 whole rows
    and GUARD elements behind row N - 1."""
    B = np.asarray(B)
    N, K = B.shape
    assert B.dtype == np.float16 and ldb >= K and lead >= 0
    start = GUARD + lead
    flat = torch.full((start + (N + 16) * ldb + GUARD,), poison, dtype=torch.float16, device=_dev(device))
    assert flat.data_ptr() % 16 == 0
    view = flat.as_strided((N, K), (ldb, 1), start)
    view.copy_(torch.from_numpy(np.ascontiguousarray(B)))
    return view


def guarded_ws(need, device=None):
    """(alloc, front, check): a uint8 allocation of need + WS_TAIL bytes, its first `need` bytes
    (the workspace to hand to a call) and check(), which asserts that the WS_TAIL bytes behind them
    still hold WS_FILL.  The front is filled too, so that two workspaces written by the same calls
    can be compared byte for byte, alignment gaps included."""
    alloc = torch.full((need + WS_TAIL,), WS_FILL, dtype=torch.uint8, device=_dev(device))
    front = alloc[:need]

    def check():
        bad = alloc[need:] != WS_FILL
        if bool(bad.any()):
            raise AssertionError(f"wrote behind the {need}-byte workspace: first at byte {need + int(torch.nonzero(bad)[0])}, "
                                 f"{int(bad.sum())} bytes in all")

    return alloc, front, check
