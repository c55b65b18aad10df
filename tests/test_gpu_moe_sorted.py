"""GPU tests of the sorted expert GEMM (gq_mmq_id_sorted: csrc/mmq_idsort.hip id_sort_kernel,
csrc/act_quant.hip act_quant_gather_kernel, csrc/mmq_rgemm.hip sgemm_id_kernel): mixture-of-experts
blocks beyond gq_mmq_id's 64 pairs, sorted on the device.  Gates and helpers as
tests/test_gpu_moe.py: every pair's row against the oracle on sampled weight rows at the GEMM
gates (Q5_K: tests/q5k_model.py at tests/test_gpu_q5k.py's), and bit for bit against the library's
own streaming GEMM per expert (one K split) -- the same x~ bytes, the same body, independent MFMA
columns.  Id patterns that hit the tile table's edges (an expert never chosen, chosen once,
exactly one tile, two tiles), independence of the other pairs' ids, ids outside [0, E), strides,
graph replay over new ids, and MoEFFN captured in a graph."""
import functools

import numpy as np
import pytest
import torch

import oracle as O
import type_models as TM
from gpu_types import dev as _dev, no_timeouts as _no_timeouts, same_bits as _same_bits, to_w as _w
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

TIGHT_GEMM = 4e-3  # tests/test_gpu_moe.py's GEMM gate vs IDEAL

# (type, E, M, K)
SHAPES = [("q4_k", 4, 130, 1024),   # row tail not a multiple of 4
          ("q5_k", 4, 200, 512),
          ("q6_k", 3, 257, 768),    # a second row tile of one row
          ("q8_0", 5, 96, 1024)]
PAIRSETS = [(5, 1), (33, 2), (40, 8)]
# the 16-token groups per tile the plan must pick: plan_sgemm's thresholds at ceil(P / min(E, P))
EXPECT_NB = {(3, 5, 1): 1, (4, 5, 1): 1, (5, 5, 1): 1,      # 2 pairs per expert
             (3, 33, 2): 2, (4, 33, 2): 2, (5, 33, 2): 1,   # 22, 17, 14
             (3, 40, 8): 8, (4, 40, 8): 8, (5, 40, 8): 4}   # 107, 80, 64
# the library's streaming GEMM, one K split, whatever the token count
PINS = dict(GQ_SGEMM=1, GQ_SGEMM_SPLITS=1, GQ_SKINNY=0, GQ_RGEMM=0, GQ_KSTREAM=0)


@functools.lru_cache(maxsize=None)
def _experts(fmt, E, M, K):
    """E packed matrices back to back (exactly E experts: nothing to read past them), read-only."""
    raw = np.concatenate([random_blocks(fmt, M, K, seed=2000 * E + 10 * M + e) for e in range(E)])
    raw.setflags(write=False)
    return raw


def _nb(P, E):
    ne = min(E, P)
    avg = (P + ne - 1) // ne
    return 8 if avg > 64 else (4 if avg > 32 else (2 if avg > 16 else 1))


def _plan_nb(kl, gtype, E, M, N, S, K):
    """The NB the library planned, from its workspace size: x~ (P*K*2), perm (4P, 16-aligned), a
    16-byte header, 16 bytes per table entry for min(E, P) + P / (16 NB) entries, 15 of slack."""
    P = N * S
    ws = int(kl.lib().gq_mmq_id_sorted_workspace_size(gtype, E, M, N, S, K))
    t_max, rem = divmod(ws - 15 - P * K * 2 - ((4 * P + 15) & ~15) - 16, 16)
    assert rem == 0 and t_max >= min(E, P)
    full = t_max - min(E, P)  # = P // (16 * NB)
    for nb in (1, 2, 4, 8):
        if P // (16 * nb) == full:
            return nb
    raise AssertionError((ws, t_max))


def _pattern(N, S, E):
    """(N, S) ids that hit the table's edges, by the plan's own tile size BN = 16 * NB."""
    P = N * S
    bn = 16 * _nb(P, E)
    if (N, S) == (5, 1):  # all on one expert
        flat = np.full(P, E - 1, dtype=np.int32)
    elif (N, S) == (33, 2):  # round robin; expert 1 never chosen, expert 2 exactly once
        rr = [e for e in range(E) if e not in (1, 2)]
        flat = np.array([rr[p % len(rr)] for p in range(P)], dtype=np.int32)
        flat[17] = 2
    else:  # skewed: 60% on expert 0 (more than one tile), the last expert exactly one tile (or 16)
        assert (N, S) == (40, 8)
        big = 192
        exact = bn if big + bn + (E - 2) <= P else 16
        mid = list(range(1, E - 1))
        rest = [mid[i % len(mid)] for i in range(P - big - exact)]
        flat = np.array([0] * big + [E - 1] * exact + rest, dtype=np.int32)
        flat = flat[np.random.default_rng(7).permutation(P)]
    return flat.reshape(N, S)


def _per_expert(kl, gtype, A, E, ids, rows, M, K):
    """(N, S, M): one streaming-GEMM mmq() (pinned: sgemm_kernel, one split) per chosen expert over
    its pairs' gathered rows in ascending pair order, padded to 5 tokens by repeating the last;
    zeros for ids outside [0, E).  rows: (N, K) shared or (N, S, K) per slot."""
    N, S = ids.shape
    per = A.numel() // E
    flat = rows.reshape(N * S, K) if rows.dim() == 3 else None
    want = torch.zeros((N * S, M), dtype=torch.float16, device=A.device)
    with kl.tuning(**PINS):
        for e, pairs in kl.pairs_by_expert(ids, E).items():
            idx = torch.tensor(pairs, dtype=torch.int64, device=A.device)
            x = flat.index_select(0, idx) if flat is not None else rows.index_select(0, idx // S)
            n = len(pairs)
            if n < 5:
                x = torch.cat([x, x[-1:].expand(5 - n, K)])
            x = x.contiguous()
            assert kl.route_name(gtype, M, x.shape[0], K) == "sgemm_kernel", (e, x.shape[0])
            want[idx] = kl.mmq(gtype, A[e * per:(e + 1) * per], x, M, x.shape[0], K)[:n]
    return want.view(N, S, M)


@pytest.mark.parametrize("N,S", PAIRSETS)
@pytest.mark.parametrize("fmt,E,M,K", SHAPES)
def test_sorted_oracle_and_bit_identity(fmt, E, M, K, N, S):
    import kernels._lib as kl
    gtype = kl.TYPES[fmt]
    P = N * S
    nb = _nb(P, E)
    assert nb == EXPECT_NB[(E, N, S)]
    assert _plan_nb(kl, gtype, E, M, N, S, K) == nb
    ids = _pattern(N, S, E)
    counts = np.bincount(ids.reshape(-1), minlength=E)
    if (N, S) == (33, 2):
        assert counts[1] == 0 and counts[2] == 1
    if (N, S) == (40, 8):
        assert counts[0] == 192 and -(-192 // (16 * nb)) >= 2  # expert 0 spans token tiles
        assert counts[E - 1] in (16 * nb, 16)                   # a group that is exactly one tile (or 16)
    raw = _experts(fmt, E, M, K)
    A = _w(raw)
    x = random_activations(N, K, seed=K + N + S)
    xt, it = torch.from_numpy(x).to(_dev()), torch.from_numpy(ids).to(_dev())
    got = kl.mmq_id_sorted(gtype, A, it, xt, E, M, K)
    torch.cuda.synchronize()
    assert got.shape == (N, S, M) and got.dtype == torch.float16
    # every pair's row against the oracle, on sampled weight rows of its expert
    rng = np.random.default_rng(P + M)
    per, rb = raw.size // E, raw.size // E // M
    g = got.cpu().numpy().reshape(P, M)
    for e, pairs in kl.pairs_by_expert(ids, E).items():
        wr = np.sort(rng.choice(M, size=24, replace=False))
        sub = np.concatenate([raw[e * per + r * rb:e * per + (r + 1) * rb] for r in wr])
        B = x[[p // S for p in pairs]]
        sel = g[pairs][:, wr]
        if fmt == "q5_k":
            err = TM.rel_err(sel, TM.judge(fmt, sub, B, len(wr), len(pairs), K))
            print(f"{fmt} E={E} {M}x{K} ({N},{S}) expert {e}: {len(pairs)} pairs, max|d|/max|C| = {err:.2e}")
            assert err <= TM.TIGHT_GEMM, (e, err)
            continue
        err = O.max_rel_err(sel, O.mmq_from_fp16(fmt, sub, B, len(wr), len(pairs), K, O.IDEAL))
        print(f"{fmt} E={E} {M}x{K} ({N},{S}) expert {e}: {len(pairs)} pairs, max|d|/max|C| = {err:.2e}")
        assert err <= TIGHT_GEMM, (e, err)
        assert O.allclose(O.mmq_from_fp16(fmt, sub, B, len(wr), len(pairs), K, O.EXACT), sel, 0.01), e
    # bit for bit the library's own streaming GEMM per expert
    assert _same_bits(got, _per_expert(kl, gtype, A, E, ids, xt, M, K))
    _no_timeouts()


def test_largest_sort():
    """The entry's limits at once -- E = 1024 experts, 65536 pairs (every wave of the sort a full
    4096-pair range, 2048 table entries) -- on tiny experts: random ids (groups of 64 +- a few: one
    or two 64-token tiles), some out of range; bit for bit the per-expert streaming GEMM."""
    import kernels._lib as kl
    dev = _dev()
    fmt, E, M, K, N, S = "q4_k", 1024, 16, 256, 8192, 8
    gtype = kl.TYPES[fmt]
    assert _nb(N * S, E) == 4 and _plan_nb(kl, gtype, E, M, N, S, K) == 4
    A = _w(random_blocks(fmt, E * M, K, seed=77))
    ids = np.random.default_rng(11).integers(0, E, size=(N, S), dtype=np.int32)
    ids[::97, 3] = E
    ids[5::1013, 0] = -1
    counts = np.bincount(ids[(ids >= 0) & (ids < E)].reshape(-1), minlength=E)
    assert counts.max() > 64 and counts.min() < 64
    x = torch.from_numpy(random_activations(N, K, seed=19)).to(dev)
    got = kl.mmq_id_sorted(gtype, A, torch.from_numpy(ids).to(dev), x, E, M, K)
    torch.cuda.synchronize()
    assert not bool(got[0, 3].any()) and not bool(got[5, 0].any())
    assert _same_bits(got, _per_expert(kl, gtype, A, E, ids, x, M, K))
    _no_timeouts()


def test_pair_independent_of_other_ids():
    """The same pair -- same expert, same row -- in two launches of one shape whose other ids
    differ (other group sizes, another place in its group and tile): identical bits."""
    import kernels._lib as kl
    dev = _dev()
    fmt, E, M, K = SHAPES[0]
    N, S = 33, 2
    A = _w(_experts(fmt, E, M, K))
    x = torch.from_numpy(random_activations(N, K, seed=31)).to(dev)
    a = _pattern(N, S, E)
    b = np.random.default_rng(5).integers(0, E, size=(N, S), dtype=np.int32)
    keep = [(0, 0), (8, 1), (20, 0), (32, 1)]
    for n, s in keep:
        b[n, s] = a[n, s]
    assert not np.array_equal(np.bincount(a.reshape(-1), minlength=E), np.bincount(b.reshape(-1), minlength=E))
    ga = kl.mmq_id_sorted(kl.TYPES[fmt], A, torch.from_numpy(a).to(dev), x, E, M, K)
    gb = kl.mmq_id_sorted(kl.TYPES[fmt], A, torch.from_numpy(b).to(dev), x, E, M, K)
    torch.cuda.synchronize()
    for n, s in keep:
        assert _same_bits(ga[n, s], gb[n, s]), (n, s)
        assert bool(ga[n, s].abs().max() > 0)
    _no_timeouts()


@pytest.mark.parametrize("fmt,E,M,K", [SHAPES[0], SHAPES[2]])
def test_invalid_ids_give_zero_rows(fmt, E, M, K):
    """Pairs whose id is -1 or E (or far out): all-zero rows (written: the buffer starts as NaN),
    the other pairs unchanged.  A holds exactly E experts."""
    import kernels._lib as kl
    dev = _dev()
    gtype = kl.TYPES[fmt]
    A = _w(_experts(fmt, E, M, K))
    N, S = 33, 2
    ids = _pattern(N, S, E)
    x = torch.from_numpy(random_activations(N, K, seed=11)).to(dev)
    clean = kl.mmq_id_sorted(gtype, A, torch.from_numpy(ids).to(dev), x, E, M, K)
    bad = [(0, 1), (2, 0), (16, 1), (32, 1)]
    for (n, s), v in zip(bad, (-1, E, E + 1000, -(1 << 31))):
        ids[n, s] = v
    out = torch.full((N, S, M), float("nan"), dtype=torch.float16, device=dev)
    kl.mmq_id_sorted(gtype, A, torch.from_numpy(ids).to(dev), x, E, M, K, out=out)
    torch.cuda.synchronize()
    for n, s in bad:
        assert torch.all(out[n, s].view(torch.int16) == 0), (n, s)
        clean[n, s] = 0
    assert _same_bits(out, clean)
    _no_timeouts()


def test_shared_vs_per_slot_rows_and_strides():
    """ldb_slot = 0 equals a materialised (N, S, K) copy; strided B views (rows 2K apart, off the
    row start; per slot: slots 2K apart) give the bits of their contiguous copies; ldc > M into a
    sentinel-filled buffer leaves the sentinels."""
    import kernels._lib as kl
    dev = _dev()
    fmt, E, M, K = SHAPES[0]
    gtype = kl.TYPES[fmt]
    N, S = 33, 2
    A = _w(_experts(fmt, E, M, K))
    ids = _pattern(N, S, E)
    it = torch.from_numpy(ids).to(dev)
    x = torch.from_numpy(random_activations(N, K, seed=5)).to(dev)
    shared = kl.mmq_id_sorted(gtype, A, it, x, E, M, K)
    copy = x[:, None, :].expand(N, S, K).contiguous()
    assert _same_bits(kl.mmq_id_sorted(gtype, A, it, copy, E, M, K), shared)
    wide = torch.from_numpy(random_activations(N, 2 * K, seed=6)).to(dev)
    view = wide[:, 301:301 + K]  # row stride 2K, 602 bytes off the row start: fp16 alignment only
    assert view.stride(0) == 2 * K and view.data_ptr() % 4 == 2
    assert _same_bits(kl.mmq_id_sorted(gtype, A, it, view, E, M, K),
                      kl.mmq_id_sorted(gtype, A, it, view.contiguous(), E, M, K))
    slots = torch.from_numpy(random_activations(N * S, 2 * K, seed=7)).to(dev).view(N, S, 2 * K)[:, :, 8:8 + K]
    assert slots.stride(1) == 2 * K and not slots.is_contiguous()
    per_slot = kl.mmq_id_sorted(gtype, A, it, slots, E, M, K)
    assert _same_bits(per_slot, kl.mmq_id_sorted(gtype, A, it, slots.contiguous(), E, M, K))
    assert _same_bits(per_slot, _per_expert(kl, gtype, A, E, ids, slots, M, K))
    buf = torch.full((N, S, M + 11), -7.0, dtype=torch.float16, device=dev)
    out = kl.mmq_id_sorted(gtype, A, it, x, E, M, K, out=buf[:, :, :M])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    assert _same_bits(buf[:, :, :M], shared)
    assert torch.all(buf[:, :, M:] == -7.0)
    _no_timeouts()


def test_graph_replay_follows_ids():
    """One captured call at (33, 2), replayed after `ids` was overwritten in place with other
    per-expert histograms (an expert going from many pairs to none, an out-of-range id): each
    replay equals the eager call on those ids bit for bit."""
    import kernels._lib as kl
    dev = _dev()
    fmt, E, M, K = SHAPES[2]
    gtype = kl.TYPES[fmt]
    N, S = 33, 2
    A = _w(_experts(fmt, E, M, K))
    first = _pattern(N, S, E)                      # expert 0: 65 pairs, expert 1: none, expert 2: one
    second = np.where(first == 0, 1, 0).astype(np.int32)  # expert 0: one pair, expert 1: 65, expert 2: none
    third = np.random.default_rng(3).integers(0, E, size=(N, S), dtype=np.int32)
    third[4, 1] = -1
    assert np.bincount(second.reshape(-1), minlength=E).tolist() == [1, 65, 0]
    x = torch.from_numpy(random_activations(N, K, seed=13)).to(dev)
    eager = [kl.mmq_id_sorted(gtype, A, torch.from_numpy(i).to(dev), x, E, M, K) for i in (first, second, third)]
    it = torch.from_numpy(first).to(dev)
    out = torch.empty((N, S, M), dtype=torch.float16, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kl.mmq_id_sorted(gtype, A, it, x, E, M, K, out=out)
    for ids, want in zip((first, second, third, first), eager + eager[:1]):
        it.copy_(torch.from_numpy(ids).to(dev))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out, want)
    assert not _same_bits(eager[0], eager[1])
    _no_timeouts()


def test_mmq_id_takes_the_sorted_path_beyond_64_pairs():
    """mmq_id at 80 pairs: gq_mmq_id refuses, the sorted entry runs -- the bits of mmq_id_sorted."""
    import kernels._lib as kl
    dev = _dev()
    fmt, E, M, K = SHAPES[0]
    gtype = kl.TYPES[fmt]
    N, S = 40, 2
    A = _w(_experts(fmt, E, M, K))
    ids = np.random.default_rng(9).integers(0, E, size=(N, S), dtype=np.int32)
    it = torch.from_numpy(ids).to(dev)
    x = torch.from_numpy(random_activations(N, K, seed=17)).to(dev)
    got = kl.mmq_id(gtype, A, it, x, E, M, K)
    assert _same_bits(got, kl.mmq_id_sorted(gtype, A, it, x, E, M, K))
    assert _same_bits(got, _per_expert(kl, gtype, A, E, ids, x, M, K))
    _no_timeouts()


def test_moe_ffn_captured_in_a_graph():
    """MoEFFN.forward at N = 40, S = 2 (80 pairs) on tests/test_gpu_moe.py's tiny block (E=4, hidden
    512, ffn 256; Q4_K gate / up, Q6_K down) captured in a torch.cuda.graph and replayed -- no host
    sync anywhere in the block -- equals the same torch ops on per-expert streaming-GEMM outputs,
    and follows new ids at replay."""
    import kernels._lib as kl
    from kernels.moe import GGUFExperts, MoEFFN
    dev = _dev()
    E, S, N, H, F = 4, 2, 40, 512, 256
    raw = {"ffn_gate_exps": ("q4_k", F, H, _experts("q4_k", E, F, H)),
           "ffn_up_exps": ("q4_k", F, H, np.concatenate([random_blocks("q4_k", F, H, seed=50 + e) for e in range(E)])),
           "ffn_down_exps": ("q6_k", H, F, _experts("q6_k", E, H, F))}
    parts = {n: GGUFExperts(t, _w(r), E, M, K) for n, (t, M, K, r) in raw.items()}
    ffn = MoEFFN(parts["ffn_gate_exps"], parts["ffn_up_exps"], parts["ffn_down_exps"])
    rng = np.random.default_rng(21)
    all_ids = [np.stack([rng.permutation(E)[:S] for _ in range(N)]).astype(np.int32) for _ in range(2)]
    all_ids[1][:, 0] = 3  # another histogram
    it = torch.from_numpy(all_ids[0]).to(dev)
    x = torch.from_numpy(random_activations(N, H, seed=21) / np.float16(16)).to(dev)  # (keeps silu(g) * u, d in fp16 range)
    w = torch.softmax(torch.from_numpy(random_activations(N, S, seed=23)).float(), dim=1).to(torch.float16).to(dev)
    ffn.forward(x, it, w)  # (first use outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ffn.forward(x, it, w)
    for ids in all_ids:
        it.copy_(torch.from_numpy(ids).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        assert y.shape == (N, H)
        g = _per_expert(kl, kl.GQ_Q4_K, parts["ffn_gate_exps"].A, E, ids, x, F, H)
        u = _per_expert(kl, kl.GQ_Q4_K, parts["ffn_up_exps"].A, E, ids, x, F, H)
        h = torch.nn.functional.silu(g) * u
        d = _per_expert(kl, kl.GQ_Q6_K, parts["ffn_down_exps"].A, E, ids, h, H, F)
        want = (w[..., None] * d).sum(1)
        assert torch.isfinite(want).all() and float(want.abs().max()) > 0
        assert y.dtype == want.dtype and _same_bits(y, want)
    _no_timeouts()
