"""GPU tests of the expert-indexed MMQ (gq_mmq_id, csrc/mmq_decode.hip stream_decode_id_kernel:
llama.cpp's mul_mat_id at decode) and the mixture-of-experts FFN block on it (kernels/moe.py).
Every (token, slot) pair's row bit for bit against a one-token mmq() on that expert's slice and
that activation row, sampled rows against the oracle at tests/test_gpu_grouped.py's decode gates
(Q5_K: tests/q5k_model.py at tests/test_gpu_q5k.py's); shared and per-slot activations, strides;
ids outside [0, E); a captured graph replayed over new ids; refused shapes and the host-sorted
fallback; MoEFFN against the same torch ops on per-pair mmq() outputs."""
import functools

import numpy as np
import pytest
import torch

import oracle as O
import type_models as TM
from gpu_types import dev as _dev, no_timeouts as _no_timeouts, same_bits as _same_bits, to_w as _w
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

TIGHT_DEC = 3e-3  # int8 x int8 dots, fp32 block scaling: vs IDEAL (tests/test_gpu_grouped.py)
TIGHT_GEMM = 4e-3  # the GEMM paths (the host-sorted fallback runs mmq() at n_e tokens)

# (type, E, M, K): one per geometry of the decode body
CASES = [("q4_k", 4, 200, 1024),
         ("q4_k", 3, 96, 14336),   # segmented rows
         ("q5_k", 4, 130, 2048),
         ("q6_k", 4, 257, 1536),   # ring image
         ("q6_k", 3, 64, 9216),    # packed, segmented
         ("q8_0", 5, 333, 1056),   # K not a multiple of 64
         ("q8_0", 3, 96, 7168)]    # segmented
PAIRS = [(1, 1), (1, 8), (4, 2), (8, 8)]


@functools.lru_cache(maxsize=None)
def _experts(fmt, E, M, K):
    """E packed matrices back to back (exactly E experts: nothing to read past them), read-only."""
    raw = np.concatenate([random_blocks(fmt, M, K, seed=1000 * E + 10 * M + e) for e in range(E)])
    raw.setflags(write=False)
    return raw


def _ids(N, S, E, seed=0):
    """(N, S) int32 choices that repeat an expert across tokens (and, when S > E, within one)."""
    rng = np.random.default_rng(seed + 97 * N + S)
    ids = rng.integers(0, E, size=(N, S), dtype=np.int32)
    ids[:, 0] = ids[0, 0]  # every token's first slot: the same expert
    return ids


def _solo(kl, gtype, A, E, ids, rows, M, K):
    """(N, S, M): one one-token mmq() per pair on its expert's slice and its activation row
    (rows: (N, K) shared or (N, S, K) per slot); zeros for ids outside [0, E)."""
    N, S = ids.shape
    per = A.numel() // E
    want = torch.zeros((N, S, M), dtype=torch.float16, device=A.device)
    for n in range(N):
        for s in range(S):
            e = int(ids[n, s])
            if 0 <= e < E:
                x = (rows[n, s] if rows.dim() == 3 else rows[n]).reshape(1, K).contiguous()
                want[n, s] = kl.mmq(gtype, A[e * per:(e + 1) * per], x, M, 1, K)[0]
    return want


@pytest.mark.parametrize("N,S", PAIRS)
@pytest.mark.parametrize("fmt,E,M,K", CASES)
def test_id_bit_identical_and_oracle(fmt, E, M, K, N, S):
    import kernels._lib as kl
    gtype = kl.TYPES[fmt]
    raw = _experts(fmt, E, M, K)
    A = _w(raw)
    ids = _ids(N, S, E)
    x = random_activations(N, K, seed=K + N)
    xt, it = torch.from_numpy(x).to(_dev()), torch.from_numpy(ids).to(_dev())
    got = kl.mmq_id(gtype, A, it, xt, E, M, K)
    torch.cuda.synchronize()
    assert got.shape == (N, S, M) and got.dtype == torch.float16
    assert _same_bits(got, _solo(kl, gtype, A, E, ids, xt, M, K))
    # sampled weight rows of sampled pairs against the oracle
    rng = np.random.default_rng(N * S + M)
    per, rb = raw.size // E, raw.size // E // M
    g = got.cpu().numpy()
    for p in sorted(set(rng.choice(N * S, size=min(3, N * S), replace=False).tolist())):
        n, s = divmod(p, S)
        e = int(ids[n, s])
        rows = np.sort(rng.choice(M, size=24, replace=False))
        sub = np.concatenate([raw[e * per + r * rb:e * per + (r + 1) * rb] for r in rows])
        B = x[n:n + 1]
        if fmt == "q5_k":
            err = TM.rel_err(g[n, s][None, rows], TM.judge(fmt, sub, B, len(rows), 1, K))
            print(f"{fmt} E={E} {M}x{K} pair ({n},{s}) expert {e}: max|d|/max|C| = {err:.2e}")
            assert err <= TM.TIGHT_GEMV, (p, err)
            continue
        ideal = O.mmq_from_fp16(fmt, sub, B, len(rows), 1, K, O.IDEAL)
        err = O.max_rel_err(g[n, s][None, rows], ideal)
        print(f"{fmt} E={E} {M}x{K} pair ({n},{s}) expert {e}: max|d|/max|C| = {err:.2e}")
        assert err <= TIGHT_DEC, (p, err)
        exact = O.mmq_from_fp16(fmt, sub, B, len(rows), 1, K, O.EXACT)
        assert O.allclose(exact, g[n, s][None, rows], 0.01), p
    _no_timeouts()


def test_shared_vs_per_slot_rows_and_strides():
    """ldb_slot = 0 (the slots share the token's row) equals a materialised (N, S, K) copy of the
    same rows; a strided B view (rows 2K apart; per slot: slots 2K apart) gives the same bits; and
    ldc > M into a sentinel-filled buffer changes nothing outside the written ranges."""
    import kernels._lib as kl
    dev = _dev()
    fmt, E, M, K, N, S = "q4_k", 4, 200, 1024, 4, 2
    A = _w(_experts(fmt, E, M, K))
    ids = _ids(N, S, E, seed=3)
    it = torch.from_numpy(ids).to(dev)
    x = torch.from_numpy(random_activations(N, K, seed=5)).to(dev)
    shared = kl.mmq_id(kl.GQ_Q4_K, A, it, x, E, M, K)
    copy = x[:, None, :].expand(N, S, K).contiguous()
    assert _same_bits(kl.mmq_id(kl.GQ_Q4_K, A, it, copy, E, M, K), shared)
    wide = torch.from_numpy(random_activations(N, 2 * K, seed=6)).to(dev)
    view = wide[:, 300:300 + K]  # row stride 2K, 600 bytes off the row start
    assert view.stride(0) == 2 * K
    assert _same_bits(kl.mmq_id(kl.GQ_Q4_K, A, it, view, E, M, K), _solo(kl, kl.GQ_Q4_K, A, E, ids, view, M, K))
    # distinct rows per slot, as a strided (N, S, K) view
    slots = torch.from_numpy(random_activations(N * S, 2 * K, seed=7)).to(dev).view(N, S, 2 * K)[:, :, 8:8 + K]
    assert slots.stride(1) == 2 * K and not slots.is_contiguous()
    assert _same_bits(kl.mmq_id(kl.GQ_Q4_K, A, it, slots, E, M, K), _solo(kl, kl.GQ_Q4_K, A, E, ids, slots, M, K))
    # ldc > M
    buf = torch.full((N, S, M + 11), -7.0, dtype=torch.float16, device=dev)
    out = kl.mmq_id(kl.GQ_Q4_K, A, it, x, E, M, K, out=buf[:, :, :M])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    assert _same_bits(buf[:, :, :M], shared)
    assert torch.all(buf[:, :, M:] == -7.0)
    _no_timeouts()


@pytest.mark.parametrize("fmt,E,M,K", [CASES[0], CASES[3], CASES[6]])
def test_invalid_ids_give_zero_rows(fmt, E, M, K):
    """Pairs whose id is -1 or E: all-zero rows (written: the buffer starts as NaN), their
    neighbours unaffected.  A holds exactly E experts."""
    import kernels._lib as kl
    dev = _dev()
    gtype = kl.TYPES[fmt]
    A = _w(_experts(fmt, E, M, K))
    N, S = 4, 2
    ids = _ids(N, S, E, seed=9)
    ids[0, 1], ids[2, 0], ids[3, 1] = -1, E, E + 1000
    x = torch.from_numpy(random_activations(N, K, seed=11)).to(dev)
    out = torch.full((N, S, M), float("nan"), dtype=torch.float16, device=dev)
    kl.mmq_id(gtype, A, torch.from_numpy(ids).to(dev), x, E, M, K, out=out)
    torch.cuda.synchronize()
    for n, s in ((0, 1), (2, 0), (3, 1)):
        assert torch.all(out[n, s].view(torch.int16) == 0), (n, s)
    assert _same_bits(out, _solo(kl, gtype, A, E, ids, x, M, K))
    _no_timeouts()


def test_graph_capture_follows_ids():
    """One captured mmq_id call, replayed after `ids` was overwritten in place: the replay
    computes the new selection (the kernel reads the ids, the host never did)."""
    import kernels._lib as kl
    dev = _dev()
    fmt, E, M, K, N, S = "q6_k", 4, 257, 1536, 4, 2
    A = _w(_experts(fmt, E, M, K))
    first, second = _ids(N, S, E, seed=1), (_ids(N, S, E, seed=2) + 1) % E
    second[1, 1] = -1
    assert not np.array_equal(first, second)
    it = torch.from_numpy(first).to(dev)
    x = torch.from_numpy(random_activations(N, K, seed=13)).to(dev)
    out = torch.empty((N, S, M), dtype=torch.float16, device=dev)
    kl.mmq_id(kl.GQ_Q6_K, A, it, x, E, M, K, out=out)  # (first use outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kl.mmq_id(kl.GQ_Q6_K, A, it, x, E, M, K, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out, _solo(kl, kl.GQ_Q6_K, A, E, first, x, M, K))
    it.copy_(torch.from_numpy(second).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out, _solo(kl, kl.GQ_Q6_K, A, E, second, x, M, K))
    _no_timeouts()


def test_refused_shape_and_host_sorted_fallback():
    """65 pairs through the C entry: GQ_EUNSUPPORTED, the output untouched.  80 pairs through
    mmq_id: the host-sorted fallback (one mmq() per expert over its pairs' rows, here 20 tokens
    each: a GEMM path), at the GEMM gates against the oracle; out-of-range pairs give zero rows."""
    import kernels._lib as kl
    dev = _dev()
    fmt, E, M, K = "q4_k", 4, 128, 1024
    raw = _experts(fmt, E, M, K)
    A = _w(raw)
    N, S = 65, 1
    it = torch.zeros((N, S), dtype=torch.int32, device=dev)
    x = torch.from_numpy(random_activations(N, K, seed=15)).to(dev)
    out = torch.full((N, S, M), 3.0, dtype=torch.float16, device=dev)
    rc = kl.lib().gq_mmq_id(kl.GQ_Q4_K, A.data_ptr(), it.data_ptr(), x.data_ptr(), out.data_ptr(), E, M, N, S, K, K, 0, M,
                            None)
    torch.cuda.synchronize()
    assert rc == kl.GQ_EUNSUPPORTED
    assert torch.all(out == 3.0)
    N, S = 40, 2
    ids = np.stack([np.arange(N) % E, (np.arange(N) + 1 + np.arange(N) // E) % E], axis=1).astype(np.int32)
    ids[5, 1], ids[17, 0] = -1, E
    x = random_activations(N, K, seed=17)
    h = random_activations(N * S, K, seed=19).reshape(N, S, K)
    per = raw.size // E
    for B in (x, h):
        got = kl.mmq_id(kl.GQ_Q4_K, A, torch.from_numpy(ids).to(dev), torch.from_numpy(B).to(dev), E, M, K)
        torch.cuda.synchronize()
        g = got.cpu().numpy()
        assert g.shape == (N, S, M)
        assert not g[5, 1].any() and not g[17, 0].any()
        for e in range(E):
            pairs = [(n, s) for n in range(N) for s in range(S) if ids[n, s] == e]
            rows = np.stack([B[n, s] if B.ndim == 3 else B[n] for n, s in pairs])
            sub = raw[e * per:(e + 1) * per]
            sel = np.stack([g[n, s] for n, s in pairs])
            ideal = O.mmq_from_fp16(fmt, sub, rows, M, len(pairs), K, O.IDEAL)
            err = O.max_rel_err(sel, ideal)
            print(f"fallback expert {e}: {len(pairs)} pairs, max|d|/max|C| = {err:.2e}")
            assert err <= TIGHT_GEMM, (e, err)
            assert O.allclose(O.mmq_from_fp16(fmt, sub, rows, M, len(pairs), K, O.EXACT), sel, 0.01), e
    _no_timeouts()


def test_moe_ffn_forward_and_from_gguf(tmp_path):
    """MoEFFN on a tiny block (E=4, S=2, N=3, hidden 512, ffn 256; Q4_K gate / up, Q6_K down): bit
    for bit the same torch ops applied to per-pair one-token mmq() outputs; the block read back
    from a GGUF file with 3-D expert tensors gives the same result."""
    import kernels._lib as kl
    from gguf.file import read_gguf, write_gguf
    from kernels.moe import GGUFExperts, MoEFFN
    dev = _dev()
    E, S, N, H, F = 4, 2, 3, 512, 256
    raw = {"ffn_gate_exps": ("q4_k", F, H, _experts("q4_k", E, F, H)),
           "ffn_up_exps": ("q4_k", F, H, np.concatenate([random_blocks("q4_k", F, H, seed=50 + e) for e in range(E)])),
           "ffn_down_exps": ("q6_k", H, F, _experts("q6_k", E, H, F))}
    parts = {n: GGUFExperts(t, _w(r), E, M, K) for n, (t, M, K, r) in raw.items()}
    ffn = MoEFFN(parts["ffn_gate_exps"], parts["ffn_up_exps"], parts["ffn_down_exps"])
    ids = np.array([[0, 3], [3, 1], [2, 0]], dtype=np.int32)
    it = torch.from_numpy(ids).to(dev)
    x = torch.from_numpy(random_activations(N, H, seed=21) / np.float16(16)).to(dev)  # (keeps silu(g) * u, d in fp16 range)
    w = torch.softmax(torch.from_numpy(random_activations(N, S, seed=23)).float(), dim=1).to(torch.float16).to(dev)
    y = ffn.forward(x, it, w)
    torch.cuda.synchronize()
    assert y.shape == (N, H)
    g = _solo(kl, kl.GQ_Q4_K, parts["ffn_gate_exps"].A, E, ids, x, F, H)
    u = _solo(kl, kl.GQ_Q4_K, parts["ffn_up_exps"].A, E, ids, x, F, H)
    h = torch.nn.functional.silu(g) * u
    d = _solo(kl, kl.GQ_Q6_K, parts["ffn_down_exps"].A, E, ids, h, H, F)
    want = (w[..., None] * d).sum(1)
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert y.dtype == want.dtype and _same_bits(y, want)
    path = str(tmp_path / "moe.gguf")
    write_gguf(path, {f"blk.2.{n}.weight": (t, (E, M, K), r) for n, (t, M, K, r) in raw.items()})
    _, tensors = read_gguf(path)
    loaded = MoEFFN.from_gguf(tensors, 2, dev)
    assert (loaded.gate.E, loaded.gate.M, loaded.gate.K, loaded.down.type_name) == (E, F, H, "q6_k")
    assert _same_bits(loaded.forward(x, it, w), y)
    _no_timeouts()
