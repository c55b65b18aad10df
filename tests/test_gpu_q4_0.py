"""GPU tests of GGUF Q4_0 (GGML type 2): every route -- the streaming decode (alone, grouped, on
the prepared copy, expert-indexed), the GEMV (long activations at 1..4 tokens, K % 256 != 0 at any
token count), the streaming GEMM (alone, grouped, split-K, row-chunked, sorted by expert),
dequantize + hipBLASLt, and the device quantizer.  The judge is the reference's Q8_0 oracle (IDEAL)
on the exactly widened blocks (tests/q4_0_model.py widen; pinned on the host by
tests/test_q4_0_host.py): max|C - ideal| / max|ideal| <= 1.5e-3 at N <= 4 and 4e-3 otherwise.
Q4_K / Q6_K / Q8_0 items of mixed cases use the oracle directly."""
import numpy as np
import pytest
import torch

import oracle as O
import q4_0_model as Q
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

Q40 = 6
RB = lambda K: K // 32 * 18  # noqa: E731  (row bytes)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _w(raw):
    return torch.from_numpy(np.array(raw).view(np.int8)).to(_dev())  # (a copy: the shared cases are read-only)


def _x(B):
    return torch.from_numpy(np.array(B)).to(_dev())


def run(raw, B, M, N, K):
    from kernels.mmq_q4_0 import mmq_q4_0
    C = mmq_q4_0(_w(raw), _x(B), M, N, K)
    torch.cuda.synchronize()
    assert C.shape == (N, M) and C.dtype == torch.float16
    return C.cpu().numpy()


def _no_timeouts():
    import kernels._lib as kl
    assert kl.lib().gq_debug_sync_timeouts() == 0


@pytest.fixture(autouse=True)
def _no_timeouts_after_each_test():
    yield
    _no_timeouts()


def _parity(M, N, K):
    raw, B, want = Q.case(M, N, K)
    err = Q.rel_err(run(raw, B, M, N, K), want)
    print(f"q4_0 {M}x{N}x{K}: max|d|/max|C| = {err:.2e}")
    assert err <= Q.tight(N), (M, N, K, err)
    _no_timeouts()


def _ideal(fmt, raw, B, M, N, K):
    if fmt == "q4_0":
        return Q.ideal(raw, B, M, N, K)
    return O.mmq_from_fp16(fmt, raw, B, M, N, K, O.IDEAL)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---- 1. parity, ragged shapes ----
@pytest.mark.parametrize("M,N,K", Q.DECODE_SHAPES)
def test_decode(M, N, K):
    """The streaming decode at K = 32 (one block, half a unit), rows that end with half a unit
    (K % 64 == 32) and start 2-byte aligned in the ring, the last K at four tokens, and K = 28672 at
    one token (seven cached chunks per lane, rows cut into ring segments)."""
    import kernels._lib as kl
    assert kl.route_name(Q40, M, N, K) == "stream_decode_kernel"
    _parity(M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMV_SHAPES)
def test_gemv(M, N, K):
    """act_quant + gemv_kernel: four tokens whose q8_1 image does not fit LDS beside the ring
    (K = 11008, and K = 10912, the first K over the limit), and K % 256 != 0 at GEMM token counts."""
    import kernels._lib as kl
    assert kl.route_name(Q40, M, N, K) == "gemv_kernel"
    _parity(M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMM_SHAPES + Q.SPLITK_SHAPES)
def test_gemm(M, N, K):
    import kernels._lib as kl
    assert "sgemm" in kl.route_name(Q40, M, N, K)
    _parity(M, N, K)


def test_splitk_shapes_split():
    import kernels._lib as kl
    for M, N, K in Q.SPLITK_SHAPES:
        r = kl.route_name(Q40, M, N, K)
        assert "split-K" in r or "reduce" in r, r


@pytest.mark.parametrize("N", [1, 16])
def test_edge_valued_weights(N):
    """Rows of all-0 nibbles (code -8), all-15 nibbles (+7) and blocks of each in turn: the signed
    nibbles of the decode (N = 1) and the biased pairs of the streaming GEMM (N = 16) at both ends
    of the code range."""
    import kernels._lib as kl
    M, K = 70, 512
    raw = Q.edge_blocks(M, K, seed=2)
    B = random_activations(N, K, seed=N)
    assert ("stream_decode_kernel" if N == 1 else "sgemm") in kl.route_name(Q40, M, N, K)
    err = Q.rel_err(run(raw, B, M, N, K), Q.ideal(raw, B, M, N, K))
    print(f"q4_0 edge-valued {M}x{N}x{K}: max|d|/max|C| = {err:.2e}")
    assert err <= Q.tight(N), err


# ---- 2. gq_dequantize, gq_quantize_weights ----
def test_dequantize_bit_equal():
    import kernels._lib as kl
    M, K = 37, 768
    raw = random_blocks("q4_0", M, K, seed=4)
    got = kl.dequantize_device(Q40, _w(raw), M, K)
    torch.cuda.synchronize()
    want = Q.dequant_f32(raw, M, K).astype(np.float16)
    assert np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16))


def test_quantize_weights_byte_equal_to_the_host():
    import kernels._lib as kl
    from utils.quantize.q4_0 import quantize_to_q4_0
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal((40, 32)), rng.uniform(0, 1, (23, 32)), np.zeros((1, 32))]).astype(np.float32)
    assert x.shape == (64, 32)
    got = kl.quantize_weights_device("q4_0", torch.from_numpy(x).to(_dev()))
    torch.cuda.synchronize()
    want = quantize_to_q4_0(torch.from_numpy(x))
    assert got.numel() == 64 * 18 and torch.equal(got.cpu(), want)
    assert want.view(64, 18)[63].tolist() == [0, -128] + [-120] * 16  # (the all-zero block: d = -0, every code 8)


# ---- 3. dequant + hipBLASLt ----
@pytest.mark.parametrize("M,N,K", Q.BLAS_SHAPES)
def test_blas_path(M, N, K, tune):
    import kernels._lib as kl
    tune(GQ_BLAS_MIN_TOKENS=9)
    assert "hipBLASLt" in kl.route_name(Q40, M, N, K)
    _parity(M, N, K)


# ---- 4. routes ----
def test_routes(tune):
    import kernels._lib as kl
    assert "stream_decode_kernel" in kl.route_name(Q40, 4096, 1, 4096)
    assert "stream_decode_kernel" in kl.route_name(Q40, 4096, 1, 4096, prepared=True)
    assert "stream_decode_kernel" in kl.route_name(Q40, 4096, 4, 4096)
    assert kl.route_name(Q40, 4096, 4, 11008) == "gemv_kernel"
    assert kl.route_name(Q40, 4096, 16, 4096 + 32) == "gemv_kernel"
    for M, N in ((4096, 5), (4096, 16), (4096, 128), (11008, 16), (11008, 128), (4096, 767)):
        for prepared in (False, True):
            assert "sgemm" in kl.route_name(Q40, M, N, 4096, prepared=prepared), (M, N, prepared)
    assert "hipBLASLt" in kl.route_name(Q40, 4096, 768, 4096)
    assert kl.route_name(Q40, 4096, 16, 4096, act="fp8") == "none"
    assert kl.route_name(Q40, 4096, 16, 4000) == "gemv_kernel"  # (125 blocks: a valid K)
    assert kl.route_name(Q40, 4096, 16, 4016) == "none"


@pytest.mark.parametrize("knob", ["GQ_RGEMM", "GQ_SKINNY", "GQ_KSTREAM", "GQ_GEMM_SPLITS", "GQ_SGEMM"])
def test_forced_routes_keep_sgemm(knob, tune):
    """Q4_0 has no resident, K-chunked, skinny or LDS-DMA GEMM form: a knob that forces one (or
    turns the streaming GEMM off for the other types) leaves it on the streaming GEMM."""
    import kernels._lib as kl
    tune(**{knob: 4 if knob == "GQ_GEMM_SPLITS" else (0 if knob == "GQ_SGEMM" else 1)})
    for M, N in ((4096, 16), (4096, 128), (11008, 16), (70, 16)):
        for prepared in (False, True):
            assert "sgemm" in kl.route_name(Q40, M, N, 4096 if M > 70 else 512, prepared=prepared), (knob, M, N)
    _parity(70, 16, 512)


def test_row_chunks_under_the_launch_limit(tune):
    """A call over the per-launch byte limit (lowered here) is cut into row chunks, each on the
    streaming GEMM: the bits of the one-launch call (rows are independent; splits pinned).
    512 rows of 288 bytes per launch (512 + 88); the limit holds one whole 128-token tile of x~, so
    the 24 tokens go into every launch."""
    import kernels._lib as kl
    M, N, K = 600, 24, 512
    raw, B = random_blocks("q4_0", M, K, seed=8), random_activations(N, K, seed=9)
    tune(GQ_SGEMM_SPLITS=1)
    whole = run(raw, B, M, N, K)
    tune(GQ_GEMM_MAX_BYTES=147600)  # (512 rows of 288 bytes = 147456 per launch)
    assert kl.lib().gq_mmq_call_workspace_size(Q40, 0, M, N, K) > 0
    assert "sgemm" in kl.route_name(Q40, M, N, K)
    assert np.array_equal(run(raw, B, M, N, K).view(np.uint16), whole.view(np.uint16))
    assert Q.rel_err(whole, Q.ideal(raw, B, M, N, K)) <= Q.TIGHT_GEMM


# ---- 5. invariants ----
@pytest.mark.parametrize("N,K", [(2, 736), (24, 768), (24, 736)])
def test_activation_scaling_is_exact(N, K):
    M = 70
    raw, B = random_blocks("q4_0", M, K, seed=N), random_activations(N, K, seed=N + 1)
    a, b = run(raw, B, M, N, K), run(raw, (B * np.float16(2)).astype(np.float16), M, N, K)
    assert np.array_equal((a * np.float16(2)).view(np.uint16), b.view(np.uint16))


@pytest.mark.parametrize("N,K", [(3, 736), (24, 768), (24, 736)])
def test_row_independence(N, K, tune):
    if N > 4:
        tune(GQ_SGEMM_SPLITS=1)
    M, r0, r1 = 300, 101, 290
    raw, B = random_blocks("q4_0", M, K, seed=N), random_activations(N, K, seed=N + 1)
    rb = RB(K)
    full = run(raw, B, M, N, K)
    sub = run(raw[r0 * rb:r1 * rb], B, r1 - r0, N, K)
    assert np.array_equal(sub.view(np.uint16), full[:, r0:r1].view(np.uint16))


# ---- 6. prepared form ----
@pytest.mark.parametrize("N,K", [(2, 1024), (3, 160), (24, 1024)])
def test_prepared(N, K):
    import kernels._lib as kl
    M = 130
    raw, B = random_blocks("q4_0", M, K, seed=N), random_activations(N, K, seed=N + 1)
    ws = torch.empty(kl.workspace_size(Q40, M, N, K), dtype=torch.uint8, device=_dev())
    kl.act_prepare(_x(B), N, K, ws)
    got = kl.mmq_prepared(Q40, _w(raw), ws, M, N, K)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    if N <= 4:
        assert "stream_decode_kernel" in kl.route_name(Q40, M, N, K, prepared=True)
        assert np.array_equal(got.view(np.uint16), run(raw, B, M, N, K).view(np.uint16))
    assert Q.rel_err(got, Q.ideal(raw, B, M, N, K)) <= Q.tight(N)
    _no_timeouts()


# ---- 7. grouped decode ----
_GROUP = (("q4_0", 96, 512), ("q4_0", 64, 160), ("q4_k", 96, 512), ("q6_k", 64, 768), ("q8_0", 64, 160))


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_grouped_decode_bit_identical(N):
    import kernels._lib as kl
    raws = [random_blocks(f, M, K, seed=10 + i) for i, (f, M, K) in enumerate(_GROUP)]
    Bs = {K: random_activations(N, K, seed=N + K) for K in (160, 512, 768)}
    items = [(kl.TYPES[f], _w(r), _x(Bs[K]), M, K, None) for (f, M, K), r in zip(_GROUP, raws)]
    outs = kl.mmq_grouped(items, N)
    assert outs is not None, kl.lib().gq_last_error()
    torch.cuda.synchronize()
    for (f, M, K), r, it, C in zip(_GROUP, raws, items, outs):
        solo = kl.mmq(it[0], it[1], it[2], M, N, K)
        torch.cuda.synchronize()
        assert torch.equal(C.view(torch.int16), solo.view(torch.int16)), (f, M, K)
        assert Q.rel_err(C.cpu().numpy(), _ideal(f, r, Bs[K], M, N, K)) <= Q.TIGHT_GEMV, (f, M, K)
    _no_timeouts()


@pytest.mark.parametrize("other", ["q2_k", "q3_k", "q5_k"])
def test_grouped_with_another_q8_1_only_type_is_refused(other):
    """No grouped decode kernel carries Q4_0's cases beside Q5_K's, Q3_K's or Q2_K's: nothing is
    launched and the caller runs the items alone."""
    import kernels._lib as kl
    N = 2
    group = (("q4_0", 96, 512), (other, 64, 768))
    items = [(kl.TYPES[f], _w(random_blocks(f, M, K, seed=i)), _x(random_activations(N, K, seed=i)), M, K, None)
             for i, (f, M, K) in enumerate(group)]
    assert kl.mmq_grouped(items, N) is None


def test_grouped_one_token_cached_chunk_cap():
    """The grouped kernel that holds a Q4_0 item carries every format to five cached chunks at one
    token (K <= 20480; with more cases it spills): a launch at the cap gives the solo bits, one
    beyond it is refused and nothing is launched."""
    import kernels._lib as kl
    N = 1
    for K, ok in ((20480, True), (24576, False)):
        group = (("q4_0", 8, K), ("q8_0", 8, 512))
        raws = [random_blocks(f, M, k, seed=40 + i) for i, (f, M, k) in enumerate(group)]
        Bs = [random_activations(N, k, seed=k) for _, _, k in group]
        items = [(kl.TYPES[f], _w(r), _x(B), M, k, None) for (f, M, k), r, B in zip(group, raws, Bs)]
        assert "stream_decode_kernel" in kl.route_name(Q40, 8, N, K)
        outs = kl.mmq_grouped(items, N)
        if not ok:
            assert outs is None
            continue
        assert outs is not None, kl.lib().gq_last_error()
        torch.cuda.synchronize()
        for (f, M, k), r, B, it, C in zip(group, raws, Bs, items, outs):
            solo = kl.mmq(it[0], it[1], it[2], M, N, k)
            torch.cuda.synchronize()
            assert torch.equal(C.view(torch.int16), solo.view(torch.int16)), (f, M, k)
            assert Q.rel_err(C.cpu().numpy(), _ideal(f, r, B, M, N, k)) <= Q.TIGHT_GEMV, (f, M, k)


def test_grouped_at_gemm_tokens_is_refused():
    import kernels._lib as kl
    N = 8
    items = [(kl.TYPES[f], _w(random_blocks(f, M, K, seed=i)), _x(random_activations(N, K, seed=i)), M, K, None)
             for i, (f, M, K) in enumerate(_GROUP)]
    assert kl.mmq_grouped(items, N) is None
    assert b"Q4_0" in kl.lib().gq_last_error()


# ---- 8. grouped prepared (the streaming GEMM) ----
@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("splits", [1, 2])
def test_grouped_prepared_bit_identical(N, splits, tune):
    import kernels._lib as kl
    tune(GQ_KSTREAM=0, GQ_SGEMM_SPLITS=splits)
    group = (("q4_0", 300, 512), ("q6_k", 64, 768), ("q8_0", 64, 768), ("q4_0", 96, 512), ("q4_k", 64, 512))
    raws = [random_blocks(f, M, K, seed=20 + i) for i, (f, M, K) in enumerate(group)]
    Bs = {K: random_activations(N, K, seed=N + K) for K in (512, 768)}
    wss = {}
    for K, B in Bs.items():
        wss[K] = torch.empty(kl.workspace_size(Q40, 300, N, K), dtype=torch.uint8, device=_dev())
        kl.act_prepare(_x(B), N, K, wss[K])
    items = [(kl.TYPES[f], _w(r), wss[K], M, K, None) for (f, M, K), r in zip(group, raws)]
    outs = kl.mmq_grouped_prepared(items, N)
    assert outs is not None, kl.lib().gq_last_error()
    torch.cuda.synchronize()
    tune(GQ_SGEMM=1, GQ_RGEMM=0, GQ_SKINNY=0)  # (the other types' per-matrix call on the streaming GEMM too)
    for (f, M, K), r, it, C in zip(group, raws, items, outs):
        ws = torch.empty(kl.workspace_size(it[0], M, N, K), dtype=torch.uint8, device=_dev())
        kl.act_prepare(_x(Bs[K]), N, K, ws)
        assert "sgemm" in kl.route_name(it[0], M, N, K, prepared=True)
        solo = kl.mmq_prepared(it[0], it[1], ws, M, N, K)
        torch.cuda.synchronize()
        assert torch.equal(C.view(torch.int16), solo.view(torch.int16)), (f, M, K)
        assert Q.rel_err(C.cpu().numpy(), _ideal(f, r, Bs[K], M, N, K)) <= Q.TIGHT_GEMM, (f, M, K)
    _no_timeouts()


# ---- 9. MoE ----
def _experts(fmt, E, M, K, seed=0):
    return np.concatenate([random_blocks(fmt, M, K, seed=3000 * E + 10 * M + e + seed) for e in range(E)])


def test_mmq_id_bit_identical_to_one_token_calls():
    """gq_mmq_id on Q4_0 experts at K = 160 (K % 64 == 32: rows end with half a unit): every pair
    the bits of its own one-token gq_mmq; an id out of range gives zeros."""
    import kernels._lib as kl
    E, M, K, N, S = 4, 70, 160, 3, 2
    raw = _experts("q4_0", E, M, K)
    A = _w(raw)
    ids = np.array([[0, 3], [3, 7], [2, 0]], dtype=np.int32)  # (7: out of range)
    x = random_activations(N, K, seed=K + N)
    xt, it, out = _x(x), torch.from_numpy(ids).to(_dev()), torch.empty((N, S, M), dtype=torch.float16, device=_dev())
    rc = kl.lib().gq_mmq_id(Q40, A.data_ptr(), it.data_ptr(), xt.data_ptr(), out.data_ptr(), E, M, N, S, K, K, 0, M, None)
    assert rc == 0, kl.lib().gq_last_error()
    torch.cuda.synchronize()
    assert _same_bits(out, kl.mmq_id(Q40, A, it, xt, E, M, K))
    per = M * RB(K)
    for n in range(N):
        for s in range(S):
            e = int(ids[n, s])
            if not 0 <= e < E:
                assert not out[n, s].any()
                continue
            solo = kl.mmq(Q40, A[e * per:(e + 1) * per], xt[n:n + 1].contiguous(), M, 1, K)
            assert torch.equal(out[n, s], solo[0]), (n, s)
            err = Q.rel_err(out[n, s].cpu().numpy()[None], Q.ideal(raw[e * per:(e + 1) * per], x[n:n + 1], M, 1, K))
            assert err <= Q.TIGHT_GEMV, (n, s, err)
    _no_timeouts()


_PINS = dict(GQ_SGEMM=1, GQ_SGEMM_SPLITS=1, GQ_SKINNY=0, GQ_RGEMM=0, GQ_KSTREAM=0)


def _by_expert(ids, E):
    flat = ids.reshape(-1)
    return {e: np.nonzero(flat == e)[0].tolist() for e in range(E) if (flat == e).any()}


@pytest.mark.parametrize("M", [70, 300])
def test_mmq_id_sorted_80_pairs(M):
    """gq_mmq_id_sorted at 80 pairs: every pair's row the bits of the one-split streaming GEMM on
    its expert's gathered rows, and within the gate of the oracle."""
    import kernels._lib as kl
    E, K, N, S = 4, 512, 40, 2
    raw = _experts("q4_0", E, M, K)
    A = _w(raw)
    ids = np.random.default_rng(M).integers(0, E, size=(N, S), dtype=np.int32)
    ids[5, 1] = E + 2  # (an id out of range: a zero row)
    x = random_activations(N, K, seed=K + N + S)
    xt, it = _x(x), torch.from_numpy(ids).to(_dev())
    got = kl.mmq_id_sorted(Q40, A, it, xt, E, M, K)
    torch.cuda.synchronize()
    assert got.shape == (N, S, M)
    g = got.reshape(N * S, M)
    per = M * RB(K)
    assert not g[5 * S + 1].any()
    for e, pairs in _by_expert(ids, E).items():
        idx = torch.tensor(pairs, dtype=torch.int64, device=_dev())
        rows = xt.index_select(0, idx // S).contiguous()
        n = len(pairs)
        assert n >= 5
        with kl.tuning(**_PINS):
            assert kl.route_name(Q40, M, n, K) == "sgemm_kernel"
            want = kl.mmq(Q40, A[e * per:(e + 1) * per], rows, M, n, K)
        torch.cuda.synchronize()
        assert _same_bits(g.index_select(0, idx), want), e
        err = Q.rel_err(want.cpu().numpy(), Q.ideal(raw[e * per:(e + 1) * per], x[[p // S for p in pairs]], M, n, K))
        print(f"q4_0 sorted E={E} {M}x{K} expert {e}: {n} pairs, max|d|/max|C| = {err:.2e}")
        assert err <= Q.TIGHT_GEMM, (e, err)
    _no_timeouts()


# ---- 10. from written GGUF files ----
@pytest.mark.parametrize("N", [1, 3, 8, 40])
def test_moe_ffn_from_gguf(tmp_path, N):
    """MoEFFN.from_gguf on a written 3-D Q4_0 file (E=4, S=2, hidden 512, ffn 256) at 2, 6 and 16
    pairs (gq_mmq_id) and 80 (the sorted GEMM), stage by stage against the oracle: the gate and up
    rows on x, the down rows on the fp16 silu(g) * u the block feeds them, each at the gate of its
    pair count; the block's output the bits of the same torch ops on those stage outputs."""
    from gguf.file import read_gguf, write_gguf
    from kernels.moe import MoEFFN
    dev = _dev()
    E, S, H, F = 4, 2, 512, 256
    raw = {"ffn_gate_exps": (F, H, _experts("q4_0", E, F, H, 1)), "ffn_up_exps": (F, H, _experts("q4_0", E, F, H, 2)),
           "ffn_down_exps": (H, F, _experts("q4_0", E, H, F, 3))}
    path = str(tmp_path / "moe.gguf")
    write_gguf(path, {f"blk.2.{n}.weight": ("q4_0", (E, M, K), r) for n, (M, K, r) in raw.items()})
    _, tensors = read_gguf(path)
    ffn = MoEFFN.from_gguf(tensors, 2, dev)
    assert (ffn.gate.type_name, ffn.up.type_name, ffn.down.type_name) == ("q4_0", "q4_0", "q4_0")
    assert (ffn.gate.E, ffn.gate.M, ffn.gate.K) == (E, F, H)
    ids = np.random.default_rng(N).integers(0, E, size=(N, S), dtype=np.int32)
    it = torch.from_numpy(ids).to(dev)
    xn = (random_activations(N, H, seed=21) / np.float16(16)).astype(np.float16)  # (keeps silu(g) * u, d in fp16 range)
    x = torch.from_numpy(xn).to(dev)
    w = torch.softmax(torch.from_numpy(random_activations(N, S, seed=23)).float(), dim=1).to(torch.float16).to(dev)
    y = ffn.forward(x, it, w)
    torch.cuda.synchronize()
    assert y.shape == (N, H)
    g, u = ffn.gate(x, it), ffn.up(x, it)
    h = torch.nn.functional.silu(g) * u
    d = ffn.down(h, it)
    torch.cuda.synchronize()
    assert _same_bits(y, (w[..., None] * d).sum(1))
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0
    gate = Q.TIGHT_GEMV if N * S <= 64 else Q.TIGHT_GEMM  # (gq_mmq_id's one-token decode / the sorted GEMM)
    gn, un, hn, dn = (t.cpu().numpy().reshape(N * S, -1) for t in (g, u, h, d))
    for e, pairs in _by_expert(ids, E).items():
        toks = [p // S for p in pairs]
        for name, got in (("ffn_gate_exps", gn), ("ffn_up_exps", un)):
            r = raw[name][2][e * F * RB(H):(e + 1) * F * RB(H)]
            err = Q.rel_err(got[pairs], Q.ideal(r, xn[toks], F, len(pairs), H))
            assert err <= gate, (name, e, err)
        r = raw["ffn_down_exps"][2][e * H * RB(F):(e + 1) * H * RB(F)]
        err = Q.rel_err(dn[pairs], Q.ideal(r, np.ascontiguousarray(hn[pairs]), H, len(pairs), F))
        assert err <= gate, ("ffn_down_exps", e, err)
    _no_timeouts()


@pytest.mark.parametrize("fuse", [True, False])
def test_layer_mix_from_gguf(tmp_path, fuse):
    from gguf import q4_0_layer_types, read_gguf, write_gguf
    from kernels.layer_mix import LayerMix
    types = q4_0_layer_types(0, 32)
    assert set(types.values()) == {"q4_0"}
    shapes = {n: (96, 512) for g in LayerMix.GROUPS[:3] for n in g}
    shapes["ffn_down"] = (64, 768)
    raw = {n: random_blocks(types[n], *shapes[n], seed=i) for i, n in enumerate(shapes)}
    p = tmp_path / "l.gguf"
    write_gguf(p, {f"blk.0.{n}.weight": (types[n], shapes[n], raw[n]) for n in shapes})
    _, tens = read_gguf(p)
    assert tens["blk.0.attn_q.weight"].type_name == "q4_0"
    layer = LayerMix.from_gguf(tens, 0, device=_dev(), fuse=fuse)
    for N in (1, 3, 8, 40):
        x, a, y = (random_activations(N, 512, seed=N + 10 * i) for i in range(3))
        h = random_activations(N, 768, seed=N + 1)
        d = {k: _x(v) for k, v in (("x", x), ("a", a), ("y", y), ("h", h))}
        out = layer.forward(d["x"], d["h"], attn=d["a"], x_ffn=d["y"])
        torch.cuda.synchronize()
        src = {"attn_q": x, "attn_k": x, "attn_v": x, "attn_output": a, "ffn_gate": y, "ffn_up": y, "ffn_down": h}
        for n, (M, K) in shapes.items():
            want = _ideal(types[n], raw[n], src[n], M, N, K)
            assert Q.rel_err(out[n].cpu().numpy(), want) <= Q.tight(N), (n, N)
    _no_timeouts()
