"""GPU tests of GGUF Q2_K (GGML type 10): every route -- the streaming decode (alone, grouped, on
the prepared copy, expert-indexed), the GEMV fallback, the streaming GEMM (alone, grouped,
split-K, row-chunked, sorted by expert), dequantize + hipBLASLt.  The judge is the fp64 ideal of
tests/q2k_model.py on the oracle's q8_1 blocks (tied to the reference's Q6_K oracle on the host,
tests/test_q2k_host.py): max|C - ideal| / max|ideal| <= 1.5e-3 at N <= 4 and 4e-3 otherwise.
Q4_K / Q6_K items of mixed cases use the oracle directly, Q5_K and Q3_K items their own models."""
import numpy as np
import pytest
import torch

import oracle as O
import q2k_model as Q
import q3k_model as Q3M
import q5k_model as Q5M
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

Q2 = 5
RB = lambda K: K // 256 * 84  # noqa: E731  (row bytes)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _w(raw):
    return torch.from_numpy(np.array(raw).view(np.int8)).to(_dev())  # (a copy: the shared cases are read-only)


def _x(B):
    return torch.from_numpy(np.array(B)).to(_dev())


def run(raw, B, M, N, K):
    from kernels.mmq_q2_k import mmq_q2_k
    C = mmq_q2_k(_w(raw), _x(B), M, N, K)
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
    print(f"q2_k {M}x{N}x{K}: max|d|/max|C| = {err:.2e}")
    assert err <= Q.tight(N), (M, N, K, err)
    _no_timeouts()


def _ideal(fmt, raw, B, M, N, K):
    if fmt == "q2_k":
        return Q.ideal(raw, B, M, N, K)
    if fmt == "q3_k":
        return Q3M.oracle_ideal(raw, B, M, N, K)
    if fmt == "q5_k":
        return Q5M.ideal(raw, B, M, N, K)
    return O.mmq_from_fp16(fmt, raw, B, M, N, K, O.IDEAL)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---- 1. parity, ragged shapes ----
@pytest.mark.parametrize("M,N,K", Q.DECODE_SHAPES)
def test_decode(M, N, K):
    import kernels._lib as kl
    assert "stream_decode_kernel" in kl.route_name(Q2, M, N, K)
    _parity(M, N, K)


@pytest.mark.parametrize("M,N,K", Q.LONG_SHAPES)
def test_long_rows(M, N, K):
    """Rows of several ring segments: one token in the streaming decode (K = 16640: five cached
    units per lane); 2-3 tokens of such rows do not fit LDS beside the ring and take the GEMV."""
    import kernels._lib as kl
    r = kl.route_name(Q2, M, N, K)
    assert r == ("stream_decode_kernel" if N == 1 else "gemv_kernel"), r
    _parity(M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMV_SHAPES)
def test_gemv_fallback(M, N, K):
    """4 tokens at K = 11008, and at K = 8960 (the first multiple of 256 over the limit of Q3_K's
    activation image, which Q2_K shares), do not fit LDS beside the ring: act_quant + gemv_kernel."""
    import kernels._lib as kl
    assert kl.route_name(Q2, M, N, K) == "gemv_kernel"
    _parity(M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMM_SHAPES + Q.SPLITK_SHAPES)
def test_gemm(M, N, K):
    import kernels._lib as kl
    assert "sgemm" in kl.route_name(Q2, M, N, K)
    _parity(M, N, K)


def test_splitk_shapes_split():
    import kernels._lib as kl
    for M, N, K in Q.SPLITK_SHAPES:
        r = kl.route_name(Q2, M, N, K)
        assert "split-K" in r or "reduce" in r, r


def test_one_token_seven_cached_chunks():
    """K = 28672 at one token: seven cached units per lane, the most Q2_K's decode carries (Q3_K
    and Q5_K stop at six); beside the shape lists, which are Q3_K's."""
    import kernels._lib as kl
    M, N, K = 8, 1, 28672
    assert "stream_decode_kernel" in kl.route_name(Q2, M, N, K)
    _parity(M, N, K)


# ---- 2. gq_dequantize ----
def test_dequantize_bit_equal():
    import kernels._lib as kl
    M, K = 37, 768
    raw = random_blocks("q2_k", M, K, seed=4)
    got = kl.dequantize_device(Q2, _w(raw), M, K)
    torch.cuda.synchronize()
    want = Q.dequant_f32(raw, M, K).astype(np.float16)
    assert np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16))


# ---- 3. dequant + hipBLASLt ----
@pytest.mark.parametrize("M,N,K", Q.BLAS_SHAPES)
def test_blas_path(M, N, K, tune):
    import kernels._lib as kl
    tune(GQ_BLAS_MIN_TOKENS=9)
    assert "hipBLASLt" in kl.route_name(Q2, M, N, K)
    _parity(M, N, K)


# ---- 4. routes ----
def test_routes(tune):
    import kernels._lib as kl
    assert "stream_decode_kernel" in kl.route_name(Q2, 4096, 1, 4096)
    assert "stream_decode_kernel" in kl.route_name(Q2, 4096, 1, 4096, prepared=True)
    assert "stream_decode_kernel" in kl.route_name(Q2, 4096, 4, 4096)
    assert kl.route_name(Q2, 4096, 4, 11008) == "gemv_kernel"
    for M, N in ((4096, 5), (4096, 16), (4096, 128), (11008, 16), (11008, 128), (4096, 767)):
        for prepared in (False, True):
            assert "sgemm" in kl.route_name(Q2, M, N, 4096, prepared=prepared), (M, N, prepared)
    assert "hipBLASLt" in kl.route_name(Q2, 4096, 768, 4096)
    assert "hipBLASLt" in kl.route_name(Q2, 4096, 1024, 4096)
    assert kl.route_name(Q2, 4096, 16, 4096, act="fp8") == "none"
    assert kl.route_name(Q2, 4096, 16, 4000) == "none"


@pytest.mark.parametrize("knob", ["GQ_RGEMM", "GQ_SKINNY", "GQ_KSTREAM", "GQ_GEMM_SPLITS", "GQ_SGEMM"])
def test_forced_routes_keep_sgemm(knob, tune):
    """Q2_K has no resident, K-chunked, skinny or LDS-DMA GEMM form: a knob that forces one (or
    turns the streaming GEMM off for the other types) leaves it on the streaming GEMM."""
    import kernels._lib as kl
    tune(**{knob: 4 if knob == "GQ_GEMM_SPLITS" else (0 if knob == "GQ_SGEMM" else 1)})
    for M, N in ((4096, 16), (4096, 128), (11008, 16), (70, 16)):
        for prepared in (False, True):
            assert "sgemm" in kl.route_name(Q2, M, N, 4096 if M > 70 else 512, prepared=prepared), (knob, M, N)
    _parity(70, 16, 512)


def test_row_chunks_under_the_launch_limit(tune):
    """A call over the per-launch byte limit (lowered here) is cut into row chunks, each on the
    streaming GEMM: the bits of the one-launch call (rows are independent; splits pinned).

    512 rows of 168 bytes per launch (512 + 88).  The 24 tokens' x~ (24 KiB) is counted exactly for
    this type: in whole 128-token tiles, as for the other types, no limit that cuts Q2_K rows at all
    admits more than 16 tokens (gq_capi.hip use_sgemm); Q3_K under the same limit is refused."""
    import kernels._lib as kl
    M, N, K = 600, 24, 512
    raw, B = random_blocks("q2_k", M, K, seed=8), random_activations(N, K, seed=9)
    tune(GQ_SGEMM_SPLITS=1)
    whole = run(raw, B, M, N, K)
    tune(GQ_GEMM_MAX_BYTES=86100)  # (512 rows of 168 bytes = 86016 per launch: 512 + 88; the 24 tokens' x~ fits)
    assert kl.lib().gq_mmq_call_workspace_size(Q2, 0, M, N, K) > 0
    assert kl.route_name(4, M, N, K) == "none"  # (Q3_K: whole 128-token tiles, 16 tokens at this limit)
    assert "sgemm" in kl.route_name(Q2, M, N, K)
    assert np.array_equal(run(raw, B, M, N, K).view(np.uint16), whole.view(np.uint16))
    assert Q.rel_err(whole, Q.ideal(raw, B, M, N, K)) <= Q.TIGHT_GEMM


# ---- 5. invariants ----
@pytest.mark.parametrize("N", [2, 24])
def test_activation_scaling_is_exact(N):
    M, K = 70, 768
    raw, B = random_blocks("q2_k", M, K, seed=N), random_activations(N, K, seed=N + 1)
    a, b = run(raw, B, M, N, K), run(raw, (B * np.float16(2)).astype(np.float16), M, N, K)
    assert np.array_equal((a * np.float16(2)).view(np.uint16), b.view(np.uint16))


@pytest.mark.parametrize("N", [3, 24])
def test_row_independence(N, tune):
    if N > 4:
        tune(GQ_SGEMM_SPLITS=1)
    M, K, r0, r1 = 300, 768, 101, 290
    raw, B = random_blocks("q2_k", M, K, seed=N), random_activations(N, K, seed=N + 1)
    rb = RB(K)
    full = run(raw, B, M, N, K)
    sub = run(raw[r0 * rb:r1 * rb], B, r1 - r0, N, K)
    assert np.array_equal(sub.view(np.uint16), full[:, r0:r1].view(np.uint16))


# ---- 6. prepared form ----
@pytest.mark.parametrize("N", [2, 24])
def test_prepared(N):
    import kernels._lib as kl
    M, K = 130, 1024
    raw, B = random_blocks("q2_k", M, K, seed=N), random_activations(N, K, seed=N + 1)
    ws = torch.empty(kl.workspace_size(Q2, M, N, K), dtype=torch.uint8, device=_dev())
    kl.act_prepare(_x(B), N, K, ws)
    got = kl.mmq_prepared(Q2, _w(raw), ws, M, N, K)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    if N <= 4:
        assert "stream_decode_kernel" in kl.route_name(Q2, M, N, K, prepared=True)
        assert np.array_equal(got.view(np.uint16), run(raw, B, M, N, K).view(np.uint16))
    assert Q.rel_err(got, Q.ideal(raw, B, M, N, K)) <= Q.tight(N)
    _no_timeouts()


# ---- 7. grouped decode ----
_GROUP = (("q2_k", 96, 512), ("q3_k", 64, 768), ("q4_k", 96, 512), ("q6_k", 64, 768), ("q5_k", 64, 768),
          ("q2_k", 64, 768))


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_grouped_decode_bit_identical(N):
    import kernels._lib as kl
    raws = [random_blocks(f, M, K, seed=10 + i) for i, (f, M, K) in enumerate(_GROUP)]
    Bs = {K: random_activations(N, K, seed=N + K) for K in (512, 768)}
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


def test_grouped_at_gemm_tokens_is_refused():
    import kernels._lib as kl
    N = 8
    items = [(kl.TYPES[f], _w(random_blocks(f, M, K, seed=i)), _x(random_activations(N, K, seed=i)), M, K, None)
             for i, (f, M, K) in enumerate(_GROUP)]
    assert kl.mmq_grouped(items, N) is None


# ---- 8. grouped prepared (the streaming GEMM) ----
@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("splits", [1, 2])
def test_grouped_prepared_bit_identical(N, splits, tune):
    import kernels._lib as kl
    tune(GQ_KSTREAM=0, GQ_SGEMM_SPLITS=splits)
    group = (("q2_k", 300, 512), ("q6_k", 64, 768), ("q3_k", 64, 768), ("q2_k", 96, 512))
    raws = [random_blocks(f, M, K, seed=20 + i) for i, (f, M, K) in enumerate(group)]
    Bs = {K: random_activations(N, K, seed=N + K) for K in (512, 768)}
    wss = {}
    for K, B in Bs.items():
        wss[K] = torch.empty(kl.workspace_size(Q2, 300, N, K), dtype=torch.uint8, device=_dev())
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
    """gq_mmq_id on Q2_K experts: every pair the bits of its own one-token gq_mmq; an id out of
    range gives zeros."""
    import kernels._lib as kl
    E, M, K, N, S = 4, 70, 512, 3, 2
    raw = _experts("q2_k", E, M, K)
    A = _w(raw)
    ids = np.array([[0, 3], [3, 7], [2, 0]], dtype=np.int32)  # (7: out of range)
    x = random_activations(N, K, seed=K + N)
    xt, it, out = _x(x), torch.from_numpy(ids).to(_dev()), torch.empty((N, S, M), dtype=torch.float16, device=_dev())
    rc = kl.lib().gq_mmq_id(Q2, A.data_ptr(), it.data_ptr(), xt.data_ptr(), out.data_ptr(), E, M, N, S, K, K, 0, M, None)
    assert rc == 0, kl.lib().gq_last_error()
    torch.cuda.synchronize()
    assert _same_bits(out, kl.mmq_id(Q2, A, it, xt, E, M, K))
    per = M * RB(K)
    for n in range(N):
        for s in range(S):
            e = int(ids[n, s])
            if not 0 <= e < E:
                assert not out[n, s].any()
                continue
            solo = kl.mmq(Q2, A[e * per:(e + 1) * per], xt[n:n + 1].contiguous(), M, 1, K)
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
    raw = _experts("q2_k", E, M, K)
    A = _w(raw)
    ids = np.random.default_rng(M).integers(0, E, size=(N, S), dtype=np.int32)
    ids[5, 1] = E + 2  # (an id out of range: a zero row)
    x = random_activations(N, K, seed=K + N + S)
    xt, it = _x(x), torch.from_numpy(ids).to(_dev())
    got = kl.mmq_id_sorted(Q2, A, it, xt, E, M, K)
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
            assert kl.route_name(Q2, M, n, K) == "sgemm_kernel"
            want = kl.mmq(Q2, A[e * per:(e + 1) * per], rows, M, n, K)
        torch.cuda.synchronize()
        assert _same_bits(g.index_select(0, idx), want), e
        err = Q.rel_err(want.cpu().numpy(), Q.ideal(raw[e * per:(e + 1) * per], x[[p // S for p in pairs]], M, n, K))
        print(f"q2_k sorted E={E} {M}x{K} expert {e}: {n} pairs, max|d|/max|C| = {err:.2e}")
        assert err <= Q.TIGHT_GEMM, (e, err)
    _no_timeouts()


@pytest.mark.parametrize("N", [3, 40])
def test_moe_ffn_from_gguf(tmp_path, N):
    """MoEFFN.from_gguf on a written 3-D file (Q2_K gate / up, Q3_K down; E=4, S=2, hidden 512, ffn
    256) at 6 pairs (gq_mmq_id) and 80 (the sorted GEMM), against the fp64 model stage by stage: the
    gate and up rows against the oracle on x, the down rows against the oracle on the fp16
    silu(g) * u that the block feeds them, each at the gate of its token count; the block's output
    the bits of the same torch ops on those stage outputs."""
    from gguf.file import read_gguf, write_gguf
    from kernels.moe import MoEFFN
    dev = _dev()
    E, S, H, F = 4, 2, 512, 256
    raw = {"ffn_gate_exps": ("q2_k", F, H, _experts("q2_k", E, F, H, 1)),
           "ffn_up_exps": ("q2_k", F, H, _experts("q2_k", E, F, H, 2)),
           "ffn_down_exps": ("q3_k", H, F, _experts("q3_k", E, H, F, 3))}
    path = str(tmp_path / "moe.gguf")
    write_gguf(path, {f"blk.2.{n}.weight": (t, (E, M, K), r) for n, (t, M, K, r) in raw.items()})
    _, tensors = read_gguf(path)
    ffn = MoEFFN.from_gguf(tensors, 2, dev)
    assert (ffn.gate.type_name, ffn.up.type_name, ffn.down.type_name) == ("q2_k", "q2_k", "q3_k")
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
            r = raw[name][3][e * F * RB(H):(e + 1) * F * RB(H)]
            err = Q.rel_err(got[pairs], Q.ideal(r, xn[toks], F, len(pairs), H))
            assert err <= gate, (name, e, err)
        r = raw["ffn_down_exps"][3][e * H * (F // 256 * 110):(e + 1) * H * (F // 256 * 110)]
        want = Q3M.oracle_ideal(r, np.ascontiguousarray(hn[pairs]), H, len(pairs), F)
        err = Q.rel_err(dn[pairs], want)
        assert err <= gate, ("ffn_down_exps", e, err)
    _no_timeouts()


# ---- 10. a Q2_K layer from a GGUF file ----
@pytest.mark.parametrize("fuse", [True, False])
def test_layer_mix_from_gguf(tmp_path, fuse):
    from gguf import q2_k_layer_types, read_gguf, write_gguf
    from kernels.layer_mix import LayerMix
    types = q2_k_layer_types(0, 32)  # attn_v, attn_output and ffn_down in Q3_K, the rest in Q2_K
    assert set(types.values()) == {"q2_k", "q3_k"}
    shapes = {n: (96, 512) for g in LayerMix.GROUPS[:3] for n in g}
    shapes["ffn_down"] = (64, 768)
    raw = {n: random_blocks(types[n], *shapes[n], seed=i) for i, n in enumerate(shapes)}
    p = tmp_path / "l.gguf"
    write_gguf(p, {f"blk.0.{n}.weight": (types[n], shapes[n], raw[n]) for n in shapes})
    _, tens = read_gguf(p)
    assert tens["blk.0.attn_q.weight"].type_name == "q2_k"
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
