"""GPU tests of GGUF Q5_K (GGML type 13): every route -- the streaming decode (alone, grouped, on
the prepared copy), the GEMV fallback, the streaming GEMM (alone, grouped, split-K), dequantize +
hipBLASLt -- against the numpy model of tests/q5k_model.py (the reference has no Q5_K):
max|C - ideal| / max|ideal| <= 1.5e-3 at N <= 4 and 4e-3 otherwise, ideal = x~ @ W^T in fp64 with
x~ from the project's q8_1 quantizer.  Q4_K / Q6_K items of mixed cases use the oracle."""
import numpy as np
import pytest
import torch

import oracle as O
import q5k_model as Q
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

Q5 = 3


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _w(raw):
    return torch.from_numpy(np.array(raw).view(np.int8)).to(_dev())  # (a copy: the shared cases are read-only)


def _x(B):
    return torch.from_numpy(np.array(B)).to(_dev())


def run(raw, B, M, N, K):
    from kernels.mmq_q5_k import mmq_q5_k
    C = mmq_q5_k(_w(raw), _x(B), M, N, K)
    torch.cuda.synchronize()
    assert C.shape == (N, M) and C.dtype == torch.float16
    return C.cpu().numpy()


def _no_timeouts():
    import kernels._lib as kl
    assert kl.lib().gq_debug_sync_timeouts() == 0


def _parity(M, N, K):
    raw, B, want = Q.case(M, N, K)
    err = Q.rel_err(run(raw, B, M, N, K), want)
    print(f"q5_k {M}x{N}x{K}: max|d|/max|C| = {err:.2e}")
    assert err <= Q.tight(N), (M, N, K, err)
    _no_timeouts()


# ---- 1. parity, ragged shapes ----
@pytest.mark.parametrize("M,N,K", Q.DECODE_SHAPES)
def test_decode(M, N, K):
    import kernels._lib as kl
    assert "stream_decode_kernel" in kl.route_name(Q5, M, N, K)
    _parity(M, N, K)


@pytest.mark.parametrize("M,N,K", Q.LONG_SHAPES)
def test_long_rows(M, N, K):
    """Rows of several ring segments: one token in the streaming decode (K = 16640: five cached
    units per lane); 2-3 tokens of such rows do not fit LDS beside the ring and take the GEMV."""
    import kernels._lib as kl
    r = kl.route_name(Q5, M, N, K)
    assert r == ("stream_decode_kernel" if N == 1 else "gemv_kernel"), r
    assert r == kl.route_name(kl.GQ_Q4_K, M, N, K)  # (decode_fused_ok(Q5_K) is Q4_K's)
    _parity(M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMV_SHAPES)
def test_gemv_fallback(M, N, K):
    """4 tokens at K = 11008 do not fit LDS beside the ring: act_quant + gemv_kernel."""
    import kernels._lib as kl
    assert kl.route_name(Q5, M, N, K) == "gemv_kernel"
    _parity(M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMM_SHAPES + Q.SPLITK_SHAPES)
def test_gemm(M, N, K):
    import kernels._lib as kl
    assert "sgemm" in kl.route_name(Q5, M, N, K)
    _parity(M, N, K)


@pytest.mark.parametrize("M,N,K", [(4096, 1, 4096), (4096, 4, 4096), (11008, 2, 4096), (4096, 1, 11008),
                                   (4096, 3, 11008), (4096, 16, 4096), (11008, 128, 4096), (4096, 40, 11008),
                                   (512, 768, 1024)])
def test_llama_shapes_sampled_rows(M, N, K):
    """The Llama-7B shapes (many tasks per wave, several rows per task, K = 11008's 43 super-blocks,
    every row tile of the GEMM, the default BLAS threshold): 192 sampled rows against the model."""
    raw, B = random_blocks("q5_k", M, K, seed=M + N), random_activations(N, K, seed=K + N)
    got = run(raw, B, M, N, K)
    rows = np.sort(np.random.default_rng(N).choice(M, size=192, replace=False))
    rb = K // 256 * 176
    sub = np.concatenate([raw[r * rb:(r + 1) * rb] for r in rows])
    err = Q.rel_err(got[:, rows], Q.ideal(sub, B, len(rows), N, K))
    print(f"q5_k {M}x{N}x{K}: max|d|/max|C| = {err:.2e} (sampled rows)")
    assert err <= Q.tight(N), (M, N, K, err)
    _no_timeouts()


def test_splitk_shapes_split():
    import kernels._lib as kl
    for M, N, K in Q.SPLITK_SHAPES:
        r = kl.route_name(Q5, M, N, K)
        assert "split-K" in r or "reduce" in r, r


# ---- 2. gq_dequantize ----
def test_dequantize_bit_equal():
    import kernels._lib as kl
    M, K = 37, 768
    raw = random_blocks("q5_k", M, K, seed=4)
    got = kl.dequantize_device(Q5, _w(raw), M, K)
    torch.cuda.synchronize()
    want = Q.dequant_f32(raw, M, K).astype(np.float16)
    assert np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16))


# ---- 3. dequant + hipBLASLt ----
@pytest.mark.parametrize("M,N,K", Q.BLAS_SHAPES)
def test_blas_path(M, N, K, tune):
    import kernels._lib as kl
    tune(GQ_BLAS_MIN_TOKENS=9)
    assert "hipBLASLt" in kl.route_name(Q5, M, N, K)
    _parity(M, N, K)


# ---- 4. routes ----
def test_routes(tune):
    import kernels._lib as kl
    assert "stream_decode_kernel" in kl.route_name(Q5, 4096, 1, 4096)
    assert "stream_decode_kernel" in kl.route_name(Q5, 4096, 1, 4096, prepared=True)
    for M, N in ((4096, 16), (4096, 128), (11008, 16), (11008, 128)):
        for prepared in (False, True):
            assert "sgemm" in kl.route_name(Q5, M, N, 4096, prepared=prepared), (M, N, prepared)
    assert "hipBLASLt" in kl.route_name(Q5, 4096, 1024, 4096)
    assert kl.route_name(Q5, 4096, 16, 4096, act="fp8") == "none"


@pytest.mark.parametrize("knob", ["GQ_RGEMM", "GQ_SKINNY", "GQ_KSTREAM", "GQ_GEMM_SPLITS", "GQ_SGEMM"])
def test_forced_routes_keep_sgemm(knob, tune):
    """Q5_K has no resident, K-chunked, skinny or LDS-DMA GEMM form: a knob that forces one (or
    turns the streaming GEMM off for the other types) leaves it on the streaming GEMM."""
    import kernels._lib as kl
    tune(**{knob: 4 if knob == "GQ_GEMM_SPLITS" else (0 if knob == "GQ_SGEMM" else 1)})
    for M, N in ((4096, 16), (4096, 128), (11008, 16), (70, 16)):
        for prepared in (False, True):
            assert "sgemm" in kl.route_name(Q5, M, N, 4096 if M > 70 else 512, prepared=prepared), (knob, M, N)
    _parity(70, 16, 512)


def test_row_chunks_under_the_launch_limit(tune):
    """A call over the per-launch byte limit (lowered here) is cut into 256-row chunks, each on the
    streaming GEMM: the bits of the one-launch call (rows are independent; splits pinned)."""
    import kernels._lib as kl
    M, N, K = 600, 24, 512
    raw, B = random_blocks("q5_k", M, K, seed=8), random_activations(N, K, seed=9)
    tune(GQ_SGEMM_SPLITS=1)
    whole = run(raw, B, M, N, K)
    tune(GQ_GEMM_MAX_BYTES=140000)  # (256 rows of 352 bytes per launch; the 24 tokens' x~ fits)
    assert "sgemm" in kl.route_name(Q5, M, N, K)
    assert np.array_equal(run(raw, B, M, N, K).view(np.uint16), whole.view(np.uint16))
    assert Q.rel_err(whole, Q.ideal(raw, B, M, N, K)) <= Q.TIGHT_GEMM


# ---- 5. invariants ----
@pytest.mark.parametrize("N", [2, 24])
def test_activation_scaling_is_exact(N):
    M, K = 70, 768
    raw, B = random_blocks("q5_k", M, K, seed=N), random_activations(N, K, seed=N + 1)
    a, b = run(raw, B, M, N, K), run(raw, (B * np.float16(2)).astype(np.float16), M, N, K)
    assert np.array_equal((a * np.float16(2)).view(np.uint16), b.view(np.uint16))


@pytest.mark.parametrize("N", [3, 24])
def test_row_independence(N, tune):
    if N > 4:
        tune(GQ_SGEMM_SPLITS=1)
    M, K, r0, r1 = 300, 768, 101, 290
    raw, B = random_blocks("q5_k", M, K, seed=N), random_activations(N, K, seed=N + 1)
    rb = K // 256 * 176
    full = run(raw, B, M, N, K)
    sub = run(raw[r0 * rb:r1 * rb], B, r1 - r0, N, K)
    assert np.array_equal(sub.view(np.uint16), full[:, r0:r1].view(np.uint16))


# ---- 6. prepared form ----
@pytest.mark.parametrize("N", [2, 24])
def test_prepared(N):
    import kernels._lib as kl
    M, K = 130, 1024
    raw, B = random_blocks("q5_k", M, K, seed=N), random_activations(N, K, seed=N + 1)
    ws = torch.empty(kl.workspace_size(Q5, M, N, K), dtype=torch.uint8, device=_dev())
    kl.act_prepare(_x(B), N, K, ws)
    got = kl.mmq_prepared(Q5, _w(raw), ws, M, N, K)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    if N <= 4:
        assert "stream_decode_kernel" in kl.route_name(Q5, M, N, K, prepared=True)
        assert np.array_equal(got.view(np.uint16), run(raw, B, M, N, K).view(np.uint16))
    assert Q.rel_err(got, Q.ideal(raw, B, M, N, K)) <= Q.tight(N)
    _no_timeouts()


# ---- 7. grouped decode ----
_GROUP = (("q5_k", 96, 512), ("q6_k", 64, 768), ("q4_k", 96, 512), ("q5_k", 64, 768))


def _ideal(fmt, raw, B, M, N, K):
    if fmt == "q5_k":
        return Q.ideal(raw, B, M, N, K)
    return O.mmq_from_fp16(fmt, raw, B, M, N, K, O.IDEAL)


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


def test_grouped_at_gemm_tokens_is_refused():
    import kernels._lib as kl
    N = 8
    items = [(kl.TYPES[f], _w(random_blocks(f, M, K, seed=i)), _x(random_activations(N, K, seed=i)), M, K, None)
             for i, (f, M, K) in enumerate(_GROUP)]
    assert kl.mmq_grouped(items, N) is None


def test_grouped_decode_long_rows_with_q5_k_refused():
    """A one-token grouped launch that holds a Q5_K item carries every format's cases up to 4
    cached chunks per lane (K <= 16384): beyond that the launch is refused, nothing runs, and each
    item's own call (the streaming decode) stands."""
    import kernels._lib as kl
    K = 20480
    items = [(kl.TYPES[f], _w(random_blocks(f, 16, K, seed=i)), _x(random_activations(1, K, seed=i)), 16, K, None)
             for i, f in enumerate(("q5_k", "q4_k"))]
    assert kl.mmq_grouped(items, 1) is None
    assert kl.mmq_grouped(items[1:], 1) is not None  # (without the Q5_K item: the other formats' kernel)
    torch.cuda.synchronize()
    raw = random_blocks("q5_k", 16, K, seed=0)
    B = random_activations(1, K, seed=0)
    assert "stream_decode_kernel" in kl.route_name(Q5, 16, 1, K)
    assert Q.rel_err(run(raw, B, 16, 1, K), Q.ideal(raw, B, 16, 1, K)) <= Q.TIGHT_GEMV


# ---- 8. grouped prepared (the streaming GEMM) ----
@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("splits", [1, 2])
def test_grouped_prepared_bit_identical(N, splits, tune):
    import kernels._lib as kl
    tune(GQ_KSTREAM=0, GQ_SGEMM_SPLITS=splits)
    group = (("q5_k", 300, 512), ("q6_k", 64, 768), ("q5_k", 64, 768), ("q6_k", 96, 512))
    raws = [random_blocks(f, M, K, seed=20 + i) for i, (f, M, K) in enumerate(group)]
    Bs = {K: random_activations(N, K, seed=N + K) for K in (512, 768)}
    wss = {}
    for K, B in Bs.items():
        wss[K] = torch.empty(kl.workspace_size(Q5, 300, N, K), dtype=torch.uint8, device=_dev())
        kl.act_prepare(_x(B), N, K, wss[K])
    items = [(kl.TYPES[f], _w(r), wss[K], M, K, None) for (f, M, K), r in zip(group, raws)]
    outs = kl.mmq_grouped_prepared(items, N)
    assert outs is not None, kl.lib().gq_last_error()
    torch.cuda.synchronize()
    tune(GQ_SGEMM=1, GQ_RGEMM=0, GQ_SKINNY=0)  # (the other types' per-matrix call on the streaming GEMM too)
    for (f, M, K), r, it, C in zip(group, raws, items, outs):
        ws = torch.empty(kl.workspace_size(it[0], M, N, K), dtype=torch.uint8, device=_dev())
        kl.act_prepare(_x(Bs[K]), N, K, ws)
        solo = kl.mmq_prepared(it[0], it[1], ws, M, N, K)
        torch.cuda.synchronize()
        assert torch.equal(C.view(torch.int16), solo.view(torch.int16)), (f, M, K)
        assert Q.rel_err(C.cpu().numpy(), _ideal(f, r, Bs[K], M, N, K)) <= Q.TIGHT_GEMM, (f, M, K)
    _no_timeouts()


# ---- 9. a Q5_K_M layer from a GGUF file ----
@pytest.mark.parametrize("fuse", [True, False])
def test_layer_mix_from_gguf(tmp_path, fuse):
    from gguf import q5_k_m_layer_types, read_gguf, write_gguf
    from kernels.layer_mix import LayerMix
    types = q5_k_m_layer_types(0, 32)  # layer 0: attn_v / ffn_down in Q6_K
    shapes = {n: (96, 512) for g in LayerMix.GROUPS[:3] for n in g}
    shapes["ffn_down"] = (64, 768)
    raw = {n: random_blocks(types[n], *shapes[n], seed=i) for i, n in enumerate(shapes)}
    p = tmp_path / "l.gguf"
    write_gguf(p, {f"blk.0.{n}.weight": (types[n], shapes[n], raw[n]) for n in shapes})
    _, tens = read_gguf(p)
    assert tens["blk.0.attn_q.weight"].type_name == "q5_k"
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
