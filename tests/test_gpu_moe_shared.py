"""GPU tests of the dense GLU decode and the shared-expert block (gq_mmq_glu: csrc/mmq_decode.hip
stream_decode_glu_kernel; gq_moe_combine_shared: csrc/moe_combine.hip; kernels/ffn.py DenseFFN;
kernels/moe.py MoEBlock(shared=...)).

gq_mmq_glu has gq_mmq_id_glu's definition on the bits of gq_mmq: with g and u read back from mmq on
the same inputs at the same N, H must be fp16(silu(g) * u).  The entry evaluates that in fp32 and
the model in float64, both rounded once to fp16: only a value within ~1e-6 of a rounding tie can
come out different, and then by one step -- "within 1 ulp16" (test_gpu_moe_fused.py _check_glu, with
its printed count).  The combine entry's arithmetic is fully specified: bit for bit."""
import functools

import numpy as np
import pytest
import torch

import moe_shared_model as MS
import test_gpu_moe_fused as TF
import type_models as TM
from gpu_types import dev as _dev, no_timeouts as _no_timeouts, same_bits as _same_bits, to_w as _w
from utils.synth import random_blocks

pytestmark = pytest.mark.gpu

_check_glu, _x = TF._check_glu, TF._x

# (type, M, K): test_gpu_moe_fused.py's geometries -- row groups, segmented rows, the Q6_K ring image,
# K % 64 == 32, several short rows per wave pass -- each at N = 1..4
CASES = [("q4_k", 200, 1024), ("q4_k", 96, 14336), ("q6_k", 257, 1536), ("q6_k", 64, 9216), ("q8_0", 333, 1056),
         ("q5_k", 130, 2048), ("q3_k", 130, 2048), ("q2_k", 130, 2048), ("q4_0", 65, 96), ("q4_0", 96, 7168)]
TOKENS = [1, 2, 3, 4]
# the shapes gq_mmq_glu must take (include/gguf_mmq.h): these at every N, every case at N = 1
NEVER_REFUSED = {("q4_k", 200, 1024), ("q6_k", 257, 1536), ("q8_0", 333, 1056)}
# the (type, token tile, cached chunks) kernels that are not built because they spill (DESIGN.md,
# "Dense GLU decode and shared experts"), as the cases of this file that ask for them: (type, M, K, N)
SPILL_REFUSED = set()


def _may_refuse(fmt, M, K, N):
    """The bound on what the fused path leaves out: the long-K rows at 3-4 tokens (their tokens do
    not fit the LDS image: gq_mmq takes the GEMV) and the spill list."""
    if N == 1 or (fmt, M, K) in NEVER_REFUSED:
        return False
    return (K >= 7168 and N >= 3) or (fmt, M, K, N) in SPILL_REFUSED


@functools.lru_cache(maxsize=None)
def _weights(fmt, M, K, which=0):
    raw = random_blocks(fmt, M, K, seed=9000 * which + 10 * M + K % 97)
    raw.setflags(write=False)
    return raw


def _entry(kl, gtype, Ag, Au, x, H, M, N, K, ldb=None, ldh=None):
    return kl.lib().gq_mmq_glu(gtype, Ag.data_ptr(), Au.data_ptr(), x.data_ptr(), H.data_ptr(), M, N, K,
                               K if ldb is None else ldb, M if ldh is None else ldh, None)


# ---- 1. the definition ----
@pytest.mark.parametrize("N", TOKENS)
@pytest.mark.parametrize("fmt,M,K", CASES)
def test_glu_definition(fmt, M, K, N):
    import kernels._lib as kl
    gtype = kl.TYPES[fmt]
    Ag, Au = _w(_weights(fmt, M, K, 0)), _w(_weights(fmt, M, K, 1))
    x = torch.from_numpy(_x(N, K, seed=K + N)).to(_dev())
    H = kl.mmq_glu(gtype, Ag, Au, x, M, N, K)
    g, u = kl.mmq(gtype, Ag, x, M, N, K), kl.mmq(gtype, Au, x, M, N, K)
    torch.cuda.synchronize()
    assert H.shape == (N, M) and H.dtype == torch.float16
    assert float(H.abs().max()) > 0
    _check_glu(H, g, u, f"{fmt} {M}x{K} N={N}")
    # the C entry itself: taken (the wrapper's bits) or refused with H untouched, within the bound
    out = torch.full((N, M), -7.0, dtype=torch.float16, device=_dev())
    rc = _entry(kl, gtype, Ag, Au, x, out, M, N, K)
    torch.cuda.synchronize()
    if rc == kl.GQ_EUNSUPPORTED:
        print(f"{fmt} {M}x{K} N={N}: refused ({kl.lib().gq_last_error().decode()}); gq_mmq's route: "
              f"{kl.route_name(gtype, M, N, K)}")
        assert torch.all(out == -7.0)
        assert _may_refuse(fmt, M, K, N), (fmt, M, K, N)
    else:
        assert rc == kl.GQ_OK, kl.lib().gq_last_error()
        assert kl.route_name(gtype, M, N, K) == "stream_decode_kernel"
        assert _same_bits(out, H)
    _no_timeouts()


# ---- 2. one token: the bits of the expert-indexed entry ----
@pytest.mark.parametrize("fmt,M,K", [CASES[0], CASES[2], CASES[4], CASES[5], CASES[6], CASES[7], CASES[8]])
def test_one_token_bits_of_id_glu(fmt, M, K):
    import kernels._lib as kl
    gtype = kl.TYPES[fmt]
    Ag, Au = _w(_weights(fmt, M, K, 0)), _w(_weights(fmt, M, K, 1))
    x = torch.from_numpy(_x(1, K, seed=K + 5)).to(_dev())
    out = torch.full((1, M), -7.0, dtype=torch.float16, device=_dev())
    assert _entry(kl, gtype, Ag, Au, x, out, M, 1, K) == kl.GQ_OK, kl.lib().gq_last_error()
    ids = torch.zeros((1, 1), dtype=torch.int32, device=_dev())
    want = kl.mmq_id_glu(gtype, Ag, Au, ids, x, 1, M, K)
    torch.cuda.synchronize()
    assert _same_bits(out, want.view(1, M))
    _no_timeouts()


# ---- 3. strides ----
@pytest.mark.parametrize("N", [1, 4])
def test_glu_strides(N):
    import kernels._lib as kl
    dev = _dev()
    fmt, M, K = CASES[0]
    Ag, Au = _w(_weights(fmt, M, K, 0)), _w(_weights(fmt, M, K, 1))
    wide = torch.from_numpy(_x(N, 2 * K, seed=6)).to(dev)
    view = wide[:, 300:300 + K]
    assert N == 1 or view.stride(0) == 2 * K
    ref = kl.mmq_glu(kl.GQ_Q4_K, Ag, Au, view.contiguous(), M, N, K)
    ref_out = torch.full((N, M), -7.0, dtype=torch.float16, device=dev)
    assert _entry(kl, kl.GQ_Q4_K, Ag, Au, view, ref_out, M, N, K, ldb=2 * K) == kl.GQ_OK  # ldb = 2K, the entry itself
    assert _same_bits(kl.mmq_glu(kl.GQ_Q4_K, Ag, Au, view, M, N, K), ref)
    flat = torch.empty(N * K + 1, dtype=torch.float16, device=dev)
    odd = flat[1:].view(N, K)  # an odd element offset: 2-byte aligned rows
    odd.copy_(view)
    assert odd.data_ptr() % 4 == 2
    assert _same_bits(kl.mmq_glu(kl.GQ_Q4_K, Ag, Au, odd, M, N, K), ref)
    buf = torch.full((N, M + 11), -7.0, dtype=torch.float16, device=dev)
    out = kl.mmq_glu(kl.GQ_Q4_K, Ag, Au, view, M, N, K, out=buf[:, :M])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    assert _same_bits(ref_out, ref)
    assert _same_bits(buf[:, :M], ref)
    assert torch.all(buf[:, M:] == -7.0)
    _no_timeouts()


# ---- 4. tokens are independent ----
@pytest.mark.parametrize("fmt,M,K", [CASES[0], CASES[3]])
def test_tokens_are_independent(fmt, M, K):
    import kernels._lib as kl
    gtype = kl.TYPES[fmt]
    Ag, Au = _w(_weights(fmt, M, K, 0)), _w(_weights(fmt, M, K, 1))
    x = torch.from_numpy(_x(4, K, seed=41)).to(_dev())
    perm = torch.tensor([2, 0, 3, 1], device=_dev())
    a = kl.mmq_glu(gtype, Ag, Au, x, M, 4, K)
    b = kl.mmq_glu(gtype, Ag, Au, x[perm].contiguous(), M, 4, K)
    torch.cuda.synchronize()
    assert _same_bits(b, a[perm])
    assert not _same_bits(a[0], a[1])
    _no_timeouts()


# ---- 5. refusal and fallback ----
def test_refusal_and_fallback_at_five_tokens():
    import kernels._lib as kl
    fmt, M, K = CASES[0]
    Ag, Au = _w(_weights(fmt, M, K, 0)), _w(_weights(fmt, M, K, 1))
    N = 5
    x = torch.from_numpy(_x(N, K, seed=15)).to(_dev())
    out = torch.full((N, M), 3.0, dtype=torch.float16, device=_dev())
    rc = _entry(kl, kl.GQ_Q4_K, Ag, Au, x, out, M, N, K)
    torch.cuda.synchronize()
    assert rc == kl.GQ_EUNSUPPORTED
    assert torch.all(out == 3.0)
    H = kl.mmq_glu(kl.GQ_Q4_K, Ag, Au, x, M, N, K)
    g, u = kl.mmq(kl.GQ_Q4_K, Ag, x, M, N, K), kl.mmq(kl.GQ_Q4_K, Au, x, M, N, K)
    torch.cuda.synchronize()
    _check_glu(H, g, u, "5 tokens (fallback)")
    _no_timeouts()


# ---- 6. the combine, bit for bit ----
@pytest.mark.parametrize("N,S,M", [(1, 1, 1), (3, 2, 513), (4, 8, 4096)])
@pytest.mark.parametrize("wdtype", [np.float16, np.float32])
@pytest.mark.parametrize("gated", [False, True])
def test_combine_shared_bit_equal(N, S, M, wdtype, gated):
    import kernels._lib as kl
    dev = _dev()
    rng = np.random.default_rng(N * 1000 + S * 10 + M + gated)
    D = rng.standard_normal((N, S, M + 5)).astype(np.float16)   # ldd > M
    Dsh = rng.standard_normal((N, M + 8)).astype(np.float16)    # ldsh > M
    W = rng.standard_normal((N, S)).astype(wdtype)
    gate = None
    if gated:
        gate = rng.standard_normal(N).astype(np.float32)
        gate[0] = -abs(gate[0]) - 0.25  # a negative, a 0 and a 1 among the gate values
        if N > 1:
            gate[1] = 0.0
        if N > 2:
            gate[2] = 1.0
    gt = torch.from_numpy(gate).to(dev) if gated else None
    Dt, St, Wt = torch.from_numpy(D).to(dev)[:, :, :M], torch.from_numpy(Dsh).to(dev)[:, :M], torch.from_numpy(W).to(dev)
    Y = kl.moe_combine_shared(Dt, Wt, St, gt)
    torch.cuda.synchronize()
    want = MS.combine_shared(D[:, :, :M], W, Dsh[:, :M], gate)
    assert Y.shape == (N, M) and Y.dtype == torch.float16
    assert np.array_equal(Y.cpu().numpy().view(np.uint16), want.view(np.uint16))
    # ldy > M into a sentinel buffer; D and Dsh shifted one element (the element-wise form): the same bits
    buf = torch.full((N, M + 3), -7.0, dtype=torch.float16, device=dev)
    flat = torch.empty(N * S * (M + 5) + 1, dtype=torch.float16, device=dev)
    odd = flat[1:].view(N, S, M + 5)
    odd.copy_(torch.from_numpy(D).to(dev))
    flat_s = torch.empty(N * (M + 8) + 1, dtype=torch.float16, device=dev)
    odd_s = flat_s[1:].view(N, M + 8)
    odd_s.copy_(torch.from_numpy(Dsh).to(dev))
    kl.moe_combine_shared(odd[:, :, :M], Wt, odd_s[:, :M], gt, out=buf[:, :M])
    torch.cuda.synchronize()
    assert np.array_equal(buf[:, :M].cpu().numpy().view(np.uint16), want.view(np.uint16))
    assert torch.all(buf[:, M:] == -7.0)
    _no_timeouts()


def test_combine_shared_vector_path_and_many_slots():
    """Aligned contiguous operands (the 16-byte path) against the model, and 65 slots through the
    wrapper's torch form."""
    import kernels._lib as kl
    dev = _dev()
    rng = np.random.default_rng(77)
    N, S, M = 4, 2, 1024
    D, Dsh = rng.standard_normal((N, S, M)).astype(np.float16), rng.standard_normal((N, M)).astype(np.float16)
    W, gate = rng.standard_normal((N, S)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    Dt, St = torch.from_numpy(D).to(dev), torch.from_numpy(Dsh).to(dev)
    assert Dt.data_ptr() % 16 == 0 and St.data_ptr() % 16 == 0
    Y = kl.moe_combine_shared(Dt, torch.from_numpy(W).to(dev), St, torch.from_numpy(gate).to(dev))
    torch.cuda.synchronize()
    assert Y.data_ptr() % 16 == 0
    assert np.array_equal(Y.cpu().numpy().view(np.uint16), MS.combine_shared(D, W, Dsh, gate).view(np.uint16))
    S = 65
    D = rng.standard_normal((N, S, 40)).astype(np.float16)
    W, Dsh = rng.standard_normal((N, S)).astype(np.float32), rng.standard_normal((N, 40)).astype(np.float16)
    out = torch.full((N, 40), 3.0, dtype=torch.float16, device=dev)
    Dt, Wt, St = torch.from_numpy(D).to(dev), torch.from_numpy(W).to(dev), torch.from_numpy(Dsh).to(dev)
    rc = kl.lib().gq_moe_combine_shared(Dt.data_ptr(), Wt.data_ptr(), 1, St.data_ptr(), 40, None, out.data_ptr(), N, S, 40, 40,
                                        40, None)
    torch.cuda.synchronize()
    assert rc == kl.GQ_EUNSUPPORTED and torch.all(out == 3.0)
    Y = kl.moe_combine_shared(Dt, Wt, St)
    torch.cuda.synchronize()
    assert np.array_equal(Y.cpu().numpy().view(np.uint16), MS.combine_shared(D, W, Dsh).view(np.uint16))
    _no_timeouts()


# ---- 7. the block ----
def _shared(kinds, fused, H=512, F=384):
    """The shared expert: ffn 384 beside the routed experts' 256.  Its down rows are 384 long, which no
    256-weight super-block type packs: where `kinds` names one for down (q6_k) the shared down is
    q8_0, the type such a tensor keeps in a K-quant file."""
    import kernels._lib as kl
    from kernels.ffn import DenseFFN
    from kernels.layer_mix import GGUFLinear
    tg, tu, td = kinds
    if F % kl.BLOCK_ELEMS[kl.TYPES[td]]:
        td = "q8_0"
    return DenseFFN(GGUFLinear(tg, _w(_weights(tg, F, H, 2)), F, H), GGUFLinear(tu, _w(_weights(tu, F, H, 3)), F, H),
                    GGUFLinear(td, _w(_weights(td, H, F, 4)), H, F), fused=fused)


def _block(kinds, fused, gated, E=4, H=512, S=2):
    from kernels.moe import MoEBlock, MoERouter
    rng = np.random.default_rng(12)
    Wr = torch.from_numpy((rng.standard_normal((E, H)) / 4).astype(np.float32)).to(_dev())
    v = torch.from_numpy((rng.standard_normal(H) / 4).astype(np.float32)).to(_dev()) if gated else None
    return MoEBlock(MoERouter(Wr, S), TF._tiny_block(kinds, fused=fused), _shared(kinds, fused), v)


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("kinds", [("q4_k", "q4_k", "q6_k"), ("q4_0", "q4_0", "q4_0")])
def test_block_is_the_composition(kinds, gated):
    import kernels._lib as kl
    blk = _block(kinds, True, gated)
    ffn, sh = blk.ffn, blk.shared
    x = torch.from_numpy(_x(3, 512, seed=21)).to(_dev())
    y = blk.forward(x)
    ids, w, _ = kl.moe_route(blk.router.Wr, x, 2)
    h = kl.mmq_id_glu(ffn.gate.gtype, ffn.gate.A, ffn.up.A, ids, x, 4, 256, 512)
    d = kl.mmq_id(ffn.down.gtype, ffn.down.A, ids, h, 4, 512, 256)
    hs = kl.mmq_glu(sh.gate.gtype, sh.gate.A, sh.up.A, x, 384, 3, 512)
    ds = kl.mmq(sh.down.gtype, sh.down.A, hs, 512, 3, 384)
    gate = None
    if gated:
        gate = kl.moe_route(blk.shared_gate, x, 1, func="sigmoid", norm=False)[1].reshape(-1)
    want = kl.moe_combine_shared(d, w, ds, gate)
    torch.cuda.synchronize()
    assert y.shape == (3, 512) and y.dtype == torch.float16
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert _same_bits(y, want)
    # the composition against the models, from the library's own g, u and d
    taken = torch.empty_like(hs)  # (the shared expert's launch is the fused one, not the wrapper's fallback)
    assert _entry(kl, sh.gate.gtype, sh.gate.A, sh.up.A, x, taken, 384, 3, 512) == kl.GQ_OK, kl.lib().gq_last_error()
    torch.cuda.synchronize()
    assert _same_bits(taken, hs)
    _check_glu(hs, sh.gate(x), sh.up(x), f"{kinds} shared expert")
    _check_glu(h, ffn.gate(x, ids), ffn.up(x, ids), f"{kinds} routed experts")
    gn = gate.cpu().numpy() if gated else None
    if gated:
        z = (x.float() @ blk.shared_gate.float().T).reshape(-1).cpu().numpy().astype(np.float64)
        assert np.allclose(gn, 1.0 / (1.0 + np.exp(-z)), rtol=1e-5) and gn.dtype == np.float32
    model = MS.combine_shared(d.cpu().numpy(), w.cpu().numpy(), ds.cpu().numpy(), gn)
    assert np.array_equal(y.cpu().numpy().view(np.uint16), model.view(np.uint16))
    # the dense FFN on its own
    assert _same_bits(sh.forward(x), ds)
    _no_timeouts()


def test_unfused_block_and_dense_ffn_are_the_torch_lines():
    kinds = ("q4_k", "q4_k", "q6_k")
    blk = _block(kinds, False, True)
    sh = blk.shared
    x = torch.from_numpy(_x(3, 512, seed=21)).to(_dev())
    ds = sh.down(torch.nn.functional.silu(sh.gate(x)) * sh.up(x))
    assert _same_bits(sh.forward(x), ds)
    ids, w = blk.router(x)
    gate = torch.sigmoid(x.float() @ blk.shared_gate.float().T).reshape(-1)
    got_gate = blk.token_gate(x)
    assert torch.allclose(got_gate, gate, rtol=1e-5)
    want = blk.ffn(x, ids, w) + got_gate[:, None] * ds
    y = blk.forward(x)
    torch.cuda.synchronize()
    assert y.dtype == want.dtype and torch.equal(y, want)
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0
    _no_timeouts()


def test_dense_ffn_mixed_types_fall_back():
    """Gate and up of different types: no fused kernel; DenseFFN(fused=True) makes the same h from two
    mmq calls and still meets the definition."""
    import kernels._lib as kl
    sh = _shared(("q4_k", "q5_k", "q6_k"), True)
    x = torch.from_numpy(_x(3, 512, seed=21)).to(_dev())
    g, u = sh.gate(x), sh.up(x)
    h = kl.glu_torch(g, u)
    _check_glu(h, g, u, "mixed types")
    y = sh.forward(x)
    torch.cuda.synchronize()
    assert _same_bits(y, sh.down(h))
    _no_timeouts()


# ---- 8. unchanged bits ----
def test_moe_ffn_bits_unchanged_and_slots():
    import kernels._lib as kl
    kinds = ("q4_k", "q4_k", "q6_k")
    it, x, w = TF._tiny_inputs()
    ffn = TF._tiny_block(kinds, fused=True)
    h = kl.mmq_id_glu(ffn.gate.gtype, ffn.gate.A, ffn.up.A, it, x, ffn.gate.E, ffn.gate.M, ffn.gate.K)
    d = kl.mmq_id(ffn.down.gtype, ffn.down.A, it, h, ffn.down.E, ffn.down.M, ffn.down.K)
    y = ffn.forward(x, it, w)
    assert _same_bits(y, kl.moe_combine(d, w))                     # (test_fused_forward_is_the_composition)
    assert _same_bits(ffn.slots(x, it), d)
    assert _same_bits(kl.moe_combine(ffn.slots(x, it), w), y)
    ffn = TF._tiny_block(kinds, fused=False)
    g, u = ffn.gate(x, it), ffn.up(x, it)
    du = ffn.down(torch.nn.functional.silu(g) * u, it)
    want = (w[..., None] * du).sum(1)                               # (test_unfused_bits_unchanged)
    y = ffn.forward(x, it, w)
    torch.cuda.synchronize()
    assert y.dtype == want.dtype and _same_bits(y, want)
    assert _same_bits(ffn.slots(x, it), du)
    _no_timeouts()


# ---- 9. graph capture ----
def test_graph_capture_follows_x():
    blk = _block(("q4_k", "q4_k", "q6_k"), True, True)
    x = torch.from_numpy(_x(3, 512, seed=21)).to(_dev())
    blk.forward(x)  # (first use outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = blk.forward(x)
    graph.replay()
    torch.cuda.synchronize()
    first = y.clone()
    assert _same_bits(first, blk.forward(x))
    x.copy_(torch.from_numpy(_x(3, 512, seed=22)).to(_dev()))
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(y, blk.forward(x))
    assert not _same_bits(y, first)
    _no_timeouts()


# ---- 10. accuracy ----
def test_accuracy_no_worse_than_unfused():
    """Against ref = silu(g64) * u64 from the float64 ideals of 24 sampled rows: the fused H errs at
    most as much as the unfused torch result plus one fp16 rounding (2^-11) -- it has the same g
    and u and one rounding fewer (test_gpu_moe_fused.py's bound, for its reason)."""
    import kernels._lib as kl
    fmt, M, K, N = "q4_k", 130, 2048, 4
    rg, ru = _weights(fmt, M, K, 0), _weights(fmt, M, K, 1)
    Ag, Au = _w(rg), _w(ru)
    x = _x(N, K, seed=31)
    xt = torch.from_numpy(x).to(_dev())
    out = torch.empty((N, M), dtype=torch.float16, device=_dev())
    assert _entry(kl, kl.GQ_Q4_K, Ag, Au, xt, out, M, N, K) == kl.GQ_OK, kl.lib().gq_last_error()
    g, u = kl.mmq(kl.GQ_Q4_K, Ag, xt, M, N, K), kl.mmq(kl.GQ_Q4_K, Au, xt, M, N, K)
    Hu = torch.nn.functional.silu(g) * u
    torch.cuda.synchronize()
    Hf, Hu = out.cpu().numpy().astype(np.float64), Hu.cpu().numpy().astype(np.float64)
    rows = np.sort(np.random.default_rng(M + K).choice(M, size=24, replace=False))
    rb = rg.size // M
    sub = [np.concatenate([r[i * rb:(i + 1) * rb] for i in rows]) for r in (rg, ru)]
    g64, u64 = (np.asarray(TM.judge(fmt, sb, x, len(rows), N, K), dtype=np.float64) for sb in sub)
    ref = g64 / (1.0 + np.exp(-g64)) * u64
    assert ref.shape == (N, len(rows))
    for n in range(N):
        ef = np.max(np.abs(Hf[n][rows] - ref[n])) / np.max(np.abs(ref[n]))
        eu = np.max(np.abs(Hu[n][rows] - ref[n])) / np.max(np.abs(ref[n]))
        print(f"{fmt} token {n}: fused {ef:.3e}, unfused {eu:.3e}")
        assert ef <= eu + 2.0 ** -11, (n, ef, eu)
    _no_timeouts()
