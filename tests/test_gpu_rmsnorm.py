"""The fused residual add + RMSNorm on the GPU (gq_rmsnorm, gq_rmsnorm_prepare; kernels/norm.py,
DenseFFN / MoEBlock.forward_normed) against tests/rmsnorm_model.py:

1. h is the numpy sum bit for bit, also written in place over x or over the residual;
2. y is within 1 fp16 ulp of the fp64 model everywhere and differs from it on at most 1% of a row --
   a condition, not a measurement: the kernel's fp32 result (a tree sum of at most ~72 additions, one
   division and square root, two products) carries a relative error of a few 2^-24 against fp16's
   half-ulp of at least 2^-12, so about 2e-4 of the elements may round the other way; a sequential
   K-long fp32 sum would not stay under it at the long rows;
3. a row's bits are its own: at every N, stride and base, and whichever outputs are asked for,
   with nothing written around any output;
4. the workspace gq_rmsnorm_prepare leaves is gq_act_prepare's of the same y, byte for byte;
5. gq_mmq_prepared on it is held to the matmul gate it always had, the oracle reading the GPU's y;
6. the blocks' forward_normed are the compositions they document;
7. a captured DenseFFN.forward_normed follows its inputs;
8. under GQ_GEMM_I8=1 the entry is the two-step path, or refuses without a Y.

Rows: utils.synth.random_activations scaled by 1e-3, 1 and 300, an all-zero row and a row whose one
non-zero element is 6e4, in that order and again from the top; w = 1 + 0.3 normal (fp32).
The workspaces are sized by gq_mmq_workspace_size_ex for Q6_K at M = 64 where K % 256 == 0 and for
Q8_0 (32-element blocks) at the other K, which no 256-element type is sized for."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle as O
import rmsnorm_model as RM
import strided as ST
import type_models as TM
from gpu_types import dev as _dev, same_bits as _same_bits, to_w as _w
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

KS = [32, 256, 2048, 2080, 4096, 11008, 16640]
EPS = [1e-5, 1e-6]
OK, EUNSUPPORTED = 0, 3


# ---- inputs: computed once, never written to ----
@functools.lru_cache(maxsize=None)
def _inputs(N, K):
    x = random_activations(N, K, seed=K + 1).astype(np.float32)
    for n in range(N):
        kind = n % 5
        if kind == 3:
            x[n] = 0.0
        elif kind == 4:
            x[n] = 0.0
            x[n, (7 * n + 3) % K] = 6e4
        else:
            x[n] *= (1e-3, 1.0, 300.0)[kind]
    x = x.astype(np.float16)
    r = random_activations(N, K, seed=K + 77)
    w = (1 + 0.3 * np.random.default_rng(K).standard_normal(K)).astype(np.float32)
    for a in (x, r, w):
        a.setflags(write=False)
    return x, r, w


def _t(a):
    return torch.from_numpy(np.array(a)).to(_dev())


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.uint16)


def _ws_bytes(kl, N, K):
    return int(kl.lib().gq_mmq_workspace_size_ex(kl.GQ_Q6_K if K % 256 == 0 else kl.GQ_Q8_0, kl.GQ_ACT_Q8_1, 64, N, K))


def _ld(t, K):
    return max(t.stride(0), K) if t is not None else K


def _p(t):
    return t.data_ptr() if t is not None else None


def _call(kl, x, r, h, w, eps, y, N, K, ws=None):
    """The raw entries on tensors or strided views; ws: the prepare entry.  Returns the status."""
    L = kl.lib()
    args = (_p(x), _p(r), _p(h), w.data_ptr(), eps, _p(y), N, K, _ld(x, K), _ld(r, K), _ld(h, K), _ld(y, K))
    if ws is None:
        return L.gq_rmsnorm(*args, None)
    return L.gq_rmsnorm_prepare(*args, ws.data_ptr(), ws.numel(), None)


@functools.lru_cache(maxsize=None)
def _reference_rows(K, with_r, eps):
    """(h, y) as (33, K) uint16 arrays whose row n is the ONE-row call's on row n (contiguous,
    aligned): what every other call's row n is held to."""
    import kernels._lib as kl
    x, r, w = _inputs(33, K)
    xd, rd, wd = _t(x), _t(r), _t(w)
    h = torch.zeros((33, K), dtype=torch.float16, device=_dev())
    y = torch.zeros((33, K), dtype=torch.float16, device=_dev())
    for n in range(33):
        assert _call(kl, xd[n:n + 1], rd[n:n + 1] if with_r else None, h[n:n + 1], wd, eps, y[n:n + 1], 1, K) == OK, \
            kl.lib().gq_last_error()
    torch.cuda.synchronize()
    hb, yb = _bits(h), _bits(y)
    hb.setflags(write=False)
    yb.setflags(write=False)
    return hb, yb


# ---- 1. and 2. ----
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("K", KS)
def test_h_is_exact_and_y_is_within_one_ulp_of_fp64(K, eps):
    import kernels._lib as kl
    N = 10
    x33, r33, w = _inputs(33, K)
    x, r = x33[:N], r33[:N]
    wd = _t(w)
    for with_r in (True, False):
        h_want = RM.h_of(x, r if with_r else None)
        y_want = RM.y_ideal(h_want, w, eps)
        assert np.isfinite(y_want).all()
        for alias in ("none", "x", "r"):
            if alias == "r" and not with_r:
                continue
            xd, rd = _t(x), (_t(r) if with_r else None)
            h = {"none": torch.zeros_like(xd), "x": xd, "r": rd}[alias]
            y = torch.zeros_like(xd)
            assert _call(kl, xd, rd, h, wd, eps, y, N, K) == OK, kl.lib().gq_last_error()
            torch.cuda.synchronize()
            what = f"K={K} eps={eps} residual={with_r} H over {alias}"
            assert np.array_equal(_bits(h), h_want.view(np.uint16)), what
            got = y.cpu().numpy()
            d = RM.ulp_dist(got, y_want)
            frac = (d != 0).sum(1) / K
            print(f"{what}: max ulp {int(d.max())}, largest differing share of a row {frac.max():.2e}")
            assert d.max() <= 1, what
            assert (frac <= 0.01).all(), f"{what}: {frac}"
            assert np.array_equal(_bits(y), _reference_rows(K, with_r, eps)[1][:N]), what  # (and 3. at N = 10)


# ---- 3. ----
OUTPUTS = [("H", "Y"), ("Y",), ("H", "ws"), ("ws",), ("H", "Y", "ws")]


@pytest.mark.parametrize("K", KS)
def test_a_row_is_its_own_at_every_n_stride_base_and_output_set(K):
    import kernels._lib as kl
    eps = 1e-5
    x33, r33, w = _inputs(33, K)
    wd = _t(w)
    calls = 0
    for with_r in (True, False):
        h_ref, y_ref = _reference_rows(K, with_r, eps)
        for N in (1, 4, 5, 7, 33):
            # the workspace of these rows' y as gq_act_prepare leaves it, contiguous and aligned
            need = _ws_bytes(kl, N, K)
            _, ws_ref, _ = ST.guarded_ws(need)
            y_dev = torch.from_numpy(np.array(y_ref[:N]).view(np.float16)).to(_dev())
            kl.act_prepare(y_dev, N, K, ws_ref)
            for ld, lead in ((K, 0), (K + 24, 1), (K, 1), (K + 24, 0)):
                xv = ST.wide_in(np.array(x33[:N]), ld, lead, ST.INF)
                rv = ST.wide_in(np.array(r33[:N]), ld, lead, ST.INF) if with_r else None
                for outs in OUTPUTS:
                    what = f"K={K} residual={with_r} N={N} ld={ld} lead={lead} outputs={outs}"
                    _, hv, hcheck = ST.wide_out(N, K, ld, lead) if "H" in outs else (None, None, None)
                    _, yv, ycheck = ST.wide_out(N, K, ld, lead) if "Y" in outs else (None, None, None)
                    alloc, ws, wcheck = ST.guarded_ws(need) if "ws" in outs else (None, None, None)
                    assert _call(kl, xv, rv, hv, wd, eps, yv, N, K, ws=ws) == OK, (what, kl.lib().gq_last_error())
                    torch.cuda.synchronize()
                    calls += 1
                    if hv is not None:
                        assert np.array_equal(_bits(hv), h_ref[:N]), what
                        hcheck()
                    if yv is not None:
                        assert np.array_equal(_bits(yv), y_ref[:N]), what
                        ycheck()
                    if ws is not None:
                        assert torch.equal(ws, ws_ref), what
                        wcheck()
    print(f"K={K}: {calls} calls held to the one-row calls")
    assert calls == 2 * 5 * 4 * len(OUTPUTS)


# ---- 4. ----
# (N, K): the forms are gq_act_prepare's own choice -- SOA codes + d + s up to 4 tokens and at every
# K that is no multiple of 256 (so (5, 2080) too), with the fp16 copy where a fused decode could read
# it ((4, 8704): yes, (4, 11008): no), the DEQ x~ otherwise
WS_CASES = [(1, 32), (1, 4096), (4, 8704), (4, 11008), (5, 256), (5, 2080), (33, 4096), (130, 512)]


def _workspace_pair(kl, N, K, with_r, eps=1e-5):
    """(ws_fused with Y NULL, ws_fused with Y, Y of that call, ws of rmsnorm -> act_prepare, its y)"""
    x, r, w = _inputs(N, K)
    xd, rd, wd = _t(x), (_t(r) if with_r else None), _t(w)
    need = _ws_bytes(kl, N, K)
    assert need > 0
    y = torch.zeros_like(xd)
    assert _call(kl, xd, rd, None, wd, eps, y, N, K) == OK, kl.lib().gq_last_error()
    _, two, check2 = ST.guarded_ws(need)
    kl.act_prepare(y, N, K, two)
    _, a, checka = ST.guarded_ws(need)
    rc_a = _call(kl, xd, rd, None, wd, eps, None, N, K, ws=a)
    _, b, checkb = ST.guarded_ws(need)
    yb = torch.zeros_like(xd)
    rc_b = _call(kl, xd, rd, None, wd, eps, yb, N, K, ws=b)
    torch.cuda.synchronize()
    for c in (check2, checka, checkb):
        c()
    return rc_a, a, rc_b, b, yb, two, y


@pytest.mark.parametrize("with_r", [True, False])
@pytest.mark.parametrize("N,K", WS_CASES)
def test_the_workspace_is_act_prepares(N, K, with_r):
    import kernels._lib as kl
    rc_a, a, rc_b, b, yb, two, y = _workspace_pair(kl, N, K, with_r)
    assert rc_a == OK and rc_b == OK, kl.lib().gq_last_error()
    assert not torch.equal(two, torch.full_like(two, ST.WS_FILL))  # (something was written)
    assert torch.equal(a, two), f"N={N} K={K}: fused workspace (Y NULL) differs from rmsnorm + act_prepare"
    assert torch.equal(b, two), f"N={N} K={K}: fused workspace (Y given) differs from rmsnorm + act_prepare"
    assert _same_bits(yb, y)


# ---- 5. ----
@pytest.mark.parametrize("M,N,K", [(65, 4, 1024), (70, 16, 512), (129, 33, 768)])
@pytest.mark.parametrize("fmt", ["q4_k", "q6_k"])
def test_mmq_prepared_on_the_fused_workspace(fmt, M, N, K):
    import kernels._lib as kl
    x, r, w = _inputs(N, K)
    raw = random_blocks(fmt, M, K, seed=M + N)
    gtype = kl.TYPES[fmt]
    ws = torch.empty(kl.workspace_size(gtype, M, N, K), dtype=torch.uint8, device=_dev())
    y = torch.zeros((N, K), dtype=torch.float16, device=_dev())
    kl.rmsnorm_prepare(_t(x), _t(w), 1e-5, ws, residual=_t(r), y_out=y)
    C = kl.mmq_prepared(gtype, _w(raw), ws, M, N, K)
    torch.cuda.synchronize()
    want = O.mmq_from_fp16(fmt, raw, y.cpu().numpy(), M, N, K, O.IDEAL)
    err = TM.rel_err(C.cpu().numpy(), want)
    print(f"{fmt} M={M} N={N} K={K}: rel err {err:.2e} (gate {TM.tight(N):.1e})")
    assert err <= TM.tight(N)


# ---- 6. ----
HID, FFN = 512, 768


def _norm():
    """(weights / 32: the synthetic weights are large, and silu(g) * u must stay in fp16 range)"""
    from kernels.norm import RMSNorm
    return RMSNorm(_t(_inputs(1, HID)[2] / np.float32(32)), 1e-5)


def _dense(fused=False, norm=True):
    from kernels.ffn import DenseFFN
    from kernels.layer_mix import GGUFLinear
    lin = lambda fmt, M, K, seed: GGUFLinear(fmt, _w(random_blocks(fmt, M, K, seed=seed)), M, K)
    return DenseFFN(lin("q4_k", FFN, HID, 1), lin("q4_k", FFN, HID, 2), lin("q6_k", HID, FFN, 3), fused=fused,
                    norm=_norm() if norm else None)


def _xr(N, seed=0):
    x = random_activations(N, HID, seed=100 + seed)
    r = random_activations(N, HID, seed=200 + seed)
    return x, r


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("N", [1, 4, 5, 33])
def test_dense_ffn_forward_normed(N, fused):
    import kernels._lib as kl
    ffn = _dense(fused)
    x, r = _xr(N)
    for res in (r, None):
        xd, rd = _t(x), (_t(res) if res is not None else None)
        out, h = ffn.forward_normed(xd, rd)
        y = ffn.norm(xd, rd)
        y = y[0] if rd is not None else y
        direct = ffn.forward(y)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(h), RM.h_of(x, res).view(np.uint16))
        assert out.shape == (N, HID) and out.dtype == torch.float16 and torch.isfinite(out).all()
        if N < 5:
            assert _same_bits(out, direct)
            continue
        err = TM.rel_err(out.cpu().numpy(), direct.cpu().numpy())
        print(f"N={N} fused={fused}: forward_normed vs forward(y) rel err {err:.2e}")
        assert err <= TM.tight(N)
        ws = torch.empty(max(ffn.gate.workspace_bytes(N), ffn.up.workspace_bytes(N)), dtype=torch.uint8, device=_dev())
        kl.act_prepare(y, N, HID, ws)
        g = kl.mmq_prepared(ffn.gate.gtype, ffn.gate.A, ws, FFN, N, HID)
        u = kl.mmq_prepared(ffn.up.gtype, ffn.up.A, ws, FFN, N, HID)
        hand = ffn.down(kl.glu_torch(g, u) if fused else torch.nn.functional.silu(g) * u)
        torch.cuda.synchronize()
        assert _same_bits(out, hand)


@pytest.mark.parametrize("N", [2, 40])
def test_moe_block_forward_normed(N):
    import test_gpu_moe_fused as TF
    from kernels.moe import MoEBlock, MoERouter
    E, S = 8, 2
    Wr = _t((np.random.default_rng(12).standard_normal((E, HID)) / 4).astype(np.float32))
    blk = MoEBlock(MoERouter(Wr, S), TF._tiny_block(("q4_k", "q4_k", "q6_k"), fused=True, E=E, H=HID, F=256), norm=_norm())
    x, r = _xr(N, seed=5)
    for res in (r, None):
        xd, rd = _t(x), (_t(res) if res is not None else None)
        out, h = blk.forward_normed(xd, rd)
        y = blk.norm(xd, rd)
        y = y[0] if rd is not None else y
        want = blk.forward(y)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(h), RM.h_of(x, res).view(np.uint16))
        assert torch.isfinite(out).all() and float(out.abs().max()) > 0
        assert _same_bits(out, want)


# ---- 7. ----
def test_graph_capture_follows_x_and_residual():
    ffn = _dense()
    N = 16
    x, r = _xr(N, seed=1)
    xd, rd = _t(x), _t(r)
    ffn.forward_normed(xd, rd)  # (first use outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, h = ffn.forward_normed(xd, rd)
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    e_out, e_h = ffn.forward_normed(xd, rd)
    assert _same_bits(first, e_out) and _same_bits(h, e_h)
    x2, r2 = _xr(N, seed=2)
    xd.copy_(_t(x2))
    rd.copy_(_t(r2))
    graph.replay()
    torch.cuda.synchronize()
    e_out, e_h = ffn.forward_normed(xd, rd)
    torch.cuda.synchronize()
    assert _same_bits(out, e_out) and _same_bits(h, e_h)
    assert not _same_bits(out, first)
    assert np.array_equal(_bits(h), RM.h_of(x2, r2).view(np.uint16))


# ---- 8. ----
def test_int8_gemm_form_takes_two_steps_or_refuses(tune):
    import kernels._lib as kl
    tune(GQ_GEMM_I8=1)
    N, K = 33, 4096
    rc_a, a, rc_b, b, yb, two, y = _workspace_pair(kl, N, K, True)
    assert rc_a == EUNSUPPORTED
    assert torch.equal(a, torch.full_like(a, ST.WS_FILL))  # (refused: nothing written)
    assert rc_b == OK
    assert torch.equal(b, two) and _same_bits(yb, y)
    # the int8 form is there: more than the fp16 x~ was written
    assert not torch.equal(two[2 * N * K:], torch.full_like(two[2 * N * K:], ST.WS_FILL))
    # the wrapper does the two steps itself when no y_out is given
    x, r, w = _inputs(N, K)
    _, c, checkc = ST.guarded_ws(_ws_bytes(kl, N, K))
    assert kl.rmsnorm_prepare(_t(x), _t(w), 1e-5, c, residual=_t(r)) is None
    torch.cuda.synchronize()
    checkc()
    assert torch.equal(c, two)
