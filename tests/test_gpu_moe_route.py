"""GPU tests of the MoE router (gq_moe_route, gq_moe_topk: csrc/moe_route.hip; kernels/moe.py
MoERouter, MoEBlock) against the float64 model (tests/moe_route_model.py).

The checks are layered so that each has a bound that follows from what it compares:
  1. the stored logits against the model, gated by torch's own fp32 product on the same inputs;
  2. the ids against the model's stable top-k OF THE STORED LOGITS -- exact, no gap needed;
  3. the weights against the model on the stored logits and the library's ids -- 2^-18 relative in
     fp32 (at most 64 fp32 additions, expf within a few ulp of an argument |L - max| <= 32 rounded
     to fp32, one division, one multiplication), one step in fp16;
  4. end to end from x and Wr: the ids of the model, under the 1e-3 gap asserted on the model's
     logits first, and the weights within 1e-4 relative.
"""
import functools

import numpy as np
import pytest
import torch

import moe_route_model as MR
from gpu_types import dev as _dev, experts as _experts, no_timeouts as _no_timeouts, same_bits as _same_bits
from gpu_types import no_timeouts_after_each_test  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu

FUNCS = {MR.SOFTMAX: "softmax", MR.SIGMOID: "sigmoid"}
F32_REL = 2.0 ** -18


@functools.lru_cache(maxsize=None)
def _routed(E, H, S, N, seed, wr_f16=False):
    """One gq_moe_route call per case (softmax, norm, fp32 weights), shared by the tests that read
    it: (model logits float64, logits, ids, weights as numpy, Wr and x on the device)."""
    import kernels._lib as kl
    Wr, x = MR.inputs(E, H, N, seed)
    Wd = Wr.astype(np.float16) if wr_f16 else Wr
    Wt, xt = torch.from_numpy(np.array(Wd)).to(_dev()), torch.from_numpy(np.array(x)).to(_dev())
    ids, w, lg = kl.moe_route(Wt, xt, S)
    torch.cuda.synchronize()
    assert kl.lib().gq_last_error() == b""  # (the device product, not the fallback)
    out = (MR.logits(Wd, x), lg.cpu().numpy(), ids.cpu().numpy(), w.cpu().numpy())
    for a in out:
        a.setflags(write=False)
    return out + (Wt, xt)


def _rel(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)))


@pytest.mark.parametrize("wr_f16", [False, True])
@pytest.mark.parametrize("E,H,S,N,seed", MR.SHAPES)
def test_logits(E, H, S, N, seed, wr_f16):
    """Measured on the device (E, H, S, N: err, err_ref = torch's fp32 product), fp32 Wr / fp16 Wr:
    see DESIGN.md section 5, "MoE router"."""
    model, lg, _, _, Wt, xt = _routed(E, H, S, N, seed, wr_f16)
    ref = torch.matmul(xt.float(), Wt.float().T)
    torch.cuda.synchronize()
    assert lg.shape == (N, E) and lg.dtype == np.float32
    err_ref = float(np.max(np.abs(ref.cpu().numpy().astype(np.float64) - model)))
    err = float(np.max(np.abs(lg.astype(np.float64) - model)))
    print(f"logits E={E} H={H} N={N} {'fp16' if wr_f16 else 'fp32'} Wr: err {err:.3e}, torch fp32 err_ref {err_ref:.3e}")
    assert err <= 8 * err_ref, (err, err_ref)
    assert 8 * err_ref < 1e-4, err_ref


@pytest.mark.parametrize("func", [MR.SOFTMAX, MR.SIGMOID])
@pytest.mark.parametrize("E,H,S,N,seed", MR.SHAPES)
def test_selection_is_a_function_of_the_stored_logits(E, H, S, N, seed, func):
    import kernels._lib as kl
    _, lg, ids0, _, Wt, xt = _routed(E, H, S, N, seed)
    if func == MR.SOFTMAX:
        ids = ids0
    else:
        it, _, lt = kl.moe_route(Wt, xt, S, func="sigmoid")
        torch.cuda.synchronize()
        assert np.array_equal(lt.cpu().numpy().view(np.uint32), lg.view(np.uint32))
        ids = it.cpu().numpy()
    assert ids.shape == (N, S) and ids.dtype == np.int32
    assert np.array_equal(ids, MR.topk(MR.keys(lg, func), S))


@pytest.mark.parametrize("E,H,S,N,seed", MR.SHAPES)
def test_selection_with_a_bias(E, H, S, N, seed):
    import kernels._lib as kl
    _, lg, _, _, Wt, xt = _routed(E, H, S, N, seed)
    bias = MR.selection_bias(E)
    keys = MR.keys(lg, MR.SIGMOID, bias)
    gap = MR.top_gap(keys, S)
    print(f"E={E} S={S} N={N}: biased key gap {gap:.2e}")
    assert gap >= MR.MIN_KEY_GAP
    it, wt, lt = kl.moe_route(Wt, xt, S, bias=torch.from_numpy(bias).to(_dev()), func="sigmoid", norm=False)
    torch.cuda.synchronize()
    assert np.array_equal(lt.cpu().numpy().view(np.uint32), lg.view(np.uint32))
    ids = it.cpu().numpy()
    assert np.array_equal(ids, MR.topk(keys, S))
    assert E == S or not np.array_equal(ids, MR.topk(lg, S))  # (the bias did move the selection)
    # the bias never enters the value
    assert _rel(wt.cpu().numpy(), MR.weights(lg, ids, MR.SIGMOID, False, 1.0)) <= F32_REL


@pytest.mark.parametrize("func", [MR.SOFTMAX, MR.SIGMOID])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 2.5])
@pytest.mark.parametrize("E,H,S,N,seed", MR.SHAPES)
def test_weights(E, H, S, N, seed, scale, norm, func):
    import kernels._lib as kl
    _, lg, _, _, _, _ = _routed(E, H, S, N, seed)
    lt = torch.from_numpy(np.array(lg)).to(_dev())
    for w_dtype in (torch.float32, torch.float16):
        it, wt = kl.moe_topk(lt, S, func=FUNCS[func], norm=bool(norm), scale=scale, w_dtype=w_dtype)
        torch.cuda.synchronize()
        ids, w = it.cpu().numpy(), wt.cpu().numpy()
        assert np.array_equal(ids, MR.topk(MR.keys(lg, func), S))
        want = MR.weights(lg, ids, func, bool(norm), scale)
        assert w.shape == (N, S) and np.isfinite(w).all()
        if w_dtype == torch.float32:
            assert w.dtype == np.float32
            rel = _rel(w, want)
            assert rel <= F32_REL, rel
        else:
            assert w.dtype == np.float16
            # (a value below fp16's normal range would still be within a step; none is that small
            # except softmax tails, which the step count covers too)
            assert int(MR.ulp16(w, want.astype(np.float16)).max()) <= 1


@pytest.mark.parametrize("E,H,S,N,seed", MR.SHAPES)
def test_end_to_end(E, H, S, N, seed):
    model, _, ids, w, _, _ = _routed(E, H, S, N, seed)
    gap = MR.top_gap(model, S)
    print(f"E={E} H={H} S={S} N={N}: model logit gap {gap:.2e}")
    assert gap >= MR.MIN_GAP
    want_ids, want_w = MR.route(model, S)
    assert np.array_equal(ids, want_ids)
    rel = _rel(w, want_w)
    assert rel <= 1e-4, rel


# ---- gq_moe_topk on hand-made logits ----
def _topk(L, S, **kw):
    import kernels._lib as kl
    it, wt = kl.moe_topk(torch.from_numpy(np.asarray(L, np.float32)).to(_dev()), S, **kw)
    torch.cuda.synchronize()
    return it.cpu().numpy(), wt.cpu().numpy()


def test_topk_duplicates_give_the_lower_index_first():
    L = np.zeros((3, 130), np.float32)
    L[0, [7, 64, 65, 129]] = 2.0
    L[1, :] = 1.0
    L[2, [100, 3]] = [5.0, 5.0]
    L[2, 70] = -0.0
    ids, w = _topk(L, 4)
    assert ids.tolist() == [[7, 64, 65, 129], [0, 1, 2, 3], [3, 100, 0, 1]]
    assert np.allclose(w[:2], 0.25, rtol=1e-6)
    ids, _ = _topk(L, 4, func="sigmoid")
    assert ids.tolist() == [[7, 64, 65, 129], [0, 1, 2, 3], [3, 100, 0, 1]]


def test_topk_nan_and_inf_rows_give_valid_ids():
    E, S = 70, 6
    L = np.random.default_rng(9).standard_normal((4, E)).astype(np.float32)
    L[0, [2, 68]] = np.nan
    L[0, 5], L[0, 66] = np.inf, -np.inf
    L[1, :] = np.nan
    L[2, :] = -np.inf
    L[3, : E - 3] = np.nan  # fewer numbers than slots: the NaN entries fill the rest, last
    L[3, E - 1] = np.inf
    for func in ("softmax", "sigmoid"):
        ids, _ = _topk(L, S, func=func)
        assert ids.min() >= 0 and ids.max() < E
        assert all(len(set(r)) == S for r in ids.tolist())
        assert np.array_equal(ids, MR.topk(L, S))
    assert ids[0, 0] == 5 and not {2, 68, 66} & set(ids[0].tolist())
    assert ids[1].tolist() == list(range(S))
    assert ids[3, 0] == E - 1 and set(ids[3, 1:3].tolist()) == {E - 3, E - 2} and ids[3, 3:].tolist() == [0, 1, 2]
    E = 40  # S == E: every expert once, -inf before the NaN entries, those last by index
    L = np.random.default_rng(10).standard_normal((2, E)).astype(np.float32)
    L[0, [30, 2]] = np.nan
    L[0, 17] = -np.inf
    ids, _ = _topk(L, E)
    assert all(sorted(r) == list(range(E)) for r in ids.tolist())
    assert ids[0, -3:].tolist() == [17, 2, 30]
    assert np.array_equal(ids, MR.topk(L, E))


def test_topk_single_expert():
    for func in ("softmax", "sigmoid"):
        ids, w = _topk([[0.3], [-4.0]], 1, func=func, norm=True, scale=2.5)
        assert ids.tolist() == [[0], [0]] and w.tolist() == [[2.5], [2.5]]
    ids, w = _topk([[0.3]], 1, norm=False, scale=2.5)
    assert w.tolist() == [[2.5]]  # softmax over one expert


def test_topk_any_token_count_and_row_stride():
    import kernels._lib as kl
    N, E, S = 300, 60, 4
    L = np.random.default_rng(11).standard_normal((N, E + 7)).astype(np.float32) * 2
    wide = torch.from_numpy(L).to(_dev())
    view = wide[:, :E]
    assert view.stride(0) == E + 7
    out = (torch.full((N, S), -1, dtype=torch.int32, device=_dev()), torch.full((N, S), -1.0, device=_dev()))
    it, wt = kl.moe_topk(view, S, out=out)
    torch.cuda.synchronize()
    assert it.data_ptr() == out[0].data_ptr() and wt.data_ptr() == out[1].data_ptr()
    want_ids, want_w = MR.route(L[:, :E], S)
    assert np.array_equal(it.cpu().numpy(), want_ids)
    assert _rel(wt.cpu().numpy(), want_w) <= F32_REL
    # the C entry with ldl > E reads the same rows
    ids2 = torch.empty((N, S), dtype=torch.int32, device=_dev())
    w2 = torch.empty((N, S), dtype=torch.float32, device=_dev())
    rc = kl.lib().gq_moe_topk(wide.data_ptr(), E + 7, None, 0, 1, 1.0, ids2.data_ptr(), w2.data_ptr(), 1, N, E, S, None)
    torch.cuda.synchronize()
    assert rc == 0, kl.lib().gq_last_error()
    assert torch.equal(ids2, it) and torch.equal(w2, wt)


# ---- a token's result is its own ----
@pytest.mark.parametrize("wr_f16", [False, True])
def test_token_independence_and_determinism(wr_f16):
    import kernels._lib as kl
    E, H, S, N, seed = 8, 4096, 2, 64, 0
    _, lg, ids, w, Wt, xt = _routed(E, H, S, N, seed, wr_f16)
    i2, w2, l2 = kl.moe_route(Wt, xt, S)
    torch.cuda.synchronize()
    assert np.array_equal(l2.cpu().numpy().view(np.uint32), lg.view(np.uint32))
    assert np.array_equal(i2.cpu().numpy(), ids) and np.array_equal(w2.cpu().numpy().view(np.uint32), w.view(np.uint32))
    for n in (0, 1, 7, 8, 37, 63):
        i1, w1, l1 = kl.moe_route(Wt, xt[n:n + 1], S)
        torch.cuda.synchronize()
        assert np.array_equal(l1.cpu().numpy().view(np.uint32), lg[n:n + 1].view(np.uint32)), n
        assert np.array_equal(i1.cpu().numpy(), ids[n:n + 1]), n
        assert np.array_equal(w1.cpu().numpy().view(np.uint32), w[n:n + 1].view(np.uint32)), n
    # every tile size of the product (1, 2, 4 and 8 tokens a pass) gives a token the same bits
    for n0, cnt in ((10, 2), (20, 3), (30, 5)):
        _, _, lc = kl.moe_route(Wt, xt[n0:n0 + cnt], S)
        torch.cuda.synchronize()
        assert np.array_equal(lc.cpu().numpy().view(np.uint32), lg[n0:n0 + cnt].view(np.uint32)), (n0, cnt)


# ---- what the entry refuses ----
@pytest.mark.parametrize("E,H,S,N,what", [(8, 256, 2, 65, b"N=65"), (8, 48, 2, 3, b"H=48")])
def test_fallback_to_the_torch_product(E, H, S, N, what):
    import kernels._lib as kl
    Wr, x = MR.inputs(E, H, N, 0)
    Wt, xt = torch.from_numpy(np.array(Wr)).to(_dev()), torch.from_numpy(np.array(x)).to(_dev())
    buf = torch.full((N, S), -5, dtype=torch.int32, device=_dev())
    rc = kl.lib().gq_moe_route(Wt.data_ptr(), 0, xt.data_ptr(), H, Wt.data_ptr(), E, None, 0, 1, 1.0, buf.data_ptr(),
                               buf.data_ptr(), 1, N, E, H, S, None)
    torch.cuda.synchronize()
    assert rc == kl.GQ_EUNSUPPORTED and torch.all(buf == -5)  # nothing launched, nothing written
    ids, w, lg = kl.moe_route(Wt, xt, S)
    torch.cuda.synchronize()
    assert what in kl.lib().gq_last_error(), kl.lib().gq_last_error()
    model = MR.logits(Wr, x)
    assert MR.top_gap(model, S) >= MR.MIN_GAP
    assert float(np.max(np.abs(lg.cpu().numpy() - model))) < 1e-4
    want_ids, want_w = MR.route(model, S)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert _rel(w.cpu().numpy(), want_w) <= 1e-4


def test_torch_only_definition_beyond_the_limits():
    """E > 1024: gq_moe_topk refuses, moe_topk answers with the documented torch definition."""
    import kernels._lib as kl
    N, E, S = 3, 1100, 5
    L = np.random.default_rng(13).standard_normal((N, E)).astype(np.float32)
    L[0, [40, 1090]] = 9.0
    ids, w = _topk(L, S)
    assert b"1024" in kl.lib().gq_last_error()
    want_ids, want_w = MR.route(L, S)
    assert np.array_equal(ids, want_ids) and ids[0, :2].tolist() == [40, 1090]
    assert _rel(w, want_w) <= 1e-5


# ---- the block ----
def _block_file(tmp):
    from gguf.file import write_gguf
    E, S, H, F = 4, 2, 512, 256
    parts = zip(("ffn_gate_exps", "ffn_up_exps", "ffn_down_exps"), ("q4_k", "q4_k", "q6_k"), ((F, H), (F, H), (H, F)))
    tensors = {f"blk.2.{n}.weight": (t, (E, M, K), _experts(t, E, M, K, i + 1)) for i, (n, t, (M, K)) in enumerate(parts)}
    tensors["blk.2.ffn_gate_inp.weight"] = ("f32", (E, H), MR.inputs(E, H, 1, 0)[0] * np.float32(16))  # (logits of order 1)
    meta = {"general.architecture": "llama", "llama.expert_count": E, "llama.expert_used_count": S}
    path = str(tmp / "block.gguf")
    write_gguf(path, tensors, metadata=meta)
    return path


@pytest.fixture(scope="module")
def block(tmp_path_factory):
    from gguf.file import read_gguf
    from kernels.moe import MoEBlock
    meta, tensors = read_gguf(_block_file(tmp_path_factory.mktemp("moe_block")))
    b = MoEBlock.from_gguf(meta, tensors, 2, _dev())
    assert b.ffn.fused and (b.router.E, b.router.H, b.router.S, b.router.func, b.router.norm) == (4, 512, 2, "softmax", True)
    return b


def _block_x(N, seed):
    from utils.synth import random_activations
    # (scaled as tests/test_gpu_moe_fused.py scales: silu(g) * u stays in fp16 range)
    return torch.from_numpy(random_activations(N, 512, seed=seed) / np.float16(16)).to(_dev())


@pytest.mark.parametrize("N", [1, 3, 40])
def test_block_is_the_composition(block, N):
    from kernels.moe import MoEFFN
    x = _block_x(N, 21 + N)
    y = block.forward(x)
    ids, w = block.router(x)
    want = MoEFFN(block.ffn.gate, block.ffn.up, block.ffn.down, fused=True).forward(x, ids, w)
    torch.cuda.synchronize()
    assert y.shape == (N, 512) and y.dtype == torch.float16
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0
    assert _same_bits(y, want)
    model = MR.logits(block.router.Wr.cpu().numpy(), x.cpu().numpy())
    if MR.top_gap(model, 2) >= MR.MIN_GAP:
        assert np.array_equal(ids.cpu().numpy(), MR.route(model, 2)[0])
    _no_timeouts()


@pytest.mark.parametrize("N", [1, 3, 40])
def test_block_graph_replay_follows_x(block, N):
    x = _block_x(N, 31 + N)
    block.forward(x)  # (first use outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = block.forward(x)
    graph.replay()
    torch.cuda.synchronize()
    first, ids_first = y.clone(), block.router(x)[0].clone()
    assert _same_bits(first, block.forward(x))
    x.copy_(_block_x(N, 77 + N))
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(y, block.forward(x))
    assert not _same_bits(y, first)
    assert not torch.equal(block.router(x)[0], ids_first)  # (the replay routed the new x)
    _no_timeouts()
