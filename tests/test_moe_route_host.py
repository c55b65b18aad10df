"""Host side of the MoE router (gq_moe_topk, gq_moe_route; kernels/moe.py MoERouter, MoEBlock): the
numpy model the GPU tests judge by (tests/moe_route_model.py) on hand-worked cases and on the test
shapes' gaps, both symbols exported and bound, their argument checks (fake pointers: every case
returns before a launch), and MoERouter.from_gguf on written files.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch

import moe_route_model as MR

OK, EINVAL, EUNSUPPORTED = 0, 1, 3


# ---- the model ----
def test_model_ties_resolve_to_the_lower_index():
    L = np.array([[1.0, 3.0, 3.0, 0.5, 3.0], [2.0, 2.0, 2.0, 2.0, 2.0]])
    assert MR.topk(L, 3).tolist() == [[1, 2, 4], [0, 1, 2]]
    assert MR.topk(L, 5).tolist() == [[1, 2, 4, 0, 3], [0, 1, 2, 3, 4]]
    assert MR.topk(np.array([[0.0, -0.0, 1.0]]), 3).tolist() == [[2, 0, 1]]


def test_model_nan_ranks_last():
    L = np.array([[np.nan, -np.inf, 1.0, np.nan, np.inf, -2.0]])
    assert MR.topk(L, 6).tolist() == [[4, 2, 5, 1, 0, 3]]


def test_model_bias_moves_the_selection_not_the_value():
    L = np.array([[2.0, 1.0, 0.0, -1.0]])
    ids, w = MR.route(L, 2, MR.SIGMOID, norm=False)
    assert ids.tolist() == [[0, 1]]
    bias = np.array([-0.5, 0.0, 0.0, 0.6])  # keys: .381, .731, .5, .869
    ids_b, w_b = MR.route(L, 2, MR.SIGMOID, norm=False, bias=bias)
    assert ids_b.tolist() == [[3, 1]]
    s = 1.0 / (1.0 + np.exp(-L[0]))
    assert np.allclose(w_b[0], [s[3], s[1]], rtol=1e-15)  # the values carry no bias
    assert np.allclose(w[0], [s[0], s[1]], rtol=1e-15)


def test_model_norm_and_scale():
    rng = np.random.default_rng(5)
    L = rng.standard_normal((7, 12))
    for func in (MR.SOFTMAX, MR.SIGMOID):
        _, w = MR.route(L, 4, func, norm=True)
        assert np.allclose(w.sum(1), 1.0, rtol=1e-14)
        _, w25 = MR.route(L, 4, func, norm=True, scale=2.5)
        assert np.allclose(w25, 2.5 * w, rtol=1e-15)
        _, raw = MR.route(L, 4, func, norm=False)
        assert np.all(raw.sum(1) < 4) and np.all(raw > 0)
    _, w1 = MR.route(L[:, :1], 1, MR.SOFTMAX, norm=True, scale=2.5)
    assert np.all(w1 == 2.5)


def test_model_renormalised_softmax_is_the_softmax_of_the_selected():
    rng = np.random.default_rng(6)
    L = rng.standard_normal((5, 16)) * 3
    ids, w = MR.route(L, 4, MR.SOFTMAX, norm=True)
    sel = np.take_along_axis(L, ids.astype(np.int64), axis=1)
    p = np.exp(sel - sel.max(1, keepdims=True))
    assert np.allclose(w, p / p.sum(1, keepdims=True), rtol=1e-13)
    assert np.all(np.diff(sel, axis=1) <= 0)  # descending key order


def test_model_ulp16():
    assert MR.ulp16(np.float16(1.0), np.float16(1.0009765625)) == 1
    assert MR.ulp16(np.float16(-0.0), np.float16(0.0)) == 0


@pytest.mark.parametrize("E,H,S,N,seed", MR.SHAPES)
def test_shapes_keep_their_gaps(E, H, S, N, seed):
    """What the GPU tests rely on, checked where it is cheap: the float64 logits of every shape keep
    MIN_GAP between neighbours among the top S + 1 (for an fp16 router matrix too), and with the
    selection bias the sigmoid keys keep MIN_KEY_GAP."""
    Wr, x = MR.inputs(E, H, N, seed)
    L = MR.logits(Wr, x)
    gap = MR.top_gap(L, S)
    gap16 = MR.top_gap(MR.logits(Wr.astype(np.float16), x), S)
    kgap = MR.top_gap(MR.keys(L, MR.SIGMOID, MR.selection_bias(E)), S)
    print(f"E={E} H={H} S={S} N={N}: logit gap {gap:.2e} (fp16 Wr {gap16:.2e}), biased key gap {kgap:.2e}")
    assert gap >= MR.MIN_GAP
    assert kgap >= MR.MIN_KEY_GAP


# ---- the ABI ----
def test_symbols_and_version():
    import kernels._lib as kl
    L = kl.lib()
    assert hasattr(L, "gq_moe_topk") and hasattr(L, "gq_moe_route")
    argtypes, restype = kl.SIGNATURES["gq_moe_topk"]
    assert len(argtypes) == 13 and restype is ctypes.c_int and argtypes[5] is ctypes.c_float
    argtypes, restype = kl.SIGNATURES["gq_moe_route"]
    assert len(argtypes) == 18 and restype is ctypes.c_int and argtypes[9] is ctypes.c_float
    assert L.gq_version() == 105  # (the entries are detected by their symbols)


def test_topk_argument_checks():
    import kernels._lib as kl
    L = kl.lib()
    p = ctypes.c_void_p(16)

    def call(logits=p, ldl=8, bias=None, func=0, norm=1, scale=1.0, ids=p, W=p, f32=1, N=2, E=8, S=2):
        return L.gq_moe_topk(logits, ldl, bias, func, norm, scale, ids, W, f32, N, E, S, None)

    for name in ("logits", "ids", "W"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null" in L.gq_last_error()
    for name in ("N", "E", "S"):
        assert call(**{name: -1}) == EINVAL, name
        assert b"negative" in L.gq_last_error()
    assert call(ldl=7) == EINVAL
    assert b"ldl" in L.gq_last_error()
    assert call(func=2) == EINVAL
    assert call(func=-1) == EINVAL
    assert call(func=0, bias=p) == EINVAL
    assert b"bias" in L.gq_last_error()
    assert call(E=1025, ldl=1025) == EUNSUPPORTED
    assert b"1024" in L.gq_last_error()
    assert call(E=128, ldl=128, S=65) == EUNSUPPORTED
    assert b"64" in L.gq_last_error()
    assert call(S=9) == EUNSUPPORTED  # S > E
    assert call(S=0) == EUNSUPPORTED
    assert call(E=0, S=0, ldl=0) == EUNSUPPORTED
    # the order: a bad argument is reported before a refused shape, an empty call before either
    assert call(E=1025, ldl=8) == EINVAL
    assert call(E=1025, ldl=1025, func=3) == EINVAL
    assert call(logits=None, ids=None, W=None, N=0) == OK
    assert call(logits=None, ids=None, W=None, N=0, E=5000, S=100, func=7) == OK
    assert L.gq_last_error() == b""


def test_route_argument_checks():
    import kernels._lib as kl
    L = kl.lib()
    p = ctypes.c_void_p(16)

    def call(Wr=p, f16=0, X=p, ldx=64, logits=p, ldl=8, bias=None, func=0, norm=1, scale=1.0, ids=p, W=p, f32=1, N=2, E=8,
             H=64, S=2):
        return L.gq_moe_route(Wr, f16, X, ldx, logits, ldl, bias, func, norm, scale, ids, W, f32, N, E, H, S, None)

    for name in ("Wr", "X", "logits", "ids", "W"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null" in L.gq_last_error()
    for name in ("N", "E", "S", "H"):
        assert call(**{name: -1}) == EINVAL, name
        assert b"negative" in L.gq_last_error()
    assert call(ldl=7) == EINVAL
    assert call(ldx=63) == EINVAL
    assert b"ldx" in L.gq_last_error()
    assert call(func=2) == EINVAL
    assert call(bias=p) == EINVAL
    assert call(E=1025, ldl=1025) == EUNSUPPORTED
    assert call(E=128, ldl=128, S=65) == EUNSUPPORTED
    assert call(S=9) == EUNSUPPORTED
    assert call(N=65) == EUNSUPPORTED
    assert b"64" in L.gq_last_error()
    assert call(H=48, ldx=48) == EUNSUPPORTED
    assert b"32" in L.gq_last_error()
    assert call(N=65, ldx=63) == EINVAL  # (a bad argument before a refused shape)
    none = dict(Wr=None, X=None, logits=None, ids=None, W=None)
    assert call(N=0, **none) == OK
    assert call(N=0, H=48, E=5000, **none) == OK
    assert L.gq_last_error() == b""


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    import kernels._lib as kl
    with pytest.raises(RuntimeError, match="ROCm device"):
        kl.moe_topk(torch.zeros(2, 8), 2)
    with pytest.raises(RuntimeError, match="ROCm device"):
        kl.moe_route(torch.zeros(8, 64), torch.zeros(2, 64, dtype=torch.float16), 2)


# ---- MoERouter.from_gguf ----
def _write(tmp_path, meta, E=4, H=64, router_type="f32", extra=None, name="r.gguf"):
    from gguf.file import read_gguf, write_gguf
    Wr = (np.random.default_rng(2).standard_normal((E, H)) / 8).astype(np.float32 if router_type == "f32" else np.float16)
    tensors = {"blk.3.ffn_gate_inp.weight": (router_type, (E, H), Wr)}
    tensors.update(extra or {})
    path = str(tmp_path / name)
    write_gguf(path, tensors, metadata=meta)
    return Wr, read_gguf(path)


def test_router_from_gguf_reads_the_fields(tmp_path):
    from kernels.moe import MoERouter
    E, H = 4, 64
    bias = np.array([0.1, -0.1, 0.05, 0.0], np.float32)
    meta = {"general.architecture": "deepseek2", "deepseek2.expert_count": E, "deepseek2.expert_used_count": 2,
            "deepseek2.expert_gating_func": 2, "deepseek2.expert_weights_norm": True, "deepseek2.expert_weights_scale": 2.5}
    Wr, (m, t) = _write(tmp_path, meta, extra={"blk.3.exp_probs_b.bias": ("f32", (1, E), bias)})
    assert t["blk.3.ffn_gate_inp.weight"].dims == (H, E)
    r = MoERouter.from_gguf(m, t, 3, "cpu")
    assert (r.E, r.H, r.S, r.func, r.norm, r.scale) == (E, H, 2, "sigmoid", True, 2.5)
    assert r.Wr.dtype == torch.float32 and np.array_equal(r.Wr.numpy(), Wr)
    assert r.bias.dtype == torch.float32 and np.array_equal(r.bias.numpy(), bias)
    Wh, (m, t) = _write(tmp_path, {**meta, "deepseek2.expert_weights_norm": False}, router_type="f16", name="h.gguf")
    r = MoERouter.from_gguf(m, t, 3, "cpu")
    assert r.Wr.dtype == torch.float16 and np.array_equal(r.Wr.numpy(), Wh) and r.bias is None and r.norm is False


def test_router_from_gguf_defaults(tmp_path):
    from kernels.moe import MoERouter
    meta = {"general.architecture": "llama", "llama.expert_count": 4, "llama.expert_used_count": 2}
    _, (m, t) = _write(tmp_path, meta)
    r = MoERouter.from_gguf(m, t, 3, "cpu")
    assert (r.S, r.func, r.norm, r.scale, r.bias) == (2, "softmax", True, 1.0, None)
    _, (m, t) = _write(tmp_path, {**meta, "llama.expert_gating_func": 0, "llama.expert_weights_scale": 0.0}, name="z.gguf")
    r = MoERouter.from_gguf(m, t, 3, "cpu")
    assert (r.func, r.norm, r.scale) == ("softmax", True, 1.0)
    _, (m, t) = _write(tmp_path, {**meta, "llama.expert_gating_func": 1}, name="s.gguf")
    assert MoERouter.from_gguf(m, t, 3, "cpu").func == "softmax"
    _, (m, t) = _write(tmp_path, {**meta, "llama.expert_gating_func": 2}, name="g.gguf")
    r = MoERouter.from_gguf(m, t, 3, "cpu")
    assert (r.func, r.norm) == ("sigmoid", False)


def test_router_from_gguf_refusals(tmp_path):
    from kernels.moe import MoEBlock, MoERouter
    meta = {"general.architecture": "llama", "llama.expert_count": 4, "llama.expert_used_count": 2}
    _, (m, t) = _write(tmp_path, {**meta, "llama.expert_count": 8}, name="a.gguf")
    with pytest.raises(ValueError, match="expert_count"):
        MoERouter.from_gguf(m, t, 3, "cpu")
    for missing in ("llama.expert_used_count", "llama.expert_count"):
        _, (m, t) = _write(tmp_path, {k: v for k, v in meta.items() if k != missing}, name="b.gguf")
        with pytest.raises(ValueError, match=missing.split(".")[1]):
            MoERouter.from_gguf(m, t, 3, "cpu")
    _, (m, t) = _write(tmp_path, {**meta, "llama.expert_gating_func": 3}, name="c.gguf")
    with pytest.raises(ValueError, match="gating_func"):
        MoERouter.from_gguf(m, t, 3, "cpu")
    _, (m, t) = _write(tmp_path, {**meta, "llama.expert_used_count": 5}, name="d.gguf")
    with pytest.raises(ValueError, match="S=5"):
        MoERouter.from_gguf(m, t, 3, "cpu")
    _, (m, t) = _write(tmp_path, meta, name="e.gguf")
    with pytest.raises(KeyError):
        MoERouter.from_gguf(m, t, 2, "cpu")  # no such layer
    shexp = {"blk.3.ffn_up_shexp.weight": ("f32", (8, 64), np.zeros((8, 64), np.float32))}
    _, (m, t) = _write(tmp_path, meta, extra=shexp, name="f.gguf")
    with pytest.raises(NotImplementedError, match="blk.3.ffn_up_shexp.weight"):
        MoERouter.from_gguf(m, t, 3, "cpu")
    with pytest.raises(NotImplementedError, match="ffn_up_shexp"):
        MoEBlock.from_gguf(m, t, 3, "cpu")


def test_router_argument_checks():
    from kernels.moe import MoERouter
    Wr = torch.zeros(4, 64)
    with pytest.raises(ValueError):
        MoERouter(Wr, 5)
    with pytest.raises(ValueError):
        MoERouter(Wr, 2, func="tanh")
    with pytest.raises(ValueError, match="bias"):
        MoERouter(Wr, 2, bias=torch.zeros(4))  # softmax gating takes none
    with pytest.raises(ValueError):
        MoERouter(Wr, 2, bias=torch.zeros(3), func="sigmoid")
    with pytest.raises(ValueError):
        MoERouter(Wr.double(), 2)
