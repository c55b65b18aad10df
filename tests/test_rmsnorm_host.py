"""Host side of the fused residual add + RMSNorm (gq_rmsnorm, gq_rmsnorm_prepare; kernels/norm.py
RMSNorm, DenseFFN / MoEBlock.forward_normed): the numpy model the GPU tests judge by
(tests/rmsnorm_model.py), both symbols exported and bound, every argument check (fake pointers:
each case returns before a launch), RMSNorm.from_gguf on written files.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch

import rmsnorm_model as RM

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
MB = 1 << 20
# fake device addresses, far enough apart that no tensor below reaches the next one's
X, R, H, W, Y, WS = (ctypes.c_void_p(i * MB) for i in range(1, 7))
N, K = 4, 64


def at(base, byte_offset):
    return ctypes.c_void_p(base.value + byte_offset)


# ---- the model ----
def test_model_h_is_the_correctly_rounded_sum():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((3, 4096)) * 37).astype(np.float16)
    r = rng.standard_normal((3, 4096)).astype(np.float16)
    want = (x.astype(np.float64) + r.astype(np.float64)).astype(np.float16)  # fp64 holds the sum exactly
    assert np.array_equal(RM.h_of(x, r).view(np.uint16), want.view(np.uint16))
    assert np.array_equal(RM.h_of(x).view(np.uint16), x.view(np.uint16))


def test_model_y_on_hand_worked_rows():
    h = np.array([[3.0, -4.0] * 16, [0.0] * 32], np.float16)   # mean(h^2) = 12.5, 0
    w = np.full(32, 2.0, np.float32)
    y = RM.y_ideal(h, w, 0.0)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(y[0], (h[0].astype(np.float64) / np.sqrt(12.5) * 2).astype(np.float16))
    assert np.isnan(y[1]).all()                                 # 0 / sqrt(0): eps = 0 is the caller's risk
    assert not RM.y_ideal(h, w, 1e-6)[1].any()                  # an all-zero row with eps gives zeros
    assert RM.y_ideal(h, w, 1e-6)[0, 0] == np.float16(3 / np.sqrt(12.5 + np.float64(np.float32(1e-6))) * 2)


def test_ulp_dist():
    f = lambda *v: np.array(v, np.float16)
    one = np.array([0x3C00, 0x3C01, 0x3BFF, 0x0001, 0x8001, 0x0000, 0x8000], np.uint16).view(np.float16)
    assert RM.ulp_dist(one[:3], f(1, 1, 1)).tolist() == [0, 1, 1]
    assert RM.ulp_dist(one[3:5], one[[4, 3]]).tolist() == [2, 2]      # across zero: +tiny .. -tiny
    assert RM.ulp_dist(one[5:7], one[[6, 5]]).tolist() == [0, 0]      # -0 is +0
    assert RM.ulp_dist(f(65504), f(np.inf)).tolist() == [1]


# ---- the symbols ----
def test_symbols_are_exported_and_bound():
    import kernels._lib as kl
    L = kl.lib()
    for name in ("gq_rmsnorm", "gq_rmsnorm_prepare"):
        assert name in kl.SIGNATURES and hasattr(L, name)
        assert getattr(L, name).argtypes == kl.SIGNATURES[name][0]
    assert L.gq_version() == 105
    assert callable(kl.rmsnorm) and callable(kl.rmsnorm_prepare)


def _norm(L, x=X, r=None, h=None, w=W, eps=1e-5, y=Y, n=N, k=K, ldx=K, ldr=K, ldh=K, ldy=K):
    return L.gq_rmsnorm(x, r, h, w, eps, y, n, k, ldx, ldr, ldh, ldy, None)


def _prep(L, x=X, r=None, h=None, w=W, eps=1e-5, y=None, n=N, k=K, ldx=K, ldr=K, ldh=K, ldy=K, ws=WS, nbytes=MB):
    return L.gq_rmsnorm_prepare(x, r, h, w, eps, y, n, k, ldx, ldr, ldh, ldy, ws, nbytes, None)


# Each case: keyword overrides of a valid call, the status, a piece of the error text.
REFUSED = [
    ("K % 32", dict(k=40, ldx=40, ldy=40), EINVAL, b"multiple of 32"),
    ("ldx < K", dict(ldx=K - 1), EINVAL, b"ldx"),
    ("ldr < K", dict(r=R, ldr=K - 8), EINVAL, b"ldr"),
    ("ldh < K", dict(h=H, ldh=K - 8), EINVAL, b"ldh"),
    ("ldy < K", dict(y=Y, ldy=K - 2), EINVAL, b"ldy"),
    ("null X", dict(x=None), EINVAL, b"null"),
    ("null w", dict(w=None), EINVAL, b"null"),
    ("negative N", dict(n=-1), EINVAL, b"negative"),
    ("negative K", dict(k=-32), EINVAL, b"negative"),
    ("eps < 0", dict(eps=-1e-6), EINVAL, b"eps"),
    ("eps NaN", dict(eps=float("nan")), EINVAL, b"eps"),
    ("eps inf", dict(eps=float("inf")), EINVAL, b"eps"),
    ("Y is X", dict(y=X), EINVAL, b"Y overlaps"),
    ("Y ends inside X", dict(y=at(X, -2 * (3 * K + K) + 2)), EINVAL, b"Y overlaps"),
    ("Y is R", dict(r=R, y=R), EINVAL, b"Y overlaps"),
    ("Y is H", dict(h=H, y=H), EINVAL, b"Y overlaps"),
    ("Y in the pad columns of a wide H", dict(h=H, ldh=2 * K, y=at(H, 2 * K), ldy=2 * K), EINVAL, b"Y overlaps"),
    ("H one row into X", dict(h=at(X, 2 * K)), EINVAL, b"H overlaps X"),
    ("H at X with another stride", dict(h=X, ldh=K + 8), EINVAL, b"H overlaps X"),
    ("H one element into R", dict(r=R, h=at(R, 2)), EINVAL, b"H overlaps R"),
]


@pytest.mark.parametrize("entry", ["norm", "prepare"])
@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_argument_checks_refuse_before_a_launch(entry, case):
    import kernels._lib as kl
    L = kl.lib()
    _, kw, status, text = case
    kw = dict(kw)
    if entry == "prepare":
        kw.setdefault("y", Y)  # (given, so that the Y cases mean the same)
    rc = (_norm if entry == "norm" else _prep)(L, **kw)
    assert rc == status, L.gq_last_error()
    assert text in L.gq_last_error(), L.gq_last_error()


def test_norm_needs_y_and_prepare_does_not():
    import kernels._lib as kl
    L = kl.lib()
    assert _norm(L, y=None) == EINVAL and b"null" in L.gq_last_error()
    # prepare with Y NULL gets as far as the workspace check
    assert _prep(L, y=None, nbytes=0) == EINVAL and b"workspace" in L.gq_last_error()


def test_workspace_checks():
    import kernels._lib as kl
    L = kl.lib()
    for n, k in ((4, 256), (4, 4096), (5, 256), (33, 4096)):
        need = L.gq_mmq_workspace_size(2, 64, n, k)
        assert need > 0
        # the entry needs the activation part only: the whole size passes the check (refused later
        # or not at all, never for its size), one byte of nothing does not
        assert _prep(L, n=n, k=k, ldx=k, ws=None, nbytes=need) == EINVAL and b"workspace" in L.gq_last_error()
        assert _prep(L, n=n, k=k, ldx=k, nbytes=0) == EINVAL and b"workspace" in L.gq_last_error()
        assert _prep(L, n=n, k=k, ldx=k, nbytes=n * k) == EINVAL and b"workspace" in L.gq_last_error()
        text = L.gq_last_error().decode()
        act = int(text.rsplit(" ", 1)[1])  # "... < required <need>": the activation part
        assert n * k < act <= need
        assert _prep(L, n=n, k=k, ldx=k, nbytes=act - 1) == EINVAL
    # a workspace over X, R, H or Y
    assert _prep(L, ws=at(X, 64)) == EINVAL and b"workspace overlaps" in L.gq_last_error()
    assert _prep(L, r=R, ws=R) == EINVAL and b"workspace overlaps" in L.gq_last_error()
    assert _prep(L, h=H, ws=at(H, -128)) == EINVAL and b"workspace overlaps" in L.gq_last_error()
    assert _prep(L, y=Y, ws=at(Y, 2 * K)) == EINVAL and b"workspace overlaps" in L.gq_last_error()


def test_empty_calls_are_no_ops():
    import kernels._lib as kl
    L = kl.lib()
    assert _norm(L, n=0) == OK and _prep(L, n=0) == OK
    assert _norm(L, k=0, ldx=0, ldy=0) == OK and _prep(L, k=0, ldx=0) == OK
    assert L.gq_rmsnorm(None, None, None, None, 1e-5, None, 0, 64, 64, 64, 64, 64, None) == OK
    assert L.gq_rmsnorm_prepare(None, None, None, None, 1e-5, None, 0, 64, 64, 64, 64, 64, None, 0, None) == OK
    # ... but their sizes and eps are still checked
    assert _norm(L, n=0, k=40) == EINVAL and _prep(L, n=0, eps=-1.0) == EINVAL


def test_wrapper_refuses_host_tensors_and_bad_shapes():
    import kernels._lib as kl
    x = torch.zeros(2, 64, dtype=torch.float16)
    w = torch.ones(64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        kl.rmsnorm(x, w, 1e-5)
    with pytest.raises(RuntimeError, match="ROCm device"):
        kl.rmsnorm_prepare(x, w, 1e-5, torch.zeros(1 << 16, dtype=torch.uint8))


# ---- RMSNorm ----
def _write(tmp_path, meta, wtype="f32", shape=(64,), name="n.gguf", tname="blk.3.ffn_norm.weight"):
    from gguf.file import read_gguf, write_gguf
    w = (1 + 0.3 * np.random.default_rng(4).standard_normal(int(np.prod(shape)))).astype(
        np.float32 if wtype == "f32" else np.float16)
    path = str(tmp_path / name)
    write_gguf(path, {tname: (wtype, shape, w)}, metadata=meta)
    return w, read_gguf(path)


META = {"general.architecture": "llama", "llama.attention.layer_norm_rms_epsilon": 1e-5}


def test_rmsnorm_from_gguf_reads_weight_and_eps(tmp_path):
    from kernels.norm import RMSNorm
    w, (meta, tensors) = _write(tmp_path, META)
    assert tensors["blk.3.ffn_norm.weight"].dims == (64,)
    n = RMSNorm.from_gguf(meta, tensors, "blk.3.ffn_norm", device="cpu")
    assert n.K == 64 and n.weight.dtype == torch.float32 and np.array_equal(n.weight.numpy(), w)
    assert n.eps == float(np.float32(1e-5))
    w2, (meta, tensors) = _write(tmp_path, META, tname="output_norm.weight", name="o.gguf")
    assert RMSNorm.from_gguf(meta, tensors, "output_norm", device="cpu").K == 64


def test_rmsnorm_from_gguf_refusals(tmp_path):
    from kernels.norm import RMSNorm
    _, (meta, tensors) = _write(tmp_path, META, wtype="f16", name="a.gguf")
    with pytest.raises(ValueError, match="1-D f32"):
        RMSNorm.from_gguf(meta, tensors, "blk.3.ffn_norm", device="cpu")
    _, (meta, tensors) = _write(tmp_path, META, shape=(1, 64), name="b.gguf")
    with pytest.raises(ValueError, match="1-D f32"):
        RMSNorm.from_gguf(meta, tensors, "blk.3.ffn_norm", device="cpu")
    _, (meta, tensors) = _write(tmp_path, {"general.architecture": "llama"}, name="c.gguf")
    with pytest.raises(ValueError, match="layer_norm_rms_epsilon"):
        RMSNorm.from_gguf(meta, tensors, "blk.3.ffn_norm", device="cpu")
    _, (meta, tensors) = _write(tmp_path, {"llama.attention.layer_norm_rms_epsilon": 1e-5}, name="d.gguf")
    with pytest.raises(ValueError, match="general.architecture"):
        RMSNorm.from_gguf(meta, tensors, "blk.3.ffn_norm", device="cpu")
    _, (meta, tensors) = _write(tmp_path, META, name="e.gguf")
    with pytest.raises(ValueError, match="no such tensor"):
        RMSNorm.from_gguf(meta, tensors, "blk.4.ffn_norm", device="cpu")


def test_rmsnorm_constructor_checks():
    from kernels.norm import RMSNorm
    with pytest.raises(ValueError, match="1-D fp32"):
        RMSNorm(torch.ones(64, dtype=torch.float16), 1e-5)
    with pytest.raises(ValueError, match="1-D fp32"):
        RMSNorm(torch.ones(1, 64), 1e-5)
    for eps in (-1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            RMSNorm(torch.ones(64), eps)
    assert RMSNorm(torch.ones(64), 0.0).eps == 0.0


def _linear(M, K):
    from kernels.layer_mix import GGUFLinear
    return GGUFLinear("q8_0", torch.zeros(M * (K // 32) * 34, dtype=torch.int8), M, K)


def test_forward_normed_without_a_norm_raises():
    from kernels.ffn import DenseFFN
    from kernels.moe import GGUFExperts, MoEBlock, MoEFFN, MoERouter
    from kernels.norm import RMSNorm
    x = torch.zeros(2, 64, dtype=torch.float16)
    ffn = DenseFFN(_linear(96, 64), _linear(96, 64), _linear(64, 96))
    assert ffn.norm is None
    with pytest.raises(RuntimeError, match="norm"):
        ffn.forward_normed(x)
    with pytest.raises(RuntimeError, match="norm"):
        ffn.forward_normed(x, x)
    ex = lambda M, K: GGUFExperts("q8_0", torch.zeros(2 * M * (K // 32) * 34, dtype=torch.int8), 2, M, K)
    blk = MoEBlock(MoERouter(torch.zeros(2, 64), 1), MoEFFN(ex(96, 64), ex(96, 64), ex(64, 96)))
    assert blk.norm is None
    with pytest.raises(RuntimeError, match="norm"):
        blk.forward_normed(x)
    # a norm of another width is refused at construction
    with pytest.raises(ValueError, match="hidden size"):
        DenseFFN(_linear(96, 64), _linear(96, 64), _linear(64, 96), norm=RMSNorm(torch.ones(32), 1e-5))
    with pytest.raises(ValueError, match="hidden size"):
        MoEBlock(MoERouter(torch.zeros(2, 64), 1), MoEFFN(ex(96, 64), ex(96, 64), ex(64, 96)), norm=RMSNorm(torch.ones(32), 1e-5))
    assert DenseFFN(_linear(96, 64), _linear(96, 64), _linear(64, 96), norm=RMSNorm(torch.ones(64), 1e-5)).norm.K == 64


def test_dense_ffn_from_gguf_loads_the_norm(tmp_path):
    from gguf.file import read_gguf, write_gguf
    from kernels.ffn import DenseFFN
    from utils.synth import random_blocks
    Hd, F = 64, 96
    w = (1 + 0.3 * np.random.default_rng(4).standard_normal(Hd)).astype(np.float32)
    tensors = {"blk.0.ffn_gate.weight": ("q8_0", (F, Hd), random_blocks("q8_0", F, Hd, 1)),
               "blk.0.ffn_up.weight": ("q8_0", (F, Hd), random_blocks("q8_0", F, Hd, 2)),
               "blk.0.ffn_down.weight": ("q8_0", (Hd, F), random_blocks("q8_0", Hd, F, 3)),
               "blk.0.ffn_norm.weight": ("f32", (Hd,), w)}
    path = str(tmp_path / "f.gguf")
    write_gguf(path, tensors, metadata=META)
    meta, t = read_gguf(path)
    ffn = DenseFFN.from_gguf(t, 0, device="cpu", norm=True, meta=meta)
    assert ffn.norm is not None and np.array_equal(ffn.norm.weight.numpy(), w) and ffn.norm.eps == float(np.float32(1e-5))
    assert DenseFFN.from_gguf(t, 0, device="cpu").norm is None
    with pytest.raises(ValueError, match="meta"):
        DenseFFN.from_gguf(t, 0, device="cpu", norm=True)
