"""Host side of the dense GLU decode and the shared-expert block (gq_mmq_glu, gq_moe_combine_shared;
kernels/ffn.py DenseFFN, kernels/moe.py MoEBlock(shared=...)): both symbols exported and bound, their
argument checks (fake pointers: every case returns before a launch), the numpy model the GPU tests
judge by (tests/moe_shared_model.py) on hand-worked cases, and MoEBlock.from_gguf on written files.
CPU only."""
import ctypes

import numpy as np
import pytest
import torch

import moe_fused_model as MF
import moe_shared_model as MS

OK, EINVAL, EUNSUPPORTED = 0, 1, 3


# ---- the ABI ----
def test_symbols_and_version():
    import kernels._lib as kl
    L = kl.lib()
    assert hasattr(L, "gq_mmq_glu") and hasattr(L, "gq_moe_combine_shared")
    argtypes, restype = kl.SIGNATURES["gq_mmq_glu"]
    assert len(argtypes) == 11 and restype is ctypes.c_int
    assert all(a is ctypes.c_void_p for a in argtypes[1:5]) and all(a is ctypes.c_int64 for a in argtypes[5:10])
    argtypes, restype = kl.SIGNATURES["gq_moe_combine_shared"]
    assert len(argtypes) == 13 and restype is ctypes.c_int and argtypes[2] is ctypes.c_int
    assert argtypes[4] is ctypes.c_int64 and all(a is ctypes.c_int64 for a in argtypes[7:12])
    assert L.gq_version() == 105  # (the entries are detected by their symbols)


def test_glu_argument_checks():
    import kernels._lib as kl
    L = kl.lib()
    p = ctypes.c_void_p(16)

    def call(t=1, A_gate=p, A_up=p, B=p, H=p, M=8, N=2, K=256, ldb=256, ldh=8):
        return L.gq_mmq_glu(t, A_gate, A_up, B, H, M, N, K, ldb, ldh, None)

    for name in ("A_gate", "A_up", "B", "H"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null" in L.gq_last_error()
    assert call(ldb=255) == EINVAL
    assert b"ldb" in L.gq_last_error()
    assert call(ldh=7) == EINVAL
    assert b"ldh" in L.gq_last_error()
    for name in ("M", "N", "K"):
        assert call(**{name: -1}) == EINVAL, name
        assert b"negative" in L.gq_last_error()
    assert call(K=100, ldb=100) == EINVAL        # Q4_K: K % 256
    assert call(t=0, K=48, ldb=48) == EINVAL     # Q8_0: K % 32
    assert call(t=7) == EUNSUPPORTED
    assert call(N=5) == EUNSUPPORTED
    assert b"at most 4" in L.gq_last_error()
    assert call(N=64) == EUNSUPPORTED
    assert call(t=0, N=1, K=1 << 20, ldb=1 << 20) == EUNSUPPORTED  # a row too long for the one-launch decode
    assert call(t=4, N=4, K=8960, ldb=8960) == EUNSUPPORTED        # Q3_K: 4 tokens do not fit the LDS image
    assert call(t=1, N=1, M=1 << 22, K=1024, ldb=1024, ldh=1 << 22) == EUNSUPPORTED  # 2.25 GiB in one matrix
    assert call(N=5, ldb=255) == EINVAL  # (a bad argument before a refused shape)
    none = dict(A_gate=None, A_up=None, B=None, H=None)
    assert call(N=0, **none) == OK
    assert call(M=0, ldh=0, **none) == OK
    assert L.gq_last_error() == b""


def test_combine_shared_argument_checks():
    import kernels._lib as kl
    L = kl.lib()
    p = ctypes.c_void_p(16)

    def call(D=p, W=p, f32=0, Dsh=p, ldsh=8, gate=None, Y=p, N=2, S=2, M=8, ldd=8, ldy=8):
        return L.gq_moe_combine_shared(D, W, f32, Dsh, ldsh, gate, Y, N, S, M, ldd, ldy, None)

    for name in ("D", "W", "Dsh", "Y"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null" in L.gq_last_error()
    for name in ("ldd", "ldsh", "ldy"):
        assert call(**{name: 7}) == EINVAL, name
        assert name.encode() in L.gq_last_error()
    for name in ("N", "S", "M"):
        assert call(**{name: -1}) == EINVAL, name
    assert call(S=0) == EINVAL  # with a shared term an empty slot sum is no no-op
    assert call(S=65) == EUNSUPPORTED
    assert b"64" in L.gq_last_error()
    none = dict(D=None, W=None, Dsh=None, Y=None)
    assert call(N=0, **none) == OK
    assert call(M=0, ldd=0, ldsh=0, ldy=0, **none) == OK
    assert call(N=0, S=0, **none) == EINVAL


def test_wrappers_refuse_cpu_tensors():
    import kernels._lib as kl
    A = torch.zeros(144 * 2, dtype=torch.int8)
    B = torch.zeros(1, 256, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        kl.mmq_glu(kl.GQ_Q4_K, A, A, B, 2, 1, 256)
    D = torch.zeros(1, 2, 8, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        kl.moe_combine_shared(D, torch.zeros(1, 2), torch.zeros(1, 8, dtype=torch.float16))


# ---- the model ----
def test_model_zero_gate_drops_the_shared_term():
    rng = np.random.default_rng(0)
    D = rng.standard_normal((3, 2, 17)).astype(np.float16)
    Dsh = rng.standard_normal((3, 17)).astype(np.float16)
    for wdtype in (np.float16, np.float32):
        W = rng.standard_normal((3, 2)).astype(wdtype)
        routed = MF.combine(D, W)
        got = MS.combine_shared(D, W, Dsh, np.zeros(3, np.float32))
        assert np.array_equal(got.view(np.uint16), routed.view(np.uint16))
        one = MS.combine_shared(D, W, Dsh, np.ones(3, np.float32))
        assert np.array_equal(one.view(np.uint16), MS.combine_shared(D, W, Dsh).view(np.uint16))
        assert not np.array_equal(one.view(np.uint16), routed.view(np.uint16))
    # one slot of weight 1 and no gate: fp16(d + dsh) from an fp32 sum
    W1 = np.ones((3, 1), np.float16)
    want = (D[:, 0].astype(np.float32) + Dsh.astype(np.float32)).astype(np.float16)
    assert np.array_equal(MS.combine_shared(D[:, :1], W1, Dsh).view(np.uint16), want.view(np.uint16))


def test_model_pins_the_unfused_order():
    """gate * dsh is rounded to fp32 before it is added: g = 2^10 (1 + 2^-23), dsh = 2^5 (1 + 2^-10).
    The exact product 2^15 (1 + 2^-10 + 2^-23 + 2^-33) rounds to P = 2^15 (1 + 2^-10 + 2^-23); with
    acc = -P (one slot: d = 1, w = -P) the defined result is 0, a fused multiply-add gives the
    residual 2^-18, a nonzero fp16."""
    g = np.float32(1024.0) * (np.float32(1.0) + np.float32(2.0 ** -23))
    dsh = np.float16(32.0 * (1.0 + 2.0 ** -10))
    assert float(dsh) == 32.03125
    P = np.float32(g * np.float32(dsh))
    exact = float(g) * float(dsh)
    assert exact - float(P) == 2.0 ** -18
    D, W = np.ones((1, 1, 1), np.float16), np.array([[-P]], np.float32)
    got = MS.combine_shared(D, W, np.array([[dsh]]), np.array([g], np.float32))
    assert got.view(np.uint16)[0, 0] == 0
    fused = np.float16(-float(P) + exact)  # what one fma would leave
    assert fused.view(np.uint16) == 64    # 2^-18 = 64 * 2^-24
    # and the routed sum keeps gq_moe_combine's order: the shared term comes last
    D2 = np.array([[[1.0], [1.0]]], np.float16)
    W2 = np.array([[2.0 ** 24, 1.0]], np.float32)  # fl32(2^24 + 1) = 2^24, then - 2^24 from the shared term
    got = MS.combine_shared(D2, W2, np.array([[-2.0]], np.float16), np.array([2.0 ** 23], np.float32))
    assert float(got[0, 0]) == 0.0


# ---- from_gguf ----
def _raw(fmt_bytes, rows, K, seed):
    """Random q4_0 blocks with small fp16 scales (the loader only moves bytes)."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(rows * K // 32, fmt_bytes), dtype=np.uint8)
    raw[:, 0:2] = np.full((raw.shape[0], 1), 2.0 ** -7, np.float16).view(np.uint8)
    return raw.reshape(-1)


def _write(tmp_path, name, shexp=("ffn_gate_shexp", "ffn_up_shexp", "ffn_down_shexp"), gate_type=None, E=4, H=64, F=32, Fs=96):
    from gguf.file import read_gguf, write_gguf
    meta = {"general.architecture": "qwen2moe", "qwen2moe.expert_count": E, "qwen2moe.expert_used_count": 2}
    Wr = (np.random.default_rng(2).standard_normal((E, H)) / 8).astype(np.float32)
    tensors = {"blk.3.ffn_gate_inp.weight": ("f32", (E, H), Wr),
               "blk.3.ffn_gate_exps.weight": ("q4_0", (E, F, H), _raw(18, E * F, H, 1)),
               "blk.3.ffn_up_exps.weight": ("q4_0", (E, F, H), _raw(18, E * F, H, 2)),
               "blk.3.ffn_down_exps.weight": ("q4_0", (E, H, F), _raw(18, E * H, F, 3))}
    shapes = {"ffn_gate_shexp": (Fs, H), "ffn_up_shexp": (Fs, H), "ffn_down_shexp": (H, Fs)}
    for i, n in enumerate(shexp):
        tensors[f"blk.3.{n}.weight"] = ("q4_0", shapes[n], _raw(18, *shapes[n], 10 + i))
    v = None
    if gate_type is not None:
        v = (np.random.default_rng(4).standard_normal((1, H)) / 8).astype(np.float32 if gate_type == "f32" else np.float16)
        tensors["blk.3.ffn_gate_inp_shexp.weight"] = (gate_type, (1, H), v)
    path = str(tmp_path / name)
    write_gguf(path, tensors, metadata=meta)
    return v, tensors, read_gguf(path)


def test_block_from_gguf_with_shared_experts(tmp_path):
    from kernels.ffn import DenseFFN
    from kernels.moe import MoEBlock, MoERouter
    _, src, (m, t) = _write(tmp_path, "a.gguf")
    with pytest.raises(NotImplementedError, match="blk.3.ffn_gate_shexp.weight"):  # the default, word for word
        MoEBlock.from_gguf(m, t, 3, "cpu")
    with pytest.raises(NotImplementedError, match="their output is added to the routed experts' and this block does not"):
        MoERouter.from_gguf(m, t, 3, "cpu")
    assert MoERouter.from_gguf(m, t, 3, "cpu", shared_experts=True).S == 2
    b = MoEBlock.from_gguf(m, t, 3, "cpu", shared_experts=True)
    assert isinstance(b.shared, DenseFFN) and b.shared.fused is True and b.shared_gate is None
    assert (b.shared.gate.M, b.shared.gate.K, b.shared.down.M, b.shared.down.K) == (96, 64, 64, 96)
    assert b.shared.gate.type_name == "q4_0"
    for lin, n in ((b.shared.gate, "ffn_gate_shexp"), (b.shared.up, "ffn_up_shexp"), (b.shared.down, "ffn_down_shexp")):
        assert np.array_equal(lin.A.numpy().view(np.uint8), src[f"blk.3.{n}.weight"][2])
    assert MoEBlock.from_gguf(m, t, 3, "cpu", fused=False, shared_experts=True).shared.fused is False
    # a layer without shared experts: the keyword changes nothing
    _, _, (m, t) = _write(tmp_path, "b.gguf", shexp=())
    assert MoEBlock.from_gguf(m, t, 3, "cpu", shared_experts=True).shared is None
    assert MoEBlock.from_gguf(m, t, 3, "cpu").shared is None


def test_block_from_gguf_wants_all_three(tmp_path):
    from kernels.moe import MoEBlock
    _, _, (m, t) = _write(tmp_path, "c.gguf", shexp=("ffn_gate_shexp", "ffn_up_shexp"))
    with pytest.raises(ValueError, match="blk.3.ffn_down_shexp.weight"):
        MoEBlock.from_gguf(m, t, 3, "cpu", shared_experts=True)


@pytest.mark.parametrize("gate_type", ["f32", "f16"])
def test_block_from_gguf_reads_the_shared_gate(tmp_path, gate_type):
    from kernels.moe import MoEBlock
    v, _, (m, t) = _write(tmp_path, "d.gguf", gate_type=gate_type)
    b = MoEBlock.from_gguf(m, t, 3, "cpu", shared_experts=True)
    assert tuple(b.shared_gate.shape) == (1, 64)
    assert b.shared_gate.dtype == (torch.float32 if gate_type == "f32" else torch.float16)
    assert np.array_equal(b.shared_gate.numpy(), v)


def test_block_argument_checks():
    from kernels.ffn import DenseFFN
    from kernels.layer_mix import GGUFLinear
    from kernels.moe import GGUFExperts, MoEBlock, MoEFFN, MoERouter
    z = torch.zeros(1, dtype=torch.int8)
    router = MoERouter(torch.zeros(4, 64), 2)
    ffn = MoEFFN(GGUFExperts("q4_0", z, 4, 32, 64), GGUFExperts("q4_0", z, 4, 32, 64), GGUFExperts("q4_0", z, 4, 64, 32))
    shared = DenseFFN(GGUFLinear("q4_0", z, 96, 64), GGUFLinear("q4_0", z, 96, 64), GGUFLinear("q4_0", z, 64, 96))
    assert MoEBlock(router, ffn, shared, torch.zeros(64)).shared_gate.shape == (1, 64)
    with pytest.raises(ValueError, match="hidden"):
        MoEBlock(router, ffn, DenseFFN(GGUFLinear("q4_0", z, 96, 32), GGUFLinear("q4_0", z, 96, 32), GGUFLinear("q4_0", z, 32, 96)))
    with pytest.raises(ValueError, match="shared_gate"):
        MoEBlock(router, ffn, None, torch.zeros(64))
    with pytest.raises(ValueError, match="shared_gate"):
        MoEBlock(router, ffn, shared, torch.zeros(63))
    with pytest.raises(ValueError):
        DenseFFN(GGUFLinear("q4_0", z, 96, 64), GGUFLinear("q4_0", z, 64, 64), GGUFLinear("q4_0", z, 64, 96))
