"""Host side of the fused MoE decode entries (gq_mmq_id_glu, gq_moe_combine): both symbols exported
and bound, their argument checks (fake pointers: every case returns before a launch), and the
numpy model the GPU tests judge by (tests/moe_fused_model.py) checked against itself and against
torch's CPU ops.  CPU only."""
import ctypes

import numpy as np
import torch

import moe_fused_model as MF

OK, EINVAL, EUNSUPPORTED = 0, 1, 3


def test_symbols_and_version():
    import kernels._lib as kl
    L = kl.lib()
    assert hasattr(L, "gq_mmq_id_glu") and hasattr(L, "gq_moe_combine")
    argtypes, restype = kl.SIGNATURES["gq_mmq_id_glu"]
    assert len(argtypes) == 15 and restype is ctypes.c_int
    assert all(a is ctypes.c_void_p for a in argtypes[1:6]) and all(a is ctypes.c_int64 for a in argtypes[6:14])
    argtypes, restype = kl.SIGNATURES["gq_moe_combine"]
    assert len(argtypes) == 10 and restype is ctypes.c_int and argtypes[2] is ctypes.c_int
    assert L.gq_version() == 105  # (the entries are detected by their symbols)


def test_glu_argument_checks():
    import kernels._lib as kl
    L = kl.lib()
    p = ctypes.c_void_p(16)

    def call(t=1, A_gate=p, A_up=p, ids=p, B=p, H=p, E=4, M=8, N=2, S=2, K=256, ldb=256, ldb_slot=0, ldh=8):
        return L.gq_mmq_id_glu(t, A_gate, A_up, ids, B, H, E, M, N, S, K, ldb, ldb_slot, ldh, None)

    for name in ("A_gate", "A_up", "ids", "B", "H"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null" in L.gq_last_error()
    assert call(ldh=7) == EINVAL
    assert call(ldb=255) == EINVAL
    assert call(ldb_slot=255) == EINVAL
    assert b"ldb_slot" in L.gq_last_error()
    assert call(ldb_slot=1) == EINVAL
    assert call(t=7) == EUNSUPPORTED
    assert call(N=65, S=1) == EUNSUPPORTED
    assert call(N=13, S=5) == EUNSUPPORTED
    assert b"64" in L.gq_last_error()
    assert call(K=100, ldb=100) == EINVAL
    assert call(t=0, K=1 << 20, ldb=1 << 20) == EUNSUPPORTED  # a row too long for the one-token decode
    none = dict(A_gate=None, A_up=None, ids=None, B=None, H=None)
    assert call(N=0, **none) == OK
    assert call(S=0, **none) == OK
    assert call(M=0, ldh=0, **none) == OK


def test_combine_argument_checks():
    import kernels._lib as kl
    L = kl.lib()
    p = ctypes.c_void_p(16)

    def call(D=p, W=p, f32=0, Y=p, N=2, S=2, M=8, ldd=8, ldy=8):
        return L.gq_moe_combine(D, W, f32, Y, N, S, M, ldd, ldy, None)

    for name in ("D", "W", "Y"):
        assert call(**{name: None}) == EINVAL, name
    assert call(ldd=7) == EINVAL
    assert call(ldy=7) == EINVAL
    assert call(N=-1) == EINVAL
    assert call(S=65) == EUNSUPPORTED
    assert b"64" in L.gq_last_error()
    assert call(D=None, W=None, Y=None, N=0) == OK
    assert call(D=None, W=None, Y=None, S=0) == OK
    assert call(D=None, W=None, Y=None, M=0, ldd=0, ldy=0) == OK


def test_model_self_checks():
    rng = np.random.default_rng(0)
    D = rng.standard_normal((3, 1, 17)).astype(np.float16)
    assert np.array_equal(MF.combine(D, np.ones((3, 1), np.float16)).view(np.uint16), D[:, 0].view(np.uint16))
    assert np.array_equal(MF.combine(D, np.ones((3, 1), np.float32)).view(np.uint16), D[:, 0].view(np.uint16))
    u = rng.standard_normal(64).astype(np.float16)
    assert not MF.glu(np.zeros(64, np.float16), u).any()
    big = MF.glu(np.full(64, -60000.0, np.float16), u)
    assert not np.isnan(big).any() and not (big.view(np.uint16) & 0x7fff).any()  # +-0
    assert MF.ulp16(np.float16(1.0), np.float16(1.0009765625)) == 1
    assert MF.ulp16(np.float16(-0.0), np.float16(0.0)) == 0
    assert MF.ulp16(np.float16(-6e-8), np.float16(6e-8)) == 2


def test_model_glu_against_torch_cpu():
    rng = np.random.default_rng(1)
    g = (rng.standard_normal(4096) * 4).astype(np.float16)
    u = (rng.standard_normal(4096) * 4).astype(np.float16)
    want = (torch.nn.functional.silu(torch.from_numpy(g).float()) * torch.from_numpy(u).float()).half().numpy()
    d = MF.ulp16(MF.glu(g, u), want)
    assert int(d.max()) <= 1, int(d.max())
