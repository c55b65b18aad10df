"""Host side of gq_mla_proj: the ctypes table and the library agree, every refusal answers before a launch (fake
pointers) with the header's status, the empty problem is a no-op, and the planner takes the few-row form up to
one MFMA tile of tokens and the tiled form beyond.  CPU only."""
import ctypes

import pytest

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
MB = 1 << 20
W, X, Y = (ctypes.c_void_p(i * 64 * MB) for i in range(1, 4))
ABSORB = dict(dir=0, w=W, x=X, ldx=16 * 192, xhs=192, y=Y, ldy=16 * 576, yhs=576, T=4, n_head=16, rank=512, dim=128)
EXPAND = dict(ABSORB, dir=1, ldx=16 * 512, xhs=512, ldy=16 * 128, yhs=128)


def _proj(L, base, **kw):
    a = dict(base, **kw)
    return L.gq_mla_proj(a["dir"], a["w"], a["x"], a["ldx"], a["xhs"], a["y"], a["ldy"], a["yhs"], a["T"], a["n_head"],
                         a["rank"], a["dim"], None)


REFUSED = [
    ("null W", ABSORB, dict(w=None), EINVAL, b"null"),
    ("null X", EXPAND, dict(x=None), EINVAL, b"null"),
    ("null Y", ABSORB, dict(y=None), EINVAL, b"null"),
    ("negative T", ABSORB, dict(T=-1), EINVAL, b"negative"),
    ("negative n_head", EXPAND, dict(n_head=-1), EINVAL, b"negative"),
    ("unknown dir", ABSORB, dict(dir=2), EUNSUPPORTED, b"direction"),
    ("rank 256", ABSORB, dict(rank=256), EUNSUPPORTED, b"(512, 128)"),
    ("dim 64", EXPAND, dict(dim=64), EUNSUPPORTED, b"(512, 128)"),
    ("129 heads", ABSORB, dict(n_head=129, ldx=129 * 192, ldy=129 * 576), EUNSUPPORTED, b"at most 128"),
    ("2^31 rows", EXPAND, dict(T=1 << 24, n_head=128, ldx=128 * 512, ldy=128 * 128), EUNSUPPORTED, b"2^31"),
    ("absorb x_head_stride", ABSORB, dict(xhs=120), EINVAL, b"x_head_stride"),
    ("expand x_head_stride", EXPAND, dict(xhs=504), EINVAL, b"x_head_stride"),
    ("absorb y_head_stride", ABSORB, dict(yhs=508), EINVAL, b"y_head_stride"),
    ("expand y_head_stride", EXPAND, dict(yhs=124), EINVAL, b"y_head_stride"),
    ("ldx short", ABSORB, dict(ldx=15 * 192 + 120), EINVAL, b"ldx"),
    ("ldy short", EXPAND, dict(ldy=15 * 128 + 124), EINVAL, b"ldy"),
    ("X misaligned", ABSORB, dict(x=ctypes.c_void_p(128 * MB + 8)), EINVAL, b"16-byte"),
    ("ldx no multiple of 8", ABSORB, dict(ldx=16 * 192 + 4), EINVAL, b"16-byte"),
    ("Y misaligned", EXPAND, dict(y=ctypes.c_void_p(192 * MB + 4)), EINVAL, b"8-byte"),
    ("y_head_stride no multiple of 4", ABSORB, dict(yhs=578, ldy=16 * 578), EINVAL, b"8-byte"),
]


@pytest.mark.parametrize("base,kw,status,text", [c[1:] for c in REFUSED], ids=[c[0] for c in REFUSED])
def test_mla_proj_refuses_before_a_launch(base, kw, status, text):
    import kernels._lib as kl
    L = kl.lib()
    assert _proj(L, base, **kw) == status, L.gq_last_error()
    assert text in L.gq_last_error(), L.gq_last_error()


@pytest.mark.parametrize("kw", [dict(T=0, w=None, x=None, y=None), dict(n_head=0, ldx=0, ldy=0, y=None)])
def test_the_empty_problem_is_a_no_op(kw):
    import kernels._lib as kl
    assert _proj(kl.lib(), ABSORB, **kw) == OK and _proj(kl.lib(), EXPAND, **kw) == OK


def test_signatures_and_the_library_agree():
    import kernels
    import kernels._lib as kl
    for name in ("gq_mla_proj", "gq_debug_mla_proj_plan"):
        assert name in kl.SIGNATURES and getattr(kl.lib(), name).argtypes == kl.SIGNATURES[name][0]
    assert callable(kernels.mla_proj)


@pytest.mark.parametrize("dir,mo", [(0, 512), (1, 128)])
def test_the_plan_takes_the_few_row_form_up_to_a_tile_and_the_tiled_form_beyond(dir, mo):
    import kernels._lib as kl
    for T in (1, 4, 16):
        assert kl.mla_proj_plan(dir, T, 16) == (0, 16, 16 * mo // 16)    # every 16-row tile of W its own workgroup
        assert kl.mla_proj_plan(dir, T, 128) == (0, 16, 128 * mo // 32)  # 2048 / 512: at least 256
    assert kl.mla_proj_plan(dir, 17, 20) == (1, 64, 20) and kl.mla_proj_plan(dir, 65, 128) == (1, 64, 256)
    with pytest.raises(RuntimeError, match="projection shape"):
        kl.mla_proj_plan(dir, 4, 129)
