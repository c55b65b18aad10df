"""Host side of gq_mla_prefill: every refusal answers before a launch (fake pointers) with gq_mla_decode's
status and message, gq_last_error set; any N the cache holds passes the planner.  CPU only."""
import ctypes

import pytest

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
MB = 1 << 20
Q, C, LEN, O = (ctypes.c_void_p(i * 64 * MB) for i in range(1, 5))
BASE = dict(q=Q, ldq=16 * 576, c=C, tok=1152, seq=1152 * 64, kv_len=LEN, cap=64, o=O, ldo=16 * 512, B=2, N=9, n_head=16,
            rank=512, rope=64)


def _prefill(L, **kw):
    a = dict(BASE, **kw)
    return L.gq_mla_prefill(a["q"], a["ldq"], a["c"], a["tok"], a["seq"], a["kv_len"], a["cap"], a["o"], a["ldo"], 0.07, a["B"],
                            a["N"], a["n_head"], a["rank"], a["rope"], None)


REFUSED = [
    ("null Q", dict(q=None), EINVAL, b"null"),
    ("null C", dict(c=None), EINVAL, b"null"),
    ("null kv_len", dict(kv_len=None), EINVAL, b"null"),
    ("null O", dict(o=None), EINVAL, b"null"),
    ("negative B", dict(B=-1), EINVAL, b"negative"),
    ("negative N", dict(N=-2), EINVAL, b"negative"),
    ("negative capacity", dict(cap=-1), EINVAL, b"negative"),
    ("ldq short", dict(ldq=16 * 576 - 1), EINVAL, b"ldq"),
    ("ldo short", dict(ldo=16 * 512 - 1), EINVAL, b"ldo"),
    ("129 heads", dict(n_head=129, ldq=129 * 576, ldo=129 * 512), EUNSUPPORTED, b"at most 128"),
    ("rank 256", dict(rank=256), EUNSUPPORTED, b"(512, 64)"),
    ("rope 32", dict(rope=32), EUNSUPPORTED, b"(512, 64)"),
    ("odd stride", dict(tok=1153), EUNSUPPORTED, b"multiples of 2"),
    ("rows overlap", dict(tok=1150), EUNSUPPORTED, b"tok_stride"),
    ("capacity < N", dict(cap=8), EUNSUPPORTED, b"capacity"),
    ("1 GiB span", dict(cap=MB), EUNSUPPORTED, b"1 GiB"),
    ("2^31 rows", dict(B=1 << 17, N=128, cap=128, n_head=128, ldq=128 * 576, ldo=128 * 512), EUNSUPPORTED, b"2^31"),
]


@pytest.mark.parametrize("kw,status,text", [c[1:] for c in REFUSED], ids=[c[0] for c in REFUSED])
def test_mla_prefill_refuses_before_a_launch(kw, status, text):
    import kernels._lib as kl
    L = kl.lib()
    assert _prefill(L, **kw) == status, L.gq_last_error()
    assert text in L.gq_last_error(), L.gq_last_error()


@pytest.mark.parametrize("kw", [dict(B=0, q=None, o=None), dict(N=0, c=None), dict(n_head=0, ldq=0, ldo=0)])
def test_empty_calls_are_no_ops(kw):
    import kernels._lib as kl
    assert _prefill(kl.lib(), **kw) == OK


@pytest.mark.parametrize("B,N,nh", [(1, 5, 16), (2, 4, 20), (1, 100000, 128), (1 << 17, 127, 128)])
def test_any_token_count_passes_the_planner(B, N, nh):
    import kernels._lib as kl
    tile, rows, grid = kl.mla_prefill_plan(B, N, nh)
    assert (tile, rows) == (32, 64) and grid == B * -(-N * nh // rows)
    with pytest.raises(RuntimeError, match="prefill shape"):
        kl.mla_prefill_plan(B, N, 129)


def test_the_cache_still_constructs_on_the_host():
    import kernels
    c = kernels.MLACache(2, 8, device="cpu")
    assert c.strides == (1152, 8 * 1152) and c.c.numel() == 2 * 8 * 1152 and callable(kernels.mla_prefill)
