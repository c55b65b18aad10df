"""Host side of prefill attention (gq_attn_prefill, gq_debug_attn_prefill_plan) and of gq_kv_append's
lifted token limit: every refusal answers before a launch (fake pointers), with gq_last_error set.
CPU only."""
import ctypes

import pytest

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
MB = 1 << 20
Q, KC, VC, LEN, O, KN, VN = (ctypes.c_void_p(i * 16 * MB) for i in range(1, 8))
BASE = dict(kv=1, q=Q, ldq=1024, kc=KC, vc=VC, tok=1088, head=136, seq=1088 * 64, kv_len=LEN, cap=64, o=O, ldo=1024,
            scale=0.1, B=2, N=40, n_head=8, n_kv=8, D=128)


def _prefill(L, **kw):
    a = dict(BASE, **kw)
    return L.gq_attn_prefill(a["kv"], a["q"], a["ldq"], a["kc"], a["vc"], a["tok"], a["head"], a["seq"], a["kv_len"], a["cap"],
                             a["o"], a["ldo"], a["scale"], a["B"], a["N"], a["n_head"], a["n_kv"], a["D"], None)


REFUSED = [
    ("unknown kv", dict(kv=2), EUNSUPPORTED, b"kv cache type"),
    ("null Q", dict(q=None), EINVAL, b"null"),
    ("null Kc", dict(kc=None), EINVAL, b"null"),
    ("null Vc", dict(vc=None), EINVAL, b"null"),
    ("null kv_len", dict(kv_len=None), EINVAL, b"null"),
    ("null O", dict(o=None), EINVAL, b"null"),
    ("negative B", dict(B=-1), EINVAL, b"negative"),
    ("negative N", dict(N=-2), EINVAL, b"negative"),
    ("negative capacity", dict(cap=-1), EINVAL, b"negative"),
    ("ldq short", dict(ldq=1023), EINVAL, b"ldq"),
    ("ldo short", dict(ldo=512), EINVAL, b"ldo"),
    ("D = 96", dict(D=96, ldq=768, ldo=768), EUNSUPPORTED, b"D=96"),
    ("heads not a multiple", dict(n_kv=3), EUNSUPPORTED, b"multiple of n_kv_head"),
    ("odd stride", dict(tok=1089), EUNSUPPORTED, b"multiples of 2"),
    ("rows overlap", dict(tok=134), EUNSUPPORTED, b"tok_stride"),
    ("capacity < N", dict(cap=39), EUNSUPPORTED, b"capacity"),
    ("1 GiB span", dict(cap=MB), EUNSUPPORTED, b"1 GiB"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_attn_prefill_refuses_before_a_launch(case):
    import kernels._lib as kl
    L = kl.lib()
    _, kw, status, text = case
    assert _prefill(L, **kw) == status, L.gq_last_error()
    assert text in L.gq_last_error(), L.gq_last_error()


def test_more_than_32_rows_is_not_a_refusal():
    """R = 33, which gq_attn_decode refuses for its row count, passes the shape checks here: the next
    check in line (capacity < N) answers, and an empty call of that shape is a no-op."""
    import kernels._lib as kl
    L = kl.lib()
    r33 = dict(N=3, n_head=11, n_kv=1, ldq=1408, ldo=1408)
    assert _prefill(L, cap=2, **r33) == EUNSUPPORTED and b"capacity" in L.gq_last_error()
    assert _prefill(L, B=0, q=None, o=None, **r33) == OK and _prefill(L, **dict(r33, N=0), kc=None) == OK


def test_prefill_plan():
    import kernels._lib as kl
    for B, N, nh, kvh, D in ((1, 3, 11, 1, 128), (1, 512, 32, 8, 128), (4, 2048, 32, 8, 64), (1, 8192, 32, 32, 128)):
        rows, tile = kl.attn_prefill_plan(B, N, nh, kvh, D)
        assert rows in (64, 128) and tile in (32, 64)
    L = kl.lib()
    assert L.gq_debug_attn_prefill_plan(1, 512, 8, 8, 96, None, None) == EUNSUPPORTED
    assert L.gq_debug_attn_prefill_plan(1, 512, 8, 3, 128, None, None) == EUNSUPPORTED


def test_kv_append_takes_more_than_32_tokens():
    import kernels._lib as kl
    L = kl.lib()
    a = dict(BASE, ldn=1024)
    call = lambda **kw: L.gq_kv_append(a["kv"], KN, VN, a["ldn"], KC, VC, a["tok"], a["head"], a["seq"], LEN,
                                       kw.get("cap", a["cap"]), kw.get("B", 2), kw.get("N", 33), a["n_kv"], a["D"], None)
    assert call(cap=32) == EUNSUPPORTED and b"capacity" in L.gq_last_error()  # N = 33 reaches the capacity check ...
    assert call(B=0) == OK                                                    # ... and is an accepted shape


def test_wrapper_refuses_host_tensors():
    import torch

    import kernels
    z = torch.zeros(80, 1024, dtype=torch.float16)
    b8, n = torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        kernels.attn_prefill("f16", z, b8, b8, (2048, 256, 4096), n, 64, 2, 40, 8, 8, 128)
