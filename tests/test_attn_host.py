"""Host side of decode attention (gq_attn_decode, gq_kv_append, gq_attn_decode_workspace_size): every
refusal answers before a launch (fake pointers), with gq_last_error set; the workspace size is
monotone and exactly what the call demands.  CPU only."""
import ctypes

import pytest

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
MB = 1 << 20
Q, KC, VC, LEN, O, WS, KN, VN = (ctypes.c_void_p(i * 16 * MB) for i in range(1, 9))
BASE = dict(kv=1, q=Q, ldq=1024, kc=KC, vc=VC, tok=1088, head=136, seq=1088 * 64, kv_len=LEN, cap=64, o=O, ldo=1024,
            scale=0.1, B=2, N=2, n_head=8, n_kv=8, D=128, ws=WS, nbytes=64 * MB)


def _attn(L, **kw):
    a = dict(BASE, **kw)
    return L.gq_attn_decode(a["kv"], a["q"], a["ldq"], a["kc"], a["vc"], a["tok"], a["head"], a["seq"], a["kv_len"], a["cap"],
                            a["o"], a["ldo"], a["scale"], a["B"], a["N"], a["n_head"], a["n_kv"], a["D"], a["ws"], a["nbytes"], None)


def _append(L, **kw):
    a = {**BASE, "kn": KN, "vn": VN, "ldn": 1024, **kw}
    return L.gq_kv_append(a["kv"], a["kn"], a["vn"], a["ldn"], a["kc"], a["vc"], a["tok"], a["head"], a["seq"], a["kv_len"],
                          a["cap"], a["B"], a["N"], a["n_kv"], a["D"], None)


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
    ("null workspace", dict(ws=None), EINVAL, b"workspace"),
    ("short workspace", dict(nbytes=1024), EINVAL, b"workspace"),
    ("unaligned workspace", dict(ws=ctypes.c_void_p(WS.value + 8)), EINVAL, b"aligned"),
    ("D = 96", dict(D=96, ldq=768, ldo=768), EUNSUPPORTED, b"D=96"),
    ("heads not a multiple", dict(n_kv=3), EUNSUPPORTED, b"multiple of n_kv_head"),
    ("no kv head", dict(n_kv=0), EUNSUPPORTED, b"multiple of n_kv_head"),
    ("R = 33", dict(N=3, n_head=11, n_kv=1, ldq=1408, ldo=1408), EUNSUPPORTED, b"query rows"),
    ("odd stride", dict(tok=1089), EUNSUPPORTED, b"multiples of 2"),
    ("rows overlap", dict(tok=134), EUNSUPPORTED, b"tok_stride"),
    ("capacity < N", dict(cap=1), EUNSUPPORTED, b"capacity"),
    ("1 GiB span", dict(cap=MB), EUNSUPPORTED, b"1 GiB"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_attn_decode_refuses_before_a_launch(case):
    import kernels._lib as kl
    L = kl.lib()
    _, kw, status, text = case
    assert _attn(L, **kw) == status, L.gq_last_error()
    assert text in L.gq_last_error(), L.gq_last_error()


@pytest.mark.parametrize("kw,status,text", [
    (dict(kv=5), EUNSUPPORTED, b"kv cache type"), (dict(kn=None), EINVAL, b"null"), (dict(vn=None), EINVAL, b"null"),
    (dict(kc=None), EINVAL, b"null"), (dict(kv_len=None), EINVAL, b"null"), (dict(ldn=1000), EINVAL, b"ldn"),
    (dict(B=-1), EINVAL, b"negative"), (dict(D=32), EUNSUPPORTED, b"D=32"), (dict(seq=7), EUNSUPPORTED, b"multiples of 2"),
    (dict(cap=1), EUNSUPPORTED, b"capacity")])
def test_kv_append_refuses_before_a_launch(kw, status, text):
    import kernels._lib as kl
    L = kl.lib()
    assert _append(L, **kw) == status, L.gq_last_error()
    assert text in L.gq_last_error(), L.gq_last_error()


def test_empty_calls_are_no_ops():
    import kernels._lib as kl
    L = kl.lib()
    assert _attn(L, B=0, q=None, o=None, ws=None, nbytes=0) == OK
    assert _attn(L, N=0, q=None, kc=None, ws=None, nbytes=0) == OK
    assert _append(L, B=0, kn=None) == OK and _append(L, N=0, kc=None) == OK


def test_workspace_size_is_monotone_and_exact():
    import kernels._lib as kl
    L = kl.lib()
    size = L.gq_attn_decode_workspace_size
    shapes = [(B, N, G * kvh, kvh, D) for B in (1, 2, 3, 7, 64, 300) for N in (1, 2, 4) for G in (1, 4, 7)
              for kvh in (1, 2, 8) for D in (64, 128) if N * G <= 32]
    for B, N, nh, kvh, D in shapes:
        need = size(B, N, nh, kvh, D)
        assert need > 0
        # growing B, N, the group (n_head at a fixed n_kv_head), the kv heads (at a fixed group) or D never shrinks it
        for B2, N2, nh2, kvh2, D2 in ((B + 1, N, nh, kvh, D), (B, N + 1, nh, kvh, D), (B, N, nh + kvh, kvh, D),
                                      (B, N, nh // kvh * (kvh + 1), kvh + 1, D), (B, N, nh, kvh, 128)):
            if N2 * (nh2 // kvh2) <= 32:
                assert size(B2, N2, nh2, kvh2, D2) >= need, (B, N, nh, kvh, D)
        kw = dict(B=B, N=N, n_head=nh, n_kv=kvh, D=D, ldq=nh * D, ldo=nh * D, q=Q, o=O, kv=0, tok=kvh * 2 * D, head=2 * D,
                  seq=64 * kvh * 2 * D)
        assert _attn(L, nbytes=need - 1, **kw) == EINVAL and str(need).encode() in L.gq_last_error()
    # unsupported or empty: nothing to size
    assert size(1, 1, 8, 8, 96) == 0 and size(1, 5, 7, 1, 128) == 0 and size(0, 1, 8, 8, 128) == 0 and size(1, 1, 8, 3, 64) == 0
    tile, W = kl.attn_plan(1, 1, 32, 8, 128)
    assert tile >= 16 and 1 <= W and size(1, 1, 32, 8, 128) >= 8 * W * 4 * 130 * 4


def test_wrappers_refuse_host_tensors():
    import torch

    import kernels
    import kernels._lib as kl
    z = torch.zeros(2, 1024, dtype=torch.float16)
    b8, n = torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        kernels.attn_decode("f16", z, b8, b8, (2048, 256, 4096), n, 2, 2, 1, 8, 8, 128, b8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        kl.kv_append("q8_0", z, z, b8, b8, (1088, 136, 4096), n, 2, 2, 1, 8, 128)
    assert kernels.KVCache.__name__ == "KVCache"
    with pytest.raises(ValueError, match="kind"):
        kernels.KVCache(1, 8, 1, 64, kind="q4_0", device="cpu")
