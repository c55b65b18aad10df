"""Host side of the latent attention entries (gq_mla_decode, gq_mla_append, gq_mla_decode_workspace_size):
every refusal answers before a launch (fake pointers), with gq_last_error set; the workspace size is
monotone and exactly what the call demands.  CPU only."""
import ctypes

import pytest

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
MB = 1 << 20
Q, C, LEN, O, WS, CKV, KPE, QPE, FREQ, NW = (ctypes.c_void_p(i * 64 * MB) for i in range(1, 11))
BASE = dict(q=Q, ldq=16 * 576, c=C, tok=1152, seq=1152 * 64, kv_len=LEN, cap=64, o=O, ldo=16 * 512, scale=0.07, B=2, N=2,
            n_head=16, rank=512, rope=64, ws=WS, nbytes=1024 * MB,
            mode=0, ckv=CKV, ldc=576, kpe=KPE, ldk=576, qpe=QPE, ldqp=16 * 192 - 128, qhs=192, freq=FREQ, nw=NW)


def _decode(L, **kw):
    a = dict(BASE, **kw)
    return L.gq_mla_decode(a["q"], a["ldq"], a["c"], a["tok"], a["seq"], a["kv_len"], a["cap"], a["o"], a["ldo"], a["scale"],
                           a["B"], a["N"], a["n_head"], a["rank"], a["rope"], a["ws"], a["nbytes"], None)


def _append(L, **kw):
    a = dict(BASE, **kw)
    return L.gq_mla_append(a["mode"], a["ckv"], a["ldc"], a["kpe"], a["ldk"], a["qpe"], a["ldqp"], a["qhs"], a["q"], a["ldq"],
                           a["c"], a["tok"], a["seq"], a["kv_len"], a["cap"], a["freq"], 1.0, a["nw"], 1e-6, a["B"], a["N"],
                           a["n_head"], a["rank"], a["rope"], None)


REFUSED = [
    (_decode, "null Q", dict(q=None), EINVAL, b"null"),
    (_decode, "null C", dict(c=None), EINVAL, b"null"),
    (_decode, "null kv_len", dict(kv_len=None), EINVAL, b"null"),
    (_decode, "null O", dict(o=None), EINVAL, b"null"),
    (_decode, "negative B", dict(B=-1), EINVAL, b"negative"),
    (_decode, "negative N", dict(N=-2), EINVAL, b"negative"),
    (_decode, "negative capacity", dict(cap=-1), EINVAL, b"negative"),
    (_decode, "ldq short", dict(ldq=16 * 576 - 1), EINVAL, b"ldq"),
    (_decode, "ldo short", dict(ldo=16 * 512 - 1), EINVAL, b"ldo"),
    (_decode, "null workspace", dict(ws=None), EINVAL, b"workspace"),
    (_decode, "short workspace", dict(nbytes=1024), EINVAL, b"workspace"),
    (_decode, "unaligned workspace", dict(ws=ctypes.c_void_p(WS.value + 8)), EINVAL, b"aligned"),
    (_decode, "N = 5", dict(N=5), EUNSUPPORTED, b"at most 4"),
    (_decode, "129 heads", dict(n_head=129, ldq=129 * 576, ldo=129 * 512), EUNSUPPORTED, b"at most 128"),
    (_decode, "rank 256", dict(rank=256), EUNSUPPORTED, b"(512, 64)"),
    (_decode, "rope 32", dict(rope=32), EUNSUPPORTED, b"(512, 64)"),
    (_decode, "odd stride", dict(tok=1153), EUNSUPPORTED, b"multiples of 2"),
    (_decode, "rows overlap", dict(tok=1150), EUNSUPPORTED, b"tok_stride"),
    (_decode, "capacity < N", dict(cap=1), EUNSUPPORTED, b"capacity"),
    (_decode, "1 GiB span", dict(cap=MB), EUNSUPPORTED, b"1 GiB"),
    (_append, "null Ckv", dict(ckv=None), EINVAL, b"null"),
    (_append, "null Kpe", dict(kpe=None), EINVAL, b"null"),
    (_append, "null Qpe", dict(qpe=None), EINVAL, b"null"),
    (_append, "null Qout", dict(q=None), EINVAL, b"null"),
    (_append, "null inv_freq", dict(freq=None), EINVAL, b"null"),
    (_append, "null norm_w", dict(nw=None), EINVAL, b"null"),
    (_append, "ldc short", dict(ldc=511), EINVAL, b"ldc"),
    (_append, "ldk short", dict(ldk=63), EINVAL, b"ldk"),
    (_append, "head stride short", dict(qhs=32), EINVAL, b"q_head_stride"),
    (_append, "ldqp short", dict(ldqp=15 * 192 + 63), EINVAL, b"ldqp"),
    (_append, "ldqo short", dict(ldq=16 * 576 - 2), EINVAL, b"ldqo"),
    (_append, "negative n_head", dict(n_head=-1), EINVAL, b"negative"),
    (_append, "unknown mode", dict(mode=2), EUNSUPPORTED, b"rope mode"),
    (_append, "rank 1024", dict(rank=1024, ldc=1024, ldq=16 * 1088, tok=2176), EUNSUPPORTED, b"(512, 64)"),
    (_append, "seq stride odd", dict(seq=7), EUNSUPPORTED, b"multiples of 2"),
    (_append, "capacity < N", dict(cap=1), EUNSUPPORTED, b"capacity"),
]


@pytest.mark.parametrize("call,kw,status,text", [c[:1] + c[2:] for c in REFUSED], ids=[f"{c[0].__name__[1:]}: {c[1]}" for c in REFUSED])
def test_mla_entries_refuse_before_a_launch(call, kw, status, text):
    import kernels._lib as kl
    L = kl.lib()
    assert call(L, **kw) == status, L.gq_last_error()
    assert text in L.gq_last_error(), L.gq_last_error()


@pytest.mark.parametrize("call,kw", [(_decode, dict(B=0, q=None, o=None, ws=None, nbytes=0)), (_decode, dict(N=0, c=None, ws=None)),
                                     (_decode, dict(n_head=0, ldq=0, ldo=0, ws=None)), (_append, dict(B=0, ckv=None)),
                                     (_append, dict(N=0, c=None)), (_append, dict(n_head=0, ldqp=0, ldq=0))])
def test_empty_calls_are_no_ops(call, kw):
    import kernels._lib as kl
    assert call(kl.lib(), **kw) == OK


@pytest.mark.parametrize("cus", [0, 80])
def test_workspace_size_is_monotone_and_exact(cus, tune):
    import kernels._lib as kl
    tune(GQ_CUS=cus)
    L = kl.lib()
    size = L.gq_mla_decode_workspace_size
    for B in (1, 2, 3, 7, 64, 300):
        for N in (1, 2, 4):
            for nh in (1, 16, 20, 64, 65, 128):
                need = size(B, N, nh, 512, 64)
                assert need > 0 and need % 16 == 0
                for B2, N2, nh2 in ((B + 1, N, nh), (B, N + 1, nh), (B, N, nh + 1)):
                    if N2 <= 4 and nh2 <= 128:
                        assert size(B2, N2, nh2, 512, 64) >= need, (B, N, nh)
                kw = dict(B=B, N=N, n_head=nh, ldq=nh * 576, ldo=nh * 512)
                assert _decode(L, nbytes=need, **{**kw, "rank": 256}) == EUNSUPPORTED  # (the shape is judged before the workspace)
                assert _decode(L, nbytes=need - 1, **kw) == EINVAL and str(need).encode() in L.gq_last_error()
    # refused or empty: nothing to size
    assert size(1, 5, 16, 512, 64) == 0 and size(1, 1, 129, 512, 64) == 0 and size(0, 1, 16, 512, 64) == 0 and size(1, 1, 16, 512, 32) == 0
    tile, rows, W = kl.mla_plan(1, 1, 128)
    assert tile == 32 and rows == 64 and W >= 1 and size(1, 1, 128, 512, 64) >= 2 * W * 64 * 514 * 4


def test_wrappers_refuse_host_tensors_and_shapes():
    import torch

    import kernels
    z, b8, n = torch.zeros(2, 16 * 576, dtype=torch.float16), torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        kernels.mla_decode(z, b8, (1152, 4608), n, 4, 2, 1, 16, b8, 0.1)
    with pytest.raises(ValueError, match="rank"):
        kernels.MLACache(1, 8, rank=256, device="cpu")
    c = kernels.MLACache(2, 8, device="cpu")
    assert c.strides == (1152, 8 * 1152) and c.c.numel() == 2 * 8 * 1152
