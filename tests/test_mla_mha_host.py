"""Host side of the un-absorbed MLA prompt pass (gq_mla_kv_expand, gq_mla_prefill_mha): the ctypes table and the
library agree, gq_version() is unchanged, every refusal answers before a launch (fake pointers) with the header's
status in the header's order, the empty problem is a no-op, and the plan takes 128-row blocks where they still give
every compute unit (256 without a device) a workgroup.  CPU only."""
import ctypes

import pytest

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
MB = 1 << 20
P = [ctypes.c_void_p(i * 64 * MB) for i in range(1, 8)]
H, CAP = 16, 256
EXPAND = dict(w=P[0], c=P[1], tok=1152, seq=CAP * 1152, kv_len=P[2], capacity=CAP, kv=P[3], ktok=H * 512, kseq=CAP * H * 512,
              kcap=CAP, B=2, N=65, n_head=H, rank=512, dim=128)
MHA = dict(EXPAND, qn=P[4], ldqn=H * 192, qnhs=192, qp=P[5], ldqp=H * 576, qphs=576, o=P[6], ldo=H * 128, rope_dim=64)


def _expand(L, **kw):
    a = dict(EXPAND, **kw)
    return L.gq_mla_kv_expand(a["w"], a["c"], a["tok"], a["seq"], a["kv_len"], a["capacity"], a["kv"], a["ktok"], a["kseq"], a["kcap"],
                              a["B"], a["N"], a["n_head"], a["rank"], a["dim"], None)


def _mha(L, **kw):
    a = dict(MHA, **kw)
    return L.gq_mla_prefill_mha(a["qn"], a["ldqn"], a["qnhs"], a["qp"], a["ldqp"], a["qphs"], a["kv"], a["ktok"], a["kseq"], a["kcap"],
                                a["c"], a["tok"], a["seq"], a["kv_len"], a["capacity"], a["o"], a["ldo"], 0.07, a["B"], a["N"],
                                a["n_head"], a["rank"], a["rope_dim"], a["dim"], None)


# every case breaks one thing; where two are broken the earlier check must answer
REFUSED = [
    (_expand, "negative N", dict(N=-1, w=None), EINVAL, b"negative"),
    (_expand, "null W", dict(w=None, rank=256), EINVAL, b"null"),
    (_expand, "null KV", dict(kv=None), EINVAL, b"null"),
    (_expand, "rank 256", dict(rank=256, n_head=129), EUNSUPPORTED, b"(512, 128)"),
    (_expand, "dim 64", dict(dim=64), EUNSUPPORTED, b"(512, 128)"),
    (_expand, "129 heads", dict(n_head=129, ktok=8), EUNSUPPORTED, b"at most 128"),
    (_expand, "odd cache stride", dict(tok=1153), EUNSUPPORTED, b"multiples of 2"),
    (_expand, "N above the capacity", dict(N=CAP + 1, ktok=8), EUNSUPPORTED, b"cannot hold"),
    (_expand, "kv_tok_stride no multiple of 16", dict(ktok=H * 512 + 8), EUNSUPPORTED, b"multiples of 16"),
    (_expand, "kv_tok_stride short", dict(ktok=H * 512 - 16), EUNSUPPORTED, b"n_head*512"),
    (_expand, "no kv_capacity", dict(kcap=0), EUNSUPPORTED, b"kv_capacity"),
    (_expand, "1 GiB of KV", dict(n_head=128, ktok=128 * 512, kcap=16385, w=ctypes.c_void_p(8)), EUNSUPPORTED, b"1 GiB"),
    (_expand, "W misaligned", dict(w=ctypes.c_void_p(64 * MB + 8)), EINVAL, b"16-byte"),
    (_mha, "null Qp", dict(qp=None, ldqn=1), EINVAL, b"null"),
    (_mha, "qn_head_stride short", dict(qnhs=120), EINVAL, b"qn_head_stride"),
    (_mha, "qp_head_stride short", dict(qphs=56), EINVAL, b"qp_head_stride"),
    (_mha, "ldqn short", dict(ldqn=15 * 192 + 120), EINVAL, b"ldqn"),
    (_mha, "ldqp short", dict(ldqp=15 * 576 + 56), EINVAL, b"ldqp"),
    (_mha, "ldo short", dict(ldo=H * 128 - 4, rank=256), EINVAL, b"ldo"),
    (_mha, "negative B", dict(B=-1), EINVAL, b"negative"),
    (_mha, "rope_dim 32", dict(rope_dim=32, qphs=32, ldqp=H * 32), EUNSUPPORTED, b"(512, 64)"),
    (_mha, "N above the capacity", dict(N=CAP + 1, dim=64), EUNSUPPORTED, b"cannot hold"),
    (_mha, "dim 64", dict(dim=64, ktok=8), EUNSUPPORTED, b"(512, 128)"),
    (_mha, "kv_tok_stride short", dict(ktok=H * 512 - 16, qn=ctypes.c_void_p(64 * MB + 2)), EUNSUPPORTED, b"n_head*512"),
    (_mha, "2^31 rows", dict(B=1 << 17, N=128, n_head=128, capacity=128, tok=1152, ldqn=128 * 192, ldqp=128 * 576, ldo=128 * 128,
                             ktok=128 * 512), EUNSUPPORTED, b"2^31"),
    (_mha, "Qn misaligned", dict(qn=ctypes.c_void_p(64 * MB + 8), o=ctypes.c_void_p(4)), EINVAL, b"16-byte"),
    (_mha, "qp_head_stride no multiple of 8", dict(qphs=580, ldqp=H * 580), EINVAL, b"16-byte"),
    (_mha, "O misaligned", dict(o=ctypes.c_void_p(64 * MB + 4)), EINVAL, b"8-byte"),
]


@pytest.mark.parametrize("call,kw,status,text", [(c[0],) + c[2:] for c in REFUSED], ids=[f"{c[0].__name__[1:]}: {c[1]}" for c in REFUSED])
def test_refused_before_a_launch(call, kw, status, text):
    import kernels._lib as kl
    L = kl.lib()
    assert call(L, **kw) == status, L.gq_last_error()
    assert text in L.gq_last_error(), L.gq_last_error()


@pytest.mark.parametrize("kw", [dict(B=0), dict(N=0), dict(n_head=0, ktok=0, ldqn=0, ldqp=0, ldo=0)])
def test_the_empty_problem_is_a_no_op(kw):
    import kernels._lib as kl
    none = dict(w=None, c=None, kv=None, kv_len=None, qn=None, qp=None, o=None)
    assert _expand(kl.lib(), **{k: v for k, v in dict(kw, **none).items() if k in EXPAND}) == OK
    assert _mha(kl.lib(), **kw, **none) == OK


def test_signatures_the_library_and_the_version_agree():
    import kernels
    import kernels._lib as kl
    for name in ("gq_mla_kv_expand", "gq_mla_prefill_mha", "gq_debug_mla_prefill_mha_plan"):
        assert name in kl.SIGNATURES and getattr(kl.lib(), name).argtypes == kl.SIGNATURES[name][0]
    assert kl.lib().gq_version() == 105
    assert callable(kernels.mla_kv_expand) and callable(kernels.mla_prefill_mha)


def test_the_plan_takes_128_rows_where_the_chip_stays_full():
    import kernels._lib as kl
    plan = kl.mla_prefill_mha_plan  # -> (rows, tile, grid = B * n_head * ceil(N / rows))
    assert plan(1, 65, 16) == (64, 64, 32) and plan(2, 130, 3) == (64, 64, 18)  # 16 resp. 12 blocks of 128: under 256 units
    assert plan(1, 4096, 16) == (128, 64, 512) and plan(1, 512, 128) == (128, 64, 512) and plan(2, 5, 128) == (128, 64, 256)
    assert plan(1, 2047, 16) == (128, 64, 256) and plan(1, 1920, 16) == (64, 64, 480)  # 15 blocks of 128 x 16 heads = 240
    for bad in ((1, 5, 129), (0, 5, 16), (1 << 17, 128, 128)):
        with pytest.raises(RuntimeError, match="MHA prefill shape"):
            plan(*bad)
