"""The guards of tests/strided.py catch a planted overwrite and name where it is, and the strided
entry points refuse a stride shorter than the row before they launch anything.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch

import strided as S

N, M, LDC, LEAD = 5, 37, 40, 3


def test_wide_out_passes_untouched_and_written_inside():
    flat, view, check = S.wide_out(N, M, LDC, LEAD, "cpu")
    assert view.shape == (N, M) and view.stride() == (LDC, 1) and view.dtype == torch.float16
    assert view.data_ptr() - flat.data_ptr() == 2 * (S.GUARD + LEAD)
    assert torch.isnan(flat).all()  # (the sentinel is a NaN: a view left unwritten fails every gate)
    check()
    view.fill_(1.0)  # the whole result, every row's last element included
    check()
    assert int((flat.view(torch.int16) != S.SENTINEL).sum()) == N * M


@pytest.mark.parametrize("where,offset,named", [
    ("the first pad column of a middle row", 2 * LDC + M, (2, M)),
    ("the last pad column of a middle row", 3 * LDC - 1, (2, LDC - 1)),
    ("the element after the last row's M", (N - 1) * LDC + M, (N - 1, M)),
    ("the guard before the view", -1, (-1, LDC - 1)),
    ("the allocation's first element", -(S.GUARD + LEAD), divmod(-(S.GUARD + LEAD), LDC)),
])
def test_wide_out_names_a_planted_element(where, offset, named):
    flat, view, check = S.wide_out(N, M, LDC, LEAD, "cpu")
    view.fill_(0.5)
    flat[S.GUARD + LEAD + offset] = 0.0
    with pytest.raises(AssertionError, match=rf"\(row {named[0]}, column {named[1]}\), 1 elements"):
        check()


def test_wide_out_catches_the_last_guard_element_and_a_contiguous_overrun():
    flat, view, check = S.wide_out(N, M, M, 0, "cpu")  # ldc == M: only the guards
    check()
    flat[-1] = 1.0
    with pytest.raises(AssertionError, match="row"):
        check()
    flat, view, check = S.wide_out(N, M, M, 0, "cpu")
    flat[S.GUARD + N * M] = 1.0  # one element too many behind the last row
    with pytest.raises(AssertionError, match=rf"\(row {N}, column 0\)"):
        check()


@pytest.mark.parametrize("poison", (S.INF, S.FMAX))
def test_wide_in_holds_b_and_poison_everywhere_else(poison):
    B = np.arange(N * 32, dtype=np.float16).reshape(N, 32)
    ldb, lead = 35, 1
    v = S.wide_in(B, ldb, lead, poison, "cpu")
    assert v.stride() == (ldb, 1) and np.array_equal(v.numpy(), B)
    assert v.data_ptr() % 16 == 2 * lead
    flat = torch.as_strided(v, (v.untyped_storage().nbytes() // 2,), (1,), 0)
    start = S.GUARD + lead
    assert flat.numel() >= start + (N + 16) * ldb
    e = torch.arange(flat.numel()) - start
    inside = (e >= 0) & (e < (N - 1) * ldb + 32) & (e % ldb < 32)
    assert bool((flat[~inside] == poison).all()) and int((~inside).sum()) == flat.numel() - N * 32


def test_guarded_ws_names_the_byte_after_need():
    need = 1000
    alloc, front, check = S.guarded_ws(need, "cpu")
    assert alloc.numel() == need + 4096 and front.numel() == need and front.data_ptr() == alloc.data_ptr()
    assert bool((alloc[need:] == 0xA5).all())
    check()
    front.zero_()
    check()
    alloc[need] = 0
    with pytest.raises(AssertionError, match=rf"first at byte {need}, 1 bytes"):
        check()
    alloc, front, check = S.guarded_ws(0, "cpu")
    assert front.numel() == 0
    alloc[-1] = 1
    with pytest.raises(AssertionError, match="first at byte 4095"):
        check()


def test_short_strides_are_refused_before_any_launch():
    """ldb < K, ldc < M, ldw < K, ldx < K: GQ_EINVAL from the host-side checks (the pointers are
    not device memory: a launch would fault), with the stride named in gq_last_error."""
    import kernels._lib as kl
    L = kl.lib()
    p, big = ctypes.c_void_p(4096), 1 << 30
    for t, K in ((kl.GQ_Q4_K, 256), (kl.GQ_Q8_0, 96), (kl.GQ_Q4_0, 96), (kl.GQ_Q2_K, 512)):
        for act in (kl.GQ_ACT_Q8_1, kl.GQ_ACT_FP8_E4M3):
            if act == kl.GQ_ACT_FP8_E4M3 and (K % 256 or t > kl.GQ_Q6_K):
                continue
            for n in (1, 4, 20, 64):
                assert L.gq_mmq_ex(t, act, p, p, p, 8, n, K, K - 1, 8, p, big, None) == kl.GQ_EINVAL
                assert b"ldb" in L.gq_last_error()
                assert L.gq_mmq_ex(t, act, p, p, p, 8, n, K, K, 7, p, big, None) == kl.GQ_EINVAL
                assert b"ldc" in L.gq_last_error()
                assert L.gq_mmq_prepared_ex(t, act, p, p, big, p, 8, n, K, 7, None) == kl.GQ_EINVAL
                assert b"ldc" in L.gq_last_error()
                assert L.gq_act_prepare_ex(act, p, n, K, K - 1, p, big, None) == kl.GQ_EINVAL
                assert b"ldb" in L.gq_last_error()
        assert L.gq_mmq(t, p, p, p, 8, 4, K, K - 1, 8, p, big, None) == kl.GQ_EINVAL
        assert L.gq_mmq_prepared(t, p, p, big, p, 8, 4, K, 7, None) == kl.GQ_EINVAL
        assert L.gq_act_prepare(p, 4, K, K - 1, p, big, None) == kl.GQ_EINVAL
        assert L.gq_dequantize(t, p, p, 8, K, K - 1, None) == kl.GQ_EINVAL
        assert b"ldw" in L.gq_last_error()
        assert L.gq_quantize_q8_1(p, p, 4, K, K - 1, None) == kl.GQ_EINVAL
        assert b"ldx" in L.gq_last_error()
        assert L.gq_quantize_fp8(p, p, p, 4, K, K - 1, None) == kl.GQ_EINVAL
        assert b"ldx" in L.gq_last_error()
