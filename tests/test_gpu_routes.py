"""The library's routing as measured (gq_debug_route: the kernels a call launches).  Pins the
defaults DESIGN.md §5 "Round 4" reports, so a routing change is a visible test change."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt,M,N,K,prepared,want", [
    ("q8_0", 4096, 1, 4096, False, "stream_decode_kernel"),
    ("q6_k", 28672, 1, 8192, False, "stream_decode_kernel"),
    ("q8_0", 4096, 128, 4096, False, "rgemm_kernel"),        # the headline: resident split, q8_1 in-kernel
    ("q4_k", 4096, 128, 4096, True, "rgemm_kernel"),
    ("q4_k", 4096, 16, 4096, False, "rgemm_kernel"),         # ahead of the skinny kernel
    ("q4_k", 11008, 16, 4096, False, "kstream_kernel"),      # raw 5..16 tokens on >= 8192 rows (round 5)
    ("q8_0", 11008, 16, 4096, False, "kstream_kernel"),
    ("q4_k", 11008, 32, 4096, False, "rgemm_kernel"),        # up to four resident rounds at <= 32 tokens
    ("q6_k", 11008, 16, 4096, True, "kstream_kernel"),      # prepared 5..32 tokens, K <= 4096 (round 5)
    ("q4_k", 4096, 16, 4096, True, "kstream_kernel"),
    ("q4_k", 22016, 16, 4096, False, "kstream_kernel"),
    ("q4_k", 22016, 24, 4096, False, "rgemm_kernel"),
    ("q8_0", 28672, 16, 8192, False, "skinny_kernel"),        # (more than four rounds)
    ("q6_k", 28672, 16, 8192, True, "sgemm_kernel"),
    ("q6_k", 28672, 128, 8192, True, "sgemm_kernel"),
    ("q4_k", 11008, 128, 4096, True, "sgemm_kernel"),
    ("q6_k", 28672, 512, 8192, True, "sgemm_kernel"),
    ("q4_k", 4096, 1024, 4096, True, "hipBLASLt"),
])
def test_default_routes(fmt, M, N, K, prepared, want):
    import kernels._lib as kl
    assert torch.cuda.is_available()
    got = kl.route_name(kl.TYPES[fmt], M, N, K, prepared=prepared)
    assert want in got, got


@pytest.mark.parametrize("knob,kernel", [("GQ_KSTREAM", "kstream_kernel"), ("GQ_RGEMM", "rgemm_kernel")])
@pytest.mark.parametrize("fmt", ["q4_k", "q8_0"])
def test_raw_call_alignment_fallback(tune, knob, kernel, fmt):
    """A raw call takes the one-launch kernels (activations quantized inside) only when B's rows are
    16-byte aligned (ldb % 8 == 0, B & 15 == 0); gq_debug_route sees the shape alone.  A B that is
    not falls back to act_quant + a prepared kernel: the same result within the GEMM tolerance
    (another kernel may sum over K in another order)."""
    import numpy as np

    import kernels._lib as kl
    import oracle as O
    from test_gpu_route_sweep import GEMM_TOL
    from utils.synth import random_activations, random_blocks
    dev = torch.device("cuda:0")
    t = kl.TYPES[fmt]
    tune(**{knob: 1})
    M, N, K = 256, 16, 512
    for step in range(10):  # the smallest shape the forced kernel takes, M and K doubled in turn
        if kernel in kl.route_name(t, M, N, K, prepared=False):
            break
        M, K = (2 * M, K) if step % 2 == 0 else (M, 2 * K)
    assert kernel in kl.route_name(t, M, N, K, prepared=False), (M, N, K, kl.route_name(t, M, N, K))
    A = torch.from_numpy(np.ascontiguousarray(random_blocks(fmt, M, K, seed=11).view(np.int8))).to(dev)
    B = torch.from_numpy(random_activations(N, K, seed=12)).to(dev)
    strided = torch.zeros((N, K + 4), dtype=torch.float16, device=dev)[:, :K]  # ldb % 8 == 4
    strided.copy_(B)
    shifted = torch.zeros(N * K + 8, dtype=torch.float16, device=dev)[1:1 + N * K].view(N, K)  # B & 15 == 2
    shifted.copy_(B)
    assert B.data_ptr() % 16 == 0 and strided.data_ptr() % 16 == 0 and strided.stride(0) % 8 != 0
    assert shifted.data_ptr() % 16 == 2 and shifted.stride(0) == K
    outs = [kl.mmq(t, A, x, M, N, K) for x in (B, strided, shifted)]
    torch.cuda.synchronize()
    ref = outs[0].cpu().numpy().astype(np.float32)
    assert np.isfinite(ref).all()
    for name, o in zip(("ldb % 8 != 0", "B & 15 != 0"), outs[1:]):
        got = o.cpu().numpy()
        assert np.isfinite(got.astype(np.float32)).all(), name
        err = O.max_rel_err(got, ref)
        print(f"{fmt} {knob}=1 {M}x{N}x{K} {name}: max rel err {err:.3g}")
        assert err <= GEMM_TOL, (name, err)
    # and every one of them against the oracle, at the GEMM gate of the type tests
    import type_models as TM
    want = O.mmq_from_fp16(fmt, random_blocks(fmt, M, K, seed=11), random_activations(N, K, seed=12), M, N, K, O.IDEAL)
    for name, o in zip(("aligned", "ldb % 8 != 0", "B & 15 != 0"), outs):
        err = TM.rel_err(o.cpu().numpy(), want)
        print(f"{fmt} {knob}=1 {M}x{N}x{K} {name}: max|d|/max|C| = {err:.2e} vs the oracle")
        assert err <= TM.tight(N), (name, err)


def test_route_knobs(tune):
    import kernels._lib as kl
    tune(GQ_GEMM_SPLITS=4)  # a GEMM knob pins the LDS-DMA GEMM
    assert "gemm_kernel" in kl.route_name(kl.GQ_Q8_0, 4096, 128, 4096) and "rgemm" not in kl.route_name(kl.GQ_Q8_0, 4096, 128, 4096)
    tune(GQ_GEMM_SPLITS=0, GQ_SGEMM_STREAMK=1)
    assert "stream-K" in kl.route_name(kl.GQ_Q6_K, 28672, 128, 8192, prepared=True)
