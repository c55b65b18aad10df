"""GPU tests of GGUF Q5_K (GGML type 13): every route -- the streaming decode (alone, grouped, on
the prepared copy), the GEMV fallback, the streaming GEMM (alone, grouped, split-K), dequantize +
hipBLASLt -- against the numpy model of tests/q5k_model.py (the reference has no Q5_K):
max|C - ideal| / max|ideal| <= 1.5e-3 at N <= 4 and 4e-3 otherwise, ideal = x~ @ W^T in fp64 with
x~ from the project's q8_1 quantizer.  Q4_K / Q6_K items of mixed cases use the oracle.  The bodies
shared with the other added types are in tests/gpu_types.py."""
import numpy as np
import pytest
import torch

import gpu_types as G
import kernels._lib as kl
import q5k_model as Q
from gpu_types import no_timeouts_after_each_test  # noqa: F401  (autouse, by import)
from kernels.mmq_q5_k import mmq_q5_k
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

T = G.GpuType("q5_k", Q, mmq_q5_k)
Q5 = T.gtype


# ---- 1. parity, ragged shapes ----
@pytest.mark.parametrize("M,N,K", Q.DECODE_SHAPES)
def test_decode(M, N, K):
    G.check_decode(T, M, N, K)


@pytest.mark.parametrize("M,N,K", Q.LONG_SHAPES)
def test_long_rows(M, N, K):
    """Rows of several ring segments: one token in the streaming decode (K = 16640: five cached
    units per lane); 2-3 tokens of such rows do not fit LDS beside the ring and take the GEMV."""
    assert kl.route_name(Q5, M, N, K) == kl.route_name(kl.GQ_Q4_K, M, N, K)  # (decode_fused_ok(Q5_K) is Q4_K's)
    G.check_long_rows(T, M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMV_SHAPES)
def test_gemv_fallback(M, N, K):
    """4 tokens at K = 11008 do not fit LDS beside the ring: act_quant + gemv_kernel."""
    G.check_gemv(T, M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMM_SHAPES + Q.SPLITK_SHAPES)
def test_gemm(M, N, K):
    G.check_gemm(T, M, N, K)


@pytest.mark.parametrize("M,N,K", [(4096, 1, 4096), (4096, 4, 4096), (11008, 2, 4096), (4096, 1, 11008),
                                   (4096, 3, 11008), (4096, 16, 4096), (11008, 128, 4096), (4096, 40, 11008),
                                   (512, 768, 1024)])
def test_llama_shapes_sampled_rows(M, N, K):
    """The Llama-7B shapes (many tasks per wave, several rows per task, K = 11008's 43 super-blocks,
    every row tile of the GEMM, the default BLAS threshold): 192 sampled rows against the model."""
    raw, B = random_blocks("q5_k", M, K, seed=M + N), random_activations(N, K, seed=K + N)
    got = G.run(T, raw, B, M, N, K)
    rows = np.sort(np.random.default_rng(N).choice(M, size=192, replace=False))
    rb = T.row_bytes(K)
    sub = np.concatenate([raw[r * rb:(r + 1) * rb] for r in rows])
    err = Q.rel_err(got[:, rows], Q.ideal(sub, B, len(rows), N, K))
    print(f"q5_k {M}x{N}x{K}: max|d|/max|C| = {err:.2e} (sampled rows)")
    assert err <= Q.tight(N), (M, N, K, err)
    G.no_timeouts()


def test_splitk_shapes_split():
    G.check_splitk_shapes_split(T)


# ---- 2. gq_dequantize ----
def test_dequantize_bit_equal():
    G.check_dequantize_bit_equal(T)


# ---- 3. dequant + hipBLASLt ----
@pytest.mark.parametrize("M,N,K", Q.BLAS_SHAPES)
def test_blas_path(M, N, K, tune):
    G.check_blas_path(T, M, N, K, tune)


# ---- 4. routes ----
def test_routes(tune):
    assert "stream_decode_kernel" in kl.route_name(Q5, 4096, 1, 4096)
    assert "stream_decode_kernel" in kl.route_name(Q5, 4096, 1, 4096, prepared=True)
    for M, N in ((4096, 16), (4096, 128), (11008, 16), (11008, 128)):
        for prepared in (False, True):
            assert "sgemm" in kl.route_name(Q5, M, N, 4096, prepared=prepared), (M, N, prepared)
    assert "hipBLASLt" in kl.route_name(Q5, 4096, 1024, 4096)
    assert kl.route_name(Q5, 4096, 16, 4096, act="fp8") == "none"


@pytest.mark.parametrize("knob", ["GQ_RGEMM", "GQ_SKINNY", "GQ_KSTREAM", "GQ_GEMM_SPLITS", "GQ_SGEMM"])
def test_forced_routes_keep_sgemm(knob, tune):
    """Q5_K has no resident, K-chunked, skinny or LDS-DMA GEMM form: a knob that forces one (or
    turns the streaming GEMM off for the other types) leaves it on the streaming GEMM."""
    G.check_forced_routes_keep_sgemm(T, knob, tune)


def test_row_chunks_under_the_launch_limit(tune):
    """A call over the per-launch byte limit (lowered here) is cut into 256-row chunks, each on the
    streaming GEMM: the bits of the one-launch call (rows are independent; splits pinned)."""
    G.check_row_chunks_under_the_launch_limit(T, tune, 140000)  # (256 rows of 352 bytes per launch; the 24 tokens' x~ fits)


# ---- 5. invariants ----
@pytest.mark.parametrize("N", [2, 24])
def test_activation_scaling_is_exact(N):
    G.check_activation_scaling_is_exact(T, N)


@pytest.mark.parametrize("N", [3, 24])
def test_row_independence(N, tune):
    G.check_row_independence(T, N, tune)


# ---- 6. prepared form ----
@pytest.mark.parametrize("N", [2, 24])
def test_prepared(N):
    G.check_prepared(T, N)


# ---- 7. grouped decode ----
_GROUP = (("q5_k", 96, 512), ("q6_k", 64, 768), ("q4_k", 96, 512), ("q5_k", 64, 768))


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_grouped_decode_bit_identical(N):
    G.check_grouped_decode_bit_identical(_GROUP, N)


def test_grouped_at_gemm_tokens_is_refused():
    G.check_grouped_at_gemm_tokens_is_refused(_GROUP)


def test_grouped_decode_long_rows_with_q5_k_refused():
    """A one-token grouped launch that holds a Q5_K item carries every format's cases up to 4
    cached chunks per lane (K <= 16384): beyond that the launch is refused, nothing runs, and each
    item's own call (the streaming decode) stands."""
    K = 20480
    items = G.grouped_items((("q5_k", 16, K), ("q4_k", 16, K)), 1)
    assert kl.mmq_grouped(items, 1) is None
    assert kl.mmq_grouped(items[1:], 1) is not None  # (without the Q5_K item: the other formats' kernel)
    torch.cuda.synchronize()
    raw = random_blocks("q5_k", 16, K, seed=0)
    B = random_activations(1, K, seed=0)
    assert "stream_decode_kernel" in kl.route_name(Q5, 16, 1, K)
    assert Q.rel_err(G.run(T, raw, B, 16, 1, K), Q.ideal(raw, B, 16, 1, K)) <= Q.TIGHT_GEMV


# ---- 8. grouped prepared (the streaming GEMM) ----
@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("splits", [1, 2])
def test_grouped_prepared_bit_identical(N, splits, tune):
    group = (("q5_k", 300, 512), ("q6_k", 64, 768), ("q5_k", 64, 768), ("q6_k", 96, 512))
    G.check_grouped_prepared_bit_identical(T, group, N, splits, tune)


# ---- 9. a Q5_K_M layer from a GGUF file ----
@pytest.mark.parametrize("fuse", [True, False])
def test_layer_mix_from_gguf(tmp_path, fuse):
    from gguf import q5_k_m_layer_types
    types = q5_k_m_layer_types(0, 32)  # layer 0: attn_v / ffn_down in Q6_K
    G.check_layer_mix_from_gguf(T, tmp_path, fuse, types, {"q5_k", "q6_k"})
