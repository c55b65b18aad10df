"""GPU tests of GGUF Q3_K (GGML type 11): every route -- the streaming decode (alone, grouped, on
the prepared copy, expert-indexed), the GEMV fallback, the streaming GEMM (alone, grouped,
split-K, row-chunked, sorted by expert), dequantize + hipBLASLt.  The judge is the reference's
Q6_K arithmetic on the losslessly transcoded blocks (tests/q3k_model.py to_q6_k, oracle IDEAL):
max|C - ideal| / max|ideal| <= 1.5e-3 at N <= 4 and 4e-3 otherwise.  Q4_K / Q6_K items of mixed
cases use the oracle directly, Q5_K items tests/q5k_model.py (tests/type_models.py judge).  The
bodies shared with the other added types are in tests/gpu_types.py."""
import pytest

import gpu_types as G
import kernels._lib as kl
import q3k_model as Q
from gpu_types import no_timeouts_after_each_test  # noqa: F401  (autouse, by import)
from kernels.mmq_q3_k import mmq_q3_k

pytestmark = pytest.mark.gpu

T = G.GpuType("q3_k", Q, mmq_q3_k)
Q3 = T.gtype


# ---- 1. parity, ragged shapes ----
@pytest.mark.parametrize("M,N,K", Q.DECODE_SHAPES)
def test_decode(M, N, K):
    G.check_decode(T, M, N, K)


@pytest.mark.parametrize("M,N,K", Q.LONG_SHAPES)
def test_long_rows(M, N, K):
    """Rows of several ring segments: one token in the streaming decode (K = 16640: five cached
    units per lane); 2-3 tokens of such rows do not fit LDS beside the ring and take the GEMV."""
    G.check_long_rows(T, M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMV_SHAPES)
def test_gemv_fallback(M, N, K):
    """4 tokens at K = 11008, and at K = 8960 (the first multiple of 256 over Q3_K's own limit), do
    not fit LDS beside the ring: act_quant + gemv_kernel."""
    G.check_gemv(T, M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMM_SHAPES + Q.SPLITK_SHAPES)
def test_gemm(M, N, K):
    G.check_gemm(T, M, N, K)


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
    assert "stream_decode_kernel" in kl.route_name(Q3, 4096, 1, 4096)
    assert "stream_decode_kernel" in kl.route_name(Q3, 4096, 1, 4096, prepared=True)
    assert "stream_decode_kernel" in kl.route_name(Q3, 4096, 4, 4096)
    assert kl.route_name(Q3, 4096, 4, 11008) == "gemv_kernel"
    for M, N in ((4096, 5), (4096, 16), (4096, 128), (11008, 16), (11008, 128), (4096, 767)):
        for prepared in (False, True):
            assert "sgemm" in kl.route_name(Q3, M, N, 4096, prepared=prepared), (M, N, prepared)
    assert "hipBLASLt" in kl.route_name(Q3, 4096, 768, 4096)
    assert "hipBLASLt" in kl.route_name(Q3, 4096, 1024, 4096)
    assert kl.route_name(Q3, 4096, 16, 4096, act="fp8") == "none"
    assert kl.route_name(Q3, 4096, 16, 4000) == "none"


@pytest.mark.parametrize("knob", ["GQ_RGEMM", "GQ_SKINNY", "GQ_KSTREAM", "GQ_GEMM_SPLITS", "GQ_SGEMM"])
def test_forced_routes_keep_sgemm(knob, tune):
    """Q3_K has no resident, K-chunked, skinny or LDS-DMA GEMM form: a knob that forces one (or
    turns the streaming GEMM off for the other types) leaves it on the streaming GEMM."""
    G.check_forced_routes_keep_sgemm(T, knob, tune)


def test_row_chunks_under_the_launch_limit(tune):
    """A call over the per-launch byte limit (lowered here) is cut into row chunks, each on the
    streaming GEMM: the bits of the one-launch call (rows are independent; splits pinned)."""
    # (512 rows of 220 bytes per launch: 512 + 88; the 24 tokens' x~ fits)
    G.check_row_chunks_under_the_launch_limit(T, tune, 140000)


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
_GROUP = (("q3_k", 96, 512), ("q6_k", 64, 768), ("q4_k", 96, 512), ("q5_k", 64, 768), ("q3_k", 64, 768))


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_grouped_decode_bit_identical(N):
    G.check_grouped_decode_bit_identical(_GROUP, N)


def test_grouped_at_gemm_tokens_is_refused():
    G.check_grouped_at_gemm_tokens_is_refused(_GROUP)


# ---- 8. grouped prepared (the streaming GEMM) ----
@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("splits", [1, 2])
def test_grouped_prepared_bit_identical(N, splits, tune):
    group = (("q3_k", 300, 512), ("q6_k", 64, 768), ("q3_k", 64, 768), ("q6_k", 96, 512))
    G.check_grouped_prepared_bit_identical(T, group, N, splits, tune)


# ---- 9. MoE ----
def test_mmq_id_bit_identical_to_one_token_calls():
    """gq_mmq_id on Q3_K experts: every pair the bits of its own one-token gq_mmq; an id out of
    range gives zeros."""
    G.check_mmq_id_bit_identical_to_one_token_calls(T)


@pytest.mark.parametrize("M", [70, 300])
def test_mmq_id_sorted_80_pairs(M):
    """gq_mmq_id_sorted at 80 pairs: every pair's row the bits of the one-split streaming GEMM on
    its expert's gathered rows, and within the gate of the oracle."""
    G.check_mmq_id_sorted_80_pairs(T, M)


@pytest.mark.parametrize("N", [3, 40])
def test_moe_ffn_from_gguf(tmp_path, N):
    """MoEFFN.from_gguf on a written 3-D file (Q3_K gate / up, Q4_K down; E=4, S=2, hidden 512, ffn
    256) at 6 pairs (gq_mmq_id) and 80 (the sorted GEMM), against the fp64 model stage by stage: the
    gate and up rows against the oracle on x, the down rows against the oracle on the fp16
    silu(g) * u that the block feeds them, each at the gate of its token count; the block's output
    the bits of the same torch ops on those stage outputs."""
    G.check_moe_ffn_from_gguf(tmp_path, N, ("q3_k", "q3_k", "q4_k"))


# ---- 10. a Q3_K_M layer from a GGUF file ----
@pytest.mark.parametrize("fuse", [True, False])
def test_layer_mix_from_gguf(tmp_path, fuse):
    from gguf import q3_k_m_layer_types
    types = q3_k_m_layer_types(0, 32)  # layer 0: attn_v and ffn_down in Q5_K, attn_output in Q4_K
    G.check_layer_mix_from_gguf(T, tmp_path, fuse, types, {"q3_k", "q4_k", "q5_k"})
