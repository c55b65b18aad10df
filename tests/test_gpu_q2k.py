"""GPU tests of GGUF Q2_K (GGML type 10): every route -- the streaming decode (alone, grouped, on
the prepared copy, expert-indexed), the GEMV fallback, the streaming GEMM (alone, grouped,
split-K, row-chunked, sorted by expert), dequantize + hipBLASLt.  The judge is the fp64 ideal of
tests/q2k_model.py on the oracle's q8_1 blocks (tied to the reference's Q6_K oracle on the host,
tests/test_q2k_host.py): max|C - ideal| / max|ideal| <= 1.5e-3 at N <= 4 and 4e-3 otherwise.
Q4_K / Q6_K items of mixed cases use the oracle directly, Q5_K and Q3_K items their own models
(tests/type_models.py judge).  The bodies shared with the other added types are in
tests/gpu_types.py."""
import pytest

import gpu_types as G
import kernels._lib as kl
import q2k_model as Q
from gpu_types import no_timeouts_after_each_test  # noqa: F401  (autouse, by import)
from kernels.mmq_q2_k import mmq_q2_k

pytestmark = pytest.mark.gpu

T = G.GpuType("q2_k", Q, mmq_q2_k)
Q2 = T.gtype


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
    """4 tokens at K = 11008, and at K = 8960 (the first multiple of 256 over the limit of Q3_K's
    activation image, which Q2_K shares), do not fit LDS beside the ring: act_quant + gemv_kernel."""
    G.check_gemv(T, M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMM_SHAPES + Q.SPLITK_SHAPES)
def test_gemm(M, N, K):
    G.check_gemm(T, M, N, K)


def test_splitk_shapes_split():
    G.check_splitk_shapes_split(T)


def test_one_token_seven_cached_chunks():
    """K = 28672 at one token: seven cached units per lane, the most Q2_K's decode carries (Q3_K
    and Q5_K stop at six); beside the shape lists, which are Q3_K's."""
    G.check_decode(T, 8, 1, 28672)


# ---- 2. gq_dequantize ----
def test_dequantize_bit_equal():
    G.check_dequantize_bit_equal(T)


# ---- 3. dequant + hipBLASLt ----
@pytest.mark.parametrize("M,N,K", Q.BLAS_SHAPES)
def test_blas_path(M, N, K, tune):
    G.check_blas_path(T, M, N, K, tune)


# ---- 4. routes ----
def test_routes(tune):
    assert "stream_decode_kernel" in kl.route_name(Q2, 4096, 1, 4096)
    assert "stream_decode_kernel" in kl.route_name(Q2, 4096, 1, 4096, prepared=True)
    assert "stream_decode_kernel" in kl.route_name(Q2, 4096, 4, 4096)
    assert kl.route_name(Q2, 4096, 4, 11008) == "gemv_kernel"
    for M, N in ((4096, 5), (4096, 16), (4096, 128), (11008, 16), (11008, 128), (4096, 767)):
        for prepared in (False, True):
            assert "sgemm" in kl.route_name(Q2, M, N, 4096, prepared=prepared), (M, N, prepared)
    assert "hipBLASLt" in kl.route_name(Q2, 4096, 768, 4096)
    assert "hipBLASLt" in kl.route_name(Q2, 4096, 1024, 4096)
    assert kl.route_name(Q2, 4096, 16, 4096, act="fp8") == "none"
    assert kl.route_name(Q2, 4096, 16, 4000) == "none"


@pytest.mark.parametrize("knob", ["GQ_RGEMM", "GQ_SKINNY", "GQ_KSTREAM", "GQ_GEMM_SPLITS", "GQ_SGEMM"])
def test_forced_routes_keep_sgemm(knob, tune):
    """Q2_K has no resident, K-chunked, skinny or LDS-DMA GEMM form: a knob that forces one (or
    turns the streaming GEMM off for the other types) leaves it on the streaming GEMM."""
    G.check_forced_routes_keep_sgemm(T, knob, tune)


def test_row_chunks_under_the_launch_limit(tune):
    """A call over the per-launch byte limit (lowered here) is cut into row chunks, each on the
    streaming GEMM: the bits of the one-launch call (rows are independent; splits pinned).

    512 rows of 168 bytes per launch (512 + 88).  The 24 tokens' x~ (24 KiB) is counted exactly for
    this type: in whole 128-token tiles, as for the other types, no limit that cuts Q2_K rows at all
    admits more than 16 tokens (gq_capi.hip use_sgemm); Q3_K under the same limit is refused."""
    # (512 rows of 168 bytes = 86016 per launch: 512 + 88; the 24 tokens' x~ fits)
    M, N, K = G.check_row_chunks_under_the_launch_limit(T, tune, 86100)
    assert kl.route_name(kl.GQ_Q3_K, M, N, K) == "none"  # (Q3_K: whole 128-token tiles, 16 tokens at this limit)


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
_GROUP = (("q2_k", 96, 512), ("q3_k", 64, 768), ("q4_k", 96, 512), ("q6_k", 64, 768), ("q5_k", 64, 768),
          ("q2_k", 64, 768))


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_grouped_decode_bit_identical(N):
    G.check_grouped_decode_bit_identical(_GROUP, N)


def test_grouped_at_gemm_tokens_is_refused():
    G.check_grouped_at_gemm_tokens_is_refused(_GROUP)


# ---- 8. grouped prepared (the streaming GEMM) ----
@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("splits", [1, 2])
def test_grouped_prepared_bit_identical(N, splits, tune):
    group = (("q2_k", 300, 512), ("q6_k", 64, 768), ("q3_k", 64, 768), ("q2_k", 96, 512))
    G.check_grouped_prepared_bit_identical(T, group, N, splits, tune)


# ---- 9. MoE ----
def test_mmq_id_bit_identical_to_one_token_calls():
    """gq_mmq_id on Q2_K experts: every pair the bits of its own one-token gq_mmq; an id out of
    range gives zeros."""
    G.check_mmq_id_bit_identical_to_one_token_calls(T)


@pytest.mark.parametrize("M", [70, 300])
def test_mmq_id_sorted_80_pairs(M):
    """gq_mmq_id_sorted at 80 pairs: every pair's row the bits of the one-split streaming GEMM on
    its expert's gathered rows, and within the gate of the oracle."""
    G.check_mmq_id_sorted_80_pairs(T, M)


@pytest.mark.parametrize("N", [3, 40])
def test_moe_ffn_from_gguf(tmp_path, N):
    """MoEFFN.from_gguf on a written 3-D file (Q2_K gate / up, Q3_K down; E=4, S=2, hidden 512, ffn
    256) at 6 pairs (gq_mmq_id) and 80 (the sorted GEMM), against the fp64 model stage by stage: the
    gate and up rows against the oracle on x, the down rows against the oracle on the fp16
    silu(g) * u that the block feeds them, each at the gate of its token count; the block's output
    the bits of the same torch ops on those stage outputs."""
    G.check_moe_ffn_from_gguf(tmp_path, N, ("q2_k", "q2_k", "q3_k"))


# ---- 10. a Q2_K layer from a GGUF file ----
@pytest.mark.parametrize("fuse", [True, False])
def test_layer_mix_from_gguf(tmp_path, fuse):
    from gguf import q2_k_layer_types
    types = q2_k_layer_types(0, 32)  # attn_v, attn_output and ffn_down in Q3_K, the rest in Q2_K
    G.check_layer_mix_from_gguf(T, tmp_path, fuse, types, {"q2_k", "q3_k"})
