"""GPU tests of GGUF Q4_0 (GGML type 2): every route -- the streaming decode (alone, grouped, on
the prepared copy, expert-indexed), the GEMV (long activations at 1..4 tokens, K % 256 != 0 at any
token count), the streaming GEMM (alone, grouped, split-K, row-chunked, sorted by expert),
dequantize + hipBLASLt, and the device quantizer.  The judge is the reference's Q8_0 oracle (IDEAL)
on the exactly widened blocks (tests/q4_0_model.py widen; pinned on the host by
tests/test_q4_0_host.py): max|C - ideal| / max|ideal| <= 1.5e-3 at N <= 4 and 4e-3 otherwise.
Q4_K / Q6_K / Q8_0 items of mixed cases use the oracle directly.  The bodies shared with the other
added types are in tests/gpu_types.py."""
import numpy as np
import pytest
import torch

import gpu_types as G
import kernels._lib as kl
import q4_0_model as Q
import type_models as TM
from gpu_types import no_timeouts_after_each_test  # noqa: F401  (autouse, by import)
from kernels.mmq_q4_0 import mmq_q4_0
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

T = G.GpuType("q4_0", Q, mmq_q4_0)
Q40 = T.gtype


# ---- 1. parity, ragged shapes ----
@pytest.mark.parametrize("M,N,K", Q.DECODE_SHAPES)
def test_decode(M, N, K):
    """The streaming decode at K = 32 (one block, half a unit), rows that end with half a unit
    (K % 64 == 32) and start 2-byte aligned in the ring, the last K at four tokens, and K = 28672 at
    one token (seven cached chunks per lane, rows cut into ring segments)."""
    G.check_decode(T, M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMV_SHAPES)
def test_gemv(M, N, K):
    """act_quant + gemv_kernel: four tokens whose q8_1 image does not fit LDS beside the ring
    (K = 11008, and K = 10912, the first K over the limit), and K % 256 != 0 at GEMM token counts."""
    G.check_gemv(T, M, N, K)


@pytest.mark.parametrize("M,N,K", Q.GEMM_SHAPES + Q.SPLITK_SHAPES)
def test_gemm(M, N, K):
    G.check_gemm(T, M, N, K)


def test_splitk_shapes_split():
    G.check_splitk_shapes_split(T)


@pytest.mark.parametrize("N", [1, 16])
def test_edge_valued_weights(N):
    """Rows of all-0 nibbles (code -8), all-15 nibbles (+7) and blocks of each in turn: the signed
    nibbles of the decode (N = 1) and the biased pairs of the streaming GEMM (N = 16) at both ends
    of the code range."""
    M, K = 70, 512
    raw = Q.edge_blocks(M, K, seed=2)
    B = random_activations(N, K, seed=N)
    assert ("stream_decode_kernel" if N == 1 else "sgemm") in kl.route_name(Q40, M, N, K)
    err = Q.rel_err(G.run(T, raw, B, M, N, K), Q.ideal(raw, B, M, N, K))
    print(f"q4_0 edge-valued {M}x{N}x{K}: max|d|/max|C| = {err:.2e}")
    assert err <= Q.tight(N), err


# ---- 2. gq_dequantize, gq_quantize_weights ----
def test_dequantize_bit_equal():
    G.check_dequantize_bit_equal(T)


def test_quantize_weights_byte_equal_to_the_host():
    from utils.quantize.q4_0 import quantize_to_q4_0
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal((40, 32)), rng.uniform(0, 1, (23, 32)), np.zeros((1, 32))]).astype(np.float32)
    assert x.shape == (64, 32)
    got = kl.quantize_weights_device("q4_0", torch.from_numpy(x).to(G.dev()))
    torch.cuda.synchronize()
    want = quantize_to_q4_0(torch.from_numpy(x))
    assert got.numel() == 64 * 18 and torch.equal(got.cpu(), want)
    assert want.view(64, 18)[63].tolist() == [0, -128] + [-120] * 16  # (the all-zero block: d = -0, every code 8)


# ---- 3. dequant + hipBLASLt ----
@pytest.mark.parametrize("M,N,K", Q.BLAS_SHAPES)
def test_blas_path(M, N, K, tune):
    G.check_blas_path(T, M, N, K, tune)


# ---- 4. routes ----
def test_routes(tune):
    assert "stream_decode_kernel" in kl.route_name(Q40, 4096, 1, 4096)
    assert "stream_decode_kernel" in kl.route_name(Q40, 4096, 1, 4096, prepared=True)
    assert "stream_decode_kernel" in kl.route_name(Q40, 4096, 4, 4096)
    assert kl.route_name(Q40, 4096, 4, 11008) == "gemv_kernel"
    assert kl.route_name(Q40, 4096, 16, 4096 + 32) == "gemv_kernel"
    for M, N in ((4096, 5), (4096, 16), (4096, 128), (11008, 16), (11008, 128), (4096, 767)):
        for prepared in (False, True):
            assert "sgemm" in kl.route_name(Q40, M, N, 4096, prepared=prepared), (M, N, prepared)
    assert "hipBLASLt" in kl.route_name(Q40, 4096, 768, 4096)
    assert kl.route_name(Q40, 4096, 16, 4096, act="fp8") == "none"
    assert kl.route_name(Q40, 4096, 16, 4000) == "gemv_kernel"  # (125 blocks: a valid K)
    assert kl.route_name(Q40, 4096, 16, 4016) == "none"


@pytest.mark.parametrize("knob", ["GQ_RGEMM", "GQ_SKINNY", "GQ_KSTREAM", "GQ_GEMM_SPLITS", "GQ_SGEMM"])
def test_forced_routes_keep_sgemm(knob, tune):
    """Q4_0 has no resident, K-chunked, skinny or LDS-DMA GEMM form: a knob that forces one (or
    turns the streaming GEMM off for the other types) leaves it on the streaming GEMM."""
    G.check_forced_routes_keep_sgemm(T, knob, tune)


def test_row_chunks_under_the_launch_limit(tune):
    """A call over the per-launch byte limit (lowered here) is cut into row chunks, each on the
    streaming GEMM: the bits of the one-launch call (rows are independent; splits pinned).
    512 rows of 288 bytes per launch (512 + 88); the limit holds one whole 128-token tile of x~, so
    the 24 tokens go into every launch."""
    G.check_row_chunks_under_the_launch_limit(T, tune, 147600)  # (512 rows of 288 bytes = 147456 per launch)


# ---- 5. invariants ----
@pytest.mark.parametrize("N,K", [(2, 736), (24, 768), (24, 736)])
def test_activation_scaling_is_exact(N, K):
    G.check_activation_scaling_is_exact(T, N, K)


@pytest.mark.parametrize("N,K", [(3, 736), (24, 768), (24, 736)])
def test_row_independence(N, K, tune):
    G.check_row_independence(T, N, tune, K)


# ---- 6. prepared form ----
@pytest.mark.parametrize("N,K", [(2, 1024), (3, 160), (24, 1024)])
def test_prepared(N, K):
    G.check_prepared(T, N, K)


# ---- 7. grouped decode ----
_GROUP = (("q4_0", 96, 512), ("q4_0", 64, 160), ("q4_k", 96, 512), ("q6_k", 64, 768), ("q8_0", 64, 160))


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_grouped_decode_bit_identical(N):
    G.check_grouped_decode_bit_identical(_GROUP, N)


@pytest.mark.parametrize("other", ["q2_k", "q3_k", "q5_k"])
def test_grouped_with_another_q8_1_only_type_is_refused(other):
    """No grouped decode kernel carries Q4_0's cases beside Q5_K's, Q3_K's or Q2_K's: nothing is
    launched and the caller runs the items alone."""
    assert kl.mmq_grouped(G.grouped_items((("q4_0", 96, 512), (other, 64, 768)), 2), 2) is None


def test_grouped_one_token_cached_chunk_cap():
    """The grouped kernel that holds a Q4_0 item carries every format to five cached chunks at one
    token (K <= 20480; with more cases it spills): a launch at the cap gives the solo bits, one
    beyond it is refused and nothing is launched."""
    N = 1
    for K, ok in ((20480, True), (24576, False)):
        group = (("q4_0", 8, K), ("q8_0", 8, 512))
        raws = [random_blocks(f, M, k, seed=40 + i) for i, (f, M, k) in enumerate(group)]
        Bs = [random_activations(N, k, seed=k) for _, _, k in group]
        items = [(kl.TYPES[f], G.to_w(r), G.to_x(B), M, k, None) for (f, M, k), r, B in zip(group, raws, Bs)]
        assert "stream_decode_kernel" in kl.route_name(Q40, 8, N, K)
        outs = kl.mmq_grouped(items, N)
        if not ok:
            assert outs is None
            continue
        assert outs is not None, kl.lib().gq_last_error()
        torch.cuda.synchronize()
        for (f, M, k), r, B, it, C in zip(group, raws, Bs, items, outs):
            solo = kl.mmq(it[0], it[1], it[2], M, N, k)
            torch.cuda.synchronize()
            assert torch.equal(C.view(torch.int16), solo.view(torch.int16)), (f, M, k)
            assert Q.rel_err(C.cpu().numpy(), TM.judge(f, r, B, M, N, k)) <= Q.TIGHT_GEMV, (f, M, k)


def test_grouped_at_gemm_tokens_is_refused():
    G.check_grouped_at_gemm_tokens_is_refused(_GROUP)
    assert b"Q4_0" in kl.lib().gq_last_error()


# ---- 8. grouped prepared (the streaming GEMM) ----
@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("splits", [1, 2])
def test_grouped_prepared_bit_identical(N, splits, tune):
    group = (("q4_0", 300, 512), ("q6_k", 64, 768), ("q8_0", 64, 768), ("q4_0", 96, 512), ("q4_k", 64, 512))
    G.check_grouped_prepared_bit_identical(T, group, N, splits, tune)


# ---- 9. MoE ----
def test_mmq_id_bit_identical_to_one_token_calls():
    """gq_mmq_id on Q4_0 experts at K = 160 (K % 64 == 32: rows end with half a unit): every pair
    the bits of its own one-token gq_mmq; an id out of range gives zeros."""
    G.check_mmq_id_bit_identical_to_one_token_calls(T, K=160)


@pytest.mark.parametrize("M", [70, 300])
def test_mmq_id_sorted_80_pairs(M):
    """gq_mmq_id_sorted at 80 pairs: every pair's row the bits of the one-split streaming GEMM on
    its expert's gathered rows, and within the gate of the oracle."""
    G.check_mmq_id_sorted_80_pairs(T, M)


# ---- 10. from written GGUF files ----
@pytest.mark.parametrize("N", [1, 3, 8, 40])
def test_moe_ffn_from_gguf(tmp_path, N):
    """MoEFFN.from_gguf on a written 3-D Q4_0 file (E=4, S=2, hidden 512, ffn 256) at 2, 6 and 16
    pairs (gq_mmq_id) and 80 (the sorted GEMM), stage by stage against the oracle: the gate and up
    rows on x, the down rows on the fp16 silu(g) * u the block feeds them, each at the gate of its
    pair count; the block's output the bits of the same torch ops on those stage outputs."""
    G.check_moe_ffn_from_gguf(tmp_path, N, ("q4_0", "q4_0", "q4_0"))


@pytest.mark.parametrize("fuse", [True, False])
def test_layer_mix_from_gguf(tmp_path, fuse):
    from gguf import q4_0_layer_types
    G.check_layer_mix_from_gguf(T, tmp_path, fuse, q4_0_layer_types(0, 32), {"q4_0"})
