"""Q5_K on the host (no GPU): the block producers, the CPU MMQ, GGUF I/O, the C ABI's host-side
checks, and a numpy model of the GPU paths' roundings held to the GPU tests' tolerances on the
GPU tests' own inputs.  The format and the models are in tests/q5k_model.py (the reference has no
Q5_K, so the oracle does not know it)."""
import ctypes

import numpy as np
import pytest
import torch

import q5k_model as Q
from utils.synth import random_activations, random_blocks


def _i8(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int8))


# ---- 1. host dequantize ----
def test_dequantize_bit_equal_to_formula():
    from utils.quantize._qlib import dequantize
    M, K = 24, 768
    raw = random_blocks("q5_k", M, K, seed=3)
    got = dequantize("q5_k", _i8(raw)).numpy().reshape(M, K)
    assert np.array_equal(got.view(np.uint32), Q.dequant_f32(raw, M, K).view(np.uint32))
    from utils.quantize.q5_k import dequantize_q5_k
    h = dequantize_q5_k(_i8(raw), (M, K))
    assert h.dtype == torch.float16 and np.array_equal(h.numpy(), got.astype(np.float16))


def _q5_from_q4(raw4, nblk, qh=0):
    """Q5_K blocks with a Q4_K block's header and qs, and every qh byte = qh."""
    b4 = raw4.reshape(nblk, 144)
    b5 = np.empty((nblk, 176), np.uint8)
    b5[:, :16] = b4[:, :16]
    b5[:, 16:48] = qh
    b5[:, 48:] = b4[:, 16:]
    return b5.reshape(-1)


def test_dequantize_qh_zero_equals_q4_k():
    from utils.quantize._qlib import dequantize
    raw4 = random_blocks("q4_k", 8, 1024, seed=11)
    raw5 = _q5_from_q4(raw4, 32)
    a, b = dequantize("q5_k", _i8(raw5)).numpy(), dequantize("q4_k", _i8(raw4)).numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 2. host quantizer ----
def _roundtrip(fmt, x):
    from utils.quantize._qlib import dequantize, quantize
    return dequantize(fmt, quantize(fmt, torch.from_numpy(x))).numpy().reshape(x.shape)


def test_quantizer_size_determinism_zero_and_constant():
    from utils.quantize.q5_k import dequantize_q5_k, quantize_to_q5_k
    rng = np.random.default_rng(0)
    x = rng.standard_normal((6, 512)).astype(np.float32)
    q = quantize_to_q5_k(torch.from_numpy(x))
    assert q.dtype == torch.int8 and q.numel() == 6 * 2 * 176
    assert torch.equal(q, quantize_to_q5_k(torch.from_numpy(x.copy())))
    assert dequantize_q5_k(q, (6, 512)).shape == (6, 512)
    with pytest.raises(ValueError):
        quantize_to_q5_k(torch.zeros(100))
    z = _roundtrip("q5_k", np.zeros(256, np.float32))
    assert np.array_equal(z, np.zeros(256, np.float32))
    for c in (0.37, -1.25, 3.0):
        r = _roundtrip("q5_k", np.full(256, c, np.float32))
        # a constant block is one level (or the min alone) times a 6-bit scale times an fp16 d (or
        # dmin): the header's fp16 rounding is the only error, one fp16 ulp of |c| at most
        assert np.max(np.abs(r - c)) <= abs(c) * 2.0 ** -10, (c, np.max(np.abs(r - c)))


@pytest.mark.parametrize("dist", ("normal", "uniform"))
def test_quantizer_beats_q4_k(dist):
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((64, 256)) if dist == "normal" else rng.uniform(0, 1, (64, 256))).astype(np.float32)
    rms = lambda fmt: float(np.sqrt(np.mean((_roundtrip(fmt, x) - x) ** 2)))  # noqa: E731
    e5, e4 = rms("q5_k"), rms("q4_k")
    print(f"round-trip RMS {dist}: q5_k {e5:.5f}  q4_k {e4:.5f}")
    assert e5 < e4, (dist, e5, e4)


def test_quantizer_codes_use_the_fifth_bit():
    from utils.quantize._qlib import quantize
    rng = np.random.default_rng(2)
    raw = quantize("q5_k", torch.from_numpy(rng.standard_normal(256 * 8).astype(np.float32))).numpy().view(np.uint8)
    _, _, _, _, q = Q.unpack(raw, 1, 2048)
    assert q.min() == 0 and q.max() == 31


# ---- 3. CPU MMQ ----
def test_cpu_mmq_gate_threads_and_q4_k_identity():
    import oracle as O
    from kernels.cpu_impls.mmq_q4_k_q8_1_cpu import mmq_q4_k_q8_1_cpu
    from kernels.cpu_impls.mmq_q5_k_q8_1_cpu import mmq_q5_k_q8_1_cpu
    M, N, K = 37, 5, 1024
    raw = random_blocks("q5_k", M, K, seed=5)
    B = random_activations(N, K, seed=6)
    qB = _i8(O.quantize_q8_1(B))
    got = mmq_q5_k_q8_1_cpu(_i8(raw), qB, M, N, K)
    assert got.shape == (N, M) and got.dtype == torch.float16
    want = Q.ideal(raw, B, M, N, K)
    assert O.allclose(got.numpy(), want, 0.01)  # the reference's 1% gate, atol = 1% of max|C|
    for th in (1, 3):
        assert torch.equal(mmq_q5_k_q8_1_cpu(_i8(raw), qB, M, N, K, threads=th), got)
    raw4 = random_blocks("q4_k", M, K, seed=9)
    a = mmq_q5_k_q8_1_cpu(_i8(_q5_from_q4(raw4, M * K // 256)), qB, M, N, K)
    assert torch.equal(a, mmq_q4_k_q8_1_cpu(_i8(raw4), qB, M, N, K))


# ---- 4. GGUF I/O and the layer-type map ----
def test_gguf_type_13_roundtrip(tmp_path):
    from gguf import GGML_TYPES, read_gguf, write_gguf
    assert GGML_TYPES[13] == ("q5_k", 256, 176)
    raw = random_blocks("q5_k", 12, 512, seed=1)
    p = tmp_path / "t.gguf"
    write_gguf(p, {"blk.0.attn_q.weight": ("q5_k", (12, 512), raw)})
    _, tens = read_gguf(p)
    t = tens["blk.0.attn_q.weight"]
    assert t.type_name == "q5_k" and t.shape == (12, 512)
    assert np.array_equal(np.asarray(t.data).reshape(-1), raw)


def test_q5_k_m_layer_types():
    from gguf import q4_k_m_layer_types, q5_k_m_layer_types
    from gguf.mix import _more_bits
    t0 = q5_k_m_layer_types(0, 32)
    assert {n for n, t in t0.items() if t == "q6_k"} == {"attn_v", "ffn_down"}
    assert all(t == "q5_k" for n, t in t0.items() if n not in ("attn_v", "ffn_down"))
    for layer in (10, 11, 12, 13):
        t = q5_k_m_layer_types(layer, 32)
        assert t["attn_v"] == t["ffn_down"] == ("q6_k" if _more_bits(layer, 32) else "q5_k")
        assert {k: v.replace("q4_k", "q5_k") for k, v in q4_k_m_layer_types(layer, 32).items()} == t


def test_python_tables():
    import kernels._lib as kl
    from utils.quantize._qlib import BLOCK as QB
    from utils.synth import BLOCK as YB
    assert kl.TYPES["q5_k"] == kl.GQ_Q5_K == 3
    assert kl.BLOCK_ELEMS[3] == 256 and kl.BLOCK_BYTES[3] == 176
    assert QB["q5_k"] == YB["q5_k"] == (256, 176)


# ---- 5. ABI host checks (every call returns before any launch) ----
def test_abi_host_checks():
    import kernels._lib as kl
    L = kl.lib()
    p = ctypes.c_void_p(16)
    assert L.gq_block_elems(3) == 256 and L.gq_block_bytes(3) == 176
    assert L.gq_version() == 105
    assert L.gq_mmq(3, p, p, p, 4, 4, 100, 100, 4, p, 1 << 20, None) == 1
    assert b"multiple of 256" in L.gq_last_error()
    assert L.gq_mmq_ex(3, 1, p, p, p, 8, 4, 256, 256, 8, p, 1 << 20, None) == 3
    assert L.gq_mmq_prepared_ex(3, 1, p, p, 1 << 20, p, 8, 4, 256, 8, None) == 3
    assert L.gq_quantize_weights(3, p, p, 256, None) == 3
    assert L.gq_mmq(7, p, p, p, 4, 4, 256, 256, 4, p, 1 << 20, None) == 3
    assert b"unknown" in L.gq_last_error()
    assert L.gq_mmq(3, None, None, None, 0, 4, 256, 256, 4, None, 0, None) == 0
    # null pointer and short workspace at a GEMM token count: refused before the launch
    assert L.gq_mmq(3, None, p, p, 4, 64, 256, 256, 4, p, 1 << 20, None) == 1
    need = L.gq_mmq_call_workspace_size(3, 0, 4, 64, 256)
    assert 0 < need <= L.gq_mmq_workspace_size(3, 4, 64, 256)
    assert L.gq_mmq(3, p, p, p, 4, 64, 256, 256, 4, p, need - 1, None) == 1
    assert L.gq_mmq_call_workspace_size(3, 0, 4, 4, 256) == 0  # a one-launch decode
    # a grouped launch at 5..32 tokens with a Q5_K item: unsupported (the caller runs per item)
    item = (kl.GroupItem * 1)(kl.GroupItem(3, 16, 16, 256, 16, 16, 16, 256))
    assert L.gq_mmq_grouped(item, 1, 8, None) == 3


def test_workspace_of_other_types_unchanged_by_q5_k():
    """Q5_K's activation part is every type's (it depends on the activation format, N and K only)."""
    import kernels._lib as kl
    for N, K in ((1, 4096), (4, 4096), (4, 11008), (16, 4096)):
        assert kl.workspace_size(3, 0, N, K) == kl.workspace_size(1, 0, N, K)


# ---- the GPU paths' roundings, modelled: within the GPU tests' tolerances on their inputs ----
@pytest.mark.parametrize("M,N,K", Q.ALL_SHAPES)
def test_rounding_models_within_tolerance(M, N, K):
    raw, B, want = Q.case(M, N, K)
    tol = Q.tight(N)
    e_out = Q.rel_err(want.astype(np.float16), want)  # the fp16 output rounding alone
    e_mfma = Q.rel_err(Q.model_mfma(raw, B, M, N, K), want)
    print(f"{M}x{N}x{K}: fp16 output {e_out:.2e}  MFMA model {e_mfma:.2e}")
    assert e_out <= tol and e_mfma <= tol, (e_out, e_mfma)
    if N <= 4:
        e_dec = Q.rel_err(Q.model_decode(raw, B, M, N, K), want)
        print(f"{M}x{N}x{K}: decode model {e_dec:.2e}")
        assert e_dec <= tol, e_dec
