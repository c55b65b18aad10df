"""Q3_K on the host (no GPU): the format pinned against the reference's Q6_K oracle through the
lossless transcode of tests/q3k_model.py, a hand-written block, the block producer, the CPU MMQ,
GGUF I/O, the C ABI's host-side checks, and a numpy model of the GPU paths' roundings held to the
GPU tests' gates on the GPU tests' own inputs."""
import ctypes

import numpy as np
import pytest
import torch

import oracle as O
import q3k_model as Q
from utils.synth import random_activations, random_blocks

Q3 = 4


def _i8(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int8))


def _cpu_mmq(gtype, raw, qB, M, N, K, threads=0):
    from kernels.cpu_impls._cpu import cpu_mmq
    return cpu_mmq(gtype, _i8(raw), qB, M, N, K, threads)


# ---- 1. the format, pinned against the oracle ----
def test_dequantize_equals_oracle_q6_k_on_transcoded_blocks():
    from utils.quantize._qlib import dequantize
    M, K = 24, 768
    raw = random_blocks("q3_k", M, K, seed=3)
    got = dequantize("q3_k", _i8(raw)).numpy()
    want = O.dequant("q6_k", Q.to_q6_k(raw))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), Q.dequant_f32(raw, M, K).reshape(-1).view(np.uint32))
    from utils.quantize.q3_k import dequantize_q3_k
    h = dequantize_q3_k(_i8(raw), (M, K))
    assert h.dtype == torch.float16 and np.array_equal(h.numpy().reshape(-1), got.astype(np.float16))


def test_cpu_mmq_equals_oracle_q6_k_on_transcoded_blocks():
    from kernels.cpu_impls.mmq_q3_k_q8_1_cpu import mmq_q3_k_q8_1_cpu
    M, N, K = 37, 5, 1024
    raw = random_blocks("q3_k", M, K, seed=5)
    B = random_activations(N, K, seed=6)
    qB = _i8(O.quantize_q8_1(B))
    got = mmq_q3_k_q8_1_cpu(_i8(raw), qB, M, N, K)
    assert got.shape == (N, M) and got.dtype == torch.float16
    q6 = Q.to_q6_k(raw)
    want = O.mmq("q6_k", q6, O.quantize_q8_1(B), M, N, K, O.EXACT)
    assert np.array_equal(got.numpy().view(np.uint16), want.view(np.uint16))
    assert torch.equal(got, _cpu_mmq(2, q6, qB, M, N, K))
    for th in (1, 3):
        assert torch.equal(mmq_q3_k_q8_1_cpu(_i8(raw), qB, M, N, K, threads=th), got)


def test_model_ideal_agrees_with_oracle_ideal():
    """The oracle's IDEAL is an fp64 sum rounded once to fp16: the model's fp64 ideal lies within
    half an fp16 ulp of it (plus fp64 rounding of the two summation orders)."""
    M, N, K = 37, 5, 1024
    raw = random_blocks("q3_k", M, K, seed=5)
    B = random_activations(N, K, seed=6)
    want = O.mmq_from_fp16("q6_k", Q.to_q6_k(raw), B, M, N, K, O.IDEAL)
    mine = Q.ideal(raw, B, M, N, K)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    assert np.all(np.abs(mine - want.astype(np.float64)) <= 0.5 * ulp + 1e-12 * np.abs(mine))
    # and, rounded the same way, the same bits but where the fp64 value sits on a rounding tie
    assert np.mean(mine.astype(np.float16).view(np.uint16) == want.view(np.uint16)) > 0.99


# ---- 2. a hand-written block: the index formulas, independent of to_q6_k and of unpack ----
_SC = [-32, 31, -1, 0, 1, 5, -17, 16, 15, -16, 7, -8, 30, -31, 2, -2]  # sub-blocks 0..15, all distinct
_CYC = [-4, -3, -2, -1, 0, 1, 2, 3]


def _hand_block():
    """d = 0.5; sub-block s has scale _SC[s]; element e of bit plane p = 4*(e/128) + (e%128)/32 has
    code _CYC[(e%32 + p) % 8]: every plane's low bits and high bit differ from every other's."""
    q = [_CYC[(e % 32 + 4 * (e // 128) + (e % 128) // 32) % 8] for e in range(256)]
    b = np.zeros(110, np.uint8)
    for e in range(256):
        h, j, l, c = e // 128, (e % 128) // 32, e % 32, q[e] + 4
        b[32 + 32 * h + l] |= (c & 3) << (2 * j)
        b[l] |= (c >> 2) << (4 * h + j)
    for s in range(16):
        v = _SC[s] + 32
        if s < 8:
            b[96 + s] |= v & 15
        else:
            b[96 + s - 8] |= (v & 15) << 4
        b[96 + 8 + s % 4] |= (v >> 4) << (2 * (s // 4))
    b[108:110] = np.array([0.5], np.float16).view(np.uint8)
    return b, np.array([0.5 * _SC[e // 16] * q[e] for e in range(256)], np.float64)


def test_hand_written_block():
    from utils.quantize._qlib import dequantize
    b, want = _hand_block()
    assert sorted(set(_SC)) == sorted(_SC) and min(_SC) == -32 and max(_SC) == 31
    # a few weights by hand: (element, 0.5 * scale * code)
    for e, w in ((0, 64.0), (31, 46.5), (32, 1.5), (127, -16.0), (128, 0.0), (200, 30.0), (255, -2.0)):
        assert want[e] == w, (e, want[e])
    assert np.array_equal(Q.dequant_exact(b, 1, 256).reshape(-1), want)
    assert np.array_equal(dequantize("q3_k", _i8(b)).numpy().astype(np.float64), want)
    d, sc, q = Q.unpack(b, 1, 256)
    assert sc.reshape(-1).tolist() == _SC


# ---- 3. host quantizer ----
def _roundtrip(x):
    from utils.quantize._qlib import dequantize, quantize
    return dequantize("q3_k", quantize("q3_k", torch.from_numpy(x))).numpy().reshape(x.shape)


def test_quantizer_size_determinism_and_zeros():
    from utils.quantize.q3_k import dequantize_q3_k, quantize_to_q3_k
    rng = np.random.default_rng(0)
    x = rng.standard_normal((6, 512)).astype(np.float32)
    q = quantize_to_q3_k(torch.from_numpy(x))
    assert q.dtype == torch.int8 and q.numel() == 6 * 2 * 110
    assert torch.equal(q, quantize_to_q3_k(torch.from_numpy(x.copy())))
    assert dequantize_q3_k(q, (6, 512)).shape == (6, 512)
    with pytest.raises(ValueError):
        quantize_to_q3_k(torch.zeros(100))
    z = _roundtrip(np.zeros(512, np.float32))
    assert np.array_equal(z, np.zeros(512, np.float32))


def test_quantizer_uses_the_high_bit_and_negative_scales():
    from utils.quantize._qlib import quantize
    rng = np.random.default_rng(2)
    raw = quantize("q3_k", torch.from_numpy(rng.standard_normal(256 * 8).astype(np.float32))).numpy().view(np.uint8)
    _, sc, q = Q.unpack(raw, 1, 2048)
    assert q.min() == -4 and q.max() == 3
    assert (q >= 0).any() and (q < 0).any()  # hmask bit set and clear
    assert sc.min() < 0 < sc.max()


@pytest.mark.parametrize("dist", ("normal", "uniform"))
def test_quantizer_no_worse_than_the_naive_one(dist):
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((64, 256)) if dist == "normal" else rng.uniform(0, 1, (64, 256))).astype(np.float32)
    rms = lambda y: float(np.sqrt(np.mean((y - x) ** 2)))  # noqa: E731
    mine = rms(_roundtrip(x))
    naive = rms(Q.dequant_f32(Q.naive_quantize(x), 64, 256))
    print(f"round-trip RMSE {dist}: gq_quantize_q3_k {mine:.5f}  naive {naive:.5f}")
    assert mine <= naive, (dist, mine, naive)


# ---- 4. the GPU paths' roundings, modelled: within the GPU tests' gates on their inputs ----
@pytest.mark.parametrize("M,N,K", Q.ALL_SHAPES)
def test_rounding_models_within_gates(M, N, K):
    raw, B, want = Q.case(M, N, K)
    tol = Q.tight(N)
    e_mfma = Q.rel_err(Q.model_mfma(raw, B, M, N, K), want)
    e_dec = Q.rel_err(Q.model_decode(raw, B, M, N, K), want)
    print(f"{M}x{N}x{K}: MFMA model {e_mfma:.2e}  decode model {e_dec:.2e}")
    assert e_mfma <= tol and e_dec <= tol, (e_mfma, e_dec)


# ---- 5. GGUF I/O, the layer-type map, the Python tables ----
def test_gguf_type_11_roundtrip(tmp_path):
    from gguf import GGML_TYPES, read_gguf, write_gguf
    assert GGML_TYPES[11] == ("q3_k", 256, 110)
    raw = random_blocks("q3_k", 12, 512, seed=1)
    exps = random_blocks("q3_k", 3 * 10, 256, seed=2)
    p = tmp_path / "t.gguf"
    write_gguf(p, {"blk.0.attn_q.weight": ("q3_k", (12, 512), raw),
                   "blk.0.ffn_gate_exps.weight": ("q3_k", (3, 10, 256), exps)})
    _, tens = read_gguf(p)
    t = tens["blk.0.attn_q.weight"]
    assert t.type_name == "q3_k" and t.shape == (12, 512)
    assert np.array_equal(np.asarray(t.data).reshape(-1), raw)
    e = tens["blk.0.ffn_gate_exps.weight"]
    assert e.type_name == "q3_k" and e.shape == (3, 10, 256)
    assert np.array_equal(np.asarray(e.data).reshape(-1), exps)


def test_q3_k_m_layer_types():
    from gguf import LLAMA_LAYER_SHAPES, q3_k_m_layer_types
    rest = {n: "q3_k" for n in LLAMA_LAYER_SHAPES if n not in ("attn_v", "attn_output", "ffn_down")}
    for layer, v, down in ((0, "q5_k", "q5_k"), (1, "q5_k", "q5_k"), (2, "q4_k", "q4_k"), (31, "q4_k", "q4_k")):
        t = q3_k_m_layer_types(layer, 32)
        assert t == dict(rest, attn_v=v, attn_output="q4_k", ffn_down=down), (layer, t)
    assert q3_k_m_layer_types(2, 48)["ffn_down"] == "q5_k"  # (layer < 48 // 16)
    assert "memory" in q3_k_m_layer_types.__doc__


def test_python_tables():
    import kernels._lib as kl
    from kernels.cpu_impls._cpu import _BYTES, _QK
    from utils.quantize._qlib import BLOCK as QB
    from utils.synth import BLOCK as YB
    assert kl.TYPES["q3_k"] == kl.GQ_Q3_K == 4
    assert kl.BLOCK_ELEMS[4] == 256 and kl.BLOCK_BYTES[4] == 110
    assert QB["q3_k"] == YB["q3_k"] == (256, 110)
    assert _BYTES[4] == 110 and _QK[4] == 256
    raw = random_blocks("q3_k", 2, 512, seed=1).reshape(4, 110)
    d = raw[:, 108:110].copy().view(np.float16).astype(np.float32)
    assert np.all((d >= 0.5 * 2.0 ** -7) & (d <= 1.5 * 2.0 ** -7))
    _, sc, _ = Q.unpack(random_blocks("q3_k", 8, 1024, seed=1), 8, 1024)
    assert sc.min() == -32 and sc.max() == 31  # (the random 6-bit scales stay, negative ones included)


# ---- 6. ABI host checks (every call returns before any launch) ----
def test_abi_host_checks():
    import kernels._lib as kl
    L = kl.lib()
    p = ctypes.c_void_p(16)
    assert L.gq_block_elems(4) == 256 and L.gq_block_bytes(4) == 110
    assert L.gq_version() == 105
    assert L.gq_mmq(4, p, p, p, 4, 4, 100, 100, 4, p, 1 << 20, None) == 1
    assert b"multiple of 256" in L.gq_last_error()
    assert L.gq_mmq_ex(4, 1, p, p, p, 8, 4, 256, 256, 8, p, 1 << 20, None) == 3
    assert b"Q3_K" in L.gq_last_error()
    assert L.gq_mmq_prepared_ex(4, 1, p, p, 1 << 20, p, 8, 4, 256, 8, None) == 3
    assert L.gq_quantize_weights(4, p, p, 256, None) == 3
    assert L.gq_mmq(7, p, p, p, 4, 4, 256, 256, 4, p, 1 << 20, None) == 3
    assert b"unknown" in L.gq_last_error()
    assert L.gq_block_bytes(7) == 210  # (an unknown type's answer, as before)
    assert L.gq_mmq(4, None, None, None, 0, 4, 256, 256, 4, None, 0, None) == 0
    # null pointer and short workspace at a GEMM token count: refused before the launch
    assert L.gq_mmq(4, None, p, p, 4, 64, 256, 256, 4, p, 1 << 20, None) == 1
    need = L.gq_mmq_call_workspace_size(4, 0, 4, 64, 256)
    assert 0 < need <= L.gq_mmq_workspace_size(4, 4, 64, 256)
    assert L.gq_mmq(4, p, p, p, 4, 64, 256, 256, 4, p, need - 1, None) == 1
    assert L.gq_mmq_call_workspace_size(4, 0, 4, 4, 256) == 0  # a one-launch decode
    # Q3_K's activation part is every type's (it depends on the activation format, N and K only)
    for N, K in ((1, 4096), (4, 4096), (4, 11008), (16, 4096)):
        assert kl.workspace_size(4, 0, N, K) == kl.workspace_size(1, 0, N, K)
    # a grouped launch at 5..32 tokens with a Q3_K item: unsupported (the caller runs per item)
    item = (kl.GroupItem * 1)(kl.GroupItem(4, 16, 16, 256, 16, 16, 16, 256))
    assert L.gq_mmq_grouped(item, 1, 8, None) == 3


# gq_mmq_workspace_size(type, M, N, K) of the four earlier types, recorded from a build of the
# parent commit (e0e067f, on a machine without a GPU: 256 compute units assumed, as on an MI355X)
_PARENT_WS = {
    (0, 4096, 1, 4096): 13312, (0, 4096, 4, 11008): 143360, (0, 4096, 16, 4096): 2320640,
    (0, 11008, 16, 4096): 5876992, (0, 4096, 128, 11008): 21367040, (0, 300, 24, 512): 105728,
    (0, 32000, 64, 4096): 9054720, (0, 4096, 1024, 4096): 80740352,
    (1, 4096, 1, 4096): 13312, (1, 4096, 4, 11008): 143360, (1, 4096, 16, 4096): 2320640,
    (1, 11008, 16, 4096): 5876992, (1, 4096, 128, 11008): 21367040, (1, 300, 24, 512): 105728,
    (1, 32000, 64, 4096): 66468608, (1, 4096, 1024, 4096): 80740352,
    (2, 4096, 1, 4096): 13312, (2, 4096, 4, 11008): 143360, (2, 4096, 16, 4096): 2320640,
    (2, 11008, 16, 4096): 5876992, (2, 4096, 128, 11008): 21367040, (2, 300, 24, 512): 105728,
    (2, 32000, 64, 4096): 9054720, (2, 4096, 1024, 4096): 80740352,
    (3, 4096, 1, 4096): 13312, (3, 4096, 4, 11008): 143360, (3, 4096, 16, 4096): 2320640,
    (3, 11008, 16, 4096): 1983232, (3, 4096, 128, 11008): 21367040, (3, 300, 24, 512): 105728,
    (3, 32000, 64, 4096): 9054720, (3, 4096, 1024, 4096): 80740352,
}


def test_workspace_of_other_types_unchanged():
    import kernels._lib as kl
    assert len(_PARENT_WS) == 4 * 8
    for (t, M, N, K), want in _PARENT_WS.items():
        assert kl.workspace_size(t, M, N, K) == want, (t, M, N, K)
