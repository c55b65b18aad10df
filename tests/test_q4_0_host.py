"""Q4_0 on the host (no GPU): the format pinned bit for bit against the reference's Q8_0 oracle
through the exact widening of tests/q4_0_model.py (a Q4_0 block is a Q8_0 block with the same d and
the codes nibble - 8), a hand-written block, the CPU MMQ, the block producer, GGUF I/O, the Python
tables, the C ABI's host-side checks, the routes against Q3_K's recorded ones, and numpy models of
the GPU paths' roundings held to the GPU tests' gates on the GPU tests' own inputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle as O
import q4_0_model as Q
from utils.synth import random_activations, random_blocks

Q40, Q3 = 6, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _i8(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int8))


# ---- 1. the format, pinned against the oracle ----
def test_dequantize_equals_oracle_q8_0_on_the_widened_blocks():
    from utils.quantize._qlib import dequantize
    M, K = 24, 1120
    raw = random_blocks("q4_0", M, K, seed=3)
    got = dequantize("q4_0", _i8(raw)).numpy()
    want = O.dequant("q8_0", Q.widen(raw))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), Q.dequant_f32(raw, M, K).reshape(-1).view(np.uint32))
    from utils.quantize.q4_0 import dequantize_q4_0
    h = dequantize_q4_0(_i8(raw), (M, K))
    assert h.dtype == torch.float16 and np.array_equal(h.numpy().reshape(-1), got.astype(np.float16))
    # the synthetic nibbles reach both ends of the code range
    assert Q.codes(raw).min() == -8 and Q.codes(raw).max() == 7


# ---- 2. a hand-written block: both nibble planes, codes 0 and 15 ----
def _hand_block():
    """d = 0.5; element e < 16 has code (3*e) % 16, element e >= 16 has code (15 - 5*(e - 16)) % 16:
    the two planes differ, and both 0 and 15 occur."""
    q = [(3 * e) % 16 if e < 16 else (15 - 5 * (e - 16)) % 16 for e in range(32)]
    b = np.zeros(18, np.uint8)
    b[0:2] = np.array([0.5], np.float16).view(np.uint8)
    for j in range(16):
        b[2 + j] = q[j] | (q[16 + j] << 4)
    return b, q, np.array([0.5 * (c - 8) for c in q], np.float64)


def test_hand_written_block():
    from utils.quantize._qlib import dequantize
    b, q, want = _hand_block()
    assert {0, 15} <= set(q) and q[:16] != q[16:]
    # a few weights by hand: (element, 0.5 * (code - 8))
    #   e = 0:  low nibble of qs[0], code 0                    -> -4.0
    #   e = 5:  low nibble of qs[5], code 15                   ->  3.5
    #   e = 7:  low nibble of qs[7], code 21 % 16 = 5          -> -1.5
    #   e = 16: high nibble of qs[0], code 15                  ->  3.5
    #   e = 19: high nibble of qs[3], code (15 - 15) % 16 = 0  -> -4.0
    #   e = 31: high nibble of qs[15], code (15 - 75) % 16 = 4 -> -2.0
    for e, w in ((0, -4.0), (5, 3.5), (7, -1.5), (16, 3.5), (19, -4.0), (31, -2.0)):
        assert want[e] == w, (e, want[e])
    assert b[2] == 0xF0 and b[2 + 3] == 0x09 and b[2 + 5] == 0x6F  # (qs[5]: 15 | ((15 - 25) % 16) << 4)
    assert np.array_equal(dequantize("q4_0", _i8(b)).numpy().astype(np.float64), want)
    assert np.array_equal(O.dequant("q8_0", Q.widen(b)).astype(np.float64), want)
    d, uq = Q.unpack(b, 1, 32)
    assert float(d[0, 0]) == 0.5 and (uq.reshape(-1) + 8).tolist() == q
    w8 = Q.widen(b)
    assert w8.size == 34 and w8[:2].tolist() == b[:2].tolist()
    assert w8[2:].view(np.int8).tolist() == [c - 8 for c in q]


# ---- 3. the CPU product ----
@pytest.mark.parametrize("M,N,K", [(37, 5, 1120), (9, 3, 32)])
def test_cpu_mmq_equals_the_oracle_bit_for_bit(M, N, K):
    from kernels.cpu_impls.mmq_q4_0_q8_1_cpu import mmq_q4_0_q8_1_cpu
    from kernels.cpu_impls.mmq_q8_0_q8_1_cpu import mmq_q8_0_q8_1_cpu
    assert K % 256 != 0
    raw = random_blocks("q4_0", M, K, seed=5)
    B = random_activations(N, K, seed=6)
    Bq = O.quantize_q8_1(B)
    got = mmq_q4_0_q8_1_cpu(_i8(raw), _i8(Bq), M, N, K)
    assert got.shape == (N, M) and got.dtype == torch.float16
    want = O.mmq("q8_0", Q.widen(raw), Bq, M, N, K, O.EXACT)
    assert np.array_equal(got.numpy().view(np.uint16), want.view(np.uint16))
    wide = mmq_q8_0_q8_1_cpu(_i8(Q.widen(raw)), _i8(Bq), M, N, K)
    assert torch.equal(got.contiguous().view(torch.int16), wide.contiguous().view(torch.int16))
    for th in (1, 3):
        assert torch.equal(mmq_q4_0_q8_1_cpu(_i8(raw), _i8(Bq), M, N, K, threads=th), got)


def test_cpu_mmq_refuses_a_bad_k():
    from kernels.cpu_impls._cpu import cpu_mmq
    with pytest.raises(RuntimeError):
        cpu_mmq(6, torch.zeros(18, dtype=torch.int8), torch.zeros(36, dtype=torch.int8), 1, 1, 48)


# ---- 4. host quantizer ----
def _quant(x):
    from utils.quantize._qlib import quantize
    return quantize("q4_0", torch.from_numpy(x)).numpy().view(np.uint8)


def test_quantizer_size_determinism_and_zeros():
    from utils.quantize.q4_0 import dequantize_q4_0, quantize_to_q4_0
    rng = np.random.default_rng(0)
    x = rng.standard_normal((6, 96)).astype(np.float32)
    q = quantize_to_q4_0(torch.from_numpy(x))
    assert q.dtype == torch.int8 and q.numel() == 6 * 3 * 18
    assert torch.equal(q, quantize_to_q4_0(torch.from_numpy(x.copy())))
    assert dequantize_q4_0(q, (6, 96)).shape == (6, 96)
    with pytest.raises(ValueError):
        quantize_to_q4_0(torch.zeros(100))
    z = _quant(np.zeros(64, np.float32))
    assert np.array_equal(Q.dequant_f32(z, 1, 64), np.zeros((1, 64), np.float32))
    assert z.reshape(2, 18)[:, :2].tolist() == [[0, 0x80], [0, 0x80]]  # d = 0 / -8 = -0
    assert np.all(z.reshape(2, 18)[:, 2:] == 0x88)  # (id = 0: every code trunc(8.5) = 8, the weight 0)


@pytest.mark.parametrize("sign", (1.0, -1.0))
def test_the_extreme_element_gets_code_zero(sign):
    """d = m / -8 with m the element of largest magnitude, sign kept: m itself is code 0 (weight
    -8 d = m up to d's fp16 rounding), whichever its sign."""
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (40, 32)).astype(np.float32)
    pos = rng.integers(0, 32, 40)
    x[np.arange(40), pos] = np.float32(sign * 1.5)
    raw = _quant(x)
    d, q = Q.unpack(raw, 40, 32)
    assert np.all(q[np.arange(40), 0, pos] == -8)
    assert np.array_equal(d[:, 0], np.full(40, np.float16(sign * 1.5 / -8), np.float32))
    assert q.max() <= 7 and q.min() == -8


def test_quantizer_equals_the_rule_restated_in_numpy():
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.standard_normal((64, 32)), rng.uniform(0, 1, (64, 32)), np.zeros((1, 32))]).astype(np.float32)
    assert np.array_equal(_quant(x), Q.new_rule_quantize(x))


@pytest.mark.parametrize("dist", ("normal", "uniform01", "uniform11"))
def test_quantizer_no_worse_than_the_naive_one(dist):
    rng = np.random.default_rng(7)
    x = {"normal": lambda: rng.standard_normal((512, 32)), "uniform01": lambda: rng.uniform(0, 1, (512, 32)),
         "uniform11": lambda: rng.uniform(-1, 1, (512, 32))}[dist]().astype(np.float32)
    rms = lambda y: float(np.sqrt(np.mean((y - x) ** 2)))  # noqa: E731
    mine = rms(Q.dequant_f32(_quant(x), 512, 32))
    naive = rms(Q.dequant_f32(Q.naive_quantize(x), 512, 32))
    print(f"round-trip RMSE {dist}: gq_quantize_q4_0 {mine:.5f}  naive {naive:.5f}")
    assert mine <= naive, (dist, mine, naive)


# ---- 5. the GPU paths' roundings, modelled: within the GPU tests' gates on their inputs ----
@pytest.mark.parametrize("M,N,K", Q.ALL_SHAPES)
def test_rounding_models_within_gates(M, N, K):
    raw, B, want = Q.case(M, N, K)
    tol = Q.tight(N)
    e_dec = Q.rel_err(Q.model_decode(raw, B, M, N, K), want)
    print(f"{M}x{N}x{K}: decode model {e_dec:.2e}", end="")
    assert e_dec <= tol, e_dec
    if K % 256 == 0:  # (the MFMA paths take whole 256-element groups only)
        e_mfma = Q.rel_err(Q.model_mfma(raw, B, M, N, K), want)
        print(f"  MFMA model {e_mfma:.2e}", end="")
        assert e_mfma <= tol, e_mfma
    print()


def test_edge_valued_weights_model():
    M, K = 70, 512
    raw = Q.edge_blocks(M, K, seed=2)
    q = Q.codes(raw).reshape(M, K // 32, 32)
    assert np.all(q[:23] == -8) and np.all(q[23:46] == 7)
    assert np.all(q[46:, 0::2] == -8) and np.all(q[46:, 1::2] == 7)
    for N in (1, 16):
        B = random_activations(N, K, seed=N)
        want = Q.ideal(raw, B, M, N, K)
        assert Q.rel_err(Q.model_decode(raw, B, M, N, K), want) <= Q.tight(N)
        assert Q.rel_err(Q.model_mfma(raw, B, M, N, K), want) <= Q.tight(N)


# ---- 6. GGUF I/O, the layer-type map, the Python tables ----
def test_gguf_type_2_roundtrip(tmp_path):
    from gguf import GGML_TYPES, read_gguf, write_gguf
    assert GGML_TYPES[2] == ("q4_0", 32, 18)
    raw = random_blocks("q4_0", 12, 160, seed=1)
    exps = random_blocks("q4_0", 3 * 10, 96, seed=2)
    p = tmp_path / "t.gguf"
    write_gguf(p, {"blk.0.attn_q.weight": ("q4_0", (12, 160), raw),
                   "blk.0.ffn_gate_exps.weight": ("q4_0", (3, 10, 96), exps)})
    _, tens = read_gguf(p)
    t = tens["blk.0.attn_q.weight"]
    assert t.type_name == "q4_0" and t.shape == (12, 160)
    assert np.array_equal(np.asarray(t.data).reshape(-1), raw)
    e = tens["blk.0.ffn_gate_exps.weight"]
    assert e.type_name == "q4_0" and e.shape == (3, 10, 96)
    assert np.array_equal(np.asarray(e.data).reshape(-1), exps)


def test_q4_0_layer_types():
    from gguf import LLAMA_LAYER_SHAPES, q4_0_layer_types
    for layer in (0, 5, 31):
        assert q4_0_layer_types(layer, 32) == {n: "q4_0" for n in LLAMA_LAYER_SHAPES}
    assert len(q4_0_layer_types(0)) == 7
    assert "memory" in q4_0_layer_types.__doc__


def test_python_tables():
    import kernels._lib as kl
    from gguf.blocks import BLOCK
    from kernels.cpu_impls._cpu import _BYTES, _QK
    from utils.quantize._qlib import BLOCK as QB
    from utils.synth import BLOCK as YB
    assert kl.TYPES["q4_0"] == kl.GQ_Q4_0 == 6
    assert kl.BLOCK_ELEMS[6] == 32 and kl.BLOCK_BYTES[6] == 18
    assert BLOCK["q4_0"] == QB["q4_0"] == YB["q4_0"] == (32, 18)
    assert _BYTES[6] == 18 and _QK[6] == 32
    raw = random_blocks("q4_0", 2, 512, seed=1).reshape(32, 18)
    d = raw[:, 0:2].copy().view(np.float16).astype(np.float32)
    assert np.all((d >= 0.5 * 2.0 ** -7) & (d <= 1.5 * 2.0 ** -7))
    q = Q.codes(random_blocks("q4_0", 8, 1024, seed=1))
    assert sorted(np.unique(q).tolist()) == list(range(-8, 8))
    from kernels.mmq_q4_0 import mmq_q4_0  # noqa: F401
    from utils.quantize.q4_0 import quantize_to_q4_0  # noqa: F401


# ---- 7. ABI host checks (every call returns before any launch) ----
def test_abi_host_checks():
    import kernels._lib as kl
    L = kl.lib()
    p = ctypes.c_void_p(16)
    assert L.gq_block_elems(6) == 32 and L.gq_block_bytes(6) == 18
    assert L.gq_version() == 105
    assert L.gq_mmq(6, p, p, p, 4, 4, 100, 100, 4, p, 1 << 20, None) == 1
    assert b"multiple of 32" in L.gq_last_error()
    assert L.gq_mmq_ex(6, 1, p, p, p, 8, 4, 256, 256, 8, p, 1 << 20, None) == 3
    assert b"Q4_0" in L.gq_last_error()
    assert L.gq_mmq_prepared_ex(6, 1, p, p, 1 << 20, p, 8, 4, 256, 8, None) == 3
    assert b"Q4_0" in L.gq_last_error()
    assert L.gq_mmq(7, p, p, p, 4, 4, 256, 256, 4, p, 1 << 20, None) == 3
    assert b"unknown" in L.gq_last_error()
    assert L.gq_block_bytes(7) == 210  # (an unknown type's answer, as before)
    assert L.gq_mmq(6, None, None, None, 0, 4, 96, 96, 4, None, 0, None) == 0
    # the device quantizer exists (the one departure from the other q8_1-only types): its host checks
    assert L.gq_quantize_weights(6, p, p, 100, None) == 1
    assert b"multiple of 32" in L.gq_last_error()
    assert L.gq_quantize_weights(6, None, p, 64, None) == 1
    assert L.gq_quantize_weights(6, None, None, 0, None) == 0
    assert L.gq_quantize_weights(5, p, p, 256, None) == 3  # (Q2_K: host only, as before)
    # null pointer and short workspace at a GEMM token count: refused before the launch
    assert L.gq_mmq(6, None, p, p, 4, 64, 256, 256, 4, p, 1 << 20, None) == 1
    need = L.gq_mmq_call_workspace_size(6, 0, 4, 64, 256)
    assert need == L.gq_mmq_call_workspace_size(4, 0, 4, 64, 256)
    assert 0 < need <= L.gq_mmq_workspace_size(6, 4, 64, 256)
    assert L.gq_mmq(6, p, p, p, 4, 64, 256, 256, 4, p, need - 1, None) == 1
    assert L.gq_mmq_call_workspace_size(6, 0, 4, 4, 256) == 0  # a one-launch decode
    assert L.gq_mmq_call_workspace_size(6, 0, 4, 4, 96) == 0   # (at any K % 32 == 0)
    # Q4_0's activation part is every type's (it depends on the activation format, N and K only)
    for N, K in ((1, 4096), (4, 4096), (4, 11008), (16, 4096), (16, 160)):
        assert kl.workspace_size(6, 0, N, K) == kl.workspace_size(0, 0, N, K)
    # a grouped launch at 5..32 tokens with a Q4_0 item: unsupported, naming the type
    item = (kl.GroupItem * 1)(kl.GroupItem(6, 16, 16, 256, 16, 16, 16, 256))
    assert L.gq_mmq_grouped(item, 1, 8, None) == 3
    assert b"Q4_0" in L.gq_last_error()
    # the sorted expert GEMM and the grouped GEMM take whole 256-element groups only
    assert L.gq_mmq_id_sorted_workspace_size(6, 4, 70, 40, 2, 160) == 0
    assert L.gq_mmq_id_sorted_workspace_size(6, 4, 70, 40, 2, 512) == L.gq_mmq_id_sorted_workspace_size(4, 4, 70, 40, 2, 512) > 0


def test_every_valid_k_has_a_route():
    """K = 32 n at any token count: nothing answers "none" (GQ_EUNSUPPORTED) for a valid K."""
    import kernels._lib as kl
    try:
        kl.reset_tuning()
        kl.set_tuning("GQ_CUS", 256)
        for K in (32, 96, 160, 1120, 2848, 4096 + 32):
            for N in (1, 2, 3, 4, 5, 8, 9, 16, 130, 800):
                for prepared in (False, True):
                    r = kl.route_name(Q40, 70, N, K, prepared=prepared)
                    assert r in ("stream_decode_kernel", "gemv_kernel"), (N, K, prepared, r)
                    assert r == kl.route_name(0, 70, N, K, prepared=prepared)  # (Q8_0's rule)
        # the limit of the four-token decode, as tests/q4_0_model.py derives it
        assert kl.route_name(Q40, 16, 4, 10880) == "stream_decode_kernel"
        assert kl.route_name(Q40, 16, 4, 10912) == "gemv_kernel"
        assert kl.route_name(Q40, 8, 1, 28672) == "stream_decode_kernel"
        assert kl.route_name(Q40, 16, 16, 4016) == "none" and kl.route_name(Q40, 16, 16, 4096, act="fp8") == "none"
    finally:
        kl.reset_tuning()


# ---- 8. routes: Q3_K's at K % 256 == 0, over the grid recorded for type 4 ----
# (act, M, N, K) rows at which type 6 is meant to differ from type 4, with the reason: none on this
# grid.  The GEMM routes, split counts and partial sizes depend on M, N and K alone, and the
# per-launch row limit (2 GiB / row bytes) is not reached by the grid's shapes.  (Off the grid the
# decode limits part: Q4_0's decode keeps Q8_0's activation image in LDS, 1.125 K bytes per token,
# where Q3_K's keeps two code sums per block besides, 1.375 K -- four tokens of K = 8960..10880 are on
# the one-launch decode for Q4_0 and on act_quant + gemv_kernel for Q3_K;
# test_every_valid_k_has_a_route holds that limit to Q8_0's.)
_INTENDED_DIFFERENCES = {}


def test_routes_and_sizes_follow_q3_k():
    import kernels._lib as kl
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_routes.npz"))
    assert str(g["knobs"][0]) == ""  # (knob 0: the default tuning)
    sel = (g["type"] == Q3) & (g["knob"] == 0)
    rows = sorted({(int(a), int(M), int(N), int(K)) for a, M, N, K in
                   zip(g["act"][sel], g["M"][sel], g["N"][sel], g["K"][sel])})
    assert len(rows) > 100
    L = kl.lib()

    def ask(t, a, M, N, K):
        return (L.gq_debug_route(t, a, M, N, K, 0).decode(), L.gq_debug_route(t, a, M, N, K, 1).decode(),
                int(L.gq_mmq_workspace_size_ex(t, a, M, N, K)), int(L.gq_mmq_call_workspace_size(t, a, M, N, K)))
    bad, seen = [], set()
    try:
        kl.reset_tuning()
        kl.set_tuning("GQ_CUS", 256)  # (host-only answers, as test_route_golden.py)
        for a, M, N, K in rows:
            if (a, M, N, K) in _INTENDED_DIFFERENCES:
                continue
            got, want = ask(Q40, a, M, N, K), ask(Q3, a, M, N, K)
            seen.update(got[:2])
            if got != want:
                bad.append((a, M, N, K, got, want))
        # the valid K set is the other difference: Q3_K refuses what is no multiple of 256
        assert ask(Q40, 0, 70, 16, 160)[0] == "gemv_kernel" and ask(Q3, 0, 70, 16, 160)[0] == "none"
        assert kl.route_name(Q40, 16, 4, 10880) == "stream_decode_kernel"
        assert kl.route_name(Q3, 16, 4, 10752) == "gemv_kernel" and kl.route_name(Q40, 16, 4, 10752) == "stream_decode_kernel"
    finally:
        kl.reset_tuning()
    assert not bad, f"{len(bad)} rows differ (act, M, N, K, type 6, type 4), the first: {bad[:5]}"
    # the grid reaches every route of the type
    for name in ("stream_decode_kernel", "gemv_kernel", "sgemm_kernel", "hipBLASLt", "none"):
        assert any(name in r for r in seen), (name, sorted(seen))


# ---- 9. the earlier types' workspace sizes: unchanged ----
def test_workspace_of_other_types_unchanged():
    import kernels._lib as kl
    from test_q2k_host import _PARENT_WS_Q3
    from test_q3k_host import _PARENT_WS
    table = {**_PARENT_WS, **_PARENT_WS_Q3}
    assert len(table) == 5 * 8
    for (t, M, N, K), want in table.items():
        assert kl.workspace_size(t, M, N, K) == want, (t, M, N, K)
        if t == 4:  # (Q4_0 at these shapes: Q3_K's sizes)
            assert kl.workspace_size(Q40, M, N, K) == want
