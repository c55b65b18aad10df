"""Q2_K on the host (no GPU): the format pinned against the reference's Q6_K oracle through the
exact split of tests/q2k_model.py (W = W1 - W2), a hand-written block, the block producer, the CPU
MMQ, GGUF I/O, the C ABI's host-side checks, the routes against Q3_K's recorded ones, and a numpy
model of the GPU paths' roundings held to the GPU tests' gates on the GPU tests' own inputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle as O
import q2k_model as Q
from utils.synth import random_activations, random_blocks

Q2, Q3 = 5, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _i8(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int8))


# ---- 1. the format, pinned against the oracle ----
def test_dequantize_equals_oracle_q6_k_difference():
    from utils.quantize._qlib import dequantize
    M, K = 24, 768
    raw = random_blocks("q2_k", M, K, seed=3)
    got = dequantize("q2_k", _i8(raw)).numpy()
    w1, w2 = Q.split_q6_k(raw)
    want = (O.dequant("q6_k", w1).astype(np.float32) - O.dequant("q6_k", w2).astype(np.float32)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32))
    assert np.array_equal(got.view(np.uint32), Q.dequant_f32(raw, M, K).reshape(-1).view(np.uint32))
    from utils.quantize.q2_k import dequantize_q2_k
    h = dequantize_q2_k(_i8(raw), (M, K))
    assert h.dtype == torch.float16 and np.array_equal(h.numpy().reshape(-1), got.astype(np.float16))


def test_model_ideal_agrees_with_oracle_ideal():
    """The oracle's IDEAL rounds each part's fp64 sum once to fp16: the model's fp64 ideal lies
    within half an fp16 ulp of I1 plus half an fp16 ulp of I2 of I1 - I2 (plus the fp64 rounding of
    the summation orders)."""
    M, N, K = 37, 5, 1024
    raw = random_blocks("q2_k", M, K, seed=5)
    B = random_activations(N, K, seed=6)
    w1, w2 = Q.split_q6_k(raw)
    i1 = O.mmq_from_fp16("q6_k", w1, B, M, N, K, O.IDEAL)
    i2 = O.mmq_from_fp16("q6_k", w2, B, M, N, K, O.IDEAL)
    mine = Q.ideal(raw, B, M, N, K)
    bound = 0.5 * np.spacing(np.abs(i1)).astype(np.float64) + 0.5 * np.spacing(np.abs(i2)).astype(np.float64)
    diff = i1.astype(np.float64) - i2.astype(np.float64)
    slack = 1e-12 * (np.abs(i1).astype(np.float64) + np.abs(i2).astype(np.float64))
    assert np.all(np.abs(mine - diff) <= bound + slack)


# ---- 2. a hand-written block: the index formulas, independent of split_q6_k and of unpack ----
# sub-blocks 0..15: sixteen distinct (sc, m) pairs, 0 and 15 of each among them
_SC = [0, 15, 1, 14, 2, 13, 3, 12, 4, 11, 5, 10, 6, 9, 7, 8]
_MN = [15, 0, 3, 7, 1, 14, 9, 2, 12, 5, 8, 11, 4, 13, 6, 10]


def _hand_block():
    """d = 0.5, dmin = 0.25; sub-block s has scale _SC[s] and min _MN[s]; element e of plane
    p = 4*(e/128) + (e%128)/32 has code (e%32 + p) % 4 in the first half (p < 4) and
    ((e%32)/2 + p) % 4 in the second: the eight 32-element planes all differ."""
    def code(e):
        p, l = 4 * (e // 128) + (e % 128) // 32, e % 32
        return (l + p) % 4 if p < 4 else (l // 2 + p) % 4
    q = [code(e) for e in range(256)]
    b = np.zeros(84, np.uint8)
    for e in range(256):
        h, j, l = e // 128, (e % 128) // 32, e % 32
        b[16 + 32 * h + l] |= q[e] << (2 * j)
    for s in range(16):
        b[s] = _SC[s] | (_MN[s] << 4)
    b[80:82] = np.array([0.5], np.float16).view(np.uint8)
    b[82:84] = np.array([0.25], np.float16).view(np.uint8)
    return b, q, np.array([0.5 * _SC[e // 16] * q[e] - 0.25 * _MN[e // 16] for e in range(256)], np.float64)


def test_hand_written_block():
    from utils.quantize._qlib import dequantize
    b, q, want = _hand_block()
    assert len(set(zip(_SC, _MN))) == 16
    assert {0, 15} <= set(_SC) and {0, 15} <= set(_MN)
    planes = [tuple(q[32 * p:32 * p + 32]) for p in range(8)]
    assert len(set(planes)) == 8
    # a few weights by hand: (element, 0.5 * sc * code - 0.25 * m)
    #   e = 0:   plane 0, sub-block 0 (0, 15), code 0                 -> -3.75
    #   e = 17:  plane 0, sub-block 1 (15, 0), code 17 % 4 = 1        -> 7.5
    #   e = 33:  plane 1, sub-block 2 (1, 3), code (1 + 1) % 4 = 2    -> 0.25
    #   e = 127: plane 3, sub-block 7 (12, 2), code (31 + 3) % 4 = 2  -> 11.5
    #   e = 130: plane 4, sub-block 8 (4, 12), code (1 + 4) % 4 = 1   -> -1.0
    #   e = 200: plane 6, sub-block 12 (6, 4), code (4 + 6) % 4 = 2   -> 5.0
    #   e = 255: plane 7, sub-block 15 (8, 10), code (15 + 7) % 4 = 2 -> 5.5
    for e, w in ((0, -3.75), (17, 7.5), (33, 0.25), (127, 11.5), (130, -1.0), (200, 5.0), (255, 5.5)):
        assert want[e] == w, (e, want[e])
    assert np.array_equal(Q.dequant_exact(b, 1, 256).reshape(-1), want)
    assert np.array_equal(dequantize("q2_k", _i8(b)).numpy().astype(np.float64), want)
    d, dmin, sc, m, uq = Q.unpack(b, 1, 256)
    assert sc.reshape(-1).tolist() == _SC and m.reshape(-1).tolist() == _MN
    assert uq.reshape(-1).tolist() == q and float(d[0, 0]) == 0.5 and float(dmin[0, 0]) == 0.25


# ---- 3. the CPU product ----
def test_cpu_mmq_equals_the_model_bit_for_bit():
    from kernels.cpu_impls.mmq_q2_k_q8_1_cpu import mmq_q2_k_q8_1_cpu
    M, N, K = 37, 5, 1024
    raw = random_blocks("q2_k", M, K, seed=5)
    B = random_activations(N, K, seed=6)
    qB = _i8(O.quantize_q8_1(B))
    got = mmq_q2_k_q8_1_cpu(_i8(raw), qB, M, N, K)
    assert got.shape == (N, M) and got.dtype == torch.float16
    want = Q.model_cpu(raw, B, M, N, K)
    assert np.array_equal(got.numpy().view(np.uint16), want.view(np.uint16))
    for th in (1, 3):
        assert torch.equal(mmq_q2_k_q8_1_cpu(_i8(raw), qB, M, N, K, threads=th), got)
    err = Q.rel_err(got.numpy(), Q.ideal(raw, B, M, N, K))
    print(f"gq_cpu_mmq type 5 {M}x{N}x{K}: max|d|/max|C| = {err:.2e}")
    assert err <= Q.tight(N)


# ---- 4. host quantizer ----
def _roundtrip(x):
    from utils.quantize._qlib import dequantize, quantize
    return dequantize("q2_k", quantize("q2_k", torch.from_numpy(x))).numpy().reshape(x.shape)


def test_quantizer_size_determinism_and_zeros():
    from utils.quantize.q2_k import dequantize_q2_k, quantize_to_q2_k
    rng = np.random.default_rng(0)
    x = rng.standard_normal((6, 512)).astype(np.float32)
    q = quantize_to_q2_k(torch.from_numpy(x))
    assert q.dtype == torch.int8 and q.numel() == 6 * 2 * 84
    assert torch.equal(q, quantize_to_q2_k(torch.from_numpy(x.copy())))
    assert dequantize_q2_k(q, (6, 512)).shape == (6, 512)
    with pytest.raises(ValueError):
        quantize_to_q2_k(torch.zeros(100))
    z = _roundtrip(np.zeros(512, np.float32))
    assert np.array_equal(z, np.zeros(512, np.float32))


def test_quantizer_uses_every_code_and_the_mins():
    from utils.quantize._qlib import quantize
    rng = np.random.default_rng(2)
    raw = quantize("q2_k", torch.from_numpy(rng.standard_normal(256 * 8).astype(np.float32))).numpy().view(np.uint8)
    _, _, sc, m, q = Q.unpack(raw, 1, 2048)
    assert set(np.unique(q).tolist()) == {0, 1, 2, 3}
    assert (m > 0).any() and (sc > 0).any()


@pytest.mark.parametrize("dist", ("normal", "uniform"))
def test_quantizer_no_worse_than_the_naive_one(dist):
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((64, 256)) if dist == "normal" else rng.uniform(0, 1, (64, 256))).astype(np.float32)
    rms = lambda y: float(np.sqrt(np.mean((y - x) ** 2)))  # noqa: E731
    mine = rms(_roundtrip(x))
    naive = rms(Q.dequant_f32(Q.naive_quantize(x), 64, 256))
    print(f"round-trip RMSE {dist}: gq_quantize_q2_k {mine:.5f}  naive {naive:.5f}")
    assert mine <= naive, (dist, mine, naive)


# ---- 5. the GPU paths' roundings, modelled: within the GPU tests' gates on their inputs ----
@pytest.mark.parametrize("M,N,K", Q.ALL_SHAPES)
def test_rounding_models_within_gates(M, N, K):
    raw, B, want = Q.case(M, N, K)
    tol = Q.tight(N)
    e_mfma = Q.rel_err(Q.model_mfma(raw, B, M, N, K), want)
    e_dec = Q.rel_err(Q.model_decode(raw, B, M, N, K), want)
    print(f"{M}x{N}x{K}: MFMA model {e_mfma:.2e}  decode model {e_dec:.2e}")
    assert e_mfma <= tol and e_dec <= tol, (e_mfma, e_dec)


# ---- 6. GGUF I/O, the layer-type map, the Python tables ----
def test_gguf_type_10_roundtrip(tmp_path):
    from gguf import GGML_TYPES, read_gguf, write_gguf
    assert GGML_TYPES[10] == ("q2_k", 256, 84)
    raw = random_blocks("q2_k", 12, 512, seed=1)
    exps = random_blocks("q2_k", 3 * 10, 256, seed=2)
    p = tmp_path / "t.gguf"
    write_gguf(p, {"blk.0.attn_q.weight": ("q2_k", (12, 512), raw),
                   "blk.0.ffn_gate_exps.weight": ("q2_k", (3, 10, 256), exps)})
    _, tens = read_gguf(p)
    t = tens["blk.0.attn_q.weight"]
    assert t.type_name == "q2_k" and t.shape == (12, 512)
    assert np.array_equal(np.asarray(t.data).reshape(-1), raw)
    e = tens["blk.0.ffn_gate_exps.weight"]
    assert e.type_name == "q2_k" and e.shape == (3, 10, 256)
    assert np.array_equal(np.asarray(e.data).reshape(-1), exps)


def test_q2_k_layer_types():
    from gguf import LLAMA_LAYER_SHAPES, q2_k_layer_types
    rest = {n: "q2_k" for n in LLAMA_LAYER_SHAPES if n not in ("attn_v", "attn_output", "ffn_down")}
    assert len(rest) == 4
    for layer in (0, 5, 31):
        assert q2_k_layer_types(layer, 32) == dict(rest, attn_v="q3_k", attn_output="q3_k", ffn_down="q3_k")
        assert q2_k_layer_types(layer, 32, n_gqa=1) == q2_k_layer_types(layer, 32)
        assert q2_k_layer_types(layer, 32, n_gqa=8) == dict(rest, attn_v="q4_k", attn_output="q3_k", ffn_down="q3_k")
    assert q2_k_layer_types(0, 32, n_gqa=4)["attn_v"] == "q4_k" and q2_k_layer_types(0, 32, n_gqa=2)["attn_v"] == "q3_k"
    assert "memory" in q2_k_layer_types.__doc__


def test_python_tables():
    import kernels._lib as kl
    from kernels.cpu_impls._cpu import _BYTES, _QK
    from utils.quantize._qlib import BLOCK as QB
    from utils.synth import BLOCK as YB
    assert kl.TYPES["q2_k"] == kl.GQ_Q2_K == 5
    assert kl.BLOCK_ELEMS[5] == 256 and kl.BLOCK_BYTES[5] == 84
    assert QB["q2_k"] == YB["q2_k"] == (256, 84)
    assert _BYTES[5] == 84 and _QK[5] == 256
    raw = random_blocks("q2_k", 2, 512, seed=1).reshape(4, 84)
    dd = raw[:, 80:84].copy().view(np.float16).astype(np.float32)
    assert dd.shape == (4, 2) and np.all((dd >= 0.5 * 2.0 ** -7) & (dd <= 1.5 * 2.0 ** -7))
    _, _, sc, m, _ = Q.unpack(random_blocks("q2_k", 8, 1024, seed=1), 8, 1024)
    assert sc.min() == 0 and sc.max() == 15 and m.min() == 0 and m.max() == 15


# ---- 7. ABI host checks (every call returns before any launch) ----
def test_abi_host_checks():
    import kernels._lib as kl
    L = kl.lib()
    p = ctypes.c_void_p(16)
    assert L.gq_block_elems(5) == 256 and L.gq_block_bytes(5) == 84
    assert L.gq_version() == 105
    assert L.gq_mmq(5, p, p, p, 4, 4, 100, 100, 4, p, 1 << 20, None) == 1
    assert b"multiple of 256" in L.gq_last_error()
    assert L.gq_mmq_ex(5, 1, p, p, p, 8, 4, 256, 256, 8, p, 1 << 20, None) == 3
    assert b"Q2_K" in L.gq_last_error()
    assert L.gq_mmq_prepared_ex(5, 1, p, p, 1 << 20, p, 8, 4, 256, 8, None) == 3
    assert b"Q2_K" in L.gq_last_error()
    assert L.gq_quantize_weights(5, p, p, 256, None) == 3
    assert b"Q2_K" in L.gq_last_error()
    assert L.gq_mmq(7, p, p, p, 4, 4, 256, 256, 4, p, 1 << 20, None) == 3
    assert b"unknown" in L.gq_last_error()
    assert L.gq_block_bytes(7) == 210  # (an unknown type's answer, as before)
    assert L.gq_mmq(5, None, None, None, 0, 4, 256, 256, 4, None, 0, None) == 0
    # null pointer and short workspace at a GEMM token count: refused before the launch
    assert L.gq_mmq(5, None, p, p, 4, 64, 256, 256, 4, p, 1 << 20, None) == 1
    need = L.gq_mmq_call_workspace_size(5, 0, 4, 64, 256)
    assert need == L.gq_mmq_call_workspace_size(4, 0, 4, 64, 256)
    assert 0 < need <= L.gq_mmq_workspace_size(5, 4, 64, 256)
    assert L.gq_mmq(5, p, p, p, 4, 64, 256, 256, 4, p, need - 1, None) == 1
    assert L.gq_mmq_call_workspace_size(5, 0, 4, 4, 256) == 0  # a one-launch decode
    # Q2_K's activation part is every type's (it depends on the activation format, N and K only)
    for N, K in ((1, 4096), (4, 4096), (4, 11008), (16, 4096)):
        assert kl.workspace_size(5, 0, N, K) == kl.workspace_size(1, 0, N, K)
    # a grouped launch at 5..32 tokens with a Q2_K item: unsupported (the caller runs per item)
    item = (kl.GroupItem * 1)(kl.GroupItem(5, 16, 16, 256, 16, 16, 16, 256))
    assert L.gq_mmq_grouped(item, 1, 8, None) == 3


# ---- 8. routes: Q3_K's, over the grid recorded for type 4 ----
# (act, M, N, K) rows at which type 5 is meant to differ from type 4, with the reason: none.  The
# two types share a kTypes row but for the block bytes, and every route choice, split count and
# partial size of the streaming GEMM depends on M, N and K alone; the per-launch row limit that
# does depend on the row bytes (2 GiB / row bytes) is not reached by the grid's shapes.
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
            got, want = ask(Q2, a, M, N, K), ask(Q3, a, M, N, K)
            seen.update(got[:2])
            if got != want:
                bad.append((a, M, N, K, got, want))
    finally:
        kl.reset_tuning()
    assert not bad, f"{len(bad)} rows differ (act, M, N, K, type 5, type 4), the first: {bad[:5]}"
    # the grid reaches every route of the type
    for name in ("stream_decode_kernel", "gemv_kernel", "sgemm_kernel", "hipBLASLt", "none"):
        assert any(name in r for r in seen), (name, sorted(seen))


# ---- 9. the earlier types' workspace sizes: unchanged ----
# gq_mmq_workspace_size(4, M, N, K) at test_q3k_host._PARENT_WS's eight shapes, recorded from a
# build of the parent commit (32ea0dc, on a machine without a GPU: 256 compute units assumed, as on
# an MI355X); types 0..3 are that table's own
_PARENT_WS_Q3 = {
    (4, 4096, 1, 4096): 13312, (4, 4096, 4, 11008): 143360, (4, 4096, 16, 4096): 2320640,
    (4, 11008, 16, 4096): 1983232, (4, 4096, 128, 11008): 21367040, (4, 300, 24, 512): 105728,
    (4, 32000, 64, 4096): 9054720, (4, 4096, 1024, 4096): 80740352,
}


def test_workspace_of_other_types_unchanged():
    import kernels._lib as kl
    from test_q3k_host import _PARENT_WS
    table = {**_PARENT_WS, **_PARENT_WS_Q3}
    assert len(table) == 5 * 8
    for (t, M, N, K), want in table.items():
        assert kl.workspace_size(t, M, N, K) == want, (t, M, N, K)
