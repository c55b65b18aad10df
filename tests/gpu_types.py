"""The GPU checks that the added block types share (tests/test_gpu_q5k.py, test_gpu_q3k.py,
test_gpu_q2k.py, test_gpu_q4_0.py), as plain functions over a per-type descriptor: each of those
files keeps its own test functions, names and parameters, and a shared test's body is one call
into here.  What differs between types is an argument.  The device helpers serve the MoE files too.

A type's file builds `T = GpuType(name, model module, kernels.mmq_<t> entry)` and imports the
autouse fixture `no_timeouts_after_each_test` by name."""
import dataclasses
import types
import typing

import numpy as np
import pytest
import torch

import kernels._lib as kl
import type_models as TM
from utils.synth import random_activations, random_blocks

# the library's streaming GEMM, one K split, whatever the token count
SGEMM_PINS = dict(GQ_SGEMM=1, GQ_SGEMM_SPLITS=1, GQ_SKINNY=0, GQ_RGEMM=0, GQ_KSTREAM=0)


@dataclasses.dataclass(frozen=True)
class GpuType:
    name: str                 # "q2_k"
    model: types.ModuleType   # tests/q2k_model.py: the format's own functions
    mmq: typing.Callable      # kernels.mmq_q2_k.mmq_q2_k

    @property
    def gtype(self):
        return kl.TYPES[self.name]

    def row_bytes(self, K):
        return K // kl.BLOCK_ELEMS[self.gtype] * kl.BLOCK_BYTES[self.gtype]

    def ideal(self, raw, B, M, N, K):
        return TM.judge(self.name, raw, B, M, N, K)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def to_w(raw):
    return torch.from_numpy(np.array(raw).view(np.int8)).to(dev())  # (a copy: the shared cases are read-only)


def to_x(B):
    return torch.from_numpy(np.array(B)).to(dev())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def no_timeouts():
    assert kl.lib().gq_debug_sync_timeouts() == 0


@pytest.fixture(autouse=True)
def no_timeouts_after_each_test():
    yield
    no_timeouts()


def run(T, raw, B, M, N, K):
    C = T.mmq(to_w(raw), to_x(B), M, N, K)
    torch.cuda.synchronize()
    assert C.shape == (N, M) and C.dtype == torch.float16
    return C.cpu().numpy()


def parity(T, M, N, K):
    raw, B, want = T.model.case(M, N, K)
    err = TM.rel_err(run(T, raw, B, M, N, K), want)
    print(f"{T.name} {M}x{N}x{K}: max|d|/max|C| = {err:.2e}")
    assert err <= TM.tight(N), (M, N, K, err)
    no_timeouts()


def experts(fmt, E, M, K, seed=0):
    return np.concatenate([random_blocks(fmt, M, K, seed=3000 * E + 10 * M + e + seed) for e in range(E)])


def by_expert(ids, E):
    flat = ids.reshape(-1)
    return {e: np.nonzero(flat == e)[0].tolist() for e in range(E) if (flat == e).any()}


def grouped_items(group, N):
    """One (type id, weights, activations, M, K, None) item per (type name, M, K) of the group, for
    launches that are to be refused."""
    return [(kl.TYPES[f], to_w(random_blocks(f, M, K, seed=i)), to_x(random_activations(N, K, seed=i)), M, K, None)
            for i, (f, M, K) in enumerate(group)]


# ---- parity on the type's shapes, by route ----
def check_decode(T, M, N, K):
    assert kl.route_name(T.gtype, M, N, K) == "stream_decode_kernel"
    parity(T, M, N, K)


def check_long_rows(T, M, N, K):
    r = kl.route_name(T.gtype, M, N, K)
    assert r == ("stream_decode_kernel" if N == 1 else "gemv_kernel"), r
    parity(T, M, N, K)


def check_gemv(T, M, N, K):
    assert kl.route_name(T.gtype, M, N, K) == "gemv_kernel"
    parity(T, M, N, K)


def check_gemm(T, M, N, K):
    assert "sgemm" in kl.route_name(T.gtype, M, N, K)
    parity(T, M, N, K)


def check_splitk_shapes_split(T):
    for M, N, K in T.model.SPLITK_SHAPES:
        r = kl.route_name(T.gtype, M, N, K)
        assert "split-K" in r or "reduce" in r, r


def check_dequantize_bit_equal(T):
    M, K = 37, 768
    raw = random_blocks(T.name, M, K, seed=4)
    got = kl.dequantize_device(T.gtype, to_w(raw), M, K)
    torch.cuda.synchronize()
    want = T.model.dequant_f32(raw, M, K).astype(np.float16)
    assert np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16))


def check_blas_path(T, M, N, K, tune):
    tune(GQ_BLAS_MIN_TOKENS=9)
    assert "hipBLASLt" in kl.route_name(T.gtype, M, N, K)
    parity(T, M, N, K)


def check_forced_routes_keep_sgemm(T, knob, tune):
    tune(**{knob: 4 if knob == "GQ_GEMM_SPLITS" else (0 if knob == "GQ_SGEMM" else 1)})
    for M, N in ((4096, 16), (4096, 128), (11008, 16), (70, 16)):
        for prepared in (False, True):
            assert "sgemm" in kl.route_name(T.gtype, M, N, 4096 if M > 70 else 512, prepared=prepared), (knob, M, N)
    parity(T, 70, 16, 512)


def check_row_chunks_under_the_launch_limit(T, tune, max_bytes):
    """600 x 24 x 512 in one launch, then under GQ_GEMM_MAX_BYTES = max_bytes (left set for the
    caller's own route assertions): row chunks, each on the streaming GEMM, the same bits."""
    M, N, K = 600, 24, 512
    raw, B = random_blocks(T.name, M, K, seed=8), random_activations(N, K, seed=9)
    tune(GQ_SGEMM_SPLITS=1)
    whole = run(T, raw, B, M, N, K)
    tune(GQ_GEMM_MAX_BYTES=max_bytes)
    assert kl.lib().gq_mmq_call_workspace_size(T.gtype, 0, M, N, K) > 0
    assert "sgemm" in kl.route_name(T.gtype, M, N, K)
    assert np.array_equal(run(T, raw, B, M, N, K).view(np.uint16), whole.view(np.uint16))
    assert TM.rel_err(whole, T.ideal(raw, B, M, N, K)) <= TM.TIGHT_GEMM
    return M, N, K


# ---- invariants ----
def check_activation_scaling_is_exact(T, N, K=768):
    M = 70
    raw, B = random_blocks(T.name, M, K, seed=N), random_activations(N, K, seed=N + 1)
    a, b = run(T, raw, B, M, N, K), run(T, raw, (B * np.float16(2)).astype(np.float16), M, N, K)
    assert np.array_equal((a * np.float16(2)).view(np.uint16), b.view(np.uint16))


def check_row_independence(T, N, tune, K=768):
    if N > 4:
        tune(GQ_SGEMM_SPLITS=1)
    M, r0, r1 = 300, 101, 290
    raw, B = random_blocks(T.name, M, K, seed=N), random_activations(N, K, seed=N + 1)
    rb = T.row_bytes(K)
    full = run(T, raw, B, M, N, K)
    sub = run(T, raw[r0 * rb:r1 * rb], B, r1 - r0, N, K)
    assert np.array_equal(sub.view(np.uint16), full[:, r0:r1].view(np.uint16))


def check_prepared(T, N, K=1024):
    M = 130
    raw, B = random_blocks(T.name, M, K, seed=N), random_activations(N, K, seed=N + 1)
    ws = torch.empty(kl.workspace_size(T.gtype, M, N, K), dtype=torch.uint8, device=dev())
    kl.act_prepare(to_x(B), N, K, ws)
    got = kl.mmq_prepared(T.gtype, to_w(raw), ws, M, N, K)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    if N <= 4:
        assert "stream_decode_kernel" in kl.route_name(T.gtype, M, N, K, prepared=True)
        assert np.array_equal(got.view(np.uint16), run(T, raw, B, M, N, K).view(np.uint16))
    assert TM.rel_err(got, T.ideal(raw, B, M, N, K)) <= TM.tight(N)
    no_timeouts()


# ---- grouped launches: `group` is the type's tuple of (type name, M, K) items ----
def check_grouped_decode_bit_identical(group, N):
    raws = [random_blocks(f, M, K, seed=10 + i) for i, (f, M, K) in enumerate(group)]
    Bs = {K: random_activations(N, K, seed=N + K) for K in sorted({K for _, _, K in group})}
    items = [(kl.TYPES[f], to_w(r), to_x(Bs[K]), M, K, None) for (f, M, K), r in zip(group, raws)]
    outs = kl.mmq_grouped(items, N)
    assert outs is not None, kl.lib().gq_last_error()
    torch.cuda.synchronize()
    for (f, M, K), r, it, C in zip(group, raws, items, outs):
        solo = kl.mmq(it[0], it[1], it[2], M, N, K)
        torch.cuda.synchronize()
        assert torch.equal(C.view(torch.int16), solo.view(torch.int16)), (f, M, K)
        assert TM.rel_err(C.cpu().numpy(), TM.judge(f, r, Bs[K], M, N, K)) <= TM.TIGHT_GEMV, (f, M, K)
    no_timeouts()


def check_grouped_at_gemm_tokens_is_refused(group):
    assert kl.mmq_grouped(grouped_items(group, 8), 8) is None


def check_grouped_prepared_bit_identical(T, group, N, splits, tune):
    tune(GQ_KSTREAM=0, GQ_SGEMM_SPLITS=splits)
    raws = [random_blocks(f, M, K, seed=20 + i) for i, (f, M, K) in enumerate(group)]
    Bs = {K: random_activations(N, K, seed=N + K) for K in sorted({K for _, _, K in group})}
    wss = {}
    for K, B in Bs.items():
        wss[K] = torch.empty(kl.workspace_size(T.gtype, 300, N, K), dtype=torch.uint8, device=dev())
        kl.act_prepare(to_x(B), N, K, wss[K])
    items = [(kl.TYPES[f], to_w(r), wss[K], M, K, None) for (f, M, K), r in zip(group, raws)]
    outs = kl.mmq_grouped_prepared(items, N)
    assert outs is not None, kl.lib().gq_last_error()
    torch.cuda.synchronize()
    tune(GQ_SGEMM=1, GQ_RGEMM=0, GQ_SKINNY=0)  # (the other types' per-matrix call on the streaming GEMM too)
    for (f, M, K), r, it, C in zip(group, raws, items, outs):
        ws = torch.empty(kl.workspace_size(it[0], M, N, K), dtype=torch.uint8, device=dev())
        kl.act_prepare(to_x(Bs[K]), N, K, ws)
        assert "sgemm" in kl.route_name(it[0], M, N, K, prepared=True)
        solo = kl.mmq_prepared(it[0], it[1], ws, M, N, K)
        torch.cuda.synchronize()
        assert torch.equal(C.view(torch.int16), solo.view(torch.int16)), (f, M, K)
        assert TM.rel_err(C.cpu().numpy(), TM.judge(f, r, Bs[K], M, N, K)) <= TM.TIGHT_GEMM, (f, M, K)
    no_timeouts()


# ---- MoE ----
def check_mmq_id_bit_identical_to_one_token_calls(T, K=512):
    E, M, N, S = 4, 70, 3, 2
    raw = experts(T.name, E, M, K)
    A = to_w(raw)
    ids = np.array([[0, 3], [3, 7], [2, 0]], dtype=np.int32)  # (7: out of range)
    x = random_activations(N, K, seed=K + N)
    xt, it, out = to_x(x), torch.from_numpy(ids).to(dev()), torch.empty((N, S, M), dtype=torch.float16, device=dev())
    rc = kl.lib().gq_mmq_id(T.gtype, A.data_ptr(), it.data_ptr(), xt.data_ptr(), out.data_ptr(), E, M, N, S, K, K, 0, M, None)
    assert rc == 0, kl.lib().gq_last_error()
    torch.cuda.synchronize()
    assert same_bits(out, kl.mmq_id(T.gtype, A, it, xt, E, M, K))
    per = M * T.row_bytes(K)
    for n in range(N):
        for s in range(S):
            e = int(ids[n, s])
            if not 0 <= e < E:
                assert not out[n, s].any()
                continue
            solo = kl.mmq(T.gtype, A[e * per:(e + 1) * per], xt[n:n + 1].contiguous(), M, 1, K)
            assert torch.equal(out[n, s], solo[0]), (n, s)
            err = TM.rel_err(out[n, s].cpu().numpy()[None], T.ideal(raw[e * per:(e + 1) * per], x[n:n + 1], M, 1, K))
            assert err <= TM.TIGHT_GEMV, (n, s, err)
    no_timeouts()


def check_mmq_id_sorted_80_pairs(T, M):
    E, K, N, S = 4, 512, 40, 2
    raw = experts(T.name, E, M, K)
    A = to_w(raw)
    ids = np.random.default_rng(M).integers(0, E, size=(N, S), dtype=np.int32)
    ids[5, 1] = E + 2  # (an id out of range: a zero row)
    x = random_activations(N, K, seed=K + N + S)
    xt, it = to_x(x), torch.from_numpy(ids).to(dev())
    got = kl.mmq_id_sorted(T.gtype, A, it, xt, E, M, K)
    torch.cuda.synchronize()
    assert got.shape == (N, S, M)
    g = got.reshape(N * S, M)
    per = M * T.row_bytes(K)
    assert not g[5 * S + 1].any()
    for e, pairs in by_expert(ids, E).items():
        idx = torch.tensor(pairs, dtype=torch.int64, device=dev())
        rows = xt.index_select(0, idx // S).contiguous()
        n = len(pairs)
        assert n >= 5
        with kl.tuning(**SGEMM_PINS):
            assert kl.route_name(T.gtype, M, n, K) == "sgemm_kernel"
            want = kl.mmq(T.gtype, A[e * per:(e + 1) * per], rows, M, n, K)
        torch.cuda.synchronize()
        assert same_bits(g.index_select(0, idx), want), e
        err = TM.rel_err(want.cpu().numpy(), T.ideal(raw[e * per:(e + 1) * per], x[[p // S for p in pairs]], M, n, K))
        print(f"{T.name} sorted E={E} {M}x{K} expert {e}: {n} pairs, max|d|/max|C| = {err:.2e}")
        assert err <= TM.TIGHT_GEMM, (e, err)
    no_timeouts()


# ---- from written GGUF files ----
def check_moe_ffn_from_gguf(tmp_path, N, kinds):
    """kinds: the (gate, up, down) type names of the written block (E=4, S=2, hidden 512, ffn 256)."""
    from gguf.file import read_gguf, write_gguf
    from kernels.moe import MoEFFN
    E, S, H, F = 4, 2, 512, 256
    parts = zip(("ffn_gate_exps", "ffn_up_exps", "ffn_down_exps"), kinds, ((F, H), (F, H), (H, F)))
    raw = {n: (t, M, K, experts(t, E, M, K, i + 1)) for i, (n, t, (M, K)) in enumerate(parts)}
    path = str(tmp_path / "moe.gguf")
    write_gguf(path, {f"blk.2.{n}.weight": (t, (E, M, K), r) for n, (t, M, K, r) in raw.items()})
    _, tensors = read_gguf(path)
    ffn = MoEFFN.from_gguf(tensors, 2, dev())
    assert (ffn.gate.type_name, ffn.up.type_name, ffn.down.type_name) == tuple(kinds)
    assert (ffn.gate.E, ffn.gate.M, ffn.gate.K) == (E, F, H)
    ids = np.random.default_rng(N).integers(0, E, size=(N, S), dtype=np.int32)
    it = torch.from_numpy(ids).to(dev())
    xn = (random_activations(N, H, seed=21) / np.float16(16)).astype(np.float16)  # (keeps silu(g) * u, d in fp16 range)
    x = torch.from_numpy(xn).to(dev())
    w = torch.softmax(torch.from_numpy(random_activations(N, S, seed=23)).float(), dim=1).to(torch.float16).to(dev())
    y = ffn.forward(x, it, w)
    torch.cuda.synchronize()
    assert y.shape == (N, H)
    g, u = ffn.gate(x, it), ffn.up(x, it)
    h = torch.nn.functional.silu(g) * u
    d = ffn.down(h, it)
    torch.cuda.synchronize()
    assert same_bits(y, (w[..., None] * d).sum(1))
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0
    gate = TM.TIGHT_GEMV if N * S <= 64 else TM.TIGHT_GEMM  # (gq_mmq_id's one-token decode / the sorted GEMM)
    gn, un, hn, dn = (t.cpu().numpy().reshape(N * S, -1) for t in (g, u, h, d))
    for e, pairs in by_expert(ids, E).items():
        toks = [p // S for p in pairs]
        for name, got, B in (("ffn_gate_exps", gn, xn[toks]), ("ffn_up_exps", un, xn[toks]),
                             ("ffn_down_exps", dn, np.ascontiguousarray(hn[pairs]))):
            t, M, K, r = raw[name]
            per = r.size // E
            err = TM.rel_err(got[pairs], TM.judge(t, r[e * per:(e + 1) * per], B, M, len(pairs), K))
            assert err <= gate, (name, e, err)
    no_timeouts()


def check_layer_mix_from_gguf(T, tmp_path, fuse, types, want_types):
    """types: the layer's tensor name -> type name (gguf.<mix>_layer_types(0, 32)), which must use
    exactly want_types."""
    from gguf import read_gguf, write_gguf
    from kernels.layer_mix import LayerMix
    assert set(types.values()) == want_types
    shapes = {n: (96, 512) for g in LayerMix.GROUPS[:3] for n in g}
    shapes["ffn_down"] = (64, 768)
    raw = {n: random_blocks(types[n], *shapes[n], seed=i) for i, n in enumerate(shapes)}
    p = tmp_path / "l.gguf"
    write_gguf(p, {f"blk.0.{n}.weight": (types[n], shapes[n], raw[n]) for n in shapes})
    _, tens = read_gguf(p)
    assert tens["blk.0.attn_q.weight"].type_name == T.name
    layer = LayerMix.from_gguf(tens, 0, device=dev(), fuse=fuse)
    for N in (1, 3, 8, 40):
        x, a, y = (random_activations(N, 512, seed=N + 10 * i) for i in range(3))
        h = random_activations(N, 768, seed=N + 1)
        d = {k: to_x(v) for k, v in (("x", x), ("a", a), ("y", y), ("h", h))}
        out = layer.forward(d["x"], d["h"], attn=d["a"], x_ffn=d["y"])
        torch.cuda.synchronize()
        src = {"attn_q": x, "attn_k": x, "attn_v": x, "attn_output": a, "ffn_gate": y, "ffn_up": y, "ffn_down": h}
        for n, (M, K) in shapes.items():
            want = TM.judge(types[n], raw[n], src[n], M, N, K)
            assert TM.rel_err(out[n].cpu().numpy(), want) <= TM.tight(N), (n, N)
    no_timeouts()
