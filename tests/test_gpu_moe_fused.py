"""GPU tests of the fused MoE decode (gq_mmq_id_glu: csrc/mmq_decode.hip stream_decode_id_glu_kernel;
gq_moe_combine: csrc/moe_combine.hip; kernels/moe.py MoEFFN(fused=True)).

The GLU entry is defined on bits the library already produces: with g and u read back from
mmq_id on the same inputs, H must be fp16(silu(g) * u).  The entry evaluates that in fp32 (errors
of a few 2^-24 relative) and the model (tests/moe_fused_model.py) in float64, both rounded once to
fp16 (half an ulp = 2^-12 relative): only a value within ~1e-6 of a rounding tie can come out
different, and then by one step -- hence "within 1 ulp16", with the count of such elements printed.
The combine entry's arithmetic is fully specified, so it is compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

import moe_fused_model as MF
import q2k_model as Q2
import q3k_model as Q3
import q4_0_model as Q40
import q5k_model as Q5
from gpu_types import dev as _dev, no_timeouts as _no_timeouts, same_bits as _same_bits, to_w as _w
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

# (type, E, M, K): one per geometry of the decode body and per type
CASES = [("q4_k", 4, 200, 1024),
         ("q4_k", 3, 96, 14336),   # segmented rows
         ("q6_k", 4, 257, 1536),   # ring image
         ("q6_k", 3, 64, 9216),    # packed, segmented
         ("q8_0", 5, 333, 1056),   # K not a multiple of 64
         ("q5_k", 4, 130, 2048),
         ("q3_k", 4, 130, 2048),
         ("q2_k", 4, 130, 2048),
         ("q4_0", 3, 65, 96),      # several short rows per wave pass
         ("q4_0", 3, 96, 7168)]
PAIRS = [(1, 1), (4, 2), (8, 8)]


@functools.lru_cache(maxsize=None)
def _experts(fmt, E, M, K, which=0):
    """E packed matrices back to back, read-only (which: 0 gate, 1 up, 2 down)."""
    raw = np.concatenate([random_blocks(fmt, M, K, seed=7000 * which + 1000 * E + 10 * M + e) for e in range(E)])
    raw.setflags(write=False)
    return raw


def _ids(N, S, E, seed=0):
    rng = np.random.default_rng(seed + 97 * N + S)
    ids = rng.integers(0, E, size=(N, S), dtype=np.int32)
    ids[:, 0] = ids[0, 0]
    return ids


def _x(N, K, seed):
    """Activations scaled so that silu(g) * u stays in fp16 range."""
    return random_activations(N, K, seed=seed) / np.float16(16)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check_glu(H, g, u, what):
    """H within 1 ulp16 of the model on g, u (all torch fp16 device tensors); prints the flips."""
    h, want = H.cpu().numpy(), MF.glu(g.cpu().numpy(), u.cpu().numpy())
    assert np.isfinite(h).all() and np.isfinite(want).all(), what
    d = MF.ulp16(h, want)
    print(f"{what}: {int((d != 0).sum())} of {d.size} elements one step from the float64 model, max {int(d.max())}")
    assert int(d.max()) <= 1, (what, int(d.max()))


@pytest.mark.parametrize("N,S", PAIRS)
@pytest.mark.parametrize("fmt,E,M,K", CASES)
def test_glu_definition(fmt, E, M, K, N, S):
    import kernels._lib as kl
    gtype = kl.TYPES[fmt]
    Ag, Au = _w(_experts(fmt, E, M, K, 0)), _w(_experts(fmt, E, M, K, 1))
    it = torch.from_numpy(_ids(N, S, E)).to(_dev())
    x = torch.from_numpy(_x(N, K, seed=K + N)).to(_dev())
    H = kl.mmq_id_glu(gtype, Ag, Au, it, x, E, M, K)
    g, u = kl.mmq_id(gtype, Ag, it, x, E, M, K), kl.mmq_id(gtype, Au, it, x, E, M, K)
    torch.cuda.synchronize()
    assert H.shape == (N, S, M) and H.dtype == torch.float16
    assert float(H.abs().max()) > 0
    _check_glu(H, g, u, f"{fmt} E={E} {M}x{K} N={N} S={S}")
    _no_timeouts()


@pytest.mark.parametrize("fmt,E,M,K", [CASES[0], CASES[2], CASES[9]])
def test_glu_invalid_ids_give_zero_rows(fmt, E, M, K):
    import kernels._lib as kl
    dev = _dev()
    gtype = kl.TYPES[fmt]
    Ag, Au = _w(_experts(fmt, E, M, K, 0)), _w(_experts(fmt, E, M, K, 1))
    N, S = 4, 2
    ids = _ids(N, S, E, seed=9)
    ids[0, 1], ids[2, 0], ids[3, 1] = -1, E, E + 1000
    it = torch.from_numpy(ids).to(dev)
    x = torch.from_numpy(_x(N, K, seed=11)).to(dev)
    out = torch.full((N, S, M), float("nan"), dtype=torch.float16, device=dev)
    kl.mmq_id_glu(gtype, Ag, Au, it, x, E, M, K, out=out)
    g, u = kl.mmq_id(gtype, Ag, it, x, E, M, K), kl.mmq_id(gtype, Au, it, x, E, M, K)
    torch.cuda.synchronize()
    for n, s in ((0, 1), (2, 0), (3, 1)):
        assert torch.all(_bits(out[n, s]) == 0), (n, s)
    _check_glu(out, g, u, f"{fmt} invalid ids")  # (the neighbours: glu(0, 0) = 0 for the zero rows)
    _no_timeouts()


def test_glu_strides():
    """ldh > M into a sentinel buffer leaves the padding untouched; a strided B view (shared rows
    2K apart; per-slot rows 2K apart) gives the bits of the contiguous copy."""
    import kernels._lib as kl
    dev = _dev()
    fmt, E, M, K, N, S = "q4_k", 4, 200, 1024, 4, 2
    Ag, Au = _w(_experts(fmt, E, M, K, 0)), _w(_experts(fmt, E, M, K, 1))
    it = torch.from_numpy(_ids(N, S, E, seed=3)).to(dev)
    wide = torch.from_numpy(_x(N, 2 * K, seed=6)).to(dev)
    view = wide[:, 300:300 + K]
    assert view.stride(0) == 2 * K
    ref = kl.mmq_id_glu(kl.GQ_Q4_K, Ag, Au, it, view.contiguous(), E, M, K)
    assert _same_bits(kl.mmq_id_glu(kl.GQ_Q4_K, Ag, Au, it, view, E, M, K), ref)
    slots = torch.from_numpy(_x(N * S, 2 * K, seed=7)).to(dev).view(N, S, 2 * K)[:, :, 8:8 + K]
    assert slots.stride(1) == 2 * K and not slots.is_contiguous()
    assert _same_bits(kl.mmq_id_glu(kl.GQ_Q4_K, Ag, Au, it, slots, E, M, K),
                      kl.mmq_id_glu(kl.GQ_Q4_K, Ag, Au, it, slots.contiguous(), E, M, K))
    buf = torch.full((N, S, M + 11), -7.0, dtype=torch.float16, device=dev)
    out = kl.mmq_id_glu(kl.GQ_Q4_K, Ag, Au, it, view, E, M, K, out=buf[:, :, :M])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    assert _same_bits(buf[:, :, :M], ref)
    assert torch.all(buf[:, :, M:] == -7.0)
    _no_timeouts()


@pytest.mark.parametrize("N,S,M", [(1, 1, 1), (3, 2, 513), (8, 8, 4096)])
@pytest.mark.parametrize("wdtype", [np.float16, np.float32])
def test_combine_bit_equal(N, S, M, wdtype):
    import kernels._lib as kl
    dev = _dev()
    rng = np.random.default_rng(N * 1000 + S * 10 + M)
    D = rng.standard_normal((N, S, M + 5)).astype(np.float16)  # ldd > M
    W = rng.standard_normal((N, S)).astype(wdtype)  # negative weights among them
    W.reshape(-1)[0] = 0
    if N * S > 1:
        W.reshape(-1)[1] = np.float16(3e-7).astype(wdtype)  # a subnormal fp16 value
        assert 0 < float(np.float16(W.reshape(-1)[1])) < 6.1e-5
    if N * S > 2:
        W.reshape(-1)[2] = -W.reshape(-1)[2] if W.reshape(-1)[2] > 0 else W.reshape(-1)[2]
    Dt = torch.from_numpy(D).to(dev)[:, :, :M]
    assert M == 1 or not Dt.is_contiguous()
    Y = kl.moe_combine(Dt, torch.from_numpy(W).to(dev))
    torch.cuda.synchronize()
    want = MF.combine(D[:, :, :M], W)
    assert Y.shape == (N, M) and Y.dtype == torch.float16
    assert np.array_equal(Y.cpu().numpy().view(np.uint16), want.view(np.uint16))
    # ldy > M into a sentinel buffer; an unaligned D (the element-wise form) gives the same bits
    buf = torch.full((N, M + 3), -7.0, dtype=torch.float16, device=dev)
    flat = torch.empty(N * S * (M + 5) + 1, dtype=torch.float16, device=dev)
    odd = flat[1:].view(N, S, M + 5)
    odd.copy_(torch.from_numpy(D).to(dev))
    kl.moe_combine(odd[:, :, :M], torch.from_numpy(W).to(dev), out=buf[:, :M])
    torch.cuda.synchronize()
    assert np.array_equal(buf[:, :M].cpu().numpy().view(np.uint16), want.view(np.uint16))
    assert torch.all(buf[:, M:] == -7.0)
    _no_timeouts()


def _tiny_block(kinds, fused, E=4, H=512, F=256):
    """test_gpu_moe.py's tiny block (E=4, hidden 512, ffn 256) with the given (gate, up, down) types."""
    from kernels.moe import GGUFExperts, MoEFFN
    tg, tu, td = kinds
    gate = GGUFExperts(tg, _w(_experts(tg, E, F, H, 0)), E, F, H)
    up = GGUFExperts(tu, _w(_experts(tu, E, F, H, 1)), E, F, H)
    down = GGUFExperts(td, _w(_experts(td, E, H, F, 2)), E, H, F)
    return MoEFFN(gate, up, down, fused=fused)


def _tiny_inputs(N=3, S=2, H=512):
    dev = _dev()
    ids = np.array([[0, 3], [3, 1], [2, 0]], dtype=np.int32)
    x = torch.from_numpy(_x(N, H, seed=21)).to(dev)
    w = torch.softmax(torch.from_numpy(random_activations(N, S, seed=23)).float(), dim=1).to(torch.float16).to(dev)
    return torch.from_numpy(ids).to(dev), x, w


@pytest.mark.parametrize("kinds", [("q4_k", "q4_k", "q6_k"), ("q4_0", "q4_0", "q4_0")])
def test_fused_forward_is_the_composition(kinds):
    import kernels._lib as kl
    ffn = _tiny_block(kinds, fused=True)
    it, x, w = _tiny_inputs()
    y = ffn.forward(x, it, w)
    h = kl.mmq_id_glu(ffn.gate.gtype, ffn.gate.A, ffn.up.A, it, x, ffn.gate.E, ffn.gate.M, ffn.gate.K)
    d = kl.mmq_id(ffn.down.gtype, ffn.down.A, it, h, ffn.down.E, ffn.down.M, ffn.down.K)
    want = kl.moe_combine(d, w)
    torch.cuda.synchronize()
    assert y.shape == (3, 512) and y.dtype == torch.float16
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert _same_bits(y, want)
    # and against the model end to end from the library's own g, u, d
    g, u = ffn.gate(x, it), ffn.up(x, it)
    _check_glu(h, g, u, f"{kinds} block")
    assert np.array_equal(y.cpu().numpy().view(np.uint16), MF.combine(d.cpu().numpy(), w.cpu().numpy()).view(np.uint16))
    _no_timeouts()


def test_unfused_bits_unchanged():
    """fused=False (the default) still is the torch composition of tests/test_gpu_moe.py."""
    ffn = _tiny_block(("q4_k", "q4_k", "q6_k"), fused=False)
    from kernels.moe import MoEFFN
    assert MoEFFN(ffn.gate, ffn.up, ffn.down).fused is False
    it, x, w = _tiny_inputs()
    y = ffn.forward(x, it, w)
    g, u = ffn.gate(x, it), ffn.up(x, it)
    h = torch.nn.functional.silu(g) * u
    want = (w[..., None] * ffn.down(h, it)).sum(1)
    torch.cuda.synchronize()
    assert y.dtype == want.dtype and _same_bits(y, want)
    _no_timeouts()


def test_mixed_gate_up_types_fall_back():
    """Gate and up of different types: no fused kernel; MoEFFN(fused=True) makes the same h from two
    mmq_id calls and still matches the definition and the composition."""
    import kernels._lib as kl
    ffn = _tiny_block(("q4_k", "q5_k", "q6_k"), fused=True)
    it, x, w = _tiny_inputs()
    y = ffn.forward(x, it, w)
    g, u = ffn.gate(x, it), ffn.up(x, it)
    h = kl.glu_torch(g, u)
    _check_glu(h, g, u, "mixed types")
    want = kl.moe_combine(ffn.down(h, it), w)
    torch.cuda.synchronize()
    assert _same_bits(y, want)
    _no_timeouts()


def test_graph_capture_follows_ids_and_weights():
    ffn = _tiny_block(("q4_k", "q4_k", "q6_k"), fused=True)
    it, x, w = _tiny_inputs()
    ffn.forward(x, it, w)  # (first use outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ffn.forward(x, it, w)
    graph.replay()
    torch.cuda.synchronize()
    first = y.clone()
    assert _same_bits(first, ffn.forward(x, it, w))
    it.copy_((it + 1) % 4)
    it[1, 1] = -1
    w.copy_(torch.flip(w, dims=(1,)) * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(y, ffn.forward(x, it, w))
    assert not _same_bits(y, first)
    _no_timeouts()


@pytest.mark.parametrize("fmt,E,M,K,Q", [("q3_k", 4, 130, 2048, Q3), ("q2_k", 4, 130, 2048, Q2),
                                         ("q5_k", 4, 130, 2048, Q5), ("q4_0", 3, 96, 7168, Q40)])
def test_accuracy_no_worse_than_unfused(fmt, E, M, K, Q):
    """Against ref = silu(g64) * u64 from the float64 ideals of sampled rows: the fused H errs at
    most as much as the unfused torch result plus one fp16 rounding (2^-11) -- it has the same g
    and u and one rounding fewer."""
    import kernels._lib as kl
    gtype = kl.TYPES[fmt]
    rg, ru = _experts(fmt, E, M, K, 0), _experts(fmt, E, M, K, 1)
    Ag, Au = _w(rg), _w(ru)
    N, S = 4, 2
    ids = _ids(N, S, E, seed=5)
    it = torch.from_numpy(ids).to(_dev())
    x = _x(N, K, seed=31)
    xt = torch.from_numpy(x).to(_dev())
    H = kl.mmq_id_glu(gtype, Ag, Au, it, xt, E, M, K)
    g, u = kl.mmq_id(gtype, Ag, it, xt, E, M, K), kl.mmq_id(gtype, Au, it, xt, E, M, K)
    Hu = torch.nn.functional.silu(g) * u
    torch.cuda.synchronize()
    Hf, Hu = H.cpu().numpy().astype(np.float64), Hu.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(M + K)
    per, rb = rg.size // E, rg.size // E // M
    for p in (0, 3, 6):
        n, s = divmod(p, S)
        e = int(ids[n, s])
        rows = np.sort(rng.choice(M, size=24, replace=False))
        sub = [np.concatenate([r[e * per + i * rb:e * per + (i + 1) * rb] for i in rows]) for r in (rg, ru)]
        g64, u64 = (Q.ideal(sb, x[n:n + 1], len(rows), 1, K)[0] for sb in sub)
        ref = g64 / (1.0 + np.exp(-g64)) * u64
        ef = np.max(np.abs(Hf[n, s][rows] - ref)) / np.max(np.abs(ref))
        eu = np.max(np.abs(Hu[n, s][rows] - ref)) / np.max(np.abs(ref))
        print(f"{fmt} pair ({n},{s}) expert {e}: fused {ef:.3e}, unfused {eu:.3e}")
        assert ef <= eu + 2.0 ** -11, (p, ef, eu)
    _no_timeouts()


def test_refusal_and_fallback_beyond_64_pairs():
    """65 pairs through the C entry: GQ_EUNSUPPORTED, H untouched.  80 pairs through mmq_id_glu: the
    same definition from two mmq_id calls."""
    import kernels._lib as kl
    dev = _dev()
    fmt, E, M, K = "q4_k", 4, 128, 1024
    Ag, Au = _w(_experts(fmt, E, M, K, 0)), _w(_experts(fmt, E, M, K, 1))
    N, S = 65, 1
    it = torch.zeros((N, S), dtype=torch.int32, device=dev)
    x = torch.from_numpy(_x(N, K, seed=15)).to(dev)
    out = torch.full((N, S, M), 3.0, dtype=torch.float16, device=dev)
    rc = kl.lib().gq_mmq_id_glu(kl.GQ_Q4_K, Ag.data_ptr(), Au.data_ptr(), it.data_ptr(), x.data_ptr(), out.data_ptr(), E, M,
                                N, S, K, K, 0, M, None)
    torch.cuda.synchronize()
    assert rc == kl.GQ_EUNSUPPORTED
    assert torch.all(out == 3.0)
    N, S = 40, 2
    ids = np.stack([np.arange(N) % E, (np.arange(N) + 1 + np.arange(N) // E) % E], axis=1).astype(np.int32)
    ids[5, 1], ids[17, 0] = -1, E
    it = torch.from_numpy(ids).to(dev)
    x = torch.from_numpy(_x(N, K, seed=17)).to(dev)
    H = kl.mmq_id_glu(kl.GQ_Q4_K, Ag, Au, it, x, E, M, K)
    g, u = kl.mmq_id(kl.GQ_Q4_K, Ag, it, x, E, M, K), kl.mmq_id(kl.GQ_Q4_K, Au, it, x, E, M, K)
    torch.cuda.synchronize()
    assert not H[5, 1].any() and not H[17, 0].any()
    _check_glu(H, g, u, "80 pairs (fallback)")
    _no_timeouts()
