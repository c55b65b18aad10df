"""Decode attention on the GPU (gq_attn_decode, gq_kv_append; kernels/attention.py KVCache) against
the plain formula in float64 torch on the CPU over the dequantized cache (Q8_0: float(d) * code,
exact).  Every output element is held to |o - ref| <= 2^-9 * Vmax, Vmax the largest |v| among the
positions the query attends in its kv head: 2^-11 each for P rounded to fp16, the value block's scale
folded into P (Q8_0), the final fp16 rounding, and fp32 summation order with exp2.  Derived, not
measured.  The tile length and W come from the library (gq_debug_attn_plan)."""
import functools

import numpy as np
import pytest
import torch

import kernels._lib as kl
from gpu_types import dev as _dev
from utils.quantize.q8_0 import quantize_to_q8_0

pytestmark = pytest.mark.gpu
NAN16 = np.frombuffer(np.array([0x7E00], np.uint16).tobytes(), np.uint8)  # bytes of an fp16 NaN


@functools.lru_cache(maxsize=None)
def _cache(kind, B, cap, kvh, D, seed=0):
    """Random normal k and v: (row bytes (B, cap, kvh, rb) uint8, dequantized float64 (B, cap, kvh, D)) each."""
    out = []
    for s in (0, 1):
        x = torch.randn(B, cap, kvh, D, generator=torch.Generator().manual_seed(2 * seed + s)).to(torch.float16)
        if kind == "f16":
            out.append((x.view(torch.uint8), x.double()))
        else:
            raw = quantize_to_q8_0(x.reshape(-1)).view(torch.uint8).reshape(B, cap, kvh, D // 32, 34)
            d = raw[..., :2].contiguous().view(torch.float16).double()
            out.append((raw.reshape(B, cap, kvh, -1), (d * raw[..., 2:].view(torch.int8).double()).reshape(B, cap, kvh, D)))
    return out


def _q(B, N, nh, D, seed=7):
    return torch.randn(B * N, nh * D, generator=torch.Generator().manual_seed(seed)).to(torch.float16)


def _ref(q, Kd, Vd, lens, N, nh, scale):
    """(o float64 (B*N, nh*D), Vmax (B*N, nh)) of the formula; lens include the N new tokens."""
    B, _, kvh, D = Kd.shape
    o, vmax = torch.zeros(B * N, nh, D, dtype=torch.float64), torch.zeros(B * N, nh, dtype=torch.float64)
    for b in range(B):
        for i in range(N):
            L = lens[b] - N + i + 1
            k, v = (t[b, :L].repeat_interleave(nh // kvh, dim=1) for t in (Kd, Vd))       # (L, nh, D)
            p = torch.softmax(torch.einsum("lhd,hd->hl", k, q[b * N + i].double().view(nh, D)) * scale, dim=1)
            o[b * N + i], vmax[b * N + i] = torch.einsum("hl,lhd->hd", p, v), v.abs().amax(dim=(0, 2))
    return o.reshape(B * N, nh * D), vmax


def _check(out, ref, vmax, what):
    nh = vmax.shape[1]
    err = (out.double().cpu() - ref).abs().view(ref.shape[0], nh, -1)
    assert torch.isfinite(out).all(), what
    worst = (err / (2.0 ** -9 * vmax[..., None])).max().item()
    print(f"{what}: max error = {worst:.3f} of the 2^-9 Vmax bound")
    assert worst <= 1.0, what
    return worst


def _call(kind, rows, lens, q, cap, N, nh, kvh, D, head_major=False, shift=0, out=None, ws=None, kv_len=None):
    """rows: (K bytes, V bytes) (B, cap, kvh, rb) uint8 on the CPU."""
    B, rb = len(lens), rows[0].shape[-1]
    dv = _dev()
    lay = [r.permute(0, 2, 1, 3) if head_major else r for r in rows]
    bufs = [torch.cat([torch.zeros(shift, dtype=torch.uint8), t.contiguous().reshape(-1)]).to(dv) for t in lay]
    strides = (rb, cap * rb, kvh * cap * rb) if head_major else (kvh * rb, rb, cap * kvh * rb)
    if kv_len is None:
        kv_len = torch.tensor(lens, dtype=torch.int32, device=dv)
    if ws is None:
        ws = torch.empty(kl.attn_workspace_size(B, N, nh, kvh, D), dtype=torch.uint8, device=dv)
    o = kl.attn_decode(kind, q if q.is_cuda else q.to(dv), bufs[0], bufs[1], strides, kv_len, cap, B, N, nh, kvh, D, ws,
                       out=out, kv_offset=shift)
    return o, (bufs, strides, kv_len, ws)


@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("nh,kvh", [(4, 4), (8, 2), (7, 1)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_attention_matches_the_formula(kind, D, nh, kvh, N, tune):
    B = 12
    tile, W = kl.attn_plan(B, N, nh, kvh, D)
    cap = 13 * tile + 3
    # the edges of a tile, the lengths at which a workgroup's share goes from empty to one tile (the last
    # workgroup at one tile, the first at W tiles), and the capacity; then one workgroup per (b, h),
    # where a wave walks four tiles and its ring wraps
    lens = [N, 31, 32, 33, tile - 1, tile + 1, 2 * tile, 2 * tile + 1, min(W * tile - 1, cap), min(W * tile + 1, cap), cap - 1, cap]
    (kb, kd), (vb, vd) = _cache(kind, B, cap, kvh, D)
    q = _q(B, N, nh, D)
    ref, vmax = _ref(q, kd, vd, lens, N, nh, D ** -0.5)
    for pin in (0, 1):
        tune(GQ_ATTN_W=pin)
        out, _ = _call(kind, (kb, vb), lens, q, cap, N, nh, kvh, D)
        _check(out, ref, vmax, f"{kind} D={D} heads {nh}/{kvh} N={N} W={pin or W}")


def test_new_tokens_are_causal_among_themselves():
    kind, D, nh, kvh, cap, L = "f16", 64, 8, 2, 100, 70
    (kb, kd), (vb, vd) = _cache(kind, 1, cap, kvh, D, seed=3)
    q = _q(1, 4, nh, D)
    four, _ = _call(kind, (kb, vb), [L], q, cap, 4, nh, kvh, D)
    _, vmax = _ref(q, kd, vd, [L], 4, nh, D ** -0.5)
    for i in range(4):
        one, _ = _call(kind, (kb, vb), [L - 3 + i], q[i:i + 1], cap, 1, nh, kvh, D)
        err = (one.double() - four[i:i + 1].double()).abs().cpu().view(nh, D)
        assert (err <= 2.0 ** -9 * vmax[i][:, None]).all(), i


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_dead_positions_are_never_used_and_the_length_is_read_on_the_device(kind):
    D, nh, kvh, cap, N, lens = 128, 8, 2, 150, 2, [45, 97, 130]
    (kb, kd), (vb, vd) = _cache(kind, 1, cap, kvh, D, seed=5)
    q, dv = _q(1, N, nh, D), _dev()
    rows = [r.clone() for r in (kb, vb)]
    for r in rows:  # every row at or beyond the shortest length: NaN (Q8_0: NaN in every d)
        r[:, min(lens):] = torch.from_numpy(np.tile(NAN16, r.shape[-1] // 2))
    out, (bufs, strides, kv_len, ws) = _call(kind, rows, [min(lens)], q, cap, N, nh, kvh, D)
    _check(out, *_ref(q, kd, vd, [min(lens)], N, nh, D ** -0.5), f"{kind} NaN beyond the length")
    # the same pointers, only kv_len changed -- eagerly, then as replays of one captured graph
    bufs = [r.reshape(-1).to(dv) for r in (kb, vb)]  # (the whole cache valid again)
    qd, o = q.to(dv), torch.empty(N, nh * D, dtype=torch.float16, device=dv)
    call = lambda: kl.attn_decode(kind, qd, bufs[0], bufs[1], strides, kv_len, cap, 1, N, nh, kvh, D, ws, out=o)
    eager = {}
    for L in lens:
        kv_len.fill_(L)
        eager[L] = call().clone()
        _check(eager[L], *_ref(q, kd, vd, [L], N, nh, D ** -0.5), f"{kind} length {L} from the device")
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        call()
        s.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    for L in lens + lens[::-1]:
        kv_len.fill_(L)
        o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), eager[L].view(torch.int16)), L


def test_a_sequence_does_not_depend_on_its_batch(tune):
    kind, D, nh, kvh, cap, N, lens = "q8_0", 128, 8, 2, 200, 2, [2, 77, 200]
    (kb, kd), (vb, vd) = _cache(kind, 3, cap, kvh, D, seed=9)
    q = _q(3, N, nh, D)
    three, _ = _call(kind, (kb, vb), lens, q, cap, N, nh, kvh, D)
    tune(GQ_ATTN_W=kl.attn_plan(3, N, nh, kvh, D)[1])  # the split depends on the own length and W only
    for b, L in enumerate(lens):
        one, _ = _call(kind, (kb[b:b + 1], vb[b:b + 1]), [L], q[b * N:(b + 1) * N], cap, N, nh, kvh, D)
        assert torch.equal(one.view(torch.int16), three[b * N:(b + 1) * N].view(torch.int16)), b


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_strides_bases_and_padding(kind):
    D, nh, kvh, cap, N, lens, pad = 64, 7, 1, 90, 4, [90, 37], 24
    (kb, kd), (vb, vd) = _cache(kind, 2, cap, kvh, D, seed=11)
    q, dv = _q(2, N, nh, D), _dev()
    ref = _ref(q, kd, vd, lens, N, nh, D ** -0.5)
    qw = torch.full((2 * N, nh * D + pad), 3.0, dtype=torch.float16, device=dv)
    qw[:, 2:2 + nh * D] = q.to(dv)
    for head_major, shift in ((False, 0), (True, 6)):
        ow = torch.full((2 * N, nh * D + pad), -7.0, dtype=torch.float16, device=dv)
        _call(kind, (kb, vb), lens, qw[:, 2:2 + nh * D], cap, N, nh, kvh, D, head_major, shift, out=ow[:, 4:4 + nh * D])
        _check(ow[:, 4:4 + nh * D], *ref, f"{kind} head_major={head_major} shift={shift}")
        assert (ow[:, :4] == -7).all() and (ow[:, 4 + nh * D:] == -7).all()


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_kv_append_writes_the_producer_bytes_and_nothing_else(kind):
    B, N, kvh, D, cap, dv = 2, 3, 2, 64, 9, _dev()
    rb, lens = kl.kv_row_bytes(kind, D), [5, 9]
    k, v = (torch.randn(B * N, kvh * D, generator=torch.Generator().manual_seed(s)).to(torch.float16).to(dv) for s in (1, 2))
    caches = [torch.full((B, cap, kvh, rb), 0xA5, dtype=torch.uint8, device=dv) for _ in range(2)]
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dv)
    kl.kv_append(kind, k, v, caches[0], caches[1], (kvh * rb, rb, cap * kvh * rb), kv_len, cap, B, N, kvh, D)
    for x, got in zip((k, v), caches):
        want = torch.full_like(got, 0xA5)
        rows = x.view(torch.uint8) if kind == "f16" else kl.quantize_weights_device("q8_0", x).view(torch.uint8)
        rows = rows.reshape(B, N, kvh, rb)
        for b, L in enumerate(lens):
            want[b, L - N:L] = rows[b]
        assert torch.equal(got, want)


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_kvcache_append_then_attend_over_three_steps(kind):
    from kernels import KVCache
    B, kvh, nh, D, cap, dv = 2, 2, 8, 128, 40, _dev()
    cache = KVCache(B, cap, kvh, D, kind, dv)
    ks, vs = [], []
    for step, N in enumerate((4, 1, 1)):
        k, v, q = (_q(B, N, h, D, seed=10 * step + s) for s, h in ((0, kvh), (1, kvh), (2, nh)))
        cache.append(k.to(dv), v.to(dv))
        out = cache.attend(q.to(dv))
        ks.append(k.view(B, N, kvh, D)), vs.append(v.view(B, N, kvh, D))
        L = sum(t.shape[1] for t in ks)
        assert cache.kv_len.tolist() == [L, L]
        kd, vd = (torch.cat(t, dim=1) for t in (ks, vs))
        if kind == "q8_0":  # what the cache holds: the producer's blocks of the same rows
            deq = lambda x: kl.dequantize_device(kl.GQ_Q8_0, kl.quantize_weights_device("q8_0", x.contiguous().to(dv)),
                                                 x.numel() // 32, 32).cpu().reshape(x.shape)
            kd, vd = deq(kd), deq(vd)
        _check(out, *_ref(q, kd.double(), vd.double(), [L] * B, N, nh, D ** -0.5), f"{kind} step {step}")
