"""Attention for Gemma on the GPU: head dim 256, the sliding window and the logit soft-cap of
gq_attn_decode_ex / gq_attn_prefill_ex, against the plain formula in float64 torch on the CPU over the
dequantized cache.  Every element is held to the project's |o - ref| <= 2^-9 * Vmax, Vmax over the
positions the row really attends, and to an exact zero where it attends none (tests/test_gpu_attn.py,
DESIGN.md: a window only removes terms, the cap is 1-Lipschitz and its tanh adds cap * 2^-21)."""
import ctypes

import numpy as np
import pytest
import torch

import kernels._lib as kl
from gpu_types import dev as _dev
from test_gpu_attn import NAN16, _cache, _q
from test_gpu_attn_prefill import _check
from test_gpu_rope import test_rope_append_matches_the_formula as _rope_case  # its bound and byte rule, any D

pytestmark = pytest.mark.gpu
BIG16 = np.frombuffer(np.array([0x7B53], np.uint16).tobytes(), np.uint8)  # fp16 60000 (Q8_0: d = 60000, codes 83 / 123)


def _ref(q, Kd, Vd, lens, N, nh, scale, window=0, cap=0.0):
    """(o float64 (B*N, nh*D), Vmax (B*N, nh)); token at position p attends max(0, p - window + 1) .. p."""
    B, _, kvh, D = Kd.shape
    o, vmax = torch.zeros(B * N, nh, D, dtype=torch.float64), torch.zeros(B * N, nh, dtype=torch.float64)
    for b in range(B):
        k, v = (t[b].repeat_interleave(nh // kvh, dim=1) for t in (Kd, Vd))
        for i in range(max(0, N - lens[b]), N):
            hi = lens[b] - N + i + 1
            lo = max(0, hi - window) if window else 0
            s = torch.einsum("lhd,hd->hl", k[lo:hi], q[b * N + i].double().view(nh, D)) * scale
            p = torch.softmax(cap * torch.tanh(s / cap) if cap else s, dim=1)
            o[b * N + i], vmax[b * N + i] = torch.einsum("hl,lhd->hd", p, v[lo:hi]), v[lo:hi].abs().amax(dim=(0, 2))
    return o.reshape(B * N, nh * D), vmax


def _call(kind, rows, lens, q, cap, N, nh, kvh, D, prefill, kv_len=None, out=None, **opts):
    """rows: (K bytes, V bytes) (B, cap, kvh, rb) uint8 on the CPU -> (o, the call's device arguments)."""
    B, rb, dv = len(lens), rows[0].shape[-1], _dev()
    bufs = [r.reshape(-1).to(dv) for r in rows]
    strides = (kvh * rb, rb, cap * kvh * rb)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dv) if kv_len is None else kv_len
    if prefill:
        return kl.attn_prefill(kind, q.to(dv), *bufs, strides, kv_len, cap, B, N, nh, kvh, D, out=out, **opts), (bufs, strides, kv_len)
    ws = torch.empty(kl.attn_workspace_size(B, N, nh, kvh, D, **opts), dtype=torch.uint8, device=dv)
    return kl.attn_decode(kind, q.to(dv), *bufs, strides, kv_len, cap, B, N, nh, kvh, D, ws, out=out, **opts), (bufs, strides, kv_len, ws)


@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("nh,kvh", [(4, 4), (8, 2), (7, 1)])
@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_decode_256_matches_the_formula(kind, nh, kvh, N, tune):
    D, tile = 256, kl.attn_plan(7, N, nh, kvh, 256)[0]
    # at W = 1 a wave walks 1 tile up to 3 * tile + 5, then 3 (2) and 4 (3) of them: its one slot refilled, both parities
    lens = [tile - 1, tile, tile + 1, 3 * tile + 5, N - 1, 9 * tile + 5, 13 * tile + 3]
    cap = max(lens) + 3
    (kb, kd), (vb, vd) = _cache(kind, 7, cap, kvh, D)
    q = _q(7, N, nh, D)
    ref, vmax = _ref(q, kd, vd, lens, N, nh, D ** -0.5)
    for pin in (1, 3):
        tune(GQ_ATTN_W=pin)
        _check(_call(kind, (kb, vb), lens, q, cap, N, nh, kvh, D, False)[0], ref, vmax, f"{kind} heads {nh}/{kvh} N={N} W={pin}")


@pytest.mark.parametrize("blocks", ["rows-1", "rows+1", "2rows+3"])
@pytest.mark.parametrize("nh,kvh", [(4, 4), (8, 2), (7, 1)])
@pytest.mark.parametrize("kind", ["f16", "q8_0"])
@pytest.mark.parametrize("cus", [1024, 1])
def test_prefill_256_matches_the_formula(cus, kind, nh, kvh, blocks, tune):
    D, G = 256, nh // kvh
    tune(GQ_CUS=cus)
    rows, tile = kl.attn_prefill_plan(5, 64, nh, kvh, D)
    assert rows == (64 if cus == 1024 else 128)
    N = -(-{"rows-1": rows - 1, "rows+1": rows + 1, "2rows+3": 2 * rows + 3}[blocks] // G)
    lens = [P + N for P in (0, 1, tile - 1, tile, 3 * tile + 5)]
    cap = max(lens) + 3
    (kb, kd), (vb, vd) = _cache(kind, 5, cap, kvh, D)
    q = _q(5, N, nh, D)
    _check(_call(kind, (kb, vb), lens, q, cap, N, nh, kvh, D, True)[0], *_ref(q, kd, vd, lens, N, nh, D ** -0.5),
           f"{kind} heads {nh}/{kvh} N={N} rows={rows} tile={tile}")


@pytest.mark.parametrize("N,prefill", [(1, False), (4, False), (40, True)])
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_window_cuts_the_key_range(kind, D, N, prefill, tune):
    nh, kvh = 8, 2
    tile = kl.attn_prefill_plan(3, N, nh, kvh, D)[1] if prefill else kl.attn_plan(3, N, nh, kvh, D)[0]
    cap = 5 * tile + 20 + N
    tune(GQ_ATTN_W=cap // 32 + 3)  # more workgroups than any window has tiles: empty shares occur
    (kb, kd), (vb, vd) = _cache(kind, 3, cap, kvh, D, seed=4)
    q = _q(3, N, nh, D)
    for wd in [w for w in (1, N - 1, tile - 1, tile, tile + 1, 3 * tile + 5, cap - 1) if w >= 1]:
        # the last row's window starts on a tile edge, inside a tile, before position 0
        lens = [L if wd < cap - 1 else min(L, cap - 2) for L in (wd + 2 * tile, wd + tile + 7, max(N, wd - 3))]
        ref, vmax = _ref(q, kd, vd, lens, N, nh, D ** -0.5, wd)
        clean, _ = _call(kind, (kb, vb), lens, q, cap, N, nh, kvh, D, prefill, window=wd)
        _check(clean, ref, vmax, f"{kind} D={D} N={N} window={wd}")
        rows = [r.clone() for r in (kb, vb)]
        for r in rows:  # outside every row's window: +-60000 before the first row's start, NaN from the length on
            for b, L in enumerate(lens):
                r[b, :max(0, L - N - wd + 1)] = torch.from_numpy(np.tile(BIG16, r.shape[-1] // 2))
                r[b, L:] = torch.from_numpy(np.tile(NAN16, r.shape[-1] // 2))
        assert torch.equal(_call(kind, rows, lens, q, cap, N, nh, kvh, D, prefill, window=wd)[0], clean), wd
        if wd == cap - 1:  # a window above every length: the unwindowed call's bits
            assert torch.equal(_call(kind, (kb, vb), lens, q, cap, N, nh, kvh, D, prefill)[0], clean)


@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_one_workgroup_walks_a_long_window_at_256(kind, N, tune):
    D, nh, kvh, tile = 256, 7, 1, 32
    wd, lens = 10 * tile + 5, [11 * tile, 12 * tile + 9, 14 * tile + 7]  # 11 or 12 tiles in the window: 2 or 3 a wave
    tune(GQ_ATTN_W=1)
    (kb, kd), (vb, vd) = _cache(kind, 3, max(lens) + 1, kvh, D, seed=12)
    q = _q(3, N, nh, D)
    out, _ = _call(kind, (kb, vb), lens, q, max(lens) + 1, N, nh, kvh, D, False, window=wd)
    _check(out, *_ref(q, kd, vd, lens, N, nh, D ** -0.5, wd), f"{kind} N={N} window={wd} W=1")


@pytest.mark.parametrize("window", [0, 40])
@pytest.mark.parametrize("N,prefill", [(2, False), (40, True)])
@pytest.mark.parametrize("kind", ["f16", "q8_0"])
@pytest.mark.parametrize("softcap", [50.0, 1.0])
def test_softcap(softcap, kind, N, prefill, window):
    D, nh, kvh, lens = 256, 8, 2, [N + 3, 97, 150]
    (kb, kd), (vb, vd) = _cache(kind, 3, 150, kvh, D, seed=6)
    q = (_q(3, N, nh, D) * (2 * softcap)).to(torch.float16)  # scaled scores of several caps
    out, _ = _call(kind, (kb, vb), lens, q, 150, N, nh, kvh, D, prefill, window=window, softcap=softcap)
    _check(out, *_ref(q, kd, vd, lens, N, nh, D ** -0.5, window, softcap), f"{kind} cap={softcap} N={N} window={window}")


@pytest.mark.parametrize("N,prefill", [(2, False), (40, True)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_options_off_are_the_plain_entries(kind, D, N, prefill):
    nh, kvh, cap, lens = 8, 2, 150, [N, 97, 150]
    (kb, _), (vb, _) = _cache(kind, 3, cap, kvh, D, seed=8)
    q, dv, L = _q(3, N, nh, D).to(_dev()), _dev(), kl.lib()
    want, (bufs, strides, kv_len, *ws) = _call(kind, (kb, vb), lens, q, cap, N, nh, kvh, D, prefill)  # {0, 0.0f} through _ex
    name = "gq_attn_prefill" if prefill else "gq_attn_decode"
    for fn, tail in ((getattr(L, name), ()), (getattr(L, name + "_ex"), (None,))):  # the old entry, then _ex with NULL
        o = torch.zeros_like(want)
        args = [kl.KV_KINDS[kind], q.data_ptr(), nh * D, bufs[0].data_ptr(), bufs[1].data_ptr(), *strides, kv_len.data_ptr(), cap,
                o.data_ptr(), nh * D, D ** -0.5, 3, N, nh, kvh, D] + ([] if prefill else [ws[0].data_ptr(), ws[0].numel()])
        assert fn(*args, *tail, ctypes.c_void_p(kl._stream(dv))) == 0, L.gq_last_error()
        assert torch.equal(o, want)


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "qknorm"])
@pytest.mark.parametrize("n_rot", [256, 64])
@pytest.mark.parametrize("mode", ["norm", "neox"])
@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_rope_append_256_matches_the_formula(kind, mode, n_rot, norm):
    _rope_case(kind, 256, mode, 256 // n_rot, norm)


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_kv_append_256_writes_the_producer_bytes(kind):
    B, N, kvh, D, cap, dv = 2, 3, 2, 256, 9, _dev()
    rb, lens = kl.kv_row_bytes(kind, D), [5, 9]
    k, v = (_q(B, N, kvh, D, seed=s).to(dv) for s in (1, 2))
    caches = [torch.full((B, cap, kvh, rb), 0xA5, dtype=torch.uint8, device=dv) for _ in range(2)]
    kl.kv_append(kind, k, v, *caches, (kvh * rb, rb, cap * kvh * rb), torch.tensor(lens, dtype=torch.int32, device=dv), cap, B, N, kvh, D)
    for x, got in zip((k, v), caches):
        want = torch.full_like(got, 0xA5)
        rows = (x.view(torch.uint8) if kind == "f16" else kl.quantize_weights_device("q8_0", x).view(torch.uint8)).reshape(B, N, kvh, rb)
        for b, L in enumerate(lens):
            want[b, L - N:L] = rows[b]
        assert torch.equal(got, want)


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_kvcache_256_windowed_prefill_chunk_then_decode(kind):
    from kernels import KVCache
    B, kvh, nh, D, cap, dv = 2, 2, 8, 256, 70, _dev()
    cache = KVCache(B, cap, kvh, D, kind, dv)
    ks, vs = [], []
    for step, N in enumerate((40, 24, 1)):
        k, v, q = (_q(B, N, h, D, seed=10 * step + s) for s, h in ((0, kvh), (1, kvh), (2, nh)))
        cache.append(k.to(dv), v.to(dv))
        out = cache.attend(q.to(dv), window=24, softcap=50.0)
        ks.append(k.view(B, N, kvh, D)), vs.append(v.view(B, N, kvh, D))
        kd, vd = (torch.cat(t, dim=1) for t in (ks, vs))
        if kind == "q8_0":  # what the cache holds: the producer's blocks of the same rows
            deq = lambda x: kl.dequantize_device(kl.GQ_Q8_0, kl.quantize_weights_device("q8_0", x.contiguous().to(dv)),  # noqa: E731
                                                 x.numel() // 32, 32).cpu().reshape(x.shape)
            kd, vd = deq(kd), deq(vd)
        _check(out, *_ref(q, kd.double(), vd.double(), [kd.shape[1]] * B, N, nh, D ** -0.5, 24, 50.0), f"{kind} step {step}")


def test_windowed_decode_replays_from_a_graph_over_changing_lengths():
    kind, D, nh, kvh, cap, N, lens, dv = "f16", 256, 8, 2, 150, 2, [45, 97, 130], _dev()
    (kb, _), (vb, _) = _cache(kind, 1, cap, kvh, D, seed=5)
    q, o = _q(1, N, nh, D).to(dv), torch.empty(N, nh * D, dtype=torch.float16, device=dv)
    _, (bufs, strides, kv_len, ws) = _call(kind, (kb, vb), [lens[0]], q, cap, N, nh, kvh, D, False, window=40)
    call = lambda: kl.attn_decode(kind, q, *bufs, strides, kv_len, cap, 1, N, nh, kvh, D, ws, out=o, window=40)  # noqa: E731
    eager = {L: (kv_len.fill_(L), call().clone())[1] for L in lens}
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
