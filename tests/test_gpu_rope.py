"""Fused per-head norm + RoPE + KV append on the GPU (gq_rope_append; kernels/attention.py RoPE,
KVCache.append_rope) against the plain formula in float64 torch on the CPU.  Every rotated element is held
to |out - exact| <= 2^-11 |exact| + 2^-25 + kappa m (|y0| + |y1|), kappa = 2^-19 without a norm and 2^-16
with one (include/gguf_mmq.h derives it; a pass-through element: |y| for m (|y0| + |y1|)); V rows and
Q8_0 bytes are exact."""
import functools

import pytest
import torch

import kernels._lib as kl
from gpu_types import dev as _dev
from kernels import KVCache, RoPE

pytestmark = pytest.mark.gpu
M = 1.25


def _rows(T, heads, D, seed):
    return torch.randn(T, heads * D, generator=torch.Generator().manual_seed(seed)).to(torch.float16)


@functools.lru_cache(maxsize=None)
def _rope(D, n_rot, mode, norm, base=10000.0):
    f, _ = RoPE.table(n_rot, base)
    w = [1 + 0.1 * torch.randn(D, generator=torch.Generator().manual_seed(40 + s)) for s in (0, 1)] if norm else [None, None]
    return RoPE(torch.from_numpy(f).float(), n_rot, mode, M, w[0], w[1], 1e-6)


def _on(rope, dv):
    mv = lambda t: None if t is None else t.to(dv)  # noqa: E731
    return RoPE(mv(rope.inv_freq), rope.n_rot, rope.mode, rope.mscale, mv(rope.q_norm), mv(rope.k_norm), rope.eps)


def _ref(x, pos, rope, w, D):
    """x fp16 (T, heads*D), pos (T) -> (exact float64, bound), both (T, heads*D)."""
    y = x.double().view(x.shape[0], -1, D)
    kappa = 2.0 ** -19
    if w is not None:
        y, kappa = y * torch.rsqrt((y * y).mean(-1, keepdim=True) + rope.eps) * w.double(), 2.0 ** -16
    h = rope.n_rot // 2
    th = torch.tensor(pos, dtype=torch.float64)[:, None, None] * rope.inv_freq.double()
    c, s = rope.mscale * torch.cos(th), rope.mscale * torch.sin(th)
    i0 = torch.arange(0, rope.n_rot, 2) if rope.mode == "norm" else torch.arange(h)
    i1 = i0 + 1 if rope.mode == "norm" else i0 + h
    out, mag = y.clone(), y.abs()
    out[..., i0], out[..., i1] = y[..., i0] * c - y[..., i1] * s, y[..., i0] * s + y[..., i1] * c
    mag[..., i0] = mag[..., i1] = rope.mscale * (y[..., i0].abs() + y[..., i1].abs())
    return out.reshape(x.shape), (2.0 ** -11 * out.abs() + 2.0 ** -25 + kappa * mag).reshape(x.shape)


def _within(got, ref, what):
    exact, bound = ref
    worst = ((got.double().cpu() - exact).abs() / bound).max().item()
    print(f"{what}: max error = {worst:.3f} of the bound")
    assert worst <= 1.0, what


def _positions(lens, N):
    return [L - N + i for L in lens for i in range(N)]


def _append_rope(kind, rope, q, k, v, lens, cap, kvh, D):
    """KVCache.append_rope on caches pre-filled with 0xA5 -> (q out, K cache, V cache (B, cap, kvh, rb) uint8)."""
    dv, B = _dev(), len(lens)
    N = q.shape[0] // B
    cache = KVCache(B, cap, kvh, D, kind, dv)
    cache.k.fill_(0xA5), cache.v.fill_(0xA5)
    cache.kv_len.copy_(torch.tensor(lens, dtype=torch.int32) - N)
    out = cache.append_rope(q.to(dv), k.to(dv), v.to(dv), _on(rope, dv))
    assert cache.kv_len.tolist() == lens
    return out, cache.k.view(B, cap, kvh, -1), cache.v.view(B, cap, kvh, -1)


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "qknorm"])
@pytest.mark.parametrize("part", [1, 2], ids=["full", "half"])
@pytest.mark.parametrize("mode", ["norm", "neox"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_rope_append_matches_the_formula(kind, D, mode, part, norm):
    B, N, nh, kvh, cap, lens = 3, 5, 4, 2, 70, [5, 40, 70]
    rope = _rope(D, D // part, mode, norm)
    q, k, v = _rows(B * N, nh, D, 1), _rows(B * N, kvh, D, 2), _rows(B * N, kvh, D, 3)
    pos = _positions(lens, N)
    qo, Kf, Vf = _append_rope("f16", rope, q, k, v, lens, cap, kvh, D)
    qk, Kk, Vk = (qo, Kf, Vf) if kind == "f16" else _append_rope(kind, rope, q, k, v, lens, cap, kvh, D)
    _within(qk, _ref(q, pos, rope, rope.q_norm, D), "q")
    assert torch.equal(qk, qo)
    krot = torch.stack([Kf[b, L - N:L] for b, L in enumerate(lens)]).contiguous().view(torch.float16).reshape(B * N, kvh * D)
    dv, rb = _dev(), kl.kv_row_bytes(kind, D)
    want = [torch.full((B, cap, kvh, rb), 0xA5, dtype=torch.uint8, device=dv) for _ in range(2)]
    if kind == "f16":
        _within(krot, _ref(k, pos, rope, rope.k_norm, D), "k")
        for full, rows in zip(want, (krot, v.to(dv))):
            for b, L in enumerate(lens):
                full[b, L - N:L] = rows.view(torch.uint8).reshape(B, N, kvh, rb)[b]
    else:  # the bytes gq_kv_append makes of the f16 form's rotated k, and of v, in the same pattern
        kl.kv_append(kind, krot, v.to(dv), want[0], want[1], (kvh * rb, rb, cap * kvh * rb),
                     torch.tensor(lens, dtype=torch.int32, device=dv), cap, B, N, kvh, D)
    assert torch.equal(Kk, want[0]) and torch.equal(Vk, want[1])


@pytest.mark.parametrize("mode", ["norm", "neox"])
def test_far_positions_keep_the_bound(mode):
    D, nh, kvh, N, cap = 64, 2, 1, 3, 131072
    rope = _rope(D, D, mode, False)
    q, k, v = _rows(N, nh, D, 4), _rows(N, kvh, D, 5), _rows(N, kvh, D, 6)
    qo, Kc, Vc = _append_rope("f16", rope, q, k, v, [cap], cap, kvh, D)
    pos = _positions([cap], N)
    _within(qo, _ref(q, pos, rope, None, D), f"q at {pos}")
    _within(Kc[0, cap - N:].contiguous().view(torch.float16).reshape(N, D), _ref(k, pos, rope, None, D), f"k at {pos}")
    assert torch.equal(Vc[0, cap - N:].contiguous().view(torch.float16).reshape(N, D).cpu(), v)


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_strides_in_place_and_packed_qkv(kind):
    B, N, nh, kvh, D, cap, lens, shift, dv = 2, 3, 4, 2, 64, 20, [3, 20], 6, _dev()
    rope, rb = _rope(D, D // 2, "neox", True), kl.kv_row_bytes(kind, D)
    q, k, v = _rows(B * N, nh, D, 7), _rows(B * N, kvh, D, 8), _rows(B * N, kvh, D, 9)
    qo, Kc, Vc = _append_rope(kind, rope, q, k, v, lens, cap, kvh, D)
    buf = torch.full((B * N, (nh + 2 * kvh) * D + 24), 3.0, dtype=torch.float16, device=dv)
    cq, ck = nh * D, (nh + kvh) * D
    buf[:, :cq], buf[:, cq:ck], buf[:, ck:ck + kvh * D] = q.to(dv), k.to(dv), v.to(dv)
    before = buf.clone()
    caches = [torch.full((shift + B * kvh * cap * rb,), 0xA5, dtype=torch.uint8, device=dv) for _ in range(2)]
    r = _on(rope, dv)
    out = kl.rope_append(kind, r.mode, buf[:, :cq], buf[:, cq:ck], buf[:, ck:ck + kvh * D], caches[0], caches[1],
                         (rb, cap * rb, kvh * cap * rb), torch.tensor(lens, dtype=torch.int32, device=dv), cap, r.inv_freq,
                         r.n_rot, B, N, nh, kvh, D, r.mscale, r.q_norm, r.k_norm, r.eps, out=buf[:, :cq], kv_offset=shift)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf[:, :cq], qo)
    assert torch.equal(buf[:, cq:], before[:, cq:])
    for got, want in zip(caches, (Kc, Vc)):  # head-major at a shifted base: the same rows
        assert (got[:shift] == 0xA5).all()
        assert torch.equal(got[shift:].view(B, kvh, cap, rb).permute(0, 2, 1, 3), want)


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_a_position_outside_the_cache_is_skipped(kind):
    B, N, nh, kvh, D, cap, guard, dv = 2, 3, 2, 1, 128, 8, 4096, _dev()
    lens, rb, rope = [cap + 2, 5], kl.kv_row_bytes(kind, D), _rope(D, D, "norm", False)
    q, k, v = _rows(B * N, nh, D, 10), _rows(B * N, kvh, D, 11), _rows(B * N, kvh, D, 12)
    caches = [torch.full((B * cap * kvh * rb + guard,), 0xA5, dtype=torch.uint8, device=dv) for _ in range(2)]
    r = _on(rope, dv)
    out = kl.rope_append(kind, r.mode, q.to(dv), k.to(dv), v.to(dv), caches[0], caches[1], (kvh * rb, rb, cap * kvh * rb),
                         torch.tensor(lens, dtype=torch.int32, device=dv), cap, r.inv_freq, r.n_rot, B, N, nh, kvh, D, r.mscale)
    _within(out, _ref(q, _positions(lens, N), rope, None, D), "q, two positions past the capacity")
    # sequence 0 holds its first token alone, at cap - 1: what a one-token call at that length writes
    _, K1, V1 = _append_rope(kind, rope, q[::N], k[::N], v[::N], [cap, lens[1] - N + 1], cap, kvh, D)
    for got, one in zip(caches, (K1, V1)):
        assert (got[-guard:] == 0xA5).all()
        got = got[:-guard].view(B, cap, kvh, rb)
        assert torch.equal(got[0], one[0])
        assert (got[1, :lens[1] - N] == 0xA5).all() and (got[1, lens[1]:] == 0xA5).all() and (got[1, lens[1] - N:lens[1]] != 0xA5).any()


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_append_rope_then_attend_is_the_unfused_path(kind):
    B, nh, kvh, D, cap, dv = 2, 8, 2, 128, 64, _dev()
    rope = _rope(D, D, "neox", True)
    fused, plain = KVCache(B, cap, kvh, D, kind, dv), KVCache(B, cap, kvh, D, kind, dv)
    L, vs = 0, []
    for step, N in enumerate((40, 1)):  # a prompt (gq_attn_prefill), then a decode step (gq_attn_decode)
        q, k, v = (_rows(B * N, h, D, 20 + 3 * step + s) for s, h in ((0, nh), (1, kvh), (2, kvh)))
        pos = _positions([L + N] * B, N)
        a = fused.attend(fused.append_rope(q.to(dv), k.to(dv), v.to(dv), _on(rope, dv)))
        plain.append(_ref(k, pos, rope, rope.k_norm, D)[0].to(torch.float16).to(dv), v.to(dv))
        b = plain.attend(_ref(q, pos, rope, rope.q_norm, D)[0].to(torch.float16).to(dv))
        vs.append(v.view(B, N, kvh, D))
        vmax = torch.cat(vs, dim=1).abs().double().cummax(dim=1)[0].amax(dim=3)[:, L:]      # (B, N, kvh): positions <= the token's
        L += N
        err = (a.double() - b.double()).abs().cpu().view(B, N, kvh, -1)
        worst = (err / (2.0 ** -9 * vmax[..., None])).max().item()
        print(f"{kind} N={N}: max |fused - unfused| = {worst:.3f} of 2^-9 Vmax")
        assert worst <= 1.0
