"""DeepSeek's latent attention on the GPU (gq_mla_decode, gq_mla_append; kernels/attention.py MLACache,
MLAttention) against the plain formulas in float64 torch on the CPU.  Every attention output element is held
to |o - ref| <= 2^-9 * Vmax, Vmax the largest |c_kv| among the positions the row attends: the bound of the
fp16 decode path (P rounded to fp16, the final rounding, fp32 summation order with exp2; nothing in it
depends on the row width), derived, not measured.  The appended rows are held to gq_rope_append's bounds.
The tile length and W come from the library (gq_debug_mla_plan)."""
import functools

import pytest
import torch

import kernels._lib as kl
from gpu_types import dev as _dev
from kernels import MLACache, MLAttention, RoPE

pytestmark = pytest.mark.gpu
RANK, ROPE, DK, SCALE = 512, 64, 576, 192 ** -0.5


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(torch.float16)


@functools.lru_cache(maxsize=None)
def _cache(B, cap, seed=0):
    return _randn(B, cap, DK, seed=seed)


@functools.lru_cache(maxsize=None)
def _ref(lens, N, nh, seed=0, qseed=7):
    """(q fp16 (B*N, nh*576), o float64 (B*N, nh*512), Vmax (B*N, 1)) of the formula over _cache(B, cap, seed)."""
    B, cap = len(lens), max(lens)
    q, C = _randn(B * N, nh * DK, seed=qseed), _cache(B, cap, seed).double()
    o, vmax = torch.zeros(B * N, nh, RANK, dtype=torch.float64), torch.zeros(B * N, 1, dtype=torch.float64)
    for b, L in enumerate(lens):
        c, lim = C[b, :L], L - N + torch.arange(N)
        s = torch.einsum("nhd,ld->nhl", q[b * N:(b + 1) * N].double().view(N, nh, DK), c) * SCALE
        s = s.masked_fill((torch.arange(L)[None, :] > lim[:, None])[:, None, :], float("-inf"))
        o[b * N:(b + 1) * N] = torch.einsum("nhl,ld->nhd", torch.softmax(s, dim=2), c[:, :RANK])
        vmax[b * N:(b + 1) * N, 0] = c[:, :RANK].abs().amax(dim=1).cummax(dim=0)[0][lim]
    return q, o.reshape(B * N, nh * RANK), vmax


def _check(out, ref, vmax, what):
    assert torch.isfinite(out).all(), what
    worst = ((out.double().cpu() - ref).abs() / (2.0 ** -9 * vmax)).max().item()
    print(f"{what}: max error = {worst:.3f} of the 2^-9 Vmax bound")
    assert worst <= 1.0, what


def _call(rows, lens, q, N, nh, ws=None):
    """rows: fp16 (B, cap, 576) on the CPU."""
    B, cap, dv = rows.shape[0], rows.shape[1], _dev()
    if ws is None:
        ws = torch.empty(kl.mla_workspace_size(B, N, nh), dtype=torch.uint8, device=dv)
    return kl.mla_decode(q.to(dv), rows.to(dv), (2 * DK, cap * 2 * DK), torch.tensor(lens, dtype=torch.int32, device=dv), cap, B, N,
                         nh, ws, SCALE)


def _lens(N, nh):
    """The edges of a tile, the lengths at which a workgroup's share goes from empty to one tile, the capacity."""
    tile, _, W = kl.mla_plan(12, N, nh)
    cap = 13 * tile + 3
    return (N, 31, 32, 33, tile - 1, tile + 1, 2 * tile, 2 * tile + 1, min(W * tile - 1, cap), min(W * tile + 1, cap), cap - 1, cap)


@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("nh", [16, 20, 128])  # one live tile of a group; a partly filled second; two to eight groups
def test_mla_decode_matches_the_formula(nh, N, tune):
    lens = _lens(N, nh)
    q, ref, vmax = _ref(lens, N, nh)
    for pin in (0, 1):
        tune(GQ_ATTN_W=pin)
        _check(_call(_cache(12, max(lens)), lens, q, N, nh), ref, vmax, f"heads {nh} N={N} W={pin or kl.mla_plan(12, N, nh)[2]}")


def test_new_tokens_are_causal_among_themselves():
    nh, cap, L = 20, 100, 70
    rows, q = _cache(1, cap, 3), _randn(4, nh * DK, seed=7)
    ref, vmax = _ref_at(rows, q, L, nh)
    _check(_call(rows, [L], q, 4, nh), ref, vmax, "one call of four tokens")
    for i in range(4):
        _check(_call(rows, [L - 3 + i], q[i:i + 1], 1, nh), ref[i:i + 1], vmax[i:i + 1], f"token {i} alone")


def _ref_at(rows, q, L, nh):
    """(o, Vmax) of the four tokens that end a sequence of length L, from the formula token by token."""
    C, o, vm = rows[0].double(), [], []
    for i in range(4):
        c = C[:L - 3 + i]
        p = torch.softmax(q[i].double().view(nh, DK) @ c.T * SCALE, dim=1)
        o.append((p @ c[:, :RANK]).reshape(1, -1)), vm.append(c[:, :RANK].abs().max().reshape(1, 1))
    return torch.cat(o), torch.cat(vm)


def test_dead_bytes_and_other_sequences_change_no_bit():
    nh, N, dv = 16, 4, _dev()
    lens = _lens(N, nh)
    q, ref, vmax = _ref(lens, N, nh)
    rows = _cache(12, max(lens))
    clean = _call(rows, lens, q, N, nh)
    _check(clean, ref, vmax, "clean")
    dirty = rows.clone()
    for b, L in enumerate(lens):  # every row at or beyond its sequence's length: NaN; the workspace too
        dirty[b, L:] = float("nan")
    ws = torch.full((kl.mla_workspace_size(12, N, nh) // 4,), float("nan"), dtype=torch.float32, device=dv).view(torch.uint8)
    assert torch.equal(_call(dirty, lens, q, N, nh, ws).view(torch.int16), clean.view(torch.int16))
    other, q2 = _cache(12, max(lens), 1).clone(), _randn(12 * N, nh * DK, seed=8)
    for b in (3, 11):  # sequence b among eleven other sequences of other lengths
        lens2 = [lens[b] if i == b else lens[(i + 5) % 12] for i in range(12)]
        other[b], q2[b * N:(b + 1) * N] = rows[b], q[b * N:(b + 1) * N]
        got = _call(other, lens2, q2, N, nh)
        assert torch.equal(got[b * N:(b + 1) * N].view(torch.int16), clean[b * N:(b + 1) * N].view(torch.int16)), b


def _rope64(x, pos, inv_freq, mode, m):
    """x float64 (T, heads, 64), pos (T) -> (exact rotation, gq_rope_append's bound without a norm)."""
    th = torch.tensor(pos, dtype=torch.float64)[:, None, None] * inv_freq.double()
    c, s = m * torch.cos(th), m * torch.sin(th)
    i0 = torch.arange(0, ROPE, 2) if mode == "norm" else torch.arange(ROPE // 2)
    i1 = i0 + 1 if mode == "norm" else i0 + ROPE // 2
    out, mag = x.clone(), x.clone()
    out[..., i0], out[..., i1] = x[..., i0] * c - x[..., i1] * s, x[..., i0] * s + x[..., i1] * c
    mag[..., i0] = mag[..., i1] = m * (x[..., i0].abs() + x[..., i1].abs())
    return out, 2.0 ** -11 * out.abs() + 2.0 ** -25 + 2.0 ** -19 * mag


@pytest.mark.parametrize("mode", ["norm", "neox"])
@pytest.mark.parametrize("nh", [16, 128])
@pytest.mark.parametrize("N", [1, 4])
def test_mla_append_matches_the_formula_and_writes_nothing_else(N, nh, mode):
    B, cap, dv, m, eps = 3, 131072, _dev(), 1.25, 1e-6
    lens = [N, 70, cap]  # positions 0 .. N - 1, some in the middle, and up to 131071
    pos = [L - N + i for L in lens for i in range(N)]
    kv, q = _randn(B * N, DK, seed=1), _randn(B * N, nh * 192, seed=2)
    w = 1 + 0.1 * torch.randn(RANK, generator=torch.Generator().manual_seed(3))
    inv_freq = torch.from_numpy(RoPE.table(ROPE)[0]).float()
    cache = torch.full((B, cap, 2 * DK), 0xA5, dtype=torch.uint8, device=dv)
    qout = torch.full((B * N, nh * DK), -7.0, dtype=torch.float16, device=dv)
    kvd, qd = kv.to(dv), q.to(dv)
    kl.mla_append(mode, kvd[:, :RANK], kvd[:, RANK:], qd[:, 128:], 192, qout, cache, (2 * DK, cap * 2 * DK),
                  torch.tensor(lens, dtype=torch.int32, device=dv), cap, inv_freq.to(dv), m, w.to(dv), eps, B, N, nh)
    rows = torch.stack([cache[b, L - N:L] for b, L in enumerate(lens)]).view(torch.float16).reshape(B * N, DK).double().cpu()
    x = kv[:, :RANK].double()
    y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w.double()
    worst = {"c_kv": ((rows[:, :RANK] - y).abs() / (2.0 ** -11 * y.abs() + 2.0 ** -25 + 2.0 ** -16 * y.abs())).max().item()}
    k_exact, k_bound = _rope64(kv[:, None, RANK:].double(), pos, inv_freq, mode, m)
    worst["k_pe"] = ((rows[:, None, RANK:] - k_exact).abs() / k_bound).max().item()
    q_exact, q_bound = _rope64(q.double().view(B * N, nh, 192)[:, :, 128:], pos, inv_freq, mode, m)
    got = qout.view(B * N, nh, DK)
    worst["q_pe"] = ((got[:, :, RANK:].double().cpu() - q_exact).abs() / q_bound).max().item()
    print(f"N={N} heads {nh} {mode}: max error / bound = {worst}")
    assert max(worst.values()) <= 1.0, worst
    assert (got[:, :, :RANK] == -7.0).all()
    for b, L in enumerate(lens):  # nothing but the N rows of each sequence was written
        cache[b, L - N:L] = 0xA5
    assert (cache == 0xA5).all()


def test_the_layer_is_the_unabsorbed_attention():
    """MLAttention.forward on a V2-Lite-shaped layer (16 heads, 128 + 64 / 128) against the un-absorbed float64
    attention: keys [W_UK c | k_pe] of 192, values W_UV c of 128.  The tolerance is twice the error that the
    implementation's fp16 roundings (cache row, rotated q_pe, the absorbed q, the latent output, the result)
    cause in the same float64 formula.  Measured on an MI355X: max error 1.53e-3, the roundings alone 1.51e-3."""
    B, H, P, N, dv = 2, 16, 70, 2, _dev()
    f, m = RoPE.table(ROPE)
    k_b, v_b = _randn(H, RANK, 128, seed=20) * 128 ** -0.5, _randn(H, 128, RANK, seed=21) * RANK ** -0.5
    w = 1 + 0.1 * torch.randn(RANK, generator=torch.Generator().manual_seed(22))
    layer = MLAttention(k_b.to(dv), v_b.to(dv), w.to(dv), RoPE(torch.from_numpy(f).float().to(dv), ROPE, "norm", m), 1e-6)
    cache = layer.new_cache(B, P + N, dv)
    q, kv = [_randn(B * n, H * 192, seed=23 + n) for n in (P, N)], [_randn(B * n, DK, seed=33 + n) for n in (P, N)]
    cache.append(kv[0][:, :RANK].to(dv), kv[0][:, RANK:].to(dv), q[0].to(dv), layer.rope, layer.norm_w, 1e-6)  # the prefix
    out = layer.forward(q[1].to(dv), kv[1].to(dv)).double().cpu()
    assert cache.kv_len.tolist() == [P + N] * B and out.shape == (B * N, H * 128)

    h16 = lambda t: t.to(torch.float16).double()  # noqa: E731
    inv_freq, kb, vb = layer.rope.inv_freq.cpu(), k_b.to(torch.float16).double(), v_b.to(torch.float16).double()
    exact, rounded = torch.zeros(B * N, H, 128, dtype=torch.float64), torch.zeros(B * N, H, 128, dtype=torch.float64)
    for b in range(B):
        rows = torch.cat([kv[0][b * P:(b + 1) * P], kv[1][b * N:(b + 1) * N]]).double()
        c = rows[:, :RANK] * torch.rsqrt((rows[:, :RANK] ** 2).mean(-1, keepdim=True) + 1e-6) * w.double()
        kpe = _rope64(rows[:, None, RANK:], list(range(P + N)), inv_freq, "norm", m)[0][:, 0]
        for i in range(N):
            L, qi = P + i + 1, q[1][b * N + i].double().view(H, 192)
            qpe = _rope64(qi[None, :, 128:], [L - 1], inv_freq, "norm", m)[0][0]
            # un-absorbed, nothing rounded: k = [W_UK c | k_pe] per head, v = W_UV c
            k = torch.cat([torch.einsum("hrd,lr->lhd", kb, c[:L]), kpe[:L, None, :].expand(L, H, ROPE)], dim=2)
            p = torch.softmax(torch.einsum("hd,lhd->hl", torch.cat([qi[:, :128], qpe], dim=1), k) * layer.scale, dim=1)
            exact[b * N + i] = torch.einsum("hl,lhv->hv", p, torch.einsum("hvr,lr->lhv", vb, c[:L]))
            # the same numbers with the implementation's fp16 roundings
            c16, q_abs = h16(c[:L]), h16(torch.einsum("hrd,hd->hr", kb, qi[:, :128]))
            p = torch.softmax((q_abs @ c16.T + h16(qpe) @ h16(kpe[:L]).T) * layer.scale, dim=1)
            rounded[b * N + i] = h16(torch.einsum("hvr,hr->hv", vb, h16(p @ c16)))
    own = (rounded - exact).abs().max().item()
    err = (out.view(B * N, H, 128) - exact).abs().max().item()
    print(f"layer: max |out - exact| = {err:.3e}, the fp16 roundings alone = {own:.3e} (tolerance 2x)")
    assert err <= 2 * own
