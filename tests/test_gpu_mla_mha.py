"""The un-absorbed MLA prompt pass on the GPU (gq_mla_kv_expand, gq_mla_prefill_mha; MLAttention(unabsorbed_from=n))
against float64 torch on the CPU over the same fp16 inputs.  The expansion is held to gq_mla_proj's bound with Kc =
512, |y - exact| <= 2^-11 |exact| + 2^-25 + 512 2^-23 sum_c |x_c w_c|; every attention output to |o - exact| <=
2^-9 max|v| over the positions its row attends (the fp16 prefill path's bound: P rounded to fp16, the final
rounding, fp32 summation order with exp2).  Buffers have rows longer than their width; KV is pre-filled with 0xA5."""
import functools

import pytest
import torch

import kernels._lib as kl
from gpu_types import dev as _dev
from kernels import MLAttention, RoPE
from test_gpu_mla import DK, RANK, ROPE, SCALE, _randn, _rope64

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5A5 - 65536
CAP, KVCAP, LENS0, N2 = 140, 136, (63, 131), 7  # the expansion's cache: two calls, lengths LENS0 and LENS0 + N2


@functools.lru_cache(maxsize=None)
def _expansion(nh):
    """(C fp16 (2, CAP, 576), W fp16 (nh, 256, 512), exact float64 (2, CAP, nh*256), the bound)."""
    C, W = _randn(2, CAP, DK, seed=1), _randn(nh, 256, RANK, seed=2) * RANK ** -0.5
    x, w = C[:, :, :RANK].double(), W.double()
    exact, mag = torch.einsum("bpc,hmc->bphm", x, w), torch.einsum("bpc,hmc->bphm", x.abs(), w.abs())
    return C, W, exact.flatten(2), (2.0 ** -11 * exact.abs() + 2.0 ** -25 + RANK * 2.0 ** -23 * mag).flatten(2)


@pytest.mark.parametrize("N", [1, 17, 65])  # one row of a tile; a partly filled second tile; a second block, negative positions
@pytest.mark.parametrize("nh", [1, 3, 16])
@pytest.mark.parametrize("cus", [0, 4])  # the chip's units: a head per 64-token workgroup; 4: 128-token blocks, 16 heads in ranges of 4
def test_kv_expand_matches_the_formula_and_writes_nothing_else(nh, N, cus, tune):
    tune(GQ_CUS=cus)
    C, W, exact, bound = _expansion(nh)
    dv, width = _dev(), nh * 256
    store = torch.full((2, KVCAP, width + 8), SENTINEL, dtype=torch.int16, device=dv)
    kv = store.view(torch.float16)[:, :, :width]
    written = torch.zeros(2, KVCAP, dtype=torch.bool)
    for lens, n in ((LENS0, N), (tuple(L + N2 for L in LENS0), N2)):  # the second call extends what the first left
        before = kv.cpu()
        kl.mla_kv_expand(W.to(dv), C.to(dv), (2 * DK, CAP * 2 * DK), torch.tensor(lens, dtype=torch.int32, device=dv), CAP, kv, 2, n, nh)
        new = torch.zeros(2, KVCAP, dtype=torch.bool)
        for b, L in enumerate(lens):
            new[b, max(L - n, 0):min(L, KVCAP)] = True  # (63 < 65: negative positions; 138 > KVCAP: positions beyond the buffer)
        got = kv.cpu()
        worst = ((got.double() - exact[:, :KVCAP]).abs() / bound[:, :KVCAP])[new].max().item()
        print(f"heads {nh} N={n}: max error = {worst:.3f} of the bound")
        assert worst <= 1.0
        assert torch.equal(got.view(torch.int16)[~new], before.view(torch.int16)[~new])  # the first call's rows, the sentinel
        written |= new
    assert (kv.cpu().view(torch.int16)[~written] == SENTINEL).all() and (store[:, :, width:] == SENTINEL).all()
    assert written.sum() == sum(min(L + N2, KVCAP) - max(L - N, 0) for L in LENS0)


def _lens(N):
    """No prefix; a prefix ending on a 64-key tile edge and one past it; the last row on a tile edge; a few hundred."""
    return (N, 64 + N, 65 + N, 192, 300 + N)


@functools.lru_cache(maxsize=None)
def _attention(nh, N, seed=0):
    """(C (B, cap, 576), KV (B, cap, nh*256), qn storage (B*N, nh*192), qp storage (B*N, nh*576), exact float64 (B*N, nh*128), vmax)."""
    lens = _lens(N)
    B, cap = len(lens), max(lens) + 2
    C, KV = _randn(B, cap, DK, seed=seed + 3), _randn(B, cap, nh * 256, seed=seed + 4)
    qn, qp = _randn(B * N, nh * 192, seed=seed + 5), _randn(B * N, nh * DK, seed=seed + 6)
    q = torch.cat([qn.view(-1, nh, 192)[:, :, :128], qp.view(-1, nh, DK)[:, :, RANK:]], dim=2).double()
    exact, vmax = torch.zeros(B * N, nh, 128, dtype=torch.float64), torch.zeros(B * N, nh, 1, dtype=torch.float64)
    for b, L in enumerate(lens):
        kv, lim = KV[b, :L].double().view(L, nh, 256), L - N + torch.arange(N)
        k = torch.cat([kv[:, :, :128], C[b, :L, None, RANK:].double().expand(L, nh, ROPE)], dim=2)
        s = torch.einsum("nhd,lhd->nhl", q[b * N:(b + 1) * N], k) * SCALE
        s = s.masked_fill((torch.arange(L)[None, :] > lim[:, None])[:, None, :], float("-inf"))
        exact[b * N:(b + 1) * N] = torch.einsum("nhl,lhd->nhd", torch.softmax(s, dim=2), kv[:, :, 128:])
        vmax[b * N:(b + 1) * N, :, 0] = kv[:, :, 128:].abs().amax(dim=2).cummax(dim=0)[0][lim]
    return C, KV, qn, qp, exact, vmax


def _attend(C, KV, qn, qp, lens, N, nh):
    """fp16 (B*N, nh*128) on the CPU; the q views are the layer's: q_nope in 192-wide heads, q_pe from column 512 of 576-wide ones."""
    dv, B, cap = _dev(), C.shape[0], C.shape[1]
    out = kl.mla_prefill_mha(qn.to(dv), 192, qp.to(dv)[:, RANK:], DK, KV.to(dv), C.to(dv), (2 * DK, cap * 2 * DK),
                             torch.tensor(lens, dtype=torch.int32, device=dv), cap, B, N, nh, SCALE)
    return out.cpu()


@pytest.mark.parametrize("N", [5, 65, 130])  # a padded tile; a second 64-row block of one row; two 128-row blocks or three of 64
@pytest.mark.parametrize("nh", [1, 3, 16])
@pytest.mark.parametrize("cus", [0, 4])  # the chip's units: 64-row workgroups at these sizes; 4: 128-row ones, two tiles a wave
def test_prefill_mha_matches_the_formula(nh, N, cus, tune):
    tune(GQ_CUS=cus)
    assert kl.mla_prefill_mha_plan(len(_lens(N)), N, nh)[0] == (128 if cus else 64)
    C, KV, qn, qp, exact, vmax = _attention(nh, N)
    out = _attend(C, KV, qn, qp, _lens(N), N, nh)
    assert torch.isfinite(out).all()
    worst = ((out.double().view(-1, nh, 128) - exact).abs() / (2.0 ** -9 * vmax)).max().item()
    print(f"heads {nh} N={N} rows {kl.mla_prefill_mha_plan(len(_lens(N)), N, nh)[0]}: max error = {worst:.3f} of the 2^-9 max|v| bound")
    assert worst <= 1.0


@pytest.mark.parametrize("nh,N,cus", [(3, 65, 0), (16, 130, 4)])
def test_dead_positions_and_other_sequences_change_no_bit(nh, N, cus, tune):
    tune(GQ_CUS=cus)
    C, KV, qn, qp, _, _ = _attention(nh, N)
    lens, nan = _lens(N), float("nan")
    clean = _attend(C, KV, qn, qp, lens, N, nh).view(len(lens), N, -1).view(torch.int16)
    Cd, KVd = C.clone(), KV.clone()
    for b, L in enumerate(lens):
        Cd[b, L:], KVd[b, L:] = nan, nan
    assert torch.equal(_attend(Cd, KVd, qn, qp, lens, N, nh).view(torch.int16).view(clean.shape), clean)
    b = 2  # every other sequence NaN throughout, then the sequence alone
    others = [x.clone() for x in (C, KV, qn.view(len(lens), N, -1), qp.view(len(lens), N, -1))]
    for x in others:
        x[:b], x[b + 1:] = nan, nan
    got = _attend(others[0], others[1], others[2].view(qn.shape), others[3].view(qp.shape), lens, N, nh)
    assert torch.equal(got.view(torch.int16).view(clean.shape)[b], clean[b])
    alone = _attend(C[b:b + 1], KV[b:b + 1], qn[b * N:(b + 1) * N], qp[b * N:(b + 1) * N], lens[b:b + 1], N, nh)
    assert torch.equal(alone.view(torch.int16), clean[b])
    # a length below N: the rows without a position are zeros
    short = _attend(C[b:b + 1], KV[b:b + 1], qn[b * N:(b + 1) * N], qp[b * N:(b + 1) * N], (N - 3,), N, nh)
    assert (short[:3] == 0).all() and torch.isfinite(short).all() and (short[3:] != 0).any()


@pytest.mark.parametrize("P,N", [(70, 24), (0, 65)])  # a chunk after a prefix that was only appended; a fresh prompt of two blocks
def test_the_unabsorbed_layer_is_the_unabsorbed_attention(P, N):
    """MLAttention(unabsorbed_from=5).forward on test_the_fused_layer_is_the_unabsorbed_attention's shape and by its
    criterion: twice the error the path's own fp16 roundings (the cache row, k_nope, v, the rotated q_pe and k_pe, the
    output) cause in the same float64 formula.  unabsorbed_from=0 returns the bits of the absorbed launches made by hand."""
    B, H, dv = 2, 16, _dev()
    f, m = RoPE.table(ROPE)
    k_b, v_b = _randn(H, RANK, 128, seed=20) * 128 ** -0.5, _randn(H, 128, RANK, seed=21) * RANK ** -0.5
    w = 1 + 0.1 * torch.randn(RANK, generator=torch.Generator().manual_seed(22))
    rope = RoPE(torch.from_numpy(f).float().to(dv), ROPE, "norm", m)
    q, kv = [_randn(B * n, H * 192, seed=23 + n) for n in (P, N)], [_randn(B * n, DK, seed=33 + n) for n in (P, N)]

    def run(**kw):
        layer = MLAttention(k_b.to(dv), v_b.to(dv), w.to(dv), rope, 1e-6, fused=True, **kw)
        cache = layer.new_cache(B, P + N, dv)
        if P:
            cache.append(kv[0][:, :RANK].to(dv), kv[0][:, RANK:].to(dv), q[0].to(dv), rope, layer.norm_w, 1e-6)
        return layer, cache, layer.forward(q[1].to(dv), kv[1].to(dv))

    layer, cache, out = run(unabsorbed_from=5)
    assert cache.kv_len.tolist() == [P + N] * B and out.shape == (B * N, H * 128) and cache.expanded == P + N
    _, c0, out0 = run()
    qbuf = c0._for(N, H)[0]  # (append left q_pe there; the absorbed pass by hand over the same cache)
    kl.mla_proj(0, layer.k_b, q[1].to(dv), 192, qbuf, DK, B * N, H)
    o = kl.mla_prefill(qbuf, c0.c, c0.strides, c0.kv_len, c0.capacity, B, N, H, layer.scale)
    hand = kl.mla_proj(1, layer.v_b, o, RANK, torch.empty_like(out0), 128, B * N, H)
    assert c0.kv is None and torch.equal(out0.view(torch.int16), hand.view(torch.int16))

    h16 = lambda t: t.to(torch.float16).double()  # noqa: E731
    inv_freq, kb, vb = rope.inv_freq.cpu(), k_b.to(torch.float16).double(), v_b.to(torch.float16).double()
    exact, rounded = torch.zeros(B * N, H, 128, dtype=torch.float64), torch.zeros(B * N, H, 128, dtype=torch.float64)
    for b in range(B):
        rows = torch.cat([kv[0][b * P:(b + 1) * P], kv[1][b * N:(b + 1) * N]]).double()
        c = rows[:, :RANK] * torch.rsqrt((rows[:, :RANK] ** 2).mean(-1, keepdim=True) + 1e-6) * w.double()
        kpe = _rope64(rows[:, None, RANK:], list(range(P + N)), inv_freq, "norm", m)[0][:, 0]
        qb = q[1][b * N:(b + 1) * N].double().view(N, H, 192)
        qpe = _rope64(qb[:, :, 128:], list(range(P, P + N)), inv_freq, "norm", m)[0]
        mask = torch.arange(P + N)[None, :] > P + torch.arange(N)[:, None]
        # nothing rounded, then the same numbers from the path's fp16 intermediates
        for dst, cc, r in ((exact, c, lambda t: t), (rounded, h16(c), h16)):
            kn, v = r(torch.einsum("hrd,lr->lhd", kb, cc)), r(torch.einsum("hvr,lr->lhv", vb, cc))
            s = (torch.einsum("nhd,lhd->nhl", qb[:, :, :128], kn) + torch.einsum("nhd,ld->nhl", r(qpe), r(kpe))) * layer.scale
            p = torch.softmax(s.masked_fill(mask[:, None, :], float("-inf")), dim=2)
            dst[b * N:(b + 1) * N] = r(torch.einsum("nhl,lhv->nhv", p, v))
    own = (rounded - exact).abs().max().item()
    err = (out.double().cpu().view(B * N, H, 128) - exact).abs().max().item()
    print(f"un-absorbed layer, P={P} N={N}: max |out - exact| = {err:.3e}, the fp16 roundings alone = {own:.3e} (tolerance 2x)")
    assert err <= 2 * own
