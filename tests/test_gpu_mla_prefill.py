"""gq_mla_prefill on the GPU (MLACache.attend beyond four new tokens) against the plain formula in float64
torch on the CPU, test_gpu_mla.py's reference and bound: every output element within 2^-9 * Vmax, Vmax the
largest |c_kv| among the positions the row attends (derived for this arithmetic, not measured).  The tile
length and the rows of a workgroup come from the library (gq_debug_mla_prefill_plan)."""
import pytest
import torch

import kernels._lib as kl
from gpu_types import dev as _dev
from kernels import MLACache, MLAttention, RoPE
from test_gpu_mla import DK, RANK, ROPE, SCALE, _cache, _check, _randn, _ref, _rope64
from test_gpu_mla import _call as _decode

pytestmark = pytest.mark.gpu


def _call(rows, lens, q, N, nh):
    """rows: fp16 (B, cap, 576) on the CPU."""
    B, cap, dv = rows.shape[0], rows.shape[1], _dev()
    return kl.mla_prefill(q.to(dv), rows.to(dv), (2 * DK, cap * 2 * DK), torch.tensor(lens, dtype=torch.int32, device=dv), cap, B, N,
                          nh, SCALE)


def _lens(N, nh):
    """Twelve lengths: the empty prefix, the edges of a tile, the lengths at which the last row of the first and
    of a middle row block attends exactly a whole number of tiles and one key more, the capacity.  (A length
    below N is no call: those are raised to N.)"""
    tile, rows, _ = kl.mla_prefill_plan(12, N, nh)
    edges = []
    for blk in (0, (N * nh + rows - 1) // rows // 2):
        tok = (min((blk + 1) * rows, N * nh) - 1) // nh  # the block's last row's token: it attends L - N + tok + 1 keys
        edges += [N + 2 * tile - tok - 1, N + 2 * tile - tok]
    return tuple(max(L, N) for L in (N, N + 1, tile - 1, tile, tile + 1, 2 * tile + 1, 3 * tile, *edges, 5 * tile + 3))


@pytest.mark.parametrize("N", [5, 13, 40])      # decode's first refusal; 260 rows at 20 heads; several blocks at 16 heads
@pytest.mark.parametrize("nh", [16, 20, 128])   # several tokens a block; block edges inside a token; whole blocks a token
def test_mla_prefill_matches_the_formula(nh, N):
    lens = _lens(N, nh)
    q, ref, vmax = _ref(lens, N, nh)
    _check(_call(_cache(12, max(lens)), lens, q, N, nh), ref, vmax, f"prefill heads {nh} N={N}")


def test_new_tokens_are_causal_as_at_decode():
    nh, cap, L, N = 20, 100, 70, 9
    rows, q = _cache(1, cap, 3), _randn(N, nh * DK, seed=7)
    C, o, vm = rows[0].double(), [], []
    for i in range(N):  # each token's own prefix, alone
        c = C[:L - N + 1 + i]
        p = torch.softmax(q[i].double().view(nh, DK) @ c.T * SCALE, dim=1)
        o.append((p @ c[:, :RANK]).reshape(1, -1)), vm.append(c[:, :RANK].abs().max().reshape(1, 1))
    ref, vmax = torch.cat(o), torch.cat(vm)
    _check(_call(rows, [L], q, N, nh), ref, vmax, "one call of nine tokens")
    for i in range(N):
        _check(_decode(rows, [L - N + 1 + i], q[i:i + 1], 1, nh), ref[i:i + 1], vmax[i:i + 1], f"token {i} alone, at decode")


def test_dead_bytes_and_other_sequences_change_no_bit():
    nh, N = 16, 13
    lens = _lens(N, nh)
    q, ref, vmax = _ref(lens, N, nh)
    rows = _cache(12, max(lens))
    clean = _call(rows, lens, q, N, nh)
    _check(clean, ref, vmax, "clean")
    dirty = rows.clone()
    for b, L in enumerate(lens):  # every row at or beyond its sequence's length: NaN
        dirty[b, L:] = float("nan")
    assert torch.equal(_call(dirty, lens, q, N, nh).view(torch.int16), clean.view(torch.int16))
    other, q2 = _cache(12, max(lens), 1).clone(), _randn(12 * N, nh * DK, seed=8)
    for b in (3, 11):  # sequence b among eleven other sequences of other lengths
        lens2 = [lens[b] if i == b else lens[(i + 5) % 12] for i in range(12)]
        other[b], q2[b * N:(b + 1) * N] = rows[b], q[b * N:(b + 1) * N]
        got = _call(other, lens2, q2, N, nh)
        assert torch.equal(got[b * N:(b + 1) * N].view(torch.int16), clean[b * N:(b + 1) * N].view(torch.int16)), b


def test_the_layer_serves_a_chunk_after_a_prefix():
    """MLAttention.forward with 24 new tokens after a 70-token prefix on test_the_layer_is_the_unabsorbed_attention's
    V2-Lite shape, against the un-absorbed float64 attention; that test's rule: the tolerance is twice the error the
    implementation's fp16 roundings cause in the same float64 formula, measured here the same way."""
    B, H, P, N, dv = 2, 16, 70, 24, _dev()
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
            k = torch.cat([torch.einsum("hrd,lr->lhd", kb, c[:L]), kpe[:L, None, :].expand(L, H, ROPE)], dim=2)
            p = torch.softmax(torch.einsum("hd,lhd->hl", torch.cat([qi[:, :128], qpe], dim=1), k) * layer.scale, dim=1)
            exact[b * N + i] = torch.einsum("hl,lhv->hv", p, torch.einsum("hvr,lr->lhv", vb, c[:L]))
            c16, q_abs = h16(c[:L]), h16(torch.einsum("hrd,hd->hr", kb, qi[:, :128]))
            p = torch.softmax((q_abs @ c16.T + h16(qpe) @ h16(kpe[:L]).T) * layer.scale, dim=1)
            rounded[b * N + i] = h16(torch.einsum("hvr,hr->hv", vb, h16(p @ c16)))
    own = (rounded - exact).abs().max().item()
    err = (out.view(B * N, H, 128) - exact).abs().max().item()
    print(f"layer, 24 tokens: max |out - exact| = {err:.3e}, the fp16 roundings alone = {own:.3e} (tolerance 2x)")
    assert err <= 2 * own


def test_attend_routes_four_tokens_to_decode_and_five_to_prefill():
    B, cap, nh, dv = 2, 40, 16, _dev()
    f, m = RoPE.table(ROPE)
    rope, w = RoPE(torch.from_numpy(f).float().to(dv), ROPE, "norm", m), torch.ones(RANK, device=dv)
    cache = MLACache(B, cap, device=dv)
    for N, direct in ((4, kl.mla_decode), (5, kl.mla_prefill)):
        kv, q = _randn(B * N, DK, seed=40 + N).to(dv), _randn(B * N, nh * 192, seed=50 + N).to(dv)
        qbuf = cache.append(kv[:, :RANK], kv[:, RANK:], q, rope, w)
        qbuf.view(B * N, nh, DK)[:, :, :RANK] = _randn(B * N, nh, RANK, seed=60 + N).to(dv)
        got, ws = cache.attend(qbuf, SCALE).clone(), cache._for(N, nh)[1]
        assert (ws is None) == (N == 5)  # no workspace on the prefill route
        args = (qbuf, cache.c, cache.strides, cache.kv_len, cap, B, N, nh) + ((ws,) if N == 4 else ())
        assert torch.equal(got.view(torch.int16), direct(*args, SCALE).view(torch.int16)), N
