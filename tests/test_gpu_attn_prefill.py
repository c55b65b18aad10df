"""Prefill attention on the GPU (gq_attn_prefill; KVCache.attend beyond 32 rows per kv head) against the
plain formula in float64 torch on the CPU over the dequantized cache.  The arithmetic is decode
attention's, so every output element is held to the same derived bound |o - ref| <= 2^-9 * Vmax, Vmax
the largest |v| among the positions the query attends in its kv head (tests/test_gpu_attn.py).
The rows per workgroup and the keys per tile come from the library (gq_debug_attn_prefill_plan)."""
import numpy as np
import pytest
import torch

import kernels._lib as kl
from gpu_types import dev as _dev
from test_gpu_attn import NAN16, _cache, _q  # the decode tests' random caches (bytes + float64) and queries

pytestmark = pytest.mark.gpu


def _ref(q, Kd, Vd, lens, N, nh, scale):
    """(o float64 (B*N, nh*D), Vmax (B*N, nh)) of the formula; lens include the N new tokens.  A token
    with no position to attend gives zeros."""
    B, _, kvh, D = Kd.shape
    o, vmax = torch.zeros(B * N, nh, D, dtype=torch.float64), torch.zeros(B * N, nh, dtype=torch.float64)
    for b in range(B):
        k, v = (t[b].repeat_interleave(nh // kvh, dim=1) for t in (Kd, Vd))              # (cap, nh, D)
        for i in range(max(0, N - lens[b]), N):
            L = lens[b] - N + i + 1
            p = torch.softmax(torch.einsum("lhd,hd->hl", k[:L], q[b * N + i].double().view(nh, D)) * scale, dim=1)
            o[b * N + i], vmax[b * N + i] = torch.einsum("hl,lhd->hd", p, v[:L]), v[:L].abs().amax(dim=(0, 2))
    return o.reshape(B * N, nh * D), vmax


def _check(out, ref, vmax, what):
    nh = vmax.shape[1]
    err = (out.double().cpu() - ref).abs().view(ref.shape[0], nh, -1)
    assert torch.isfinite(out).all(), what
    dead = vmax == 0  # no position attended: exactly zero
    assert (out.cpu().reshape(ref.shape[0], nh, -1)[dead] == 0).all(), what
    worst = (err / (2.0 ** -9 * vmax[..., None]))[~dead].max().item()
    print(f"{what}: max error = {worst:.3f} of the 2^-9 Vmax bound")
    assert worst <= 1.0, what


def _call(kind, rows, lens, q, cap, N, nh, kvh, D, head_major=False, shift=0, out=None):
    """rows: (K bytes, V bytes) (B, cap, kvh, rb) uint8 on the CPU."""
    B, rb = len(lens), rows[0].shape[-1]
    dv = _dev()
    lay = [r.permute(0, 2, 1, 3) if head_major else r for r in rows]
    bufs = [torch.cat([torch.zeros(shift, dtype=torch.uint8), t.contiguous().reshape(-1)]).to(dv) for t in lay]
    strides = (rb, cap * rb, kvh * cap * rb) if head_major else (kvh * rb, rb, cap * kvh * rb)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dv)
    o = kl.attn_prefill(kind, q if q.is_cuda else q.to(dv), bufs[0], bufs[1], strides, kv_len, cap, B, N, nh, kvh, D,
                        out=out, kv_offset=shift)
    return o, (bufs, strides, kv_len)


@pytest.mark.parametrize("blocks", ["rows-1", "rows+1", "2rows+3"])
@pytest.mark.parametrize("nh,kvh", [(4, 4), (8, 2), (7, 1)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", ["f16", "q8_0"])
@pytest.mark.parametrize("cus", [1024, 1])
def test_prefill_matches_the_formula(cus, kind, D, nh, kvh, blocks, tune):
    G = nh // kvh
    tune(GQ_CUS=cus)  # 128 rows per workgroup are planned where they fill the compute units: never / always at these sizes
    rows, tile = kl.attn_prefill_plan(6, 64, nh, kvh, D)
    assert rows == (64 if cus == 1024 else 128)
    target = {"rows-1": rows - 1, "rows+1": rows + 1, "2rows+3": 2 * rows + 3}[blocks]
    N = -(-target // G)
    assert kl.attn_prefill_plan(6, N, nh, kvh, D) == (rows, tile)
    # prefixes at the edges of a tile and over a ring wrap, and one sequence whose first two tokens attend nothing
    lens = [P + N for P in (0, 1, tile - 1, tile, 3 * tile + 5)] + [N - 2]
    cap = max(lens) + 3
    (kb, kd), (vb, vd) = _cache(kind, 6, cap, kvh, D)
    q = _q(6, N, nh, D)
    ref, vmax = _ref(q, kd, vd, lens, N, nh, D ** -0.5)
    assert (vmax[5 * N:5 * N + 2] == 0).all() and (vmax[5 * N + 2:] > 0).all()
    for trv in (1, 0) if kind == "f16" else (1,):  # fp16 V^T by the transposing LDS read (the default), then by the gather
        tune(GQ_ATTN_TRV=trv)
        out, _ = _call(kind, (kb, vb), lens, q, cap, N, nh, kvh, D)
        _check(out, ref, vmax, f"{kind} D={D} heads {nh}/{kvh} N={N} rows={rows} tile={tile} trv={trv}")


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_dead_positions_are_never_used_and_the_length_is_read_on_the_device(kind):
    D, nh, kvh, cap, N, lens = 128, 8, 2, 300, 40, [45, 197, 260]
    (kb, kd), (vb, vd) = _cache(kind, 1, cap, kvh, D, seed=5)
    q, dv = _q(1, N, nh, D), _dev()
    rows = [r.clone() for r in (kb, vb)]
    for r in rows:  # every row at or beyond the shortest length: NaN (Q8_0: NaN in every d)
        r[:, min(lens):] = torch.from_numpy(np.tile(NAN16, r.shape[-1] // 2))
    out, (bufs, strides, kv_len) = _call(kind, rows, [min(lens)], q, cap, N, nh, kvh, D)
    _check(out, *_ref(q, kd, vd, [min(lens)], N, nh, D ** -0.5), f"{kind} NaN beyond the length")
    # the same pointers, only kv_len changed -- eagerly, then as replays of one captured graph
    bufs = [r.reshape(-1).to(dv) for r in (kb, vb)]  # (the whole cache valid again)
    qd, o = q.to(dv), torch.empty(N, nh * D, dtype=torch.float16, device=dv)
    call = lambda: kl.attn_prefill(kind, qd, bufs[0], bufs[1], strides, kv_len, cap, 1, N, nh, kvh, D, out=o)
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


def test_a_sequence_does_not_depend_on_its_batch():
    kind, D, nh, kvh, cap, N, lens = "q8_0", 128, 8, 2, 200, 40, [40, 77, 200]
    (kb, kd), (vb, vd) = _cache(kind, 3, cap, kvh, D, seed=9)
    q = _q(3, N, nh, D)
    three, _ = _call(kind, (kb, vb), lens, q, cap, N, nh, kvh, D)
    for b, L in enumerate(lens):
        one, _ = _call(kind, (kb[b:b + 1], vb[b:b + 1]), [L], q[b * N:(b + 1) * N], cap, N, nh, kvh, D)
        assert torch.equal(one.view(torch.int16), three[b * N:(b + 1) * N].view(torch.int16)), b


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_strides_bases_and_padding(kind):
    D, nh, kvh, cap, N, lens, pad = 64, 7, 1, 90, 12, [90, 37], 24
    (kb, kd), (vb, vd) = _cache(kind, 2, cap, kvh, D, seed=11)
    q, dv = _q(2, N, nh, D), _dev()
    ref = _ref(q, kd, vd, lens, N, nh, D ** -0.5)
    qw = torch.full((2 * N, nh * D + pad), 3.0, dtype=torch.float16, device=dv)
    qw[:, 2:2 + nh * D] = q.to(dv)
    for head_major, shift, at in ((True, 6, 4), (False, 0, 3)):  # (O's slice 8-byte aligned, then not)
        ow = torch.full((2 * N, nh * D + pad), -7.0, dtype=torch.float16, device=dv)
        _call(kind, (kb, vb), lens, qw[:, 2:2 + nh * D], cap, N, nh, kvh, D, head_major, shift, out=ow[:, at:at + nh * D])
        _check(ow[:, at:at + nh * D], *ref, f"{kind} head_major={head_major} shift={shift}")
        assert (ow[:, :at] == -7).all() and (ow[:, at + nh * D:] == -7).all()


@pytest.mark.parametrize("kind", ["f16", "q8_0"])
def test_kvcache_prefill_chunk_then_decode(kind):
    from kernels import KVCache
    B, kvh, nh, D, cap, dv = 2, 2, 8, 128, 70, _dev()
    cache = KVCache(B, cap, kvh, D, kind, dv)
    ks, vs = [], []
    for step, N in enumerate((40, 24, 1)):  # a prompt, a chunk over that prefix (both the prefill path), a decode step
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
