"""The latent projections on the GPU (gq_mla_proj; MLAttention(fused=True)) against a float64 einsum on the CPU over
the same fp16 inputs.  Every element is held to the derived bound
    |y - exact| <= 2^-11 |exact| + 2^-25 + Kc 2^-23 sum_k |x_k w_k|:
the final fp16 rounding, half the smallest subnormal, and twice the textbook bound of a Kc-term fp32 sum in any
order (the fp16 products are exact in fp32).  X and Y use the layer's head strides (192 -> 576, 512 -> 128), rows
longer than their width and a shifted base; Y is pre-filled with 0xA5 bytes."""
import functools

import pytest
import torch

import kernels._lib as kl
from gpu_types import dev as _dev
from kernels import MLAttention, RoPE
from test_gpu_mla import DK, RANK, ROPE, _randn, _rope64

pytestmark = pytest.mark.gpu
SHAPE = {0: (512, 128, 192, 576), 1: (128, 512, 512, 128)}  # dir -> (Mo, Kc, x_head_stride, y_head_stride)


@functools.lru_cache(maxsize=None)
def _problem(dir, nh, T, seed=0):
    """(W, the X storage, exact float64 (T, nh, Mo), the bound) -- X is the storage's (T, nh*xhs) view 8 elements in, rows ldx apart."""
    mo, kc, xhs, _ = SHAPE[dir]
    W, xs = _randn(nh, mo, kc, seed=seed + 1) * kc ** -0.5, _randn(T * (nh * xhs + 24) + 8, seed=seed + 2)
    x = _view(xs, T, nh * xhs, 24, 8).view(T, nh, xhs)[:, :, :kc].double()
    exact, mag = torch.einsum("thk,hmk->thm", x, W.double()), torch.einsum("thk,hmk->thm", x.abs(), W.double().abs())
    return W, xs, exact, 2.0 ** -11 * exact.abs() + 2.0 ** -25 + kc * 2.0 ** -23 * mag


def _view(storage, T, width, pad, shift):
    return storage.as_strided((T, width), (width + pad, 1), shift)


def _run(dir, nh, T, xs, W):
    """-> (Y fp16 (T, nh, Mo) on the CPU, Y's whole storage as int16 with the Mo values of every (t, h) blanked to 0xA5A5)."""
    mo, _, xhs, yhs = SHAPE[dir]
    dv = _dev()
    ys = torch.full((2 * (T * (nh * yhs + 12) + 4),), 0xA5, dtype=torch.uint8, device=dv).view(torch.float16)
    Y = _view(ys, T, nh * yhs, 12, 4)
    kl.mla_proj(dir, W.to(dv), _view(xs.to(dv), T, nh * xhs, 24, 8), xhs, Y, yhs, T, nh)
    got = Y.view(T, nh, yhs)[:, :, :mo].cpu()
    Y.view(T, nh, yhs)[:, :, :mo] = torch.tensor(0xA5A5 - 65536, dtype=torch.int16).view(torch.float16).item()
    return got, ys.view(torch.int16).cpu()


@pytest.mark.parametrize("T", [1, 4, 16, 17, 65])  # a padded tile, a full one, one row past it, a partly filled second block
@pytest.mark.parametrize("nh", [1, 20, 128])
@pytest.mark.parametrize("dir", [0, 1])
def test_mla_proj_matches_the_formula(dir, nh, T):
    W, xs, exact, bound = _problem(dir, nh, T)
    got = _run(dir, nh, T, xs, W)[0]
    assert torch.isfinite(got).all()
    worst = ((got.double() - exact).abs() / bound).max().item()
    print(f"dir {dir} heads {nh} T={T} form {kl.mla_proj_plan(dir, T, nh)[0]}: max error = {worst:.3f} of the bound")
    assert worst <= 1.0
    assert kl.mla_proj_plan(dir, T, nh)[:2] == ((0, 16) if T <= 16 else (1, 64))  # the T above reach both forms


@pytest.mark.parametrize("T", [4, 65])
@pytest.mark.parametrize("dir", [0, 1])
def test_nothing_else_is_written(dir, T):
    W, xs, _, _ = _problem(dir, 20, T)
    rest = _run(dir, 20, T, xs, W)[1]
    assert (rest == 0xA5A5 - 65536).all()  # q_pe's columns 512..575, the padding past the width, before and after


@pytest.mark.parametrize("T", [16, 65])
@pytest.mark.parametrize("dir", [0, 1])
def test_a_row_is_its_own(dir, T):
    nh, i = 20, T // 2
    W, xs, _, _ = _problem(dir, nh, T)
    other = _problem(dir, nh, T, seed=10)[1].clone()
    ldx = nh * SHAPE[dir][2] + 24
    other[8 + i * ldx:8 + (i + 1) * ldx] = xs[8 + i * ldx:8 + (i + 1) * ldx]
    a, b = _run(dir, nh, T, xs, W)[0], _run(dir, nh, T, other, W)[0]
    assert torch.equal(a[i].view(torch.int16), b[i].view(torch.int16)) and not torch.equal(a[i - 1], b[i - 1])


@pytest.mark.parametrize("N", [2, 24])  # T = 4: the few-row form and gq_mla_decode; T = 48: the tiled form and gq_mla_prefill
def test_the_fused_layer_is_the_unabsorbed_attention(N):
    """MLAttention(fused=True).forward on test_the_layer_is_the_unabsorbed_attention's V2-Lite shape (16 heads, a
    prefix of 70) against the un-absorbed float64 attention, with that test's criterion: twice the error that the
    implementation's fp16 roundings alone cause in the same float64 formula."""
    B, H, P, dv = 2, 16, 70, _dev()
    f, m = RoPE.table(ROPE)
    k_b, v_b = _randn(H, RANK, 128, seed=20) * 128 ** -0.5, _randn(H, 128, RANK, seed=21) * RANK ** -0.5
    w = 1 + 0.1 * torch.randn(RANK, generator=torch.Generator().manual_seed(22))
    layer = MLAttention(k_b.to(dv), v_b.to(dv), w.to(dv), RoPE(torch.from_numpy(f).float().to(dv), ROPE, "norm", m), 1e-6, fused=True)
    cache = layer.new_cache(B, P + N, dv)
    q, kv = [_randn(B * n, H * 192, seed=23 + n) for n in (P, N)], [_randn(B * n, DK, seed=33 + n) for n in (P, N)]
    cache.append(kv[0][:, :RANK].to(dv), kv[0][:, RANK:].to(dv), q[0].to(dv), layer.rope, layer.norm_w, 1e-6)  # the prefix
    out = layer.forward(q[1].to(dv), kv[1].to(dv)).double().cpu()
    assert cache.kv_len.tolist() == [P + N] * B and out.shape == (B * N, H * 128)
    assert [kl.mla_proj_plan(d, B * N, H)[0] for d in (0, 1)] == [int(N > 8)] * 2

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
    print(f"fused layer, N={N}: max |out - exact| = {err:.3e}, the fp16 roundings alone = {own:.3e} (tolerance 2x)")
    assert err <= 2 * own
