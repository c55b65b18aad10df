"""Every instantiated decode kernel (csrc/mmq_decode.hip) against the oracle, case by case.

tests/decode_cases.py lists, from the library's cap and plan queries, every kernel of the five decode
families with the smallest and the largest K that select it; tests/test_decode_cases_host.py proves
the list complete.  Here each case runs at both K on a 37-row matrix (odd: a ragged last row group),
into NaN-filled outputs, after asserting through the plan query that the call takes the intended
kernel:

  dense          gq_mmq_ex held to the judges and gates of the per-type files (type_models.judge at
                 TIGHT_GEMV; the fp8 form: oracle.mmq_fp8_ideal at test_gpu_fp8.py's gate)
  id             gq_mmq_id: every valid pair the bits of the dense one-token call on its expert, the
                 pair with an id out of range zeros
  id_glu, glu    gq_mmq_id_glu / gq_mmq_glu: H within 1 ulp16 of moe_fused_model.glu on the fp16 g
                 and u of the dense calls (test_gpu_moe_fused.py _check_glu)
  grouped        gq_mmq_grouped_ex: the item beside the smallest item of the set's type, every
                 output the bits of its solo call

and once more under GQ_CUS = 1: eight waves for the matrix, so several rows per task
(G > 1) or several tasks per wave -- ring slots reused, a GLU stash of several rows -- where a whole
chip gives 37 rows one row per task and one task per wave.  mmq_decode.hip: "a row's arithmetic
depends on F, NT and K only", so those outputs must be the default run's bit for bit."""
import functools

import numpy as np
import pytest
import torch

import decode_cases as DC
import kernels._lib as kl
import moe_fused_model as MF
import oracle as O
import type_models as TM
from gpu_types import dev as _dev, no_timeouts_after_each_test, same_bits as _same_bits, to_w as _w  # noqa: F401
from test_gpu_fp8 import TIGHT_FP8
from test_gpu_moe_fused import _check_glu
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

M = DC.M
E, IDS = 3, np.array([[0, 2], [3, 1]], dtype=np.int32)  # N = 2 tokens x S = 2 slots; 3: out of range
assert IDS.size == DC.ID_PAIRS


def _cases(family):
    return [pytest.param(c, id=DC.case_id(c)) for c in DC.table().cases[family]]


@functools.lru_cache(maxsize=6)
def _raw(fmt, rows, K, which=0):
    raw = random_blocks(fmt, rows, K, seed=5000 * which + 10 * rows + K % 89)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=6)
def _acts(N, K):
    B = random_activations(N, K, seed=K + N)
    B.setflags(write=False)
    return B


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device=_dev())


def _x(B):
    return torch.from_numpy(np.array(B)).to(_dev())


def _force(c, tune):
    if c.force is not None:
        tune(GQ_DECODE_Q6_IMG=c.force)


def _plan(c, K, n=None, geometry=False):
    """The plan query's entries for the case's matrix at K, asserted to be the case's kernel (and, under
    GQ_CUS = 1, to give the waves several rows per task or several tasks)."""
    k = c.kernel
    ps = [p for p in kl.decode_plan(k.family, DC.items_of(k.family, k.set, k.fmt, K), c.N if n is None else n, DC.act_of(k))
          if p.item == 0]
    assert ps and all((p.nt, p.itc, p.img, p.fp8, p.set) == (k.nt, k.itc, k.img, k.fp8, k.set) for p in ps), \
        (c, K, [(p.nt, p.itc, p.img, p.fp8, p.set) for p in ps])
    if geometry:
        assert all(DC.busy(p) for p in ps), (c, K, [(p.G, p.ngroups, p.nseg, p.grid) for p in ps])
    return ps


def _twice(c, K, tune, run, n=None):
    """run() under the default plan and under GQ_CUS = 1, the plan asserted before each; the second
    output must have the first's bits.  Returns the first."""
    _plan(c, K, n)
    first = run()
    tune(GQ_CUS=1)
    _plan(c, K, n, geometry=True)
    second = run()
    tune(GQ_CUS=0)
    assert not torch.isnan(first).any(), (c, K, "default: output not written")
    assert not torch.isnan(second).any(), (c, K, "GQ_CUS=1: output not written")
    assert _same_bits(first, second), (c, K, "GQ_CUS=1 differs from the default run")
    return first


# ---- dense ----
@pytest.mark.parametrize("c", _cases("dense"))
def test_dense(c, tune):
    k = c.kernel
    gtype, act, N = kl.TYPES[k.fmt], DC.act_of(k), c.N
    _force(c, tune)
    for K in (c.kmin, c.kmax):
        raw, B = _raw(k.fmt, M, K), _acts(N, K)
        A, X = _w(raw), _x(B)
        assert kl.route_name(gtype, M, N, K, act) == "stream_decode_kernel"

        def run():
            C = kl.mmq(gtype, A, X, M, N, K, out=_nan(N, M), act=act)
            torch.cuda.synchronize()
            return C

        got = _twice(c, K, tune, run).cpu().numpy()
        if k.fp8:
            err, gate = O.max_rel_err(got, O.mmq_fp8_ideal(k.fmt, raw, B, M, N, K)), TIGHT_FP8
        else:
            err, gate = TM.rel_err(got, TM.judge(k.fmt, raw, B, M, N, K)), TM.TIGHT_GEMV
        print(f"{DC.case_id(c)} K={K}: max|d|/max|C| = {err:.2e}")
        assert err <= gate, (c, K, err)


# ---- expert-indexed ----
def _solo_rows(c, K, A, X, per):
    """(N, S, M): every valid pair's dense one-token call on its expert (asserted to plan the case's
    kernel), zeros for the pair whose id is out of range."""
    k = c.kernel
    gtype = kl.TYPES[k.fmt]
    p = kl.decode_plan("dense", [(gtype, M, K)], 1)
    assert len(p) == 1 and (p[0].nt, p[0].itc, p[0].img) == (1, k.itc, k.img), (c, K)
    out = torch.zeros((2, 2, M), dtype=torch.float16, device=_dev())
    for n in range(2):
        for s in range(2):
            e = int(IDS[n, s])
            if 0 <= e < E:
                out[n, s] = kl.mmq(gtype, A[e * per:(e + 1) * per], X[n:n + 1].contiguous(), M, 1, K)[0]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", _cases("id"))
def test_expert_indexed(c, tune):
    k = c.kernel
    gtype = kl.TYPES[k.fmt]
    _force(c, tune)
    it = torch.from_numpy(IDS).to(_dev())
    for K in (c.kmin, c.kmax):
        A, X = _w(_raw(k.fmt, E * M, K)), _x(_acts(2, K))
        per = A.numel() // E

        def run():
            C = _nan(2, 2, M)
            rc = kl.lib().gq_mmq_id(gtype, A.data_ptr(), it.data_ptr(), X.data_ptr(), C.data_ptr(), E, M, 2, 2, K, K, 0, M, None)
            assert rc == kl.GQ_OK, kl.lib().gq_last_error()
            torch.cuda.synchronize()
            return C

        got = _twice(c, K, tune, run, n=DC.ID_PAIRS)
        assert not got[1, 0].view(torch.int16).any(), (c, K, "the pair with an id out of range is not zeros")
        assert _same_bits(got, _solo_rows(c, K, A, X, per)), (c, K)


# ---- the GLU forms ----
def _glu_x(ideal_gu, B):
    """The activations scaled by a power of two -- 1/16 as test_gpu_moe_fused.py, or the first smaller one
    at which silu(g) * u of the dense ideal stays under half of fp16's range (long rows of Q6_K reach
    |g| ~ 300 at 1/16).  Decided on the CPU before anything runs; a power of two scales q8_1 exactly."""
    for sh in range(4, 12):
        x = (B * np.float16(2.0 ** -sh)).astype(np.float16)
        g, u = (np.asarray(v, np.float64) for v in ideal_gu(x))
        h = g / (1.0 + np.exp(-g)) * u
        if np.isfinite(h).all() and float(np.abs(h).max()) < 32768.0:
            assert np.isfinite(MF.glu(g.astype(np.float16), u.astype(np.float16))).all()
            return x
    raise AssertionError("no activation scale keeps silu(g) * u in fp16 range")


@pytest.mark.parametrize("c", _cases("id_glu"))
def test_expert_indexed_glu(c, tune):
    k = c.kernel
    gtype = kl.TYPES[k.fmt]
    _force(c, tune)
    it = torch.from_numpy(IDS).to(_dev())
    for K in (c.kmin, c.kmax):
        rg, ru = _raw(k.fmt, E * M, K, 0), _raw(k.fmt, E * M, K, 1)
        per = rg.size // E
        pairs = [(n, int(IDS[n, s])) for n in range(2) for s in range(2) if 0 <= IDS[n, s] < E]

        def ideal_gu(x):
            return [np.stack([TM.judge(k.fmt, r[e * per:(e + 1) * per], x[n:n + 1], M, 1, K)[0] for n, e in pairs])
                    for r in (rg, ru)]

        Ag, Au, X = _w(rg), _w(ru), _x(_glu_x(ideal_gu, _acts(2, K)))

        def run():
            H = _nan(2, 2, M)
            rc = kl.lib().gq_mmq_id_glu(gtype, Ag.data_ptr(), Au.data_ptr(), it.data_ptr(), X.data_ptr(), H.data_ptr(), E, M,
                                        2, 2, K, K, 0, M, None)
            assert rc == kl.GQ_OK, kl.lib().gq_last_error()
            torch.cuda.synchronize()
            return H

        H = _twice(c, K, tune, run, n=DC.ID_PAIRS)
        assert not H[1, 0].view(torch.int16).any(), (c, K, "the pair with an id out of range is not zeros")
        _check_glu(H, _solo_rows(c, K, Ag, X, per), _solo_rows(c, K, Au, X, per), f"{DC.case_id(c)} K={K}")


@pytest.mark.parametrize("c", _cases("glu"))
def test_dense_glu(c, tune):
    k = c.kernel
    gtype, N = kl.TYPES[k.fmt], c.N
    _force(c, tune)
    for K in (c.kmin, c.kmax):
        rg, ru = _raw(k.fmt, M, K, 0), _raw(k.fmt, M, K, 1)
        Ag, Au = _w(rg), _w(ru)
        X = _x(_glu_x(lambda x: [TM.judge(k.fmt, r, x, M, N, K) for r in (rg, ru)], _acts(N, K)))

        def run():
            H = _nan(N, M)
            rc = kl.lib().gq_mmq_glu(gtype, Ag.data_ptr(), Au.data_ptr(), X.data_ptr(), H.data_ptr(), M, N, K, K, M, None)
            assert rc == kl.GQ_OK, kl.lib().gq_last_error()
            torch.cuda.synchronize()
            return H

        H = _twice(c, K, tune, run)
        # g and u: the dense calls at this N, the dense family's kernel of the same (nt, itc, img)
        p = kl.decode_plan("dense", [(gtype, M, K)], N)
        assert p and all((q.nt, q.itc, q.img) == (k.nt, k.itc, k.img) for q in p), (c, K)
        g, u = kl.mmq(gtype, Ag, X, M, N, K), kl.mmq(gtype, Au, X, M, N, K)
        torch.cuda.synchronize()
        _check_glu(H, g, u, f"{DC.case_id(c)} K={K}")


# ---- grouped ----
@pytest.mark.parametrize("c", _cases("grouped"))
def test_grouped(c, tune):
    k = c.kernel
    act, N = DC.act_of(k), c.N
    _force(c, tune)
    f2, m2, k2 = DC.SET_ITEM[k.set]
    for K in (c.kmin, c.kmax):
        group = [(k.fmt, M, K), (f2, m2, k2)]
        data = [(kl.TYPES[f], _w(_raw(f, m, kk, i)), _x(_acts(N, kk)), m, kk) for i, (f, m, kk) in enumerate(group)]
        solos = [kl.mmq(t, A, X, m, N, kk, act=act) for t, A, X, m, kk in data]
        torch.cuda.synchronize()
        for cus in (0, 1):  # the chip, then one CU: one workgroup per item
            tune(GQ_CUS=cus)
            _plan(c, K, geometry=cus == 1)
            outs = kl.mmq_grouped([d + (_nan(N, d[3]),) for d in data], N, act)
            assert outs is not None, (c, K, kl.lib().gq_last_error())
            torch.cuda.synchronize()
            for (f, m, kk), C, solo in zip(group, outs, solos):
                assert not torch.isnan(C).any(), (c, K, f, cus, "NaN: the launch wrote no output for this item")
                assert _same_bits(C, solo), (c, K, f, cus)
        tune(GQ_CUS=0)
