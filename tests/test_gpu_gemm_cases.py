"""Every instantiated MFMA GEMM kernel (csrc/mmq_rgemm.hip, mmq_gemm.hip, mmq_skinny.hip, mmq_kstream.hip)
against the oracle, case by case.

tests/gemm_cases.py lists, from the library's symbol table and its plan query, every kernel of the four
files in every run-time form, with the call of smallest K that selects it at each token count;
tests/test_gemm_cases_host.py proves the list complete.  Here each case first asserts through the plan
query that its call launches the kernels and forms it is kept for, then runs it -- 293 rows (two 256-row
tiles, the last of 37 rows), 304 for the K-chunked stream -- into a NaN-filled output with one sentinel
token row after the last, and asserts: no NaN left, the sentinel untouched, max|d| <= 4e-3 max|C| against
the high-precision statement of the operation (oracle IDEAL / type_models.judge; the fp8 variant:
oracle.mmq_fp8_ideal at test_gpu_fp8.py's gate), no synchronisation wait given up.

Then the identities the code base claims, bit for bit, each other side planned and asserted by the query
before it runs:
  * the plan made for the other chip size (GQ_CUS = 8, or 4, against 256) wherever the kernel and its splits are
    unchanged -- within the gate where they change;
  * in-kernel quantization (rgemm_kernel's and gemm_kernel's AQ, the K-chunked stream's raw call) = the
    prepared call; rgemm_kernel's early store (ES = 1) = the classic epilogue; the in-launch split-K sum
    (GQ_RGEMM_ILC) = the reduce launch, which also sets sgemm_kernel's orders 1 against 0 and 2;
    GQ_SGEMM_FULL 1 = 0;
  * a grouped item = its solo call at the same split (whole-tile splits; the stream-K unit split is
    held to the gate), an item of the K-chunked stream's grouped launch = its solo call;
  * the sorted entry: every valid pair within the gate of the dense prepared call on its expert and of the
    oracle, the pair with an id out of range zeros, GQ_SGEMM_FULL 1 = 0.
Which reruns keep kernel and split is gemm_cases.identities' reading of the plan query; the host test asserts that
each identity has pairs in each family it applies to."""
import functools

import numpy as np
import pytest
import torch

import gemm_cases as GC
import kernels._lib as kl
import oracle as O
import type_models as TM
from gpu_types import dev as _dev, no_timeouts_after_each_test, same_bits as _same_bits, to_w as _w, to_x as _x  # noqa: F401
from test_gpu_fp8 import TIGHT_FP8
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

GATE = {"q8_1": TM.TIGHT_GEMM, "fp8": TIGHT_FP8}
NAME = kl.GEMM_KERNELS


def _cases(family):
    return [pytest.param(c, id=GC.case_id(c)) for c in GC.table().cases[family]]


@functools.lru_cache(maxsize=None)
def _raw(fmt, rows, K, which=0):
    raw = random_blocks(fmt, rows, K, seed=7000 * which + 10 * rows + K % 89)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def _acts(N, K):
    B = random_activations(N, K, seed=K + N)
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def _want(fmt, rows, N, K, act, which=0):
    """The high-precision (N, rows) result: computed once, never written to."""
    raw, B = _raw(fmt, rows, K, which), _acts(N, K)
    want = O.mmq_fp8_ideal(fmt, raw, B, rows, N, K) if act == "fp8" else TM.judge(fmt, raw, B, rows, N, K)
    want = np.asarray(want, np.float64)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=16)
def _dev_w(fmt, rows, K, which=0):
    return _w(_raw(fmt, rows, K, which))


@functools.lru_cache(maxsize=16)
def _dev_x(N, K):
    return _x(_acts(N, K))


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device=_dev())


def _set(tune, call, cus=None, **more):
    kl.reset_tuning()
    tune(**dict(GC.TUNING[call.vector], GQ_CUS=call.cus if cus is None else cus, **more))


def _prepared_ws(N, K, act):
    ws = torch.empty(kl.workspace_size(kl.GQ_Q8_0, 512, N, K, act), dtype=torch.uint8, device=_dev())
    kl.act_prepare(_dev_x(N, K), N, K, ws, act=act)
    return ws


def _run(call):
    """The call under the current tuning: [(N + 1, M) output per item], row N the sentinel."""
    N, act = call.N, call.act
    data = [(kl.TYPES[f], _dev_w(f, m, k, i), m, k) for i, (f, m, k) in enumerate(call.items)]
    outs = [_nan(N + 1, m) for _, _, m, _ in data]
    if call.entry == "ex":
        (t, A, m, k), = data
        kl.mmq(t, A, _dev_x(N, k), m, N, k, out=outs[0][:N], act=act)
    elif call.entry == "prepared":
        (t, A, m, k), = data
        ws = torch.empty(kl.workspace_size(t, m, N, k, act), dtype=torch.uint8, device=_dev())
        kl.act_prepare(_dev_x(N, k), N, k, ws, act=act)
        kl.mmq_prepared(t, A, ws, m, N, k, out=outs[0][:N], act=act)
    elif call.entry == "grouped_prepared":
        got = kl.mmq_grouped_prepared([(t, A, _prepared_ws(N, k, act), m, k, C[:N]) for (t, A, m, k), C in zip(data, outs)], N, act)
        assert got is not None, (call, kl.lib().gq_last_error())
    elif call.entry == "grouped_ex":
        got = kl.mmq_grouped([(t, A, _dev_x(N, k), m, k, C[:N]) for (t, A, m, k), C in zip(data, outs)], N, act)
        assert got is not None, (call, kl.lib().gq_last_error())
    else:
        raise AssertionError(call.entry)
    torch.cuda.synchronize()
    return outs


def _mine(call):
    """The plan entries of the matrix under test, under the current tuning."""
    return GC.under_test(GC.plan(call))


def _check_output(c, C, item=0, what=""):
    call = c.call
    fmt, rows, K = call.items[item]
    N = call.N
    assert torch.isnan(C[N]).all(), (c, what, "the sentinel row after the last token was written")
    assert not torch.isnan(C[:N]).any(), (c, what, "NaN: part of the output was not written")
    err = TM.rel_err(C[:N].cpu().numpy(), _want(fmt, rows, N, K, call.act, item))
    print(f"{GC.case_id(c)} {what}: max|d|/max|C| = {err:.2e}")
    assert err <= GATE[call.act], (c, what, err)


def _case(c, tune):
    """The case as the module's docstring says; returns its plan entries and the output of the matrix under test."""
    call = c.call
    assert torch.cuda.get_device_properties(0).multi_processor_count >= GC.CUS  # (never plan for more CUs than the chip has)
    entries, same = GC.identities(c)
    _set(tune, call)
    got = {(GC.kernel_of(p), GC.form_of(p, call.cus)) for p in _mine(call)}
    assert set(c.covers) <= got, (c, got)
    outs = _run(call)
    for i in range(len(call.items)):
        _check_output(c, outs[i], i, "case")
    first = outs[0]
    # the plan for the other chip size: within the gate whatever it splits into
    other = GC.other_cus(call)
    if not any(label == "cus" for label, _, _ in same):
        _set(tune, call, cus=other)
        assert _mine(call), (c, other)
        _check_output(c, _run(call)[0], 0, f"GQ_CUS={other}")
    # the reruns that keep kernel and K split (gemm_cases.identities): the first run's bits
    for label, over, rerun in same:
        GC.apply(call, **dict(over))
        assert _same_bits(first, _run(rerun)[0]), (c, f"{label} {over}: the output differs at the same kernel and split")
    return entries, first


@pytest.mark.parametrize("c", _cases("rgemm_kernel"))
def test_rgemm(c, tune):
    _case(c, tune)


@pytest.mark.parametrize("c", _cases("sgemm_kernel"))
def test_sgemm(c, tune):
    _case(c, tune)


@pytest.mark.parametrize("c", _cases("gemm_kernel"))
def test_gemm(c, tune):
    _case(c, tune)


@pytest.mark.parametrize("c", _cases("skinny_kernel"))
def test_skinny(c, tune):
    _case(c, tune)


@pytest.mark.parametrize("c", _cases("kstream_kernel"))
def test_kstream(c, tune):
    call = c.call
    entries, first = _case(c, tune)
    if call.entry in ("grouped_ex", "grouped_prepared"):
        # "a matrix's bits do not depend on the launch it is in": the item's solo call on the stream
        _set(tune, call, GQ_KSTREAM=1)
        solo = call._replace(entry="ex" if call.entry == "grouped_ex" else "prepared", items=call.items[:1])
        es = _mine(solo)
        assert es and NAME[es[0].kernel] == "kstream_kernel" and es[0].aq == entries[0].aq, (c, es)
        assert _same_bits(first, _run(solo)[0]), (c, "the grouped launch's item differs from its solo call")


@pytest.mark.parametrize("c", _cases("sgemm_grouped_kernel"))
def test_sgemm_grouped(c, tune):
    call = c.call
    entries, first = _case(c, tune)
    mine = [p for p in entries if NAME[p.kernel] == "sgemm_grouped_kernel" and p.item == 0]
    if call.entry != "grouped_prepared" or not mine or mine[0].streamk:
        return  # (a single matrix on the stream-K plan, or the unit split: the oracle gate above)
    # whole-tile splits: the item's solo call on the streaming GEMM at the same split, bit for bit
    kl.reset_tuning()
    tune(GQ_CUS=call.cus, GQ_SGEMM=1, GQ_RGEMM=0, GQ_SKINNY=0, GQ_KSTREAM=0, GQ_SGEMM_SPLITS=mine[0].splits)
    solo = call._replace(entry="prepared", items=call.items[:1])
    es = _mine(solo)
    assert es and NAME[es[0].kernel] == "sgemm_kernel" and es[0].splits == mine[0].splits, (c, es)
    assert _same_bits(first, _run(solo)[0]), (c, "the grouped item differs from its solo call at the same split")


# ---- the sorted entry ----
def _ids(N):
    """(N, S) expert ids over E = 3: experts 0 and 2 take every token, expert 1 no pair, one id out of range."""
    ids = np.tile(np.array([0, 2], dtype=np.int32), (N, 1))
    ids[N // 2, 1] = GC.E  # out of range
    return ids


@pytest.mark.parametrize("c", _cases("sgemm_id_kernel"))
def test_sgemm_id(c, tune):
    call = c.call
    (fmt, M, K), N, t = call.items[0], call.N, kl.TYPES[call.items[0][0]]
    E, S = GC.E, GC.S
    _set(tune, call)
    entries = _mine(call)
    assert set(c.covers) <= {(GC.kernel_of(p), GC.form_of(p, call.cus)) for p in entries}, (c, entries)
    raws = [_raw(fmt, M, K, e) for e in range(E)]
    A = _w(np.concatenate(raws))
    per = A.numel() // E
    ids = _ids(N)
    xt, it = _dev_x(N, K), torch.from_numpy(ids).to(_dev())
    out = _nan(N + 1, S, M)
    kl.mmq_id_sorted(t, A, it, xt, E, M, K, out=out[:N])
    torch.cuda.synchronize()
    assert torch.isnan(out[N]).all(), (c, "the sentinel rows after the last token were written")
    assert not torch.isnan(out[:N]).any(), (c, "NaN: a pair's row was not written")
    g = out[:N].reshape(N * S, M)
    bad = (N // 2) * S + 1
    assert not g[bad].view(torch.int16).any(), (c, "the pair with an id out of range is not zeros")
    flat = ids.reshape(-1)
    assert not (flat == 1).any()
    for e in (0, 2):
        pairs = np.nonzero(flat == e)[0]
        idx = torch.from_numpy(pairs).to(_dev())
        toks = pairs // S
        n = len(pairs)
        want = TM.judge(fmt, raws[e], np.ascontiguousarray(_acts(N, K)[toks]), M, n, K)
        got = g.index_select(0, idx)
        err = TM.rel_err(got.cpu().numpy(), want)
        print(f"{GC.case_id(c)} expert {e}: {n} pairs, max|d|/max|C| = {err:.2e}")
        assert err <= TM.TIGHT_GEMM, (c, e, err)
        # the dense prepared call on the expert, over the expert's gathered rows
        rows = xt.index_select(0, torch.from_numpy(toks).to(_dev())).contiguous()
        ws = torch.empty(kl.workspace_size(t, M, n, K), dtype=torch.uint8, device=_dev())
        kl.act_prepare(rows, n, K, ws)
        dense = kl.mmq_prepared(t, A[e * per:(e + 1) * per], ws, M, n, K)
        torch.cuda.synchronize()
        assert TM.rel_err(got.cpu().numpy(), dense.cpu().numpy().astype(np.float64)) <= TM.TIGHT_GEMM, (c, e)
    # GQ_SGEMM_FULL 1 = 0, where the kernel has the whole-super-block form
    full = entries[0].full
    GC.apply(call, GQ_SGEMM_FULL=0 if full else 1)
    e2 = _mine(call)
    if e2[0].full != full:
        assert GC.kernel_of(e2[0]) == GC.kernel_of(entries[0])
        out2 = _nan(N + 1, S, M)
        kl.mmq_id_sorted(t, A, it, xt, E, M, K, out=out2[:N])
        torch.cuda.synchronize()
        assert _same_bits(out[:N], out2[:N]), (c, "GQ_SGEMM_FULL changes the sorted GEMM's output")
