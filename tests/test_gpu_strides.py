"""Every dense route at the strides and bases include/gguf_mmq.h documents: a result written into
a wider, sentinel-filled C (ldc > M, rows that start 2 or 6 bytes off an 8-byte boundary),
activations read from a wider, poisoned B (ldb > K, rows that are not 16 bytes, a base one
element off), and a workspace of exactly the size the library asks for with a guard band behind.

One test per route, the type as its parameter; each (shape, form) is one sweep():
  * the route is asserted by name (gq_debug_route) under the stated knobs;
  * the contiguous call, judged against the oracle at the suite's gates (type_models.judge and
    tight(N); the fp8 decode against tests/test_gpu_fp8.py's reference and bounds);
  * every stride variant: the same gate, bit identity with the call the header says it equals,
    untouched guards (tests/strided.py), a finite result under +inf and 65504 in B's padding.

Which call a variant equals:
  * the same kernel runs for every C variant and for every B variant of the decode, the GEMV and
    the kernels that read act_quant's x~: the contiguous call's bits;
  * the K-chunked stream stores 8 bytes through a buffer resource: only with ldc % 4 == 0 and C on
    an 8-byte boundary (gq_capi.hip kstream_fits).  Every other C takes what plan_call picks next,
    the route of the same call under GQ_KSTREAM=0 (at these shapes the skinny kernel for Q4_K and
    Q8_0 up to 16 tokens, the streaming GEMM for Q6_K from 5 tokens and for every type from 17;
    sweep() prints its name): that call's bits;
  * the kernels that quantize B themselves (the stream, the resident GEMM, the LDS-DMA GEMM with
    GQ_GEMM_AQ) given rows that are not 16 bytes: act_quant + the prepared call, so the bits of
    gq_act_prepare + gq_mmq_prepared on the contiguous copy.
hipBLASLt is given ldc = M, M + 24 and M + 3 on an aligned base only (the header lists a
misaligned C there as untested)."""
import numpy as np
import pytest
import torch

import kernels._lib as kl
import oracle as O
import type_models as TM
from gpu_types import dev, no_timeouts_after_each_test, same_bits, to_w, to_x  # noqa: F401 (the autouse fixture)
from strided import FMAX, INF, guarded_ws, wide_in, wide_out
from test_gpu_fp8 import FP8_BOUND, TIGHT_FP8
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

REF = ("q8_0", "q4_k", "q6_k")                 # the reference's types: every GEMM kernel
ADDED = ("q5_k", "q3_k", "q2_k", "q4_0")       # q8_1 activations, the streaming GEMM only
ALL = REF + ADDED


def c_variants(M):
    return [(M, 0), (M + 24, 0), (M + 3, 0), (M + 4, 1), (M + 1, 3)]


def b_variants(K):
    return [(K, 0), (K + 64, 0), (K + 4, 0), (K + 1, 0), (K, 1)]


class Case:
    """One (type, shape, activation format): inputs on the device, the reference, the two call forms."""

    def __init__(self, fmt, M, N, K, act):
        self.fmt, self.t, self.M, self.N, self.K, self.act = fmt, kl.TYPES[fmt], M, N, K, act
        raw = random_blocks(fmt, M, K, seed=7 * M + N)
        self.B = random_activations(N, K, seed=K + N)
        self.A, self.Bc = to_w(raw), to_x(self.B)
        if act == "fp8":
            self.want, self.loose = O.mmq_fp8_ideal(fmt, raw, self.B, M, N, K), O.mmq_fp32_dequant(fmt, raw, self.B, M, N, K)
        else:
            self.want = TM.judge(fmt, raw, self.B, M, N, K)

    def gate(self, C, what):
        got = C.cpu().numpy()
        assert np.isfinite(got.astype(np.float32)).all(), what
        if self.act == "fp8":
            err, loose = O.max_rel_err(got, self.want), O.max_rel_err(got, self.loose)
            assert err <= TIGHT_FP8 and loose <= FP8_BOUND, (what, err, loose)
        else:
            err = TM.rel_err(got, self.want)
            assert err <= TM.tight(self.N), (what, err)
        return err

    def raw(self, Bv, out):
        """gq_mmq_ex with exactly gq_mmq_call_workspace_size bytes."""
        need = int(kl.lib().gq_mmq_call_workspace_size(self.t, kl.ACTS[self.act], self.M, self.N, self.K))
        _, front, tail = guarded_ws(need)
        kl.mmq(self.t, self.A, Bv, self.M, self.N, self.K, out=out, workspace=front if need else None, act=self.act)
        torch.cuda.synchronize()
        tail()

    def prepared(self, Bv, out):
        """gq_act_prepare_ex + gq_mmq_prepared_ex with exactly gq_mmq_workspace_size_ex bytes."""
        need = kl.workspace_size(self.t, self.M, self.N, self.K, self.act)
        _, front, tail = guarded_ws(need)
        kl.act_prepare(Bv, self.N, self.K, front, act=self.act)
        kl.mmq_prepared(self.t, self.A, front, self.M, self.N, self.K, out=out, act=self.act)
        torch.cuda.synchronize()
        tail()

    def contiguous(self, call):
        _, view, check = wide_out(self.N, self.M, self.M, 0)
        call(self.Bc, view)
        check()
        return view


def sweep(tune, fmt, shape, route, knobs, form="raw", act="q8_1", quantizes=False, kstream=False, cvars=None,
          bvars=True, combined=True, apart=None):
    """The module docstring's checks for one (type, shape, form) under `knobs` (every other knob at
    its default).  quantizes: the raw call's kernel quantizes B itself; kstream: it is the K-chunked
    stream, and `apart` collects whether the off-stream call's bits differ from the stream's.
    Returns the contiguous call's result."""
    M, N, K = shape
    kl.reset_tuning()
    tune(**knobs)
    c = Case(fmt, M, N, K, act)
    name = kl.route_name(c.t, M, N, K, act=act, prepared=form == "prepared")
    assert name == route, (fmt, shape, form, knobs, name)
    call = c.raw if form == "raw" else c.prepared
    what = f"{fmt} {M}x{N}x{K} {act} {form} {name}"
    base = c.contiguous(call)
    print(f"{what}: max|d|/max|C| = {c.gate(base, what):.2e}")
    refs = {}

    def ref(kind):
        """'prep': the prepared form of the contiguous call; '...k0': under GQ_KSTREAM=0."""
        if kind not in refs:
            if kind.endswith("k0"):
                tune(GQ_KSTREAM=0)
                print(f"{what}: off the stream -> {kl.route_name(c.t, M, N, K, act=act, prepared=kind != 'k0')}")
            refs[kind] = c.contiguous(c.prepared if kind.startswith("prep") else call)
            if kind.endswith("k0"):
                tune(GQ_KSTREAM=1)
        return refs[kind]

    def judge(view, check, want, tag):
        assert same_bits(view, want), (what, tag)
        c.gate(view, (what, tag))
        check()

    for ldc, lead in (cvars or c_variants(M))[1:]:
        _, view, check = wide_out(N, M, ldc, lead)
        call(c.Bc, view)
        off_stream = kstream and (ldc % 4 != 0 or lead % 4 != 0)
        judge(view, check, ref("k0" if form == "raw" else "prepk0") if off_stream else base, f"ldc={ldc} lead={lead}")
    if kstream:
        apart.append(not same_bits(base, ref("k0" if form == "raw" else "prepk0")))
    if form != "raw" or not bvars:
        return base
    for poison in (INF, FMAX):
        for ldb, lead in b_variants(K):
            _, view, check = wide_out(N, M, M, 0)
            c.raw(wide_in(c.B, ldb, lead, poison), view)
            rows16 = ldb % 8 == 0 and lead % 8 == 0
            judge(view, check, base if rows16 or not quantizes else ref("prep"), f"ldb={ldb} lead={lead} pad={poison}")
    if combined:
        _, view, check = wide_out(N, M, M + 3, 1)
        c.raw(wide_in(c.B, K + 1, 0, INF), view)
        judge(view, check, base if not quantizes else ref("prepk0" if kstream else "prep"), "ldc=M+3 lead=1 ldb=K+1")
    return base


# ---- the decode and the GEMV ----
DECODE = "stream_decode_kernel"
DECODE_SHAPES = [(65, 4, 1024), (5, 3, 512), (63, 2, 768)]


@pytest.mark.parametrize("fmt", ALL)
def test_stream_decode(fmt, tune):
    for shape in DECODE_SHAPES + ([(37, 3, 96)] if fmt in ("q8_0", "q4_0") else []):
        for form in ("raw", "prepared"):
            sweep(tune, fmt, shape, DECODE, {}, form)


@pytest.mark.parametrize("fmt", REF)
def test_fp8_decode(fmt, tune):
    # (one token at 97 rows, not the decode list's 5: FP8_BOUND is a bound on max|d| / max|C|, and over
    # five outputs the two references themselves are 0.064 apart -- Q4_K (5, 1, 512), no kernel
    # involved; tests/test_gpu_fp8.py's smallest shape has 96 rows)
    for shape in [(65, 2, 1024), (97, 1, 512), (63, 2, 768)]:
        for form in ("raw", "prepared"):
            sweep(tune, fmt, shape, DECODE, {}, form, act="fp8")


@pytest.mark.parametrize("fmt", ALL)
def test_gemv(fmt, tune):
    off = dict(GQ_NO_FUSED_DECODE=1)
    for form in ("raw", "prepared"):
        sweep(tune, fmt, (37, 3, 512), "gemv_kernel", off, form)
    # the long rows: Q3_K's and Q2_K's four tokens of K = 8960 fit no decode image (the GEMV by
    # default); the other types' do, and take it with the decode off
    sweep(tune, fmt, (16, 4, 8960), "gemv_kernel", {} if fmt in ("q3_k", "q2_k") else off)


# ---- the K-chunked stream ----
@pytest.mark.parametrize("fmt", REF)
def test_kstream(fmt, tune):
    on, apart = dict(GQ_KSTREAM=1), []
    for shape in [(48, 31, 512), (16, 5, 256)]:
        for form in ("raw", "prepared"):
            sweep(tune, fmt, shape, "kstream_kernel", on, form, quantizes=True, kstream=True, apart=apart)
    # K = 4352: two K ranges into fp32 partials, summed by kstream_reduce_kernel
    sweep(tune, fmt, (256, 32, 4352), "kstream_kernel + kstream_reduce_kernel", on, quantizes=True, kstream=True,
          apart=apart)
    # the off-stream variants were held to the GQ_KSTREAM=0 call's bits: that tells the two routes
    # apart only where those differ from the stream's (another fp32 order of the sum over K)
    print(f"{fmt}: off-stream bits differ from the stream's in {sum(apart)} of {len(apart)} sweeps")
    assert any(apart)


# ---- the resident GEMM ----
RGEMM = dict(GQ_RGEMM=1, GQ_SKINNY=0, GQ_KSTREAM=0)
RGEMM_REDUCE = "rgemm_kernel + gemm_reduce_f16_kernel"


@pytest.mark.parametrize("fmt", REF)
def test_rgemm(fmt, tune):
    for shape in [(513, 20, 768), (300, 100, 1024)]:
        for form in ("raw", "prepared"):
            sweep(tune, fmt, shape, RGEMM_REDUCE, RGEMM, form, quantizes=True)
    on = sweep(tune, fmt, (256, 128, 512), RGEMM_REDUCE, RGEMM, quantizes=True)  # (GQ_RGEMM_ESTORE at its default)
    off = sweep(tune, fmt, (256, 128, 512), RGEMM_REDUCE, dict(RGEMM, GQ_RGEMM_ESTORE=0), quantizes=True)
    assert same_bits(on, off)


def test_rgemm_in_launch_sum(tune):
    sweep(tune, "q8_0", (300, 100, 1024), "rgemm_kernel (in-launch split-K sum)", dict(RGEMM, GQ_RGEMM_ILC=1),
          quantizes=True)


# ---- the skinny kernel ----
@pytest.mark.parametrize("fmt", REF)
def test_skinny(fmt, tune):
    for shape in [(33, 20, 512), (129, 7, 768)]:
        for form in ("raw", "prepared"):
            sweep(tune, fmt, shape, "skinny_kernel", dict(GQ_SKINNY=1), form)


# ---- the streaming GEMM ----
SGEMM = dict(GQ_SGEMM=1, GQ_RGEMM=0, GQ_SKINNY=0, GQ_KSTREAM=0)
SGEMM_REDUCE = "sgemm_kernel + gemm_reduce_f16_kernel"
STREAMK = "sgemm_grouped_kernel + reduce_grouped_kernel (stream-K)"
STREAMK_SHAPE = (300, 40, 2048)  # (two row tiles x eight super-blocks dealt over the chip's workgroups)


@pytest.mark.parametrize("fmt", ALL)
def test_sgemm(fmt, tune):
    for shape in [(129, 17, 768), (70, 16, 512)]:
        for form in ("raw", "prepared"):
            sweep(tune, fmt, shape, "sgemm_kernel", dict(SGEMM, GQ_SGEMM_SPLITS=1), form)
    sweep(tune, fmt, (257, 40, 2816), SGEMM_REDUCE, dict(SGEMM, GQ_SGEMM_SPLITS=3))
    sweep(tune, fmt, (257, 40, 2816), SGEMM_REDUCE, dict(SGEMM, GQ_SGEMM_SPLITS=3), "prepared")


@pytest.mark.parametrize("fmt", ALL)
def test_sgemm_stream_k(fmt, tune):
    sweep(tune, fmt, STREAMK_SHAPE, STREAMK, dict(SGEMM, GQ_SGEMM_STREAMK=1))


# ---- the LDS-DMA GEMM ----
GEMM = dict(GQ_SGEMM=0, GQ_RGEMM=0, GQ_SKINNY=0, GQ_KSTREAM=0)
GEMM_NAME = "gemm_kernel + gemm_reduce_f16_kernel"


@pytest.mark.parametrize("fmt", REF)
def test_gemm(fmt, tune):
    for shape, splits in (((130, 33, 256), 1), ((300, 128, 2048), 4)):
        outs = []
        for aq in ({}, dict(GQ_GEMM_AQ=0)):  # (the kernel quantizes 16/32-token tiles itself / reads act_quant's x~)
            knobs = dict(GEMM, GQ_GEMM_SPLITS=splits, **aq)
            outs.append(sweep(tune, fmt, shape, GEMM_NAME, knobs, quantizes=True))
            sweep(tune, fmt, shape, GEMM_NAME, knobs, "prepared")
        assert same_bits(*outs)


# ---- calls cut into row and token chunks (C + n0*ldc + m0 per chunk) ----
CHUNK_LIMITS = {"q5_k": 140000, "q3_k": 140000, "q2_k": 86100, "q4_0": 147600}  # (each type file's own limit)


def chunked(tune, fmt, shape, route, knobs, limit):
    whole = sweep(tune, fmt, shape, route, knobs, bvars=False, cvars=c_variants(shape[0])[:1])
    assert same_bits(sweep(tune, fmt, shape, route, dict(knobs, GQ_GEMM_MAX_BYTES=limit), bvars=False), whole)


@pytest.mark.parametrize("fmt", ADDED)
def test_sgemm_row_chunks(fmt, tune):
    chunked(tune, fmt, (600, 24, 512), "sgemm_kernel", dict(GQ_SGEMM_SPLITS=1), CHUNK_LIMITS[fmt])


@pytest.mark.parametrize("fmt", REF)
def test_skinny_row_chunks(fmt, tune):
    chunked(tune, fmt, (600, 20, 2048), "skinny_kernel", dict(GQ_SKINNY=1), 256 * 1024)


@pytest.mark.parametrize("fmt", REF)
def test_gemm_row_and_token_chunks(fmt, tune):
    # 128 KiB: 256 rows of K = 512 and 128 tokens per launch -- 3 x 2 chunks, the last 88 rows x 22 tokens
    chunked(tune, fmt, (600, 150, 512), GEMM_NAME, dict(GEMM, GQ_GEMM_SPLITS=1, GQ_BLAS_MIN_TOKENS=0), 128 * 1024)


# ---- dequantize + hipBLASLt ----
@pytest.mark.parametrize("fmt", ALL)
def test_hipblaslt(fmt, tune):
    for shape in [(65, 24, 1024), (130, 33, 256)]:
        M = shape[0]
        for form in ("raw", "prepared"):
            sweep(tune, fmt, shape, "dequant_kernel + hipBLASLt", dict(GQ_BLAS_MIN_TOKENS=9), form,
                  cvars=[(M, 0), (M + 24, 0), (M + 3, 0)], combined=False)


# ---- the stand-alone kernels ----
def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("fmt", ALL)
def test_dequantize_strided(fmt):
    t, M, K = kl.TYPES[fmt], 37, 768
    A = to_w(random_blocks(fmt, M, K, seed=4))
    outs = []
    for ldw, lead in ((K, 0), (K + 24, 0), (K + 1, 0), (K + 1, 1)):
        _, view, check = wide_out(M, K, ldw, lead)
        assert kl.lib().gq_dequantize(t, A.data_ptr(), view.data_ptr(), M, K, ldw, stream()) == 0, kl.lib().gq_last_error()
        torch.cuda.synchronize()
        check()
        outs.append(view)
        assert same_bits(view, outs[0]), (ldw, lead)
    assert same_bits(outs[0], kl.dequantize_device(t, A, M, K))
    assert bool(torch.isfinite(outs[0]).all())


X_VARIANTS = [(lambda K: K + 4, 0), (lambda K: K + 1, 0), (lambda K: K, 1)]
TOKENS = (1, 3, 20, 77)  # (77: scale_ld(N) = 80, the pad columns of the block-major scales)


def x_views(x):
    K = x.shape[1]
    yield "contiguous", to_x(x)
    for poison in (INF, FMAX):
        for ld, lead in X_VARIANTS:
            yield f"ldx={ld(K)} lead={lead} pad={poison}", wide_in(x, ld(K), lead, poison)


@pytest.mark.parametrize("act,i8", [("q8_1", 0), ("q8_1", 1), ("fp8", 0)])
def test_act_prepare_strided(act, i8, tune):
    """gq_act_prepare_ex writes the contiguous copy's bytes from every view, every form it keeps:
    the decode's SOA q8_1 and raw copy, x~, with GQ_GEMM_I8=1 the int8 codes and block-major scales."""
    K = 1280
    tune(GQ_GEMM_I8=i8)
    for N in TOKENS:
        x = random_activations(N, K, seed=N)
        need = kl.workspace_size(kl.GQ_Q8_0, 16, N, K, act)
        want = None
        for tag, view in x_views(x):
            alloc, front, tail = guarded_ws(need)
            kl.act_prepare(view, N, K, front, act=act)
            torch.cuda.synchronize()
            tail()
            assert bool((front != 0xA5).any())
            want = front if want is None else want
            assert torch.equal(front, want), (N, tag)


def test_quantize_q8_1_strided():
    K = 1280
    for N in TOKENS:
        x = random_activations(N, K, seed=N + 100)
        need, want = N * (K // 32) * 36, None
        for tag, view in x_views(x):
            _, front, tail = guarded_ws(need)
            rc = kl.lib().gq_quantize_q8_1(view.data_ptr(), front.data_ptr(), N, K, view.stride(0), stream())
            assert rc == 0, kl.lib().gq_last_error()
            torch.cuda.synchronize()
            tail()
            want = front if want is None else want
            assert torch.equal(front, want), (N, tag)
        assert np.array_equal(want.cpu().numpy(), O.quantize_q8_1(x).reshape(-1).view(np.uint8))


def test_quantize_fp8_strided():
    K = 1280
    for N in TOKENS:
        x = random_activations(N, K, seed=N + 200)
        ld, want = (N + 3) & ~3, None
        for tag, view in x_views(x):
            _, codes, ctail = guarded_ws(N * K)
            _, scales, stail = guarded_ws(K // 32 * ld * 4)
            rc = kl.lib().gq_quantize_fp8(view.data_ptr(), codes.data_ptr(), scales.data_ptr(), N, K, view.stride(0), stream())
            assert rc == 0, kl.lib().gq_last_error()
            torch.cuda.synchronize()
            ctail()
            stail()
            want = (codes, scales) if want is None else want
            assert torch.equal(codes, want[0]) and torch.equal(scales, want[1]), (N, tag)
        want_c, want_x = O.quantize_fp8(x)
        assert np.array_equal(want[0].cpu().numpy().reshape(N, K), O.fp8_permuted(want_c))
        assert np.array_equal(want[1].view(torch.float32).cpu().numpy().reshape(K // 32, ld)[:, :N].T, want_x)
