"""GPU tests of the resident GEMM's early-store form (csrc/mmq_rgemm.hip mul_half1_early,
GQ_RGEMM_ESTORE): the second half multiply runs token group by token group and every group's
split-K partials are stored, scaled for a wave exponent of 0, under the next group's MFMAs; a wave
whose exponent turns out above 0 waits for those stores and writes its units again with the true
scale.  Only independent MFMAs are reordered and stores moved, so knob 1 must equal knob 0 (the
classic epilogue, store_tile after the last MFMA) bit for bit: on every format, token tile, split
count, call form and activation type, ragged rows and tokens, on inputs that really take the
re-store path, in a replayed graph and under the in-launch combine."""
import numpy as np
import pytest
import torch

import oracle as O
from utils.synth import random_activations, random_blocks

pytestmark = pytest.mark.gpu

TIGHT = 4e-3  # tests/test_gpu_rgemm.py's tolerance against the oracle's IDEAL mode
FMTS = ("q8_0", "q4_k", "q6_k")
# ragged rows and tokens, NB 2 / 4 / 8, 2..8 splits, and the one-split form (K = 256: fp16 C)
SHAPES = [(256, 128, 512), (300, 100, 1024), (513, 20, 768), (700, 33, 2048), (1000, 40, 512), (256, 128, 256)]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _raw(kl, t, A, B, M, N, K, act):
    C = torch.full((N, M), float("nan"), dtype=torch.float16, device=_dev())
    need = int(kl.lib().gq_mmq_call_workspace_size(t, kl.ACTS[act], M, N, K))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=_dev())
    rc = kl.lib().gq_mmq_ex(t, kl.ACTS[act], A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, K, M, ws.data_ptr(),
                            ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, kl.lib().gq_last_error()
    torch.cuda.synchronize()
    return C


def _prep(kl, t, A, B, M, N, K, act):
    ws = torch.empty(kl.workspace_size(t, M, N, K, act), dtype=torch.uint8, device=_dev())
    kl.act_prepare(B, N, K, ws, act=act)
    C = torch.full((N, M), float("nan"), dtype=torch.float16, device=_dev())
    kl.mmq_prepared(t, A, ws, M, N, K, out=C, act=act)
    torch.cuda.synchronize()
    return C


def _knob(kl, v, fn, *a):
    kl.set_tuning("GQ_RGEMM_ESTORE", v)
    return fn(kl, *a)


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_estore_bits_equal_classic(fmt, M, N, K, tune):
    import kernels._lib as kl
    tune(GQ_RGEMM=1, GQ_SKINNY=0, GQ_KSTREAM=0)
    t = kl.TYPES[fmt]
    A = _t(random_blocks(fmt, M, K, seed=M + K).view(np.int8))
    B = _t(random_activations(N, K, seed=N + 3 * K))
    for prepared in (False, True):
        name = kl.route_name(t, M, N, K, prepared=prepared)
        assert name.startswith("rgemm_kernel"), name
    before = kl.lib().gq_debug_sync_timeouts()
    for act in ("q8_1", "fp8"):
        for fn in (_raw, _prep):
            got = _knob(kl, 1, fn, t, A, B, M, N, K, act)
            ref = _knob(kl, 0, fn, t, A, B, M, N, K, act)
            assert not torch.isnan(ref).any()
            assert _same(got, ref), (act, fn.__name__)
    assert kl.lib().gq_debug_sync_timeouts() == before


def _spiked_case(fmt):
    """(qA, B) at M = 256, N = 128, K = 512 whose split 0 takes the re-store path in the wave of
    rows 0..31 only: those rows' weights are 64 times the others', and token SPIKE's activations
    are scaled, in super-block 0, until its largest partial is about 46000 -- inside [2^15, 65504),
    so that wave's exponent is 1 and every fp16 output is finite -- and zero in super-block 1."""
    from utils.quantize.q4_k import quantize_to_q4_k
    from utils.quantize.q6_k import quantize_to_q6_k
    from utils.quantize.q8_0 import quantize_to_q8_0
    M, N, K, spike = 256, 128, 512, 5
    rng = np.random.default_rng(11)
    W = rng.standard_normal((M, K), dtype=np.float32)
    W[32:] *= 1.0 / 64
    quant = {"q8_0": quantize_to_q8_0, "q4_k": quantize_to_q4_k, "q6_k": quantize_to_q6_k}[fmt]
    qA = quant(torch.from_numpy(W).to(torch.float16)).numpy().view(np.uint8)
    B = random_activations(N, K, seed=12).copy()
    B[spike, 256:] = 0
    B[spike, :256] = (B[spike, :256].astype(np.float32) * 64).astype(np.float16)
    for _ in range(2):  # (the second pass corrects what the requantization of the scaled row moved)
        top = np.abs(_split0(fmt, qA, B, M, N).astype(np.float32)).max()
        assert np.isfinite(top) and top > 0
        B[spike, :256] = (B[spike, :256].astype(np.float32) * (46000.0 / top)).astype(np.float16)
    return qA, B, M, N, K


def _split0(fmt, qA, B, M, N):
    """IDEAL partials of split 0 (the first super-block of every row) as fp16 (N, M)."""
    rb = qA.size // M
    sb0 = np.ascontiguousarray(qA.reshape(M, rb)[:, :rb // 2])
    return O.mmq_from_fp16(fmt, sb0, np.ascontiguousarray(B[:, :256]), M, N, 256, O.IDEAL)


@pytest.mark.parametrize("fmt", FMTS)
def test_estore_rewrite_path_runs(fmt, tune):
    import kernels._lib as kl
    qA, B, M, N, K = _spiked_case(fmt)
    # the preconditions, on the CPU: per wave (32 rows x every token of the tile) the largest
    # |partial| of split 0 -- one wave at least re-stores, one at least does not, nothing overflows
    p0 = np.abs(_split0(fmt, qA, B, M, N).astype(np.float32))
    assert np.isfinite(p0).all()
    wave_max = p0.reshape(N, M // 32, 32).max(axis=(0, 2))
    assert (wave_max >= 2.0 ** 15).any(), wave_max
    assert (wave_max < 2.0 ** 15).any(), wave_max
    ideal = O.mmq_from_fp16(fmt, qA, B, M, N, K, O.IDEAL)
    assert np.isfinite(ideal.astype(np.float32)).all()

    tune(GQ_RGEMM=1, GQ_SKINNY=0, GQ_KSTREAM=0)
    t = kl.TYPES[fmt]
    assert kl.route_name(t, M, N, K).startswith("rgemm_kernel")
    A_t, B_t = _t(qA.view(np.int8)), _t(B)
    for fn in (_raw, _prep):
        got = _knob(kl, 1, fn, t, A_t, B_t, M, N, K, "q8_1")
        ref = _knob(kl, 0, fn, t, A_t, B_t, M, N, K, "q8_1")
        assert _same(got, ref), fn.__name__
        for c in (got, ref):
            err = O.max_rel_err(c.cpu().numpy(), ideal)
            assert err <= TIGHT, err


def test_estore_graph_replays(tune):
    """The (256, 128, 512) Q8_0 raw call captured once and replayed three times into a NaN-filled
    output: every replay has the eager call's bits."""
    import kernels._lib as kl
    tune(GQ_RGEMM=1, GQ_SKINNY=0, GQ_KSTREAM=0, GQ_RGEMM_ESTORE=1)
    t, M, N, K = kl.GQ_Q8_0, 256, 128, 512
    A = _t(random_blocks("q8_0", M, K, seed=21).view(np.int8))
    B = _t(random_activations(N, K, seed=22))
    ref = _raw(kl, t, A, B, M, N, K, "q8_1")
    need = int(kl.lib().gq_mmq_call_workspace_size(t, 0, M, N, K))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=_dev())
    C = torch.empty(N, M, dtype=torch.float16, device=_dev())

    def call():
        rc = kl.lib().gq_mmq_ex(t, 0, A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, K, M, ws.data_ptr(), need,
                                torch.cuda.current_stream().cuda_stream)
        assert rc == 0

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(3):
        C.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert _same(C, ref)


@pytest.mark.parametrize("M,N,K", [(4096, 128, 4096), (300, 100, 1024)])
def test_estore_under_in_launch_combine(M, N, K, tune):
    """With the in-launch split-K combine on top (it starts from drained stores): knob 1 = knob 0."""
    import kernels._lib as kl
    tune(GQ_RGEMM=1, GQ_SKINNY=0, GQ_KSTREAM=0, GQ_RGEMM_ILC=1)
    t = kl.GQ_Q8_0
    assert kl.route_name(t, M, N, K) == "rgemm_kernel (in-launch split-K sum)"
    A = _t(random_blocks("q8_0", M, K, seed=M + 1).view(np.int8))
    B = _t(random_activations(N, K, seed=N + 2))
    before = kl.lib().gq_debug_sync_timeouts()
    got = _knob(kl, 1, _raw, t, A, B, M, N, K, "q8_1")
    ref = _knob(kl, 0, _raw, t, A, B, M, N, K, "q8_1")
    assert not torch.isnan(ref).any()
    assert _same(got, ref)
    assert kl.lib().gq_debug_sync_timeouts() == before
