"""Loader and thin torch front end for libgguf_mmq.so (the C ABI in include/gguf_mmq.h).

The library is built in-tree (`make -C gguf-triton-kernel_amd`, or __graft_entry__.build()).
There is no fallback: if the HIP library is missing or no ROCm device is present, the
MMQ entry points raise.
"""
from __future__ import annotations

import ctypes
import os

import torch

from gguf.blocks import BLOCK

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(os.path.dirname(_HERE), "lib")
LIB_PATH = os.path.join(LIB_DIR, "libgguf_mmq.so")

GQ_Q8_0, GQ_Q4_K, GQ_Q6_K, GQ_Q5_K, GQ_Q3_K, GQ_Q2_K, GQ_Q4_0 = 0, 1, 2, 3, 4, 5, 6
GQ_ACT_Q8_1, GQ_ACT_FP8_E4M3 = 0, 1
ACTS = {"q8_1": GQ_ACT_Q8_1, "fp8": GQ_ACT_FP8_E4M3}
TYPES = {"q8_0": GQ_Q8_0, "q4_k": GQ_Q4_K, "q6_k": GQ_Q6_K, "q5_k": GQ_Q5_K, "q3_k": GQ_Q3_K,
         "q2_k": GQ_Q2_K, "q4_0": GQ_Q4_0}
BLOCK_ELEMS = {TYPES[f]: qk for f, (qk, _) in BLOCK.items()}
BLOCK_BYTES = {TYPES[f]: nbytes for f, (_, nbytes) in BLOCK.items()}

# symbol -> (argtypes, restype); mirrors include/gguf_mmq.h
_P, _I64, _I, _SZ = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
GQ_OK, GQ_EINVAL, GQ_EHIP, GQ_EUNSUPPORTED = 0, 1, 2, 3


class GroupItem(ctypes.Structure):
    """gq_group_item (include/gguf_mmq.h)."""
    _fields_ = [("type", ctypes.c_int), ("A", _P), ("B", _P), ("ldb", _I64), ("C", _P), ("ldc", _I64),
                ("M", _I64), ("K", _I64)]


class PrepItem(ctypes.Structure):
    """gq_prep_item (include/gguf_mmq.h)."""
    _fields_ = [("B", _P), ("N", _I64), ("K", _I64), ("ldb", _I64), ("workspace", _P), ("workspace_bytes", _SZ)]


class GemmItem(ctypes.Structure):
    """gq_gemm_item (include/gguf_mmq.h)."""
    _fields_ = [("type", ctypes.c_int), ("A", _P), ("ws", _P), ("C", _P), ("ldc", _I64), ("M", _I64), ("K", _I64)]


class DecodePlan(ctypes.Structure):
    """gq_decode_plan (include/gguf_mmq.h)."""
    _fields_ = [(f, ctypes.c_int32) for f in ("nt", "itc", "img", "fp8", "lds_split", "nseg", "G", "lp2", "grid",
                                              "ngroups", "stash_rows", "tokens", "set", "item", "lds")]


class GemmPlan(ctypes.Structure):
    """gq_gemm_plan (include/gguf_mmq.h)."""
    _fields_ = [(f, ctypes.c_int32) for f in ("kernel", "fmt", "nb", "rg", "am", "nl", "aq", "es", "set", "cwm", "splits",
                                              "chunks_per_split", "pf16", "ilc", "order", "full", "streamk", "tiles_m",
                                              "tiles_n", "blocks", "item")] + \
               [("rows", _I64), ("toks", _I64), ("partial_bytes", ctypes.c_uint64)]


# gq_gemm_plan.kernel (GQ_GK_*)
GEMM_KERNELS = ("none", "rgemm_kernel", "sgemm_kernel", "sgemm_id_kernel", "sgemm_grouped_kernel", "reduce_grouped_kernel",
                "gemm_kernel", "gemm_reduce_f16_kernel", "gemm_reduce_kernel", "skinny_kernel", "kstream_kernel",
                "kstream_reduce_kernel")
GEMM_ENTRIES = {"ex": 0, "prepared": 1, "id_sorted": 2, "grouped_prepared": 3, "grouped_ex": 4}
DECODE_FAMILIES = {"dense": 0, "id": 1, "id_glu": 2, "glu": 3, "grouped": 4}

SIGNATURES = {
    "gq_block_elems": ([_I], _I),
    "gq_block_bytes": ([_I], _I),
    "gq_mmq_workspace_size": ([_I, _I64, _I64, _I64], _SZ),
    "gq_mmq": ([_I, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _P, _SZ, _P], _I),
    "gq_act_prepare": ([_P, _I64, _I64, _I64, _P, _SZ, _P], _I),
    "gq_mmq_prepared": ([_I, _P, _P, _SZ, _P, _I64, _I64, _I64, _I64, _P], _I),
    "gq_quantize_q8_1": ([_P, _P, _I64, _I64, _I64, _P], _I),
    "gq_dequantize": ([_I, _P, _P, _I64, _I64, _I64, _P], _I),
    "gq_mmq_workspace_size_ex": ([_I, _I, _I64, _I64, _I64], _SZ),
    "gq_mmq_call_workspace_size": ([_I, _I, _I64, _I64, _I64], _SZ),
    "gq_mmq_ex": ([_I, _I, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _P, _SZ, _P], _I),
    "gq_act_prepare_ex": ([_I, _P, _I64, _I64, _I64, _P, _SZ, _P], _I),
    "gq_mmq_prepared_ex": ([_I, _I, _P, _P, _SZ, _P, _I64, _I64, _I64, _I64, _P], _I),
    "gq_quantize_fp8": ([_P, _P, _P, _I64, _I64, _I64, _P], _I),
    "gq_quantize_weights": ([_I, _P, _P, _I64, _P], _I),
    "gq_shard_rows": ([_I64, _I, _I, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                       ctypes.POINTER(ctypes.c_int64)], _I),
    "gq_assemble_shards": ([_P, _P, _I, _I64, _I64, _I64, _I64, _P], _I),
    "gq_mmq_sharded_workspace_size": ([_I, _I64, _I64, _I64, _I], _SZ),
    "gq_mmq_sharded": ([_I, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _I, _I, _P, _P, _SZ, _P], _I),
    "gq_mmq_grouped": ([ctypes.POINTER(GroupItem), _I, _I64, _P], _I),
    "gq_mmq_grouped_ex": ([_I, ctypes.POINTER(GroupItem), _I, _I64, _P], _I),
    "gq_mmq_id": ([_I, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _P], _I),
    "gq_mmq_id_sorted_workspace_size": ([_I, _I64, _I64, _I64, _I64, _I64], _SZ),
    "gq_mmq_id_sorted": ([_I, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _P, _SZ, _P], _I),
    "gq_mmq_id_glu": ([_I, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _P], _I),
    "gq_moe_combine": ([_P, _P, _I, _P, _I64, _I64, _I64, _I64, _I64, _P], _I),
    "gq_mmq_glu": ([_I, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _P], _I),
    "gq_moe_combine_shared": ([_P, _P, _I, _P, _I64, _P, _P, _I64, _I64, _I64, _I64, _I64, _P], _I),
    "gq_moe_topk": ([_P, _I64, _P, _I, _I, ctypes.c_float, _P, _P, _I, _I64, _I64, _I64, _P], _I),
    "gq_moe_route": ([_P, _I, _P, _I64, _P, _I64, _P, _I, _I, ctypes.c_float, _P, _P, _I, _I64, _I64, _I64, _I64, _P], _I),
    "gq_rmsnorm": ([_P, _P, _P, _P, ctypes.c_float, _P, _I64, _I64, _I64, _I64, _I64, _I64, _P], _I),
    "gq_rmsnorm_prepare": ([_P, _P, _P, _P, ctypes.c_float, _P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _SZ, _P], _I),
    "gq_act_prepare_grouped": ([_I, ctypes.POINTER(PrepItem), _I, _P], _I),
    "gq_debug_route": ([_I, _I, _I64, _I64, _I64, _I], ctypes.c_char_p),
    "gq_debug_decode_plan": ([_I, _I, ctypes.POINTER(GroupItem), _I, _I64, ctypes.POINTER(DecodePlan), _I], _I),
    "gq_debug_decode_cap": ([_I, _I, _I, _I, _I], _I),
    "gq_debug_gemm_plan": ([_I, _I, ctypes.POINTER(GroupItem), _I, _I64, _I64, _I64, ctypes.POINTER(GemmPlan), _I], _I),
    "gq_mmq_grouped_prepared_workspace_size": ([_I, ctypes.POINTER(GemmItem), _I, _I64], _SZ),
    "gq_mmq_grouped_prepared": ([_I, ctypes.POINTER(GemmItem), _I, _I64, _P, _SZ, _P], _I),
    "gq_last_error": ([], ctypes.c_char_p),
    "gq_version": ([], _I),
    "gq_debug_set_tuning": ([ctypes.c_char_p, ctypes.c_longlong], _I),
    "gq_debug_reset_tuning": ([], None),
    "gq_debug_sync_timeouts": ([], ctypes.c_uint),
}

_lib = None
_call_ws = {}  # (gtype, act, M, N, K) -> bytes one gq_mmq_ex call needs (0: one-launch decode)


def lib():
    """The loaded libgguf_mmq.so (raises RuntimeError when it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build the HIP library first "
                "(make -C gguf-triton-kernel_amd, or python -c 'import __graft_entry__ as g; g.build()')")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = handle
    return _lib


def _bind_mmq_ex():
    """gq_mmq_ex as the eager path calls it: through lib/_gqcall (csrc/gq_pycall.c, a METH_FASTCALL
    entry bound to the ctypes-loaded library's gq_mmq_ex -- ~0.2 us per call instead of ctypes'
    ~1.5-2 us of argument conversion), or the ctypes function when that module was not built.
    Both reach the same gq_mmq_ex in the same loaded libgguf_mmq.so."""
    import importlib.machinery
    import importlib.util
    fn = lib().gq_mmq_ex
    # only a build for THIS interpreter's ABI (lib/ may hold builds for several Pythons)
    for suffix in importlib.machinery.EXTENSION_SUFFIXES:
        path = os.path.join(LIB_DIR, "_gqcall" + suffix)
        if not os.path.exists(path):
            continue
        try:
            spec = importlib.util.spec_from_file_location("_gqcall", path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        except ImportError:
            continue
        mod.bind(ctypes.cast(fn, ctypes.c_void_p).value)
        return mod.mmq_ex
    return fn


def set_tuning(key: str, value: int):
    """Override one GQ_* tuning default by name for later calls (gq_debug_set_tuning; the
    library reads the environment once, so setting os.environ later has no effect)."""
    _call_ws.clear()  # (the workspace a shape needs depends on the tuning)
    _check(lib().gq_debug_set_tuning(key.encode(), int(value)))


def route_name(gtype: int, M: int, N: int, K: int, act: str = "q8_1", prepared: bool = False) -> str:
    """The kernel(s) the library would launch for this call (gq_debug_route)."""
    return lib().gq_debug_route(gtype, ACTS[act], M, N, K, int(prepared)).decode()


def decode_plan(family: str, items, N: int, act: str = "q8_1") -> list:
    """The one-launch decode's plan for a call (gq_debug_decode_plan; host only once GQ_CUS is set):
    a list of DecodePlan, one per (item, token group), empty when the family's entry point would not
    take its one-launch decode.  items: (gtype, M, K) -- one for "dense", "id", "id_glu" (N: the
    pairs) and "glu", the launch's list for "grouped"."""
    arr = (GroupItem * len(items))(*[GroupItem(t, None, None, K, None, M, M, K) for t, M, K in items])
    out = (DecodePlan * 32)()
    n = lib().gq_debug_decode_plan(DECODE_FAMILIES[family], ACTS[act], arr, len(items), N, out, 32)
    return [out[i] for i in range(n)]


def decode_cap(family: str, gtype: int, nt: int, fp8: bool = False, group_set: int = 0) -> int:
    """The most cached chunks a decode kernel of the family exists for (gq_debug_decode_cap), -1: none."""
    return int(lib().gq_debug_decode_cap(DECODE_FAMILIES[family], group_set, gtype, nt, int(fp8)))


def gemm_plan(entry: str, items, N: int, act: str = "q8_1", E: int = 0, S: int = 0) -> list:
    """The GEMM kernels a call would launch (gq_debug_gemm_plan; host only once GQ_CUS is set): a list of
    GemmPlan in launch order, empty when the call takes none of them.  entry: "ex" (gq_mmq_ex),
    "prepared", "id_sorted" (N tokens x S slots on E experts), "grouped_prepared", "grouped_ex";
    items: (gtype, M, K), one for the first three, the launch's list for the grouped entries."""
    arr = (GroupItem * len(items))(*[GroupItem(t, None, None, K, None, M, M, K) for t, M, K in items])
    cap = 48
    while True:  # (the entry counts every launch and writes the first `cap`: asked again when there are more)
        out = (GemmPlan * cap)()
        n = lib().gq_debug_gemm_plan(GEMM_ENTRIES[entry], ACTS[act], arr, len(items), N, E, S, out, cap)
        if n <= cap:
            return [out[i] for i in range(n)]
        cap = n


def reset_tuning():
    """Back to the tuning values the environment gave at first use."""
    _call_ws.clear()
    lib().gq_debug_reset_tuning()


class tuning:
    """Context manager: `with tuning(GQ_GEMM_SPLITS=8, GQ_RGEMM=0): ...` (values reset on exit)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            set_tuning(k, v)
        return self

    def __exit__(self, *exc):
        reset_tuning()
        return False


def _check(status: int):
    if status != 0:
        msg = lib().gq_last_error().decode(errors="replace")
        raise RuntimeError(f"gguf_mmq error {status}: {msg}")


def _require_device(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a ROCm device tensor (got device {t.device}); "
                           "the MMQ kernels have no CPU path")


def workspace_size(gtype: int, M: int, N: int, K: int, act: str = "q8_1") -> int:
    return int(lib().gq_mmq_workspace_size_ex(gtype, ACTS[act], M, N, K))


def _check_weights(gtype: int, A: torch.Tensor, M: int, K: int):
    qk, bb = BLOCK_ELEMS[gtype], BLOCK_BYTES[gtype]
    _require_device(A, "A")
    if A.dtype not in (torch.int8, torch.uint8):
        raise RuntimeError(f"A must be the packed int8/uint8 block tensor, got {A.dtype}")
    if not A.is_contiguous():
        raise RuntimeError("A (packed blocks) must be contiguous")
    if A.numel() != M * (K // qk) * bb:
        raise RuntimeError(f"A has {A.numel()} bytes, expected M*K/{qk}*{bb} = {M * (K // qk) * bb}")


def _check_acts(B: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """B as the fp16 (N, K) unit-column-stride tensor the ABI reads."""
    _require_device(B, "B")
    if B.dtype != torch.float16:
        B = B.to(torch.float16)
    if B.dim() != 2 or B.shape[0] != N or B.shape[1] != K:
        if B.numel() != N * K:
            raise RuntimeError(f"B has {B.numel()} elements, expected N*K = {N * K}")
        B = B.reshape(N, K)
    if B.stride(1) != 1:
        B = B.contiguous()
    return B


def _check_out(out: torch.Tensor | None, N: int, M: int, dev) -> torch.Tensor:
    C = out if out is not None else torch.empty((N, M), dtype=torch.float16, device=dev)
    if C.dtype != torch.float16 or C.dim() != 2 or C.stride(1) != 1 or C.shape[0] != N or C.shape[1] != M:
        raise RuntimeError("out must be an fp16 (N, M) tensor with unit column stride")
    if C.device != dev:
        raise RuntimeError(f"out on {C.device}, expected {dev}")
    return C


def _check_workspace(ws: torch.Tensor, need: int, dev):
    if ws.device != dev or ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise RuntimeError("workspace must be a contiguous uint8 tensor on the weights' device")
    if ws.numel() < need:
        raise RuntimeError(f"workspace has {ws.numel()} bytes, this call needs {need}")


def _stream(dev) -> int:
    """torch's current HIP stream on `dev` (the raw handle: the Stream object costs ~2 us)."""
    return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())


_F16, _I8, _U8 = torch.float16, torch.int8, torch.uint8
_empty, _get_device, _raw_stream = torch.empty, torch._C._cuda_getDevice, torch._C._cuda_getCurrentRawStream
_mmq_ex = None  # the bound gq_mmq_ex (set on first use)


def mmq(gtype: int, A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int,
        out: torch.Tensor | None = None, workspace: torch.Tensor | None = None, act: str = "q8_1") -> torch.Tensor:
    """C = (A @ B^T)^T as fp16 (N, M) on A's device; the common body of mmq_q8_0/q4_k/q6_k.
    act="fp8": the fp8 activation variant (gq_mmq_ex, GQ_ACT_FP8_E4M3) instead of q8_1.
    The common eager form (contiguous device A, fp16 (N, K) B with unit column stride on A's
    device, no out/workspace given) takes a short path: the same checks, fewer Python calls."""
    global _mmq_ex
    if (out is None and workspace is None and A.is_cuda and B.dtype is _F16 and B.dim() == 2 and
            (A.dtype is _I8 or A.dtype is _U8)):
        ns, ks = B.shape
        if ns == N and ks == K and B.stride(1) == 1 and A.is_contiguous() and \
                A.numel() == M * (K // BLOCK_ELEMS[gtype]) * BLOCK_BYTES[gtype]:
            idx = A.get_device()  # (an int: cheaper than building A.device)
            if B.get_device() != idx:
                raise RuntimeError(f"A on {A.device} but B on {B.device}")
            if M == 0 or N == 0:
                return _empty((N, M), dtype=_F16, device=A.device)
            key = (gtype, act, M, N, K)
            need = _call_ws.get(key)
            if need is None:
                need = _call_ws[key] = int(lib().gq_mmq_call_workspace_size(gtype, ACTS[act], M, N, K))
            if _mmq_ex is None:
                _mmq_ex = _bind_mmq_ex()
            if idx == _get_device():
                C = _empty((N, M), dtype=_F16, device=idx)
                if need:
                    ws = _empty(need, dtype=_U8, device=idx)
                    rc = _mmq_ex(gtype, ACTS[act], A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, B.stride(0), M,
                                 ws.data_ptr(), need, _raw_stream(idx))
                else:
                    rc = _mmq_ex(gtype, ACTS[act], A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, B.stride(0), M,
                                 None, 0, _raw_stream(idx))
                if rc:
                    _check(rc)
                return C
    _check_weights(gtype, A, M, K)
    _require_device(B, "B")
    dev = A.device
    if B.device != dev:
        raise RuntimeError(f"A on {dev} but B on {B.device}")
    B = _check_acts(B, N, K)
    C = _check_out(out, N, M, dev)
    if M == 0 or N == 0:
        return C
    key = (gtype, act, M, N, K)
    need = _call_ws.get(key)
    if need is None:
        need = _call_ws[key] = int(lib().gq_mmq_call_workspace_size(gtype, ACTS[act], M, N, K))
    if need and (workspace is None or workspace.numel() < need):
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    wp, wn = (workspace.data_ptr(), workspace.numel()) if need else (None, 0)
    if dev.index == torch.cuda.current_device():
        rc = lib().gq_mmq_ex(gtype, ACTS[act], A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, B.stride(0),
                             C.stride(0), wp, wn, _stream(dev))
    else:
        with torch.cuda.device(dev):
            rc = lib().gq_mmq_ex(gtype, ACTS[act], A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, B.stride(0),
                                 C.stride(0), wp, wn, _stream(dev))
    _check(rc)
    return C


def mmq_grouped(items, N: int, act: str = "q8_1"):
    """One grouped launch (gq_mmq_grouped_ex) for several MMQs with the same token count N:
    items = [(gtype, A, B, M, K, out or None), ...], every B an fp16 (N, K) tensor.  1..4 tokens
    (act="fp8": 1..2): the streaming decode kernel, bit-identical to mmq() per item; 5..32 (fp8:
    3..32): the K-chunked streaming MMQ (K <= 4096, M % 16 == 0), bit-identical to each item's
    call on that kernel.  Returns the (N, M) outputs, or None when the library reports the shapes
    unsupported (N > 32, or an item that is no shape of the launch) -- nothing was launched then
    and the caller runs mmq() per item."""
    if not items:
        return []
    dev = items[0][1].device
    arr = (GroupItem * len(items))()
    outs, keep = [], []
    for i, (gtype, A, B, M, K, out) in enumerate(items):
        _check_weights(gtype, A, M, K)
        if A.device != dev or B.device != dev:
            raise RuntimeError("grouped items must share one device")
        B = _check_acts(B, N, K)
        C = _check_out(out, N, M, dev)
        keep.append(B)
        outs.append(C)
        arr[i] = GroupItem(gtype, A.data_ptr(), B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0), M, K)
    with torch.cuda.device(dev):
        rc = lib().gq_mmq_grouped_ex(ACTS[act], arr, len(items), N, torch.cuda.current_stream(dev).cuda_stream)
    if rc == GQ_EUNSUPPORTED:
        return None
    _check(rc)
    return outs


def pairs_by_expert(ids_np, E: int) -> dict:
    """{expert: indices of the (token, slot) pairs that chose it, ascending} for the flattened
    (N, S) id array; experts no pair chose are absent, ids outside [0, E) are dropped."""
    flat = [int(v) for v in ids_np.reshape(-1)]
    groups = {}
    for p, e in enumerate(flat):
        if 0 <= e < E:
            groups.setdefault(e, []).append(p)
    return groups


def _id_args(gtype: int, A: torch.Tensor, ids: torch.Tensor, B: torch.Tensor, E: int, M: int, K: int,
             out: torch.Tensor | None):
    """The checks and strides mmq_id and mmq_id_sorted share: (B, N, S, per_slot, ldb, ldb_slot, C,
    ldc, ebytes), ldc None when there is nothing to compute."""
    _require_device(A, "A")
    _require_device(ids, "ids")
    _require_device(B, "B")
    qk, bb = BLOCK_ELEMS[gtype], BLOCK_BYTES[gtype]
    if A.dtype not in (torch.int8, torch.uint8) or not A.is_contiguous():
        raise RuntimeError("A must be the contiguous packed int8/uint8 expert tensor")
    ebytes = M * (K // qk) * bb
    if A.numel() != E * ebytes:
        raise RuntimeError(f"A has {A.numel()} bytes, expected E*M*K/{qk}*{bb} = {E * ebytes}")
    if ids.dtype != torch.int32 or ids.dim() != 2 or not ids.is_contiguous():
        raise RuntimeError("ids must be a contiguous (N, S) int32 tensor")
    N, S = ids.shape
    dev = A.device
    if ids.device != dev or B.device != dev:
        raise RuntimeError("A, ids and B must share one device")
    if B.dtype != torch.float16:
        B = B.to(torch.float16)
    if B.dim() == 2 and tuple(B.shape) == (N, K):
        per_slot = False
    elif B.dim() == 3 and tuple(B.shape) == (N, S, K):
        per_slot = True
    else:
        raise RuntimeError(f"B is {tuple(B.shape)}, expected ({N}, {K}) or ({N}, {S}, {K})")
    # the ABI's strides: rows of unit element stride, ldb >= K, ldb_slot >= K (or 0: shared)
    if N * S > 0 and (B.stride(-1) != 1 or (N > 1 and B.stride(0) < K) or
                      (per_slot and S > 1 and B.stride(1) < K)):
        B = B.contiguous()
    ldb = max(B.stride(0), K)
    ldb_slot = max(B.stride(1), K) if per_slot else 0
    C = out if out is not None else torch.empty((N, S, M), dtype=torch.float16, device=dev)
    if C.dtype != torch.float16 or tuple(C.shape) != (N, S, M) or C.device != dev:
        raise RuntimeError(f"out must be an fp16 ({N}, {S}, {M}) tensor on A's device")
    if N * S * M == 0:
        return B, N, S, per_slot, ldb, ldb_slot, C, None, ebytes
    # pair p = n*S + s writes at element p*ldc: rows evenly spaced, ldc >= M apart
    ldc = C.stride(1) if S > 1 else (C.stride(0) if N > 1 else M)
    if (M > 1 and C.stride(2) != 1) or ldc < M or (S > 1 and N > 1 and C.stride(0) != S * ldc):
        raise RuntimeError("out rows must have unit element stride and be evenly spaced, at least M apart")
    return B, N, S, per_slot, ldb, ldb_slot, C, ldc, ebytes


def _id_sorted_call(gtype, A, ids, B, C, E, M, N, S, K, ldb, ldb_slot, ldc) -> int:
    """gq_mmq_id_sorted with its workspace from torch's allocator (inside a graph capture: the
    graph's pool); the status, GQ_EUNSUPPORTED when the entry refuses the shape."""
    need = int(lib().gq_mmq_id_sorted_workspace_size(gtype, E, M, N, S, K))
    if need == 0:
        return GQ_EUNSUPPORTED
    dev = A.device
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return lib().gq_mmq_id_sorted(gtype, A.data_ptr(), ids.data_ptr(), B.data_ptr(), C.data_ptr(), E, M, N, S, K,
                                      ldb, ldb_slot, ldc, ws.data_ptr(), need, _stream(dev))


def mmq_id_sorted(gtype: int, A: torch.Tensor, ids: torch.Tensor, B: torch.Tensor, E: int, M: int, K: int,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """The sorted expert GEMM (gq_mmq_id_sorted): mmq_id's arguments and result at any pair count
    the entry admits (K % 256 == 0, E <= 1024, N*S <= 65536).  Three launches -- a device-side sort
    of the pairs by expert, the activation quantizer gathering through the permutation, the
    streaming GEMM over the (expert, token tile) table -- with no host sync: graph-capturable, a
    replay follows the ids.  Row (n, s) is bit-identical to its row of the streaming GEMM on that
    expert and the expert's gathered rows at one K split, whatever the other ids are; an id
    outside [0, E) gives a zero row.  Raises when the entry refuses the shape (no fallback here)."""
    B, N, S, per_slot, ldb, ldb_slot, C, ldc, ebytes = _id_args(gtype, A, ids, B, E, M, K, out)
    if ldc is None:
        return C
    _check(_id_sorted_call(gtype, A, ids, B, C, E, M, N, S, K, ldb, ldb_slot, ldc))
    return C


def mmq_id(gtype: int, A: torch.Tensor, ids: torch.Tensor, B: torch.Tensor, E: int, M: int, K: int,
           out: torch.Tensor | None = None) -> torch.Tensor:
    """Expert-indexed MMQ (llama.cpp's mul_mat_id): A = E packed (M, K) matrices back to back (a
    GGUF 3-D expert tensor as stored), ids an (N, S) int32 DEVICE tensor of expert choices,
    B fp16 (N, K) -- the S slots of a token share its row (gate / up) -- or (N, S, K) -- one row
    per slot (down).  Returns (N, S, M) fp16; an id outside [0, E) gives a zero row.
    Up to 64 pairs (gq_mmq_id): one launch, row (n, s) bit-identical to
    mmq(gtype, A[expert ids[n, s]], that row, M, 1, K).  Beyond that, or where gq_mmq_id refuses
    the shape otherwise (GQ_EUNSUPPORTED), the sorted expert GEMM (gq_mmq_id_sorted, see
    mmq_id_sorted): pairs that share an expert share one weight stream, at the GEMM paths'
    tolerance.  Both read the ids on the device: no host sync, graph-capturable.
    Only when both refuse (K % 256 != 0 beyond 64 pairs, e.g. Q8_0 at K = 1056; more than 1024
    experts or 65536 pairs) the call falls back to a host-sorted path: the ids are copied to the
    host (this SYNCHRONISES and cannot be captured in a graph), and every expert some pair chose
    runs one mmq() over its pairs' gathered rows."""
    B, N, S, per_slot, ldb, ldb_slot, C, ldc, ebytes = _id_args(gtype, A, ids, B, E, M, K, out)
    if ldc is None:
        return C
    dev = A.device
    with torch.cuda.device(dev):
        rc = lib().gq_mmq_id(gtype, A.data_ptr(), ids.data_ptr(), B.data_ptr(), C.data_ptr(), E, M, N, S, K, ldb,
                             ldb_slot, ldc, _stream(dev))
    if rc == GQ_EUNSUPPORTED:
        rc = _id_sorted_call(gtype, A, ids, B, C, E, M, N, S, K, ldb, ldb_slot, ldc)
    if rc != GQ_EUNSUPPORTED:
        _check(rc)
        return C
    # host-sorted fallback (synchronises: ids.cpu())
    experts = A.reshape(E, ebytes)
    rows = B.reshape(N * S, K) if per_slot else None
    flat = C.view(N * S, M) if C.is_contiguous() else None
    res = flat if flat is not None else torch.empty((N * S, M), dtype=torch.float16, device=dev)
    res.zero_()  # pairs whose id is out of range
    for e, pairs in pairs_by_expert(ids.cpu().numpy(), E).items():
        idx = torch.tensor(pairs, dtype=torch.int64, device=dev)
        x = rows.index_select(0, idx) if per_slot else B.index_select(0, idx // S)
        res.index_copy_(0, idx, mmq(gtype, experts[e], x, M, len(pairs), K))
    if flat is None:
        C.copy_(res.view(N, S, M))
    return C


def glu_torch(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """gq_mmq_id_glu's definition on fp16 g and u with torch ops: fp16(silu(g) * u) in fp32."""
    return (torch.nn.functional.silu(g.float()) * u.float()).half()


def mmq_id_glu(gtype: int, A_gate: torch.Tensor, A_up: torch.Tensor, ids: torch.Tensor, B: torch.Tensor, E: int, M: int,
               K: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Gate and up of every (token, slot) pair with SwiGLU (gq_mmq_id_glu): A_gate and A_up two
    expert tensors of one type, E, M and K (mmq_id's A), ids and B as mmq_id's.  Returns (N, S, M)
    fp16 H = fp16(silu(g) * u), evaluated in fp32 from the fp16 g and u that mmq_id gives for
    A_gate and A_up.  Up to 64 pairs: one launch, the token's row quantized once for both streams.
    Where the entry refuses the shape (GQ_EUNSUPPORTED: more than 64 pairs, a long K) the same
    definition is made from two mmq_id calls and torch ops (mmq_id's own fallbacks apply)."""
    B, N, S, per_slot, ldb, ldb_slot, C, ldc, ebytes = _id_args(gtype, A_gate, ids, B, E, M, K, out)
    _require_device(A_up, "A_up")
    if A_up.dtype not in (torch.int8, torch.uint8) or not A_up.is_contiguous() or A_up.numel() != E * ebytes or \
            A_up.device != A_gate.device:
        raise RuntimeError("A_up must be a packed expert tensor of A_gate's type, E, M, K and device")
    if ldc is None:
        return C
    dev = A_gate.device
    with torch.cuda.device(dev):
        rc = lib().gq_mmq_id_glu(gtype, A_gate.data_ptr(), A_up.data_ptr(), ids.data_ptr(), B.data_ptr(), C.data_ptr(), E,
                                 M, N, S, K, ldb, ldb_slot, ldc, _stream(dev))
    if rc == GQ_EUNSUPPORTED:
        C.copy_(glu_torch(mmq_id(gtype, A_gate, ids, B, E, M, K), mmq_id(gtype, A_up, ids, B, E, M, K)))
        return C
    _check(rc)
    return C


def moe_combine(D: torch.Tensor, W: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """The router-weighted sum over slots (gq_moe_combine): D fp16 (N, S, M), W (N, S) fp16 or fp32
    -> fp16 (N, M), Y[n] = fp16(sum_s W[n, s] * D[n, s]) with the products and the sum in fp32 in
    slot order, unfused -- one launch, deterministic.  More than 64 slots: the same definition
    with torch ops."""
    _require_device(D, "D")
    _require_device(W, "W")
    if D.dtype != torch.float16 or D.dim() != 3:
        raise RuntimeError("D must be an fp16 (N, S, M) tensor")
    N, S, M = D.shape
    if tuple(W.shape) != (N, S) or W.device != D.device:
        raise RuntimeError(f"W is {tuple(W.shape)} on {W.device}, expected ({N}, {S}) on {D.device}")
    if W.dtype not in (torch.float16, torch.float32):
        W = W.float()
    W = W.contiguous()
    Y = _check_out(out, N, M, D.device)
    if N * S * M == 0:
        if S == 0:
            Y.zero_()
        return Y
    ldd = D.stride(1) if S > 1 else (D.stride(0) if N > 1 else M)
    if (M > 1 and D.stride(2) != 1) or ldd < M or (S > 1 and N > 1 and D.stride(0) != S * ldd):
        D = D.contiguous()
        ldd = M
    dev = D.device
    with torch.cuda.device(dev):
        rc = lib().gq_moe_combine(D.data_ptr(), W.data_ptr(), int(W.dtype == torch.float32), Y.data_ptr(), N, S, M, ldd,
                                  Y.stride(0) if N > 1 else max(Y.stride(0), M), _stream(dev))
    if rc == GQ_EUNSUPPORTED:
        acc = torch.zeros((N, M), dtype=torch.float32, device=dev)
        for s in range(S):
            acc = acc + W[:, s, None].float() * D[:, s].float()
        Y.copy_(acc.half())
        return Y
    _check(rc)
    return Y


def mmq_glu(gtype: int, A_gate: torch.Tensor, A_up: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """Dense gate and up with SwiGLU (gq_mmq_glu): A_gate and A_up two packed (M, K) weights of one
    type (mmq's A), B fp16 (N, K).  Returns (N, M) fp16 H = fp16(silu(g) * u), evaluated in fp32
    from the fp16 g and u that mmq gives for A_gate and A_up at this N.  1..4 tokens where mmq's
    route is the one-launch decode: one launch, the tokens quantized once for both weight streams.
    Where the entry refuses the shape (GQ_EUNSUPPORTED: more than 4 tokens, a long K, a kernel that
    is not built) the same definition is made from two mmq calls and torch ops."""
    _check_weights(gtype, A_gate, M, K)
    _check_weights(gtype, A_up, M, K)
    _require_device(B, "B")
    dev = A_gate.device
    if A_up.device != dev or B.device != dev:
        raise RuntimeError(f"A_gate on {dev} but A_up on {A_up.device} and B on {B.device}")
    B = _check_acts(B, N, K)
    C = _check_out(out, N, M, dev)
    if M == 0 or N == 0:
        return C
    if N > 1 and B.stride(0) < K:
        B = B.contiguous()
    with torch.cuda.device(dev):
        rc = lib().gq_mmq_glu(gtype, A_gate.data_ptr(), A_up.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K,
                              max(B.stride(0), K), max(C.stride(0), M), _stream(dev))
    if rc == GQ_EUNSUPPORTED:
        C.copy_(glu_torch(mmq(gtype, A_gate, B, M, N, K), mmq(gtype, A_up, B, M, N, K)))
        return C
    _check(rc)
    return C


def moe_combine_shared(D: torch.Tensor, W: torch.Tensor, Dsh: torch.Tensor, gate: torch.Tensor | None = None,
                       out: torch.Tensor | None = None) -> torch.Tensor:
    """moe_combine plus a shared expert's term (gq_moe_combine_shared): D fp16 (N, S, M), W (N, S)
    fp16 or fp32, Dsh fp16 (N, M) the shared expert's down output, gate None or N fp32 values (a
    per-token gate of the shared term) -> fp16 (N, M),
    Y[n] = fp16((sum_s W[n, s] * D[n, s]) + gate[n] * Dsh[n]) with every product and sum in fp32, the
    slots in order and the shared term last, unfused -- one launch, deterministic.  More than 64
    slots: the same definition with torch ops."""
    _require_device(D, "D")
    _require_device(W, "W")
    _require_device(Dsh, "Dsh")
    if D.dtype != torch.float16 or D.dim() != 3:
        raise RuntimeError("D must be an fp16 (N, S, M) tensor")
    N, S, M = D.shape
    dev = D.device
    if S < 1:
        raise RuntimeError("moe_combine_shared needs at least one slot")
    if tuple(W.shape) != (N, S) or W.device != dev:
        raise RuntimeError(f"W is {tuple(W.shape)} on {W.device}, expected ({N}, {S}) on {dev}")
    if Dsh.dtype != torch.float16 or tuple(Dsh.shape) != (N, M) or Dsh.device != dev:
        raise RuntimeError(f"Dsh must be an fp16 ({N}, {M}) tensor on {dev}")
    if gate is not None:
        _require_device(gate, "gate")
        if gate.numel() != N or gate.device != dev:
            raise RuntimeError(f"gate has {gate.numel()} elements on {gate.device}, expected {N} on {dev}")
        gate = gate.reshape(N).to(torch.float32).contiguous()
    if W.dtype not in (torch.float16, torch.float32):
        W = W.float()
    W = W.contiguous()
    Y = _check_out(out, N, M, dev)
    if N * M == 0:
        return Y
    ldd = D.stride(1) if S > 1 else (D.stride(0) if N > 1 else M)
    if (M > 1 and D.stride(2) != 1) or ldd < M or (S > 1 and N > 1 and D.stride(0) != S * ldd):
        D = D.contiguous()
        ldd = M
    if (M > 1 and Dsh.stride(1) != 1) or (N > 1 and Dsh.stride(0) < M):
        Dsh = Dsh.contiguous()
    with torch.cuda.device(dev):
        rc = lib().gq_moe_combine_shared(D.data_ptr(), W.data_ptr(), int(W.dtype == torch.float32), Dsh.data_ptr(),
                                         max(Dsh.stride(0), M), gate.data_ptr() if gate is not None else None,
                                         Y.data_ptr(), N, S, M, ldd, max(Y.stride(0), M), _stream(dev))
    if rc == GQ_EUNSUPPORTED:
        acc = torch.zeros((N, M), dtype=torch.float32, device=dev)
        for s in range(S):
            acc = acc + W[:, s, None].float() * D[:, s].float()
        acc = acc + (Dsh.float() if gate is None else gate[:, None] * Dsh.float())
        Y.copy_(acc.half())
        return Y
    _check(rc)
    return Y


GATING = {"softmax": 0, "sigmoid": 1}


def moe_topk_torch(logits, S, bias=None, func="softmax", norm=True, scale=1.0, w_dtype=torch.float32):
    """gq_moe_topk's definition with torch ops, for the shapes the entry refuses (E > 1024, S > 64):
    keys (the logits; sigmoid + bias when a bias is given), a stable descending sort (the lower
    index first among equal keys; a NaN key is ranked with -inf), the values (softmax over all E,
    or sigmoid) gathered at the S first ids, optionally divided by their sum, times scale.  Several
    launches, no host sync."""
    L = logits.float()
    s = torch.sigmoid(L) if func == "sigmoid" else None
    key = L if bias is None else s + bias.float()
    key = torch.where(torch.isnan(key), torch.full_like(key, float("-inf")), key)
    ids = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :S]
    v = (torch.softmax(L, dim=1) if func == "softmax" else s).gather(1, ids)
    if norm:
        v = v / v.sum(1, keepdim=True)
    return ids.to(torch.int32), (v * scale).to(w_dtype)


def _route_args(S, E, N, bias, func, w_dtype, out, dev, n_out):
    if func not in GATING:
        raise ValueError(f"func is {func!r}, expected 'softmax' or 'sigmoid'")
    if bias is not None:
        if func != "sigmoid":
            raise ValueError("a selection bias goes with sigmoid gating only")
        if bias.device != dev or bias.numel() != E:
            raise RuntimeError(f"bias has {bias.numel()} elements on {bias.device}, expected {E} on {dev}")
        bias = bias.to(torch.float32).contiguous()
    if w_dtype not in (torch.float32, torch.float16):
        raise ValueError("w_dtype is torch.float32 or torch.float16")
    if not 1 <= S <= E:
        raise ValueError(f"S={S} outside 1..E={E}")
    if out is None:
        out = (torch.empty((N, S), dtype=torch.int32, device=dev), torch.empty((N, S), dtype=w_dtype, device=dev),
               torch.empty((N, E), dtype=torch.float32, device=dev))[:n_out]
    if len(out) != n_out:
        raise RuntimeError(f"out must hold {n_out} tensors")
    ids, W = out[0], out[1]
    if ids.dtype != torch.int32 or tuple(ids.shape) != (N, S) or not ids.is_contiguous() or ids.device != dev:
        raise RuntimeError(f"out ids must be a contiguous int32 ({N}, {S}) tensor on {dev}")
    if W.dtype != w_dtype or tuple(W.shape) != (N, S) or not W.is_contiguous() or W.device != dev:
        raise RuntimeError(f"out weights must be a contiguous {w_dtype} ({N}, {S}) tensor on {dev}")
    if n_out == 3:
        lg = out[2]
        if lg.dtype != torch.float32 or tuple(lg.shape) != (N, E) or lg.device != dev or (E > 1 and lg.stride(1) != 1) or \
                (N > 1 and lg.stride(0) < E):
            raise RuntimeError(f"out logits must be an fp32 ({N}, {E}) tensor on {dev} with unit column stride")
    return bias, out


def moe_topk(logits: torch.Tensor, S: int, bias: torch.Tensor | None = None, func: str = "softmax", norm: bool = True,
             scale: float = 1.0, w_dtype=torch.float32, out=None):
    """The router's selection (gq_moe_topk): logits fp32 (N, E) -> (ids int32 (N, S), weights (N, S)
    of w_dtype, fp32 or fp16).  Token n's ids are the S experts of largest key in descending order,
    the lower index first on ties -- key = the logit, or with func="sigmoid" and a bias (E fp32)
    sigmoid(logit) + bias; the weights are softmax(logits) over all E (func="softmax") or
    sigmoid(logit) at the chosen ids, divided by their sum when norm, times scale.  One launch at
    any N, deterministic, no host sync.  out = (ids, weights) to write into.  Only E > 1024 or
    S > 64 (GQ_EUNSUPPORTED) takes moe_topk_torch, the same definition in torch ops."""
    _require_device(logits, "logits")
    if logits.dim() != 2:
        raise RuntimeError("logits must be an (N, E) tensor")
    if logits.dtype != torch.float32:
        logits = logits.float()
    N, E = logits.shape
    if (E > 1 and logits.stride(1) != 1) or (N > 1 and logits.stride(0) < E):
        logits = logits.contiguous()
    dev = logits.device
    bias, (ids, W) = _route_args(S, E, N, bias, func, w_dtype, out, dev, 2)
    if N == 0:
        return ids, W
    with torch.cuda.device(dev):
        rc = lib().gq_moe_topk(logits.data_ptr(), logits.stride(0) if N > 1 else max(logits.stride(0), E),
                               bias.data_ptr() if bias is not None else None, GATING[func], int(bool(norm)), float(scale),
                               ids.data_ptr(), W.data_ptr(), int(w_dtype == torch.float32), N, E, S, _stream(dev))
    if rc == GQ_EUNSUPPORTED:
        i, w = moe_topk_torch(logits, S, bias, func, norm, scale, w_dtype)
        ids.copy_(i)
        W.copy_(w)
        return ids, W
    _check(rc)
    return ids, W


def moe_route(Wr: torch.Tensor, x: torch.Tensor, S: int, bias: torch.Tensor | None = None, func: str = "softmax",
              norm: bool = True, scale: float = 1.0, w_dtype=torch.float32, out=None):
    """The router of a MoE block (gq_moe_route): Wr the (E, H) router matrix, fp32 or fp16, x fp16
    (N, H) -> (ids, weights, logits): logits = x @ Wr^T accumulated in fp32, stored as fp32 (N, E),
    and moe_topk's selection on exactly those stored values.  Two launches, no host sync; a token's
    logits, ids and weights are the bits of its own one-token call.  out = (ids, weights, logits).
    Where the entry refuses the product (GQ_EUNSUPPORTED: more than 64 tokens, H % 32 != 0) the
    logits are torch.matmul(x.float(), Wr.float().T) and moe_topk does the rest."""
    _require_device(Wr, "Wr")
    _require_device(x, "x")
    if Wr.dim() != 2 or Wr.dtype not in (torch.float32, torch.float16):
        raise RuntimeError("Wr must be an fp32 or fp16 (E, H) tensor")
    E, H = Wr.shape
    dev = Wr.device
    if x.device != dev:
        raise RuntimeError(f"Wr on {dev} but x on {x.device}")
    if x.dim() != 2 or x.shape[1] != H:
        raise RuntimeError(f"x is {tuple(x.shape)}, expected (N, {H})")
    if x.dtype != torch.float16:
        x = x.to(torch.float16)
    N = x.shape[0]
    if (H > 1 and x.stride(1) != 1) or (N > 1 and x.stride(0) < H):
        x = x.contiguous()
    Wr = Wr.contiguous()
    bias, (ids, W, logits) = _route_args(S, E, N, bias, func, w_dtype, out, dev, 3)
    if N == 0:
        return ids, W, logits
    def entry():
        return lib().gq_moe_route(Wr.data_ptr(), int(Wr.dtype == torch.float16), x.data_ptr(),
                                  x.stride(0) if N > 1 else max(x.stride(0), H), logits.data_ptr(),
                                  logits.stride(0) if N > 1 else max(logits.stride(0), E),
                                  bias.data_ptr() if bias is not None else None, GATING[func], int(bool(norm)),
                                  float(scale), ids.data_ptr(), W.data_ptr(), int(w_dtype == torch.float32), N, E, H, S,
                                  _stream(dev))

    with torch.cuda.device(dev):
        rc = entry()
    if rc == GQ_EUNSUPPORTED:
        logits.copy_(torch.matmul(x.float(), Wr.float().T))
        moe_topk(logits, S, bias, func, norm, scale, w_dtype, out=(ids, W))
        # (moe_topk's own call reset the thread's error text: the refused entry is asked again -- it
        # answers from its host-side checks, launching nothing -- so that gq_last_error() still says
        # why this call took the torch product)
        with torch.cuda.device(dev):
            entry()
        return ids, W, logits
    _check(rc)
    return ids, W, logits


def mmq_grouped_prepared(items, N: int, act: str = "q8_1"):
    """One grouped streaming-GEMM launch (gq_mmq_grouped_prepared) for several prepared MMQs with
    the same token count N: items = [(gtype, A, ws, M, K, out or None), ...], ws the workspace the
    item's input was prepared into (act_prepare / act_prepare_grouped with this N, K, act).
    Returns the (N, M) outputs, or None when the library reports the shapes unsupported (N < 5,
    K % 256 != 0, > 16 items): nothing was launched then, call mmq_prepared per item."""
    if not items:
        return []
    dev = items[0][1].device
    arr = (GemmItem * len(items))()
    outs = []
    for i, (gtype, A, ws, M, K, out) in enumerate(items):
        _check_weights(gtype, A, M, K)
        if A.device != dev or ws.device != dev:
            raise RuntimeError("grouped items must share one device")
        C = _check_out(out, N, M, dev)
        outs.append(C)
        arr[i] = GemmItem(gtype, A.data_ptr(), ws.data_ptr(), C.data_ptr(), C.stride(0), M, K)
    need = int(lib().gq_mmq_grouped_prepared_workspace_size(ACTS[act], arr, len(items), N))
    part = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    with torch.cuda.device(dev):
        rc = lib().gq_mmq_grouped_prepared(ACTS[act], arr, len(items), N, part.data_ptr() if need else None, need,
                                           torch.cuda.current_stream(dev).cuda_stream)
    if rc == GQ_EUNSUPPORTED:
        return None
    _check(rc)
    return outs


def quantize_q8_1_device(X: torch.Tensor) -> torch.Tensor:
    """Device q8_1 quantizer (bit-exact with utils/quantize/q8_1.py) -> flat int8 bytes."""
    _require_device(X, "X")
    if X.dtype != torch.float16:
        X = X.to(torch.float16)
    X2 = X.reshape(-1, X.shape[-1]) if X.dim() > 1 else X.reshape(1, -1)
    if X2.stride(-1) != 1:
        X2 = X2.contiguous()
    rows, K = X2.shape
    if K % 32 != 0:
        raise ValueError("The total number of elements must be divisible by 32.")
    Y = torch.empty(rows * (K // 32) * 36, dtype=torch.int8, device=X.device)
    with torch.cuda.device(X.device):
        stream = torch.cuda.current_stream(X.device).cuda_stream
        _check(lib().gq_quantize_q8_1(X2.data_ptr(), Y.data_ptr(), rows, K, X2.stride(0), stream))
    return Y


def dequantize_device(gtype: int, A: torch.Tensor, M: int, K: int) -> torch.Tensor:
    """fp16 (M, K) weights from packed blocks on the device (gq_dequantize)."""
    _require_device(A, "A")
    qk, bb = BLOCK_ELEMS[gtype], BLOCK_BYTES[gtype]
    if A.numel() != M * (K // qk) * bb:
        raise RuntimeError(f"A has {A.numel()} bytes, expected {M * (K // qk) * bb}")
    W = torch.empty((M, K), dtype=torch.float16, device=A.device)
    with torch.cuda.device(A.device):
        stream = torch.cuda.current_stream(A.device).cuda_stream
        _check(lib().gq_dequantize(gtype, A.data_ptr(), W.data_ptr(), M, K, K, stream))
    return W


def act_prepare(B: torch.Tensor, N: int, K: int, workspace: torch.Tensor, act: str = "q8_1"):
    """Quantize the activations once into the front of `workspace` (gq_act_prepare_ex); any
    number of mmq_prepared calls with the same (N, K, act) then reuse them."""
    B = _check_acts(B, N, K)
    _check_workspace(workspace, 0, B.device)
    with torch.cuda.device(B.device):
        stream = torch.cuda.current_stream(B.device).cuda_stream
        _check(lib().gq_act_prepare_ex(ACTS[act], B.data_ptr(), N, K, B.stride(0), workspace.data_ptr(),
                                       workspace.numel(), stream))


def act_prepare_grouped(items, act: str = "q8_1"):
    """Several act_prepare calls in as few launches as possible (gq_act_prepare_grouped):
    items = [(B, N, K, workspace), ...] -- each workspace gets exactly what act_prepare would
    write; one launch per 8 items whose form is the GEMM paths' fp16 x~ (q8_1 at N >= 5; the fp8
    variant's widened codes at every N)."""
    if not items:
        return
    dev = items[0][0].device
    arr = (PrepItem * len(items))()
    keep = []
    for i, (B, N, K, ws) in enumerate(items):
        B = _check_acts(B, N, K)
        _check_workspace(ws, 0, B.device)
        if B.device != dev:
            raise RuntimeError("grouped items must share one device")
        keep.append(B)
        arr[i] = PrepItem(B.data_ptr(), N, K, B.stride(0), ws.data_ptr(), ws.numel())
    with torch.cuda.device(dev):
        _check(lib().gq_act_prepare_grouped(ACTS[act], arr, len(items), torch.cuda.current_stream(dev).cuda_stream))


def _norm_rows(t: torch.Tensor | None, name: str, N: int, K: int, dev, out: bool = False):
    """An fp16 (N, K) tensor of the norm entries with unit column stride and rows >= K apart:
    (tensor, ld); an input of another layout is copied, an output must have it."""
    if t is None:
        return None, K
    _require_device(t, name)
    if t.device != dev:
        raise RuntimeError(f"{name} on {t.device}, expected {dev}")
    ok = t.dtype == torch.float16 and t.dim() == 2 and tuple(t.shape) == (N, K) and (K <= 1 or t.stride(1) == 1) and \
        (N <= 1 or t.stride(0) >= K)
    if not ok:
        if out:
            raise RuntimeError(f"{name} must be an fp16 ({N}, {K}) tensor with unit column stride and rows at least K apart")
        if t.dim() != 2 or tuple(t.shape) != (N, K):
            raise RuntimeError(f"{name} is {tuple(t.shape)}, expected ({N}, {K})")
        t = t.to(torch.float16).contiguous()
    return t, (t.stride(0) if N > 1 else max(t.stride(0), K))


def _norm_args(x, w, eps, residual, y, h_out, need_y: bool):
    _require_device(x, "x")
    if x.dim() != 2:
        raise RuntimeError("x must be an (N, K) tensor")
    N, K = x.shape
    dev = x.device
    if K % 32 != 0:
        raise RuntimeError(f"K={K} is not a multiple of 32")
    _require_device(w, "w")
    if w.device != dev or w.dtype != torch.float32 or w.numel() != K or not w.is_contiguous():
        raise RuntimeError(f"w must hold K = {K} contiguous fp32 values on {dev}")
    x, ldx = _norm_rows(x, "x", N, K, dev)
    r, ldr = _norm_rows(residual, "residual", N, K, dev)
    if y is None and need_y:
        y = torch.empty((N, K), dtype=torch.float16, device=dev)
    y, ldy = _norm_rows(y, "out", N, K, dev, out=True)
    h, ldh = _norm_rows(h_out, "h_out", N, K, dev, out=True)
    return x, ldx, r, ldr, y, ldy, h, ldh, N, K, dev


def _ptr(t):
    return t.data_ptr() if t is not None else None


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, residual: torch.Tensor | None = None,
            out: torch.Tensor | None = None, h_out: torch.Tensor | None = None) -> torch.Tensor:
    """Residual add + RMSNorm in one launch (gq_rmsnorm): x fp16 (N, K), w K fp32 values ->
    y = fp16((h / sqrt(mean(h^2) + eps)) * w) with h = fp16(x + residual) (h = x without a residual).
    h_out: an fp16 (N, K) tensor that receives h, the new residual stream; it may be x or residual
    themselves (the in-place update).  Returns y (out, when given).  No host sync, no fallback."""
    x, ldx, r, ldr, y, ldy, h, ldh, N, K, dev = _norm_args(x, w, eps, residual, out, h_out, True)
    if N * K == 0:
        return y
    with torch.cuda.device(dev):
        _check(lib().gq_rmsnorm(x.data_ptr(), _ptr(r), _ptr(h), w.data_ptr(), float(eps), y.data_ptr(), N, K, ldx, ldr,
                                ldh, ldy, _stream(dev)))
    return y


def rmsnorm_prepare(x: torch.Tensor, w: torch.Tensor, eps: float, workspace: torch.Tensor,
                    residual: torch.Tensor | None = None, y_out: torch.Tensor | None = None,
                    h_out: torch.Tensor | None = None):
    """rmsnorm whose y is left in `workspace` as act_prepare(y, N, K, workspace) would leave it
    (gq_rmsnorm_prepare, q8_1 activations): one launch, then any number of mmq_prepared calls with
    this (N, K).  y_out: an fp16 (N, K) tensor that also receives y; h_out as rmsnorm's.  Where the
    library writes the int8 GEMM form too (the GQ_GEMM_I8 tuning) and no y_out was given, the two
    steps run here: rmsnorm into a temporary, then act_prepare -- the same bytes.  Returns y_out."""
    x, ldx, r, ldr, y, ldy, h, ldh, N, K, dev = _norm_args(x, w, eps, residual, y_out, h_out, False)
    _check_workspace(workspace, 0, dev)
    if N * K == 0:
        return y
    with torch.cuda.device(dev):
        rc = lib().gq_rmsnorm_prepare(x.data_ptr(), _ptr(r), _ptr(h), w.data_ptr(), float(eps), _ptr(y), N, K, ldx, ldr,
                                      ldh, ldy, workspace.data_ptr(), workspace.numel(), _stream(dev))
    if rc == GQ_EUNSUPPORTED and y is None:
        act_prepare(rmsnorm(x, w, eps, r, None, h), N, K, workspace)
        return None
    _check(rc)
    return y


def mmq_prepared(gtype: int, A: torch.Tensor, workspace: torch.Tensor, M: int, N: int, K: int,
                 out: torch.Tensor | None = None, act: str = "q8_1") -> torch.Tensor:
    """C (N, M) fp16 from packed A and the activations act_prepare left in `workspace`."""
    _check_weights(gtype, A, M, K)
    _check_workspace(workspace, workspace_size(gtype, M, N, K, act), A.device)
    C = _check_out(out, N, M, A.device)
    if M == 0 or N == 0:
        return C
    with torch.cuda.device(A.device):
        stream = torch.cuda.current_stream(A.device).cuda_stream
        _check(lib().gq_mmq_prepared_ex(gtype, ACTS[act], A.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                        C.data_ptr(), M, N, K, C.stride(0), stream))
    return C


def quantize_weights_device(fmt: str, X: torch.Tensor) -> torch.Tensor:
    """GGUF weight quantization on the device (gq_quantize_weights): the bytes of
    utils.quantize.quantize_to_<fmt> (int8, flat), from an fp16 (q8_0) or fp32 (q4_k, q6_k, q4_0)
    device tensor read as flat blocks."""
    want = torch.float16 if fmt == "q8_0" else torch.float32
    if not X.is_cuda or X.dtype != want:
        raise RuntimeError(f"quantize_weights_device({fmt}) needs a {want} device tensor")
    X = X.contiguous().reshape(-1)
    qk, nbytes = BLOCK[fmt]
    if X.numel() % qk:
        raise RuntimeError(f"{X.numel()} elements are not whole {fmt} blocks")
    out = torch.empty(X.numel() // qk * nbytes, dtype=torch.int8, device=X.device)
    with torch.cuda.device(X.device):
        _check(lib().gq_quantize_weights(TYPES[fmt], X.data_ptr(), out.data_ptr(), X.numel(),
                                         torch.cuda.current_stream(X.device).cuda_stream))
    return out


def quantize_fp8_device(X: torch.Tensor):
    """The fp8 variant's activation quantizer (gq_quantize_fp8) -> (codes uint8 (rows, K) in the
    (0,2,1,3) group order, scales float32 (K/32, (rows+3)&~3))."""
    _require_device(X, "X")
    X2 = X.to(torch.float16).reshape(-1, X.shape[-1]).contiguous()
    rows, K = X2.shape
    codes = torch.empty((rows, K), dtype=torch.uint8, device=X.device)
    scales = torch.empty((K // 32, (rows + 3) & ~3), dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        stream = torch.cuda.current_stream(X.device).cuda_stream
        _check(lib().gq_quantize_fp8(X2.data_ptr(), codes.data_ptr(), scales.data_ptr(), rows, K, X2.stride(0),
                                     stream))
    return codes, scales


def shard_rows(M: int, world: int, rank: int):
    """(row0, rows, R) of rank `rank` (gq_shard_rows; the rule of dist/row_shard.shard_rows)."""
    r0, rows, R = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _check(lib().gq_shard_rows(M, world, rank, ctypes.byref(r0), ctypes.byref(rows), ctypes.byref(R)))
    return r0.value, rows.value, R.value


def assemble_shards(gathered: torch.Tensor, M: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """(world, N, R) fp16 slabs -> (N, M) on the device (gq_assemble_shards)."""
    _require_device(gathered, "gathered")
    if gathered.dtype != torch.float16 or gathered.dim() != 3 or not gathered.is_contiguous():
        raise RuntimeError("gathered must be a contiguous (world, N, R) fp16 tensor")
    W, N, R = gathered.shape
    C = _check_out(out, N, M, gathered.device)
    with torch.cuda.device(gathered.device):
        stream = torch.cuda.current_stream(gathered.device).cuda_stream
        _check(lib().gq_assemble_shards(gathered.data_ptr(), C.data_ptr(), W, N, R, M, C.stride(0), stream))
    return C


def mmq_sharded_single(gtype: int, A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int) -> torch.Tensor:
    """gq_mmq_sharded at world 1 (no communicator): the C-ABI sharded entry point end to end on
    one device (multi-rank callers pass their own RCCL communicator through the C ABI)."""
    _require_device(A, "A")
    _check_weights(gtype, A, M, K)
    B = _check_acts(B, N, K)
    C = _check_out(None, N, M, A.device)
    need = int(lib().gq_mmq_sharded_workspace_size(gtype, M, N, K, 1))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=A.device)
    with torch.cuda.device(A.device):
        stream = torch.cuda.current_stream(A.device).cuda_stream
        _check(lib().gq_mmq_sharded(gtype, A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, B.stride(0), C.stride(0),
                                    1, 0, None, ws.data_ptr(), ws.numel(), stream))
    return C

