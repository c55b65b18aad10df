"""Host side of the sorted expert GEMM (gq_mmq_id_sorted, mixture-of-experts prefill): the header,
the library and kernels._lib.SIGNATURES agree on the two entries; the workspace size; the
argument checks (fake pointers: every case returns before a launch).  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
NAMES = ["t", "A", "ids", "B", "C", "E", "M", "N", "S", "K", "ldb", "ldb_slot", "ldc", "workspace", "workspace_bytes",
         "stream"]


def _protos():
    text = open(os.path.join(ROOT, "include", "gguf_mmq.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    size = re.search(r"size_t\s+gq_mmq_id_sorted_workspace_size\s*\(([^)]*)\)\s*;", text)
    call = re.search(r"int\s+gq_mmq_id_sorted\s*\(([^)]*)\)\s*;", text)
    return size, call


def test_entries_declared_exported_bound():
    import kernels._lib as kl
    size, call = _protos()
    assert size, "include/gguf_mmq.h does not declare gq_mmq_id_sorted_workspace_size"
    assert call, "include/gguf_mmq.h does not declare gq_mmq_id_sorted"
    args = [a.strip() for a in call.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == NAMES
    assert args[2].replace(" ", "") == "constint32_t*ids"
    assert [a.split()[-1] for a in size.group(1).split(",")] == ["t", "E", "M", "N", "S", "K"]
    L = kl.lib()
    assert hasattr(L, "gq_mmq_id_sorted") and hasattr(L, "gq_mmq_id_sorted_workspace_size")
    argtypes, restype = kl.SIGNATURES["gq_mmq_id_sorted"]
    assert len(argtypes) == 16 and restype is ctypes.c_int
    assert argtypes[0] is ctypes.c_int and argtypes[14] is ctypes.c_size_t
    assert all(a is ctypes.c_void_p for a in argtypes[1:5] + [argtypes[13], argtypes[15]])
    assert all(a is ctypes.c_int64 for a in argtypes[5:13])
    argtypes, restype = kl.SIGNATURES["gq_mmq_id_sorted_workspace_size"]
    assert argtypes == [ctypes.c_int] + [ctypes.c_int64] * 5 and restype is ctypes.c_size_t
    assert L.gq_version() == 105  # (the entries are detected by their symbols)


def test_workspace_size():
    import kernels._lib as kl
    size = kl.lib().gq_mmq_id_sorted_workspace_size
    E, M, K = 8, 512, 1024
    last = 0
    for N, S in ((5, 1), (33, 2), (40, 8), (512, 2), (8192, 8)):
        b = size(kl.GQ_Q4_K, E, M, N, S, K)
        assert b >= N * S * K * 2, (N, S, b)
        assert b > last, (N, S, b, last)  # grows with N*S
        last = b
    for t in (kl.GQ_Q8_0, kl.GQ_Q6_K, kl.GQ_Q5_K):
        assert size(t, E, M, 40, 8, K) >= 320 * K * 2
    # nothing to do, or a shape the entry refuses: 0
    assert size(kl.GQ_Q4_K, E, M, 0, 2, K) == 0
    assert size(kl.GQ_Q4_K, E, M, 4, 0, K) == 0
    assert size(kl.GQ_Q4_K, E, 0, 4, 2, K) == 0
    assert size(kl.GQ_Q8_0, E, M, 4, 2, 1056) == 0


def _caller(L, ws_bytes=None):
    p = ctypes.c_void_p(16)

    def call(t=1, A=p, ids=p, B=p, C=p, E=4, M=8, N=40, S=2, K=256, ldb=256, ldb_slot=0, ldc=8, ws=p, ws_bytes=ws_bytes):
        if ws_bytes is None:
            ws_bytes = L.gq_mmq_id_sorted_workspace_size(t, E, M, N, S, K)
        return L.gq_mmq_id_sorted(t, A, ids, B, C, E, M, N, S, K, ldb, ldb_slot, ldc, ws, ws_bytes, None)
    return call


def test_einval():
    import kernels._lib as kl
    L = kl.lib()
    call = _caller(L)
    assert call(K=100, ldb=100) == EINVAL  # K not a multiple of the block
    for name in ("A", "ids", "B", "C"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null" in L.gq_last_error()
    assert call(ldb=255) == EINVAL
    assert call(ldc=7) == EINVAL
    for slot in (1, 128, 255):
        assert call(ldb_slot=slot) == EINVAL, slot
        assert b"ldb_slot" in L.gq_last_error()
    need = L.gq_mmq_id_sorted_workspace_size(1, 4, 8, 40, 2, 256)
    assert need >= 80 * 256 * 2
    assert call(ws=None) == EINVAL
    assert b"workspace" in L.gq_last_error()
    assert call(ws_bytes=need - 1) == EINVAL
    assert b"workspace" in L.gq_last_error()
    assert call(ws_bytes=0) == EINVAL


def test_eunsupported():
    import kernels._lib as kl
    L = kl.lib()
    call = _caller(L, ws_bytes=1 << 40)
    assert call(t=0, K=1056, ldb=1056) == EUNSUPPORTED  # Q8_0: whole blocks, not whole super-blocks
    assert b"256" in L.gq_last_error()
    assert call(E=1025) == EUNSUPPORTED
    assert call(N=65537, S=1) == EUNSUPPORTED
    assert call(N=1, S=65537) == EUNSUPPORTED
    assert call(N=65537, S=1, ws=None) == EUNSUPPORTED  # (the shape is judged before the workspace)
    assert call(t=7) == EUNSUPPORTED
    # x~ of 4 GiB or more; one expert of 2 GiB or more
    assert call(N=32768, S=2, K=32768, ldb=32768) == EUNSUPPORTED
    assert call(t=0, M=1 << 20, ldc=1 << 20, K=2048, ldb=2048) == EUNSUPPORTED


def test_empty_is_a_no_op():
    import kernels._lib as kl
    call = _caller(kl.lib(), ws_bytes=0)
    none = dict(A=None, ids=None, B=None, C=None, ws=None)
    assert call(N=0, **none) == OK
    assert call(S=0, **none) == OK
    assert call(M=0, ldc=0, **none) == OK
