"""Host side of the expert-indexed MMQ (gq_mmq_id, mixture-of-experts FFN blocks): the header, the
library and kernels._lib.SIGNATURES agree on the entry; its argument checks (fake pointers: every
case returns before a launch); the host-sorted fallback's grouping; GGUF 3-D expert tensors
through write_gguf / read_gguf, 2-D files byte for byte as before.  CPU only."""
import ctypes
import os
import re
import struct

import numpy as np

from utils.synth import random_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, EINVAL, EUNSUPPORTED = 0, 1, 3


def test_entry_declared_exported_bound():
    import kernels._lib as kl
    text = open(os.path.join(ROOT, "include", "gguf_mmq.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"int\s+gq_mmq_id\s*\(([^)]*)\)\s*;", text)
    assert proto, "include/gguf_mmq.h does not declare gq_mmq_id"
    args = [a.strip() for a in proto.group(1).split(",")]
    assert len(args) == 14
    assert args[2].replace(" ", "") == "constint32_t*ids"
    assert [a.split()[-1].lstrip("*") for a in args] == ["t", "A", "ids", "B", "C", "E", "M", "N", "S", "K", "ldb",
                                                          "ldb_slot", "ldc", "stream"]
    assert hasattr(kl.lib(), "gq_mmq_id")
    argtypes, restype = kl.SIGNATURES["gq_mmq_id"]
    assert len(argtypes) == 14 and restype is ctypes.c_int
    assert argtypes[0] is ctypes.c_int and argtypes[-1] is ctypes.c_void_p
    assert all(a is ctypes.c_void_p for a in argtypes[1:5]) and all(a is ctypes.c_int64 for a in argtypes[5:13])
    assert kl.lib().gq_version() == 105  # (the entry is detected by its symbol, not by the version)


def test_argument_checks():
    import kernels._lib as kl
    L = kl.lib()
    p = ctypes.c_void_p(16)

    def call(t=1, A=p, ids=p, B=p, C=p, E=4, M=8, N=2, S=2, K=256, ldb=256, ldb_slot=0, ldc=8):
        return L.gq_mmq_id(t, A, ids, B, C, E, M, N, S, K, ldb, ldb_slot, ldc, None)

    # K not a multiple of the block
    assert call(K=100, ldb=100) == EINVAL
    assert b"multiple of 256" in L.gq_last_error()
    assert call(t=0, K=48, ldb=48) == EINVAL
    # unknown type
    assert call(t=7) == EUNSUPPORTED
    # null pointers
    for name in ("A", "ids", "B", "C"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null" in L.gq_last_error()
    # short leading dimensions; a slot stride that is neither 0 nor a whole row
    assert call(ldc=7) == EINVAL
    assert call(ldb=255) == EINVAL
    assert call(ldb_slot=255) == EINVAL
    assert b"ldb_slot" in L.gq_last_error()
    # more pairs than one launch takes: refused, whatever N x S makes them
    assert call(N=65, S=1) == EUNSUPPORTED
    assert call(N=13, S=5) == EUNSUPPORTED
    assert call(N=5, S=13) == EUNSUPPORTED
    assert b"64" in L.gq_last_error()
    # a row too long for the one-token decode's LDS image
    assert call(t=0, K=1 << 20, ldb=1 << 20) == EUNSUPPORTED
    # empty problems are a no-op, even with null pointers
    assert call(A=None, ids=None, B=None, C=None, N=0) == OK
    assert call(A=None, ids=None, B=None, C=None, S=0) == OK
    assert call(A=None, ids=None, B=None, C=None, M=0, ldc=0) == OK


def test_pairs_by_expert():
    import kernels._lib as kl
    E = 5
    ids = np.array([[3, 0], [3, -1], [0, E], [4, 3]], dtype=np.int32)
    got = kl.pairs_by_expert(ids, E)
    assert got == {3: [0, 2, 7], 0: [1, 4], 4: [6]}  # expert 1, 2: unused; pairs 3 and 5: out of range
    assert all(isinstance(p, int) for v in got.values() for p in v)
    assert kl.pairs_by_expert(np.zeros((0, 2), dtype=np.int32), E) == {}
    assert kl.pairs_by_expert(np.array([[-1, E, E + 7]], dtype=np.int32), E) == {}


def _w_str(s):
    b = s.encode("utf-8")
    return struct.pack("<Q", len(b)) + b


def _expected_file(tensors, alignment=32):
    """The file's bytes from the documented layout (gguf/file.py's module docstring): header, the
    general.alignment entry (int64), tensor infos with dims innermost first, aligned data."""
    out = b"GGUF" + struct.pack("<IQQ", 3, len(tensors), 1)
    out += _w_str("general.alignment") + struct.pack("<Iq", 11, alignment)
    off, blobs = 0, []
    for name, (type_id, dims, raw) in tensors.items():
        out += _w_str(name) + struct.pack("<I", len(dims)) + b"".join(struct.pack("<Q", d) for d in dims)
        out += struct.pack("<IQ", type_id, off)
        blobs.append((off, raw))
        off = (off + len(raw) + alignment - 1) // alignment * alignment
    out += b"\0" * (-len(out) % alignment)
    data0 = len(out)
    for o, raw in blobs:
        out += b"\0" * (data0 + o - len(out)) + raw
    return out


def test_gguf_3d_round_trip(tmp_path):
    from gguf.file import read_gguf, write_gguf
    E, M, K = 3, 8, 256
    exps = np.concatenate([random_blocks("q4_k", M, K, seed=20 + e) for e in range(E)]).view(np.uint8)
    flat = random_blocks("q6_k", 5, 512, seed=30).view(np.uint8)
    path = str(tmp_path / "moe.gguf")
    write_gguf(path, {"blk.0.ffn_gate_exps.weight": ("q4_k", (E, M, K), exps),
                      "blk.0.attn_v.weight": ("q6_k", (5, 512), flat)})
    meta, tensors = read_gguf(path)
    t = tensors["blk.0.ffn_gate_exps.weight"]
    assert t.dims == (K, M, E) and t.shape == (E, M, K) and t.type_name == "q4_k"
    assert t.data.size == E * M * (K // 256) * 144 and bytes(t.data) == exps.tobytes()
    per = M * (K // 256) * 144  # expert e's matrix: bytes [e * per, (e + 1) * per)
    assert bytes(t.data[per:2 * per]) == random_blocks("q4_k", M, K, seed=21).view(np.uint8).tobytes()
    v = tensors["blk.0.attn_v.weight"]
    assert v.dims == (512, 5) and v.shape == (5, 512) and bytes(v.data) == flat.tobytes()
    want = _expected_file({"blk.0.ffn_gate_exps.weight": (12, (K, M, E), exps.tobytes()),
                           "blk.0.attn_v.weight": (14, (512, 5), flat.tobytes())})
    assert open(path, "rb").read() == want


def test_gguf_2d_file_bytes_unchanged(tmp_path):
    """A file of 2-D tensors only: byte for byte what the writer produced before it took 3-D
    shapes (n_dims = 2, dims (K, M))."""
    from gguf.file import write_gguf
    a = random_blocks("q8_0", 3, 96, seed=1).view(np.uint8)   # 306 bytes: padding before the next tensor
    b = random_blocks("q4_k", 2, 256, seed=2).view(np.uint8)
    path = str(tmp_path / "dense.gguf")
    write_gguf(path, {"a.weight": ("q8_0", (3, 96), a), "b.weight": ("q4_k", (2, 256), b)})
    want = _expected_file({"a.weight": (8, (96, 3), a.tobytes()), "b.weight": (12, (256, 2), b.tobytes())})
    assert open(path, "rb").read() == want
