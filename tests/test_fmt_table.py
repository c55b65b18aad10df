"""The Python block table (gguf/blocks.py) against the built library's (csrc/gguf_blocks.hpp kFmt,
read through gq_block_elems / gq_block_bytes) and against every Python table derived from it.  CPU only."""
from gguf import GGML_TYPES
from gguf.blocks import BLOCK, Q8_1


def test_python_table_equals_the_library():
    import kernels._lib as kl
    L = kl.lib()
    assert list(BLOCK) == list(kl.TYPES) and sorted(kl.TYPES.values()) == list(range(len(BLOCK)))
    for name, t in kl.TYPES.items():
        assert BLOCK[name] == (L.gq_block_elems(t), L.gq_block_bytes(t)), name
        assert (kl.BLOCK_ELEMS[t], kl.BLOCK_BYTES[t]) == BLOCK[name], name
    # the types the library knows: an empty problem (M = 0, before any launch) is GQ_OK for a known
    # type and GQ_EUNSUPPORTED for an unknown one
    known = [t for t in range(-1, 64) if L.gq_mmq(t, None, None, None, 0, 4, 256, 256, 4, None, 0, None) == kl.GQ_OK]
    assert known == list(range(len(BLOCK)))
    assert L.gq_mmq(len(BLOCK), None, None, None, 0, 4, 256, 256, 4, None, 0, None) == kl.GQ_EUNSUPPORTED


def test_derived_python_tables():
    from kernels.cpu_impls._cpu import _BYTES, _QK
    from utils.quantize._qlib import BLOCK as QB
    from utils.synth import BLOCK as YB
    import kernels._lib as kl
    by_name = {name: (qk, nbytes) for name, qk, nbytes in GGML_TYPES.values()}
    for name, t in kl.TYPES.items():
        assert by_name[name] == QB[name] == YB[name] == (_QK[t], _BYTES[t]) == BLOCK[name], name
    assert set(by_name) == set(BLOCK) | {"f32", "f16"}
    assert set(QB) == set(BLOCK) | {"q8_1"} and QB["q8_1"] == Q8_1 == (32, 36)
