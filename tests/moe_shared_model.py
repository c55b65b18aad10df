"""Numpy model of gq_moe_combine_shared: what the entry is defined to return from its inputs.  The
GLU entry (gq_mmq_glu) has gq_mmq_id_glu's definition: moe_fused_model.glu and ulp16 serve it."""
import numpy as np

from moe_fused_model import glu, ulp16  # noqa: F401  (the tests of the shared block import them from here)


def combine_shared(D16, W, Dsh16, gate=None):
    """gq_moe_combine_shared's defined order exactly: acc = 0.f; for s in order
    acc = fl32(acc + fl32(w*d)); then acc = fl32(acc + dsh), or with a gate
    acc = fl32(acc + fl32(gate[n]*dsh)); one rounding to fp16.
    D16 (N, S, M) fp16, W (N, S) fp16 or fp32, Dsh16 (N, M) fp16, gate None or (N,) fp32 -> (N, M) fp16."""
    D = np.asarray(D16, dtype=np.float16).astype(np.float32)
    Dsh = np.asarray(Dsh16, dtype=np.float16).astype(np.float32)
    W = np.asarray(W)
    assert W.dtype in (np.float16, np.float32)
    W = W.astype(np.float32)
    N, S, M = D.shape
    assert S >= 1 and Dsh.shape == (N, M)
    acc = np.zeros((N, M), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(S):
            prod = (W[:, s, None] * D[:, s, :]).astype(np.float32)
            acc = (acc + prod).astype(np.float32)
        if gate is None:
            term = Dsh
        else:
            g = np.asarray(gate)
            assert g.dtype == np.float32 and g.shape == (N,)
            term = (g[:, None] * Dsh).astype(np.float32)
        acc = (acc + term).astype(np.float32)
        return acc.astype(np.float16)
