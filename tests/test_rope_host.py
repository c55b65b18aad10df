"""Host side of gq_rope_append and kernels.attention.RoPE: every refusal answers before a launch (fake
pointers) with gq_last_error set; RoPE.from_gguf's tables against the formulas in float64.  CPU only."""
import ctypes
import math

import numpy as np
import pytest

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
MB = 1 << 20
Q, KN, VN, QO, KC, VC, LEN, FREQ, WQ, WK = (ctypes.c_void_p(i * 16 * MB) for i in range(1, 11))
BASE = dict(kv=1, mode=1, q=Q, ldq=1024, kn=KN, ldk=256, vn=VN, ldv=256, qo=QO, ldqo=1024, kc=KC, vc=VC, tok=272, head=136,
            seq=272 * 64, kv_len=LEN, cap=64, freq=FREQ, n_rot=128, m=1.0, wq=WQ, wk=WK, eps=1e-6, B=2, N=2, n_head=8, n_kv=2, D=128)


def _rope(L, **kw):
    a = dict(BASE, **kw)
    return L.gq_rope_append(a["kv"], a["mode"], a["q"], a["ldq"], a["kn"], a["ldk"], a["vn"], a["ldv"], a["qo"], a["ldqo"], a["kc"],
                            a["vc"], a["tok"], a["head"], a["seq"], a["kv_len"], a["cap"], a["freq"], a["n_rot"], a["m"], a["wq"],
                            a["wk"], a["eps"], a["B"], a["N"], a["n_head"], a["n_kv"], a["D"], None)


@pytest.mark.parametrize("kw,status,text", [
    (dict(kv=5), EUNSUPPORTED, b"kv cache type"), (dict(mode=2), EUNSUPPORTED, b"rope mode"),
    (dict(n_rot=127), EUNSUPPORTED, b"n_rot"), (dict(n_rot=0), EUNSUPPORTED, b"n_rot"), (dict(n_rot=130), EUNSUPPORTED, b"n_rot"),
    (dict(q=None), EINVAL, b"null"), (dict(kn=None), EINVAL, b"null"), (dict(vn=None), EINVAL, b"null"),
    (dict(qo=None), EINVAL, b"null"), (dict(kc=None), EINVAL, b"null"), (dict(kv_len=None), EINVAL, b"null"),
    (dict(freq=None), EINVAL, b"null"), (dict(wq=None), EINVAL, b"norm weight"), (dict(wk=None), EINVAL, b"norm weight"),
    (dict(ldq=1023), EINVAL, b"ldq"), (dict(ldqo=512), EINVAL, b"ldqo"), (dict(ldk=255), EINVAL, b"ldk"), (dict(ldv=128), EINVAL, b"ldv"),
    (dict(B=-1), EINVAL, b"negative"), (dict(D=32, n_rot=32), EUNSUPPORTED, b"D=32"), (dict(n_kv=3, ldk=384, ldv=384), EUNSUPPORTED, b"multiple of n_kv_head"),
    (dict(seq=7), EUNSUPPORTED, b"multiples of 2"), (dict(tok=134), EUNSUPPORTED, b"tok_stride"), (dict(cap=1), EUNSUPPORTED, b"capacity")])
def test_rope_append_refuses_before_a_launch(kw, status, text):
    import kernels._lib as kl
    L = kl.lib()
    assert _rope(L, **kw) == status, L.gq_last_error()
    assert text in L.gq_last_error(), L.gq_last_error()


def test_empty_calls_are_no_ops_and_wrappers_refuse_host_tensors():
    import torch

    import kernels
    import kernels._lib as kl
    L = kl.lib()
    assert _rope(L, B=0, q=None) == OK and _rope(L, N=0, kc=None) == OK and _rope(L, n_head=0, n_kv=0, freq=None) == OK
    z, b8, n = torch.zeros(2, 1024, dtype=torch.float16), torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        kernels.rope_append("q8_0", "neox", z, z, z, b8, b8, (1088, 136, 4096), n, 2, torch.zeros(64), 128, 2, 1, 8, 8, 128)
    with pytest.raises(ValueError, match="together"):
        kernels.RoPE(torch.zeros(32), 64, "norm", q_norm=torch.ones(64))
    with pytest.raises(ValueError, match="mode"):
        kernels.RoPE(torch.zeros(32), 64, "gptj")


META = {"general.architecture": "llama", "llama.embedding_length": 4096, "llama.attention.head_count": 32}
CASES = {
    "base 1e6": ({"llama.rope.freq_base": 1e6}, {}),
    "linear 4": ({"llama.rope.scaling.type": "linear", "llama.rope.scaling.factor": 4.0}, {}),
    "yarn 4 over 32768": ({"llama.rope.scaling.type": "yarn", "llama.rope.scaling.factor": 4.0,
                           "llama.rope.scaling.original_context_length": 32768, "llama.rope.freq_base": 1e6}, {}),
    "rope_freqs": ({"llama.rope.freq_base": 5e5}, {"rope_freqs.weight": np.linspace(1.0, 8.0, 64, dtype=np.float32)}),
    "partial": ({"llama.rope.dimension_count": 64}, {}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_from_gguf_tables_follow_the_formulas(name):
    from kernels import RoPE
    extra, tensors = CASES[name]
    meta = dict(META, **extra)
    r = RoPE.from_gguf(meta, tensors, 0, "cpu")
    n_rot = meta.get("llama.rope.dimension_count", 128)
    base, factor = meta.get("llama.rope.freq_base", 10000.0), meta.get("llama.rope.scaling.factor", 1.0)
    kind, want, mscale = meta.get("llama.rope.scaling.type", "none"), [], 1.0
    for j in range(n_rot // 2):
        f = base ** (-2.0 * j / n_rot)
        if tensors:
            f /= float(tensors["rope_freqs.weight"][j])
        if kind == "linear":
            f /= factor
        if kind == "yarn":
            corr = lambda beta: n_rot * math.log(32768 / (2 * math.pi * beta)) / (2 * math.log(base))  # noqa: E731
            lo, hi = max(0, math.floor(corr(32))), min(n_rot - 1, math.ceil(corr(1)))
            ramp = 1 - min(1.0, max(0.0, (j - lo) / max(0.001, hi - lo)))
            f, mscale = f * ((1 - ramp) / factor + ramp), 1 + 0.1 * math.log(factor)
        want.append(f)
    assert (r.n_rot, r.mode, r.q_norm, r.k_norm) == (n_rot, "norm", None, None) and r.mscale == pytest.approx(mscale, rel=1e-15)
    assert np.array_equal(r.inv_freq.numpy(), np.array(want, dtype=np.float64).astype(np.float32))
    if kind == "yarn":  # the fast pairs keep their frequency, the slow ones are divided by the factor
        assert want[0] == 1.0 and want[-1] == pytest.approx(base ** (-2.0 * 63 / 128) / 4, rel=1e-12)


def test_modes_by_architecture_and_the_norm_weights():
    from kernels import RoPE
    from kernels.attention import ROPE_MODE
    assert {a for a, m in ROPE_MODE.items() if m == "norm"} == {"llama", "llama4", "deepseek", "deepseek2"}
    assert {a for a, m in ROPE_MODE.items() if m == "neox"} == {"qwen2", "qwen2moe", "qwen3", "qwen3moe", "gemma", "gemma2", "gemma3",
                                                                "phi3", "falcon", "stablelm", "olmo2", "gptneox"}
    meta = {"general.architecture": "qwen3", "qwen3.attention.key_length": 64, "qwen3.embedding_length": 4096,
            "qwen3.attention.head_count": 32, "qwen3.attention.layer_norm_rms_epsilon": 1e-5}
    w = {f"blk.3.attn_{n}_norm.weight": np.full(64, v, np.float32) for n, v in (("q", 1.5), ("k", 0.5))}
    r = RoPE.from_gguf(meta, w, 3, "cpu")
    assert (r.mode, r.n_rot, r.eps) == ("neox", 64, 1e-5) and float(r.q_norm[0]) == 1.5 and float(r.k_norm[63]) == 0.5
    assert RoPE.from_gguf(meta, w, 0, "cpu").q_norm is None
    with pytest.raises(ValueError, match="mamba"):
        RoPE.from_gguf({"general.architecture": "mamba", "mamba.attention.key_length": 64}, {}, 0, "cpu")
    assert RoPE.from_gguf({"general.architecture": "mamba", "mamba.attention.key_length": 64}, {}, 0, "cpu", mode="neox").mode == "neox"
