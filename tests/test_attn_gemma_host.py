"""Host side of the attention options (gq_attn_decode_ex, gq_attn_prefill_ex, their plans and workspace
size) and of kernels.attention.attn_options: every refusal answers before a launch (fake pointers).  CPU only."""
import ctypes

import pytest

from test_attn_host import BASE, EINVAL, EUNSUPPORTED, OK


def _ex(L, entry, window=0, softcap=0.0, **kw):
    import kernels._lib as kl
    a = dict(BASE, **kw)
    ws = (a["ws"], a["nbytes"]) if entry == "decode" else ()
    return getattr(L, f"gq_attn_{entry}_ex")(a["kv"], a["q"], a["ldq"], a["kc"], a["vc"], a["tok"], a["head"], a["seq"], a["kv_len"],
                                             a["cap"], a["o"], a["ldo"], a["scale"], a["B"], a["N"], a["n_head"], a["n_kv"],
                                             a["D"], *ws, ctypes.byref(kl.AttnOpts(window, softcap)), None)


@pytest.mark.parametrize("entry", ["decode", "prefill"])
@pytest.mark.parametrize("opts,status,text", [
    (dict(window=-1), EINVAL, b"window"), (dict(softcap=float("inf")), EINVAL, b"softcap"),
    (dict(softcap=float("nan")), EINVAL, b"softcap"), (dict(softcap=-1.0), EINVAL, b"softcap"), (dict(softcap=1e-30), EINVAL, b"softcap"),
    (dict(window=8, D=96, ldq=768, ldo=768), EUNSUPPORTED, b"D=96"),
    (dict(window=8, D=256, ldq=2047), EINVAL, b"ldq")])  # (D = 256 passes the shape check: the next one answers)
def test_options_and_shapes_are_checked_before_a_launch(entry, opts, status, text):
    import kernels._lib as kl
    L = kl.lib()
    kw = dict(dict(ldq=2048, ldo=2048, tok=2176, head=272, seq=2176 * 64) if opts.get("D") == 256 else {}, **opts)
    assert _ex(L, entry, **kw) == status, L.gq_last_error()
    assert text in L.gq_last_error(), L.gq_last_error()


def test_decode_rows_plans_and_workspace_at_256():
    import kernels._lib as kl
    L = kl.lib()
    assert _ex(L, "decode", window=8, N=3, n_head=11, n_kv=1, ldq=1408, ldo=1408) == EUNSUPPORTED and b"query rows" in L.gq_last_error()
    size = lambda D, R=2, **o: L.gq_attn_decode_workspace_size_ex(1, R, 8, 8, D, ctypes.byref(kl.AttnOpts(**o)))  # noqa: E731
    assert size(256) > 0 and size(256, window=1024, softcap=50.0) > 0 and size(256) == L.gq_attn_decode_workspace_size(1, 2, 8, 8, 256)
    assert size(96) == 0 and size(256, R=33) == 0 and size(128, window=-1) == 0
    assert kl.attn_plan(1, 2, 8, 8, 256)[0] == 32 and kl.attn_prefill_plan(1, 512, 8, 8, 256)[1] == 32
    assert kl.attn_plan(1, 1, 8, 8, 128, window=40)[1] <= 3 < kl.attn_plan(1, 1, 8, 8, 128)[1]  # W follows the window's tiles
    assert L.gq_debug_attn_prefill_plan_ex(1, 512, 8, 8, 96, None, None, None) == EUNSUPPORTED
    assert L.gq_debug_attn_plan_ex(1, 2, 8, 8, 256, None, None, None) == OK
    with pytest.raises(ValueError):
        __import__("kernels").KVCache(1, 8, 1, 96)


@pytest.mark.parametrize("meta,layer,want", [
    ({"general.architecture": "gemma2", "gemma2.attention.sliding_window": 4096, "gemma2.attn_logit_softcapping": 50.0}, 0, (4096, 50.0)),
    ({"general.architecture": "gemma2", "gemma2.attention.sliding_window": 4096, "gemma2.attn_logit_softcapping": 50.0}, 1, (0, 50.0)),
    ({"general.architecture": "gemma3", "gemma3.attention.sliding_window": 1024}, 4, (1024, 0.0)),
    ({"general.architecture": "gemma3", "gemma3.attention.sliding_window": 1024}, 5, (0, 0.0)),
    ({"general.architecture": "gemma3", "gemma3.attention.sliding_window": 512, "gemma3.attention.sliding_window_pattern": 3}, 2, (0, 0.0)),
    ({"general.architecture": "gemma3", "gemma3.attention.sliding_window": 512, "gemma3.attention.sliding_window_pattern": 3}, 5, (0, 0.0)),
    ({"general.architecture": "gemma3", "gemma3.attention.sliding_window": 512, "gemma3.attention.sliding_window_pattern": 3}, 4, (512, 0.0)),
    ({"general.architecture": "phi3", "phi3.attention.sliding_window": 2047}, 7, (2047, 0.0)),
    ({"general.architecture": "llama"}, 3, (0, 0.0))])
def test_attn_options_from_metadata(meta, layer, want):
    from kernels.attention import attn_options
    assert attn_options(meta, layer) == {"window": want[0], "softcap": want[1]}
