"""Host side of the int8 / fp8 attention forward (include/ftmi355.h: ftmi_attn_q8_workspace_bytes, ftmi_attn_q8_quant, ftmi_attn_fwd_q8; ops.attn_fwd_q8; the
mi355x_sage provider): every call returns before a launch, so the pointers handed to the library are host addresses that are never read."""

import ctypes

import pytest
import torch

from test_attention_refusals_host import BASE, INVALID, UNSUPPORTED, desc, lib, refused  # noqa: F401  (lib: the library fixture)

WS = BASE + 1024  # 256-byte aligned


def fwd_q8(lib, t, ws=WS, ws_bytes=1 << 30, **ptrs):
    p = dict(q=BASE, k=BASE + 16, v=BASE + 32, out=BASE + 48)
    p.update(ptrs)
    return lib.ftmi_attn_fwd_q8(ctypes.byref(t), p["q"], p["k"], p["v"], p["out"], None, 1, ws, ws_bytes, None)


def quant(lib, t, ws=WS, ws_bytes=1 << 30, **ptrs):
    p = dict(q=BASE, k=BASE + 16, v=BASE + 32)
    p.update(ptrs)
    return lib.ftmi_attn_q8_quant(ctypes.byref(t), p["q"], p["k"], p["v"], 1, ws, ws_bytes, None)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("call,who,tensors", [(fwd_q8, "attn_fwd_q8", ("q", "k", "v", "out")), (quant, "attn_q8_quant", ("q", "k", "v"))])
def test_library_refusals(lib, d, call, who, tensors):
    refused(lib, call(lib, desc(d=96)), UNSUPPORTED, "head_dim must be 64 or 128")
    refused(lib, call(lib, desc(d=d, Sk=0)), INVALID, f"{who}: empty problem")
    strides = dict(q="q_strides", k="k_strides", v="v_strides", out="o_strides")
    for name in tensors:
        refused(lib, call(lib, desc(d=d), **{name: None}), INVALID, f"{who}: null tensor")
        refused(lib, call(lib, desc(d=d), **{name: BASE + 8}), INVALID, f"{who}: {name}:", "16-byte alignment")
        t = desc(d=d)
        getattr(t, strides[name])[2] += 4
        refused(lib, call(lib, t), INVALID, f"{who}: {name}:", "16-byte alignment")
    refused(lib, call(lib, desc(d=d), ws=None), INVALID, f"{who}: null workspace")
    refused(lib, call(lib, desc(d=d), ws=WS + 16), INVALID, f"{who}: workspace:", "256-byte alignment")
    refused(lib, call(lib, desc(d=d), ws_bytes=lib.ftmi_attn_q8_workspace_bytes(ctypes.byref(desc(d=d))) - 1), INVALID, f"{who}: workspace of")


def test_workspace_bytes(lib):
    """Monotone in Sk, 0 for a refused problem, and at (1, 1, 1, 1, 64) the sum of the documented pieces, each rounded up to 256 bytes."""
    sizes = [lib.ftmi_attn_q8_workspace_bytes(ctypes.byref(desc(d=128, B=1, H=12, Sq=300, Sk=sk))) for sk in (1, 63, 64, 65, 256, 257, 1000, 10752)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[0]
    assert lib.ftmi_attn_q8_workspace_bytes(ctypes.byref(desc(d=32))) == 0
    r256 = lambda n: (n + 255) & ~255  # noqa: E731
    pieces = (64, 4, 64 * 64, 4, 64 * 64, 64 * 4, 64 * 4, 64 * 4)  # q8, sq, k8 (one tile), sk, v8 (one tile), sv, the two statistics buffers (one chunk)
    assert lib.ftmi_attn_q8_workspace_bytes(ctypes.byref(desc(d=64, B=1, H=1, Sq=1, Sk=1))) == sum(r256(n) for n in pieces)


@pytest.mark.parametrize("case,word", [("d32", "head_dim 64 and 128"), ("dtype", "must be torch.bfloat16"), ("Sk", "key/value shapes"), ("cpu", "must live in GPU memory")])
def test_ops_refusals(case, word):
    from finetrainers_amd import ops

    d = 32 if case == "d32" else 64
    q, k, v = (torch.zeros(1, 2, S, d, dtype=torch.float16 if case == "dtype" else torch.bfloat16) for S in (5, 7, 8 if case == "Sk" else 7))
    for call in (ops.attn_fwd_q8, ops.attn_q8_quantize):
        with pytest.raises(ValueError, match=word):
            call(q, k, v)


def test_provider_is_registered():
    from finetrainers_amd.attention_dispatch import AttentionProvider, _AttentionProviderRegistry, attention_provider

    assert AttentionProvider("mi355x_sage") is AttentionProvider.MI355X_SAGE
    assert AttentionProvider.MI355X_SAGE in _AttentionProviderRegistry.list_providers()
    assert not _AttentionProviderRegistry.supports_context_parallel(AttentionProvider.MI355X_SAGE)
    with pytest.raises(ValueError, match="context parallelism"):
        with attention_provider(AttentionProvider.MI355X_SAGE, mesh=object()):
            pass
