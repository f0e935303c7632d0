"""The refusals ftmi_attn_fwd_carry and ftmi_accum_bf16 add to those of ftmi_attn_fwd (include/ftmi355.h), on the host: every call returns before a launch, so
the pointers are host addresses that are never read."""

import ctypes

import pytest

from test_attention_refusals_host import BASE, INVALID, UNSUPPORTED, desc, lib, refused  # noqa: F401  (lib: the library fixture)


def carry(lib, t, **ptrs):
    p = dict(q=BASE, k=BASE + 16, v=BASE + 32, acc=BASE + 48, lse=BASE + 64, out=BASE + 80)
    p.update(ptrs)
    return lib.ftmi_attn_fwd_carry(ctypes.byref(t), p["q"], p["k"], p["v"], p["acc"], p["lse"], p["out"], None, 0, None)


@pytest.mark.parametrize("d", [64, 128])
def test_carry_refusals(lib, d):
    refused(lib, carry(lib, desc(d=96)), UNSUPPORTED, "head_dim must be 64 or 128")
    for name in ("acc", "lse"):
        refused(lib, carry(lib, desc(d=d), **{name: None}), INVALID, "ftmi_attn_fwd_carry: null state")
    refused(lib, carry(lib, desc(d=d), q=None), INVALID, "ftmi_attn_fwd_carry: null tensor")
    for off in (8, 4):
        refused(lib, carry(lib, desc(d=d), acc=BASE + 48 + off), INVALID, "attn_fwd_carry: acc:", "16-byte alignment")
    refused(lib, carry(lib, desc(d=d, Sk=0)), INVALID, "attn_fwd_carry: empty problem")
    for name, field in (("q", "q_strides"), ("k", "k_strides"), ("v", "v_strides"), ("out", "o_strides")):
        t = desc(d=d)
        getattr(t, field)[2] += 4
        refused(lib, carry(lib, t), INVALID, f"attn_fwd_carry: {name}:", "16-byte alignment")
    t = desc(d=d)
    t.o_strides[2] += 4  # no out, no rule for its strides: accepted as far as the next check
    refused(lib, carry(lib, t, out=None, acc=BASE + 52), INVALID, "acc:")


def test_accum_refusals(lib):
    t = desc(d=128)
    refused(lib, lib.ftmi_accum_bf16(ctypes.byref(t), None, BASE, None, None), INVALID, "ftmi_accum_bf16: null tensor")
    refused(lib, lib.ftmi_accum_bf16(ctypes.byref(t), BASE + 4, BASE + 16, None, None), INVALID, "accum_bf16: acc:", "16-byte alignment")
    t.dq_strides[1] += 4
    refused(lib, lib.ftmi_accum_bf16(ctypes.byref(t), BASE, BASE + 16, None, None), INVALID, "accum_bf16: x:", "16-byte alignment")
