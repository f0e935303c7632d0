"""Every refusal of the four attention entry points (include/ftmi355.h: ftmi_attn_fwd, ftmi_attn_bwd, ftmi_attn_ctx2_fwd, ftmi_attn_ctx2_dq) by error code and
message, on the host: each of them returns before anything is launched, so the pointers handed over are host addresses that are never read, and a call that
is NOT refused here (B = 0 / Sq = 0 of the second-context calls) returns 0 without a launch by contract.

The alignment rule (csrc/attention.hip: attn_misaligned; csrc/attn_ctx2.hip: rows8 / aligned16): every kernel moves rows of q, k, v, out, dout, dq, dk, dv in
16-byte pieces at base + b * batch stride + h * head stride + s * token stride + a multiple of 8 elements, so the base pointer and all three strides of every
tensor must be 16-byte aligned -- at head_dim 64 and 128 alike (the backward used to check the token strides at head_dim 64 only)."""

import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -2
FWD_T = ("q", "k", "v", "out")
BWD_T = ("q", "k", "v", "out", "dout", "dq", "dk", "dv")
STRIDES_OF = {"q": "q_strides", "k": "k_strides", "v": "v_strides", "out": "o_strides", "dout": "do_strides", "dq": "dq_strides", "dk": "dk_strides",
              "dv": "dv_strides"}


@pytest.fixture(scope="module")
def lib():
    from finetrainers_amd import _lib

    return _lib.load()


_keep = ctypes.create_string_buffer(4096)
BASE = (ctypes.addressof(_keep) + 255) & ~255  # an aligned host address (never dereferenced: every call below returns before a launch)


def last_error(lib):
    buf = ctypes.create_string_buffer(512)
    lib.ftmi_last_error(buf, 512)
    return buf.value.decode()


def desc(d=64, B=2, H=3, Sq=5, Sk=7):
    from finetrainers_amd import _lib

    t = _lib.AttnDesc()
    t.B, t.H, t.Sq, t.Sk, t.d, t.scale = B, H, Sq, Sk, d, 0.125
    for name in STRIDES_OF.values():
        a = getattr(t, name)
        a[0], a[1], a[2] = 64 * H * d, d, H * d  # [B, S, H, d] with room: multiples of 8
    t.bias_strides[0], t.bias_strides[1] = Sk, 0
    return t


def fwd(lib, t, ptrs=None, bias=None):
    p = dict(q=BASE, k=BASE + 16, v=BASE + 32, out=BASE + 48, lse=BASE + 64)
    p.update(ptrs or {})
    return lib.ftmi_attn_fwd(ctypes.byref(t) if t is not None else None, p["q"], p["k"], p["v"], p["out"], p["lse"], bias, None)


def bwd(lib, t, ptrs=None, bias=None):
    p = dict(q=BASE, k=BASE + 16, v=BASE + 32, out=BASE + 48, lse=BASE + 64, dout=BASE + 80, dq=BASE + 96, dk=BASE + 112, dv=BASE + 128, delta=BASE + 144)
    p.update(ptrs or {})
    return lib.ftmi_attn_bwd(ctypes.byref(t) if t is not None else None, p["q"], p["k"], p["v"], p["out"], p["lse"], p["dout"], p["dq"], p["dk"], p["dv"],
                             p["delta"], bias, None)


def c2fwd(lib, t, ptrs=None):
    p = dict(q=BASE, k=BASE + 16, v=BASE + 32, out_first=BASE + 48, out=BASE + 64, lse=BASE + 80)
    p.update(ptrs or {})
    return lib.ftmi_attn_ctx2_fwd(ctypes.byref(t) if t is not None else None, p["q"], p["k"], p["v"], p["out_first"], p["out"], p["lse"], None)


def c2dq(lib, t, ptrs=None):
    p = dict(q=BASE, k=BASE + 16, v=BASE + 32, lse=BASE + 48, dout=BASE + 64, dq_first=BASE + 80, dq=BASE + 96)
    p.update(ptrs or {})
    return lib.ftmi_attn_ctx2_dq(ctypes.byref(t) if t is not None else None, p["q"], p["k"], p["v"], p["lse"], p["dout"], p["dq_first"], p["dq"], None)


ENTRIES = {"ftmi_attn_fwd": fwd, "ftmi_attn_bwd": bwd, "ftmi_attn_ctx2_fwd": c2fwd, "ftmi_attn_ctx2_dq": c2dq}


def refused(lib, rc, code, *words):
    msg = last_error(lib)
    assert rc == code, (rc, code, msg)
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_descriptor_and_head_dim(lib, entry):
    call = ENTRIES[entry]
    refused(lib, call(lib, None), INVALID, "null descriptor")
    for d in (0, 32, 96, 192, 256, -64):
        refused(lib, call(lib, desc(d=d)), UNSUPPORTED, "head_dim must be 64 or 128")
    if "ctx2" in entry:
        refused(lib, call(lib, desc(d=64)), UNSUPPORTED, "attn_ctx2", "head_dim must be 128")


@pytest.mark.parametrize("entry,d", [("ftmi_attn_fwd", 64), ("ftmi_attn_fwd", 128), ("ftmi_attn_bwd", 64), ("ftmi_attn_bwd", 128)])
def test_empty_and_negative_sizes(lib, entry, d):
    call, who = ENTRIES[entry], entry[5:]
    for field in ("B", "H", "Sq", "Sk"):
        for val in (0, -1, -2**31):
            t = desc(d=d)
            setattr(t, field, val)
            refused(lib, call(lib, t), INVALID, who, "empty problem")


@pytest.mark.parametrize("entry", ["ftmi_attn_ctx2_fwd", "ftmi_attn_ctx2_dq"])
def test_ctx2_sizes(lib, entry):
    call = ENTRIES[entry]
    for field, val in (("Sk", 0), ("Sk", -1), ("H", 0), ("H", -3), ("B", -1), ("Sq", -1)):
        t = desc(d=128)
        setattr(t, field, val)
        refused(lib, call(lib, t), INVALID, "attn_ctx2", "empty key set or negative size")
    refused(lib, call(lib, desc(d=128, Sk=321)), UNSUPPORTED, "attn_ctx2", "at most 320 keys")
    refused(lib, call(lib, desc(d=128, Sk=2**31 - 1)), UNSUPPORTED, "at most 320 keys")
    # the largest key count is accepted as far as the next check (a null tensor), and an empty batch or query set returns 0 without a launch
    refused(lib, call(lib, desc(d=128, Sk=320), {"q": None}), INVALID, "null tensor")
    assert call(lib, desc(d=128, B=0)) == 0
    assert call(lib, desc(d=128, Sq=0)) == 0
    assert call(lib, desc(d=128, B=0, Sq=0, Sk=1)) == 0


def test_null_tensors(lib):
    for d in (64, 128):
        for name in FWD_T:
            refused(lib, fwd(lib, desc(d=d), {name: None}), INVALID, "ftmi_attn_fwd: null tensor")
        for name in BWD_T + ("lse", "delta"):
            refused(lib, bwd(lib, desc(d=d), {name: None}), INVALID, "ftmi_attn_bwd: null tensor")
    for name in ("q", "k", "v", "out_first", "out", "lse"):
        refused(lib, c2fwd(lib, desc(d=128), {name: None}), INVALID, "ftmi_attn_ctx2_fwd: null tensor")
    for name in ("q", "k", "v", "lse", "dout", "dq_first", "dq"):
        refused(lib, c2dq(lib, desc(d=128), {name: None}), INVALID, "ftmi_attn_ctx2_dq: null tensor")


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("entry", ["ftmi_attn_fwd", "ftmi_attn_bwd"])
def test_misaligned_strides_and_base_pointers(lib, entry, d):
    """Per tensor: the batch, head and token stride each off by 4 and by 1 element, and the base pointer off by 8, 4 and 2 bytes (buf[..., 4:68] of a wider
    buffer has legal strides and a base 8 bytes off)."""
    call, who = ENTRIES[entry], entry[5:]
    for name in (FWD_T if entry.endswith("fwd") else BWD_T):
        for axis in range(3):
            for off in (4, 1, -4):
                t = desc(d=d)
                getattr(t, STRIDES_OF[name])[axis] += off
                refused(lib, call(lib, t), INVALID, f"{who}: {name}:", "16-byte alignment")
        for off in (8, 4, 2):
            refused(lib, call(lib, desc(d=d), {name: BASE + off}), INVALID, f"{who}: {name}:", "16-byte alignment")


def test_order_of_the_checks(lib):
    """Sizes before alignment (an empty problem has no rows to align), the descriptor before the tensors."""
    t = desc(d=128, Sq=0)
    t.q_strides[2] += 4
    refused(lib, bwd(lib, t), INVALID, "empty problem")
    refused(lib, fwd(lib, desc(d=96), {"q": None}), UNSUPPORTED, "head_dim")


def test_ctx2_misaligned(lib):
    for name, call, tensors, word in (("fwd", c2fwd, ("q", "k", "v"), "q / k / v rows"), ("dq", c2dq, ("q", "k", "v"), "q / k / v rows"),
                                      ("fwd", c2fwd, ("out",), "output rows"), ("dq", c2dq, ("dout", "dq"), "dO / dQ rows")):
        for tn in tensors:
            for axis in range(3):
                t = desc(d=128)
                getattr(t, STRIDES_OF[tn])[axis] += 4
                refused(lib, call(lib, t), INVALID, "attn_ctx2", word, "16-byte alignment")
            refused(lib, call(lib, desc(d=128), {tn: BASE + 8}), INVALID, "attn_ctx2", word, "16-byte alignment")
    refused(lib, c2fwd(lib, desc(d=128), {"out_first": BASE + 8}), INVALID, "output rows")
    refused(lib, c2dq(lib, desc(d=128), {"dq_first": BASE + 8}), INVALID, "dO / dQ rows")
