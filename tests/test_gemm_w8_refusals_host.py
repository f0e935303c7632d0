"""The refusals of ftmi_gemm_nt_w8 / ftmi_gemm_nn_w8 and of ftmi_linear_lora_w8_fwd / _bwd (include/ftmi355.h), on the host: every call returns before a launch,
so the pointers are host addresses that are never read.  Then the ValueErrors of the ops wrappers and the construction-time rounding of MI355XFp8LoRALinear."""

import ctypes

import pytest
import torch

from finetrainers_amd import _lib
from test_attention_refusals_host import BASE, INVALID, UNSUPPORTED, lib, refused  # noqa: F401  (lib: the library fixture)

P = [BASE + 16 * i for i in range(12)]  # aligned addresses


def nt(lib, **kw):
    f = dict(x=P[0], ldx=192, w8=P[1], ldw8=192, bias=P[2], M=5, N=256, K=192, x2=P[3], ldx2=64, w2=P[4], ldw2=64, K2=64, out=P[5], ldo=256, out2=P[6], ldo2=256, epilogue=1)
    f.update(kw)
    return lib.ftmi_gemm_nt_w8(ctypes.byref(_lib.GemmW8Args(**f)), None)


def nn(lib, **kw):
    f = dict(dy=P[0], lddy=192, w=P[1], ldw=256, M=5, N=192, K=256, x2=P[3], ldx2=64, w2=P[4], ldw2=64, K2=64, aux=P[6], ldaux=256, out=P[5], ldo=256, epilogue=3)
    f.update(kw)
    return lib.ftmi_gemm_nn_w8(ctypes.byref(_lib.GemmNnArgs(**f)), None)


@pytest.mark.parametrize("call,who,fields,code,words", [
    (lambda lib: lib.ftmi_gemm_nt_w8(None, None), "ftmi_gemm_nt_w8", {}, INVALID, ("null argument block",)),
    (lambda lib: lib.ftmi_gemm_nn_w8(None, None), "ftmi_gemm_nn_w8", {}, INVALID, ("null argument block",)),
    (nt, "gemm_nt_w8", dict(w8=None), INVALID, ("null tensor",)),
    (nt, "gemm_nt_w8", dict(K=160, ldx=160, ldw8=160), UNSUPPORTED, ("K", "multiple of 64")),
    (nt, "gemm_nt_w8", dict(N=192), UNSUPPORTED, ("N", "multiple of 128")),
    (nt, "gemm_nt_w8", dict(K2=96, ldx2=96, ldw2=96), UNSUPPORTED, ("K2 must be a multiple of 64",)),
    (nt, "gemm_nt_w8", dict(epilogue=3), UNSUPPORTED, ("epilogue must be 0 (store) or 1 (gelu)",)),
    (nt, "gemm_nt_w8", dict(out2=None), INVALID, ("gelu epilogue without out2",)),
    (nt, "gemm_nt_w8", dict(w2=None), INVALID, ("K-extension without its operands",)),
    (nt, "gemm_nt_w8", dict(bias=P[2] + 8), INVALID, ("16-byte alignment",)),
    (nt, "gemm_nt_w8", dict(ldw8=200), INVALID, ("leading dimensions", "16-byte")),
    (nt, "gemm_nt_w8", dict(ldx=196), INVALID, ("leading dimensions", "16-byte")),
    (nt, "gemm_nt_w8", dict(ldw8=176), INVALID, ("smaller than its row",)),
    (nt, "gemm_nt_w8", dict(ldw8=1 << 25), UNSUPPORTED, ("too large", "32-bit offsets")),
    (nn, "gemm_nn_w8", dict(w=None), INVALID, ("null tensor",)),
    (nn, "gemm_nn_w8", dict(N=160, lddy=160), UNSUPPORTED, ("N", "multiple of 64")),
    (nn, "gemm_nn_w8", dict(K=192), UNSUPPORTED, ("K", "multiple of 128")),
    (nn, "gemm_nn_w8", dict(K2=96, ldx2=96, ldw2=96), UNSUPPORTED, ("K2 must be a multiple of 64",)),
    (nn, "gemm_nn_w8", dict(epilogue=1), UNSUPPORTED, ("epilogue must be 0 (store) or 3 (gelu')",)),
    (nn, "gemm_nn_w8", dict(aux=None), INVALID, ("gelu' epilogue without pre-activation",)),
    (nn, "gemm_nn_w8", dict(x2=None), INVALID, ("K-extension without its operands",)),
    (nn, "gemm_nn_w8", dict(w=P[1] + 8), INVALID, ("16-byte alignment",)),
    (nn, "gemm_nn_w8", dict(ldw=264), INVALID, ("leading dimensions", "16-byte")),
    (nn, "gemm_nn_w8", dict(ldo=128), INVALID, ("smaller than its row",)),
    (nn, "gemm_nn_w8", dict(ldw=1 << 26), UNSUPPORTED, ("too large", "32-bit offsets")),
])
def test_gemm_w8_refusals(lib, call, who, fields, code, words):
    refused(lib, call(lib, **fields), code, who + ": ", *words)


def fwd(lib, M=5, K=128, N=256, r=64, **kw):
    p = dict(x=P[0], w8=P[1], bias=P[2], a_sp=P[3], b_ext=P[4], y=P[5], xa=P[6])
    p.update(kw)
    return lib.ftmi_linear_lora_w8_fwd(M, K, N, r, 0.5, p["x"], p["w8"], p["bias"], p["a_sp"], p["b_ext"], p["y"], p["xa"], None)


def bwd(lib, M=5, K=128, N=256, r=64, **kw):
    p = dict(x=P[0], dy=P[1], xa=P[2], w8=P[3], bt_sp=P[4], at_ext=P[5], dxa=P[6], dx=P[7], ga=P[8], gb=P[9])
    p.update(kw)
    return lib.ftmi_linear_lora_w8_bwd(M, K, N, r, 0.5, p["x"], p["dy"], p["xa"], p["w8"], p["bt_sp"], p["at_ext"], p["dxa"], p["dx"], p["ga"], p["gb"], None)


@pytest.mark.parametrize("call,kw,code,words", [
    (fwd, dict(w8=None), INVALID, ("ftmi_linear_lora_w8_fwd: null tensor",)),
    (fwd, dict(b_ext=None), INVALID, ("ftmi_linear_lora_w8_fwd: LoRA tensors missing",)),
    (fwd, dict(r=96), UNSUPPORTED, ("ftmi_linear_lora_w8_fwd: rank must be 0 or a multiple of 64",)),
    (fwd, dict(N=192), UNSUPPORTED, ("gemm_nt_w8: N", "multiple of 128")),  # the GEMM's refusal, in front of the down-projection's launch
    (fwd, dict(x=P[0] + 8, r=0), INVALID, ("gemm_nt_w8: ", "16-byte alignment")),
    (bwd, dict(w8=None), INVALID, ("ftmi_linear_lora_w8_bwd: null tensor",)),
    (bwd, dict(ga=None), INVALID, ("ftmi_linear_lora_w8_bwd: LoRA tensors missing",)),
    (bwd, dict(r=32), UNSUPPORTED, ("ftmi_linear_lora_w8_bwd: rank must be 0 or a multiple of 64",)),
    (bwd, dict(K=192), UNSUPPORTED, ("gemm_nn_w8: K", "multiple of 128")),
])
def test_linear_lora_w8_refusals(lib, call, kw, code, words):
    refused(lib, call(lib, **kw), code, *words)


class _OnGpu(torch.Tensor):  # a CPU tensor that says it is on the GPU: the wrappers' own checks all come before the library is called
    is_cuda = True


def _t(rows, cols, dtype=torch.bfloat16):
    return torch.zeros(rows, cols).to(dtype).as_subclass(_OnGpu)


@pytest.mark.parametrize("fn,args,kw,words", [
    ("gemm_nt_w8", lambda: (_t(4, 64), _t(128, 64)), {}, "w8 must be torch.float8_e4m3fn"),
    ("gemm_nt_w8", lambda: (_t(4, 64, torch.float32), _t(128, 64, torch.float8_e4m3fn)), {}, "activation must be torch.bfloat16"),
    ("gemm_nt_w8", lambda: (_t(4, 64), _t(128, 128, torch.float8_e4m3fn)), {}, "do not chain"),
    ("gemm_nt_w8", lambda: (_t(4, 64), _t(64, 128, torch.float8_e4m3fn).t()), {}, "contiguous columns"),
    ("gemm_nt_w8", lambda: (_t(4, 64), _t(128, 64, torch.float8_e4m3fn)), dict(x2=_t(4, 64)), "needs both x2 and w2"),
    ("gemm_nt_w8", lambda: (_t(4, 64), _t(128, 64, torch.float8_e4m3fn), _t(1, 64)[0]), {}, "bias must be a contiguous [N] vector"),
    ("gemm_nn_w8", lambda: (_t(4, 64), _t(64, 128, torch.float8_e4m3fn)), dict(aux=_t(4, 64)), "aux must be an [M, K] view"),
    ("gemm_nn_w8", lambda: (_t(4, 64), _t(64, 128, torch.float8_e4m3fn)), dict(x2=_t(4, 64), w2=_t(64, 64)), "x2 must be [M, K2] and w2 [K, K2]"),
    ("gemm_nn_w8", lambda: (torch.zeros(4, 64, dtype=torch.bfloat16), _t(64, 128, torch.float8_e4m3fn)), {}, "GPU memory"),
    ("linear_lora_w8_fwd", lambda: (_t(4, 128), _t(128, 128), None, None, None, 1.0), {}, "contiguous 2-D float8_e4m3fn"),
    ("linear_lora_w8_bwd", lambda: (None, _t(4, 128), None, _t(128, 128), None, None, 1.0), {}, "contiguous 2-D float8_e4m3fn"),
])
def test_ops_wrappers_check_before_the_library(fn, args, kw, words):
    from finetrainers_amd import ops

    with pytest.raises(ValueError, match=words.replace("[", r"\[").replace("]", r"\]")):
        getattr(ops, fn)(*args(), **kw)


def test_module_stores_the_weight_once_as_e4m3fn():
    from finetrainers_amd import MI355XFp8LoRALinear

    w = torch.randn(128, 256, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    w[0, :6] = torch.tensor([448.0, -448.0, 2.0**-9, -2.0**-9, 0.0, 2.0**-10], dtype=torch.bfloat16)  # the largest codes, the smallest subnormal, a tie to zero
    mod = MI355XFp8LoRALinear(w, torch.zeros(128), r=16, lora_alpha=32.0)
    sd = mod.state_dict()
    assert sd["weight"].dtype == torch.float8_e4m3fn and torch.equal(sd["weight"].view(torch.uint8), w.to(torch.float8_e4m3fn).view(torch.uint8))
    assert sorted(sd) == ["bias", "lora_A.default.weight", "lora_B.default.weight", "weight"] and sd["lora_A.default.weight"].dtype == torch.float32
    assert sd["lora_A.default.weight"].shape == (16, 256) and sd["lora_B.default.weight"].shape == (128, 16) and mod.padded_rank == 64 and mod.scaling == 2.0
    given = w.to(torch.float8_e4m3fn)
    assert MI355XFp8LoRALinear(given).weight.data_ptr() == given.data_ptr()  # an fp8 weight is taken as it is
