"""The refusals of ftmi_gemm_nn (include/ftmi355.h), on the host: every call returns before a launch, so the pointers are host addresses that are never read."""

import ctypes

import pytest

from test_attention_refusals_host import BASE, INVALID, UNSUPPORTED, lib, refused  # noqa: F401  (lib: the library fixture)


def call(lib, **kw):
    from finetrainers_amd import _lib

    f = dict(dy=BASE, lddy=192, w=BASE + 16, ldw=256, M=5, N=192, K=256, x2=BASE + 32, ldx2=64, w2=BASE + 48, ldw2=64, K2=64, aux=BASE + 64, ldaux=256,
             out=BASE + 80, ldo=256, epilogue=3)
    f.update(kw)
    return lib.ftmi_gemm_nn(ctypes.byref(_lib.GemmNnArgs(**f)), None)


@pytest.mark.parametrize("fields,code,words", [
    (dict(N=160, lddy=160), UNSUPPORTED, ("N", "multiple of 64")),
    (dict(K=192), UNSUPPORTED, ("K", "multiple of 128")),
    (dict(K2=96, ldx2=96, ldw2=96), UNSUPPORTED, ("K2 must be a multiple of 64",)),
    (dict(aux=None), INVALID, ("gelu' epilogue without pre-activation",)),
    (dict(w=None), INVALID, ("null tensor",)),
    (dict(ldw=260), INVALID, ("leading dimensions", "16-byte")),
    (dict(w=BASE + 24), INVALID, ("16-byte alignment",)),
    (dict(ldo=128), INVALID, ("smaller than its row",)),
])
def test_gemm_nn_refusals(lib, fields, code, words):
    refused(lib, call(lib, **fields), code, "gemm_nn", *words)
