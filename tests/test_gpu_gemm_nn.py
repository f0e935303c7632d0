"""ops.gemm_nn (ftmi_gemm_nn) per element against fp64 with the contract's bf16 rounding points: y = bf(dy w); K2 > 0: y = bf(y) + x2 w2^T; epilogue 0:
out = bf(y); 3: out = bf(bf(y) * gelu_tanh'(aux)).  BOUND (the rule of tests/test_gpu_gemm_contract.py, restated), u = 2^-24, ulp = the bf16 spacing:
  a rounding of a value v known to e moves by at most e + ulp(|v| + e);
  fp32 accumulation adds 2 u sum|terms| per product (dy w, x2 w2^T), an fp32 product after the accumulator 2 u |result|;
  the GELU' factor adds |bf(y)| (GRAD_ERR + 2^-20): the kernels' sigmoid form in fp32 against the fp64 tanh form on every finite bf16, + the hardware exp2 / rcp.
Cases: M a lone row / a ragged tile / a ragged second tile; N one stage / three (the ring wraps); K one / three column tiles; extension, epilogue, strides."""

import pytest
import torch

pytestmark = pytest.mark.gpu
bf16, U = torch.bfloat16, 2.0**-24
BETA, KAPPA = 0.7978845608028654, 0.044715


def bfr(t):
    return t.float().to(bf16).to(t.dtype)


def ulp_bf(a):
    _, e = torch.frexp(a)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - 8), torch.zeros_like(a))


def gelu_grad(x):
    th = torch.tanh(BETA * (x + KAPPA * x * x * x))
    return 0.5 * (1.0 + th) + 0.5 * x * (1.0 - th * th) * BETA * (1.0 + 3.0 * KAPPA * x * x)


def _grad_err():  # csrc/common.hip.h gelu_tanh_grad_f in fp32 on every finite bf16 input against the fp64 tanh form: largest absolute error
    x = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(bf16).float()
    x = x[torch.isfinite(x) & (x.abs() <= 64)]
    c1 = torch.tensor(-2.0 * 1.4426950408889634 * BETA, dtype=torch.float32)
    s = 1.0 / (1.0 + torch.exp2(x * (c1 * torch.tensor(KAPPA, dtype=torch.float32) * (x * x) + c1)))
    gd = s * (2.0 * ((x * (1.0 - s)) * (torch.tensor(3.0 * KAPPA * BETA, dtype=torch.float32) * (x * x) + torch.tensor(BETA, dtype=torch.float32))) + 1.0)
    return (gd.double() - gelu_grad(x.double())).abs().max().item()


GRAD_ERR = _grad_err()


def view(rows, cols, wide, seed):  # unit-scale bf16 [rows, cols]: dense, or columns 8 .. 8 + cols of a buffer 24 columns wider
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(rows, cols + (24 if wide else 0), generator=g).to(bf16).cuda()
    return t[:, 8:8 + cols] if wide else t


@pytest.mark.parametrize("M,N,K,K2,epi,wide", [(1, 64, 128, 0, 0, False), (130, 192, 128, 0, 0, False), (300, 192, 384, 0, 0, True), (300, 64, 384, 192, 0, False), (130, 192, 384, 192, 3, True),
    (300, 192, 128, 0, 3, False), (1, 192, 384, 192, 3, False), (130, 64, 128, 192, 0, True), (300, 64, 128, 0, 3, True)])
def test_gemm_nn_against_fp64(M, N, K, K2, epi, wide):
    from finetrainers_amd import ops

    dy, w = view(M, N, wide, 1), view(N, K, wide, 2)
    x2, w2 = (view(M, K2, wide, 3), view(K, K2, wide, 4)) if K2 else (None, None)
    aux = view(M, K, wide, 5) if epi == 3 else None
    out = view(M, K, wide, 6)
    assert ops.gemm_nn(dy, w, out, x2=x2, w2=w2, aux=aux) is out
    torch.cuda.synchronize()
    d = lambda t: t.double().cpu()
    y = d(dy) @ d(w)
    e = 2 * U * (d(dy).abs() @ d(w).abs())
    if K2:
        e = e + ulp_bf(y.abs() + e) + 2 * U * (d(x2).abs() @ d(w2).abs().T)
        y = bfr(y) + d(x2) @ d(w2).T
    if epi == 3:
        e = e + ulp_bf(y.abs() + e)
        t, gd = bfr(y), gelu_grad(d(aux))
        y = t * gd
        e = gd.abs() * e + t.abs() * (GRAD_ERR + 2.0**-20) + 2 * U * y.abs()
    bound = e + ulp_bf(y.abs() + e)
    got = d(out)
    assert torch.isfinite(got).all()
    ratio = ((got - bfr(y)).abs() / bound).max().item()
    print(f"gemm_nn M={M} N={N} K={K} K2={K2} epi={epi} wide={wide}: max |got - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_gemm_nn_touches_nothing_outside_its_views():
    from finetrainers_amd import ops

    M, N, K = 130, 192, 384  # NaN behind the last rows of dy and w, beside their columns, and all around out
    nan = lambda r, c: torch.full((r, c), float("nan"), dtype=bf16, device="cuda")
    dyb, wb, ob = nan(M + 1, N + 16), nan(N + 1, K + 16), nan(M + 2, K + 16)
    dyb[:M, :N], wb[:N, :K] = view(M, N, False, 1), view(N, K, False, 2)
    ops.gemm_nn(dyb[:M, :N], wb[:N, :K], ob[1:M + 1, 8:8 + K])
    torch.cuda.synchronize()
    assert torch.isfinite(ob[1:M + 1, 8:8 + K]).all()
    ob[1:M + 1, 8:8 + K] = float("nan")
    assert torch.isnan(ob).all()
