"""ops.gemm_nt_w8 / ops.gemm_nn_w8 (csrc/gemm_w8.hip: the weight operand is the stored e4m3fn bytes) per element against fp64 with the contract's bf16 rounding
points, and the LoRA linear built on them.  The up-cast e4m3 -> bf16 is exact, so the BOUND is the rule of tests/test_gpu_gemm_nn.py, restated, with no new
constant (u = 2^-24, ulp = the bf16 spacing):
  a rounding of a value v known to e moves by at most e + ulp(|v| + e);
  fp32 accumulation adds 2 u sum|terms| per product (the bias is one more term of the first), an fp32 product after the accumulator 2 u |result|;
  GELU' (epilogue 3): |bf(y)| (GRAD_ERR + 2^-20);  GELU (epilogue 1): e_o = 1.13 e_z + GELU_ERR + 2^-22 |o| (tests/test_gpu_gemm_contract.py derives both:
  the kernels' sigmoid form in fp32 on every finite bf16 against the fp64 tanh form, + the hardware exp2 / rcp; |gelu'| <= 1.13).
Reduction depths: one stage (64) and ring slots + 1 = 4 stages (256).  "wide": every operand, the fp8 weight included, is a strided view."""

import pytest
import torch

pytestmark = pytest.mark.gpu
bf16, fp8, U, BETA, KAPPA = torch.bfloat16, torch.float8_e4m3fn, 2.0**-24, 0.7978845608028654, 0.044715


def bfr(t):
    return t.float().to(bf16).to(t.dtype)


def ulp_bf(a):
    _, e = torch.frexp(a)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - 8), torch.zeros_like(a))


def gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(BETA * (x + KAPPA * x * x * x)))


def gelu_grad(x):
    th = torch.tanh(BETA * (x + KAPPA * x * x * x))
    return 0.5 * (1.0 + th) + 0.5 * x * (1.0 - th * th) * BETA * (1.0 + 3.0 * KAPPA * x * x)


def _formula_errors():  # csrc/common.hip.h gelu_tanh_f / gelu_tanh_grad_f in fp32 on every finite bf16 input against the fp64 tanh forms: largest absolute errors
    x = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(bf16).float()
    x = x[torch.isfinite(x) & (x.abs() <= 64)]
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    c1 = f(-2.0 * 1.4426950408889634 * BETA)
    s = 1.0 / (1.0 + torch.exp2(x * (c1 * f(KAPPA) * (x * x) + c1)))
    gd = s * (2.0 * ((x * (1.0 - s)) * (f(3.0 * KAPPA * BETA) * (x * x) + f(BETA))) + 1.0)
    return ((x * s).double() - gelu(x.double())).abs().max().item(), (gd.double() - gelu_grad(x.double())).abs().max().item()


GELU_ERR, GRAD_ERR = _formula_errors()
CODES = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8)  # the 254 finite e4m3fn codes


def view(rows, cols, wide, seed):  # unit-scale bf16 [rows, cols]: dense, or columns 8 .. 8 + cols of a buffer 24 columns wider
    t = torch.randn(rows, cols + (24 if wide else 0), generator=torch.Generator().manual_seed(seed)).to(bf16).cuda()
    return t[:, 8:8 + cols] if wide else t


def weight(rows, cols, wide, codes=False):  # fp8 [rows, cols]: randn rounded to e4m3fn, or every finite code; dense, or bytes 16 .. 16 + cols of rows 48 wider
    if codes:  # the table, permuted, repeated along both indices with steps coprime to 254
        idx = (torch.arange(rows)[:, None] * 37 + torch.arange(cols)[None, :] * 5) % 254
        w = CODES[torch.randperm(254, generator=torch.Generator().manual_seed(7))][idx].view(fp8)
    else:
        w = torch.randn(rows, cols, generator=torch.Generator().manual_seed(2)).to(fp8)
    buf = torch.zeros(rows, cols + (48 if wide else 0), dtype=torch.uint8).view(fp8).cuda()
    v = buf[:, 16:16 + cols] if wide else buf
    v.view(torch.uint8).copy_(w.view(torch.uint8))
    return v


d = lambda t: t.cpu().to(torch.float64)  # noqa: E731


def bounds(act, wm, bias, x2, w2, epi, aux):
    """fp64 references and bounds of epi(bf(act wm + bias) (+ x2 w2^T)) -> [(reference, bound), ...]: out, and the pre-activation for epilogue 1."""
    y = act @ wm + bias
    e = 2 * U * (act.abs() @ wm.abs() + bias.abs())
    if x2 is not None:
        e = e + ulp_bf(y.abs() + e) + 2 * U * (x2.abs() @ w2.abs().T)
        y = bfr(y) + x2 @ w2.T
    if epi == 0:
        return [(bfr(y), e + ulp_bf(y.abs() + e))]
    e = e + ulp_bf(y.abs() + e)  # the error of t = bf(y)
    t = bfr(y)
    if epi == 1:
        o = gelu(t)
        e_o = 1.13 * e + GELU_ERR + 2.0**-22 * o.abs()
        return [(bfr(o), e_o + ulp_bf(o.abs() + e_o)), (t, e)]
    gd = gelu_grad(aux)
    o = t * gd
    e_o = gd.abs() * e + t.abs() * (GRAD_ERR + 2.0**-20) + 2 * U * o.abs()
    return [(bfr(o), e_o + ulp_bf(o.abs() + e_o))]


@pytest.mark.parametrize("M,R,C,K2,side,wide", [(1, 64, 128, 0, 0, False), (130, 256, 128, 0, 1, False), (300, 256, 384, 0, 0, True), (300, 64, 384, 192, 0, False), (130, 256, 384, 192, 1, True),
          (1, 256, 384, 192, 1, False), (130, 64, 128, 192, 0, True), (300, 64, 128, 0, 1, True), (130, 256, 384, 0, 0, "codes")])  # R: reduction depth, C: output width; side: the kernel's second epilogue (NT: GELU, NN: GELU')
@pytest.mark.parametrize("kind", ["nt", "nn"])
def test_gemm_w8_against_fp64(kind, M, R, C, K2, side, wide):
    from finetrainers_amd import ops

    codes, wide = wide == "codes", wide is True
    act = view(M, R, wide, 1)
    w8 = weight(*((C, R) if kind == "nt" else (R, C)), wide, codes)
    x2, w2 = (view(M, K2, wide, 3), view(C, K2, wide, 4)) if K2 else (None, None)
    out = view(M, C, wide, 6)
    wm = d(w8).T if kind == "nt" else d(w8)  # (the CPU forms the fp64 weight from the bytes themselves)
    if kind == "nt":
        bias = None if M == 1 else view(1, C, wide, 8)[0]
        got = ops.gemm_nt_w8(act, w8, bias, out, x2=x2, w2=w2, gelu=bool(side))
        got, epi, aux = (got if side else (got,)), side, None
        bias = torch.zeros(C, dtype=torch.float64) if bias is None else d(bias)
    else:
        aux = view(M, C, wide, 5) if side else None
        got, epi, bias = (ops.gemm_nn_w8(act, w8, out, x2=x2, w2=w2, aux=aux),), 3 * side, torch.zeros(C, dtype=torch.float64)
    assert got[0] is out
    torch.cuda.synchronize()
    for g, (ref, bound) in zip(got, bounds(d(act), wm, bias, None if x2 is None else d(x2), None if w2 is None else d(w2), epi, None if aux is None else d(aux))):
        ratio = ((d(g) - ref).abs() / bound).max().item()
        print(f"gemm_{kind}_w8 M={M} R={R} C={C} K2={K2} epi={epi} wide={wide} codes={codes}: max |got - ref| / bound = {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("kind", ["nt", "nn"])
def test_gemm_w8_touches_nothing_outside_its_views(kind):
    from finetrainers_amd import ops

    M, R, C = 130, 192, 384  # NaN behind the last rows of the activation and the weight, beside their columns, and all around out
    wr, wc = (C, R) if kind == "nt" else (R, C)
    ab, ob = torch.full((M + 1, R + 16), float("nan"), dtype=bf16, device="cuda"), torch.full((M + 2, C + 16), float("nan"), dtype=bf16, device="cuda")
    wb = torch.full((wr + 1, wc + 16), 0x7F, dtype=torch.uint8, device="cuda").view(fp8)
    ab[:M, :R] = view(M, R, False, 1)
    wb[:wr, :wc].view(torch.uint8).copy_(weight(wr, wc, False).view(torch.uint8))
    (ops.gemm_nt_w8 if kind == "nt" else ops.gemm_nn_w8)(ab[:M, :R], wb[:wr, :wc], out=ob[1:M + 1, 8:8 + C])
    torch.cuda.synchronize()
    assert torch.isfinite(ob[1:M + 1, 8:8 + C]).all()
    ob[1:M + 1, 8:8 + C] = float("nan")
    assert torch.isnan(ob).all()


@pytest.mark.parametrize("kind", ["nt", "nn"])
def test_a_nan_byte_reaches_exactly_its_outputs(kind):
    from finetrainers_amd import ops

    M, R, C, col = 130, 256, 384, 200  # NT: row `col` of W is output column `col`;  NN: column `col` of W is output column `col`, whatever dy holds there (0 x NaN)
    act, w8 = view(M, R, False, 1), weight(*((C, R) if kind == "nt" else (R, C)), False)
    act[:, 77] = 0
    w8.view(torch.uint8)[(col, 77) if kind == "nt" else (77, col)] = 0xFF
    out = (ops.gemm_nt_w8 if kind == "nt" else ops.gemm_nn_w8)(act, w8)
    nan = torch.isnan(out)
    assert nan[:, col].all() and int(nan.sum()) == M


@pytest.mark.parametrize("KN,r", [(128, 0), (256, 64)])
def test_linear_lora_w8_against_the_bf16_pair(KN, r):
    """The w8 pair against the bf16 pair on ops.fp8_upcast(w8) and its transpose, M = 130: K = N = 128 for the plain linear; with adapters K = N = 256, the
    smallest the (hi, lo) down-projection both pairs share accepts (gemm_nt's split mode refuses K < 256, so neither pair runs r = 64 at 128).  y and dx: both kernels are within `bound` of one exact value, so they differ
    by at most 2 bound; the extension's operands are the same bits both ways (same down-projection), its sum|terms| is bounded by 1.02 s (|x| |A|^T) |B|^T
    (planes hi | lo | hi against hi, hi, lo: (1 + 2^-8)^2 + 2 2^-8 (1 + 2^-8) < 1.02) and the planes' own 2^-16 is added to e.  grad_a / grad_b: the same
    launches on bit-equal operands, 1e-6 of the largest element for the order of the fp32 atomics."""
    from finetrainers_amd import ops

    M, K, N, s = 130, KN, KN, 0.5
    x, dy, bias, w8 = view(M, K, False, 1), view(M, N, False, 9), view(1, N, False, 8)[0], weight(N, K, False)
    g = torch.Generator().manual_seed(5)
    A, B = ((0.1 * torch.randn(r, K, generator=g)).cuda(), (0.1 * torch.randn(N, r, generator=g)).cuda()) if r else (None, None)
    w = ops.fp8_upcast(w8)
    y8, xa8 = ops.linear_lora_w8_fwd(x, w8, bias, A, B, s)
    y16, xa16 = ops.linear_lora_fwd(x, w, bias, A, B, s)
    dx8, ga8, gb8 = ops.linear_lora_w8_bwd(x, dy, xa8, w8, A, B, s)
    dx16, ga16, gb16 = ops.linear_lora_bwd(x, dy, xa16, ops.transpose_bf16(w), A, B, s)
    torch.cuda.synchronize()
    Ad, Bd = (d(A), d(B)) if r else (None, None)
    for name, a8, a16, act, wm, b, fa, fb in (("y", y8, y16, d(x), d(w8).T, d(bias), r and Ad.T, r and Bd.T), ("dx", dx8, dx16, d(dy), d(w8), 0 * d(x)[0], Bd, Ad)):
        yv = act @ wm + b
        e = 2 * U * (act.abs() @ wm.abs() + b.abs())
        if r:
            lo, lo_abs = s * (act @ fa) @ fb, s * (act.abs() @ fa.abs()) @ fb.abs()
            e = e + ulp_bf(yv.abs() + e) + (2 * U * 1.02 + 2.0**-16) * lo_abs
            yv = bfr(yv) + lo
        ratio = ((d(a8) - d(a16)).abs() / (2 * (e + ulp_bf(yv.abs() + e)))).max().item()
        print(f"linear_lora_w8 r={r} {name}: max |w8 - bf16| / (2 bound) = {ratio:.3f}")
        assert ratio <= 1.0
    if r:
        assert torch.equal(xa8, xa16)
        for a8, a16 in ((ga8, ga16), (gb8, gb16)):
            assert (a8 - a16).abs().max().item() <= 1e-6 * a16.abs().max().item()


def test_fp8_lora_linear_module():
    """MI355XFp8LoRALinear at M = 130, K = N = 256 (the down-projection's smallest depth), r = 16 (padded to 64): loss.backward() against the fp64 graph x (W + s B A)^T.  dy = g exactly, so the adapter gradients are
    grad_B = g^T (s x A^T), grad_A = (s g B)^T x.  Bound per element: (2^-15 + (inner + M + 4) u) sum|terms| -- the (hi, lo) bf16 planes carry the fp32 factors
    and the down-projected rows to 2^-16 each, the down-projection sums `inner` (K resp. N) terms in fp32, the weight-gradient GEMM M terms (+ atomics)."""
    from finetrainers_amd import MI355XFp8LoRALinear

    M, K, N, r, alpha = 130, 256, 256, 16, 32.0
    gen = torch.Generator().manual_seed(3)
    wt = torch.randn(N, K, generator=gen).to(bf16)
    mod = MI355XFp8LoRALinear(wt.cuda(), view(1, N, False, 8)[0], r=r, lora_alpha=alpha)
    mod.lora_B["default"].weight.data.copy_(0.1 * torch.randn(N, r, generator=gen))
    sd = mod.state_dict()
    assert [k for k, v in sd.items() if v.dtype == fp8] == ["weight"] and not [k for k, v in sd.items() if v.dtype == bf16 and v.dim() == 2]
    assert torch.equal(sd["weight"].cpu().view(torch.uint8), wt.to(fp8).view(torch.uint8))
    x, g = view(M, K, False, 1).requires_grad_(), view(M, N, False, 9)
    (mod(x.view(2, M // 2, K)).view(M, N) * g).sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(x.grad).all()
    A, B, s = d(mod.lora_A["default"].weight.data), d(mod.lora_B["default"].weight.data), alpha / r
    xd, gd = d(x.detach()), d(g)
    for name, got, ref, mag, inner in (("lora_B", mod.lora_B["default"].weight.grad, gd.T @ (s * xd @ A.T), gd.abs().T @ (s * xd.abs() @ A.abs().T), K),
                                       ("lora_A", mod.lora_A["default"].weight.grad, (s * gd @ B).T @ xd, (s * gd.abs() @ B.abs()).T @ xd.abs(), N)):
        ratio = ((d(got) - ref).abs() / ((2.0**-15 + (inner + M + 4) * U) * mag)).max().item()
        print(f"MI355XFp8LoRALinear {name}.grad: max |got - fp64| / bound = {ratio:.3f}")
        assert ratio <= 1.0
