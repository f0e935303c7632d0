"""The launch contract of the NT and TN GEMMs (csrc/kernels.h: GemmNtArgs / GemmTnArgs) per output tile against fp64, through ftmi_gemm_nt_ex / ftmi_gemm_tn_ex.

CONTRACT (read from gemm_nt_kernel / nt16_body / the skinny kernels / gemm_tn*_kernel in csrc/gemm.hip; bf() = round to nearest even to bf16, everything else fp32):
  NT   y = alpha * x.w^T + bias                        (the scaling and the bias in fp32 on the fp32 accumulator)
       K-extension (K2 > 0):  y = bf(y) + x2.w2^T      (the base is rounded BEFORE the extension is added: peft's bf16 base + fp32 LoRA)
       STORE  out = bf(y)
       GELU   out2 = bf(y), out = bf(gelu_tanh(out2))
       RESID  t = bf(y); gate: t = bf(t * gate[b, n]); out = bf(resid + t); out2 = bf(out * gate2[b, n]);  b = m // rows_per_batch
       DGELU  out = bf(bf(y) * gelu_tanh'(aux))
       split  t = alpha * (x.hi^T + x.lo^T) in fp32, W = the (hi, lo) bf16 planes of an fp32 matrix interleaved in groups of 32 rows; written as the three
              bf16 planes (hi(t), lo(t) = bf(t - hi(t)), hi(t)) per group of split_r outputs
       addressing: X columns of tile column n0 start at (n0 / xk_grp_n) * xk_grp_stride (X2: x2_grp_*); W row n at (n / w_grp_n) * w_grp_stride + (n % w_grp_n) * ldw
  TN   C[b] += scale * u[b]^T v[b] (fp32 atomics); U column of p = (p / u_grp_p) * u_grp_stride + p % u_grp_p; the V columns of row group p / v_grp_p start at
       (p / v_grp_p) * v_grp_stride; a folded operand (u_fold / v_fold = distance of its lo plane in columns) contributes hi^T.other + lo^T.other.
  The 32 x 32 kernels (gemm_nt_kernel, every tile shape and K loop), the 16 x 16 ones (nt16_body, every K loop) and the skinny kernels round at the same points:
  no two kernels of the family disagree on a rounding point (checked by reading; and every case below is judged by the one reference).

BOUNDS, per element, u = 2^-24, ulp(a) = the bf16 spacing at |a| (2^(floor(log2 a) - 7)):
  d      = (K + K2 + 4) u (|alpha| |x|.|w|^T + |x2|.|w2|^T + |bias|)          worst case of any fp32 summation order + the alpha / bias operations
  a rounding of a value v known to e moves by at most e + ulp(|v| + e); fp32 products / sums after the accumulator add 2 u |result|;
  pushed through the later steps with |gate|, |gate2|, |gelu_tanh'| <= 1.13 (GELU), |gelu_tanh'(aux)| (DGELU).  The sigmoid-form GELU of csrc/common.hip.h
  (x / (1 + exp2(x (c3 x^2 + c1)))) is evaluated here in fp32 on EVERY finite bf16 input against the fp64 tanh form (_formula_errors()): max abs error
  GELU_ERR for the function, GRAD_ERR for the derivative, to which 2^-22 |gelu| resp. 2^-20 is added for the hardware exp2 / rcp (1 ulp each instead of 0.5).
  TN     (M + 2) u |scale| |u|^T|v| (both planes) + 2 ceil(M / 64) u (|C0| + |scale| |u|^T|v|): at most one atomic add per 64-token step and plane into C.
         This worst-case bound grows with M (about 1.5e-2 on order-one elements at M = 5376): there a fault as small as a dropped lo plane of one tile is seen
         by the 1e-4 rel-L2 only; the per-element bound sees it at M = 333, where the seeded fault is shown.
  split  d + 2^-16 |t| for hi + lo (what lo cannot hold), the hi plane as a bf16 output, the third plane equal to the first.
  Asserted: |got - ref| <= bound for every element, every output finite, and for every block of 32 rows x 64 columns of a bf16 output (a ragged last row block of
  fewer than 8 rows joins the block above it; an output of fewer than 8 rows is one block) at most 2 % of the elements differ from the reference at all
  (test_gemm_nt_store's number, per block).  TN and hi + lo: the element bound and the existing rel-L2 figures (1e-4; 2e-5 for x A^T).
  The fp64 -> bf16 roundings of the reference go through fp32 (torch); the double rounding can move the reference by one ulp in ~2^-21 of the elements, which the
  bound allows for.

CPU SELF-CHECKS (unmarked tests at the end): the fp32 stand-ins (torch matmul; K in 64-chunks last to first, TN: eight partial sums) pass every bound with at
most 0.2 % per block; every seeded fault is rejected; the automatic cases reach every kernel the product build can choose; the tails pair every pinned
kernel with its own tile height; the library's own route (ftmi_gemm_nt_route, what gemm_nt() launches) has, for every case, the tile this file states.  (The production-size cases, M >= 1024 of TN and split mode and the automatic shapes, are not part of the CPU stand-in test:
their fp64 products belong on the GPU; the epilogue and addressing code they run is the same.)
  seeded fault                                   stands for
  bias from column n - 64 in the 2nd column tile  column offset of bias / gate / resid / aux / out2 in a second column tile
  gate of sample b - 1 in a straddling row tile   rows_per_batch, gate_bstride, gate2_bstride
  one 64-wide K stage dropped, one 16-row block   the K loop prologue / tail of a ragged row tile (ldx, ldw, K)
  resid read with ldo                             ldr / ldaux / ldo2 against ldo
  base not rounded before the K-extension         X2 / W2 / K2 rounding point
  out2 from the unrounded out                     gate2 / out2
  last M % 32 rows unwritten                      row tails (M, ldo)
  lo plane of a folded TN operand dropped         u_fold / v_fold
  batch 1 reads batch 0's V                       batch, u_bstride / v_bstride / c_bstride
  TN overwrites instead of adding                 the accumulate contract of C

CASES -> KERNEL (nt_route() of csrc/gemm.hip: split_r > 0 -> skinny2 / skinny4; N <= 256, plain store, M >= 512 -> skinny2 (K % 256 == 0) or skinny<4>; else by variant):
  tails      each of the 13 shipped variants at an N that is a multiple of its tile width (TILE below; on_own_kernel()), all 6 epilogue forms, M = h - 1, h + 1,
             2 h - 1, 2 h + 1 of ITS tile height h under two forms each, a short M (1 / 31 / 33) and a long one (449 / 1000); N over one, two and three column
             tiles, K over {64 .. 2112}, rows_per_batch over {1, 77, 150, M}, every stride padded                                        the pinned kernel (8: 128 x 128)
  n64        N = 64 / 192 under all 6 forms, any variant named                                                                              the 128 x 64 kernel
  fallback   the 256-wide variants at N = 384 / 640 (N % 256 != 0)                                                                           the 192 x 128 kernel
  samples    M = 449 / 1000, rows_per_batch 77 / 128 / 150 (boundaries on and off a tile edge), gate and gate2, every variant              the pinned kernel
  ext        K2 in {64, 192, 384} x 6 epilogue forms with x2 / w2 groups                                                                     as above, EXT kernels
  groups     xk_grp_n = w_grp_n in {64, 128, 256} x variants {8, 44, 47, 70, 80, 1386}                                                       128 x 64 / 128-wide / pinned
             (a variant that pins a 256-wide tile takes the 192 x 128 kernel over 128-wide groups: one rule of nt_route() for every row of the variant table)
  narrow     N <= 256, M >= 512, plain store                                                                                                 skinny2 / skinny<4>
  split      M in {1, 33, 300, 5400}, split_r in {64, 128}, grouped W, FTMI_SKINNY4 in {0, 1, 2}                                             skinny2 / skinny4<64> / <32>
  auto       the shapes of test_gemm_dispatch_rule_matches_the_design + M = 2688, 256, N = 1920, 192, all four epilogues, variant 8          80 / 87 / 1386 / 42 / 44 / 1 / 2
  tn         M in {1, 63, 65, 333, 5376}, P, Q from {64, 128, 192, 2048}, groups, folds, batches                                             tn_kernel / tn2 ring / 256-wide
  Variant 47 is never the automatic choice at the default switches (test_the_automatic_cases_reach_every_kernel: derivation and host scan of the plan).

MEASURED on an MI355X (largest |got - ref| / bound and largest block mismatch share per case group; a single flipped rounding costs one ulp against a bound of
one ulp + d, hence the figures just below 1):
  group         kernels reached                                                     err / bound   block share
  tails         every pinned variant on its own kernel (8: 128 x 128)                 0.998         0.0020
  n64           the 128 x 64 kernel                                                   0.679         0.0005
  fallback      the 192 x 128 kernel under the 256-wide variants                      0.991         0.0010
  samples       every pinned variant, residual epilogue with gate / gate2             0.979         0.0005
  ext           EXT kernels of every family, grouped X2 / W2                          0.913         0.0020
  groups        128 x 64 (64-wide groups), 128-wide tiles, pinned 256-wide            0.995         0.0020
  narrow        skinny2 (K % 256 == 0), skinny<4>                                     0.813         0.0020
  split         skinny2, skinny4<64>, skinny4<32>                                     0.975         0.0010
  auto          80 / 87 / 1386 / 42 / 44 / 128 x 64 / skinny, four epilogues each     0.919         0.0020
  plain entry   ftmi_gemm_nt with ld_side                                             0.790         0.0005
  tn            tn_kernel, tn2 ring (64 / 128 / 256 wide), 256 x 128 big tiles        0.492         -
  Every case is within its bounds.  The groups-v47 cases with 128-wide groups guard an eligibility rule of gemm_nt(): variant 47 takes its 256-wide tile only
  where 256-wide column groups allow it (it used to look at N % 256 alone and let a tile span two groups).
fp32 stand-ins on the CPU over the same case list (test_fp32_stand_ins_pass_every_bound): largest err / bound 0.996; largest block share 0.0020 (= 1 of 512) for
STORE and every RESID form, 0.0088 for GELU and 0.0059 for GELU' -- there the fp32 evaluation of the activation itself (not the product) crosses bf16 boundaries
where the function is small (|z| > 3), so these two forms are held to the 2 % cap only and their figure is printed; the 0.2 % holds for all the others.
"""

import math

import pytest
import torch

bf16 = torch.bfloat16
U = 2.0**-24
IN_SENT = 3.0e4     # padding of the inputs: wrecks the result if read as data
OUT_SENT = -1536.0  # padding of the outputs (exact in bf16): must survive the launch
EPI_STORE, EPI_GELU, EPI_RESID, EPI_DGELU = 0, 1, 2, 3
FORMS = ("store", "gelu", "resid", "resid_g", "resid_g2", "dgelu")
FORM_EPI = {"store": EPI_STORE, "gelu": EPI_GELU, "resid": EPI_RESID, "resid_g": EPI_RESID, "resid_g2": EPI_RESID, "dgelu": EPI_DGELU}
SHIPPED_VARIANTS = [8, 42, 44, 47, 70, 72, 80, 86, 87, 2286, 1386, 1387, 1380]  # tests/test_gpu_kernels.py
BETA, KAPPA = 0.7978845608028654, 0.044715


def _threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))


# ----------------------------------------------------------------------------------------------------
# number formats

def bfr(t):
    """Round to bf16 (nearest even), keep the dtype."""
    return t.float().to(bf16).to(t.dtype)


def ulp_bf(a):
    m, e = torch.frexp(a)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - 8), torch.zeros_like(a))


def gelu_t(x):
    return 0.5 * x * (1.0 + torch.tanh(BETA * (x + KAPPA * x * x * x)))


def gelu_grad_t(x):
    th = torch.tanh(BETA * (x + KAPPA * x * x * x))
    return 0.5 * (1.0 + th) + 0.5 * x * (1.0 - th * th) * BETA * (1.0 + 3.0 * KAPPA * x * x)


def _formula_errors():
    """The kernels' sigmoid-form GELU / GELU' (csrc/common.hip.h) in fp32 on every finite bf16 input against the fp64 tanh form: (max abs error, same for the grad)."""
    bits = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16)
    x = bits.view(bf16).float()
    x = x[torch.isfinite(x) & (x.abs() <= 1.0e4)]
    c1 = torch.tensor(-2.0 * 1.4426950408889634 * BETA, dtype=torch.float32)
    c3 = (c1 * torch.tensor(KAPPA, dtype=torch.float32))
    xsq = x * x
    s = 1.0 / (1.0 + torch.exp2(x * (c3 * xsq + c1)))
    g = x * s
    du = torch.tensor(3.0 * KAPPA * BETA, dtype=torch.float32) * xsq + torch.tensor(BETA, dtype=torch.float32)
    w = (x * (1.0 - s)) * du
    gd = s * (2.0 * w + 1.0)
    xd = x.double()
    ok = xd.abs() <= 64  # beyond: s saturates to exactly 0 / 1 in both (the fp64 tanh form evaluates x^3 exactly there too)
    return (g.double() - gelu_t(xd))[ok].abs().max().item(), (gd.double() - gelu_grad_t(xd))[ok].abs().max().item()


GELU_ERR, GRAD_ERR = _formula_errors()


# ----------------------------------------------------------------------------------------------------
# NT cases

def nt_case(M, N, K, form="store", variant=8, alpha=1.0, rpb=0, K2=0, xk_grp_n=0, w_grp_n=0, x2_grp_n=0, w2_grp_n=0, split_r=0, bias=True, seed=0, group="tails",
            cpu=True, sk4=None):
    return dict(M=M, N=N, K=K, form=form, variant=variant, alpha=alpha, rpb=rpb or M, K2=K2, xk_grp_n=xk_grp_n, w_grp_n=w_grp_n, x2_grp_n=x2_grp_n,
                w2_grp_n=w2_grp_n, split_r=split_r, bias=bias and not split_r, seed=seed, group=group, cpu=cpu, sk4=sk4)


def nt_id(c):
    s = f"{c['group']}-v{c['variant']}-{c['M']}x{c['N']}x{c['K']}-{c['form']}"
    if c["K2"]:
        s += f"-K2_{c['K2']}"
    if c["alpha"] != 1.0:
        s += f"-a{c['alpha']}"
    if c["rpb"] != c["M"]:
        s += f"-rpb{c['rpb']}"
    for k in ("xk_grp_n", "w_grp_n", "x2_grp_n", "w2_grp_n", "split_r"):
        if c[k]:
            s += f"-{k.replace('_grp_n', 'g')}{c[k]}"
    if c["sk4"] is not None:
        s += f"-sk4_{c['sk4']}"
    return s


TAIL_MS = [1, 31, 33, 127, 129, 191, 193, 223, 225, 255, 257, 449, 1000]
TAIL_KS = [64, 128, 192, 320, 2112]
# rows x columns of the tile a PINNED variant runs at an ungrouped N that is a multiple of its tile width (written against the variant table of csrc/gemm.hip and held
# against the library by test_the_library_routes_every_case_as_the_table_states; variant 8 is the automatic choice: 128 x 128 (44) at these small M).  Other wide N
# (N % 128 == 0) fall back to the 192 x 128 kernel, N % 128 != 0 takes the 128 x 64 kernel.
TILE = {8: (128, 128), 42: (192, 128), 44: (128, 128), 47: (256, 256), 70: (256, 256), 72: (256, 256), 80: (256, 256), 86: (192, 256), 87: (224, 256),
        2286: (192, 256), 1386: (192, 256), 1387: (224, 256), 1380: (256, 256)}


def on_own_kernel(c):
    """True if the launch of this (ungrouped, non-split) case runs the tile kernel its variant pins, with the tile of TILE[variant]."""
    skinny = c["N"] <= 256 and c["K2"] == 0 and c["form"] == "store" and c["M"] >= 512
    grouped = any(c[k] for k in ("xk_grp_n", "w_grp_n", "x2_grp_n", "w2_grp_n", "split_r"))
    return not skinny and not grouped and c["N"] % TILE[c["variant"]][1] == 0


def _nt_cases():
    cases = []
    # tails: every shipped variant runs all six epilogue forms ON ITS OWN KERNEL, at M one below and one above one and two tile heights of that kernel, a short
    # M and a long one; N over two and three column tiles (one tile for some), K over one, two, three stages, an odd stage count and a long K; all strides padded
    for vi, v in enumerate(SHIPPED_VARIANTS):
        h, wd = TILE[v]
        ms = [h - 1, h + 1, 2 * h - 1, 2 * h + 1, (1, 31, 33)[vi % 3], (1000, 449)[vi % 2]]
        ns = [2 * wd, 3 * wd, wd] if wd == 256 else [256, 384, 512, 768]
        for fi, form in enumerate(FORMS):
            i = vi * len(FORMS) + fi
            M = ms[(fi + vi) % 6]
            N = ns[(vi + fi) % len(ns)]
            if M < 8 and N < 512:
                N = 512  # (an output of fewer than 8 rows is ONE block: at least 512 elements)
            if N <= 256 and form == "store" and M >= 512:
                N = 512  # (a narrow plain store over many rows is the skinny route)
            K = TAIL_KS[(2 * vi + fi) % len(TAIL_KS)]
            cases.append(nt_case(M, N, K, form, v, alpha=(1.0, 0.5)[(vi + fi) % 2], rpb=(1, 77, 150, M)[i % 4], seed=i))
    # the same tails with the forms turned by three, so that every (kernel, M) pair is seen by two epilogue forms
    for vi, v in enumerate(SHIPPED_VARIANTS):
        h, wd = TILE[v]
        ms = [h - 1, h + 1, 2 * h - 1, 2 * h + 1]
        for mi, M in enumerate(ms):
            form = FORMS[(mi + vi + 3) % 6]
            N = (512, 768)[(vi + mi) % 2] if wd == 256 or (form == "store" and M >= 512) else (384, 512)[(vi + mi) % 2]
            cases.append(nt_case(M, N, TAIL_KS[(vi + mi + 1) % len(TAIL_KS)], form, v, alpha=(0.5, 1.0)[(vi + mi) % 2], rpb=(150, 77, M, 1)[(vi + mi) % 4], seed=1000 + 4 * vi + mi))
    # the 128 x 64 route (N % 128 != 0: N = 64, 192) under every form, whatever variant is named
    for fi, form in enumerate(FORMS):
        for ni, N in enumerate((64, 192)):
            i = 2 * fi + ni
            M = TAIL_MS[(5 * i + 3) % len(TAIL_MS)]
            if M < 8:
                M = 127
            cases.append(nt_case(M, N, TAIL_KS[i % len(TAIL_KS)], form, SHIPPED_VARIANTS[(3 * i) % len(SHIPPED_VARIANTS)], alpha=(1.0, 0.5)[i % 2], rpb=(77, 150, 1, M)[i % 4],
                                 seed=1100 + i, group="n64"))
    # the 192 x 128 fall-back of the variants that pin a 256-wide tile: a wide N that is no multiple of 256
    for vi, v in enumerate(v for v in SHIPPED_VARIANTS if TILE[v][1] == 256):
        cases.append(nt_case((191, 193, 383, 385, 1000)[vi % 5], (384, 640)[vi % 2], TAIL_KS[vi % len(TAIL_KS)], FORMS[vi % 6], v, alpha=(1.0, 0.5)[vi % 2], rpb=(77, 150)[vi % 2],
                             seed=1200 + vi, group="fallback"))
    # M = 1000 and 449 with several sample boundaries inside a row tile, one on a tile edge (rpb 128 -> 128, 256, ...) and off it
    for vi, v in enumerate(SHIPPED_VARIANTS):
        cases.append(nt_case((1000, 449)[vi % 2], (512, 768, 256)[vi % 3], (128, 320)[vi % 2], ("resid_g2", "resid_g")[vi % 2], v, alpha=0.5,
                             rpb=(77, 128, 150)[vi % 3], seed=100 + vi, group="samples"))
    # K-extension under every epilogue form, grouped X2 / W2
    for ki, K2 in enumerate((64, 192, 384)):
        for fi, form in enumerate(FORMS):
            i = ki * len(FORMS) + fi
            g = (0, 64, 128, 256)[i % 4]
            N = 512 if g != 0 else (256, 512, 768, 192)[i % 4]  # (192: the 128 x 64 kernel with a K-extension)
            cases.append(nt_case(TAIL_MS[(3 * i + 4) % len(TAIL_MS)] if i % 3 else 1000, N, (128, 192, 2112)[i % 3], form, SHIPPED_VARIANTS[i % len(SHIPPED_VARIANTS)],
                                 alpha=(1.0, 0.5)[i % 2], rpb=(150, 77)[i % 2], K2=K2, x2_grp_n=g, w2_grp_n=g, seed=200 + i, group="ext"))
    # column groups of X and W: the three eligibility classes of gemm_nt()
    for gi, g in enumerate((64, 128, 256)):
        for vi, v in enumerate((8, 44, 47, 70, 80, 1386)):
            i = gi * 6 + vi
            cases.append(nt_case((257, 1000, 449)[i % 3], 512, (128, 320)[i % 2], FORMS[i % len(FORMS)], v, rpb=150, xk_grp_n=g, w_grp_n=g, seed=300 + i, group="groups"))
    # the narrow-store skinny route (N <= 256, M >= 512, plain store): K % 256 == 0 and not
    for i, (M, N, K) in enumerate(((1000, 192, 2048), (1000, 256, 320), (513, 64, 512), (1000, 128, 2112))):
        cases.append(nt_case(M, N, K, "store", 8, alpha=(0.5, 1.0)[i % 2], seed=400 + i, group="narrow"))
    return cases


NT_CASES = _nt_cases()
SPLIT_CASES = [nt_case(M, 2 * No, K, "store", 8, alpha=(1.0, 0.5)[i % 2], w_grp_n=(0, 64, 128, 0)[i % 4] if r == 64 else (0, 128)[i % 2], split_r=r, seed=500 + i,
                       group="split", sk4=sk4, cpu=M < 1024)  # (cpu: part of the CPU stand-in test; the production-size products stay on the GPU)
               for i, (M, No, K, r, sk4) in enumerate([(1, 64, 256, 64, 1), (33, 128, 320, 64, 1), (300, 128, 2048, 128, 1), (5400, 64, 512, 64, 1), (5400, 64, 512, 64, 2),
                                                       (5400, 64, 512, 64, 0), (5400, 128, 2048, 128, 1), (5400, 128, 320, 64, 2), (300, 192, 256, 64, 0)])]
# the automatic choice at production shapes (M, N, K, K2), every epilogue; reference product in fp64 on the GPU
AUTO_SHAPES = [(5376, 6144, 2048, 192), (5376, 8192, 2048, 0), (5376, 2048, 8192, 0), (5376, 2048, 6144, 192), (5376, 2048, 2048, 192), (2688, 2048, 2048, 0),
               (256, 4096, 2048, 192), (5376, 1920, 1920, 0), (2688, 6144, 2048, 192), (256, 2048, 2048, 0), (256, 192, 2048, 0), (5376, 192, 2048, 0)]
AUTO_FORMS = ("store", "gelu", "resid_g2", "dgelu")
AUTO_MUST_REACH = {1, 2, 42, 44, 80, 87, 1386}


# ----------------------------------------------------------------------------------------------------
# NT inputs: backing tensors filled with a sentinel, the operands are views into them

def _grp_cols(G, width, stride):
    return torch.cat([torch.arange(width) + j * stride for j in range(G)])


def make_nt(c):
    """Returns dict: 'buf' name -> backing tensor (CPU), 'view' name -> (size, stride) of the operand inside it (offset 0), plus the launch fields."""
    g = torch.Generator().manual_seed(7000 + c["seed"])
    M, N, K, K2 = c["M"], c["N"], c["K"], c["K2"]
    buf, view, f = {}, {}, {}

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(bf16)

    def rows_operand(name, width, grp_n, kk):  # X / X2: [M, ld], column groups `kk + 16` apart
        G = N // grp_n if grp_n else 1
        stride = kk + 16
        ld = (G - 1) * stride + kk + 8
        b = torch.full((M + 2, ld), IN_SENT, dtype=bf16)
        for j in range(G):
            b[:M, j * stride:j * stride + kk] = rn(M, kk)
        buf[name], view[name] = b, ((M, kk), (ld, 1))
        return stride if grp_n else 0

    def weight_operand(name, rows, kk, grp_n, scale, data=None):  # W / W2: rows in groups of grp_n, w_grp_stride > grp_n * ld apart
        ld = kk + 64
        gn = grp_n if grp_n else rows
        G = rows // gn
        stride = gn * ld + 64
        b = torch.full((G * stride + ld,), IN_SENT, dtype=bf16)
        b.as_strided((G, gn, kk), (stride, ld, 1)).copy_((rn(rows, kk, scale=scale) if data is None else data).reshape(G, gn, kk))
        buf[name], view[name] = b, ((rows, kk), (ld, 1))
        return stride if grp_n else 0

    f["xk_grp_stride"] = rows_operand("x", K, c["xk_grp_n"], K)
    if c["split_r"]:
        w32 = torch.randn(N // 2, K, generator=g) / math.sqrt(K)
        hi = w32.to(bf16)
        lo = (w32 - hi.float()).to(bf16)
        inter = torch.stack([hi.reshape(-1, 32, K), lo.reshape(-1, 32, K)], 1).reshape(N, K)  # [hi 0-31 | lo 0-31 | hi 32-63 | ...]
        f["w_grp_stride"] = weight_operand("w", N, K, c["w_grp_n"], 1.0, inter)
    else:
        f["w_grp_stride"] = weight_operand("w", N, K, c["w_grp_n"], 1.0 / math.sqrt(K))
    if K2:
        f["x2_grp_stride"] = rows_operand("x2", K2, c["x2_grp_n"], K2)
        f["w2_grp_stride"] = weight_operand("w2", N, K2, c["w2_grp_n"], 1.0 / math.sqrt(K2))
    if c["bias"]:
        buf["bias"], view["bias"] = rn(N), ((N,), (1,))
    ncols_out = 3 * (N // 2) if c["split_r"] else N
    buf["out"], view["out"] = torch.full((M + 2, ncols_out + 8), OUT_SENT, dtype=bf16), ((M, ncols_out), (ncols_out + 8, 1))
    form = c["form"]
    nb = (M + c["rpb"] - 1) // c["rpb"]

    def side(name, ld, fill, data):
        b = torch.full((data.shape[0] + 2, ld), fill, dtype=bf16)
        if data is not None and fill == IN_SENT:
            b[:data.shape[0], :N] = data
        buf[name], view[name] = b, ((data.shape[0], N), (ld, 1))

    if form == "gelu" or form == "resid_g2":
        side("out2", N + 32, OUT_SENT, torch.empty(M, 0))
    if form.startswith("resid"):
        side("resid", N + 24, IN_SENT, rn(M, N))
    if form in ("resid_g", "resid_g2"):
        side("gate", N + 40, IN_SENT, rn(nb, N))
    if form == "resid_g2":
        side("gate2", N + 48, IN_SENT, rn(nb, N))
    if form == "dgelu":
        side("aux", N + 24, IN_SENT, rn(M, N, scale=1.5))
    return dict(case=c, buf=buf, view=view, fields=f)


def _view(inp, name, bufs=None):
    if name not in inp["view"]:
        return None
    size, stride = inp["view"][name]
    return (bufs or inp["buf"])[name].as_strided(size, stride)


def nt_logical(inp, dev="cpu"):
    """The dense operands the launch description denotes (gathered from the backing tensors), on `dev`."""
    c, f = inp["case"], inp["fields"]
    M, N, K, K2 = c["M"], c["N"], c["K"], c["K2"]
    L = {}

    def xs(name, kk, grp_n, stride):
        b = inp["buf"][name]
        G = N // grp_n if grp_n else 1
        return [b[:M, j * stride:j * stride + kk].to(dev) for j in range(G)]

    def ws(name, kk, grp_n, stride):
        b = inp["buf"][name]
        ld = kk + 64
        gn = grp_n if grp_n else N
        return b.as_strided((N // gn, gn, kk), (stride if grp_n else gn * ld + 64, ld, 1)).reshape(N, kk).to(dev)

    L["x"], L["w"] = xs("x", K, c["xk_grp_n"], f["xk_grp_stride"]), ws("w", K, c["w_grp_n"], f["w_grp_stride"])
    if K2:
        L["x2"], L["w2"] = xs("x2", K2, c["x2_grp_n"], f["x2_grp_stride"]), ws("w2", K2, c["w2_grp_n"], f["w2_grp_stride"])
    for n in ("bias", "resid", "gate", "gate2", "aux"):
        v = _view(inp, n)
        if v is not None:
            L[n] = v.to(dev)
    return L


# matrix products a [M, K] . b [N, K]^T in the precision / order under test
def mm64(a, b):
    return a.double() @ b.double().t()


def mm32(a, b):
    return (a.float() @ b.float().t())


def mm32_rev(a, b):
    K = a.shape[1]
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    for k0 in reversed(range(0, K, 64)):
        acc += a[:, k0:k0 + 64].float() @ b[:, k0:k0 + 64].float().t()
    return acc


def _product(xl, w, N, mm, absolute=False):
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t)
    if len(xl) == 1:
        return mm(f(xl[0]), f(w))
    gw = N // len(xl)
    return torch.cat([mm(f(xl[j]), f(w[j * gw:(j + 1) * gw])) for j in range(len(xl))], 1)


def nt_products(inp, L, mm):
    c = inp["case"]
    P = {"acc1": _product(L["x"], L["w"], c["N"], mm)}
    if c["K2"]:
        P["acc2"] = _product(L["x2"], L["w2"], c["N"], mm)
    return P


def nt_abs_products(inp, L):
    c = inp["case"]
    A = {"A1": _product(L["x"], L["w"], c["N"], mm64, True)}
    if c["K2"]:
        A["A2"] = _product(L["x2"], L["w2"], c["N"], mm64, True)
    return A


def _expand(gt, M, rpb, dt):
    idx = torch.arange(M, device=gt.device) // rpb
    return gt.to(dt)[idx]


def nt_contract(inp, L, P, dt=torch.float64, fault=None, form=None):
    """The contract after the products, in dtype dt (fp64: the reference; fp32: the stand-ins).  Returns the outputs and the intermediates the bounds need."""
    c = inp["case"]
    M, N = c["M"], c["N"]
    form = form or c["form"]
    acc1 = P["acc1"].to(dt)
    R = {}
    if c["split_r"]:
        # acc1 [M, N]: columns in groups of 64 = (hi 0-31 | lo 0-31); t = alpha * (hi part + lo part)
        a4 = acc1.reshape(M, N // 64, 2, 32)
        t = ((a4[:, :, 0] + a4[:, :, 1]) * c["alpha"]).reshape(M, N // 2)
        R["t"] = t
        return R
    bias = L["bias"].to(dt) if "bias" in L else torch.zeros(N, dtype=dt, device=acc1.device)
    if fault == "bias_col":
        bias = bias.clone()
        bias[256:] = L["bias"].to(dt)[192:N - 64]
    if fault == "k_stage":
        r0 = (M - 1) // 128 * 128  # first 16-row block of the tail tile, K stage 0
        acc1 = acc1.clone()
        acc1[r0:r0 + 16] -= (L["x"][0][r0:r0 + 16, :64].double() @ L["w"][:, :64].double().t()).to(dt)
    y0 = acc1 * c["alpha"] + bias
    R["y0"] = y0
    y = y0
    if c["K2"]:
        y = (y0 if fault == "base_unrounded" else bfr(y0)) + P["acc2"].to(dt)
    R["y"] = y
    if form == "store":
        R["out"] = bfr(y)
        if fault == "tail_rows" and M % 32:
            R["out"] = R["out"].clone()
            R["out"][M - M % 32:] = OUT_SENT
    elif form == "gelu":
        R["out2"] = bfr(y)
        R["o"] = torch.nn.functional.gelu(R["out2"], approximate="tanh") if dt == torch.float32 else gelu_t(R["out2"])
        R["out"] = bfr(R["o"])
    elif form == "dgelu":
        R["t"] = bfr(y)
        R["gd"] = gelu_grad_t(L["aux"].to(dt))
        R["p"] = R["t"] * R["gd"]
        R["out"] = bfr(R["p"])
    else:
        t = bfr(y)
        R["t"] = t
        if form in ("resid_g", "resid_g2"):
            gx = _expand(L["gate"], M, c["rpb"], dt)
            if fault == "gate_sample":
                rows = _straddling_tile_rows(M, c["rpb"], 128)
                idx = (torch.arange(M) // c["rpb"])
                idx[rows] = (idx[rows] - 1).clamp_min(0)
                gx = L["gate"].to(dt)[idx]
            R["g"] = gx
            R["p"] = t * gx
            t = bfr(R["p"])
        R["t2"] = t
        resid = L["resid"].to(dt)
        if fault == "resid_ld":  # read with ldo = N + 8 instead of ldr = N + 24 (inside the backing tensor)
            flat = inp["buf"]["resid"].reshape(-1)
            resid = flat.as_strided((M, N), (N + 8, 1)).to(dt)
        R["o"] = resid + t
        R["out"] = bfr(R["o"])
        if form == "resid_g2":
            R["g2"] = _expand(L["gate2"], M, c["rpb"], dt)
            R["q"] = (R["o"] if fault == "out2_unrounded" else R["out"]) * R["g2"]
            R["out2"] = bfr(R["q"])
    return R


def _straddling_tile_rows(M, rpb, tile):
    """Rows of the first `tile`-row tile that holds a sample boundary strictly inside it."""
    for t0 in range(0, M, tile):
        t1 = min(M, t0 + tile)
        if t0 // rpb != (t1 - 1) // rpb:
            return torch.arange(t0, t1)
    raise AssertionError("no row tile straddles a sample boundary")


def nt_bounds(inp, L, R, A, form=None):
    """Per-element bounds on |got - ref| for every output of the case (derivation: module docstring).  R: the fp64 contract."""
    c = inp["case"]
    form = form or c["form"]
    K, K2 = c["K"], c["K2"]
    al = abs(c["alpha"])
    if c["split_r"]:
        a4 = A["A1"].reshape(c["M"], c["N"] // 64, 2, 32)
        d = (K + 4) * U * al * (a4[:, :, 0] + a4[:, :, 1]).reshape(c["M"], c["N"] // 2)
        t = R["t"].abs()
        return {"t": d + 2.0**-16 * t, "hi": d + ulp_bf(t + d)}
    bias = L["bias"].double().abs() if "bias" in L else 0.0
    d = (K + K2 + 4) * U * (al * A["A1"] + (A["A2"] if K2 else 0.0) + bias)
    e_y = d + ulp_bf(R["y0"].abs() + d) if K2 else d
    B = {}
    rnd = lambda v, e: e + ulp_bf(v.abs() + e)
    if form == "store":
        B["out"] = rnd(R["y"], e_y)
    elif form == "gelu":
        e_z = rnd(R["y"], e_y)
        B["out2"] = e_z
        e_o = 1.13 * e_z + GELU_ERR + 2.0**-22 * R["o"].abs()
        B["out"] = rnd(R["o"], e_o)
    elif form == "dgelu":
        e_t = rnd(R["y"], e_y)
        e_p = R["gd"].abs() * e_t + R["t"].abs() * (GRAD_ERR + 2.0**-20) + 2 * U * R["p"].abs()
        B["out"] = rnd(R["p"], e_p)
    else:
        e_t = rnd(R["y"], e_y)
        if "g" in R:
            e_p = R["g"].abs() * e_t + 2 * U * R["p"].abs()
            e_t = rnd(R["p"], e_p)
        e_o = e_t + 2 * U * R["o"].abs()
        B["out"] = rnd(R["o"], e_o)
        if "q" in R:
            e_q = R["g2"].abs() * B["out"] + 2 * U * R["q"].abs()
            B["out2"] = rnd(R["q"], e_q)
    return B


# ----------------------------------------------------------------------------------------------------
# the checker

CAP = 0.02


def block_shares(mism):
    """mism [M, N] bool -> list of (share, r0, r1, c0, c1) over the 32 x 64 blocks (ragged last row block of < 8 rows joined to the one above; < 8 rows: one block)."""
    M, N = mism.shape
    m = mism.double()
    if M < 8 or N % 64:
        return [(m.mean().item(), 0, M, 0, N)]
    edges = list(range(0, M, 32)) + [M]
    if edges[-1] - edges[-2] < 8 and len(edges) > 2:
        del edges[-2]
    res = []
    for r0, r1 in zip(edges[:-1], edges[1:]):
        sh = m[r0:r1].reshape(r1 - r0, N // 64, 64).mean(dim=(0, 2))
        j = int(sh.argmax())
        res.append((sh[j].item(), r0, r1, j * 64, j * 64 + 64))
    return res


def judge(name, got, ref, bound, cap=CAP, exact=True, info=""):
    """got / ref / bound [M, N]; asserts finite, |got - ref| <= bound everywhere and (exact) the block mismatch cap.  Returns (max ratio, max share)."""
    got, ref = got.double(), ref.double()
    assert torch.isfinite(got).all(), f"{name}: non-finite output ({(~torch.isfinite(got)).sum().item()} entries) {info}"
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    worst = ratio.max().item()
    share, blk = 0.0, None
    if exact:
        share, *blk = max(block_shares(got != ref))
    print(f"[parity] {name:64s} max_err_over_bound={worst:.3f} max_block_mismatch={share:.4f}")
    if worst > 1.0:
        i = int(ratio.argmax())
        m_, n_ = i // got.shape[1], i % got.shape[1]
        bad = (ratio > 1.0)
        rows, cols = bad.any(1).nonzero().flatten(), bad.any(0).nonzero().flatten()
        raise AssertionError(f"{name}: element ({m_}, {n_}) got {got[m_, n_].item():.6g} ref {ref[m_, n_].item():.6g} bound {bound[m_, n_].item():.3g}; {int(bad.sum())} elements "
                             f"over their bound, rows {int(rows[0])}..{int(rows[-1])}, columns {int(cols[0])}..{int(cols[-1])} {info}")
    assert share <= cap, f"{name}: {share:.4f} of the block rows {blk[0]}..{blk[1] - 1} x columns {blk[2]}..{blk[3] - 1} differs from the reference (cap {cap}) {info}"
    return worst, share


def judge_nt(tag, inp, outs, R, B, cap=CAP, info=""):
    """outs: name -> [M, ncols] tensor of the launch (or of a stand-in / a faulted reference)."""
    c = inp["case"]
    res = []
    if c["split_r"]:
        r, M = c["split_r"], c["M"]
        o = outs["out"].double().reshape(M, -1, 3, r)
        hi, lo, hi2 = (o[:, :, i].reshape(M, -1) for i in range(3))
        assert torch.equal(hi, hi2), f"{tag}: the third plane differs from the first {info}"
        t = R["t"].double()
        res.append(judge(tag + " hi", hi, bfr(t), B["hi"], cap, True, info))
        res.append(judge(tag + " hi+lo", hi + lo, t, B["t"], cap, False, info))
        rel = ((hi + lo - t).norm() / t.norm().clamp_min(1e-300)).item()
        assert rel <= 2e-5, f"{tag}: hi + lo rel_l2 {rel:.3e} > 2e-5 {info}"
        return res
    for n in ("out", "out2"):
        if n in B:
            res.append(judge(f"{tag} {n}", outs[n], R[n], B[n], cap, True, info))
    return res


# ----------------------------------------------------------------------------------------------------
# GPU: launches

def _dev():
    return torch.device("cuda", 0)


@pytest.fixture
def sw():
    """Local copy of tests/test_gpu_kernels.py's switch fixture: set an FTMI_* switch for the rest of the test (ftmi_reload_switches() after every change)."""
    import os

    from finetrainers_amd import _lib

    saved = {}

    def set_(name, value):
        if name not in saved:
            saved[name] = os.environ.get(name)
        os.environ[name] = value
        _lib.load().ftmi_reload_switches()

    yield set_
    for k_, v_ in saved.items():
        if v_ is None:
            os.environ.pop(k_, None)
        else:
            os.environ[k_] = v_
    _lib.load().ftmi_reload_switches()


def launch_nt(inp, form=None, dev=None, bufs=None):
    """Runs the case; returns (outs: name -> [M, ncols] device views, bufs).  Checks afterwards that the padding of every output still holds the sentinel."""
    from finetrainers_amd import ops

    c, f = inp["case"], inp["fields"]
    form = form or c["form"]
    dev = dev or _dev()
    if bufs is None:
        bufs = {n: b.to(dev) for n, b in inp["buf"].items()}
    v = lambda n: _view(inp, n, bufs)
    kw = dict(M=c["M"], N=c["N"], K=c["K"], bias=v("bias"), alpha=c["alpha"], epilogue=FORM_EPI[form], variant=c["variant"], split_r=c["split_r"],
              xk_grp_n=c["xk_grp_n"], xk_grp_stride=f["xk_grp_stride"], w_grp_n=c["w_grp_n"], w_grp_stride=f["w_grp_stride"])
    if c["K2"]:
        kw.update(x2=v("x2"), w2=v("w2"), K2=c["K2"], x2_grp_n=c["x2_grp_n"], x2_grp_stride=f["x2_grp_stride"], w2_grp_n=c["w2_grp_n"], w2_grp_stride=f["w2_grp_stride"])
    if form.startswith("resid"):
        kw.update(resid=v("resid"), rows_per_batch=c["rpb"])
    if form in ("resid_g", "resid_g2"):
        kw.update(gate=v("gate"))
    if form == "resid_g2":
        kw.update(gate2=v("gate2"), out2=v("out2"))
    if form == "gelu":
        kw.update(out2=v("out2"))
    if form == "dgelu":
        kw.update(aux=v("aux"))
    ops.gemm_nt_ex(v("x"), v("w"), v("out"), **kw)
    torch.cuda.synchronize()
    outs = {}
    for n in ("out", "out2"):
        if n == "out" or n in kw:
            b = bufs[n]
            M, ncols = inp["view"][n][0]
            assert (b[M:] == OUT_SENT).all() and (b[:, ncols:] == OUT_SENT).all(), f"{nt_id(c)}: the launch wrote outside the [M, N] view of {n}"
            outs[n] = b[:M, :ncols]
    return outs, bufs


def _info(c):
    from finetrainers_amd import _lib

    plan = _lib.load().ftmi_gemm_nt_plan(c["M"], c["N"], c["K"], c["K2"], FORM_EPI[c["form"]])
    return f"[variant {c['variant']}, plan of the shape {plan}, fields { {k: v for k, v in c.items() if v and k not in ('group', 'cpu', 'seed')} }]"


def _run_nt_case(c):
    _threads()
    inp = make_nt(c)
    L = nt_logical(inp)
    R = nt_contract(inp, L, nt_products(inp, L, mm64))
    B = nt_bounds(inp, L, R, nt_abs_products(inp, L))
    outs, _ = launch_nt(inp)
    return judge_nt(nt_id(c), inp, {n: t.cpu() for n, t in outs.items()}, R, B, info=_info(c))


@pytest.mark.gpu
@pytest.mark.parametrize("c", NT_CASES, ids=nt_id)
def test_gemm_nt_contract(c):
    _run_nt_case(c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", SPLIT_CASES, ids=nt_id)
def test_gemm_nt_split_contract(c, sw):
    sw("FTMI_SKINNY4", str(c["sk4"]))
    _run_nt_case(c)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", AUTO_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_nt_contract_automatic_choice_at_production_shapes(shape):
    """Variant 8 at the shapes where the plan picks 80 / 87 / 1386 / 42 / 44 / 1 / 2, all four epilogues; the fp64 products are taken once per shape on the GPU."""
    M, N, K, K2 = shape
    dev = _dev()
    base = nt_case(M, N, K, "resid_g2", 8, alpha=0.5, rpb=(M + 6) // 7 if M >= 1024 else 77, K2=K2, seed=600 + N // 64 + K2, group="auto")
    inp = make_nt(base)
    dgelu_in = make_nt(dict(base, form="dgelu"))
    inp["buf"]["aux"], inp["view"]["aux"] = dgelu_in["buf"]["aux"], dgelu_in["view"]["aux"]
    L = nt_logical(inp, dev)
    P, A = nt_products(inp, L, mm64), nt_abs_products(inp, L)
    bufs = {n: b.to(dev) for n, b in inp["buf"].items()}
    for form in AUTO_FORMS:
        c = dict(base, form=form)
        inp["case"] = c
        R = nt_contract(inp, L, P, form=form)
        B = nt_bounds(inp, L, R, A, form=form)
        for n in ("out", "out2"):
            bufs[n].fill_(OUT_SENT)
        outs, _ = launch_nt(inp, form, dev, bufs)
        judge_nt(nt_id(c), inp, outs, R, B, info=_info(c))
        del R, B
    inp["case"] = base


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [8, 44, 80])
def test_gemm_nt_contract_through_the_plain_entry_point(variant):
    """The existing ops.gemm_nt(out=...) with strided x, w, out and a common side stride (ld_side)."""
    from finetrainers_amd import ops

    c = nt_case(449, 512, 320, "resid", variant, seed=650 + variant)
    inp = make_nt(c)
    L = nt_logical(inp)
    R = nt_contract(inp, L, nt_products(inp, L, mm64))
    B = nt_bounds(inp, L, R, nt_abs_products(inp, L))
    bufs = {n: b.to(_dev()) for n, b in inp["buf"].items()}
    v = lambda n: _view(inp, n, bufs)
    ops.gemm_nt(v("x"), v("w"), v("bias"), epilogue=EPI_RESID, resid=v("resid"), variant=variant, out=v("out"))
    torch.cuda.synchronize()
    assert (bufs["out"][449:] == OUT_SENT).all() and (bufs["out"][:, 512:] == OUT_SENT).all()
    judge_nt("plain entry " + nt_id(c), inp, {"out": bufs["out"][:449, :512].cpu()}, R, B)


# ----------------------------------------------------------------------------------------------------
# TN

def tn_case(M, P, Q, scale=1.0, u_grp=False, v_grp=False, fold=None, batch=1, shared=None, seed=0, cpu=True):
    return dict(M=M, P=P, Q=Q, scale=scale, u_grp=u_grp, v_grp=v_grp, fold=fold, batch=batch, shared=shared, seed=seed, cpu=cpu and M < 1024)


def tn_id(c):
    s = f"tn-{c['M']}x{c['P']}x{c['Q']}-s{c['scale']}"
    for k in ("u_grp", "v_grp"):
        if c[k]:
            s += "-" + k
    if c["fold"]:
        s += f"-fold_{c['fold']}"
    if c["batch"] > 1:
        s += f"-b{c['batch']}" + (f"-shared_{c['shared']}" if c["shared"] else "")
    return s


TN_CASES = [
    tn_case(1, 64, 64, seed=1), tn_case(63, 128, 64, 0.25, seed=2), tn_case(65, 64, 128, seed=3), tn_case(333, 192, 64, 0.25, seed=4), tn_case(333, 128, 192, seed=5),
    tn_case(5376, 2048, 64, 0.25, seed=6), tn_case(5376, 64, 2048, seed=7), tn_case(5376, 2048, 512, seed=8), tn_case(5376, 192, 128, 0.25, seed=9),
    tn_case(333, 128, 64, u_grp=True, seed=10), tn_case(5376, 2048, 64, u_grp=True, v_grp=True, seed=11), tn_case(65, 192, 64, v_grp=True, seed=12),
    tn_case(5376, 128, 64, v_grp=True, scale=0.25, seed=13),
    tn_case(333, 128, 64, fold="v", seed=14), tn_case(5376, 2048, 64, fold="v", seed=15), tn_case(63, 64, 128, fold="u", seed=16), tn_case(5376, 64, 2048, 0.25, fold="u", seed=17),
    tn_case(5376, 2048, 64, fold="v", v_grp=True, seed=18),
    tn_case(333, 128, 64, batch=2, seed=19), tn_case(5376, 2048, 64, batch=5, shared="v", fold="v", seed=20), tn_case(65, 64, 128, batch=5, shared="u", seed=21),
    tn_case(5376, 192, 64, 0.25, batch=2, shared="u", seed=22), tn_case(1, 128, 128, batch=2, shared="v", seed=23),
]
C_SENT = 777.0


def _tile_p(P, Q):
    return 256 if P % 256 == 0 else (128 if P % 128 == 0 else 64)


def make_tn(c):
    g = torch.Generator().manual_seed(9000 + c["seed"])
    M, P, Q, nb = c["M"], c["P"], c["Q"], c["batch"]
    gp = _tile_p(P, Q)  # group width of P (both operands' groups are groups of OUTPUT ROWS p)
    G = P // gp
    f = dict(u_grp_p=gp if c["u_grp"] else 0, v_grp_p=gp if c["v_grp"] else 0)
    ucols = _grp_cols(G, gp, gp + 16) if c["u_grp"] else torch.arange(P)
    f["u_grp_stride"] = gp + 16 if c["u_grp"] else 0
    uw = int(ucols[-1]) + 1
    vstarts = [j * (Q + 16) for j in range(G)] if c["v_grp"] else [0]
    f["v_grp_stride"] = Q + 16 if c["v_grp"] else 0
    vw = vstarts[-1] + Q
    f["u_fold"] = uw + 8 if c["fold"] == "u" else 0
    f["v_fold"] = vw + 8 if c["fold"] == "v" else 0
    ldu = (f["u_fold"] + uw if f["u_fold"] else uw) + 8
    ldv = (f["v_fold"] + vw if f["v_fold"] else vw) + 8
    nu, nv = (1 if c["shared"] == "u" else nb), (1 if c["shared"] == "v" else nb)
    ub = torch.full((nu, M + 1, ldu), IN_SENT, dtype=bf16)
    vb = torch.full((nv, M + 1, ldv), IN_SENT, dtype=bf16)

    def fill(b, cols, fold, scale):
        t = torch.randn(b.shape[0], M, len(cols), generator=g) * scale
        hi = t.to(bf16)
        b[:, :M, cols] = hi
        if fold:
            b[:, :M, cols + fold] = (t - hi.float()).to(bf16)

    fill(ub, ucols, f["u_fold"] if c["fold"] == "u" else 0, 1.0)
    vcols = torch.cat([torch.arange(Q) + s for s in vstarts])
    fill(vb, vcols, f["v_fold"] if c["fold"] == "v" else 0, 1.0 / math.sqrt(M))  # the update of C is of order one, like C0
    cb = torch.full((nb, P + 1, Q + 8), C_SENT, dtype=torch.float32)
    cb[:, :P, :Q] = torch.randn(nb, P, Q, generator=g)
    f.update(ldu=ldu, ldv=ldv, u_bstride=0 if c["shared"] == "u" else (M + 1) * ldu, v_bstride=0 if c["shared"] == "v" else (M + 1) * ldv, c_bstride=(P + 1) * (Q + 8))
    return dict(case=c, u=ub, v=vb, c=cb, fields=f, ucols=ucols, vstarts=vstarts, gp=gp)


def mm_tn64(u, v):
    return u.double().t() @ v.double()


def mm_tn32(u, v):
    return u.float().t() @ v.float()


def mm_tn32_parts(u, v):
    M = u.shape[0]
    parts = [u[i:j].float().t() @ v[i:j].float() for i, j in ((M * s // 8, M * (s + 1) // 8) for s in range(8)) if j > i]
    acc = parts[-1]
    for p in reversed(parts[:-1]):
        acc = acc + p
    return acc


def tn_contract(inp, mm, dt=torch.float64, fault=None, dev="cpu"):
    """Returns (C_ref [nb, P, Q] in dt, S = |u|^T|v| in fp64 (both planes)) on dev."""
    c, f = inp["case"], inp["fields"]
    M, P, Q, nb, gp = c["M"], c["P"], c["Q"], c["batch"], inp["gp"]
    out, S = [], []
    for b in range(nb):
        ub = inp["u"][0 if c["shared"] == "u" else b, :M].to(dev)
        vb_i = 0 if c["shared"] == "v" else b
        if fault == "batch_v" and b == 1:
            vb_i = 0
        vb = inp["v"][vb_i, :M].to(dev)
        uplanes = [ub[:, inp["ucols"]]] + ([ub[:, inp["ucols"] + f["u_fold"]]] if f["u_fold"] else [])
        prod = torch.zeros(P, Q, dtype=dt, device=dev)
        sabs = torch.zeros(P, Q, dtype=torch.float64, device=dev)
        for j, vs in enumerate(inp["vstarts"]):
            rows = slice(j * gp, (j + 1) * gp) if c["v_grp"] else slice(0, P)
            vplanes = [vb[:, vs:vs + Q]] + ([vb[:, vs + f["v_fold"]:vs + f["v_fold"] + Q]] if f["v_fold"] else [])
            for ui, up in enumerate(uplanes):
                for vi, vp in enumerate(vplanes):
                    sabs[rows] += mm_tn64(up[:, rows].abs(), vp.abs())
                    if fault == "lo_dropped" and (ui or vi) and j == 0:
                        prod[rows][64:] += mm(up[:, rows], vp).to(dt)[64:]  # the lo plane missing for the first 64 x Q tile
                        continue
                    prod[rows] += mm(up[:, rows], vp).to(dt)
        c0 = inp["c"][b, :P, :Q].to(dev).to(dt)
        out.append(prod * c["scale"] if fault == "overwrite" else c0 + prod * c["scale"])
        S.append(sabs)
    return torch.stack(out), torch.stack(S)


def tn_bound(inp, S, dev="cpu"):
    c = inp["case"]
    M, P, Q = c["M"], c["P"], c["Q"]
    sc = abs(c["scale"]) * S
    c0 = inp["c"][:, :P, :Q].to(dev).double().abs()
    return (M + 2) * U * sc + 2 * ((M + 63) // 64) * U * (c0 + sc)


def judge_tn(tag, inp, got, ref, bound):
    res = judge(tag, got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1]), bound.reshape(-1, bound.shape[-1]), exact=False)
    c = inp["case"]
    upd_g = got.double() - inp["c"][:, :c["P"], :c["Q"]].to(got.device).double()
    upd_r = ref.double() - inp["c"][:, :c["P"], :c["Q"]].to(got.device).double()
    rel = ((upd_g - upd_r).norm() / upd_r.norm().clamp_min(1e-300)).item()
    assert rel <= 1e-4, f"{tag}: rel_l2 of the update {rel:.3e} > 1e-4"
    return res


def launch_tn(inp, dev):
    from finetrainers_amd import ops

    c, f = inp["case"], inp["fields"]
    u, v, cc = inp["u"].to(dev), inp["v"].to(dev), inp["c"].to(dev)
    ops.gemm_tn_ex(u[0], v[0], cc[0], M=c["M"], P=c["P"], Q=c["Q"], scale=c["scale"], u_grp_p=f["u_grp_p"], u_grp_stride=f["u_grp_stride"], v_grp_p=f["v_grp_p"],
                   v_grp_stride=f["v_grp_stride"], u_fold=f["u_fold"], v_fold=f["v_fold"], batch=c["batch"], u_bstride=f["u_bstride"], v_bstride=f["v_bstride"],
                   c_bstride=f["c_bstride"])
    torch.cuda.synchronize()
    assert (cc[:, c["P"]:] == C_SENT).all() and (cc[:, :, c["Q"]:] == C_SENT).all(), f"{tn_id(c)}: the launch wrote outside the [P, Q] view of C"
    return cc[:, :c["P"], :c["Q"]]


@pytest.mark.gpu
@pytest.mark.parametrize("c", TN_CASES, ids=tn_id)
def test_gemm_tn_contract(c):
    _threads()
    dev = _dev()
    inp = make_tn(c)
    big = c["M"] * c["P"] * c["Q"] >= 2**30
    rdev = dev if big else "cpu"
    ref, S = tn_contract(inp, mm_tn64, dev=rdev)
    got = launch_tn(inp, dev)
    judge_tn(tn_id(c), inp, got.to(rdev), ref, tn_bound(inp, S, rdev))


# ----------------------------------------------------------------------------------------------------
# GPU: every documented refusal returns an error code and launches nothing

def _refusal_nt(match, **kw):
    from finetrainers_amd import ops

    dev = _dev()
    t = lambda: torch.full((256, 1024), 1.0, dtype=bf16, device=dev)
    x, w, out, side = t(), t(), torch.full((256, 1024), OUT_SENT, dtype=bf16, device=dev), t()
    args = dict(M=128, N=128, K=128)
    args.update(kw)
    for k in ("resid", "aux", "gate2", "x2", "w2", "bias"):
        if args.get(k) is True:
            args[k] = side
    if args.get("out2") is True:
        args["out2"] = torch.full((256, 1024), OUT_SENT, dtype=bf16, device=dev)
    with pytest.raises(ValueError, match=match):
        ops.gemm_nt_ex(x, w, out, **args)
    torch.cuda.synchronize()
    assert (out == OUT_SENT).all(), f"a refused launch wrote its output: {kw}"


@pytest.mark.gpu
def test_gemm_nt_ex_refusals():
    """Each refusal by the text the launcher / the entry point documents for it (csrc/gemm.hip gemm_nt(), csrc/api.hip)."""
    K64, LD, SPLIT = "K and K2 must be multiples of 64", "16-byte row alignment", r"split \(hi/lo\) mode"
    _refusal_nt(K64, K=100)                                                   # K % 64
    _refusal_nt(K64, K2=96, x2=True, w2=True)                                 # K2 % 64
    _refusal_nt("N must be a multiple of 64", N=100)                          # N % 64
    _refusal_nt(LD, _override={"ldx": 1028})                                  # ld % 8
    _refusal_nt(LD, _override={"ldw": 1028})
    _refusal_nt(LD, _override={"ldo": 1028})
    _refusal_nt(LD, K2=64, x2=True, w2=True, _override={"ldx2": 1028})
    _refusal_nt("weight group size must be a multiple of 64", w_grp_n=32, w_grp_stride=64 * 1024)
    _refusal_nt("group width must be a multiple of 64", N=192, xk_grp_n=32, xk_grp_stride=128)   # (the 128 x 64 route)
    _refusal_nt(SPLIT, K=256, split_r=64, bias=True)                          # split mode: no bias
    _refusal_nt(SPLIT, K=128, split_r=64)                                     # split mode: K >= 256
    _refusal_nt(SPLIT, K=256, split_r=64, epilogue=EPI_GELU)                  # split mode: plain store
    _refusal_nt(SPLIT, K=256, split_r=32)                                     # split mode: split_r % 64
    _refusal_nt(SPLIT, K=256, N=192, split_r=64)                              # split mode: whole groups of split_r outputs (N / 2 = 96)
    _refusal_nt("group width must be a multiple of 64", K=256, split_r=64, w_grp_n=32, w_grp_stride=64 * 1024)
    _refusal_nt("bad epilogue", epilogue=7)                                   # epilogue range
    _refusal_nt("residual epilogue without residual", epilogue=EPI_RESID)     # an epilogue without its input
    _refusal_nt("without pre-activation", epilogue=EPI_DGELU)
    _refusal_nt("without gate2", epilogue=EPI_RESID, resid=True, out2=True)   # out2 on the residual epilogue without gate2
    _refusal_nt("K-extension without its operands", K2=64)
    _refusal_nt("stream-K kernel", variant=60)                                # not in the product build


@pytest.mark.gpu
def test_gemm_tn_ex_refusals():
    from finetrainers_amd import ops

    dev = _dev()
    u = torch.full((128, 1024), 1.0, dtype=bf16, device=dev)
    v = torch.full((128, 1024), 1.0, dtype=bf16, device=dev)
    P64, LD = "P and Q must be multiples of 64", "16-byte row alignment"
    for match, kw in ((P64, dict(P=100)), (P64, dict(Q=100)), (LD, dict(_override={"ldu": 1028})), (LD, dict(_override={"ldv": 1028})),
                      ("gemm_tn: group width vs tile", dict(P=128, v_grp_p=64, v_grp_stride=64)), ("U group width vs tile", dict(P=128, u_grp_p=64, u_grp_stride=80)),
                      ("only one operand may be", dict(u_fold=256, v_fold=256))):
        c = torch.full((256, 256), C_SENT, dtype=torch.float32, device=dev)
        args = dict(M=128, P=64, Q=64)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.gemm_tn_ex(u, v, c, **args)
        torch.cuda.synchronize()
        assert (c == C_SENT).all(), f"a refused launch wrote C: {kw}"


# ----------------------------------------------------------------------------------------------------
# CPU: the checker, the inputs and the bounds judge themselves (no GPU; runs under -m "not gpu")

STANDIN_CAP = 0.002


def _cpu_nt_cases():
    return [c for c in NT_CASES + SPLIT_CASES if c["cpu"]]


def test_fp32_stand_ins_pass_every_bound():
    """The contract evaluated in fp32 on the CPU in two summation orders passes every element bound and stays at or below 0.2 % mismatches in every block (a
    tenth of the cap), over every case flagged cpu (all but the production-size ones).  Measured over this case list: see the [parity] lines (pytest -s); the largest block share of any stand-in is recorded in the docstring."""
    _threads()
    worst, by_form = [0.0, 0.0], {}
    for c in _cpu_nt_cases():
        inp = make_nt(c)
        L = nt_logical(inp)
        R = nt_contract(inp, L, nt_products(inp, L, mm64))
        B = nt_bounds(inp, L, R, nt_abs_products(inp, L))
        for name, mm in (("torch", mm32), ("rev64", mm32_rev)):
            S = nt_contract(inp, L, nt_products(inp, L, mm), dt=torch.float32)
            if c["split_r"]:
                t = S["t"]
                hi = t.to(bf16)
                lo = (t - hi.float()).to(bf16)
                outs = {"out": torch.stack([hi.reshape(c["M"], -1, c["split_r"]), lo.reshape(c["M"], -1, c["split_r"]), hi.reshape(c["M"], -1, c["split_r"])], 2).reshape(c["M"], -1)}
            else:
                outs = {n: S[n] for n in ("out", "out2") if n in S}
            for r_, s_ in judge_nt(f"standin {name} {nt_id(c)}", inp, outs, R, B, cap=CAP):
                worst = [max(worst[0], r_), max(worst[1], s_)]
                by_form[c["form"]] = max(by_form.get(c["form"], 0.0), s_)
                # (GELU / GELU': the fp32 evaluation of the activation itself moves results across bf16 boundaries where the function is small -- measured,
                #  reported, held to the 2 % cap only; see the module docstring)
                assert s_ <= STANDIN_CAP or c["form"] in ("gelu", "dgelu"), f"standin {name} {nt_id(c)}: block mismatch share {s_:.4f} > {STANDIN_CAP}"
    for c in TN_CASES:
        if not c["cpu"]:
            continue
        inp = make_tn(c)
        ref, S = tn_contract(inp, mm_tn64)
        for name, mm in (("torch", mm_tn32), ("parts8", mm_tn32_parts)):
            got, _ = tn_contract(inp, mm, dt=torch.float32)
            for r_, s_ in [judge_tn(f"standin {name} {tn_id(c)}", inp, got, ref, tn_bound(inp, S))]:
                worst[0] = max(worst[0], r_)
    print(f"[parity] fp32 stand-ins: largest err/bound {worst[0]:.3f}, largest block mismatch share {worst[1]:.4f}, per epilogue form { {k: round(v, 4) for k, v in by_form.items()} }")


def _find(pred, cases=None):
    for c in (cases or NT_CASES):
        if pred(c):
            return c
    raise AssertionError("no case carries the fields this fault needs")


def _rejected(c, fault, form=None):
    inp = make_nt(c)
    L = nt_logical(inp)
    P, A = nt_products(inp, L, mm64), nt_abs_products(inp, L)
    R = nt_contract(inp, L, P)
    B = nt_bounds(inp, L, R, A)
    judge_nt("clean " + nt_id(c), inp, R, R, B)  # the reference passes its own check
    Fd = nt_contract(inp, L, P, fault=fault)
    with pytest.raises(AssertionError):
        judge_nt(f"fault {fault} " + nt_id(c), inp, Fd, R, B)


def test_seeded_faults_fail():
    """Each fault this file exists for, applied to the fp64 reference, is rejected by the checker (table in the module docstring)."""
    _threads()
    _rejected(_find(lambda c: c["N"] >= 512 and c["bias"] and not c["K2"] and c["group"] == "tails"), "bias_col")
    _rejected(_find(lambda c: c["form"] in ("resid_g", "resid_g2") and c["M"] >= 449 and c["rpb"] in (77, 150)), "gate_sample")
    _rejected(_find(lambda c: c["M"] % 128 >= 16 and c["M"] > 128 and not c["xk_grp_n"] and c["K"] >= 128 and c["group"] == "tails"), "k_stage")
    _rejected(_find(lambda c: c["form"].startswith("resid") and c["M"] >= 31), "resid_ld")
    for form in FORMS:
        _rejected(_find(lambda c: c["K2"] and c["form"] == form), "base_unrounded")
    _rejected(_find(lambda c: c["form"] == "resid_g2"), "out2_unrounded")
    _rejected(_find(lambda c: c["form"] == "store" and c["M"] % 32 and not c["split_r"] and c["M"] > 32), "tail_rows")
    for pred, fault in ((lambda c: c["fold"] and c["M"] >= 333, "lo_dropped"), (lambda c: c["batch"] >= 2 and c["shared"] != "v" and c["M"] <= 333, "batch_v"),
                        (lambda c: c["M"] == 333, "overwrite")):
        c = _find(pred, TN_CASES)
        inp = make_tn(c)
        ref, S = tn_contract(inp, mm_tn64)
        judge_tn("clean " + tn_id(c), inp, ref, ref, tn_bound(inp, S))
        bad, _ = tn_contract(inp, mm_tn64, fault=fault)
        with pytest.raises(AssertionError):
            judge_tn(f"fault {fault} " + tn_id(c), inp, bad, ref, tn_bound(inp, S))


def test_case_inputs_are_order_one_and_distinct():
    """bias / gate / gate2 / resid / aux differ in every row, column and sample (a wrong index moves an element by far more than its bound), the strides differ
    from the widths and from each other; and the (tile height, M) pairing of the tails: each pinned kernel gets M = h - 1, h + 1, 2 h - 1, 2 h + 1 of its own tile height h,
    under two epilogue forms each, and all six forms, at an N that keeps the launch on that kernel (on_own_kernel: mirrors the routing of gemm_nt())."""
    for c in NT_CASES[:24]:
        inp = make_nt(c)
        for n in ("bias", "gate", "gate2", "resid", "aux"):
            v = _view(inp, n)
            if v is None:
                continue
            v = v.float()
            assert 0.5 < v.std().item() < 2.5 and (v.abs() < 100).all(), (nt_id(c), n)
            if v.dim() == 2 and v.shape[0] > 1:
                assert (v[1:] != v[:-1]).float().mean() > 0.9, (nt_id(c), n)
        lds = [inp["view"][n][1][0] for n in inp["view"] if n not in ("bias",)]
        assert all(ld % 8 == 0 for ld in lds)
        widths = {"x": c["K"], "w": c["K"], "out": c["N"]}
        for n, wd in widths.items():
            assert inp["view"][n][1][0] != wd
    # every pinned variant runs all six epilogue forms on its own kernel, and that kernel sees M one below and one above one and two of ITS tile heights
    for v in SHIPPED_VARIANTS:
        own = [c for c in NT_CASES if c["variant"] == v and c["group"] == "tails" and on_own_kernel(c)]
        h = TILE[v][0]
        assert {c["form"] for c in own} == set(FORMS), v
        assert {h - 1, h + 1, 2 * h - 1, 2 * h + 1} <= {c["M"] for c in own}, v
        for M in (h - 1, h + 1, 2 * h - 1, 2 * h + 1):
            assert len({c["form"] for c in own if c["M"] == M}) >= 2, (v, M)
        assert any(c["N"] // TILE[v][1] >= 3 for c in own) and any(c["N"] // TILE[v][1] == 2 for c in own), v  # second and third column tile
    assert {TILE[v][0] for v in SHIPPED_VARIANTS} == {128, 192, 224, 256}
    assert set(TAIL_MS) <= {c["M"] for c in NT_CASES}  # the row counts the issue lists all occur
    assert {c["form"] for c in NT_CASES if c["group"] == "n64"} == set(FORMS) and {c["N"] for c in NT_CASES if c["group"] == "n64"} == {64, 192}
    assert all(c["N"] % 256 and c["N"] % 128 == 0 for c in NT_CASES if c["group"] == "fallback")


@pytest.fixture(scope="module")
def lib():
    from finetrainers_amd import _lib

    if not _lib.lib_available():
        from finetrainers_amd.csrc.build import build

        build()
    return _lib.load()


def test_the_automatic_cases_reach_every_kernel(lib):
    """Through ftmi_gemm_nt_plan (host only): the automatic cases return, between them, every variant the product build chooses at the default switches.
    47 (256 x 256, 8 waves) is only a candidate of the cost model in the last branch of nt_auto_variant(), entered with 256-wide tiles allowed only when the
    16 x 16 pipeline was refused: M >= 1024, one short round with fewer than 192 tiles of 192 x 256 and n192 = 2 t192 >= 342, i.e. 171 <= ceil(M / 192) * (N / 256) < 192.
    There the model prices 42 at two rounds of 1618 = 3236 units and 47 at one round of 3408, and takes 47 only below 0.97 x 3236: never.  At the default switches
    NO shape reaches 47 automatically (the scan below confirms it on the plan); the pinned variant 47 runs in the tails / samples / ext / groups cases."""
    reached = set()
    for (M, N, K, K2) in AUTO_SHAPES:
        for form in AUTO_FORMS:
            reached.add(lib.ftmi_gemm_nt_plan(M, N, K, K2, FORM_EPI[form]))
    assert AUTO_MUST_REACH <= reached, AUTO_MUST_REACH - reached
    assert lib.ftmi_gemm_nt_plan(5376, 2048, 100, 0, 0) == 0  # not a tiled launch: refused (test_gemm_nt_ex_refusals)
    assert scan_for_47(lib) is None  # a spot check of the window (M = whole 192-row tiles, K2 = 0, four K): the statement rests on the derivation above


def scan_for_47(lib):
    for N in range(256, 8192 + 1, 256):
        for tm in range(1, 192 * 256 // N + 2):
            t = tm * (N // 256)
            if not (171 <= t < 192):
                continue
            M = tm * 192
            if M < 1024:
                continue
            for K in (64, 256, 1024, 2048):
                for epi in range(4):
                    if lib.ftmi_gemm_nt_plan(M, N, K, 0, epi) == 47:
                        return (M, N, K, 0, epi)
    return None


SKINNY_KINDS = {3, 4, 5, 6, 7}  # include/ftmi355.h, ftmi_gemm_nt_route: LDS ring, direct gather x 4 / x 8, 64-row split kernel with 64- / 32-deep stages


def stated_tile(c):
    """What this file says the launch of case c runs: "skinny", or rows x columns of a tiled kernel.  For ungrouped cases this is TILE / on_own_kernel() and the two
    fall-backs stated above TILE; column groups count like N (module docstring, groups: 128 x 64 / 128-wide / pinned)."""
    if c["split_r"] or (c["N"] <= 256 and c["K2"] == 0 and c["form"] == "store" and c["M"] >= 512):
        return "skinny"
    fits = lambda wd: all(v % wd == 0 for v in (c["N"], c["xk_grp_n"], c["w_grp_n"], c["x2_grp_n"], c["w2_grp_n"]))
    if not fits(128):
        return (128, 64)
    return TILE[c["variant"]] if fits(TILE[c["variant"]][1]) else (192, 128)


def test_the_library_routes_every_case_as_the_table_states(lib, sw):
    """ftmi_gemm_nt_route (host only; gemm_nt() launches what it returns) for EVERY case of NT_CASES, SPLIT_CASES and the automatic shapes: the tile is the one
    TILE / on_own_kernel() state -- TILE[variant] on the variant's own kernel, 192 x 128 for other wide N, 128 x 64 for N % 128 != 0, a skinny kernel for the narrow
    stores and split mode -- and the resolved variant is the pinned one, 42 after the fall-back.  The automatic shapes: the route is the plan's code, with TILE's tile."""
    from finetrainers_amd import ops

    def route(c):
        inp_ld = {n: 8 * ((w + 15) // 8) for n, w in (("ldx", c["K"]), ("ldw", c["K"]), ("ldo", c["N"]), ("ldx2", c["K2"]), ("ldw2", c["K2"]))}  # padded, 16-byte rows
        return ops.gemm_nt_route(M=c["M"], N=c["N"], K=c["K"], K2=c["K2"], epilogue=FORM_EPI[c["form"]], variant=c["variant"], split_r=c["split_r"],
                                 xk_grp_n=c["xk_grp_n"], w_grp_n=c["w_grp_n"], x2_grp_n=c["x2_grp_n"], w2_grp_n=c["w2_grp_n"], **inp_ld)

    own = set()
    for c in NT_CASES:
        kind, variant, bm, bn = route(c)
        want = stated_tile(c)
        if on_own_kernel(c):
            assert want == TILE[c["variant"]], nt_id(c)
            own.add(c["variant"])
        if want == "skinny":
            assert kind in SKINNY_KINDS and not on_own_kernel(c), (nt_id(c), kind)
        else:
            assert (bm, bn) == want, (nt_id(c), kind, variant, (bm, bn), want)
            assert kind == (2 if want == (128, 64) else 1), (nt_id(c), kind)
            if kind == 1:
                assert variant == ((44 if c["variant"] == 8 else c["variant"]) if want == TILE[c["variant"]] else 42), (nt_id(c), variant)
    assert own == set(SHIPPED_VARIANTS)
    kinds = set()
    for c in SPLIT_CASES:
        sw("FTMI_SKINNY4", str(c["sk4"]))
        kind, variant, bm, bn = route(c)
        assert stated_tile(c) == "skinny" and kind in SKINNY_KINDS and bn == 64, (nt_id(c), kind)
        assert (kind in (6, 7)) == (bm == 64) and (c["sk4"] != 0 or kind == 3), (nt_id(c), kind, bm)  # FTMI_SKINNY4=0: the 32-row LDS-ring kernel
        kinds.add(kind)
    assert kinds == {3, 6, 7}  # skinny2 / skinny4<64> / skinny4<32> (module docstring, split)
    sw("FTMI_SKINNY4", "1")
    reached = set()
    for (M, N, K, K2) in AUTO_SHAPES:
        for form in AUTO_FORMS:
            kind, variant, bm, bn = route(nt_case(M, N, K, form, 8, K2=K2))
            plan = lib.ftmi_gemm_nt_plan(M, N, K, K2, FORM_EPI[form])
            reached.add(plan)
            if plan == 2:
                assert kind in SKINNY_KINDS, (M, N, K, K2, form, kind)
            elif plan == 1:
                assert (kind, bm, bn) == (2, 128, 64), (M, N, K, K2, form, kind, bm, bn)
            else:
                assert (kind, variant) == (1, plan) and (bm, bn) == TILE[plan], (M, N, K, K2, form, kind, variant, bm, bn)
    assert AUTO_MUST_REACH <= reached
    with pytest.raises(ValueError, match="multiples of 64"):
        ops.gemm_nt_route(M=5376, N=2048, K=100)  # refused like the launch (test_gemm_nt_ex_refusals)
