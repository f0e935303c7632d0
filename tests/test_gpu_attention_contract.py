"""The launch contract of the attention kernels (csrc/attention.hip, csrc/attention_pl.hip.h, csrc/attn_ctx2.hip) per row and element against fp64.

CONTRACT (read from the kernels; bf() = round to nearest even to bf16, everything else fp32; sl = fp32(scale * log2 e); b2[b, h, j] = fp32(key_bias * log2 e), 0
without a bias; s_ij = q_i . k_j summed over head_dim in fp32 by the matrix pipe; the softmax lives in the log2 domain; tiles are 64 keys / 64 query rows)
  forward (attn_fwd_kernel, head_dim 64 and 128, biased / ragged / whole)
    x_ij = fma(s_ij, sl, b2_j) (biased) or s_ij sl inside the exp2 argument (no bias); per tile a reference maximum m (the running row maximum, raised only when
    some row of the wave outgrew it by more than 8: "lazy rescale", so p <= 2^8), p_ij = bf(exp2(x_ij - m)) -- ROUNDED to bf16 before P V and before the sum
    l = sum_j p_ij that the matrix pipe forms from the same bf16 numbers; O and l are rescaled by exp2(m_old - m_new) when m moves.
    out = bf(acc * (1 / l)) (one rounding), lse = m + log2(l) in the LOG2 domain (fp32, [B, H, Sq] contiguous).
    Padded keys (j >= Sk of the last tile): their rows are a re-read of the last real key (tile DMA clamps), never memory past Sk; their score is -inf (b2 = -inf
    on the biased path, a mask on the ragged one), p exactly 0.  A bias of -inf: p exactly 0, a tile of them leaves m = -inf and the exponent is taken against 0.
    A row whose keys are ALL -inf has no softmax: out = NaN (0 * inf), lse = -inf; never sent by the provider, never asserted here (one key per row is kept).
    Padded query rows (i >= Sq of the last block) compute on a re-read of row Sq - 1 and are not stored.
  backward, a function of (q, k, v, out, lse, dout) -- it never looks at the forward's registers
    delta_i = sum_c dout_ic out_ic in fp32 over the bf16 `out` it is GIVEN (any order), published in delta_ws [B, H, Sq] (overwritten, not accumulated) by the dQ
    kernel and read by the dK / dV kernel, which runs after it.
    dQ kernels  attn_bwd_dq_kernel<., 2> (head_dim 128), attn_bwd_dq2_kernel<.>, attn_bwd_dq_res_kernel<.> (same bits as dq2):
                p_ij = exp2(fma(s_ij, sl, fp32(b2_j - lse_i))), dP_ij = dout_i . v_j, dS_ij = p_ij (dP_ij - delta_i), dQ = bf(scale * sum_j bf(dS_ij) k_j)
                attn_bwd_dq_pl_kernel<2, 1, .> (no bias, Sk >= 256): -delta_i enters as the accumulator input of the dP chain, dS = p (dP - delta) with the
                subtraction inside the matrix pipe: one rounding per score less / elsewhere; ragged Sk: zero-filled padded keys (exact DMA bounds), p clamped to
                [0, 1] by the exp2 instruction's clamp bit (a padded key's p = 1 meets k = 0; a real p changes only where it came out above 1)
    dK / dV     attn_bwd_dkdv_kernel<1, 2> / <2, 0 | 1>, attn_bwd_dkdv_sq_kernel<2>, attn_bwd_dkdv_pl_kernel<1>, attn_bwd_dkdv_pl128_kernel<1> (same bits):
                the score chain starts from fp32(-lse_i * (1 / sl)), the dP chain from -delta_i; p_ij = exp2(fma(s'_ij, sl, b2_j)), dS_ij = p_ij dP'_ij,
                dV = bf(sum_i bf(p_ij) dout_i), dK = bf(scale * sum_i bf(dS_ij) q_i)
    Padded keys: p = 0 through b2 = -inf (dq2 / dq / res) or k = v = 0 (pl); padded query rows: lse = +inf -> p = 0 (dkdv, sq) or q = dout = 0 rows (pl kernels).
    scale enters the scores through sl and multiplies dQ and dK once, in fp32, right before their rounding; the bias enters only the exp2 argument.
  second context (attn_ctx2.hip; the contract is the one of include/ftmi355.h: head_dim 128, 1 <= Sk <= 320, no bias)
    fwd  p_ij = bf(exp2(fp32(s_ij sl) - m)) with the exact running maximum, l summed over the bf16 p; out = bf(float(out_first) + float(bf(acc / l))), lse written
    dq   p_ij = exp2(fp32(s_ij sl) - lse_i) (0 for padded keys), delta_i = sum_j p_ij dP_ij in fp32 (NOT from a saved O), dS = p (dP - delta),
         dq = bf(float(dq_first) + float(bf(scale * sum_j bf(dS_ij) k_j))); dq_first may be dq itself.  B == 0 or Sq == 0: 0 without a launch.

REFERENCE: the table above in fp64 on the CPU over the same bf16 inputs.  The backward gets out = bf(O_fp64) and lse = fp32(lse_fp64) made HERE (a forward error
cannot hide a backward one); one chained case per head_dim feeds it the device's own out / lse instead.  The backward reference rounds p and dS to bf16 where the
kernels do.  The forward's p is NOT rounded in the reference: the kernel rounds exp2(x - m) for a lazily updated m the reference cannot know (m is no power of two,
so the rounding grid differs); every p carries the half-spacing 2^-8 p instead.

BOUNDS per element (u = 2^-24, ulp(a) = bf16 spacing at |a|, n-term fp32 sums in any order: (n + 2) u sum |term|), built from the inputs and the fp64 intermediates
only:  e_s = (d + 2) u |q| . |k|;  e_x = sl e_s + u |x| + u (rowmax - x + 8);  forward p: relative D = expm1(ln 2 e_x) + EXP2_REL + 2^-8;
  out   e = [sum_j P_j D_j (|v_j| + |O|)] / (1 - sum_j P_j D_j) + (Sk + 2 ntiles + 8) u (sum_j P_j |v_j| + |O|);  bound = e + ulp(|O| + e)
  lse   log2(e) [s / (1 - s)], s = sum_j P_j D_j + (Sk + 2 ntiles + 2) u;  + LOG2_REL max(1, log2 Sk + 9) + 2 u (|lse| + log2 Sk + 9)
  delta (d + 2) u sum_c |dout out|
  backward p: e_arg = (d + 6) u (|lse| + |b2| + sl |q| . |k|) + u |arg|;  e_p = p (expm1(ln 2 e_arg) + EXP2_REL) (+ max(0, p + e_p - 1) in the dQ bound where the clamped
  dQ stream runs, not in dK / dV);  e_dP = (d + 3) u (|dout| . |v| + |delta|);  e_dS = e_p |dP - delta| + (p + e_p)(e_dP + e_delta + u (|dP| + |delta|)) + u |dS|;  bf(v) known to e: e + ulp(|v| + e)
  dV    e = sum_i e_bf(p) |dout_i| + (Sq + 2) u sum_i (bf(p) + e) |dout_i|;  dK, dQ alike over bf(dS) with one more u for the scale;  bound = e + ulp(|.| + e)
  ctx2  fwd as the forward (exact maximum: no + 8), then bf(o_i) known to e_i: out bound = e_i + ulp(|o_i| + e_i) + ulp(|out| + that); dq alike with
        delta_i = sum_j p dP known to sum_j (e_p |dP| + p e_dP) + (Sk + 2) u sum |p dP|.
  EXP2_REL / LOG2_REL: the error of the exp2 / log2 instructions (v_exp_f32, v_log_f32) is not in the ISA notes at hand, so swept on the device through the kernels
  that use them (test_instruction_error_figures): exp2 through dV = bf(exp2(b2_j)) of a one-query launch (q = 0, lse = 0, dout = 1: every other operation exact)
  over 2^18 arguments b2 in [-29, 9], 241 280 of them AIMED at the bf16 rounding boundaries (the fp32 neighbours of log2 of every boundary of 29 binades: exp2(b2)
  a few u off a boundary, on either side); for every output that differs from bf(reference) (the fp64 value rounded ONCE to bf16) the distance of the fp64 value to the
  bf16 rounding boundary bounds the instruction's error from below (the elementwise contract's method).  This figure is a LOWER bound, as sharp as the
  sample's distances are dense near 0 (hence the aimed arguments; 2^18 uniform ones put 2 within 1 u of a boundary and showed no flip at all): no fp32 output of these kernels shows an exp2 result before a bf16 rounding (lse and delta are the only fp32 outputs; l sums bf16 numbers, and the
  rescale factor exp2(m_old - m_new) reaches lse only inside 1 + 64 alpha, alpha <= 2^-8, where fp32 resolves it to 2^-22).  An error of e at an argument flips
  its output only if the fp64 value lies within e of a boundary on the error's side; the test prints how many of the 2^18 arguments lie within 0.5 / 1 / 2 u of
  one (figures under MEASURED).  Against the 2^-8 p every bf(p) carries, EXP2_REL is about 2^-15 of the budget.  log2 through lse = log2(n) of a launch with q = 0 and n kept keys, n = 1 .. 4096 (fp32
  output, compared directly, relative to max(1, log2 n)).  Bounds use twice the largest figure seen, never less than 2 u.  The reciprocals are compiled IEEE
  divisions (1.0f / x, correctly rounded: u), there is no reciprocal instruction in these kernels.
  Asserted per case: every output finite; |got - ref| <= bound for EVERY element of out, lse, dQ, dK, dV and the published delta; every sentinel intact (output gaps,
  the element after lse and delta_ws); the second launch onto the same buffers bit-equal to the first.

INPUTS, two seeded regimes per case:  "randn": q, k ~ N(0, 1), v, dout ~ N(0, 1).  "edge": the edge keys E = {0, 63, 64, Sk - 1, first key of the last tile} each own
  eight head-dim slots holding a = sqrt(6 / (8 scale)); query row i carries a in the slot of E[i mod |E|]: that key sits 6 nat above the rest of row i; the boundary
  rows (Sq - 1, the first and last row of every 32-row wave tile, hence of every 128-row block) carry 8 x dout.  test_edge_constructor checks from the fp64
  reference alone (bias left out: a masked edge key has no weight to lose) that dropping any edge key moves some row's out by >= 8 bounds and dropping any
  boundary row moves some dV element by >= 8 bounds.

CASES (H B a multiple of 8 and not: the two block orders of attn_block; * = scale other than 1 / sqrt(d); bias: bk = [B, Sk] shared by the heads, bhk = per head,
+w = row stride Sk + 5 with a NaN gap, inf-tiles = whole leading / middle / ragged trailing tiles at -inf, inf-scatter = 30 % of the keys; one key per row kept)
  name      d   B  H   Sq   Sk  bias               forward        dQ                        dK / dV
  w64       64  2  4  128  128  -                  whole          dq2<false>                dkdv<1,2>
  r64       64  3  5  129   65  -                  ragged         dq2<false,true>           dkdv<1,2>
  r64b      64  1  1  127  129  - *                ragged         dq2<false,true>           dkdv<1,2>
  b64       64  2  4   33   63  bk                 biased         dq2<true>                 dkdv<1,2>
  b64inf    64  2  4   31  257  bhk+w inf-tiles    biased         dq2<true>                 dkdv<1,2>
  one64     64  2  3    1    1  bk+w               biased         dq2<true>                 dkdv<1,2>
  fewb      64  2  4  512  128  bhk inf-scatter    biased         dq_res<true>              dkdv_sq<2>
  feww      64  2 32  640   64  -                  whole          dq_res<false> (bpw 2)     dkdv_sq<2>
  fewr      64  1  1  513  127  - *                ragged         dq_res<true>              dkdv_sq<2>
  plw       64  2  4  257  256  -                  whole          dq_pl<2,1,whole>          dkdv_pl<1>
  plr       64  3  5  511  257  - *                ragged         dq_pl<2,1,ragged>         dkdv_pl<1>
  sq255     64  1  1  512  255  -                  ragged         dq2<false,true>           dkdv_sq<2> (Sk > 128)
  sq256     64  1  1  513  256  -                  whole          dq_pl<2,1,whole>          dkdv_sq<2> (Sk > 128)
  plbig     64  4 32  512  256  -                  whole          dq_pl<2,1,whole>          dkdv_pl<1> (Sq >= 512: 2 x 128 = 256 workgroups of 128 keys)
  w128     128  2  4  128  128  -                  whole          dq<false,2>               dkdv_pl128
  r128     128  3  5  129  257  - *                ragged         dq<true,2>                dkdv_pl128
  b128     128  2  4  257  129  bk inf-scatter     biased         dq<true,2>                dkdv_pl128
  s128     128  1  1   33   65  -                  ragged         dq<true,2>                dkdv<2,0> + dkdv<2,1>
  s128b    128  2  4  127   64  bhk+w inf-tiles    biased         dq<true,2>                dkdv<2,0> + dkdv<2,1>
  s128w    128  1  1  512   64  -                  whole          dq<false,2>               dkdv<2,0> + dkdv<2,1>
  one128   128  1  1    1    1  -                  ragged         dq<true,2>                dkdv<2,0> + dkdv<2,1>
  ctx2: (B, H, Sq, Sk) = (1,1,1,1) (2,4,48,63) (3,5,129,64) (1,1,48,65) (2,4,129,257) (3,5,1,320), dq out of place and in place; + the exact case below.
  Views: every one of q, k, v, out (forward output), out (backward input), dout, dq, dk, dv has a layout AND a stride triple of its own in the launch: the kinds
  [B, S+1, H d + pad], [B, H, S+1, d + pad], [B, H, S+2, d] with pad between heads and samples, slot 1 of [B, S+1, H, 2, d] rows + pad rotate over the tensors,
  and tensor number t of the launch has pad = 8 (t + 1), so no two triples coincide at any shape (asserted on the CPU for every case, and in build_buffers);
  q, k, v of w64 / w128 are the three slots of one [B, S+1, 3, H, d] buffer (one triple for the trio by construction, every other tensor apart);
  every stride a multiple of 8, every base 16-byte aligned; input gaps, the spare rows behind Sq / Sk and the bias gap hold NaN, output gaps OUT_SENT.

CPU SELF-CHECKS (unmarked): an fp32 / bf16 stand-in of each family (same rounding points, sums tile by tile, reading and writing the same strided buffers) passes
every bound; each seeded fault, applied to the stand-in, is rejected by at least one case; the case list reaches every branch of the restated dispatch rules.
  last_row_unstored  key_last_dropped  pad_keys_in_l  pad_rows_in_dkdv  hb_swap  bias_head0  bias_prev_sample  bias_gap  dk_with_dv_strides  dout_with_o_strides
  o_with_q_strides  dq_with_q_strides (each must be rejected by EVERY case listed for it, the B = 1 cases and one64, Sq = Sk = 1 with its batch and head
  strides, among them; one128 is one row of one head of one sample: no stride of it is ever multiplied by anything)
  no_scale_dq  no_scale_dk  delta_unrounded_o  lse_nat  delta_accumulated  ctx2_sum_before_round (seen on the exact case: q = 0, Sk a power of two, v and
  out_first multiples of 2^-3: every operation exact, the reference is bit-exact and the bound 0)  ctx2_tail_dropped

MEASURED on an MI355X (largest |got - ref| / bound over the cases and both regimes that reach the kernel; every element of every case is within its bound):
  forward      fwd64<whole>   out 0.492 lse 0.265   fwd64<ragged>   out 0.483 lse 0.618   fwd64<biased>   out 0.486 lse 0.712
               fwd128<whole>  out 0.482 lse 0.195   fwd128<ragged>  out 0.476 lse 0.277   fwd128<biased>  out 0.489 lse 0.809
  dQ (+ delta) dq2<false> 0.321 (0.014)   dq2<false,true> 0.480 (0.012)   dq2<true> 0.776 (0.011)   dq_res<false> 0.704 (0.019)   dq_res<true> 0.598 (0.013)
               dq_pl<2,1,whole> 0.879 (0.020)   dq_pl<2,1,ragged> 0.831 (0.018)   dq<false,2> 0.305 (0.006)   dq<true,2> 0.615 (0.007)
  dK / dV      dkdv<1,2> 0.370 / 0.480   dkdv_sq<2> 0.205 / 0.287   dkdv_pl<1> 0.352 / 0.270   dkdv_pl128<1> 0.382 / 0.322   dkdv<2,0>+dkdv<2,1> 0.396 / 0.301
  chained      r64: out 0.479 lse 0.572 dq 0.607 dk 0.398 dv 0.224 delta 0.012     r128: out 0.464 lse 0.277 dq 0.382 dk 0.399 dv 0.320 delta 0.006
  ctx2         out 0.934 lse 0.249 dq 0.847 (the exact cases: bit-equal)
  The edge regime's lse figures (0.5 - 0.8) are the lazy rescale at work: a row's dominant key holds p = exp2(x - m) for an m up to 8 below the row's maximum, so its
  bf16 rounding moves l by up to 2^-8; the stand-in, which keeps the exact maximum, rounds that p = 1 without error (0.03 - 0.18 on the same rows).
  Instructions: exp2: 2042 / 3719 / 6721 of the 262 144 arguments lie within 0.5 / 1 / 2 u of a rounding boundary (smallest distance 2.1e-11); 1226 outputs
  differ from bf(reference), the farthest of them 6.7910e-08 (1.139 u) from its boundary: EXP2_SEEN 6.7910e-08 -> EXP2_REL 1.3582e-07; log2: LOG2_SEEN 1.1759e-07
  (1.973 u of max(1, log2 n)) over n = 1 .. 4096 -> LOG2_REL 2.3518e-07.
  Run time of the whole file: the 32 device tests 9.4 s (5.0 s of it the fp64 reference of plbig), the 68 CPU self-checks 18 s.
fp32 stand-ins on the CPU over the same cases (test_fp32_stand_in_passes_every_bound, test_ctx2_stand_in_passes_every_bound): largest err / bound out 0.484, lse 0.258,
dq 0.879, dk 0.398, dv 0.322, delta 0.017; ctx2 out 0.934, lse 0.249, dq 0.975.
"""

import ctypes
import functools
import math
import time

import pytest
import torch

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0**-24
LN2 = math.log(2.0)
LOG2E32 = float(torch.tensor(1.4426950408889634, dtype=f32))  # kLog2e as the kernels hold it
EXP2_SEEN, LOG2_SEEN = 6.7910e-08, 1.1759e-07  # largest figures of test_instruction_error_figures on an MI355X (relative; log2: relative to max(1, |log2 n|))
EXP2_REL, LOG2_REL = 2.0 * max(EXP2_SEEN, U), 2.0 * max(LOG2_SEEN, U)
OUT_SENT = -1536.0   # padding of the bf16 outputs (exact in bf16): must survive the launch
F32_SENT = -7777.0   # behind lse and delta_ws
NAN = float("nan")
TENSORS = ("q", "k", "v", "out", "oin", "dout", "dq", "dk", "dv")


@pytest.fixture(autouse=True)
def _at_most_16_threads():
    """The fp64 references on at most 16 threads, for this file's tests only: the process-wide setting is put back after each of them."""
    before = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, before)))
    yield
    torch.set_num_threads(before)


def f32r(x):
    return float(torch.tensor(x, dtype=f32))


def bfr(t):
    return t.float().to(bf16).to(t.dtype)


def ulp_bf(a):
    _, e = torch.frexp(a)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - 8), torch.zeros_like(a))


def cdiv(a, b):
    return (a + b - 1) // b


# ----------------------------------------------------------------------------------------------------
# cases and the restated dispatch rules

class Case:
    def __init__(self, name, d, B, H, Sq, Sk, bias=None, inf=None, wide=False, scale_mul=1.0, fused=False):
        self.name, self.d, self.B, self.H, self.Sq, self.Sk = name, d, B, H, Sq, Sk
        self.bias, self.inf, self.wide, self.fused = bias, inf, wide, fused
        self.scale = f32r(scale_mul / math.sqrt(d))
        self.sl = float(torch.tensor(self.scale, dtype=f32) * torch.tensor(LOG2E32, dtype=f32))

    def __repr__(self):
        return self.name


CASES = [
    Case("w64", 64, 2, 4, 128, 128, fused=True),
    Case("r64", 64, 3, 5, 129, 65),
    Case("r64b", 64, 1, 1, 127, 129, scale_mul=1.7),
    Case("b64", 64, 2, 4, 33, 63, bias="bk"),
    Case("b64inf", 64, 2, 4, 31, 257, bias="bhk", inf="tiles", wide=True),
    Case("one64", 64, 2, 3, 1, 1, bias="bk", wide=True),
    Case("fewb", 64, 2, 4, 512, 128, bias="bhk", inf="scatter"),
    Case("feww", 64, 2, 32, 640, 64),
    Case("fewr", 64, 1, 1, 513, 127, scale_mul=0.6),
    Case("plw", 64, 2, 4, 257, 256),
    Case("plr", 64, 3, 5, 511, 257, scale_mul=1.3),
    Case("sq255", 64, 1, 1, 512, 255),
    Case("sq256", 64, 1, 1, 513, 256),
    Case("plbig", 64, 4, 32, 512, 256),
    Case("w128", 128, 2, 4, 128, 128, fused=True),
    Case("r128", 128, 3, 5, 129, 257, scale_mul=0.8),
    Case("b128", 128, 2, 4, 257, 129, bias="bk", inf="scatter"),
    Case("s128", 128, 1, 1, 33, 65),
    Case("s128b", 128, 2, 4, 127, 64, bias="bhk", inf="tiles", wide=True),
    Case("s128w", 128, 1, 1, 512, 64),
    Case("one128", 128, 1, 1, 1, 1),
]
BY_NAME = {c.name: c for c in CASES}
CTX2_CASES = [(1, 1, 1, 1), (2, 4, 48, 63), (3, 5, 129, 64), (1, 1, 48, 65), (2, 4, 129, 257), (3, 5, 1, 320)]
REGIMES = ("randn", "edge")


def dispatch(d, B, H, Sq, Sk, bias):
    """The kernel choice of attn_fwd / attn_bwd (csrc/attention.hip) with the shipped switches: (forward, dQ, dK / dV, extra tags)."""
    ragged = Sk % 64 != 0
    fwd = f"fwd{d}<" + ("biased" if bias else "ragged" if ragged else "whole") + ">"
    tags = {"xcd_order" if (H * B) % 8 == 0 else "plain_order"}
    if d == 128:
        dq = "dq<true,2>" if bias or ragged else "dq<false,2>"
        dkv = "dkdv_pl128<1>" if Sq >= 128 and Sk >= 128 else "dkdv<2,0>+dkdv<2,1>"
        return fwd, dq, dkv, tags
    nblk, bpw = cdiv(Sq, 128), 1
    while cdiv(nblk, bpw) * H * B > 256 and bpw <= 8:
        bpw += 1
    if Sk <= 128 and Sq >= 512 and bpw <= 8:
        dq = "dq_res<true>" if bias or ragged else "dq_res<false>"
        tags.add(f"res_bpw{min(bpw, 2)}")
    elif not bias and Sk >= 256:
        dq = "dq_pl<2,1,ragged>" if ragged else "dq_pl<2,1,whole>"
    elif bias:
        dq = "dq2<true>"
    elif ragged:
        dq = "dq2<false,true>"
    else:
        dq = "dq2<false>"
    wg128 = cdiv(Sk, 128) * H * B
    if wg128 < 256 and Sq >= 512:
        dkv = "dkdv_sq<2>"
        if Sk > 128:
            tags.add("sq_above_128_keys")
    elif not bias and Sq >= 128 and Sk >= 256:
        dkv = "dkdv_pl<1>"
        if Sq >= 512:
            tags.add("pl_dkdv_from_512_rows")
    else:
        dkv = "dkdv<1,2>"
    return fwd, dq, dkv, tags


ALL_BRANCHES = {
    "fwd64<biased>", "fwd64<ragged>", "fwd64<whole>", "fwd128<biased>", "fwd128<ragged>", "fwd128<whole>",
    "dq_res<true>", "dq_res<false>", "dq_pl<2,1,ragged>", "dq_pl<2,1,whole>", "dq2<true>", "dq2<false,true>", "dq2<false>", "dq<true,2>", "dq<false,2>",
    "dkdv_sq<2>", "dkdv_pl<1>", "dkdv<1,2>", "dkdv_pl128<1>", "dkdv<2,0>+dkdv<2,1>",
    "xcd_order", "plain_order", "res_bpw1", "res_bpw2", "sq_above_128_keys", "pl_dkdv_from_512_rows",
}


def test_case_list_reaches_every_dispatch_branch():
    seen, per_kernel_orders = set(), {}
    for c in CASES:
        fwd, dq, dkv, tags = dispatch(c.d, c.B, c.H, c.Sq, c.Sk, c.bias)
        seen |= {fwd, dq, dkv} | tags
        order = "xcd_order" if "xcd_order" in tags else "plain_order"
        for fam in (fwd[:6], "dq" + str(c.d), "dkv" + str(c.d)):
            per_kernel_orders.setdefault(fam, set()).add(order)
    assert seen == ALL_BRANCHES, (ALL_BRANCHES - seen, seen - ALL_BRANCHES)
    for fam, orders in per_kernel_orders.items():  # both block orders of attn_block per head_dim and pass
        assert orders == {"xcd_order", "plain_order"}, (fam, orders)
    assert {c.Sq for c in CASES} >= {1, 31, 33, 127, 128, 129, 257, 511, 512, 513}
    assert {c.Sk for c in CASES} >= {1, 63, 64, 65, 127, 128, 129, 255, 256, 257}
    assert {s[3] for s in CTX2_CASES} >= {1, 63, 64, 65, 257, 320} and {s[2] for s in CTX2_CASES} >= {1, 48, 129}
    assert dispatch(64, 2, 32, 640, 64, None)[3] >= {"res_bpw2"}


def test_every_tensor_of_a_launch_has_strides_of_its_own():
    """build_buffers asserts it for the data it is given; here for every case without any data (layouts depend on the shape and the case number only)."""
    for n, c in enumerate(CASES):
        bufs = build_buffers(c, n, {})
        assert distinct_strides(c, bufs), c.name
        for name in TENSORS:
            assert bufs[name].off % 8 == 0 and all(x % 8 == 0 for x in bufs[name].st), (c.name, name)


# ----------------------------------------------------------------------------------------------------
# inputs

def seed_of(name, regime):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name + regime))


def edge_keys(Sk):
    return sorted({0, 63, 64, Sk - 1, (cdiv(Sk, 64) - 1) * 64} & set(range(Sk)))


def boundary_rows(Sq):
    return sorted({i for i in range(Sq) if i % 32 in (0, 31)} | {Sq - 1})


def make_qkvdo(d, B, H, Sq, Sk, scale, regime, seed):
    g = torch.Generator()
    g.manual_seed(seed)
    q = torch.randn(B, H, Sq, d, generator=g)
    k = torch.randn(B, H, Sk, d, generator=g)
    v = torch.randn(B, H, Sk, d, generator=g)
    do = torch.randn(B, H, Sq, d, generator=g)
    if regime == "edge":
        E = edge_keys(Sk)
        a = math.sqrt(6.0 / (8.0 * scale))
        ns = 8 * len(E)
        q[..., :ns] = 0.0
        k[..., :ns] = 0.0
        q[..., ns:] *= 0.5
        k[..., ns:] *= 0.5
        for e, j in enumerate(E):
            k[:, :, j, 8 * e:8 * e + 8] = a
            q[:, :, e::len(E), 8 * e:8 * e + 8] = a
        do[:, :, boundary_rows(Sq)] *= 8.0
    return q.to(bf16), k.to(bf16), v.to(bf16), do.to(bf16)


def make_bias(c, seed):
    """fp32 key bias in natural units as a padded flat buffer: (flat, strides (sb, sh), logical [B, H, Sk])."""
    if c.bias is None:
        return None
    g = torch.Generator()
    g.manual_seed(seed + 17)
    B, H, Sk = c.B, c.H, c.Sk
    heads = H if c.bias == "bhk" else 1
    kb = torch.randn(B, heads, Sk, generator=g)
    if c.inf == "tiles":
        nt = cdiv(Sk, 64)
        for b in range(B):
            for h in range(heads):
                for t in {0, nt // 2, nt - 1} - {(b + h) % nt}:  # leading, middle and (ragged) trailing tiles; one of them is kept per row when they are all there are
                    kb[b, h, t * 64:(t + 1) * 64] = -math.inf
                kb[b, h, (7 * b + 3 * h) % Sk::11] = -math.inf
                if torch.isinf(kb[b, h]).all():
                    kb[b, h, (b + h) % Sk] = 0.25
    elif c.inf == "scatter":
        kb[torch.rand(B, heads, Sk, generator=g) < 0.3] = -math.inf
        for b in range(B):
            for h in range(heads):
                kb[b, h, (5 * b + h) % Sk] = 0.5
    row = Sk + 5 if c.wide else Sk
    flat = torch.full((B * heads * row + 8,), NAN, dtype=f32)
    flat[:B * heads * row].view(B, heads, row)[:, :, :Sk] = kb
    return flat, (heads * row, row if c.bias == "bhk" else 0), kb.expand(B, H, Sk)


# ----------------------------------------------------------------------------------------------------
# strided buffers

KINDS = ("bshd", "bhsd8", "bhsd", "bsh2d")


def layout(kind, B, H, S, d, t=0):
    """(offset, (batch, head, token strides), elements) of a [B, H, S, d] view; every figure a multiple of 8.  t = the tensor's place in the launch: its
    pad of 8 (t + 1) elements makes the stride triple its own whatever S is (two tensors of one kind, Sq = Sk = 1 included)."""
    pad = 8 * (t + 1)
    if kind == "bshd":  # [B, S + 1, H d + pad]
        ss = H * d + pad
        return 64, ((S + 1) * ss, d, ss), 64 + B * (S + 1) * ss + 8
    if kind == "bhsd8":  # [B, H, S + 1, d + pad] (+ pad between samples)
        ss = d + pad
        sh = (S + 1) * ss
        return 8, (H * sh + pad, sh, ss), 8 + B * (H * sh + pad) + 8
    if kind == "bhsd":  # [B, H, S + 2, d] with pad elements between heads and twice that between samples
        sh = (S + 2) * d + pad
        return 0, (H * sh + 2 * pad, sh, d), B * (H * sh + 2 * pad) + 8
    if kind == "bsh2d":  # slot 1 of [B, S + 1, H, 2, d] rows, pad elements behind each row
        ss = H * 2 * d + pad
        return d, ((S + 1) * ss, 2 * d, ss), B * (S + 1) * ss + 8
    raise KeyError(kind)


def view_index(off, st, shape):
    B, H, S, d = shape
    return (off + torch.arange(B)[:, None, None, None] * st[0] + torch.arange(H)[None, :, None, None] * st[1] + torch.arange(S)[None, None, :, None] * st[2]
            + torch.arange(d)[None, None, None, :])


class Buf:
    """A flat buffer and the [B, H, S, d] view a launch is given into it."""

    def __init__(self, flat, off, st, shape):
        self.flat, self.off, self.st, self.shape = flat, off, st, shape

    def idx(self, st=None):
        return view_index(self.off, st or self.st, self.shape) % self.flat.numel()

    def get(self, st=None):
        return self.flat[self.idx(st)]

    def put(self, val, st=None):
        self.flat[self.idx(st)] = val.to(self.flat.dtype)

    def clone(self):
        return Buf(self.flat.clone(), self.off, self.st, self.shape)


def distinct_strides(c, bufs):
    """Every tensor of the two launches has a (batch, head, token) stride triple no other has.  The fused cases hold q, k, v as the three slots of ONE buffer
    (same strides by construction, offsets apart): there k and v are left out of the comparison, q stands for the trio."""
    names = [nm for nm in TENSORS if not (c.fused and nm in ("k", "v"))]
    triples = [tuple(bufs[nm].st) for nm in names]
    return len(set(triples)) == len(triples)


def build_buffers(c, n, data):
    """Every tensor of forward + backward in a layout of its own (rotating with the case number n); inputs in NaN, outputs in OUT_SENT."""
    B, H, Sq, Sk, d = c.B, c.H, c.Sq, c.Sk, c.d
    bufs = {}
    if c.fused:  # q, k, v: the three slots of one [B, S + 1, 3, H, d] buffer
        assert Sq == Sk
        flat = torch.full((B * (Sq + 1) * 3 * H * d + 8,), NAN, dtype=bf16)
        for i, name in enumerate(("q", "k", "v")):
            bufs[name] = Buf(flat, i * H * d, ((Sq + 1) * 3 * H * d, d, 3 * H * d), (B, H, Sq, d))
    for t, name in enumerate(TENSORS):
        S = Sk if name in ("k", "v", "dk", "dv") else Sq
        if name not in bufs:
            off, st, numel = layout(KINDS[(n + t) % 4], B, H, S, d, t)
            assert off + (B - 1) * st[0] + (H - 1) * st[1] + (S - 1) * st[2] + d <= numel and off % 8 == 0 and all(x % 8 == 0 for x in st)
            is_in = name in ("q", "k", "v", "oin", "dout")
            bufs[name] = Buf(torch.full((numel,), NAN if is_in else OUT_SENT, dtype=bf16), off, st, (B, H, S, d))
        if name in data:
            bufs[name].put(data[name])
    assert distinct_strides(c, bufs), (c.name, {name: bufs[name].st for name in TENSORS})
    rows = B * H * Sq
    for name in ("lse", "lse_in", "delta"):
        bufs[name] = torch.full((rows + 16,), F32_SENT, dtype=f32)
    if "lse_in" in data:
        bufs["lse_in"][:rows] = data["lse_in"].flatten()
    bufs["bias"] = data.get("bias")
    return bufs


# ----------------------------------------------------------------------------------------------------
# the reference and its bounds (fp64, one batch sample at a time)

def _bias2(kb):
    """[.., Sk] fp32 natural-unit bias -> the log2-domain fp32 number the kernels add, as fp64."""
    return (kb.float() * torch.tensor(LOG2E32, dtype=f32)).double()


def ref_forward(c, q, k, v, kb, exact_max=False, keep=False):
    """out (unrounded fp64), its error bound before the output rounding, lse, its bound; per sample to bound the memory."""
    B, H, Sq, Sk, d = c.B, c.H, c.Sq, c.Sk, c.d
    nt = cdiv(Sk, 64)
    O, eO, L, eL, keepers = [], [], [], [], []
    for b in range(B):
        qd, kd, vd = q[b].double(), k[b].double(), v[b].double()
        S = qd @ kd.transpose(-1, -2)
        eS = (d + 2) * U * (qd.abs() @ kd.abs().transpose(-1, -2))
        x = S * c.sl
        if kb is not None:
            x = x + _bias2(kb[b])[:, None, :]
        live = torch.isfinite(x)
        xmax = x.max(-1, keepdim=True).values
        lse = xmax + torch.log2(torch.exp2(x - xmax).sum(-1, keepdim=True))
        P = torch.exp2(x - lse)
        xa = torch.where(live, x, torch.zeros_like(x))
        ex = c.sl * eS + U * xa.abs() + U * (xmax - xa + (0.0 if exact_max else 8.0))
        D = torch.where(live, torch.expm1(LN2 * ex) + EXP2_REL + 2.0**-8, torch.zeros_like(x))
        PD = P * D
        s = PD.sum(-1, keepdim=True)
        assert float(s.max()) < 0.25
        o = P @ vd
        nsum = (Sk + 2 * nt + 8) * U
        e = (PD @ vd.abs() + s * o.abs()) / (1.0 - s) + nsum * (P @ vd.abs() + o.abs())
        s2 = s + (Sk + 2 * nt + 2) * U
        span = math.log2(Sk) + 9.0
        el = (s2 / (1.0 - s2)) / LN2 + LOG2_REL * max(1.0, span) + 2 * U * (lse.abs() + span)
        O.append(o), eO.append(e), L.append(lse.squeeze(-1)), eL.append(el.squeeze(-1))
        if keep:
            keepers.append((P, D))
    out = (torch.stack(O), torch.stack(eO), torch.stack(L), torch.stack(eL))
    return out + (keepers,) if keep else out


def rounded(v, e):
    """bf(v) for v known to e: (bf(v), e + ulp(|v| + e))."""
    return bfr(v), e + ulp_bf(v.abs() + e)


def ref_backward(c, q, k, v, kb, oin, lse_in, do, clamp_p=False, keep=False):
    """dq, dk, dv, delta with their bounds from (q, k, v, out, lse, dout): {name: (reference, bound)}."""
    B, H, Sq, Sk, d = c.B, c.H, c.Sq, c.Sk, c.d
    res = {n: ([], []) for n in ("dq", "dk", "dv", "delta")}
    keepers = []
    for b in range(B):
        qd, kd, vd, od, dod = q[b].double(), k[b].double(), v[b].double(), oin[b].double(), do[b].double()
        lse = lse_in[b].double()[..., None]
        delta = (dod * od).sum(-1, keepdim=True)
        e_delta = (d + 2) * U * (dod * od).abs().sum(-1, keepdim=True)
        S = qd @ kd.transpose(-1, -2)
        A = qd.abs() @ kd.abs().transpose(-1, -2)
        b2 = _bias2(kb[b]) if kb is not None else torch.zeros(H, 1, Sk, dtype=f64)
        if b2.dim() == 2:
            b2 = b2[:, None, :]
        live = torch.isfinite(b2).expand(H, Sq, Sk)
        b2a = torch.where(torch.isfinite(b2), b2, torch.zeros_like(b2))
        arg = S * c.sl + b2 - lse
        arga = torch.where(live, arg, torch.zeros_like(arg))
        e_arg = (d + 6) * U * (lse.abs() + b2a.abs() + c.sl * A) + U * arga.abs()
        p = torch.exp2(arg)
        e_p = torch.where(live, p * (torch.expm1(LN2 * e_arg) + EXP2_REL), torch.zeros_like(p))
        dP = dod @ vd.transpose(-1, -2)
        e_dP = (d + 3) * U * (dod.abs() @ vd.abs().transpose(-1, -2) + delta.abs())
        dS = p * (dP - delta)
        e_dS = e_p * (dP - delta).abs() + (p + e_p) * (e_dP + e_delta + U * (dP.abs() + delta.abs())) + U * dS.abs()
        pb, e_pb = rounded(p, e_p)
        dSb, e_dSb = rounded(dS, e_dS)
        e_dSq = e_dSb
        if clamp_p:  # the clamped exp2 of the ragged pipelined dQ stream only: dK / dV come from another kernel
            e_pq = e_p + (p + e_p - 1.0).clamp_min(0.0)
            e_dSq = rounded(dS, e_pq * (dP - delta).abs() + (p + e_pq) * (e_dP + e_delta + U * (dP.abs() + delta.abs())) + U * dS.abs())[1]
        dv = pb.transpose(-1, -2) @ dod
        e_dv = e_pb.transpose(-1, -2) @ dod.abs() + (Sq + 2) * U * ((pb + e_pb).transpose(-1, -2) @ dod.abs())
        dk = c.scale * (dSb.transpose(-1, -2) @ qd)
        e_dk = c.scale * (e_dSb.transpose(-1, -2) @ qd.abs() + (Sq + 3) * U * ((dSb.abs() + e_dSb).transpose(-1, -2) @ qd.abs()))
        dq = c.scale * (dSb @ kd)
        e_dq = c.scale * (e_dSq @ kd.abs() + (Sk + 3) * U * ((dSb.abs() + e_dSq) @ kd.abs()))
        for n, val, err in (("dq", dq, e_dq), ("dk", dk, e_dk), ("dv", dv, e_dv)):
            r, e = rounded(val, err)
            res[n][0].append(r), res[n][1].append(e)
        res["delta"][0].append(delta.squeeze(-1)), res["delta"][1].append(e_delta.squeeze(-1))
        if keep:
            keepers.append((pb, dod))
    out = {n: (torch.stack(a), torch.stack(e)) for n, (a, e) in res.items()}
    if keep:
        out["keep"] = keepers
    return out


@functools.lru_cache(maxsize=None)
def prepared(name, regime):
    """Inputs, the fp64 reference and the bounds of one case, computed once and left unchanged."""
    c = BY_NAME[name]
    seed = seed_of(name, regime)
    q, k, v, do = make_qkvdo(c.d, c.B, c.H, c.Sq, c.Sk, c.scale, regime, seed)
    bias = make_bias(c, seed)
    kb = bias[2] if bias is not None else None
    o64, e_o, lse64, e_lse = ref_forward(c, q, k, v, kb)
    data = {"q": q, "k": k, "v": v, "dout": do, "oin": o64.to(bf16), "lse_in": lse64.float(), "bias": bias}
    ref = {"out": rounded(o64, e_o), "lse": (lse64, e_lse)}
    clamp = dispatch(c.d, c.B, c.H, c.Sq, c.Sk, c.bias)[1] == "dq_pl<2,1,ragged>"
    ref.update(ref_backward(c, q, k, v, kb, data["oin"], data["lse_in"], do, clamp_p=clamp))
    return c, data, ref


# ----------------------------------------------------------------------------------------------------
# the fp32 / bf16 stand-in of the kernels (reads and writes the strided buffers; `fault` seeds one defect)

def _f32_fma(a, b, cc):
    return (a.double() * b + cc.double()).float()


def _pad_keys(t, Skp, dup):
    Sk = t.shape[-2]
    if Skp == Sk:
        return t
    tail = t[..., Sk - 1:Sk, :].expand(*t.shape[:-2], Skp - Sk, t.shape[-1]) if dup else torch.zeros(*t.shape[:-2], Skp - Sk, t.shape[-1])
    return torch.cat([t, tail], -2)


def _standin_bias2(c, bufs, fault, Skp):
    """[B, H, Skp] log2-domain bias as the kernels see it: -inf behind Sk (fault bias_gap: whatever the buffer holds there), 0 without a bias."""
    B, H, Sk = c.B, c.H, c.Sk
    if bufs["bias"] is None:
        b2 = torch.zeros(B, H, Skp)
    else:
        flat, (sb, sh), _ = bufs["bias"]
        bi, hi = torch.arange(B)[:, None, None], torch.arange(H)[None, :, None]
        if fault == "bias_head0":
            hi = hi * 0
        if fault == "bias_prev_sample":
            bi = (bi - 1).clamp_min(0)
        idx = (bi * sb + hi * sh + torch.arange(Skp)[None, None, :]) % flat.numel()
        b2 = flat[idx] * torch.tensor(LOG2E32, dtype=f32)
    if fault != "bias_gap":
        b2[..., Sk:] = -math.inf
    if fault == "pad_keys_in_l":
        b2[..., Sk:] = 0.0
    if fault == "key_last_dropped" and Sk > 1:
        b2[..., Sk - 1] = -math.inf
    return b2


def _hb_swap(c, t):
    """Results of (batch, head) pair hb land where the swapped decode (h = hb // B, b = hb % B) points."""
    B, H = c.B, c.H
    flat = t.reshape(B * H, *t.shape[2:])
    out = torch.empty_like(flat)
    hb = torch.arange(B * H)
    out[(hb % B) * H + hb // B] = flat
    return out.reshape(t.shape)


def standin_forward(c, bufs, fault=None):
    B, H, Sq, Sk, d = c.B, c.H, c.Sq, c.Sk, c.d
    nt = cdiv(Sk, 64)
    Skp = nt * 64
    q, k, v = bufs["q"].get().float(), bufs["k"].get().float(), bufs["v"].get().float()
    dup = fault == "bias_gap"
    k, v = _pad_keys(k, Skp, dup), _pad_keys(v, Skp, dup)
    b2 = _standin_bias2(c, bufs, fault, Skp)
    m = torch.full((B, H, Sq), -math.inf)
    l = torch.zeros(B, H, Sq)
    acc = torch.zeros(B, H, Sq, d)
    for t in range(nt):
        ks, vs = k[:, :, t * 64:(t + 1) * 64], v[:, :, t * 64:(t + 1) * 64]
        x = _f32_fma(q @ ks.transpose(-1, -2), c.sl, b2[:, :, None, t * 64:(t + 1) * 64])
        m_new = torch.maximum(m, x.max(-1).values)
        m_eff = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m - m_eff)
        pb = bfr(torch.exp2(x - m_eff[..., None]))
        l = l * alpha + pb.sum(-1)
        acc = acc * alpha[..., None] + pb @ vs
        m = m_new
    out = bfr(acc * (1.0 / l)[..., None])
    lse = m + torch.log2(l)
    if fault == "lse_nat":
        lse = lse * LN2
    if fault == "hb_swap" and (B * H) % 8 == 0:
        out, lse = _hb_swap(c, out), _hb_swap(c, lse)
    rows = Sq - 1 if fault == "last_row_unstored" and Sq % 32 else Sq
    idx = bufs["out"].idx()[:, :, :rows]
    bufs["out"].flat[idx] = out[:, :, :rows].to(bf16)
    bufs["lse"][:B * H * Sq].view(B, H, Sq)[:, :, :rows] = lse[:, :, :rows]


def standin_backward(c, bufs, fault=None):
    B, H, Sq, Sk, d = c.B, c.H, c.Sq, c.Sk, c.d
    nt, ni = cdiv(Sk, 64), cdiv(Sq, 64)
    Skp = nt * 64
    q, k0, v0 = bufs["q"].get().float(), bufs["k"].get().float(), bufs["v"].get().float()
    do = bufs["dout"].get(bufs["oin"].st if fault == "dout_with_o_strides" else None).float()
    o = bufs["oin"].get(bufs["q"].st if fault == "o_with_q_strides" else None).float()
    lse = bufs["lse_in"][:B * H * Sq].view(B, H, Sq).clone()
    if fault == "lse_nat":
        lse = lse * LOG2E32
    b2 = _standin_bias2(c, bufs, fault if fault in ("bias_head0", "bias_prev_sample", "bias_gap", "key_last_dropped") else None, Skp)
    if fault == "delta_unrounded_o":  # the stand-in's own fp32 softmax(q k^T) v in place of the bf16 `out` it was given
        x = _f32_fma(q @ k0.transpose(-1, -2), c.sl, b2[:, :, None, :Sk])
        o = torch.softmax(x * LN2, -1) @ v0
    delta = torch.zeros(B, H, Sq)
    for c0 in reversed(range(0, d, 16)):
        delta = delta + (do[..., c0:c0 + 16] * o[..., c0:c0 + 16]).sum(-1)
    dws = bufs["delta"][:B * H * Sq].view(B, H, Sq)
    delta = dws + delta if fault == "delta_accumulated" else delta
    # dQ: a lane owns a query row, tiles of 64 keys
    dup = fault == "bias_gap"
    k, v = _pad_keys(k0, Skp, dup), _pad_keys(v0, Skp, dup)
    acc = torch.zeros(B, H, Sq, d)
    for t in range(nt):
        ks, vs = k[:, :, t * 64:(t + 1) * 64], v[:, :, t * 64:(t + 1) * 64]
        arg = _f32_fma(q @ ks.transpose(-1, -2), c.sl, b2[:, :, None, t * 64:(t + 1) * 64] - lse[..., None])
        p = torch.exp2(arg)
        dS = p * (do @ vs.transpose(-1, -2) - delta[..., None])
        acc = acc + bfr(dS) @ ks
    dq = bfr(acc * (1.0 if fault == "no_scale_dq" else c.scale))
    # dK / dV: a lane owns a key, tiles of 64 query rows; the chains start from -lse / sl and -delta
    inv_sl = torch.tensor(1.0, dtype=f32) / torch.tensor(c.sl, dtype=f32)
    s0 = -lse * inv_sl
    Sqp = ni * 64
    extra = Sqp - Sq if fault == "pad_rows_in_dkdv" else 0  # padded query rows (re-reads of row Sq - 1) counted
    dk, dv = torch.zeros(B, H, Sk, d), torch.zeros(B, H, Sk, d)
    for t in range(ni):
        sl_ = slice(t * 64, min((t + 1) * 64, Sq))
        qs, dos = q[:, :, sl_], do[:, :, sl_]
        s = s0[:, :, sl_, None] + qs @ k0.transpose(-1, -2)
        p = torch.exp2(_f32_fma(s, c.sl, b2[:, :, None, :Sk]))
        dS = p * (-delta[:, :, sl_, None] + dos @ v0.transpose(-1, -2))
        pb, dSb = bfr(p), bfr(dS)
        if extra and t == ni - 1:
            w = torch.ones(qs.shape[2])
            w[-1] += extra
            pb, dSb = pb * w[:, None], dSb * w[:, None]
        dv = dv + pb.transpose(-1, -2) @ dos
        dk = dk + dSb.transpose(-1, -2) @ qs
    dk = bfr(dk * (1.0 if fault == "no_scale_dk" else c.scale))
    dv = bfr(dv)
    if fault == "hb_swap" and (B * H) % 8 == 0:
        dq, dk, dv, delta = _hb_swap(c, dq), _hb_swap(c, dk), _hb_swap(c, dv), _hb_swap(c, delta)
    rows = Sq - 1 if fault == "last_row_unstored" and Sq % 32 else Sq
    bufs["dq"].flat[bufs["dq"].idx(bufs["q"].st if fault == "dq_with_q_strides" else None)[:, :, :rows]] = dq[:, :, :rows].to(bf16)
    dws[:, :, :rows] = delta[:, :, :rows]
    bufs["dk"].put(dk, bufs["dv"].st if fault == "dk_with_dv_strides" else None)
    bufs["dv"].put(dv)


def run_standin(c, bufs, fault=None):
    standin_forward(c, bufs, fault)
    standin_backward(c, bufs, fault)


# ----------------------------------------------------------------------------------------------------
# the device

def _dev():
    return torch.device("cuda", 0)


def _desc(c, bufs, out_name):
    from finetrainers_amd import _lib

    t = _lib.AttnDesc()
    t.B, t.H, t.Sq, t.Sk, t.d, t.scale = c.B, c.H, c.Sq, c.Sk, c.d, c.scale
    for field, name in (("q_strides", "q"), ("k_strides", "k"), ("v_strides", "v"), ("o_strides", out_name), ("do_strides", "dout"), ("dq_strides", "dq"),
                        ("dk_strides", "dk"), ("dv_strides", "dv")):
        a = getattr(t, field)
        a[0], a[1], a[2] = bufs[name].st
    if bufs["bias"] is not None:
        t.bias_strides[0], t.bias_strides[1] = bufs["bias"][1]
    return t


class DeviceBufs:
    """The buffers of a case on the device; q, k, v of a fused case stay one allocation."""

    def __init__(self, bufs):
        self.host, self.dev, seen = bufs, {}, {}
        for name in TENSORS:
            flat = bufs[name].flat
            if id(flat) not in seen:
                seen[id(flat)] = flat.to(_dev())
            self.dev[name] = seen[id(flat)]
        for name in ("lse", "lse_in", "delta"):
            self.dev[name] = bufs[name].to(_dev())
        self.dev["bias"] = bufs["bias"][0].to(_dev()) if bufs["bias"] is not None else None

    def ptr(self, name):
        if name in TENSORS:
            p = self.dev[name].data_ptr() + 2 * self.host[name].off
            assert p % 16 == 0
            return p
        return self.dev[name].data_ptr() if self.dev[name] is not None else None

    def fetch(self):
        for name in ("out", "dq", "dk", "dv"):
            self.host[name].flat.copy_(self.dev[name].cpu())
        for name in ("lse", "delta"):
            self.host[name].copy_(self.dev[name].cpu())


def run_device(c, bufs, chained=False):
    from finetrainers_amd import _lib

    lib = _lib.load()
    db = DeviceBufs(bufs)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.ftmi_attn_fwd(ctypes.byref(_desc(c, bufs, "out")), db.ptr("q"), db.ptr("k"), db.ptr("v"), db.ptr("out"), db.ptr("lse"), db.ptr("bias"), st),
               "ftmi_attn_fwd")
    o_name, lse_name = ("out", "lse") if chained else ("oin", "lse_in")
    _lib.check(lib.ftmi_attn_bwd(ctypes.byref(_desc(c, bufs, o_name)), db.ptr("q"), db.ptr("k"), db.ptr("v"), db.ptr(o_name), db.ptr(lse_name), db.ptr("dout"),
                                 db.ptr("dq"), db.ptr("dk"), db.ptr("dv"), db.ptr("delta"), db.ptr("bias"), st), "ftmi_attn_bwd")
    torch.cuda.synchronize()
    db.fetch()


# ----------------------------------------------------------------------------------------------------
# the comparison

def outside_intact(buf, sentinel):
    mask = torch.ones(buf.flat.numel(), dtype=torch.bool)
    mask[buf.idx().flatten()] = False
    return bool((buf.flat[mask].float() == sentinel).all())


def compare(c, bufs, ref, names=("out", "lse", "dq", "dk", "dv", "delta")):
    """Largest |got - ref| / bound per output over EVERY element; raises on a non-finite value, an element outside its bound or a damaged sentinel."""
    rows = c.B * c.H * c.Sq
    worst = {}
    for name in names:
        want, bound = ref[name]
        if name in ("lse", "delta"):
            got = bufs[name][:rows].view(c.B, c.H, c.Sq).double()
            assert bool((bufs[name][rows:] == F32_SENT).all()), f"{c.name}: the sentinel behind {name} is damaged"
        else:
            got = bufs[name].get().double()
            assert outside_intact(bufs[name], OUT_SENT), f"{c.name}: {name} wrote outside its view"
        assert got.shape == want.shape and got.numel() == want.numel()
        assert bool(torch.isfinite(got).all()), f"{c.name}: {name} holds a non-finite value"
        err = (got - want).abs()
        bad = err > bound
        if bool(bad.any()):
            at = [int(i) for i in torch.nonzero(bad)[0]]
            ratio = float((err / bound.clamp_min(1e-300))[bad].max())
            raise AssertionError(f"{c.name}: {name}{at} is {float(got[tuple(at)]):.6g}, reference {float(want[tuple(at)]):.6g}, bound {float(bound[tuple(at)]):.3g}; "
                                 f"{int(bad.sum())} elements out of bound, worst err / bound {ratio:.3g}")
        worst[name] = float((err / bound.clamp_min(1e-300)).max())
    return worst


_PREV_DELTA = [torch.full((64,), 3.25, dtype=f32)]  # the workspace as the case before left it


def run_case(c, n, regime, backend, fault=None, chained=False):
    """Two launches onto the same buffers (delta_ws used), bit-equal, every element inside its bound."""
    _, data, ref = prepared(c.name, regime)
    bufs = build_buffers(c, n, data)
    rows = c.B * c.H * c.Sq
    prev = _PREV_DELTA[0]
    bufs["delta"][:rows] = prev.repeat(cdiv(rows, prev.numel()))[:rows]
    backend(c, bufs) if fault is None else backend(c, bufs, fault)
    first = {name: (bufs[name].flat.clone() if name in TENSORS else bufs[name].clone()) for name in ("out", "dq", "dk", "dv", "lse", "delta")}
    backend(c, bufs) if fault is None else backend(c, bufs, fault)
    for name, t in first.items():
        now = bufs[name].flat if name in TENSORS else bufs[name]
        assert torch.equal(now.view(torch.int16 if name in TENSORS else torch.int32), t.view(torch.int16 if name in TENSORS else torch.int32)), \
            f"{c.name}: {name} differs between two launches onto the same buffers"
    if fault is None:
        _PREV_DELTA[0] = bufs["delta"][:rows].clone()
    if chained:  # the backward ran on the device's own out / lse: its reference is a function of those
        o_dev, lse_dev = bufs["out"].get(), bufs["lse"][:rows].view(c.B, c.H, c.Sq)
        kb = data["bias"][2] if data["bias"] is not None else None
        clamp = dispatch(c.d, c.B, c.H, c.Sq, c.Sk, c.bias)[1] == "dq_pl<2,1,ragged>"
        ref = dict(ref)
        ref.update(ref_backward(c, data["q"], data["k"], data["v"], kb, o_dev, lse_dev, data["dout"], clamp_p=clamp))
    return compare(c, bufs, ref)


# ----------------------------------------------------------------------------------------------------
# CPU self-checks

SMALL = ("w64", "r64", "r64b", "b64", "b64inf", "one64", "w128", "s128", "s128b", "one128", "plw", "fewr")


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_fp32_stand_in_passes_every_bound(name):
    c = BY_NAME[name]
    n = CASES.index(c)
    for regime in REGIMES:
        worst = run_case(c, n, regime, run_standin)
        print(f"[attention stand-in] {name:7s} {regime:5s} " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


FAULTS = {
    "last_row_unstored": ("r64", "b64", "s128"),
    "key_last_dropped": ("r64", "w64", "s128"),
    "pad_keys_in_l": ("r64", "s128"),
    "pad_rows_in_dkdv": ("r64", "b64", "s128"),
    "hb_swap": ("w64", "b64", "w128"),
    "bias_head0": ("b64inf", "s128b"),
    "bias_prev_sample": ("b64", "s128b"),
    "bias_gap": ("b64", "b64inf", "b128"),
    "dk_with_dv_strides": ("w64", "r64", "s128"),
    "dout_with_o_strides": ("w64", "r64", "s128"),
    "o_with_q_strides": ("b64", "one64", "fewr", "plw", "s128", "s128w"),
    "dq_with_q_strides": ("b64", "one64", "fewr", "plw", "s128", "s128w"),
    "no_scale_dq": ("w64", "s128"),
    "no_scale_dk": ("w64", "s128"),
    "delta_unrounded_o": ("w64", "r64", "w128"),
    "lse_nat": ("w64", "s128"),
    "delta_accumulated": ("w64", "s128"),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_seeded_fault_is_rejected(fault):
    """At head_dim 64 and 128 where the fault exists at both: the first listed case of each must reject it."""
    rejected = []
    for name in FAULTS[fault]:
        c = BY_NAME[name]
        for regime in REGIMES:
            try:
                run_case(c, CASES.index(c), regime, run_standin, fault=fault)
            except AssertionError as e:
                rejected.append((name, regime, str(e)[:110]))
    print(f"[attention fault] {fault}: rejected by {len(rejected)} of {2 * len(FAULTS[fault])} runs; first: {rejected[:1]}")
    assert rejected, f"{fault}: no case notices it"
    if fault.endswith("_with_q_strides"):  # a pair of tensors sharing a stride triple in ANY of these cases would let it through there
        assert {r[:2] for r in rejected} == {(nm, rg) for nm in FAULTS[fault] for rg in REGIMES}, rejected
    heads = {BY_NAME[r[0]].d for r in rejected}
    assert heads == {BY_NAME[nm].d for nm in FAULTS[fault]}, f"{fault}: only noticed at head_dim {heads}"


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_edge_constructor(name):
    """From the fp64 reference alone: every edge key carries, for some row, enough weight that dropping it moves an element of that row's out by >= 8 bounds, and
    every boundary row moves some element of dV by >= 8 bounds when dropped.  (plbig: its own inputs, checked on sample 0, heads 0 and 1 -- the edge keys and boundary rows are the
    same for every sample and head, only the random part differs.)"""
    c = BY_NAME[name]
    q, k, v, do = make_qkvdo(c.d, c.B, c.H, c.Sq, c.Sk, c.scale, "edge", seed_of(name, "edge"))
    if name == "plbig":
        q, k, v, do = (t[:1, :2] for t in (q, k, v, do))
        c = Case(name, c.d, 1, 2, c.Sq, c.Sk)
    o64, e_o, lse64, _, keepers = ref_forward(c, q, k, v, None, keep=True)
    bound = rounded(o64, e_o)[1]
    E = edge_keys(c.Sk)
    for e, j in enumerate(E):
        if c.Sk == 1:
            continue  # a row with its only key dropped has no softmax
        moved = 0.0
        for b in range(c.B):
            P = keepers[b][0]
            rows = torch.arange(e, c.Sq, len(E))
            if rows.numel() == 0:
                continue
            pj = P[:, rows, j][..., None]
            shift = (pj / (1.0 - pj).clamp_min(1e-9)) * (o64[b][:, rows] - v[b][:, j].double()[:, None, :]).abs()  # out without key j, exactly
            moved = max(moved, float((shift / bound[b][:, rows]).max()))
            assert float(pj.min()) > 0.25, (name, j, float(pj.min()))
        assert moved >= 8.0, (name, "key", j, moved)
    back = ref_backward(c, q, k, v, None, o64.to(bf16), lse64.float(), do, keep=True)
    bdv = back["dv"][1]
    for r in boundary_rows(c.Sq):
        moved = 0.0
        for b in range(c.B):
            pb, dod = back["keep"][b]
            contrib = pb[:, r, :, None] * dod[:, r, None, :]  # [H, Sk, d]: what row r adds to dV
            moved = max(moved, float((contrib.abs() / bdv[b]).max()))
        assert moved >= 8.0, (name, "row", r, moved)


# ----------------------------------------------------------------------------------------------------
# second context

def ctx2_inputs(B, H, Sq, Sk, regime, exact=False):
    d = 128
    scale = f32r(1.0 / math.sqrt(d))
    seed = 1000 * Sk + 10 * Sq + B + (0 if regime == "randn" else 5)
    q, k, v, do = make_qkvdo(d, B, H, Sq, Sk, scale, regime, seed)
    g = torch.Generator()
    g.manual_seed(seed + 1)
    first = torch.randn(B, H, Sq, d, generator=g).to(bf16)
    if exact:  # q = 0: every p is 1, l = Sk (a power of two); v and out_first multiples of 2^-3 below 4: every sum exact in fp32
        q = torch.zeros_like(q)
        v = (torch.randint(-31, 32, v.shape, generator=g).float() / 8.0).to(bf16)
        first = (torch.randint(-31, 32, first.shape, generator=g).float() / 8.0).to(bf16)
    return q, k, v, do, first, scale


def ctx2_reference(B, H, Sq, Sk, q, k, v, do, o_first, dq_first, scale):
    c = Case("ctx2", 128, B, H, Sq, Sk)
    o64, e_o, lse64, e_lse = ref_forward(c, q, k, v, None, exact_max=True)
    oi, e_oi = rounded(o64, e_o)
    out = oi + o_first.double()
    ref = {"out": rounded(out, e_oi), "lse": (lse64, e_lse)}
    # dq from the lse it is given (fp32 of the reference's), delta formed from p dP
    lse_in = lse64.float()
    d = 128
    DQ, EDQ = [], []
    for b in range(B):
        qd, kd, vd, dod = q[b].double(), k[b].double(), v[b].double(), do[b].double()
        lse = lse_in[b].double()[..., None]
        S = qd @ kd.transpose(-1, -2)
        A = qd.abs() @ kd.abs().transpose(-1, -2)
        arg = S * c.sl - lse
        e_arg = (d + 6) * U * (lse.abs() + c.sl * A) + U * arg.abs()
        p = torch.exp2(arg)
        e_p = p * (torch.expm1(LN2 * e_arg) + EXP2_REL)
        dP = dod @ vd.transpose(-1, -2)
        e_dP = (d + 3) * U * (dod.abs() @ vd.abs().transpose(-1, -2))
        delta = (p * dP).sum(-1, keepdim=True)
        e_delta = (e_p * dP.abs() + (p + e_p) * e_dP).sum(-1, keepdim=True) + (Sk + 3) * U * ((p + e_p) * (dP.abs() + e_dP)).sum(-1, keepdim=True)
        dS = p * (dP - delta)
        e_dS = e_p * (dP - delta).abs() + (p + e_p) * (e_dP + e_delta + U * (dP.abs() + delta.abs())) + U * dS.abs()
        dSb, e_dSb = rounded(dS, e_dS)
        dq = scale * (dSb @ kd)
        e_dq = scale * (e_dSb @ kd.abs() + (Sk + 3) * U * ((dSb.abs() + e_dSb) @ kd.abs()))
        dqb, e_dqb = rounded(dq, e_dq)
        r, e = rounded(dqb + dq_first[b].double(), e_dqb)
        DQ.append(r), EDQ.append(e)
    ref["dq"] = (torch.stack(DQ), torch.stack(EDQ))
    return c, ref, lse_in


def ctx2_standin(c, bufs, fault=None):
    """bufs: q, k, v, dout, first (out_first), out, dqf (dq_first), dq as Buf; lse, lse_in flat."""
    B, H, Sq, Sk, d = c.B, c.H, c.Sq, c.Sk, c.d
    nt = cdiv(Sk, 64)
    q, k0, v0, do = bufs["q"].get().float(), bufs["k"].get().float(), bufs["v"].get().float(), bufs["dout"].get().float()
    live = Sk - 1 if fault == "ctx2_tail_dropped" and Sk % 64 else Sk
    k, v = _pad_keys(k0, nt * 64, False), _pad_keys(v0, nt * 64, False)
    mask = torch.zeros(nt * 64)
    mask[live:] = -math.inf
    m = torch.full((B, H, Sq), -math.inf)
    l = torch.zeros(B, H, Sq)
    acc = torch.zeros(B, H, Sq, d)
    for t in range(nt):
        ks, vs = k[:, :, t * 64:(t + 1) * 64], v[:, :, t * 64:(t + 1) * 64]
        s = q @ ks.transpose(-1, -2) + mask[t * 64:(t + 1) * 64]
        x = (s * torch.tensor(c.sl, dtype=f32))
        m_new = torch.maximum(m, x.max(-1).values)
        alpha = torch.exp2(m - m_new)
        pb = bfr(torch.exp2(x - m_new[..., None]))
        l = l * alpha + pb.sum(-1)
        acc = acc * alpha[..., None] + pb @ vs
        m = m_new
    oi = acc * (1.0 / l)[..., None]
    first = bufs["first"].get().float()
    out = bfr(first + oi) if fault == "ctx2_sum_before_round" else bfr(first + bfr(oi))
    bufs["out"].put(out)
    bufs["lse"][:B * H * Sq] = (m + torch.log2(l)).flatten()
    lse = bufs["lse_in"][:B * H * Sq].view(B, H, Sq)
    ps, dps = [], []
    for t in range(nt):
        ks, vs = k[:, :, t * 64:(t + 1) * 64], v[:, :, t * 64:(t + 1) * 64]
        x = (q @ ks.transpose(-1, -2)) * torch.tensor(c.sl, dtype=f32)
        p = torch.where(torch.arange(t * 64, t * 64 + 64) < live, torch.exp2(x - lse[..., None]), torch.zeros(()))
        ps.append(p), dps.append(do @ vs.transpose(-1, -2))
    delta = sum((p * dp).sum(-1) for p, dp in zip(ps, dps))
    dq = torch.zeros(B, H, Sq, d)
    for t in range(nt):
        dq = dq + bfr(ps[t] * (dps[t] - delta[..., None])) @ k[:, :, t * 64:(t + 1) * 64]
    bufs["dq"].put(bfr(bufs["dqf"].get().float() + bfr(dq * c.scale)))


def ctx2_buffers(B, H, Sq, Sk, n, q, k, v, do, first, dq_first, lse_in, inplace):
    d = 128
    bufs = {}
    for t, (name, val, S, is_in) in enumerate((("q", q, Sq, True), ("k", k, Sk, True), ("v", v, Sk, True), ("dout", do, Sq, True), ("first", first, Sq, True),
                                               ("out", None, Sq, False), ("dq", dq_first if inplace else None, Sq, False))):
        off, st, numel = layout(KINDS[(n + t) % 4], B, H, S, d, t)
        if name == "out":
            off, st, numel = bufs["first"].off, bufs["first"].st, bufs["first"].flat.numel()  # out_first has out's strides
        bufs[name] = Buf(torch.full((numel,), NAN if is_in else OUT_SENT, dtype=bf16), off, st, (B, H, S, d))
        if val is not None:
            bufs[name].put(val)
    st6 = [tuple(bufs[nm].st) for nm in ("q", "k", "v", "dout", "out", "dq")]  # (out_first / dq_first share out's / dq's strides by contract)
    assert len(set(st6)) == 6, st6
    if inplace:
        bufs["dqf"] = bufs["dq"]
    else:
        bufs["dqf"] = Buf(torch.full_like(bufs["dq"].flat, NAN), bufs["dq"].off, bufs["dq"].st, bufs["dq"].shape)
        bufs["dqf"].put(dq_first)
    rows = B * H * Sq
    bufs["lse"] = torch.full((rows + 16,), F32_SENT, dtype=f32)
    bufs["lse_in"] = torch.full((rows + 16,), F32_SENT, dtype=f32)
    bufs["lse_in"][:rows] = lse_in.flatten()
    return bufs


def ctx2_device(c, bufs):
    from finetrainers_amd import _lib

    lib = _lib.load()
    dev = {}
    for name in ("q", "k", "v", "dout", "first", "out", "dq", "dqf"):
        dev[name] = dev["dq"] if name == "dqf" and bufs["dqf"] is bufs["dq"] else bufs[name].flat.to(_dev())
    lse, lse_in = bufs["lse"].to(_dev()), bufs["lse_in"].to(_dev())
    t = _lib.AttnDesc()
    t.B, t.H, t.Sq, t.Sk, t.d, t.scale = c.B, c.H, c.Sq, c.Sk, c.d, c.scale
    for field, name in (("q_strides", "q"), ("k_strides", "k"), ("v_strides", "v"), ("o_strides", "out"), ("do_strides", "dout"), ("dq_strides", "dq")):
        a = getattr(t, field)
        a[0], a[1], a[2] = bufs[name].st
    p = lambda name: dev[name].data_ptr() + 2 * bufs[name].off
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.ftmi_attn_ctx2_fwd(ctypes.byref(t), p("q"), p("k"), p("v"), p("first"), p("out"), lse.data_ptr(), st), "ftmi_attn_ctx2_fwd")
    _lib.check(lib.ftmi_attn_ctx2_dq(ctypes.byref(t), p("q"), p("k"), p("v"), lse_in.data_ptr(), p("dout"), p("dqf"), p("dq"), st), "ftmi_attn_ctx2_dq")
    torch.cuda.synchronize()
    bufs["out"].flat.copy_(dev["out"].cpu()), bufs["dq"].flat.copy_(dev["dq"].cpu()), bufs["lse"].copy_(lse.cpu())


def run_ctx2(shape, n, regime, backend, fault=None, inplace=False, exact=False):
    B, H, Sq, Sk = shape
    q, k, v, do, first, scale = ctx2_inputs(B, H, Sq, Sk, regime, exact)
    g = torch.Generator()
    g.manual_seed(Sq + Sk)
    dq_first = torch.randn(B, H, Sq, 128, generator=g).to(bf16)
    c, ref, lse_in = ctx2_reference(B, H, Sq, Sk, q, k, v, do, first, dq_first, scale)
    if exact:  # every operation of the forward is exact: the reference is the output, bit for bit
        oi = bfr(v.double().sum(-2, keepdim=True) / Sk).expand(B, H, Sq, 128)
        ref["out"] = (bfr(first.double() + oi), torch.zeros(B, H, Sq, 128, dtype=f64))
    bufs = ctx2_buffers(B, H, Sq, Sk, n, q, k, v, do, first, dq_first, lse_in, inplace)
    backend(c, bufs) if fault is None else backend(c, bufs, fault)
    if not inplace:  # a second launch onto used outputs (in place the second launch would add onto the first's result)
        keep = {nm: bufs[nm].flat.clone() for nm in ("out", "dq")}
        backend(c, bufs) if fault is None else backend(c, bufs, fault)
        for nm, tns in keep.items():
            assert torch.equal(tns.view(torch.int16), bufs[nm].flat.view(torch.int16)), f"ctx2 {shape}: {nm} differs between two launches"
    return compare(c, bufs, ref, names=("out", "lse", "dq"))


@pytest.mark.parametrize("shape", CTX2_CASES)
def test_ctx2_stand_in_passes_every_bound(shape):
    for regime in REGIMES:
        for inplace in (False, True):
            worst = run_ctx2(shape, CTX2_CASES.index(shape), regime, ctx2_standin, inplace=inplace)
        print(f"[attention stand-in] ctx2 {shape} {regime:5s} " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_ctx2_seeded_faults_are_rejected():
    run_ctx2((2, 4, 48, 64), 1, "randn", ctx2_standin, exact=True)
    with pytest.raises(AssertionError):
        run_ctx2((2, 4, 48, 64), 1, "randn", ctx2_standin, fault="ctx2_sum_before_round", exact=True)
    hits = 0
    for shape in ((2, 4, 48, 63), (1, 1, 48, 65), (2, 4, 129, 257)):
        for regime in REGIMES:
            try:
                run_ctx2(shape, 0, regime, ctx2_standin, fault="ctx2_tail_dropped")
            except AssertionError:
                hits += 1
    assert hits >= 3, hits


# ----------------------------------------------------------------------------------------------------
# device tests

def boundary_distance(v):
    """Relative distance of fp64 values to the nearest bf16 rounding boundary."""
    a = v.abs()
    ulp = ulp_bf(a)
    frac = torch.remainder(a / ulp.clamp_min(1e-300), 1.0)
    return (frac - 0.5).abs() * ulp / a.clamp_min(1e-300)


def bf_nearest(x):
    """fp64 -> the nearest bf16 number in ONE rounding (through fp32 it would be two), as fp64."""
    b = bfr(x)
    u = ulp_bf(x.abs())
    cands = torch.stack([b - u, b, b + u])
    return cands.gather(0, (cands - x).abs().argmin(0, keepdim=True))[0]


def sweep_exp2_inputs():
    """[1, 64, 4096] fp32 biases (natural units).  Aimed at the rounding boundaries: for every midpoint m of two neighbouring bf16 numbers in [2^-20, 2^9) the
    fp32 bias whose b2 = fp32(kb log2 e) is nearest log2(m) and its 32 fp32 neighbours on either side, so that exp2(b2) lies a few u from a boundary, on both sides,
    at a step of about ulp(b2) ln 2; the remaining slots hold uniform values with b2 in [-29, 9]."""
    g = torch.Generator()
    g.manual_seed(11)
    kb = (torch.rand(64 * 4096, generator=g, dtype=f64) * 26.0 - 20.0).float()
    kb[:4] = torch.tensor([0.0, 1.0, -1.0, 6.0])
    mids = (2.0 ** torch.arange(-20, 9, dtype=f64))[:, None] * (1.0 + (2.0 * torch.arange(128, dtype=f64) + 1.0) / 256.0)[None, :]
    kb0 = (torch.log2(mids.flatten()) / LOG2E32).float()
    aimed = (kb0.view(torch.int32)[:, None] + torch.arange(-32, 33, dtype=torch.int32)[None, :]).view(f32).flatten()
    assert aimed.numel() <= kb.numel() - 4 and bool(torch.isfinite(aimed).all())
    kb[4:4 + aimed.numel()] = aimed
    return kb.view(1, 64, 4096)


@pytest.mark.gpu
def test_instruction_error_figures():
    """EXP2_SEEN and LOG2_SEEN on the device (see BOUNDS): each within the figure the bounds use, and below 2^-20 (anything larger is a finding, not a figure)."""
    from finetrainers_amd import _lib

    lib = _lib.load()
    dev, st = _dev(), torch.cuda.current_stream().cuda_stream
    # exp2 through dV of attn_bwd_dkdv_kernel<1, 2>: one query row, q = 0, lse = 0, out = 0, v = 0, dout = 1 -> dV[j, :] = bf(exp2(b2_j))
    B, H, Sq, Sk, d = 1, 64, 1, 4096, 64
    kb = sweep_exp2_inputs()
    z = lambda S, val: torch.full((B, H, S, d), val, dtype=bf16, device=dev)
    q, k, v, o, do = z(Sq, 0.0), z(Sk, 0.0), z(Sk, 0.0), z(Sq, 0.0), z(Sq, 1.0)
    dq, dk, dv = z(Sq, 0.0), z(Sk, 0.0), z(Sk, 0.0)
    lse, delta, kbd = torch.zeros(B, H, Sq, device=dev), torch.zeros(B, H, Sq, device=dev), kb.to(dev)
    t = _lib.AttnDesc()
    t.B, t.H, t.Sq, t.Sk, t.d, t.scale = B, H, Sq, Sk, d, 0.125
    for field, S in (("q_strides", Sq), ("k_strides", Sk), ("v_strides", Sk), ("o_strides", Sq), ("do_strides", Sq), ("dq_strides", Sq), ("dk_strides", Sk),
                     ("dv_strides", Sk)):
        a = getattr(t, field)
        a[0], a[1], a[2] = H * S * d, S * d, d
    t.bias_strides[0], t.bias_strides[1] = H * Sk, Sk
    _lib.check(lib.ftmi_attn_bwd(ctypes.byref(t), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                 dv.data_ptr(), delta.data_ptr(), kbd.data_ptr(), st), "ftmi_attn_bwd")
    torch.cuda.synchronize()
    got = dv.cpu().float()
    assert bool((got == got[..., :1]).all())
    want64 = torch.exp2(_bias2(kb)).flatten()
    mism = got[..., 0].flatten() != bf_nearest(want64).float()
    dist = boundary_distance(want64)
    exp2_seen, flips = (float(dist[mism].max()) if bool(mism.any()) else 0.0), int(mism.sum())
    near = {k: int((dist < k * U).sum()) for k in (0.5, 1, 2)}  # arguments that an error of k u (relative) towards the boundary would have flipped
    print(f"[attention] exp2 sweep resolution: {near[0.5]} / {near[1]} / {near[2]} of {dist.numel()} arguments lie within 0.5 / 1 / 2 u of a bf16 rounding boundary; "
          f"smallest distance {float(dist.min()):.3e}")
    # log2 through lse of the biased forward: q = 0 -> every kept key has p = 1, l = n exactly, m = 0: lse = log2(n)
    Sk2 = 4096
    keep = torch.arange(Sk2)[None, :] < torch.arange(1, Sk2 + 1)[:, None]
    kb2 = torch.where(keep, torch.zeros(()), torch.full((), -math.inf)).float().view(1, Sk2, Sk2).to(dev)
    z2 = lambda heads, S: torch.zeros(1, heads, S, d, dtype=bf16, device=dev)
    q2, k2, v2, o2 = z2(Sk2, 1), z2(1, Sk2), z2(1, Sk2), z2(Sk2, 1)  # one K / V shared by every head: head stride 0
    lse2 = torch.zeros(1, Sk2, 1, device=dev)
    t.B, t.H, t.Sq, t.Sk = 1, Sk2, 1, Sk2
    for field, sh in (("q_strides", d), ("k_strides", 0), ("v_strides", 0), ("o_strides", d)):
        a = getattr(t, field)
        a[0], a[1], a[2] = 0, sh, d
    t.bias_strides[0], t.bias_strides[1] = Sk2 * Sk2, Sk2
    _lib.check(lib.ftmi_attn_fwd(ctypes.byref(t), q2.data_ptr(), k2.data_ptr(), v2.data_ptr(), o2.data_ptr(), lse2.data_ptr(), kb2.data_ptr(), st), "ftmi_attn_fwd")
    torch.cuda.synchronize()
    n = torch.arange(1, Sk2 + 1, dtype=f64)
    want = torch.log2(n)
    log2_seen = float(((lse2.cpu().flatten().double() - want).abs() / want.clamp_min(1.0)).max())
    print(f"[attention] exp2: EXP2_SEEN {exp2_seen:.4e} = {exp2_seen / U:.3f} u over {flips} flipped outputs of {want64.numel()} (in use {EXP2_SEEN:.4e}, "
          f"EXP2_REL {EXP2_REL:.4e}); log2: LOG2_SEEN {log2_seen:.4e} = {log2_seen / U:.3f} u over {n.numel()} arguments (in use {LOG2_SEEN:.4e}, LOG2_REL {LOG2_REL:.4e})")
    for fig, rel in ((exp2_seen, EXP2_REL), (log2_seen, LOG2_REL)):
        assert fig <= 2.0**-20, f"instruction error {fig:.3e} above 2^-20: a finding, not a figure to adopt"
        assert fig <= rel, f"instruction error {fig:.3e} above the figure the bounds use ({rel:.3e})"


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_attention_contract(name):
    c = BY_NAME[name]
    t0 = time.time()
    for regime in REGIMES:
        worst = run_case(c, CASES.index(c), regime, run_device)
        print(f"[attention] {name:7s} {regime:5s} {' '.join(dispatch(c.d, c.B, c.H, c.Sq, c.Sk, c.bias)[:3])}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    print(f"[attention] {name}: {time.time() - t0:.1f} s")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["r64", "r128"])
def test_attention_chained_forward_to_backward(name):
    """The backward on the device's own out and lse (the way the provider runs it); its reference is the fp64 backward of exactly those inputs."""
    c = BY_NAME[name]
    for regime in REGIMES:
        run = functools.partial(run_device, chained=True)
        worst = run_case(c, CASES.index(c), regime, run, chained=True)
        print(f"[attention chained] {name:7s} {regime:5s} " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CTX2_CASES)
def test_ctx2_contract(shape):
    for regime in REGIMES:
        for inplace in (False, True):
            worst = run_ctx2(shape, CTX2_CASES.index(shape), regime, ctx2_device, inplace=inplace)
            print(f"[attention] ctx2 {shape} {regime:5s} inplace={inplace}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    run_ctx2((2, 4, 48, 64), 1, "randn", ctx2_device, exact=True)
    run_ctx2((1, 1, 33, 256), 2, "randn", ctx2_device, exact=True)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
def test_ops_place_out_dq_dk_where_the_caller_says(d):
    """ops.attn_fwd(out=) / ops.attn_bwd(dq=, dk=, dv_out=): the same bits as the self-allocated outputs, written into views of padded buffers whose
    padding survives; a view of the wrong shape or type is refused."""
    from finetrainers_amd import ops

    dev = _dev()
    B, H, Sq, Sk = 2, 3, 65, 33
    q, k, v, do = (t.to(dev) for t in make_qkvdo(d, B, H, Sq, Sk, f32r(1.0 / math.sqrt(d)), "randn", 5 + d))
    o0, lse0 = ops.attn_fwd(q, k, v)
    dq0, dk0, dv0 = ops.attn_bwd(q, k, v, o0, lse0, do)

    def padded(S):  # [B, H, S + 1, d + 8] buffer, the view in its corner
        buf = torch.full((B, H, S + 1, d + 8), OUT_SENT, dtype=bf16, device=dev)
        return buf, buf[:, :, :S, :d]

    (ob, o1), (qb, dq1), (kb, dk1), (vb, dv1) = padded(Sq), padded(Sq), padded(Sk), padded(Sk)
    o_ret, lse1 = ops.attn_fwd(q, k, v, out=o1)
    assert o_ret is o1 and torch.equal(o1, o0) and torch.equal(lse1, lse0)
    got = ops.attn_bwd(q, k, v, o1, lse1, do, dv_out=dv1, dq=dq1, dk=dk1)
    assert got[0] is dq1 and got[1] is dk1 and got[2] is dv1
    assert torch.equal(dq1, dq0) and torch.equal(dk1, dk0) and torch.equal(dv1, dv0)
    for buf, S in ((ob, Sq), (qb, Sq), (kb, Sk), (vb, Sk)):
        assert bool((buf[:, :, S:, :] == OUT_SENT).all()) and bool((buf[:, :, :, d:] == OUT_SENT).all())
    with pytest.raises(ValueError):
        ops.attn_fwd(q, k, v, out=o1[:, :, :-1])
    with pytest.raises(ValueError):
        ops.attn_bwd(q, k, v, o1, lse1, do, dq=dq1.float())
    with pytest.raises(ValueError):
        ops.attn_bwd(q, k, v, o1, lse1, do, dk=dq1)
