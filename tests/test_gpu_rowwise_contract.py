"""The launch contract of the row-wise kernels (csrc/wan.hip, csrc/cogvideox.hip, csrc/rowwise.hip) per element against fp64.

CONTRACT (read from the kernels; bf() = round to nearest even to bf16, everything else fp32; LN(x) = (x - mean) * rstd, rstd = rsqrtf(var + eps), var the mean
of (x - mean)^2 -- two passes; sums over a row in any order; b = row // rows_per_batch, pos = row % rows_per_batch):
  Wan (one wavefront per row, NC 16-byte chunks per lane; FTMI_WAN_DISPATCH: NC = ceil(D / 512) for 1..4, 8 for 5..8, else 10)
    ln            y = bf(LN(x) [* w + b] [* (1 + scale_b) + shift_b])                                one rounding; scale / shift fp32, rows mod_bstride apart
    ln_bwd        g = dy * (w | 1 + scale_b | w (1 + scale_b));  d = rstd (g - mean(g) - xhat mean(g xhat));  dx = bf(d), with dres: bf(dres + bf(d));
                  dres and dx are both addressed with ld_y;  red1[r] += sum dy, red2[r] += sum dy xhat over the rows (r = b if red_per_batch else 0)
    rms_rope      rstd = rsqrtf(mean(x^2) + eps); n = bf(x rstd w); y = bf(n rotated): pair k of a head, (n[2k], n[2k+1]) * (cos + i sin)[pos, k]; no table: y = n
    rms_rope_bwd  dn = bf(dy rotated by the conjugate) (no table: dy); red2 += sum dn xhat; g = dn w; dx = bf(rstd (g - xhat mean(g xhat)))
    gate_res      y = bf(x + branch * gate_b) (gate fp32; none: bf(x + branch))                       exact: one fp32 product, one fp32 sum, one rounding
    gate_res_bwd  dy = bf(dout * gate_b) (exact);  red1[r] += sum dout * branch (only when red1 is given; the branch is not read otherwise)
    colsum        red1[r] += sum over rows of x; rows wider than 4096 in slabs of 4096 columns, each slab its own launch and NC
  CogVideoX / HunyuanVideo (FTMI_COG_DISPATCH: NC = ceil(D / 512) for 1..4, else 8; tables bf16, row (b, pos >= seg0) of [B, 2, D] or row b of [B, D] if seg0 == 0)
    ln_mod        y = bf(bf(bf(LN(x) w + b) onep) + shift)
    ln_mod_bwd    g = bf(dy onep) w;  d = rstd (g - mean(g) - xhat mean(g xhat));  dx = bf(d), with dres: bf(dres + bf(d))
    head_ln       per head of 64 channels LN(x) w + b, or (rms) per head of 128 channels x rstd w; on the rows pos >= seg0 with table row pos - seg0 (cos / sin fp32
                  [rows_per_batch - seg0, head_dim]): n = bf(.), out[2i] = n[2i] cos[2i] - n[2i+1] sin[2i], out[2i+1] = n[2i+1] cos[2i+1] + n[2i] sin[2i+1]; y = bf(out)
    head_ln_bwd   on the rotated rows t[2i] = bf(bf(dy[2i] cos[2i]) + bf(dy[2i+1] sin[2i+1])), t[2i+1] = bf(bf(dy[2i+1] cos[2i+1]) - bf(dy[2i] sin[2i])) (each branch a
                  bf16 tensor); g = t w; dx = bf(rstd (g - mean(g) - xhat mean(g xhat))) over the head (rms: no mean(g) term)
    gate_residual out = bf(res + bf(gate y)), without res: bf(gate y)                                 exact
  LTX (width 2048, no NC dispatch; Dv = valid width of a zero-padded row, 0 = 2048; tables bf16)
    norm_modulate      mean and var over the Dv valid channels (rms: mean(x^2) over Dv, no mean); y = bf(bf(bf(norm x) onep_b) + shift_b); LN: channels >= Dv are 0
    norm_modulate_bwd  g = bf(dy onep_b); d as above with the means over Dv (rms: no mean(g) term); dx = bf(d) | bf(dres + bf(d)); LN: channels >= Dv are 0;
                       dx2 = bf(dx gate2_b)  (the ROUNDED dx)
    qknorm_rope        rstd over Dv; weight row (row % w_rows); n = bf(x rstd w); y = bf(n rotated by (cos, sin)[pos, k], pair k = column // 2) (no table: n);
                       pair launch: (x2, w2, y2) with the same strides, table rows and w_rows
    qknorm_rope_bwd    dn[2k] = bf(bf(dy[2k] c) + bf(dy[2k+1] s)), dn[2k+1] = bf(bf(dy[2k+1] c) - bf(dy[2k] s)); g = dn w; dx = bf(rstd (g - xhat mean(g xhat)));
                       row groups: logical row i sits at buffer row (i // row_grp) * row_grp_span + i % row_grp of x / dy / dx
  Every launcher returns 0 without a launch for rows == 0.

REFERENCE: the table above in fp64 (torch, CPU), one function per launcher (c_*), each written once over a small value type: V carries the fp64 value AND a bound
on what an fp32 evaluation of the same expression can differ by; the same functions run on plain fp32 tensors as the stand-in of the CPU self-checks.

BOUNDS (u = 2^-24, ulp(a) = bf16 spacing at |a|), the rules V applies (no figure here comes from a kernel's output):
  a + b, a - b, a * b, a / n   the propagated error of the operands + u (|result| + that error)
  sum of n terms, any order    sum of the terms' errors + (n + 2) u sum(|term| + its error)
  rsqrtf(a), a known to e      e / 2 (a - e)^-3/2 + RSQ_REL rsqrt(a);  RSQ_REL: the hardware instruction's own error, not in the ISA notes at hand, so measured:
                               test_rsqrtf_error_figure reads rstd out of wan_rms_rope_bwd (a row holding one power of two p and one t, dy = 1 at p's column: red2 =
                               p rsqrtf((p^2 + t^2) / D + eps), every other operation exact) over 3072 arguments in 2^-17 .. 2^11 (eps alone is 2^-20, the mean square
                               of an offset row 2^10) against fp64: largest relative error RSQ_SEEN = 8.6129e-08 (1.445 u); RSQ_REL = 2 RSQ_SEEN = 1.7226e-07
  bf(v), v known to e          e + ulp(|v| + e)
  column sums, launched twice onto a non-zero buffer: init + 2 S with (2 (rows + strips) + 3) u (|init| + 2 sum(|term| + error)) + 2 sum of the terms' errors
  exact outputs (gate_res, gate_res_bwd dy, gate_residual, padded LN channels, sentinels): bound 0; the reference rounds to fp32 after each of their operations.
  Asserted per case: every output finite; |got - ref| <= bound for every element; for every block of 32 rows x 512 columns of a bf16 output (a ragged last row
  block of fewer than 8 rows joins the one above; fewer than 8 rows or a width that is no multiple of 512: the ragged column tail joins the block to its left, a
  narrower output is one block) at most 2 % of the elements differ from the reference at all; padding sentinels of every output intact.

CASES (every operand that has a stride is a view of width D into rows of D + 64 elements (ln_bwd / rms_rope_bwd outputs: D + 128, so that ld_y differs from ld_x),
one spare row below; input padding IN_SENT, output padding OUT_SENT; modulation rows D + 64 apart; row 1 of x is 30 + normal, row 2 exact zeros)
  family            D -> NC
  Wan               64:1 512:1 576:2 1024:2 1536:3 2048:4 2112:8 4096:8 4160:10 5120:10          all seven launchers (colsum also 8960 = 8 + 8 + 2, 4160 = 8 + 1)
  Cog               64:1 512:1 576:2 1536:3 1920:4 2112:8 4096:8                                   ln_mod, ln_mod_bwd, head_ln (64, LN) fwd / bwd, gate_residual
  Cog head RMS 128  128:1 640:2 1536:3 2048:4 3072:8 4096:8                                        head_ln (128, RMS) fwd / bwd through ftmi_head_rms_rope_*
  LTX               2048, valid width 0 / 32 / 1024
  rows: (rows_per_batch, B) over {1, 3, 31, 33, 75} x {1, 3}, every pair for every launcher; Cog seg0 over {0, 1, rows_per_batch - 1, rows_per_batch};
  LTX w_rows {1, 3}, row_grp {0, 5} (span 7); optional arguments present and absent; red buffers start non-zero and every launch runs twice.

CPU SELF-CHECKS: the fp32 stand-ins (sums in 512-column / 32-row slices last to first) pass every bound with at most 0.5 % per block; each seeded fault below,
applied to the stand-in, is rejected by at least one case; the case list reaches every NC of every kernel template.
  seeded fault         stands for
  last_slot            the NC dispatch: columns >= 512 (NC - 1) keep the sentinel
  mod_prev_sample      rows_per_batch / mod_bstride: first row of sample b uses sample b - 1's modulation
  seg_swap             mod_row: the row at pos == seg0 takes the text row
  rope_text_row / rope_row_pos / pair_from_column      seg0, head_dim: rope on the last text row; table row pos; Wan pair index from the column
  dres_ld_x            the ld_y rule of dres
  strip_tail           the last rows_per_batch % 32 rows missing from a column sum
  store_not_add        += of the column sums
  all_in_row0          red_per_batch
  slab_offset          slab 2 of colsum written at slab 1
  n_unrounded / dx2_unrounded / dyonep_unrounded      rounding points
  mean_over_D / pad_nonzero                            valid width
  w_rows_ignored / x2_with_w / grp_span_ignored        the LTX _ex arguments
  half_head_128        head_dim 128 at D % 128 != 0 (now refused; shown on a CPU-only case, D = 192)

MEASURED on an MI355X (largest |got - ref| / bound and largest block mismatch share over the cases of each launcher; a flipped rounding costs one ulp against a
bound of one ulp + the propagated error, hence the figures just below 1; the column sums and the exact outputs stay far inside):
  family  launcher                       err / bound   block share
  Wan     ln                               0.954         0.0007
          ln_bwd (dx, red1, red2)          0.903         0.0005
          rms_rope                         0.617         0.0007
          rms_rope_bwd (dx, red2)          0.954         0.0004
          gate_res                         exact         0
          gate_res_bwd (dy exact, red1)    0.082         0
          colsum                           0.198         -
  Cog     ln_mod                           0.345         0.0001
          ln_mod_bwd                       0.280         0.0004
          head_ln (64, LN)                 0.998         0.0002
          head_ln_bwd (64, LN)             0.995         0.0002
          gate_residual                    exact         0
          head_ln (128, RMS)               0.999         0.0007
          head_ln_bwd (128, RMS)           0.998         0.0001
  LTX     norm_modulate                    0.520         0.0020
          norm_modulate_bwd (dx, dx2)      0.448         0.0001
          qknorm_rope (+ pair)             0.507         0.0002
          qknorm_rope_bwd (+ pair, groups) 0.976         0.0001
  rsqrtf: 8.6129e-08 (see BOUNDS).  Every case is within its bounds.
fp32 stand-ins on the CPU over the same cases (test_fp32_stand_ins_pass_every_bound): largest err / bound 0.999, largest block share 0.0007, except the RMS form of
norm_modulate_bwd: 0.0052.  There d = rstd g on a zero row, g of 8 significant bits and rstd = rsqrt(fp32(1e-6)) = 1000 exactly in fp32 but 1000.0000015 in fp64, so
2^-7 of the products sit on a bf16 tie that fp32 rounds to even and the reference upwards (a third of a three-row block is such a row): the fp32 evaluation itself
crosses bf16 boundaries, and this form is held to the 2 % cap only.  (The hardware's rsqrtf does not return 1000 there; the kernel's figure is in the table.)
"""

import math

import pytest
import torch

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0**-24
RSQ_SEEN = 8.6129e-08  # largest relative error of rsqrtf seen by test_rsqrtf_error_figure on an MI355X
RSQ_REL = 2.0 * RSQ_SEEN
IN_SENT = 3.0e4     # padding of the inputs: wrecks the result if read as data
OUT_SENT = -1536.0  # padding of the outputs (exact in bf16): must survive the launch
CAP, STANDIN_CAP = 0.02, 0.005
EPS6, EPS5 = float(torch.tensor(1e-6, dtype=f32)), float(torch.tensor(1e-5, dtype=f32))  # the fp32 values the launchers receive


def _threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))


# ----------------------------------------------------------------------------------------------------
# the value type: fp64 value + bound on the error of an fp32 evaluation

def bfr(t):
    return t.float().to(bf16).to(t.dtype)


def ulp_bf(a):
    _, e = torch.frexp(a)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - 8), torch.zeros_like(a))


class V:
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v if torch.is_tensor(v) and v.dtype == f64 else torch.as_tensor(v, dtype=f64)
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def of(o):
        return o if isinstance(o, V) else V(o)

    def _done(self, v, e):
        return V(v, e + U * (v.abs() + e))

    def __add__(self, o):
        o = V.of(o)
        return self._done(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return self._done(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        return self._done(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, n):  # by an exact count
        return self._done(self.v / n, self.e / n)

    def __neg__(self):
        return V(-self.v, self.e)


def lift(t, dt):
    return V(t.double()) if dt is f64 else t.float()


def S(fn, *xs):
    """A structural operation (indexing, reshaping, stacking) on values and errors alike."""
    if isinstance(xs[0], V):
        return V(fn(*[x.v for x in xs]), fn(*[x.e for x in xs]))
    return fn(*xs)


def bf(x):
    if isinstance(x, V):
        return V(bfr(x.v), x.e + ulp_bf(x.v.abs() + x.e))
    return bfr(x)


def fl(x):
    """The fp32 rounding of ONE operation on exact operands (the exact outputs): the value rounded to fp32, no error left."""
    return V(x.v.float().double()) if isinstance(x, V) else x


def rsum(x, sl=512):
    """Sum over the last axis (kept).  fp32: slices of `sl` columns, last to first."""
    n = x.v.shape[-1] if isinstance(x, V) else x.shape[-1]
    if isinstance(x, V):
        return V(x.v.sum(-1, keepdim=True), x.e.sum(-1, keepdim=True) + (n + 2) * U * (x.v.abs() + x.e).sum(-1, keepdim=True))
    acc = torch.zeros_like(x[..., :1])
    for c0 in reversed(range(0, n, sl)):
        acc = acc + x[..., c0:c0 + sl].sum(-1, keepdim=True)
    return acc


def rsq(x):
    if isinstance(x, V):
        assert (x.v > 2 * x.e).all(), "rsqrt argument not known well enough"
        v = x.v.rsqrt()
        return V(v, 0.5 * x.e * (x.v - x.e).pow(-1.5) + RSQ_REL * v)
    return torch.rsqrt(x)


def recip(n, like):
    """The fp32 constant 1.0f / n (LTX: sums are multiplied by it)."""
    return V(torch.tensor(1.0 / n, dtype=f64), torch.tensor(U / n, dtype=f64)) if isinstance(like, V) else torch.tensor(1.0 / n, dtype=f32)


def sel(mask, a, b):
    return S(lambda p, q: torch.where(mask, p, q), a, b)


def pairs(x):
    return S(lambda t: t[..., 0::2], x), S(lambda t: t[..., 1::2], x)


def interleave(a, b):
    return S(lambda p, q: torch.stack([p, q], -1).flatten(-2), a, b)


def csum(T, init, B, rpb, per_batch, fault=None):
    """Column sums of the terms T [B * rpb, D] added TWICE (two launches) onto init ([B, D] when per_batch, else [D])."""
    strips = (rpb + 31) // 32
    D = init.shape[-1]
    if isinstance(T, V):
        tv, te = T.v.reshape(B, rpb, D), (T.v.abs() + T.e).reshape(B, rpb, D)
        ee = T.e.reshape(B, rpb, D)
        if per_batch:
            s, a, e, n = tv.sum(1), te.sum(1), ee.sum(1), rpb
        else:
            s, a, e, n = tv.sum((0, 1)), te.sum((0, 1)), ee.sum((0, 1)), B * rpb
        i64 = init.double()
        return V(i64 + 2 * s, 2 * e + (2 * (n + (strips if per_batch else strips * B)) + 3) * U * (i64.abs() + 2 * a))
    t = T.reshape(B, rpb, D)
    if fault == "strip_tail" and rpb % 32:
        t = t[:, :rpb - rpb % 32]
    part = torch.zeros(B, D, dtype=f32)
    for r0 in reversed(range(0, t.shape[1], 32)):
        part = part + t[:, r0:r0 + 32].sum(1)
    if fault == "store_not_add":
        return part.clone() if per_batch else part.sum(0)
    if per_batch:
        if fault == "all_in_row0":
            out = init.clone()
            out[0] = out[0] + part.sum(0) + part.sum(0)
            return out
        return init + part + part
    return init + part.sum(0) + part.sum(0)


def batch_rows(rows, rpb, fault=None):
    r = torch.arange(rows)
    b = r // rpb
    if fault == "mod_prev_sample":
        b = torch.where((r % rpb == 0) & (b > 0), b - 1, b)
    return b


def mod_of(tab, idx, dt):
    """Rows idx of a modulation table."""
    return S(lambda t: t[idx], lift(tab, dt))


# ----------------------------------------------------------------------------------------------------
# the contract, one function per launcher: p = logical inputs and launch fields, dt = f64 (reference and bounds) or f32 (stand-in), fault = a seeded fault

def _ln_stats(x, n, eps):
    mean = rsum(x) / n
    d = x - mean
    return d, rsq(rsum(d * d) / n + eps)


def c_wan_ln(p, dt, fault=None):
    x = lift(p["x"], dt)
    d, rstd = _ln_stats(x, p["D"], p["eps"])
    o = d * rstd
    if p.get("w") is not None:
        o = o * lift(p["w"], dt) + lift(p["b"], dt)
    if p.get("scale") is not None:
        idx = batch_rows(p["rows"], p["rpb"], fault)
        o = o * (1.0 + mod_of(p["scale"], idx, dt)) + mod_of(p["shift"], idx, dt)
    return {"y": bf(o)}


def _dres(p, dt, fault, ld_wrong):
    if fault == "dres_ld_x":  # the rows of dres found with the stride of x
        flat = p["dres_buf"].flatten()
        idx = torch.arange(p["rows"])[:, None] * ld_wrong + torch.arange(p["D"])[None]
        return lift(flat[idx], dt)
    return lift(p["dres"], dt)


def _ln_bwd_tail(g, xh, rstd, n, c1_term=True):
    c2 = rsum(g * xh) / n
    if c1_term:
        return rstd * (g - rsum(g) / n - xh * c2)
    return rstd * (g - xh * c2)


def c_wan_ln_bwd(p, dt, fault=None):
    x, dy = lift(p["x"], dt), lift(p["dy"], dt)
    d, rstd = _ln_stats(x, p["D"], p["eps"])
    xh = d * rstd
    g = dy
    if p.get("w") is not None:
        g = dy * lift(p["w"], dt)
    if p.get("scale") is not None:
        m = 1.0 + mod_of(p["scale"], batch_rows(p["rows"], p["rpb"], fault), dt)
        g = dy * (lift(p["w"], dt) * m) if p.get("w") is not None else dy * m
    dv = _ln_bwd_tail(g, xh, rstd, p["D"])
    out = {"dx": bf(_dres(p, dt, fault, p["ld_x"]) + bf(dv)) if p.get("dres") is not None else bf(dv)}
    if p.get("red1") is not None:
        out["red1"] = csum(dy, p["red1"], p["B"], p["rpb"], p["per_batch"], fault)
    if p.get("red2") is not None:
        out["red2"] = csum(dy * xh, p["red2"], p["B"], p["rpb"], p["per_batch"], fault)
    return out


def _wan_tables(p, dt, fault):
    """cos / sin of every pair of every row: [rows, D / 2]."""
    half, pos = p["head_dim"] // 2, torch.arange(p["rows"]) % p["rpb"]
    if fault == "pair_from_column":
        idx = (pos[:, None] * half + torch.arange(p["D"] // 2)[None]) % (p["rpb"] * half)
        g = lambda t: t.flatten()[idx]
    else:
        g = lambda t: t[pos].repeat(1, p["D"] // p["head_dim"])
    return lift(g(p["cos"]), dt), lift(g(p["sin"]), dt)


def c_wan_rms_rope(p, dt, fault=None):
    x = lift(p["x"], dt)
    rstd = rsq(rsum(x * x) / p["D"] + p["eps"])
    n = x * rstd * lift(p["w"], dt)
    if p.get("cos") is None:
        return {"y": bf(n)}
    if fault != "n_unrounded":
        n = bf(n)
    cs, sn = _wan_tables(p, dt, fault)
    ne, no = pairs(n)
    return {"y": bf(interleave(ne * cs - no * sn, no * cs + ne * sn))}


def c_wan_rms_rope_bwd(p, dt, fault=None):
    x, dy = lift(p["x"], dt), lift(p["dy"], dt)
    rstd = rsq(rsum(x * x) / p["D"] + p["eps"])
    xh = x * rstd
    dn = dy
    if p.get("cos") is not None:
        cs, sn = _wan_tables(p, dt, fault)
        de, do = pairs(dy)
        r = (lambda t: t) if fault == "n_unrounded" else bf
        dn = interleave(r(de * cs + do * sn), r(do * cs - de * sn))
    out = {"dx": bf(_ln_bwd_tail(dn * lift(p["w"], dt), xh, rstd, p["D"], c1_term=False))}
    if p.get("red2") is not None:
        out["red2"] = csum(dn * xh, p["red2"], p["B"], p["rpb"], False, fault)
    return out


def c_wan_gate_res(p, dt, fault=None):
    x, y = lift(p["x"], dt), lift(p["dy"], dt)
    if p.get("scale") is None:
        return {"y": bf(fl(x + y))}
    return {"y": bf(fl(x + fl(y * mod_of(p["scale"], batch_rows(p["rows"], p["rpb"], fault), dt))))}


def c_wan_gate_res_bwd(p, dt, fault=None):
    dout = lift(p["x"], dt)
    out = {"dy": bf(fl(dout * mod_of(p["scale"], batch_rows(p["rows"], p["rpb"], fault), dt)))}
    if p.get("red1") is not None:
        out["red1"] = csum(dout * lift(p["dy"], dt), p["red1"], p["B"], p["rpb"], p["per_batch"], fault)
    return out


def c_wan_colsum(p, dt, fault=None):
    r = csum(lift(p["x"], dt), p["red1"], p["B"], p["rpb"], p["per_batch"], fault)
    if fault == "slab_offset" and p["D"] > 8192:  # the third slab (columns 8192 ..) lands on the second
        w = p["D"] - 8192
        r = r.clone()
        r[..., 4096:4096 + w] += r[..., 8192:] - p["red1"][..., 8192:]
        r[..., 8192:] = p["red1"][..., 8192:]
    return {"red1": r}


def cog_mod_rows(p, fault=None):
    r = torch.arange(p["rows"])
    b, pos = batch_rows(p["rows"], p["rpb"], fault), r % p["rpb"]
    if p["seg0"] == 0:
        return b
    return b * 2 + ((pos > p["seg0"]) if fault == "seg_swap" else (pos >= p["seg0"])).long()


def c_cog_ln_mod(p, dt, fault=None):
    x = lift(p["x"], dt)
    d, rstd = _ln_stats(x, p["D"], p["eps"])
    n = bf(d * rstd * lift(p["w"], dt) + lift(p["b"], dt))
    mr = cog_mod_rows(p, fault)
    return {"y": bf(bf(n * mod_of(p["onep"], mr, dt)) + mod_of(p["shift"], mr, dt))}


def c_cog_ln_mod_bwd(p, dt, fault=None):
    x, dy = lift(p["x"], dt), lift(p["dy"], dt)
    t = dy * mod_of(p["onep"], cog_mod_rows(p, fault), dt)
    g = (t if fault == "dyonep_unrounded" else bf(t)) * lift(p["w"], dt)
    d, rstd = _ln_stats(x, p["D"], p["eps"])
    dv = _ln_bwd_tail(g, d * rstd, rstd, p["D"])
    return {"dx": bf(lift(p["dres"], dt) + bf(dv)) if p.get("dres") is not None else bf(dv)}


def _heads(p, dt, fault):
    """x as [rows, heads, HD] (a ragged last head zero-filled: only the CPU-only case of the head_dim 128 hole has one), channels per head, rope row mask, tables."""
    HD, D, rows = p["head_dim"], p["D"], p["rows"]
    H = (D + HD - 1) // HD
    cnt = torch.full((H, 1), float(HD), dtype=f64 if dt is f64 else f32)
    if D % HD and fault != "half_head_128":
        cnt[-1] = D % HD

    def split(t):
        t = lift(t, dt)
        return S(lambda a: torch.nn.functional.pad(a, (0, H * HD - D)).reshape(rows, H, HD), t)

    pos = torch.arange(rows) % p["rpb"]
    mask, tabs = None, None
    if p.get("cos") is not None:
        nt = p["cos"].shape[0]
        seg0 = p["seg0"]
        mask = pos >= (seg0 - 1 if fault == "rope_text_row" else seg0)
        tr = (pos % nt) if fault == "rope_row_pos" else (pos - seg0).clamp(0, nt - 1)
        tabs = tuple(lift(t[tr][:, None, :], dt) for t in (p["cos"], p["sin"]))
        mask = mask[:, None, None]
    return split, cnt, mask, tabs


def c_cog_head_ln(p, dt, fault=None):
    split, cnt, mask, tabs = _heads(p, dt, fault)
    x, w = split(p["x"]), lift(p["w"], dt)
    if p["rms"]:
        d = x
    else:
        d = x - rsum(x, 32) / cnt
    rstd = rsq(rsum(d * d, 32) / cnt + p["eps"])
    o = d * rstd * w if p["rms"] else d * rstd * w + lift(p["b"], dt)
    if mask is not None:
        n = o if fault == "n_unrounded" else bf(o)
        (ce, co), (se, so) = pairs(tabs[0]), pairs(tabs[1])
        ne, no = pairs(n)
        o = sel(mask, interleave(ne * ce - no * se, no * co + ne * so), o)
    return {"y": S(lambda t: t.reshape(p["rows"], -1)[:, :p["D"]], bf(o))}


def c_cog_head_ln_bwd(p, dt, fault=None):
    split, cnt, mask, tabs = _heads(p, dt, fault)
    x, dv, w = split(p["x"]), split(p["dy"]), lift(p["w"], dt)
    d = x if p["rms"] else x - rsum(x, 32) / cnt
    rstd = rsq(rsum(d * d, 32) / cnt + p["eps"])
    if mask is not None:
        (ce, co), (se, so) = pairs(tabs[0]), pairs(tabs[1])
        de, do = pairs(dv)
        dv = sel(mask, interleave(bf(bf(de * ce) + bf(do * so)), bf(bf(do * co) - bf(de * se))), dv)
    g = dv * w
    xh = d * rstd
    c2 = rsum(g * xh, 32) / cnt
    o = rstd * (g - xh * c2) if p["rms"] else rstd * (g - rsum(g, 32) / cnt - xh * c2)
    return {"dx": S(lambda t: t.reshape(p["rows"], -1)[:, :p["D"]], bf(o))}


def c_cog_gate_residual(p, dt, fault=None):
    t = bf(fl(mod_of(p["onep"], cog_mod_rows(p, fault), dt) * lift(p["x"], dt)))
    return {"y": bf(fl(lift(p["dres"], dt) + t)) if p.get("dres") is not None else t}


def _ltx_norm(p, x, fault):
    D, Dv = p["D"], p["Dv"] or p["D"]
    inv = recip(D if fault == "mean_over_D" else Dv, x)
    valid = torch.arange(D) < Dv
    if p["ln"]:
        mean = rsum(x) * inv
        d = x - mean
        dd = d * d
        rstd = rsq(rsum(sel(valid, dd, S(torch.zeros_like, dd))) * inv + p["eps"])
    else:
        d, rstd = x, rsq(rsum(x * x) * inv + p["eps"])
    return d, rstd, inv, valid


def _mask_pad(p, o, valid, fault):
    if p["ln"] and fault != "pad_nonzero":
        return sel(valid, o, S(torch.zeros_like, o))
    return o


def c_ltx_nm(p, dt, fault=None):
    x = lift(p["x"], dt)
    d, rstd, inv, valid = _ltx_norm(p, x, fault)
    idx = batch_rows(p["rows"], p["rpb"], fault)
    o = bf(bf(d * rstd) * mod_of(p["onep"], idx, dt)) + mod_of(p["shift"], idx, dt)
    return {"y": bf(_mask_pad(p, o, valid, fault))}


def c_ltx_nm_bwd(p, dt, fault=None):
    x, dy = lift(p["x"], dt), lift(p["dy"], dt)
    idx = batch_rows(p["rows"], p["rpb"], fault)
    t = dy * mod_of(p["onep"], idx, dt)
    g = t if fault == "dyonep_unrounded" else bf(t)
    d, rstd, inv, valid = _ltx_norm(p, x, fault)
    xh = d * rstd
    c2 = rsum(g * xh) * inv
    dv = rstd * (g - rsum(g) * inv - xh * c2) if p["ln"] else rstd * (g - xh * c2)
    o = _mask_pad(p, lift(p["dres"], dt) + bf(dv) if p.get("dres") is not None else dv, valid, fault)
    out = {"dx": bf(o)}
    if p.get("gate2") is not None:
        out["dx2"] = bf((o if fault == "dx2_unrounded" else bf(o)) * mod_of(p["gate2"], idx, dt))
    return out


def _ltx_tables(p, dt):
    pos = torch.arange(p["rows"]) % p["rpb"]
    return lift(p["cos"][pos], dt), lift(p["sin"][pos], dt)


def _ltx_w(p, name, dt, fault):
    r = torch.arange(p["rows"]) % p["w_rows"]
    if fault == "w_rows_ignored":
        r = r * 0
    return mod_of(p[name], r, dt)


def c_ltx_qk(p, dt, fault=None):
    out = {}
    for xn, wn, yn in (("x", "w", "y"), ("x2", "w2", "y2")):
        if p.get(xn) is None:
            continue
        x = lift(p[xn], dt)
        rstd = rsq(rsum(x * x) * recip(p["Dv"] or p["D"], x) + p["eps"])
        n = bf(x * rstd * _ltx_w(p, "w" if fault == "x2_with_w" else wn, dt, fault))
        if p.get("cos") is not None:
            cs, sn = _ltx_tables(p, dt)
            ne, no = pairs(n)
            n = bf(interleave(ne * cs + (-no) * sn, no * cs + ne * sn))
        out[yn] = n
    return out


def c_ltx_qk_bwd(p, dt, fault=None):
    out = {}
    for xn, wn, dyn, dxn in (("x", "w", "dy", "dx"), ("x2", "w2", "dy2", "dx2")):
        if p.get(xn) is None:
            continue
        x, dn = lift(p[xn], dt), lift(p[dyn], dt)
        if p.get("cos") is not None:
            cs, sn = _ltx_tables(p, dt)
            de, do = pairs(dn)
            dn = interleave(bf(bf(de * cs) + bf(do * sn)), bf(bf(do * cs) + (-bf(de * sn))))
        inv = recip(p["Dv"] or p["D"], x)
        rstd = rsq(rsum(x * x) * inv + p["eps"])
        g = dn * _ltx_w(p, "w" if fault == "x2_with_w" else wn, dt, fault)
        xh = x * rstd
        o = bf(rstd * (g - xh * (rsum(g * xh) * inv)))
        if fault == "grp_span_ignored" and p["row_grp"]:  # rows past the first group are written elsewhere: theirs keep the sentinel
            o = o.clone()
            o[p["row_grp"]:] = OUT_SENT
        out[dxn] = o
    return out


CONTRACT = {"wan_ln": c_wan_ln, "wan_ln_bwd": c_wan_ln_bwd, "wan_rms_rope": c_wan_rms_rope, "wan_rms_rope_bwd": c_wan_rms_rope_bwd, "wan_gate_res": c_wan_gate_res,
            "wan_gate_res_bwd": c_wan_gate_res_bwd, "wan_colsum": c_wan_colsum, "cog_ln_mod": c_cog_ln_mod, "cog_ln_mod_bwd": c_cog_ln_mod_bwd,
            "cog_head_ln": c_cog_head_ln, "cog_head_ln_bwd": c_cog_head_ln_bwd, "cog_gate_residual": c_cog_gate_residual, "ltx_nm": c_ltx_nm,
            "ltx_nm_bwd": c_ltx_nm_bwd, "ltx_qk": c_ltx_qk, "ltx_qk_bwd": c_ltx_qk_bwd}
EXACT = {("wan_gate_res", "y"), ("wan_gate_res_bwd", "dy"), ("cog_gate_residual", "y")}


def nc_wan(D):
    n = (D + 511) // 512
    return n if n <= 4 else (8 if n <= 8 else 10)


def nc_cog(D):
    n = (D + 511) // 512
    return n if n <= 4 else 8


def slabs(D):
    return [min(4096, D - c0) for c0 in range(0, D, 4096)]


# ----------------------------------------------------------------------------------------------------
# cases

WAN_D = [64, 512, 576, 1024, 1536, 2048, 2112, 4096, 4160, 5120]
COG_D = [64, 512, 576, 1536, 1920, 2112, 4096]
RMS_D = [128, 640, 1536, 2048, 3072, 4096]
COLSUM_D = WAN_D + [8960]
ROWS = [(rpb, B) for rpb in (1, 3, 31, 33, 75) for B in (1, 3)]
NC_TABLE = {"wan": {64: 1, 512: 1, 576: 2, 1024: 2, 1536: 3, 2048: 4, 2112: 8, 4096: 8, 4160: 10, 5120: 10},
            "cog": {64: 1, 512: 1, 576: 2, 1536: 3, 1920: 4, 2112: 8, 4096: 8}, "rms": {128: 1, 640: 2, 1536: 3, 2048: 4, 3072: 8, 4096: 8},
            "colsum": {4096: [8], 4160: [8, 1], 8960: [8, 8, 2]}}


def shapes(widths, fill):
    """(D, rpb, B): one row pair per width -- the narrowest width with the most rows, so that no output is a handful of elements --, the pairs left over at `fill`."""
    res = [(D, *ROWS[(3 * i + 9) % 10]) for i, D in enumerate(widths)]
    left = [r for r in ROWS if r not in [(a, b) for _, a, b in res]]
    return res + [(fill, *r) for r in left]


def _cases():
    cs = []

    def add(op, D, rpb, B, **kw):
        c = dict(op=op, D=D, rpb=rpb, B=B, seed=len(cs), cpu_only=False)
        c.update(kw)
        cs.append(c)

    for i, (D, rpb, B) in enumerate(shapes(WAN_D, 576)):
        add("wan_ln", D, rpb, B, affine=bool(i & 1), mod=bool(i & 2) or i % 4 == 0)
        add("wan_ln_bwd", D, rpb, B, affine=i % 3 == 1 or i % 5 == 4, mod=i % 3 != 1, dres=bool(i & 1), red1=i % 4 != 3, red2=i % 4 != 2, per_batch=i % 3 != 1 and i % 2 == 0)
        add("wan_rms_rope", D, rpb, B, head_dim=(128 if D % 128 == 0 else 64, 8, 64, 0)[i % 4])
        add("wan_rms_rope_bwd", D, rpb, B, head_dim=(64, 128 if D % 128 == 0 else 8, 0, 8)[i % 4], red2=i % 3 != 2)
        add("wan_gate_res", D, rpb, B, mod=i % 3 != 2)
        add("wan_gate_res_bwd", D, rpb, B, red1=i % 3 != 1, per_batch=bool(i & 1))
    for i, (D, rpb, B) in enumerate(shapes(COLSUM_D, 4160)):
        add("wan_colsum", D, rpb, B, per_batch=B == 1 and bool(i & 1))
    for i, (D, rpb, B) in enumerate(shapes(COG_D, 576)):
        segs = [0, 1, rpb - 1, rpb]
        add("cog_ln_mod", D, rpb, B, seg0=max(0, segs[i % 4]))
        add("cog_ln_mod_bwd", D, rpb, B, seg0=max(0, segs[(i + 1) % 4]), dres=bool(i & 1))
        add("cog_head_ln", D, rpb, B, seg0=max(0, segs[(i + 2) % 4]), rope=i % 3 != 2, head_dim=64, rms=0)
        add("cog_head_ln_bwd", D, rpb, B, seg0=max(0, segs[(i + 3) % 4]), rope=i % 3 != 1, head_dim=64, rms=0)
        add("cog_gate_residual", D, rpb, B, seg0=max(0, segs[i % 4]), dres=i % 3 != 0)
    for i, (D, rpb, B) in enumerate(shapes(RMS_D, 640)):
        segs = [0, 1, rpb - 1, rpb]
        add("cog_head_ln", D, rpb, B, seg0=max(0, segs[i % 4]), rope=i % 3 != 2, head_dim=128, rms=1)
        add("cog_head_ln_bwd", D, rpb, B, seg0=max(0, segs[(i + 1) % 4]), rope=i % 3 != 1, head_dim=128, rms=1)
    for i, (rpb, B) in enumerate(ROWS):
        Dv = (0, 32, 1024)[i % 3]
        add("ltx_nm", 2048, rpb, B, ln=i & 1, Dv=Dv)
        add("ltx_nm", 2048, rpb, B, ln=1 - (i & 1), Dv=(0, 32, 1024)[(i + 1) % 3])
        add("ltx_nm_bwd", 2048, rpb, B, ln=i & 1, Dv=Dv, dres=i % 3 != 0, gate2=i % 4 < 2)
        add("ltx_nm_bwd", 2048, rpb, B, ln=1 - (i & 1), Dv=(0, 32, 1024)[(i + 2) % 3], dres=i % 3 == 0, gate2=i % 4 >= 2)
        add("ltx_qk", 2048, rpb, B, rope=i % 3 != 1, w_rows=(1, 3)[i & 1], pair=i % 4 < 2, Dv=Dv)
        add("ltx_qk_bwd", 2048, rpb, B, rope=i % 3 != 2, w_rows=(3, 1)[i & 1], pair=i % 4 >= 2 or i == 9, row_grp=(0, 5)[(i // 2) % 2 if i != 9 else 1], Dv=(0, 32, 1024)[(i + 1) % 3])
    # the head_dim 128 hole (D = 192: a last head of 64 channels), refused by the library since this file: on the CPU only, for its seeded fault
    add("cog_head_ln", 192, 33, 1, seg0=0, rope=False, head_dim=128, rms=1, cpu_only=True)
    return cs


CASES = _cases()
GPU_CASES = [c for c in CASES if not c["cpu_only"]]


def case_id(c):
    skip = ("op", "seed", "cpu_only")
    return c["op"] + "-" + "-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in c.items() if k not in skip)


# ----------------------------------------------------------------------------------------------------
# inputs: logical CPU tensors (what the kernel is to see through its views)

def make(c):
    g = torch.Generator().manual_seed(9000 + c["seed"])
    op, D, rpb, B = c["op"], c["D"], c["rpb"], c["B"]
    rows = rpb * B
    p = dict(c, rows=rows, eps=EPS6)
    for k in ("dres", "red1", "red2", "gate2"):  # (case flags named like the tensor they ask for)
        p.pop(k, None)

    def rn(*shape, scale=1.0, shift=0.0, dtype=bf16):
        return (torch.randn(*shape, generator=g) * scale + shift).to(dtype)

    def data(width=D):
        x = torch.randn(rows, width, generator=g)
        if rows >= 3:
            x[1] += 30.0
            x[2] = 0.0
        return x.to(bf16)

    def tables(n, width):  # (cos, sin) fp32 [n, width // 2]
        ang = torch.rand(max(n, 1), width // 2, generator=g) * (2 * math.pi)
        return ang.cos().float(), ang.sin().float()

    def reds(per_batch):
        return rn(B, D, dtype=f32) if per_batch else rn(D, dtype=f32)

    if op == "wan_ln":
        p["x"] = data()
        if c["affine"]:
            p["w"], p["b"] = rn(D, scale=0.1, shift=1.0), rn(D, scale=0.1)
        if c["mod"]:
            p["scale"], p["shift"] = rn(B, D, scale=0.3, dtype=f32), rn(B, D, scale=0.3, dtype=f32)
    elif op == "wan_ln_bwd":
        p["x"], p["dy"] = data(), rn(rows, D)
        p["ld_x"] = D + 64
        if c["affine"]:
            p["w"] = rn(D, scale=0.1, shift=1.0)
        if c["mod"]:
            p["scale"] = rn(B, D, scale=0.3, dtype=f32)
        if c["dres"]:
            p["dres_buf"] = torch.full((rows + 1, D + 128), IN_SENT, dtype=bf16)
            p["dres_buf"][:rows, :D] = rn(rows, D)
            p["dres"] = p["dres_buf"][:rows, :D]
        if c["red1"]:
            p["red1"] = reds(c["per_batch"])
        if c["red2"]:
            p["red2"] = reds(c["per_batch"])
    elif op in ("wan_rms_rope", "wan_rms_rope_bwd"):
        p["x"], p["w"] = data(), rn(D, scale=0.1, shift=1.0)
        if c["head_dim"]:
            p["cos"], p["sin"] = tables(rpb, c["head_dim"])
        if op == "wan_rms_rope_bwd":
            p["dy"] = rn(rows, D)
            if c["red2"]:
                p["red2"] = reds(False)
    elif op == "wan_gate_res":
        p["x"], p["dy"] = data(), rn(rows, D)
        if c["mod"]:
            p["scale"] = rn(B, D, scale=0.3, dtype=f32)
    elif op == "wan_gate_res_bwd":
        p["x"], p["scale"] = data(), rn(B, D, scale=0.3, dtype=f32)
        if c["red1"]:
            p["dy"], p["red1"] = rn(rows, D), reds(c["per_batch"])
    elif op == "wan_colsum":
        p["x"], p["red1"] = data(), rn(1, D, dtype=f32) if c["per_batch"] else rn(D, dtype=f32)
    elif op.startswith("cog_"):
        nmod = B * 2 if c["seg0"] > 0 else B
        if op == "cog_ln_mod":
            p.update(x=data(), w=rn(D, scale=0.1, shift=1.0), b=rn(D, scale=0.1), onep=rn(nmod, D, scale=0.3, shift=1.0), shift=rn(nmod, D, scale=0.3), eps=EPS5)
        elif op == "cog_ln_mod_bwd":
            p.update(x=data(), dy=rn(rows, D), w=rn(D, scale=0.1, shift=1.0), onep=rn(nmod, D, scale=0.3, shift=1.0), eps=EPS5)
            if c["dres"]:
                p["dres"] = rn(rows, D)
        elif op == "cog_gate_residual":
            p.update(x=data(), onep=rn(nmod, D, scale=0.3))
            if c["dres"]:
                p["dres"] = rn(rows, D)
        else:
            HD = c["head_dim"]
            p.update(x=data(), w=rn(HD, scale=0.1, shift=1.0))
            if not c["rms"]:
                p["b"] = rn(HD, scale=0.1)
            if op == "cog_head_ln_bwd":
                p["dy"] = rn(rows, D)
            if c["rope"]:
                ang = torch.rand(max(rpb - c["seg0"], 1), HD // 2, generator=g) * (2 * math.pi)
                p["cos"], p["sin"] = ang.cos().float().repeat_interleave(2, 1), ang.sin().float().repeat_interleave(2, 1)
    else:  # LTX: a zero-padded narrow row has exact zeros past its valid width, in the data and in the incoming gradients
        Dv = c["Dv"] or D

        def padded(t):
            t[:, Dv:] = 0
            return t

        p["eps"] = EPS6 if op.startswith("ltx_nm") else EPS5
        if op == "ltx_nm":
            p.update(x=padded(data()), onep=rn(B, D, scale=0.3, shift=1.0), shift=rn(B, D, scale=0.3))
        elif op == "ltx_nm_bwd":
            p.update(x=padded(data()), dy=padded(rn(rows, D)), onep=rn(B, D, scale=0.3, shift=1.0))
            if c["dres"]:
                p["dres"] = padded(rn(rows, D))
            if c["gate2"]:
                p["gate2"] = rn(B, D, scale=0.3)
        else:
            names = (("x", "w", "dy"), ("x2", "w2", "dy2")) if c["pair"] else (("x", "w", "dy"),)
            for xn, wn, dyn in names:
                p[xn], p[wn] = padded(data()), padded(rn(c["w_rows"], D, scale=0.1, shift=1.0))
                if op == "ltx_qk_bwd":
                    p[dyn] = padded(rn(rows, D))
            if c["rope"]:
                p["cos"], p["sin"] = tables(rpb, D)
    return p


def reference(p):
    """name -> (reference value, bound), both fp64."""
    return {k: (v.v, v.e) for k, v in CONTRACT[p["op"]](p, f64).items()}


# ----------------------------------------------------------------------------------------------------
# the check

def block_shares(mism):
    """mism [M, N] bool -> list of (share, r0, r1, c0, c1) over blocks of 32 rows x 512 columns (ragged tails joined to their neighbour, see the docstring)."""
    M, N = mism.shape
    m = mism.double()
    re = list(range(0, M, 32)) + [M]
    if len(re) > 2 and re[-1] - re[-2] < 8:
        del re[-2]
    ce = list(range(0, N, 512)) + [N]
    if len(ce) > 2 and ce[-1] - ce[-2] < 512:
        del ce[-2]
    return [(m[r0:r1, c0:c1].mean().item(), r0, r1, c0, c1) for r0, r1 in zip(re[:-1], re[1:]) for c0, c1 in zip(ce[:-1], ce[1:])]


def judge(name, got, ref, bound, cap=CAP, blocks=True):
    """Asserts finite, |got - ref| <= bound everywhere and (bf16 outputs) the block mismatch cap.  Returns (max err / bound, max share)."""
    got = got.double().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output ({(~torch.isfinite(got)).sum().item()} entries)"
    err = (got - ref).abs()
    bad = err > bound
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = ratio.max().item() if ratio.numel() else 0.0
    share, blk = 0.0, (0, 0, 0, 0)
    if blocks and got.dim() == 2 and got.numel():
        share, *blk = max(block_shares(got != ref))
    print(f"[rowwise] {name:100s} max_err_over_bound={worst:.3f} max_block_mismatch={share:.4f}")
    if bad.any():
        i = [int(t[0]) for t in bad.nonzero(as_tuple=True)]
        raise AssertionError(f"{name}: element {i} got {got[tuple(i)].item():.6g} ref {ref[tuple(i)].item():.6g} bound {bound[tuple(i)].item():.3g}; "
                             f"{int(bad.sum())} elements over their bound")
    assert share <= cap, f"{name}: {share:.4f} of rows {blk[0]}..{blk[1] - 1} x columns {blk[2]}..{blk[3] - 1} differs from the reference (cap {cap})"
    return worst, share


def judge_case(tag, c, outs, R, cap=CAP):
    assert set(outs) == set(R), (sorted(outs), sorted(R))
    res = []
    for n, (ref, bound) in R.items():
        if (c["op"], n) in EXACT:
            bound = torch.zeros_like(bound)
        res.append(judge(f"{tag} {case_id(c)} {n}", outs[n], ref, bound, cap, blocks=not n.startswith("red")))
    return res


def stand_in(p, fault=None):
    outs = CONTRACT[p["op"]](p, f32, fault)
    if fault == "last_slot":
        nc = nc_wan(p["D"]) if p["op"].startswith("wan") else nc_cog(p["D"])
        for k, v in outs.items():
            if not k.startswith("red"):
                v[:, 512 * (nc - 1):] = OUT_SENT
    return outs


# ----------------------------------------------------------------------------------------------------
# GPU: launches.  Every strided operand is a view into a sentinel-filled backing tensor the test owns.

def _dev():
    return torch.device("cuda", 0)


class Bufs:
    def __init__(self, dev):
        self.dev, self.outs = dev, {}

    def inp(self, t, ld=None, fill=IN_SENT):
        """t [rows, D] -> device view of it inside [rows + 1, ld] (ld None: dense, no padding)."""
        if t is None:
            return None
        if ld is None:
            return t.contiguous().to(self.dev)
        b = torch.full((t.shape[0] + 1, ld), fill, dtype=t.dtype)
        b[:t.shape[0], :t.shape[1]] = t
        return b.to(self.dev)[:t.shape[0], :t.shape[1]]

    def out(self, name, rows, D, ld=None, nbuf=None):
        nbuf = (rows if nbuf is None else nbuf) + 1
        b = torch.full((nbuf, ld or D), OUT_SENT, dtype=bf16, device=self.dev)
        self.outs[name] = (b, rows, D)
        return b[:nbuf - 1, :D]

    def collect(self, rows_of=None):
        res = {}
        for name, (b, rows, D) in self.outs.items():
            h = b.cpu()
            nb = h.shape[0] - 1
            keep = torch.zeros(h.shape, dtype=torch.bool)
            idx = torch.arange(rows) if rows_of is None or nb == rows else rows_of
            keep[idx, :D] = True
            assert (h[~keep] == OUT_SENT).all(), f"{name}: padding overwritten"
            res[name] = h[idx, :D]
        return res


def _rc(rc, what):
    from finetrainers_amd import _lib

    _lib.check(rc, what)


def launch(p, dev=None, twice=True):
    """Runs the case's launcher (column sums: twice) and returns name -> CPU tensor; asserts the output padding intact."""
    import ctypes

    from finetrainers_amd import _lib, ops

    dev = dev or _dev()
    lib, ptr, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
    op, D, rows, rpb, B = p["op"], p["D"], p["rows"], p["rpb"], p["B"]
    bufs, ld = Bufs(dev), D + 64
    res = {}
    if op.startswith("wan_"):
        a = _lib.WanRowArgs()
        keep = []

        def I(name, ld_=ld):
            t = bufs.inp(p.get(name), ld_)
            keep.append(t)
            return t

        x = I("x")
        a.x, a.ld_x = ptr(x), x.stride(0)
        a.rows, a.D, a.rows_per_batch, a.eps = rows, D, rpb, p["eps"]
        for n in ("w", "b"):
            setattr(a, n, ptr(I(n, None)))
        for n in ("scale", "shift"):
            t = I(n)
            setattr(a, n, ptr(t))
            if t is not None:
                a.mod_bstride = t.stride(0)
        dy = I("dy")
        if dy is not None:
            a.dy, a.ld_dy = ptr(dy), dy.stride(0)
        ld_y = D + 128 if op in ("wan_ln_bwd", "wan_rms_rope_bwd") else ld
        if p.get("dres") is not None:
            a.dres = ptr(I("dres", ld_y))
        if p.get("cos") is not None:
            cos, sin = I("cos", None), I("sin", None)
            a.rope_cos, a.rope_sin, a.head_dim = ptr(cos), ptr(sin), p["head_dim"]
        oname = {"wan_ln": "y", "wan_ln_bwd": "dx", "wan_rms_rope": "y", "wan_rms_rope_bwd": "dx", "wan_gate_res": "y", "wan_gate_res_bwd": "dy"}.get(op)
        if oname:
            y = bufs.out(oname, rows, D, ld_y)
            a.y, a.ld_y = ptr(y), y.stride(0)
        rd = {}
        for n in ("red1", "red2"):
            if p.get(n) is not None:
                rd[n] = torch.full((p[n].numel() + 64,), OUT_SENT, dtype=f32)
                rd[n][:p[n].numel()] = p[n].flatten()
                rd[n] = rd[n].to(dev)
                setattr(a, n, ptr(rd[n]))
        a.red_per_batch = int(bool(p.get("per_batch")))
        fn = getattr(lib, "ftmi_" + {"wan_ln": "wan_ln_fwd", "wan_rms_rope": "wan_rms_rope_fwd", "wan_gate_res": "wan_gate_res_fwd"}.get(op, op))
        for _ in range(2 if twice else 1):
            _rc(fn(ctypes.byref(a), st), op)
        torch.cuda.synchronize()
        for n, t in rd.items():
            h = t.cpu()
            assert (h[p[n].numel():] == OUT_SENT).all(), f"{n}: padding overwritten"
            res[n] = h[:p[n].numel()].reshape(p[n].shape)
    elif op.startswith("cog_"):
        I = lambda name, ld_=None: bufs.inp(p.get(name), ld_)
        x = I("x", ld if "head" in op else None)
        if op == "cog_ln_mod":
            w, b, sh, on = I("w"), I("b"), I("shift"), I("onep")
            _rc(lib.ftmi_cog_ln_mod_fwd(ptr(x), ptr(w), ptr(b), ptr(sh), ptr(on), ptr(bufs.out("y", rows, D)), rows, D, rpb, p["seg0"], p["eps"], st), op)
        elif op == "cog_ln_mod_bwd":
            w, on, dy, dres = I("w"), I("onep"), I("dy"), I("dres")
            _rc(lib.ftmi_cog_ln_mod_bwd(ptr(x), ptr(w), ptr(on), ptr(dy), ptr(dres), ptr(bufs.out("dx", rows, D)), rows, D, rpb, p["seg0"], p["eps"], st), op)
        elif op == "cog_gate_residual":
            on, dres = I("onep"), I("dres")
            _rc(lib.ftmi_cog_gate_residual(ptr(dres), ptr(x), ptr(on), ptr(bufs.out("y", rows, D)), rows, D, rpb, p["seg0"], st), op)
        else:
            w, b, cos, sin, dy = I("w"), I("b"), I("cos"), I("sin"), I("dy", ld)
            if p["rms"]:  # HunyuanVideo's entries: own strides for every operand
                if op == "cog_head_ln":
                    y = bufs.out("y", rows, D, D + 128)
                    _rc(lib.ftmi_head_rms_rope_fwd(ptr(x), ld, ptr(w), ptr(y), y.stride(0), rows, D, 128, p["eps"], ptr(cos), ptr(sin), rpb, p["seg0"], st), op)
                else:
                    dx = bufs.out("dx", rows, D, D + 128)
                    _rc(lib.ftmi_head_rms_rope_bwd(ptr(x), ld, ptr(w), ptr(dy), ld, ptr(dx), dx.stride(0), rows, D, 128, p["eps"], ptr(cos), ptr(sin), rpb,
                                                   p["seg0"], st), op)
            elif op == "cog_head_ln":  # one row stride for x and y
                _rc(lib.ftmi_cog_head_ln_fwd(ptr(x), ld, ptr(w), ptr(b), ptr(bufs.out("y", rows, D, ld)), rows, D, p["eps"], ptr(cos), ptr(sin), rpb, p["seg0"], st), op)
            else:
                _rc(lib.ftmi_cog_head_ln_bwd(ptr(x), ld, ptr(w), ptr(dy), ptr(bufs.out("dx", rows, D, ld)), rows, D, p["eps"], ptr(cos), ptr(sin), rpb, p["seg0"], st), op)
        torch.cuda.synchronize()
    else:
        I = lambda name, ld_=None: bufs.inp(p.get(name), ld_)
        kw = dict(rows_per_batch=rpb, eps=p["eps"], valid_width=p["Dv"])
        rows_of = None
        if op == "ltx_nm":
            ops.norm_modulate_ex(I("x"), I("shift", ld), I("onep", ld), bufs.out("y", rows, D), layernorm=bool(p["ln"]), **kw)
        elif op == "ltx_nm_bwd":
            g2 = I("gate2", D + 128)
            ops.norm_modulate_bwd_ex(I("x"), I("dy"), I("onep", ld), bufs.out("dx", rows, D), layernorm=bool(p["ln"]), dres=I("dres"), gate2=g2,
                                     dx2=bufs.out("dx2", rows, D) if g2 is not None else None, **kw)
        elif op == "ltx_qk":
            pair = (I("x2", ld), I("w2"), bufs.out("y2", rows, D, D + 128)) if p["pair"] else None
            ops.qknorm_rope_ex(I("x", ld), I("w"), bufs.out("y", rows, D, D + 128), I("cos"), I("sin"), w_rows=p["w_rows"], pair=pair, **kw)
        else:
            grp, span = p["row_grp"], 7
            nbuf = rows
            if grp:
                rows_of = (torch.arange(rows) // grp) * span + torch.arange(rows) % grp
                nbuf = int(rows_of[-1]) + 1

            def G(name, ld_):  # the logical rows scattered to their group positions, sentinel rows between the groups
                t = p.get(name)
                if grp:
                    full = torch.full((nbuf, D), IN_SENT, dtype=bf16)
                    full[rows_of] = t
                    t = full
                return bufs.inp(t, ld_)

            pair = (G("x2", ld), I("w2"), G("dy2", D + 72), bufs.out("dx2", rows, D, D + 128, nbuf)) if p["pair"] else None
            ops.qknorm_rope_bwd_ex(G("x", ld), I("w"), G("dy", D + 72), bufs.out("dx", rows, D, D + 128, nbuf), I("cos"), I("sin"), rows=rows, w_rows=p["w_rows"], pair=pair,
                                   row_grp=grp, row_grp_span=span if grp else 0, **kw)
        torch.cuda.synchronize()
        res.update(bufs.collect(rows_of))
        return res
    res.update(bufs.collect())
    return res


def _run(c):
    _threads()
    p = make(c)
    R = reference(p)
    outs = launch(p)
    return judge_case("gpu", c, outs, R)


@pytest.mark.gpu
@pytest.mark.parametrize("c", GPU_CASES, ids=case_id)
def test_rowwise_contract(c):
    _run(c)


RSQ_PIVOTS = (-4, -1, 0, 2, 5, 9)


def _rsq_probe_rows():
    """Six blocks of 512 rows of width 512: row j of block i holds piv = 2^k_i at column j and t = piv m 2^s / 1024 (m in 128 .. 255, s in 0 .. 3) at the next
    column, so that red2[j] of wan_rms_rope_bwd with dy = e_j is piv rsqrtf(piv^2 (1 + (t / piv)^2) / 512 + eps), every other operation of the launch being
    exact (2^20 + (m 2^s)^2 < 2^24 is an integer).  Returns (D, [(piv, t [512] bf16)])."""
    g = torch.Generator().manual_seed(77)
    D, blocks = 512, []
    for k in RSQ_PIVOTS:
        m = torch.randint(128, 256, (D,), generator=g).double()
        s = torch.randint(0, 4, (D,), generator=g).double()
        piv = 2.0 ** k
        blocks.append((piv, (piv * m * 2.0 ** s / 1024).to(bf16)))
    return D, blocks


@pytest.mark.gpu
def test_rsqrtf_error_figure():
    """RSQ_REL against the hardware: the rstd of wan_rms_rope_bwd, read back exactly through its fp32 weight-gradient sum, against fp64."""
    import ctypes

    from finetrainers_amd import _lib

    D, blocks = _rsq_probe_rows()
    dev, worst, n = _dev(), 0.0, 0
    for piv, tb in blocks:
        j = torch.arange(D)
        n += D
        x = torch.zeros(D, D, dtype=bf16)
        x[j, j] = piv
        x[j, (j + 1) % D] = tb
        dy = torch.zeros(D, D, dtype=bf16)
        dy[j, j] = 1.0
        s2 = torch.tensor(piv * piv, dtype=f32) + tb.float() * tb.float()
        assert torch.equal(s2.double(), piv * piv + tb.double() ** 2)    # exact in fp32
        arg = (s2 / D + torch.tensor(EPS6, dtype=f32))                       # one fp32 rounding, the kernel's own
        a = _lib.WanRowArgs()
        xd, dyd, w = x.to(dev), dy.to(dev), torch.ones(D, dtype=bf16, device=dev)
        dx, red = torch.empty(D, D, dtype=bf16, device=dev), torch.zeros(D, dtype=f32, device=dev)
        a.x, a.ld_x, a.w, a.dy, a.ld_dy, a.y, a.ld_y, a.red2 = xd.data_ptr(), D, w.data_ptr(), dyd.data_ptr(), D, dx.data_ptr(), D, red.data_ptr()
        a.rows, a.D, a.rows_per_batch, a.eps = D, D, D, EPS6
        _lib.check(_lib.load().ftmi_wan_rms_rope_bwd(ctypes.byref(a), _lib.stream_ptr()), "probe")
        torch.cuda.synchronize()
        got = red.cpu().double() / piv
        ref = arg.double().rsqrt()
        worst = max(worst, ((got - ref).abs() / ref).max().item())
    print(f"[rowwise] rsqrtf over {n} arguments: largest relative error {worst:.4e} = {worst / U:.3f} u (RSQ_SEEN {RSQ_SEEN:.4e}, RSQ_REL {RSQ_REL:.4e})")
    assert worst <= RSQ_REL, f"rsqrtf relative error {worst:.3e} above the figure the bounds use ({RSQ_REL:.3e})"


def _refused(fn, code, what):
    from finetrainers_amd import _lib

    rc = fn()
    assert rc == code, f"{what}: returned {rc}, expected refusal {code} ({_lib.last_error()})"


@pytest.mark.gpu
def test_rowwise_refusals():
    """Bad launch descriptions come back as errors before any launch: every output keeps its sentinel."""
    import ctypes

    from finetrainers_amd import _lib

    lib, ptr, st, dev = _lib.load(), _lib.ptr, _lib.stream_ptr(), _dev()
    INV, UNS = _lib.FTMI_ERR_INVALID, _lib.FTMI_ERR_UNSUPPORTED
    big = torch.full((8, 8192), 1.0, dtype=bf16, device=dev)
    out = torch.full((8, 8192), OUT_SENT, dtype=bf16, device=dev)
    f = torch.full((8, 8192), 0.5, dtype=f32, device=dev)

    def wan(name, rows=4, D=512, rpb=2, ld=8192, **kw):
        a = _lib.WanRowArgs()
        a.x, a.ld_x, a.dy, a.ld_dy, a.y, a.ld_y, a.w, a.b = ptr(big), ld, ptr(big), ld, ptr(out), ld, ptr(big), ptr(big)
        a.scale, a.shift, a.mod_bstride, a.red1, a.red2 = ptr(f), ptr(f), 8192, ptr(f), ptr(f)
        a.rows, a.D, a.rows_per_batch, a.eps = rows, D, rpb, EPS6
        for k_, v_ in kw.items():
            setattr(a, k_, v_)
        return lambda: getattr(lib, "ftmi_wan_" + name)(ctypes.byref(a), st)

    for name in ("ln_fwd", "ln_bwd", "rms_rope_fwd", "rms_rope_bwd", "gate_res_fwd", "gate_res_bwd"):
        _refused(wan(name, D=96), UNS, f"wan {name} D = 96")
        _refused(wan(name, D=5184), UNS, f"wan {name} D = 5184")
        _refused(wan(name, ld=516), INV, f"wan {name} stride 516")
        _refused(wan(name, rows=5, rpb=2), INV, f"wan {name} rows 5 of samples of 2")
    _refused(wan("colsum", D=96), INV, "wan colsum D = 96")
    _refused(wan("colsum", ld=8196), INV, "wan colsum stride 8196")
    _refused(wan("colsum", rows=4, rpb=2, red_per_batch=1), UNS, "wan colsum per-sample sums of several samples")
    _refused(wan("rms_rope_fwd", rope_cos=ptr(f), rope_sin=ptr(f), head_dim=96), INV, "wan rope head_dim 96 at D = 512")

    p, o = ptr(big), ptr(out)
    for D, code, why in ((96, UNS, "D = 96"), (4160, UNS, "D = 4160")):
        _refused(lambda: lib.ftmi_cog_ln_mod_fwd(p, p, p, p, p, o, 4, D, 2, 0, EPS5, st), code, f"cog ln_mod {why}")
        _refused(lambda: lib.ftmi_cog_ln_mod_bwd(p, p, p, p, None, o, 4, D, 2, 0, EPS5, st), code, f"cog ln_mod_bwd {why}")
        _refused(lambda: lib.ftmi_cog_gate_residual(None, p, p, o, 4, D, 2, 0, st), code, f"cog gate_residual {why}")
        _refused(lambda: lib.ftmi_cog_head_ln_fwd(p, 8192, p, p, o, 4, D, EPS6, None, None, 2, 0, st), code, f"cog head_ln {why}")
        _refused(lambda: lib.ftmi_cog_head_ln_bwd(p, 8192, p, p, o, 4, D, EPS6, None, None, 2, 0, st), code, f"cog head_ln_bwd {why}")
    _refused(lambda: lib.ftmi_cog_ln_mod_fwd(p, p, p, p, p, o, 4, 512, 2, 3, EPS5, st), INV, "cog ln_mod seg0 3 of 2 rows")
    _refused(lambda: lib.ftmi_cog_gate_residual(None, p, p, o, 4, 512, 2, 3, st), INV, "cog gate_residual seg0 3 of 2 rows")
    _refused(lambda: lib.ftmi_cog_head_ln_fwd(p, 8192, p, p, o, 4, 512, EPS6, ptr(f), ptr(f), 2, 3, st), INV, "cog head_ln seg0 3 of 2 rows")
    _refused(lambda: lib.ftmi_cog_head_ln_fwd(p, 516, p, p, o, 4, 512, EPS6, None, None, 2, 0, st), INV, "cog head_ln stride 516")
    _refused(lambda: lib.ftmi_cog_head_ln_fwd(p, 256, p, p, o, 4, 512, EPS6, None, None, 2, 0, st), INV, "cog head_ln stride below D")
    for hd in (64, 96, 256):  # rms with anything but 128
        _refused(lambda: lib.ftmi_head_rms_rope_fwd(p, 8192, p, o, 8192, 4, 768, hd, EPS6, None, None, 4, 0, st), UNS, f"head rms head_dim {hd}")
        _refused(lambda: lib.ftmi_head_rms_rope_bwd(p, 8192, p, p, 8192, o, 8192, 4, 768, hd, EPS6, None, None, 4, 0, st), UNS, f"head rms bwd head_dim {hd}")
    for D in (192, 320, 4032):  # head_dim 128 needs whole heads
        _refused(lambda: lib.ftmi_head_rms_rope_fwd(p, 8192, p, o, 8192, 4, D, 128, EPS6, None, None, 4, 0, st), UNS, f"head rms D = {D}")
        _refused(lambda: lib.ftmi_head_rms_rope_bwd(p, 8192, p, p, 8192, o, 8192, 4, D, 128, EPS6, None, None, 4, 0, st), UNS, f"head rms bwd D = {D}")
    _refused(lambda: lib.ftmi_head_rms_rope_fwd(p, 8192, p, o, 256, 4, 512, 128, EPS6, None, None, 4, 0, st), INV, "head rms output stride below D")
    _refused(lambda: lib.ftmi_head_rms_rope_bwd(p, 8192, p, p, 256, o, 8192, 4, 512, 128, EPS6, None, None, 4, 0, st), INV, "head rms dy stride below D")
    _refused(lambda: lib.ftmi_head_rms_rope_bwd(p, 8192, p, p, 8192, o, 256, 4, 512, 128, EPS6, None, None, 4, 0, st), INV, "head rms dx stride below D")
    _refused(lambda: lib.ftmi_head_rms_rope_fwd(p, 8192, p, o, 8196, 4, 512, 128, EPS6, None, None, 4, 0, st), INV, "head rms output stride 8196")

    for D in (1024, 2112):
        _refused(lambda: lib.ftmi_norm_modulate_fwd_ex(p, p, p, 8192, o, 4, 2, D, EPS6, 0, 0, st), UNS, f"ltx norm_modulate D = {D}")
        _refused(lambda: lib.ftmi_norm_modulate_bwd_ex(p, p, p, 8192, None, o, 4, 2, D, EPS6, 0, None, 0, None, 0, st), UNS, f"ltx norm_modulate_bwd D = {D}")
        _refused(lambda: lib.ftmi_qknorm_rope_fwd_ex(p, 8192, p, None, None, o, 8192, 4, 2, D, EPS5, 1, None, None, None, 0, st), UNS, f"ltx qknorm_rope D = {D}")
        _refused(lambda: lib.ftmi_qknorm_rope_bwd_ex(p, 8192, p, None, None, p, 8192, o, 8192, 4, 2, D, EPS5, 1, None, None, None, None, 0, 0, 0, st), UNS,
                 f"ltx qknorm_rope_bwd D = {D}")
    _refused(lambda: lib.ftmi_qknorm_rope_fwd_ex(p, 8196, p, None, None, o, 8192, 4, 2, 2048, EPS5, 1, None, None, None, 0, st), INV, "ltx qknorm_rope stride 8196")
    _refused(lambda: lib.ftmi_qknorm_rope_bwd_ex(p, 8192, p, None, None, p, 8192, o, 8196, 4, 2, 2048, EPS5, 1, None, None, None, None, 0, 0, 0, st), INV,
             "ltx qknorm_rope_bwd stride 8196")
    _refused(lambda: lib.ftmi_qknorm_rope_fwd_ex(p, 8192, p, None, None, o, 8192, 4, 2, 2048, EPS5, 1, p, None, None, 0, st), INV, "ltx qknorm_rope half a pair")
    _refused(lambda: lib.ftmi_qknorm_rope_bwd_ex(p, 8192, p, None, None, p, 8192, o, 8192, 4, 2, 2048, EPS5, 1, None, None, None, None, 5, 3, 0, st), INV,
             "ltx qknorm_rope_bwd span below the group")
    _refused(lambda: lib.ftmi_norm_modulate_bwd_ex(p, p, p, 8192, None, o, 4, 2, 2048, EPS6, 0, p, 8192, None, 0, st), INV, "ltx norm_modulate_bwd gate2 without dx2")
    _refused(lambda: lib.ftmi_norm_modulate_fwd_ex(p, p, p, 8192, o, 4, 2, 2048, EPS6, 0, 2056, st), INV, "ltx valid width above D")
    # an empty launch is no error and launches nothing
    assert lib.ftmi_norm_modulate_fwd_ex(p, p, p, 8192, o, 0, 2, 2048, EPS6, 0, 0, st) == 0
    assert lib.ftmi_norm_modulate_bwd_ex(p, p, p, 8192, None, o, 0, 2, 2048, EPS6, 1, None, 0, None, 0, st) == 0
    assert lib.ftmi_qknorm_rope_fwd_ex(p, 8192, p, None, None, o, 8192, 0, 2, 2048, EPS5, 1, None, None, None, 0, st) == 0
    assert lib.ftmi_qknorm_rope_bwd_ex(p, 8192, p, None, None, p, 8192, o, 8192, 0, 2, 2048, EPS5, 1, None, None, None, None, 0, 0, 0, st) == 0
    assert wan("ln_fwd", rows=0)() == 0 and lib.ftmi_cog_gate_residual(None, p, p, o, 0, 512, 2, 0, st) == 0
    torch.cuda.synchronize()
    assert (out == OUT_SENT).all(), "a refused launch wrote its output"


# ----------------------------------------------------------------------------------------------------
# CPU self-checks

def test_fp32_stand_ins_pass_every_bound():
    """The contract in fp32 on the CPU (sums in slices, last to first) is inside every bound with at most 0.5 % per block, over every case."""
    _threads()
    worst = {}
    for c in CASES:
        p = make(c)
        # (TIES: the RMS norm_modulate_bwd has d = rstd g on a zero row, g of 8 significant bits and rstd = rsqrtf(fp32(1e-6)) = 1000 exactly in
        #  fp32 but 1000.0000015 in fp64: 2^-7 of such products sit on a bf16 tie, which fp32 rounds to even and the reference upwards; held to the 2 % cap)
        ties = c["op"] == "ltx_nm_bwd" and not c["ln"]
        for r_, s_ in judge_case("standin", c, stand_in(p), reference(p), cap=CAP if ties else STANDIN_CAP):
            w = worst.setdefault(c["op"], [0.0, 0.0])
            worst[c["op"]] = [max(w[0], r_), max(w[1], s_)]
    for op, (r_, s_) in worst.items():
        print(f"[rowwise] fp32 stand-in {op:20s} largest err/bound {r_:.3f} largest block mismatch share {s_:.4f}")


def has_red(c):
    return {"wan_colsum": True, "wan_ln_bwd": c.get("red1") or c.get("red2"), "wan_gate_res_bwd": c.get("red1"), "wan_rms_rope_bwd": c.get("red2")}.get(c["op"], False)


FAULTS = [  # (fault, the cases it can show in)
    ("last_slot", lambda c: c["op"] in ("wan_ln", "cog_ln_mod", "wan_gate_res_bwd", "cog_head_ln") and c["D"] > 512 and not c["cpu_only"]),
    ("mod_prev_sample", lambda c: c["B"] > 1 and (c.get("mod") or c["op"] in ("wan_gate_res_bwd", "cog_ln_mod", "cog_gate_residual", "ltx_nm", "ltx_nm_bwd"))),
    ("seg_swap", lambda c: c["op"] in ("cog_ln_mod", "cog_ln_mod_bwd", "cog_gate_residual") and 0 < c["seg0"] < c["rpb"]),
    ("rope_text_row", lambda c: c["op"].startswith("cog_head") and c["rope"] and c["seg0"] >= 1 and not c["cpu_only"]),
    ("rope_row_pos", lambda c: c["op"].startswith("cog_head") and c["rope"] and 1 <= c["seg0"] < c["rpb"] - 1),
    ("pair_from_column", lambda c: c["op"].startswith("wan_rms") and c["head_dim"] and c["D"] > c["head_dim"] and c["rpb"] > 1),
    ("dres_ld_x", lambda c: c["op"] == "wan_ln_bwd" and c["dres"] and c["rpb"] * c["B"] > 1),
    ("strip_tail", lambda c: has_red(c) and c["rpb"] % 32),
    ("store_not_add", has_red),
    ("all_in_row0", lambda c: c["op"] in ("wan_ln_bwd", "wan_gate_res_bwd") and c["per_batch"] and c["B"] > 1 and has_red(c)),
    ("slab_offset", lambda c: c["op"] == "wan_colsum" and c["D"] == 8960),
    ("n_unrounded", lambda c: (c["op"].startswith("wan_rms") and c["head_dim"]) or (c["op"] == "cog_head_ln" and c["rope"] and c["seg0"] < c["rpb"])),
    ("dx2_unrounded", lambda c: c["op"] == "ltx_nm_bwd" and c["gate2"]),
    ("dyonep_unrounded", lambda c: c["op"] in ("cog_ln_mod_bwd", "ltx_nm_bwd")),
    ("mean_over_D", lambda c: c["op"] in ("ltx_nm", "ltx_nm_bwd") and c["Dv"]),
    ("pad_nonzero", lambda c: c["op"] in ("ltx_nm", "ltx_nm_bwd") and c["Dv"] and c["ln"]),
    ("w_rows_ignored", lambda c: c["op"] in ("ltx_qk", "ltx_qk_bwd") and c["w_rows"] > 1 and c["rpb"] * c["B"] > 1),
    ("x2_with_w", lambda c: c["op"] in ("ltx_qk", "ltx_qk_bwd") and c["pair"]),
    ("grp_span_ignored", lambda c: c["op"] == "ltx_qk_bwd" and c["row_grp"] and c["rpb"] * c["B"] > c["row_grp"]),
    ("half_head_128", lambda c: c["cpu_only"]),
]


def _fails(c, fault):
    p = make(c)
    try:
        judge_case(f"fault {fault}", c, stand_in(p, fault), reference(p))
    except AssertionError:
        return True
    return False


def test_seeded_faults_fail():
    """Each fault of the docstring's table, applied to the fp32 stand-in, is rejected in EVERY launcher it can occur in (by at least one of that launcher's cases);
    the clean stand-in of the same cases passes (test_fp32_stand_ins_pass_every_bound)."""
    _threads()
    for fault, pred in FAULTS:
        by_op = {}
        for c in CASES:
            if pred(c):
                by_op.setdefault(c["op"] + ("-rms" if c.get("rms") else ""), []).append(c)
        assert by_op, f"no case carries the fields the fault {fault} needs"
        for op, cs in by_op.items():
            assert any(_fails(c, fault) for c in cs[:6]), f"the seeded fault {fault} passes every case of {op}"


def test_the_cases_reach_every_instantiation():
    """NC as the two dispatch macros compute it, against the docstring's table; every (launcher, NC) pair of every kernel template has a case, and every row pair."""
    for D, nc in NC_TABLE["wan"].items():
        assert nc_wan(D) == nc, (D, nc_wan(D))
    for fam in ("cog", "rms"):
        for D, nc in NC_TABLE[fam].items():
            assert nc_cog(D) == nc, (D, nc_cog(D))
    for D, ncs in NC_TABLE["colsum"].items():
        assert [nc_wan(w) for w in slabs(D)] == ncs, (D, slabs(D))
    reach = {}
    for c in GPU_CASES:
        key = c["op"] + ("-rms" if c.get("rms") else "")
        ncs = [nc_wan(w) for w in slabs(c["D"])] if c["op"] == "wan_colsum" else [nc_wan(c["D"]) if c["op"].startswith("wan") else nc_cog(c["D"])]
        reach.setdefault(key, set()).update(ncs)
        reach.setdefault(key + " rows", set()).add((c["rpb"], c["B"]))
    for key, got in reach.items():
        if key.endswith(" rows"):
            assert got == set(ROWS), (key, sorted(set(ROWS) - got))
        elif key.startswith("wan"):  # (colsum_kernel<10> cannot be reached: a slab is at most 4096 columns wide)
            assert got == ({1, 2, 3, 4, 8} if key == "wan_colsum" else {1, 2, 3, 4, 8, 10}), (key, got)
        elif key.startswith("cog"):
            assert got == {1, 2, 3, 4, 8}, (key, got)
    assert {k for k in reach if not k.endswith(" rows")} == set(CONTRACT) | {"cog_head_ln-rms", "cog_head_ln_bwd-rms"}
    # optional arguments both ways, the segment boundaries, the LTX arguments
    def both(op, key, vals=(False, True)):
        got = {type(vals[0])(c[key]) for c in GPU_CASES if c["op"] == op}
        assert got >= set(vals), (op, key, got)

    for op, key in (("wan_ln", "affine"), ("wan_ln", "mod"), ("wan_ln_bwd", "affine"), ("wan_ln_bwd", "mod"), ("wan_ln_bwd", "dres"), ("wan_ln_bwd", "red1"),
                    ("wan_ln_bwd", "red2"), ("wan_ln_bwd", "per_batch"), ("wan_rms_rope_bwd", "red2"), ("wan_gate_res", "mod"), ("wan_gate_res_bwd", "red1"),
                    ("wan_gate_res_bwd", "per_batch"), ("wan_colsum", "per_batch"), ("cog_ln_mod_bwd", "dres"), ("cog_head_ln", "rope"), ("cog_head_ln_bwd", "rope"),
                    ("cog_gate_residual", "dres"), ("ltx_nm_bwd", "dres"), ("ltx_nm_bwd", "gate2"), ("ltx_qk", "rope"), ("ltx_qk", "pair"), ("ltx_qk_bwd", "rope"),
                    ("ltx_qk_bwd", "pair")):
        both(op, key)
    for op in ("wan_rms_rope", "wan_rms_rope_bwd"):
        both(op, "head_dim", (0, 8, 64, 128))
    for op in ("ltx_nm", "ltx_nm_bwd", "ltx_qk", "ltx_qk_bwd"):
        both(op, "Dv", (0, 32, 1024))
    for op in ("ltx_nm", "ltx_nm_bwd"):
        both(op, "ln", (0, 1))
    both("ltx_qk", "w_rows", (1, 3))
    both("ltx_qk_bwd", "w_rows", (1, 3))
    both("ltx_qk_bwd", "row_grp", (0, 5))
    for op in ("cog_ln_mod", "cog_ln_mod_bwd", "cog_head_ln", "cog_head_ln_bwd", "cog_gate_residual"):
        kinds = {("0" if c["seg0"] == 0 else "1" if c["seg0"] == 1 and c["rpb"] > 2 else "last" if c["seg0"] == c["rpb"] - 1 else "all" if c["seg0"] == c["rpb"] else "?")
                 for c in GPU_CASES if c["op"] == op and c["rpb"] > 2}
        assert kinds >= {"0", "1", "last", "all"}, (op, kinds)


def test_the_rsqrt_probe_is_exact_on_the_host():
    """The probe rows of test_rsqrtf_error_figure: every sum of the probe is exact in fp32, and the arguments span the rstd arguments of the cases (eps alone,
    2^-20, up to the mean square of a row with offset 30, about 2^10)."""
    D, blocks = _rsq_probe_rows()
    lo, hi = math.inf, 0.0
    for piv, t in blocks:
        assert torch.equal(t.double() * 1024 / piv, (t.double() * 1024 / piv).round())
        s2 = piv * piv + t.double() ** 2
        assert torch.equal(s2.float().double(), s2)
        lo, hi = min(lo, (s2 / D).min().item()), max(hi, (s2 / D).max().item())
    assert lo < 2.0**-16 and hi > 2.0**10, (lo, hi)
