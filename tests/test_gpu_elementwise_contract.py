"""The launch contract of the loss, optimiser and data-preparation kernels (second half of csrc/rowwise.hip) per element against fp64.

CONTRACT (read from the kernels; bf() = round to nearest even to bf16, everything else one fp32 operation per sign, -ffp-contract=off, no fast-math)
  EXACT class: every operation is IEEE, the reference is the fp64 expression rounded to fp32 after each operation, the comparison is bitwise.
    noise_pack        x0 = bf(((lat - mean_c) * 1) / std_c);  x_t = bf((1 - t) x0 + t n) (two products, one sum);  target = bf(n - x0);  t = sigma_first_b for
                      tokens < first_frame_tokens when sigma_first is given, else sigma_b;  [B, C, S] -> [B, S, C], 64 x 64 tiles
    ddim_mix          add_noise: x0 = bf(lat * scale), noisy = bf(bf(sa_b x0) + bf(so_b noise));  get_velocity: out = bf(bf(sa_b noise) - bf(so_b sample))
    clip_scale        norm = sqrtf(*sumsq) (written to grad_norm_out); coef = max_norm / (norm + 1e-6f); g *= coef only when coef < 1 and max_norm > 0
    adamw_bf16        host scalars in double from the fp32 arguments, cast to fp32: decay = 1 - lr wd, w1 = 1 - beta1, omb2 = 1 - beta2, step = -(lr / (1 - beta1^t)),
                      bc2s = sqrt(1 - beta2^t).  coef = min(max_norm / (sqrtf(*sumsq) + 1e-6f), 1), 1 when sumsq is NULL or max_norm <= 0.  gi = bf(g), and
                      gi = bf(gi coef) only when coef < 1;  p' = bf(p decay);  m = bf(w1 < 0.5 ? m + w1 (gi - m) : gi - (gi - m)(1 - w1));  v' = bf(v beta2);
                      v = bf(v' + (omb2 gi) gi);  d = bf(sqrtf(v)); d = bf(d / bc2s); d = bf(d + eps);  p = bf(p' + step (m / d))
    lora_split        hi = bf(w), lo = bf(w - hi);  sp [2 rows, cols]: hi at row (r // 32) 64 + r % 32, lo 32 rows below;  ext [rows, 3 cols] = [hi | hi | lo];
                      t_sp [2 cols, rows], t_ext [cols, 3 rows]: the same of w^T.  ftmi_lora_refresh_n: A [L, n, r, D] -> a_sp = sp, at_ext = t_ext per adapter,
                      at_qkv_ext [L, D, 9 r]: t_ext of adapters 0, 1, 2 side by side (inner_n = 3);  B [L, n, D, r] -> b_ext = ext, bt_sp = t_sp
    transpose_bf16    out [cols, rows] = in^T
    ada_prep          slots 0..5 = bf(table[l, i] + temb[b, i]); slot 6 = bf(1 + slot 1); slot 7 = bf(1 + slot 4);  ada [L, B, 8, D]
    ada_out_prep      shift = bf(table2[0] + emb_b); scale = bf(table2[1] + emb_b); third = bf(1 + scale);  [B, 3, D]
  BOUNDED class (value type V: fp64 value + bound on an fp32 evaluation)
    mse_loss          loss = sum over workgroups of (partial * inv_count), partial = sum w_b (d d), d = pred - target, inv_count = 1 / (per_sample * B);
                      dpred = bf((w_b (2 d)) (inv_count grad_scale)) is of the EXACT class (four IEEE operations per element; with B = 3 and a power-of-two
                      per_sample a third of the fp32 products are dyadic and many sit on bf16 ties, which only the operation-by-operation reference follows)
    sumsq             scratch[0] = sum g^2, any order
    adamw (fp32)      coef as clip_scale (uniform scalars are exact class) but min(coef, 1);  gi = g coef;  p' = p (1 - lr wd);  m = m + (gi - m)(1 - beta1);
                      v = v beta2 + ((1 - beta2) gi) gi;  p = p' - (lr / bc1)(m / (sqrtf(v) / bc2s + eps));  bc1, bc2s fp64 from the fp32 betas, allowed 4 u
    small_linear      y = bf(sum_k xin W + bias), xin = silu_in ? bf(x / (1 + __expf(-x))) : x
    timestep_sinusoid out[b, j] = bf(cosf(t_b f_j)), out[b, 128 + j] = bf(sinf(t_b f_j)), f_j = expf((-9.2103403f j) / 128)
    posterior_sample  out = bf(mean + bf(bf(expf(bf(0.5 clamp(logvar, -30, 20)))) eps)): exact apart from its one expf
  ZERO SIZES  return 0 without a launch: noise_pack (B, C or S), ddim (per_sample), clip_by_sumsq, clip_adamw_step, adamw_bf16_step (n), lora_split /
              lora_refresh_n (rows, cols, L), transpose_bf16, the four time-embedding entry points.  Refused (FTMI_ERR_INVALID): mse_loss (B or per_sample),
              posterior_sample (B or per_sample), ddim (B), grad_sumsq and clip_grad_norm (n).

REFERENCE: the table above in fp64 (torch, CPU), one function per launcher (c_*); the same functions run on fp32 tensors as the stand-in of the CPU self-checks.

BOUNDS (u = 2^-24; rules of tests/test_gpu_rowwise_contract.py, plus 2^-150 per operation for results in the subnormal range)
  a + b, a - b, a * b, a / b   propagated error + u (|result| + that error);   sqrtf: the interval's image + u;   bf(v): e + ulp_bf(|v| + e)
  sum of n terms, any order    sum of the terms' errors + (n + 2) u sum(|term| + error)
  transcendentals: nothing under the ROCm installation (headers, documents) states an error figure for HIP's expf / cosf / sinf / __expf (the only ulp table,
  lib/llvm/lib/clang/*/include/opencl-c.h, is about OpenCL's half_ / native_ functions), so measured by test_transcendental_error_figures: a sweep of >= 2^18
  arguments per function through the kernel that uses it; for every output that differs from bf(reference) the relative distance of the fp64 value to the nearest
  bf16 rounding boundary is a lower bound on the function's error there; the largest is T_SEEN and the bounds use T_REL = 2 max(T_SEEN, u):
  an fp32 result is itself rounded to fp32, and a sweep that meets no flipped output cannot show less than that u.
    expf   posterior_sample (mean 0, eps 1: out = bf(expf(h))), every bf16 h in [-15, 10], four times over
    cosf / sinf   timestep_sinusoid columns 0 and 128 (f_0 = expf(0) = 1: the argument is t itself), 2^18 values of t in [0, 1000]
    silu   small_linear with a one-hot weight (y = bf(silu(x))), every bf16 x in [-20, 20], eight times over; __expf(y) is exp2 of the fp32 product y log2(e), whose
           rounding alone moves the result by |y| u, so the model is T_SILU (1 + |x|) |silu(x)| and the sweep records distance / (1 + |x|)
  In timestep_sinusoid the error of the argument t f_j (f_j known to T_EXP) goes through V: |d cos|, |d sin| <= 1.
  Asserted per case: every output finite; |got - ref| <= bound per element (bitwise for the exact class); for a bounded bf16 output at most 2 % of any block of
  4096 consecutive elements differ from the reference at all (a shorter tail joins the block before it); every output and every tensor updated in place sits
  between sentinel padding, intact after the launch; inputs sit between padding that wrecks the result if read; every launch runs twice on the same scratch
  and returns the same bits.

CASES
  noise_pack    C x S over {1, 63, 64, 65, 128} x {1, 63, 64, 65, 200}, B in {1, 3}, first_frame_tokens in {0, 1, 70, S, S + 5}, sigma_first given / NULL
  ddim, posterior   per_sample in {8, 2040, 2048, 2056, 2097152, 2097160, 4196704} x B in {1, 3}; x0 present / absent; log-variances -40 .. 30 with -30, 20, +-0
  mse_loss      per_sample in {8, 2040, 2048, 2056, 524288, 524296, 1050976} x B in {1, 3} x weight x dpred x grad_scale {1, 1/4}; sample 1 (B = 3) weighs 64
  sumsq         n in {1, 3, 4, 5, 6, 1024, 1027, 2097152, 2097155, 4195335}: powers of two at the probe positions (exact), and Gaussian
  clip, adamw, adamw_bf16   n in {1, 255, 256, 257, 1048576, 1048577, 2097229} with one setting each; at n = 257 step {1, 2, 1000} x betas x clip active /
                inactive / disabled (max_norm 0), zero gradient, beta1 0.4 (bf16: the other lerp branch).  Data: p = 0 on elements 16..47, gradients of 3e-20
                (g^2 subnormal) and 1e-30 (g^2 = 0) on elements 48..79, moments non-zero.
  lora_split, transpose   (1, 1) (31, 33) (33, 31) (32, 32) (64, 96) (1, 4097) (4097, 1); planes: rows, cols in {32, 64, 96}; refresh_n L = 2, n in {3, 4, 8}, r = 32,
                D = 64.  The entry points fix ld_ext = 3 cols and ld_t_ext = 3 rows (9 r in at_qkv_ext, where the three adapters interleave within a row), so the
                rows are dense and the padding lies before and after each output; values: w - hi subnormal on every 7th element, lo = 0 on the next
  sinusoid B {1, 3, 8}, t in {0, 0.5, 1, 999, 1000}; small_linear: ten (rows, N, K) triples that cover rows 1..8, N {1, 4, 5, 2048} and K {8, 256, 512, 520,
                2048} (SL_CASES), each with and without silu_in and bias; ada_prep L {1, 3} x B {1, 3} x D {64, 2048}; ada_out_prep B x D

CPU SELF-CHECKS: the fp32 stand-ins pass every bound (bitwise for the exact class, at most 0.5 % per block otherwise); each seeded fault below, applied to the
stand-in, is rejected by at least one case; the grids computed from the cases reach one workgroup, exactly the cap and beyond it for every capped launcher, every
small_linear template and every sumsq tail length.
  tail_dropped / last_wg_dropped / second_pass_dropped   sumsq's n % 4 tail; the last workgroup's partial (sumsq, mse); the grid-stride pass (every capped kernel)
  partial_unscaled / finish_store        mse: inv_count missing; the finish keeps the last partial only
  prev_sample          sigma (noise_pack), weight (mse), coefficients (ddim) of sample b - 1
  fft_le               first_frame_tokens compared with <=
  unrounded            a rounding point removed: x0 of noise_pack, bf(sa x0) of ddim, bf(g) of adamw_bf16, bf(silu) of small_linear
  lerp_ignored / coef_ge1 / maxnorm0_clips   adamw_bf16: the w1 >= 0.5 branch; coef applied when >= 1; max_norm <= 0 not treated as "no clip" (the defect fixed here)
  bc_powf              fp32 adamw: bias corrections as 1 - powf(beta, step) in fp32 (the launcher before this test; seen at step 2, beta2 = 0.999 on the p = 0 stretch)
  lo_is_hi / ext_off_cols / inner_ignored   lora_split
  slot6_from_slot0 / bias_dropped        ada_prep, small_linear

MEASURED on an MI355X (largest |got - ref| / bound and largest block mismatch share over the cases of each launcher; "exact": no element differs)
  launcher (outputs)                            err / bound   block share     fp32 stand-in on the CPU: err / bound, block share
  noise_pack (x_t, target)                      exact         0               exact
  ddim add_noise (x0, noisy), get_velocity      exact         0               exact
  posterior_sample                              0.000         0               0.000, 0         (no output differs from bf(fp64))
  mse_loss: loss                                0.045         -               0.045
            dpred                               exact         0               exact
  grad_sumsq: probes                            exact         -               exact
              Gaussian                          0.210         -               0.229
  clip_grad_norm, clip_adamw_step: their sumsq  0.092         -               -
  clip_by_sumsq, clip_grad_norm (g, norm)       exact         -               exact
  clip_adamw_step (p, m, v)                     0.964 0.948 0.988   -         0.841            (norm exact)
  adamw_bf16_step (p, m, v, norm)               exact         0               exact
  lora_split, lora_refresh_n (every layout)     exact         0               exact
  transpose_bf16                                exact         0               exact
  ada_prep, ada_out_prep                        exact         0               exact
  small_linear                                  0.332         0.0005          0.984, 0.0007
  timestep_sinusoid                             0.208         0.0010          0.208, 0.0010
  T_SEEN over 2^18 arguments each: expf 0 (no flipped output), cosf 0 (none), sinf 4.1857e-08 = 0.70 u (3 flipped outputs), silu 0 (none): T_REL = 2 u for all
  four.  Every case is within its bounds; the zero-size and refusal calls return as stated above with every sentinel intact.
"""

import math

import pytest
import torch

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0**-24
TINY = 2.0**-150
CAP, STANDIN_CAP = 0.02, 0.005
IN_SENT = 3.0e4     # padding of the inputs: wrecks the result if read as data
OUT_SENT = -1536.0  # padding of the outputs (exact in bf16 and fp32): must survive the launch
PAD = 64            # elements of padding on either side (keeps the 16-byte alignment)
# largest error seen by test_transcendental_error_figures on an MI355X (relative; silu: relative / (1 + |x|)).  The bounds use twice these, and never less than
# 2 u: the result of an fp32 function is itself rounded to fp32, which a sweep that meets no flipped output cannot show
T_SEEN = {"expf": 0.0, "cosf": 0.0, "sinf": 4.1857e-08, "silu": 0.0}
T_REL = {k: 2.0 * max(v, U) for k, v in T_SEEN.items()}


def _threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))


def f32v(x):
    """The fp32 value of a Python number, as the C entry point receives it."""
    return float(torch.tensor(x, dtype=f32))


# ----------------------------------------------------------------------------------------------------
# the value type of the bounded class (tests/test_gpu_rowwise_contract.py's V with a subnormal floor, a division and a square root)

def ulp_bf(a):
    _, e = torch.frexp(a)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - 8).clamp_min(2.0**-133), torch.zeros_like(a))


def bfr(t):
    """Round to nearest even to bf16, kept in t's dtype (fp64: in one rounding, not through fp32)."""
    if t.dtype != f64:
        return t.float().to(bf16).to(t.dtype)
    u = ulp_bf(t.abs()).clamp_min(2.0**-133)
    return torch.round(t / u) * u  # t / u is exact (a power of two) and torch.round rounds halves to even


class V:
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v if torch.is_tensor(v) and v.dtype == f64 else torch.as_tensor(v, dtype=f64)
        self.e = torch.zeros_like(self.v) if e is None else torch.as_tensor(e, dtype=f64)

    @staticmethod
    def of(o):
        return o if isinstance(o, V) else V(o)

    @staticmethod
    def _done(v, e):
        return V(v, e + U * (v.abs() + e) + TINY)

    def __add__(self, o):
        o = V.of(o)
        return V._done(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V._done(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        return V._done(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        lo = o.v.abs() - o.e
        assert (lo > 0).all(), "divisor not known well enough"
        v = self.v / o.v
        return V._done(v, (self.e + v.abs() * o.e) / lo)


def isV(x):
    return isinstance(x, V)


def lift(t, dt):
    return V(t.double()) if dt is f64 else t.float()


def sc(x, dt, rel=0.0):
    """A uniform fp32 scalar (known to rel * |x|)."""
    return V(torch.tensor(x, dtype=f64), torch.tensor(abs(x) * rel, dtype=f64)) if dt is f64 else torch.tensor(x, dtype=f32)


def S(fn, *xs):
    if isV(xs[0]):
        return V(fn(*[x.v for x in xs]), fn(*[x.e for x in xs]))
    return fn(*xs)


def bf(x):
    if isV(x):
        return V(bfr(x.v), x.e + ulp_bf(x.v.abs() + x.e))
    return bfr(x)


def vsum(x):
    """Sum of all terms, any order (fp32 stand-in: torch's pairwise sum)."""
    if isV(x):
        n = x.v.numel()
        return V(x.v.sum(), x.e.sum() + (n + 2) * U * (x.v.abs() + x.e).sum() + TINY)
    return x.sum()


def vsum_last(x):
    if isV(x):
        n = x.v.shape[-1]
        return V(x.v.sum(-1), x.e.sum(-1) + (n + 2) * U * (x.v.abs() + x.e).sum(-1) + TINY)
    return x.sum(-1)


def vsqrt(x):
    if isV(x):
        v = x.v.sqrt()
        return V(v, (x.v + x.e).sqrt() - (x.v - x.e).clamp_min(0).sqrt() + U * (x.v + x.e).sqrt() + TINY)
    return x.sqrt()


def vfun(name, x):
    """expf / cosf / sinf of a value known to x.e (|derivative| <= |value| for exp, <= 1 for cos and sin)."""
    fn = {"expf": torch.exp, "cosf": torch.cos, "sinf": torch.sin}[name]
    if isV(x):
        v = fn(x.v)
        slope = (x.v + x.e).exp() if name == "expf" else torch.ones_like(v)
        return V(v, slope * x.e + T_REL[name] * v.abs() + TINY)
    return fn(x)


def vsilu(x):
    """x / (1 + __expf(-x)) of an exact x."""
    if isV(x):
        v = x.v / (1.0 + (-x.v).exp())
        return V(v, T_REL["silu"] * (1.0 + x.v.abs()) * v.abs() + TINY)
    return x / (1.0 + torch.exp(-x))


# the exact class works on plain tensors: X(dt) gives (lift, r) with r the rounding to fp32 after one operation (identity on fp32 tensors)
def X(dt):
    if dt is f64:
        return (lambda t: t.double()), (lambda t: t.float().double())
    return (lambda t: t.float()), (lambda t: t)


def prev_sample(B):
    return (torch.arange(B) - 1) % B


# ----------------------------------------------------------------------------------------------------
# the contract, one function per launcher: p = inputs and launch fields, dt = f64 (reference) or f32 (stand-in), fault = a seeded fault

def c_noise_pack(p, dt, fault=None):
    L, r = X(dt)
    lat, nz = L(p["lat"]), L(p["noise"])  # [B, C, S]
    B, C, Sn = lat.shape
    mean, std = L(p["mean"])[None, :, None], L(p["std"])[None, :, None]
    x0 = r(r(r(lat - mean) * 1.0) / std)
    if fault != "unrounded":
        x0 = bfr(x0)
    sg = L(p["sigma"])
    sgf = L(p["sigma_first"]) if p.get("sigma_first") is not None else sg
    if fault == "prev_sample":
        sg, sgf = sg[prev_sample(B)], sgf[prev_sample(B)]
    s = torch.arange(Sn)
    first = (s <= p["fft"]) if fault == "fft_le" else (s < p["fft"])
    t = torch.where(first[None, None, :], sgf[:, None, None], sg[:, None, None])
    xt = bfr(r(r(r(1.0 - t) * x0) + r(t * nz)))
    tg = bfr(r(nz - x0))
    return {"xt": xt.transpose(1, 2).contiguous(), "target": tg.transpose(1, 2).contiguous()}


def _second_pass(x, cap_elems, fault, keep):
    """fault second_pass_dropped: the elements beyond one grid pass keep `keep`."""
    if fault == "second_pass_dropped" and x.shape[-1] > cap_elems:
        x = x.clone()
        x[..., cap_elems:] = keep[..., cap_elems:] if torch.is_tensor(keep) else keep
    return x


def c_ddim(p, dt, fault=None):
    L, r = X(dt)
    a, b = L(p["a"]), L(p["b"])  # [B, per]
    ca, co = L(p["sa"])[:, None], L(p["so"])[:, None]
    if fault == "prev_sample":
        ca, co = ca[prev_sample(a.shape[0])], co[prev_sample(a.shape[0])]
    rb = (lambda t: t) if fault == "unrounded" else bfr
    out = {}
    if p["mode"] == 0:
        x0 = bfr(r(a * p["scale"]))
        o = bfr(r(rb(r(ca * x0)) + bfr(r(co * b))))
        if p["want_x0"]:
            out["x0"] = _second_pass(x0, 1024 * 2048, fault, OUT_SENT)
    else:
        o = bfr(r(rb(r(ca * b)) - bfr(r(co * a))))
    out["out"] = _second_pass(o, 1024 * 2048, fault, OUT_SENT)
    return out


def c_posterior(p, dt, fault=None):
    mom, ev = lift(p["moments"], dt), lift(p["eps"], dt)  # [B, 2, half], [B, half]
    mv, lv = S(lambda t: t[:, 0], mom), S(lambda t: t[:, 1], mom)
    if fault == "prev_sample":
        lv = S(lambda t: t[prev_sample(t.shape[0])], lv)
    h = S(lambda t: bfr(0.5 * t.clamp(-30.0, 20.0)), lv)  # exact: a clamp and a halving
    if isV(h):
        h = V(h.v)
    sd = bf(vfun("expf", h))
    o = bf(mv + bf(sd * ev))
    return {"out": o if isV(o) else _second_pass(o, 1024 * 2048, fault, OUT_SENT)}


def mse_blocks(per):
    return min((per // 8 + 255) // 256, 256)


def c_mse(p, dt, fault=None):
    pr, tg = lift(p["pred"], dt), lift(p["target"], dt)  # [B, per]
    B, per = p["pred"].shape
    w = p["weight"] if p.get("weight") is not None else torch.ones(B)
    if fault == "prev_sample":
        w = w[prev_sample(B)]
    w = lift(w, dt)
    w = S(lambda t: t[:, None], w)
    inv = f32v(1.0 / f32v(float(per) * float(B)))
    d = pr - tg
    terms = w * (d * d)
    if fault in ("last_wg_dropped", "second_pass_dropped", "finish_store"):
        nb = mse_blocks(per)
        blk = (torch.arange(per) // 8 // 256) % nb  # the workgroup of every element
        keep = {"last_wg_dropped": blk != nb - 1, "second_pass_dropped": torch.arange(per) < nb * 2048,
                "finish_store": blk == nb - 1}[fault]
        terms = terms * keep.float()[None]
        if fault == "finish_store":
            terms = terms[-1:]
    loss = vsum(terms) if fault == "partial_unscaled" else vsum(terms) * sc(inv, dt)
    out = {"loss": S(lambda t: t.reshape(1), loss)}
    if p["want_dpred"]:
        L, r = X(dt)  # dpred is of the exact class: four IEEE operations and one rounding per element
        wx = (w.v if isV(w) else w)
        de = r(L(p["pred"]) - L(p["target"]))
        out["dpred"] = bfr(r(r(wx * r(2.0 * de)) * f32v(inv * p["grad_scale"])))
    return out


def sumsq_blocks(n):
    return max(1, min((n // 4 + 255) // 256, 2048))


def c_sumsq(p, dt, fault=None):
    g = p["g"]
    n = g.numel()
    if fault == "tail_dropped":
        g = g[:n - n % 4]
    elif fault == "last_wg_dropped":
        nb = sumsq_blocks(n)
        g = g[((torch.arange(g.numel()) // 1024) % nb) != nb - 1]
    elif fault == "second_pass_dropped":
        g = g[:sumsq_blocks(n) * 1024]
    g = lift(g, dt)
    return {"sumsq": S(lambda t: t.reshape(1), vsum(g * g))}


def clip_coef(s, max_norm, r):
    """(norm, max_norm / (norm + 1e-6f)) of the exact class: s a 0-dim tensor holding an fp32 value."""
    norm = r(s.sqrt())
    return norm, r(torch.full_like(norm, max_norm) / r(norm + f32v(1e-6)))  # a tensor divided by a tensor: scalar / tensor is a reciprocal and a product in torch


def c_clip(p, dt, fault=None):
    L, r = X(dt)
    g = L(p["g"])
    norm, coef = clip_coef(L(p["s"]), p["max_norm"], r)
    out = g
    if (bool(coef < 1.0) or fault == "coef_ge1") and (p["max_norm"] > 0 or fault == "maxnorm0_clips"):
        out = _second_pass(r(g * coef), 4096 * 256, fault, g)
    return {"g": out, "norm": norm.reshape(1)}


def c_adamw(p, dt, fault=None):
    L, r = X(dt)
    norm, coef = clip_coef(L(p["s"]), p["max_norm"], r)
    coef = float(min(coef, 1.0)) if p["max_norm"] > 0 else 1.0
    b1, b2, lr, wd, eps = (p[k] for k in ("beta1", "beta2", "lr", "wd", "eps"))  # fp32 values
    bc1 = 1.0 - b1 ** p["step"]
    bc2s = math.sqrt(1.0 - b2 ** p["step"])
    if fault == "bc_powf":  # the launcher before this test: 1 - powf(beta, step) in fp32
        pw = lambda b_: float(torch.tensor(b_, dtype=f32).pow(torch.tensor(float(p["step"]), dtype=f32)))
        bc1, bc2s = f32v(1.0 - pw(b1)), f32v(math.sqrt(f32v(1.0 - pw(b2))))
    decay, omb1, omb2 = f32v(1.0 - f32v(lr * wd)), f32v(1.0 - b1), f32v(1.0 - b2)
    g, p0, m0, v0 = (lift(p[k], dt) for k in ("g", "p", "m", "v"))
    gi = g * coef
    pi = p0 * decay
    mi = m0 + (gi - m0) * omb1
    vi = v0 * b2 + (gi * omb2) * gi
    denom = vsqrt(vi) / sc(bc2s, dt, 4 * U) + eps
    step_size = sc(lr, dt) / sc(bc1, dt, 4 * U)
    pn = pi - step_size * (mi / denom)
    out = {"p": pn, "m": mi, "v": vi}
    if fault == "second_pass_dropped":
        out = {k: _second_pass(o, 4096 * 256, fault, p[k].float()) for k, o in out.items()}
    out["norm"] = lift(norm.reshape(1).float(), dt)
    return out


def adamw_bf16_scalars(p):
    b1, b2, lr, wd = (p[k] for k in ("beta1", "beta2", "lr", "wd"))
    bc1, bc2 = 1.0 - b1 ** p["step"], 1.0 - b2 ** p["step"]
    return dict(decay=f32v(1.0 - lr * wd), w1=f32v(1.0 - b1), omb2=f32v(1.0 - b2), step_size=f32v(-(lr / bc1)), bc2s=f32v(math.sqrt(bc2)))


def c_adamw_bf16(p, dt, fault=None):
    L, r = X(dt)
    k = adamw_bf16_scalars(p)
    coef = 1.0
    out = {}
    if p.get("s") is not None:
        norm, c = clip_coef(L(p["s"]), p["max_norm"], r)
        coef = min(float(c), 1.0)
        if p["max_norm"] <= 0 and fault != "maxnorm0_clips":
            coef = 1.0
        if fault == "coef_ge1":
            coef = float(c)
        out["norm"] = norm.reshape(1)
    g, p0, m0, v0 = (L(p[k_]) for k_ in ("g", "p", "m", "v"))
    gi = g if fault == "unrounded" else bfr(g)
    if coef < 1.0 or (fault == "coef_ge1" and coef != 1.0):
        gi = bfr(r(gi * coef))
    pi = bfr(r(p0 * k["decay"]))
    w1 = k["w1"]
    if w1 < 0.5 or fault == "lerp_ignored":
        mi = bfr(r(m0 + r(w1 * r(gi - m0))))
    else:
        mi = bfr(r(gi - r(r(gi - m0) * f32v(1.0 - w1))))
    vi = bfr(r(v0 * p["beta2"]))
    vi = bfr(r(vi + r(r(k["omb2"] * gi) * gi)))
    d = bfr(r(vi.sqrt()))
    d = bfr(r(d / torch.full_like(d, k["bc2s"])))
    d = bfr(r(d + p["eps"]))
    pn = bfr(r(pi + r(k["step_size"] * r(mi / d))))
    res = {"p": pn, "m": mi, "v": vi}
    if fault == "second_pass_dropped":
        res = {k_: _second_pass(o, 4096 * 256, fault, L(p[k_])) for k_, o in res.items()}
    out.update(res)
    return out


def split_planes(w, dt, fault=None):
    L, r = X(dt)
    w = L(w)
    hi = bfr(w)
    lo = bfr(r(w - hi))
    return hi, (hi if fault == "lo_is_hi" else lo)


def lay_sp(hi, lo):
    rows, cols = hi.shape
    return torch.stack([hi.reshape(rows // 32, 32, cols), lo.reshape(rows // 32, 32, cols)], 1).reshape(2 * rows, cols)


def lay_ext(hi, lo, fault=None):
    if fault == "ext_off_cols":  # lo lands one plane early, the third plane keeps the sentinel
        return torch.cat([hi, lo, torch.full_like(lo, OUT_SENT)], 1)
    return torch.cat([hi, hi, lo], 1)


def c_lora_split(p, dt, fault=None):
    hi, lo = split_planes(p["w"], dt, fault)
    out = {}
    if "sp" in p["want"]:
        out["sp"] = lay_sp(hi, lo)
    if "ext" in p["want"]:
        out["ext"] = lay_ext(hi, lo, fault)
    if "t_sp" in p["want"]:
        out["t_sp"] = lay_sp(hi.t().contiguous(), lo.t().contiguous())
    if "t_ext" in p["want"]:
        out["t_ext"] = lay_ext(hi.t().contiguous(), lo.t().contiguous(), fault)
    return out


def c_lora_refresh(p, dt, fault=None):
    A, Bm = p["A"], p["B"]  # [L, n, r, D], [L, n, D, r]
    Ln, n, rk, D = A.shape
    a_sp, at_ext, b_ext, bt_sp = [], [], [], []
    for l in range(Ln):
        for i in range(n):
            hi, lo = split_planes(A[l, i], dt, fault)
            a_sp.append(lay_sp(hi, lo))
            at_ext.append(lay_ext(hi.t().contiguous(), lo.t().contiguous()))
            hi, lo = split_planes(Bm[l, i], dt, fault)
            b_ext.append(lay_ext(hi, lo))
            bt_sp.append(lay_sp(hi.t().contiguous(), lo.t().contiguous()))
    qkv = torch.stack([torch.cat([at_ext[l * n + (0 if fault == "inner_ignored" else i)] for i in range(3)], 1) for l in range(Ln)])
    return {"a_sp": torch.stack(a_sp), "at_ext": torch.stack(at_ext), "b_ext": torch.stack(b_ext), "bt_sp": torch.stack(bt_sp), "at_qkv_ext": qkv}


def c_transpose(p, dt, fault=None):
    L, _ = X(dt)
    return {"out": L(p["x"]).t().contiguous()}


def c_ada_prep(p, dt, fault=None):
    L, r = X(dt)
    tab, temb = L(p["tables"]), L(p["temb"])  # [L, 6, D], [B, 6, D]
    s = bfr(r(tab[:, None] + temb[None]))  # [L, B, 6, D]
    s6 = bfr(r(1.0 + s[:, :, 0 if fault == "slot6_from_slot0" else 1]))
    s7 = bfr(r(1.0 + s[:, :, 4]))
    return {"ada": torch.cat([s, s6[:, :, None], s7[:, :, None]], 2)}


def c_ada_out_prep(p, dt, fault=None):
    L, r = X(dt)
    t2, e = L(p["table2"]), L(p["emb"])  # [2, D], [B, D]
    shift, scale = bfr(r(t2[0][None] + e)), bfr(r(t2[1][None] + e))
    return {"out": torch.stack([shift, scale, bfr(r(1.0 + scale))], 1)}


def c_small_linear(p, dt, fault=None):
    x, w = lift(p["x"], dt), lift(p["w"], dt)  # [rows, K], [N, K]
    if p["silu_in"]:
        x = vsilu(x) if fault == "unrounded" else bf(vsilu(x))
    acc = vsum_last(S(lambda t: t[:, None, :], x) * S(lambda t: t[None], w))
    if p.get("bias") is not None and fault != "bias_dropped":
        acc = acc + S(lambda t: t[None], lift(p["bias"], dt))
    else:
        acc = acc + 0.0
    return {"y": bf(acc)}


def sinus_freq_args():
    """The fp32 arguments of expf: (-9.210340371976184f * (float)j) / 128.0f."""
    c = torch.tensor(-9.210340371976184, dtype=f32)
    return (c * torch.arange(128, dtype=f32)) / 128.0


def c_sinusoid(p, dt, fault=None):
    t = lift(p["t"], dt)  # [B]
    freq = vfun("expf", lift(sinus_freq_args(), dt))
    a = S(lambda q: q[:, None], t) * S(lambda q: q[None], freq)
    co, si = bf(vfun("cosf", a)), bf(vfun("sinf", a))
    return {"out": S(lambda x, y: torch.cat([x, y], 1), co, si)}


CONTRACT = {"noise_pack": c_noise_pack, "ddim": c_ddim, "posterior": c_posterior, "mse": c_mse, "sumsq": c_sumsq, "clip": c_clip, "adamw": c_adamw,
            "adamw_bf16": c_adamw_bf16, "lora_split": c_lora_split, "lora_refresh": c_lora_refresh, "transpose": c_transpose, "ada_prep": c_ada_prep,
            "ada_out_prep": c_ada_out_prep, "small_linear": c_small_linear, "sinusoid": c_sinusoid}
BOUNDED = {"posterior", "mse", "sumsq", "adamw", "small_linear", "sinusoid"}
BF16_OUT = {("posterior", "out"), ("mse", "dpred"), ("small_linear", "y"), ("sinusoid", "out")}


def reference(p):
    """name -> (reference, bound), fp64.  Exact class: bound 0."""
    out = CONTRACT[p["op"]](p, f64)
    out = {k: ((v.v, v.e) if isV(v) else (v.double(), torch.zeros_like(v, dtype=f64))) for k, v in out.items()}
    return {k: (v, torch.zeros_like(e)) for k, (v, e) in out.items()} if p.get("exact") else out


def stand_in(p, fault=None):
    return {k: v for k, v in CONTRACT[p["op"]](p, f32, fault).items()}


# ----------------------------------------------------------------------------------------------------
# the check

def block_share(mism):
    m = mism.flatten().double()
    n = m.numel()
    edges = list(range(0, n, 4096)) + [n]
    if len(edges) > 2 and edges[-1] - edges[-2] < 4096:
        del edges[-2]
    cs = torch.cat([torch.zeros(1, dtype=f64), m.cumsum(0)])
    e = torch.tensor(edges)
    return float(((cs[e[1:]] - cs[e[:-1]]) / (e[1:] - e[:-1]).double()).max()) if n else 0.0


FIGURES = {}  # launcher -> [largest err / bound, largest block share or mismatch count]


def judge(tag, op, name, got, ref, bound, cap=CAP):
    got = got.double().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{tag} {name}: non-finite output ({(~torch.isfinite(got)).sum().item()} entries)"
    err = (got - ref).abs()
    bad = err > bound
    worst = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.0
    share = block_share(got != ref) if (op, name) in BF16_OUT else 0.0
    fig = FIGURES.setdefault(op, [0.0, 0.0])
    fig[0], fig[1] = max(fig[0], worst), max(fig[1], share)
    print(f"[elementwise] {tag} {name}: max_err_over_bound={worst:.3f} max_block_mismatch={share:.4f}")
    if bad.any():
        i = tuple(int(t[0]) for t in bad.nonzero(as_tuple=True))
        raise AssertionError(f"{tag} {name}: element {list(i)} got {got[i].item():.9g} ref {ref[i].item():.9g} bound {bound[i].item():.3g}; "
                             f"{int(bad.sum())} of {bad.numel()} elements over their bound")
    assert share <= cap, f"{tag} {name}: {share:.4f} of a block of 4096 differs from the reference (cap {cap})"


def judge_case(tag, p, outs, R=None, cap=CAP):
    R = R or reference(p)
    assert set(outs) == set(R), (sorted(outs), sorted(R))
    for n, (ref, bound) in R.items():
        judge(tag, p["op"], n, outs[n], ref, bound, cap)


# ----------------------------------------------------------------------------------------------------
# inputs

def gen(seed):
    return torch.Generator().manual_seed(seed)


def rbf(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(bf16)


def mk_noise_pack(C, Sn, B, fft, sf):
    g = gen(1000 * C + Sn + B)
    p = {"op": "noise_pack", "lat": rbf((B, C, Sn), g, 2.0), "noise": rbf((B, C, Sn), g), "mean": torch.randn(C, generator=g) * 0.5,
         "std": torch.rand(C, generator=g) + 0.5, "sigma": torch.tensor([0.3, 0.7, 0.55][:B]), "fft": fft}
    p["sigma_first"] = torch.tensor([0.05, 0.9, 0.2][:B]) if sf else None
    return p


PER_BIG = [8, 8 * 255, 8 * 256, 8 * 257, 2097152, 2097160, 2 * 2097152 + 8 * 300]
PER_MSE = [8, 8 * 255, 8 * 256, 8 * 257, 524288, 524296, 2 * 524288 + 8 * 300]
N_SUMSQ = [1, 3, 4, 5, 6, 1024, 1027, 2097152, 2097155, 2 * 2097152 + 1031]
N_OPT = [1, 255, 256, 257, 1048576, 1048577, 2 * 1048576 + 77]
SHAPES_2D = [(1, 1), (31, 33), (33, 31), (32, 32), (64, 96), (1, 4097), (4097, 1)]


def mk_ddim(per, B, mode, want_x0):
    g = gen(per % 9973 + B)
    bfv = lambda v: torch.tensor(v).to(bf16).float()
    return {"op": "ddim", "a": rbf((B, per), g, 3.0), "b": rbf((B, per), g), "sa": bfv([0.96, 0.31, 0.7][:B]), "so": bfv([0.28, 0.95, 0.71][:B]),
            "scale": f32v(0.7) if mode == 0 else 1.0, "mode": mode, "want_x0": want_x0 and mode == 0}


def mk_posterior(per, B):
    g = gen(per % 9973 + 7 * B)
    lv = (torch.rand((B, per), generator=g) * 70.0 - 40.0).to(bf16)  # beyond both clamps
    sp = torch.tensor([-30.0, 20.0, 0.0, -0.0, -30.25, 20.125, -40.0, 30.0]).to(bf16)
    lv[:, :8] = sp
    lv[:, -8:] = sp.flip(0)
    mom = torch.stack([rbf((B, per), g, 2.0), lv], 1)
    return {"op": "posterior", "moments": mom, "eps": rbf((B, per), g)}


def mk_mse(per, B, weight, want_dpred, grad_scale):
    g = gen(per % 9973 + 11 * B)
    return {"op": "mse", "pred": rbf((B, per), g), "target": rbf((B, per), g), "weight": torch.tensor([1.37, 64.0, 0.21][:B]) if weight else None,
            "want_dpred": want_dpred, "grad_scale": grad_scale}


def probe_positions(n):
    nb, n4 = sumsq_blocks(n), n // 4
    pos = [0, 3, 4, n4 * 4 - 1, n4 * 4, n - 1, 1023, 1024, nb * 1024 - 1, nb * 1024, nb * 1024 + 1]
    return sorted({q for q in pos if 0 <= q < n})


def mk_sumsq(n, probes):
    if probes:
        gg = torch.zeros(n)
        for k, q in enumerate(probe_positions(n)):
            gg[q] = 2.0**k
    else:
        gg = torch.randn(n, generator=gen(n % 9973)) * 0.01
    return {"op": "sumsq", "g": gg, "exact": probes}  # the probes' squares add up exactly in fp32 in any order: bound 0


def opt_data(n, zero_grad=False):
    g = gen(n % 9973 + 3)
    i = torch.arange(n, dtype=f64)
    p0 = (torch.randn(n, generator=g) * 0.02 + (i % 977).float() * 1e-5)
    gr = torch.randn(n, generator=g) * 1e-3 * (1.0 + (i % 131).float())
    m0 = torch.randn(n, generator=g) * 1e-3
    v0 = torch.rand(n, generator=g) * 1e-5
    p0[16:48] = 0.0
    gr[48:64] = 3e-20
    gr[64:80] = 1e-30
    v0[56:72] = 0.0
    if zero_grad:
        gr = torch.zeros(n)
    return p0, gr, m0, v0


HYPER = [dict(step=st, betas=bt, clip=cl) for st in (1, 2, 1000) for bt in ((0.9, 0.95), (0.9, 0.999)) for cl in ("active", "inactive", "disabled")]
HYPER += [dict(step=2, betas=(0.9, 0.95), clip="active", zero_grad=True), dict(step=3, betas=(0.4, 0.95), clip="active"),
          dict(step=1, betas=(0.4, 0.999), clip="none")]


def hyper_id(h):
    return f"step{h['step']}-b{h['betas'][0]}-{h['betas'][1]}-{h['clip']}" + ("-zerograd" if h.get("zero_grad") else "")


def mk_opt(op, n, h):
    """h: step, betas, clip in active / inactive / disabled / none (bf16 only: sumsq NULL).  The sum of squares is a chosen fp32 value (the fp32 AdamW test
    replaces it by what ftmi_clip_adamw_step left in its scratch)."""
    p0, gr, m0, v0 = opt_data(n, h.get("zero_grad", False))
    true = float((gr.double() ** 2).sum())
    s = {"active": f32v(true), "inactive": f32v(true), "disabled": f32v(true), "none": None}[h["clip"]]
    norm = math.sqrt(true)
    max_norm = {"active": f32v(0.37 * norm) if norm > 0 else 1.0, "inactive": f32v(norm * 1.5 + 1.0), "disabled": 0.0, "none": 1.0}[h["clip"]]
    p = {"op": op, "g": gr, "p": p0, "m": m0, "v": v0, "s": None if s is None else torch.tensor(s, dtype=f32), "max_norm": max_norm, "step": h["step"],
         "beta1": f32v(h["betas"][0]), "beta2": f32v(h["betas"][1]), "lr": f32v(5e-3), "wd": f32v(1e-2), "eps": f32v(1e-8)}
    if op == "adamw_bf16":
        p["p"], p["m"], p["v"] = p0.to(bf16), m0.to(bf16), v0.to(bf16)
    if op == "clip":
        p = {"op": "clip", "g": gr, "s": p["s"], "max_norm": max_norm}
    return p


def size_hyper(k):
    return HYPER[(5 * k + 1) % 18]


def lora_values(rows, cols, seed):
    w = torch.randn((rows, cols), generator=gen(seed)) * 0.05
    flat = w.flatten()
    k = flat[0::7].numel()
    flat[0::7] = 2.0**-120 * (1.0 + (torch.arange(k) % 15 + 1).float() * 2.0**-12)    # hi = 2^-120, w - hi = k 2^-132: subnormal
    flat[1::7] = flat[1::7].to(bf16).float()                                       # lo plane exactly zero
    return flat.reshape(rows, cols)


def mk_lora_split(rows, cols, want):
    return {"op": "lora_split", "w": lora_values(rows, cols, rows * 131 + cols), "want": want}


def mk_lora_refresh(nadp, Ln=2, rk=32, D=64):
    return {"op": "lora_refresh", "A": torch.stack([lora_values(rk, D, 50 + i) for i in range(Ln * nadp)]).reshape(Ln, nadp, rk, D),
            "B": torch.stack([lora_values(D, rk, 90 + i) for i in range(Ln * nadp)]).reshape(Ln, nadp, D, rk)}


def mk_transpose(rows, cols):
    return {"op": "transpose", "x": rbf((rows, cols), gen(rows + 3 * cols))}


def mk_ada_prep(Ln, B, D):
    g = gen(Ln + 10 * B + D)
    return {"op": "ada_prep", "tables": rbf((Ln, 6, D), g), "temb": rbf((B, 6, D), g, 2.0)}


def mk_ada_out_prep(B, D):
    g = gen(B + D)
    return {"op": "ada_out_prep", "table2": rbf((2, D), g), "emb": rbf((B, D), g, 2.0)}


def mk_small_linear(rows, N, K, silu_in, bias):
    g = gen(rows + 10 * N + K)
    return {"op": "small_linear", "x": rbf((rows, K), g, 3.0 if silu_in else 1.0), "w": rbf((N, K), g, 0.05), "bias": rbf((N,), g) if bias else None, "silu_in": silu_in}


def mk_sinusoid(B):
    return {"op": "sinusoid", "t": torch.tensor([0.0, 0.5, 1.0, 999.0, 1000.0, 0.5, 999.0, 1.0][:B])}


SL_CASES = [(rows, N, K) for rows, N, K in
            [(1, 1, 8), (2, 4, 256), (3, 5, 512), (4, 2048, 520), (5, 5, 2048), (6, 4, 8), (7, 1, 520), (8, 2048, 256), (8, 5, 512), (1, 2048, 2048)]]


def cpu_cases(big=False):
    """The cases the CPU self-checks walk: every structure at its small sizes (big: the cap-crossing sizes too)."""
    out = []
    for C, Sn in ((1, 1), (63, 65), (65, 200), (128, 64)):
        for B in (1, 3):
            for fft in (0, 1, 70, Sn, Sn + 5):
                for sf in (True, False):
                    out.append(mk_noise_pack(C, Sn, B, fft, sf))
    pers = PER_BIG if big else PER_BIG[:4]
    for per in pers:
        for B in (1, 3):
            out += [mk_ddim(per, B, 0, True), mk_ddim(per, B, 0, False), mk_ddim(per, B, 1, False), mk_posterior(per, B)]
    for per in (PER_MSE if big else PER_MSE[:4]):
        for B in (1, 3):
            out += [mk_mse(per, B, wt, dp, gs) for wt in (True, False) for dp in (True, False) for gs in (1.0, 0.25)]
    for n in (N_SUMSQ if big else N_SUMSQ[:7]):
        out += [mk_sumsq(n, True), mk_sumsq(n, False)]
    for k, n in enumerate(N_OPT if big else N_OPT[:4]):
        out += [mk_opt(op, n, size_hyper(k)) for op in ("clip", "adamw", "adamw_bf16")]
    for h in HYPER:
        out += [mk_opt(op, 257, h) for op in ("clip", "adamw", "adamw_bf16") if h["clip"] != "none" or op == "adamw_bf16"]
    for rows, cols in SHAPES_2D:
        out += [mk_lora_split(rows, cols, ("ext", "t_ext")), mk_transpose(rows, cols)]
    out += [mk_lora_split(rows, cols, ("sp", "ext", "t_sp", "t_ext")) for rows in (32, 64, 96) for cols in (32, 64, 96)]
    out += [mk_lora_refresh(n) for n in (3, 4, 8)]
    out += [mk_ada_prep(Ln, B, D) for Ln in (1, 3) for B in (1, 3) for D in (64, 2048)]
    out += [mk_ada_out_prep(B, D) for B in (1, 3) for D in (64, 2048)]
    out += [mk_small_linear(rows, N, K, si, bi) for rows, N, K in SL_CASES for si in (False, True) for bi in (True, False)]
    out += [mk_sinusoid(B) for B in (1, 3, 8)]
    return out


def tag_of(p):
    d = {k: (tuple(v.shape) if torch.is_tensor(v) and v.dim() else (float(v) if torch.is_tensor(v) else v)) for k, v in p.items() if k != "op"}
    return p["op"] + " " + " ".join(f"{k}={v}" for k, v in d.items())


# ----------------------------------------------------------------------------------------------------
# GPU: every tensor the kernels see lies between sentinel padding in a buffer the test owns

def _dev():
    return torch.device("cuda", 0)


class Bufs:
    def __init__(self):
        self.dev, self.outs, self.keep = _dev(), {}, []  # keep: the inputs stay allocated until the launch has run

    def inp(self, t, fill=IN_SENT):
        if t is None:
            return None
        b = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype)
        b[PAD:PAD + t.numel()] = t.flatten()
        self.keep.append(b.to(self.dev))
        return self.keep[-1][PAD:PAD + t.numel()]

    def out(self, name, shape, dtype=bf16, init=None):
        n = math.prod(shape)
        b = torch.full((n + 2 * PAD,), OUT_SENT, dtype=dtype)
        if init is not None:
            b[PAD:PAD + n] = init.flatten().to(dtype)
        b = b.to(self.dev)
        self.outs[name] = (b, shape)
        return b[PAD:PAD + n]

    def collect(self):
        res = {}
        for name, (b, shape) in self.outs.items():
            h = b.cpu()
            n = math.prod(shape)
            assert (h[:PAD] == OUT_SENT).all() and (h[PAD + n:] == OUT_SENT).all(), f"{name}: padding overwritten"
            res[name] = h[PAD:PAD + n].reshape(shape)
        return res


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def launch_once(p, scratch):
    """One launch of the case's entry point on fresh padded buffers (scratch: the caller's, reused by the second launch)."""
    from finetrainers_amd import _lib

    lib, ptr, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
    b, op = Bufs(), p["op"]
    ck = lambda rc: _lib.check(rc, op)
    extra = {}
    if op == "noise_pack":
        B, C, Sn = p["lat"].shape
        xt, tg = b.out("xt", (B, Sn, C)), b.out("target", (B, Sn, C))
        ck(lib.ftmi_ltx_noise_pack(ptr(b.inp(p["lat"])), ptr(b.inp(p["noise"])), ptr(b.inp(p["mean"])), ptr(b.inp(p["std"])), ptr(b.inp(p["sigma"])),
                                   ptr(b.inp(p["sigma_first"])), p["fft"], ptr(xt), ptr(tg), B, C, Sn, st))
    elif op == "ddim":
        B, per = p["a"].shape
        o = b.out("out", (B, per))
        a_, b_, sa, so = b.inp(p["a"]), b.inp(p["b"]), b.inp(p["sa"]), b.inp(p["so"])
        if p["mode"] == 0:
            x0 = b.out("x0", (B, per)) if p["want_x0"] else None
            ck(lib.ftmi_ddim_add_noise(ptr(a_), ptr(b_), ptr(sa), ptr(so), p["scale"], ptr(x0), ptr(o), B, per, st))
        else:
            ck(lib.ftmi_ddim_get_velocity(ptr(a_), ptr(b_), ptr(sa), ptr(so), ptr(o), B, per, st))
    elif op == "posterior":
        B, per = p["eps"].shape
        o = b.out("out", (B, per))
        ck(lib.ftmi_posterior_sample(ptr(b.inp(p["moments"])), ptr(b.inp(p["eps"])), ptr(o), B, per, st))
    elif op == "mse":
        B, per = p["pred"].shape
        loss = b.out("loss", (1,), f32)
        dp = b.out("dpred", (B, per)) if p["want_dpred"] else None
        ck(lib.ftmi_mse_loss(ptr(b.inp(p["pred"])), ptr(b.inp(p["target"])), ptr(b.inp(p["weight"])), ptr(loss), ptr(dp), B, per, p["grad_scale"],
                             ptr(scratch), st))
    elif op == "sumsq":
        ck(lib.ftmi_grad_sumsq(ptr(b.inp(p["g"])), p["g"].numel(), ptr(scratch), st))
        extra["sumsq"] = scratch[:1].cpu()
    elif op == "clip":
        n = p["g"].numel()
        g, norm = b.out("g", (n,), f32, p["g"]), b.out("norm", (1,), f32)
        if p.get("via_norm"):  # ftmi_clip_grad_norm: its own sum of squares, left in scratch[0]
            ck(lib.ftmi_clip_grad_norm(ptr(g), n, p["max_norm"], ptr(scratch), ptr(norm), st))
            extra["s_used"] = scratch[:1].cpu()
        else:
            ck(lib.ftmi_clip_by_sumsq(ptr(g), n, ptr(b.inp(p["s"].reshape(1))), p["max_norm"], ptr(norm), st))
    elif op == "adamw":
        n = p["g"].numel()
        t = {k: b.out(k, (n,), f32, p[k]) for k in ("p", "m", "v")}
        norm = b.out("norm", (1,), f32)
        ck(lib.ftmi_clip_adamw_step(ptr(t["p"]), ptr(b.inp(p["g"])), ptr(t["m"]), ptr(t["v"]), n, p["max_norm"], p["lr"], p["beta1"], p["beta2"], p["eps"],
                                    p["wd"], p["step"], ptr(scratch), ptr(norm), st))
        extra["s_used"] = scratch[:1].cpu()
    elif op == "adamw_bf16":
        n = p["g"].numel()
        t = {k: b.out(k, (n,), bf16, p[k]) for k in ("p", "m", "v")}
        norm = b.out("norm", (1,), f32) if p.get("s") is not None else None
        s = b.inp(p["s"].reshape(1)) if p.get("s") is not None else None
        ck(lib.ftmi_adamw_bf16_step(ptr(t["p"]), ptr(b.inp(p["g"])), ptr(t["m"]), ptr(t["v"]), n, ptr(s), p["max_norm"], p["lr"], p["beta1"], p["beta2"],
                                    p["eps"], p["wd"], p["step"], ptr(norm), st))
    elif op == "lora_split":
        rows, cols = p["w"].shape
        shp = {"sp": (2 * rows, cols), "ext": (rows, 3 * cols), "t_sp": (2 * cols, rows), "t_ext": (cols, 3 * rows)}
        o = {k: (b.out(k, shp[k]) if k in p["want"] else None) for k in shp}
        ck(lib.ftmi_lora_split(ptr(b.inp(p["w"])), rows, cols, ptr(o["sp"]), ptr(o["ext"]), ptr(o["t_sp"]), ptr(o["t_ext"]), st))
    elif op == "lora_refresh":
        Ln, n, rk, D = p["A"].shape
        o = {"a_sp": b.out("a_sp", (Ln * n, 2 * rk, D)), "bt_sp": b.out("bt_sp", (Ln * n, 2 * rk, D)), "b_ext": b.out("b_ext", (Ln * n, D, 3 * rk)),
             "at_ext": b.out("at_ext", (Ln * n, D, 3 * rk)), "at_qkv_ext": b.out("at_qkv_ext", (Ln, D, 9 * rk))}
        ck(lib.ftmi_lora_refresh_n(ptr(b.inp(p["A"])), ptr(b.inp(p["B"])), ptr(o["a_sp"]), ptr(o["bt_sp"]), ptr(o["b_ext"]), ptr(o["at_ext"]),
                                   ptr(o["at_qkv_ext"]), Ln, n, rk, D, st))
    elif op == "transpose":
        rows, cols = p["x"].shape
        ck(lib.ftmi_transpose_bf16(ptr(b.inp(p["x"])), ptr(b.out("out", (cols, rows))), rows, cols, st))
    elif op == "ada_prep":
        (Ln, _, D), B = p["tables"].shape, p["temb"].shape[0]
        ck(lib.ftmi_ada_prep(ptr(b.inp(p["tables"])), ptr(b.inp(p["temb"])), ptr(b.out("ada", (Ln, B, 8, D))), Ln, B, D, st))
    elif op == "ada_out_prep":
        B, D = p["emb"].shape
        ck(lib.ftmi_ada_out_prep(ptr(b.inp(p["table2"])), ptr(b.inp(p["emb"])), ptr(b.out("out", (B, 3, D))), B, D, st))
    elif op == "small_linear":
        (rows, K), N = p["x"].shape, p["w"].shape[0]
        ck(lib.ftmi_small_linear(ptr(b.inp(p["x"])), ptr(b.inp(p["w"])), ptr(b.inp(p["bias"])), ptr(b.out("y", (rows, N))), rows, N, K, int(p["silu_in"]), st))
    elif op == "sinusoid":
        B = p["t"].numel()
        ck(lib.ftmi_timestep_sinusoid(ptr(b.inp(p["t"])), ptr(b.out("out", (B, 256))), B, st))
    else:
        raise KeyError(op)
    torch.cuda.synchronize()
    res = b.collect()
    res.update(extra)
    return res


def launch(p):
    """Runs the case twice on the same scratch and asserts the same bits; returns the outputs of the second run."""
    B = p["pred"].shape[0] if p["op"] == "mse" else 1
    scratch = torch.full((max(2050, 256 * B) + 2 * PAD,), IN_SENT, dtype=f32, device=_dev())
    first = launch_once(p, scratch[PAD:-PAD])
    second = launch_once(p, scratch[PAD:-PAD])
    h = scratch.cpu()
    assert (h[:PAD] == IN_SENT).all() and (h[-PAD:] == IN_SENT).all(), "scratch padding overwritten"
    for k in first:
        assert torch.equal(bits(first[k]), bits(second[k])), f"{tag_of(p)} {k}: two launches on the same scratch differ"
    return second


def run_gpu(p):
    _threads()
    outs = launch(p)
    s_used = outs.pop("s_used", None)
    if s_used is not None:  # the sum of squares the kernel took: inside sumsq's bound, and the input of the reference
        ref, bound = reference({"op": "sumsq", "g": p["g"]})["sumsq"]
        judge(tag_of(p), "sumsq", "s_used", s_used, ref, bound)
        p = dict(p, s=s_used.reshape(()))
    judge_case(tag_of(p), p, outs)


# ---- GPU tests -------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("C,Sn", [(C, Sn) for C in (1, 63, 64, 65, 128) for Sn in (1, 63, 64, 65, 200)])
def test_noise_pack(C, Sn):
    for B in (1, 3):
        for fft in (0, 1, 70, Sn, Sn + 5):
            for sf in (True, False):
                run_gpu(mk_noise_pack(C, Sn, B, fft, sf))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", PER_BIG)
def test_ddim_mix(per, B):
    for mode, x0 in ((0, True), (0, False), (1, False)):
        run_gpu(mk_ddim(per, B, mode, x0))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", PER_BIG)
def test_posterior_sample(per, B):
    run_gpu(mk_posterior(per, B))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", PER_MSE)
def test_mse_loss(per, B):
    for wt in (True, False):
        for dp in (True, False):
            for gs in (1.0, 0.25):
                run_gpu(mk_mse(per, B, wt, dp, gs))


@pytest.mark.gpu
@pytest.mark.parametrize("n", N_SUMSQ)
def test_sumsq(n):
    run_gpu(mk_sumsq(n, True))
    run_gpu(mk_sumsq(n, False))


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["clip", "adamw", "adamw_bf16"])
@pytest.mark.parametrize("k", range(len(N_OPT)), ids=[str(n) for n in N_OPT])
def test_optimiser_sizes(k, op):
    run_gpu(mk_opt(op, N_OPT[k], size_hyper(k)))
    if op == "clip":
        run_gpu(dict(mk_opt(op, N_OPT[k], size_hyper(k)), via_norm=True))
    if op == "adamw_bf16" and N_OPT[k] == 1048577:
        run_gpu(mk_opt(op, N_OPT[k], HYPER[-2]))  # w1 >= 0.5 at a size where the two lerp forms are told apart (see FAULTS)


@pytest.mark.gpu
@pytest.mark.parametrize("h", HYPER, ids=hyper_id)
def test_optimiser_settings(h):
    for op in ("clip", "adamw", "adamw_bf16"):
        if h["clip"] == "none" and op != "adamw_bf16":
            continue
        run_gpu(mk_opt(op, 257, h))
        if op == "clip":
            run_gpu(dict(mk_opt(op, 257, h), via_norm=True))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SHAPES_2D)
def test_lora_split_and_transpose(rows, cols):
    for want in (("ext", "t_ext"), ("ext",), ("t_ext",)):
        run_gpu(mk_lora_split(rows, cols, want))
    run_gpu(mk_transpose(rows, cols))


@pytest.mark.gpu
def test_lora_split_planes_and_refresh():
    for rows in (32, 64, 96):
        for cols in (32, 64, 96):
            run_gpu(mk_lora_split(rows, cols, ("sp", "ext", "t_sp", "t_ext")))
            run_gpu(mk_lora_split(rows, cols, ("sp", "t_sp")))
    for n in (3, 4, 8):
        run_gpu(mk_lora_refresh(n))


@pytest.mark.gpu
def test_time_embedding_chain():
    for B in (1, 3, 8):
        run_gpu(mk_sinusoid(B))
    for Ln in (1, 3):
        for B in (1, 3):
            for D in (64, 2048):
                run_gpu(mk_ada_prep(Ln, B, D))
    for B in (1, 3):
        for D in (64, 2048):
            run_gpu(mk_ada_out_prep(B, D))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,N,K", SL_CASES)
def test_small_linear(rows, N, K):
    for si in (False, True):
        for bi in (True, False):
            run_gpu(mk_small_linear(rows, N, K, si, bi))


def boundary_distance(v):
    """Relative distance of fp64 values to the nearest bf16 rounding boundary (the midpoint of two neighbouring bf16 numbers)."""
    a = v.abs()
    ulp = ulp_bf(a)
    frac = torch.remainder(a / ulp.clamp_min(1e-300), 1.0)
    return (frac - 0.5).abs() * ulp / a.clamp_min(1e-300)


def sweep_figure(got, ref64, weight=None):
    """Largest boundary distance among the outputs that differ from bf(reference), and their count."""
    want = bfr(ref64).float().to(bf16)
    mism = got.flatten().float() != want.flatten().float()  # by value: the probes' sums of zeros lose the sign of a zero
    d = boundary_distance(ref64.flatten())
    if weight is not None:
        d = d / weight.flatten()
    return (float(d[mism].max()) if mism.any() else 0.0), int(mism.sum())


def bf16_values(lo, hi):
    """Every bf16 number in [lo, hi]."""
    allv = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(bf16).float()
    return allv[torch.isfinite(allv) & (allv >= lo) & (allv <= hi)].to(bf16)


def sweep_inputs():
    h = bf16_values(-15.0, 10.0)
    h = h.repeat((2**18 + h.numel() - 1) // h.numel())
    h = h[:(h.numel() // 8) * 8]
    x = bf16_values(-20.0, 20.0)
    x = x.repeat((2**18 + x.numel() - 1) // x.numel())
    x = x[: (x.numel() // 16384) * 16384]
    t = torch.rand(2**18, generator=gen(5), dtype=f64).mul(1000.0).float()
    t[:3] = torch.tensor([0.0, 1000.0, 0.5])
    return h, x, t


@pytest.mark.gpu
def test_transcendental_error_figures():
    """T_SEEN of expf, cosf, sinf and silu on the device (see BOUNDS): each must stay within the T_REL the bounds use, and below 2^-20."""
    from finetrainers_amd import ops

    _threads()
    dev = _dev()
    h, x, t = sweep_inputs()
    seen = {}
    mom = torch.stack([torch.zeros_like(h), (h.float() * 2.0).to(bf16)], 0)[None]  # [1, 2, n]; bf(0.5 l) = h exactly
    got = ops.posterior_sample(mom.to(dev), torch.ones((1, 1, h.numel()), dtype=bf16, device=dev)).cpu()
    seen["expf"] = sweep_figure(got, h.double().exp())
    sin_out = torch.cat([ops.timestep_sinusoid(t[i:i + 2**15].to(dev))[:, [0, 128]].cpu() for i in range(0, t.numel(), 2**15)])
    seen["cosf"] = sweep_figure(sin_out[:, 0], t.double().cos())
    seen["sinf"] = sweep_figure(sin_out[:, 1], t.double().sin())
    eye = torch.eye(2048, dtype=bf16, device=dev)
    xs = x.reshape(-1, 8, 2048)
    y = torch.cat([ops.small_linear(xs[i].to(dev), eye, None, silu_in=True).cpu() for i in range(xs.shape[0])])
    xd = x.double()
    seen["silu"] = sweep_figure(y, xd / (1.0 + (-xd).exp()), 1.0 + xd.abs())
    for k, (fig, cnt) in seen.items():
        print(f"[elementwise] {k}: T_SEEN {fig:.4e} = {fig / U:.3f} u over {cnt} flipped outputs (T_SEEN in use {T_SEEN[k]:.4e}, T_REL {T_REL[k]:.4e})")
    for k, (fig, cnt) in seen.items():
        assert fig <= 2.0**-20, f"{k}: error {fig:.3e} above 2^-20: a finding, not a figure to adopt"
        assert fig <= T_REL[k], f"{k}: error {fig:.3e} above the figure the bounds use ({T_REL[k]:.3e})"


@pytest.mark.gpu
def test_elementwise_refusals_and_zero_sizes():
    """Bad sizes come back as errors and zero sizes as 0, both before any launch: every output keeps its sentinel."""
    from finetrainers_amd import _lib

    lib, ptr, st, dev = _lib.load(), _lib.ptr, _lib.stream_ptr(), _dev()
    INV, UNS = _lib.FTMI_ERR_INVALID, _lib.FTMI_ERR_UNSUPPORTED
    xb = torch.full((8192,), 1.0, dtype=bf16, device=dev)
    ob = torch.full((8192,), OUT_SENT, dtype=bf16, device=dev)
    xf = torch.full((8192,), 0.5, dtype=f32, device=dev)
    of = torch.full((8192,), OUT_SENT, dtype=f32, device=dev)
    X_, O, F, G = ptr(xb), ptr(ob), ptr(xf), ptr(of)
    calls = [
        (lambda: lib.ftmi_ltx_noise_pack(X_, X_, F, F, F, None, 0, O, O, 0, 4, 4, st), 0, "noise_pack B = 0"),
        (lambda: lib.ftmi_ltx_noise_pack(X_, X_, F, F, F, None, 0, O, O, 2, 0, 4, st), 0, "noise_pack C = 0"),
        (lambda: lib.ftmi_ltx_noise_pack(X_, X_, F, F, F, None, 0, O, O, 2, 4, 0, st), 0, "noise_pack S = 0"),
        (lambda: lib.ftmi_ltx_noise_pack(X_, X_, F, F, F, None, 0, O, O, 2, -4, 4, st), INV, "noise_pack C < 0"),
        (lambda: lib.ftmi_ddim_add_noise(X_, X_, F, F, 1.0, O, O, 2, 0, st), 0, "ddim_add_noise per_sample = 0"),
        (lambda: lib.ftmi_ddim_add_noise(X_, X_, F, F, 1.0, O, O, 0, 8, st), INV, "ddim_add_noise B = 0"),
        (lambda: lib.ftmi_ddim_add_noise(X_, X_, F, F, 1.0, O, O, 2, 12, st), UNS, "ddim_add_noise per_sample = 12"),
        (lambda: lib.ftmi_ddim_get_velocity(X_, X_, F, F, O, 2, 0, st), 0, "ddim_get_velocity per_sample = 0"),
        (lambda: lib.ftmi_ddim_get_velocity(X_, X_, F, F, O, 0, 8, st), INV, "ddim_get_velocity B = 0"),
        (lambda: lib.ftmi_posterior_sample(X_, X_, O, 2, 0, st), INV, "posterior_sample per_sample = 0"),
        (lambda: lib.ftmi_posterior_sample(X_, X_, O, 0, 8, st), INV, "posterior_sample B = 0"),
        (lambda: lib.ftmi_posterior_sample(X_, X_, O, 2, 12, st), UNS, "posterior_sample per_sample = 12"),
        (lambda: lib.ftmi_mse_loss(X_, X_, None, G, O, 0, 8, 1.0, F, st), INV, "mse_loss B = 0"),
        (lambda: lib.ftmi_mse_loss(X_, X_, None, G, O, 2, 0, 1.0, F, st), INV, "mse_loss per_sample = 0"),
        (lambda: lib.ftmi_mse_loss(X_, X_, None, G, O, 2, 12, 1.0, F, st), UNS, "mse_loss per_sample = 12"),
        (lambda: lib.ftmi_grad_sumsq(F, 0, G, st), INV, "grad_sumsq n = 0"),
        (lambda: lib.ftmi_clip_grad_norm(G, 0, 1.0, F, G, st), INV, "clip_grad_norm n = 0"),
        (lambda: lib.ftmi_clip_by_sumsq(G, 0, F, 0.001, G, st), 0, "clip_by_sumsq n = 0"),
        (lambda: lib.ftmi_clip_by_sumsq(G, -1, F, 0.001, G, st), INV, "clip_by_sumsq n < 0"),
        (lambda: lib.ftmi_clip_adamw_step(G, F, G, G, 0, 1.0, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1, G, G, st), 0, "clip_adamw_step n = 0"),
        (lambda: lib.ftmi_clip_adamw_step(G, F, G, G, -1, 1.0, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1, G, G, st), INV, "clip_adamw_step n < 0"),
        (lambda: lib.ftmi_clip_adamw_step(G, F, G, G, 8, 1.0, 1e-3, 0.9, 0.95, 1e-8, 0.0, 0, G, G, st), INV, "clip_adamw_step step = 0"),
        (lambda: lib.ftmi_adamw_bf16_step(O, F, O, O, 0, F, 1.0, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1, G, st), 0, "adamw_bf16_step n = 0"),
        (lambda: lib.ftmi_adamw_bf16_step(O, F, O, O, -1, F, 1.0, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1, G, st), INV, "adamw_bf16_step n < 0"),
        (lambda: lib.ftmi_lora_split(F, 0, 32, O, O, O, O, st), 0, "lora_split rows = 0"),
        (lambda: lib.ftmi_lora_split(F, 32, 0, O, O, O, O, st), 0, "lora_split cols = 0"),
        (lambda: lib.ftmi_lora_split(F, 33, 32, O, None, None, None, st), UNS, "lora_split sp with 33 rows"),
        (lambda: lib.ftmi_lora_split(F, 32, 31, None, None, O, None, st), UNS, "lora_split t_sp with 31 columns"),
        (lambda: lib.ftmi_lora_refresh_n(F, F, O, O, O, O, O, 0, 4, 32, 64, st), 0, "lora_refresh_n L = 0"),
        (lambda: lib.ftmi_lora_refresh_n(F, F, O, O, O, O, O, 1, 2, 32, 64, st), INV, "lora_refresh_n with 2 adapters"),
        (lambda: lib.ftmi_lora_refresh_n(F, F, O, O, O, O, O, 1, 4, 16, 64, st), UNS, "lora_refresh_n r = 16"),
        (lambda: lib.ftmi_transpose_bf16(X_, O, 0, 8, st), 0, "transpose rows = 0"),
        (lambda: lib.ftmi_transpose_bf16(X_, O, 8, 0, st), 0, "transpose cols = 0"),
        (lambda: lib.ftmi_transpose_bf16(X_, O, -8, 8, st), INV, "transpose rows < 0"),
        (lambda: lib.ftmi_timestep_sinusoid(F, O, 0, st), 0, "timestep_sinusoid B = 0"),
        (lambda: lib.ftmi_timestep_sinusoid(None, O, 1, st), INV, "timestep_sinusoid null"),
        (lambda: lib.ftmi_small_linear(X_, X_, X_, O, 9, 4, 8, 0, st), UNS, "small_linear rows = 9"),
        (lambda: lib.ftmi_small_linear(X_, X_, X_, O, 0, 4, 8, 0, st), UNS, "small_linear rows = 0"),
        (lambda: lib.ftmi_small_linear(X_, X_, X_, O, 2, 4, 12, 0, st), UNS, "small_linear K = 12"),
        (lambda: lib.ftmi_small_linear(X_, X_, X_, O, 2, 0, 8, 0, st), 0, "small_linear N = 0"),
        (lambda: lib.ftmi_ada_prep(X_, X_, O, 0, 2, 64, st), 0, "ada_prep L = 0"),
        (lambda: lib.ftmi_ada_prep(X_, X_, O, 1, 0, 64, st), 0, "ada_prep B = 0"),
        (lambda: lib.ftmi_ada_prep(X_, X_, O, 1, 2, -64, st), INV, "ada_prep D < 0"),
        (lambda: lib.ftmi_ada_out_prep(X_, X_, O, 0, 64, st), 0, "ada_out_prep B = 0"),
        (lambda: lib.ftmi_ada_out_prep(X_, X_, None, 2, 64, st), INV, "ada_out_prep null"),
    ]
    for fn, code, what in calls:
        rc = fn()
        assert rc == code, f"{what}: returned {rc}, expected {code} ({_lib.last_error()})"
    torch.cuda.synchronize()
    assert (ob == OUT_SENT).all() and (of == OUT_SENT).all(), "a refused or empty call wrote to its output"


# ---- CPU self-checks ----------------------------------------------------------------------------------

def _passes(p, outs, cap):
    try:
        judge_case("self-check " + tag_of(p), p, outs, cap=cap)
    except AssertionError:
        return False
    return True


def test_fp32_stand_ins_pass_every_bound(capsys):
    _threads()
    FIGURES.clear()
    for p in cpu_cases():
        judge_case("stand-in " + tag_of(p), p, stand_in(p), cap=STANDIN_CAP)
    with capsys.disabled():
        for op, (w, s) in sorted(FIGURES.items()):
            print(f"[elementwise] stand-in {op:14s} err/bound {w:.3f} block share {s:.4f}")


def test_fp32_stand_ins_pass_beyond_the_caps():
    """One case per capped kernel beyond its cap (the grid-stride pass), the stand-in against the fp64 reference."""
    _threads()
    for p in (mk_ddim(PER_BIG[-1], 1, 0, True), mk_posterior(PER_BIG[-2], 1), mk_mse(PER_MSE[-1], 3, True, True, 0.25), mk_sumsq(N_SUMSQ[-1], False),
              mk_opt("clip", N_OPT[-2], HYPER[0]), mk_opt("adamw", N_OPT[-2], HYPER[0]), mk_opt("adamw_bf16", N_OPT[-2], HYPER[0])):
        judge_case("stand-in " + tag_of(p), p, stand_in(p), cap=STANDIN_CAP)


FAULTS = [  # (fault, cases it must show in: at least one)
    ("tail_dropped", lambda: [mk_sumsq(n, pr) for n in (3, 5, 1027) for pr in (True, False)]),
    ("last_wg_dropped", lambda: [mk_sumsq(2051, True), mk_sumsq(2051, False), mk_mse(8 * 257, 1, False, False, 1.0)]),
    ("second_pass_dropped", lambda: [mk_sumsq(N_SUMSQ[-1], False), mk_mse(PER_MSE[-1], 1, False, False, 1.0), mk_ddim(PER_BIG[-2], 1, 0, True),
                                     mk_ddim(PER_BIG[-2], 1, 1, False), mk_posterior(PER_BIG[-2], 1), mk_opt("clip", N_OPT[-2], HYPER[0]),
                                     mk_opt("adamw", N_OPT[-2], HYPER[0]), mk_opt("adamw_bf16", N_OPT[-2], HYPER[0])]),
    ("partial_unscaled", lambda: [mk_mse(8, 1, False, False, 1.0), mk_mse(8 * 257, 3, True, True, 0.25)]),
    ("finish_store", lambda: [mk_mse(8 * 257, 1, False, False, 1.0), mk_mse(8, 3, True, False, 1.0)]),
    ("prev_sample", lambda: [mk_noise_pack(63, 65, 3, 1, True), mk_noise_pack(1, 1, 3, 0, False), mk_mse(8 * 255, 3, True, True, 1.0),
                             mk_ddim(8, 3, 0, True), mk_ddim(8 * 257, 3, 1, False)]),
    ("fft_le", lambda: [mk_noise_pack(65, 200, 1, 70, True), mk_noise_pack(64, 64, 3, 0, True), mk_noise_pack(1, 63, 1, 1, True)]),
    ("unrounded", lambda: [mk_noise_pack(65, 200, 3, 70, True), mk_ddim(8 * 255, 3, 0, True), mk_ddim(8 * 255, 1, 1, False),
                           mk_opt("adamw_bf16", 257, HYPER[0]), mk_small_linear(4, 2048, 520, True, True)]),
    ("lerp_ignored", lambda: [mk_opt("adamw_bf16", N_OPT[-2], HYPER[-2])]),  # the two forms differ after the bf16 rounding in about one element of 2^15
    ("coef_ge1", lambda: [mk_opt("adamw_bf16", 257, HYPER[1]), mk_opt("clip", 257, HYPER[1])]),
    ("maxnorm0_clips", lambda: [mk_opt("adamw_bf16", 257, HYPER[2]), mk_opt("clip", 257, HYPER[2])]),
    ("bc_powf", lambda: [mk_opt("adamw", 257, HYPER[9])]),
    ("lo_is_hi", lambda: [mk_lora_split(31, 33, ("ext", "t_ext")), mk_lora_split(32, 32, ("sp", "t_sp")), mk_lora_refresh(3)]),
    ("ext_off_cols", lambda: [mk_lora_split(31, 33, ("ext",)), mk_lora_split(33, 31, ("t_ext",))]),
    ("inner_ignored", lambda: [mk_lora_refresh(3), mk_lora_refresh(8)]),
    ("slot6_from_slot0", lambda: [mk_ada_prep(1, 1, 64), mk_ada_prep(3, 3, 2048)]),
    ("bias_dropped", lambda: [mk_small_linear(1, 1, 8, False, True), mk_small_linear(8, 2048, 256, True, True)]),
]


@pytest.mark.parametrize("fault,cases", FAULTS, ids=[f for f, _ in FAULTS])
def test_seeded_faults_fail(fault, cases):
    _threads()
    for p in cases():
        assert _passes(p, stand_in(p), STANDIN_CAP), f"{tag_of(p)}: the unfaulted stand-in does not pass"
        assert not _passes(p, stand_in(p, fault), STANDIN_CAP), f"{fault} is not seen by {tag_of(p)}"


def grid_of(op, p):
    """(workgroups along x, cap) of the case's launch, from the launchers' arithmetic."""
    if op in ("ddim", "posterior"):
        per = (p["a"] if op == "ddim" else p["eps"]).shape[1]
        return min((per // 8 + 255) // 256, 1024), 1024
    if op == "mse":
        return mse_blocks(p["pred"].shape[1]), 256
    if op == "sumsq":
        return sumsq_blocks(p["g"].numel()), 2048
    if op in ("clip", "adamw", "adamw_bf16"):
        return min((p["g"].numel() + 255) // 256, 4096), 4096
    raise KeyError(op)


def test_the_cases_reach_every_path():
    cases = cpu_cases(big=True)
    for op, cap_elems in (("ddim", 2048), ("posterior", 2048), ("mse", 2048), ("sumsq", 1024), ("clip", 256), ("adamw", 256), ("adamw_bf16", 256)):
        mine = [p for p in cases if p["op"] == op]
        sizes = {(p["a"].shape[1] if op == "ddim" else p["eps"].shape[1] if op == "posterior" else p["pred"].shape[1] if op == "mse" else p["g"].numel())
                 for p in mine}
        grids = {grid_of(op, p) for p in mine}
        cap = next(iter(grids))[1]
        assert (1, cap) in grids, f"{op}: no case with one workgroup"
        assert cap * cap_elems in sizes, f"{op}: no case at exactly the cap"
        assert any(s > cap * cap_elems for s in sizes), f"{op}: no case beyond the cap"
        assert any(cap_elems < s < cap * cap_elems and s % cap_elems for s in sizes), f"{op}: no ragged last workgroup"
    assert {p["x"].shape[0] for p in cases if p["op"] == "small_linear"} == set(range(1, 9)), "small_linear templates"
    assert {p["w"].shape[0] for p in cases if p["op"] == "small_linear"} >= {1, 4, 5, 2048}
    assert {p["x"].shape[1] for p in cases if p["op"] == "small_linear"} >= {8, 256, 512, 520, 2048}
    assert {n % 4 for n in N_SUMSQ} == {0, 1, 2, 3}, "sumsq tails"
    for n in N_SUMSQ:
        assert len(probe_positions(n)) <= 12 and (n < 4 or {0, 3, n - 1} <= set(probe_positions(n)))
    assert {hyper_id(size_hyper(k)) for k in range(len(N_OPT))}.__len__() == len(N_OPT)


def test_the_sweep_reads_boundary_distances():
    """The sweep machinery on the host: a value 1 + 2^-8 (1 - 2^-10) lies 2^-18 (relative to ~1) below a bf16 boundary; an output rounded the other way is counted with
    that distance, outputs that agree are not counted."""
    v = torch.tensor([1.0 + 2.0**-8 * (1.0 - 2.0**-10), 3.0, -(0.75 + 2.0**-9 + 2.0**-30)], dtype=f64)
    d = boundary_distance(v)
    assert abs(d[0].item() - 2.0**-18 / v[0].item()) < 1e-12 and abs(d[1].item() - 2.0**-7 / 3.0) < 1e-12 and abs(d[2].item() - 2.0**-30 / 0.75) < 1e-10
    got = torch.tensor([1.0 + 2.0**-7, 3.0, -0.75], dtype=f32).to(bf16)  # the first and the third rounded the wrong way
    fig, cnt = sweep_figure(got, v)
    assert cnt == 2 and abs(fig - d[0].item()) < 1e-15
    h, x, t = sweep_inputs()
    assert min(h.numel(), x.numel(), t.numel()) >= 2**18 and h.numel() % 8 == 0 and x.numel() % 16384 == 0
    assert float(h.float().min()) == -15.0 and float(h.float().max()) == 10.0 and float(x.float().abs().max()) == 20.0 and float(t.max()) <= 1000.0
