"""The launch contract of the sampling, layout and cast kernels (csrc/sample_layout.hip, ltx_sample.hip, wan_control.hip, cast.hip and cog_patch_permute of
cogvideox.hip) per element against fp64, bit for bit.

CONTRACT (read from the kernels; bf() = round to nearest even to bf16, every other operation one IEEE fp32 operation, -ffp-contract=off, no fast-math;
          fma() = __builtin_fmaf, one rounding)
  EXACT class: all of them.  The reference is the fp64 expression rounded to fp32 after each operation (fma: see REFERENCE); the comparison is bitwise.
    wan_sample_init / cog_sample_init   x [B, S, Kc] = the latents, an exact copy, column c pv + dt ph pw + dy pw + dx of token (f', h', w') = latent (c, f' pt + dt,
                      h' ph + dy, w' pw + dx), pv = pt ph pw (Wan: latents [B, C, F, H, W]; CogVideoX: [B, F, C, H, W]);  cols [P B S, copies Kp]: in every one of the P
                      row groups and `copies` copies, columns [0, Kc) = bf(x), [Kc, Kc + Kx) the extra bf16 channels in the same order (a copy of their bits),
                      [Kc + Kx, Kp) = +0
    wan_sample_step   d = c - u; v = fma(g, d, u) (guidance 1: v = c, pred has one half);  dt = sigma_next[b] - sigma[b];  x <- fma(dt, v, x);  bf(x) to columns [0, Kc) of
                      every row group and copy of cols, the other columns untouched.  State column c pv + p takes pred column p C + c of the same token.
                      pred == NULL: only the copies (x untouched);  cols == NULL: only the update.  A workgroup's 2048 elements are whole tokens (2048 % Kc == 0).
    cog_sample_step   the same combine;  x <- fma(cx, x, cv v), (cx, cv) = coef[2 step], coef[2 step + 1];  pred in the state's own column order
    cfg_euler_step    the same combine and Euler update on [B, per_sample];  held prefix: the first `hold` elements of every sample are not updated and pred is not
                      read there, only bf(x) goes to both halves of x_next
    wan_sample_finish latents [B, C, F, H, W] = bf(x std[c] + mean[c]): a product, a sum, one bf16 rounding (NOT an fma)
    cog_sample_finish latents [B, F - drop, C, H, W] = bf(x k) (-0 stays -0); the first `drop` frames are not written
    unpack_denorm     out [B, C, S] = bf(x[B, S, C] std[c] + mean[c]), the same affine
    wan_sample_mod    mod [L, rows, 6 D] = float(table_l) + float(tproj), the same values in every one of the `rows` rows
    wan_control_pack  z = bf((mu - mean) istd);  noisy = bf((1 - sigma_b) z + sigma_b n) (a difference, two products, a sum);  target = bf(n - z);
                      ctrl = bf((mu_ctrl - mean) istd) for f < Fc, its magnitude cleared (sign kept) where keep[b, f] == 0, +0 for f >= Fc;  cols2 [B S, 2 Kp],
                      Kp = 2 C pv: channel c -> noisy, channel C + c -> ctrl, both written to both halves
    fp8_upcast        the e4m3fn -> bf16 table (exact; 0x7f / 0xff -> NaN, subnormals m 2^-9 kept), plain [rows cols] and transposed [cols, rows]
    cog_patchify / cog_unpatchify   tokens[b, (f h + hy) w + wx, (c p + py) p + px] <-> lat[b, f, c, hy p + py, wx p + px]: a permutation
    f32_gemm          acc = 0; acc = fma(a[m, k], b[k, n], acc) for k = 0 .. K - 1;  v = scale acc;  accumulate: v = old + v;  c[m ldc + n] = v;
                      planes: hl[m ld_hl + n] = bf(v), hl[m ld_hl + N + n] = bf(v - bf(v)).  The operand fetch mode (0: k contiguous, 16-byte loads; 1: the outer
                      index contiguous; 2: scalar loads) follows from pointer alignment and strides and does not change a bit of the result.
                      Besides the bitwise check the order-independent bound |got - exact| <= (K + 2) u |scale| (|a| |b|) + 2 u |c| is kept, so that a failure
                      says which of the two broke (a changed accumulation order breaks the bits and keeps the bound).
  REFUSALS AND ZERO SIZES (REFUSALS below; every one returns before any launch, tested on the host with pointers that are never read)
    FTMI_ERR_INVALID      a null tensor; misaligned pointers (16 bytes; f32_gemm planes 8) in every launcher of the family except wan_control_pack (element accesses);
                          an extent <= 0 (the family's zero-size rule: an empty extent is refused, except f32_gemm M or N = 0 and fp8_upcast rows or cols <= 0,
                          which return 0); copies not 1 / 2; P not 1 / 2; Kc != po; Kc + Kx > Kp; extra channels without their tensor and the reverse; P and
                          guidance disagreeing; sigma / coef missing or step < 0 with a pred; drop < 0 or >= pt; hold < 0 or > per_sample; ldc < N, ldc % 4,
                          ld_hl < 2 N, ld_hl % 4; a null or misaligned table of wan_sample_mod
    FTMI_ERR_UNSUPPORTED  a latent size that is not whole patches (cog_patch_permute: INVALID); Kc % 8, Kx % 8, Kp % 8; 2048 % Kc; Kc > 2048; pt > 2 (CogVideoX);
                          a row of patches beyond the 64 KiB of LDS; per_sample % 8, hold % 8; C % 4 (unpack_denorm); B > 65535 (unpack_denorm); L > 40 and
                          6 D % 8 (wan_sample_mod); M, N or K % 64; rows cols % 16 (fp8 plain), rows or cols % 64 (fp8 transposing)
    "the latents must be a whole number of 16-byte vectors" (launch_limits) cannot fire: B C F H W = B Kc S with Kc % 8 == 0.
  FIXED WITH THIS TEST  fp8_upcast checked no alignment although both kernels move 16-byte vectors: it now refuses a misaligned src or dst (no caller passes one:
    hunyuan_video/block.py offsets its arenas by sums of element counts that are multiples of 16).  cog_patch_permute accepted H <= 0 and W <= 0 (an empty or
    negative grid); it now refuses them like B, F, C <= 0.  Both are host checks, see test_refusals_return_before_any_launch; no seeded fault stands for them
    (they change no result).  No kernel differed from its contract.
  NOT REACHABLE through the C ABI, so not covered here: sig_stride = 0 (ftmi_wan_sample_step and ftmi_ltx_cfg_euler_step* pass 1; the one-call loops pass 0) and
    x_next == NULL with a held prefix (both entry points refuse a null x_next).  The loops' composition tests in test_gpu_*_sampling.py run those paths.

REFERENCE  one function per launcher (c_*), run on fp64 tensors (the reference) and on fp32 tensors (the stand-in of the CPU self-checks).  The layout launchers have two
  independent forms: the reference is a reshape / permute of the whole tensor, the stand-in computes every address with the kernels' formulas (col_src, run_start),
  which is also where the seeded loop faults live.
  fp32 fma: the fp64 product of two fp32 numbers is exact; the addend is added with a TwoSum; when the error term is non-zero the fp64 sum is moved to the neighbour
  with an odd last bit (round to odd); rounding that to fp32 is the correctly rounded fma.  Validated by test_fma_emulation against fractions.Fraction on 12 000
  random and tie-seeking triples (this interpreter has no math.fma; where one exists it is compared too), so no launcher had to move to a bounded class.  The
  stand-in uses the same fma (torch has no fused fp32 multiply-add on the CPU); every other operation of the stand-in is torch's own fp32 operation.

CASES (the smallest shapes that reach each condition; test_the_cases_reach_every_path computes the conditions from the launch formulas)
  init / finish   LAYOUT_CASES: Wan t2v / i2v / control and two more patch shapes, CogVideoX pt 1 / 2, B and P in {1, 2}; staging loop > 1 pass (W = 32), extra staging
                  > 1 pass (Cx = 20, W = 52), gather loop > 1 pass (W = 66 at Kp 64, W = 34 at Kp 128 x 2 copies, W = 22 at Kp 192), bf16 run start & 7 in {0, 2, 4, 6}
                  (patch (1, 1, 2), W = 10), fp32 run start & 3 in {0, 1, 2, 3} (patch (1, 1, 1), W = 5, H = 4), finish vector path > 1 pass (W = 68), element path > 1
                  pass, drop = 1 with pt = 2 over two rows of patches and B = 2, the real row W = 104, H = 4, F = 2
  wan / cog step  Kc in {16, 64, 128, 2048}; S Kc % 2048 != 0 with B = 3 and three sigma pairs; n8 % 256 != 0; guidance 1 / 5; pred NULL; cols NULL; copies 1 / 2;
                  CogVideoX step 0 and 3 of a 4-entry table
  cfg_euler_step  (B, per) in {(2, 344064), (3, 2368), (1, 8)} x guidance {1, 3, 7.5}; hold in {0, 8, per - 8, per} and 1000 (no multiple of 2048)
  unpack_denorm   C {4, 60, 64, 68, 128} x S {1, 7, 8, 63, 64, 65, 72, 200} x B {1, 3}
  wan_sample_mod  L {1, 3, 40} x rows {1, 2} x D {64, 1536, 100 (6 D / 8 = 75)}, every table its own allocation
  control_pack    B = 3, patch (1, 2, 2) / (2, 2, 2), Fc {1, F - 1, F}, keep all / frame 0 / first and last / none, W {6, 34}
  f32_gemm        the nine (mode_a, mode_b) pairs at 64^3, mode 2 by stride and by pointer; M, N {64, 128, 192}, K {64, 192, 320}; scale {1, 0.3}; accumulate;
                  ldc = N + 4; planes with ld_hl = 2 N + 8; M = 0, N = 0 (refusal table)
  fp8_upcast      all 256 bytes; plain n {16, 4080, 4096 256 16 + 16 300}; transposing rows, cols {64, 128, 192} into a view of an arena
  cog_patchify    p {1, 2}, W / p odd, B {1, 2}, one shape past 8192 256 elements; both directions
  Data: seeded; exact zeros, -0 and bf16 ties (1 + 2^-8, 1 + 3 2^-8, both signs) in latents and states, a zero prediction under them so that the step's fma lands on
  the tie; mean / std no powers of two, and states x = (T - mean) / std that put the two-operation affine on a bf16 tie T which the exact value misses (affine_ties).  Inputs lie between IN_SENT padding (init reads whole 16-byte vectors inside its tensor), outputs and tensors updated
  in place between OUT_SENT padding that must survive; untouched columns of cols keep OUT_SENT; every launch runs twice and gives the same bits.

CPU SELF-CHECKS  test_fp32_stand_ins_pass_every_case (bitwise); test_seeded_faults_fail (FAULTS: each fault of the stand-in is rejected by every case listed);
  test_fma_emulation; test_the_cases_reach_every_path; test_refusals_return_before_any_launch.
  stage_pass2 / xstage_pass2 / gather_pass2 / fin_read_pass2 / fin_store_pass2 / upcast_pass2 / permute_pass2   the second pass of a 256-stride loop dropped
  residue / xresidue        run_start & 3 / & 7 ignored when reading the staged runs
  group2                    second row group (P = 2) or second copy not written: init, steps, mod rows, control_pack halves
  extra_copy0 / pad_kept    extra columns in copy 0 only; padding columns not zeroed
  no_perm                   pred read in the state's column order (Wan)
  prev_sample / stride0     sigma of sample b - 1; sigma[0] for every sample
  hold_off / held_updated   hold boundary one vector late; held x updated
  drop_shifted              the dropped frames shifted, not dropped
  affine_fma / plus0        the affine as one fma; x k + 0
  pitch                     the finish store reads its LDS with the run length as pitch
  lo_half_ld / lo_is_hi     f32_gemm planes: lo at ld_hl / 2; hi written twice
  k_desc / two_partial      f32_gemm accumulation order: seen by the bitwise check ONLY, the bound passes (asserted)
  other_strides             an operand read with the other mode's strides (the transpose)
  scale_after               scale applied to old + acc
  keep_prev / sign_dropped  control_pack: keep mask of frame f - 1; +0 for a dropped frame
  nan_inf / sub_flushed     fp8 table: NaN codes as infinity; subnormals flushed

MEASURED on an MI355X (every launcher of the family is of the exact class: "exact" = no element of any output of any case differs from the reference in a bit;
  342 outputs over all cases, sentinels intact, both launches equal)
  launcher (outputs)                            MI355X        fp32 stand-in on the CPU
  wan_sample_init, cog_sample_init (x, cols)    exact         exact
  wan_sample_step, cog_sample_step (x, cols)    exact         exact
  cfg_euler_step (x, x_next)                    exact         exact
  wan_sample_finish, cog_sample_finish          exact         exact
  unpack_denorm                                 exact         exact
  wan_sample_mod                                exact         exact
  wan_control_pack (cols2, target)              exact         exact
  f32_gemm (c, planes)                          exact         exact
            largest err / order-independent bound   0.062     0.062 (the same bits)
  fp8_upcast (plain, transposing)               exact         exact
  cog_patchify, cog_unpatchify                  exact         exact
  Not measured: sig_stride = 0 and x_next == NULL with a held prefix (see NOT REACHABLE).
"""

import ctypes
import fractions
import math

import pytest
import torch

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0**-24
IN_SENT = 3.0e4     # padding of the inputs: wrecks the result if read as data
OUT_SENT = -1536.0  # padding of the outputs (exact in bf16 and fp32): must survive the launch
PAD = 64            # elements of padding on either side (keeps the 16-byte alignment)
JUNK = 777.0        # what a seeded fault leaves where the kernel would read an LDS slot that nobody wrote
INVALID, UNSUPPORTED = -1, -2


def _threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))


def f32v(x):
    """The fp32 value of a Python number, as the C entry point receives it."""
    return float(torch.tensor(x, dtype=f32))


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------------
# arithmetic: tensors hold fp32 values, in fp64 (reference) or fp32 (stand-in)

def fma32(a, b, c):
    """The correctly rounded fp32 fma of fp32 values (any float dtype), as an fp32 tensor: exact product, TwoSum, round to odd, round to fp32."""
    a, b, c = torch.broadcast_tensors(*(torch.as_tensor(t).double() for t in (a, b, c)))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.contiguous().view(torch.int64)
    fix = (err != 0) & ((bits & 1) == 0)
    grow = (err > 0) == (s > 0)  # the exact sum lies further from zero than s
    one = torch.ones_like(bits)
    bits = torch.where(fix, bits + torch.where(grow, one, -one), bits)
    return bits.view(f64).float()


def X(dt):
    """(lift, r, fma): r rounds to fp32 after one operation (the identity on fp32 tensors)."""
    if dt is f64:
        return (lambda t: t.double()), (lambda t: t.float().double()), (lambda a, b, c: fma32(a, b, c).double())
    return (lambda t: t.float()), (lambda t: t), fma32


def bf(t):
    """bf16 of fp32 values: one rounding to nearest even."""
    return t.float().to(bf16)


def prev_sample(B):
    return (torch.arange(B) - 1) % B


# ----------------------------------------------------------------------------------------------------
# the layout (sample_layout.hip: Lay, lay_derive, wan_lay / cog_lay)

def mk_geo(model, B, P, F, H, W, C=16, Cx=0, patch=(1, 2, 2), Kp=None, copies=1, drop=0):
    pt, ph, pw = patch
    pv = pt * ph * pw
    Kc, Kx = C * pv, Cx * pv
    g = dict(model=model, B=B, P=P, F=F, H=H, W=W, C=C, Cx=Cx, pt=pt, ph=ph, pw=pw, Kp=Kp or Kc, copies=copies, drop=drop, pv=pv, Kc=Kc, Kx=Kx)
    g["ld"] = copies * g["Kp"]
    g["fpn"], g["hpn"], g["wpn"] = F // pt, H // ph, W // pw
    g["S"] = g["fpn"] * g["hpn"] * g["wpn"]
    g["seg"] = ph * W
    g["pitch_f"] = 4 * ((g["seg"] + 3) // 4 + 1)
    g["pitch_h"] = 8 * ((g["seg"] + 7) // 8 + 1)
    g["sc"], g["sf"] = (F * H * W, H * W) if model == "wan" else (H * W, C * H * W)
    assert F % pt == 0 and H % ph == 0 and W % pw == 0 and Kc % 8 == 0 and Kx % 8 == 0 and g["Kp"] % 8 == 0 and Kc + Kx <= g["Kp"]
    assert (model == "cog" or 2048 % Kc == 0) and lds_bytes(g, True) <= 65536
    return g


def lds_bytes(g, init):
    return g["C"] * g["pt"] * g["pitch_f"] * 4 + g["Cx"] * g["pt"] * g["pitch_h"] * 2 if init else g["C"] * g["pt"] * g["pitch_h"] * 2


def patchify(t, g):
    """[B, n, F', H, W] -> [B, S', n pv]: the reference's form, a reshape and a permute."""
    B, n, F, H, W = t.shape
    pt, ph, pw = g["pt"], g["ph"], g["pw"]
    return t.reshape(B, n, F // pt, pt, H // ph, ph, W // pw, pw).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, -1, n * pt * ph * pw)


def unpatchify(x, g, n, F):
    B = x.shape[0]
    pt, ph, pw, H, W = g["pt"], g["ph"], g["pw"], g["H"], g["W"]
    return x.reshape(B, F // pt, H // ph, W // pw, n, pt, ph, pw).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(B, n, F, H, W)


def lay_index(g, nch, frames, first):
    """The kernels' addresses (col_src, run_start) for every (b, f', h', w, k): int64 tensors [B, fpn, hpn, wpn, nch pv]."""
    b, fp, hp, w, k = torch.meshgrid(torch.arange(g["B"]), torch.arange(g["fpn"]), torch.arange(g["hpn"]), torch.arange(g["wpn"]), torch.arange(nch * g["pv"]),
                                     indexing="ij")
    pp = g["ph"] * g["pw"]
    run, rem = k // pp, k % pp
    off = (rem // g["pw"]) * g["W"] + w * g["pw"] + rem % g["pw"]
    c, dtt = run // g["pt"], run % g["pt"]
    start = b * nch * frames * g["H"] * g["W"] + c * g["sc"] + (fp * g["pt"] + dtt - first) * g["sf"] + hp * g["ph"] * g["W"]
    return dict(w=w, k=k, run=run, off=off, c=c, start=start, frame=fp * g["pt"] + dtt)


def _staged(src, g, nch, vec, pitch, fault, fresidue, fpass2):
    """The stand-in's read of a latent tensor through the staged runs: vec elements per 16-byte vector."""
    ix = lay_index(g, nch, g["F"], 0)
    res = ix["start"] & (vec - 1)
    flat = ix["start"] + ix["off"] - (res if fault == fresidue else 0)
    v = src.flatten()[flat]
    if fault == fpass2:
        sidx = ix["run"] * (pitch // vec) + (res + ix["off"]) // vec
        v = torch.where(sidx >= 256, torch.full_like(v, JUNK), v)
    return v.reshape(g["B"], g["S"], nch * g["pv"])


def c_init(p, dt, fault=None):
    g = p["geo"]
    B, S, Kc, Kx, Kp, P, copies = (g[k] for k in ("B", "S", "Kc", "Kx", "Kp", "P", "copies"))
    if dt is f64:
        x = patchify(p["lat"] if g["model"] == "wan" else p["lat"].transpose(1, 2), g)
        ex = patchify(p["extra"], g) if g["Cx"] else None
    else:
        x = _staged(p["lat"], g, g["C"], 4, g["pitch_f"], fault, "residue", "stage_pass2")
        ex = _staged(p["extra"], g, g["Cx"], 8, g["pitch_h"], fault, "xresidue", "xstage_pass2") if g["Cx"] else None
    x = x.float().clone()
    row = torch.zeros((B, S, Kp), dtype=bf16)
    row[..., :Kc] = bf(x)
    if ex is not None:
        row[..., Kc:Kc + Kx] = ex
    if fault == "pad_kept":
        row[..., Kc + Kx:] = OUT_SENT
    cols = row[None, :, :, None, :].expand(P, B, S, copies, Kp).clone()
    if fault == "extra_copy0" and copies == 2:
        cols[:, :, :, 1, Kc:Kc + Kx] = OUT_SENT
    if fault == "gather_pass2":
        lost = (torch.arange(g["wpn"])[:, None] * (Kp // 8) + torch.arange(Kp)[None] // 8) >= 256  # [wpn, Kp]
        lost = lost[None, None].expand(g["fpn"], g["hpn"], g["wpn"], Kp).reshape(S, Kp)
        cols[:, :, lost.nonzero()[:, 0], :, lost.nonzero()[:, 1]] = OUT_SENT
        lx = lost[:, :Kc]
        x[:, lx.nonzero()[:, 0], lx.nonzero()[:, 1]] = OUT_SENT
    if fault == "group2":
        if P == 2:
            cols[1] = OUT_SENT
        elif copies == 2:
            cols[:, :, :, 1] = OUT_SENT
    return {"x": x, "cols": cols.reshape(P, B, S, copies * Kp)}


def c_finish(p, dt, fault=None):
    g = p["geo"]
    L, r, fma = X(dt)
    B, C, F, H, W, S, Kc, drop, seg = (g[k] for k in ("B", "C", "F", "H", "W", "S", "Kc", "drop", "seg"))
    wan = g["model"] == "wan"

    def affine(v, c):
        if wan:
            sd, mn = L(p["std"])[c], L(p["mean"])[c]
            return fma(v, sd, mn) if fault == "affine_fma" else r(r(v * sd) + mn)
        return r(r(v * p["k"]) + 0.0) if fault == "plus0" else r(v * p["k"])

    if dt is f64:
        xc = unpatchify(L(p["x"]), g, C, F)
        out = bf(affine(xc, torch.arange(C)[None, :, None, None, None].expand_as(xc)))
        return {"out": out if wan else out[:, :, drop:].transpose(1, 2).contiguous()}
    shifted = fault == "drop_shifted"
    ix = lay_index(g, C, F - drop, 0 if shifted else drop)
    vals = bf(affine(L(p["x"]).reshape(ix["c"].shape), ix["c"]))
    if fault == "fin_read_pass2":
        vals = torch.where(ix["w"] * (Kc // 4) + ix["k"] // 4 >= 256, torch.full_like(vals, JUNK), vals)
    if fault == "pitch":  # the LDS [run][pitch_h] read back with the run length as pitch
        shp = vals.shape
        lds = torch.full(shp[:3] + (C * g["pt"] * g["pitch_h"],), JUNK, dtype=bf16)
        lds.scatter_(3, (ix["run"] * g["pitch_h"] + ix["off"]).reshape(shp[:3] + (-1,)), vals.reshape(shp[:3] + (-1,)))
        vals = lds.gather(3, (ix["run"] * seg + ix["off"]).reshape(shp[:3] + (-1,))).reshape(shp)
    kept = (ix["frame"] < F - drop) if shifted else (ix["frame"] >= drop)
    if fault == "fin_store_pass2":
        sidx = ix["run"] * (seg // 8) + ix["off"] // 8 if seg % 8 == 0 else ix["run"] * seg + ix["off"]
        kept = kept & (sidx < 256)
    out = torch.full((B * C * (F - drop) * H * W,), OUT_SENT, dtype=bf16)
    out[(ix["start"] + ix["off"])[kept]] = vals[kept]
    return {"out": out.reshape((B, C, F, H, W) if wan else (B, F - drop, C, H, W))}


def c_step(p, dt, fault=None):
    """wan_sample_step / cog_sample_step / cfg_euler_step: x [B, n]; pred [P B, n] or None; the copies [P, B, rows, ld] or None."""
    L, r, fma = X(dt)
    kind, B, P = p["kind"], p["x"].shape[0], p["P"]
    x = L(p["x"])
    n = x.shape[1]
    xn = x
    if p["pred"] is not None:
        pr = L(p["pred"]).reshape(P, B, n)
        v = fma(p["g"], r(pr[1] - pr[0]), pr[0]) if P == 2 else pr[0]
        if kind == "wan" and fault != "no_perm":
            g = p["geo"]
            v = v.reshape(B, g["S"], g["pv"], g["C"]).transpose(2, 3).reshape(B, n)
        if kind == "cog":
            cx, cv = (float(p["coef"][2 * p["step"] + i]) for i in (0, 1))
            xn = fma(cx, x, r(cv * v))
        else:
            sg, sn = L(p["sigma"]), L(p["sigma_next"])
            if fault == "prev_sample":
                sg, sn = sg[prev_sample(B)], sn[prev_sample(B)]
            if fault == "stride0":
                sg, sn = sg[:1].expand(B), sn[:1].expand(B)
            xn = fma(r(sn - sg)[:, None], v, x)
        hold = p.get("hold", 0) + (8 if fault == "hold_off" else 0)
        if hold and fault != "held_updated":
            xn = xn.clone()
            xn[:, :hold] = x[:, :hold]
    out = {"x": xn.float()}
    if p["want_copies"]:
        rows, Kc, Kp, copies = p["rows"], n // p["rows"], p["Kp"], p["copies"]
        cols = torch.full((P, B, rows, copies, Kp), OUT_SENT, dtype=bf16)
        cols[..., :Kc] = bf(xn).reshape(1, B, rows, 1, Kc)
        if fault == "group2":
            if P == 2:
                cols[1] = OUT_SENT
            elif copies == 2:
                cols[:, :, :, 1] = OUT_SENT
        out["cols"] = cols.reshape(P, B, rows, copies * Kp)
    return out


def c_unpack(p, dt, fault=None):
    L, r, fma = X(dt)
    x, sd, mn = L(p["x"]), L(p["std"])[None, None], L(p["mean"])[None, None]
    v = fma(x, sd, mn) if fault == "affine_fma" else r(r(x * sd) + mn)
    return {"out": bf(v).transpose(1, 2).contiguous()}


def c_mod(p, dt, fault=None):
    L, r, _ = X(dt)
    s = r(L(torch.stack(p["tables"])) + L(p["tproj"])[None]).float()  # [L, 6 D]
    out = s[:, None].expand(-1, p["rows"], -1).clone()
    if fault == "group2" and p["rows"] == 2:
        out[:, 1] = OUT_SENT
    return {"mod": out}


def c_pack(p, dt, fault=None):
    L, r, _ = X(dt)
    g = p["geo"]  # a Wan layout with Cx = C, copies = 2
    B, C, F, Fc = g["B"], g["C"], g["F"], p["Fc"]
    mean, istd = L(p["mean"])[None, :, None, None, None], L(p["istd"])[None, :, None, None, None]
    z = L(bf(r(r(L(p["moments"])[:, :C] - mean) * istd)))
    nz, sg = L(p["noise"]), L(p["sigmas"])[:, None, None, None, None]
    noisy = bf(r(r(r(1.0 - sg) * z) + r(sg * nz)))
    target = bf(r(nz - z))
    ctrl = torch.zeros_like(noisy)
    cv = bf(r(r(L(p["control"])[:, :C] - mean) * istd))
    keep = p["keep"][:, (torch.arange(F) - 1) % F] if fault == "keep_prev" else p["keep"]
    dropped = (keep[:, :Fc] == 0)[:, None, :, None, None].expand_as(cv)
    zero = torch.zeros_like(cv) if fault == "sign_dropped" else (cv.view(torch.int16) & -32768).view(bf16)
    ctrl[:, :, :Fc] = torch.where(dropped, zero, cv)
    row = patchify(torch.cat([noisy, ctrl], 1), g)  # [B, S, Kp]
    cols2 = torch.stack([row, row], 2)
    if fault == "group2":
        cols2[:, :, 1] = OUT_SENT
    return {"cols2": cols2.reshape(B * g["S"], 2 * row.shape[-1]), "target": target}


def fp8_table(fault=None):
    """e4m3fn byte -> value, from the format's definition: (-1)^s (1 + m / 8) 2^(e - 7), e = 0: m 2^-9, 0x7f / 0xff: NaN."""
    t = torch.zeros(256, dtype=f64)
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 15, b & 7
        v = m * 2.0**-9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
        if e == 0 and fault == "sub_flushed":
            v = 0.0
        if (b & 0x7f) == 0x7f:
            v = math.inf if fault == "nan_inf" else math.nan
        t[b] = -v if s else v
    return t


def c_fp8(p, dt, fault=None):
    src = p["src"]  # uint8 [rows, cols]
    out = fp8_table(fault).to(dt)[src.long()].to(bf16)
    if p["transpose"]:
        return {"out": out.t().contiguous()}
    out = out.flatten()
    if fault == "upcast_pass2":
        out[4096 * 256 * 16:] = OUT_SENT
    return {"out": out}


def c_permute(p, dt, fault=None):
    B, F, C, H, W, pp = p["dims"]
    src = p["src"]
    if dt is f64:
        if p["to_tokens"]:
            out = src.reshape(B, F, C, H // pp, pp, W // pp, pp).permute(0, 1, 3, 5, 2, 4, 6)
        else:
            out = src.reshape(B, F, H // pp, W // pp, C, pp, pp).permute(0, 1, 4, 2, 5, 3, 6)
        return {"out": out.reshape(-1).clone()}
    i = torch.arange(src.numel())
    E, h, w = C * pp * pp, H // pp, W // pp
    e, t = i % E, i // E
    wx, t = t % w, t // w
    hy, t = t % h, t // h
    f, b = t % F, t // F
    px, py, c = e % pp, (e // pp) % pp, e // (pp * pp)
    li = (((b * F + f) * C + c) * H + (hy * pp + py)) * W + (wx * pp + px)
    out = torch.full((src.numel(),), OUT_SENT, dtype=bf16)
    live = i < (8192 * 256 if fault == "permute_pass2" else src.numel())
    if p["to_tokens"]:
        out[i[live]] = src.flatten()[li[live]]
    else:
        out[li[live]] = src.flatten()[i[live]]
    return {"out": out}


def c_gemm(p, dt, fault=None):
    L, r, fma = X(dt)
    a, b = L(p["a"]), L(p["b"])  # [M, K], [K, N]
    M, K = a.shape
    N = b.shape[1]
    if fault == "other_strides":
        a = a.t()
    order = range(K - 1, -1, -1) if fault == "k_desc" else range(K)
    accs = [torch.zeros((M, N), dtype=dt), torch.zeros((M, N), dtype=dt)]
    for k in order:
        i = 1 if (fault == "two_partial" and k >= K // 2) else 0
        accs[i] = fma(a[:, k, None], b[None, k, :], accs[i])
    acc = r(accs[0] + accs[1]) if fault == "two_partial" else accs[0]
    old = L(p["c0"])
    if fault == "scale_after" and p["accumulate"]:
        v = r(p["scale"] * r(old + acc))
    else:
        v = r(p["scale"] * acc)
        if p["accumulate"]:
            v = r(old + v)
    c = torch.full((M, p["ldc"]), OUT_SENT, dtype=f32)
    c[:, :N] = v.float()
    out = {"c": c}
    if p["planes"]:
        hi = bf(v)
        lo = hi if fault == "lo_is_hi" else bf(r(v - L(hi)))
        hl = torch.full((M, p["ld_hl"]), OUT_SENT, dtype=bf16)
        at = p["ld_hl"] // 2 if fault == "lo_half_ld" else N
        hl[:, :N] = hi
        hl[:, at:at + N] = lo
        out["hl"] = hl
    return out


CONTRACT = {"init": c_init, "finish": c_finish, "step": c_step, "unpack": c_unpack, "mod": c_mod, "pack": c_pack, "fp8": c_fp8, "permute": c_permute, "gemm": c_gemm}


def reference(p):
    return CONTRACT[p["op"]](p, f64)


def stand_in(p, fault=None):
    return CONTRACT[p["op"]](p, f32, fault)


# ----------------------------------------------------------------------------------------------------
# the check

def bits(t):
    return t.contiguous().view({bf16: torch.int16, f32: torch.int32, torch.uint8: torch.uint8}[t.dtype])


FIGURES = {}  # launcher -> [elements that differ, largest err / bound of f32_gemm]


def judge_case(tag, p, outs, R=None):
    """Bitwise against the reference (NaN matches NaN); f32_gemm's order-independent bound first, so that the message says which of the two broke."""
    R = R or reference(p)
    assert set(outs) == set(R), (sorted(outs), sorted(R))
    fig = FIGURES.setdefault(p["op"] + (":" + p["kind"] if "kind" in p else ""), [0, 0.0])
    if p["op"] == "gemm":
        M, N = p["a"].shape[0], p["b"].shape[1]
        a, b = p["a"].double(), p["b"].double()
        exact = p["scale"] * (a @ b) + (p["c0"].double() if p["accumulate"] else 0.0)
        bound = (p["a"].shape[1] + 2) * U * abs(p["scale"]) * (a.abs() @ b.abs()) + 2 * U * exact.abs()
        err = (outs["c"][:, :N].double() - exact).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        fig[1] = max(fig[1], worst)
        print(f"[sampling] {tag} c: max_err_over_bound={worst:.3f}")
        assert (err <= bound).all(), f"bound: {tag}: {int((err > bound).sum())} of {M * N} elements over the order-independent bound (worst {worst:.3f})"
    for name, ref in R.items():
        got = outs[name].reshape(ref.shape)
        assert got.dtype == ref.dtype, (name, got.dtype, ref.dtype)
        bad = (bits(got) != bits(ref)) & ~(torch.isnan(got.float()) & torch.isnan(ref.float()))
        fig[0] += int(bad.sum())
        print(f"[sampling] {tag} {name}: differing={int(bad.sum())} of {bad.numel()}")
        if bad.any():
            i = tuple(int(t[0]) for t in bad.nonzero(as_tuple=True))
            raise AssertionError(f"bits: {tag} {name}: element {list(i)} got {got[i].item():.9g} ref {ref[i].item():.9g}; {int(bad.sum())} of {bad.numel()} elements differ")


# ----------------------------------------------------------------------------------------------------
# inputs

SPECIALS = [0.0, -0.0, 1.0 + 2.0**-8, 1.0 + 3 * 2.0**-8, -(1.0 + 2.0**-8), -(2.0 + 3 * 2.0**-7), 2.0**-8 + 2.0**-17, -3.0]  # zeros and bf16 ties


def vals32(shape, g, scale=1.0):
    t = torch.randn(shape, generator=g) * scale
    flat = t.reshape(-1)
    if flat.numel() >= 8:
        flat[:8] = torch.tensor(SPECIALS)
        flat[-8:] = torch.tensor(SPECIALS).flip(0)
    return t


def rbf(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(bf16)


def affine_params(C, g):
    return torch.randn(C, generator=g) * 0.7 + 0.1, torch.rand(C, generator=g) * 1.7 + 0.6  # mean, std: no powers of two


def affine_ties(mean, std, per=2):
    """(channel, x) pairs for which the two-operation affine lands exactly on a bf16 tie while the exact x std + mean lies off it, so that an fma (or any other
    rounding point) rounds the other way: x = (T - mean) / std over the bf16 midpoints T of [2^-6, 2^-2), kept where the two forms differ."""
    j = torch.arange(128.0)
    T = torch.cat([2.0**e * (1 + (2 * j + 1) * 2.0**-8) for e in range(-6, -2)])
    T = torch.cat([T, -T]).float()
    out = []
    for c in range(mean.numel()):
        x = (T - mean[c]) / std[c]
        hit = (bits(bf(x * std[c] + mean[c])) != bits(bf(fma32(x, std[c], mean[c])))).nonzero().flatten()[:per]
        out += [(c, float(x[i])) for i in hit]
    return out


WAN_LAYOUTS = {"t2v": dict(Kp=64, Cx=0, copies=1), "i2v": dict(Kp=192, Cx=20, copies=1), "control": dict(Kp=128, Cx=16, copies=2)}
# (name, geometry): see CASES
LAYOUT_CASES = [
    ("t2v-W32", lambda: mk_geo("wan", 2, 2, 2, 4, 32, **WAN_LAYOUTS["t2v"])),
    ("i2v-W52", lambda: mk_geo("wan", 1, 1, 2, 4, 52, **WAN_LAYOUTS["i2v"])),
    ("t2v-W66", lambda: mk_geo("wan", 1, 2, 2, 2, 66, **WAN_LAYOUTS["t2v"])),
    ("control-W34", lambda: mk_geo("wan", 2, 1, 3, 4, 34, **WAN_LAYOUTS["control"])),
    ("i2v-W22", lambda: mk_geo("wan", 2, 2, 2, 4, 22, **WAN_LAYOUTS["i2v"])),
    ("p112-W10", lambda: mk_geo("wan", 1, 2, 2, 4, 10, C=16, Cx=4, patch=(1, 1, 2), Kp=64)),
    ("p111-W5", lambda: mk_geo("wan", 1, 1, 2, 4, 5, C=16, patch=(1, 1, 1), Kp=16)),
    ("t2v-W68", lambda: mk_geo("wan", 1, 1, 2, 2, 68, **WAN_LAYOUTS["t2v"])),
    ("t2v-W104", lambda: mk_geo("wan", 1, 2, 2, 4, 104, **WAN_LAYOUTS["t2v"])),
    ("cog-pt1-W34", lambda: mk_geo("cog", 2, 2, 3, 4, 34, patch=(1, 2, 2))),
    ("cog-pt1-W68", lambda: mk_geo("cog", 1, 1, 2, 4, 68, patch=(1, 2, 2))),
    ("cog-pt2-drop0", lambda: mk_geo("cog", 1, 1, 2, 4, 12, patch=(2, 2, 2))),
    ("cog-pt2-drop1", lambda: mk_geo("cog", 2, 2, 4, 4, 12, patch=(2, 2, 2), drop=1)),
]
LAYOUT = dict(LAYOUT_CASES)


def mk_init(name):
    g = LAYOUT[name]()
    q = gen(len(name) * 131 + g["W"])
    shape = (g["B"], g["C"], g["F"], g["H"], g["W"]) if g["model"] == "wan" else (g["B"], g["F"], g["C"], g["H"], g["W"])
    return {"op": "init", "name": name, "geo": g, "lat": vals32(shape, q, 2.0),
            "extra": rbf((g["B"], g["Cx"], g["F"], g["H"], g["W"]), q) if g["Cx"] else None}


def mk_finish(name):
    g = LAYOUT[name]()
    q = gen(len(name) * 137 + g["W"])
    p = {"op": "finish", "name": name, "geo": g, "x": vals32((g["B"], g["S"], g["Kc"]), q, 2.0)}
    if g["model"] == "wan":
        p["mean"], p["std"] = affine_params(g["C"], q)
        for n, (c, xv) in enumerate(affine_ties(p["mean"], p["std"])):
            p["x"][0, 1 + n % (g["S"] - 1), c * g["pv"]] = xv
    else:
        p["k"] = f32v(1.0 / 0.7)
    return p


STEP_GEOS = {  # Kc 16, 64, 64 x 2 copies, 128, 2048 (Wan) and 64, 128 (CogVideoX): S Kc % 2048 != 0 except at Kc = 2048
    "wan-Kc16": lambda B, P: mk_geo("wan", B, P, 1, 5, 7, C=16, patch=(1, 1, 1), Kp=16),
    "wan-Kc64": lambda B, P: mk_geo("wan", B, P, 3, 4, 6, **WAN_LAYOUTS["t2v"]),
    "wan-Kc64x2": lambda B, P: mk_geo("wan", B, P, 3, 4, 6, **WAN_LAYOUTS["control"]),
    "wan-Kc128": lambda B, P: mk_geo("wan", B, P, 2, 4, 6, C=16, patch=(2, 2, 2), Kp=128),
    "wan-Kc2048": lambda B, P: mk_geo("wan", B, P, 1, 2, 6, C=512, patch=(1, 2, 2), Kp=2048),
    "cog-Kc64": lambda B, P: mk_geo("cog", B, P, 3, 4, 6, patch=(1, 2, 2)),
    "cog-Kc128": lambda B, P: mk_geo("cog", B, P, 2, 4, 10, patch=(2, 2, 2)),
}
SIGMAS = ([0.9, 0.55, 0.31], [0.77, 0.4, 0.05])


def step_data(B, n, P, q, with_pred, token):
    x = vals32((B, n), q, 2.0)
    pred = None
    if with_pred:
        pred = rbf((P * B, n), q)
        pred[::B, :token] = 0  # a zero prediction under the ties at the head of sample 0's row: the fma lands on them
    return x, pred


def mk_step(name, B, guidance, with_pred=True, with_cols=True, step=0):
    P = 1 if guidance == 1.0 else 2
    g = STEP_GEOS[name](B, P)
    n = g["S"] * g["Kc"]
    x, pred = step_data(B, n, P, gen(len(name) + 10 * B + int(guidance)), with_pred, g["Kc"])
    p = {"op": "step", "kind": g["model"], "name": name, "geo": g, "P": P, "g": f32v(guidance), "x": x, "pred": pred, "want_copies": with_cols, "rows": g["S"],
         "Kp": g["Kp"], "copies": g["copies"]}
    if g["model"] == "wan":
        p["sigma"], p["sigma_next"] = torch.tensor(SIGMAS[0][:B]), torch.tensor(SIGMAS[1][:B])
    else:
        p["coef"], p["step"] = torch.tensor([0.9987, -0.0507, 0.93, -0.3, 0.71, -0.6, 1.0, -0.12]), step
    return p


CFG_SIZES = [(2, 2688 * 128), (3, 37 * 64), (1, 8)]


def mk_cfg(B, per, guidance, hold=0, plain_entry=False):
    P = 1 if guidance == 1.0 else 2
    x, pred = step_data(B, per, P, gen(B * 1000 + per % 997 + hold), True, 8)
    return {"op": "step", "kind": "cfg", "P": P, "g": f32v(guidance), "x": x, "pred": pred, "want_copies": True, "rows": 1, "Kp": per, "copies": 1, "hold": hold,
            "sigma": torch.tensor(SIGMAS[0][:B]), "sigma_next": torch.tensor(SIGMAS[1][:B]), "plain_entry": plain_entry}


def cfg_holds(per):
    return sorted({h for h in (0, 8, 1000, per - 8, per) if 0 <= h <= per})


UNPACK_C, UNPACK_S = (4, 60, 64, 68, 128), (1, 7, 8, 63, 64, 65, 72, 200)


def mk_unpack(B, C, Sn):
    q = gen(B + 10 * C + 1000 * Sn)
    mean, std = affine_params(C, q)
    x = vals32((B, Sn, C), q, 2.0)
    for n, (c, xv) in enumerate(affine_ties(mean, std)):
        x[B - 1, n % Sn, c] = xv
    return {"op": "unpack", "x": x, "mean": mean, "std": std}


MOD_D = (64, 1536, 100)


def mk_mod(Ln, rows, D):
    q = gen(Ln + 10 * rows + D)
    return {"op": "mod", "tables": [rbf((6 * D,), q) for _ in range(Ln)], "tproj": rbf((6 * D,), q, 2.0), "rows": rows, "D": D}


KEEPS = {"all": lambda F: [1] * F, "frame0": lambda F: [1] + [0] * (F - 1), "ends": lambda F: [1] + [0] * (F - 2) + [1], "none": lambda F: [0] * F}


def mk_pack(patch, Fc_kind, keep_kind, W):
    B, C, F, H = 3, 16, 6, 2  # 3 * 16 * 6 * 2 * W is no multiple of 256 at W = 6 and W = 34
    g = mk_geo("wan", B, 1, F, H, W, C=C, Cx=C, patch=patch, Kp=2 * C * patch[0] * patch[1] * patch[2], copies=2)
    Fc = {"one": 1, "F-1": F - 1, "F": F}[Fc_kind]
    q = gen(W + 7 * Fc + 13 * len(keep_kind) + patch[0])
    mean, std = affine_params(C, q)
    keep = torch.tensor([KEEPS[keep_kind](F), KEEPS["ends"](F), KEEPS[keep_kind](F)[::-1]], dtype=torch.uint8)
    return {"op": "pack", "geo": g, "Fc": Fc, "moments": rbf((B, 2 * C, F, H, W), q, 2.0), "control": rbf((B, 2 * C, Fc, H, W), q, 2.0), "noise": rbf((B, C, F, H, W), q),
            "sigmas": torch.tensor([0.3, 0.7, 0.55]), "mean": mean, "istd": 1.0 / std, "keep": keep}


def pack_cases():
    out = [mk_pack(patch, fc, kp, 6) for patch in ((1, 2, 2), (2, 2, 2)) for fc in ("one", "F-1", "F") for kp in KEEPS]
    return out + [mk_pack((1, 2, 2), "F-1", "ends", 34), mk_pack((2, 2, 2), "F", "frame0", 34)]


FP8_PLAIN = (16, 4080, 4096 * 256 * 16 + 16 * 300)


def fp8_bytes(n, q):
    t = torch.randint(0, 256, (n,), generator=q, dtype=torch.int64).to(torch.uint8)
    m = min(n, 256)
    t[:m] = torch.arange(256, dtype=torch.int64)[:m].to(torch.uint8)
    if n >= 512:
        t[-256:] = torch.arange(256, dtype=torch.int64).to(torch.uint8)  # every byte value again in the last (second-pass) stretch
    return t


def mk_fp8(rows, cols, transpose):
    return {"op": "fp8", "src": fp8_bytes(rows * cols, gen(rows + 3 * cols)).reshape(rows, cols), "transpose": transpose}


PERMUTE_DIMS = [(1, 2, 4, 3, 5, 1), (2, 3, 16, 4, 6, 2), (1, 1, 8, 2, 14, 2), (2, 2, 4, 5, 7, 1), (2, 5, 16, 64, 206, 2)]  # (B, F, C, H, W, p); the last: 2 109 440 elements


def mk_permute(dims, to_tokens):
    n = math.prod(dims[:5])
    src = (torch.arange(n, dtype=torch.int64) * 40503 % 65521 - 32000).to(torch.int16).view(bf16)  # distinct bit patterns (a few are NaN: compared as bits)
    src = torch.where(torch.isnan(src.float()), torch.ones_like(src), src)
    return {"op": "permute", "dims": dims, "src": src, "to_tokens": to_tokens}


# an operand's storage: (stride of the outer index, stride of the reduction index, offset of element (0, 0) in floats) from (outer extent O, reduction extent K)
STORE = {"k": lambda O, K: (K + 4, 1, 0), "o": lambda O, K: (1, O + 4, 0), "s_ld": lambda O, K: (K + 1, 1, 0), "s_off": lambda O, K: (K, 1, 1),
         "s_off_o": lambda O, K: (1, O, 1)}


def operand_mode(off, ld_o, ld_k):
    """wan_control.hip operand_mode, with the pointer's alignment as the float offset from an aligned base."""
    if off % 4 == 0 and ld_k == 1 and ld_o % 4 == 0:
        return 0
    if off % 4 == 0 and ld_o == 1 and ld_k % 4 == 0:
        return 1
    return 2


def mk_gemm(M, N, K, sa="k", sb="k", scale=1.0, accumulate=False, ldc=None, planes=False, ld_hl=None):
    q = gen(M + 3 * N + 7 * K + len(sa) + 5 * len(sb))
    a, b = vals32((M, K), q), vals32((K, N), q)
    return {"op": "gemm", "a": a, "b": b, "sa": sa, "sb": sb, "scale": f32v(scale), "accumulate": accumulate, "ldc": ldc or N, "planes": planes, "ld_hl": ld_hl or 2 * N,
            "c0": vals32((M, N), q, 3.0)}


GEMM_MODES = [("k", "k"), ("k", "o"), ("k", "s_ld"), ("o", "k"), ("o", "o"), ("o", "s_off"), ("s_ld", "k"), ("s_off", "o"), ("s_off_o", "s_ld")]


def gemm_cases():
    out = [mk_gemm(64, 64, 64, sa, sb, scale=0.3, planes=(i % 2 == 0)) for i, (sa, sb) in enumerate(GEMM_MODES)]
    out += [mk_gemm(128, 192, 192, "k", "o", planes=True, ld_hl=2 * 192 + 8), mk_gemm(192, 64, 320, "o", "k", scale=0.3, accumulate=True, ldc=68),
            mk_gemm(64, 128, 320, "s_ld", "s_off", accumulate=True, planes=True, ldc=132, ld_hl=2 * 128 + 8), mk_gemm(192, 192, 64, "k", "k", scale=0.3, accumulate=True)]
    return out


def layout_cases():
    return [mk_init(n) for n, _ in LAYOUT_CASES] + [mk_finish(n) for n, _ in LAYOUT_CASES]


def step_cases():
    out = []
    for name in STEP_GEOS:
        B = 2 if name == "wan-Kc2048" else 3
        out += [mk_step(name, B, 5.0), mk_step(name, B, 1.0, step=3), mk_step(name, B, 5.0, with_pred=False), mk_step(name, B, 1.0, with_cols=False, step=3)]
    out += [mk_step("wan-Kc64", 1, 5.0), mk_step("cog-Kc64", 1, 5.0, step=3), mk_step("wan-Kc64x2", 2, 1.0, with_pred=False)]
    return out


def cfg_cases():
    out = [mk_cfg(B, per, gd, plain_entry=True) for B, per in CFG_SIZES for gd in (1.0, 3.0, 7.5)]
    return out + [mk_cfg(B, per, gd, hold) for B, per in CFG_SIZES for hold in cfg_holds(per) for gd in ((1.0, 7.5) if per < 10000 else (3.0,))]


def unpack_cases():
    return [mk_unpack(B, C, Sn) for C in UNPACK_C for Sn in UNPACK_S for B in (1, 3)]


def mod_cases():
    return [mk_mod(Ln, rows, D) for Ln in (1, 3, 40) for rows in (1, 2) for D in MOD_D]


def fp8_cases():
    return [mk_fp8(1, n, False) for n in FP8_PLAIN] + [mk_fp8(r_, c_, True) for r_ in (64, 128, 192) for c_ in (64, 128, 192)]


def permute_cases():
    return [mk_permute(d, t) for d in PERMUTE_DIMS for t in (1, 0)]


FAMILIES = {"layout": layout_cases, "step": step_cases, "cfg": cfg_cases, "unpack": unpack_cases, "mod": mod_cases, "pack": pack_cases, "gemm": gemm_cases,
            "fp8": fp8_cases, "permute": permute_cases}


def tag_of(p):
    skip = ("op", "geo", "lat", "extra", "x", "pred", "tables", "tproj", "moments", "control", "noise", "a", "b", "c0", "src", "mean", "std", "istd", "coef", "sigma",
            "sigma_next", "sigmas")
    d = {k: v for k, v in p.items() if k not in skip and not torch.is_tensor(v)}
    shapes = {k: tuple(p[k].shape) for k in ("x", "a", "b", "src", "moments") if torch.is_tensor(p.get(k))}
    return p["op"] + " " + " ".join(f"{k}={v}" for k, v in {**d, **shapes}.items())


# ----------------------------------------------------------------------------------------------------
# GPU: every tensor the kernels see lies between sentinel padding in a buffer the test owns

def _dev():
    return torch.device("cuda", 0)


class Bufs:
    def __init__(self):
        self.dev, self.outs, self.keep = _dev(), {}, []

    def inp(self, t, fill=None):
        if t is None:
            return None
        if fill is None:
            fill = 0x7f if t.dtype == torch.uint8 else IN_SENT  # bytes: the fp8 NaN code, a kept frame
        b = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype)
        b[PAD:PAD + t.numel()] = t.flatten()
        self.keep.append(b.to(self.dev))
        return self.keep[-1][PAD:PAD + t.numel()]

    def out(self, name, shape, dtype=bf16, init=None, lead=0):
        """lead: extra sentinel elements in front (an offset view of a larger arena)."""
        n = math.prod(shape)
        b = torch.full((n + 2 * PAD + lead,), OUT_SENT, dtype=dtype)
        if init is not None:
            b[PAD + lead:PAD + lead + n] = init.flatten().to(dtype)
        b = b.to(self.dev)
        self.outs[name] = (b, shape, PAD + lead)
        return b[PAD + lead:PAD + lead + n]

    def collect(self):
        res = {}
        for name, (b, shape, at) in self.outs.items():
            h = b.cpu()
            n = math.prod(shape)
            assert (h[:at] == OUT_SENT).all() and (h[at + n:] == OUT_SENT).all(), f"{name}: padding overwritten"
            res[name] = h[at:at + n].reshape(shape)
        return res


def wan_geo(g):
    from finetrainers_amd import _lib

    t = _lib.WanSampleGeometry()
    for k in ("B", "C", "Cx", "F", "H", "W", "pt", "ph", "pw", "Kp", "copies", "P"):
        setattr(t, k, g[k])
    t.po = g["Kc"]
    return t


def cog_geo(g):
    from finetrainers_amd import _lib

    t = _lib.CogSampleGeometry()
    t.B, t.C, t.F, t.H, t.W, t.p, t.pt, t.P, t.drop = g["B"], g["C"], g["F"], g["H"], g["W"], g["ph"], g["pt"], g["P"], g["drop"]
    return t


def stored(mat, kind):
    """mat [O, K] (outer, reduction) in the storage `kind`: (host buffer filled with IN_SENT around the data, ld_o, ld_k, offset)."""
    O, K = mat.shape
    ld_o, ld_k, off = STORE[kind](O, K)
    size = off + (O - 1) * ld_o + (K - 1) * ld_k + 1
    buf = torch.full(((size + 3) // 4 * 4,), IN_SENT, dtype=f32)
    buf.as_strided((O, K), (ld_o, ld_k), off).copy_(mat)
    return buf, ld_o, ld_k, off


def launch_once(p):
    from finetrainers_amd import _lib

    lib, ptr, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
    b, op = Bufs(), p["op"]
    ck = lambda rc: _lib.check(rc, tag_of(p))
    g = p.get("geo")
    if op == "init":
        x, cols = b.out("x", (g["B"], g["S"], g["Kc"]), f32), b.out("cols", (g["P"], g["B"], g["S"], g["ld"]))
        if g["model"] == "wan":
            ck(lib.ftmi_wan_sample_init(ctypes.byref(wan_geo(g)), ptr(b.inp(p["lat"])), ptr(b.inp(p["extra"])), ptr(x), ptr(cols), st))
        else:
            ck(lib.ftmi_cog_sample_init(ctypes.byref(cog_geo(g)), ptr(b.inp(p["lat"])), ptr(x), ptr(cols), st))
    elif op == "finish":
        if g["model"] == "wan":
            o = b.out("out", (g["B"], g["C"], g["F"], g["H"], g["W"]))
            ck(lib.ftmi_wan_sample_finish(ctypes.byref(wan_geo(g)), ptr(b.inp(p["x"])), ptr(b.inp(p["mean"])), ptr(b.inp(p["std"])), ptr(o), st))
        else:
            o = b.out("out", (g["B"], g["F"] - g["drop"], g["C"], g["H"], g["W"]))
            ck(lib.ftmi_cog_sample_finish(ctypes.byref(cog_geo(g)), ptr(b.inp(p["x"])), p["k"], ptr(o), st))
    elif op == "step":
        B, n = p["x"].shape
        x = b.out("x", (B, n), f32, p["x"])
        cols = b.out("cols", (p["P"], B, p["rows"], p["copies"] * p["Kp"])) if p["want_copies"] else None
        pred = b.inp(p["pred"])
        if p["kind"] == "wan":
            ck(lib.ftmi_wan_sample_step(ctypes.byref(wan_geo(g)), ptr(pred), ptr(x), ptr(b.inp(p["sigma"])), ptr(b.inp(p["sigma_next"])), p["g"], ptr(cols), st))
        elif p["kind"] == "cog":
            ck(lib.ftmi_cog_sample_step(ctypes.byref(cog_geo(g)), ptr(pred), ptr(x), ptr(b.inp(p["coef"])), p["step"], p["g"], ptr(cols), st))
        elif p["plain_entry"]:
            ck(lib.ftmi_ltx_cfg_euler_step(ptr(pred), ptr(x), ptr(b.inp(p["sigma"])), ptr(b.inp(p["sigma_next"])), p["g"], ptr(cols), B, n, st))
        else:
            ck(lib.ftmi_ltx_cfg_euler_step_held(ptr(pred), ptr(x), ptr(b.inp(p["sigma"])), ptr(b.inp(p["sigma_next"])), p["g"], ptr(cols), B, n, p["hold"], st))
    elif op == "unpack":
        B, Sn, C = p["x"].shape
        ck(lib.ftmi_ltx_unpack_denorm(ptr(b.inp(p["x"])), ptr(b.inp(p["mean"])), ptr(b.inp(p["std"])), ptr(b.out("out", (B, C, Sn))), B, C, Sn, st))
    elif op == "mod":
        Ln = len(p["tables"])
        tabs = (ctypes.c_void_p * Ln)(*[ptr(b.inp(t)) for t in p["tables"]])
        ck(lib.ftmi_wan_sample_mod(tabs, Ln, ptr(b.inp(p["tproj"])), ptr(b.out("mod", (Ln, p["rows"], 6 * p["D"]), f32)), p["rows"], p["D"], st))
    elif op == "pack":
        cfg = _lib.WanControlPackConfig()
        cfg.B, cfg.C, cfg.F, cfg.Fc, cfg.H, cfg.W, cfg.pt, cfg.ph, cfg.pw = g["B"], g["C"], g["F"], p["Fc"], g["H"], g["W"], g["pt"], g["ph"], g["pw"]
        cols2, tg = b.out("cols2", (g["B"] * g["S"], 2 * g["Kp"])), b.out("target", tuple(p["noise"].shape))
        ck(lib.ftmi_wan_control_pack(ctypes.byref(cfg), ptr(b.inp(p["moments"])), ptr(b.inp(p["control"])), ptr(b.inp(p["noise"])), ptr(b.inp(p["sigmas"])),
                                     ptr(b.inp(p["mean"])), ptr(b.inp(p["istd"])), ptr(b.inp(p["keep"], fill=1)), ptr(cols2), ptr(tg), st))
    elif op == "fp8":
        rows, cols_ = p["src"].shape
        o = b.out("out", (cols_, rows) if p["transpose"] else (rows * cols_,), lead=8 * 24 if p["transpose"] else 0)  # the transposed copy: an offset view of an arena
        ck(lib.ftmi_fp8_upcast(ptr(b.inp(p["src"])), ptr(o), rows, cols_, int(p["transpose"]), st))
    elif op == "permute":
        B, F, C, H, W, pp = p["dims"]
        o = b.out("out", (p["src"].numel(),))
        fn = lib.ftmi_cog_patchify if p["to_tokens"] else lib.ftmi_cog_unpatchify
        ck(fn(ptr(b.inp(p["src"])), ptr(o), B, F, C, H, W, pp, st))
    elif op == "gemm":
        (M, K), N = p["a"].shape, p["b"].shape[1]
        ab, lda_row, lda_col, aoff = stored(p["a"], p["sa"])
        bb, ldb_col, ldb_row, boff = stored(p["b"].t(), p["sb"])
        init = torch.full((M, p["ldc"]), OUT_SENT)
        init[:, :N] = p["c0"]
        c = b.out("c", (M, p["ldc"]), f32, init)
        hl = b.out("hl", (M, p["ld_hl"])) if p["planes"] else None
        ck(lib.ftmi_f32_gemm(M, N, K, ptr(b.inp(ab)) + 4 * aoff, lda_row, lda_col, ptr(b.inp(bb)) + 4 * boff, ldb_row, ldb_col, ptr(c), p["ldc"], p["scale"],
                             int(p["accumulate"]), ptr(hl), p["ld_hl"], st))
    else:
        raise KeyError(op)
    torch.cuda.synchronize()
    return b.collect()


def run_gpu(p):
    """Runs the case twice on fresh padded buffers, asserts the same bits, and judges the second run."""
    _threads()
    first, second = launch_once(p), launch_once(p)
    for k in first:
        assert torch.equal(bits(first[k]), bits(second[k])), f"{tag_of(p)} {k}: two launches differ"
    judge_case(tag_of(p), p, second)


# ---- GPU tests -------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in LAYOUT_CASES])
def test_sample_init_and_finish(name):
    run_gpu(mk_init(name))
    run_gpu(mk_finish(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STEP_GEOS))
def test_sample_step(name):
    for p in step_cases():
        if p["name"] == name:
            run_gpu(p)


@pytest.mark.gpu
@pytest.mark.parametrize("B,per", CFG_SIZES)
def test_cfg_euler_step(B, per):
    for p in cfg_cases():
        if p["x"].shape == (B, per):
            run_gpu(p)


@pytest.mark.gpu
@pytest.mark.parametrize("C", UNPACK_C)
def test_unpack_denorm(C):
    for Sn in UNPACK_S:
        for B in (1, 3):
            run_gpu(mk_unpack(B, C, Sn))


@pytest.mark.gpu
def test_wan_sample_mod():
    for p in mod_cases():
        run_gpu(p)


@pytest.mark.gpu
def test_wan_control_pack():
    for p in pack_cases():
        run_gpu(p)


@pytest.mark.gpu
def test_f32_gemm():
    for p in gemm_cases():
        run_gpu(p)


@pytest.mark.gpu
def test_fp8_upcast():
    for p in fp8_cases():
        run_gpu(p)


@pytest.mark.gpu
def test_cog_patch_permute():
    for dims in PERMUTE_DIMS:
        fwd, back = mk_permute(dims, 1), mk_permute(dims, 0)
        run_gpu(fwd)
        run_gpu(back)
        assert torch.equal(bits(reference(dict(back, src=reference(fwd)["out"]))["out"]), bits(fwd["src"].flatten())), "the round trip is not the identity"


# ---- CPU self-checks ----------------------------------------------------------------------------------

def _failure(p, outs):
    try:
        judge_case("self-check " + tag_of(p), p, outs)
    except AssertionError as e:
        return str(e).split(":")[0]
    return None


@pytest.mark.parametrize("family", list(FAMILIES))
def test_fp32_stand_ins_pass_every_case(family, capsys):
    _threads()
    FIGURES.clear()
    for p in FAMILIES[family]():
        judge_case("stand-in " + tag_of(p), p, stand_in(p))
    with capsys.disabled():
        for op, (n, w) in sorted(FIGURES.items()):
            print(f"[sampling] stand-in {op:12s} differing elements {n}" + (f", err/bound {w:.3f}" if op == "gemm" else ""))


FAULTS = [  # (fault, the cases that must each reject it)
    ("stage_pass2", lambda: [mk_init("t2v-W32"), mk_init("t2v-W104")]),
    ("xstage_pass2", lambda: [mk_init("i2v-W52")]),
    ("gather_pass2", lambda: [mk_init("t2v-W66"), mk_init("control-W34"), mk_init("i2v-W22"), mk_init("t2v-W104")]),
    ("fin_read_pass2", lambda: [mk_finish("t2v-W66"), mk_finish("t2v-W104"), mk_finish("cog-pt1-W34")]),
    ("fin_store_pass2", lambda: [mk_finish("t2v-W68"), mk_finish("t2v-W104"), mk_finish("t2v-W66"), mk_finish("i2v-W22")]),
    ("residue", lambda: [mk_init("p111-W5")]),
    ("xresidue", lambda: [mk_init("p112-W10"), mk_init("i2v-W22")]),
    ("group2", lambda: [mk_init("t2v-W32"), mk_init("control-W34"), mk_step("wan-Kc64", 3, 5.0), mk_step("wan-Kc64x2", 2, 1.0, with_pred=False),
                        mk_step("cog-Kc64", 3, 5.0), mk_cfg(1, 8, 7.5), mk_mod(3, 2, 64), mk_pack((1, 2, 2), "F", "all", 6)]),
    ("extra_copy0", lambda: [mk_init("control-W34")]),
    ("pad_kept", lambda: [mk_init("i2v-W22"), mk_init("p112-W10")]),
    ("no_perm", lambda: [mk_step(n, 2, gd) for n in ("wan-Kc64", "wan-Kc64x2", "wan-Kc128", "wan-Kc2048") for gd in (1.0, 5.0)]),
    ("prev_sample", lambda: [mk_step("wan-Kc64", 3, 5.0), mk_step("wan-Kc16", 3, 1.0), mk_cfg(3, 37 * 64, 3.0)]),
    ("stride0", lambda: [mk_step("wan-Kc128", 3, 5.0), mk_cfg(2, 2688 * 128, 1.0)]),
    ("hold_off", lambda: [mk_cfg(3, 37 * 64, 7.5, 8), mk_cfg(3, 37 * 64, 1.0, 1000), mk_cfg(3, 37 * 64, 1.0, 37 * 64 - 8)]),
    ("held_updated", lambda: [mk_cfg(3, 37 * 64, 7.5, 8), mk_cfg(3, 37 * 64, 1.0, 37 * 64), mk_cfg(2, 2688 * 128, 3.0, 1000)]),
    ("drop_shifted", lambda: [mk_finish("cog-pt2-drop1")]),
    ("affine_fma", lambda: [mk_finish("t2v-W104"), mk_unpack(3, 128, 200)]),
    ("plus0", lambda: [mk_finish("cog-pt1-W34"), mk_finish("cog-pt2-drop1")]),
    ("pitch", lambda: [mk_finish("t2v-W68"), mk_finish("p111-W5"), mk_finish("cog-pt1-W34")]),
    ("lo_half_ld", lambda: [mk_gemm(64, 128, 320, "s_ld", "s_off", accumulate=True, planes=True, ldc=132, ld_hl=2 * 128 + 8)]),
    ("lo_is_hi", lambda: [mk_gemm(64, 64, 64, planes=True)]),
    ("k_desc", lambda: [mk_gemm(64, 64, 64), mk_gemm(192, 64, 320, "o", "k", scale=0.3, accumulate=True, ldc=68)]),
    ("two_partial", lambda: [mk_gemm(64, 64, 64), mk_gemm(128, 192, 192, "k", "o", planes=True, ld_hl=2 * 192 + 8)]),
    ("other_strides", lambda: [mk_gemm(64, 64, 64, sa, sb) for sa, sb in GEMM_MODES[:2]]),
    ("scale_after", lambda: [mk_gemm(192, 64, 320, "o", "k", scale=0.3, accumulate=True, ldc=68)]),
    ("keep_prev", lambda: [mk_pack((1, 2, 2), "F", "frame0", 6), mk_pack((2, 2, 2), "F-1", "ends", 6)]),
    ("sign_dropped", lambda: [mk_pack((1, 2, 2), "F", "none", 6), mk_pack((2, 2, 2), "one", "none", 6)]),
    ("nan_inf", lambda: [mk_fp8(1, 4080, False), mk_fp8(64, 64, True)]),
    ("sub_flushed", lambda: [mk_fp8(1, 16, False), mk_fp8(192, 64, True)]),
    ("upcast_pass2", lambda: [mk_fp8(1, FP8_PLAIN[-1], False)]),
    ("permute_pass2", lambda: [mk_permute(PERMUTE_DIMS[-1], 1), mk_permute(PERMUTE_DIMS[-1], 0)]),
]
ORDER_FAULTS = ("k_desc", "two_partial")  # f32_gemm's fixed accumulation order: inside the order-independent bound, so only the bitwise check can see them


@pytest.mark.parametrize("fault,cases", FAULTS, ids=[f for f, _ in FAULTS])
def test_seeded_faults_fail(fault, cases):
    _threads()
    for p in cases():
        assert _failure(p, stand_in(p)) is None, f"{tag_of(p)}: the unfaulted stand-in does not pass"
        why = _failure(p, stand_in(p, fault))
        assert why is not None, f"{fault} is not seen by {tag_of(p)}"
        if fault in ORDER_FAULTS:
            assert why == "bits", f"{fault}: expected to pass the bound and fail the bits, failed {why}"


def fma_exact(a, b, c):
    """fma of three fp32 values (Python floats) in exact rational arithmetic, rounded once to fp32 (nearest, ties to even)."""
    v = fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c)
    if v == 0:
        return 0.0
    sgn, v = (-1.0 if v < 0 else 1.0), abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if fractions.Fraction(2) ** e > v:
        e -= 1
    e = max(e, -126)
    n = round(v / fractions.Fraction(2) ** (e - 23))  # an integer below 2^24 + 1; round() of a Fraction rounds halves to even
    return sgn * float(n) * 2.0 ** (e - 23)


def fma_triples():
    q = gen(11)
    n = 6000
    sc = lambda: torch.ldexp(torch.randn(n, generator=q), torch.randint(-20, 21, (n,), generator=q)).float()
    a, b = sc(), sc()
    c = torch.where(torch.rand(n, generator=q) < 0.5, sc(), -(a.double() * b.double()).float() * (1 + torch.randint(-3, 4, (n,), generator=q).float() * 2.0**-22))
    # tie seekers: C = +-(2^24 + 2 k) 2^j has ulp 2^(j + 1); a b = +-2^j (1 - i^2 2^-46) puts the sum 2^(j - 46) i^2 off an fp32 midpoint, below the fp64 sum's ulp
    i = torch.randint(1, 60, (n,), generator=q).double()
    j = torch.randint(-12, 13, (n,), generator=q)
    k = torch.randint(0, 2**22, (n,), generator=q).double()
    sC = torch.where(torch.rand(n, generator=q) < 0.5, -1.0, 1.0).double()
    sP = torch.where(torch.rand(n, generator=q) < 0.5, -1.0, 1.0).double()
    ta = torch.ldexp(1.0 + i * 2.0**-23, j)
    tb = sP * (1.0 - i * 2.0**-23)
    tc = torch.ldexp(sC * (2.0**24 + 2.0 * k), j)
    A, B, C = torch.cat([a.double(), ta]), torch.cat([b.double(), tb]), torch.cat([c.double(), tc])
    assert torch.equal(A, A.float().double()) and torch.equal(B, B.float().double()) and torch.equal(C, C.float().double())
    return A, B, C, n


def test_fma_emulation():
    """fma32 against exact rational arithmetic on 6 000 random triples (half of them with a cancelling addend) and 6 000 tie seekers, on which the plain fp64
    expression rounded to fp32 is wrong more than a thousand times."""
    A, B, C, n = fma_triples()
    got = fma32(A, B, C)
    want = torch.tensor([fma_exact(x, y, z) for x, y, z in zip(A.tolist(), B.tolist(), C.tolist())], dtype=f64)
    assert torch.equal(want, want.float().double())
    assert torch.equal(bits(got), bits(want.float())), f"{int((bits(got) != bits(want.float())).sum())} of {2 * n} triples differ"
    naive = (A * B + C).float()
    assert int((bits(naive) != bits(want.float())).sum()) > 1000, "the tie seekers do not seek ties"
    if hasattr(math, "fma"):
        ref = torch.tensor([math.fma(x, y, z) for x, y, z in zip(A.tolist(), B.tolist(), C.tolist())], dtype=f64)
        assert torch.equal(bits(fma32(A, B, C)), bits(ref.float()))  # the double fma of fp32 inputs, rounded to fp32, is NOT in general the fp32 fma: checked above


def test_the_cases_reach_every_path():
    """The conditions of CASES, computed from the launchers' own formulas."""
    geos = {n: f() for n, f in LAYOUT_CASES}
    G = list(geos.values())
    vec_f = lambda g: g["C"] * g["pt"] * (g["pitch_f"] // 4)
    vec_h = lambda g: g["Cx"] * g["pt"] * (g["pitch_h"] // 8)
    gather = lambda g: g["wpn"] * (g["Kp"] // 8)
    assert {g["B"] for g in G} == {1, 2} and {g["P"] for g in G} == {1, 2}
    assert {(g["model"], g["Cx"], g["copies"]) for g in G} >= {("wan", 0, 1), ("wan", 20, 1), ("wan", 16, 2), ("cog", 0, 1)} and {g["pt"] for g in G if g["model"] == "cog"} == {1, 2}
    assert any(vec_f(g) > 256 for g in G) and any(vec_f(g) <= 256 for g in G), "staging loop"
    assert any(vec_h(g) > 256 for g in G) and any(0 < vec_h(g) <= 256 for g in G), "extra-channel staging loop"
    assert {g["Kp"] * g["copies"] for g in G if gather(g) > 256 and g["model"] == "wan"} >= {64, 256, 192}, "gather loop at every stored width"
    res = lambda g, nch, m: {int(v) for v in (lay_index(g, nch, g["F"], 0)["start"] & m).unique()}
    assert set().union(*(res(g, g["Cx"], 7) for g in G if g["Cx"])) == {0, 2, 4, 6}, "bf16 run starts"
    assert res(geos["p111-W5"], 16, 3) == {0, 1, 2, 3}, "fp32 run starts"
    assert any(g["seg"] % 8 == 0 and g["C"] * g["pt"] * (g["seg"] // 8) > 256 for g in G), "finish vector stores, second pass"
    assert any(g["seg"] % 8 == 0 and g["C"] * g["pt"] * (g["seg"] // 8) <= 256 for g in G)
    assert any(g["seg"] % 8 and g["C"] * g["pt"] * g["seg"] > 256 for g in G), "finish element stores, second pass"
    assert any(g["wpn"] * (g["Kc"] // 4) > 256 for g in G), "finish read loop"
    assert any(g["drop"] == 1 and g["pt"] == 2 and g["B"] == 2 and g["fpn"] * g["hpn"] > 1 for g in G), "drop"
    assert any((g["W"], g["H"], g["F"]) == (104, 4, 2) for g in G), "the real row"
    assert all(2 <= g["H"] <= 4 and 2 <= g["F"] <= 4 for g in G)
    st_ = [p for p in step_cases()]
    wan = [p for p in st_ if p["kind"] == "wan"]
    assert {p["geo"]["Kc"] for p in wan} == {16, 64, 128, 2048} and {p["copies"] for p in wan} == {1, 2}
    for kind in ("wan", "cog"):
        mine = [p for p in st_ if p["kind"] == kind]
        assert any(p["x"].shape[0] == 3 and p["x"].shape[1] % 2048 for p in mine), "a sample boundary inside a workgroup"
        assert any((p["x"].numel() // 8) % 256 and p["x"].numel() // 8 > 256 for p in mine), "a masked tail workgroup after a full one"
        assert {p["g"] for p in mine} == {1.0, 5.0} and any(p["pred"] is None for p in mine) and any(not p["want_copies"] for p in mine)
    assert {p["step"] for p in st_ if p["kind"] == "cog"} == {0, 3} and {p["geo"]["Kc"] for p in st_ if p["kind"] == "cog"} == {64, 128}
    cf = cfg_cases()
    assert {tuple(p["x"].shape) for p in cf} == set(CFG_SIZES)
    for B, per in CFG_SIZES:
        assert {p["hold"] for p in cf if p["x"].shape == (B, per)} >= {0, 8, per - 8, per} - ({8, per - 8} if per == 8 else set()) | {min(8, per)}
    assert any(p["hold"] % 2048 and p["hold"] > 2048 or p["hold"] == 1000 for p in cf), "a hold boundary inside a workgroup"
    assert any(m["D"] * 6 // 8 % 256 for m in mod_cases()) and {len(m["tables"]) for m in mod_cases()} == {1, 3, 40}
    pk = pack_cases()
    assert any(p["noise"].numel() % 256 for p in pk) and {p["geo"]["W"] for p in pk} == {6, 34} and {p["Fc"] for p in pk} == {1, 5, 6}
    assert any(((p["keep"][:, :p["Fc"]] == 0)[:, None, :, None, None] & (p["control"][:, :16].float() * s > 0.5)).any() for p in pk for s in (1, -1)), "both signs dropped"
    modes = set()
    for p in gemm_cases():
        (M, K), N = p["a"].shape, p["b"].shape[1]
        la, lb = STORE[p["sa"]](M, K), STORE[p["sb"]](N, K)
        modes.add((operand_mode(la[2], la[0], la[1]), operand_mode(lb[2], lb[0], lb[1])))
    assert modes == {(i, j) for i in range(3) for j in range(3)}, modes
    assert {operand_mode(*[STORE[s](64, 64)[i] for i in (2, 0, 1)]) for s in ("s_ld", "s_off", "s_off_o")} == {2}
    gm = gemm_cases()
    assert {p["a"].shape[0] for p in gm} == {64, 128, 192} == {p["b"].shape[1] for p in gm} and {p["a"].shape[1] for p in gm} == {64, 192, 320}
    assert any(p["ldc"] == p["b"].shape[1] + 4 for p in gm) and any(p["planes"] and p["ld_hl"] == 2 * p["b"].shape[1] + 8 for p in gm) and any(p["accumulate"] for p in gm)
    assert FP8_PLAIN[-1] // 16 > 4096 * 256 and (FP8_PLAIN[-1] // 16) % 256 and FP8_PLAIN[1] // 16 < 256
    assert math.prod(PERMUTE_DIMS[-1][:5]) > 8192 * 256 and all((d[4] // d[5]) % 2 for d in PERMUTE_DIMS) and {d[5] for d in PERMUTE_DIMS} == {1, 2}


# ---- refusals: on the host, with pointers that are never read ------------------------------------------------

_keep = ctypes.create_string_buffer(8192)
BASE = (ctypes.addressof(_keep) + 255) & ~255
P_ = [BASE + 256 * i for i in range(12)]  # aligned host addresses


def _wan(**kw):
    g = dict(B=1, C=16, Cx=0, F=2, H=4, W=6, pt=1, ph=2, pw=2, Kp=64, copies=1, P=2, po=64)
    g.update(kw)
    from finetrainers_amd import _lib

    t = _lib.WanSampleGeometry()
    for k, v in g.items():
        setattr(t, k, v)
    return ctypes.byref(t)


def _cog(**kw):
    g = dict(B=1, C=16, F=2, H=4, W=6, p=2, pt=1, P=2, drop=0)
    g.update(kw)
    from finetrainers_amd import _lib

    t = _lib.CogSampleGeometry()
    for k, v in g.items():
        setattr(t, k, v)
    return ctypes.byref(t)


def _pack(**kw):
    g = dict(B=1, C=16, F=2, Fc=2, H=4, W=6, pt=1, ph=2, pw=2)
    g.update(kw)
    from finetrainers_amd import _lib

    t = _lib.WanControlPackConfig()
    for k, v in g.items():
        setattr(t, k, v)
    return ctypes.byref(t)


def refusals(lib):
    """(call, expected code, a word of the message or None, what)."""
    a, b, c, d, e, f = P_[:6]
    odd = a + 8
    tabs = lambda *ps: (ctypes.c_void_p * len(ps))(*ps)
    R = []
    add = lambda fn, code, word, what: R.append((fn, code, word, what))
    # wan_sample_init / _step / _finish: the geometry (wan_lay), then the launcher's own checks
    init = lambda geo, lat=a, ex=None, x=b, cols=c: (lambda: lib.ftmi_wan_sample_init(geo, lat, ex, x, cols, None))
    for kw, code, word in (
            (dict(B=0), INVALID, "positive"), (dict(W=-6), INVALID, "positive"), (dict(Kp=0), INVALID, "positive"), (dict(copies=3), INVALID, "copies"),
            (dict(P=3), INVALID, "P is"), (dict(P=0), INVALID, "P is"), (dict(W=5), UNSUPPORTED, "whole patches"), (dict(H=3), UNSUPPORTED, "whole patches"),
            (dict(F=3, pt=2), UNSUPPORTED, "whole patches"), (dict(C=1024, po=4096, Kp=4096), UNSUPPORTED, "too wide"), (dict(C=3, po=12), UNSUPPORTED, "multiples of 8"),
            (dict(Kp=60), UNSUPPORTED, "row stride"), (dict(po=128), INVALID, "po"), (dict(Cx=4), INVALID, "do not fit"),
            (dict(C=12, po=48), UNSUPPORTED, "divide 2048"), (dict(W=1024, H=2), UNSUPPORTED, "LDS")):
        add(init(_wan(**kw), ex=(d if kw.get("Cx") else None)), code, word, f"wan_sample_init {kw}")
    add(init(_wan(Cx=16, Kp=128)), INVALID, "extra channels", "wan_sample_init Cx without extra")
    add(init(_wan(), ex=d), INVALID, "extra channels", "wan_sample_init extra without Cx")
    for name, kw in (("latents", dict(lat=odd)), ("x", dict(x=odd)), ("cols", dict(cols=odd))):
        add(init(_wan(), **kw), INVALID, "16-byte aligned", f"wan_sample_init misaligned {name}")
    add(init(_wan(Cx=16, Kp=128), ex=odd), INVALID, "16-byte aligned", "wan_sample_init misaligned extra")
    add(init(None), INVALID, "null", "wan_sample_init null geometry")
    add(init(_wan(), lat=None), INVALID, "null", "wan_sample_init null latents")
    step = lambda geo, gd=5.0, pred=a, x=b, s=c, sn=d, cols=e: (lambda: lib.ftmi_wan_sample_step(geo, pred, x, s, sn, gd, cols, None))
    add(step(_wan(P=2), gd=1.0), INVALID, "guidance", "wan_sample_step P = 2 with guidance 1")
    add(step(_wan(P=1), gd=5.0), INVALID, "guidance", "wan_sample_step P = 1 with guidance 5")
    add(step(_wan(), s=None), INVALID, "sigma", "wan_sample_step null sigma")
    add(step(_wan(), sn=None), INVALID, "sigma", "wan_sample_step null sigma_next")
    add(step(_wan(), pred=None, cols=None), INVALID, "null", "wan_sample_step neither pred nor cols")
    add(step(_wan(C=12, po=48)), UNSUPPORTED, "divide 2048", "wan_sample_step 2048 % Kc")
    for name, kw in (("pred", dict(pred=odd)), ("x", dict(x=odd)), ("cols", dict(cols=odd))):
        add(step(_wan(), **kw), INVALID, "16-byte aligned", f"wan_sample_step misaligned {name}")
    fin = lambda geo, x=a, mean=b, std=c, out=d: (lambda: lib.ftmi_wan_sample_finish(geo, x, mean, std, out, None))
    add(fin(_wan(W=1024, H=2)), UNSUPPORTED, "LDS", "wan_sample_finish row beyond the LDS")
    add(fin(_wan(po=32)), INVALID, "po", "wan_sample_finish Kc != po")
    add(fin(_wan(), x=odd), INVALID, "16-byte aligned", "wan_sample_finish misaligned x")
    add(fin(_wan(), out=odd), INVALID, "16-byte aligned", "wan_sample_finish misaligned latents")
    add(fin(_wan(), mean=None), INVALID, "null", "wan_sample_finish null mean")
    # cog_sample_*
    cinit = lambda geo, lat=a, x=b, cols=c: (lambda: lib.ftmi_cog_sample_init(geo, lat, x, cols, None))
    for kw, code, word in ((dict(F=0), INVALID, "positive"), (dict(p=0), INVALID, "positive"), (dict(P=3), INVALID, "P is"), (dict(pt=3, F=3), UNSUPPORTED, "patch_size_t"),
                           (dict(W=7), UNSUPPORTED, "whole patches"), (dict(drop=1), INVALID, "drop"), (dict(pt=2, drop=2), INVALID, "drop"),
                           (dict(drop=-1), INVALID, "drop"), (dict(C=3), UNSUPPORTED, "multiple of 8"), (dict(C=1024), UNSUPPORTED, "too wide"),
                           (dict(W=8194), UNSUPPORTED, "too wide"), (dict(W=2048, C=32), UNSUPPORTED, "LDS")):
        add(cinit(_cog(**kw)), code, word, f"cog_sample_init {kw}")
    add(cinit(_cog(), x=odd), INVALID, "16-byte aligned", "cog_sample_init misaligned x")
    add(cinit(_cog(), cols=None), INVALID, "null", "cog_sample_init null cols")
    cstep = lambda geo, gd=5.0, pred=a, x=b, coef=c, stp=0, cols=d: (lambda: lib.ftmi_cog_sample_step(geo, pred, x, coef, stp, gd, cols, None))
    add(cstep(_cog(P=2), gd=1.0), INVALID, "guidance", "cog_sample_step P = 2 with guidance 1")
    add(cstep(_cog(P=1)), INVALID, "guidance", "cog_sample_step P = 1 with guidance 5")
    add(cstep(_cog(), coef=None), INVALID, "coefficient", "cog_sample_step null coef")
    add(cstep(_cog(), stp=-1), INVALID, "step index", "cog_sample_step step < 0")
    add(cstep(_cog(), pred=odd), INVALID, "16-byte aligned", "cog_sample_step misaligned pred")
    add(cstep(_cog(), pred=None, cols=None), INVALID, "null", "cog_sample_step neither pred nor cols")
    cfin = lambda geo, x=a, out=b: (lambda: lib.ftmi_cog_sample_finish(geo, x, 1.5, out, None))
    add(cfin(_cog(pt=2, drop=2)), INVALID, "drop", "cog_sample_finish drop = pt")
    add(cfin(_cog(), out=odd), INVALID, "16-byte aligned", "cog_sample_finish misaligned latents")
    add(cfin(_cog(W=4096)), UNSUPPORTED, "LDS", "cog_sample_finish row beyond the LDS")
    # cfg_euler_step
    held = lambda B=2, per=64, hold=8, pred=a, x=b, xin=c, s=d: (lambda: lib.ftmi_ltx_cfg_euler_step_held(pred, x, s, e, 3.0, xin, B, per, hold, None))
    for kw, code, word in ((dict(B=0), INVALID, "empty"), (dict(per=0), INVALID, "empty"), (dict(per=-8), INVALID, "empty"), (dict(per=12), UNSUPPORTED, "multiple of 8"),
                           (dict(hold=4), UNSUPPORTED, "held prefix"), (dict(hold=72), INVALID, "held prefix"), (dict(hold=-8), INVALID, "held prefix"),
                           (dict(pred=odd), INVALID, "16-byte aligned"), (dict(x=odd), INVALID, "16-byte aligned"), (dict(xin=odd), INVALID, "16-byte aligned"),
                           (dict(xin=None), INVALID, "null"), (dict(s=None), INVALID, "null")):
        add(held(**kw), code, word, f"cfg_euler_step_held {kw}")
    add(lambda: lib.ftmi_ltx_cfg_euler_step(a, b, d, e, 3.0, c, 2, 12, None), UNSUPPORTED, "multiple of 8", "cfg_euler_step per_sample = 12")
    add(lambda: lib.ftmi_ltx_cfg_euler_step(a, b, d, e, 3.0, None, 2, 64, None), INVALID, "null", "cfg_euler_step null x_next")
    # unpack_denorm
    unp = lambda B=1, C=8, Sn=8, x=a, mean=b, std=c, out=d: (lambda: lib.ftmi_ltx_unpack_denorm(x, mean, std, out, B, C, Sn, None))
    for kw, code, word in ((dict(B=0), INVALID, "empty"), (dict(C=0), INVALID, "empty"), (dict(Sn=0), INVALID, "empty"), (dict(C=6), UNSUPPORTED, "multiple of 4"),
                           (dict(B=65536), UNSUPPORTED, "too large"), (dict(x=odd), INVALID, "16-byte aligned"), (dict(mean=odd), INVALID, "16-byte aligned"),
                           (dict(std=odd), INVALID, "16-byte aligned"), (dict(out=odd), INVALID, "16-byte aligned"), (dict(out=None), INVALID, "null")):
        add(unp(**kw), code, word, f"unpack_denorm {kw}")
    # wan_sample_mod
    mod = lambda tb, Ln, tproj=b, out=c, rows=1, D=64: (lambda: lib.ftmi_wan_sample_mod(tb, Ln, tproj, out, rows, D, None))
    add(mod(tabs(a), 0), INVALID, "empty", "wan_sample_mod L = 0")
    add(mod(tabs(a), 1, rows=0), INVALID, "empty", "wan_sample_mod rows = 0")
    add(mod(tabs(a), 1, D=0), INVALID, "empty", "wan_sample_mod D = 0")
    add(mod(tabs(*([a] * 41)), 41), UNSUPPORTED, "40 blocks", "wan_sample_mod L = 41")
    add(mod(tabs(a), 1, D=2), UNSUPPORTED, "multiple of 8", "wan_sample_mod 6 D % 8")
    add(mod(tabs(a, None), 2), INVALID, "scale_shift_table", "wan_sample_mod null table")
    add(mod(tabs(a, odd), 2), INVALID, "scale_shift_table", "wan_sample_mod misaligned table")
    add(mod(tabs(a), 1, tproj=odd), INVALID, "16-byte aligned", "wan_sample_mod misaligned tproj")
    add(mod(tabs(a), 1, out=odd), INVALID, "16-byte aligned", "wan_sample_mod misaligned mod")
    add(mod(None, 1), INVALID, "null", "wan_sample_mod null tables")
    # f32_gemm
    gm = lambda M=64, N=64, K=64, A=a, Bm=b, Cm=c, ldc=64, hl=None, ld_hl=0: (lambda: lib.ftmi_f32_gemm(M, N, K, A, K, 1, Bm, N, 1, Cm, ldc, 1.0, 0, hl, ld_hl, None))
    for kw, code, word in ((dict(M=-64), INVALID, "M, N >= 0"), (dict(K=0), INVALID, "K > 0"), (dict(A=None), INVALID, "null"), (dict(Cm=None), INVALID, "null"),
                           (dict(M=65), UNSUPPORTED, "multiples of 64"), (dict(N=96, ldc=96), UNSUPPORTED, "multiples of 64"), (dict(K=32), UNSUPPORTED, "multiples of 64"),
                           (dict(ldc=60), INVALID, "at least N"), (dict(ldc=66), INVALID, "at least N"), (dict(Cm=odd), INVALID, "at least N"),
                           (dict(hl=d, ld_hl=124), INVALID, "planes"), (dict(hl=d, ld_hl=130), INVALID, "planes"), (dict(hl=d + 4, ld_hl=128), INVALID, "planes"),
                           (dict(M=0), 0, None), (dict(N=0, ldc=0), 0, None), (dict(M=0, N=0, ldc=0), 0, None)):
        add(gm(**kw), code, word, f"f32_gemm {kw}")
    # wan_control_pack
    pk = lambda cfg, mom=a: (lambda: lib.ftmi_wan_control_pack(cfg, mom, b, c, d, e, f, P_[6], P_[7], P_[8], None))
    for kw, code, word in ((dict(B=0), INVALID, "positive"), (dict(Fc=0), INVALID, "positive"), (dict(pw=0), INVALID, "positive"), (dict(H=-4), INVALID, "positive"),
                           (dict(W=7), UNSUPPORTED, "whole patches"), (dict(F=3, pt=2), UNSUPPORTED, "whole patches")):
        add(pk(_pack(**kw)), code, word, f"wan_control_pack {kw}")
    add(pk(None), INVALID, "null", "wan_control_pack null config")
    add(pk(_pack(), mom=None), INVALID, "null", "wan_control_pack null moments")
    # fp8_upcast (the alignment refusal is new with this test)
    up = lambda rows=64, cols=64, tr=0, src=a, dst=b: (lambda: lib.ftmi_fp8_upcast(src, dst, rows, cols, tr, None))
    for kw, code, word in ((dict(rows=0), 0, None), (dict(cols=0, tr=1), 0, None), (dict(rows=-64), 0, None), (dict(rows=3, cols=5), UNSUPPORTED, "multiple of 16"),
                           (dict(rows=32, tr=1), UNSUPPORTED, "multiples of 64"), (dict(cols=96, tr=1), UNSUPPORTED, "multiples of 64"),
                           (dict(src=odd), INVALID, "16-byte aligned"), (dict(dst=odd), INVALID, "16-byte aligned"), (dict(src=a + 1), INVALID, "16-byte aligned"),
                           (dict(dst=b + 2, tr=1), INVALID, "16-byte aligned"), (dict(src=odd, tr=1), INVALID, "16-byte aligned"), (dict(src=None), INVALID, "null"),
                           (dict(dst=None, tr=1), INVALID, "null")):
        add(up(**kw), code, word, f"fp8_upcast {kw}")
    # cog_patchify / cog_unpatchify (H <= 0 and W <= 0 are refused with this test)
    for nm in ("ftmi_cog_patchify", "ftmi_cog_unpatchify"):
        pm = lambda B=1, F=1, C=4, H=4, W=4, pp=2, src=a, dst=b, fn=getattr(lib, nm): (lambda: fn(src, dst, B, F, C, H, W, pp, None))
        for kw, code, word in ((dict(B=0), INVALID, "geometry"), (dict(F=-1), INVALID, "geometry"), (dict(C=0), INVALID, "geometry"), (dict(pp=0), INVALID, "geometry"),
                               (dict(H=0), INVALID, "geometry"), (dict(W=0), INVALID, "geometry"), (dict(H=-4), INVALID, "geometry"), (dict(W=-2), INVALID, "geometry"),
                               (dict(H=5), INVALID, "geometry"), (dict(W=3), INVALID, "geometry"), (dict(src=None), INVALID, "null"), (dict(dst=None), INVALID, "null")):
            add(pm(**kw), code, word, f"{nm} {kw}")
    return R


def test_refusals_return_before_any_launch():
    """The table of REFUSALS AND ZERO SIZES on the host: every pointer is a host address that no kernel may read, so each call must return its code (or 0 for
    an empty problem) before anything is launched."""
    from finetrainers_amd import _lib

    lib = _lib.load()
    table = refusals(lib)
    assert len(table) > 150
    for fn, code, word, what in table:
        rc = fn()
        msg = _lib.last_error()
        assert rc == code, f"{what}: returned {rc}, expected {code} ({msg})"
        assert word is None or word in msg, f"{what}: '{word}' not in '{msg}'"
