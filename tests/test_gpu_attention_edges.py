"""The attention kernels against fp64 at the inputs where online-softmax kernels break (tests/test_gpu_kernels.py feeds them randn only: logits ~ N(0, 1)).

Reference: fp64 on the CPU, on the same bf16-rounded inputs, chunked over heads -- S = q k^T scale + bias, P = softmax(S), O = P v, lse = logsumexp(S),
the gradients by fp64 autograd.  Beside it a CONTRACT reference for dQ / dK: the same fp64 P, but delta = rowsum(dO * O_kernel) over the bf16 output the
backward is given (ftmi_attn_bwd receives `out`; delta is defined over it).  In peaked rows (P ~ 1 on one key) dS = P (dP - delta) cancels, and what is
left is the rounding of O to bf16 -- the contract reference is asserted there and the distance to the true gradient printed; everywhere else both.

Bounds: out rel-L2 <= 6e-3 and max-abs <= 5e-3 max(1, |O_ref|) (the existing ones); dQ, dK, dV rel-L2 <= 1e-2; lse rel-L2 <= 1e-4 and, per row,
  |lse - lse_ref| <= 2^-8 + Sk 2^-24 + max_j d 2^-24 scale sum_c |q_c k_jc| + 2^-22 (|lse_ref| + max_j |bias_j|)
(lse_bound below): the kernel's l is a sum of bf16-rounded probabilities -- each off by at most 2^-8 relative (one dominant probability rounded gives
that much), so ln l by at most 2^-8 nat -- summed in fp32 (Sk 2^-24 relative, worst case); each score is an fp32 dot product of d terms (the standard
d 2^-24 sum|terms| bound), and lse moves by at most the largest score error; the fp32 rows (m, lse2, the log2 e / ln 2 conversions, the bias scaled
to log2) add a few ulps of the largest magnitude involved.  Every output must be finite.

Regimes (seeded constructors; each at head_dim 64 and 128, whole and ragged Sq / Sk):
  R1 negative rows: every real logit of a row near an offset (-20, -60, -95, -150, -400 nat): q positive, k negative along the same direction, plus noise.
     lse ~ offset + ln Sk + a few nat: once it is below -88.7 nat (lse2 < -128), a zero-filled padded key's exp2 argument -lse2 exceeds 128 -- every row
     at -150 / -400 is past it, none at -20 / -60, and -95 straddles it at every shape (test_r1_rows_cross_the_exp2_overflow_threshold_where_stated).
  R2 growing max: a key in a late tile beats the earlier tiles by 10-40 nat for half the rows of every 32-row wave (the lazy-rescale ballot of
     attn_fwd_kernel diverges within the wave); mirror case with that key in the first tile.
  R3 large logits / peaked rows: per-row temperatures up to logits of several hundred nat of either sign; most rows have P ~ 1 on one key.
  R4 bias contract: a per-head [B, H, Sk] bias that differs between heads (kb_sh != 0), values up to +20 nat, -1e30 over whole 64-key tiles at the start,
     in the middle and at the ragged end (head by head), and one sample with every key masked: its output must be the fp64 result (uniform over the
     masked keys) and its gradients finite.  (Its gradients are NOT the fp64 ones: at |lse| = 1e30 fp32 cannot hold ln Sk, so the backward sees P = 1 per
     key instead of 1 / Sk -- the provider only promises a finite step for such a row; the other samples are compared as usual.)

Case -> kernel (dispatch rules of attn_fwd / attn_bwd, csrc/attention.hip; default FTMI_ATTN_PL = 0x111B, FTMI_ATTN_FEWKEYS = 1):
  head_dim 64   B  H   Sq    Sk  bias  forward                      dQ                                   dK / dV
                1  2  300  1000   -    attn_fwd_kernel ragged       attn_bwd_dq_pl_kernel<2,1,ragged>    attn_bwd_dkdv_pl_kernel<1>      (Sq < 512)
                1  2  256  1024   -    attn_fwd_kernel whole        attn_bwd_dq_pl_kernel<2,1>           attn_bwd_dkdv_pl_kernel<1>
                1  2  600   100   -    attn_fwd_kernel ragged       attn_bwd_dq_res_kernel<true>         attn_bwd_dkdv_sq_kernel<2>      (Sk <= 128, Sq >= 512)
                1  2  640   128   -    attn_fwd_kernel whole        attn_bwd_dq_res_kernel<false>        attn_bwd_dkdv_sq_kernel<2>
                1  2  200   100   -    attn_fwd_kernel ragged       attn_bwd_dq2_kernel<false,true>      attn_bwd_dkdv_kernel<1,2>
                1  2  128   192   -    attn_fwd_kernel whole        attn_bwd_dq2_kernel<false>           attn_bwd_dkdv_kernel<1,2>
                2  2  300  1000   x    attn_fwd_kernel biased       attn_bwd_dq2_kernel<true>            attn_bwd_dkdv_kernel<1,2>
                2  2  600   100   x    attn_fwd_kernel biased       attn_bwd_dq_res_kernel<true>         attn_bwd_dkdv_sq_kernel<2>
  head_dim 128  1  2  300  1000   -    attn_fwd_kernel<ND 2> ragged attn_bwd_dq_kernel<true,2>           attn_bwd_dkdv_pl128_kernel
                1  2  256   512   -    attn_fwd_kernel<ND 2> whole  attn_bwd_dq_kernel<false,2>          attn_bwd_dkdv_pl128_kernel
                1  2  100    77   -    attn_fwd_kernel<ND 2> ragged attn_bwd_dq_kernel<true,2>           attn_bwd_dkdv_kernel<2,0> + <2,1>  (Sq < 128)
                2  2  300   333   x    attn_fwd_kernel<ND 2> biased attn_bwd_dq_kernel<true,2>           attn_bwd_dkdv_pl128_kernel
  Every head_dim-64 case also runs with FTMI_ATTN_PL = 0x011 (attn_bwd_dq_pl_kernel<1,1>, 32 rows x two waves per SIMD) against fp64; the bit-identity
  tests add 0x001 / 0x101 (the x0 streams), 0 (attn_bwd_dq2_kernel for every dQ, attn_bwd_dkdv_kernel<1,2> / <2,0|1> for dK / dV), 0x1113 / 0x2113
  (attn_bwd_dkdv_pl_kernel<1> / <2>), 0x8 (pl128 on / off) and FTMI_ATTN_FEWKEYS = 0 (attn_bwd_dq2_kernel in place of the resident kernel).
  CogVideoX's real self-attention length (1 x 2 heads x 17 776 keys = 277 x 64 + 48, R1 at -150 nat): dQ on a strided sample of query rows against fp64,
  dK / dV finite and bit-identical across the switches.  (attn_bwd_dkdv_sq_kernel<1> is chosen by FTMI_DKVSQ_GROUPS, read once per process: not here.)

The unmarked tests at the end check on the CPU, from the fp64 reference alone, that every constructor still produces its regime.
"""

import math

import pytest
import torch

bf16 = torch.bfloat16
NEG = -1.0e30  # the provider's stand-in for -inf (attention_dispatch._MASKED)
R1_OFFSETS = (-20.0, -60.0, -95.0, -150.0, -400.0)
LSE_OVERFLOW = -128.0 * math.log(2.0)  # lse below this (nat): exp2(-lse2) of a zero-filled key overflows fp32

SHAPES = [
    # head_dim, B, H, Sq, Sk, biased  (kernels: module docstring)
    (64, 1, 2, 300, 1000, False),
    (64, 1, 2, 256, 1024, False),
    (64, 1, 2, 600, 100, False),
    (64, 1, 2, 640, 128, False),
    (64, 1, 2, 200, 100, False),
    (64, 1, 2, 128, 192, False),
    (64, 2, 2, 300, 1000, True),
    (64, 2, 2, 600, 100, True),
    (128, 1, 2, 300, 1000, False),
    (128, 1, 2, 256, 512, False),
    (128, 1, 2, 100, 77, False),
    (128, 2, 2, 300, 333, True),
]
BIASED_SHAPES = [s for s in SHAPES if s[5]] + [(64, 2, 2, 256, 1024, True), (128, 2, 2, 256, 512, True), (128, 2, 2, 100, 77, True)]


def _sid(s):
    return f"d{s[0]}-B{s[1]}H{s[2]}-{s[3]}x{s[4]}{'-bias' if s[5] else ''}"


# ----------------------------------------------------------------------------------------------------
# regime constructors: (q, k, v, dout) bf16 [B, H, S, d] on the CPU, bias fp32 [B, H, Sk] or None

def _base(B, H, Sq, Sk, d, g):
    q = torch.randn(B, H, Sq, d, generator=g, dtype=torch.float64)
    k = torch.randn(B, H, Sk, d, generator=g, dtype=torch.float64)
    v = torch.randn(B, H, Sk, d, generator=g, dtype=torch.float64)
    dout = torch.randn(B, H, Sq, d, generator=g, dtype=torch.float64)
    return q, k, v, dout


def _mild_bias(B, H, Sk, g):
    return (torch.randn(B, H, Sk, generator=g, dtype=torch.float64) * 0.5).float()


def make_r1(B, H, Sq, Sk, d, offset, biased=False, seed=0):
    """Every real logit of a row near `offset` nat: q = a_i u + n_q (positive entries along u = ones / sqrt(d)), k = -b u + n_k, the noise orthogonal to u,
    scale a_i b = -offset (1 +- 5 % per row): s_ij = offset (1 + jitter_i) + scale n_q.n_k -- rows differ, and within a row the logits spread by ~1.4 nat.
    b = 1 keeps the common part of K small: sum_j dS_ij = 0, so a large common K component would only amplify the bf16 rounding of dS in dQ."""
    g = torch.Generator().manual_seed(1000 + seed)
    q, k, v, dout = _base(B, H, Sq, Sk, d, g)
    scale = 1.0 / math.sqrt(d)
    u = torch.ones(d, dtype=torch.float64) / math.sqrt(d)
    b_ = 1.0
    jit = 1.0 + 0.05 * (2 * torch.rand(B, H, Sq, 1, generator=g, dtype=torch.float64) - 1)
    nq, nk = q * 1.2, k * 1.2
    nq = nq - (nq @ u)[..., None] * u
    nk = nk - (nk @ u)[..., None] * u
    q = nq + (-offset / (scale * b_)) * jit * u
    k = nk - b_ * u
    bias = _mild_bias(B, H, Sk, g) if biased else None
    return q.to(bf16), k.to(bf16), v.to(bf16), dout.to(bf16), bias


def spike_rows(Sq):
    """The rows that get the spike: half of every 32-row wave (a fixed pattern, so both halves of the ballot are represented in each wave)."""
    i = torch.arange(Sq)
    return ((i * 7 + (i // 32)) % 32) < 16


def make_r2(B, H, Sq, Sk, d, where="late", biased=False, seed=0):
    """randn logits (~N(0,1)) plus one spike key whose logit is 10-40 nat above the others for the rows of spike_rows(); the spike sits in the last
    tile ('late': the running max of those rows grows by far more than 2^8 mid-sequence while the other rows of the wave do not grow) or in tile 0 ('first').
    A channel c0 is reserved for it: k[:, :, :, c0] = 0 except the spike key, q[..., c0] = 0 except the spike rows."""
    g = torch.Generator().manual_seed(2000 + seed)
    q, k, v, dout = _base(B, H, Sq, Sk, d, g)
    scale = 1.0 / math.sqrt(d)
    nt = (Sk + 63) // 64
    j = (nt - 1) * 64 + min(5, Sk - 1 - (nt - 1) * 64) if where == "late" else 3
    k[..., 0] = 0
    q[..., 0] = 0
    K0 = 16.0
    k[:, :, j, 0] = K0
    rows = spike_rows(Sq)
    gain = 14.0 + 30.0 * torch.rand(B, H, Sq, generator=g, dtype=torch.float64)  # nat above 0: 10-40 above the earlier tiles' max (~3-4 nat)
    q[..., 0] = torch.where(rows, gain / (scale * K0), torch.zeros_like(gain))
    bias = _mild_bias(B, H, Sk, g) if biased else None
    return q.to(bf16), k.to(bf16), v.to(bf16), dout.to(bf16), bias


def make_r3(B, H, Sq, Sk, d, biased=False, seed=0):
    """Per-row temperatures: s_ij ~ N(0, (3 t_i)^2) nat with t_i log-uniform in [0.3, 30] -- logits up to several hundred nat of either sign; the hot rows
    put P ~ 1 on one key."""
    g = torch.Generator().manual_seed(3000 + seed)
    q, k, v, dout = _base(B, H, Sq, Sk, d, g)
    t = torch.exp(torch.empty(B, H, Sq, 1, dtype=torch.float64).uniform_(math.log(0.3), math.log(30.0), generator=g))
    q = q * t * math.sqrt(3.0)
    k = k * math.sqrt(3.0)
    bias = _mild_bias(B, H, Sk, g) if biased else None
    return q.to(bf16), k.to(bf16), v.to(bf16), dout.to(bf16), bias


def make_r4(B, H, Sq, Sk, d, seed=0):
    """randn q / k / v; bias [B, H, Sk]: N(0, 4^2) clamped to [-20, +20] nat, different per head; -1e30 over the whole first tile (head 0), a middle tile
    (head 1) and the last tile with its ragged end (every head >= 2); sample B-1 entirely -1e30 (needs B >= 2)."""
    assert B >= 2
    g = torch.Generator().manual_seed(4000 + seed)
    q, k, v, dout = _base(B, H, Sq, Sk, d, g)
    bias = (torch.randn(B, H, Sk, generator=g, dtype=torch.float64) * 4.0).clamp(-20.0, 20.0)
    bias[:, :, ::17] = 20.0  # some keys at the top of the moderate range
    nt = (Sk + 63) // 64
    if nt >= 2:
        bias[:, 0, 0:64] = NEG
    if nt >= 3:
        mid = nt // 2
        bias[:, 1 % H, mid * 64:(mid + 1) * 64] = NEG
    for h in range(2, H):
        bias[:, h, (nt - 1) * 64:] = NEG
    if H == 2 and nt >= 3:
        bias[:, 1, (nt - 1) * 64:] = NEG  # head 1 also masks the ragged end
    bias[B - 1] = NEG
    return q.to(bf16), k.to(bf16), v.to(bf16), dout.to(bf16), bias.float()


def make(regime, shape, seed=0):
    d, B, H, Sq, Sk, biased = shape
    if regime.startswith("r1"):
        return make_r1(B, H, Sq, Sk, d, float(regime[3:]), biased, seed)
    if regime == "r2-late":
        return make_r2(B, H, Sq, Sk, d, "late", biased, seed)
    if regime == "r2-first":
        return make_r2(B, H, Sq, Sk, d, "first", biased, seed)
    if regime == "r3":
        return make_r3(B, H, Sq, Sk, d, biased, seed)
    if regime == "r4":
        return make_r4(B, H, Sq, Sk, d, seed)
    raise ValueError(regime)


REGIMES = [f"r1:{o:g}" for o in R1_OFFSETS] + ["r2-late", "r2-first", "r3"]
PEAKED = {"r3", "r2-late", "r2-first"}  # rows with P ~ 1 on one key: dQ / dK asserted against the contract reference


# ----------------------------------------------------------------------------------------------------
# fp64 reference

def _threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))


def ref64(q, k, v, bias, dout, o_kernel=None, rows=None, grads=True):
    """fp64 attention on the bf16-rounded inputs, one head at a time.  rows: evaluate only these query rows (forward, lse, dQ -- dK / dV need every row).
    Returns dict: o, lse (nat), and with grads: dq, dk, dv (fp64 autograd) and, with o_kernel, dq_c / dk_c (delta = rowsum(dO * O_kernel))."""
    _threads()
    B, H, Sq, d = q.shape
    scale = 1.0 / math.sqrt(d)
    rs = slice(None) if rows is None else rows
    out = {n: [] for n in ("o", "lse", "dq", "dk", "dv", "dq_c", "dk_c")}
    for b in range(B):
        for h in range(H):
            qh = q[b, h, rs].double().requires_grad_(grads)
            kh = k[b, h].double().requires_grad_(grads)
            vh = v[b, h].double().requires_grad_(grads)
            s = (qh @ kh.t()) * scale
            if bias is not None:
                s = s + (bias[b, h] if bias.dim() == 3 else bias[b]).double()
            lse = torch.logsumexp(s, dim=-1)
            p = torch.softmax(s, dim=-1)  # (not exp(s - lse): at |s| ~ 1e30 even fp64 loses ln Sk, and the all-masked row must come out uniform)
            o = p @ vh
            out["o"].append(o.detach())
            out["lse"].append(lse.detach())
            if not grads:
                continue
            do = dout[b, h, rs].double()
            dq, dk, dv = torch.autograd.grad(o, (qh, kh, vh), do)
            out["dq"].append(dq)
            out["dk"].append(dk)
            out["dv"].append(dv)
            if o_kernel is not None:
                pd = p.detach()
                delta = (do * o_kernel[b, h, rs].double()).sum(-1, keepdim=True)
                ds = pd * (do @ vh.detach().t() - delta)
                out["dq_c"].append(ds @ kh.detach() * scale)
                out["dk_c"].append(ds.t() @ qh.detach() * scale)
    res = {}
    for n, lst in out.items():
        if lst:
            res[n] = torch.stack(lst).reshape(B, H, *lst[0].shape)
    return res


def lse_bound(q, k, bias, lse_ref, rows=None):
    """Per-row bound on |lse_kernel - lse_ref| in nat (derivation in the module docstring)."""
    B, H, Sq, d = q.shape
    Sk = k.shape[2]
    scale = 1.0 / math.sqrt(d)
    rs = slice(None) if rows is None else rows
    qa, ka = q[:, :, rs].double().abs(), k.double().abs()
    dot_err = d * 2.0**-24 * scale * (qa @ ka.transpose(-1, -2)).amax(-1)  # [B, H, rows]
    bmax = torch.zeros(B, H, 1, dtype=torch.float64)
    if bias is not None:
        bb = bias.double() if bias.dim() == 3 else bias.double()[:, None, :]
        bmax = bb.masked_fill(bb <= NEG / 2, 0.0).abs().amax(-1, keepdim=True).expand(B, H, 1)
    return 2.0**-8 + Sk * 2.0**-24 + dot_err + 2.0**-22 * (lse_ref.abs() + bmax)


def rel_l2(got, ref):
    got, ref = got.double(), ref.double()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def check(name, got, ref, tol):
    got = got.detach().float().cpu()
    assert torch.isfinite(got).all(), f"{name}: non-finite output ({(~torch.isfinite(got)).sum().item()} entries)"
    err = rel_l2(got, ref)
    print(f"[edges] {name:60s} rel_l2={err:.3e} max_abs={(got.double() - ref.double()).abs().max().item():.3e}")
    assert err <= tol, f"{name}: rel_l2 {err:.3e} > {tol:.1e}"
    return err


def check_out_lse(tag, out, lse2, ref, q, k, bias, rows=None, samples=None):
    o = out.float().cpu()
    lse = lse2.cpu().double() * math.log(2.0)
    o_ref, lse_ref = ref["o"], ref["lse"]
    if rows is not None:
        o, lse = o[:, :, rows], lse[:, :, rows]
    if samples is not None:
        o, lse, o_ref, lse_ref = o[samples], lse[samples], o_ref[samples], lse_ref[samples]
        q, k = q[samples], k[samples]
        bias = None if bias is None else bias[samples]
    check(tag + " out", o, o_ref, 6e-3)
    assert (o.double() - o_ref).abs().max().item() <= 5e-3 * max(1.0, o_ref.abs().max().item()), f"{tag} out: max-abs bound"
    assert torch.isfinite(lse).all(), f"{tag} lse: non-finite"
    check(tag + " lse", lse, lse_ref, 1e-4)
    bound = lse_bound(q, k, bias, lse_ref, rows)
    excess = ((lse - lse_ref).abs() - bound).max().item()
    assert excess <= 0, f"{tag} lse: a row exceeds its bound by {excess:.3e} nat"


def check_grads(tag, grads, ref, peaked, samples=None, rows=None):
    dq, dk, dv = (t.float().cpu() for t in grads)
    if rows is not None:
        dq = dq[:, :, rows]
    sel = (lambda t: t) if samples is None else (lambda t: t[samples])
    dq, dk, dv = sel(dq), sel(dk), sel(dv)
    r = {n: sel(t) for n, t in ref.items()}
    check(tag + " dv", dv, r["dv"], 1e-2)
    if peaked:
        check(tag + " dq (contract)", dq, r["dq_c"], 1e-2)
        check(tag + " dk (contract)", dk, r["dk_c"], 1e-2)
        print(f"[edges] {tag} distance to the true fp64 gradient: dq {rel_l2(dq, r['dq']):.3e} dk {rel_l2(dk, r['dk']):.3e}")
    else:
        for n, g_ in (("dq", dq), ("dk", dk)):
            check(f"{tag} {n}", g_, r[n], 1e-2)
            check(f"{tag} {n} (contract)", g_, r[n + "_c"], 1e-2)


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


def _run(q, k, v, dout, bias):
    from finetrainers_amd import ops

    dev = _dev()
    qd, kd, vd, dd = q.to(dev), k.to(dev), v.to(dev), dout.to(dev)
    bd = None if bias is None else bias.to(dev)
    out, lse = ops.attn_fwd(qd, kd, vd, bd)
    return (qd, kd, vd, dd, bd), out, lse


# ----------------------------------------------------------------------------------------------------
# GPU: every regime x every shape against fp64

@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("regime", REGIMES)
def test_attention_regime_against_fp64(regime, shape, sw):
    from finetrainers_amd import ops

    q, k, v, dout, bias = make(regime, shape)
    dev_in, out, lse = _run(q, k, v, dout, bias)
    out_c = out.cpu()
    ref = ref64(q, k, v, bias, dout, o_kernel=out_c)
    tag = f"{regime} {_sid(shape)}"
    check_out_lse(tag, out, lse, ref, q, k, bias)
    settings = ("default", "0x011") if shape[0] == 64 else ("default",)
    for pl in settings:
        if pl != "default":
            sw("FTMI_ATTN_PL", pl)
        grads = ops.attn_bwd(*dev_in[:3], out, lse, dev_in[3], dev_in[4])
        torch.cuda.synchronize()
        check_grads(f"{tag} pl={pl}", grads, ref, regime in PEAKED)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BIASED_SHAPES, ids=_sid)
def test_attention_bias_contract_against_fp64(shape):
    """R4: per-head bias (kb_sh != 0), masked whole tiles at the start / middle / ragged end, biases up to +20 nat, one all-masked sample."""
    from finetrainers_amd import ops

    q, k, v, dout, bias = make("r4", shape)
    B = q.shape[0]
    dev_in, out, lse = _run(q, k, v, dout, bias)
    ref = ref64(q, k, v, bias, dout, o_kernel=out.cpu())
    tag = f"r4 {_sid(shape)}"
    check_out_lse(tag, out, lse, ref, q, k, bias)  # the all-masked sample included: uniform over its keys
    grads = ops.attn_bwd(*dev_in[:3], out, lse, dev_in[3], dev_in[4])
    torch.cuda.synchronize()
    for n, t in zip(("dq", "dk", "dv"), grads):
        assert torch.isfinite(t.float()).all(), f"{tag} {n}: non-finite"
    check_grads(tag, grads, ref, peaked=False, samples=slice(0, B - 1))


@pytest.mark.gpu
def test_attention_bias_contract_through_the_provider():
    """R4 end to end through attention_dispatch: a bool mask [B, H, 1, Sk] that differs per head (-> [B, H, Sk] key bias) with one all-False sample."""
    from finetrainers_amd.attention_dispatch import attention_dispatch

    d, B, H, Sq, Sk = 64, 2, 3, 300, 1000
    q, k, v, dout, bias = make_r4(B, H, Sq, Sk, d, seed=5)
    mask = bias > NEG / 2  # True = keep
    bias_ref = torch.where(mask, torch.zeros_like(bias), torch.full_like(bias, NEG))
    dev = _dev()
    qd, kd, vd = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    o = attention_dispatch(qd, kd, vd, attn_mask=mask[:, :, None, :].to(dev))
    o.backward(dout.to(dev))
    torch.cuda.synchronize()
    ref = ref64(q, k, v, bias_ref, dout, o_kernel=o.detach().cpu())
    tag = "r4 provider"
    check(tag + " out", o.detach().cpu(), ref["o"], 6e-3)
    assert (o.detach().float().cpu().double() - ref["o"]).abs().max().item() <= 5e-3 * max(1.0, ref["o"].abs().max().item())
    for n, t in (("dq", qd.grad), ("dk", kd.grad), ("dv", vd.grad)):
        assert torch.isfinite(t.float()).all(), f"{tag} {n}: non-finite"
    check_grads(tag, (qd.grad, kd.grad, vd.grad), ref, peaked=False, samples=slice(0, B - 1))


# ----------------------------------------------------------------------------------------------------
# GPU: bit identity of the kernel pairs on the new inputs

BIT_SHAPES = [(64, 1, 2, 300, 1000, False), (64, 1, 2, 256, 1024, False), (64, 1, 2, 600, 100, False), (64, 2, 2, 600, 100, True),
              (128, 1, 2, 300, 1000, False), (128, 2, 2, 300, 333, True)]
BIT_CASES = [(r, s) for r in ("r1:-150", "r1:-400", "r1:-20", "r2-late", "r3") for s in BIT_SHAPES] + [("r4", s) for s in BIT_SHAPES if s[5]]


def _bwd_under(sw, dev_in, out, lse, settings):
    from finetrainers_amd import ops

    res = {}
    for name, value in settings:
        sw(name, value)
        res[(name, value)] = ops.attn_bwd(*dev_in[:3], out, lse, dev_in[3], dev_in[4])
        torch.cuda.synchronize()
    return res


def _same(tag, x, y):
    assert torch.equal(x, y), f"{tag}: not bit-identical (max |diff| {(x.float() - y.float()).abs().max().item():.3e})"


@pytest.mark.gpu
@pytest.mark.parametrize("regime,shape", BIT_CASES, ids=[f"{r}-{_sid(s)}" for r, s in BIT_CASES])
def test_attention_kernel_pairs_bit_identical_on_edge_inputs(regime, shape, sw):
    """The bit-identity comparisons of tests/test_gpu_kernels.py on R1-R4 inputs: FTMI_ATTN_PL 0x001 / 0x101 against 0 (the x0 dQ streams against
    attn_bwd_dq2_kernel, dK / dV through the delta they publish), 0x1113 / 0x2113 against 0x111 (pipelined dK / dV), 0x8 against 0 (head_dim 128), and
    FTMI_ATTN_FEWKEYS 1 against 0; the shipped streams 0x011 / 0x111 within 1e-3 of the compiler-scheduled dQ (dK / dV equal).  Every output finite."""
    q, k, v, dout, bias = make(regime, shape)
    dev_in, out, lse = _run(q, k, v, dout, bias)
    tag = f"{regime} {_sid(shape)}"
    d, _, _, Sq, Sk, _ = shape
    PL = "FTMI_ATTN_PL"
    if d == 64:
        res = _bwd_under(sw, dev_in, out, lse, [(PL, p) for p in ("0", "0x001", "0x101", "0x011", "0x111", "0x1113", "0x2113")])
        for key, val in res.items():
            for n, t in zip(("dq", "dk", "dv"), val):
                assert torch.isfinite(t.float()).all(), f"{tag} {key} {n}: non-finite"
        for p in ("0x001", "0x101"):
            for n, x, y in zip(("dq", "dk", "dv"), res[(PL, p)], res[(PL, "0")]):
                _same(f"{tag} {PL}={p} {n}", x, y)
        for p in ("0x011", "0x111"):
            rel = rel_l2(res[(PL, p)][0].float().cpu(), res[(PL, "0")][0].float().cpu())
            print(f"[edges] {tag} dq {p} vs compiler-scheduled: rel_l2 {rel:.2e}")
            assert rel < 1e-3, f"{tag} {PL}={p} dq: rel_l2 {rel:.2e} against the compiler-scheduled kernel"
            _same(f"{tag} {PL}={p} dk", res[(PL, p)][1], res[(PL, "0")][1])
            _same(f"{tag} {PL}={p} dv", res[(PL, p)][2], res[(PL, "0")][2])
        for p in ("0x1113", "0x2113"):
            for n, x, y in zip(("dq", "dk", "dv"), res[(PL, p)], res[(PL, "0x111")]):
                _same(f"{tag} {PL}={p} {n}", x, y)
        if Sk <= 128 and Sq >= 512:
            sw(PL, "0x111B")
            few = _bwd_under(sw, dev_in, out, lse, [("FTMI_ATTN_FEWKEYS", "1"), ("FTMI_ATTN_FEWKEYS", "0")])
            for n, x, y in zip(("dq", "dk", "dv"), few[("FTMI_ATTN_FEWKEYS", "1")], few[("FTMI_ATTN_FEWKEYS", "0")]):
                _same(f"{tag} FTMI_ATTN_FEWKEYS=1 {n}", x, y)
    else:
        res = _bwd_under(sw, dev_in, out, lse, [(PL, "0"), (PL, "0x8")])
        for n, x, y in zip(("dq", "dk", "dv"), res[(PL, "0x8")], res[(PL, "0")]):
            assert torch.isfinite(x.float()).all(), f"{tag} 0x8 {n}: non-finite"
            _same(f"{tag} {PL}=0x8 {n}", x, y)


# ----------------------------------------------------------------------------------------------------
# GPU: CogVideoX's real self-attention length

COG = (64, 1, 2, 17776, 17776, False)


@pytest.mark.gpu
def test_attention_cogvideox_length_negative_rows(sw):
    """R1 at -150 nat on 1 x 2 heads x 17 776 tokens (= 277 x 64 + 48: every tile loop of the launch is ragged).  Forward and dQ on every 37th query row
    against fp64 (the default pipelined dQ and 0x011); dQ of the x0 stream (0x101) bit-identical to the masking kernel (0); dK / dV finite and
    bit-identical across the dK / dV kernels."""
    from finetrainers_amd import ops

    d, B, H, Sq, Sk, _ = COG
    q, k, v, dout, _ = make_r1(B, H, Sq, Sk, d, -150.0, seed=9)
    rows = torch.arange(0, Sq, 37)
    dev_in, out, lse = _run(q, k, v, dout, None)
    ref = ref64(q, k, v, None, dout, o_kernel=out.cpu(), rows=rows, grads=False)
    tag = "r1:-150 cogvideox 17776"
    check_out_lse(tag, out, lse, ref, q, k, None, rows=rows)
    assert ref["lse"].max().item() < LSE_OVERFLOW  # the regime crosses at this length
    # dQ of the sampled rows, fp64: dS = P (dO V^T - delta), delta over the kernel's output (not peaked: the true and the contract delta agree to bf16)
    scale = 1.0 / math.sqrt(d)
    results = {}
    for pl in ("0x111B", "0x011", "0x111", "0x1113", "0x2113", "0x101", "0"):
        sw("FTMI_ATTN_PL", pl)
        results[pl] = ops.attn_bwd(*dev_in[:3], out, lse, dev_in[3], None)
        torch.cuda.synchronize()
    _threads()
    for pl in ("0x111B", "0x011"):
        dq = results[pl][0].float().cpu()[:, :, rows]
        errs = []
        for h in range(H):
            qh, kh, vh = q[0, h, rows].double(), k[0, h].double(), v[0, h].double()
            s = qh @ kh.t() * scale
            p = torch.softmax(s, dim=-1)
            do = dout[0, h, rows].double()
            for delta in ((do * (p @ vh)).sum(-1, keepdim=True), (do * out[0, h, rows].float().cpu().double()).sum(-1, keepdim=True)):
                dq_ref = (p * (do @ vh.t() - delta)) @ kh * scale
                errs.append((dq[0, h], dq_ref))
        for i, (got, r) in enumerate(errs):
            check(f"{tag} pl={pl} dq head {i // 2} ({'true' if i % 2 == 0 else 'contract'} delta)", got, r, 1e-2)
    for pl, val in results.items():
        for n, t in zip(("dq", "dk", "dv"), val):
            assert torch.isfinite(t.float()).all(), f"{tag} {pl} {n}: non-finite"
    for pl in ("0x1113", "0x2113"):
        for n, x, y in zip(("dq", "dk", "dv"), results[pl], results["0x111"]):
            _same(f"{tag} {pl} {n}", x, y)
    for n, x, y in zip(("dq", "dk", "dv"), results["0x101"], results["0"]):
        _same(f"{tag} 0x101 {n}", x, y)


# ----------------------------------------------------------------------------------------------------
# CPU: the constructors still produce their regimes (no GPU; runs under -m "not gpu")

def _lse64(q, k, bias):
    B, H, Sq, d = q.shape
    s = q.double() @ k.double().transpose(-1, -2) / math.sqrt(d)
    if bias is not None:
        s = s + bias.double()[:, :, None, :]
    return s, torch.logsumexp(s, dim=-1)


def test_r1_rows_cross_the_exp2_overflow_threshold_where_stated():
    """lse ~ offset (1 +- 5 % per row) + ln Sk + (spread of a row's logits)^2 / 2, the last two 7-10 nat at these shapes: every row at -150 and -400 is
    below -88.7 nat (lse2 < -128) at every shape, no row at -20 and -60; at -95 the threshold falls INSIDE the rows at every shape (some cross, some do
    not: the boundary itself is exercised)."""
    for shape in SHAPES:
        q, k, v, dout, bias = make("r1:-95", shape)
        _, lse = _lse64(q, k, bias)
        assert (lse < LSE_OVERFLOW).any() and (lse > LSE_OVERFLOW).any(), (_sid(shape), lse.min().item(), lse.max().item())
        for off, expect in ((-20.0, False), (-60.0, False), (-150.0, True), (-400.0, True)):
            q, k, v, dout, bias = make(f"r1:{off:g}", shape)
            s, lse = _lse64(q, k, bias)
            if expect:
                assert lse.max().item() < LSE_OVERFLOW, (off, _sid(shape), lse.max().item())
            else:
                assert lse.min().item() > LSE_OVERFLOW, (off, _sid(shape), lse.min().item())
            # rows differ, and no row is a single-key spike: the logits of a row spread over a few nat around the offset
            assert lse.std().item() > 0.5
            assert abs(s.mean().item() - off) < 0.1 * abs(off) + 3
    d, B, H, Sq, Sk, _ = COG
    q, k, _, _, _ = make_r1(B, H, 64, Sk, d, -150.0, seed=9)
    assert _lse64(q, k, None)[1].max().item() < LSE_OVERFLOW


def _tile_growth(s, Sk):
    """Per row: the largest growth (log2 units) of the running max from one 64-key tile to the next."""
    nt = (Sk + 63) // 64
    tm = torch.stack([s[..., t * 64:min(Sk, (t + 1) * 64)].amax(-1) for t in range(nt)], -1) / math.log(2.0)
    run = torch.cummax(tm, dim=-1).values
    return (tm[..., 1:] - run[..., :-1]).amax(-1)


def test_r2_ballot_diverges_within_every_wave():
    for shape in SHAPES:
        Sk, Sq = shape[4], shape[3]
        q, k, v, dout, bias = make("r2-late", shape)
        s, _ = _lse64(q, k, bias)
        grow = _tile_growth(s, Sk)  # [B, H, Sq]
        for w0 in range(0, Sq - 31, 32):
            gw = grow[..., w0:w0 + 32]
            assert ((gw > 8).any(-1) & (gw < 8).any(-1)).all(), (_sid(shape), w0)
        rows = spike_rows(Sq)
        assert (grow[..., rows] > 8).all() and (grow[..., ~rows] < 8).all(), _sid(shape)
        q, k, v, dout, bias = make("r2-first", shape)
        s, _ = _lse64(q, k, bias)
        assert (_tile_growth(s, Sk) < 8).all(), _sid(shape)  # the mirror: the max is in the first tile
        assert (s.amax(-1)[..., rows] - s[..., 0:64].amax(-1)[..., rows]).abs().max() < 1e-9


def test_r3_logits_are_large_and_rows_peaked():
    for shape in SHAPES:
        q, k, v, dout, bias = make("r3", shape)
        s, lse = _lse64(q, k, bias)
        assert s.amax().item() > 200 and s.amin().item() < -200, _sid(shape)
        pmax = torch.exp(s.amax(-1) - lse)
        assert (pmax > 0.99).float().mean().item() > 0.2, _sid(shape)  # peaked rows
        assert (pmax < 0.5).float().mean().item() > 0.05, _sid(shape)  # and some that are not


def test_r4_bias_contract_inputs():
    for shape in BIASED_SHAPES:
        d, B, H, Sq, Sk, _ = shape
        q, k, v, dout, bias = make("r4", shape)
        assert bias.shape == (B, H, Sk) and bias.dtype == torch.float32
        assert not torch.equal(bias[:, 0], bias[:, 1]), _sid(shape)  # per-head bias differs between heads
        assert (bias[B - 1] == NEG).all(), _sid(shape)  # the all-masked sample
        live = bias[: B - 1]
        assert (live[live > NEG / 2].max() == 20.0) and (live[live > NEG / 2] <= 20.0).all()
        nt = (Sk + 63) // 64
        assert (live[:, 0, :64] == NEG).all()  # a whole first tile masked
        if nt >= 3:
            mid = nt // 2
            assert (live[:, 1, mid * 64:(mid + 1) * 64] == NEG).all()  # a middle tile
            assert (live[:, 1, (nt - 1) * 64:] == NEG).all()  # the (ragged) end
        # every live row keeps at least one unmasked key
        assert (live > NEG / 2).any(-1).all()
