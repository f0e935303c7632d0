"""CogVideoX latent sampling on the GPU: the three layout kernels against tests/cog_sampling_reference.py (bit for bit where the arithmetic is exact, against
fp64 where it rounds), the one-call loop against its composition from ``model.forward`` and ``ops.cog_sample_step`` bit for bit for the three geometries and
a model without adapters, the sampler's view of live adapters, the workspace plan, the trajectory against ``oracle.cogvideox`` in bf16 and fp32, and the
Wan entry points against the CogVideoX ones on a geometry both express (one set of layout kernels, csrc/sample_layout.hip)."""
import ctypes

import pytest
import torch

import cog_sampling_reference as ref

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
C = 16
# (F, H, W, patch_size_t): one token; 18 tokens with W = 6 (runs of 12 elements that start off the 16-byte grid, a tail in the step's only workgroup);
# W = 8 (runs of 16 elements: the vector-store path of finish), with and without patches over two frames (Kc = 128)
GRIDS = [(1, 2, 2, 1), (3, 4, 6, 1), (2, 4, 8, 1), (2, 4, 8, 2)]


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def _geo(B, P, F_, H, W, pt, drop=0):
    from finetrainers_amd import ops

    return ops.cog_sample_geometry(B, C, F_, H, W, patch=2, patch_t=pt if pt > 1 else None, guidance=P == 2, drop=drop)


def _dims(F_, H, W, pt):
    return (F_ // pt) * (H // 2) * (W // 2), C * pt * 4


# ---- 1. init -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F_,H,W,pt", GRIDS)
def test_init_is_the_models_patchify_bit_for_bit(F_, H, W, pt, B, P):
    from finetrainers_amd import ops
    from finetrainers_amd.cogvideox.model import patches_3d

    dev = _dev()
    lat = torch.randn(B, F_, C, H, W, generator=torch.Generator().manual_seed(F_ * 7 + B))
    S, Kc = _dims(F_, H, W, pt)
    x = torch.full((B, S, Kc), float("nan"), device=dev)
    cols = torch.full((P * B * S, Kc), float("nan"), dtype=bf16, device=dev)
    ops.cog_sample_init(_geo(B, P, F_, H, W, pt), lat.to(dev), x=x, cols=cols)
    torch.cuda.synchronize()
    x_ref, cols_ref = ref.init_ref(lat, 2, pt, P)
    assert torch.equal(_bits(x.cpu()), _bits(x_ref)), "x holds the noise exactly"
    assert torch.equal(_bits(cols.cpu()), _bits(cols_ref)), "cols"
    # what the model's own forward feeds its patch embedding with for the same noise
    own = ops.cog_patchify(lat.to(dev, bf16), 2) if pt == 1 else patches_3d(lat.to(dev, bf16), 2, pt)
    for p in range(P):
        assert torch.equal(_bits(cols[p * B * S:(p + 1) * B * S].cpu()), _bits(own.reshape(B * S, Kc).cpu())), p


# ---- 2. step -----------------------------------------------------------------------------------------------------------------------------------------------------
def _pred(B, S, Kc, P, g):
    """u and c on the 1 / 64 grid, |.| <= 4.04: pred differs from column to column (steps of 1 / 8) and from token to token."""
    tok = torch.arange(B * S, dtype=torch.float32).view(B, S, 1)
    cond = ((torch.arange(Kc, dtype=torch.float32) % 64 - 31.5) / 8 + (tok % 7) / 64 + (torch.arange(Kc) // 64).float() / 32).to(bf16)
    if P == 1:
        return cond
    return torch.cat([(torch.randint(-256, 257, (B, S, Kc), generator=g).float() / 64).to(bf16), cond])


@pytest.mark.parametrize("guidance", [1.0, 6.0])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F_,H,W,pt", GRIDS)
def test_step_with_dyadic_coefficients_against_fp64(F_, H, W, pt, B, guidance):
    """x within 2 fp32 ulps of the fp64 result rounded to fp32.  The inputs are built so that the bound follows from the kernel's roundings: the coefficients
    are dyadic (cx = 7/8 or 15/16, cv = -1/8 or -1/16: their fp32 casts are exact and cv v is exact); u and c are bf16 values of like magnitude, |.| <= 4.07,
    on the 1 / 64 grid, so c - u is exact and v = fma(g, c - u, u) carries at most one rounding (|v| <= 52.5: 2^-19 absolute, 2^-22 after the scaling by
    |cv| <= 1/8); with |x| in [16, 32), |cx x| >= 14 and |cv v| <= 6.57, so |x'| >= 7.43 and one fp32 ulp of x' is at least 2^-21: the rounding of v reaches
    x' as at most half an ulp, the fma adds half an ulp, the reference's own rounding to fp32 another half -- 1.5 ulps.  pred[token, j] steps by 1 / 8 from
    column to column and differs from token to token, so a misplaced element moves x by at least |cv| / 64 = 2^-10, thousands of ulps."""
    from finetrainers_amd import ops

    dev = _dev()
    P = 2 if guidance != 1.0 else 1
    geo = _geo(B, P, F_, H, W, pt)
    S, Kc = _dims(F_, H, W, pt)
    g = torch.Generator().manual_seed(S + B)
    pred = _pred(B, S, Kc, P, g)
    x0 = (16 + 16 * torch.rand(B, S, Kc, generator=g)) * (torch.randint(0, 2, (B, S, Kc), generator=g) * 2 - 1).float()
    coef = torch.tensor([[0.875, -0.125], [0.9375, -0.0625]])
    step = B - 1  # both rows of the table are read over the cases
    sentinel = torch.full((P * B * S, Kc), -7.0, dtype=bf16)
    x, cols = x0.to(dev), sentinel.to(dev)
    ops.cog_sample_step(geo, pred.to(dev), x, coef.to(dev), step, guidance, cols)
    torch.cuda.synchronize()
    x, cols = x.cpu(), cols.cpu()
    want = ref.step_ref(pred, x0, float(coef[step, 0]), float(coef[step, 1]), guidance).float()  # fp64, rounded to fp32
    ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
    err = (x.double() - want.double()).abs() / ulp.double()
    print(f"[cog_sample_step dyadic B={B} S={S} Kc={Kc} g={guidance}] max error {float(err.max()):.2f} ulp, min |x'| {float(want.abs().min()):.2f}")
    assert bool(torch.isfinite(x).all()) and float(err.max()) <= 2.0
    assert not torch.equal(x, x0)
    rne = x.to(bf16).view(B * S, Kc)
    for p in range(P):
        assert torch.equal(_bits(cols[p * B * S:(p + 1) * B * S]), _bits(rne)), p
    # the copies-only form: x untouched, bf16(x) in every row group
    cols2, xg = sentinel.to(dev), x.to(dev)
    ops.cog_sample_step(geo, None, xg, None, 0, guidance, cols2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(xg.cpu()), _bits(x)) and torch.equal(_bits(cols2.cpu()), _bits(cols))


@pytest.mark.parametrize("guidance", [1.0, 6.0])
@pytest.mark.parametrize("F_,H,W,pt", [(3, 4, 6, 1), (2, 4, 8, 2)])
def test_step_with_the_schedulers_coefficients_against_fp64(F_, H, W, pt, guidance):
    """Every row of ``cog_ddim_tables(4)`` against fp64 with the UNROUNDED coefficients.  A derived bound, not a measured one: the fp32 casts of cx and cv
    (2^-24 relative each), the rounding of v (2^-24 |v|, scaled by |cv|), the product cv v (2^-24 |cv v|), the fma (2^-24 |x'| <= 2^-24 (|cx x| + |cv v|)) and
    the reference's own rounding (the same) give, to first order, 2^-24 (3 |cx x| + 5 |cv v|); asserted: |x - want| <= 6 2^-24 (|cx x| + |cv v|), the five
    rounded up for the second-order terms.  (c - u of two bf16 values is exact in fp32 unless their exponents are more than 16 apart.)"""
    from finetrainers_amd import ops
    from finetrainers_amd.cogvideox import cog_ddim_tables
    from finetrainers_amd.cogvideox.sampler import cog_ddim_coefficients_f64

    dev = _dev()
    B, P = 2, 2 if guidance != 1.0 else 1
    geo = _geo(B, P, F_, H, W, pt)
    S, Kc = _dims(F_, H, W, pt)
    g = torch.Generator().manual_seed(S)
    _, coef = cog_ddim_tables(4)
    _, coef64 = cog_ddim_coefficients_f64(4)
    coef_dev = coef.to(dev)
    for i in range(4):
        pred = torch.randn(P * B, S, Kc, generator=g).to(bf16)
        x0 = torch.randn(B, S, Kc, generator=g)
        x = x0.to(dev)
        ops.cog_sample_step(geo, pred.to(dev), x, coef_dev, i, guidance, None)
        torch.cuda.synchronize()
        cx, cv = float(coef64[i, 0]), float(coef64[i, 1])
        want = ref.step_ref(pred, x0, cx, cv, guidance)
        pr = pred.double()
        v = pr if P == 1 else pr[:B] + guidance * (pr[B:] - pr[:B])
        bound = 6 * 2.0 ** -24 * ((cx * x0.double()).abs() + (cv * v).abs())
        err = (x.cpu().double() - want).abs()
        print(f"[cog_sample_step n=4 step {i} g={guidance}] cx {cx:.6f} cv {cv:.6f} max err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())


# ---- 3. finish ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F_,H,W,pt,drop", [(1, 2, 2, 1, 0), (3, 4, 6, 1, 0), (2, 4, 8, 1, 0), (2, 4, 8, 2, 0), (2, 4, 8, 2, 1), (4, 4, 6, 2, 1)])
def test_finish_scales_drops_and_inverts_init(F_, H, W, pt, drop, B):
    """Within one bf16 rounding of x k in fp64 (half a bf16 ulp is at most 2^-8 relative; the fp32 cast of k and the fp32 product add 2^-23); with k = 1 and
    bf16-exact x the exact inverse of init; the dropped leading frames are absent, and a sentinel on both sides of the output stays untouched."""
    from finetrainers_amd import _lib, ops

    dev = _dev()
    S, Kc = _dims(F_, H, W, pt)
    geo = _geo(B, 1, F_, H, W, pt, drop)
    lat = torch.randn(B, F_, C, H, W, generator=torch.Generator().manual_seed(F_ + W + B))
    x, _ = ops.cog_sample_init(geo, lat.to(dev))
    k = 1.0 / 1.15258426
    out = ops.cog_sample_finish(geo, x, k)
    torch.cuda.synchronize()
    assert out.shape == (B, F_ - drop, C, H, W) and out.dtype == bf16
    want = ref.finish_ref(ref.patchify(lat, 2, pt), k, F_, C, H, W, 2, pt, drop)
    assert bool(((out.cpu().double() - want).abs() <= (2.0 ** -8 + 2.0 ** -22) * want.abs()).all())
    # exact inverse, written between two sentinel stretches through the C entry point
    latb = lat.to(bf16)
    xb, _ = ops.cog_sample_init(geo, latb.float().to(dev))
    n, guard = B * (F_ - drop) * C * H * W, 64
    buf = torch.full((n + 2 * guard,), -7.0, dtype=bf16, device=dev)
    _lib.check(_lib.load().ftmi_cog_sample_finish(ctypes.byref(geo), _lib.ptr(xb), 1.0, buf.data_ptr() + 2 * guard, _lib.stream_ptr()), "ftmi_cog_sample_finish")
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert torch.equal(_bits(buf[guard:guard + n]), _bits(latb[:, drop:].contiguous().view(-1)))
    assert bool((buf[:guard] == -7.0).all()) and bool((buf[guard + n:] == -7.0).all())


# ---- 4. the loop -------------------------------------------------------------------------------------------------------------------------------------------------
CLIP = (3, 8, 12)  # 72 video tokens + 16 text tokens: 88 joint keys, ragged
N_STEPS = 4


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(kind):
        if kind not in cache:
            omodel = ref.oracle_model(kind)
            cache[kind] = (omodel, ref.gpu_model(omodel, kind, _dev()))
        return cache[kind]

    return get


def _case(kind, B=1, seed=21):
    F_, H, W = CLIP
    pt = 2 if kind == "1.5" else 1
    drop = (pt - F_ % pt) % pt  # 1.5: 3 frames -> 4 drawn, the first dropped after the loop
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(B, F_ + drop, C, H, W, generator=g).to(bf16).float()  # bf16-exact: the bf16 oracle, the fp32 oracle and the kernels start from one state
    text = torch.randn(B, 16, 4096, generator=g).to(bf16)
    neg = torch.randn(B, 16, 4096, generator=g).to(bf16)
    return dict(noise=noise, text=text, neg=neg, pt=pt, drop=drop)


def _one_call(sampler, c, guidance, n=N_STEPS):
    """``MI355XCogVideoXLatentSampler.sample`` step by step, keeping the fp32 state: -> (x fp32 [B, S, Kc], denormalised latents, workspace bytes)."""
    from finetrainers_amd import ops
    from finetrainers_amd.cogvideox import cog_ddim_tables

    dev = _dev()
    ts, coef = cog_ddim_tables(n, sampler.scheduler_config)
    noise = c["noise"].to(dev)
    B, F_, _, H, W = noise.shape
    geo = sampler.geometry(B, F_, H, W, guidance != 1.0, c["drop"])
    text = (c["text"] if guidance == 1.0 else torch.cat([c["neg"], c["text"]])).to(dev)
    temb, shift, onep = sampler.step_tables(ts, geo.P * B)
    cfg, w, keep = sampler.c_arguments(geo, n, guidance)
    x, cols = ops.cog_sample_init(geo, noise)
    ops.cog_sample(cfg, w, cols, x, text, temb, shift, onep, coef.to(dev))
    out = ops.cog_sample_finish(geo, x, 1.0 / 1.15258426)
    torch.cuda.synchronize()
    return x, out, ops.cog_sample_workspace_bytes(cfg)


def _composition(gmodel, c, guidance, n=N_STEPS):
    """The same loop from the model's training forward (under no_grad) and ``ops.cog_sample_step``: one Python round trip per launch group."""
    from finetrainers_amd import ops
    from finetrainers_amd.cogvideox import cog_ddim_tables
    from finetrainers_amd.cogvideox.model import rotary_tables

    dev = _dev()
    ts, coef = cog_ddim_tables(n)
    coef = coef.to(dev)
    noise = c["noise"].to(dev)
    B, F_, _, H, W = noise.shape
    pt, P = c["pt"], 2 if guidance != 1.0 else 1
    geo = ops.cog_sample_geometry(B, C, F_, H, W, patch=2, patch_t=pt if pt > 1 else None, guidance=P == 2, drop=c["drop"])
    text = (c["text"] if P == 1 else torch.cat([c["neg"], c["text"]])).to(dev)
    rope = tuple(t.to(dev) for t in rotary_tables(gmodel.config, H, W, F_)) if gmodel.config.use_rotary_positional_embeddings else None
    x, cols = ops.cog_sample_init(geo, noise)
    S = cols.shape[0] // (P * B)
    with torch.no_grad():
        for i, t in enumerate(ts.tolist()):
            inp = ref.unpatchify(cols[:B * S].view(B, S, -1), F_, C, H, W, 2, pt)  # bf16(x), as the pipeline hands the latents to the transformer
            inp = torch.cat([inp] * P)
            vel = gmodel(inp, text, torch.full((P * B,), t, dtype=torch.int64, device=dev), image_rotary_emb=rope)[0]
            ops.cog_sample_step(geo, ref.patchify(vel, 2, pt), x, coef, i, guidance, cols)
    out = ops.cog_sample_finish(geo, x, 1.0 / 1.15258426)
    torch.cuda.synchronize()
    return x, out


@pytest.mark.parametrize("guidance", [6.0, 1.0])
@pytest.mark.parametrize("kind", ["sincos", "rotary", "1.5", "plain"])
def test_one_call_loop_is_its_composition_bit_for_bit(models, kind, guidance):
    """``ftmi_cog_sample`` issues the launches of ``model.forward`` + ``ops.cog_sample_step`` in their order: the state and the result are the same bits.
    (guidance 1: the conditional rows only.)"""
    from finetrainers_amd.cogvideox import MI355XCogVideoXLatentSampler

    _, gmodel = models(kind)
    c = _case(kind, B=2 if kind == "sincos" else 1)
    x1, out1, _ = _one_call(MI355XCogVideoXLatentSampler(gmodel), c, guidance)
    x2, out2 = _composition(gmodel, c, guidance)
    F_ = CLIP[0]
    assert out1.shape == (c["noise"].shape[0], F_, C, CLIP[1], CLIP[2]), "the padded leading frame is dropped"
    assert bool(torch.isfinite(x1).all())
    diff = int((_bits(x1.cpu()) != _bits(x2.cpu())).sum())
    print(f"[cog_sample vs composition {kind} g={guidance}] differing state elements: {diff} of {x1.numel()}")
    assert diff == 0 and torch.equal(_bits(out1.cpu()), _bits(out2.cpu()))
    assert float((x1.cpu() - ref.patchify(c["noise"], 2, c["pt"])).norm() / c["noise"].norm()) > 0.1, "the loop moved the state"


def test_public_sample_is_the_one_call_and_sees_the_adapters_as_they_are(models):
    from finetrainers_amd.cogvideox import MI355XCogVideoXLatentSampler

    _, gmodel = models("rotary")
    c = _case("rotary", seed=5)
    dev = _dev()
    sampler = MI355XCogVideoXLatentSampler(gmodel)
    run = lambda s: s.sample(c["noise"].to(dev), c["text"].to(dev), c["neg"].to(dev), num_inference_steps=N_STEPS)
    first = run(sampler)
    _, direct, _ = _one_call(sampler, c, 6.0)
    assert torch.equal(_bits(first.cpu()), _bits(direct.cpu()))
    saved = gmodel.lora_flat.clone()
    try:
        with torch.no_grad():
            n = gmodel.lora_flat.numel() // 2
            gmodel.lora_flat[n:].mul_(2.0)  # an optimiser step between two samples: the up-projections doubled
        second = run(sampler)
        fresh = run(MI355XCogVideoXLatentSampler(gmodel))
        torch.cuda.synchronize()
        assert not torch.equal(_bits(second.cpu()), _bits(first.cpu())), "the second call read the adapters again"
        assert torch.equal(_bits(second.cpu()), _bits(fresh.cpu()))
    finally:
        with torch.no_grad():
            gmodel.lora_flat.copy_(saved)


def test_workspace_is_forward_only(models):
    """bytes(L = 4) - bytes(L = 2) is exactly two blocks' modulation bytes (the GEMM's output rows and the tables; every entry here is a multiple of 256
    bytes), and the plan is below the training workspace at the same shape from L = 2 on."""
    from finetrainers_amd import _lib, ops
    from finetrainers_amd.cogvideox import MI355XCogVideoXLatentSampler

    _, gmodel = models("sincos")
    sampler = MI355XCogVideoXLatentSampler(gmodel)
    geo = sampler.geometry(1, *CLIP, True)
    cfg, _, _ = sampler.c_arguments(geo, N_STEPS, 6.0)
    rows, D, N = 2, 1920, 16 + 72

    def both(L):
        cfg.L = L
        train = _lib.CogConfig(B=rows, T=16, S=72, D=D, H=30, L=L, D_ff=4 * D, D_temb=512, r=64, lora_scale=cfg.lora_scale, eps_norm=1e-5, eps_qk=1e-6, gemm_variant=8)
        return ops.cog_sample_workspace_bytes(cfg), int(_lib.load().ftmi_cog_workspace_bytes(ctypes.byref(train)))

    (s2, t2), (s4, t4), (s30, t30) = both(2), both(4), both(30)
    assert s4 - s2 == 2 * (rows * 2 * 6 * D * 2 + 2 * 3 * rows * 2 * D * 2)
    assert s2 < t2 and s4 < t4 and s30 < t30 // 10
    print(f"[cog_sample workspace, {rows} x {N} tokens] L=2: {s2} vs training {t2}; L=30: {s30} vs {t30}")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_trajectory_against_the_oracle(models):
    """The pipeline loop over ``oracle.cogvideox`` twice -- in bf16 with the state rounded to bf16 after every step, as upstream does, and as an fp32 copy of the
    same weights -- and ``ftmi_cog_sample``: d_kernel = rel_l2(kernels, fp32) may not exceed 1.5 d_oracle = 1.5 rel_l2(bf16, fp32), the factor of the LTX and
    Wan trajectory tests against the same kind of yardstick.  The state must have moved by more than 0.1 relative, so that a loop that does nothing fails.
    Measured on an MI355X: d_oracle 1.459e-2, d_kernel 1.450e-2, the state moved by 0.845."""
    from finetrainers_amd.cogvideox import CogVideoXDDIMTables, MI355XCogVideoXLatentSampler

    omodel, gmodel = models("sincos")
    c = _case("sincos", seed=33)
    sched = ref.ddim_schedule(N_STEPS, CogVideoXDDIMTables(snr_shift_scale=3.0, rescale_betas_zero_snr=True).alphas_cumprod)
    t16 = ref.trajectory(omodel, bf16, c["noise"], c["text"], c["neg"], sched, 6.0, round_state=True).float()
    t32 = ref.trajectory(ref.fp32_copy(omodel), torch.float32, c["noise"], c["text"], c["neg"], sched, 6.0, round_state=False)
    x, _, _ = _one_call(MI355XCogVideoXLatentSampler(gmodel), c, 6.0)
    got = ref.unpatchify(x.cpu(), CLIP[0], C, CLIP[1], CLIP[2])
    d_oracle, d_kernel, moved = _rel(t16, t32), _rel(got, t32), _rel(t32, c["noise"])
    print(f"[cog_sample trajectory n={N_STEPS} g=6] d_oracle {d_oracle:.3e} d_kernel {d_kernel:.3e} moved {moved:.3f}")
    assert moved > 0.1 and _rel(got, c["noise"]) > 0.1
    assert d_kernel <= 1.5 * d_oracle


# ---- 5. one layout, two entry families -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F_,H,W", [(1, 2, 2), (3, 4, 6), (2, 4, 8)])
def test_wan_and_cog_entry_points_are_one_layout(F_, H, W, B, P):
    """A geometry both families can express -- C = 16, patch (1, 2, 2), Kp = Kc = 64, one copy, no extra channels, nothing dropped -- through
    ``wan_sample_*`` on latents [B, C, F, H, W] and through ``cog_sample_*`` on the same values permuted to [B, F, C, H, W]: the same bits.  (1, 2, 2) is one
    token; (3, 4, 6) has runs of 12 elements that start off the 16-byte grid (the covering vectors of init, the element stores of finish); (2, 4, 8) is the
    16-byte store path of finish.  Wan's finish runs with mean = 0, std = 1 and CogVideoX's with k = 1: x * 1 + 0 and x * 1 differ only for x = -0 (-0 + 0
    is +0), and seeded randn draws hold no zero of either sign (asserted), so the two affines agree exactly here."""
    from finetrainers_amd import ops

    dev = _dev()
    lat = torch.randn(B, C, F_, H, W, generator=torch.Generator().manual_seed(F_ * 11 + W + B))
    assert bool((lat != 0).all())
    wgeo = ops.wan_sample_geometry(B, C, F_, H, W, Kp=64, guidance=P == 2)
    cgeo = _geo(B, P, F_, H, W, 1)
    xw, colsw = ops.wan_sample_init(wgeo, lat.to(dev))
    xc, colsc = ops.cog_sample_init(cgeo, lat.permute(0, 2, 1, 3, 4).contiguous().to(dev))
    torch.cuda.synchronize()
    assert xw.shape == xc.shape and colsw.shape == colsc.shape
    assert torch.equal(_bits(xw.cpu()), _bits(xc.cpu())), "x"
    assert torch.equal(_bits(colsw.cpu()), _bits(colsc.cpu())), "cols"
    outw = ops.wan_sample_finish(wgeo, xw, torch.zeros(C, device=dev), torch.ones(C, device=dev))  # [B, C, F, H, W]
    outc = ops.cog_sample_finish(cgeo, xw, 1.0)  # [B, F, C, H, W]
    torch.cuda.synchronize()
    assert torch.equal(_bits(outw.permute(0, 2, 1, 3, 4).cpu()), _bits(outc.cpu())), "finish"
    assert torch.equal(_bits(outw.cpu()), _bits(lat.to(bf16))), "and both are the inverse of init"
