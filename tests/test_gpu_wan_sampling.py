"""Wan latent sampling on the GPU: the three layout kernels against tests/wan_sampling_reference.py (bit for bit where the arithmetic is exact, against fp64
where it rounds), the one-call loop against its composition from ``model.forward`` and ``ops.wan_sample_step`` bit for bit for the three recipes, the
trajectory against ``oracle.wan`` in bf16 and fp32, and the sampler's view of live adapters."""
import copy
import ctypes

import pytest
import torch

import wan_sampling_reference as ref

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
C = 16
# (stored patch width Kp, extra channels, copies): text-to-video, image-to-video (144 of 192 columns used), control with the folded adapter ([cols | cols])
LAYOUTS = {"t2v": (64, 0, 1), "i2v": (192, 20, 1), "control": (128, 16, 2)}
GRIDS = [(1, 2, 2), (3, 4, 6)]  # one token; 18 tokens (no multiple of any tile, W = 6: runs of 12 elements that start off the 16-byte grid)


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def _geo(layout, B, P, F_, H, W):
    from finetrainers_amd import ops

    Kp, Cx, copies = LAYOUTS[layout]
    return ops.wan_sample_geometry(B, C, F_, H, W, Kp, extra_channels=Cx, copies=copies, guidance=P == 2)


def _inputs(layout, B, F_, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, C, F_, H, W, generator=g)
    Cx = LAYOUTS[layout][1]
    extra = torch.randn(B, Cx, F_, H, W, generator=g).to(bf16) if Cx else None
    return lat, extra


# ---- 1. init -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F_,H,W", GRIDS)
def test_init_is_the_torch_patchify_bit_for_bit(F_, H, W, B, P, layout):
    from finetrainers_amd import ops

    dev = _dev()
    Kp, Cx, copies = LAYOUTS[layout]
    lat, extra = _inputs(layout, B, F_, H, W, seed=F_ * 7 + B)
    geo = _geo(layout, B, P, F_, H, W)
    S = F_ * (H // 2) * (W // 2)
    x = torch.full((B, S, 64), float("nan"), device=dev)
    cols = torch.full((P * B * S, copies * Kp), float("nan"), dtype=bf16, device=dev)  # every column must be written, the padding included
    ops.wan_sample_init(geo, lat.to(dev), None if extra is None else extra.to(dev), x=x, cols=cols)
    torch.cuda.synchronize()
    x_ref, cols_ref = ref.init_ref(lat, extra, Kp, copies, P)
    assert torch.equal(_bits(x.cpu()), _bits(x_ref)), "x"
    assert torch.equal(_bits(cols.cpu()), _bits(cols_ref)), "cols"
    used = 64 + 4 * Cx
    if used < Kp:  # exact +0: no sign bit
        assert not bool((_bits(cols[:, used:Kp].cpu()) != 0).any())
    if copies == 2:
        assert torch.equal(_bits(cols[:, :Kp].cpu()), _bits(cols[:, Kp:].cpu()))


# ---- 2. step -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("guidance", [1.0, 5.0])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F_,H,W", GRIDS)
def test_step_against_fp64(F_, H, W, B, guidance, layout):
    """x within 2 fp32 ulps of the fp64 result rounded to fp32.  The inputs are built so that the bound follows from the kernel's roundings: sigmas are dyadic
    (sigma_next - sigma is exact), c - u is exact (two bf16 values of like magnitude), so v = fma(g, c - u, u) and x = fma(dt, v, x) carry one rounding each;
    with |x| in [16, 32), |u|, |c| <= 4 and |dt| <= 1 / 8, |dt v| <= 5.5 and |x'| >= 10.5: the first rounding reaches x' as at most 0.53 ulp, the second adds half
    an ulp, the reference's own rounding to fp32 another half -- 1.53 ulps.  pred[token, j] steps by 1 / 8 from column to column and differs from token to
    token, so a wrong permutation moves x by at least |dt| / 8 = 2^-7, thousands of ulps."""
    from finetrainers_amd import ops

    dev = _dev()
    Kp, Cx, copies = LAYOUTS[layout]
    P = 2 if guidance != 1.0 else 1
    geo = _geo(layout, B, P, F_, H, W)
    S = F_ * (H // 2) * (W // 2)
    g = torch.Generator().manual_seed(S + B)
    tok = torch.arange(B * S, dtype=torch.float32).view(B, S, 1)
    cond = ((torch.arange(64, dtype=torch.float32) - 31.5) / 8 + (tok % 7) / 64).to(bf16)  # |c| < 4.04, distinct along the columns and from token to token
    pred = cond if P == 1 else torch.cat([(torch.rand(B, S, 64, generator=g) * 8 - 4).to(bf16), cond])
    x0 = (16 + 16 * torch.rand(B, S, 64, generator=g)) * (torch.randint(0, 2, (B, S, 64), generator=g) * 2 - 1).float()
    sigma, sigma_next = torch.tensor([0.75, 0.5][:B]), torch.tensor([0.625, 0.4375][:B])  # two different steps in the batch: dt = -1/8, -1/16
    sentinel = torch.full((P * B * S, copies * Kp), -7.0, dtype=bf16)
    x, cols = x0.to(dev), sentinel.to(dev)
    ops.wan_sample_step(geo, pred.to(dev), x, sigma.to(dev), sigma_next.to(dev), guidance, cols)
    torch.cuda.synchronize()
    x, cols = x.cpu(), cols.cpu()
    want = ref.step_ref(pred, x0, sigma, sigma_next, guidance, C).float()  # fp64, rounded to fp32
    ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
    err = (x.double() - want.double()).abs() / ulp.double()
    print(f"[wan_sample_step {layout} B={B} S={S} g={guidance}] max error {float(err.max()):.2f} ulp")
    assert bool(torch.isfinite(x).all()) and float(err.max()) <= 2.0
    assert not torch.equal(x, x0)
    rne = x.to(bf16).view(B * S, 64)
    for p in range(P):
        rows = cols[p * B * S:(p + 1) * B * S]
        for cp in range(copies):
            assert torch.equal(_bits(rows[:, cp * Kp:cp * Kp + 64]), _bits(rne)), (p, cp)
            assert torch.equal(_bits(rows[:, cp * Kp + 64:(cp + 1) * Kp]), _bits(sentinel[:B * S, 64:Kp])), "a constant column was written"
    # the copies-only form: x untouched, bf16(x) everywhere
    cols2 = sentinel.to(dev)
    xg = x.to(dev)
    ops.wan_sample_step(geo, None, xg, None, None, guidance, cols2)
    torch.cuda.synchronize()
    assert torch.equal(xg.cpu(), x) and torch.equal(_bits(cols2.cpu()), _bits(cols))


# ---- 3. finish ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F_,H,W", GRIDS + [(2, 4, 8)])  # W = 8: runs of 16 elements, the vector-store path
def test_finish_denormalises_and_inverts_init(F_, H, W, B):
    """bf16(fp64(x) std + mean) to within one bf16 rounding: round-to-nearest moves a value by at most 2^-8 of its magnitude, and the two fp32 operations
    before it (x std, + mean) by 2^-24 of |x std| + |mean| each (2^-22 covers both and their passage through the rounding)."""
    from finetrainers_amd import ops

    dev = _dev()
    lat, _ = _inputs("t2v", B, F_, H, W, seed=3 * F_ + W)
    geo = _geo("t2v", B, 1, F_, H, W)
    x, _ = ops.wan_sample_init(geo, lat.to(dev))
    zero, one = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    back = ops.wan_sample_finish(geo, x, zero, one)
    torch.cuda.synchronize()
    assert back.shape == lat.shape and back.dtype == bf16 and torch.equal(back.cpu(), lat.to(bf16)), "mean 0, std 1 inverts init exactly"
    g = torch.Generator().manual_seed(1)
    mean, std = 0.3 * torch.randn(C, generator=g), 1.0 + 2.0 * torch.rand(C, generator=g)
    out = ops.wan_sample_finish(geo, x, mean.to(dev), std.to(dev)).cpu()
    want = ref.finish_ref(x.cpu(), mean, std, C, F_, H, W)
    mag = ref.finish_ref(x.cpu().abs(), mean.abs(), std, C, F_, H, W)
    err = (out.double() - want).abs()
    bound = 2.0 ** -8 * want.abs() + 2.0 ** -22 * mag
    print(f"[wan_sample_finish B={B} {F_}x{H}x{W}] max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_mod_is_the_blocks_expression():
    """``blk.param("scale_shift_table").float() + temb.float()`` (wan/block.py) for every block and row."""
    from finetrainers_amd import ops

    dev = _dev()
    g = torch.Generator().manual_seed(2)
    tables = [torch.randn(6 * 256, generator=g).to(bf16).to(dev) for _ in range(3)]
    tproj = torch.randn(6 * 256, generator=g).to(bf16).to(dev)
    mod = ops.wan_sample_mod(tables, tproj, rows=2)
    torch.cuda.synchronize()
    want = torch.stack([(t.float() + tproj.float()).view(1, 6, 256).expand(2, 6, 256) for t in tables])
    assert mod.shape == (3, 2, 6, 256) and torch.equal(mod, want)


# ---- 4. / 5. the loop is its composition ---------------------------------------------------------------------------------------------------------------------------
F_, H, W, T = 2, 8, 12, 16  # 48 tokens


def _case(kind, dev, B=1, seed=21):
    g = torch.Generator().manual_seed(seed)
    c = dict(latents=torch.randn(B, C, F_, H, W, generator=g).to(dev), pos=torch.randn(B, T, 64, generator=g).to(bf16).to(dev),
             neg=torch.randn(B, T, 64, generator=g).to(bf16).to(dev), image=None, extra=None)
    if kind == "i2v":
        c["image"] = torch.randn(B, 5, 64, generator=g).to(bf16).to(dev)
        c["extra"] = torch.randn(B, 20, F_, H, W, generator=g).to(bf16).to(dev)
    if kind == "control":
        c["extra"] = torch.randn(B, 16, F_, H, W, generator=g).to(bf16).to(dev)
    return c


def _loop_inputs(sampler, c, sigmas, guidance):
    """What ``MI355XWanLatentSampler.sample`` computes before the loop, piece by piece."""
    from finetrainers_amd import ops

    B = c["latents"].shape[0]
    sig, ts = sampler.schedule(len(sigmas) - 1, sigmas, None)
    geo = sampler.geometry(B, F_, H, W, guidance=guidance != 1.0)
    enc = sampler.text_rows(c["pos"], c["neg"] if guidance != 1.0 else None)
    enc_img = None if c["image"] is None else sampler.transformer._embed_image(torch.cat([c["image"]] * geo.P))
    tables = sampler.step_tables(ts, geo.P * B)
    x, cols = ops.wan_sample_init(geo, c["latents"], c["extra"])
    return geo, sig, ts, enc, enc_img, tables, x, cols


def _one_call(sampler, c, sigmas, guidance):
    from finetrainers_amd import ops

    tr = sampler.transformer
    geo, sig, ts, enc, enc_img, (tproj, shift, scale), x, cols = _loop_inputs(sampler, c, sigmas, guidance)
    cfg, weights, keep = sampler.c_arguments(geo, T, 0 if enc_img is None else enc_img.shape[1], ts.numel(), guidance)
    need = ops.wan_sample_workspace_bytes(cfg)
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    ops.wan_sample(cfg, weights, cols, x, tproj, shift, scale, enc, enc_img, tr._rope(F_, H, W), sig.to(x.device), workspace=ws)
    torch.cuda.synchronize()
    return x, cols, need


@torch.no_grad()
def _composition(sampler, kind, c, sigmas, guidance):
    """The same loop from Python: ``model.forward`` at batch [unconditional, conditional] (the model patchifies the columns' values again, un-patchifies its
    output; here the output goes back to proj_out's order) and ``ops.wan_sample_step``."""
    from finetrainers_amd import ops

    tr = sampler.transformer
    dev = tr.device
    B = c["latents"].shape[0]
    sig, ts = sampler.schedule(len(sigmas) - 1, sigmas, None)
    geo = sampler.geometry(B, F_, H, W, guidance=guidance != 1.0)
    P, S = geo.P, F_ * (H // 2) * (W // 2)
    x, cols = ops.wan_sample_init(geo, c["latents"], c["extra"])
    text = torch.cat([c["neg"], c["pos"]]) if P == 2 else c["pos"]
    kw = {} if c["image"] is None else dict(encoder_hidden_states_image=torch.cat([c["image"]] * P))
    used = tr.config.in_channels * 4
    for i in range(ts.numel()):
        t = torch.full((P * B,), float(ts[i]), dtype=torch.float32, device=dev)
        if kind == "control":
            out = tr(None, t, text, patch_columns=cols, latent_shape=(P * B, F_, H, W))[0]
        else:
            hidden = ref.unpatchify(cols[:, :used].reshape(P * B, S, used), tr.config.in_channels, F_, H, W)
            out = tr(hidden, t, text, **kw)[0]
        pred = ref.pred_tokens(out).contiguous()
        ops.wan_sample_step(geo, pred, x, sig[i].expand(B).contiguous().to(dev), sig[i + 1].expand(B).contiguous().to(dev), guidance, cols)
    torch.cuda.synchronize()
    return x, cols


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(kind, layers=2):
        if (kind, layers) not in cache:
            cache[(kind, layers)] = ref.gpu_model(kind, _dev(), layers=layers)
        return cache[(kind, layers)]

    return get


@pytest.mark.parametrize("kind", ["t2v", "i2v", "ten", "control"])
def test_one_call_loop_is_its_composition_bit_for_bit(models, kind):
    """2 blocks, rank-64 adapters with non-zero B (the control model's folded patch adapter too), 3 steps, guidance 5, one sample: final state and final model
    input of ``ftmi_wan_sample`` against ``model.forward`` + ``ops.wan_sample_step`` called from Python."""
    from finetrainers_amd.wan import MI355XWanLatentSampler

    gmodel = models(kind)
    if kind == "control":
        assert gmodel.patch_lora_A is not None and float(gmodel.patch_lora_B.detach().abs().max()) > 0
    if kind == "ten":
        assert gmodel.blocks[0].lora_ffn is not None
    assert float(gmodel.blocks[0].lora_B.detach().abs().max()) > 0
    sampler = MI355XWanLatentSampler(gmodel)
    c = _case(kind, _dev())
    sigmas = [1.0, 0.7, 0.35, 0.0]
    x1, cols1, _ = _one_call(sampler, c, sigmas, 5.0)
    x2, cols2 = _composition(sampler, kind, c, sigmas, 5.0)
    x0 = ref.patchify(c["latents"].cpu())
    print(f"[wan_sample {kind}] one call vs composition: x {ref.rel_l2(x1, x2):.2e}; moved from the noise by {ref.rel_l2(x1, x0):.3f}")
    assert bool(torch.isfinite(x1).all()) and ref.rel_l2(x1, x0) > 0.05
    assert torch.equal(_bits(x1), _bits(x2)), "final state"
    assert torch.equal(_bits(cols1), _bits(cols2)), "final model input"
    assert torch.equal(_bits(cols1[:48, :64]), _bits(x1.to(bf16).view(48, 64)))


def test_guidance_1_runs_the_conditional_rows_only(models):
    from finetrainers_amd.wan import MI355XWanLatentSampler

    sampler = MI355XWanLatentSampler(models("t2v"))
    c = _case("t2v", _dev(), seed=5)
    sigmas = [1.0, 0.6, 0.0]
    x1, cols1, ws_one = _one_call(sampler, c, sigmas, 1.0)
    assert cols1.shape == (48, 64)
    x2, cols2 = _composition(sampler, "t2v", c, sigmas, 1.0)
    assert torch.equal(_bits(x1), _bits(x2)) and torch.equal(_bits(cols1), _bits(cols2))
    _, _, ws_two = _one_call(sampler, c, sigmas, 5.0)
    assert 0 < ws_one < ws_two


# ---- 6. the trajectory ---------------------------------------------------------------------------------------------------------------------------------------------
def test_trajectory_against_the_oracle():
    """Text-to-video, 2 blocks, rank-64 adapters (B ~ N(0, 0.02)) in both models, sigmas [1, .75, .5, .25, 0], guidance 5.  The oracle runs the loop of
    tests/wan_sampling_reference.py twice -- in bf16 and as an fp32 copy of the same weights; d_oracle = rel_l2(bf16 oracle, fp32 oracle) is the distance the
    reference's own dtype puts between itself and exact arithmetic, d_kernel = rel_l2(ftmi_wan_sample, fp32 oracle).  d_kernel <= 1.5 d_oracle: at block level
    the kernels sit slightly closer to fp32 than the bf16 oracle (4.2e-3 against 4.6e-3), the factor covers four steps of compounding with another summation
    order; a wrong rounding point or a permuted column moves the result by order 1.  Measured on an MI355X: see BASELINE.md."""
    from finetrainers_amd.wan import MI355XWanLatentSampler

    dev = _dev()
    omodel, gmodel = ref.t2v_pair(dev)
    c = _case("t2v", dev, seed=33)
    sigmas, g = [1.0, 0.75, 0.5, 0.25, 0.0], 5.0
    lat, pos, neg = c["latents"].cpu(), c["pos"].cpu(), c["neg"].cpu()
    x_bf = ref.trajectory(omodel, bf16, lat, neg, pos, sigmas, g)
    x_32 = ref.trajectory(copy.deepcopy(omodel).float(), torch.float32, lat, neg, pos, sigmas, g)
    x_k, _, _ = _one_call(MI355XWanLatentSampler(gmodel), c, sigmas, g)
    d_oracle, d_kernel = ref.rel_l2(x_bf, x_32), ref.rel_l2(x_k, x_32)
    move = ref.rel_l2(x_32, ref.patchify(lat))
    print(f"[wan latent sampling trajectory] d_oracle (bf16 oracle vs fp32 oracle) {d_oracle:.3e}; d_kernel (ftmi_wan_sample vs fp32 oracle) {d_kernel:.3e}; "
          f"ratio {d_kernel / d_oracle:.2f}; the trajectory moves the state by {move:.3f}")
    assert d_oracle == d_oracle and 0.0 < d_oracle < float("inf")
    assert move > 0.1
    assert d_kernel <= 1.5 * d_oracle


# ---- 7. live adapters ----------------------------------------------------------------------------------------------------------------------------------------------
def test_sampler_sees_the_adapters_as_they_are(models):
    from finetrainers_amd.wan import MI355XWanControlModelSpecification, MI355XWanLatentSampler

    dev = _dev()
    gmodel = models("control")
    sampler = MI355XWanLatentSampler(gmodel)
    c = _case("control", dev, seed=9)
    g = torch.Generator().manual_seed(4)
    mean, std = 0.1 * torch.randn(C, generator=g), 1.0 + torch.rand(C, generator=g)

    def run():
        gen = torch.Generator(device=dev).manual_seed(1234)
        out = sampler.sample(c["pos"], c["neg"], F_, H, W, num_inference_steps=2, guidance_scale=5.0, generator=gen, latents_mean=mean, latents_std=std,
                             control_latents=c["extra"])
        torch.cuda.synchronize()
        return out

    first = run()
    assert first.shape == (1, C, F_, H, W) and first.dtype == bf16 and bool(torch.isfinite(first.float()).all())
    assert torch.equal(_bits(first), _bits(run())), "one seed, one result"
    blk_b, patch_b = gmodel.blocks[1].lora_B.detach().clone(), gmodel.patch_lora_B.detach().clone()
    with torch.no_grad():
        gmodel.blocks[1].lora_B.mul_(3.0)
    moved_block = run()
    with torch.no_grad():
        gmodel.blocks[1].lora_B.copy_(blk_b)
        gmodel.patch_lora_B.mul_(-2.0)
    gmodel.mark_patch_adapter_updated()
    moved_patch = run()
    assert not torch.equal(_bits(first), _bits(moved_block)), "a changed block adapter must show"
    assert not torch.equal(_bits(first), _bits(moved_patch)), "a changed patch adapter must show (it is folded again)"
    with torch.no_grad():
        gmodel.patch_lora_B.copy_(patch_b)
    gmodel.mark_patch_adapter_updated()
    assert torch.equal(_bits(first), _bits(run())), "restored adapters, the first result's bits"
    # the control specification's thin method: full conditioning of already-normalised latents (mean 0, std 1 here) is this sampler call
    spec = MI355XWanControlModelSpecification(pretrained_model_name_or_path=None)
    via_spec = spec.validation_latents(gmodel, c["pos"], c["neg"], c["extra"], F_, H, W, torch.zeros(C), torch.ones(C), num_inference_steps=2,
                                       generator=torch.Generator(device=dev).manual_seed(1234))
    gen = torch.Generator(device=dev).manual_seed(1234)
    direct = sampler.sample(c["pos"], c["neg"], F_, H, W, num_inference_steps=2, generator=gen, control_latents=c["extra"])
    assert torch.equal(_bits(via_spec), _bits(direct))


# ---- 8. forward-only memory ----------------------------------------------------------------------------------------------------------------------------------------
def test_workspace_does_not_grow_with_the_blocks(models):
    from finetrainers_amd import _lib, ops
    from finetrainers_amd.wan import MI355XWanLatentSampler

    lib = _lib.load()
    sizes = {}
    for layers in (2, 4):
        sampler = MI355XWanLatentSampler(models("t2v", layers))
        geo = sampler.geometry(1, F_, H, W, guidance=True)
        cfg, _, _ = sampler.c_arguments(geo, T, 0, 3, 5.0)
        assert cfg.L == layers
        sizes[layers] = ops.wan_sample_workspace_bytes(cfg)
    blk = _lib.WanLoraFfnBlockConfig(B=2, S=48, T=T, D=256, H=2, F=512, eps=1e-6, gemm_variant=8, r=64, lora_scale=1.0, TI=0, ffn=0)
    saved = lib.ftmi_wan_lora_ffn_block_saved_bytes(ctypes.byref(blk))
    print(f"[wan_sample workspace] {sizes[4]} bytes at 2 and at 4 blocks; one block's saved activations {saved} bytes")
    assert sizes[4] == sizes[2] and sizes[4] < 4 * saved
    # and the 4-block model samples inside it
    sampler = MI355XWanLatentSampler(models("t2v", 4))
    x, _, need = _one_call(sampler, _case("t2v", _dev()), [1.0, 0.5, 0.0], 5.0)
    assert need == sizes[4] and bool(torch.isfinite(x).all())
