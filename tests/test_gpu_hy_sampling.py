"""HunyuanVideo latent sampling on the GPU: the column order of ``proj_out`` against the patch operand order, the three layout kernels (bit for bit where
the arithmetic is exact, against fp64 where it rounds), the one-call loop against its composition from ``model.forward`` and ``ops.hy_sample_step`` bit for
bit (batch, text mask, adapters, true CFG, block counts, fp8 storage), the sampler's view of live adapters, and the trajectory against ``oracle.hunyuan`` in
bf16 and fp32."""
import copy

import pytest
import torch

import hy_sampling_reference as ref

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
C = 16
# (F, H, W): one token (8 vectors under a 256-thread workgroup: the grid tail); 18 tokens with W = 6 (runs of 12 elements that start off the 16-byte grid);
# W = 8 (runs of 16 elements: the vector-store path of finish)
GRIDS = [(1, 2, 2), (3, 4, 6), (2, 4, 8)]
SMALL = dict(num_attention_heads=2, attention_head_dim=128, num_refiner_layers=1, text_embed_dim=64, pooled_projection_dim=64)
GRID, T, N_STEPS = (3, 8, 12), 8, 4  # 72 video tokens + 8 text tokens (5 real in sample 0): 80 joint keys, ragged, with masked keys


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _geo(B, P, F_, H, W):
    from finetrainers_amd import ops

    return ops.hy_sample_geometry(B, C, F_, H, W, patch=2, patch_t=1, true_cfg=P == 2)


def _dims(F_, H, W):
    return F_ * (H // 2) * (W // 2), C * 4


# ---- 1. one layout: proj_out's column order is the patch operand order; init is that patchify -------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F_,H,W", GRIDS)
def test_proj_out_columns_are_the_patch_operand_order_and_init_is_that_patchify(F_, H, W, B, P):
    """model.py patchifies with view(B, C, f, pt, h, p, w, p).permute(0, 2, 4, 6, 1, 3, 5, 7) and un-patchifies proj_out's output with
    reshape(B, f, h, w, -1, pt, p, p).permute(0, 4, 1, 5, 2, 6, 3, 7): distinct values make a bit-equal round trip, so the two column orders are one, and
    ftmi_hy_sample_init writes exactly that patchify."""
    from finetrainers_amd import ops

    dev = _dev()
    S, Kc = _dims(F_, H, W)
    p, pt = 2, 1
    f, h, w = F_ // pt, H // p, W // p
    lat = (torch.randperm(B * C * F_ * H * W, generator=torch.Generator().manual_seed(F_ + B)).float() - 1000.0).reshape(B, C, F_, H, W) / 4
    assert lat.unique().numel() == lat.numel()
    cols_model = lat.view(B, C, f, pt, h, p, w, p).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B * S, C * pt * p * p)  # model.py, the patch embedding's operand
    back = cols_model.view(B, S, -1).reshape(B, f, h, w, -1, pt, p, p).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(B, -1, F_, H, W)  # model.py, after proj_out
    assert torch.equal(_bits(back), _bits(lat)), "proj_out's columns are (c, pt, ph, pw), the patch operand order"
    assert torch.equal(cols_model.view(B, S, Kc), ref.patchify(lat)) and torch.equal(ref.unpatchify(cols_model.view(B, S, Kc), C, F_, H, W), lat)
    x = torch.full((B, S, Kc), float("nan"), device=dev)
    cols = torch.full((P * B * S, Kc), float("nan"), dtype=bf16, device=dev)
    ops.hy_sample_init(_geo(B, P, F_, H, W), lat.to(dev), x=x, cols=cols)
    torch.cuda.synchronize()
    assert torch.equal(_bits(x.cpu()), _bits(cols_model.view(B, S, Kc))), "x holds the noise exactly"
    for g in range(P):
        assert torch.equal(_bits(cols[g * B * S:(g + 1) * B * S].cpu()), _bits(cols_model.to(bf16))), g


# ---- 2. step -----------------------------------------------------------------------------------------------------------------------------------------------------
def _guarded(n, dtype, dev, fill):
    """A tensor of n elements with one sentinel row of 64 elements on either side."""
    buf = torch.full((n + 128,), fill, dtype=dtype, device=dev)
    return buf, buf[64:64 + n]


@pytest.mark.parametrize("true_cfg", [1.0, 3.0])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F_,H,W", GRIDS)
def test_step_against_fp64(F_, H, W, B, true_cfg):
    """x within 1 fp32 ulp of float32(float64(dt32) float64(v) + float64(x)), dt32 the fp32 difference of the two table entries the kernel reads: the fma
    rounds once (at most half an ulp), the other half covers the fp64 reference's own final rounding.  Derived, not measured.  With true CFG, v is the fp32
    value of the combine, d = c - u; v = fma(g, d, u): u and c sit on the 1 / 64 grid with |.| <= 4.1 and g = 3, so d, g d and g d + u are exact in fp32 and
    the fp64 evaluation below IS that fp32 value.  cols = bf16(x_new) bit for bit in every row group; the copies-only and the update-only forms; the sentinel
    rows on either side of x and cols are untouched."""
    from finetrainers_amd import ops
    from finetrainers_amd.hunyuan_video import hy_flow_match_sigmas

    dev = _dev()
    P = 2 if true_cfg != 1.0 else 1
    geo = _geo(B, P, F_, H, W)
    S, Kc = _dims(F_, H, W)
    n = B * S * Kc
    g = torch.Generator().manual_seed(S * 3 + B)
    sig32 = hy_flow_match_sigmas(N_STEPS).to(torch.float32)
    sig_dev = sig32.to(dev)
    for step in range(N_STEPS):
        if P == 1:
            pred = torch.randn(B, S, Kc, generator=g).to(bf16)
            v = pred.double()
        else:
            pred = (torch.randint(-262, 263, (2 * B, S, Kc), generator=g).float() / 64).to(bf16)
            assert torch.equal(pred.float() * 64, (pred.float() * 64).round())
            u, c = pred[:B].double(), pred[B:].double()
            v = true_cfg * (c - u) + u
            assert torch.equal(v, v.float().double())
        x0 = torch.randn(B, S, Kc, generator=g)
        xbuf, xv = _guarded(n, torch.float32, dev, -3.0)
        cbuf, cv = _guarded(P * n, bf16, dev, -7.0)
        x, cols = xv.view(B, S, Kc), cv.view(P * B * S, Kc)
        x.copy_(x0)
        ops.hy_sample_step(geo, pred.to(dev), x, sig_dev, step, true_cfg, cols)
        torch.cuda.synchronize()
        dt32 = (sig32[step + 1] - sig32[step]).double()
        want = (dt32 * v + x0.double()).float()
        ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
        err = (x.cpu().double() - want.double()).abs() / ulp.double()
        print(f"[hy_sample_step B={B} S={S} P={P} step {step}] dt {float(dt32):.6f} max error {float(err.max()):.2f} ulp")
        assert bool(torch.isfinite(x).all()) and float(err.max()) <= 1.0
        assert not torch.equal(x.cpu(), x0)
        rne = x.cpu().to(bf16).view(B * S, Kc)
        for p in range(P):
            assert torch.equal(_bits(cols[p * B * S:(p + 1) * B * S].cpu()), _bits(rne)), p
        for buf, fill in ((xbuf, -3.0), (cbuf, -7.0)):
            assert bool((buf[:64] == fill).all()) and bool((buf[-64:] == fill).all()), "sentinel rows"
        # the update-only form: the same x, cols untouched
        x2buf, x2v = _guarded(n, torch.float32, dev, -3.0)
        x2 = x2v.view(B, S, Kc)
        x2.copy_(x0)
        ops.hy_sample_step(geo, pred.to(dev), x2, sig_dev, step, true_cfg, None)
        # the copies-only form: x untouched, bf16(x) in every row group
        c3buf, c3v = _guarded(P * n, bf16, dev, -7.0)
        before = x.clone()
        ops.hy_sample_step(geo, None, x, None, 0, true_cfg, c3v.view(P * B * S, Kc))
        torch.cuda.synchronize()
        assert torch.equal(_bits(x2.cpu()), _bits(x.cpu())) and torch.equal(_bits(x.cpu()), _bits(before.cpu()))
        assert torch.equal(_bits(c3buf.cpu()), _bits(cbuf.cpu())) and bool((x2buf[:64] == -3.0).all()) and bool((x2buf[-64:] == -3.0).all())


# ---- 3. finish ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F_,H,W", GRIDS)
def test_finish_scales_and_inverts_init(F_, H, W, B):
    """Within one bf16 rounding of x k in fp64 (half a bf16 ulp is at most 2^-8 relative; the fp32 cast of k and the fp32 product add 2^-23); with k = 1 and
    bf16-exact x the exact inverse of init; a sentinel on both sides of the output stays untouched."""
    from finetrainers_amd import _lib, ops
    import ctypes

    dev = _dev()
    S, Kc = _dims(F_, H, W)
    geo = _geo(B, 1, F_, H, W)
    lat = torch.randn(B, C, F_, H, W, generator=torch.Generator().manual_seed(S + B))
    x, _ = ops.hy_sample_init(geo, lat.to(dev))
    k = 1.0 / 0.476986
    out = ops.hy_sample_finish(geo, x, k).cpu()
    want = lat.double() * k
    assert out.shape == lat.shape and bool(((out.double() - want).abs() <= want.abs() * (2.0 ** -8 + 2.0 ** -22)).all())
    assert not torch.equal(out, lat.to(bf16))
    latb = lat.to(bf16)
    xb, _ = ops.hy_sample_init(geo, latb.float().to(dev))
    n = latb.numel()
    obuf, ov = _guarded(n, bf16, dev, -7.0)
    _lib.check(_lib.load().ftmi_hy_sample_finish(ctypes.byref(geo), xb.data_ptr(), 1.0, ov.data_ptr(), torch.cuda.current_stream().cuda_stream), "finish")
    torch.cuda.synchronize()
    assert torch.equal(_bits(ov.view(lat.shape).cpu()), _bits(latb)), "k = 1: the exact inverse of init"
    assert bool((obuf[:64] == -7.0).all()) and bool((obuf[-64:] == -7.0).all())


# ---- 4. the one-call loop --------------------------------------------------------------------------------------------------------------------------------------------
def _to_diffusers_key(k):
    """oracle/hunyuan.py module names -> diffusers HunyuanVideoTransformer3DModel parameter names."""
    k = k.replace("context_embedder.refiner_blocks.", "context_embedder.token_refiner.refiner_blocks.").replace(".norm_out_linear.", ".norm_out.linear.")
    if k.startswith("norm_out_linear."):
        k = "norm_out.linear." + k[len("norm_out_linear."):]
    if k.startswith("x_embedder."):
        k = "x_embedder.proj." + k[len("x_embedder."):]
    for a in ("ff_context", "ff"):
        k = k.replace(f"{a}.proj_in.", f"{a}.net.0.proj.").replace(f"{a}.proj_out.", f"{a}.net.2.")
    return k


def _oracle(nl, ns, lora):
    from oracle import hunyuan as hy
    from oracle import ltx

    omodel = hy.build_model(hy.HunyuanVideoConfig(num_layers=nl, num_single_layers=ns, **SMALL), seed=0, dtype=torch.float32)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in omodel.named_parameters():
            if "norm" in n and n.endswith("weight") and p.dim() == 1:
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
    omodel = omodel.to(bf16)
    for p in omodel.parameters():
        p.requires_grad_(False)
    if lora:
        for blk in omodel.transformer_blocks:
            for t in ("to_q", "to_k", "to_v"):
                setattr(blk.attn, t, ltx.LoraLinear(getattr(blk.attn, t), 64, 64.0))
            blk.attn.to_out[0] = ltx.LoraLinear(blk.attn.to_out[0], 64, 64.0)
        for blk in omodel.single_transformer_blocks:
            for t in ("to_q", "to_k", "to_v"):
                setattr(blk.attn, t, ltx.LoraLinear(getattr(blk.attn, t), 64, 64.0))
        with torch.no_grad():
            for n, p in omodel.named_parameters():
                if "lora_B" in n:
                    p.normal_(0, 0.02, generator=g)
        for p in omodel.parameters():
            p.requires_grad_(False)
    return omodel


def _gpu_model(omodel, nl, ns, lora, fp8=False):
    from finetrainers_amd.hunyuan_video import HunyuanVideoTransformerConfig, MI355XHunyuanVideoTransformer3DModel

    sd = {_to_diffusers_key(k): v for k, v in omodel.state_dict().items()}
    m = MI355XHunyuanVideoTransformer3DModel(HunyuanVideoTransformerConfig(num_layers=nl, num_single_layers=ns, **SMALL), device=_dev())
    m.load_diffusers_state_dict(sd)
    if lora:
        m.add_adapter(r=64, lora_alpha=64.0)
        m.load_lora_state_dict({k: v for k, v in sd.items() if "lora_" in k})
    if fp8:
        m.apply_layerwise_casting()
    return m


@pytest.fixture(scope="module")
def models():
    o = _oracle(2, 3, True)
    out = {"oracle": o, "lora": _gpu_model(o, 2, 3, True), "fp8": _gpu_model(o, 2, 3, True, fp8=True)}
    plain = _oracle(2, 3, False)
    out["plain"] = _gpu_model(plain, 2, 3, False)
    out["single"] = _gpu_model(_oracle(0, 1, True), 0, 1, True)
    return out


def _inputs(B, masked, seed=11):
    g = torch.Generator().manual_seed(seed)
    F_, H, W = GRID
    d = {"noise": torch.randn(B, C, F_, H, W, generator=g), "text": torch.randn(B, T, 64, generator=g).to(bf16), "pooled": torch.randn(B, 64, generator=g).to(bf16),
         "neg": torch.randn(B, T, 64, generator=g).to(bf16), "neg_pooled": torch.randn(B, 64, generator=g).to(bf16), "mask": None, "neg_mask": None}
    if masked:
        m = torch.ones(B, T, dtype=torch.bool)
        m[0, 5:] = False  # 5 of the 8 text tokens of sample 0 are real
        d["mask"], d["neg_mask"] = m, torch.ones(B, T, dtype=torch.bool)
        d["neg_mask"][-1, 6:] = False
    return d


def _rows(d, g):
    """The model-batch inputs: unconditional rows first with true CFG."""
    dev = _dev()
    if g == 1.0:
        return d["text"].to(dev), d["pooled"].to(dev), None if d["mask"] is None else d["mask"].to(dev)
    mask = None if d["mask"] is None else torch.cat([d["neg_mask"], d["mask"]]).to(dev)
    return torch.cat([d["neg"], d["text"]]).to(dev), torch.cat([d["neg_pooled"], d["pooled"]]).to(dev), mask


def _one_call(model, d, g, guidance_scale=6.0, n=N_STEPS):
    from finetrainers_amd import ops
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoLatentSampler, hy_flow_match_sigmas

    dev = _dev()
    s = MI355XHunyuanVideoLatentSampler(model)
    B = d["noise"].shape[0]
    geo = s.geometry(B, *GRID, true_cfg=g != 1.0)
    text, pooled, mask = _rows(d, g)
    sig = hy_flow_match_sigmas(n)
    with torch.no_grad():
        temb_silu, enc, shift, onep = s.step_tables(sig, guidance_scale, text, mask, pooled)
    cfg, w, keep = s.c_arguments(geo, T, n, g)
    x, cols = ops.hy_sample_init(geo, d["noise"].to(dev))
    cos, sin = (t.contiguous() for t in model._rope(*GRID))
    ops.hy_sample(cfg, w, cols, x, temb_silu, enc, shift, onep, s.key_bias(mask, geo, T), cos, sin, sig.to(torch.float32).to(dev))
    out = ops.hy_sample_finish(geo, x, 1.0 / 0.476986)
    torch.cuda.synchronize()
    del keep
    return x.cpu(), out.cpu()


def _composition(model, d, g, guidance_scale=6.0, n=N_STEPS):
    """model.forward under no_grad at float timesteps, then ops.hy_sample_step: the launches the one call issues, call by call."""
    from finetrainers_amd import ops
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoLatentSampler, hy_flow_match_sigmas

    dev = _dev()
    s = MI355XHunyuanVideoLatentSampler(model)
    B = d["noise"].shape[0]
    F_, H, W = GRID
    geo = s.geometry(B, F_, H, W, true_cfg=g != 1.0)
    S, Kc = _dims(F_, H, W)
    text, pooled, mask = _rows(d, g)
    rows = text.shape[0]
    sig = hy_flow_match_sigmas(n)
    sig_dev = sig.to(torch.float32).to(dev)
    guidance = torch.full((rows,), guidance_scale, dtype=bf16, device=dev) * 1000.0
    x, cols = ops.hy_sample_init(geo, d["noise"].to(dev))
    for i, t in enumerate(s.timesteps(sig).tolist()):
        lat = ref.unpatchify(cols.view(rows, S, Kc), C, F_, H, W)
        with torch.no_grad():
            v = model(lat, torch.full((rows,), t, dtype=torch.float32, device=dev), text, mask, pooled, guidance=guidance)[0]
        ops.hy_sample_step(geo, ref.patchify(v).contiguous(), x, sig_dev, i, g, cols)
    out = ops.hy_sample_finish(geo, x, 1.0 / 0.476986)
    torch.cuda.synchronize()
    return x.cpu(), out.cpu()


CASES = [("lora", 1, False, 1.0), ("lora", 2, True, 3.0), ("lora", 1, True, 3.0), ("plain", 2, True, 1.0), ("single", 1, True, 3.0), ("single", 2, False, 1.0),
         ("fp8", 2, True, 1.0), ("fp8", 1, True, 3.0)]


@pytest.mark.parametrize("kind,B,masked,true_cfg", CASES)
def test_one_call_loop_is_its_composition_bit_for_bit(models, kind, B, masked, true_cfg):
    """ftmi_hy_sample_text against model.forward + ops.hy_sample_step on the same model: state and output bit for bit.  "lora": 2 dual + 3 single blocks with
    adapters of rank 64; "plain": no adapters; "single": (Ld, Ls) = (0, 1); "fp8": apply_layerwise_casting() with real fp8 storage."""
    model = models[kind]
    d = _inputs(B, masked)
    x1, o1 = _one_call(model, d, true_cfg)
    x2, o2 = _composition(model, d, true_cfg)
    moved = _rel(x1, ref.patchify(d["noise"]))
    print(f"[hy_sample {kind} B={B} masked={masked} true_cfg={true_cfg}] moved {moved:.3f}")
    assert bool(torch.isfinite(x1).all()) and moved > 0.1
    assert torch.equal(_bits(x1), _bits(x2)), "state"
    assert torch.equal(_bits(o1), _bits(o2)), "output"


# ---- 5. the public sample ------------------------------------------------------------------------------------------------------------------------------------------
def test_public_sample_is_the_one_call_and_sees_the_adapters_as_they_are(models):
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoLatentSampler, MI355XHunyuanVideoModelSpecification

    dev = _dev()
    model = copy.deepcopy(models["lora"])
    d = _inputs(2, True)
    s = MI355XHunyuanVideoLatentSampler(model)
    kw = dict(negative_prompt_embeds=d["neg"], negative_prompt_attention_mask=d["neg_mask"], negative_pooled_prompt_embeds=d["neg_pooled"],
              num_inference_steps=N_STEPS, true_cfg_scale=3.0)
    a = s.sample(d["noise"], d["text"], d["mask"], d["pooled"], **kw).cpu()
    assert a.dtype == bf16 and a.shape == d["noise"].shape
    assert torch.equal(_bits(a), _bits(_one_call(model, d, 3.0)[1]))
    spec = MI355XHunyuanVideoModelSpecification(pretrained_model_name_or_path=None)
    via_spec = spec.validation_latents(model, d["text"], d["mask"], d["pooled"], *GRID, latents=d["noise"].to(dev), **kw).cpu()
    assert torch.equal(_bits(via_spec), _bits(a))
    with torch.no_grad():
        for blk in list(model.transformer_blocks) + list(model.single_transformer_blocks):
            blk.lora_B.mul_(2.0)
    b = s.sample(d["noise"], d["text"], d["mask"], d["pooled"], **kw).cpu()
    fresh = MI355XHunyuanVideoLatentSampler(model).sample(d["noise"], d["text"], d["mask"], d["pooled"], **kw).cpu()
    assert not torch.equal(_bits(a), _bits(b)), "the sampler reads the adapters at every call"
    assert torch.equal(_bits(b), _bits(fresh))


# ---- 6. trajectory ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_trajectory_against_the_oracle(models):
    """The loop of tests/hy_sampling_reference.py over ``oracle.hunyuan``'s model in bf16 with the state rounded to bf16 after every step, as upstream keeps
    it, over an fp32 copy of the same weights, and ``ftmi_hy_sample_text``: d_kernel = rel_l2(kernels, fp32) may not exceed 1.5 d_oracle = 1.5 rel_l2(bf16, fp32),
    the factor of the LTX, Wan and CogVideoX trajectory tests against the same kind of yardstick.  The state must have moved by more than 0.1 relative, so
    that a loop that does nothing fails.  The embedded guidance is bf16(6000) = 6016 in all three.
    Measured on an MI355X: d_oracle 3.862e-3, d_kernel 2.290e-3, the state moved by 0.579."""
    omodel = models["oracle"]
    d = _inputs(1, True)
    F_, H, W = GRID
    sig = ref.sigmas(N_STEPS)
    guidance = float((torch.full((1,), 6.0, dtype=bf16) * 1000.0)[0])
    assert guidance == 6016.0

    def run(model, dtype, round_to):
        def f(x, i, t):
            lat = ref.unpatchify(x, C, F_, H, W).to(dtype)
            with torch.no_grad():
                v = model(lat, torch.full((1,), t, dtype=torch.float32), d["text"].to(dtype), d["mask"], d["pooled"].to(dtype),
                          guidance=torch.full((1,), guidance, dtype=dtype), return_dict=False)[0]
            return ref.patchify(v.float())
        return ref.trajectory(f, ref.patchify(d["noise"]), sig, round_to=round_to)

    t16 = run(omodel, bf16, bf16)
    t32 = run(copy.deepcopy(omodel).float(), torch.float32, None)
    got, _ = _one_call(models["lora"], d, 1.0)
    d_oracle, d_kernel, moved = _rel(t16, t32), _rel(got, t32), _rel(t32, ref.patchify(d["noise"]))
    print(f"[hy_sample trajectory n={N_STEPS} guidance 6] d_oracle {d_oracle:.3e} d_kernel {d_kernel:.3e} moved {moved:.3f}")
    assert moved > 0.1
    assert d_kernel <= 1.5 * d_oracle
