"""Torch restatement of the Wan latent sampler (finetrainers_amd/wan/sampler.py, csrc/sample_layout.hip): the three layout kernels -- init, step, finish -- and
the denoising loop, on the CPU.  The loop here is the one the GPU trajectory test drives ``oracle.wan.WanTransformer3DModel`` with: the state is fp32 in the
patch embedding's column order (c, pt, ph, pw), the model output arrives in proj_out's order (pt, ph, pw, c), the guidance combine and the Euler update run in
the state's precision.  Model builders for the GPU tests live here too (the geometry of tests/test_gpu_wan_control.py)."""
import torch

bf16 = torch.bfloat16
PATCH = (1, 2, 2)
SMALL = dict(num_attention_heads=2, attention_head_dim=128, ffn_dim=512, text_dim=64)
TEN_REGEX = "blocks.*(to_q|to_k|to_v|to_out.0|ffn.net.0.proj|ffn.net.2)"
CONTROL_RECIPE = "(^patch_embedding$)|(blocks.*(to_q|to_k|to_v|to_out.0|ff.net.0.proj|ff.net.2))"


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------------------
def patchify(lat, patch=PATCH):
    """[B, C, F, H, W] -> [B, S, C pt ph pw]: tokens in (f, h, w) order, columns in (c, pt, ph, pw) order (the Conv3d weight's)."""
    B, C, F_, H, W = lat.shape
    pt, ph, pw = patch
    f, h, w = F_ // pt, H // ph, W // pw
    return lat.reshape(B, C, f, pt, h, ph, w, pw).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, f * h * w, C * pt * ph * pw)


def unpatchify(cols, C, F_, H, W, patch=PATCH):
    """The inverse of ``patchify``."""
    B = cols.shape[0]
    pt, ph, pw = patch
    f, h, w = F_ // pt, H // ph, W // pw
    return cols.reshape(B, f, h, w, C, pt, ph, pw).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(B, C, F_, H, W)


def pred_tokens(out, patch=PATCH):
    """A model output [B, C, F, H, W] -> [B, S, po] as proj_out wrote it: columns in (pt, ph, pw, c) order."""
    B, C, F_, H, W = out.shape
    pt, ph, pw = patch
    f, h, w = F_ // pt, H // ph, W // pw
    return out.reshape(B, C, f, pt, h, ph, w, pw).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(B, f * h * w, pt * ph * pw * C)


def pred_in_state_order(pred, C, patch=PATCH):
    """[..., po] in (pt, ph, pw, c) order -> the state's (c, pt, ph, pw) order: state column c pv + p is pred column p C + c."""
    pv = patch[0] * patch[1] * patch[2]
    return pred.reshape(*pred.shape[:-1], pv, C).transpose(-1, -2).reshape(*pred.shape[:-1], C * pv)


def init_ref(latents, extra, Kp, copies=1, P=1, patch=PATCH):
    """-> (x fp32 [B, S, Kc], cols bf16 [P B S, copies Kp]): bf16(x) | patchified extra | +0 padding, every row group and copy alike."""
    x = patchify(latents.float(), patch).contiguous()
    B, S, Kc = x.shape
    row = torch.zeros(B, S, Kp, dtype=bf16)
    row[..., :Kc] = x.to(bf16)
    if extra is not None:
        e = patchify(extra.to(bf16), patch)
        row[..., Kc:Kc + e.shape[-1]] = e
    cols = torch.cat([row] * copies, dim=-1)
    return x, torch.cat([cols] * P, dim=0).reshape(P * B * S, copies * Kp).contiguous()


def step_ref(pred, x, sigma, sigma_next, guidance, C, patch=PATCH, dtype=torch.float64):
    """pred [P B, S, po] (P = 2: unconditional rows first), x [B, S, Kc], sigma / sigma_next [B] -> the new x in ``dtype``:
    v = u + g (c - u) (guidance == 1: v = c), x + (sigma_next - sigma) v."""
    B = x.shape[0]
    p = pred_in_state_order(pred.to(dtype), C, patch)
    if guidance != 1.0:
        u, c = p[:B], p[B:]
        v = u + guidance * (c - u)
    else:
        v = p
    dt = (sigma_next.to(dtype) - sigma.to(dtype)).view(B, 1, 1)
    return x.to(dtype) + dt * v


def finish_ref(x, mean, std, C, F_, H, W, patch=PATCH, dtype=torch.float64):
    """x [B, S, Kc] -> (x std[c] + mean[c]) as [B, C, F, H, W] in ``dtype`` (the caller rounds)."""
    lat = unpatchify(x.to(dtype), C, F_, H, W, patch)
    return lat * std.to(dtype).view(1, C, 1, 1, 1) + mean.to(dtype).view(1, C, 1, 1, 1)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def trajectory(model, dtype, latents, text_uncond, text_cond, sigmas, guidance, num_train_timesteps=1000.0, patch=PATCH):
    """The sampler's loop over a callable with the diffusers signature, evaluated in ``dtype``: state fp32, the model sees ``dtype(state)`` un-patchified at
    batch [unconditional, conditional] with timestep sigma * num_train_timesteps, combine and update in fp32.  -> the final state fp32 [B, S, Kc]."""
    B, C, F_, H, W = latents.shape
    x = patchify(latents.float(), patch)
    two = guidance != 1.0
    text = (torch.cat([text_uncond, text_cond]) if two else text_cond).to(dtype)
    for i in range(len(sigmas) - 1):
        hidden = unpatchify(x.to(dtype), C, F_, H, W, patch)
        hidden = torch.cat([hidden, hidden]) if two else hidden
        t = torch.full((hidden.shape[0],), float(sigmas[i]) * num_train_timesteps, dtype=torch.float32)
        out = model(hidden_states=hidden, timestep=t, encoder_hidden_states=text, return_dict=False)[0]
        s, sn = torch.full((B,), float(sigmas[i])), torch.full((B,), float(sigmas[i + 1]))
        x = step_ref(pred_tokens(out, patch), x, s, sn, guidance, C, patch, dtype=torch.float32)
    return x


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


# ---- models ------------------------------------------------------------------------------------------------------------------------------------------------
def _fix(k):
    return k.replace("ffn.proj_in.", "ffn.net.0.proj.").replace("ffn.proj_out.", "ffn.net.2.")


def _oracle_base(layers, seed, i2v=False):
    from oracle import wan

    torch.manual_seed(seed)
    if i2v:
        import wan_i2v_reference as i2vref

        omodel = i2vref.WanI2VTransformer3DModel(i2vref.WanI2VConfig(num_layers=layers, image_dim=64, **SMALL))
    else:
        omodel = wan.WanTransformer3DModel(wan.WanConfig(num_layers=layers, **SMALL))
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in omodel.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return omodel.to(bf16)


def t2v_pair(device, layers=2, rank=64, alpha=64.0, seed=0):
    """(oracle model with oracle.ltx.LoraLinear on the eight attention projections of every block, B ~ N(0, 0.02); the MI355X model with the same base weights
    and adapters), as tests/test_gpu_wan_control.py loads them."""
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig
    from oracle import ltx

    omodel = _oracle_base(layers, seed)
    gmodel = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, **SMALL), device=device)
    gmodel.load_diffusers_state_dict({_fix(k): v for k, v in omodel.state_dict().items()})
    for p in omodel.parameters():
        p.requires_grad_(False)
    for blk in omodel.blocks:
        for attn in (blk.attn1, blk.attn2):
            for t in ("to_q", "to_k", "to_v"):
                setattr(attn, t, ltx.LoraLinear(getattr(attn, t), rank, alpha))
            attn.to_out[0] = ltx.LoraLinear(attn.to_out[0], rank, alpha)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in omodel.named_parameters():
            if "lora_B" in n:
                p.normal_(0, 0.02, generator=g)
    gmodel.add_adapter(rank, alpha)
    gmodel.load_lora_state_dict({n.replace(".default.", "."): p.detach() for n, p in omodel.named_parameters() if "lora_" in n})
    return omodel, gmodel


def randomize_adapters(gmodel, seed=5, std=0.02):
    """Non-zero up-projections everywhere (peft initialises them to zero), the patch adapter's included."""
    g = torch.Generator(device=gmodel.device).manual_seed(seed)
    with torch.no_grad():
        for blk in gmodel.blocks:
            blk.lora_B.normal_(0, std, generator=g)
            if blk.lora_ffn is not None:
                blk.lora_ffn[1].normal_(0, std, generator=g)
                blk.lora_ffn[3].normal_(0, std, generator=g)
        if gmodel.patch_lora_B is not None:
            gmodel.patch_lora_B.normal_(0, std, generator=g)
            gmodel.mark_patch_adapter_updated()


def gpu_model(kind, device, layers=2, rank=64, seed=0):
    """The MI355X model of one recipe with rank-``rank`` adapters whose B is non-zero: "t2v" (eight adapters), "ten" (with the feed-forward ones), "i2v"
    (image_dim 64, 36 input channels), "control" (patch embedding widened to 32 channels, folded full-rank adapter), "plain" (no adapters)."""
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig

    omodel = _oracle_base(layers, seed, i2v=kind == "i2v")
    extra = dict(image_dim=64, in_channels=36) if kind == "i2v" else {}
    gmodel = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, **SMALL, **extra), device=device)
    gmodel.load_diffusers_state_dict({_fix(k): v for k, v in omodel.state_dict().items()})
    if kind == "plain":
        return gmodel
    if kind == "control":
        gmodel.expand_patch_embedding(32)
        with torch.no_grad():  # the widened columns are zero after the expansion: give the control channels a weight so that they reach the output
            w = gmodel.rparam("patch_embedding.weight")
            w[:, 64:].copy_((0.05 * torch.randn(w.shape[0], 64, generator=torch.Generator().manual_seed(3))).to(bf16))
        D = gmodel.config.inner_dim
        gmodel.add_adapter(rank, float(rank), target_modules=CONTROL_RECIPE, rank_pattern={"patch_embedding": D}, alpha_pattern={"patch_embedding": D})
    elif kind == "ten":
        gmodel.add_adapter(rank, float(rank), target_modules=TEN_REGEX)
    else:
        gmodel.add_adapter(rank, float(rank))
    randomize_adapters(gmodel)
    return gmodel
