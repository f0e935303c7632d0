"""LTX-Video latent sampling on the MI355X: the step and unpack kernels against exact arithmetic, the one-call denoising loop against the composition
of the entry points the parity tests already cover (bit for bit), and a trajectory against the CPU oracle.  Run on the MI355X box: pytest -m gpu."""

import ctypes
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
ROPE_SCALE = [1 / (25 / 8), 32, 32]  # specification.py forward / base_specification.py:324-334


def _dev():
    return torch.device("cuda", 0)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ---------------------------------------------------------------------------------------------------------------- a. step kernel
# (videos, elements per video): config 2's 2 688 x 128; a size that is no multiple of 8 elements x 256 threads (3 x 2 368 = 7 104 = 3.47 blocks, the
# sample boundary inside a block); one vector
STEP_SIZES = [(2, 2688 * 128), (3, 37 * 64), (1, 8)]


@pytest.mark.parametrize("guidance", [1.0, 3.0, 7.5])
@pytest.mark.parametrize("B,per", STEP_SIZES)
def test_cfg_euler_step_vs_fp64(B, per, guidance):
    from finetrainers_amd import ops

    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(B * 1000 + per % 997)
    halves = 1 if guidance == 1.0 else 2
    pred = torch.randn((halves * B, per), generator=g, device=dev).to(bf16)
    x = torch.randn((B, per), generator=g, device=dev) * 2
    sigma = torch.rand(B, generator=g, device=dev) * 0.5 + 0.5
    sigma_next = sigma * torch.rand(B, generator=g, device=dev)
    x0 = x.clone()
    xin = ops.ltx_cfg_euler_step(pred, x, sigma, sigma_next, guidance)
    torch.cuda.synchronize()

    # exact arithmetic on the kernel's own inputs
    p64 = pred.double()
    c = p64[-B:]
    u = p64[:B] if halves == 2 else torch.zeros_like(c)
    v = u + guidance * (c - u) if halves == 2 else c
    dt = (sigma_next.double() - sigma.double()).view(B, 1)
    want = x0.double() + dt * v
    # forward error bound of the kernel's four fp32 roundings (c - u, fma, sigma_next - sigma, fma), each relative 2^-24 -- derived, not measured
    bound = 4 * 2.0**-24 * (x0.double().abs() + dt.abs() * (u.abs() + abs(guidance) * (c.abs() + u.abs())))
    err = (x.double() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"[cfg_euler_step B={B} per={per} g={guidance}] max err / bound = {worst:.3f}; max abs err {err.max().item():.3e}")
    assert torch.isfinite(x).all()
    assert (err <= bound).all(), f"max err / bound = {worst}"
    assert not torch.equal(x, x0)
    # the bf16 copy: round-to-nearest-even of the kernel's OWN fp32 result, bit for bit, in every half
    assert xin.shape == pred.shape and xin.dtype == bf16
    rne = x.to(bf16)
    for h in range(halves):
        assert torch.equal(xin[h * B:(h + 1) * B].view(torch.int16), rne.view(torch.int16)), f"half {h}"


# ---------------------------------------------------------------------------------------------------------------- b. unpack
@pytest.mark.parametrize("B,C,F_,H_,W_", [(2, 128, 7, 16, 24), (1, 128, 3, 5, 5), (3, 64, 1, 2, 4)])
def test_unpack_denorm_inverts_noise_pack(B, C, F_, H_, W_):
    from finetrainers_amd import ops

    dev = _dev()
    S = F_ * H_ * W_
    g = torch.Generator(device=dev).manual_seed(S)
    lat = torch.randn((B, C, F_, H_, W_), generator=g, device=dev).to(bf16)
    noise = torch.randn((B, C, F_, H_, W_), generator=g, device=dev).to(bf16)
    zero = torch.zeros(B, device=dev)

    # mean 0, std 1: bit-exact round trip (sigma = 0: x_t = bf16(1 * x0 + 0 * noise) = x0 = latents)
    m0, s1 = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    xt, _ = ops.noise_pack(lat, noise, m0, s1, zero)
    back = ops.ltx_unpack_denorm(xt.float(), m0, s1, F_, H_, W_)
    assert back.shape == lat.shape and back.dtype == bf16
    assert torch.equal(back.view(torch.int16), lat.view(torch.int16))

    # real statistics: two bf16 roundings lie between input and output.  bf16 carries 8 significant bits (7 stored): the spacing at 2^e <= |v| < 2^(e+1)
    # is 2^(e-7), so round-to-nearest moves v by at most half of it, 2^(e-8) <= 2^-8 |v|.  x0 = bf16((lat - mean) / std) is off by at most 2^-8 |x0|,
    # i.e. 2^-8 |lat - mean| after the multiplication by std, and out = bf16(x0 std + mean) XX
    # binade from above).  The fp32 operations in between (relative 2^-24 each) and the second-order term are covered by the factor 1.01.
    mean = torch.randn(C, generator=g, device=dev) * 0.1
    std = 1.0 + 0.2 * torch.rand(C, generator=g, device=dev)
    xt, _ = ops.noise_pack(lat, noise, mean, std, zero)
    back = ops.ltx_unpack_denorm(xt.float(), mean, std, F_, H_, W_)
    l64, m64 = lat.double(), mean.double().view(1, C, 1, 1, 1)
    bound = 1.01 * 2.0**-8 * ((l64 - m64).abs() + back.double().abs())
    err = (back.double() - l64).abs()
    print(f"[unpack_denorm B={B} C={C} S={S}] max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= bound).all()

    # layout: tensors whose values spell their own index (each component < 256: exact in bf16)
    b_i, s_i, c_i = torch.meshgrid(torch.arange(B, device=dev), torch.arange(S, device=dev), torch.arange(C, device=dev), indexing="ij")
    for name, comp in (("b", b_i), ("c", c_i), ("s % 256", s_i % 256), ("s // 256", s_i // 256)):
        out = ops.ltx_unpack_denorm(comp.float().contiguous(), m0, s1, F_, H_, W_).view(B, C, S)
        assert torch.equal(out.float(), comp.float().transpose(1, 2)), f"component {name} lands in the wrong place"
    # ... and the affine part picks the channel's statistics
    cm, cs = torch.arange(C, device=dev).float(), (torch.arange(C, device=dev) % 7 + 1).float()
    out = ops.ltx_unpack_denorm(torch.ones((B, S, C), device=dev), cm, cs, F_, H_, W_).view(B, C, S)
    assert torch.equal(out.float(), (cs + cm).to(bf16).float().view(1, C, 1).expand(B, C, S))


# ---------------------------------------------------------------------------------------------------------------- c / e. the loop is the composition
F2, H2, W2, T2 = 7, 16, 24, 128  # BASELINE config 2's clip: 2 688 tokens, 128 text tokens


def _random_model(num_layers, rank, seed=3):
    from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoModelSpecification

    dev = _dev()
    spec = MI355XLTXVideoModelSpecification(transformer_config=LTXTransformerConfig(num_layers=num_layers))
    model = spec.load_diffusion_models(device=dev, random_init_seed=0)["transformer"]
    if rank:
        model.add_adapter(r=rank, lora_alpha=float(rank))
        g = torch.Generator(device=dev).manual_seed(seed)
        with torch.no_grad():  # trained-looking adapters: A and B both non-zero
            model.lora_flat.copy_(torch.randn(model.lora_flat.shape, generator=g, device=dev) * 0.01)
    return spec, model


@pytest.fixture(scope="module")
def two_blocks():
    return _random_model(2, 64)


def _prompts(B, T, D_cap, lens_c, lens_u, seed):
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(seed)
    text_c = torch.randn((B, T, D_cap), generator=g, device=dev).to(bf16)
    text_u = torch.randn((B, T, D_cap), generator=g, device=dev).to(bf16)
    mask_c = torch.zeros((B, T), dtype=bf16, device=dev)
    mask_u = torch.zeros((B, T), dtype=bf16, device=dev)
    for b in range(B):
        mask_c[b, :lens_c[b]] = 1
        mask_u[b, :lens_u[b]] = 1
    return text_c, text_u, mask_c, mask_u


def _bias(mask):
    return ((1 - mask) * -10000.0).float().contiguous()


def _composition(model, text_c, text_u, kb_c, kb_u, x0, sigmas, timesteps, guidance, F_, H_, W_):
    """The loop in Python over the training forward, ftmi_ltx_ff_forward (checkpoint = 0, the model's batch in one call) + ftmi_ltx_cfg_euler_step."""
    from finetrainers_amd import _lib, ops
    from finetrainers_amd._lib import check, ptr, stream_ptr

    lib = _lib.load()
    dev = x0.device
    B, S, C = x0.shape
    two = guidance != 1.0
    nb = 2 * B if two else B
    text = torch.cat([text_u, text_c]).contiguous() if two else text_c
    kb = torch.cat([kb_u, kb_c]).contiguous() if two else kb_c
    cos, sin = model.rope_tables(F_, H_, W_, ROPE_SCALE)
    model.refresh_lora_copies()
    cfg = model._c_config(nb, S, text.shape[1], checkpoint=False)
    weights = model._c_weights(cos, sin)
    ws_bytes = lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(cfg), ctypes.byref(weights))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    x = x0.clone()
    xin = torch.cat([x.to(bf16)] * (2 if two else 1)).contiguous()
    pred = torch.empty((nb, S, C), dtype=bf16, device=dev)
    for i in range(timesteps.numel()):
        tv = timesteps[i].expand(nb).contiguous()
        check(lib.ftmi_ltx_ff_forward(ctypes.byref(cfg), ctypes.byref(weights), ptr(xin), ptr(text), ptr(kb), ptr(tv), ptr(pred), ptr(ws), ws_bytes,
                                      stream_ptr()), "ftmi_ltx_ff_forward")
        xin = ops.ltx_cfg_euler_step(pred, x, sigmas[i].expand(B).contiguous(), sigmas[i + 1].expand(B).contiguous(), guidance)
    torch.cuda.synchronize()
    return x


def _one_call(model, text_c, text_u, kb_c, kb_u, x0, sigmas, timesteps, guidance, F_, H_, W_):
    from finetrainers_amd import ops

    B, S, _ = x0.shape
    cos, sin = model.rope_tables(F_, H_, W_, ROPE_SCALE)
    model.refresh_lora_copies()
    cfg = model._c_config(B, S, text_c.shape[1])
    x = x0.clone()
    ops.ltx_sample(cfg, model._c_weights(cos, sin), text_c, text_u, kb_c, kb_u, x, sigmas, timesteps, guidance)
    torch.cuda.synchronize()
    return x


def _attention_flops(reset=True):
    """FLOPs and launches of every attention-forward launch since the last reset (ftmi_prof_summary, class 2)."""
    from finetrainers_amd import _lib

    launches, flops = ctypes.c_long(0), ctypes.c_double(0)
    _lib.check(_lib.load().ftmi_prof_summary(2, None, None, None, ctypes.byref(launches), ctypes.byref(flops), int(reset)), "ftmi_prof_summary")
    return launches.value, flops.value


def _loop_inputs(B, seed=11):
    dev = _dev()
    text_c, text_u, mask_c, mask_u = _prompts(B, T2, 4096, [96, 57][:B], [32, 8][:B], seed)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    x0 = torch.randn((B, F2 * H2 * W2, 128), generator=g, device=dev)
    sigmas = torch.tensor([1.0, 0.71, 0.33, 0.0], device=dev)
    timesteps = (sigmas[:-1] * 1000.0).contiguous()
    return text_c, text_u, _bias(mask_c), _bias(mask_u), x0, sigmas, timesteps


def test_sample_is_the_composition_bit_for_bit(two_blocks):
    """2 blocks, config-2 width, S = 2 688, T = 128, rank 64 with non-zero B, 3 steps, g = 3: ftmi_ltx_ff_sample (forward-only workspace, text-side work
    hoisted out of the step loop) against the Python loop over ftmi_ltx_ff_forward + ftmi_ltx_cfg_euler_step -- every bit of the final state."""
    _, model = two_blocks
    args = _loop_inputs(1)
    want = _composition(model, *args, 3.0, F2, H2, W2)
    got = _one_call(model, *args, 3.0, F2, H2, W2)
    assert torch.isfinite(got).all() and not torch.equal(got, args[4])
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"rel_l2 {rel_l2(got, want):.3e}"
    # two videos in one call: model batch 4
    args = _loop_inputs(2, seed=21)
    want = _composition(model, *args, 3.0, F2, H2, W2)
    got = _one_call(model, *args, 3.0, F2, H2, W2)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"rel_l2 {rel_l2(got, want):.3e}"
    # the unhoisted A/B partner of the timing in DESIGN.md computes the same bits
    import os

    from finetrainers_amd import _lib

    os.environ["FTMI_SAMPLE_HOIST"] = "0"
    try:
        _lib.load().ftmi_reload_switches()
        again = _one_call(model, *args, 3.0, F2, H2, W2)
    finally:
        del os.environ["FTMI_SAMPLE_HOIST"]
        _lib.load().ftmi_reload_switches()
    assert torch.equal(again.view(torch.int32), want.view(torch.int32))


def test_guidance_one_runs_the_conditional_rows_only(two_blocks):
    from finetrainers_amd import _lib, ops

    _, model = two_blocks
    lib = _lib.load()
    text_c, text_u, kb_c, kb_u, x0, sigmas, timesteps = _loop_inputs(1, seed=31)
    S = x0.shape[1]
    cfg = model._c_config(1, S, T2)
    none = _lib.LtxFfWeights()  # (this model has no feed-forward adapters; a planner never dereferences the weights)
    one, two = ops.ltx_sample_workspace_bytes(cfg, False), ops.ltx_sample_workspace_bytes(cfg, True)
    ref1 = lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(model._c_config(1, S, T2, checkpoint=True)), ctypes.byref(none))
    ref2 = lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(model._c_config(2, S, T2, checkpoint=True)), ctypes.byref(none))
    assert ref1 <= one <= 1.05 * ref1 and ref2 <= two <= 1.05 * ref2 and one < 0.6 * two

    want = _composition(model, text_c, None, kb_c, None, x0, sigmas, timesteps, 1.0, F2, H2, W2)
    lib.ftmi_prof_enable(1 << 20)  # count every launch, bracket (almost) none with events
    try:
        _attention_flops()
        got = _one_call(model, text_c, None, kb_c, None, x0, sigmas, timesteps, 1.0, F2, H2, W2)
        n1, f1 = _attention_flops()
        _one_call(model, text_c, text_u, kb_c, kb_u, x0, sigmas, timesteps, 3.0, F2, H2, W2)
        n2, f2 = _attention_flops()
    finally:
        lib.ftmi_prof_enable(0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"rel_l2 {rel_l2(got, want):.3e}"
    # same launches (2 attentions x 2 blocks x 3 steps), half the rows
    print(f"[guidance 1] attention launches {n1} vs {n2}, FLOPs {f1:.4e} vs {f2:.4e}")
    assert n1 == n2 == 2 * 2 * 3
    assert f1 > 0 and f2 == 2 * f1


# ---------------------------------------------------------------------------------------------------------------- d. oracle parity over a trajectory
def test_sample_trajectory_vs_oracle():
    """4 steps, g = 3, 2 blocks, 240 video tokens: the oracle (bf16, CPU) driven by the torch loop of tests/test_ltx_sampling_host.py against
    ftmi_ltx_ff_sample on the same prompt embeddings, noise and sigmas.  bf16 errors compound over steps, so the yardstick is measured here: the oracle
    against itself under accumulation_order_variant, and kernel-vs-oracle may be at most 2 x that (the headroom of the full-depth
    parity test: 2.0e-3 claimed over 1.17e-3 self-distance).

    The yardstick on the host CPU for these inputs: 2.94e-3 (BASELINE.md, row "latent sampling trajectory"; the kernel's distance is printed here)."""
    from test_ltx_sampling_host import torch_sampling_loop

    from finetrainers_amd import ops
    from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoModelSpecification
    from oracle import ltx

    dev = _dev()
    F_, H_, W_, B, guidance = 3, 8, 10, 1, 3.0
    S = F_ * H_ * W_
    cfg = ltx.LTXConfig.production(num_layers=2)
    omodel = ltx.build_model(cfg, seed=0, rank=64, alpha=64.0, lora_b_std=0.02)
    g = torch.Generator().manual_seed(5)
    text_c = torch.randn((B, cfg.text_seq_len, cfg.caption_channels), generator=g).to(bf16)
    text_u = torch.randn((B, cfg.text_seq_len, cfg.caption_channels), generator=g).to(bf16)
    mask_c = torch.zeros((B, cfg.text_seq_len), dtype=bf16)
    mask_u = torch.zeros((B, cfg.text_seq_len), dtype=bf16)
    mask_c[:, :96] = 1
    mask_u[:, :32] = 1
    x0 = torch.randn((B, S, cfg.in_channels), generator=g)
    sigmas = torch.tensor([1.0, 0.75, 0.5, 0.25, 0.0])
    timesteps = sigmas[:-1] * 1000.0

    text = torch.cat([text_u, text_c])
    mask = torch.cat([mask_u, mask_c])

    def oracle_model(xin, i):
        with torch.no_grad():
            return omodel(hidden_states=xin, encoder_hidden_states=text, timestep=timesteps[i].expand(xin.shape[0]), encoder_attention_mask=mask,
                          num_frames=F_, height=H_, width=W_, rope_interpolation_scale=ROPE_SCALE, return_dict=False)[0]

    t0 = time.time()
    ref = torch_sampling_loop(oracle_model, x0, sigmas, guidance)
    with ltx.accumulation_order_variant(512):
        ref_ord = torch_sampling_loop(oracle_model, x0, sigmas, guidance)
    t_oracle = time.time() - t0
    yardstick = rel_l2(ref_ord, ref)
    assert yardstick > 0 and yardstick == yardstick and yardstick != float("inf"), f"unusable yardstick {yardstick}"

    spec = MI355XLTXVideoModelSpecification(transformer_config=LTXTransformerConfig(num_layers=2))
    gmodel = spec.load_diffusion_models(state_dict=omodel.state_dict(), device=dev)["transformer"]
    gmodel.add_adapter(r=64, lora_alpha=64.0)
    gmodel.load_lora_state_dict({k: v for k, v in omodel.state_dict().items() if "lora_" in k})
    cos, sin = gmodel.rope_tables(F_, H_, W_, ROPE_SCALE)
    gmodel.refresh_lora_copies()
    x = x0.to(dev).clone()
    ops.ltx_sample(gmodel._c_config(B, S, cfg.text_seq_len), gmodel._c_weights(cos, sin), text_c.to(dev), text_u.to(dev), _bias(mask_c.to(dev)),
                   _bias(mask_u.to(dev)), x, sigmas.to(dev), timesteps.to(dev), guidance)
    torch.cuda.synchronize()
    dist = rel_l2(x, ref)
    print(f"[sampling trajectory] kernel-vs-oracle rel_l2 {dist:.3e}; oracle-vs-reordered-oracle {yardstick:.3e}; ratio {dist / yardstick:.2f} "
          f"(oracle time {t_oracle:.0f} s)")
    assert torch.isfinite(x).all()
    assert rel_l2(ref, x0) > 0.1  # the trajectory moved
    assert dist <= 2 * yardstick, f"kernel-vs-oracle {dist:.3e} > 2 x {yardstick:.3e}"


# ---------------------------------------------------------------------------------------------------------------- f. adapters are live
def test_sampler_sees_the_live_adapters(two_blocks):
    from finetrainers_amd.ltx_video import MI355XLTXLatentSampler

    dev = _dev()
    spec, model = two_blocks
    _, base = _random_model(2, 0)  # the same frozen weights without an adapter: r == 0
    F_, H_, W_ = 2, 8, 10
    text_c, text_u, mask_c, mask_u = _prompts(1, T2, 4096, [96], [32], seed=41)
    kw = dict(prompt_embeds=text_c, prompt_attention_mask=mask_c, negative_prompt_embeds=text_u, negative_prompt_attention_mask=mask_u, num_frames=F_,
              height=H_, width=W_, num_inference_steps=3, guidance_scale=3.0)
    gen = lambda: torch.Generator(device=dev).manual_seed(7)
    saved = model.lora_flat.clone()
    try:
        first = MI355XLTXLatentSampler(model).sample(generator=gen(), **kw)
        assert first.shape == (1, 128, F_, H_, W_) and first.dtype == bf16 and torch.isfinite(first.float()).all()
        again = spec.validation_latents(transformer=model, generator=gen(), **kw)  # the specification's entry point delegates
        assert torch.equal(first.view(torch.int16), again.view(torch.int16)), "one seed, two results"
        plain = MI355XLTXLatentSampler(base).sample(generator=gen(), **kw)
        assert torch.isfinite(plain.float()).all() and not torch.equal(plain, first), "the adapters do not reach the sample"
        with torch.no_grad():
            model.lora_B.mul_(1.5)  # an optimiser step's in-place update
        moved = MI355XLTXLatentSampler(model).sample(generator=gen(), **kw)
        assert not torch.equal(moved, first), "the working copies were not refreshed"
        with torch.no_grad():
            model.lora_B.zero_()  # B = 0: the base model again, bit for bit
        zero_b = MI355XLTXLatentSampler(model).sample(generator=gen(), **kw)
        assert torch.equal(zero_b.view(torch.int16), plain.view(torch.int16))
        # another seed is another sample; caller-supplied noise takes the generator's place
        assert not torch.equal(MI355XLTXLatentSampler(base).sample(generator=torch.Generator(device=dev).manual_seed(8), **kw), plain)
        noise = torch.randn((1, 128, F_, H_, W_), generator=gen(), device=dev, dtype=torch.float32)
        assert torch.equal(MI355XLTXLatentSampler(base).sample(latents=noise, **kw), plain)
    finally:
        with torch.no_grad():
            model.lora_flat.copy_(saved)


# ---------------------------------------------------------------------------------------------------------------- g. full size
def test_full_size_sampling_runs_in_forward_only_memory():
    """BASELINE config 2 at 28 blocks, one video (cond + uncond = the step's 2 x 2 688 tokens), 4 steps: finite latents, and the peak memory of the
    sampling call stays below that of the training step (checkpoint = 0) on the same model."""
    from finetrainers_amd.ltx_video import MI355XLTXLatentSampler
    from finetrainers_amd.trainer import sft_loss

    dev = _dev()
    spec, model = _random_model(28, 64)
    text_c, text_u, mask_c, mask_u = _prompts(1, T2, 4096, [96], [32], seed=51)

    def peak(fn):
        model._ws_pool.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    def sample():
        return MI355XLTXLatentSampler(model).sample(text_c, mask_c, text_u, mask_u, F2, H2, W2, num_inference_steps=4, guidance_scale=3.0,
                                                    generator=torch.Generator(device=dev).manual_seed(1))

    def train_step():
        g = torch.Generator(device=dev).manual_seed(2)
        lat = torch.randn((2, 128, F2, H2, W2), generator=g, device=dev).to(bf16)
        pred, target, sig = spec.forward(
            transformer=model,
            condition_model_conditions={"encoder_hidden_states": torch.cat([text_u, text_c]), "encoder_attention_mask": torch.cat([mask_u, mask_c])},
            latent_model_conditions={"latents": lat, "latents_mean": torch.zeros(128, device=dev), "latents_std": torch.ones(128, device=dev)},
            sigmas=torch.tensor([0.25, 0.7], device=dev), force_first_frame_branch=False)
        sft_loss(pred, target, sig).backward()
        return pred

    assert not model.gradient_checkpointing
    mem_sample, latents = peak(sample)
    assert latents.shape == (1, 128, F2, H2, W2) and torch.isfinite(latents.float()).all() and latents.float().std() > 1e-3
    mem_train, _ = peak(train_step)
    print(f"[full size] peak memory above the model: sampling {mem_sample / 2**30:.2f} GiB, training step (checkpoint = 0) {mem_train / 2**30:.2f} GiB")
    assert mem_sample < mem_train
