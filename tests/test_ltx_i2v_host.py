"""CPU-side tests of LTX-Video image-conditioned latent sampling: the C ABI carries the per-frame forward and the conditioned sampler, the conditioned
loop the GPU tests compose equals the unconditioned one for k = 0 and the image-to-video pipeline's update written out in fp64, the initial state keeps
the pipeline's noise outside the held frames, and wrong arguments are refused before anything is launched."""

import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

I2V_SYMBOLS = ("ftmi_ltx_ff_forward_frames", "ftmi_ltx_ff_forward_frames_workspace_bytes", "ftmi_ltx_ff_sample_cond", "ftmi_ltx_ff_sample_cond_workspace_bytes",
               "ftmi_ltx_cfg_euler_step_held")


@pytest.fixture(scope="module")
def lib():
    from finetrainers_amd import _lib

    if not _lib.lib_available():
        from finetrainers_amd.csrc.build import build

        build()
    return _lib.load()


def torch_cond_sampling_loop(model, x0, sigmas, guidance, hold_tokens):
    """The conditioned denoising loop, restated in torch ([upstream, unpinned] LTXImageToVideoPipeline.__call__): ``x0`` fp32 [B, S, C] with the first
    ``hold_tokens`` tokens of every sample the clean conditioning latents.  ``model(x_in bf16 [nb, S, C], step) -> pred bf16 [nb, S, C]`` sees the bf16
    rounding of the whole state (the caller's model feeds timestep 0 to the held tokens); the state stays fp32; v = u + g (c - u) and
    x += (sigma_next - sigma) v on the tokens past the held ones only -- the held ones are never written."""
    x = x0.float().clone()
    B = x.shape[0]
    for i in range(len(sigmas) - 1):
        xin = x.to(torch.bfloat16)
        if guidance != 1.0:
            pred = model(torch.cat([xin, xin]), i).float()
            u, c = pred[:B], pred[B:]
            v = u + guidance * (c - u)
        else:
            v = model(xin, i).float()
        x[:, hold_tokens:] = x[:, hold_tokens:] + (sigmas[i + 1] - sigmas[i]) * v[:, hold_tokens:]
    return x


def test_i2v_symbols_declared_and_exported(lib):
    from finetrainers_amd import _lib

    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", header))
    for name in I2V_SYMBOLS:
        assert name in declared, f"include/ftmi355.h does not declare {name}"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"libftmi355.so does not export {name}"


def _toy_model(B, S, C, n, guidance, seed=0):
    """A model whose prediction depends on the step only (pre-drawn bf16 tensors), so that two loops in different precisions see the same predictions."""
    g = torch.Generator().manual_seed(seed)
    nb = 2 * B if guidance != 1.0 else B
    preds = [torch.randn((nb, S, C), generator=g).to(torch.bfloat16) for _ in range(n)]
    seen = []

    def model(xin, i):
        assert xin.dtype == torch.bfloat16 and tuple(xin.shape) == (nb, S, C)
        seen.append(xin.clone())
        return preds[i]

    return model, preds, seen


@pytest.mark.parametrize("guidance", [1.0, 3.0])
def test_cond_loop_with_nothing_held_is_the_plain_loop(guidance):
    from test_ltx_sampling_host import torch_sampling_loop

    B, F_, HW, C, n = 2, 3, 10, 16, 5
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn((B, F_ * HW, C), generator=g)
    sigmas = torch.tensor([1.0, 0.8, 0.55, 0.3, 0.1, 0.0])

    def model(xin, i):  # depends on the state: the two loops must feed it the same bits at every step
        scale = torch.linspace(0.4, 0.7, xin.shape[0]).view(-1, 1, 1)  # (the unconditional and the conditional rows differ)
        return (scale * xin.float() + 0.1 * (i + 1)).to(torch.bfloat16)

    want = torch_sampling_loop(model, x0, sigmas, guidance)
    got = torch_cond_sampling_loop(model, x0, sigmas, guidance, 0)
    assert torch.equal(got, want)


@pytest.mark.parametrize("guidance", [1.0, 3.0])
@pytest.mark.parametrize("k", [1, 2])
def test_cond_loop_is_the_pipeline_update_in_fp64(guidance, k):
    """[upstream, unpinned] LTXImageToVideoPipeline.__call__, per step, on unpacked [B, C, F, H, W] tensors:
         noise_pred = uncond + g (text - uncond);  noise_pred = noise_pred[:, :, 1:];  noise_latents = latents[:, :, 1:]
         pred_latents = scheduler.step(noise_pred, t, noise_latents)      (sample + (sigma_next - sigma) * model_output)
         latents = cat([latents[:, :, :1], pred_latents], dim=2)
    written out in fp64 (with k frames held instead of 1), against the fp32 restatement.  Bound: the restatement makes four fp32 roundings per element and
    step (c - u, u + g d, sigma_next - sigma, x + dt v; each relative 2^-24, as derived for the step kernel in tests/test_gpu_ltx_sampling.py), n steps."""
    B, F_, H_, W_, C, n = 2, 4, 2, 5, 16, 5
    S, hold = F_ * H_ * W_, k * H_ * W_
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn((B, S, C), generator=g) * 2
    sigmas = torch.tensor([1.0, 0.8, 0.55, 0.3, 0.1, 0.0])
    model, preds, seen = _toy_model(B, S, C, n, guidance, seed=3)
    got = torch_cond_sampling_loop(model, x0, sigmas, guidance, hold)

    unpack = lambda t: t.double().view(-1, F_, H_, W_, C).permute(0, 4, 1, 2, 3)  # [., S, C] -> [., C, F, H, W]
    latents = unpack(x0)
    bound = torch.zeros_like(latents)
    for i in range(n):
        p = unpack(preds[i])
        if guidance != 1.0:
            u, c = p[:B], p[B:]
            noise_pred = u + guidance * (c - u)
            mag = u.abs() + guidance * (c.abs() + u.abs())
        else:
            noise_pred, mag = p, p.abs()
        noise_pred = noise_pred[:, :, k:]
        noise_latents = latents[:, :, k:]
        dt = sigmas[i + 1].double() - sigmas[i].double()
        bound[:, :, k:] += 4 * 2.0**-24 * (noise_latents.abs() + dt.abs() * mag[:, :, k:])
        pred_latents = noise_latents + dt * noise_pred
        latents = torch.cat([latents[:, :, :k], pred_latents], dim=2)
    want = latents.permute(0, 2, 3, 4, 1).reshape(B, S, C)
    bound = bound.permute(0, 2, 3, 4, 1).reshape(B, S, C)
    err = (got.double() - want).abs()
    assert (err <= bound).all(), f"max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}"
    assert err[:, hold:].max() > 0 or n == 0  # fp32 against fp64: the comparison is not vacuous
    # the held frames are the input, bit for bit; the model saw their bf16 rounding at every step
    assert torch.equal(got[:, :hold], x0[:, :hold])
    assert not torch.equal(got[:, hold:], x0[:, hold:])
    for xin in seen:
        for h in range(xin.shape[0] // B):
            assert torch.equal(xin[h * B:(h + 1) * B, :hold], x0[:, :hold].to(torch.bfloat16))


def test_initial_state_keeps_the_noise_outside_the_held_frames():
    from finetrainers_amd.ltx_video import MI355XLTXLatentSampler

    B, C, F_, H_, W_ = 2, 16, 4, 3, 5
    cpu = torch.device("cpu")
    gen = lambda: torch.Generator().manual_seed(11)
    plain = MI355XLTXLatentSampler.initial_state(B, C, F_, H_, W_, cpu, generator=gen())
    assert plain.shape == (B, F_ * H_ * W_, C) and plain.dtype == torch.float32
    want_noise = torch.randn((B, C, F_, H_, W_), generator=gen(), dtype=torch.float32)  # the pipeline's draw: the whole shape, one call
    assert torch.equal(plain, want_noise.flatten(2).transpose(1, 2))
    for k in (1, 2, F_):
        img = torch.randn((B, C, k, H_, W_), generator=torch.Generator().manual_seed(12 + k))
        cond = MI355XLTXLatentSampler.initial_state(B, C, F_, H_, W_, cpu, generator=gen(), image_latents=img)
        hold = k * H_ * W_
        assert torch.equal(cond[:, hold:], plain[:, hold:]), "the noise outside the held frames depends on the conditioning"
        assert torch.equal(cond[:, :hold], img.flatten(2).transpose(1, 2)), "the held frames are not the image latents"
        # upstream for k = 1: the encoded frame repeated over all frames, blended with the noise by the conditioning mask
        if k == 1:
            mask = torch.zeros((B, 1, F_, H_, W_))
            mask[:, :, :1] = 1.0
            blended = img.repeat(1, 1, F_, 1, 1) * mask + want_noise * (1 - mask)
            assert torch.equal(cond, blended.flatten(2).transpose(1, 2))
    # caller-supplied initial state: the image latents still land in the held frames, the caller's tensor is not written
    lat = torch.randn((B, C, F_, H_, W_), generator=gen())
    keep = lat.clone()
    img = torch.ones((B, C, 1, H_, W_))
    cond = MI355XLTXLatentSampler.initial_state(B, C, F_, H_, W_, cpu, latents=lat, image_latents=img)
    assert torch.equal(lat, keep) and (cond[:, :H_ * W_] == 1).all() and torch.equal(cond[:, H_ * W_:], keep.flatten(2).transpose(1, 2)[:, H_ * W_:])


def _cpu_model(layers=1, rank=64):
    from finetrainers_amd.ltx_video.transformer import LTXTransformerConfig, MI355XLTXVideoTransformer3DModel

    model = MI355XLTXVideoTransformer3DModel(LTXTransformerConfig(num_layers=layers), device=torch.device("cpu"))
    if rank:
        model.add_adapter(r=rank, lora_alpha=float(rank))
    return model


def test_sampler_refuses_wrong_conditioning_arguments():
    from finetrainers_amd.ltx_video import MI355XLTXLatentSampler

    model = _cpu_model()
    C = model.config.in_channels
    sampler = MI355XLTXLatentSampler(model)
    B, T, F_, H_, W_ = 1, 8, 3, 2, 4
    kw = dict(prompt_embeds=torch.zeros(B, T, model.config.caption_channels), prompt_attention_mask=None, negative_prompt_embeds=None,
              negative_prompt_attention_mask=None, num_frames=F_, height=H_, width=W_, num_inference_steps=2, guidance_scale=1.0)
    with pytest.raises(ValueError, match="frames"):  # k > F
        sampler.sample(image_latents=torch.zeros(B, C, F_ + 1, H_, W_), **kw)
    with pytest.raises(ValueError, match="cond_frames"):
        sampler.sample(cond_frames=F_ + 1, **kw)
    with pytest.raises(ValueError, match="cond_frames"):
        sampler.sample(cond_frames=-1, **kw)
    with pytest.raises(ValueError, match="cond_frames"):  # disagrees with the image latents
        sampler.sample(image_latents=torch.zeros(B, C, 1, H_, W_), cond_frames=2, **kw)
    for bad in ((B, C, 1, H_ + 1, W_), (B, C + 1, 1, H_, W_), (B + 1, C, 1, H_, W_), (B, C, H_, W_)):
        with pytest.raises(ValueError, match="image_latents"):
            sampler.sample(image_latents=torch.zeros(*bad), **kw)


def test_frame_timestep_is_forward_only():
    model = _cpu_model()
    c = model.config
    B, F_, H_, W_, T = 1, 2, 2, 2, 8
    S = F_ * H_ * W_
    kw = dict(hidden_states=torch.zeros(B, S, c.in_channels), encoder_hidden_states=torch.zeros(B, T, c.caption_channels), timestep=torch.zeros(B),
              encoder_attention_mask=None, num_frames=F_, height=H_, width=W_)
    assert model.lora_A.requires_grad
    with pytest.raises(NotImplementedError, match="no backward"):  # grad enabled, adapter trainable
        model(frame_timestep=torch.zeros(B, F_), **kw)
    with pytest.raises(ValueError, match="frame_timestep"):  # one value per latent frame
        model(frame_timestep=torch.zeros(B, F_ + 1), **kw)
    with pytest.raises(ValueError, match="frame_timestep"):
        model(frame_timestep=torch.zeros(B * S), **kw)
    # with grad disabled, or no adapter that requires grad, the limit does not apply: the call gets as far as the device check
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="GPU only"):
            model(frame_timestep=torch.zeros(B, F_), **kw)
    model.lora_A.requires_grad_(False)
    model.lora_B.requires_grad_(False)
    with pytest.raises(RuntimeError, match="GPU only"):
        model(frame_timestep=torch.zeros(B, F_), **kw)
    with pytest.raises(RuntimeError, match="GPU only"):
        _cpu_model(rank=0)(frame_timestep=torch.zeros(B, F_), **kw)


def _cfg(B=1, S=64, L=1, C=128, **kw):
    from finetrainers_amd import _lib

    return _lib.LtxConfig(B=B, S=S, T=128, D=2048, H=32, L=L, C_in=C, C_out=C, D_ff=8192, D_cap=4096, r=0, lora_scale=0.0, eps_norm=1e-6, eps_qk=1e-5,
                          gemm_variant=8, **kw)


def test_i2v_entry_points_check_arguments(lib):
    from finetrainers_amd import _lib

    p = ctypes.c_void_p(256)
    w = _lib.LtxFfWeights()
    big = 1 << 40
    # held step: null, hold outside the sample, hold off a 16-byte vector
    assert lib.ftmi_ltx_cfg_euler_step_held(None, None, None, None, 3.0, None, 1, 64, 8, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_ltx_cfg_euler_step_held(p, p, p, p, 3.0, p, 1, 64, 72, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_ltx_cfg_euler_step_held(p, p, p, p, 3.0, p, 1, 64, -8, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_ltx_cfg_euler_step_held(p, p, p, p, 3.0, p, 1, 64, 12, None) == _lib.FTMI_ERR_UNSUPPORTED and "multiple of 8" in _lib.last_error()
    # per-frame forward: frames must divide the tokens; B x frames is bounded; no narrow geometry; workspace checked
    cfg = _cfg(S=64)
    fwd = lambda c, frames, ws_bytes=big: lib.ftmi_ltx_ff_forward_frames(ctypes.byref(c), ctypes.byref(w), p, p, None, p, frames, p, p, ws_bytes, None)
    assert fwd(cfg, 0) == _lib.FTMI_ERR_INVALID
    assert fwd(cfg, 3) == _lib.FTMI_ERR_UNSUPPORTED and "frames" in _lib.last_error()
    assert fwd(cfg, 4, 1024) == _lib.FTMI_ERR_INVALID and "workspace too small" in _lib.last_error()
    assert fwd(_cfg(B=9, S=160), 16) == _lib.FTMI_ERR_UNSUPPORTED  # 144 groups
    assert fwd(_cfg(B=8, S=160), 16, 1024) == _lib.FTMI_ERR_INVALID  # 128 groups pass the bound (and 8 model rows x 16 frames is the stated cap)
    assert fwd(_cfg(B=16, S=64), 4, 1024) == _lib.FTMI_ERR_INVALID  # the batch itself is not limited to 8 here
    assert fwd(_cfg(S=64, d_valid=32, head_dim_valid=8), 4) == _lib.FTMI_ERR_UNSUPPORTED and "narrow" in _lib.last_error()
    assert lib.ftmi_ltx_ff_forward_frames(ctypes.byref(cfg), ctypes.byref(w), p, p, None, None, 4, p, p, big, None) == _lib.FTMI_ERR_INVALID
    # conditioned sampler
    smp = lambda c, frames, k, g=3.0, ws_bytes=big, tu=p: lib.ftmi_ltx_ff_sample_cond(ctypes.byref(c), ctypes.byref(w), p, tu, None, None, p, p, p, 2, g, frames, k, p,
                                                                                  ws_bytes, None)
    assert smp(cfg, 0, 0) == _lib.FTMI_ERR_INVALID
    assert smp(cfg, 4, 5) == _lib.FTMI_ERR_INVALID and "cond_frames" in _lib.last_error()  # k > F
    assert smp(cfg, 4, -1) == _lib.FTMI_ERR_INVALID
    assert smp(cfg, 3, 1) == _lib.FTMI_ERR_UNSUPPORTED
    assert smp(cfg, 4, 1, tu=None) == _lib.FTMI_ERR_INVALID  # guidance without the unconditional prompt
    assert smp(cfg, 4, 1, ws_bytes=1024) == _lib.FTMI_ERR_INVALID and "workspace too small" in _lib.last_error()
    assert smp(_cfg(B=5), 4, 1) == _lib.FTMI_ERR_UNSUPPORTED  # 10 model rows
    assert smp(_cfg(B=4, S=160), 16, 1, ws_bytes=1024) == _lib.FTMI_ERR_INVALID  # 4 model rows x 2 x 16 frames = 128 groups: inside the bound


def test_conditioned_workspace_is_the_sampler_workspace_plus_taller_tables(lib):
    """Config-2 size: per-frame conditioning adds (G - nb) rows to the tables and the embedding scratch, G = nb x frames, plus the two hoisted embedding
    rows -- nothing that grows with the token count."""
    from finetrainers_amd import _lib

    L, D, F_ = 28, 2048, 7
    w = ctypes.byref(_lib.LtxFfWeights())  # (no feed-forward adapters; a planner never dereferences the weights)
    for videos, two_pass in ((1, 1), (2, 1), (1, 0)):
        cfg = _cfg(B=videos, S=2688, L=L)
        nb = videos * (2 if two_pass else 1)
        plain = lib.ftmi_ltx_ff_sample_workspace_bytes(ctypes.byref(cfg), w, two_pass)
        cond = lib.ftmi_ltx_ff_sample_cond_workspace_bytes(ctypes.byref(cfg), w, two_pass, F_)
        rows = nb * F_ - nb
        tables = rows * 2 * (256 + D + D + 6 * D + L * 8 * D + 3 * D) + rows * 4 + 2 * 7 * D * 2
        assert plain < cond <= plain + tables + 10 * 256, (plain, cond, tables)  # (every buffer is rounded up to 256 bytes)
        assert cond - plain < 0.01 * plain
        # one frame: one group per model row, the plain layout plus the two hoisted rows
        one = lib.ftmi_ltx_ff_sample_cond_workspace_bytes(ctypes.byref(cfg), w, two_pass, 1)
        assert plain < one <= plain + 2 * 7 * D * 2 + 2 * 256
        fwd = lib.ftmi_ltx_ff_forward_frames_workspace_bytes(ctypes.byref(_cfg(B=nb, S=2688, L=L)), w, F_)
        ref = lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(_cfg(B=nb, S=2688, L=L, checkpoint=1)), w)
        assert ref < fwd <= ref + tables + 10 * 256
