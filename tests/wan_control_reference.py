"""Test reference for the Wan control recipe (``--training_type control-lora``): oracle.wan's model with what the reference's control trainer and
control specification add (finetrainers/models/wan/control_specification.py, trainer/control_trainer/trainer.py:130-144), restated in eager torch:

* the patch embedding widened to 2C input channels with zero weights for the new ones (models/utils.py: _expand_conv3d_with_zeroed_weights);
* peft's ``lora.Conv3d`` around it ([upstream]): ``lora_A`` a Conv3d with the base's kernel and stride, ``lora_B`` a 1 x 1 x 1 Conv3d, fp32 adapters over the
  bf16 base, ``result = base(x) + lora_B(lora_A(x.float())) * scaling`` cast back to the base dtype;
* the specification's input construction (:243-308): normalised means (the posterior's mode), flow-match mix, control frames kept or multiplied by zero,
  channel concatenation -- with the kept frames given as a [B, F] mask (the frame-conditioning function itself is pinned by the golden fixtures);
* the pack kernel's two outputs, and the folded patch adapter's forward / gradients in the reference's dtypes and in fp64."""
import math

import torch
import torch.nn as nn

from oracle import wan

bf16 = torch.bfloat16


def expand_conv3d(conv: nn.Conv3d, new_in_channels: int) -> nn.Conv3d:
    new = nn.Conv3d(new_in_channels, conv.out_channels, kernel_size=conv.kernel_size, stride=conv.stride, bias=conv.bias is not None).to(conv.weight.dtype)
    with torch.no_grad():
        new.weight.zero_()
        new.weight[:, :conv.in_channels].copy_(conv.weight)
        if conv.bias is not None:
            new.bias.copy_(conv.bias)
    return new


class LoraConv3d(nn.Module):
    def __init__(self, base: nn.Conv3d, r: int, alpha: float):
        super().__init__()
        self.base_layer, self.r, self.scaling = base, r, alpha / r
        self.lora_A = nn.ModuleDict({"default": nn.Conv3d(base.in_channels, r, base.kernel_size, base.stride, bias=False)})
        self.lora_B = nn.ModuleDict({"default": nn.Conv3d(r, base.out_channels, (1, 1, 1), (1, 1, 1), bias=False)})
        nn.init.kaiming_uniform_(self.lora_A["default"].weight, a=math.sqrt(5))
        nn.init.zeros_(self.lora_B["default"].weight)

    def forward(self, x):
        result = self.base_layer(x)
        dt = result.dtype
        a, b = self.lora_A["default"], self.lora_B["default"]
        result = result + b(a(x.to(a.weight.dtype))) * self.scaling
        return result.to(dt)


def control_model_input(moments, control_moments, latents_mean, latents_std, sigmas, noise, keep):
    """-> (hidden_states [B, 2C, F, H, W], latents, timesteps).  ``sigmas`` [B] fp32, ``keep`` [B, F] (1 keeps the control frame)."""
    B, _, F_ = moments.shape[:3]
    latents = wan.normalize_latents(torch.chunk(moments, 2, dim=1)[0], latents_mean, latents_std)
    control = wan.normalize_latents(torch.chunk(control_moments, 2, dim=1)[0], latents_mean, latents_std)
    s = sigmas.view(B, 1, 1, 1, 1)
    noisy = (1.0 - s) * latents + s * noise
    mask = torch.zeros_like(control)
    n = min(control.shape[2], F_)
    mask[:, :, :n] = keep[:, :n].to(mask).view(B, 1, n, 1, 1)
    control = control * mask
    if control.shape[2] >= F_:
        control = control[:, :, :F_]
    else:
        control = torch.cat([control, control.new_zeros(B, control.shape[1], F_ - control.shape[2], *control.shape[3:])], dim=2)
    return torch.cat([noisy, control], dim=1).to(latents), latents, (sigmas.flatten() * 1000.0).long()


def spec_forward_control(transformer, moments, control_moments, latents_mean, latents_std, encoder_hidden_states, sigmas, noise, keep):
    hidden, latents, timesteps = control_model_input(moments, control_moments, latents_mean, latents_std, sigmas, noise, keep)
    pred = transformer(hidden_states=hidden, encoder_hidden_states=encoder_hidden_states, timestep=timesteps, return_dict=False)[0]
    return pred, noise - latents, sigmas


def patch_columns(hidden, patch=(1, 2, 2)):
    """[B, C, F, H, W] -> [B S, C pt ph pw]: tokens in (f, h, w) order, columns in (c, pt, ph, pw) order."""
    B, C, F_, H, W = hidden.shape
    pt, ph, pw = patch
    f, h, w = F_ // pt, H // ph, W // pw
    return hidden.view(B, C, f, pt, h, ph, w, pw).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B * f * h * w, C * pt * ph * pw)


def pack_reference(moments, control_moments, latents_mean, latents_std, sigmas, noise, keep, patch=(1, 2, 2)):
    """What ``ftmi_wan_control_pack`` writes: (cols2 [B S, 2 Kp] = [cols | cols], target)."""
    hidden, latents, _ = control_model_input(moments, control_moments, latents_mean, latents_std, sigmas, noise, keep)
    cols = patch_columns(hidden, patch)
    return torch.cat([cols, cols], dim=1), noise - latents


def _patch_adapter(cols, w, bias, a, b, s, dy, dt, rnd):
    a, b = a.to(dt).requires_grad_(True), b.to(dt).requires_grad_(True)
    base = rnd(cols.to(dt) @ w.to(dt).t() + bias.to(dt))
    y = rnd(base + ((cols.to(dt) @ a.t()) @ b.t()) * s)
    ga, gb = torch.autograd.grad(y, (a, b), dy.to(dt))
    return y.detach(), ga, gb


def patch_adapter_eager(cols, w, bias, a, b, s, dy):
    """The reference's dtypes: the bf16 base layer (its output rounded to bf16), the adapter branch in fp32, the sum rounded to bf16; gradients by autograd
    (the straight-through roundings are what eager bf16 storage gives)."""
    y, ga, gb = _patch_adapter(cols, w, bias, a, b, s, dy, torch.float32, lambda t: t + (t.to(bf16).float() - t).detach())
    return y.to(bf16), ga, gb


def patch_adapter_fp64(cols, w, bias, a, b, s, dy):
    return _patch_adapter(cols, w, bias, a, b, s, dy, torch.float64, lambda t: t)
