"""peft ``lora.Linear`` over a frozen ``nn.Linear`` whose weight is STORED as float8_e4m3fn (the reference's ``--layerwise_upcasting_modules transformer``:
storage fp8, compute bf16) -- the building block for adopting one layer at a time.  The weight is kept once, as bytes: the forward (``ftmi_gemm_nt_w8``) and
the input gradient (``ftmi_gemm_nn_w8``) read the same tensor, converting to bf16 in registers; no bf16 copy and no transposed copy exists at any time."""

from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from . import ops

FP8 = torch.float8_e4m3fn


def _pad_rank(a: torch.Tensor, b: torch.Tensor, rp: int):
    """A [r, K] / B [N, r] zero-padded to rank rp (the kernels take ranks in multiples of 64; the padding contributes exact zeros)."""
    r = a.shape[0]
    if r == rp:
        return a, b
    ap = a.new_zeros((rp, a.shape[1]))
    bp = b.new_zeros((b.shape[0], rp))
    ap[:r], bp[:, :r] = a, b
    return ap, bp


class _Fp8LoRALinearFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lora_a, lora_b, mod):
        r = 0 if lora_a is None else lora_a.shape[0]
        ap, bp = _pad_rank(lora_a.detach(), lora_b.detach(), mod.padded_rank) if r else (None, None)
        y, xa = ops.linear_lora_w8_fwd(x, mod.weight, mod.bias, ap, bp, mod.scaling)
        ctx.mod, ctx.r = mod, r
        ctx.save_for_backward(x, xa, ap, bp)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, xa, ap, bp = ctx.saved_tensors
        dx, ga, gb = ops.linear_lora_w8_bwd(x, dy.contiguous(), xa, ctx.mod.weight, ap, bp, ctx.mod.scaling, need_dx=ctx.needs_input_grad[0])
        r = ctx.r
        return dx, (ga[:r] if r else None), (gb[:, :r] if r else None), None


class MI355XFp8LoRALinear(nn.Module):
    """y = bf16(bf16(x W^T + b) + (lora_alpha / r) (x A^T) B^T) with W [N, K] stored as float8_e4m3fn and fp32 A [r, K], B [N, r].

    ``weight``: a floating-point [N, K] tensor, rounded to e4m3fn here (``tensor.to(torch.float8_e4m3fn)``), or an fp8 tensor taken as it is; N and K multiples
    of 128.  ``bias``: [N] or None (kept in bf16).  ``r = 0``: the plain frozen linear.  Parameter names are peft's (``lora_A.default.weight`` /
    ``lora_B.default.weight``); A starts kaiming-uniform, B zero.  Inputs are bf16 [..., K] on the GPU."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, r: int = 0, lora_alpha: Optional[float] = None):
        super().__init__()
        if weight.dim() != 2 or r < 0:
            raise ValueError("MI355XFp8LoRALinear: weight must be [out_features, in_features] and r >= 0")
        self.out_features, self.in_features = weight.shape
        self.register_buffer("weight", (weight if weight.dtype == FP8 else weight.detach().to(FP8)).contiguous())
        self.register_buffer("bias", None if bias is None else bias.detach().to(torch.bfloat16).contiguous())
        self.r, self.padded_rank = r, (r + 63) // 64 * 64
        self.scaling = float(r if lora_alpha is None else lora_alpha) / r if r else 0.0
        if r:
            self.lora_A = nn.ModuleDict({"default": nn.Linear(self.in_features, r, bias=False, device=weight.device, dtype=torch.float32)})
            self.lora_B = nn.ModuleDict({"default": nn.Linear(r, self.out_features, bias=False, device=weight.device, dtype=torch.float32)})
            nn.init.kaiming_uniform_(self.lora_A["default"].weight, a=math.sqrt(5))
            nn.init.zeros_(self.lora_B["default"].weight)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        a, b = (self.lora_A["default"].weight, self.lora_B["default"].weight) if self.r else (None, None)
        y = _Fp8LoRALinearFunction.apply(x.reshape(-1, self.in_features).contiguous(), a, b, self)
        return y.view(*x.shape[:-1], self.out_features)
