"""A plain torch restatement of the HunyuanVideo validation loop, written from the description of [upstream, unpinned] ``HunyuanVideoPipeline`` +
``FlowMatchEulerDiscreteScheduler`` (static shift, embedded guidance, optional true CFG): what the tests of the latent sampler compare against.  Nothing here
calls the library."""
from typing import Callable, Optional

import torch


def sigmas(n: int, shift: float = 7.0) -> torch.Tensor:
    """fp64 [n + 1], the way the scheduler gets there: the pipeline's ``linspace(1, 0, n + 1)[:-1]``, the static shift, a terminal zero."""
    s = torch.linspace(1.0, 0.0, n + 1, dtype=torch.float64)[:-1]
    s = shift * s / (1.0 + (shift - 1.0) * s)
    return torch.cat([s, s.new_zeros(1)])


def patchify(latents: torch.Tensor, p: int = 2, pt: int = 1) -> torch.Tensor:
    """[B, C, F, H, W] -> [B, S, C pt p p]: tokens in (f, h, w) order, columns in (c, pt, ph, pw) order (the Conv3d patch embedding as a GEMM)."""
    B, C, F_, H, W = latents.shape
    f, h, w = F_ // pt, H // p, W // p
    return latents.reshape(B, C, f, pt, h, p, w, p).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, f * h * w, C * pt * p * p)


def unpatchify(tokens: torch.Tensor, C: int, F_: int, H: int, W: int, p: int = 2, pt: int = 1) -> torch.Tensor:
    """The model's un-patchify of ``proj_out``'s output: [B, S, C pt p p] -> [B, C, F, H, W]."""
    B = tokens.shape[0]
    f, h, w = F_ // pt, H // p, W // p
    return tokens.reshape(B, f, h, w, -1, pt, p, p).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(B, C, F_, H, W)


def trajectory(model: Callable[[torch.Tensor, int, float], torch.Tensor], x0: torch.Tensor, sig: torch.Tensor, true_cfg: float = 1.0,
               round_to: Optional[torch.dtype] = None) -> torch.Tensor:
    """x <- x + (sigma_{i+1} - sigma_i) v over the steps of ``sig`` [n + 1].  ``model(x, i, t)`` returns the velocity for the state ``x`` at step ``i`` and
    timestep ``t = 1000 sigma_i``; with ``true_cfg != 1`` it returns [2 B, ...], unconditional rows first, combined as ``u + g (c - u)``.  ``round_to``: the
    dtype upstream keeps the latents in (they are rounded to it after every step)."""
    x = x0.clone()
    B = x.shape[0]
    for i in range(sig.numel() - 1):
        v = model(x, i, float(sig[i]) * 1000.0).to(x.dtype)
        if true_cfg != 1.0:
            u, c = v[:B], v[B:]
            v = u + true_cfg * (c - u)
        x = x + (float(sig[i + 1]) - float(sig[i])) * v
        if round_to is not None:
            x = x.to(round_to).to(x0.dtype)
    return x
