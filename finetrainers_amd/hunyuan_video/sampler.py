"""Validation sampling in latent space for the MI355X HunyuanVideo backend: text-to-video over the transformer that is being trained, with or without adapters,
with bf16 weights or real fp8 storage (``apply_layerwise_casting()``).

The reference validates by running ``HunyuanVideoPipeline`` over a diffusers transformer (finetrainers/models/hunyuan_video/base_specification.py:332-355).  That
pipeline cannot take this backend's blocks -- flat frozen buffers, fp32 adapters, fp8 bytes that exist as bf16 only inside a shared arena -- and
``MI355XHunyuanVideoTransformer3DModel.forward`` is a training path: an autograd function and a ``saved`` area per block, torch permutes around the patch
embedding, a ``torch.cat`` of the two streams.  Here the loop -- DiT forward, optional true-CFG combine, flow-match Euler update -- is ONE C call
(``ftmi_hy_sample_text``, no host synchronisation) that issues the same block launches out of a workspace that does not grow with the number of blocks, with the
adapters as they are at the moment of the call.  The sampler state stays in the patch embedding's operand layout, which is also ``proj_out``'s column order
(csrc/sample_layout.hip), so nothing is patchified between steps.  Text encoding and the VAE stay outside: the sampler takes embeddings and noise and returns
``latents / scaling_factor`` (INTEGRATION.md shows the hand-over to the reference pipeline's VAE decode).

[upstream, unpinned] The arithmetic restates ``HunyuanVideoPipeline`` / ``FlowMatchEulerDiscreteScheduler`` as of diffusers 0.33 (neither is vendored here):
``sigmas = linspace(1, 0, n + 1)[:-1]`` through the static shift (7.0 for the checkpoint), a terminal 0 appended; the model sees ``t = 1000 sigma`` as a
float; the guidance scale is EMBEDDED (``guidance_scale * 1000`` in the transformer dtype), not classifier-free; newer pipelines add an optional true CFG over a
negative prompt, ``v = u + g (c - u)`` with the unconditional rows first; ``x <- x + (sigma_next - sigma) v``.

The state and the true-CFG combine are kept in fp32 -- a deliberate choice, like the LTX, Wan and CogVideoX samplers': upstream rounds the latents to the
transformer dtype (bf16) after every step; here the model still sees bf16(x) every step, but the state between steps carries no extra rounding.  Not covered,
refused by name: dynamic shifting, ``guidance_embeds = False`` checkpoints (and with them image-to-video), ``patch_size_t != 1``.  Per-sample timesteps and
multi-GPU sampling are not built."""

from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional

import torch

from .. import _lib, ops
from .._lib import HY_DUAL_WEIGHT_FIELDS, HY_SINGLE_WEIGHT_FIELDS
from .model import MI355XHunyuanVideoTransformer3DModel, bf16

# [upstream, unpinned] scheduler/scheduler_config.json of hunyuanvideo-community/HunyuanVideo (FlowMatchEulerDiscreteScheduler)
HY_SCHEDULER_CONFIG: Dict[str, Any] = {"num_train_timesteps": 1000, "shift": 7.0}


def hy_flow_match_sigmas(num_inference_steps: int, scheduler_config: Optional[Dict[str, Any]] = None) -> torch.Tensor:
    """-> sigmas fp64 [n + 1] on the host.  [upstream, unpinned] the pipeline passes ``sigmas = linspace(1, 0, n + 1)[:-1]``; ``set_timesteps`` applies the
    static shift ``s sigma / (1 + (s - 1) sigma)`` and appends 0: ``sigma_i = s (1 - i/n) / (1 + (s - 1)(1 - i/n))``, ``sigma_0 = 1``, ``sigma_n = 0``."""
    cfg = dict(HY_SCHEDULER_CONFIG if scheduler_config is None else scheduler_config)
    if cfg.get("use_dynamic_shifting", False):
        raise NotImplementedError("hy_flow_match_sigmas: use_dynamic_shifting (a resolution-dependent shift) is not what the HunyuanVideo checkpoints configure")
    n = int(num_inference_steps)
    if n < 1:
        raise ValueError("hy_flow_match_sigmas: at least one step")
    s = float(cfg.get("shift", 7.0))
    if not s > 0:
        raise ValueError(f"hy_flow_match_sigmas: shift must be positive, got {s}")
    u = 1.0 - torch.arange(n + 1, dtype=torch.float64) / n
    sig = s * u / (1.0 + (s - 1.0) * u)
    sig[0], sig[n] = 1.0, 0.0
    return sig


def _block_weights(blk, fields, struct, arena: Optional[torch.Tensor]):
    """-> (the C weight structure of one block for a forward, its fp8 up-cast list, the tensors it points into).  With fp8 storage the 2-D weights are the
    views ``_materialize_fwd`` would make: consecutive pieces of the shared arena in the order of ``_w8``."""
    w, ups, keep = struct(), [], []
    offsets = {}
    if blk._w8 is not None:
        off = 0
        for n, w8 in blk._w8.items():
            offsets[n] = off
            ups.append((w8, int(w8.shape[0]), int(w8.shape[1]), off))
            off += w8.numel()
    for n in fields:
        if n in ("lora_a", "lora_b") or n.endswith("_t"):
            continue
        if n in offsets:
            setattr(w, n, arena.data_ptr() + 2 * offsets[n])
            continue
        t = getattr(blk, n)
        if t is None or not t.is_contiguous():
            raise RuntimeError(f"sample: block weight '{n}' is not materialised")
        keep.append(t)
        setattr(w, n, t.data_ptr())
    if blk.lora_A is not None:
        la, lb = blk.lora_A.detach().contiguous(), blk.lora_B.detach().contiguous()
        keep += [la, lb]
        w.lora_a, w.lora_b = la.data_ptr(), lb.data_ptr()
    return w, ups, keep


class MI355XHunyuanVideoLatentSampler:
    """Denoising loop over a ``MI355XHunyuanVideoTransformer3DModel`` (``ftmi_hy_sample_text``).  The adapters are read at every ``sample``: a sample taken between
    two optimiser steps sees them as they are."""

    def __init__(self, transformer: MI355XHunyuanVideoTransformer3DModel, scheduler_config: Optional[Dict[str, Any]] = None):
        self.transformer = transformer
        self.scheduler_config = dict(HY_SCHEDULER_CONFIG if scheduler_config is None else scheduler_config)

    # -- every refusal, with its reason --------------------------------------------------------------------------------------------------------------
    def check_inputs(self, latents, prompt_embeds, prompt_attention_mask, pooled_prompt_embeds, negative_prompt_embeds, negative_prompt_attention_mask,
                     negative_pooled_prompt_embeds, true_cfg_scale: float) -> None:
        tr = self.transformer
        c = tr.config
        if not c.guidance_embeds:
            raise NotImplementedError("sample: this model has guidance_embeds = False (an image-to-video or distillation-free checkpoint); only the "
                                      "guidance-embedding text-to-video checkpoints are restated here")
        if c.patch_size_t != 1:
            raise NotImplementedError(f"sample: patch_size_t = {c.patch_size_t}; every published HunyuanVideo checkpoint has patch_size_t = 1")
        if prompt_embeds.dim() != 3 or prompt_embeds.shape[-1] != c.text_embed_dim:
            raise ValueError(f"sample: prompt_embeds must be [B, T, {c.text_embed_dim}], got {tuple(prompt_embeds.shape)}")
        B, T = prompt_embeds.shape[:2]
        if pooled_prompt_embeds is None or tuple(pooled_prompt_embeds.shape) != (B, c.pooled_projection_dim):
            raise ValueError(f"sample: pooled_prompt_embeds must be [{B}, {c.pooled_projection_dim}]")
        if prompt_attention_mask is not None and tuple(prompt_attention_mask.shape) != (B, T):
            raise ValueError(f"sample: prompt_attention_mask must be [{B}, {T}], got {tuple(prompt_attention_mask.shape)}")
        if float(true_cfg_scale) != 1.0:
            if negative_prompt_embeds is None or negative_pooled_prompt_embeds is None:
                raise ValueError("sample: true_cfg_scale != 1 needs negative_prompt_embeds and negative_pooled_prompt_embeds")
            if tuple(negative_prompt_embeds.shape) != tuple(prompt_embeds.shape) or tuple(negative_pooled_prompt_embeds.shape) != tuple(pooled_prompt_embeds.shape):
                raise ValueError("sample: the negative inputs must be shaped like the prompt's")
            if negative_prompt_attention_mask is not None and tuple(negative_prompt_attention_mask.shape) != (B, T):
                raise ValueError(f"sample: negative_prompt_attention_mask must be [{B}, {T}]")
        p = c.patch_size
        if latents.dim() != 5 or latents.shape[0] != B or latents.shape[1] != c.in_channels:
            raise ValueError(f"sample: latents must be [{B}, {c.in_channels}, F, H, W] (the initial noise), got {list(latents.shape)}")
        if latents.shape[3] % p or latents.shape[4] % p:
            raise ValueError(f"sample: the latent height and width must be multiples of patch_size = {p}, got {latents.shape[3]} x {latents.shape[4]}")
        blocks = list(tr.transformer_blocks) + list(tr.single_transformer_blocks)
        if not blocks:
            raise ValueError("sample: a model without blocks")
        ranks = {0 if b.lora_A is None else int(b.lora_A.shape[1]) for b in blocks}
        scales = {float(b.lora_scale) for b in blocks if b.lora_A is not None}
        if len(ranks) > 1 or len(scales) > 1:
            raise NotImplementedError("sample: every block carries the same adapter rank and scale (add_adapter on the model), or none does")
        if len({b.text_adapters for b in tr.transformer_blocks}) > 1:
            raise NotImplementedError("sample: every dual-stream block carries text-stream adapters (add_adapter on the model with the recipe's "
                                      "target_modules), or none does")
        if tr.proj_out_w_t is None:
            raise RuntimeError("sample: load_diffusers_state_dict first")

    # -- the state-independent inputs of the loop ----------------------------------------------------------------------------------------------------
    def step_tables(self, sigmas: torch.Tensor, guidance_scale: float, text: torch.Tensor, mask: Optional[torch.Tensor], pooled: torch.Tensor):
        """-> (temb_silu bf16 [n, rows, D], enc bf16 [n, rows, T, D], head shift bf16 [n, rows, D], head 1 + scale bf16 [n, rows, D]) for the n steps of
        ``sigmas`` [n + 1].  Every step runs the model's own ``_conditioning`` / ``_refine_text`` / ``norm_out.linear`` launches at ``rows`` = P B equal float
        timesteps ``1000 sigma_i``: the rounding points are ``forward``'s.  The refined text depends on the timestep, so it is per step.
        ``guidance_scale * 1000`` is formed in bf16 as ``MI355XHunyuanVideoSpecOps.forward`` forms it for training: 6000 rounds to 6016."""
        tr = self.transformer
        D, silu = tr.config.inner_dim, torch.nn.functional.silu
        rows = text.shape[0]
        guidance = torch.full((rows,), float(guidance_scale), dtype=bf16, device=tr.device) * 1000.0
        tembs, encs, shifts, oneps = [], [], [], []
        for t in self.timesteps(sigmas).tolist():
            ts = torch.full((rows,), t, dtype=torch.float32, device=tr.device)
            temb = tr._conditioning(ts, guidance, pooled)
            encs.append(tr._refine_text(text, ts, mask))
            mod = tr._lin(silu(temb), "norm_out.linear").view(rows, 2, D)
            tembs.append(silu(temb.to(bf16)))
            shifts.append(mod[:, 1])
            oneps.append(1 + mod[:, 0])
        return tuple(torch.stack(v).contiguous() for v in (tembs, encs, shifts, oneps))

    @staticmethod
    def timesteps(sigmas: torch.Tensor) -> torch.Tensor:
        """[upstream, unpinned] ``timesteps = sigmas * num_train_timesteps`` in fp32, without the terminal sigma."""
        return sigmas[:-1].to(torch.float32) * 1000.0

    def geometry(self, B: int, frames: int, height: int, width: int, true_cfg: bool = False) -> "_lib.HySampleGeometry":
        c = self.transformer.config
        return ops.hy_sample_geometry(B, c.out_channels, frames, height, width, patch=c.patch_size, patch_t=c.patch_size_t, true_cfg=true_cfg)

    def c_arguments(self, geo, T: int, steps: int, true_cfg_scale: float = 1.0):
        """-> (ftmi_hy_sample_text_config, ftmi_hy_sample_weights, the objects the two structures point into).  The adapters are read here; ``text_adapters`` is 1
        for a model whose dual-stream blocks carry the text stream's adapters."""
        tr = self.transformer
        c = tr.config
        duals, singles = list(tr.transformer_blocks), list(tr.single_transformer_blocks)
        blocks = duals + singles
        first = blocks[0]
        r = 0 if first.lora_A is None else int(first.lora_A.shape[1])
        text_adapters = int(bool(duals) and duals[0].text_adapters)  # (check_inputs: all dual blocks alike)
        base = _lib.HySampleConfig(geo=geo, T=int(T), D=c.inner_dim, H=c.num_attention_heads, mlp=int(c.inner_dim * c.mlp_ratio), Ld=len(duals), Ls=len(singles), r=r,
                                   lora_scale=float(first.lora_scale), eps=1e-6, gemm_variant=8, steps=int(steps), true_cfg=float(true_cfg_scale))
        cfg = _lib.HySampleTextConfig(base=base, text_adapters=text_adapters)
        fp8 = any(b._w8 is not None for b in blocks)
        arena = getattr(tr, "_weight_arena_fwd", None) if fp8 else None
        if fp8 and (arena is None or not all(b._w8 is not None for b in blocks)):
            raise RuntimeError("sample: fp8 storage covers every block and comes with the model's arena (apply_layerwise_casting on the model)")
        keep: List[Any] = [arena]
        dw, sw = (_lib.HyDualWeights * max(1, len(duals)))(), (_lib.HySingleWeights * max(1, len(singles)))()
        ups, counts = [], []
        for arr, blks, fields, struct in ((dw, duals, HY_DUAL_WEIGHT_FIELDS, _lib.HyDualWeights), (sw, singles, HY_SINGLE_WEIGHT_FIELDS, _lib.HySingleWeights)):
            for i, blk in enumerate(blks):
                arr[i], u, k = _block_weights(blk, fields, struct, arena)
                ups += u
                counts.append(len(u))
                keep += k
        w = _lib.HySampleWeights()
        w.dual, w.single = ctypes.cast(dw, ctypes.POINTER(_lib.HyDualWeights)), ctypes.cast(sw, ctypes.POINTER(_lib.HySingleWeights))
        keep += [dw, sw]
        if fp8:
            ua = (_lib.HySampleUpcast * max(1, len(ups)))()
            for i, (w8, rows, cols, off) in enumerate(ups):
                ua[i] = _lib.HySampleUpcast(src=w8.data_ptr(), rows=rows, cols=cols, offset=off)
            ca = (ctypes.c_int * len(counts))(*counts)
            w.upcasts, w.upcast_count = ctypes.cast(ua, ctypes.POINTER(_lib.HySampleUpcast)), ctypes.cast(ca, ctypes.POINTER(ctypes.c_int))
            w.arena = arena.data_ptr()
            keep += [ua, ca, [u[0] for u in ups]]
        for field, t in (("patch_w", tr.p["x_embedder.proj.weight"]), ("patch_b", tr.p["x_embedder.proj.bias"]), ("proj_w", tr.p["proj_out.weight"]),
                         ("proj_b", tr.p["proj_out.bias"]), ("ones", tr.ones), ("zeros", tr.zeros)):
            setattr(w, field, t.data_ptr())
        return cfg, w, keep

    @torch.no_grad()
    def sample(self, latents: torch.Tensor, prompt_embeds: torch.Tensor, prompt_attention_mask: Optional[torch.Tensor], pooled_prompt_embeds: torch.Tensor,
               negative_prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_attention_mask: Optional[torch.Tensor] = None,
               negative_pooled_prompt_embeds: Optional[torch.Tensor] = None, num_inference_steps: int = 50, guidance_scale: float = 6.0,
               true_cfg_scale: float = 1.0, scaling_factor: float = 0.476986) -> torch.Tensor:
        """-> ``latents / scaling_factor`` bf16 [B, C, F, H, W] (the VAE decoder's input).

        ``latents`` [B, C, F, H, W] is the initial noise, drawn by the caller -- ``randn`` of that shape in the pipeline's order, so one seed gives the same
        noise.  ``prompt_embeds`` [B, T, text_embed_dim] with ``prompt_attention_mask`` [B, T] (1 = real token; None: all real) and ``pooled_prompt_embeds``
        [B, pooled_projection_dim].  ``guidance_scale`` is EMBEDDED: the model sees ``guidance_scale * 1000`` in bf16 (6000 rounds to 6016, as in training).
        ``true_cfg_scale`` != 1 runs the negative prompt's rows as well (unconditional rows first) and combines ``v = u + g (c - u)``; 1.0 runs the conditional
        rows only."""
        tr = self.transformer
        dev = tr.device
        g = float(true_cfg_scale)
        self.check_inputs(latents, prompt_embeds, prompt_attention_mask, pooled_prompt_embeds, negative_prompt_embeds, negative_prompt_attention_mask,
                          negative_pooled_prompt_embeds, g)
        sigmas = hy_flow_match_sigmas(num_inference_steps, self.scheduler_config)
        B, _, F_, H, W = latents.shape
        T = prompt_embeds.shape[1]
        geo = self.geometry(B, F_, H, W, true_cfg=g != 1.0)
        text, pooled, mask = prompt_embeds.to(dev), pooled_prompt_embeds.to(dev), prompt_attention_mask
        if g != 1.0:
            text = torch.cat([negative_prompt_embeds.to(dev), text], dim=0)
            pooled = torch.cat([negative_pooled_prompt_embeds.to(dev), pooled], dim=0)
            if mask is not None or negative_prompt_attention_mask is not None:
                ones = torch.ones((B, T), dtype=torch.bool, device=dev)
                mask = torch.cat([ones if negative_prompt_attention_mask is None else negative_prompt_attention_mask.to(dev).bool(),
                                  ones if mask is None else mask.to(dev).bool()], dim=0)
        temb_silu, enc, shift, onep = self.step_tables(sigmas, guidance_scale, text, mask, pooled)
        key_bias = self.key_bias(mask, geo, T)
        cos, sin = (t.contiguous() for t in tr._rope(F_, H, W))
        cfg, weights, keep = self.c_arguments(geo, T, num_inference_steps, g)
        x, cols = ops.hy_sample_init(geo, latents.to(dev, torch.float32).contiguous())
        ops.hy_sample(cfg, weights, cols, x, temb_silu, enc, shift, onep, key_bias, cos, sin, sigmas.to(torch.float32).to(dev))
        del keep
        return ops.hy_sample_finish(geo, x, 1.0 / float(scaling_factor))

    def key_bias(self, mask: Optional[torch.Tensor], geo, T: int) -> Optional[torch.Tensor]:
        """fp32 [P B, T + S]: -inf on the padded text keys, as the blocks build it from ``text_mask``; None without a mask."""
        if mask is None:
            return None
        dev = self.transformer.device
        S = (geo.F // geo.pt) * (geo.H // geo.p) * (geo.W // geo.p)
        kb = torch.zeros((mask.shape[0], T + S), dtype=torch.float32, device=dev)
        kb[:, :T].masked_fill_(~mask.to(dev).bool(), float("-inf"))
        return kb
