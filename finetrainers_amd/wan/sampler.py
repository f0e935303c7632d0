"""Validation sampling in latent space for the MI355X Wan backend: text-to-video, image-to-video and control.

The reference validates by running a diffusers pipeline's denoising loop over the transformer that is being trained (finetrainers/models/wan/
base_specification.py:495-529; control_specification.py:310-377 with the control latents concatenated on the channels).  Here the loop -- DiT forward on the
unconditional + conditional prompt, classifier-free-guidance combine, flow-match Euler update -- is ONE C call (``ftmi_wan_sample``, no host synchronisation)
over this backend's flat-buffer model with its current adapters.  The sampler state stays in the patch embedding's operand layout (csrc/sample_layout.hip), so
nothing is patchified between steps.  Text / image encoding and the VAE stay outside: the sampler takes embeddings and latents and returns denormalised
latents (INTEGRATION.md shows the hand-over to the reference pipeline's VAE decode).

The state and the guidance combine are kept in fp32 -- a deliberate choice, like the LTX sampler's: [upstream, unpinned] ``WanPipeline`` holds the latents in
fp32 as well and casts them to the transformer's dtype per step; its combine runs on the bf16 model output, here on its fp32 values (one rounding less).
"""

from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from .. import _lib, ops
from ..cogvideox.model import timestep_embedding
from .block import _WanLoRABlockNativeFunction
from .model import MI355XWanTransformer3DModel, bf16

# [upstream, unpinned] ``FlowMatchEulerDiscreteScheduler()`` with no arguments, which is what the reference builds for Wan (base_specification.py:328)
WAN_SCHEDULER_CONFIG: Dict[str, Any] = {"num_train_timesteps": 1000, "shift": 1.0, "use_dynamic_shifting": False}


def wan_flow_match_sigmas(num_inference_steps: int, scheduler_config: Optional[Dict[str, Any]] = None) -> torch.Tensor:
    """Sigma table of a sampling run: fp32 [num_inference_steps + 1] on the host, decreasing, ending in 0.

    [upstream, unpinned] restates ``FlowMatchEulerDiscreteScheduler.set_timesteps(n)`` without dynamic shifting.  The constructor builds
    ``sigmas = shift * s / (1 + (shift - 1) * s)`` over ``s = (N, ..., 1) / N`` and keeps ``sigma_max = sigmas[0]`` (= 1) and ``sigma_min = sigmas[-1]`` (the
    shifted ``1 / N``); ``set_timesteps`` takes ``linspace(sigma_max, sigma_min, n)`` and applies the static shift to it -- again, the way the scheduler does
    -- then appends 0.  With shift 1 the table is ``linspace(1, 1 / N, n)``.  The timestep the model sees at step i is ``sigma_i * N``."""
    cfg = dict(WAN_SCHEDULER_CONFIG if scheduler_config is None else scheduler_config)
    n = int(num_inference_steps)
    if n < 1:
        raise ValueError("wan_flow_match_sigmas: at least one step")
    if cfg.get("use_dynamic_shifting", False):
        raise NotImplementedError("wan_flow_match_sigmas: dynamic shifting is not part of the scheduler the reference builds for Wan")
    N, shift = float(cfg.get("num_train_timesteps", 1000)), float(cfg.get("shift", 1.0))
    apply = lambda s: shift * s / (1.0 + (shift - 1.0) * s)
    sigma_max, sigma_min = apply(1.0), apply(1.0 / N)
    s = apply(torch.linspace(sigma_max, sigma_min, n, dtype=torch.float64))
    return torch.cat([s, s.new_zeros(1)]).to(torch.float32)


class MI355XWanLatentSampler:
    """Denoising loop over a ``MI355XWanTransformer3DModel`` (``ftmi_wan_sample``).  The adapters are read at every ``sample``: a sample taken between two
    optimiser steps sees them as they are, the folded patch adapter is folded again at the first step of every call."""

    def __init__(self, transformer: MI355XWanTransformer3DModel, scheduler_config: Optional[Dict[str, Any]] = None):
        self.transformer = transformer
        self.scheduler_config = dict(WAN_SCHEDULER_CONFIG if scheduler_config is None else scheduler_config)

    # -- what the model is ---------------------------------------------------------------------------------------------------------------------------
    @property
    def extra_channels(self) -> int:
        """Input channels past the latents: 20 for image-to-video (4 mask + 16 condition), 16 for a control model, 0 for text-to-video."""
        c = self.transformer.config
        return c.in_channels - c.out_channels

    def _check_model(self) -> None:
        tr = self.transformer
        if tr.root.numel() < tr.root_layout.total or tr._root_src is not None or any(b.flat.numel() < b.layout.total or b._param_src is not None for b in tr.blocks):
            raise RuntimeError("MI355XWanLatentSampler: the parameters are sharded over the ranks (FSDP); sample from a model that holds its whole flat buffers")
        first = tr.blocks[0]
        for blk in tr.blocks:
            same = (blk.lora_A is None) == (first.lora_A is None) and (blk.lora_ffn is None) == (first.lora_ffn is None) and blk.lora_scale == first.lora_scale
            if not same or (blk.lora_A is not None and blk.lora_A.shape != first.lora_A.shape):
                raise NotImplementedError("MI355XWanLatentSampler: every block carries the same adapter set, rank and scale")

    # -- the state-independent inputs of the loop ----------------------------------------------------------------------------------------------------
    def _lin(self, t: torch.Tensor, name: str, **kw):
        tr = self.transformer
        return ops.gemm_nt(t.reshape(-1, t.shape[-1]), tr.rparam(f"{name}.weight"), tr.rparam(f"{name}.bias"), **kw)

    def text_rows(self, prompt_embeds: torch.Tensor, negative_prompt_embeds: Optional[torch.Tensor]) -> torch.Tensor:
        """enc bf16 [P B, T, D]: the text embedder on the unconditional rows, then the conditional ones (the launches of the model's forward at batch P B)."""
        dev = self.transformer.device
        text = prompt_embeds if negative_prompt_embeds is None else torch.cat([negative_prompt_embeds.to(prompt_embeds.device), prompt_embeds], dim=0)
        text = text.to(dev, bf16).contiguous()
        act, _ = self._lin(text, "condition_embedder.text_embedder.linear_1", epilogue=1, want_out2=True)
        return self._lin(act, "condition_embedder.text_embedder.linear_2").view(text.shape[0], text.shape[1], -1)

    def step_tables(self, timesteps: torch.Tensor, rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (tproj bf16 [n, 6 D], head shift fp32 [n, D], head scale fp32 [n, D]) for the n timesteps of a run.  Every step runs the condition embedder's
        launches at ``rows`` = P B equal timesteps, as the model's forward does, and keeps one row: the rounding points are those of model.py's forward
        (``mod = table + temb`` in bf16, ``shift = float(mod[0])``, ``scale = float(1 + mod[1]) - 1``)."""
        tr = self.transformer
        c, silu = tr.config, torch.nn.functional.silu
        tprojs, shifts, scales = [], [], []
        table = tr.rparam("scale_shift_table")
        for t in timesteps.tolist():
            ts = torch.full((rows,), t, dtype=torch.float32, device=tr.device)
            t_emb = timestep_embedding(ts, c.freq_dim).to(bf16)
            temb = self._lin(silu(self._lin(t_emb, "condition_embedder.time_embedder.linear_1")), "condition_embedder.time_embedder.linear_2")
            tprojs.append(self._lin(silu(temb), "condition_embedder.time_proj")[0])
            mod = table + temb.unsqueeze(1)  # [rows, 2, D] bf16
            shifts.append(mod[0, 0].float())
            scales.append((1 + mod[0, 1]).float() - 1)
        return torch.stack(tprojs).contiguous(), torch.stack(shifts).contiguous(), torch.stack(scales).contiguous()

    def geometry(self, B: int, num_frames: int, height: int, width: int, guidance: bool) -> "_lib.WanSampleGeometry":
        tr = self.transformer
        c = tr.config
        Kp = tr.root_layout.offsets["patch_embedding.weight"][1][1]
        return ops.wan_sample_geometry(B, c.out_channels, num_frames, height, width, Kp, extra_channels=self.extra_channels,
                                       copies=2 if tr.patch_lora_A is not None else 1, guidance=guidance, patch_size=tuple(c.patch_size),
                                       po=tr.root_layout.offsets["proj_out.weight"][1][0])

    def c_arguments(self, geo, T: int, TI: int, steps: int, guidance_scale: float):
        """-> (ftmi_wan_sample_config, ftmi_wan_sample_weights, the objects the two structures point into).  ``TI``: the image tokens of one row of enc_img; of a
        first/last-frame model (``config.pos_embed_seq_len``) both images', whose second half goes into the structures as TI2."""
        tr = self.transformer
        c = tr.config
        TI2 = c.second_image_tokens if TI > 0 else 0
        if TI2 and TI != 2 * TI2:
            raise ValueError(f"sample: a first/last-frame model takes {2 * TI2} image tokens (pos_embed_seq_len), got {TI}")
        TI -= TI2
        S, rows = (geo.F // geo.pt) * (geo.H // geo.ph) * (geo.W // geo.pw), geo.P * geo.B
        L = len(tr.blocks)
        blocks = (_lib.WanLoraFfnBlockWeights * L)()
        img = (ctypes.c_void_p * L)()
        keep: List[Any] = [blocks, img]
        first = tr.blocks[0]
        for i, blk in enumerate(tr.blocks):
            ffn = tuple(blk.lora_ffn) if blk.lora_ffn is not None else None
            _, wf, k = _WanLoRABlockNativeFunction._args(blk, rows, S, T, blk.lora_A, blk.lora_B, backward=False, TI=TI, ffn=ffn)
            blocks[i] = wf
            keep += k
            if TI > 0:
                img[i] = blk._img_params().data_ptr()
        r = 0 if first.lora_A is None else int(first.lora_A.shape[1])
        fold = tr.patch_lora_A is not None
        cfg = _lib.WanSampleConfig(geo=geo, T=T, TI=TI, D=c.inner_dim, heads=c.num_attention_heads, ffn_dim=c.ffn_dim, L=L, eps=float(c.eps), gemm_variant=8, r=r,
                                   lora_scale=float(first.lora_scale), ffn=int(first.lora_ffn is not None), patch_fold=int(fold),
                                   patch_r=int(tr.patch_lora_A.shape[0]) if fold else 0, patch_scale=float(tr.patch_lora_scale) if fold else 0.0, steps=steps,
                                   guidance=float(guidance_scale), TI2=TI2)
        w = _lib.WanSampleWeights()
        w.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.WanLoraFfnBlockWeights))
        w.img_params = ctypes.cast(img, ctypes.POINTER(ctypes.c_void_p)) if TI > 0 else None
        w.patch_w, w.patch_b = tr.rparam("patch_embedding.weight").data_ptr(), tr.rparam("patch_embedding.bias").data_ptr()
        w.proj_w, w.proj_b = tr.rparam("proj_out.weight").data_ptr(), tr.rparam("proj_out.bias").data_ptr()
        if fold:
            la, lb = tr.patch_lora_A.detach().contiguous(), tr.patch_lora_B.detach().contiguous()
            dw, w2, _ = tr._patch_ws
            keep += [la, lb]
            w.patch_lora_a, w.patch_lora_b, w.patch_dw, w.patch_w2 = la.data_ptr(), lb.data_ptr(), dw.data_ptr(), w2.data_ptr()
            tr._patch_fold_key = None  # the call folds the adapter as it is now into the model's workspace: the next training forward folds for itself
        return cfg, w, keep

    def schedule(self, num_inference_steps: int, sigmas, timesteps) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (sigmas fp32 [n + 1], timesteps fp32 [n]) on the host."""
        sig = wan_flow_match_sigmas(num_inference_steps, self.scheduler_config) if sigmas is None else torch.as_tensor(sigmas, dtype=torch.float32).reshape(-1).cpu()
        n = sig.numel() - 1
        if n < 1:
            raise ValueError("sample: sigmas must hold n + 1 values")
        ts = sig[:-1] * float(self.scheduler_config.get("num_train_timesteps", 1000)) if timesteps is None else torch.as_tensor(timesteps, dtype=torch.float32).reshape(-1).cpu()
        if ts.numel() != n:
            raise ValueError("sample: timesteps must hold one value per step")
        return sig, ts

    def check_inputs(self, prompt_embeds, negative_prompt_embeds, guidance_scale: float, image_embeds, condition_latents, control_latents, B: int, num_frames: int,
                     height: int, width: int) -> Optional[torch.Tensor]:
        """Every refusal of ``sample``, with its reason; -> the extra input channels [B, Cx, F, H, W] bf16 (None for text-to-video)."""
        tr = self.transformer
        c = tr.config
        self._check_model()
        if prompt_embeds.dim() != 3 or prompt_embeds.shape[-1] != c.text_dim:
            raise ValueError(f"sample: prompt_embeds must be [B, T, {c.text_dim}], got {tuple(prompt_embeds.shape)}")
        if float(guidance_scale) != 1.0:
            if negative_prompt_embeds is None:
                raise ValueError("sample: guidance_scale != 1 needs negative_prompt_embeds")
            if tuple(negative_prompt_embeds.shape) != tuple(prompt_embeds.shape):
                raise ValueError("sample: negative_prompt_embeds must be shaped like prompt_embeds (pad both prompts to one length)")
        i2v = c.image_dim is not None
        widened = not i2v and c.in_channels > c.out_channels
        if (image_embeds is not None or condition_latents is not None) and not i2v:
            raise ValueError("sample: image_embeds / condition_latents go with an image-to-video model (config.image_dim); this model has none")
        if i2v and (image_embeds is None or condition_latents is None):
            raise ValueError("sample: an image-to-video model (config.image_dim) needs image_embeds and condition_latents")
        if control_latents is not None and not widened:
            raise ValueError("sample: control_latents go with a model whose patch embedding was widened (expand_patch_embedding); this one takes "
                             f"{c.in_channels} channels for {c.out_channels} latent channels")
        if widened and control_latents is None:
            raise ValueError(f"sample: the patch embedding was widened to {c.in_channels} channels: the model needs control_latents")
        extra = condition_latents if i2v else control_latents
        if extra is None:
            return None
        want = (B, self.extra_channels, num_frames, height, width)
        if tuple(extra.shape) != want:
            raise ValueError(f"sample: {'condition_latents' if i2v else 'control_latents'} must be {list(want)}, got {list(extra.shape)}")
        if i2v and c.pos_embed_seq_len is not None:  # first/last-frame: both layouts of the image embedder, see MI355XWanTransformer3DModel._embed_image
            n = c.pos_embed_seq_len
            if image_embeds.dim() != 3 or tuple(image_embeds.shape) not in ((B, n, c.image_dim), (2 * B, n // 2, c.image_dim)):
                raise ValueError(f"sample: image_embeds of a first/last-frame model must be [{B}, {n}, {c.image_dim}] or [{2 * B}, {n // 2}, {c.image_dim}], "
                                 f"got {tuple(image_embeds.shape)}")
        elif i2v and (image_embeds.dim() != 3 or image_embeds.shape[0] != B or image_embeds.shape[-1] != c.image_dim):
            raise ValueError(f"sample: image_embeds must be [{B}, TI, {c.image_dim}], got {tuple(image_embeds.shape)}")
        return extra.to(tr.device, bf16).contiguous()

    @torch.no_grad()
    def sample(self, prompt_embeds: torch.Tensor, negative_prompt_embeds: Optional[torch.Tensor], num_frames: int, height: int, width: int,
               num_inference_steps: int = 50, guidance_scale: float = 5.0, sigmas: Optional[Sequence[float]] = None, timesteps: Optional[Sequence[float]] = None,
               generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None, latents_mean: Optional[torch.Tensor] = None,
               latents_std: Optional[torch.Tensor] = None, image_embeds: Optional[torch.Tensor] = None, condition_latents: Optional[torch.Tensor] = None,
               control_latents: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> denormalised latents [B, C, F, H, W] bf16 (the VAE decoder's input).

        ``num_frames`` / ``height`` / ``width`` are the LATENT grid.  ``sigmas`` [n + 1] / ``timesteps`` [n] override the schedule (default:
        ``wan_flow_match_sigmas`` and ``sigma * num_train_timesteps``); the rows of one step share one timestep, as in the pipeline.  The initial noise is
        ``torch.randn([B, C, F, H, W], fp32, generator)`` on the transformer's device -- the pipeline's draw order, so one seed gives the same noise -- or
        ``latents``.  ``latents_mean`` / ``latents_std`` ([C]: the VAE's statistics, the standard deviation ITSELF, not the 1 / std of the training
        processors) denormalise the result; without them it stays normalised.

        Image-to-video: ``image_embeds`` [B, TI, image_dim] (the CLIP tokens, sent through the model's image embedder; a first/last-frame model takes
        [B, TI + TI2, image_dim] = [B, pos_embed_seq_len, image_dim], a sample's first image and then its last, or [2B, TI, image_dim]) and ``condition_latents``
        [B, 20, F, H, W] (4 mask + 16 normalised condition channels, what the pipeline concatenates to the latents).  Control: ``control_latents``
        [B, 16, F, H, W], normalised and frame-conditioned (``validation_latents`` of the control specification does both).  These channels are constant over
        the loop: they are written into the model input once."""
        tr = self.transformer
        dev, c = tr.device, tr.config
        B, T = prompt_embeds.shape[0], prompt_embeds.shape[1]
        g = float(guidance_scale)
        extra = self.check_inputs(prompt_embeds, negative_prompt_embeds, g, image_embeds, condition_latents, control_latents, B, num_frames, height, width)
        sig, ts = self.schedule(num_inference_steps, sigmas, timesteps)
        if latents is None:
            latents = torch.randn((B, c.out_channels, num_frames, height, width), generator=generator, device=dev, dtype=torch.float32)
        elif tuple(latents.shape) != (B, c.out_channels, num_frames, height, width):
            raise ValueError(f"sample: latents must be [{B}, {c.out_channels}, {num_frames}, {height}, {width}], got {list(latents.shape)}")
        latents = latents.to(dev, torch.float32).contiguous()

        geo = self.geometry(B, num_frames, height, width, guidance=g != 1.0)
        enc = self.text_rows(prompt_embeds, negative_prompt_embeds if g != 1.0 else None)
        enc_img = None
        if image_embeds is not None:
            if c.pos_embed_seq_len is not None:
                image_embeds = image_embeds.reshape(B, c.pos_embed_seq_len, c.image_dim)
            enc_img = tr._embed_image(torch.cat([image_embeds] * geo.P, dim=0))
        tproj, shift, scale = self.step_tables(ts, geo.P * B)
        cfg, weights, keep = self.c_arguments(geo, T, 0 if enc_img is None else enc_img.shape[1], ts.numel(), g)
        x, cols = ops.wan_sample_init(geo, latents, extra)
        ops.wan_sample(cfg, weights, cols, x, tproj, shift, scale, enc, enc_img, tr._rope(num_frames, height, width), sig.to(dev))
        del keep
        C = c.out_channels
        mean = torch.zeros(C, dtype=torch.float32, device=dev) if latents_mean is None else latents_mean.reshape(-1)[:C].to(dev, torch.float32).contiguous()
        std = torch.ones(C, dtype=torch.float32, device=dev) if latents_std is None else latents_std.reshape(-1)[:C].to(dev, torch.float32).contiguous()
        return ops.wan_sample_finish(geo, x, mean, std)
