"""Validation sampling in latent space for the MI355X CogVideoX backend: text-to-video, for the 2b (sincos table), 5b (rotary) and 1.5 (``patch_size_t``)
geometries, with or without adapters.

The reference validates by running ``CogVideoXPipeline`` over the transformer that is being trained (finetrainers/models/cogvideox/base_specification.py:
335-364).  A diffusers pipeline cannot take this backend's stacked flat weights, and ``MI355XCogVideoXTransformer3DModel.forward`` is a training path (its
workspace keeps every block's activations for a backward).  Here the loop -- DiT forward on the unconditional + conditional prompt, classifier-free-guidance
combine, DDIM update -- is ONE C call (``ftmi_cog_sample``, no host synchronisation) over a forward-only walk of the same block launches, with the adapters as
they are at the moment of the call.  The sampler state stays in the patch embedding's operand layout, which is also ``proj_out``'s column order
(csrc/sample_layout.hip), so nothing is patchified between steps.  Text encoding and the VAE stay outside: the sampler takes embeddings and noise and returns
denormalised latents (INTEGRATION.md shows the hand-over to the reference pipeline's VAE decode).

[upstream, unpinned] The arithmetic restates ``CogVideoXDDIMScheduler`` / ``CogVideoXPipeline`` as of diffusers 0.33 (neither is vendored here):
``timestep_spacing = "trailing"``, v-prediction, eta = 0, ``set_alpha_to_one``; guidance ``v = u + g (c - u)`` with the unconditional rows first.  The
scheduler's step is linear in (x, v), so the host folds it, in fp64, into two numbers per step (``cog_ddim_tables``) and the kernel needs no scheduler logic.

The state and the guidance combine are kept in fp32 -- a deliberate choice, like the LTX and Wan samplers': upstream rounds the latents to the prompt dtype
(bf16) after every step and combines the bf16 model outputs; here the model still sees bf16(x) every step, but the state between steps carries no extra
rounding.  Not covered, refused by name: ``use_dynamic_cfg`` with this scheduler, image-to-video (``ofs``, doubled input channels).

[upstream, unpinned] The 5b and 1.5 checkpoints ship ``CogVideoXDPMScheduler``, and the reference's trainers hand ``load_pipeline`` no scheduler, so that is what
their validation videos are sampled with.  A scheduler config whose ``_class_name`` contains ``DPM`` selects it here: a second-order multistep SDE solver that
keeps the previous step's x0 prediction and adds fresh noise at every step but the last.  The host folds it, in fp64, into eight numbers per step
(``cog_dpm_tables``), the per-step guidance scale of ``use_dynamic_cfg`` among them; the loop is ``ftmi_cog_sample_ms``, the same per-step launches with
``ftmi_cog_sample_step_dpm`` last, the history in its workspace and the noise of every step (``cog_dpm_step_noise``: torch's generator in the pipeline's draw
order, so a seed means what it means there) packed into the state's layout before the call.
"""

from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch

from .. import _lib, ops
from .model import MI355XCogVideoXTransformer3DModel, bf16, rotary_tables, timestep_embedding
from .specification import CogVideoXDDIMTables

# [upstream, unpinned] scheduler/scheduler_config.json of the CogVideoX-2b checkpoint (CogVideoXDDIMScheduler)
COG_SCHEDULER_CONFIG: Dict[str, Any] = {"num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.0120, "snr_shift_scale": 3.0,
                                        "rescale_betas_zero_snr": True, "timestep_spacing": "trailing", "prediction_type": "v_prediction",
                                        "set_alpha_to_one": True}


# [upstream, unpinned] scheduler/scheduler_config.json of the CogVideoX-5b and CogVideoX1.5-5B checkpoints (CogVideoXDPMScheduler), written from memory of the
# checkpoints: a default only -- in real use ``wire.load_scheduler_config(dir)`` reads the file itself.
COG_DPM_SCHEDULER_CONFIG: Dict[str, Any] = {"_class_name": "CogVideoXDPMScheduler", "num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.0120,
                                            "snr_shift_scale": 1.0, "rescale_betas_zero_snr": True, "timestep_spacing": "trailing",
                                            "prediction_type": "v_prediction", "set_alpha_to_one": True}


def is_dpm(cfg: Optional[Dict[str, Any]]) -> bool:
    """Whether a scheduler config names the multistep solver (``_class_name`` contains ``DPM``)."""
    return cfg is not None and "DPM" in str(cfg.get("_class_name", ""))


def _scheduler_tables(cfg: Dict[str, Any], multistep: bool = False) -> CogVideoXDDIMTables:
    name = str(cfg.get("_class_name", "CogVideoXDDIMScheduler"))
    if "DPM" in name and not multistep:
        raise NotImplementedError(f"cog_ddim_tables: {name} is a multistep solver: cog_dpm_tables restates it")
    if cfg.get("timestep_spacing", "trailing") != "trailing" or cfg.get("prediction_type", "v_prediction") != "v_prediction":
        raise NotImplementedError("cog_ddim_tables: the CogVideoX checkpoints sample with timestep_spacing = 'trailing' and prediction_type = 'v_prediction'")
    if not cfg.get("set_alpha_to_one", True):
        raise NotImplementedError("cog_ddim_tables: set_alpha_to_one = False is not what the CogVideoX checkpoints configure")
    return CogVideoXDDIMTables(num_train_timesteps=int(cfg.get("num_train_timesteps", 1000)), beta_start=float(cfg.get("beta_start", 0.00085)),
                               beta_end=float(cfg.get("beta_end", 0.0120)), snr_shift_scale=float(cfg.get("snr_shift_scale", 3.0)),
                               rescale_betas_zero_snr=bool(cfg.get("rescale_betas_zero_snr", True)))


def cog_ddim_schedule(num_inference_steps: int, scheduler_config: Optional[Dict[str, Any]] = None) -> Tuple[List[int], List[int], torch.Tensor, torch.Tensor]:
    """-> (timesteps t_i, prev_i, alpha_bar_t fp64 [n], alpha_bar_prev fp64 [n]).  [upstream, unpinned] ``set_timesteps`` with trailing spacing:
    ``t_i = round(N - i N / n) - 1``; ``step``: ``prev_i = t_i - N // n`` (NOT t_{i+1} when n does not divide N; kept as upstream has it), and
    ``alpha_bar_prev = alphas_cumprod[prev_i]`` if ``prev_i >= 0`` else ``final_alpha_cumprod = 1``."""
    cfg = dict(COG_SCHEDULER_CONFIG if scheduler_config is None else scheduler_config)
    return _schedule(num_inference_steps, cfg, multistep=False)


def _schedule(num_inference_steps: int, cfg: Dict[str, Any], multistep: bool) -> Tuple[List[int], List[int], torch.Tensor, torch.Tensor]:
    """``cog_ddim_schedule`` over a given config; ``multistep``: a ``CogVideoXDPMScheduler`` config is accepted (the two schedulers share timesteps and prev)."""
    n = int(num_inference_steps)
    tables = _scheduler_tables(cfg, multistep)
    N = tables.config.num_train_timesteps
    if n < 1 or n > N:
        raise ValueError(f"cog_ddim_tables: between 1 and {N} steps")
    ts = [int(round(N - i * N / n)) - 1 for i in range(n)]
    prev = [t - N // n for t in ts]
    ac = tables.alphas_cumprod.double()
    a_t = torch.stack([ac[t] for t in ts])
    a_prev = torch.stack([ac[p] if p >= 0 else ac.new_ones(()) for p in prev])
    return ts, prev, a_t, a_prev


def cog_ddim_coefficients_f64(num_inference_steps: int, scheduler_config: Optional[Dict[str, Any]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (timesteps int64 [n], coef fp64 [n, 2]): the step ``x0 = sqrt(ab_t) x - sqrt(1 - ab_t) v;  a = sqrt((1 - ab_prev) / (1 - ab_t));
    b = sqrt(ab_prev) - sqrt(ab_t) a;  x <- a x + b x0`` folded into ``x <- cx x + cv v`` with ``cx = a + b sqrt(ab_t)``, ``cv = -b sqrt(1 - ab_t)``.
    With theta = atan2(sqrt(1 - ab), sqrt(ab)) these are cos / -sin of (theta_t - theta_prev): cx^2 + cv^2 = 1."""
    ts, _, a_t, a_prev = cog_ddim_schedule(num_inference_steps, scheduler_config)
    a = ((1 - a_prev) / (1 - a_t)).sqrt()
    b = a_prev.sqrt() - a_t.sqrt() * a
    coef = torch.stack([a + b * a_t.sqrt(), -b * (1 - a_t).sqrt()], dim=1)
    if not bool(torch.isfinite(coef).all()):
        raise ValueError("cog_ddim_tables: the scheduler configuration gives a non-finite step")
    return torch.tensor(ts, dtype=torch.int64), coef


def cog_ddim_tables(num_inference_steps: int, scheduler_config: Optional[Dict[str, Any]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (timesteps int64 [n], coef fp32 [n, 2]) on the host, computed in fp64 and then rounded: step i is ``x <- coef[i, 0] x + coef[i, 1] v``."""
    ts, coef = cog_ddim_coefficients_f64(num_inference_steps, scheduler_config)
    return ts, coef.to(torch.float32)


def cog_guidance_table(num_inference_steps: int, timesteps: List[int], guidance_scale: float, use_dynamic_cfg: bool = False) -> List[float]:
    """The guidance scale of every step.  [upstream, unpinned] ``CogVideoXPipeline`` with ``use_dynamic_cfg``:
    ``g_i = 1 + g (1 - cos(pi ((n - t_i) / n) ** 5.0)) / 2`` with ``t_i`` the timestep VALUE (up to 999) and ``n`` the number of inference steps -- kept as
    upstream has it, odd as that is.  Without it: ``g`` at every step."""
    import math

    n, g = int(num_inference_steps), float(guidance_scale)
    if not use_dynamic_cfg:
        return [g] * len(timesteps)
    if g == 1.0:
        raise ValueError("use_dynamic_cfg changes the guidance scale per step; guidance_scale = 1 runs no unconditional rows to guide against")
    return [1.0 + g * ((1.0 - math.cos(math.pi * ((n - t) / n) ** 5.0)) / 2.0) for t in timesteps]


def cog_dpm_coefficients_f64(num_inference_steps: int, scheduler_config: Optional[Dict[str, Any]] = None, guidance_scale: float = 6.0,
                             use_dynamic_cfg: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (timesteps int64 [n], rows fp64 [n, 8]).  [upstream, unpinned] ``CogVideoXDPMScheduler.step`` as of diffusers 0.33, restated from memory (diffusers is
    not vendored here), for v-prediction.  Timesteps and ``prev_i`` are ``cog_ddim_schedule``'s; ``ab_back = alphas_cumprod[t_{i-1}]``.  One upstream step, with
    ``old`` the previous step's x0 and ``z`` fresh noise::

        x0    = sqrt(ab_t) x - sqrt(1 - ab_t) v
        lam   = log sqrt(ab_t / (1 - ab_t));  lam_next = the same of ab_prev;  h = lam_next - lam
        mult0 = sqrt((1 - ab_prev) / (1 - ab_t)) exp(-h);  mult1 = expm1(-2 h) sqrt(ab_prev);  mn = sqrt(1 - ab_prev) sqrt(1 - exp(-2 h))
        first step or prev_i < 0:   x' = mult0 x - mult1 x0 + mn z
        otherwise:                  r = (lam - lam_back) / h;  D = (1 + 1 / (2 r)) x0 - old / (2 r);  x' = mult0 x - mult1 D + mn z

    folded into the row ``(sa, sb, m0, e0, e1, mn, g, 0)``: ``x0 = sa x - sb v;  x' = m0 x + e0 x0 + e1 old + mn z`` with ``e0 = -mult1 (1 + 1 / (2 r))``,
    ``e1 = mult1 / (2 r)`` (single-step rows: ``-mult1``, 0); ``g`` is the step's guidance scale (``cog_guidance_table``).  The infinities of a zero terminal
    SNR (``ab_t = 0``: h = inf at step 0, r = inf at step 1) and of the last step (``ab_prev = 1``) come out as finite rows through the limits of exp / expm1;
    a row that is still not finite is a ValueError.  Only a ``CogVideoXDPMScheduler`` config is folded here; DDIM has ``cog_ddim_tables``."""
    cfg = dict(COG_DPM_SCHEDULER_CONFIG if scheduler_config is None else scheduler_config)
    if not is_dpm(cfg):
        raise NotImplementedError(f"cog_dpm_tables: {cfg.get('_class_name', 'CogVideoXDDIMScheduler')} is not the multistep solver: cog_ddim_tables restates it")
    ts, prev, a_t, a_prev = _schedule(num_inference_steps, cfg, multistep=True)
    gs = cog_guidance_table(len(ts), ts, guidance_scale, use_dynamic_cfg)
    n = len(ts)
    rows = torch.zeros(n, 8, dtype=torch.float64)
    rows[:, 0], rows[:, 1], rows[:, 6] = a_t.sqrt(), (1 - a_t).sqrt(), torch.tensor(gs, dtype=torch.float64)
    lam, lam_next = (a_t / (1 - a_t)).sqrt().log(), (a_prev / (1 - a_prev)).sqrt().log()
    h = lam_next - lam
    mult0 = ((1 - a_prev) / (1 - a_t)).sqrt() * torch.exp(-h)
    mult1 = torch.expm1(-2 * h) * a_prev.sqrt()
    rows[:, 2], rows[:, 3], rows[:, 5] = mult0, -mult1, (1 - a_prev).sqrt() * (1 - torch.exp(-2 * h)).sqrt()
    for i in range(1, n):
        if prev[i] >= 0:  # a multistep row: lam_back is the previous step's lam
            inv2r = 1.0 / (2.0 * ((lam[i] - lam[i - 1]) / h[i]))
            rows[i, 3], rows[i, 4] = -mult1[i] * (1.0 + inv2r), mult1[i] * inv2r
    if not bool(torch.isfinite(rows).all()):
        raise ValueError("cog_dpm_tables: the scheduler configuration gives a non-finite step")
    return torch.tensor(ts, dtype=torch.int64), rows


def cog_dpm_tables(num_inference_steps: int, scheduler_config: Optional[Dict[str, Any]] = None, guidance_scale: float = 6.0,
                   use_dynamic_cfg: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (timesteps int64 [n], rows fp32 [n, 8]) on the host, computed in fp64 and rounded once: ``ftmi_cog_sample_step_dpm``'s ``coef_row`` of step i."""
    ts, rows = cog_dpm_coefficients_f64(num_inference_steps, scheduler_config, guidance_scale, use_dynamic_cfg)
    return ts, rows.to(torch.float32)


def cog_dpm_step_noise(shape, n: int, prev: List[int], generator: Optional[torch.Generator], device, dtype: torch.dtype = bf16) -> torch.Tensor:
    """-> fp32 [n, *shape]: the noise of every step, drawn in the pipeline's order so that one generator state gives the pipeline's sequence.
    [upstream, unpinned] ``CogVideoXDPMScheduler.step`` draws ``randn(shape)`` once per step -- the last step included, whose row usually has ``mn = 0`` and
    leaves the draw unused -- and on a multistep row (``i > 0`` and ``prev[i] >= 0``) draws a SECOND time and uses the second draw.  Slice i is the draw
    step i uses.  A generator draws on its own device (a CPU generator: on the host, then moved), as the pipeline's ``randn_tensor`` does."""
    shape = tuple(int(s) for s in shape)
    where = generator.device if generator is not None else torch.device(device)
    out = torch.empty((int(n),) + shape, dtype=torch.float32, device=device)
    for i in range(int(n)):
        z = torch.randn(shape, generator=generator, device=where, dtype=dtype)
        if i > 0 and prev[i] >= 0:
            z = torch.randn(shape, generator=generator, device=where, dtype=dtype)
        out[i] = z.to(device=device, dtype=torch.float32)
    return out


class StepNoiseRequired(ValueError, NotImplementedError):
    """``sample`` with ``CogVideoXDPMScheduler`` and neither ``generator`` nor ``step_noise``.  A ValueError, because arguments are missing; also the
    NotImplementedError this call has always been: drawing the noise of the steps without the caller's generator (on the device, say) is not implemented."""


class MI355XCogVideoXLatentSampler:
    """Denoising loop over a ``MI355XCogVideoXTransformer3DModel`` (``ftmi_cog_sample``; ``ftmi_cog_sample_ms`` for the multistep scheduler).  The adapters are
    read at every ``sample``: a sample taken between two optimiser steps sees them as they are."""

    def __init__(self, transformer: MI355XCogVideoXTransformer3DModel, scheduler_config: Optional[Dict[str, Any]] = None):
        self.transformer = transformer
        self.scheduler_config = dict(COG_SCHEDULER_CONFIG if scheduler_config is None else scheduler_config)

    # -- every refusal, with its reason --------------------------------------------------------------------------------------------------------------
    def check_inputs(self, latents, prompt_embeds, negative_prompt_embeds, guidance_scale: float, drop_frames: int, use_dynamic_cfg: bool) -> None:
        tr = self.transformer
        c = tr.config
        if use_dynamic_cfg and not is_dpm(self.scheduler_config):
            raise NotImplementedError("sample: use_dynamic_cfg (a guidance scale that changes per step) travels in the rows of the multistep loop; with "
                                      "CogVideoXDDIMScheduler, whose loop takes one scale per call, it is not restated here")
        if use_dynamic_cfg and float(guidance_scale) == 1.0:
            raise ValueError("sample: use_dynamic_cfg changes the guidance scale per step; guidance_scale = 1 runs no unconditional rows to guide against")
        if c.ofs_embed_dim is not None or c.in_channels != c.out_channels:
            raise NotImplementedError("sample: text-to-video only -- this model has an ofs embedding or in_channels != out_channels (an image-to-video checkpoint)")
        if c.patch_size_t is not None and not c.use_rotary_positional_embeddings:
            raise ValueError("sample: CogVideoX 1.5 checkpoints use rotary position embeddings")
        if prompt_embeds.dim() != 3 or prompt_embeds.shape[-1] != c.text_embed_dim:
            raise ValueError(f"sample: prompt_embeds must be [B, T, {c.text_embed_dim}], got {tuple(prompt_embeds.shape)}")
        if prompt_embeds.shape[1] != c.max_text_seq_length:
            raise ValueError(f"sample: CogVideoX expects {c.max_text_seq_length} text tokens (max_text_seq_length), got {prompt_embeds.shape[1]}")
        if float(guidance_scale) != 1.0:
            if negative_prompt_embeds is None:
                raise ValueError("sample: guidance_scale != 1 needs negative_prompt_embeds")
            if tuple(negative_prompt_embeds.shape) != tuple(prompt_embeds.shape):
                raise ValueError("sample: negative_prompt_embeds must be shaped like prompt_embeds")
        B, p, pt = prompt_embeds.shape[0], c.patch_size, c.patch_size_t or 1
        if latents.dim() != 5 or latents.shape[0] != B or latents.shape[2] != c.in_channels:
            raise ValueError(f"sample: latents must be [{B}, F, {c.in_channels}, H, W] (the initial noise), got {list(latents.shape)}")
        if latents.shape[1] % pt:
            raise ValueError(f"sample: the latent frame count {latents.shape[1]} must be a multiple of patch_size_t = {pt} (the pipeline pads it at the front: "
                             "drop_frames)")
        if latents.shape[3] % p or latents.shape[4] % p:
            raise ValueError(f"sample: the latent height and width must be multiples of patch_size = {p}, got {latents.shape[3]} x {latents.shape[4]}")
        if not 0 <= int(drop_frames) < pt:
            raise ValueError(f"sample: drop_frames counts the frames padded at the front, 0 <= drop_frames < patch_size_t = {pt}")
        if tr.proj_out_w_t is None or not tr._stack:
            raise RuntimeError("sample: load_diffusers_state_dict first")

    # -- the state-independent inputs of the loop ----------------------------------------------------------------------------------------------------
    def step_tables(self, timesteps: torch.Tensor, rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (temb_silu bf16 [n, rows, D_temb], head shift bf16 [n, D], head 1 + scale bf16 [n, D]).  Every step runs the time embedding's and norm_out's
        launches at ``rows`` = P B equal timesteps, as the model's ``_embed`` does, and keeps one row of the head's: the rounding points are ``_embed``'s."""
        tr = self.transformer
        D, silu = tr.config.inner_dim, torch.nn.functional.silu
        tembs, shifts, oneps = [], [], []
        for t in timesteps.tolist():
            ts = torch.full((rows,), t, dtype=torch.int64, device=tr.device)
            t_emb = timestep_embedding(ts, D).to(bf16)
            emb = ops.gemm_nt(silu(ops.gemm_nt(t_emb, tr.time1_w, tr.time1_b)), tr.time2_w, tr.time2_b)
            mod = ops.gemm_nt(silu(emb), tr.norm_out_lin_w, tr.norm_out_lin_b)
            tembs.append(silu(emb.to(bf16)))
            shifts.append(mod[0, :D])
            oneps.append((1 + mod[:, D:])[0])
        return torch.stack(tembs).contiguous(), torch.stack(shifts).contiguous(), torch.stack(oneps).contiguous()

    def geometry(self, B: int, frames: int, height: int, width: int, guidance: bool, drop_frames: int = 0) -> "_lib.CogSampleGeometry":
        c = self.transformer.config
        return ops.cog_sample_geometry(B, c.out_channels, frames, height, width, patch=c.patch_size, patch_t=c.patch_size_t, guidance=guidance, drop=drop_frames)

    def c_arguments(self, geo, steps: int, guidance_scale: float):
        """-> (ftmi_cog_sample_config, ftmi_cog_sample_weights, the objects the two structures point into).  The adapters' working copies are refreshed here."""
        tr = self.transformer
        c = tr.config
        T = c.max_text_seq_length
        S = (geo.F // geo.pt) * (geo.H // geo.p) * (geo.W // geo.p)
        rope = None
        if c.use_rotary_positional_embeddings:
            rope = tuple(t.to(device=tr.device, dtype=torch.float32).contiguous() for t in rotary_tables(c, geo.H, geo.W, geo.F))
        pos = None if rope is not None else tr._pos_table(geo.F, geo.H, geo.W)
        bc = tr._c_config(geo.P * geo.B, T + S)
        cfg = _lib.CogSampleConfig(geo=geo, T=T, D_text=c.text_embed_dim, D=bc.D, heads=bc.H, L=bc.L, D_ff=bc.D_ff, D_temb=bc.D_temb, r=bc.r,
                                   lora_scale=bc.lora_scale, eps_norm=bc.eps_norm, eps_qk=bc.eps_qk, gemm_variant=bc.gemm_variant, steps=steps,
                                   guidance=float(guidance_scale))
        w = _lib.CogSampleWeights()
        w.blocks = tr._c_weights(rope)
        for field, name in (("patch_w", "patch_w"), ("patch_b", "patch_b"), ("text_w", "text_w"), ("text_b", "text_b"), ("norm_final_w", "norm_final_w"),
                            ("norm_final_b", "norm_final_b"), ("norm_out_w", "norm_out_w"), ("norm_out_b", "norm_out_b"), ("proj_w", "proj_out_w"),
                            ("proj_b", "proj_out_b"), ("ones", "_ones_row"), ("zeros", "_zeros_row")):
            setattr(w, field, getattr(tr, name).data_ptr())
        w.pos = None if pos is None else pos.data_ptr()
        return cfg, w, [rope, pos]

    @torch.no_grad()
    def sample(self, latents: torch.Tensor, prompt_embeds: torch.Tensor, negative_prompt_embeds: Optional[torch.Tensor] = None, num_inference_steps: int = 50,
               guidance_scale: float = 6.0, drop_frames: int = 0, scaling_factor: float = 1.15258426, invert_scale_latents: bool = False,
               use_dynamic_cfg: bool = False, generator: Optional[torch.Generator] = None, step_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> denormalised latents bf16 [B, F - drop_frames, C, H, W] (the VAE decoder's input): ``latents / scaling_factor``, or ``latents * scaling_factor``
        for the ``invert_scale_latents`` checkpoints.

        ``latents`` [B, F, C, H, W] is the initial noise (``init_noise_sigma`` = 1), drawn by the caller -- ``randn`` of that shape in the pipeline's order, so
        one seed gives the same noise.  For CogVideoX 1.5 ``F`` includes the frames the pipeline pads at the FRONT to reach a multiple of ``patch_size_t``;
        ``drop_frames`` of them are discarded after the loop, as the pipeline does.  ``prompt_embeds`` / ``negative_prompt_embeds`` [B, max_text_seq_length,
        text_embed_dim]; ``guidance_scale`` = 1 runs the conditional rows only.

        A ``CogVideoXDPMScheduler`` config (the 5b and 1.5 checkpoints') runs the multistep loop, which adds fresh noise at every step but the last:
        ``step_noise`` [n, B, F, C, H, W] is used as given (slice i at step i); otherwise ``cog_dpm_step_noise`` draws it from ``generator`` on the transformer's
        device, AFTER the caller drew ``latents`` from the same generator -- the pipeline's order.  The step noise is held in the state's layout for the whole
        call, because the call does not return to the host: ``4 n B S Kc`` bytes, about 23 MB per step and 1.1 GB for 50 steps at 81 x 768 x 1360.
        With neither, ``StepNoiseRequired`` (a ValueError).  ``use_dynamic_cfg`` (a guidance scale per step, ``cog_guidance_table``) runs with that scheduler,
        whose rows carry the scale; with DDIM, whose loop takes one scale per call, it stays refused.  DDIM is ``ftmi_cog_sample`` and keeps its bits."""
        tr = self.transformer
        dev = tr.device
        g = float(guidance_scale)
        dpm = is_dpm(self.scheduler_config)
        if dpm and generator is None and step_noise is None:
            raise StepNoiseRequired("sample: CogVideoXDPMScheduler adds noise at every step: pass generator (drawn from in the pipeline's order) or step_noise")
        self.check_inputs(latents, prompt_embeds, negative_prompt_embeds, g, drop_frames, use_dynamic_cfg)
        B, F_, _, H, W = latents.shape
        geo = self.geometry(B, F_, H, W, guidance=g != 1.0, drop_frames=int(drop_frames))
        text = prompt_embeds if g == 1.0 else torch.cat([negative_prompt_embeds.to(prompt_embeds.device), prompt_embeds], dim=0)
        text = text.to(dev, bf16).contiguous()
        if not dpm:
            ts, coef = cog_ddim_tables(num_inference_steps, self.scheduler_config)
            temb_silu, shift, onep = self.step_tables(ts, geo.P * B)
            cfg, weights, keep = self.c_arguments(geo, ts.numel(), g)
            x, cols = ops.cog_sample_init(geo, latents.to(dev, torch.float32).contiguous())
            ops.cog_sample(cfg, weights, cols, x, text, temb_silu, shift, onep, coef.to(dev))
        else:
            ts, rows = cog_dpm_tables(num_inference_steps, self.scheduler_config, g, use_dynamic_cfg)
            n = ts.numel()
            k = max([i + 1 for i in range(n) if float(rows[i, 5]) != 0.0], default=0)  # the leading steps whose row has noise
            noise = None
            if k > 0:
                if step_noise is None:
                    _, prev, _, _ = _schedule(n, self.scheduler_config, multistep=True)
                    step_noise = cog_dpm_step_noise((B, F_, latents.shape[2], H, W), n, prev, generator, dev)
                if tuple(step_noise.shape) != (n,) + tuple(latents.shape):
                    raise ValueError(f"sample: step_noise must be [{n}, {', '.join(str(s) for s in latents.shape)}], got {list(step_noise.shape)}")
                noise = ops.cog_sample_pack(geo, step_noise[:k].to(dev, torch.float32).contiguous())
            temb_silu, shift, onep = self.step_tables(ts, geo.P * B)
            cfg, weights, keep = self.c_arguments(geo, n, g)
            x, cols = ops.cog_sample_init(geo, latents.to(dev, torch.float32).contiguous())
            ops.cog_sample_ms(cfg, weights, cols, x, text, temb_silu, shift, onep, rows.to(dev).contiguous(), noise)
        del keep
        k = float(scaling_factor) if invert_scale_latents else 1.0 / float(scaling_factor)
        return ops.cog_sample_finish(geo, x, k)
