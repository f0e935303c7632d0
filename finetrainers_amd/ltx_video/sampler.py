"""Validation sampling in latent space for the MI355X LTX-Video backend.

The reference validates by building an ``LTXPipeline`` and running its denoising loop per prompt (finetrainers/models/ltx_video/
base_specification.py:347-377).  Here the loop -- DiT forward on the conditional + unconditional prompt, classifier-free-guidance combine, flow-match Euler
update -- is ONE C call (``ftmi_ltx_ff_sample``, no host synchronisation) over the transformer that is being trained, with its current LoRA state.  A
validation row with an image runs the image-to-video pipeline there (:360-361); here that is ``image_latents``: the first latent frames held, timestep 0
on them (``ftmi_ltx_ff_sample_cond``).  Text encoding, VAE encoding of the image and VAE decoding stay outside: the sampler takes prompt embeddings and returns denormalised latents (INTEGRATION.md shows the hand-over to the
reference pipeline's VAE decode).
"""

from __future__ import annotations

import math
from typing import Any, Dict, Optional, Sequence, Tuple

import torch

from .. import ops
from .transformer import MI355XLTXVideoTransformer3DModel, bf16

# [upstream, unpinned] scheduler/scheduler_config.json of Lightricks/LTX-Video (FlowMatchEulerDiscreteScheduler): the file specification.py's
# ``_save_lora_weights`` writes a subset of.  Only a default for callers that have no scheduler config at hand; ``flow_match_sigmas`` itself reads every
# constant from the dict it is given.
LTX_SCHEDULER_CONFIG: Dict[str, Any] = {
    "num_train_timesteps": 1000,
    "shift": 1.0,
    "use_dynamic_shifting": True,
    "base_shift": 0.95,
    "max_shift": 2.05,
    "base_image_seq_len": 1024,
    "max_image_seq_len": 4096,
    "shift_terminal": 0.1,
}


def _need(config: Dict[str, Any], key: str):
    if key not in config or config[key] is None:
        raise ValueError(f"flow_match_sigmas: the scheduler config enables dynamic shifting but has no {key!r}")
    return config[key]


def flow_match_sigmas(num_inference_steps: int, seq_len: int, scheduler_config: Dict[str, Any]) -> torch.Tensor:
    """Sigma table of a sampling run: fp32 [num_inference_steps + 1], decreasing, ending in 0.

    [upstream, unpinned] restates ``LTXPipeline.__call__`` (``sigmas = linspace(1, 1 / n, n)``, ``mu = calculate_shift(video_sequence_length, ...)``) +
    ``FlowMatchEulerDiscreteScheduler.set_timesteps(sigmas=..., mu=...)``: with ``use_dynamic_shifting`` the table is time-shifted by
    ``exp(mu) / (exp(mu) + (1 / sigma - 1))`` where ``mu`` is linear in the token count between (base_image_seq_len, base_shift) and
    (max_image_seq_len, max_shift); otherwise by the static ``shift`` (1.0: the linear table itself); ``shift_terminal`` stretches the table so that its
    last non-zero entry is that value.  Every constant comes from ``scheduler_config``.  ``seq_len``: video tokens per sample."""
    n = int(num_inference_steps)
    if n < 1:
        raise ValueError("flow_match_sigmas: at least one step")
    s = torch.linspace(1.0, 1.0 / n, n, dtype=torch.float64)
    if scheduler_config.get("use_dynamic_shifting", False):
        x0, x1 = float(_need(scheduler_config, "base_image_seq_len")), float(_need(scheduler_config, "max_image_seq_len"))
        y0, y1 = float(_need(scheduler_config, "base_shift")), float(_need(scheduler_config, "max_shift"))
        m = (y1 - y0) / (x1 - x0)
        mu = float(seq_len) * m + (y0 - m * x0)
        s = math.exp(mu) / (math.exp(mu) + (1.0 / s - 1.0))
    else:
        shift = float(scheduler_config.get("shift", 1.0))
        if shift != 1.0:
            s = shift * s / (1.0 + (shift - 1.0) * s)
    terminal = scheduler_config.get("shift_terminal", None)
    if terminal and s[-1] < 1.0:  # (a single step starts at sigma = 1: nothing to stretch)
        one_minus = 1.0 - s
        s = 1.0 - one_minus / (one_minus[-1] / (1.0 - float(terminal)))
    return torch.cat([s, s.new_zeros(1)]).to(torch.float32)


def latent_grid(num_frames: int, height: int, width: int, temporal_compression: int = 8, spatial_compression: int = 32) -> Tuple[int, int, int]:
    """Latent (frames, height, width) of a pixel-space clip under the LTX VAE's compression (49 x 512 x 768 -> 7 x 16 x 24 = 2 688 tokens)."""
    return (num_frames - 1) // temporal_compression + 1, height // spatial_compression, width // spatial_compression


class MI355XLTXLatentSampler:
    """Denoising loop over a ``MI355XLTXVideoTransformer3DModel`` (``ftmi_ltx_ff_sample`` / ``ftmi_ltx_ff_sample_cond``)."""

    def __init__(self, transformer: MI355XLTXVideoTransformer3DModel, scheduler_config: Optional[Dict[str, Any]] = None, frame_rate: int = 25):
        if getattr(transformer, "_narrow", None) is not None:
            raise NotImplementedError("MI355XLTXLatentSampler: narrow (zero-padded) geometries (ltx_video/narrow.py) are not supported; sample with the "
                                      "production geometry")
        self.transformer = transformer
        self.scheduler_config = dict(LTX_SCHEDULER_CONFIG if scheduler_config is None else scheduler_config)
        self.frame_rate = frame_rate

    @staticmethod
    def _key_bias(mask: Optional[torch.Tensor], B: int, T: int, dev) -> Optional[torch.Tensor]:
        if mask is None:
            return None
        # patch.py:55-57, as MI355XLTXVideoTransformer3DModel.forward builds it
        return ((1 - mask.to(device=dev).reshape(B, T).to(bf16)) * -10000.0).float().contiguous()

    @staticmethod
    def _cond_frames(image_latents: Optional[torch.Tensor], cond_frames: Optional[int], B: int, C: int, num_frames: int, height: int, width: int) -> int:
        """The number of held latent frames, after checking ``image_latents`` [B, C, k, H, W] against the grid."""
        k_img = 0
        if image_latents is not None:
            if image_latents.ndim != 5 or tuple(image_latents.shape[:2]) != (B, C) or tuple(image_latents.shape[3:]) != (height, width):
                raise ValueError(f"sample: image_latents must be [{B}, {C}, k, {height}, {width}], got {tuple(image_latents.shape)}")
            k_img = image_latents.shape[2]
            if not 1 <= k_img <= num_frames:
                raise ValueError(f"sample: image_latents hold {k_img} frames, the clip has {num_frames}")
        k = k_img if cond_frames is None else int(cond_frames)
        if not 0 <= k <= num_frames:
            raise ValueError(f"sample: cond_frames {k} outside [0, {num_frames}]")
        if image_latents is not None and k != k_img:
            raise ValueError(f"sample: cond_frames {k} != the {k_img} frames of image_latents")
        return k

    @staticmethod
    def initial_state(B: int, C: int, num_frames: int, height: int, width: int, device, generator: Optional[torch.Generator] = None,
                      latents: Optional[torch.Tensor] = None, image_latents: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The sampler state at step 0, packed fp32 [B, S, C]: ``latents`` or ``randn([B, C, F, H, W], generator)`` -- drawn for the whole shape, whatever is
        held, so one seed gives one noise tensor -- with ``image_latents`` [B, C, k, H, W] written over latent frames [0, k)."""
        if latents is None:
            latents = torch.randn((B, C, num_frames, height, width), generator=generator, device=device, dtype=torch.float32)
        elif tuple(latents.shape) != (B, C, num_frames, height, width):
            raise ValueError(f"sample: latents must be [{B}, {C}, {num_frames}, {height}, {width}]")
        latents = latents.to(device=device, dtype=torch.float32)
        if image_latents is not None:
            MI355XLTXLatentSampler._cond_frames(image_latents, None, B, C, num_frames, height, width)
            latents = latents.clone()
            latents[:, :, :image_latents.shape[2]] = image_latents.to(device=device, dtype=torch.float32)
        return latents.flatten(2).transpose(1, 2).contiguous()  # pack: [B, S, C]

    @torch.no_grad()
    def sample(self, prompt_embeds: torch.Tensor, prompt_attention_mask: Optional[torch.Tensor], negative_prompt_embeds: Optional[torch.Tensor],
               negative_prompt_attention_mask: Optional[torch.Tensor], num_frames: int, height: int, width: int, num_inference_steps: int = 50,
               guidance_scale: float = 3.0, sigmas: Optional[Sequence[float]] = None, timesteps: Optional[Sequence[float]] = None,
               generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None, latents_mean: Optional[torch.Tensor] = None,
               latents_std: Optional[torch.Tensor] = None, image_latents: Optional[torch.Tensor] = None,
               cond_frames: Optional[int] = None) -> torch.Tensor:
        """-> denormalised latents [B, C, F, H, W] bf16 (the VAE decoder's input).

        ``num_frames`` / ``height`` / ``width`` are the LATENT grid, as for the transformer's forward (``latent_grid`` converts a pixel-space clip).
        ``sigmas`` [n + 1] / ``timesteps`` [n] override the schedule (default: ``flow_match_sigmas`` and ``sigma * num_train_timesteps``, the value the
        pipeline feeds the model).  The initial noise is ``torch.randn([B, C, F, H, W], generator=generator)`` in fp32 on the transformer's device, then
        packed -- the order a pipeline draws it in, so one seed gives the same noise -- or ``latents`` in that layout.  ``latents_mean`` / ``latents_std``
        ([C], the VAE's statistics) denormalise the result; without them it stays normalised (mean 0, std 1).

        Image-to-video ([upstream, unpinned] restates ``LTXImageToVideoPipeline.prepare_latents`` / ``__call__``): ``image_latents`` [B, C, k, H, W] are the
        NORMALISED latents of the conditioning frames -- the VAE encoding of the image after ``_normalize_latents`` (base_specification.py:427-436), not the
        raw encoder output; ``latents_mean`` / ``latents_std`` are used for the final denormalisation only.  They occupy latent frames [0, k) of the initial
        state and are held: the model sees timestep 0 on them, the guidance combine and the Euler update skip them, and they come back in the result,
        denormalised like the rest (``ftmi_ltx_ff_sample_cond``).  The noise is drawn for the whole [B, C, F, H, W] shape first and the held frames are then
        overwritten, so one seed gives the noise the pipeline draws; upstream repeats the one encoded frame over all frames and blends by its mask, which for
        k = 1 is this state.  ``cond_frames`` (default: the k of ``image_latents``; 0 without them) holds the first frames of ``latents`` when the caller
        supplies the whole initial state itself."""
        tr = self.transformer
        dev = tr.device
        c = tr.config
        B, T = prompt_embeds.shape[0], prompt_embeds.shape[1]
        C, S = c.in_channels, num_frames * height * width
        g = float(guidance_scale)
        two_pass = g != 1.0
        if two_pass and negative_prompt_embeds is None:
            raise ValueError("sample: guidance_scale != 1 needs negative_prompt_embeds")
        if two_pass and (prompt_attention_mask is None) != (negative_prompt_attention_mask is None):
            raise ValueError("sample: give the attention mask of both prompts or of neither")
        text_c = prompt_embeds.to(device=dev, dtype=bf16).contiguous()
        kb_c = self._key_bias(prompt_attention_mask, B, T, dev)
        text_u = kb_u = None
        if two_pass:
            if tuple(negative_prompt_embeds.shape) != tuple(prompt_embeds.shape):
                raise ValueError("sample: negative_prompt_embeds must be shaped like prompt_embeds (pad both prompts to one length)")
            text_u = negative_prompt_embeds.to(device=dev, dtype=bf16).contiguous()
            kb_u = self._key_bias(negative_prompt_attention_mask, B, T, dev)

        if sigmas is None:
            sig = flow_match_sigmas(num_inference_steps, S, self.scheduler_config)
        else:
            sig = torch.as_tensor(sigmas, dtype=torch.float32).reshape(-1).cpu()
        n = sig.numel() - 1
        if n < 1:
            raise ValueError("sample: sigmas must hold n + 1 values")
        if timesteps is None:
            ts = sig[:-1] * float(self.scheduler_config["num_train_timesteps"])
        else:
            ts = torch.as_tensor(timesteps, dtype=torch.float32).reshape(-1).cpu()
        if ts.numel() != n:
            raise ValueError("sample: timesteps must hold one value per step")

        k = self._cond_frames(image_latents, cond_frames, B, C, num_frames, height, width)
        x = self.initial_state(B, C, num_frames, height, width, dev, generator=generator, latents=latents, image_latents=image_latents)

        # specification.py forward / base_specification.py:324-334
        temporal_compression_ratio, vae_spatial_compression_ratio = 8, 32
        rope_interpolation_scale = [1 / (self.frame_rate / temporal_compression_ratio), vae_spatial_compression_ratio, vae_spatial_compression_ratio]
        cos, sin = tr.rope_tables(num_frames, height, width, rope_interpolation_scale)
        tr.refresh_lora_copies()  # mid-training validation sees the adapters as they are now
        cfg = tr._c_config(B, S, T)
        weights = tr._c_weights(cos, sin)
        conditioned = image_latents is not None or cond_frames is not None
        ws_bytes = (ops.ltx_sample_cond_workspace_bytes(cfg, two_pass, num_frames, weights) if conditioned
                    else ops.ltx_sample_workspace_bytes(cfg, two_pass, weights))
        ws = tr._acquire_workspace(ws_bytes, dev)
        try:
            if conditioned:
                ops.ltx_sample_cond(cfg, weights, text_c, text_u, kb_c, kb_u, x, sig.to(dev), ts.to(dev), g, num_frames, k, workspace=ws)
            else:
                ops.ltx_sample(cfg, weights, text_c, text_u, kb_c, kb_u, x, sig.to(dev), ts.to(dev), g, workspace=ws)
        finally:
            tr._release_workspace(ws)
        mean = torch.zeros(C, dtype=torch.float32, device=dev) if latents_mean is None else latents_mean.reshape(-1)[:C].to(device=dev, dtype=torch.float32)
        std = torch.ones(C, dtype=torch.float32, device=dev) if latents_std is None else latents_std.reshape(-1)[:C].to(device=dev, dtype=torch.float32)
        return ops.ltx_unpack_denorm(x, mean, std, num_frames, height, width)
