"""``WanControlModelSpecification`` (finetrainers/models/wan/control_specification.py) for ``--training_type control-lora`` on the MI355X: the patch embedding
takes 2 x 16 channels -- the noisy latents, then the control latents -- and carries a full-rank LoRA adapter next to the blocks' adapters
(trainer/control_trainer/trainer.py:130-144).

The input construction (control_specification.py:243-308): both sets of stored moments are normalised and the posterior's MODE is taken (the normalised
mean: no draw), the latents are mixed with noise by the flow-match rule, frame conditioning is applied to the control latents (finetrainers_amd/control.py),
and the two are concatenated on the channels.  On the fast path ONE kernel (``ops.wan_control_pack``) goes from the batch to the patch embedding's GEMM
operand and the target; the torch path builds the 32-channel ``hidden_states`` with the same rounding points and is what a foreign callable gets.

Refused, each with its reason: ``frame_conditioning_concatenate_mask`` (the reference builds a 2C-channel layer but its mask adds C more channels -- the
one-channel slice in ``apply_frame_conditioning_on_latents`` is computed and never applied -- so that path cannot run there either), ``--train_qk_norm``,
``control-full-finetune`` and control on an image-to-video model."""

from __future__ import annotations

import dataclasses
import os
from typing import Dict, List, Optional

import torch

from .. import ops
from ..control import apply_frame_conditioning_on_latents, frame_keep_mask
from ..utils.reference_base import as_drop_in, keep_or_default
from .specification import MI355XWanModelSpecification, MI355XWanSpecOps

bf16 = torch.bfloat16

_MASK_REASON = ("frame_conditioning_concatenate_mask is not covered: the reference widens the patch embedding to 2C channels, but the mask its frame conditioning "
                "concatenates has C channels, not one (the one-channel slice is computed and never applied), so that path cannot run in the reference either")


class MI355XWanControlSpecOps(MI355XWanSpecOps):
    """The arithmetic of the control specification's ``forward`` around the DiT call, on tensors."""

    frame_conditioning_type = "full"
    frame_conditioning_index: Optional[int] = 0
    frame_conditioning_concatenate_mask = False

    def control_hidden_states(self, moments, control_latents, latents_mean, latents_std, sigmas, noise, keep):
        """The torch path -> (hidden_states [B, 2C, F, H, W], target): the eager graph of control_specification.py:265-306 with ``keep`` [B, F] deciding the
        control frames (a dropped frame is multiplied by zero, frames past the control clip are zero padding)."""
        B, _, F_ = moments.shape[:3]
        z = self.normalize_latents(torch.chunk(moments, 2, dim=1)[0], latents_mean, latents_std)
        s = sigmas.view(B, 1, 1, 1, 1).to(z.device)
        noisy = ((1.0 - s) * z + s * noise).to(z)
        ctrl = self.normalize_latents(torch.chunk(control_latents, 2, dim=1)[0], latents_mean, latents_std)
        n = min(ctrl.shape[2], F_)
        ctrl = ctrl[:, :, :n] * keep[:, :n].to(ctrl).view(B, 1, n, 1, 1)
        if n < F_:
            ctrl = torch.cat([ctrl, ctrl.new_zeros((B, ctrl.shape[1], F_ - n) + tuple(ctrl.shape[3:]))], dim=2)
        return torch.cat([noisy, ctrl], dim=1), noise - z

    def forward(self, transformer, moments, encoder_hidden_states, sigmas, latents_mean, latents_std, posterior_noise=None, noise=None, generator=None,
                control_latents=None, use_pack_kernel: Optional[bool] = None, keep=None, **unused):
        """-> (pred, target, sigmas).  ``keep`` [F] or [B, F] (tests): the control frames to keep, instead of the draw of ``frame_conditioning_type``.
        ``use_pack_kernel``: None = the kernel whenever ``transformer`` is this backend's model with adapters attached."""
        if self.frame_conditioning_concatenate_mask:
            raise NotImplementedError(_MASK_REASON)
        if control_latents is None:
            raise ValueError("the control specification needs control_latents (the control clip's stored moments [B, 2C, Fc, H, W])")
        if unused.get("latent_condition") is not None or unused.get("encoder_hidden_states_image") is not None:
            raise NotImplementedError("control on an image-to-video model is not covered")
        moments, control_latents = moments.to(bf16), control_latents.to(moments.device, bf16)
        B, C2, F_, H, W = moments.shape
        if control_latents.shape[:2] != (B, C2) or tuple(control_latents.shape[3:]) != (H, W):
            raise ValueError(f"control_latents {tuple(control_latents.shape)} do not go with latents {tuple(moments.shape)}")
        dev = moments.device
        if noise is None:
            noise = torch.zeros((B, C2 // 2, F_, H, W), dtype=bf16, device=dev).normal_(generator=generator)
        noise = noise.to(dev, bf16)
        if keep is None:  # ONE draw for the batch: the reference masks the whole batch tensor with the same frames
            keep = frame_keep_mask(control_latents.shape[2], F_, self.frame_conditioning_type, self.frame_conditioning_index)
        keep = torch.as_tensor(keep, dtype=torch.uint8).to(dev)
        keep = (keep.view(1, F_).expand(B, F_) if keep.dim() == 1 else keep).contiguous()
        sig = sigmas.flatten().to(dev, torch.float32)
        timesteps = (sigmas.flatten() * 1000.0).long()
        fast = getattr(transformer, "lora_config", None) is not None and hasattr(transformer, "expand_patch_embedding")
        if use_pack_kernel is None:
            use_pack_kernel = fast
        if use_pack_kernel:
            if not fast:
                raise ValueError("the pack kernel's output goes to this backend's model with adapters attached")
            mean, std = (t.to(dev, torch.float32).reshape(-1).contiguous() for t in (latents_mean, latents_std))
            cols2, target = ops.wan_control_pack(moments, control_latents, noise, sig, mean, std, keep, tuple(transformer.config.patch_size))
            pred = transformer(hidden_states=None, patch_columns=cols2, latent_shape=(B, F_, H, W), timestep=timesteps, encoder_hidden_states=encoder_hidden_states,
                               return_dict=False)[0]
        else:
            hidden, target = self.control_hidden_states(moments, control_latents, latents_mean, latents_std, sig, noise, keep)
            pred = transformer(hidden_states=hidden, timestep=timesteps, encoder_hidden_states=encoder_hidden_states, return_dict=False)[0]
        return pred, target, sigmas


class MI355XWanControlModelSpecification(MI355XWanControlSpecOps, MI355XWanModelSpecification.MI355X_OVERRIDES):
    """Mirror of ``WanControlModelSpecification``: the constructor keywords (``control_model_processors`` included), ``control_injection_layer_name``,
    ``_original_control_layer_in_features`` / ``_out_features``, ``_qk_norm_identifiers``, ``_trainer_init``, ``load_diffusion_models(new_in_features)``,
    ``forward`` with the reference's signature and ``_save_lora_weights`` with the norm state dict.  Text encoder, VAE, ``prepare_latents`` (which adds
    ``control_latents`` through ``control_model_processors``), pipeline and the inherited ``validation`` stay with the reference; ``validation_latents`` runs its
    denoising loop over this backend's transformer (wan/sampler.py)."""

    def __init__(self, control_model_processors: Optional[List] = None, **kwargs) -> None:
        MI355XWanModelSpecification.MI355X_OVERRIDES.__init__(self, **kwargs)
        self.control_model_processors = keep_or_default(self, "control_model_processors", control_model_processors, [])
        self.frame_conditioning_type = getattr(self, "frame_conditioning_type", None) or "full"
        self.frame_conditioning_index = getattr(self, "frame_conditioning_index", None) or 0
        self.frame_conditioning_concatenate_mask = False

    def _trainer_init(self, frame_conditioning_type, frame_conditioning_index: int, concatenate_mask: bool) -> None:
        if concatenate_mask:
            raise NotImplementedError(_MASK_REASON)
        self.frame_conditioning_type, self.frame_conditioning_index = frame_conditioning_type, frame_conditioning_index
        self.frame_conditioning_concatenate_mask = False

    @staticmethod
    def check_training_arguments(training_type, train_qk_norm: bool = False) -> None:
        """What of the control trainer's arguments this backend runs: ``control-lora`` without trainable QK norms."""
        name = getattr(training_type, "value", training_type)
        if name == "control-full-finetune":
            raise NotImplementedError("control-full-finetune is not covered: the Wan full fine-tune of this backend has no widened patch embedding "
                                      "(use --training_type control-lora)")
        if name != "control-lora":
            raise NotImplementedError(f"training type {name!r}: the control specification goes with --training_type control-lora")
        if train_qk_norm:
            raise NotImplementedError("--train_qk_norm is not covered: the blocks run over a frozen base, their norm_q / norm_k weights get no gradient")

    @property
    def control_injection_layer_name(self) -> str:
        return "patch_embedding"

    def _original_config(self):
        if getattr(self, "transformer_config", None) is None:
            raise RuntimeError("the transformer config is not known yet: load_diffusion_models first (or pass transformer_config)")
        return self.transformer_config

    @property
    def _original_control_layer_in_features(self) -> int:
        c = self._original_config()
        return c["in_channels"] if isinstance(c, dict) else c.in_channels

    @property
    def _original_control_layer_out_features(self) -> int:
        c = self._original_config()
        get = (lambda k: c[k]) if isinstance(c, dict) else (lambda k: getattr(c, k))
        return get("num_attention_heads") * get("attention_head_dim")

    @property
    def _qk_norm_identifiers(self) -> List[str]:
        return ["norm_q", "norm_k", "norm_added_q", "norm_added_k"]

    def load_diffusion_models(self, new_in_features: int, state_dict: Optional[Dict[str, torch.Tensor]] = None, device: Optional[torch.device] = None) -> Dict[str, object]:
        """control_specification.py:122-144: the base model, then the patch embedding widened to ``new_in_features`` input channels with zero weights for
        the new ones.  ``self.transformer_config`` keeps the ORIGINAL channel count (``_original_control_layer_in_features``)."""
        out = MI355XWanModelSpecification.MI355X_OVERRIDES.load_diffusion_models(self, state_dict=state_dict, device=device)
        transformer = out["transformer"]
        self.transformer_config = dataclasses.replace(transformer.config)
        transformer.expand_patch_embedding(new_in_features)
        return out

    def forward(self, transformer, condition_model_conditions: Dict[str, torch.Tensor], latent_model_conditions: Dict[str, torch.Tensor], sigmas: torch.Tensor,
                generator: Optional[torch.Generator] = None, compute_posterior: bool = True, **kwargs):
        """control_specification.py:243-308 -> (pred, target, sigmas); ``compute_posterior`` is forced off there, and ignored here."""
        latents = latent_model_conditions.pop("latents")
        control = latent_model_conditions.pop("control_latents")
        mean, std = latent_model_conditions.pop("latents_mean"), latent_model_conditions.pop("latents_std")
        return MI355XWanControlSpecOps.forward(self, transformer, latents, condition_model_conditions["encoder_hidden_states"], sigmas, mean, std, generator=generator,
                                               control_latents=control, noise=kwargs.get("noise"), use_pack_kernel=kwargs.get("use_pack_kernel"), keep=kwargs.get("keep"))

    def validation_latents(self, transformer, prompt_embeds: torch.Tensor, negative_prompt_embeds: Optional[torch.Tensor], control_latents: torch.Tensor,
                           num_frames: int, height: int, width: int, latents_mean: torch.Tensor, latents_std: torch.Tensor, num_inference_steps: int = 50,
                           guidance_scale: float = 5.0, generator: Optional[torch.Generator] = None, frame_conditioning_type="full",
                           frame_conditioning_index: int = 0, scheduler_config=None, **sample_kwargs) -> torch.Tensor:
        """The denoising loop of ``validation`` (control_specification.py:310-377) in latent space.  ``control_latents`` [B, C, Fc, H, W]: the VAE encoding of the
        control clip (the posterior's mode), not yet normalised; ``latents_mean`` / ``latents_std`` [C]: the VAE's statistics themselves.  As the reference
        does (:350-359) the control latents are normalised with ``1 / std`` and frame-conditioned to ``num_frames`` latent frames (control.py); the sampler
        then holds them in the second half of the model's input channels.  -> denormalised latents [B, C, F, H, W] bf16 for the pipeline's VAE decode."""
        from .sampler import MI355XWanLatentSampler

        if self.frame_conditioning_concatenate_mask:
            raise NotImplementedError(_MASK_REASON)
        ctrl = self.normalize_latents(control_latents.to(bf16), latents_mean.float(), 1.0 / latents_std.float())
        ctrl = apply_frame_conditioning_on_latents(ctrl, num_frames, channel_dim=1, frame_dim=2, frame_conditioning_type=frame_conditioning_type,
                                                   frame_conditioning_index=frame_conditioning_index, concatenate_mask=False)
        return MI355XWanLatentSampler(transformer, scheduler_config).sample(prompt_embeds, negative_prompt_embeds, num_frames, height, width,
                                                                            num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                                                            generator=generator, latents_mean=latents_mean, latents_std=latents_std,
                                                                            control_latents=ctrl, **sample_kwargs)

    def _save_lora_weights(self, directory: str, transformer_state_dict: Optional[Dict[str, torch.Tensor]] = None,
                           norm_state_dict: Optional[Dict[str, torch.Tensor]] = None, scheduler=None, metadata: Optional[Dict[str, str]] = None, *args, **kwargs) -> None:
        """control_specification.py:379-400: the adapter file (``wire.lora_config_metadata`` with ``rank_pattern`` / ``alpha_pattern``), the scheduler config and,
        when a norm dictionary is given, ``norm_state_dict.safetensors``."""
        MI355XWanModelSpecification.MI355X_OVERRIDES._save_lora_weights(self, directory, transformer_state_dict, scheduler, metadata)
        if norm_state_dict is not None:
            from safetensors.torch import save_file

            os.makedirs(directory, exist_ok=True)
            save_file({k: v.detach().to("cpu").contiguous() for k, v in norm_state_dict.items()}, os.path.join(directory, "norm_state_dict.safetensors"))


MI355XWanControlModelSpecification = as_drop_in(MI355XWanControlModelSpecification, "finetrainers.models.wan", "WanControlModelSpecification")
