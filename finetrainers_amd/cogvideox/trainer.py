"""One CogVideoX LoRA SFT optimisation step (reference loop: finetrainers/trainer/sft_trainer/trainer.py:430-503 with the CogVideoX
specification): sigma draw -> DDIM noising -> DiT forward -> velocity -> x0 -> 1 / (1 - alphas_cumprod) weighted MSE -> backward -> LoRA-gradient
average over the data-parallel ranks -> global-norm clip -> AdamW, the last two fused over the model-wide flat LoRA buffer.  The gradients of a
block (native block stack: of a range of blocks) are all-reduced (AVG, asynchronously on RCCL's stream) as soon as the backward has produced them,
while the earlier blocks still compute (``lora_step.FlatLoRAStep``).  ``--gradient_checkpointing`` is the transformer's flag
(``apply_activation_checkpointing`` / ``enable_gradient_checkpointing``): the step follows it, block ranges and buckets included, and takes no argument for it."""

from __future__ import annotations

from typing import Dict, Optional

import torch

from ..lora_step import FlatLoRAStep
from .model import MI355XCogVideoXTransformer3DModel
from .specification import MI355XCogVideoXSpecOps


class MI355XCogVideoXSFTStep(FlatLoRAStep):
    def __init__(self, transformer: MI355XCogVideoXTransformer3DModel, spec: Optional[MI355XCogVideoXSpecOps] = None, lr: float = 5e-5,
                 betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 1e-4, max_grad_norm: float = 1.0, parallel=None,
                 generator: Optional[torch.Generator] = None, lr_scheduler=None, grad_bucket_blocks: int = 5):
        if transformer.lora_flat is None:
            raise ValueError("attach a LoRA adapter first (transformer.add_adapter)")
        self.transformer, self.spec, self.generator = transformer, spec or MI355XCogVideoXSpecOps(), generator
        self.grad_bucket_blocks = grad_bucket_blocks  # native block stack: blocks per all-reduce bucket (2 x 5 x 4 x r x D fp32 = 39 MB at rank 128)
        self._init_optimizer(transformer.lora_flat, lr, betas, eps, weight_decay, max_grad_norm, lr_scheduler)
        self._init_exchange(parallel, transformer.lora_flat)
        # utils/diffusion.py:75-81: the DDIM "sigma" table is scheduler.timesteps / num_train_timesteps, timesteps = 999 ... 0
        n = self.spec.scheduler.config.num_train_timesteps
        self.num_train_timesteps = n
        self.sigma_table = (torch.arange(n - 1, -1, -1, device=transformer.device).float() / float(n))

    flat = property(lambda self: self.transformer.lora_flat)
    gflat = property(lambda self: self.transformer.flat_lora_grad())

    def sample_sigmas(self, batch_size: int) -> torch.Tensor:
        """utils/diffusion.py:107-114: uniform draw, index into the table."""
        u = torch.rand((batch_size,), device=self.transformer.device, generator=self.generator)
        return self.sigma_table[(u * self.num_train_timesteps).long()]

    def _install_hooks(self, reducer) -> None:
        """Both hooks are called from inside the backward, last block first, with a bucket's (A, B) slices: every rank issues the same sequence."""
        tr = self.transformer
        per_block = None if reducer is None else (lambda ga, gb: reducer.bucket_ready(None, None, ga, gb))
        for blk in tr.transformer_blocks:  # per-block Python composition: one bucket per block
            blk._grad_hook = per_block
        # native block stack: the backward runs in ranges of grad_bucket_blocks blocks, each range's slices of the flat gradient are one bucket
        tr._grad_bucket_hook = None if reducer is None else reducer.bucket_ready
        tr.grad_bucket_blocks = self.grad_bucket_blocks

    def _clear_hooks(self) -> None:
        self.transformer._grad_bucket_hook = None
        for blk in self.transformer.transformer_blocks:
            blk._grad_hook = None

    def _after_update(self) -> None:
        self.transformer._lora_versions = None  # parameters changed in place by the library: refresh the bf16 working copies next forward

    def step(self, latents: torch.Tensor, encoder_hidden_states: torch.Tensor, sigmas: Optional[torch.Tensor] = None,
             noise: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        tr = self.transformer
        if sigmas is None:
            sigmas = self.sample_sigmas(latents.shape[0])
        pred, target, _ = MI355XCogVideoXSpecOps.forward(self.spec, tr, latents, encoder_hidden_states, sigmas, noise=noise, generator=self.generator)
        loss = self._backward_exchanging(lambda: self.spec.loss_backward(pred, target, sigmas), exchange=True)
        gn = self._clip_adamw(tr.lora_flat, tr.flat_lora_grad())
        for blk in tr.transformer_blocks:
            blk.lora_A.grad = blk.lora_B.grad = None
        return {"loss": loss.detach(), "grad_norm": gn}
