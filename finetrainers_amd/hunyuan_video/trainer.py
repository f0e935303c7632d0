"""One HunyuanVideo LoRA SFT optimisation step (reference loop: finetrainers/trainer/sft_trainer/trainer.py:430-503 with the HunyuanVideo specification):
noising -> DiT forward -> MSE -> backward -> LoRA-gradient average over the data-parallel ranks -> global-norm clip -> AdamW, the last two fused over ONE flat
fp32 buffer that the blocks' adapter Parameters are views of.  The gradients live in a second flat buffer of the same layout: the blocks' backward adds into
its views in place (no concatenation), and under data parallelism every ``grad_bucket_blocks`` finished blocks -- a contiguous slice, the backward walks the
buffer from its end -- are all-reduced (AVG) asynchronously on RCCL's stream while the earlier blocks still compute (315 MB at rank 64 in 8 buckets for the default 200 adapters)."""

from __future__ import annotations

from typing import Dict, Optional

import torch

from ..lora_step import FlatLoRAStep
from .model import MI355XHunyuanVideoTransformer3DModel
from .specification import MI355XHunyuanVideoSpecOps


class MI355XHunyuanVideoSFTStep(FlatLoRAStep):
    def __init__(self, transformer: MI355XHunyuanVideoTransformer3DModel, spec: Optional[MI355XHunyuanVideoSpecOps] = None, lr: float = 2e-5, betas=(0.9, 0.95),
                 eps: float = 1e-8, weight_decay: float = 1e-4, max_grad_norm: float = 1.0, guidance: float = 1.0, parallel=None,
                 generator: Optional[torch.Generator] = None, lr_scheduler=None, grad_bucket_blocks: int = 8):
        self.params = transformer.lora_parameters()
        if not self.params:
            raise ValueError("attach a LoRA adapter first (transformer.add_adapter)")
        self.transformer, self.spec, self.guidance, self.generator = transformer, spec or MI355XHunyuanVideoSpecOps(), guidance, generator
        self.flat = self.flatten_parameters(self.params)  # every adapter of the model: 200 with the default target, 280 with the text-stream adapters
        # gradient storage: one flat buffer laid out like the parameters; every block writes its two views
        self.gflat = torch.zeros_like(self.flat)
        self.grad_bucket_blocks = max(1, int(grad_bucket_blocks))
        self._blocks = list(transformer.transformer_blocks) + list(transformer.single_transformer_blocks)
        self._spans = {}
        off = 0
        for blk in self._blocks:
            na, nb = blk.lora_A.numel(), blk.lora_B.numel()
            blk._grad_a_view = self.gflat[off:off + na].view(blk.lora_A.shape)
            blk._grad_b_view = self.gflat[off + na:off + na + nb].view(blk.lora_B.shape)
            self._spans[id(blk)] = (off, off + na + nb)
            off += na + nb
        assert off == self.flat.numel()
        self._init_optimizer(self.flat, lr, betas, eps, weight_decay, max_grad_norm, lr_scheduler)
        self._init_exchange(parallel, self.flat, self.gflat)

    def _install_hooks(self, reducer) -> None:
        for blk in self._blocks:  # called from inside the backward when a block's gradient is complete (last block first)
            blk._grad_hook = None if reducer is None else self._block_done

    def _clear_hooks(self) -> None:
        for blk in self._blocks:
            blk._grad_hook = None

    def step(self, latents: torch.Tensor, conditions: Dict[str, torch.Tensor], sigmas: torch.Tensor, compute_posterior: bool = True,
             posterior_noise: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        pred, target, _ = self.spec.forward(self.transformer, latents, dict(conditions), sigmas, guidance=self.guidance, compute_posterior=compute_posterior,
                                            posterior_noise=posterior_noise, noise=noise, generator=self.generator)
        self.gflat.zero_()
        loss = self._backward_exchanging(lambda: self.spec.loss_backward(pred, target), exchange=True)
        gn = self._clip_adamw(self.flat, self.gflat)
        for p in self.params:
            p.grad = None
        return {"loss": loss.detach(), "grad_norm": gn}
