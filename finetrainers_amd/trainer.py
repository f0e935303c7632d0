"""The SFT optimisation step of finetrainers, MI355X-native.

``MI355XSFTStep.step`` restates the body of ``SFTTrainer._train`` (finetrainers/trainer/sft_trainer/trainer.py:
430-528) for the LoRA path: sigma sampling -> ``ModelSpecification.forward`` -> weighted MSE -> backward ->
(DP: all-reduce of the flat LoRA gradient over RCCL/xGMI) -> global-norm clip -> AdamW.  Differences that are
design, not drift:
  * loss + d(loss)/d(pred) is one kernel, clip + AdamW is one kernel over the flat fp32 LoRA buffer;
  * no host synchronisation inside the step: loss / grad-norm stay on the device (the reference does five
    ``.item()`` calls per step, trainer.py:483,506 and parallel/utils.py:11); ``step`` returns device scalars.
``sft_loss`` is the drop-in for trainer.py:473-480 when the reference's own loop is kept (a torch scalar whose
``backward()`` feeds the DiT backward).
"""

from __future__ import annotations

from typing import Any, Dict, Optional

import torch

from . import ops
from .lora_step import FlatLoRAStep
from .utils import diffusion as diffusion_utils


class _MSELossFunction(torch.autograd.Function):
    """loss = scale * mean_b mean w_b (pred - target)^2 with d loss / d pred from the same kernel.  ``scale`` (1 / accumulation
    steps) is applied exactly ONCE: the kernel folds it into the saved gradient, the returned loss is multiplied here."""

    @staticmethod
    def forward(ctx, pred, target, weight, scale):
        loss, dpred = ops.mse_loss(pred.contiguous(), target.contiguous(), weight, want_grad=True, grad_scale=scale)
        ctx.save_for_backward(dpred)
        loss = loss.reshape(())
        return loss * scale if scale != 1.0 else loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g.to(dpred.dtype), None, None, None  # g = 1 for loss.backward(); no host sync either way


def sft_loss(pred: torch.Tensor, target: torch.Tensor, sigmas: torch.Tensor, flow_weighting_scheme: str = "none",
             gradient_accumulation_steps: int = 1) -> torch.Tensor:
    """trainer.py:463-480: ``weights * (pred.float() - target.float())**2`` averaged over all non-batch dims then the
    batch, divided by the accumulation steps.  ``sigmas`` as returned by the spec ([B,S,1], constant per sample)."""
    per_sample_sigma = sigmas.reshape(sigmas.shape[0], -1)[:, 0].float()
    weights = diffusion_utils.compute_loss_weighting_for_sd3(flow_weighting_scheme, per_sample_sigma).float().contiguous()
    return _MSELossFunction.apply(pred, target, weights, 1.0 / gradient_accumulation_steps)


class MI355XSFTStep(FlatLoRAStep):
    """One LoRA SFT optimisation step on one rank (one process per GPU).  ``parallel`` is a
    ``finetrainers_amd.parallel.DataParallelBackend`` (or None for a single GPU).

    Data parallelism (reference: ``apply_ddp`` -> ``replicate``, parallel/ptd.py:462-463): on construction the LoRA parameters are
    broadcast from rank 0 (DDP broadcasts module state the same way), every step each rank runs its own samples, and the LoRA
    gradients are averaged bucket by bucket WHILE the backward is still running (``GradBucketReducer``).  With
    ``gradient_accumulation_steps`` > 1 only the last micro-step of a group applies AdamW; every micro-step exchanges and clips, as the
    reference loop does (trainer.py:479-503), unless ``no_sync_accumulation``."""

    def __init__(self, transformer, specification, lr: float = 5e-5, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 1e-4,
                 max_grad_norm: float = 1.0, flow_weighting_scheme: str = "none", flow_logit_mean: float = 0.0, flow_logit_std: float = 1.0,
                 flow_mode_scale: float = 1.29, parallel=None, generator: Optional[torch.Generator] = None,
                 gradient_accumulation_steps: int = 1, grad_bucket_blocks: int = 7, lr_scheduler=None, compute_posterior: bool = True, no_sync_accumulation: bool = False):
        if transformer.lora_A is None:
            raise ValueError("attach a LoRA adapter first (transformer.add_adapter)")
        if gradient_accumulation_steps < 1:
            raise ValueError("gradient_accumulation_steps must be >= 1")
        self.transformer = transformer
        self.spec = specification
        self.scheme = flow_weighting_scheme
        self.flow_logit_mean, self.flow_logit_std, self.flow_mode_scale = flow_logit_mean, flow_logit_std, flow_mode_scale
        self.generator = generator
        self.gradient_accumulation_steps, self.grad_bucket_blocks = gradient_accumulation_steps, grad_bucket_blocks
        # False = the batches carry the VAE posterior's moments (what --enable_precomputation stores, trainer.py:374) and every step samples them
        self.compute_posterior = compute_posterior
        # Data parallelism x gradient accumulation: the reference wraps the model with replicate() and never enters no_sync (trainer.py:479-503,
        # "TODO revisit no_sync"), so EVERY backward all-reduces the accumulated .grad and the per-backward clip sees the same averaged sums on
        # all ranks.  That is the default here too; True skips the exchange (and the clip) on the non-stepping micro-steps -- equal results
        # whenever no partial sum exceeds max_grad_norm, half the traffic.
        self.no_sync_accumulation = no_sync_accumulation
        self._micro_step = 0
        dev = transformer.device
        transformer._assert_flat_aliasing()
        # flat fp32 optimiser state matching transformer.lora_flat = [A | B] (with feed-forward adapters [A | B | FF]: the fused clip + AdamW and the
        # exchange cover the whole buffer either way)
        self.n_a, self.n_b = transformer._lora_A_full.numel(), transformer._lora_B_full.numel()  # storage size (rank padded to a multiple of 64)
        self.n_ff = transformer._lora_ff_full.numel() if getattr(transformer, "lora_ff", False) else 0
        self._init_optimizer(transformer.lora_flat, lr, betas, eps, weight_decay, max_grad_norm, lr_scheduler)
        # MI355XParallelBackend.apply_ddp() installs the exchange ON THE MODEL (hook + finish, like DDP's reducer): a step that is handed such a model
        # leaves those hooks where they are -- the backward then returns with averaged gradients -- and must not bring a second exchange of its own
        self._model_owns_exchange = getattr(transformer, "_grad_bucket_hook", None) is not None and getattr(transformer, "_grad_bucket_finish", None) is not None
        if self._model_owns_exchange and parallel is not None and parallel.active:
            raise ValueError("MI355XSFTStep(parallel=...) on a model that apply_ddp() already wired for the gradient exchange: the gradients would be averaged "
                             "twice -- pass parallel=None (the model's own hooks do the exchange) or do not call apply_ddp")
        self._init_exchange(parallel, transformer.lora_flat, native=None)  # (native: the in-library communicator where FTMI_NATIVE_ALLREDUCE=1 asks for it)
        if self.reducer is not None:
            transformer._lora_versions = None
            transformer.grad_bucket_blocks = grad_bucket_blocks
        from .ltx_video.specification import FlowMatchSigmas

        self.scheduler = FlowMatchSigmas()
        self.scheduler_sigmas = self.scheduler.sigmas.to(dev)

    def sample_sigmas(self, batch_size: int) -> torch.Tensor:
        """trainer.py:436-448."""
        return diffusion_utils.prepare_sigmas(
            scheduler=self.scheduler, sigmas=self.scheduler_sigmas, batch_size=batch_size, num_train_timesteps=1000,
            flow_weighting_scheme=self.scheme, flow_logit_mean=self.flow_logit_mean, flow_logit_std=self.flow_logit_std,
            flow_mode_scale=self.flow_mode_scale, device=self.scheduler_sigmas.device, generator=self.generator,
        )

    def step(self, condition_model_conditions: Dict[str, Any], latent_model_conditions: Dict[str, Any], sigmas: Optional[torch.Tensor] = None,
             **spec_kwargs) -> Dict[str, Optional[torch.Tensor]]:
        """One micro-step.  Returns device scalars ``loss`` (already divided by the accumulation steps, as trainer.py:479 logs it) and
        ``grad_norm`` (None on the non-final micro-steps of an accumulation group, where no optimiser step happens)."""
        tr = self.transformer
        tr._assert_flat_aliasing()
        latents = latent_model_conditions["latents"]
        B = latents.shape[0]
        if sigmas is None:
            sigmas = self.sample_sigmas(B)
        gas = self.gradient_accumulation_steps
        self._micro_step += 1
        sync = self._micro_step % gas == 0  # last micro-step of the group: exchange gradients, clip, step (trainer.py:498)
        # 3. forward (trainer.py:452-461)
        pred, target, sig = self.spec.forward(
            transformer=tr, condition_model_conditions=dict(condition_model_conditions), latent_model_conditions=dict(latent_model_conditions),
            sigmas=sigmas, generator=self.generator, compute_posterior=self.compute_posterior, **spec_kwargs,
        )
        # 4. loss + backward (trainer.py:463-481): loss and d loss / d pred come out of one kernel and the DiT backward is seeded with
        # that gradient directly (what loss.backward() would hand it, without the unit-seed multiply)
        per_sample_sigma = sig.reshape(B, -1)[:, 0].float()
        weights = diffusion_utils.compute_loss_weighting_for_sd3(self.scheme, per_sample_sigma).float().contiguous()
        loss, dpred = ops.mse_loss(pred.detach().contiguous(), target.contiguous(), weights, want_grad=True, grad_scale=1.0 / gas)
        loss = loss.reshape(()) / gas if gas > 1 else loss.reshape(())
        exchange = self.reducer is not None and (sync or not self.no_sync_accumulation)
        # Who owns the exchange is decided PER STEP, not at construction: apply_ddp() may be called on the model after this object was built (a step
        # that then blanked the model's hooks for its backward would leave the replicas to diverge silently).
        self._model_owns_exchange = tr._grad_bucket_hook is not None and tr._grad_bucket_finish is not None
        if self._model_owns_exchange and self.reducer is not None:
            raise RuntimeError("MI355XSFTStep has its own gradient exchange (parallel=...) and the model now carries apply_ddp()'s hooks as well: the gradients "
                               "would be averaged twice -- build the step with parallel=None or do not call apply_ddp on this model")
        self._backward_exchanging(lambda: pred.backward(dpred), exchange)
        if not sync:
            # the reference clips after every backward (trainer.py:487-492), i.e. also the partial sums of an accumulation window -- in place
            # on .grad (under DP on the all-reduced sums, see no_sync_accumulation)
            if self.max_grad_norm and self.max_grad_norm > 0 and (self.reducer is None or exchange):
                ops.clip_grad_norm_(self._flat_grad(tr.lora_A.grad, tr.lora_B.grad, [p.grad for p in self._ff_params()]), self.max_grad_norm, scratch=self._scratch)
            return {"loss": loss.detach(), "grad_norm": None}
        # 5-6. clip + AdamW, fused over the flat buffer
        grad_norm = self._clip_adamw(tr.lora_flat, self._flat_grad(tr.lora_A.grad, tr.lora_B.grad, [p.grad for p in self._ff_params()]))
        tr.lora_A.grad = None  # optimizer.zero_grad(set_to_none=True) (trainer.py:503)
        tr.lora_B.grad = None
        for p in self._ff_params():
            p.grad = None
        return {"loss": loss.detach(), "grad_norm": grad_norm}

    # ---- the model's hooks for the duration of the backward ---------------------------------------------------------------------------------
    def _install_hooks(self, reducer) -> None:
        tr = self.transformer
        self._prev_hooks = tr._grad_bucket_hook, tr._grad_bucket_finish
        if not self._model_owns_exchange:  # this step's own reducer (or none); a model wired by apply_ddp() keeps its hooks and ends the exchange itself
            tr._grad_bucket_hook, tr._grad_bucket_finish = (None if reducer is None else reducer.bucket_ready), None

    def _clear_hooks(self) -> None:  # put back what was there
        self.transformer._grad_bucket_hook, self.transformer._grad_bucket_finish = self._prev_hooks

    def _after_update(self) -> None:
        self.transformer._lora_versions = None  # parameters changed in place by the library: refresh the bf16 working copies next forward

    flat = property(lambda self: self.transformer.lora_flat)
    gflat = property(lambda self: self.transformer._grad_flat)

    def state_dict(self) -> Dict[str, Any]:
        """AdamW moments laid out like ``transformer.lora_flat`` ([A | B], rank-padded storage); the LoRA parameters travel in ``transformer.state_dict()``."""
        hyper = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay, "max_grad_norm": self.max_grad_norm}
        return dict(super().state_dict(), hyper=hyper)

    def _ff_params(self):
        tr = self.transformer
        return tr._ff_params() if self.n_ff else ()

    def _flat_grad(self, ga: torch.Tensor, gb: torch.Tensor, gff=()) -> torch.Tensor:
        gflat = self.transformer._grad_flat
        n_ab = self.n_a + self.n_b
        ff_own = self.n_ff == 0 or (gflat is not None and all(g is not None and g.data_ptr() == gflat.data_ptr() + 4 * (n_ab + off)
                                                              for g, off in zip(gff, self.transformer._ff_offsets())))
        if gflat is not None and ga.data_ptr() == gflat.data_ptr() and gb.data_ptr() == gflat.data_ptr() + 4 * self.n_a and ff_own:
            return gflat  # .grad IS the flat buffer the kernels wrote (the usual case)
        if self.reducer is not None:
            raise RuntimeError("data-parallel step: lora_A.grad / lora_B.grad are not the backend's flat gradient buffer (foreign .grad tensors "
                               "were installed); the bucketed exchange would have missed them")
        tr = self.transformer  # foreign .grad tensors (single GPU only): lay them out like the (rank-padded) parameter storage
        flat = torch.zeros(n_ab + self.n_ff, dtype=torch.float32, device=ga.device)
        flat[:self.n_a].view_as(tr._lora_A_full)[:, :, :tr.lora_rank, :].copy_(ga)
        flat[self.n_a:n_ab].view_as(tr._lora_B_full)[:, :, :, :tr.lora_rank].copy_(gb)
        if self.n_ff:
            for dst, g in zip(tr._ff_views(flat[n_ab:].view_as(tr._lora_ff_full)), gff):
                dst.copy_(g)
        return flat
