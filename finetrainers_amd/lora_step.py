"""What the four LoRA step objects (LTX, CogVideoX, HunyuanVideo, Wan) share: the adapters in one flat fp32 buffer, the fused clip + AdamW over it with its
state and resume format, and the backward run under the overlapped gradient exchange (``parallel.GradBucketReducer``).  A family's step object adds its
constructor checks, the specification's forward / loss_backward call, its accumulation window, and how its model's gradient hooks are installed and cleared."""

from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional

import torch

from . import ops


class FlatLoRAStep:
    reducer = None    # parallel.GradBucketReducer under data parallelism; read at every step (a test or tool may swap it)
    _exchange = None  # the reducer while a backward runs under it
    _micro_step = 0   # kept by the families that accumulate over micro-steps

    @staticmethod
    def flatten_parameters(params: List[torch.nn.Parameter]) -> torch.Tensor:
        """Re-home the adapter Parameters into ONE buffer (values kept, order of ``params``): one fused clip + AdamW launch covers all of them."""
        flat = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
        off = 0
        for p in params:
            n = p.numel()
            p.data = flat[off:off + n].view(p.shape)
            off += n
        return flat

    def _init_optimizer(self, flat: torch.Tensor, lr: float, betas, eps: float, weight_decay: float, max_grad_norm: float, lr_scheduler=None) -> None:
        """AdamW state laid out like ``flat``.  ``lr_scheduler``: ``utils.lr_schedule.LRSchedule`` (or anything with current_lr() / step()): its rate is read
        for every optimiser step and it is stepped right after, as trainer.py:500-503 does with the LambdaLR."""
        self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm, self.lr_scheduler = lr, betas, eps, weight_decay, max_grad_norm, lr_scheduler
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(flat), torch.zeros_like(flat)
        self._scratch = torch.zeros(ops.CLIP_SCRATCH_FLOATS, dtype=torch.float32, device=flat.device)
        self.step_count = 0

    def _init_exchange(self, parallel, flat: torch.Tensor, gflat: Optional[torch.Tensor] = None, native: Optional[bool] = False) -> None:
        """Replicas start from rank 0's adapters (DDP broadcasts module state the same way; add_adapter draws A from each process's own RNG) and average
        their gradients through one reducer.  ``gflat``: the flat gradient buffer whose block spans ``_block_done`` reports."""
        self.parallel = parallel
        if parallel is not None and parallel.active:
            from .parallel import GradBucketReducer

            parallel.broadcast_(flat, src=0)
            self.reducer = GradBucketReducer(parallel, native=native, gflat=gflat, bucket_blocks=self.grad_bucket_blocks)

    @property
    def buckets_issued(self) -> int:
        """Buckets of the last exchange (0 without data parallelism, and after a micro-step that did not exchange)."""
        return 0 if self.reducer is None else self.reducer.exchange_buckets

    # ---- the backward under the exchange ----------------------------------------------------------------------------------------------------------
    def _install_hooks(self, reducer) -> None:
        """Point the model's gradient hooks at ``reducer`` (None: no exchange in this backward)."""
        raise NotImplementedError

    def _clear_hooks(self) -> None:
        raise NotImplementedError

    def _block_done(self, blk) -> None:
        """``blk._grad_hook`` of the span-reporting families: the block's adapter gradients are final (last block first)."""
        self._exchange.span_done(self._spans[id(blk)])

    def _begin_exchange(self, exchange: bool) -> None:
        if self.reducer is not None:
            self.reducer.begin()
        self._exchange = self.reducer if exchange else None
        self._install_hooks(self._exchange)

    def _finish_exchange(self, failed: bool = False) -> None:
        """The hooks go in every path.  failed: a backward that raised after issuing some buckets -- drained and dropped, never carried into the next step."""
        reducer, self._exchange = self._exchange, None
        self._clear_hooks()
        if reducer is not None:
            reducer.abort() if failed else reducer.finish()

    def _backward_exchanging(self, backward: Callable[[], Any], exchange: bool) -> Any:
        """Run ``backward`` with the gradient hooks installed: buckets of finished blocks are all-reduced (AVG) on RCCL's stream while it still runs, and
        the compute stream has waited for all of them when this returns."""
        self._begin_exchange(exchange)
        try:
            out = backward()
        except BaseException:
            self._finish_exchange(failed=True)
            raise
        self._finish_exchange()
        return out

    # ---- the optimiser tail -----------------------------------------------------------------------------------------------------------------------
    def _clip_adamw(self, flat: torch.Tensor, gflat: torch.Tensor) -> torch.Tensor:
        """Global-norm clip (utils/torch.py:99-161) + AdamW (optimizer.py:117-125), fused over the flat buffer; returns the gradient norm (device scalar)."""
        self.step_count += 1
        gn = torch.empty(1, dtype=torch.float32, device=gflat.device)
        lr = self.lr if self.lr_scheduler is None else self.lr_scheduler.current_lr()
        ops.clip_adamw_step(flat, gflat, self.exp_avg, self.exp_avg_sq, self.step_count, lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm,
                            scratch=self._scratch, grad_norm_out=gn)
        self._after_update()
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        return gn

    def _after_update(self) -> None:
        """The library moved the adapters in place: whatever the model derives from them is stale."""

    # ---- resume (reference: utils/state_checkpoint.py saves optimizer + scheduler state next to the model's) --------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        """Optimiser state laid out like ``flat``, the step counters and the schedule clock; the adapters themselves travel with the model."""
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self.step_count, "micro_step": self._micro_step,
                "lr_scheduler": None if self.lr_scheduler is None else self.lr_scheduler.state_dict()}

    @torch.no_grad()
    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        if sd["exp_avg"].numel() != self.exp_avg.numel():
            raise ValueError(f"optimizer state holds {sd['exp_avg'].numel()} values, the attached adapter needs {self.exp_avg.numel()}")
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count, self._micro_step = int(sd["step"]), int(sd.get("micro_step", 0))
        if self.lr_scheduler is not None and sd.get("lr_scheduler") is not None:
            self.lr_scheduler.load_state_dict(sd["lr_scheduler"])
