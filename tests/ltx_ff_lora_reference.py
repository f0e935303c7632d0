"""Oracle side of the LTX-Video feed-forward adapters (tests only): after ``oracle.ltx.build_model`` wraps ``ff.net.0.proj`` and ``ff.net.2`` of every block in
``oracle.ltx.LoraLinear`` -- what peft does for a ``target_modules`` that names them (finetrainers/trainer/control_trainer/config.py:60).  fp32 adapter
parameters that require grad; A drawn as peft does (uniform within 1 / sqrt(fan_in)), B from N(0, b_std) so that no gradient is identically zero."""
import math

import torch

from oracle import ltx

CONTROL_TARGET_MODULES = "(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|ff.net.0.proj|ff.net.2)"
FF_MODULES = ("ff.net.0.proj", "ff.net.2")


def add_ff_lora(model, rank: int, alpha: float, b_std: float = 0.02, seed: int = 7):
    """Wrap the two feed-forward projections of every block; returns the wrapped module paths.  Deterministic in ``seed`` (its own generator)."""
    g = torch.Generator().manual_seed(seed)
    names = []
    for li, block in enumerate(model.transformer_blocks):
        for path in FF_MODULES:
            holder, leaf = (block.ff.net[0], "proj") if path.endswith("proj") else (block.ff.net, 2)
            base = getattr(holder, leaf) if isinstance(leaf, str) else holder[leaf]
            wrapped = ltx.LoraLinear(base, rank, float(alpha))
            a, b = wrapped.lora_A["default"].weight, wrapped.lora_B["default"].weight
            bound = 1.0 / math.sqrt(base.in_features)
            a.data = ((torch.rand(a.shape, generator=g) * 2 - 1) * bound).float()
            b.data = (torch.randn(b.shape, generator=g) * b_std).float()
            a.requires_grad_(True), b.requires_grad_(True)
            for p in base.parameters():
                p.requires_grad_(False)
            if isinstance(leaf, str):
                setattr(holder, leaf, wrapped)
            else:
                holder[leaf] = wrapped
            names.append(f"transformer_blocks.{li}.{path}")
    return names


def build_pair(cfg, rank: int, alpha: float, seed: int = 0):
    """(bf16 oracle, fp32 evaluation of the same graph on the same bf16-valued weights), both with ten adapters per block."""
    omodel = ltx.build_model(cfg, seed=seed, rank=rank, alpha=float(alpha), lora_b_std=0.02)
    add_ff_lora(omodel, rank, alpha)
    m32 = ltx.build_model(cfg, seed=seed, rank=rank, alpha=float(alpha), lora_b_std=0.02, dtype=torch.float32)
    add_ff_lora(m32, rank, alpha)
    m32.load_state_dict({k: v.float() for k, v in omodel.state_dict().items()})
    return omodel, m32


def float_inputs(inp):
    return ltx.StepInputs(**{k: (getattr(inp, k).float() if torch.is_tensor(getattr(inp, k)) else getattr(inp, k)) for k in
                             ("latents", "latents_mean", "latents_std", "encoder_hidden_states", "encoder_attention_mask", "sigmas", "noise", "first_frame_sigma")})
