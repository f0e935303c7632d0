"""Wan-T2V transformer for FULL fine-tuning on the MI355X (BASELINE config 4) with the call contract of the diffusers model the reference
drives (finetrainers/models/wan/base_specification.py:476-487): ``forward(hidden_states [B, C, F, H, W], timestep [B], encoder_hidden_states [B, T, 4096])``
-> ``(velocity [B, C, F, H, W],)``.

Parameters live in flat bf16 buffers -- one per block (block.py) and one ``root`` buffer for everything outside the blocks (patch embedding, condition
embedder, output table and projection) -- exactly the units FSDP-2 shards in the reference (parallel/ptd.py:466-499: ``fully_shard`` per block, then the
model).  Gradients are flat fp32 buffers of the same layouts, written by the backward kernels; nothing goes through ``.grad``.

Restated in oracle/wan.py ([upstream] diffusers transformer_wan.py + the reference's patched condition embedder, patches/models/wan/patch.py:17-33)."""

from __future__ import annotations

import math
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from .. import ops
from ..cogvideox.model import timestep_embedding
from .block import LORA_FFN_TARGETS, LORA_TARGETS, MI355XWanBlock

bf16 = torch.bfloat16


@dataclass
class WanTransformerConfig:
    """diffusers ``WanTransformer3DModel`` config keys; defaults = Wan2.1-T2V-1.3B."""

    patch_size: Tuple[int, int, int] = (1, 2, 2)
    num_attention_heads: int = 12
    attention_head_dim: int = 128
    in_channels: int = 16
    out_channels: int = 16
    text_dim: int = 4096
    freq_dim: int = 256
    ffn_dim: int = 8960
    num_layers: int = 30
    cross_attn_norm: bool = True
    qk_norm: str = "rms_norm_across_heads"
    eps: float = 1e-6
    image_dim: Optional[int] = None
    rope_max_seq_len: int = 1024
    # first/last-frame image-to-video (Wan2.1-FLF2V): the image embedder holds ``pos_embed`` [1, pos_embed_seq_len, image_dim] and attn2's image context is
    # the tokens of TWO images (2 x 257 = 514)
    pos_embed_seq_len: Optional[int] = None

    def __post_init__(self):
        n = self.pos_embed_seq_len
        if n is None:
            return
        if self.image_dim is None:
            raise ValueError("pos_embed_seq_len (first/last-frame) belongs to an image-to-video model: image_dim is missing")
        if not isinstance(n, int) or n <= 0 or n % 2 != 0:
            raise ValueError(f"pos_embed_seq_len must be a positive even number (the tokens of two images), got {n}")
        if n > 640:
            raise ValueError(f"pos_embed_seq_len = {n}: the image context of attn2 holds at most 640 tokens (two images of up to 320)")

    @property
    def second_image_tokens(self) -> int:
        """TI2 of the block: the tokens of the last frame's image (0: a single image)."""
        return 0 if self.pos_embed_seq_len is None else self.pos_embed_seq_len // 2

    @property
    def inner_dim(self) -> int:
        return self.num_attention_heads * self.attention_head_dim

    @classmethod
    def from_dict(cls, d: Dict) -> "WanTransformerConfig":
        known = {k: d[k] for k in cls.__dataclass_fields__ if k in d}
        if "patch_size" in known:
            known["patch_size"] = tuple(known["patch_size"])
        return cls(**known)


def select_module_names(names: List[str], target_modules) -> List[str]:
    """peft's rule (tuners_utils.check_target_module_exists) over a model's module names: a string is ``re.fullmatch``ed against every name; a list or
    tuple selects a name that equals an entry or ends with "." + entry.  Shared by every model that resolves a ``target_modules``."""
    if isinstance(target_modules, str):
        hit = lambda n: re.fullmatch(target_modules, n) is not None
    elif isinstance(target_modules, (list, tuple)) and all(isinstance(t, str) for t in target_modules):
        hit = lambda n: any(n == t or n.endswith("." + t) for t in target_modules)
    else:
        raise TypeError("target_modules is a regular expression (str) or a list of module-name suffixes")
    return [n for n in names if hit(n)]


def rotary_tables(cfg: WanTransformerConfig, frames: int, height: int, width: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``WanRotaryPosEmbed`` for LATENT sizes: (cos, sin) fp32 [F' H' W', head_dim / 2]; the head's complex pairs split t : h : w, position tables in
    float64 like the reference (get_1d_rotary_pos_embed(freqs_dtype=float64))."""
    pt, ph, pw = cfg.patch_size
    f, h, w = frames // pt, height // ph, width // pw
    d = cfg.attention_head_dim
    hw = 2 * (d // 6)
    dims = (d - 2 * hw, hw, hw)

    def ang(dim, n):
        freq = 1.0 / (10000.0 ** (torch.arange(0, dim, 2, dtype=torch.float64)[: dim // 2] / dim))
        return torch.outer(torch.arange(n, dtype=torch.float64), freq)

    at = ang(dims[0], f).view(f, 1, 1, -1).expand(f, h, w, -1)
    ah = ang(dims[1], h).view(1, h, 1, -1).expand(f, h, w, -1)
    aw = ang(dims[2], w).view(1, 1, w, -1).expand(f, h, w, -1)
    a = torch.cat([at, ah, aw], dim=-1).reshape(f * h * w, d // 2)
    return torch.cos(a).float().contiguous(), torch.sin(a).float().contiguous()


class RootLayout:
    """Parameters outside the blocks, diffusers names, in one flat buffer."""

    def __init__(self, cfg: WanTransformerConfig):
        D = cfg.inner_dim
        pt, ph, pw = cfg.patch_size
        pk = cfg.in_channels * pt * ph * pw
        po = cfg.out_channels * pt * ph * pw
        if po % 64 != 0 or (pk % 64 != 0 and cfg.image_dim is None):
            raise ValueError("patch embedding / output projection widths must be multiples of 64 for the GEMM")
        # image-to-video: 36 input channels (16 noised | 4 mask | 16 conditioning latents) make 144 patch columns -- stored zero-padded to the GEMM's
        # multiple of 64 (the tokens' columns are padded the same way; the state-dict view is the first ``patch_cols`` columns)
        self.patch_cols, pk = pk, (pk + 63) // 64 * 64
        self.entries: List[Tuple[str, Tuple[int, ...]]] = [
            ("patch_embedding.weight", (D, pk)), ("patch_embedding.bias", (D,)),
            ("condition_embedder.time_embedder.linear_1.weight", (D, cfg.freq_dim)), ("condition_embedder.time_embedder.linear_1.bias", (D,)),
            ("condition_embedder.time_embedder.linear_2.weight", (D, D)), ("condition_embedder.time_embedder.linear_2.bias", (D,)),
            ("condition_embedder.time_proj.weight", (6 * D, D)), ("condition_embedder.time_proj.bias", (6 * D,)),
            ("condition_embedder.text_embedder.linear_1.weight", (D, cfg.text_dim)), ("condition_embedder.text_embedder.linear_1.bias", (D,)),
            ("condition_embedder.text_embedder.linear_2.weight", (D, D)), ("condition_embedder.text_embedder.linear_2.bias", (D,)),
            ("scale_shift_table", (1, 2, D)),
            ("proj_out.weight", (po, D)), ("proj_out.bias", (po,)),
        ]
        if cfg.image_dim is not None:  # WanImageEmbedding: FP32LayerNorm -> Linear -> GELU (erf) -> Linear -> FP32LayerNorm
            Di, ie = cfg.image_dim, "condition_embedder.image_embedder."
            self.entries += [(ie + "norm1.weight", (Di,)), (ie + "norm1.bias", (Di,)), (ie + "ff.net.0.proj.weight", (Di, Di)), (ie + "ff.net.0.proj.bias", (Di,)),
                             (ie + "ff.net.2.weight", (D, Di)), (ie + "ff.net.2.bias", (D,)), (ie + "norm2.weight", (D,)), (ie + "norm2.bias", (D,))]
            if cfg.pos_embed_seq_len is not None:  # appended: without it no offset moves
                self.entries.append((ie + "pos_embed", (1, cfg.pos_embed_seq_len, Di)))
        self.offsets: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        off = 0
        for name, shape in self.entries:
            self.offsets[name] = (off, shape)
            off += (math.prod(shape) + 63) // 64 * 64
        self.total = off

    def view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        off, shape = self.offsets[name]
        return flat[off:off + math.prod(shape)].view(shape)

    def named_views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """{diffusers name: view}; the patch embedding without its padding columns."""
        out = {n: self.view(flat, n) for n, _ in self.entries}
        out["patch_embedding.weight"] = out["patch_embedding.weight"][:, :self.patch_cols]
        return out


class _LinearFunction(torch.autograd.Function):
    """y = act(x W^T + b) with trainable W, b: MFMA GEMM forward (optional GELU-tanh epilogue), input gradient as an NT GEMM against W^T, weight gradient
    with the token-reduction GEMM (dW += dY^T X, fp32, straight into the flat gradient buffer), bias gradient as column sums."""

    @staticmethod
    def forward(ctx, x, w, b, gw, gb, gelu: bool, need_dx: bool, anchor):  # anchor: a requires-grad dummy so that autograd visits layers fed by data
        x2d = x.reshape(-1, x.shape[-1])
        if gelu:
            y, pre = ops.gemm_nt(x2d, w, b, epilogue=1, want_out2=True)
        else:
            y, pre = ops.gemm_nt(x2d, w, b), None
        ctx.args = (x2d, w, gw, gb, pre, need_dx, x.shape)
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2d, w, gw, gb, pre, need_dx, xshape = ctx.args
        ctx.args = None
        dy2d = dy.reshape(-1, dy.shape[-1]).contiguous()
        if pre is not None:  # through the GELU: dz = dy * gelu'(pre), with the identity "GEMM" folded away -- elementwise on a [rows, N] tensor
            dy2d = _dgelu(dy2d, pre)
        ops.gemm_tn(dy2d, x2d, out=gw)
        ops.wan_colsum(dy2d, gb)
        dx = ops.gemm_nt(dy2d, ops.transpose_bf16(w), None).view(xshape) if need_dx else None
        return dx, None, None, None, None, None, None, None


def _dgelu(dy: torch.Tensor, pre: torch.Tensor) -> torch.Tensor:
    """dy * d/dz gelu_tanh(z) in fp32, one bf16 rounding (torch's GeluBackward on bf16 tensors).  Only the text embedder's [B T, D] tensor comes through here."""
    z = pre.float()
    k0, k1 = 0.7978845608028654, 0.044715
    u = k0 * (z + k1 * z * z * z)
    t = torch.tanh(u)
    dg = 0.5 * (1 + t) + 0.5 * z * (1 - t * t) * k0 * (1 + 3 * k1 * z * z)
    return (dy.float() * dg).to(bf16)


class _FrozenLinearFunction(torch.autograd.Function):
    """y = x W^T + b over FROZEN W, b (LoRA training: the root's output projection): input gradient only, against a cached K-contiguous twin of W."""

    @staticmethod
    def forward(ctx, x, w, b, w_t):
        ctx.w_t, ctx.xshape = w_t, x.shape
        return ops.gemm_nt(x.reshape(-1, x.shape[-1]), w, b).view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        return ops.gemm_nt(dy.reshape(-1, dy.shape[-1]).contiguous(), ctx.w_t, None).view(ctx.xshape), None, None, None


class _LnModFunction(torch.autograd.Function):
    """y = bf(LN(float(x)) * (1 + scale_b) + shift_b) with fp32 [B, D] shift / scale (the output norm); returns gradients for x, shift and scale."""

    @staticmethod
    def forward(ctx, x, shift, scale, eps: float):
        B, S, D = x.shape
        shift, scale = shift.contiguous(), scale.contiguous()
        y = ops.wan_ln(x.view(B * S, D), S, shift=shift, scale=scale, eps=eps)
        ctx.save_for_backward(x, scale)
        ctx.eps = eps
        return y.view(B, S, D)

    @staticmethod
    def backward(ctx, dy):
        x, scale = ctx.saved_tensors
        B, S, D = x.shape
        if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):  # frozen modulation (LoRA training): no reductions
            return ops.wan_ln_bwd(x.view(B * S, D), dy.contiguous().view(B * S, D), S, scale=scale, eps=ctx.eps).view(B, S, D), None, None, None
        red = torch.zeros((2, B, D), dtype=torch.float32, device=x.device)
        dx = ops.wan_ln_bwd(x.view(B * S, D), dy.contiguous().view(B * S, D), S, scale=scale, eps=ctx.eps, red1=red[0], red2=red[1], red_per_batch=True)
        return dx.view(B, S, D), red[0], red[1], None


class _PatchLoRAFunction(torch.autograd.Function):
    """The widened patch embedding with its full-rank adapter, folded: y = bf(bf(cols W^T + b) + s (cols A^T) B^T) as ONE NT GEMM whose K-extension
    runs over the bf16 planes of dW = s B A.  The backward takes block 0's input gradient and forms the two adapter gradients (``ftmi_wan_patch_lora_backward``);
    the input is data: no gradient flows further.  With a step object the gradients are added into its flat views and ``model._patch_grad_hook`` fires."""

    @staticmethod
    def forward(ctx, model: "MI355XWanTransformer3DModel", cols2, lora_a, lora_b):
        w, b = model.rparam("patch_embedding.weight"), model.rparam("patch_embedding.bias")
        key = (lora_a.data_ptr(), lora_a._version, lora_b.data_ptr(), lora_b._version, model._patch_epoch, w.data_ptr())
        refold, model._patch_fold_key = key != model._patch_fold_key, key
        dw, w2, _ = model._patch_ws
        y = ops.wan_patch_lora_forward(cols2, w, b, lora_a.detach(), lora_b.detach(), dw, w2, s=model.patch_lora_scale, refold=refold)
        ctx.model = model
        ctx.save_for_backward(cols2, lora_a, lora_b)
        return y

    @staticmethod
    def backward(ctx, dy):
        model = ctx.model
        cols2, lora_a, lora_b = ctx.saved_tensors
        own = model._patch_grad_views is not None
        ga, gb = model._patch_grad_views if own else (torch.zeros_like(lora_a), torch.zeros_like(lora_b))
        ops.wan_patch_lora_backward(cols2, dy.reshape(cols2.shape[0], -1).contiguous(), lora_a.detach(), lora_b.detach(), model._patch_ws[2], ga, gb,
                                    s=model.patch_lora_scale)
        if own:
            if model._patch_grad_hook is not None:
                model._patch_grad_hook(model)  # the first trainable thing of the model: its gradients are the last to become final
            return None, None, None, None
        return None, None, ga, gb


class MI355XWanTransformer3DModel(nn.Module):
    def __init__(self, config: Optional[WanTransformerConfig] = None, device: Optional[torch.device] = None):
        super().__init__()
        self.config = c = config or WanTransformerConfig()
        if c.attention_head_dim != 128 or c.qk_norm != "rms_norm_across_heads" or not c.cross_attn_norm:
            raise ValueError("this path covers the Wan2.1 architecture: heads of 128, RMSNorm across heads, cross_attn_norm")
        dev = device or torch.device("cuda", 0)
        self.root_layout = RootLayout(c)
        self.root = nn.Parameter(torch.zeros(self.root_layout.total, dtype=bf16, device=dev), requires_grad=False)
        self.root_grad: Optional[torch.Tensor] = None
        self._root_src: Optional[torch.Tensor] = None  # sharded training: the all-gathered root parameters
        self.blocks = nn.ModuleList([MI355XWanBlock(c.inner_dim, c.num_attention_heads, c.ffn_dim, c.eps, dev, added_kv_proj_dim=c.inner_dim if c.image_dim is not None else None,
                                                    second_image_tokens=c.second_image_tokens)
                                     for _ in range(c.num_layers)])
        self._rope_cache: Dict[Tuple[int, int, int], Tuple[torch.Tensor, torch.Tensor]] = {}
        self._anchor = torch.zeros(1, dtype=bf16, device=dev, requires_grad=True)  # tells autograd that the graph has trainable inputs
        self.lora_config: Optional[Dict[str, object]] = None  # set by add_adapter: {"r", "lora_alpha", "target_modules"}
        self._proj_out_t: Optional[torch.Tensor] = None       # LoRA training: the frozen output projection's K-contiguous twin
        # control LoRA: the full-rank adapter of the (widened) patch embedding, fp32 [r, Kp] / [D, r] with r = D; state-dict shapes are the Conv3d ones
        self.patch_lora_A: Optional[nn.Parameter] = None
        self.patch_lora_B: Optional[nn.Parameter] = None
        self.patch_lora_scale = 0.0
        self._patch_ws: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None  # dW [D, Kp] fp32, its planes [D, 2 Kp] bf16, G [D, Kp] fp32
        self._patch_fold_key, self._patch_epoch = None, 0
        self._patch_grad_views: Optional[Tuple[torch.Tensor, torch.Tensor]] = None  # the step object's flat gradient views
        self._patch_grad_hook = None

    @property
    def device(self) -> torch.device:
        return self.root.device

    # -- parameters ---------------------------------------------------------------------------------------------------------------------------
    def _root_params(self) -> torch.Tensor:
        return self.root.data if self._root_src is None else self._root_src

    def rparam(self, name: str) -> torch.Tensor:
        return self.root_layout.view(self._root_params(), name)

    def rgrad(self, name: str) -> torch.Tensor:
        return self.root_layout.view(self.root_grad, name)

    def zero_grad_flat(self) -> None:
        if self.root_grad is None:
            self.root_grad = torch.zeros(self.root_layout.total, dtype=torch.float32, device=self.device)
        else:
            self.root_grad.zero_()
        for blk in self.blocks:
            blk.zero_grad_flat()

    @torch.no_grad()
    def load_diffusers_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """A diffusers ``WanTransformer3DModel`` state dict."""
        for name, view in self.root_layout.named_views(self.root.data).items():
            view.copy_(sd[name].to(bf16).reshape(view.shape))  # Conv3d weight [D, C, pt, ph, pw] -> [D, C pt ph pw]
        for i, blk in enumerate(self.blocks):
            pre = f"blocks.{i}."
            blk.load_diffusers_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})

    def state_dict_views(self) -> Dict[str, torch.Tensor]:
        """{diffusers parameter name: view of the flat buffers} (the patch embedding in its GEMM shape [D, C pt ph pw])."""
        if self.root.numel() < self.root_layout.total:
            raise RuntimeError("the parameters are sharded over the ranks: use the step object's gathered_state_dict()")
        out = dict(self.root_layout.named_views(self.root.data))
        for i, blk in enumerate(self.blocks):
            out.update({f"blocks.{i}.{k}": v for k, v in blk.state_dict_views().items()})
        return out

    def named_grads(self) -> Dict[str, torch.Tensor]:
        out = dict(self.root_layout.named_views(self.root_grad))
        for i, blk in enumerate(self.blocks):
            out.update({f"blocks.{i}.{k}": v for k, v in blk.named_grads().items()})
        return out

    def flat_units(self):
        """(name, parameter buffer, gradient buffer) of the shardable units: root first, then the blocks."""
        return [("root", self.root.data, self.root_grad)] + [(f"blocks.{i}", b.flat.data, b.grad_flat) for i, b in enumerate(self.blocks)]

    # -- LoRA over the frozen base ------------------------------------------------------------------------------------------------------------
    def linear_module_names(self) -> List[str]:
        """The diffusers names of every module of this model peft could wrap (the Conv3d patch embedding and every Linear), in ``named_modules`` order:
        what a ``target_modules`` is resolved against."""
        c, ce = self.config, "condition_embedder."
        names = ["patch_embedding", ce + "time_embedder.linear_1", ce + "time_embedder.linear_2", ce + "time_proj", ce + "text_embedder.linear_1",
                 ce + "text_embedder.linear_2"]
        if c.image_dim is not None:
            names += [ce + "image_embedder.ff.net.0.proj", ce + "image_embedder.ff.net.2"]
        per_block = list(LORA_TARGETS) + (["attn2.add_k_proj", "attn2.add_v_proj"] if c.image_dim is not None else []) + list(LORA_FFN_TARGETS)
        per_block.sort(key=lambda n: (n.split(".")[0], n))  # (order within a block does not matter to the resolution; keep it stable)
        for i in range(c.num_layers):
            names += [f"blocks.{i}.{n}" for n in per_block]
        return names + ["proj_out"]

    def select_modules(self, target_modules) -> List[str]:
        """peft's rule (tuners_utils.check_target_module_exists): a string is ``re.fullmatch``ed against every module name; a list or tuple selects a name
        that equals an entry or ends with "." + entry."""
        return select_module_names(self.linear_module_names(), target_modules)

    @staticmethod
    def _pattern_lookup(name: str, rank_pattern, alpha_pattern, rank, lora_alpha):
        """peft's per-module override (tuners/lora/model.py, _create_and_replace): the first key of rank_pattern / alpha_pattern with ``.*\\.key$`` matching the
        module name, else the name itself, is looked up in both dictionaries."""
        rank_pattern, alpha_pattern = rank_pattern or {}, alpha_pattern or {}
        key = next((k for k in list(rank_pattern) + list(alpha_pattern) if re.match(rf".*\.{k}$", name)), name)
        return rank_pattern.get(key, rank), alpha_pattern.get(key, lora_alpha)

    def resolve_target_modules(self, target_modules, rank_pattern=None, alpha_pattern=None, rank=None, lora_alpha=None) -> bool:
        """Which adapters ``target_modules`` asks for (``select_modules``).  Accepted sets: the eight attention projections of every block (returns False) or
        those plus ffn.net.0.proj and ffn.net.2 of every block (returns True); either may come with ``patch_embedding`` (the control recipe's
        "(^patch_embedding$)|(...)"; ``patch_adapter_spec`` says whether it does) provided ``rank_pattern`` gives that module the full rank ``inner_dim``.
        Anything else raises, naming the first module that is selected but not covered or covered but not selected: a silently different adapter set is
        impossible.  Note that the reference's Wan control recipe spells the feed-forward members "ff.net.0.proj|ff.net.2", which does not match Wan's
        "ffn.net...": as written it selects the eight, like peft does; and that the list form's appended "^patch_embedding$" is a suffix no name ends with."""
        selected = self.select_modules(target_modules)
        L = self.config.num_layers
        attn = [f"blocks.{i}.{t}" for i in range(L) for t in LORA_TARGETS]
        ffn = [f"blocks.{i}.{t}" for i in range(L) for t in LORA_FFN_TARGETS]
        covered = "this backend places adapters on to_q / to_k / to_v / to_out.0 of both attentions of every block, or on those and ffn.net.0.proj / ffn.net.2 of every block"
        if "patch_embedding" in selected:
            r, alpha = self._pattern_lookup("patch_embedding", rank_pattern, alpha_pattern, rank, lora_alpha)
            if r != self.config.inner_dim or not alpha or float(alpha) <= 0:
                raise NotImplementedError(f"target_modules {target_modules!r} selects patch_embedding; {covered}; a patch_embedding adapter is the control recipe's "
                                          f"full-rank one: rank_pattern must give it r = inner_dim = {self.config.inner_dim} (got {r!r}) and alpha_pattern a positive alpha")
            if self.config.image_dim is not None:
                raise NotImplementedError(f"target_modules {target_modules!r} selects patch_embedding; control on an image-to-video model is not covered")
        extra = [n for n in selected if n not in set(attn) | set(ffn) | {"patch_embedding"}]
        if extra:
            raise NotImplementedError(f"target_modules {target_modules!r} selects {extra[0]}; {covered}")
        blocks = [n for n in selected if n != "patch_embedding"]
        if not blocks:
            raise NotImplementedError(f"target_modules {target_modules!r} selects no module of this model's blocks; {covered}")
        for n in blocks:  # a pattern that reaches into the blocks would give one projection another rank or scale
            if self._pattern_lookup(n, rank_pattern, alpha_pattern, rank, lora_alpha) != (rank, lora_alpha):
                raise NotImplementedError(f"rank_pattern / alpha_pattern change the rank or alpha of {n}; {covered} with ONE rank and alpha")
        sel = set(blocks)
        want = attn + ffn if sel & set(ffn) else attn
        missing = [n for n in want if n not in sel]
        if missing:
            raise NotImplementedError(f"target_modules {target_modules!r} leaves out {missing[0]}; {covered}")
        return bool(sel & set(ffn))

    def patch_adapter_spec(self, target_modules, rank_pattern=None, alpha_pattern=None, rank=None, lora_alpha=None) -> Optional[Tuple[int, float]]:
        """(r, s = alpha / r) of the patch-embedding adapter ``target_modules`` selects (after ``resolve_target_modules`` accepted it), or None."""
        if "patch_embedding" not in self.select_modules(target_modules):
            return None
        r, alpha = self._pattern_lookup("patch_embedding", rank_pattern, alpha_pattern, rank, lora_alpha)
        return int(r), float(alpha) / int(r)

    def expand_patch_embedding(self, new_in_channels: int) -> None:
        """The control specification's widened input layer (models/utils.py: _expand_conv3d_with_zeroed_weights): the patch embedding takes
        ``new_in_channels`` channels, the weight columns of the new channels are zero, ``config.in_channels`` follows.  The root buffer is laid out again."""
        c = self.config
        if self.lora_config is not None:
            raise RuntimeError("expand_patch_embedding comes before add_adapter (the adapter is laid out for the widened layer)")
        if c.image_dim is not None:
            raise NotImplementedError("control on an image-to-video model is not covered (its input already carries mask and conditioning channels)")
        pt, ph, pw = c.patch_size
        if new_in_channels < c.in_channels or (new_in_channels * pt * ph * pw) % 64 != 0:
            raise ValueError(f"new_in_channels {new_in_channels}: at least the present {c.in_channels} channels, and patch columns ({pt * ph * pw} per channel) "
                             "that are a multiple of 64")
        if self.root.numel() < self.root_layout.total or self._root_src is not None:
            raise RuntimeError("the parameters are sharded over the ranks: expand the patch embedding before sharding")
        old_layout, old = self.root_layout, self.root.data
        c.in_channels = int(new_in_channels)
        self.root_layout = RootLayout(c)
        new = torch.zeros(self.root_layout.total, dtype=bf16, device=old.device)
        new_views = self.root_layout.named_views(new)
        for name, view in old_layout.named_views(old).items():
            if name == "patch_embedding.weight":
                new_views[name][:, :view.shape[1]].copy_(view)  # columns are (c, pt, ph, pw): the old channels come first
            else:
                new_views[name].copy_(view)
        self.root = nn.Parameter(new, requires_grad=False)
        self.root_grad, self._proj_out_t = None, None

    def add_adapter(self, rank: int = 32, lora_alpha: float = 32.0, target_modules="blocks.*(to_q|to_k|to_v|to_out.0)", rank_pattern=None, alpha_pattern=None) -> None:
        """``--training_type lora --rank R --lora_alpha A --target_modules ...``: fp32 adapters over a frozen base on what ``target_modules`` selects by peft's
        rule -- the eight attention projections of every block (the Wan SFT recipes' "blocks.*(to_q|to_k|to_v|to_out.0)": attn1 AND attn2, the regex matches
        both), or those and the two feed-forward projections ("blocks.*(to_q|to_k|to_v|to_out.0|ffn.net.0.proj|ffn.net.2)").  ``--training_type control-lora``
        passes "(^patch_embedding$)|(...)" with ``rank_pattern = alpha_pattern = {"patch_embedding": inner_dim}``: the full-rank adapter of the widened patch
        embedding next to the block adapters (A kaiming-uniform(a = sqrt(5)) over its fan-in Cin pt ph pw, B zero, like peft initialises a conv adapter).
        Any other selection raises (``resolve_target_modules``)."""
        ffn = self.resolve_target_modules(target_modules, rank_pattern, alpha_pattern, rank, lora_alpha)
        patch = self.patch_adapter_spec(target_modules, rank_pattern, alpha_pattern, rank, lora_alpha)
        for blk in self.blocks:
            blk.add_adapter(rank, lora_alpha, ffn=ffn)
        self.lora_config = {"r": int(rank), "lora_alpha": lora_alpha, "target_modules": target_modules}
        if rank_pattern:
            self.lora_config["rank_pattern"] = dict(rank_pattern)
        if alpha_pattern:
            self.lora_config["alpha_pattern"] = dict(alpha_pattern)
        if patch is not None:
            r, s = patch
            D, Kp = self.root_layout.offsets["patch_embedding.weight"][1]
            dev = self.device
            a = torch.empty(r, Kp, dtype=torch.float32, device=dev).uniform_(-(1.0 / Kp) ** 0.5, (1.0 / Kp) ** 0.5)  # kaiming_uniform_(a = sqrt(5)): 1 / sqrt(fan_in)
            self.patch_lora_A, self.patch_lora_B = nn.Parameter(a), nn.Parameter(torch.zeros(D, r, dtype=torch.float32, device=dev))
            self.patch_lora_scale = s
            self._patch_ws = (torch.zeros(D, Kp, dtype=torch.float32, device=dev), torch.zeros(D, 2 * Kp, dtype=bf16, device=dev),
                              torch.zeros(D, Kp, dtype=torch.float32, device=dev))
            self._patch_fold_key = None

    def mark_patch_adapter_updated(self) -> None:
        """The patch adapter's parameters were changed in place by the library (the step object's fused optimiser launch): fold again at the next forward."""
        self._patch_epoch += 1

    def _patch_lora_views(self, grads: bool = False) -> Dict[str, torch.Tensor]:
        if self.patch_lora_A is None:
            return {}
        if grads and self._patch_grad_views is not None:
            a, b = self._patch_grad_views
        else:
            a, b = ((self.patch_lora_A.grad, self.patch_lora_B.grad) if grads else (self.patch_lora_A.data, self.patch_lora_B.data))
        pt, ph, pw = self.config.patch_size
        return {"patch_embedding.lora_A.weight": a.view(a.shape[0], self.config.in_channels, pt, ph, pw), "patch_embedding.lora_B.weight": b.view(*b.shape, 1, 1, 1)}

    def lora_parameters(self) -> List[nn.Parameter]:
        """The patch-embedding adapter first (the front of the step object's flat buffers: its gradients are the last to become final), then the blocks'."""
        patch = [self.patch_lora_A, self.patch_lora_B] if self.patch_lora_A is not None else []
        return patch + [p for blk in self.blocks for p in blk.lora_parameters()]

    def lora_state_dict(self) -> Dict[str, torch.Tensor]:
        """peft / diffusers keys ``blocks.{i}.attn{1,2}.to_{q,k,v}.lora_{A,B}.weight`` and ``blocks.{i}.attn{1,2}.to_out.0.lora_{A,B}.weight`` -- with the
        feed-forward adapters also ``blocks.{i}.ffn.net.0.proj.lora_{A,B}.weight`` ([r, D], [F, r]) and ``blocks.{i}.ffn.net.2.lora_{A,B}.weight`` ([r, F],
        [D, r]): views of the user's rank inside the zero-padded storage.  Control LoRA adds ``patch_embedding.lora_A.weight`` [r, Cin, pt, ph, pw] and
        ``patch_embedding.lora_B.weight`` [D, r, 1, 1, 1]."""
        out = self._patch_lora_views()
        out.update({f"blocks.{i}.{k}": v for i, blk in enumerate(self.blocks) for k, v in blk.lora_named_views().items()})
        return out

    def lora_grad_state_dict(self) -> Dict[str, torch.Tensor]:
        """The adapters' gradients under the same keys (after a backward): the step object's flat views, or ``.grad``."""
        out = self._patch_lora_views(grads=True)
        out.update({f"blocks.{i}.{k}": v for i, blk in enumerate(self.blocks) for k, v in blk.lora_named_views(grads=True).items()})
        return out

    @torch.no_grad()
    def load_lora_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        sd = {k.replace(".default.", "."): v for k, v in sd.items()}
        mine = self.lora_state_dict()
        missing, extra = sorted(set(mine) - set(sd)), sorted(set(sd) - set(mine))
        if missing or extra:
            raise KeyError(f"LoRA state dict does not match the attached adapters: missing {missing[:3]}, unexpected {extra[:3]}")
        for k, v in mine.items():
            if tuple(sd[k].shape) != tuple(v.shape):
                raise ValueError(f"{k}: expected shape {tuple(v.shape)}, got {tuple(sd[k].shape)}")
            v.copy_(sd[k].to(v))
        self.mark_patch_adapter_updated()

    def apply_activation_checkpointing(self, checkpointing_type: str = "full", n_layer: int = 1) -> "MI355XWanTransformer3DModel":
        """``--gradient_checkpointing`` (utils/activation_checkpoint.py:24-49) for LoRA training: every block ("block_skip": every ``n_layer``-th) keeps
        only its input and refills its saved activations inside the backward with the identical kernel sequence."""
        if checkpointing_type not in ("full", "block_skip"):
            raise ValueError(f"Checkpointing type '{checkpointing_type}' not supported. Supported types are ['full', 'block_skip']")
        if self.lora_config is None:
            raise NotImplementedError("activation checkpointing covers LoRA training (add_adapter first); the full fine-tune keeps its activations")
        for i, blk in enumerate(self.blocks):
            blk.gradient_checkpointing = checkpointing_type == "full" or i % max(1, int(n_layer)) == 0
        return self

    def _patch_columns(self, hidden_states: torch.Tensor) -> torch.Tensor:
        """Conv3d(kernel = stride = patch) as a GEMM: the patch columns (c, pt, ph, pw) of every token in (f, h, w) order, zero-padded to the stored width."""
        B, C, F_, H, W = hidden_states.shape
        pt, ph, pw = self.config.patch_size
        f, h, w = F_ // pt, H // ph, W // pw
        cols = hidden_states.to(bf16).view(B, C, f, pt, h, ph, w, pw).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, f * h * w, C * pt * ph * pw)
        pad = self.root_layout.offsets["patch_embedding.weight"][1][1] - cols.shape[-1]
        return torch.nn.functional.pad(cols, (0, pad)) if pad else cols

    @torch.no_grad()
    def _embed_image(self, image_embeds: torch.Tensor) -> torch.Tensor:
        """``condition_embedder.image_embedder`` on [B, TI, image_dim] (frozen; B x 257 rows once per step, plain torch ops at the reference's rounding
        points): FP32LayerNorm -> Linear -> exact GELU -> Linear -> FP32LayerNorm.

        First/last-frame (``config.pos_embed_seq_len`` = P, two images of P / 2 tokens): [upstream] WanImageEmbedding.forward first views its input as
        [-1, P, image_dim] and adds ``pos_embed`` in the model's dtype, x = bf(x + pos_embed).  Accepted are therefore [B, P, image_dim] (a sample's first
        image, then its last) and [2B, P / 2, image_dim], whose rows 2b and 2b + 1 the view pairs as sample b; the result is [B, P, D] either way.  NOTE: the
        reference's processor stacks ALL first frames and then ALL last frames (finetrainers/models/wan/base_specification.py:201, ``torch.stack([image, last_image], dim=0)``),
        which agrees with this pairing only at batch size 1 -- the recipe's batch.  The rows are taken as upstream takes them; nothing is reordered here."""
        F_, ie = torch.nn.functional, "condition_embedder.image_embedder."
        P = lambda n: self.rparam(ie + n)
        x = image_embeds.to(self.device, bf16)
        if x.dim() != 3 or x.shape[-1] != self.config.image_dim:
            raise ValueError(f"encoder_hidden_states_image must be [B, tokens, {self.config.image_dim}]")
        n_pos = self.config.pos_embed_seq_len
        if n_pos is None:
            if x.shape[1] > 320:
                raise NotImplementedError("the image context of a model without pos_embed_seq_len holds at most 320 tokens (257 CLIP tokens of one image)")
        else:
            if x.shape[1] != n_pos and not (2 * x.shape[1] == n_pos and x.shape[0] % 2 == 0):
                raise ValueError(f"first/last-frame image embedder: got {x.shape[1]} tokens per row, pos_embed_seq_len is {n_pos} "
                                 f"([B, {n_pos}, image_dim] or [2B, {n_pos // 2}, image_dim])")
            x = x.reshape(-1, n_pos, x.shape[-1]) + P("pos_embed")  # bf16 + bf16: one rounding, as upstream
        ln = lambda t, n: F_.layer_norm(t.float(), (t.shape[-1],), P(n + ".weight").float(), P(n + ".bias").float(), 1e-5).to(bf16)
        x = F_.gelu(F_.linear(ln(x, "norm1"), P("ff.net.0.proj.weight"), P("ff.net.0.proj.bias")))
        return ln(F_.linear(x, P("ff.net.2.weight"), P("ff.net.2.bias")), "norm2").contiguous()

    def _forward_frozen_root(self, hidden_states, timestep, encoder_hidden_states, return_dict: bool, encoder_hidden_states_image=None, patch_columns=None,
                             latent_shape=None):
        """The forward with adapters attached: patch embedding, condition embedder and head run FROZEN (plain launches of the same GEMMs: same bits as the
        full fine-tune's forward); the only graph autograd sees is blocks -> output norm -> output projection, which hands d x back to the last block."""
        c = self.config
        B, F_, H, W = latent_shape if hidden_states is None else (hidden_states.shape[0],) + tuple(hidden_states.shape[2:])
        pt, ph, pw = c.patch_size
        f, h, w = F_ // pt, H // ph, W // pw
        S = f * h * w
        rope = self._rope(F_, H, W)
        lin = lambda t, name, **kw: ops.gemm_nt(t.reshape(-1, t.shape[-1]), self.rparam(f"{name}.weight"), self.rparam(f"{name}.bias"), **kw)
        silu = torch.nn.functional.silu
        if self.patch_lora_A is not None:  # the first trainable thing of the frozen root: block 0's dx comes back to it
            if patch_columns is None:
                cols = self._patch_columns(hidden_states)
                patch_columns = torch.cat([cols, cols], dim=-1).view(B * S, -1)
            x = _PatchLoRAFunction.apply(self, patch_columns, self.patch_lora_A, self.patch_lora_B).view(B, S, -1)
        with torch.no_grad():
            if self.patch_lora_A is None:
                cols = self._patch_columns(hidden_states) if patch_columns is None else patch_columns[:, :patch_columns.shape[1] // 2]
                x = lin(cols, "patch_embedding").view(B, S, -1)
            t_emb = timestep_embedding(timestep.to(self.device), c.freq_dim).to(bf16)
            temb = lin(silu(lin(t_emb, "condition_embedder.time_embedder.linear_1")), "condition_embedder.time_embedder.linear_2")
            tproj = lin(silu(temb), "condition_embedder.time_proj").unflatten(1, (6, -1))
            text = encoder_hidden_states.to(bf16)
            act, _ = lin(text, "condition_embedder.text_embedder.linear_1", epilogue=1, want_out2=True)  # (the full fine-tune's launch, pre-activation and all)
            enc = lin(act, "condition_embedder.text_embedder.linear_2").view(B, text.shape[1], -1)
            mod = self.rparam("scale_shift_table") + temb.unsqueeze(1)  # [B, 2, D] bf16
            shift, scale = mod[:, 0].float(), (1 + mod[:, 1]).float() - 1
            enc_img = None if encoder_hidden_states_image is None else self._embed_image(encoder_hidden_states_image)
            if enc_img is not None and enc_img.shape[0] != B:  # (the blocks read B rows of it: a [2B', L] input of a first/last-frame model makes B' rows)
                raise ValueError(f"encoder_hidden_states_image {tuple(encoder_hidden_states_image.shape)} makes {enc_img.shape[0]} image rows of {enc_img.shape[1]} tokens "
                                 f"for a batch of {B}" + ("" if c.pos_embed_seq_len is None else
                                                          f" (pos_embed_seq_len {c.pos_embed_seq_len}: [B, {c.pos_embed_seq_len}, image_dim] or [2B, {c.pos_embed_seq_len // 2}, image_dim])"))
        for blk in self.blocks:
            x = blk(x, enc, tproj, rope, enc_img)
        y = _LnModFunction.apply(x, shift, scale, c.eps)
        if self._proj_out_t is None:
            self._proj_out_t = ops.transpose_bf16(self.rparam("proj_out.weight"))
        y = _FrozenLinearFunction.apply(y, self.rparam("proj_out.weight"), self.rparam("proj_out.bias"), self._proj_out_t)
        out = y.reshape(B, f, h, w, pt, ph, pw, -1).permute(0, 7, 1, 4, 2, 5, 3, 6).reshape(B, -1, F_, H, W)
        return {"sample": out} if return_dict else (out,)

    # -- forward ------------------------------------------------------------------------------------------------------------------------------
    def _rope(self, frames: int, height: int, width: int):
        key = (frames, height, width)
        if key not in self._rope_cache:
            self._rope_cache[key] = tuple(t.to(self.device) for t in rotary_tables(self.config, frames, height, width))
        return self._rope_cache[key]

    def _linear(self, x, name: str, gelu: bool = False, need_dx: bool = True):
        if self.root_grad is None:
            self.zero_grad_flat()
        w, b = self.rparam(f"{name}.weight"), self.rparam(f"{name}.bias")
        return _LinearFunction.apply(x, w, b, self.rgrad(f"{name}.weight"), self.rgrad(f"{name}.bias"), gelu, need_dx, self._anchor)

    def forward(self, hidden_states, timestep, encoder_hidden_states, encoder_hidden_states_image=None, return_dict: bool = False, patch_columns=None,
                latent_shape=None, **kwargs):
        """``patch_columns`` (LoRA training of a control model): the patch embedding's GEMM operand [B S, 2 Kp] = [cols | cols] as ``ops.wan_control_pack``
        writes it, in place of ``hidden_states`` (then None, with ``latent_shape`` = (B, F, H, W) of the latents).  ``encoder_hidden_states_image``
        (image-to-video): the CLIP tokens [B, TI, image_dim]; of a first/last-frame model (``config.pos_embed_seq_len``) [B, TI + TI2, image_dim] or
        [2B, TI, image_dim], see ``_embed_image`` -- every block's attn2 then attends to TI + TI2 = pos_embed_seq_len image keys."""
        c = self.config
        if (encoder_hidden_states_image is not None) != (c.image_dim is not None):
            raise NotImplementedError("encoder_hidden_states_image goes with an image-to-video model (config.image_dim), and such a model needs it")
        if patch_columns is not None:
            if self.lora_config is None or c.image_dim is not None:
                raise NotImplementedError("patch_columns is the control LoRA path: a text-to-video model with adapters attached")
            if hidden_states is not None or latent_shape is None or len(latent_shape) != 4:
                raise ValueError("patch_columns replaces hidden_states (pass None) and needs latent_shape = (B, F, H, W)")
            pt, ph, pw = c.patch_size
            B, F_, H, W = latent_shape
            want = (B * (F_ // pt) * (H // ph) * (W // pw), 2 * self.root_layout.offsets["patch_embedding.weight"][1][1])
            if tuple(patch_columns.shape) != want or patch_columns.dtype != bf16 or not patch_columns.is_contiguous():
                raise ValueError(f"patch_columns must be a contiguous bf16 {want} tensor ([cols | cols]), got {tuple(patch_columns.shape)}")
        elif hidden_states.shape[1] != c.in_channels:
            raise ValueError(f"hidden_states has {hidden_states.shape[1]} channels, the model takes {c.in_channels}")
        if self.lora_config is not None:
            return self._forward_frozen_root(hidden_states, timestep, encoder_hidden_states, return_dict, encoder_hidden_states_image, patch_columns, latent_shape)
        if c.image_dim is not None:
            raise NotImplementedError("Wan image-to-video: full fine-tuning is not covered by this backend; attach adapters first (add_adapter: LoRA training)")
        B, C, F_, H, W = hidden_states.shape
        pt, ph, pw = c.patch_size
        f, h, w = F_ // pt, H // ph, W // pw
        D, S = c.inner_dim, f * h * w
        rope = self._rope(F_, H, W)
        # Conv3d(kernel = stride = patch) as a GEMM over the patch columns (c, pt, ph, pw), tokens in (f, h, w) order
        x = self._linear(self._patch_columns(hidden_states), "patch_embedding", need_dx=False)
        # condition embedder, the reference's patched forward (patches/models/wan/patch.py:17-33): the sinusoid takes the text dtype
        t_emb = timestep_embedding(timestep.to(self.device), c.freq_dim).to(bf16)
        temb = self._linear(torch.nn.functional.silu(self._linear(t_emb, "condition_embedder.time_embedder.linear_1", need_dx=False)),
                            "condition_embedder.time_embedder.linear_2")
        tproj = self._linear(torch.nn.functional.silu(temb), "condition_embedder.time_proj").unflatten(1, (6, -1))
        enc = self._linear(self._linear(encoder_hidden_states.to(bf16), "condition_embedder.text_embedder.linear_1", gelu=True, need_dx=False),
                           "condition_embedder.text_embedder.linear_2")
        for blk in self.blocks:
            x = blk(x, enc, tproj, rope)
        # output: (scale_shift_table + temb) in bf16, (1 + scale) in bf16, the normalised tokens in fp32
        table = self.rparam("scale_shift_table")
        mod = _TableAdd.apply(table, temb.unsqueeze(1), self.rgrad("scale_shift_table"))  # [B, 2, D] bf16
        shift, onep = mod[:, 0], 1 + mod[:, 1]
        y = _LnModFunction.apply(x, shift.float(), onep.float() - 1, c.eps)  # 1 + (onep - 1) is exact: the kernel multiplies by bf(1 + scale)
        y = self._linear(y, "proj_out")
        out = y.reshape(B, f, h, w, pt, ph, pw, -1).permute(0, 7, 1, 4, 2, 5, 3, 6).reshape(B, -1, F_, H, W)
        return {"sample": out} if return_dict else (out,)


class _TableAdd(torch.autograd.Function):
    """table (bf16 parameter view [1, 2, D]) + temb [B, 1, D] in bf16; the table's gradient (sum over the samples) goes to its fp32 gradient slice."""

    @staticmethod
    def forward(ctx, table, temb, gtable):
        ctx.gtable = gtable
        return table + temb

    @staticmethod
    def backward(ctx, d):
        ctx.gtable.add_(d.float().sum(0, keepdim=True))
        return None, d.sum(1, keepdim=True), None
