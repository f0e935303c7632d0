"""Attention-provider plugin for the MI355X kernels.

Mirror of the reference's operator plugin point (finetrainers/models/attention_dispatch.py): the same
registry class, decorator, context manager and ``attention_dispatch(query, key, value, attn_mask, dropout_p,
is_causal, scale, enable_gqa, attention_kwargs)`` entry, with the provider ``mi355x`` that runs ``ftmi_attn_fwd`` / ``ftmi_attn_bwd`` and its
inference-only sibling ``mi355x_sage`` (``ftmi_attn_fwd_q8``: int8 scores, fp8 weights; the reference's ``--attn_provider_inference transformer:sage``).  The reference's other providers (flash / sage / xformers / flex / ATen
variants) are deliberately absent: no multi-backend dispatch.  With the reference installed, the same function is
registered into ITS registry by ``register_into_finetrainers()``, after which
``--attn_provider_training transformer:mi355x`` selects it for an unmodified diffusers model.

Context parallelism (``context_parallel(cp_mesh)`` here; ``attention_provider(..., mesh=cp_mesh)`` of the reference's registry, where the provider is
registered with ``supports_cp=True``; the reference's parallel/ptd.py:502-709 with ``rotate_method="allgather"``): K and V are
all-gathered over the mesh and the ranks' chunks are walked by ``ftmi_attn_fwd_carry``, a forward that continues an fp32 softmax state from chunk to chunk.
``chunked_attention`` is that walk over lists of key / value chunks on one device.

Layout contract (docs/models/attention.md:118): query/key/value ``[B, heads, S, head_dim]``, any strides with a
contiguous head_dim; returns ``[B, heads, S_q, head_dim]`` in the input dtype; differentiable.
"""

from __future__ import annotations

import contextlib
import inspect
import os
from enum import Enum
from typing import Any, Callable, Dict, List, Optional

import torch

from . import ops

# finetrainers/constants.py:7-8
FINETRAINERS_ATTN_PROVIDER = os.environ.get("FINETRAINERS_ATTN_PROVIDER", "mi355x")
FINETRAINERS_ATTN_CHECKS = os.getenv("FINETRAINERS_ATTN_CHECKS", "0") in {"1", "ON", "YES", "TRUE"}


class AttentionProvider(str, Enum):
    MI355X = "mi355x"
    MI355X_SAGE = "mi355x_sage"  # inference only: int8 scores, fp8 weights (the reference's --attn_provider_inference transformer:sage, which is CUDA-only)


class _AttentionProviderRegistry:
    """attention_dispatch.py:295-362."""

    _providers: Dict[AttentionProvider, Callable] = {}
    _constraints: Dict[AttentionProvider, List[Callable]] = {}
    _supports_cp: Dict[AttentionProvider, bool] = {}
    _supported_arg_names: Dict[AttentionProvider, set] = {}

    _active_provider = AttentionProvider(FINETRAINERS_ATTN_PROVIDER)
    _checks_enabled = FINETRAINERS_ATTN_CHECKS

    # context-parallel attributes (attention_dispatch.py:304-307), set by context_parallel(mesh)
    _mesh = None
    _convert_to_fp32: Optional[bool] = None
    _rotate_method: Optional[str] = None

    @classmethod
    def register(cls, provider: AttentionProvider, constraints: Optional[List[Callable]] = None, supports_cp: bool = False):
        def decorator(func):
            cls._providers[provider] = func
            cls._constraints[provider] = constraints or []
            cls._supports_cp[provider] = supports_cp
            cls._supported_arg_names[provider] = set(inspect.signature(func).parameters.keys())
            return func

        return decorator

    @classmethod
    def get_active_provider(cls):
        return cls._active_provider, cls._providers[cls._active_provider]

    @classmethod
    def list_providers(cls):
        return list(cls._providers.keys())

    @classmethod
    def supports_context_parallel(cls, provider: AttentionProvider):
        if provider not in cls._providers:
            raise ValueError(f"Provider {provider} is not registered.")
        return cls._supports_cp.get(provider, False)

    @classmethod
    def context_parallel_enabled(cls):
        return cls._mesh is not None


@contextlib.contextmanager
def attention_provider(provider: AttentionProvider = AttentionProvider.MI355X, *, mesh=None, convert_to_fp32: bool = True,
                       rotate_method: str = "allgather"):
    """attention_dispatch.py:365-402."""
    if provider not in _AttentionProviderRegistry._providers:
        raise ValueError(f"Provider {provider} is not registered.")
    if mesh is not None and not _AttentionProviderRegistry.supports_context_parallel(provider):
        raise ValueError(f"Provider {provider} does not support context parallelism.")
    old = _AttentionProviderRegistry._active_provider
    _AttentionProviderRegistry._active_provider = provider
    try:
        yield
    finally:
        _AttentionProviderRegistry._active_provider = old


@contextlib.contextmanager
def context_parallel(mesh, *, convert_to_fp32: bool = True, rotate_method: str = "allgather"):
    """Inside this region the mi355x provider attends each rank's query shard to the keys of every rank of ``mesh`` (a one-dimensional ``DeviceMesh`` or a
    process group; equal shards): what ``attention_provider(provider, mesh=...)`` of the REFERENCE's registry switches on once the provider is registered
    there with ``supports_cp=True`` (``register_into_finetrainers``).  The mirror registry's own ``attention_provider`` keeps refusing a mesh."""
    _cp_group(mesh)  # refuses what is neither a 1-D DeviceMesh nor a process group
    _check_rotate_method(rotate_method)
    reg = _AttentionProviderRegistry
    old = (reg._mesh, reg._convert_to_fp32, reg._rotate_method)
    reg._mesh, reg._convert_to_fp32, reg._rotate_method = mesh, convert_to_fp32, rotate_method
    try:
        yield
    finally:
        reg._mesh, reg._convert_to_fp32, reg._rotate_method = old


def attention_dispatch(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, attn_mask: Optional[torch.Tensor] = None,
                       dropout_p: float = 0.0, is_causal: bool = False, scale: Optional[float] = None, enable_gqa: bool = False,
                       attention_kwargs: Optional[Dict[str, Any]] = None) -> torch.Tensor:
    """attention_dispatch.py:405-447."""
    attention_kwargs = attention_kwargs or {}
    provider_name, provider_fn = _AttentionProviderRegistry.get_active_provider()
    kwargs = {"query": query, "key": key, "value": value, "attn_mask": attn_mask, "dropout_p": dropout_p, "is_causal": is_causal,
              "scale": scale, "enable_gqa": enable_gqa, **attention_kwargs}
    if _AttentionProviderRegistry._checks_enabled:
        for check in _AttentionProviderRegistry._constraints.get(provider_name):
            check(**kwargs)
    kwargs = {k: v for k, v in kwargs.items() if k in _AttentionProviderRegistry._supported_arg_names[provider_name]}
    return provider_fn(**kwargs)


# ---- constraint helpers (same style as attention_dispatch.py:460-519: raise ValueError) ------------------------


def _check_device_gpu(query, key, value, **kwargs) -> None:
    if not (query.is_cuda and key.is_cuda and value.is_cuda):
        raise ValueError("Query, key, and value must be on the GPU for the mi355x provider.")


def _check_qkv_dtype_bf16(query, key, value, **kwargs) -> None:
    if not (query.dtype == key.dtype == value.dtype == torch.bfloat16):
        raise ValueError("Query, key, and value must be bfloat16 for the mi355x provider.")


def _check_head_dim(query, key, value, **kwargs) -> None:
    d = query.shape[-1]
    if d not in (64, 128) or key.shape[-1] != d or value.shape[-1] != d:
        raise ValueError("The mi355x provider is built for head_dim 64 (LTX-Video, CogVideoX) and 128 (Wan, HunyuanVideo).")


def _check_no_dropout_causal_gqa(dropout_p=0.0, is_causal=False, enable_gqa=False, **kwargs) -> None:
    if dropout_p != 0.0 or is_causal or enable_gqa:
        raise ValueError("The mi355x provider supports non-causal attention without dropout or GQA.")


# -inf (and bool masks, which mean -inf) travel as a large finite negative: exp2 of it is exactly 0 for every kept key, and a row whose
# keys are ALL masked stays finite (uniform over the masked keys) instead of producing NaN in a training step
_MASKED = -1.0e30


def _key_bias_from_mask(attn_mask: Optional[torch.Tensor], B: int, H: int, Sk: int) -> Optional[torch.Tensor]:
    """``attn_mask`` in torch SDPA's convention -- bool (True = keep) or additive float, broadcastable to [B, H, S_q, S_k] with
    right-aligned dimensions -- whose value does not depend on the query (LTX's text mask is [B, H, 1, T]) -> fp32 key
    bias [B, S_k] (one row per sample) or [B, H, S_k] (the mask differs between heads).  Anything else raises ``ValueError``."""
    if attn_mask is None:
        return None
    m = attn_mask
    if m.dim() > 4:
        raise ValueError("mi355x provider: attn_mask has more than 4 dimensions")
    while m.dim() < 4:  # torch aligns mask dimensions to the right: [L, S] -> [1, 1, L, S], [X, L, S] -> [1, X, L, S] (X = heads)
        m = m.unsqueeze(0)
    if m.shape[-1] != Sk or m.shape[2] != 1 or m.shape[0] not in (1, B) or m.shape[1] not in (1, H):
        raise ValueError(f"mi355x provider: attn_mask {tuple(attn_mask.shape)} must broadcast to [B={B}, H={H}, 1, S_k={Sk}] (no per-query masks)")
    if m.shape[1] == 1 or m.stride(1) == 0:  # one mask for all heads (also an expanded view of one)
        m = m[:, :1]
    if m.dtype == torch.bool:
        m = torch.zeros(m.shape, dtype=torch.float32, device=m.device).masked_fill(~m, _MASKED)
    else:
        m = m.float().clamp_min(_MASKED)
    m = m[:, :, 0]  # [B|1, H|1, Sk]
    if m.shape[1] == 1:
        return m[:, 0].expand(B, Sk).contiguous()
    return m.expand(B, H, Sk).contiguous()  # a mask materialised per head is honoured per head, not reduced to head 0


class _MI355XAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query, key, value, key_bias, scale):
        out, lse = ops.attn_fwd(query, key, value, key_bias, scale)
        ctx.save_for_backward(query, key, value, out, lse, key_bias if key_bias is not None else torch.empty(0, device=query.device))
        ctx.has_bias = key_bias is not None
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        query, key, value, out, lse, key_bias = ctx.saved_tensors
        dq, dk, dv = ops.attn_bwd(query, key, value, out, lse, dout, key_bias if ctx.has_bias else None, ctx.scale)
        return dq, dk, dv, None, None


# ---- attention over a list of key / value chunks: one carried-softmax launch per chunk (csrc/attn_carry.hip) ----------------------------------


class _ChunkedAttention(torch.autograd.Function):
    """args = keys (n), values (n), key biases (n, each a tensor or None).  Forward: the fp32 state (acc, lse) walks the chunks in place and bf16(acc) is
    written with the last one.  Backward: ``ftmi_attn_bwd`` per chunk with the FINAL out and lse gives that chunk's dK / dV and its share of dQ, which is
    summed in fp32."""

    @staticmethod
    def forward(ctx, query, scale, n, *args):
        keys, values, biases = args[:n], args[n:2 * n], args[2 * n:]
        B, H, Sq, d = query.shape
        acc = torch.empty((B, H, Sq, d), dtype=torch.float32, device=query.device)
        lse = torch.empty((B, H, Sq), dtype=torch.float32, device=query.device)
        out = None
        for c in range(n):
            out = ops.attn_fwd_carry(query, keys[c], values[c], acc, lse, key_bias=biases[c], scale=scale, first=c == 0, last=c == n - 1)
        ctx.save_for_backward(query, out, lse, *keys, *values, *(b for b in biases if b is not None))
        ctx.n, ctx.scale, ctx.has_bias = n, scale, [b is not None for b in biases]
        return out

    @staticmethod
    def backward(ctx, dout):
        n = ctx.n
        query, out, lse = ctx.saved_tensors[:3]
        keys, values = ctx.saved_tensors[3:3 + n], ctx.saved_tensors[3 + n:3 + 2 * n]
        saved_biases = iter(ctx.saved_tensors[3 + 2 * n:])
        dq_sum = torch.zeros(query.shape, dtype=torch.float32, device=query.device)
        dq, dks, dvs = None, [], []
        for c in range(n):
            bias = next(saved_biases) if ctx.has_bias[c] else None
            dq_c, dk, dv = ops.attn_bwd(query, keys[c], values[c], out, lse, dout, bias, ctx.scale)
            dq = ops.accum_bf16(dq_sum, dq_c, last=c == n - 1)
            dks.append(dk)
            dvs.append(dv)
        return (dq, None, None, *dks, *dvs, *([None] * n))


def chunked_attention(query: torch.Tensor, keys: List[torch.Tensor], values: List[torch.Tensor], key_biases: Optional[List[Optional[torch.Tensor]]] = None,
                      scale: Optional[float] = None) -> torch.Tensor:
    """softmax(q [k_0 | k_1 | ...]^T scale + bias) [v_0 | v_1 | ...] for key / value chunks that live in separate tensors on one device, without
    concatenating them: query [B, H, Sq, d], keys[c] / values[c] [B, H, Sk_c, d] (bf16, head_dim 64 or 128 contiguous), key_biases[c] None or fp32
    [B, Sk_c] / [B, H, Sk_c].  Differentiable in query, keys and values; the result does not depend on the order of the chunks beyond summation order."""
    n = len(keys)
    if n == 0 or len(values) != n or (key_biases is not None and len(key_biases) != n):
        raise ValueError("chunked_attention: keys, values and key_biases must be lists of the same non-zero length")
    biases = list(key_biases) if key_biases is not None else [None] * n
    return _ChunkedAttention.apply(query, scale, n, *keys, *values, *biases)


# ---- context parallelism: the reference's templated ring attention with rotate_method="allgather" (parallel/ptd.py:502-709) ---------------------


def _check_rotate_method(rotate_method: Optional[str]) -> None:
    if rotate_method != "allgather":
        raise ValueError(f'mi355x provider: context parallelism gathers the key / value chunks (rotate_method="allgather"); "{rotate_method}" is not supported')


def _cp_group(mesh):
    """The process group of a context-parallel mesh: a 1-D ``DeviceMesh`` (the reference's ``cp`` sub-mesh) or a process group itself."""
    import torch.distributed as dist

    if dist.is_available():
        if isinstance(mesh, dist.ProcessGroup):
            return mesh
        if isinstance(mesh, dist.device_mesh.DeviceMesh) and mesh.ndim == 1:
            return mesh.get_group()
    raise ValueError("mi355x provider: the context-parallel mesh must be a one-dimensional DeviceMesh or a process group")


def _gather_chunks(x: torch.Tensor, group) -> List[torch.Tensor]:
    import torch.distributed as dist

    x = x.contiguous()
    chunks = [torch.empty_like(x) for _ in range(dist.get_world_size(group))]
    dist.all_gather(chunks, x, group=group)
    return chunks


def _reduce_to_owners(grads: List[torch.Tensor], group) -> torch.Tensor:
    """grads[r] is this rank's contribution to rank r's tensor: the sum over the ranks of grads[own rank].  One reduce-scatter; gloo has none, so there
    each chunk is reduced to its owner in turn."""
    import torch.distributed as dist

    rank = dist.get_rank(group)
    if dist.get_backend(group) != "gloo":
        mine = torch.empty_like(grads[rank])
        dist.reduce_scatter(mine, grads, group=group)
        return mine
    grads = [g.clone() for g in grads]  # reduce works in place, and leaves the other ranks' copies undefined
    for r, g in enumerate(grads):
        dist.reduce(g, dst=dist.get_global_rank(group, r), group=group)
    return grads[rank]


class _GatherSequence(torch.autograd.Function):
    """This rank's [B, H, S / N, d] shard -> the N ranks' shards, as a tuple in rank order.  Backward: every rank holds a gradient for every shard; each
    shard's gradients are summed onto its owner (in fp32 with ``convert_to_fp32``, as the reference's ring backward accumulates them)."""

    @staticmethod
    def forward(ctx, x, group, convert_to_fp32):
        ctx.group, ctx.fp32 = group, convert_to_fp32
        return tuple(_gather_chunks(x, group))

    @staticmethod
    def backward(ctx, *grads):
        dtype = grads[0].dtype
        grads = [g.to(dtype=torch.float32 if ctx.fp32 else dtype, memory_format=torch.contiguous_format) for g in grads]
        return _reduce_to_owners(grads, ctx.group).to(dtype), None, None


def context_parallel_attention(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, key_bias: Optional[torch.Tensor], scale: Optional[float],
                               group, convert_to_fp32: bool = True) -> torch.Tensor:
    """Attention of this rank's query shard over the keys of every rank of ``group``: K, V (and the key bias) are all-gathered, and the chunks are walked
    starting with the rank's own, the softmax state carried in fp32 from chunk to chunk."""
    import torch.distributed as dist

    world, rank = dist.get_world_size(group), dist.get_rank(group)
    order = [(rank + j) % world for j in range(world)]
    ks = _GatherSequence.apply(key, group, convert_to_fp32)
    vs = _GatherSequence.apply(value, group, convert_to_fp32)
    bs = _gather_chunks(key_bias, group) if key_bias is not None else None
    return chunked_attention(query, [ks[r] for r in order], [vs[r] for r in order], [bs[r] for r in order] if bs is not None else None, scale)


_ref_registry = None  # the reference's registry once register_into_finetrainers() has run: its attention_provider(mesh=...) sets the mesh THERE


def _context_parallel_state():
    """(process group, convert_to_fp32) of the active context-parallel region, or None outside one."""
    for reg in (_AttentionProviderRegistry, _ref_registry):
        if reg is not None and getattr(reg, "_mesh", None) is not None:
            _check_rotate_method(reg._rotate_method)
            return _cp_group(reg._mesh), bool(reg._convert_to_fp32)
    return None


@_AttentionProviderRegistry.register(
    AttentionProvider.MI355X,
    constraints=[_check_device_gpu, _check_qkv_dtype_bf16, _check_head_dim, _check_no_dropout_causal_gqa],
    supports_cp=False,  # about THIS registry's attention_provider(mesh=...); the mesh path is entered through context_parallel() or the reference's registry
)
def _mi355x_attention(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, attn_mask: Optional[torch.Tensor] = None,
                      dropout_p: float = 0.0, is_causal: bool = False, scale: Optional[float] = None, enable_gqa: bool = False) -> torch.Tensor:
    if dropout_p != 0.0 or is_causal or enable_gqa:
        raise ValueError("mi355x provider: dropout, causal masking and GQA are not supported")
    B, H, _, _ = query.shape
    key_bias = _key_bias_from_mask(attn_mask, B, H, key.shape[2])
    cp = _context_parallel_state()
    if cp is not None:
        return context_parallel_attention(query, key, value, key_bias, scale, cp[0], cp[1])
    return _MI355XAttention.apply(query, key, value, key_bias, scale)


@_AttentionProviderRegistry.register(
    AttentionProvider.MI355X_SAGE,
    constraints=[_check_device_gpu, _check_qkv_dtype_bf16, _check_head_dim, _check_no_dropout_causal_gqa],
    supports_cp=False,
)
def _mi355x_sage_attention(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, attn_mask: Optional[torch.Tensor] = None,
                           dropout_p: float = 0.0, is_causal: bool = False, scale: Optional[float] = None, enable_gqa: bool = False) -> torch.Tensor:
    """The sage providers' place (attention_dispatch.py:1651-1760): ``ftmi_attn_fwd_q8``.  Forward only -- there is no backward kernel, so a call that
    autograd would have to differentiate is refused instead of returning a result without a graph."""
    if dropout_p != 0.0 or is_causal or enable_gqa:
        raise ValueError("mi355x_sage provider: dropout, causal masking and GQA are not supported")
    if torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad):
        raise ValueError("mi355x_sage provider: inference only (no backward); call it under torch.no_grad() or use the mi355x provider for training")
    B, H, _, _ = query.shape
    return ops.attn_fwd_q8(query, key, value, _key_bias_from_mask(attn_mask, B, H, key.shape[2]), scale)


def register_into_finetrainers() -> bool:
    """Register the provider into the reference's own registry when finetrainers is importable (it needs an
    ``AttentionProvider`` enum member named MI355X = "mi355x").  Returns False when the reference is
    not installed (this container) -- the mirror registry above is then the only one."""
    try:
        from finetrainers.models import attention_dispatch as ref  # type: ignore
    except Exception:
        return False
    member = getattr(ref.AttentionProvider, "MI355X", None)
    if member is None:
        raise RuntimeError('finetrainers.models.attention_dispatch.AttentionProvider lacks MI355X = "mi355x" (INTEGRATION.md step 1)')
    ref._AttentionProviderRegistry.register(member, constraints=[_check_device_gpu, _check_qkv_dtype_bf16, _check_head_dim], supports_cp=True)(
        _mi355x_attention
    )
    sage = getattr(ref.AttentionProvider, "MI355X_SAGE", None)  # optional: registered only where the reference's enum has the member
    if sage is not None:
        ref._AttentionProviderRegistry.register(sage, constraints=[_check_device_gpu, _check_qkv_dtype_bf16, _check_head_dim], supports_cp=False)(
            _mi355x_sage_attention
        )
    global _ref_registry
    _ref_registry = ref._AttentionProviderRegistry
    return True
