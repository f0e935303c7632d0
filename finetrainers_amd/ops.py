"""Thin tensor-level wrappers over the C ABI (include/ftmi355.h).  torch.Tensor in, torch.Tensor out;
all compute happens inside libftmi355 on the current HIP stream.  No CPU / eager fallbacks."""

from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import AttnDesc, check, ptr, require_gpu_tensor, stream_ptr

bf16 = torch.bfloat16


def _strides3(t: torch.Tensor) -> Tuple[int, int, int]:
    """[B, H, S, d] tensor (any strides, d contiguous) -> (batch, head, token) element strides."""
    if t.dim() != 4 or t.stride(3) != 1:
        raise ValueError("attention tensors must be [B, H, S, d] with contiguous head_dim")
    return (t.stride(0), t.stride(1), t.stride(2))


def _desc(q, k, v, o, scale, dout=None, dq=None, dk=None, dv=None, key_bias=None) -> AttnDesc:
    B, H, Sq, d = q.shape
    Sk = k.shape[2]
    if d not in (64, 128):
        raise ValueError(f"mi355x attention supports head_dim 64 and 128, got {d}")
    if k.shape != (B, H, Sk, d) or v.shape != (B, H, Sk, d):
        raise ValueError("mi355x attention: key/value shapes must be [B, H, Sk, head_dim] (no GQA)")
    desc = AttnDesc()
    desc.B, desc.H, desc.Sq, desc.Sk, desc.d = B, H, Sq, Sk, d
    desc.scale = float(scale)
    if key_bias is not None:
        if key_bias.shape not in ((B, Sk), (B, H, Sk)) or key_bias.stride(-1) != 1:
            raise ValueError("key_bias must be fp32 [B, Sk] or [B, H, Sk] with contiguous keys")
        desc.bias_strides[0] = key_bias.stride(0)
        desc.bias_strides[1] = key_bias.stride(1) if key_bias.dim() == 3 else 0
    for name, t in (("q_strides", q), ("k_strides", k), ("v_strides", v), ("o_strides", o), ("do_strides", dout),
                    ("dq_strides", dq), ("dk_strides", dk), ("dv_strides", dv)):
        if t is not None:
            s = _strides3(t)
            arr = getattr(desc, name)
            arr[0], arr[1], arr[2] = s
    return desc


def _placed(t: Optional[torch.Tensor], shape, name: str, like: torch.Tensor) -> torch.Tensor:
    """An output the caller placed itself (a [B, H, S, head_dim] bf16 view, head_dim contiguous), or a fresh one laid out as [B, S, H, head_dim]."""
    if t is None:
        B, H, S, d = shape
        return torch.empty((B, S, H, d), dtype=bf16, device=like.device).permute(0, 2, 1, 3)
    if tuple(t.shape) != tuple(shape) or t.dtype != bf16 or t.device != like.device:
        raise ValueError(f"{name} must be a [B, H, S, head_dim] bf16 view on the inputs' device")
    return t


def attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_bias: Optional[torch.Tensor] = None,
             scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """q,k,v [B,H,S,64 | 128] bf16 (strided views allowed).  Returns (out [B,H,Sq,d] laid out as [B,Sq,H,d], lse [B,H,Sq]).  ``out``: an existing
    [B, H, Sq, d] bf16 view (head_dim contiguous) that receives the result instead."""
    for n, t in (("query", q), ("key", k), ("value", v)):
        require_gpu_tensor(t, n, bf16)
    B, H, Sq, d = q.shape
    scale = (1.0 / d**0.5) if scale is None else scale
    out = _placed(out, (B, H, Sq, d), "attn_fwd: out", q)
    lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    if key_bias is not None:
        require_gpu_tensor(key_bias, "key_bias", torch.float32)
    desc = _desc(q, k, v, out, scale, key_bias=key_bias)
    check(_lib.load().ftmi_attn_fwd(ctypes.byref(desc), ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), ptr(key_bias), stream_ptr()), "ftmi_attn_fwd")
    return out, lse


def attn_bwd(q, k, v, out, lse, dout, key_bias=None, scale=None, dv_out=None, dq=None, dk=None):
    """``dv_out`` / ``dq`` / ``dk``: existing [B, H, S, d] bf16 views (head_dim contiguous) that receive dV / dQ / dK, e.g. the thirds of a fused
    d(q|k|v) buffer."""
    B, H, Sq, d = q.shape
    Sk = k.shape[2]
    scale = (1.0 / d**0.5) if scale is None else scale
    if dout.stride(3) != 1:
        dout = dout.contiguous()
    dq = _placed(dq, (B, H, Sq, d), "attn_bwd: dq", q)
    dk = _placed(dk, (B, H, Sk, d), "attn_bwd: dk", q)
    dv = torch.empty((B, Sk, H, d), dtype=bf16, device=q.device).permute(0, 2, 1, 3) if dv_out is None else dv_out
    if dv.shape != (B, H, Sk, d) or dv.dtype != bf16:
        raise ValueError("attn_bwd: dv_out must be a [B, H, Sk, head_dim] bf16 view")
    delta = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    desc = _desc(q, k, v, out, scale, dout, dq, dk, dv, key_bias=key_bias)
    check(_lib.load().ftmi_attn_bwd(ctypes.byref(desc), ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), ptr(dout), ptr(dq), ptr(dk), ptr(dv),
                                     ptr(delta), ptr(key_bias), stream_ptr()), "ftmi_attn_bwd")
    return dq, dk, dv


def _ctx2_fwd(entry: str, q, k, v, out_first, scale):
    """The second-context forward through one C entry of the ``ftmi_attn_ctx2*_fwd`` family (narrow, wide; the tools' lab variant)."""
    for n, t in (("query", q), ("key", k), ("value", v), ("out_first", out_first)):
        require_gpu_tensor(t, n, bf16)
    B, H, Sq, d = q.shape
    if out_first.shape != q.shape:
        raise ValueError("attn_ctx2_fwd: out_first must be [B, H, Sq, head_dim]")
    scale = (1.0 / d**0.5) if scale is None else scale
    out = torch.empty_strided(out_first.shape, out_first.stride(), dtype=bf16, device=q.device)
    lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    desc = _desc(q, k, v, out, scale)
    check(getattr(_lib.load(), entry)(ctypes.byref(desc), ptr(q), ptr(k), ptr(v), ptr(out_first), ptr(out), ptr(lse), stream_ptr()), entry)
    return out, lse


def _ctx2_dq(entry: str, q, k, v, lse, dout, dq_first, scale, inplace):
    """The second-context dQ through one C entry of the ``ftmi_attn_ctx2*_dq`` family."""
    for n, t in (("query", q), ("key", k), ("value", v), ("dout", dout), ("dq_first", dq_first)):
        require_gpu_tensor(t, n, bf16)
    require_gpu_tensor(lse, "lse", torch.float32)
    B, H, Sq, d = q.shape
    scale = (1.0 / d**0.5) if scale is None else scale
    if dout.stride(3) != 1:
        dout = dout.contiguous()
    if dq_first.shape != q.shape or dout.shape != q.shape:
        raise ValueError("attn_ctx2_dq: dout and dq_first must be [B, H, Sq, head_dim]")
    if lse.shape != (B, H, Sq) or not lse.is_contiguous():
        raise ValueError("attn_ctx2_dq: lse must be the contiguous fp32 [B, H, Sq] tensor attn_ctx2_fwd returned")
    dq = dq_first if inplace else torch.empty_strided(dq_first.shape, dq_first.stride(), dtype=bf16, device=q.device)
    desc = _desc(q, k, v, None, scale, dout, dq)
    check(getattr(_lib.load(), entry)(ctypes.byref(desc), ptr(q), ptr(k), ptr(v), ptr(lse), ptr(dout), ptr(dq_first), ptr(dq), stream_ptr()), entry)
    return dq


def attn_ctx2_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out_first: torch.Tensor, scale: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Second context of a two-context cross-attention (head_dim 128, at most 320 keys), run after ``attn_fwd`` on the first one: returns
    (bf16(out_first + bf16(softmax(q k^T scale) v)) laid out like ``out_first``, lse [B, H, Sq] of this context)."""
    return _ctx2_fwd("ftmi_attn_ctx2_fwd", q, k, v, out_first, scale)


def attn_ctx2_dq(q, k, v, lse, dout, dq_first, scale=None, inplace: bool = False):
    """dQ of the second context added onto the first context's: bf16(dq_first + bf16(dq of this context)), laid out like ``dq_first`` (``inplace``: written
    into it).  There is no dK / dV (the second context's keys and values are frozen where this is used)."""
    return _ctx2_dq("ftmi_attn_ctx2_dq", q, k, v, lse, dout, dq_first, scale, inplace)


def attn_ctx2w_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out_first: torch.Tensor, scale: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``attn_ctx2_fwd`` through the wide kernel: up to 640 keys (two images in the second context: Wan first/last-frame), the next key tile staged while the
    current one is multiplied.  For at most 320 keys the result is ``attn_ctx2_fwd``'s, bit for bit."""
    return _ctx2_fwd("ftmi_attn_ctx2w_fwd", q, k, v, out_first, scale)


def attn_ctx2w_dq(q, k, v, lse, dout, dq_first, scale=None, inplace: bool = False):
    """``attn_ctx2_dq`` through the wide kernel (up to 640 keys); ``lse`` is the tensor ``attn_ctx2w_fwd`` returned."""
    return _ctx2_dq("ftmi_attn_ctx2w_dq", q, k, v, lse, dout, dq_first, scale, inplace)


def gemm_nt(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, alpha: float = 1.0, epilogue: int = 0,
            resid: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None, rows_per_batch: int = 0,
            aux: Optional[torch.Tensor] = None, want_out2: bool = False, variant: int = 8, out: Optional[torch.Tensor] = None):
    """out[M,N] = epilogue(alpha * x[M,K] @ w[N,K]^T + bias).  ``out``: write into an existing [M, N] bf16 view (row stride free, a multiple of 8)."""
    require_gpu_tensor(x, "x", bf16)
    require_gpu_tensor(w, "w", bf16)
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=bf16, device=x.device)
    elif out.shape != (M, N) or out.dtype != bf16 or out.stride(1) != 1:
        raise ValueError("gemm_nt: out must be an [M, N] bf16 view with contiguous columns")
    # out2 (allocated here, contiguous) / resid / aux share ONE row stride, which need not be out's (include/ftmi355.h: ld_side)
    out2 = torch.empty((M, N), dtype=bf16, device=x.device) if want_out2 else None
    side = [t for t in (out2, resid, aux) if t is not None]
    for t in side:
        if t.shape != (M, N) or t.stride(1) != 1 or t.stride(0) != side[0].stride(0):
            raise ValueError("gemm_nt: out2 / resid / aux must be [M, N] bf16 views with contiguous columns and one common row stride")
    ld_side = side[0].stride(0) if side else 0
    check(_lib.load().ftmi_gemm_nt(M, N, K, ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(bias), float(alpha), ptr(out), out.stride(0), epilogue,
                                    ptr(out2), ptr(resid), ptr(gate), rows_per_batch, ptr(aux), ld_side, variant, stream_ptr()), "ftmi_gemm_nt")
    return (out, out2) if want_out2 else out


def gemm_tn(u: torch.Tensor, v: torch.Tensor, out: Optional[torch.Tensor] = None, scale: float = 1.0) -> torch.Tensor:
    """out[P,Q] (fp32) += scale * u[M,P]^T @ v[M,Q]."""
    M, P = u.shape
    Q = v.shape[1]
    if out is None:
        out = torch.zeros((P, Q), dtype=torch.float32, device=u.device)
    check(_lib.load().ftmi_gemm_tn(M, P, Q, ptr(u), u.stride(0), ptr(v), v.stride(0), ptr(out), out.stride(0), float(scale), stream_ptr()),
          "ftmi_gemm_tn")
    return out


def _ld(t: Optional[torch.Tensor], name: str) -> int:
    if t is None:
        return 0
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name} must be a 2-D view with contiguous columns")
    return t.stride(0)


def _gemm_nt_args(x, w, out, *, M: int, N: int, K: int, bias=None, alpha: float = 1.0, epilogue: int = 0, out2=None,
                  resid=None, gate=None, gate_bstride: Optional[int] = None, rows_per_batch: int = 0, gate2=None, gate2_bstride: Optional[int] = None, aux=None,
                  x2=None, w2=None, K2: int = 0, xk_grp_n: int = 0, xk_grp_stride: int = 0, w_grp_n: int = 0, w_grp_stride: int = 0, w2_grp_n: int = 0,
                  w2_grp_stride: int = 0, x2_grp_n: int = 0, x2_grp_stride: int = 0, split_r: int = 0, variant: int = 8, _override: Optional[dict] = None):
    """The ftmi_gemm_nt_args block of gemm_nt_ex / gemm_nt_route."""
    a = _lib.GemmNtArgs()
    a.x, a.ldx, a.w, a.ldw, a.M, a.N, a.K = ptr(x), _ld(x, "x"), ptr(w), _ld(w, "w"), M, N, K
    a.xk_grp_n, a.xk_grp_stride, a.w_grp_n, a.w_grp_stride, a.w2_grp_n, a.w2_grp_stride = xk_grp_n, xk_grp_stride, w_grp_n, w_grp_stride, w2_grp_n, w2_grp_stride
    a.x2, a.ldx2, a.w2, a.ldw2, a.K2, a.x2_grp_n, a.x2_grp_stride = ptr(x2), _ld(x2, "x2"), ptr(w2), _ld(w2, "w2"), K2, x2_grp_n, x2_grp_stride
    a.bias, a.alpha, a.out, a.ldo, a.out2, a.ldo2 = ptr(bias), float(alpha), ptr(out), _ld(out, "out"), ptr(out2), _ld(out2, "out2")
    a.resid, a.ldr, a.aux, a.ldaux = ptr(resid), _ld(resid, "resid"), ptr(aux), _ld(aux, "aux")
    a.gate, a.gate_bstride = ptr(gate), (_ld(gate, "gate") if gate_bstride is None else gate_bstride)
    a.gate2, a.gate2_bstride = ptr(gate2), (_ld(gate2, "gate2") if gate2_bstride is None else gate2_bstride)
    a.rows_per_batch, a.epilogue, a.variant, a.split_r = rows_per_batch, epilogue, variant, split_r
    for k_, v_ in (_override or {}).items():
        setattr(a, k_, v_)
    return a


def gemm_nt_ex(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, **desc) -> None:
    """The NT GEMM with its full launch description (ftmi_gemm_nt_ex; the contract is stated in include/ftmi355.h).  Tensors are 2-D bf16 views with contiguous
    columns whose row strides become ldx / ldw / ldo / ...; the keywords (those of _gemm_nt_args: M, N, K required) say which part of them the launch uses and
    name the other operands.  gate / gate2 are [samples, >= N] views (their row stride is the sample stride unless given).  ``_override``: test hook -- raw values written over fields of the descriptor by name after it has been filled (the refusal tests pass misaligned leading dimensions)."""
    for n, t in (("x", x), ("w", w), ("out", out)):
        require_gpu_tensor(t, n, bf16)
    check(_lib.load().ftmi_gemm_nt_ex(ctypes.byref(_gemm_nt_args(x, w, out, **desc)), stream_ptr()), "ftmi_gemm_nt_ex")


def gemm_nt_route(**desc):
    """What gemm_nt_ex would run for the same description (ftmi_gemm_nt_route: host only -- nothing is launched, no tensor is read, no GPU is needed).  The
    keywords of gemm_nt_ex without the tensors; leading dimensions by name (ldx, ldw, ldo, ldx2, ldw2; default: the dense K, K, N, K2, K2).
    Returns (kind, variant, tile_rows, tile_cols) as include/ftmi355.h states them; a refusal raises like gemm_nt_ex."""
    ld = {"ldx": desc["K"], "ldw": desc["K"], "ldo": desc["N"], "ldx2": desc.get("K2", 0), "ldw2": desc.get("K2", 0)}
    ld.update({k_: desc.pop(k_) for k_ in list(ld) if k_ in desc})
    a = _gemm_nt_args(None, None, None, **desc)
    for k_, v_ in ld.items():
        setattr(a, k_, v_)
    route = (ctypes.c_int * 4)()
    check(_lib.load().ftmi_gemm_nt_route(ctypes.byref(a), route), "ftmi_gemm_nt_route")
    return tuple(route)


def gemm_tn_ex(u: torch.Tensor, v: torch.Tensor, c: torch.Tensor, *, M: int, P: int, Q: int, scale: float = 1.0, u_grp_p: int = 0, u_grp_stride: int = 0,
               v_grp_p: int = 0, v_grp_stride: int = 0, u_fold: int = 0, v_fold: int = 0, batch: int = 1, u_bstride: int = 0, v_bstride: int = 0,
               c_bstride: int = 0, _override: Optional[dict] = None) -> None:
    """The TN GEMM with its full launch description (ftmi_gemm_tn_ex): c (fp32) += scale * u^T v.  u, v, c: the 2-D views of problem 0 (row strides = ldu / ldv /
    ldc); a batched launch steps them by the element strides *_bstride (0 = shared).  ``_override``: as in gemm_nt_ex."""
    require_gpu_tensor(u, "u", bf16)
    require_gpu_tensor(v, "v", bf16)
    require_gpu_tensor(c, "c", torch.float32)
    a = _lib.GemmTnArgs()
    a.u, a.ldu, a.v, a.ldv, a.c, a.ldc, a.M, a.P, a.Q = ptr(u), _ld(u, "u"), ptr(v), _ld(v, "v"), ptr(c), _ld(c, "c"), M, P, Q
    a.v_grp_p, a.v_grp_stride, a.u_grp_p, a.u_grp_stride, a.u_fold, a.v_fold = v_grp_p, v_grp_stride, u_grp_p, u_grp_stride, u_fold, v_fold
    a.scale, a.batch, a.u_bstride, a.v_bstride, a.c_bstride = float(scale), batch, u_bstride, v_bstride, c_bstride
    for k_, v_ in (_override or {}).items():
        setattr(a, k_, v_)
    check(_lib.load().ftmi_gemm_tn_ex(ctypes.byref(a), stream_ptr()), "ftmi_gemm_tn_ex")


def fp8_upcast(w8: torch.Tensor, out: Optional[torch.Tensor] = None, transpose: bool = False) -> torch.Tensor:
    """bf16 copy of a [rows, cols] ``torch.float8_e4m3fn`` weight (exact), optionally transposed to [cols, rows]; ``out``: a contiguous bf16 tensor of the
    result's size (e.g. a slice of a per-model weight arena)."""
    if w8.dtype != torch.float8_e4m3fn or w8.dim() != 2 or not w8.is_contiguous() or not w8.is_cuda:
        raise ValueError("fp8_upcast: a contiguous 2-D float8_e4m3fn tensor on the GPU is required")
    rows, cols = w8.shape
    shape = (cols, rows) if transpose else (rows, cols)
    if out is None:
        out = torch.empty(shape, dtype=bf16, device=w8.device)
    elif out.numel() != rows * cols or out.dtype != bf16 or not out.is_contiguous():
        raise ValueError("fp8_upcast: out must be a contiguous bf16 tensor with rows * cols elements")
    check(_lib.load().ftmi_fp8_upcast(ptr(w8), ptr(out), rows, cols, int(transpose), stream_ptr()), "ftmi_fp8_upcast")
    return out.view(shape)


def transpose_bf16(x: torch.Tensor) -> torch.Tensor:
    rows, cols = x.shape
    out = torch.empty((cols, rows), dtype=bf16, device=x.device)
    check(_lib.load().ftmi_transpose_bf16(ptr(x), ptr(out), rows, cols, stream_ptr()), "ftmi_transpose_bf16")
    return out


def lora_split(w: torch.Tensor, sp: bool = False, ext: bool = False, t_sp: bool = False, t_ext: bool = False):
    """bf16 (hi, lo) working copies of an fp32 LoRA matrix w [rows, cols] (include/ftmi355.h: ftmi_lora_split).  Returns the requested
    layouts in the order (sp [2 rows, cols], ext [rows, 3 cols], t_sp [2 cols, rows], t_ext [cols, 3 rows])."""
    require_gpu_tensor(w, "w", torch.float32)
    w = w.contiguous()
    rows, cols = w.shape
    mk = lambda want, shape: torch.empty(shape, dtype=bf16, device=w.device) if want else None
    o = (mk(sp, (2 * rows, cols)), mk(ext, (rows, 3 * cols)), mk(t_sp, (2 * cols, rows)), mk(t_ext, (cols, 3 * rows)))
    check(_lib.load().ftmi_lora_split(ptr(w), rows, cols, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), stream_ptr()), "ftmi_lora_split")
    return tuple(t for t in o if t is not None)


def linear_lora_fwd(x, w, bias, lora_a, lora_b, lora_scale: float, variant: int = 8):
    """peft ``lora.Linear`` forward over a frozen bf16 Linear with fp32 adapters ``lora_a`` [r,K], ``lora_b`` [N,r] (None: plain
    linear).  Returns (y [M,N] bf16, xa [M,3r]: lora_scale * x A^T as bf16 (hi | lo | hi) planes, kept for the backward)."""
    M, K = x.shape
    N = w.shape[0]
    r = 0 if lora_a is None else lora_a.shape[0]
    y = torch.empty((M, N), dtype=bf16, device=x.device)
    xa = torch.empty((M, 3 * r), dtype=bf16, device=x.device) if r else None
    a_sp = b_ext = None
    if r:
        (a_sp,) = lora_split(lora_a, sp=True)
        (b_ext,) = lora_split(lora_b, ext=True)
    check(_lib.load().ftmi_linear_lora_fwd(M, K, N, r, float(lora_scale), ptr(x), ptr(w), ptr(bias), ptr(a_sp), ptr(b_ext), ptr(y), ptr(xa),
                                            variant, stream_ptr()), "ftmi_linear_lora_fwd")
    return y, xa


def linear_lora_bwd(x, dy, xa, w_t, lora_a, lora_b, lora_scale: float, grad_a=None, grad_b=None, need_dx: bool = True, variant: int = 8):
    """Backward of ``linear_lora_fwd``: returns (dx [M,K] bf16 or None, grad_a [r,K] fp32, grad_b [N,r] fp32); the gradient
    buffers are accumulated into when given (``.grad`` semantics).  ``w_t = W^T`` bf16; ``lora_a`` / ``lora_b`` fp32."""
    M, N = dy.shape
    K = w_t.shape[0] if w_t is not None else x.shape[1]
    r = 0 if lora_a is None else lora_a.shape[0]
    dx = torch.empty((M, K), dtype=bf16, device=dy.device) if need_dx else None
    dxa = torch.empty((M, 3 * r), dtype=bf16, device=dy.device) if r else None
    bt_sp = at_ext = None
    if r:
        (at_ext,) = lora_split(lora_a, t_ext=True)
        (bt_sp,) = lora_split(lora_b, t_sp=True)
        grad_a = torch.zeros((r, K), dtype=torch.float32, device=dy.device) if grad_a is None else grad_a
        grad_b = torch.zeros((N, r), dtype=torch.float32, device=dy.device) if grad_b is None else grad_b
    check(_lib.load().ftmi_linear_lora_bwd(M, K, N, r, float(lora_scale), ptr(x), ptr(dy), ptr(xa), ptr(w_t), ptr(bt_sp), ptr(at_ext), ptr(dxa),
                                            ptr(dx), ptr(grad_a), ptr(grad_b), variant, stream_ptr()), "ftmi_linear_lora_bwd")
    return dx, grad_a, grad_b


def norm_modulate(x, shift, onep, rows_per_batch: int, eps: float = 1e-6, layernorm: bool = False):
    """y = bf16(bf16(norm(x)) * onep[b]) + shift[b]; x [rows, 2048] bf16, shift / onep [B, 2048] bf16 (onep = 1 + scale)."""
    rows, D = x.shape
    y = torch.empty_like(x)
    check(_lib.load().ftmi_norm_modulate_fwd(ptr(x), ptr(shift), ptr(onep), shift.stride(0), ptr(y), rows, rows_per_batch, D, float(eps), int(layernorm),
                                              stream_ptr()), "ftmi_norm_modulate_fwd")
    return y


def norm_modulate_bwd(x, dy, onep, rows_per_batch: int, eps: float = 1e-6, layernorm: bool = False, dres=None):
    rows, D = x.shape
    dx = torch.empty_like(x)
    check(_lib.load().ftmi_norm_modulate_bwd(ptr(x), ptr(dy), ptr(onep), onep.stride(0), ptr(dres), ptr(dx), rows, rows_per_batch, D, float(eps),
                                              int(layernorm), stream_ptr()), "ftmi_norm_modulate_bwd")
    return dx


def qknorm_rope(x, w, cos=None, sin=None, rows_per_batch: Optional[int] = None, eps: float = 1e-5):
    """rope(bf16(rms_norm(x) * w)); x [rows, 2048] bf16 (row stride free), cos / sin fp32 [rows_per_batch, 1024] or None."""
    rows, D = x.shape
    y = torch.empty((rows, D), dtype=bf16, device=x.device)
    check(_lib.load().ftmi_qknorm_rope_fwd(ptr(x), x.stride(0), ptr(w), ptr(cos), ptr(sin), ptr(y), D, rows, rows_per_batch or rows, D, float(eps),
                                            stream_ptr()), "ftmi_qknorm_rope_fwd")
    return y


def qknorm_rope_bwd(x, w, dy, cos=None, sin=None, rows_per_batch: Optional[int] = None, eps: float = 1e-5):
    rows, D = x.shape
    dx = torch.empty((rows, D), dtype=bf16, device=x.device)
    check(_lib.load().ftmi_qknorm_rope_bwd(ptr(x), x.stride(0), ptr(w), ptr(cos), ptr(sin), ptr(dy), dy.stride(0), ptr(dx), D, rows, rows_per_batch or rows, D,
                                            float(eps), stream_ptr()), "ftmi_qknorm_rope_bwd")
    return dx


def norm_modulate_ex(x, shift, onep, y, rows_per_batch: int, eps: float = 1e-6, layernorm: bool = False, valid_width: int = 0):
    """ftmi_norm_modulate_fwd_ex: norm_modulate into ``y`` with the valid width of zero-padded rows; x / y contiguous [rows, 2048], shift / onep [B, 2048] views
    sharing one sample stride."""
    rows, D = x.shape
    check(_lib.load().ftmi_norm_modulate_fwd_ex(ptr(x), ptr(shift), ptr(onep), onep.stride(0), ptr(y), rows, int(rows_per_batch), D, float(eps), int(layernorm),
                                                 int(valid_width), stream_ptr()), "ftmi_norm_modulate_fwd_ex")
    return y


def norm_modulate_bwd_ex(x, dy, onep, dx, rows_per_batch: int, eps: float = 1e-6, layernorm: bool = False, dres=None, gate2=None, dx2=None, valid_width: int = 0):
    """ftmi_norm_modulate_bwd_ex: norm_modulate_bwd into ``dx`` and, with ``gate2`` ([B, 2048] view) and ``dx2``, dx2 = bf(bf(dx) * gate2[b])."""
    rows, D = x.shape
    check(_lib.load().ftmi_norm_modulate_bwd_ex(ptr(x), ptr(dy), ptr(onep), onep.stride(0), ptr(dres), ptr(dx), rows, int(rows_per_batch), D, float(eps),
                                                 int(layernorm), ptr(gate2), gate2.stride(0) if gate2 is not None else 0, ptr(dx2), int(valid_width),
                                                 stream_ptr()), "ftmi_norm_modulate_bwd_ex")
    return dx


def qknorm_rope_ex(x, w, y, cos=None, sin=None, rows_per_batch: Optional[int] = None, eps: float = 1e-5, w_rows: int = 1, pair=None, valid_width: int = 0):
    """ftmi_qknorm_rope_fwd_ex: x / y [rows, 2048] views (own row strides), w [w_rows, 2048] contiguous; ``pair = (x2, w2, y2)``: a second tensor set with the
    strides of the first, same launch."""
    rows, D = x.shape
    x2, w2, y2 = pair if pair is not None else (None, None, None)
    if pair is not None and (x2.stride(0) != x.stride(0) or y2.stride(0) != y.stride(0)):
        raise ValueError("qknorm_rope_ex: the second tensor set shares the row strides of the first")
    check(_lib.load().ftmi_qknorm_rope_fwd_ex(ptr(x), x.stride(0), ptr(w), ptr(cos), ptr(sin), ptr(y), y.stride(0), rows, int(rows_per_batch or rows), D,
                                               float(eps), int(w_rows), ptr(x2), ptr(w2), ptr(y2), int(valid_width), stream_ptr()), "ftmi_qknorm_rope_fwd_ex")
    return y


def qknorm_rope_bwd_ex(x, w, dy, dx, cos=None, sin=None, rows: Optional[int] = None, rows_per_batch: Optional[int] = None, eps: float = 1e-5, w_rows: int = 1,
                       pair=None, row_grp: int = 0, row_grp_span: int = 0, valid_width: int = 0):
    """ftmi_qknorm_rope_bwd_ex: ``pair = (x2, w2, dy2, dx2)``; with ``row_grp`` the ``rows`` logical rows sit in groups of row_grp, row_grp_span buffer rows
    apart (``rows`` must then be given: the buffers hold more rows than are processed)."""
    rows = x.shape[0] if rows is None else int(rows)
    D = x.shape[1]
    x2, w2, dy2, dx2 = pair if pair is not None else (None, None, None, None)
    if pair is not None and (x2.stride(0) != x.stride(0) or dy2.stride(0) != dy.stride(0) or dx2.stride(0) != dx.stride(0)):
        raise ValueError("qknorm_rope_bwd_ex: the second tensor set shares the row strides of the first")
    check(_lib.load().ftmi_qknorm_rope_bwd_ex(ptr(x), x.stride(0), ptr(w), ptr(cos), ptr(sin), ptr(dy), dy.stride(0), ptr(dx), dx.stride(0), rows,
                                               int(rows_per_batch or rows), D, float(eps), int(w_rows), ptr(x2), ptr(w2), ptr(dy2), ptr(dx2), int(row_grp),
                                               int(row_grp_span), int(valid_width), stream_ptr()), "ftmi_qknorm_rope_bwd_ex")
    return dx


def noise_pack(latents, noise, mean, std, sigma, sigma_first=None, first_frame_tokens: int = 0):
    """latents/noise [B,C,F,H,W] bf16 -> (x_t, target) [B, F*H*W, C] bf16."""
    B, C = latents.shape[:2]
    S = latents[0, 0].numel()
    latents = latents.contiguous()
    noise = noise.contiguous()
    xt = torch.empty((B, S, C), dtype=bf16, device=latents.device)
    target = torch.empty((B, S, C), dtype=bf16, device=latents.device)
    check(_lib.load().ftmi_ltx_noise_pack(ptr(latents), ptr(noise), ptr(mean), ptr(std), ptr(sigma), ptr(sigma_first), first_frame_tokens,
                                           ptr(xt), ptr(target), B, C, S, stream_ptr()), "ftmi_ltx_noise_pack")
    return xt, target


def ltx_cfg_euler_step(pred, x, sigma, sigma_next, guidance: float, x_next: Optional[torch.Tensor] = None):
    """One sampler step (include/ftmi355.h: ftmi_ltx_cfg_euler_step).  ``pred`` bf16 [2B, ...] (unconditional rows first; ``guidance == 1``: [B, ...]),
    ``x`` fp32 [B, ...] updated IN PLACE, ``sigma`` / ``sigma_next`` fp32 [B].  Returns the next model input: bf16(x) in both halves, shaped like ``pred``."""
    require_gpu_tensor(pred, "pred", bf16)
    require_gpu_tensor(x, "x", torch.float32)
    require_gpu_tensor(sigma, "sigma", torch.float32)
    require_gpu_tensor(sigma_next, "sigma_next", torch.float32)
    if not (pred.is_contiguous() and x.is_contiguous() and sigma.is_contiguous() and sigma_next.is_contiguous()):
        raise ValueError("ltx_cfg_euler_step: tensors must be contiguous (x is updated in place)")
    B = x.shape[0]
    halves = 1 if float(guidance) == 1.0 else 2
    if pred.shape[0] != halves * B or tuple(pred.shape[1:]) != tuple(x.shape[1:]):
        raise ValueError(f"ltx_cfg_euler_step: pred {tuple(pred.shape)} must be [{halves} x {B}, ...] over x {tuple(x.shape)}")
    if sigma.numel() != B or sigma_next.numel() != B:
        raise ValueError("ltx_cfg_euler_step: sigma / sigma_next hold one value per sample")
    if x_next is None:
        x_next = torch.empty_like(pred)
    else:
        require_gpu_tensor(x_next, "x_next", bf16)
        if x_next.shape != pred.shape or not x_next.is_contiguous():
            raise ValueError("ltx_cfg_euler_step: x_next must be a contiguous tensor shaped like pred")
    check(_lib.load().ftmi_ltx_cfg_euler_step(ptr(pred), ptr(x), ptr(sigma), ptr(sigma_next), float(guidance), ptr(x_next), B, x[0].numel(), stream_ptr()),
          "ftmi_ltx_cfg_euler_step")
    return x_next


def ltx_cfg_euler_step_held(pred, x, sigma, sigma_next, guidance: float, hold: int, x_next: Optional[torch.Tensor] = None):
    """``ltx_cfg_euler_step`` with the first ``hold`` elements of every sample held (include/ftmi355.h: ftmi_ltx_cfg_euler_step_held): ``x`` stays as it is
    there and only its bf16 copy reaches the returned model input.  ``hold % 8 == 0``."""
    require_gpu_tensor(pred, "pred", bf16)
    require_gpu_tensor(x, "x", torch.float32)
    require_gpu_tensor(sigma, "sigma", torch.float32)
    require_gpu_tensor(sigma_next, "sigma_next", torch.float32)
    if not (pred.is_contiguous() and x.is_contiguous() and sigma.is_contiguous() and sigma_next.is_contiguous()):
        raise ValueError("ltx_cfg_euler_step_held: tensors must be contiguous (x is updated in place)")
    B = x.shape[0]
    halves = 1 if float(guidance) == 1.0 else 2
    if pred.shape[0] != halves * B or tuple(pred.shape[1:]) != tuple(x.shape[1:]):
        raise ValueError(f"ltx_cfg_euler_step_held: pred {tuple(pred.shape)} must be [{halves} x {B}, ...] over x {tuple(x.shape)}")
    if sigma.numel() != B or sigma_next.numel() != B:
        raise ValueError("ltx_cfg_euler_step_held: sigma / sigma_next hold one value per sample")
    if x_next is None:
        x_next = torch.empty_like(pred)
    else:
        require_gpu_tensor(x_next, "x_next", bf16)
        if x_next.shape != pred.shape or not x_next.is_contiguous():
            raise ValueError("ltx_cfg_euler_step_held: x_next must be a contiguous tensor shaped like pred")
    check(_lib.load().ftmi_ltx_cfg_euler_step_held(ptr(pred), ptr(x), ptr(sigma), ptr(sigma_next), float(guidance), ptr(x_next), B, x[0].numel(), int(hold),
                                                   stream_ptr()), "ftmi_ltx_cfg_euler_step_held")
    return x_next


# The LTX wrappers below take ``weights``: a ``_lib.LtxFfWeights`` (its feed-forward extension all NULL: the eight attention adapters alone, which is also
# what the planners size for when they get no weights).
def _ltx_plan_weights(weights):
    return ctypes.byref(weights if weights is not None else _lib.LtxFfWeights())


def ltx_forward_frames_workspace_bytes(cfg, frames: int, weights=None) -> int:
    return int(_lib.load().ftmi_ltx_ff_forward_frames_workspace_bytes(ctypes.byref(cfg), _ltx_plan_weights(weights), int(frames)))


def ltx_forward_frames(cfg, weights, x_t, text, key_bias, timesteps, workspace=None, pred=None):
    """DiT forward with one timestep per latent frame, forward only (include/ftmi355.h: ftmi_ltx_ff_forward_frames).  ``x_t`` bf16 [B, S, C_in], ``text`` bf16
    [B, T, D_cap], ``key_bias`` fp32 [B, T] or None, ``timesteps`` fp32 [B, F] with S % F == 0.  Returns ``pred`` bf16 [B, S, C_out]."""
    require_gpu_tensor(x_t, "x_t", bf16)
    require_gpu_tensor(text, "text", bf16)
    require_gpu_tensor(timesteps, "timesteps", torch.float32)
    B, S, T = cfg.B, cfg.S, cfg.T
    if tuple(x_t.shape) != (B, S, cfg.C_in) or not x_t.is_contiguous():
        raise ValueError(f"ltx_forward_frames: x_t must be a contiguous [{B}, {S}, {cfg.C_in}] tensor, got {tuple(x_t.shape)}")
    if tuple(text.shape) != (B, T, cfg.D_cap) or not text.is_contiguous():
        raise ValueError(f"ltx_forward_frames: text must be a contiguous [{B}, {T}, {cfg.D_cap}] tensor, got {tuple(text.shape)}")
    if timesteps.ndim != 2 or timesteps.shape[0] != B or not timesteps.is_contiguous():
        raise ValueError(f"ltx_forward_frames: timesteps must be a contiguous [{B}, frames] tensor, got {tuple(timesteps.shape)}")
    frames = timesteps.shape[1]
    if frames < 1 or S % frames:
        raise ValueError(f"ltx_forward_frames: {S} tokens do not split into {frames} frames")
    if key_bias is not None:
        require_gpu_tensor(key_bias, "key_bias", torch.float32)
        if tuple(key_bias.shape) != (B, T) or not key_bias.is_contiguous():
            raise ValueError(f"ltx_forward_frames: key_bias must be a contiguous [{B}, {T}] tensor")
    ws_bytes = ltx_forward_frames_workspace_bytes(cfg, frames, weights=weights)
    if workspace is None:
        workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=x_t.device)
    elif workspace.numel() < ws_bytes:
        raise ValueError("ltx_forward_frames: workspace too small")
    if pred is None:
        pred = torch.empty((B, S, cfg.C_out), dtype=bf16, device=x_t.device)
    check(_lib.load().ftmi_ltx_ff_forward_frames(ctypes.byref(cfg), ctypes.byref(weights), ptr(x_t), ptr(text), ptr(key_bias), ptr(timesteps), frames, ptr(pred),
                                                 ptr(workspace), workspace.numel(), stream_ptr()), "ftmi_ltx_ff_forward_frames")
    return pred


def gelu_from_pre(z, out=None):
    """``g = bf16(gelu_tanh(z))`` from the bf16 pre-activation a GELU GEMM stashed (include/ftmi355.h: ftmi_gelu_from_pre): the bits that GEMM wrote as its
    activation.  ``z`` [rows, width] with any row stride (a column window of a wider tensor is fine); ``out`` likewise, allocated contiguous when None."""
    require_gpu_tensor(z, "z", bf16)
    if z.ndim != 2 or (z.shape[1] > 1 and z.stride(1) != 1):
        raise ValueError("gelu_from_pre: z must be [rows, width] with unit column stride")
    rows, width = z.shape
    if out is None:
        out = torch.empty((rows, width), dtype=bf16, device=z.device)
    require_gpu_tensor(out, "out", bf16)
    if tuple(out.shape) != (rows, width) or (width > 1 and out.stride(1) != 1):
        raise ValueError("gelu_from_pre: out must be shaped like z with unit column stride")
    check(_lib.load().ftmi_gelu_from_pre(ptr(z), z.stride(0) if rows > 1 else max(width, z.stride(0)), ptr(out), out.stride(0) if rows > 1 else max(width, out.stride(0)),
                                          rows, width, stream_ptr()), "ftmi_gelu_from_pre")
    return out


def ltx_unpack_denorm(x, mean, std, num_frames: int, height: int, width: int):
    """Inverse of ``noise_pack``'s normalise + pack: x fp32 [B, S, C] -> latents bf16 [B, C, F, H, W] = x * std[c] + mean[c]."""
    require_gpu_tensor(x, "x", torch.float32)
    require_gpu_tensor(mean, "mean", torch.float32)
    require_gpu_tensor(std, "std", torch.float32)
    B, S, C = x.shape
    if S != num_frames * height * width:
        raise ValueError(f"ltx_unpack_denorm: {S} tokens != num_frames * height * width = {num_frames * height * width}")
    if mean.numel() != C or std.numel() != C:
        raise ValueError("ltx_unpack_denorm: mean / std hold one value per channel")
    x, mean, std = x.contiguous(), mean.contiguous(), std.contiguous()
    out = torch.empty((B, C, num_frames, height, width), dtype=bf16, device=x.device)
    check(_lib.load().ftmi_ltx_unpack_denorm(ptr(x), ptr(mean), ptr(std), ptr(out), B, C, S, stream_ptr()), "ftmi_ltx_unpack_denorm")
    return out


def ltx_sample_workspace_bytes(cfg, two_pass: bool, weights=None) -> int:
    return int(_lib.load().ftmi_ltx_ff_sample_workspace_bytes(ctypes.byref(cfg), _ltx_plan_weights(weights), int(bool(two_pass))))


def ltx_sample(cfg, weights, text_cond, text_uncond, key_bias_cond, key_bias_uncond, x, sigmas, timesteps, guidance: float, workspace=None):
    """The whole denoising loop as one C call (include/ftmi355.h: ftmi_ltx_ff_sample).  ``cfg`` / ``weights``: ``_lib.LtxConfig`` (B = videos) /
    ``_lib.LtxFfWeights``; text_* bf16 [B, T, D_cap]; key_bias_* fp32 [B, T] or None; ``x`` fp32 [B, S, C] (noise in, latents out, IN PLACE);
    ``sigmas`` fp32 [n + 1], ``timesteps`` fp32 [n] on the device.  Returns ``x``."""
    two_pass = float(guidance) != 1.0
    require_gpu_tensor(text_cond, "text_cond", bf16)
    require_gpu_tensor(x, "x", torch.float32)
    require_gpu_tensor(sigmas, "sigmas", torch.float32)
    require_gpu_tensor(timesteps, "timesteps", torch.float32)
    B, S, T = cfg.B, cfg.S, cfg.T
    if tuple(x.shape) != (B, S, cfg.C_in) or not x.is_contiguous():
        raise ValueError(f"ltx_sample: x must be a contiguous [{B}, {S}, {cfg.C_in}] tensor (it is updated in place), got {tuple(x.shape)}")
    n = timesteps.numel()
    if n < 1 or sigmas.numel() != n + 1 or not (sigmas.is_contiguous() and timesteps.is_contiguous()):
        raise ValueError("ltx_sample: sigmas must hold one more value than timesteps")
    texts = [("text_cond", text_cond)] + ([("text_uncond", text_uncond)] if two_pass else [])
    for name, t in texts:
        if t is None:
            raise ValueError("ltx_sample: guidance != 1 needs the unconditional prompt embeddings")
        require_gpu_tensor(t, name, bf16)
        if tuple(t.shape) != (B, T, cfg.D_cap) or not t.is_contiguous():
            raise ValueError(f"ltx_sample: {name} must be a contiguous [{B}, {T}, {cfg.D_cap}] tensor, got {tuple(t.shape)}")
    biases = [("key_bias_cond", key_bias_cond)] + ([("key_bias_uncond", key_bias_uncond)] if two_pass else [])
    if len({b is None for _, b in biases}) != 1:
        raise ValueError("ltx_sample: give the key bias of both prompts or of neither")
    for name, b in biases:
        if b is not None:
            require_gpu_tensor(b, name, torch.float32)
            if tuple(b.shape) != (B, T) or not b.is_contiguous():
                raise ValueError(f"ltx_sample: {name} must be a contiguous [{B}, {T}] tensor")
    ws_bytes = ltx_sample_workspace_bytes(cfg, two_pass, weights=weights)
    if workspace is None:
        workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=x.device)
    elif workspace.numel() < ws_bytes:
        raise ValueError("ltx_sample: workspace too small")
    check(_lib.load().ftmi_ltx_ff_sample(ctypes.byref(cfg), ctypes.byref(weights), ptr(text_cond), ptr(text_uncond) if two_pass else None, ptr(key_bias_cond),
                                         ptr(key_bias_uncond) if two_pass else None, ptr(x), ptr(sigmas), ptr(timesteps), n, float(guidance), ptr(workspace),
                                         workspace.numel(), stream_ptr()), "ftmi_ltx_ff_sample")
    return x


def ltx_sample_cond_workspace_bytes(cfg, two_pass: bool, frames: int, weights=None) -> int:
    return int(_lib.load().ftmi_ltx_ff_sample_cond_workspace_bytes(ctypes.byref(cfg), _ltx_plan_weights(weights), int(bool(two_pass)), int(frames)))


def ltx_sample_cond(cfg, weights, text_cond, text_uncond, key_bias_cond, key_bias_uncond, x, sigmas, timesteps, guidance: float, frames: int, cond_frames: int,
                    workspace=None):
    """``ltx_sample`` with the first ``cond_frames`` of the ``frames`` latent frames of every sample held (include/ftmi355.h: ftmi_ltx_ff_sample_cond): those
    tokens of ``x`` are the clean conditioning latents on entry and are never written; the model sees timestep 0 on them.  Returns ``x``."""
    two_pass = float(guidance) != 1.0
    require_gpu_tensor(text_cond, "text_cond", bf16)
    require_gpu_tensor(x, "x", torch.float32)
    require_gpu_tensor(sigmas, "sigmas", torch.float32)
    require_gpu_tensor(timesteps, "timesteps", torch.float32)
    B, S, T = cfg.B, cfg.S, cfg.T
    frames, cond_frames = int(frames), int(cond_frames)
    if frames < 1 or S % frames:
        raise ValueError(f"ltx_sample_cond: {S} tokens do not split into {frames} frames")
    if not 0 <= cond_frames <= frames:
        raise ValueError(f"ltx_sample_cond: cond_frames {cond_frames} outside [0, {frames}]")
    if tuple(x.shape) != (B, S, cfg.C_in) or not x.is_contiguous():
        raise ValueError(f"ltx_sample_cond: x must be a contiguous [{B}, {S}, {cfg.C_in}] tensor (it is updated in place), got {tuple(x.shape)}")
    n = timesteps.numel()
    if n < 1 or sigmas.numel() != n + 1 or not (sigmas.is_contiguous() and timesteps.is_contiguous()):
        raise ValueError("ltx_sample_cond: sigmas must hold one more value than timesteps")
    texts = [("text_cond", text_cond)] + ([("text_uncond", text_uncond)] if two_pass else [])
    for name, t in texts:
        if t is None:
            raise ValueError("ltx_sample_cond: guidance != 1 needs the unconditional prompt embeddings")
        require_gpu_tensor(t, name, bf16)
        if tuple(t.shape) != (B, T, cfg.D_cap) or not t.is_contiguous():
            raise ValueError(f"ltx_sample_cond: {name} must be a contiguous [{B}, {T}, {cfg.D_cap}] tensor, got {tuple(t.shape)}")
    biases = [("key_bias_cond", key_bias_cond)] + ([("key_bias_uncond", key_bias_uncond)] if two_pass else [])
    if len({b is None for _, b in biases}) != 1:
        raise ValueError("ltx_sample_cond: give the key bias of both prompts or of neither")
    for name, b in biases:
        if b is not None:
            require_gpu_tensor(b, name, torch.float32)
            if tuple(b.shape) != (B, T) or not b.is_contiguous():
                raise ValueError(f"ltx_sample_cond: {name} must be a contiguous [{B}, {T}] tensor")
    ws_bytes = ltx_sample_cond_workspace_bytes(cfg, two_pass, frames, weights=weights)
    if workspace is None:
        workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=x.device)
    elif workspace.numel() < ws_bytes:
        raise ValueError("ltx_sample_cond: workspace too small")
    check(_lib.load().ftmi_ltx_ff_sample_cond(ctypes.byref(cfg), ctypes.byref(weights), ptr(text_cond), ptr(text_uncond) if two_pass else None,
                                              ptr(key_bias_cond), ptr(key_bias_uncond) if two_pass else None, ptr(x), ptr(sigmas), ptr(timesteps), n,
                                              float(guidance), frames, cond_frames, ptr(workspace), workspace.numel(), stream_ptr()), "ftmi_ltx_ff_sample_cond")
    return x


def ddim_add_noise(latents, noise, sqrt_alpha, sqrt_one_minus_alpha, scaling_factor: float = 1.0):
    """CogVideoX noising: (x0 = bf16(latents * scaling_factor), noisy = scheduler.add_noise(x0, noise, t)); per-sample coefficients fp32 [B]."""
    require_gpu_tensor(latents, "latents", bf16)
    latents, noise = latents.contiguous(), noise.contiguous()
    B = latents.shape[0]
    x0, noisy = torch.empty_like(latents), torch.empty_like(latents)
    check(_lib.load().ftmi_ddim_add_noise(ptr(latents), ptr(noise), ptr(sqrt_alpha), ptr(sqrt_one_minus_alpha), float(scaling_factor), ptr(x0), ptr(noisy), B,
                                           latents[0].numel(), stream_ptr()), "ftmi_ddim_add_noise")
    return x0, noisy


def ddim_get_velocity(sample, noise, sqrt_alpha, sqrt_one_minus_alpha):
    """scheduler.get_velocity(sample, noise, t) = sqrt(a) noise - sqrt(1 - a) sample (bf16 op by op)."""
    require_gpu_tensor(sample, "sample", bf16)
    sample, noise = sample.contiguous(), noise.contiguous()
    out = torch.empty_like(sample)
    check(_lib.load().ftmi_ddim_get_velocity(ptr(sample), ptr(noise), ptr(sqrt_alpha), ptr(sqrt_one_minus_alpha), ptr(out), sample.shape[0], sample[0].numel(),
                                              stream_ptr()), "ftmi_ddim_get_velocity")
    return out


# ---- CogVideoX block, row-wise stages (include/ftmi355.h: ftmi_cog_*) ------------------------------------------------------------------
def _cog_rows(x):
    require_gpu_tensor(x, "x", bf16)
    if x.dim() != 3 or not x.is_contiguous():
        raise ValueError("expected a contiguous [B, tokens, D] bf16 tensor (text tokens of a sample first)")
    return x.shape[0] * x.shape[1], x.shape[2], x.shape[1]


def cog_ln_mod(x, w, b, shift, onep, text_len: int, eps: float = 1e-5, out=None):
    """CogVideoXLayerNormZero body: bf(bf(LayerNorm(x; w, b)) * onep) + shift; shift / onep [B, 2, D] (text, video) or [B, D] (text_len = 0)."""
    rows, D, rpb = _cog_rows(x)
    y = torch.empty_like(x) if out is None else out
    if y.shape != x.shape or not y.is_contiguous():
        raise ValueError("cog_ln_mod: out must be a contiguous tensor of x's shape")
    check(_lib.load().ftmi_cog_ln_mod_fwd(ptr(x), ptr(w), ptr(b), ptr(shift.contiguous()), ptr(onep.contiguous()), ptr(y), rows, D, rpb, int(text_len),
                                          float(eps), stream_ptr()), "ftmi_cog_ln_mod_fwd")
    return y


def cog_ln_mod_bwd(x, w, onep, dy, text_len: int, eps: float = 1e-5, dres=None):
    rows, D, rpb = _cog_rows(x)
    dx = torch.empty_like(x)
    check(_lib.load().ftmi_cog_ln_mod_bwd(ptr(x), ptr(w), ptr(onep.contiguous()), ptr(dy.contiguous()), ptr(dres), ptr(dx), rows, D, rpb, int(text_len),
                                          float(eps), stream_ptr()), "ftmi_cog_ln_mod_bwd")
    return dx


def _rope_args(rope, rows_per_batch, text_len):
    if rope is None:
        return None, None, 0, 0
    cos, sin = rope
    require_gpu_tensor(cos, "rope cos", torch.float32)
    require_gpu_tensor(sin, "rope sin", torch.float32)
    if cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] != 64 or cos.shape[0] != rows_per_batch - text_len or not cos.is_contiguous() or not sin.is_contiguous():
        raise ValueError(f"rotary tables must be contiguous fp32 [video tokens = {rows_per_batch - text_len}, 64], got {tuple(cos.shape)}")
    return cos, sin, int(rows_per_batch), int(text_len)


def cog_head_ln(x2d, w, b, eps: float = 1e-6, out=None, rope=None, rows_per_batch: int = 0, text_len: int = 0):
    """LayerNorm over each 64-channel head of the rows of x2d [M, D] (a column slice of a wider buffer is fine: row stride = x2d.stride(0));
    ``rope = (cos, sin)`` fp32 [S, 64]: rotary embedding on the rows at position >= text_len of every rows_per_batch-token sample."""
    require_gpu_tensor(x2d, "x", bf16)
    M, D = x2d.shape
    cos, sin, rpb, tl = _rope_args(rope, rows_per_batch, text_len)
    if x2d.stride(1) != 1:
        raise ValueError("head LayerNorm: channels must be contiguous")
    y = torch.empty((M, D), dtype=bf16, device=x2d.device) if out is None else out
    if y.stride(0) != x2d.stride(0):
        y_c = torch.empty_strided((M, D), (x2d.stride(0), 1), dtype=bf16, device=x2d.device)
    else:
        y_c = y
    check(_lib.load().ftmi_cog_head_ln_fwd(ptr(x2d), x2d.stride(0), ptr(w), ptr(b), ptr(y_c), M, D, float(eps), ptr(cos), ptr(sin), rpb, tl, stream_ptr()),
          "ftmi_cog_head_ln_fwd")
    if y_c is not y:
        y.copy_(y_c)
    return y


def cog_head_ln_bwd(x2d, w, dy2d, eps: float = 1e-6, rope=None, rows_per_batch: int = 0, text_len: int = 0):
    require_gpu_tensor(x2d, "x", bf16)
    M, D = x2d.shape
    cos, sin, rpb, tl = _rope_args(rope, rows_per_batch, text_len)
    if x2d.stride(0) != dy2d.stride(0) or x2d.stride(1) != 1 or dy2d.stride(1) != 1:
        raise ValueError("head LayerNorm backward: x and dy must share one row stride")
    dx = torch.empty_strided((M, D), (x2d.stride(0), 1), dtype=bf16, device=x2d.device)
    check(_lib.load().ftmi_cog_head_ln_bwd(ptr(x2d), x2d.stride(0), ptr(w), ptr(dy2d), ptr(dx), M, D, float(eps), ptr(cos), ptr(sin), rpb, tl, stream_ptr()),
          "ftmi_cog_head_ln_bwd")
    return dx


def cog_gate_residual(res, y, gate, text_len: int, out=None):
    """res + bf(gate * y) per segment (res None: bf(gate * y)); ``out`` may be ``y`` or ``res`` themselves (element-wise, in place)."""
    rows, D, rpb = _cog_rows(y)
    out = torch.empty_like(y) if out is None else out
    if out.shape != y.shape or not out.is_contiguous() or (res is not None and (res.shape != y.shape or not res.is_contiguous())):
        raise ValueError("cog_gate_residual: res / out must be contiguous tensors of y's shape")
    check(_lib.load().ftmi_cog_gate_residual(ptr(res), ptr(y), ptr(gate.contiguous()), ptr(out), rows, D, rpb, int(text_len), stream_ptr()),
          "ftmi_cog_gate_residual")
    return out


def cog_patchify(latents, patch: int):
    """latents [B, F, C, H, W] bf16 -> tokens [B, F (H/p) (W/p), C p p] (channel order (c, py, px): the flattened Conv2d weight's)."""
    require_gpu_tensor(latents, "latents", bf16)
    B, F_, C, H, W = latents.shape
    latents = latents.contiguous()
    out = torch.empty((B, F_ * (H // patch) * (W // patch), C * patch * patch), dtype=bf16, device=latents.device)
    check(_lib.load().ftmi_cog_patchify(ptr(latents), ptr(out), B, F_, C, H, W, int(patch), stream_ptr()), "ftmi_cog_patchify")
    return out


def cog_unpatchify(tokens, F_: int, C: int, H: int, W: int, patch: int):
    """tokens [B, F (H/p) (W/p), C p p] bf16 -> latents [B, F, C, H, W]."""
    require_gpu_tensor(tokens, "tokens", bf16)
    B = tokens.shape[0]
    if tokens.shape[1:] != (F_ * (H // patch) * (W // patch), C * patch * patch):
        raise ValueError(f"cog_unpatchify: tokens {tuple(tokens.shape)} do not match F={F_} C={C} H={H} W={W} p={patch}")
    tokens = tokens.contiguous()
    out = torch.empty((B, F_, C, H, W), dtype=bf16, device=tokens.device)
    check(_lib.load().ftmi_cog_unpatchify(ptr(tokens), ptr(out), B, F_, C, H, W, int(patch), stream_ptr()), "ftmi_cog_unpatchify")
    return out


def posterior_sample(moments, eps):
    """moments [B, 2C, ...] (mean | logvar along dim 1), eps [B, C, ...] ~ N(0,1) -> mean + exp(0.5 * clamp(logvar, -30, 20)) * eps."""
    require_gpu_tensor(moments, "moments", bf16)
    require_gpu_tensor(eps, "eps", bf16)
    if moments.shape[1] != 2 * eps.shape[1] or moments.shape[2:] != eps.shape[2:] or moments.shape[0] != eps.shape[0]:
        raise ValueError(f"posterior_sample: moments {tuple(moments.shape)} do not hold (mean | logvar) for eps {tuple(eps.shape)}")
    moments, eps = moments.contiguous(), eps.contiguous()
    out = torch.empty_like(eps)
    check(_lib.load().ftmi_posterior_sample(ptr(moments), ptr(eps), ptr(out), eps.shape[0], eps[0].numel(), stream_ptr()), "ftmi_posterior_sample")
    return out


# ---- the LTX time-embedding chain one launcher at a time (include/ftmi355.h; the forward passes run it inside the C library) --------------------
def timestep_sinusoid(t: torch.Tensor) -> torch.Tensor:
    """t fp32 [B] -> bf16 [B, 256] = [cos | sin] of t * 10000^(-j / 128)."""
    require_gpu_tensor(t, "t", torch.float32)
    out = torch.empty((t.numel(), 256), dtype=bf16, device=t.device)
    check(_lib.load().ftmi_timestep_sinusoid(ptr(t), ptr(out), t.numel(), stream_ptr()), "ftmi_timestep_sinusoid")
    return out


def small_linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, silu_in: bool = False) -> torch.Tensor:
    """x [rows <= 8, K], w [N, K], bias [N] (bf16) -> bf16 [rows, N] = (silu(x) if silu_in else x) w^T + bias."""
    for t, n in ((x, "x"), (w, "w")) + (((bias, "bias"),) if bias is not None else ()):
        require_gpu_tensor(t, n, bf16)
    x, w = x.contiguous(), w.contiguous()
    if w.shape[1] != x.shape[1] or (bias is not None and bias.numel() != w.shape[0]):
        raise ValueError(f"small_linear: x {tuple(x.shape)}, w {tuple(w.shape)} and the bias do not fit")
    out = torch.empty((x.shape[0], w.shape[0]), dtype=bf16, device=x.device)
    check(_lib.load().ftmi_small_linear(ptr(x), ptr(w), ptr(bias), ptr(out), x.shape[0], w.shape[0], x.shape[1], int(silu_in), stream_ptr()), "ftmi_small_linear")
    return out


def ada_prep(tables: torch.Tensor, temb: torch.Tensor) -> torch.Tensor:
    """tables [L, 6, D], temb [B, 6, D] (bf16) -> ada [L, B, 8, D]: table + temb in slots 0..5, 1 + slot 1 and 1 + slot 4 in slots 6, 7."""
    require_gpu_tensor(tables, "tables", bf16)
    require_gpu_tensor(temb, "temb", bf16)
    tables, temb = tables.contiguous(), temb.contiguous()
    (L, _, D), B = tables.shape, temb.shape[0]
    out = torch.empty((L, B, 8, D), dtype=bf16, device=tables.device)
    check(_lib.load().ftmi_ada_prep(ptr(tables), ptr(temb), ptr(out), L, B, D, stream_ptr()), "ftmi_ada_prep")
    return out


def ada_out_prep(table2: torch.Tensor, emb: torch.Tensor) -> torch.Tensor:
    """table2 [2, D], emb [B, D] (bf16) -> [B, 3, D]: shift, scale, 1 + scale of the output norm."""
    require_gpu_tensor(table2, "table2", bf16)
    require_gpu_tensor(emb, "emb", bf16)
    table2, emb = table2.contiguous(), emb.contiguous()
    B, D = emb.shape
    out = torch.empty((B, 3, D), dtype=bf16, device=emb.device)
    check(_lib.load().ftmi_ada_out_prep(ptr(table2), ptr(emb), ptr(out), B, D, stream_ptr()), "ftmi_ada_out_prep")
    return out


MSE_SCRATCH_FLOATS_PER_SAMPLE = 256  # FTMI_MSE_SCRATCH_FLOATS_PER_SAMPLE of include/ftmi355.h


def mse_loss(pred, target, weight: Optional[torch.Tensor], want_grad: bool = True, grad_scale: float = 1.0):
    B = pred.shape[0]
    per = pred[0].numel()
    loss = torch.empty((1,), dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    scratch = torch.empty((MSE_SCRATCH_FLOATS_PER_SAMPLE * B,), dtype=torch.float32, device=pred.device)  # caller-owned partial sums (ftmi355.h)
    check(_lib.load().ftmi_mse_loss(ptr(pred), ptr(target), ptr(weight), ptr(loss), ptr(dpred), B, per, float(grad_scale), ptr(scratch), stream_ptr()),
          "ftmi_mse_loss")
    return loss, dpred


def clip_grad_norm_(grads: torch.Tensor, max_norm: float, scratch: Optional[torch.Tensor] = None, grad_norm_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In-place global-norm clip of a flat fp32 gradient buffer; returns the pre-clip norm (device scalar)."""
    require_gpu_tensor(grads, "grads", torch.float32)
    if not grads.is_contiguous():
        raise ValueError("clip_grad_norm_: the flat gradient buffer must be contiguous")
    if scratch is None:
        scratch = torch.empty((CLIP_SCRATCH_FLOATS,), dtype=torch.float32, device=grads.device)
    if grad_norm_out is None:
        grad_norm_out = torch.empty((1,), dtype=torch.float32, device=grads.device)
    check(_lib.load().ftmi_clip_grad_norm(ptr(grads), grads.numel(), float(max_norm), ptr(scratch), ptr(grad_norm_out), stream_ptr()), "ftmi_clip_grad_norm")
    return grad_norm_out


CLIP_SCRATCH_FLOATS = 2050  # include/ftmi355.h FTMI_CLIP_SCRATCH_FLOATS


def clip_adamw_step(params, grads, exp_avg, exp_avg_sq, step: int, lr: float, betas=(0.9, 0.95), eps: float = 1e-8,
                    weight_decay: float = 1e-4, max_norm: float = 1.0, scratch: Optional[torch.Tensor] = None,
                    grad_norm_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    n = params.numel()
    if scratch is None:
        scratch = torch.empty((CLIP_SCRATCH_FLOATS,), dtype=torch.float32, device=params.device)
    elif scratch.numel() < CLIP_SCRATCH_FLOATS or scratch.dtype != torch.float32:
        raise ValueError(f"clip_adamw_step: scratch must hold {CLIP_SCRATCH_FLOATS} fp32 values (FTMI_CLIP_SCRATCH_FLOATS)")
    if grad_norm_out is None:
        grad_norm_out = torch.empty((1,), dtype=torch.float32, device=params.device)
    check(_lib.load().ftmi_clip_adamw_step(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), n, float(max_norm), float(lr),
                                            float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step), ptr(scratch),
                                            ptr(grad_norm_out), stream_ptr()), "ftmi_clip_adamw_step")
    return grad_norm_out


# ---- Wan-T2V full fine-tune (include/ftmi355.h: ftmi_wan_*; csrc/wan.hip) --------------------------------------------------------------------
def _rows2d(t: torch.Tensor, name: str) -> torch.Tensor:
    require_gpu_tensor(t, name, bf16)
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 8 != 0:
        raise ValueError(f"{name}: a 2-D bf16 view with contiguous columns and a row stride that is a multiple of 8")
    return t


def _f32(t: Optional[torch.Tensor], name: str, shape=None) -> Optional[torch.Tensor]:
    if t is None:
        return None
    require_gpu_tensor(t, name, torch.float32)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: contiguous columns required")
    return t


def _wan_call(name: str, x, y, rows_per_batch, eps=1e-6, w=None, b=None, shift=None, scale=None, dy=None, dres=None, red1=None, red2=None, red_per_batch=False,
              rope=None, head_dim=0):
    rows, D = x.shape
    a = _lib.WanRowArgs()
    a.x, a.ld_x = x.data_ptr(), x.stride(0)
    a.w, a.b = ptr(w), ptr(b)
    a.shift, a.scale = ptr(shift), ptr(scale)
    a.mod_bstride = scale.stride(0) if scale is not None else 0
    if shift is not None and scale is not None and shift.stride(0) != scale.stride(0) and rows > rows_per_batch:
        raise ValueError("shift and scale must share their sample stride")
    a.dy, a.ld_dy = ptr(dy), (dy.stride(0) if dy is not None else 0)
    a.dres = ptr(dres)
    a.y, a.ld_y = ptr(y), (y.stride(0) if y is not None else 0)
    a.red1, a.red2, a.red_per_batch = ptr(red1), ptr(red2), int(bool(red_per_batch))
    if rope is not None:
        cos, sin = rope
        _f32(cos, "rope cos", (rows_per_batch, head_dim // 2))
        _f32(sin, "rope sin", (rows_per_batch, head_dim // 2))
        if not (cos.is_contiguous() and sin.is_contiguous()):
            raise ValueError("rope tables must be contiguous")
        a.rope_cos, a.rope_sin, a.head_dim = cos.data_ptr(), sin.data_ptr(), int(head_dim)
    a.rows, a.D, a.rows_per_batch, a.eps = rows, D, int(rows_per_batch), float(eps)
    check(getattr(_lib.load(), f"ftmi_wan_{name}")(ctypes.byref(a), stream_ptr()), f"ftmi_wan_{name}")


def wan_ln(x, rows_per_batch: int, w=None, b=None, shift=None, scale=None, eps: float = 1e-6, out=None):
    """y = bf(LN(float(x)) [* w + b] [* (1 + scale_b) + shift_b]); x [rows, D] bf16, shift / scale fp32 [B, D] views (sample stride free)."""
    x = _rows2d(x, "x")
    B = x.shape[0] // rows_per_batch
    out = torch.empty(x.shape, dtype=bf16, device=x.device) if out is None else _rows2d(out, "out")
    _wan_call("ln_fwd", x, out, rows_per_batch, eps, w=w, b=b, shift=_f32(shift, "shift", (B, x.shape[1])), scale=_f32(scale, "scale", (B, x.shape[1])))
    return out


def wan_ln_bwd(x, dy, rows_per_batch: int, w=None, scale=None, eps: float = 1e-6, dres=None, red1=None, red2=None, red_per_batch: bool = False):
    """dx = bf([dres +] bf(LN'(x)[dy * (w | 1 + scale_b)])); red1 += sum dy, red2 += sum dy * xhat (fp32 [B, D] views when red_per_batch, else [D])."""
    x, dy = _rows2d(x, "x"), _rows2d(dy, "dy")
    dx = torch.empty(x.shape, dtype=bf16, device=x.device)
    if dres is not None and (_rows2d(dres, "dres").stride(0) != dx.stride(0)):
        raise ValueError("dres must be contiguous like dx")
    B, D = x.shape[0] // rows_per_batch, x.shape[1]
    if red_per_batch:
        for r in (red1, red2):
            if r is not None and (tuple(r.shape) != (B, D) or r.stride(0) != D):
                raise ValueError("per-sample column sums must be contiguous [B, D] fp32")
    _wan_call("ln_bwd", x, dx, rows_per_batch, eps, w=w, scale=_f32(scale, "scale", (B, D)), dy=dy, dres=dres, red1=_f32(red1, "red1"), red2=_f32(red2, "red2"),
              red_per_batch=red_per_batch)
    return dx


def wan_rms_rope(x, w, rows_per_batch: int, rope=None, head_dim: int = 128, eps: float = 1e-6, out=None):
    x = _rows2d(x, "x")
    out = torch.empty(x.shape, dtype=bf16, device=x.device) if out is None else _rows2d(out, "out")
    _wan_call("rms_rope_fwd", x, out, rows_per_batch, eps, w=w, rope=rope, head_dim=head_dim)
    return out


def wan_rms_rope_bwd(x, w, dy, rows_per_batch: int, rope=None, head_dim: int = 128, eps: float = 1e-6, dweight=None, out=None):
    """dx of the RMSNorm (+ rotary) above; dweight (fp32 [D]) += sum dn * xhat."""
    x, dy = _rows2d(x, "x"), _rows2d(dy, "dy")
    out = torch.empty(x.shape, dtype=bf16, device=x.device) if out is None else _rows2d(out, "out")
    _wan_call("rms_rope_bwd", x, out, rows_per_batch, eps, w=w, dy=dy, rope=rope, head_dim=head_dim, red2=_f32(dweight, "dweight", (x.shape[1],)))
    return out


def wan_gate_res(x, y, rows_per_batch: int, gate=None, out=None):
    """out = bf(float(x) + float(y) * gate_b)  (gate fp32 [B, D]; None: bf(x + y))."""
    x, y = _rows2d(x, "x"), _rows2d(y, "y")
    out = torch.empty(x.shape, dtype=bf16, device=x.device) if out is None else _rows2d(out, "out")
    _wan_call("gate_res_fwd", x, out, rows_per_batch, scale=_f32(gate, "gate", (x.shape[0] // rows_per_batch, x.shape[1])), dy=y)
    return out


def wan_gate_res_bwd(dout, y, gate, rows_per_batch: int, dgate=None):
    """dy = bf(d out * gate_b); dgate (fp32 contiguous [B, D]) += sum_rows d out * y (dgate None -- a frozen gate: y is not read and may be None)."""
    if y is None and dgate is not None:
        raise ValueError("the gate's gradient needs the branch output y")
    dout, y = _rows2d(dout, "dout"), (None if y is None else _rows2d(y, "y"))
    B, D = dout.shape[0] // rows_per_batch, dout.shape[1]
    if dgate is not None and (tuple(dgate.shape) != (B, D) or dgate.stride(0) != D):
        raise ValueError("dgate must be contiguous [B, D] fp32")
    dy = torch.empty(dout.shape, dtype=bf16, device=dout.device)
    _wan_call("gate_res_bwd", dout, dy, rows_per_batch, scale=_f32(gate, "gate", (B, D)), dy=y, red1=_f32(dgate, "dgate"), red_per_batch=True)
    return dy


def wan_colsum(x, out):
    """out (fp32 [N]) += sum over the rows of x [rows, N] (bias gradients)."""
    x = _rows2d(x, "x")
    _wan_call("colsum", x, None, x.shape[0], red1=_f32(out, "out", (x.shape[1],)))
    return out


def grad_sumsq(grads: torch.Tensor, scratch: torch.Tensor) -> torch.Tensor:
    """scratch[0] <- sum g^2 of a flat fp32 gradient (shard), order-fixed; returns scratch[:1]."""
    require_gpu_tensor(grads, "grads", torch.float32)
    if scratch.numel() < CLIP_SCRATCH_FLOATS or scratch.dtype != torch.float32:
        raise ValueError(f"grad_sumsq: scratch must hold {CLIP_SCRATCH_FLOATS} fp32 values")
    check(_lib.load().ftmi_grad_sumsq(ptr(grads), grads.numel(), ptr(scratch), stream_ptr()), "ftmi_grad_sumsq")
    return scratch[:1]


def adamw_bf16_step(params, grads, exp_avg, exp_avg_sq, step: int, lr: float, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 1e-4,
                    sumsq: Optional[torch.Tensor] = None, max_norm: float = 1.0, grad_norm_out: Optional[torch.Tensor] = None) -> None:
    """torch.optim.AdamW on flat bf16 parameters / moments with an fp32 gradient (clipped by the global norm sqrt(sumsq[0]) when given)."""
    for t, n in ((params, "params"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        require_gpu_tensor(t, n, bf16)
    require_gpu_tensor(grads, "grads", torch.float32)
    if not (params.numel() == grads.numel() == exp_avg.numel() == exp_avg_sq.numel()):
        raise ValueError("adamw_bf16_step: size mismatch")
    check(_lib.load().ftmi_adamw_bf16_step(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), ptr(sumsq), float(max_norm), float(lr),
                                            float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step), ptr(grad_norm_out), stream_ptr()),
          "ftmi_adamw_bf16_step")


def clip_by_sumsq_(grads: torch.Tensor, sumsq: torch.Tensor, max_norm: float, grad_norm_out: Optional[torch.Tensor] = None) -> None:
    """grads (flat fp32) *= min(1, max_norm / (sqrt(sumsq[0]) + 1e-6)), in place."""
    require_gpu_tensor(grads, "grads", torch.float32)
    require_gpu_tensor(sumsq, "sumsq", torch.float32)
    check(_lib.load().ftmi_clip_by_sumsq(ptr(grads), grads.numel(), ptr(sumsq), float(max_norm), ptr(grad_norm_out), stream_ptr()), "ftmi_clip_by_sumsq")


# ---- HunyuanVideo (include/ftmi355.h: ftmi_head_rms_rope_*) ----------------------------------------------------------------------------------
def head_rms_rope(x2d, w, head_dim: int = 128, eps: float = 1e-6, rope=None, rows_per_batch: int = 0, rope_from: int = 0, out=None):
    """Per-head RMSNorm of x2d [rows, D] (a bf16 view, any row stride % 8) + real-form rotary embedding on the rows at position >= rope_from of each sample."""
    x2d = _rows2d(x2d, "x")
    rows, D = x2d.shape
    out = torch.empty((rows, D), dtype=bf16, device=x2d.device) if out is None else _rows2d(out, "out")
    cos, sin = (None, None) if rope is None else rope
    if rope is not None:
        n = (rows_per_batch or rows) - rope_from
        _f32(cos, "rope cos", (n, head_dim))
        _f32(sin, "rope sin", (n, head_dim))
    check(_lib.load().ftmi_head_rms_rope_fwd(ptr(x2d), x2d.stride(0), ptr(w), ptr(out), out.stride(0), rows, D, int(head_dim), float(eps), ptr(cos), ptr(sin),
                                             int(rows_per_batch or rows), int(rope_from), stream_ptr()), "ftmi_head_rms_rope_fwd")
    return out


def head_rms_rope_bwd(x2d, w, dy2d, head_dim: int = 128, eps: float = 1e-6, rope=None, rows_per_batch: int = 0, rope_from: int = 0, out=None):
    x2d, dy2d = _rows2d(x2d, "x"), _rows2d(dy2d, "dy")
    rows, D = x2d.shape
    out = torch.empty((rows, D), dtype=bf16, device=x2d.device) if out is None else _rows2d(out, "out")
    cos, sin = (None, None) if rope is None else rope
    check(_lib.load().ftmi_head_rms_rope_bwd(ptr(x2d), x2d.stride(0), ptr(w), ptr(dy2d), dy2d.stride(0), ptr(out), out.stride(0), rows, D, int(head_dim), float(eps),
                                             ptr(cos), ptr(sin), int(rows_per_batch or rows), int(rope_from), stream_ptr()), "ftmi_head_rms_rope_bwd")
    return out


# ---- Wan control LoRA outside the blocks (csrc/wan_control.hip) -----------------------------------------------------------------------------------
def f32_gemm(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, scale: float = 1.0, accumulate: bool = False,
             hi_lo: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [M, N] (fp32) = (accumulate ? out : 0) + scale * a [M, K] @ b [K, N] in fp32 FMAs with a fixed accumulation order.  ``a`` and ``b`` are 2-D fp32 views
    of any strides (pass ``w.t()`` for a transposed operand: nothing is copied).  ``hi_lo`` [M, >= 2N] bf16: also receives the result's [hi | lo] planes."""
    require_gpu_tensor(a, "a", torch.float32)
    require_gpu_tensor(b, "b", torch.float32)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0]:
        raise ValueError(f"f32_gemm: a {tuple(a.shape)} and b {tuple(b.shape)} do not multiply")
    M, K = a.shape
    N = b.shape[1]
    if out is None:
        if accumulate:
            raise ValueError("f32_gemm: accumulate needs out")
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    require_gpu_tensor(out, "out", torch.float32)
    if out.shape != (M, N) or out.stride(1) != 1:
        raise ValueError("f32_gemm: out must be an [M, N] fp32 view with contiguous columns")
    ld_hl = 0
    if hi_lo is not None:
        require_gpu_tensor(hi_lo, "hi_lo", bf16)
        if hi_lo.dim() != 2 or hi_lo.shape[0] != M or hi_lo.shape[1] < 2 * N or hi_lo.stride(1) != 1:
            raise ValueError("f32_gemm: hi_lo must be an [M, >= 2N] bf16 view with contiguous columns")
        ld_hl = hi_lo.stride(0)
    check(_lib.load().ftmi_f32_gemm(M, N, K, ptr(a), a.stride(0), a.stride(1), ptr(b), b.stride(0), b.stride(1), ptr(out), out.stride(0), float(scale),
                                     int(bool(accumulate)), ptr(hi_lo), ld_hl, stream_ptr()), "ftmi_f32_gemm")
    return out


def wan_control_pack(moments, control_moments, noise, sigmas, latents_mean, latents_std, keep, patch_size=(1, 2, 2)):
    """-> (cols2 [B S, 2 Kp] bf16 = [cols | cols], target [B, C, F, H, W] bf16): include/ftmi355.h, ftmi_wan_control_pack.  ``keep`` [B, F] uint8."""
    for n, t in (("moments", moments), ("control_moments", control_moments), ("noise", noise)):
        require_gpu_tensor(t, n, bf16)
    for n, t in (("sigmas", sigmas), ("latents_mean", latents_mean), ("latents_std", latents_std)):
        require_gpu_tensor(t, n, torch.float32)
    require_gpu_tensor(keep, "keep", torch.uint8)
    B, C, F_, H, W = noise.shape
    Fc = control_moments.shape[2]
    if tuple(moments.shape) != (B, 2 * C, F_, H, W) or tuple(control_moments.shape) != (B, 2 * C, Fc, H, W):
        raise ValueError(f"wan_control_pack: moments {tuple(moments.shape)} / control moments {tuple(control_moments.shape)} do not go with noise {tuple(noise.shape)}")
    if sigmas.numel() != B or latents_mean.numel() != C or latents_std.numel() != C or tuple(keep.shape) != (B, F_):
        raise ValueError("wan_control_pack: sigmas [B], latents_mean / latents_std [C] and keep [B, F] expected")
    pt, ph, pw = patch_size
    if F_ % pt or H % ph or W % pw:
        raise ValueError("wan_control_pack: the latent size must be whole patches")
    S, Kp = (F_ // pt) * (H // ph) * (W // pw), 2 * C * pt * ph * pw
    cols2 = torch.empty((B * S, 2 * Kp), dtype=bf16, device=noise.device)
    target = torch.empty_like(noise, memory_format=torch.contiguous_format)
    cfg = _lib.WanControlPackConfig(B=B, C=C, F=F_, Fc=Fc, H=H, W=W, pt=pt, ph=ph, pw=pw)
    args = [t.contiguous() for t in (moments, control_moments, noise, sigmas, latents_mean, latents_std, keep)]
    check(_lib.load().ftmi_wan_control_pack(ctypes.byref(cfg), *[ptr(t) for t in args], ptr(cols2), ptr(target), stream_ptr()), "ftmi_wan_control_pack")
    return cols2, target


def _patch_lora_cfg(M: int, D: int, Kp: int, r: int, s: float, refold: bool, variant: int):
    return _lib.WanPatchLoraConfig(M=M, D=D, Kp=Kp, r=r, s=float(s), gemm_variant=variant, refold=int(bool(refold)))


def wan_patch_lora_forward(cols2, w, bias, lora_a, lora_b, dw, w2, s: float = 1.0, refold: bool = True, variant: int = 8, out=None):
    """y [M, D] = bf(bf(cols W^T + b) + s (cols A^T) B^T) through the folded adapter (ftmi_wan_patch_lora_forward).  cols2 [M, 2 Kp] = [cols | cols]; w [D, Kp] bf16;
    lora_a [r, Kp], lora_b [D, r] fp32; dw [D, Kp] fp32 and w2 [D, 2 Kp] bf16 are the caller's fold buffers (``refold=False`` reuses w2)."""
    M, Kp = cols2.shape[0], cols2.shape[1] // 2
    D, r = lora_b.shape
    for n, t, dt, shape in (("cols2", cols2, bf16, (M, 2 * Kp)), ("w", w, bf16, (D, Kp)), ("lora_a", lora_a, torch.float32, (r, Kp)), ("lora_b", lora_b, torch.float32, (D, r)),
                            ("dw", dw, torch.float32, (D, Kp)), ("w2", w2, bf16, (D, 2 * Kp))):
        require_gpu_tensor(t, n, dt)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"wan_patch_lora_forward: {n} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
    if out is None:
        out = torch.empty((M, D), dtype=bf16, device=cols2.device)
    cfg = _patch_lora_cfg(M, D, Kp, r, s, refold, variant)
    check(_lib.load().ftmi_wan_patch_lora_forward(ctypes.byref(cfg), ptr(w), ptr(bias), ptr(lora_a), ptr(lora_b), ptr(cols2), ptr(dw), ptr(w2), ptr(out), stream_ptr()),
          "ftmi_wan_patch_lora_forward")
    return out


def wan_patch_lora_backward(cols2, dx0, lora_a, lora_b, g_ws, grad_a, grad_b, s: float = 1.0) -> None:
    """grad_a [r, Kp] += s B^T G, grad_b [D, r] += s G A^T with G = dx0^T cols written to g_ws [D, Kp] fp32 (ftmi_wan_patch_lora_backward)."""
    M, Kp = cols2.shape[0], cols2.shape[1] // 2
    D, r = lora_b.shape
    for n, t, dt, shape in (("cols2", cols2, bf16, (M, 2 * Kp)), ("dx0", dx0, bf16, (M, D)), ("lora_a", lora_a, torch.float32, (r, Kp)), ("lora_b", lora_b, torch.float32, (D, r)),
                            ("g_ws", g_ws, torch.float32, (D, Kp)), ("grad_a", grad_a, torch.float32, (r, Kp)), ("grad_b", grad_b, torch.float32, (D, r))):
        require_gpu_tensor(t, n, dt)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"wan_patch_lora_backward: {n} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
    cfg = _patch_lora_cfg(M, D, Kp, r, s, False, 8)
    check(_lib.load().ftmi_wan_patch_lora_backward(ctypes.byref(cfg), ptr(lora_a), ptr(lora_b), ptr(cols2), ptr(dx0), ptr(g_ws), ptr(grad_a), ptr(grad_b), stream_ptr()),
          "ftmi_wan_patch_lora_backward")


# ---- Wan latent sampling (include/ftmi355.h: ftmi_wan_sample_*; csrc/sample_layout.hip, csrc/wan_sample_dit.hip) -------------------------------------------
def wan_sample_geometry(B: int, C: int, frames: int, height: int, width: int, Kp: int, extra_channels: int = 0, copies: int = 1, guidance: bool = True,
                        patch_size=(1, 2, 2), po: Optional[int] = None) -> "_lib.WanSampleGeometry":
    """The layout of a sampling run: latents [B, C, frames, height, width] (+ ``extra_channels``), cols [P B S, copies Kp], pred [P B, S, po]."""
    pt, ph, pw = patch_size
    return _lib.WanSampleGeometry(B=B, C=C, Cx=extra_channels, F=frames, H=height, W=width, pt=pt, ph=ph, pw=pw, Kp=Kp, copies=copies, P=2 if guidance else 1,
                                  po=C * pt * ph * pw if po is None else po)


def _wan_sample_tokens(geo) -> int:
    if geo.F % geo.pt or geo.H % geo.ph or geo.W % geo.pw:
        raise ValueError("wan_sample: the latent size must be whole patches")
    return (geo.F // geo.pt) * (geo.H // geo.ph) * (geo.W // geo.pw)


def _wan_sample_buffers(geo, x, cols, what: str) -> None:
    S, Kc = _wan_sample_tokens(geo), geo.C * geo.pt * geo.ph * geo.pw
    if x is not None and (tuple(x.shape) != (geo.B, S, Kc) or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda):
        raise ValueError(f"{what}: x must be a contiguous fp32 [{geo.B}, {S}, {Kc}] GPU tensor, got {tuple(x.shape)}")
    if cols is not None and (tuple(cols.shape) != (geo.P * geo.B * S, geo.copies * geo.Kp) or cols.dtype != bf16 or not cols.is_contiguous() or not cols.is_cuda):
        raise ValueError(f"{what}: cols must be a contiguous bf16 [{geo.P * geo.B * S}, {geo.copies * geo.Kp}] GPU tensor, got {tuple(cols.shape)}")


def wan_sample_init(geo, latents, extra=None, x=None, cols=None):
    """latents fp32 [B, C, F, H, W] (+ extra bf16 [B, Cx, F, H, W]) -> (x fp32 [B, S, Kc], cols bf16 [P B S, copies Kp]): ftmi_wan_sample_init."""
    require_gpu_tensor(latents, "latents", torch.float32)
    if tuple(latents.shape) != (geo.B, geo.C, geo.F, geo.H, geo.W) or not latents.is_contiguous():
        raise ValueError(f"wan_sample_init: latents must be contiguous [{geo.B}, {geo.C}, {geo.F}, {geo.H}, {geo.W}], got {tuple(latents.shape)}")
    if (extra is not None) != (geo.Cx > 0):
        raise ValueError("wan_sample_init: the extra channels go with their tensor, and only with it")
    if extra is not None:
        require_gpu_tensor(extra, "extra", bf16)
        if tuple(extra.shape) != (geo.B, geo.Cx, geo.F, geo.H, geo.W) or not extra.is_contiguous():
            raise ValueError(f"wan_sample_init: extra must be contiguous [{geo.B}, {geo.Cx}, {geo.F}, {geo.H}, {geo.W}], got {tuple(extra.shape)}")
    S, Kc = _wan_sample_tokens(geo), geo.C * geo.pt * geo.ph * geo.pw
    x = torch.empty((geo.B, S, Kc), dtype=torch.float32, device=latents.device) if x is None else x
    cols = torch.empty((geo.P * geo.B * S, geo.copies * geo.Kp), dtype=bf16, device=latents.device) if cols is None else cols
    _wan_sample_buffers(geo, x, cols, "wan_sample_init")
    check(_lib.load().ftmi_wan_sample_init(ctypes.byref(geo), ptr(latents), ptr(extra), ptr(x), ptr(cols), stream_ptr()), "ftmi_wan_sample_init")
    return x, cols


def wan_sample_step(geo, pred, x, sigma, sigma_next, guidance: float, cols=None) -> None:
    """One sampler step in place (ftmi_wan_sample_step): pred bf16 [P B, S, po] (None: only the bf16 copies), x fp32 [B, S, Kc], sigma / sigma_next fp32 [B] on
    the device, cols bf16 [P B S, copies Kp] (None: only the update)."""
    _wan_sample_buffers(geo, x, cols, "wan_sample_step")
    S = _wan_sample_tokens(geo)
    if pred is not None:
        require_gpu_tensor(pred, "pred", bf16)
        if pred.numel() != geo.P * geo.B * S * geo.po or not pred.is_contiguous():
            raise ValueError(f"wan_sample_step: pred must be contiguous [{geo.P * geo.B}, {S}, {geo.po}], got {tuple(pred.shape)}")
        for n, t in (("sigma", sigma), ("sigma_next", sigma_next)):
            require_gpu_tensor(t, n, torch.float32)
            if t.numel() != geo.B or not t.is_contiguous():
                raise ValueError(f"wan_sample_step: {n} holds one value per sample")
    check(_lib.load().ftmi_wan_sample_step(ctypes.byref(geo), ptr(pred), ptr(x), ptr(sigma), ptr(sigma_next), float(guidance), ptr(cols), stream_ptr()),
          "ftmi_wan_sample_step")


def wan_sample_step_unipc(geo, pred, x, last, m1, m2, coef_row, sigma, guidance: float, cols=None) -> None:
    """One step of the multistep (UniPC) sampler in place (ftmi_wan_sample_step_unipc): pred bf16 [P B, S, po]; x / last / m1 / m2 fp32 [B, S, Kc], four buffers
    -- x receives the predictor's state, last the corrected one, m2 (the OLDER history buffer) this step's data prediction: swap m1 and m2 after the call;
    coef_row fp32 [8] (a row of ``wan_unipc_tables``) and sigma fp32 [1] on the device; cols bf16 [P B S, copies Kp] (None: no copies)."""
    _wan_sample_buffers(geo, x, cols, "wan_sample_step_unipc")
    S = _wan_sample_tokens(geo)
    require_gpu_tensor(pred, "pred", bf16)
    if pred.numel() != geo.P * geo.B * S * geo.po or not pred.is_contiguous():
        raise ValueError(f"wan_sample_step_unipc: pred must be contiguous [{geo.P * geo.B}, {S}, {geo.po}], got {tuple(pred.shape)}")
    for n, t in (("last", last), ("m1", m1), ("m2", m2)):
        require_gpu_tensor(t, n, torch.float32)
        if tuple(t.shape) != tuple(x.shape) or not t.is_contiguous():
            raise ValueError(f"wan_sample_step_unipc: {n} must be a contiguous fp32 {list(x.shape)} tensor like x, got {tuple(t.shape)}")
    for n, t, k in (("coef_row", coef_row, 8), ("sigma", sigma, 1)):
        require_gpu_tensor(t, n, torch.float32)
        if t.numel() != k or not t.is_contiguous():
            raise ValueError(f"wan_sample_step_unipc: {n} holds {k} contiguous value(s)")
    check(_lib.load().ftmi_wan_sample_step_unipc(ctypes.byref(geo), ptr(pred), ptr(x), ptr(last), ptr(m1), ptr(m2), ptr(coef_row), ptr(sigma), float(guidance),
                                                 ptr(cols), stream_ptr()), "ftmi_wan_sample_step_unipc")


def wan_sample_finish(geo, x, mean, std):
    """x fp32 [B, S, Kc] -> latents bf16 [B, C, F, H, W] = bf16(x * std[c] + mean[c]); ``std`` is the VAE's standard deviation itself (ftmi_wan_sample_finish)."""
    _wan_sample_buffers(geo, x, None, "wan_sample_finish")
    for n, t in (("mean", mean), ("std", std)):
        require_gpu_tensor(t, n, torch.float32)
        if t.numel() != geo.C or not t.is_contiguous():
            raise ValueError(f"wan_sample_finish: {n} holds one value per channel")
    out = torch.empty((geo.B, geo.C, geo.F, geo.H, geo.W), dtype=bf16, device=x.device)
    check(_lib.load().ftmi_wan_sample_finish(ctypes.byref(geo), ptr(x), ptr(mean), ptr(std), ptr(out), stream_ptr()), "ftmi_wan_sample_finish")
    return out


def wan_sample_mod(tables, tproj, rows: int):
    """mod fp32 [L, rows, 6, D] = float(tables[l]) + float(tproj) for the L blocks' scale_shift_table views (bf16, 6 D elements each) and one step's time
    projection bf16 [6 D] (ftmi_wan_sample_mod)."""
    L, D = len(tables), tproj.numel() // 6
    for t in list(tables) + [tproj]:
        require_gpu_tensor(t, "scale_shift_table / tproj", bf16)
        if t.numel() != 6 * D or not t.is_contiguous():
            raise ValueError("wan_sample_mod: every table and the time projection hold 6 D contiguous values")
    out = torch.empty((L, rows, 6, D), dtype=torch.float32, device=tproj.device)
    arr = (ctypes.c_void_p * L)(*[t.data_ptr() for t in tables])
    check(_lib.load().ftmi_wan_sample_mod(arr, L, ptr(tproj), ptr(out), int(rows), D, stream_ptr()), "ftmi_wan_sample_mod")
    return out


def wan_sample_workspace_bytes(cfg) -> int:
    n = int(_lib.load().ftmi_wan_sample_workspace_bytes(ctypes.byref(cfg)))
    if n == 0:
        raise ValueError(f"wan_sample: {_lib.last_error()}")
    return n


def _wan_sample_loop_inputs(cfg, cols, x, tproj, head_shift, head_scale, enc, enc_img, rope, sigmas, coef=None) -> None:
    """The tensor checks of ``wan_sample`` and ``wan_sample_ms`` (``coef``: the multistep table fp32 [steps, 8])."""
    geo, n, D = cfg.geo, cfg.steps, cfg.D
    _wan_sample_buffers(geo, x, cols, "wan_sample")
    S, rows = _wan_sample_tokens(geo), geo.P * geo.B
    want = [("tproj", tproj, bf16, (n, 6 * D)), ("head_shift", head_shift, torch.float32, (n, D)), ("head_scale", head_scale, torch.float32, (n, D)),
            ("enc", enc, bf16, (rows, cfg.T, D)), ("rope cos", rope[0], torch.float32, (S, 64)), ("rope sin", rope[1], torch.float32, (S, 64)),
            ("sigmas", sigmas, torch.float32, (n + 1,))]
    if cfg.TI > 0:
        want.append(("enc_img", enc_img, bf16, (rows, cfg.TI + cfg.TI2, D)))
    if coef is not None:
        want.append(("coef", coef, torch.float32, (n, 8)))
    for name, t, dt, shape in want:
        if t is None or not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"wan_sample: {name} must be a contiguous {dt} {shape} GPU tensor, got {None if t is None else tuple(t.shape)}")


def wan_sample_ms_config(cfg, solver: int = 1) -> "_lib.WanSampleMsConfig":
    """ftmi_wan_sample_ms_config over a ``WanSampleConfig`` (``solver`` 1: UniPC)."""
    return _lib.WanSampleMsConfig(base=cfg, solver=solver)


def wan_sample_ms_workspace_bytes(cfg, solver: int = 1) -> int:
    n = int(_lib.load().ftmi_wan_sample_ms_workspace_bytes(ctypes.byref(wan_sample_ms_config(cfg, solver))))
    if n == 0:
        raise ValueError(f"wan_sample_ms: {_lib.last_error()}")
    return n


def wan_sample_ms(cfg, weights, cols, x, tproj, head_shift, head_scale, enc, enc_img, rope, coef, sigmas, workspace=None, solver: int = 1) -> None:
    """``wan_sample`` with the multistep (UniPC) step (ftmi_wan_sample_ms): ``cfg`` is the same ``WanSampleConfig``; coef fp32 [steps, 8] (``wan_unipc_tables``) and
    sigmas fp32 [steps + 1] on the device.  ``workspace``: at least ``wan_sample_ms_workspace_bytes(cfg)`` bytes -- the solver's history lives there."""
    if coef is None:
        raise ValueError("wan_sample_ms: the coefficient table is missing")
    _wan_sample_loop_inputs(cfg, cols, x, tproj, head_shift, head_scale, enc, enc_img, rope, sigmas, coef)
    need = wan_sample_ms_workspace_bytes(cfg, solver)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    ms = wan_sample_ms_config(cfg, solver)
    check(_lib.load().ftmi_wan_sample_ms(ctypes.byref(ms), ctypes.byref(weights), ptr(cols), ptr(x), ptr(tproj), ptr(head_shift), ptr(head_scale), ptr(enc),
                                         ptr(enc_img if cfg.TI > 0 else None), ptr(rope[0]), ptr(rope[1]), ptr(coef), ptr(sigmas), ptr(workspace),
                                         workspace.numel(), stream_ptr()), "ftmi_wan_sample_ms")


def wan_sample(cfg, weights, cols, x, tproj, head_shift, head_scale, enc, enc_img, rope, sigmas, workspace=None) -> None:
    """The whole denoising loop in ONE call (ftmi_wan_sample), in place on ``x`` / ``cols`` (as ``wan_sample_init`` wrote them).  tproj bf16 [steps, 6 D];
    head_shift / head_scale fp32 [steps, D]; enc bf16 [P B, T, D] (unconditional rows first); enc_img bf16 [P B, TI + TI2, D] or None; rope = (cos, sin) fp32 [S, 64];
    sigmas fp32 [steps + 1] on the device.  ``workspace``: a uint8 GPU tensor of at least ``wan_sample_workspace_bytes(cfg)`` (allocated when None)."""
    _wan_sample_loop_inputs(cfg, cols, x, tproj, head_shift, head_scale, enc, enc_img, rope, sigmas)
    need = wan_sample_workspace_bytes(cfg)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    check(_lib.load().ftmi_wan_sample(ctypes.byref(cfg), ctypes.byref(weights), ptr(cols), ptr(x), ptr(tproj), ptr(head_shift), ptr(head_scale), ptr(enc),
                                      ptr(enc_img if cfg.TI > 0 else None), ptr(rope[0]), ptr(rope[1]), ptr(sigmas), ptr(workspace), workspace.numel(),
                                      stream_ptr()), "ftmi_wan_sample")


# ---- CogVideoX latent sampling (include/ftmi355.h: ftmi_cog_sample_*; csrc/sample_layout.hip, csrc/cog_dit.hip) ---------------------------------------------
def cog_sample_geometry(B: int, C: int, frames: int, height: int, width: int, patch: int = 2, patch_t: Optional[int] = None, guidance: bool = True,
                        drop: int = 0) -> "_lib.CogSampleGeometry":
    """The layout of a sampling run: latents [B, frames, C, height, width], x [B, S, Kc], cols [P B S, Kc], pred [P B, S, Kc]; ``drop``: the padded leading
    frames that ``cog_sample_finish`` leaves out."""
    return _lib.CogSampleGeometry(B=B, C=C, F=frames, H=height, W=width, p=patch, pt=patch_t or 1, P=2 if guidance else 1, drop=drop)


def _cog_sample_dims(geo) -> Tuple[int, int]:
    if geo.F % geo.pt or geo.H % geo.p or geo.W % geo.p:
        raise ValueError("cog_sample: the latent size must be whole patches")
    return (geo.F // geo.pt) * (geo.H // geo.p) * (geo.W // geo.p), geo.C * geo.pt * geo.p * geo.p


def _cog_sample_buffers(geo, x, cols, what: str) -> None:
    S, Kc = _cog_sample_dims(geo)
    if x is not None and (tuple(x.shape) != (geo.B, S, Kc) or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda):
        raise ValueError(f"{what}: x must be a contiguous fp32 [{geo.B}, {S}, {Kc}] GPU tensor, got {tuple(x.shape)}")
    if cols is not None and (tuple(cols.shape) != (geo.P * geo.B * S, Kc) or cols.dtype != bf16 or not cols.is_contiguous() or not cols.is_cuda):
        raise ValueError(f"{what}: cols must be a contiguous bf16 [{geo.P * geo.B * S}, {Kc}] GPU tensor, got {tuple(cols.shape)}")


def cog_sample_init(geo, latents, x=None, cols=None):
    """noise fp32 [B, F, C, H, W] -> (x fp32 [B, S, Kc], cols bf16 [P B S, Kc]): ftmi_cog_sample_init."""
    require_gpu_tensor(latents, "latents", torch.float32)
    if tuple(latents.shape) != (geo.B, geo.F, geo.C, geo.H, geo.W) or not latents.is_contiguous():
        raise ValueError(f"cog_sample_init: latents must be contiguous [{geo.B}, {geo.F}, {geo.C}, {geo.H}, {geo.W}], got {tuple(latents.shape)}")
    S, Kc = _cog_sample_dims(geo)
    x = torch.empty((geo.B, S, Kc), dtype=torch.float32, device=latents.device) if x is None else x
    cols = torch.empty((geo.P * geo.B * S, Kc), dtype=bf16, device=latents.device) if cols is None else cols
    _cog_sample_buffers(geo, x, cols, "cog_sample_init")
    check(_lib.load().ftmi_cog_sample_init(ctypes.byref(geo), ptr(latents), ptr(x), ptr(cols), stream_ptr()), "ftmi_cog_sample_init")
    return x, cols


def cog_sample_step(geo, pred, x, coef, step: int, guidance: float, cols=None) -> None:
    """One sampler step in place (ftmi_cog_sample_step): pred bf16 [P B, S, Kc] (None: only the bf16 copies), x fp32 [B, S, Kc], coef fp32 [n, 2] on the device
    (row ``step`` = (cx, cv): x <- cx x + cv v), cols bf16 [P B S, Kc] (None: only the update)."""
    _cog_sample_buffers(geo, x, cols, "cog_sample_step")
    S, Kc = _cog_sample_dims(geo)
    if pred is not None:
        require_gpu_tensor(pred, "pred", bf16)
        if pred.numel() != geo.P * geo.B * S * Kc or not pred.is_contiguous():
            raise ValueError(f"cog_sample_step: pred must be contiguous [{geo.P * geo.B}, {S}, {Kc}], got {tuple(pred.shape)}")
        require_gpu_tensor(coef, "coef", torch.float32)
        if coef.dim() != 2 or coef.shape[1] != 2 or not coef.is_contiguous() or not 0 <= int(step) < coef.shape[0]:
            raise ValueError("cog_sample_step: coef is a contiguous fp32 [n, 2] table and step one of its rows")
    check(_lib.load().ftmi_cog_sample_step(ctypes.byref(geo), ptr(pred), ptr(x), ptr(coef), int(step), float(guidance), ptr(cols), stream_ptr()),
          "ftmi_cog_sample_step")


def cog_sample_finish(geo, x, k: float):
    """x fp32 [B, S, Kc] -> latents bf16 [B, F - drop, C, H, W] = bf16(x * k) (ftmi_cog_sample_finish)."""
    _cog_sample_buffers(geo, x, None, "cog_sample_finish")
    out = torch.empty((geo.B, geo.F - geo.drop, geo.C, geo.H, geo.W), dtype=bf16, device=x.device)
    check(_lib.load().ftmi_cog_sample_finish(ctypes.byref(geo), ptr(x), float(k), ptr(out), stream_ptr()), "ftmi_cog_sample_finish")
    return out


def cog_sample_workspace_bytes(cfg) -> int:
    n = int(_lib.load().ftmi_cog_sample_workspace_bytes(ctypes.byref(cfg)))
    if n == 0:
        raise ValueError(f"cog_sample: {_lib.last_error()}")
    return n


def cog_sample(cfg, weights, cols, x, text, temb_silu, head_shift, head_onep, coef, workspace=None) -> None:
    """The whole denoising loop in ONE call (ftmi_cog_sample), in place on ``x`` / ``cols`` (as ``cog_sample_init`` wrote them).  text bf16 [P B, T, D_text]
    (unconditional rows first); temb_silu bf16 [steps, P B, D_temb]; head_shift / head_onep bf16 [steps, D]; coef fp32 [steps, 2] on the device.
    ``workspace``: a uint8 GPU tensor of at least ``cog_sample_workspace_bytes(cfg)`` (allocated when None)."""
    geo, n, D = cfg.geo, cfg.steps, cfg.D
    _cog_sample_buffers(geo, x, cols, "cog_sample")
    rows = geo.P * geo.B
    want = [("text", text, bf16, (rows, cfg.T, cfg.D_text)), ("temb_silu", temb_silu, bf16, (n, rows, cfg.D_temb)), ("head_shift", head_shift, bf16, (n, D)),
            ("head_onep", head_onep, bf16, (n, D)), ("coef", coef, torch.float32, (n, 2))]
    for name, t, dt, shape in want:
        if t is None or not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"cog_sample: {name} must be a contiguous {dt} {shape} GPU tensor, got {None if t is None else tuple(t.shape)}")
    need = cog_sample_workspace_bytes(cfg)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    check(_lib.load().ftmi_cog_sample(ctypes.byref(cfg), ctypes.byref(weights), ptr(cols), ptr(x), ptr(text), ptr(temb_silu), ptr(head_shift), ptr(head_onep),
                                      ptr(coef), ptr(workspace), workspace.numel(), stream_ptr()), "ftmi_cog_sample")


def cog_sample_step_dpm(geo, pred, x, old, noise, coef_row, cols=None) -> None:
    """One step of the multistep (DPM) sampler in place (ftmi_cog_sample_step_dpm): pred bf16 [P B, S, Kc]; x / old fp32 [B, S, Kc], two buffers (x <- x',
    old <- x0); noise fp32 [B, S, Kc], the step's slice in the state's layout, or None for a row with mn == 0; coef_row fp32 [8] on the device
    (``cog_dpm_tables``: sa, sb, m0, e0, e1, mn, g, 0); cols bf16 [P B S, Kc] (None: only the update)."""
    _cog_sample_buffers(geo, x, cols, "cog_sample_step_dpm")
    S, Kc = _cog_sample_dims(geo)
    require_gpu_tensor(pred, "pred", bf16)
    if pred.numel() != geo.P * geo.B * S * Kc or not pred.is_contiguous():
        raise ValueError(f"cog_sample_step_dpm: pred must be contiguous [{geo.P * geo.B}, {S}, {Kc}], got {tuple(pred.shape)}")
    for n, t in (("old", old), ("noise", noise)):
        if t is None and n == "noise":
            continue
        require_gpu_tensor(t, n, torch.float32)
        if tuple(t.shape) != tuple(x.shape) or not t.is_contiguous():
            raise ValueError(f"cog_sample_step_dpm: {n} must be a contiguous fp32 {list(x.shape)} tensor like x, got {tuple(t.shape)}")
    require_gpu_tensor(coef_row, "coef_row", torch.float32)
    if coef_row.numel() != 8 or not coef_row.is_contiguous():
        raise ValueError("cog_sample_step_dpm: coef_row holds 8 contiguous values")
    check(_lib.load().ftmi_cog_sample_step_dpm(ctypes.byref(geo), ptr(pred), ptr(x), ptr(old), ptr(noise), ptr(coef_row), ptr(cols), stream_ptr()),
          "ftmi_cog_sample_step_dpm")


def cog_sample_pack(geo, latents, out=None):
    """latents fp32 [n, B, F, C, H, W] -> fp32 [n, B, S, Kc], ``cog_sample_init``'s permutation over n tensors at once (ftmi_cog_sample_pack).  ``out``: a
    contiguous fp32 [>= n, B, S, Kc] GPU tensor whose first n slices are written (allocated when None)."""
    require_gpu_tensor(latents, "latents", torch.float32)
    if latents.dim() != 6 or tuple(latents.shape[1:]) != (geo.B, geo.F, geo.C, geo.H, geo.W) or not latents.is_contiguous() or latents.shape[0] < 1:
        raise ValueError(f"cog_sample_pack: latents must be contiguous [n, {geo.B}, {geo.F}, {geo.C}, {geo.H}, {geo.W}], got {tuple(latents.shape)}")
    n = latents.shape[0]
    S, Kc = _cog_sample_dims(geo)
    out = torch.empty((n, geo.B, S, Kc), dtype=torch.float32, device=latents.device) if out is None else out
    if not out.is_cuda or out.dtype != torch.float32 or out.dim() != 4 or tuple(out.shape[1:]) != (geo.B, S, Kc) or out.shape[0] < n or not out.is_contiguous():
        raise ValueError(f"cog_sample_pack: out must be a contiguous fp32 [>= {n}, {geo.B}, {S}, {Kc}] GPU tensor, got {tuple(out.shape)}")
    check(_lib.load().ftmi_cog_sample_pack(ctypes.byref(geo), ptr(latents), n, ptr(out), stream_ptr()), "ftmi_cog_sample_pack")
    return out


def cog_sample_ms_config(cfg, solver: int = 1) -> "_lib.CogSampleMsConfig":
    """ftmi_cog_sample_ms_config over a ``CogSampleConfig`` (``solver`` 1: DPM)."""
    return _lib.CogSampleMsConfig(base=cfg, solver=int(solver))


def cog_sample_ms_workspace_bytes(cfg, solver: int = 1) -> int:
    n = int(_lib.load().ftmi_cog_sample_ms_workspace_bytes(ctypes.byref(cog_sample_ms_config(cfg, solver))))
    if n == 0:
        raise ValueError(f"cog_sample_ms: {_lib.last_error()}")
    return n


def cog_sample_ms(cfg, weights, cols, x, text, temb_silu, head_shift, head_onep, coef, noise=None, workspace=None, solver: int = 1) -> None:
    """``cog_sample`` with the multistep (DPM) step (ftmi_cog_sample_ms): ``cfg`` is the same ``CogSampleConfig``; coef fp32 [steps, 8] (``cog_dpm_tables``) on the
    device; noise fp32 [k, B, S, Kc] (``cog_sample_pack``), the slices of the k <= steps leading steps -- every later row must have mn == 0 -- or None when no
    row has noise.  ``workspace``: at least ``cog_sample_ms_workspace_bytes(cfg)`` bytes -- the previous x0 prediction lives there."""
    geo, n, D = cfg.geo, cfg.steps, cfg.D
    _cog_sample_buffers(geo, x, cols, "cog_sample_ms")
    S, Kc = _cog_sample_dims(geo)
    rows = geo.P * geo.B
    want = [("text", text, bf16, (rows, cfg.T, cfg.D_text)), ("temb_silu", temb_silu, bf16, (n, rows, cfg.D_temb)), ("head_shift", head_shift, bf16, (n, D)),
            ("head_onep", head_onep, bf16, (n, D)), ("coef", coef, torch.float32, (n, 8))]
    for name, t, dt, shape in want:
        if t is None or not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"cog_sample_ms: {name} must be a contiguous {dt} {shape} GPU tensor, got {None if t is None else tuple(t.shape)}")
    k = 0
    if noise is not None:
        if not noise.is_cuda or noise.dtype != torch.float32 or noise.dim() != 4 or tuple(noise.shape[1:]) != (geo.B, S, Kc) or not noise.is_contiguous() \
                or not 1 <= noise.shape[0] <= n:
            raise ValueError(f"cog_sample_ms: noise must be a contiguous fp32 [1 .. {n}, {geo.B}, {S}, {Kc}] GPU tensor, got {tuple(noise.shape)}")
        k = noise.shape[0]
    need = cog_sample_ms_workspace_bytes(cfg, solver)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    ms = cog_sample_ms_config(cfg, solver)
    check(_lib.load().ftmi_cog_sample_ms(ctypes.byref(ms), ctypes.byref(weights), ptr(cols), ptr(x), ptr(text), ptr(temb_silu), ptr(head_shift), ptr(head_onep),
                                         ptr(coef), ptr(noise), k, ptr(workspace), workspace.numel(), stream_ptr()), "ftmi_cog_sample_ms")


# ---- HunyuanVideo latent sampling (include/ftmi355.h: ftmi_hy_sample_*; csrc/sample_layout.hip, csrc/hy_sample_dit.hip) --------------------------------------
def hy_sample_geometry(B: int, C: int, frames: int, height: int, width: int, patch: int = 2, patch_t: int = 1, true_cfg: bool = False) -> "_lib.HySampleGeometry":
    """The layout of a sampling run: latents [B, C, frames, height, width], x [B, S, Kc], cols [P B S, Kc], pred [P B, S, Kc]; P = 2 with true CFG."""
    return _lib.HySampleGeometry(B=B, C=C, F=frames, H=height, W=width, p=patch, pt=patch_t, P=2 if true_cfg else 1)


def hy_sample_init(geo, latents, x=None, cols=None):
    """noise fp32 [B, C, F, H, W] -> (x fp32 [B, S, Kc], cols bf16 [P B S, Kc]): ftmi_hy_sample_init."""
    require_gpu_tensor(latents, "latents", torch.float32)
    if tuple(latents.shape) != (geo.B, geo.C, geo.F, geo.H, geo.W) or not latents.is_contiguous():
        raise ValueError(f"hy_sample_init: latents must be contiguous [{geo.B}, {geo.C}, {geo.F}, {geo.H}, {geo.W}], got {tuple(latents.shape)}")
    S, Kc = _cog_sample_dims(geo)
    x = torch.empty((geo.B, S, Kc), dtype=torch.float32, device=latents.device) if x is None else x
    cols = torch.empty((geo.P * geo.B * S, Kc), dtype=bf16, device=latents.device) if cols is None else cols
    _cog_sample_buffers(geo, x, cols, "hy_sample_init")
    check(_lib.load().ftmi_hy_sample_init(ctypes.byref(geo), ptr(latents), ptr(x), ptr(cols), stream_ptr()), "ftmi_hy_sample_init")
    return x, cols


def hy_sample_step(geo, pred, x, sigmas, step: int, true_cfg: float, cols=None) -> None:
    """One sampler step in place (ftmi_hy_sample_step): pred bf16 [P B, S, Kc] (None: only the bf16 copies), x fp32 [B, S, Kc], sigmas fp32 [n + 1] on the
    device (x <- x + (sigmas[step + 1] - sigmas[step]) v), cols bf16 [P B S, Kc] (None: only the update)."""
    _cog_sample_buffers(geo, x, cols, "hy_sample_step")
    S, Kc = _cog_sample_dims(geo)
    if pred is not None:
        require_gpu_tensor(pred, "pred", bf16)
        if pred.numel() != geo.P * geo.B * S * Kc or not pred.is_contiguous():
            raise ValueError(f"hy_sample_step: pred must be contiguous [{geo.P * geo.B}, {S}, {Kc}], got {tuple(pred.shape)}")
        require_gpu_tensor(sigmas, "sigmas", torch.float32)
        if sigmas.dim() != 1 or not sigmas.is_contiguous() or not 0 <= int(step) < sigmas.shape[0] - 1:
            raise ValueError("hy_sample_step: sigmas is a contiguous fp32 [n + 1] table and step one of its first n entries")
    check(_lib.load().ftmi_hy_sample_step(ctypes.byref(geo), ptr(pred), ptr(x), ptr(sigmas), int(step), float(true_cfg), ptr(cols), stream_ptr()),
          "ftmi_hy_sample_step")


def hy_sample_finish(geo, x, k: float):
    """x fp32 [B, S, Kc] -> latents bf16 [B, C, F, H, W] = bf16(x * k) (ftmi_hy_sample_finish)."""
    _cog_sample_buffers(geo, x, None, "hy_sample_finish")
    out = torch.empty((geo.B, geo.C, geo.F, geo.H, geo.W), dtype=bf16, device=x.device)
    check(_lib.load().ftmi_hy_sample_finish(ctypes.byref(geo), ptr(x), float(k), ptr(out), stream_ptr()), "ftmi_hy_sample_finish")
    return out


def hy_sample_workspace_bytes(cfg) -> int:
    """``cfg``: a ``_lib.HySampleTextConfig`` (``text_adapters`` 1: text-stream adapters in the dual blocks)."""
    n = int(_lib.load().ftmi_hy_sample_text_workspace_bytes(ctypes.byref(cfg)))
    if n == 0:
        raise ValueError(f"hy_sample: {_lib.last_error()}")
    return n


def hy_sample(cfg, weights, cols, x, temb_silu, enc, head_shift, head_onep, key_bias, rope_cos, rope_sin, sigmas, workspace=None) -> None:
    """The whole denoising loop in ONE call (ftmi_hy_sample_text), in place on ``x`` / ``cols`` (as ``hy_sample_init`` wrote them).  temb_silu bf16 [steps, P B, D];
    enc bf16 [steps, P B, T, D] (the refined text of every step, unconditional rows first); head_shift / head_onep bf16 [steps, P B, D]; key_bias fp32
    [P B, T + S] or None; rope_cos / rope_sin fp32 [S, 128]; sigmas fp32 [steps + 1] on the device.  ``workspace``: a uint8 GPU tensor of at least
    ``hy_sample_workspace_bytes(cfg)`` (allocated when None).  ``cfg``: as for ``hy_sample_workspace_bytes``."""
    text_cfg, cfg = cfg, cfg.base
    geo, n, D = cfg.geo, cfg.steps, cfg.D
    _cog_sample_buffers(geo, x, cols, "hy_sample")
    S, _ = _cog_sample_dims(geo)
    rows = geo.P * geo.B
    want = [("temb_silu", temb_silu, bf16, (n, rows, D)), ("enc", enc, bf16, (n, rows, cfg.T, D)), ("head_shift", head_shift, bf16, (n, rows, D)),
            ("head_onep", head_onep, bf16, (n, rows, D)), ("rope_cos", rope_cos, torch.float32, (S, 128)), ("rope_sin", rope_sin, torch.float32, (S, 128)),
            ("sigmas", sigmas, torch.float32, (n + 1,))]
    if key_bias is not None:
        want.append(("key_bias", key_bias, torch.float32, (rows, cfg.T + S)))
    for name, t, dt, shape in want:
        if t is None or not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"hy_sample: {name} must be a contiguous {dt} {shape} GPU tensor, got {None if t is None else tuple(t.shape)}")
    need = hy_sample_workspace_bytes(text_cfg)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    check(_lib.load().ftmi_hy_sample_text(ctypes.byref(text_cfg), ctypes.byref(weights), ptr(cols), ptr(x), ptr(temb_silu), ptr(enc), ptr(head_shift), ptr(head_onep),
                                          ptr(key_bias), ptr(rope_cos), ptr(rope_sin), ptr(sigmas), ptr(workspace), workspace.numel(), stream_ptr()),
          "ftmi_hy_sample_text")
