"""Wan-T2V DiT block for FULL fine-tuning on the MI355X (BASELINE config 4): every parameter of the block trains.

Reference: [upstream] diffusers ``WanTransformerBlock`` / ``WanAttnProcessor2_0`` as driven by finetrainers/models/wan/base_specification.py:433-493,
restated in oracle/wan.py (whose rounding points the kernels follow).  One ``torch.autograd.Function`` per block; inside it everything is a call through
the C ABI (include/ftmi355.h): the MFMA GEMM (``ftmi_gemm_nt``; q|k|v of the self-attention and k|v of the cross-attention are one GEMM each), the
head_dim-128 flash attention, the Wan row-wise kernels (``ftmi_wan_*``: FP32LayerNorm + modulation, RMSNorm across heads + rotary embedding, gated
residual, each backward also producing the column sums of its parameter gradients) and the token-reduction GEMM for the weight gradients
(``ftmi_gemm_tn``: dW += dY^T X, accumulated in fp32 straight into the block's flat gradient buffer).

Parameters: ONE flat bf16 buffer per block (``flat``; the unit FSDP-2 shards, all-gathers and reduce-scatters -- parallel/ptd.py:466-499 wraps each block
with ``fully_shard``), gradients one flat fp32 buffer of the same layout (``grad_flat``; the reference reduces gradients in fp32, trainer.py:176-180).
``WanBlockLayout`` names the slices with the diffusers parameter names."""

from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

import ctypes
import os

from .. import _lib, ops
from .._lib import WanBlockConfig, WanLoraFfnBlockConfig, WanLoraFfnBlockWeights, check, ptr, stream_ptr

bf16 = torch.bfloat16
_NATIVE_SCRATCH: Dict[int, torch.Tensor] = {}  # device index -> byte buffer shared by every natively run block on that device (one stream at a time)


def _native_scratch(device: torch.device, nbytes: int) -> torch.Tensor:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    buf = _NATIVE_SCRATCH.get(idx)
    if buf is None or buf.numel() < nbytes:
        _NATIVE_SCRATCH.pop(idx, None)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _NATIVE_SCRATCH[idx] = buf
    return buf


class WanBlockLayout:
    """Order of the parameters inside a block's flat buffer.  Projections that read the same input are adjacent, so that q|k|v (self-attention) and
    k|v (cross-attention) are each ONE [3D, D] / [2D, D] matrix for the GEMM without any copy."""

    def __init__(self, dim: int, ffn_dim: int):
        if dim % 128 != 0 or ffn_dim % 64 != 0:
            raise ValueError("Wan block: dim must be a multiple of 128 (heads of 128), ffn_dim of 64")
        D, F = dim, ffn_dim
        self.dim, self.ffn_dim = D, F
        entries: List[Tuple[str, Tuple[int, ...]]] = [
            ("attn1.to_q.weight", (D, D)), ("attn1.to_k.weight", (D, D)), ("attn1.to_v.weight", (D, D)),
            ("attn1.to_q.bias", (D,)), ("attn1.to_k.bias", (D,)), ("attn1.to_v.bias", (D,)),
            ("attn1.to_out.0.weight", (D, D)), ("attn1.to_out.0.bias", (D,)),
            ("attn1.norm_q.weight", (D,)), ("attn1.norm_k.weight", (D,)),
            ("attn2.to_q.weight", (D, D)), ("attn2.to_q.bias", (D,)),
            ("attn2.to_k.weight", (D, D)), ("attn2.to_v.weight", (D, D)), ("attn2.to_k.bias", (D,)), ("attn2.to_v.bias", (D,)),
            ("attn2.to_out.0.weight", (D, D)), ("attn2.to_out.0.bias", (D,)),
            ("attn2.norm_q.weight", (D,)), ("attn2.norm_k.weight", (D,)),
            ("norm2.weight", (D,)), ("norm2.bias", (D,)),
            ("ffn.net.0.proj.weight", (F, D)), ("ffn.net.0.proj.bias", (F,)),
            ("ffn.net.2.weight", (D, F)), ("ffn.net.2.bias", (D,)),
            ("scale_shift_table", (1, 6, D)),
        ]
        self.entries = entries
        self.offsets: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        off = 0
        for name, shape in entries:
            n = 1
            for s in shape:
                n *= s
            self.offsets[name] = (off, shape)
            off += n  # every size is a multiple of 64 elements: all slices stay 16-byte aligned
        self.total = off
        # fused views: (first member, rows, cols)
        self.fused = {
            "w_qkv1": ("attn1.to_q.weight", 3 * D, D), "b_qkv1": ("attn1.to_q.bias", 3 * D, None),
            "w_kv2": ("attn2.to_k.weight", 2 * D, D), "b_kv2": ("attn2.to_k.bias", 2 * D, None),
        }

    def view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        if name in self.fused:
            first, rows, cols = self.fused[name]
            off = self.offsets[first][0]
            return flat[off:off + rows * (cols or 1)].view((rows, cols) if cols else (rows,))
        off, shape = self.offsets[name]
        n = 1
        for s in shape:
            n *= s
        return flat[off:off + n].view(shape)

    def named_views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        return {name: self.view(flat, name) for name, _ in self.entries}


class WanImageLayout:
    """Image-to-video (``added_kv_proj_dim``): attn2's second, frozen key / value set in a flat buffer of its OWN -- ``WanBlockLayout`` and the block's
    flat buffer stay what they are.  add_k_proj | add_v_proj are ONE [2D, D] matrix for the GEMM over the image rows."""

    def __init__(self, dim: int):
        D = dim
        self.entries: List[Tuple[str, Tuple[int, ...]]] = [
            ("attn2.add_k_proj.weight", (D, D)), ("attn2.add_v_proj.weight", (D, D)), ("attn2.add_k_proj.bias", (D,)), ("attn2.add_v_proj.bias", (D,)),
            ("attn2.norm_added_k.weight", (D,)),
        ]
        self.offsets = {"attn2.add_k_proj.weight": (0, (D, D)), "attn2.add_v_proj.weight": (D * D, (D, D)), "attn2.add_k_proj.bias": (2 * D * D, (D,)),
                        "attn2.add_v_proj.bias": (2 * D * D + D, (D,)), "attn2.norm_added_k.weight": (2 * D * D + 2 * D, (D,)),
                        "w_kvi": (0, (2 * D, D)), "b_kvi": (2 * D * D, (2 * D,))}
        self.total = 2 * D * D + 3 * D

    def view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        off, shape = self.offsets[name]
        n = 1
        for d in shape:
            n *= d
        return flat[off:off + n].view(shape)

    def named_views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        return {name: self.view(flat, name) for name, _ in self.entries}


# ---- the block as a composition of the library's launches from Python ----------------------------------------------------------------------------
# ONE forward and ONE backward walk for full fine-tuning and for LoRA over a frozen base, launch for launch what csrc/wan_dit.hip block_forward /
# block_backward issue: the second implementation the tests compare the C calls with (``native = False`` / ``FTMI_NATIVE_BLOCKS=0``).
# Adapter order inside lora_A [8, r, D] / lora_B [8, D, r] (the projections the recipe's regex "blocks.*(to_q|to_k|to_v|to_out.0)" selects: BOTH attentions)
LORA_TARGETS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0")
# the two feed-forward projections a target_modules spelled "...|ffn.net.0.proj|ffn.net.2" adds: rectangular, so their adapters are four Parameters of their own
# (``MI355XWanBlock.lora_ffn``: A_1 [r, D], B_1 [F, r], A_2 [r, F], B_2 [D, r], in this order)
LORA_FFN_TARGETS = ("ffn.net.0.proj", "ffn.net.2")
_TWINS = (("w_qkv1_t", "w_qkv1"), ("w_o1_t", "attn1.to_out.0.weight"), ("w_q2_t", "attn2.to_q.weight"), ("w_kv2_t", "w_kv2"), ("w_o2_t", "attn2.to_out.0.weight"),
          ("w_f1_t", "ffn.net.0.proj.weight"), ("w_f2_t", "ffn.net.2.weight"))


class _Lora(NamedTuple):
    """One call's adapters (None: no adapters, r = 0) and, for the backward, where their gradients are added."""
    a: Optional[torch.Tensor] = None  # fp32 [8, r, D]
    b: Optional[torch.Tensor] = None  # fp32 [8, D, r]
    ga: Optional[torch.Tensor] = None
    gb: Optional[torch.Tensor] = None
    f: Optional[Tuple[torch.Tensor, ...]] = None   # the feed-forward adapters (A_1 [r, D], B_1 [F, r], A_2 [r, F], B_2 [D, r]), or None
    gf: Optional[Tuple[torch.Tensor, ...]] = None  # their gradients, same order

    @property
    def r(self) -> int:
        return 0 if self.a is None else int(self.a.shape[1])


class _Acts(NamedTuple):
    """What the forward walk leaves for the backward.  a1, n3, act and f are read only by gradients of base parameters (gate_msa, W_1, W_2, gate_ff): a
    frozen base drops them; xa_*: the adapters' down-projected rows (None at r = 0)."""
    n1: Any; qkv: Any; qn: Any; kn: Any; o1: Any; lse1: Any; a1: Any; x1: Any; n2: Any; q2: Any; kv2: Any; q2n: Any; k2n: Any; o2: Any; lse2: Any; x2: Any
    n3: Any; act: Any; pre: Any; f: Any; xa_qkv: Any; xa_o1: Any; xa_q2: Any; xa_kv2: Any; xa_o2: Any
    # image-to-video: the image tokens' k|v rows, their normed keys, the image attention's lse and the SUMMED attention output (o2 stays the text branch's own)
    kvi: Any = None; kin: Any = None; lse_i: Any = None; o2s: Any = None
    xa_f1: Any = None; xa_f2: Any = None  # the feed-forward adapters' down-projected rows; with them n3 and act stay (dA_1 and dA_2 read them)

    def for_frozen_base(self) -> "_Acts":
        return self._replace(a1=None, f=None) if self.xa_f1 is not None else self._replace(a1=None, n3=None, act=None, f=None)


def _lora_linear_fwd(x, w, bias, nadp: int, a_sp, b_ext, r: int, s: float, gelu: bool = False):
    """[rows, N] = x W^T + b + s (x A^T) B^T for ``nadp`` adapters on one input (N = nadp N_out; a_sp [2 nadp r, K], b_ext [N, 3r]): the two launches of
    csrc/wan_dit.hip proj_fwd.  Returns (y, xa [rows, 3 nadp r], pre); ``gelu``: y = gelu_tanh(the sum), pre = the sum (else None)."""
    if r == 0:
        y, pre = ops.gemm_nt(x, w, bias, epilogue=1, want_out2=True) if gelu else (ops.gemm_nt(x, w, bias), None)
        return y, None, pre
    rows, K = x.shape
    N = w.shape[0]
    xa = torch.empty((rows, 3 * nadp * r), dtype=bf16, device=x.device)
    ops.gemm_nt_ex(x, a_sp, xa, M=rows, N=2 * nadp * r, K=K, alpha=s, split_r=r, variant=8)
    y = torch.empty((rows, N), dtype=bf16, device=x.device)
    pre = torch.empty_like(y) if gelu else None
    grp = dict(x2_grp_n=N // nadp, x2_grp_stride=3 * r) if nadp > 1 else {}
    ops.gemm_nt_ex(x, w, y, M=rows, N=N, K=K, bias=bias, x2=xa, w2=b_ext, K2=3 * r, variant=8, epilogue=1 if gelu else 0, out2=pre, **grp)
    return y, xa, pre


def _linear_grads(dy, inp, gw, gbias):
    """dW += dY^T X (fp32, token-reduction GEMM), db += column sums of dY; nothing when the base is frozen (gw None)."""
    if gw is not None:
        ops.gemm_tn(dy, inp, out=gw)
        ops.wan_colsum(dy, gbias)


def _lora_linear_bwd(x, dy, w_t, nadp: int, xa, bt_sp, at_ext, r: int, s: float, ga, gb, need_dx: bool = True, gw=None, gbias=None, pre=None):
    """csrc/wan_dit.hip proj_bwd, in its order, for x [rows, K], dy [rows, N = nadp N_out]: gw += dY^T x and gbias += column sums (a training base);
    dXA = s dY B (bt_sp [2 nadp r, N_out]); dx = dY W (+ dXA A: at_ext [K, 3 nadp r]), times gelu_tanh'(pre) when ``pre`` is given; gb [N, r] += dY^T XA,
    ga [nadp r, K] += dXA^T x."""
    _linear_grads(dy, x, gw, gbias)
    epi = dict(epilogue=3, aux=pre) if pre is not None else {}
    if r == 0:  # (x may be None here: a frozen base without adapters on this projection does not keep it)
        return ops.gemm_nt(dy, w_t, None, **epi) if need_dx else None
    rows, K = x.shape
    N = dy.shape[1]
    No = N // nadp
    dxa = torch.empty((rows, 3 * nadp * r), dtype=bf16, device=x.device)
    grp = dict(xk_grp_n=2 * r, xk_grp_stride=No) if nadp > 1 else {}
    ops.gemm_nt_ex(dy, bt_sp, dxa, M=rows, N=2 * nadp * r, K=No, alpha=s, split_r=r, variant=8, **grp)
    dx = None
    if need_dx:
        dx = torch.empty((rows, K), dtype=bf16, device=x.device)
        ops.gemm_nt_ex(dy, w_t, dx, M=rows, N=K, K=N, x2=dxa, w2=at_ext, K2=3 * nadp * r, variant=8, **epi)
    ops.gemm_tn_ex(dy, xa, gb, M=rows, P=N, Q=r, v_fold=r, **(dict(v_grp_p=No, v_grp_stride=3 * r) if nadp > 1 else {}))
    ops.gemm_tn_ex(dxa, x, ga, M=rows, P=nadp * r, Q=K, u_fold=r, **(dict(u_grp_p=r, u_grp_stride=3 * r) if nadp > 1 else {}))
    return dx


def _block_forward(blk: "MI355XWanBlock", x, enc, mod, rope, lora: _Lora, need_out: bool = True, enc_img=None):
    """mod: fp32 [B, 6, D] = (shift, scale, gate) of the attention, then of the feed-forward.  Returns (out [B, S, D], _Acts); ``need_out=False`` (the
    recomputation pass of gradient checkpointing) stops after the feed-forward's first GEMM: its pre-activation is the last thing the backward reads."""
    B, S, D = x.shape
    T = enc.shape[1]
    M, H, hd, eps, s, r = B * S, blk.heads, blk.head_dim, blk.eps, blk.lora_scale, lora.r
    P = blk.param
    a_sp = b_ext = None
    if r:
        a_sp = torch.stack([ops.lora_split(lora.a[i], sp=True)[0] for i in range(8)])
        b_ext = torch.stack([ops.lora_split(lora.b[i], ext=True)[0] for i in range(8)])

    def lin(t, w, b, adp, nadp):  # the attention adapters adp .. adp + nadp - 1 (all [r, D] / [D, r])
        if not r:
            return _lora_linear_fwd(t, w, b, nadp, None, None, 0, s)[:2]
        return _lora_linear_fwd(t, w, b, nadp, a_sp[adp:adp + nadp].reshape(2 * nadp * r, D), b_ext[adp:adp + nadp].reshape(nadp * D, 3 * r), r, s)[:2]

    f_sp = f_ext = (None, None)  # the feed-forward adapters' operand copies: (A_1, A_2) as row planes, (B_1, B_2) as K-extension columns
    rf = r if lora.f is not None else 0
    if rf:
        f_sp = tuple(ops.lora_split(lora.f[i], sp=True)[0] for i in (0, 2))
        f_ext = tuple(ops.lora_split(lora.f[i], ext=True)[0] for i in (1, 3))
    x2d, enc2d = x.view(M, D), enc.view(B * T, D)
    heads = lambda t, n: t.view(B, n, H, hd).permute(0, 2, 1, 3)  # [rows, D] view (any row stride) -> [B, H, n, hd]
    tok = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0] * t.shape[2], D)  # attention output [B, H, n, hd] laid out [B, n, H, hd] -> [rows, D]
    # self-attention
    n1 = ops.wan_ln(x2d, S, shift=mod[:, 0], scale=mod[:, 1], eps=eps)
    qkv, xa_qkv = lin(n1, P("w_qkv1"), P("b_qkv1"), 0, 3)
    qn = ops.wan_rms_rope(qkv[:, :D], P("attn1.norm_q.weight"), S, rope=rope, head_dim=hd, eps=eps)
    kn = ops.wan_rms_rope(qkv[:, D:2 * D], P("attn1.norm_k.weight"), S, rope=rope, head_dim=hd, eps=eps)
    o1, lse1 = ops.attn_fwd(heads(qn, S), heads(kn, S), heads(qkv[:, 2 * D:], S))
    a1, xa_o1 = lin(tok(o1), P("attn1.to_out.0.weight"), P("attn1.to_out.0.bias"), 3, 1)
    x1 = ops.wan_gate_res(x2d, a1, S, gate=mod[:, 2])
    # cross-attention to the text tokens (no rotary embedding, no gate)
    n2 = ops.wan_ln(x1, S, w=P("norm2.weight"), b=P("norm2.bias"), eps=eps)
    q2, xa_q2 = lin(n2, P("attn2.to_q.weight"), P("attn2.to_q.bias"), 4, 1)
    kv2, xa_kv2 = lin(enc2d, P("w_kv2"), P("b_kv2"), 5, 2)
    q2n = ops.wan_rms_rope(q2, P("attn2.norm_q.weight"), S, eps=eps)
    k2n = ops.wan_rms_rope(kv2[:, :D], P("attn2.norm_k.weight"), T, eps=eps)
    o2, lse2 = ops.attn_fwd(heads(q2n, S), heads(k2n, T), heads(kv2[:, D:], T))
    kvi = kin = lse_i = o2s = None
    if enc_img is not None and enc_img.shape[1] > 0:  # the image tokens' frozen keys and values; their attention is summed onto the text branch's output
        TI, IP = enc_img.shape[1], blk.img_param
        blk.first_image_tokens(enc_img, B)  # (refuses rows that cannot hold the declared second image, like the C call's configuration)
        kvi = ops.gemm_nt(enc_img.view(B * TI, D), IP("w_kvi"), IP("b_kvi"))
        kin = ops.wan_rms_rope(kvi[:, :D], IP("attn2.norm_added_k.weight"), TI, eps=eps)
        # (TI counts both images of a first/last-frame block, whose second context goes through the wide kernels)
        ctx2_fwd = ops.attn_ctx2w_fwd if blk.second_image_tokens > 0 else ops.attn_ctx2_fwd
        o2s, lse_i = ctx2_fwd(heads(q2n, S), heads(kin, TI), heads(kvi[:, D:], TI), o2)
    a2, xa_o2 = lin(tok(o2 if o2s is None else o2s), P("attn2.to_out.0.weight"), P("attn2.to_out.0.bias"), 7, 1)
    x2 = ops.wan_gate_res(x1, a2, S)
    # feed-forward
    n3 = ops.wan_ln(x2, S, shift=mod[:, 3], scale=mod[:, 4], eps=eps)
    act, xa_f1, pre = _lora_linear_fwd(n3, P("ffn.net.0.proj.weight"), P("ffn.net.0.proj.bias"), 1, f_sp[0], f_ext[0], rf, s, gelu=True)  # GELU-tanh, pre-activation kept
    f = out = xa_f2 = None
    if need_out:
        f, xa_f2, _ = _lora_linear_fwd(act, P("ffn.net.2.weight"), P("ffn.net.2.bias"), 1, f_sp[1], f_ext[1], rf, s)
        out = ops.wan_gate_res(x2, f, S, gate=mod[:, 5]).view(B, S, D)
    elif rf:  # the recomputation pass: net.2's down-projected rows are read by dB_2, its GEMM is not needed
        xa_f2 = torch.empty((M, 3 * rf), dtype=bf16, device=x.device)
        ops.gemm_nt_ex(act, f_sp[1], xa_f2, M=M, N=2 * rf, K=blk.ffn_dim, alpha=s, split_r=rf, variant=8)
    return out, _Acts(n1, qkv, qn, kn, o1, lse1, a1, x1, n2, q2, kv2, q2n, k2n, o2, lse2, x2, n3, act, pre, f, xa_qkv, xa_o1, xa_q2, xa_kv2, xa_o2, kvi, kin, lse_i, o2s,
                      xa_f1, xa_f2)


def _block_backward(blk: "MI355XWanBlock", acts: _Acts, x, enc, mod, rope, dout, lora: _Lora, train_base: bool, need_denc: bool = True):
    """Returns (dx [B, S, D], denc [B, T, D] or None, dmod fp32 [6, B, D] or None).  ``train_base``: all base gradients are added into ``blk.grad`` and the
    (shift, scale, gate) sums over the tokens into dmod; a frozen base forms none of them (no weight-gradient GEMM, no bias / norm / modulation
    reduction, and a1, n3, act and f are not read).  The adapter gradients are added into ``lora.ga / lora.gb``."""
    c = acts
    B, S, D = x.shape
    T = enc.shape[1]
    M, H, hd, eps, s, r = B * S, blk.heads, blk.head_dim, blk.eps, blk.lora_scale, lora.r
    P, Wt = blk.param, blk.transposed()
    G = blk.grad if train_base else (lambda name: None)
    dmod = torch.zeros((6, B, D), dtype=torch.float32, device=x.device) if train_base else None
    DM = (lambda i: dmod[i]) if train_base else (lambda i: None)
    bt_sp = at_ext = None
    if r:
        bt_sp = torch.stack([ops.lora_split(lora.b[i], t_sp=True)[0] for i in range(8)])
        at_ext = torch.cat([ops.lora_split(lora.a[i], t_ext=True)[0] for i in range(8)], dim=1)  # the eight adapters side by side: [D, 24r]

    def lin(t, dy, w_t, adp, nadp, xa, need_dx=True, gw=None, gbias=None):
        if not r:
            return _lora_linear_bwd(t, dy, w_t, nadp, None, None, None, 0, s, None, None, need_dx, gw, gbias)
        return _lora_linear_bwd(t, dy, w_t, nadp, xa, bt_sp[adp:adp + nadp].reshape(2 * nadp * r, D), at_ext[:, adp * 3 * r:(adp + nadp) * 3 * r], r, s,
                                lora.ga[adp:adp + nadp].view(nadp * r, D), lora.gb[adp:adp + nadp].view(nadp * D, r), need_dx, gw, gbias)

    rf = r if lora.f is not None else 0
    f_tsp = f_text = gf = (None,) * 4  # the feed-forward adapters: B^T as row planes, A^T as K-extension columns, per adapter
    if rf:
        f_tsp = tuple(ops.lora_split(lora.f[i], t_sp=True)[0] if i in (1, 3) else None for i in range(4))
        f_text = tuple(ops.lora_split(lora.f[i], t_ext=True)[0] if i in (0, 2) else None for i in range(4))
        gf = lora.gf

    x2d, enc2d = x.view(M, D), enc.view(B * T, D)
    dout = dout.contiguous().view(M, D)
    heads = lambda t, n: t.view(B, n, H, hd).permute(0, 2, 1, 3)
    tok = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0] * t.shape[2], D)
    # feed-forward branch: out = x2 + f * gate_ff
    df = ops.wan_gate_res_bwd(dout, c.f if train_base else None, mod[:, 5], S, dgate=DM(5))
    # (d f W2 [+ dXA_2 A_2]) * gelu'(pre); act and n3 are read by the base's weight gradients and by the feed-forward adapters' dA only
    dpre = _lora_linear_bwd(c.act, df, Wt["ffn.net.2.weight"], 1, c.xa_f2, f_tsp[3], f_text[2], rf, s, gf[2], gf[3], gw=G("ffn.net.2.weight"),
                            gbias=G("ffn.net.2.bias"), pre=c.pre)
    dn3 = _lora_linear_bwd(c.n3, dpre, Wt["ffn.net.0.proj.weight"], 1, c.xa_f1, f_tsp[1], f_text[0], rf, s, gf[0], gf[1], gw=G("ffn.net.0.proj.weight"),
                           gbias=G("ffn.net.0.proj.bias"))
    dx2 = ops.wan_ln_bwd(c.x2, dn3, S, scale=mod[:, 4], eps=eps, dres=dout, red1=DM(3), red2=DM(4), red_per_batch=train_base)
    # cross-attention branch: x2 = x1 + a2
    do2 = lin(tok(c.o2 if c.o2s is None else c.o2s), dx2, Wt["attn2.to_out.0.weight"], 7, 1, c.xa_o2, gw=G("attn2.to_out.0.weight"), gbias=G("attn2.to_out.0.bias"))
    dkv2 = torch.empty_like(c.kv2)
    dq2n, dk2n, _ = ops.attn_bwd(heads(c.q2n, S), heads(c.k2n, T), heads(c.kv2[:, D:], T), c.o2, c.lse2, heads(do2, S), dv_out=heads(dkv2[:, D:], T))
    if c.o2s is not None:  # the image branch's dQ, added onto the text branch's in place (frozen keys and values: no dK, dV)
        TI = c.kin.shape[0] // B
        ctx2_dq = ops.attn_ctx2w_dq if blk.second_image_tokens > 0 else ops.attn_ctx2_dq
        ctx2_dq(heads(c.q2n, S), heads(c.kin, TI), heads(c.kvi[:, D:], TI), c.lse_i, heads(do2, S), dq2n, inplace=True)
    dq2 = ops.wan_rms_rope_bwd(c.q2, P("attn2.norm_q.weight"), tok(dq2n), S, eps=eps, dweight=G("attn2.norm_q.weight"))
    ops.wan_rms_rope_bwd(c.kv2[:, :D], P("attn2.norm_k.weight"), tok(dk2n), T, eps=eps, dweight=G("attn2.norm_k.weight"), out=dkv2[:, :D])
    _linear_grads(dq2, c.n2, G("attn2.to_q.weight"), G("attn2.to_q.bias"))  # (attn2.to_q's weight gradient goes ahead of the text rows' projection)
    denc = lin(enc2d, dkv2, Wt["w_kv2"], 5, 2, c.xa_kv2, need_denc, gw=G("w_kv2"), gbias=G("b_kv2"))
    dn2 = lin(c.n2, dq2, Wt["attn2.to_q.weight"], 4, 1, c.xa_q2)
    dx1 = ops.wan_ln_bwd(c.x1, dn2, S, w=P("norm2.weight"), eps=eps, dres=dx2, red1=G("norm2.bias"), red2=G("norm2.weight"))
    # self-attention branch: x1 = x + a1 * gate_msa
    da1 = ops.wan_gate_res_bwd(dx1, c.a1 if train_base else None, mod[:, 2], S, dgate=DM(2))
    do1 = lin(tok(c.o1), da1, Wt["attn1.to_out.0.weight"], 3, 1, c.xa_o1, gw=G("attn1.to_out.0.weight"), gbias=G("attn1.to_out.0.bias"))
    dqkv = torch.empty_like(c.qkv)
    dqn, dkn, _ = ops.attn_bwd(heads(c.qn, S), heads(c.kn, S), heads(c.qkv[:, 2 * D:], S), c.o1, c.lse1, heads(do1, S), dv_out=heads(dqkv[:, 2 * D:], S))
    ops.wan_rms_rope_bwd(c.qkv[:, :D], P("attn1.norm_q.weight"), tok(dqn), S, rope=rope, head_dim=hd, eps=eps, dweight=G("attn1.norm_q.weight"), out=dqkv[:, :D])
    ops.wan_rms_rope_bwd(c.qkv[:, D:2 * D], P("attn1.norm_k.weight"), tok(dkn), S, rope=rope, head_dim=hd, eps=eps, dweight=G("attn1.norm_k.weight"),
                         out=dqkv[:, D:2 * D])
    dn1 = lin(c.n1, dqkv, Wt["w_qkv1"], 0, 3, c.xa_qkv, gw=G("w_qkv1"), gbias=G("b_qkv1"))  # the three projections' input gradients summed in the GEMM's fp32 accumulator
    dx = ops.wan_ln_bwd(x2d, dn1, S, scale=mod[:, 1], eps=eps, dres=dx1, red1=DM(0), red2=DM(1), red_per_batch=train_base)
    return dx.view(B, S, D), (denc.view(B, T, D) if denc is not None else None), dmod


class _WanBlockFunction(torch.autograd.Function):
    """Full fine-tuning through the Python walks: every parameter of the block trains."""

    @staticmethod
    def forward(ctx, blk: "MI355XWanBlock", x, enc, temb, rope_cos, rope_sin):
        # scale_shift_table (bf16 parameter [1, 6, D]) + temb.float(): fp32 [B, 6, D] = (shift, scale, gate) of the attention, then of the feed-forward
        mod = (blk.param("scale_shift_table").float() + temb.float()).contiguous()
        out, ctx.acts = _block_forward(blk, x, enc, mod, (rope_cos, rope_sin), _Lora())
        ctx.blk, ctx.rope, ctx.temb_dtype = blk, (rope_cos, rope_sin), temb.dtype
        ctx.save_for_backward(x, enc, mod)
        return out

    @staticmethod
    def backward(ctx, dout):
        blk = ctx.blk
        if blk._pre_backward is not None:
            blk._pre_backward(blk)  # sharded training: gather this block's parameters (prefetch the previous block's), take a gradient buffer
        x, enc, mod = ctx.saved_tensors
        acts, ctx.acts = ctx.acts, None
        dx, denc, dmod = _block_backward(blk, acts, x, enc, mod, ctx.rope, dout, _Lora(), train_base=True)
        dmod = dmod.permute(1, 0, 2)  # [B, 6, D]
        blk.grad("scale_shift_table").add_(dmod.sum(0, keepdim=True))
        if blk._grad_hook is not None:
            blk._grad_hook(blk)  # sharded training: this block's gradients are final -- start their reduce-scatter while the earlier blocks run
        return None, dx, denc, dmod.to(ctx.temb_dtype), None, None


class _WanBlockNativeFunction(torch.autograd.Function):
    """``_WanBlockFunction`` with ONE C call per direction (``ftmi_wan_block_forward / _backward``, csrc/wan_dit.hip: the same kernels in the same order,
    activations in one planned buffer per block, transients in a buffer shared by all blocks).  The sharding hooks run around the calls exactly as in the
    Python composition: parameters are read through ``blk._params()`` (the local or the all-gathered buffer), gradients go to ``blk.grad_flat``."""

    @staticmethod
    def _cfg(blk: "MI355XWanBlock", B: int, S: int, T: int) -> WanBlockConfig:
        return WanBlockConfig(B=B, S=S, T=T, D=blk.dim, H=blk.heads, F=blk.ffn_dim, eps=float(blk.eps), gemm_variant=8)

    @staticmethod
    def forward(ctx, blk: "MI355XWanBlock", x, enc, temb, rope_cos, rope_sin):
        B, S, D = x.shape
        T = enc.shape[1]
        mod = (blk.param("scale_shift_table").float() + temb.float()).contiguous()
        cfg = _WanBlockNativeFunction._cfg(blk, B, S, T)
        lib = _lib.load()
        params = blk._params()
        if params.numel() != lib.ftmi_wan_block_param_elements(ctypes.byref(cfg)) or not params.is_contiguous():
            raise RuntimeError("Wan block: the flat parameter buffer does not have the layout the C orchestrator expects")
        saved = torch.empty(lib.ftmi_wan_block_saved_bytes(ctypes.byref(cfg)), dtype=torch.uint8, device=x.device)
        out = torch.empty_like(x)
        check(lib.ftmi_wan_block_forward(ctypes.byref(cfg), ptr(params), ptr(x), ptr(enc), ptr(mod), ptr(rope_cos), ptr(rope_sin), ptr(out), ptr(saved), saved.numel(),
                                         stream_ptr()), "ftmi_wan_block_forward")
        ctx.blk, ctx.dims, ctx.rope, ctx.temb_dtype = blk, (B, S, T, D), (rope_cos, rope_sin), temb.dtype
        ctx.save_for_backward(x, enc, mod, saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        blk = ctx.blk
        if blk._pre_backward is not None:
            blk._pre_backward(blk)  # sharded training: gather this block's parameters (prefetch the previous block's), take a gradient buffer
        B, S, T, D = ctx.dims
        x, enc, mod, saved = ctx.saved_tensors
        dout = dout.contiguous()
        dmod = torch.zeros((6, B, D), dtype=torch.float32, device=x.device)
        if blk.grad_flat is None:
            blk.zero_grad_flat()
        cfg = _WanBlockNativeFunction._cfg(blk, B, S, T)
        lib = _lib.load()
        scratch = _native_scratch(x.device, lib.ftmi_wan_block_scratch_bytes(ctypes.byref(cfg)))
        dx, denc = torch.empty_like(x), torch.empty_like(enc)
        check(lib.ftmi_wan_block_backward(ctypes.byref(cfg), ptr(blk._params()), ptr(blk.grad_flat), ptr(x), ptr(enc), ptr(mod), ptr(ctx.rope[0]), ptr(ctx.rope[1]),
                                          ptr(dout), ptr(dx), ptr(denc), ptr(dmod), ptr(saved), saved.numel(), ptr(scratch), scratch.numel(), stream_ptr()),
              "ftmi_wan_block_backward")
        dmod = dmod.permute(1, 0, 2)  # [B, 6, D]
        blk.grad("scale_shift_table").add_(dmod.sum(0, keepdim=True))
        if blk._grad_hook is not None:
            blk._grad_hook(blk)  # sharded training: this block's gradients are final -- start their reduce-scatter while the earlier blocks run
        return None, dx, denc, dmod.to(ctx.temb_dtype), None, None


def _planned(nbytes: int) -> int:
    """A byte planner's answer; 0 means the library refused the configuration (the reason is in ftmi_last_error)."""
    if nbytes == 0:
        raise ValueError(f"Wan LoRA block: {_lib.last_error()}")
    return nbytes


def _grad_targets(blk: "MI355XWanBlock", lora_a, lora_b, ffn=None):
    """Where the adapter gradients go: the step object's flat views (added in place), or fresh tensors returned to autograd.  Returns (own, ga, gb, gf):
    gf = the four gradients of the feed-forward adapters ``ffn``, or None."""
    if lora_a is None:
        return False, None, None, None
    own = blk._grad_a_view is not None
    gf = None if ffn is None else (blk._grad_ffn_views if own else tuple(torch.zeros_like(t) for t in ffn))
    return own, (blk._grad_a_view if own else torch.zeros_like(lora_a)), (blk._grad_b_view if own else torch.zeros_like(lora_b)), gf


class _WanLoRABlockFunction(torch.autograd.Function):
    """The block over a FROZEN base through the Python walks, text-to-video and image-to-video.  ``lora_a`` [8, r, D] / ``lora_b`` [8, D, r]: the adapters on
    the eight attention projections; ``enc_img`` [B, TI, D]: the image context of an image-to-video block in attn2 (frozen: no gradient flows into it; a
    first/last-frame block, ``second_image_tokens`` = TI2 > 0, takes [B, TI + TI2, D], the second image's rows after the first one's);
    ``fa1`` [r, D], ``fb1`` [F, r], ``fa2`` [r, F], ``fb2`` [D, r]: the adapters on ffn.net.0.proj and ffn.net.2 -- each None where the block has none.  The
    backward forms dx, denc (only if asked for) and the adapter gradients -- no base-weight gradient, no bias / norm / modulation reduction, and it keeps
    neither a1 nor f (n3 and act only for the feed-forward adapters)."""

    @staticmethod
    def forward(ctx, blk: "MI355XWanBlock", x, enc, temb, rope_cos, rope_sin, lora_a, lora_b, enc_img, fa1, fb1, fa2, fb2):
        ffn = None if fa1 is None else (fa1, fb1, fa2, fb2)
        mod = (blk.param("scale_shift_table").float() + temb.float()).contiguous()
        out, acts = _block_forward(blk, x, enc, mod, (rope_cos, rope_sin), _Lora(lora_a, lora_b, f=ffn), enc_img=enc_img)
        ctx.blk, ctx.rope, ctx.recompute = blk, (rope_cos, rope_sin), bool(blk.gradient_checkpointing)
        ctx.save_for_backward(x, enc, mod, lora_a, lora_b, enc_img, fa1, fb1, fa2, fb2)
        ctx.acts = None if ctx.recompute else acts.for_frozen_base()
        return out

    @staticmethod
    def backward(ctx, dout):
        blk, rope = ctx.blk, ctx.rope
        x, enc, mod, lora_a, lora_b, enc_img = ctx.saved_tensors[:6]
        ffn = None if ctx.saved_tensors[6] is None else tuple(ctx.saved_tensors[6:10])
        acts, ctx.acts = ctx.acts, None
        if ctx.recompute:
            acts = _block_forward(blk, x, enc, mod, rope, _Lora(lora_a, lora_b, f=ffn), need_out=False, enc_img=enc_img)[1].for_frozen_base()
        own, ga, gb, gf = _grad_targets(blk, lora_a, lora_b, ffn)
        dx, denc, _ = _block_backward(blk, acts, x, enc, mod, rope, dout, _Lora(lora_a, lora_b, ga, gb, ffn, gf), train_base=False, need_denc=ctx.needs_input_grad[2])
        if own:  # the step object owns the gradients: nothing goes back through autograd
            blk._backward_done()
            ga = gb = gf = None
        return (None, dx, denc, None, None, None, ga, gb, None) + (gf or (None,) * 4)


class _WanLoRABlockNativeFunction(torch.autograd.Function):
    """``_WanLoRABlockFunction`` with ONE C call per direction (``ftmi_wan_lora_ffn_block_forward / _backward``, csrc/wan_dit.hip: the one entry for every
    LoRA configuration -- ``enc_img`` None: TI = 0, ``fa1`` None: ffn = 0).  The K-contiguous twins of the weights come from ``blk.transposed()``: cached, and
    the frozen base never invalidates them.  Gradient checkpointing keeps the block's input only and refills ``saved`` inside the backward (the forward call
    with ``out = NULL``)."""

    @staticmethod
    def _args(blk: "MI355XWanBlock", B: int, S: int, T: int, lora_a, lora_b, backward: bool, TI: int = 0, ffn=None):
        """(config, weights, the tensors whose pointers the weights hold: keep them alive over the call)."""
        cfg = WanLoraFfnBlockConfig(B=B, S=S, T=T, D=blk.dim, H=blk.heads, F=blk.ffn_dim, eps=float(blk.eps), gemm_variant=8,
                                    r=0 if lora_a is None else int(lora_a.shape[1]), lora_scale=float(blk.lora_scale), TI=TI, ffn=int(ffn is not None),
                                    TI2=blk.second_image_tokens if TI > 0 else 0)
        wf = WanLoraFfnBlockWeights()
        w = wf.base
        params = blk._params()
        if params.numel() != blk.layout.total or not params.is_contiguous():
            raise RuntimeError("Wan block: the flat parameter buffer does not have the layout the C orchestrator expects")
        keep = [params]
        w.params = ptr(params)
        if backward:
            Wt = blk.transposed()
            for field, name in _TWINS:
                keep.append(Wt[name])
                setattr(w, field, ptr(Wt[name]))
        if lora_a is not None:
            la, lb = lora_a.contiguous(), lora_b.contiguous()
            keep += [la, lb]
            w.lora_a, w.lora_b = ptr(la), ptr(lb)
        if ffn is not None:
            ffn = [t.contiguous() for t in ffn]
            keep += ffn
            wf.ffn_a1, wf.ffn_b1, wf.ffn_a2, wf.ffn_b2 = (ptr(t) for t in ffn)
        return cfg, wf, keep

    @staticmethod
    def _forward_call(blk, x, enc, mod, rope_cos, rope_sin, lora_a, lora_b, out, enc_img=None, ffn=None):
        B, S, _ = x.shape
        lib = _lib.load()
        TI = 0 if enc_img is None else blk.first_image_tokens(enc_img, B)
        cfg, w, keep = _WanLoRABlockNativeFunction._args(blk, B, S, enc.shape[1], lora_a, lora_b, backward=False, TI=TI, ffn=ffn)
        saved = torch.empty(_planned(lib.ftmi_wan_lora_ffn_block_saved_bytes(ctypes.byref(cfg))), dtype=torch.uint8, device=x.device)
        scratch = _native_scratch(x.device, _planned(lib.ftmi_wan_lora_ffn_block_scratch_bytes(ctypes.byref(cfg))))
        img = blk._img_params() if TI > 0 else None
        check(lib.ftmi_wan_lora_ffn_block_forward(ctypes.byref(cfg), ctypes.byref(w), ptr(img), ptr(x), ptr(enc), ptr(enc_img if TI > 0 else None), ptr(mod),
                                                  ptr(rope_cos), ptr(rope_sin), ptr(out), ptr(saved), saved.numel(), ptr(scratch), scratch.numel(), stream_ptr()),
              "ftmi_wan_lora_ffn_block_forward")
        return saved

    @staticmethod
    def forward(ctx, blk: "MI355XWanBlock", x, enc, temb, rope_cos, rope_sin, lora_a, lora_b, enc_img, fa1, fb1, fa2, fb2):
        ffn = None if fa1 is None else (fa1, fb1, fa2, fb2)
        mod = (blk.param("scale_shift_table").float() + temb.float()).contiguous()
        out = torch.empty_like(x)
        saved = _WanLoRABlockNativeFunction._forward_call(blk, x, enc, mod, rope_cos, rope_sin, lora_a, lora_b, out, enc_img, ffn)
        ctx.blk, ctx.rope, ctx.recompute = blk, (rope_cos, rope_sin), bool(blk.gradient_checkpointing)
        ctx.save_for_backward(x, enc, mod, lora_a, lora_b, enc_img, fa1, fb1, fa2, fb2, None if ctx.recompute else saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        blk, rope = ctx.blk, ctx.rope
        x, enc, mod, lora_a, lora_b, enc_img = ctx.saved_tensors[:6]
        ffn = None if ctx.saved_tensors[6] is None else tuple(ctx.saved_tensors[6:10])
        saved = ctx.saved_tensors[10]
        if ctx.recompute:
            saved = _WanLoRABlockNativeFunction._forward_call(blk, x, enc, mod, rope[0], rope[1], lora_a, lora_b, None, enc_img, ffn)
        B, S, _ = x.shape
        TI = 0 if enc_img is None else blk.first_image_tokens(enc_img, B)
        dout = dout.contiguous()
        own, ga, gb, gf = _grad_targets(blk, lora_a, lora_b, ffn)
        lib = _lib.load()
        dx = torch.empty_like(x)
        denc = torch.empty_like(enc) if ctx.needs_input_grad[2] else None  # frozen text embedder: no gradient into the text rows, its GEMM is skipped
        cfg, w, keep = _WanLoRABlockNativeFunction._args(blk, B, S, enc.shape[1], lora_a, lora_b, backward=True, TI=TI, ffn=ffn)
        scratch = _native_scratch(x.device, _planned(lib.ftmi_wan_lora_ffn_block_scratch_bytes(ctypes.byref(cfg))))
        img = blk._img_params() if TI > 0 else None
        g4 = gf or (None,) * 4
        check(lib.ftmi_wan_lora_ffn_block_backward(ctypes.byref(cfg), ctypes.byref(w), ptr(img), ptr(x), ptr(enc), ptr(enc_img if TI > 0 else None), ptr(mod),
                                                   ptr(rope[0]), ptr(rope[1]), ptr(dout), ptr(dx), ptr(denc), ptr(ga), ptr(gb), ptr(g4[0]), ptr(g4[1]),
                                                   ptr(g4[2]), ptr(g4[3]), ptr(saved), saved.numel(), ptr(scratch), scratch.numel(), stream_ptr()),
              "ftmi_wan_lora_ffn_block_backward")
        if own:  # the step object owns the gradients: nothing goes back through autograd
            blk._backward_done()
            ga = gb = gf = None
        return (None, dx, denc, None, None, None, ga, gb, None) + (gf or (None,) * 4)


class MI355XWanBlock(nn.Module):
    """Holds the block's flat bf16 parameters and flat fp32 gradients; ``forward(hidden_states, encoder_hidden_states, temb, rotary)`` like the
    reference block, ``temb`` = the [B, 6, D] time projection, ``rotary`` = (cos, sin) fp32 [S, head_dim / 2]."""

    # one C call per direction (csrc/wan_dit.hip); False (or FTMI_NATIVE_BLOCKS=0 in the environment): the per-kernel composition from Python -- the tests compare the two
    native = os.environ.get("FTMI_NATIVE_BLOCKS", "1") != "0"

    def __init__(self, dim: int = 1536, heads: int = 12, ffn_dim: int = 8960, eps: float = 1e-6, device: Optional[torch.device] = None,
                 added_kv_proj_dim: Optional[int] = None, second_image_tokens: int = 0):
        super().__init__()
        if second_image_tokens < 0 or second_image_tokens > 320 or (second_image_tokens and added_kv_proj_dim is None):
            raise ValueError("Wan first/last-frame: the second image holds 0 .. 320 tokens and needs the image context (added_kv_proj_dim)")
        self.second_image_tokens = int(second_image_tokens)  # TI2 of ftmi_wan_lora_ffn_block_config: the last rows of enc_img [B, TI + TI2, D]
        if added_kv_proj_dim is not None and added_kv_proj_dim != dim:
            raise ValueError("Wan image-to-video: added_kv_proj_dim is the block width (the image embedder projects to it)")
        if dim % heads != 0 or dim // heads != 128:
            raise ValueError("the Wan path uses the head_dim-128 attention kernels")
        self.dim, self.heads, self.head_dim, self.ffn_dim, self.eps = dim, heads, dim // heads, ffn_dim, eps
        self.layout = WanBlockLayout(dim, ffn_dim)
        dev = device or torch.device("cuda", 0)
        # gradients do not go through ``.grad`` (they are fp32, the parameters bf16): the block's backward writes ``grad_flat``
        self.flat = nn.Parameter(torch.zeros(self.layout.total, dtype=bf16, device=dev), requires_grad=False)
        # image-to-video: attn2.add_k_proj / add_v_proj / norm_added_k in a flat buffer of their own (frozen; LoRA training only)
        self.added_kv_proj_dim = added_kv_proj_dim
        self.img_layout = WanImageLayout(dim) if added_kv_proj_dim is not None else None
        self.img_flat = nn.Parameter(torch.zeros(self.img_layout.total, dtype=bf16, device=dev), requires_grad=False) if self.img_layout else None
        self.grad_flat: Optional[torch.Tensor] = None  # fp32, allocated by ``zero_grad_flat`` (the sharded trainer hands in its own buffer)
        self._transposed: Optional[Dict[str, torch.Tensor]] = None
        self._transposed_version = None
        self._grad_hook = None     # callable(block) at the end of the block's backward (its gradients are final)
        self._pre_forward = None   # callable(block) before the block's forward / backward: sharded training gathers the parameters there
        self._pre_backward = None
        self._param_src: Optional[torch.Tensor] = None  # sharded training: the all-gathered parameters to compute with instead of ``flat``
        # LoRA over a frozen base (add_adapter): fp32 adapters on the eight attention projections, LORA_TARGETS order, ranks zero-padded to multiples of 64
        self.frozen = False
        self.lora_A: Optional[nn.Parameter] = None  # [8, r, D]
        self.lora_B: Optional[nn.Parameter] = None  # [8, D, r]
        self.lora_ffn: Optional[nn.ParameterList] = None  # add_adapter(ffn=True): A_1 [r, D], B_1 [F, r], A_2 [r, F], B_2 [D, r] of ffn.net.0.proj / ffn.net.2
        self.lora_scale, self.lora_rank_user = 0.0, 0
        self.gradient_checkpointing = False  # True: the block keeps only its input and refills its saved activations inside the backward
        self._grad_a_view: Optional[torch.Tensor] = None  # the step object's flat gradient views (wan/trainer.py MI355XWanLoRAStep): added to in place
        self._grad_b_view: Optional[torch.Tensor] = None
        self._grad_ffn_views: Optional[Tuple[torch.Tensor, ...]] = None

    # -- parameter / gradient views -----------------------------------------------------------------------------------------------------------
    def _params(self) -> torch.Tensor:
        return self.flat.data if self._param_src is None else self._param_src

    def param(self, name: str) -> torch.Tensor:
        return self.layout.view(self._params(), name)

    def _img_params(self) -> torch.Tensor:
        return self.img_flat.data

    def first_image_tokens(self, enc_img: torch.Tensor, batch: Optional[int] = None) -> int:
        """TI of the C call for ``enc_img`` [B, TI + TI2, D]; ``batch``: the B its rows are read with."""
        n = int(enc_img.shape[1])
        if batch is not None and (enc_img.dim() != 3 or enc_img.shape[0] != batch or enc_img.shape[2] != self.dim or not enc_img.is_contiguous()):
            raise ValueError(f"Wan block: the image context must be a contiguous [{batch}, tokens, {self.dim}] tensor, got {tuple(enc_img.shape)}")
        if n > 0 and n <= self.second_image_tokens:
            raise ValueError(f"Wan first/last-frame block: {n} image tokens, of which {self.second_image_tokens} belong to the second image")
        return n - self.second_image_tokens if n > 0 else 0

    def img_param(self, name: str) -> torch.Tensor:
        return self.img_layout.view(self.img_flat.data, name)

    def grad(self, name: str) -> torch.Tensor:
        if self.grad_flat is None:
            self.zero_grad_flat()
        return self.layout.view(self.grad_flat, name)

    def zero_grad_flat(self, buffer: Optional[torch.Tensor] = None) -> None:
        if buffer is not None:
            if buffer.shape != (self.layout.total,) or buffer.dtype != torch.float32:
                raise ValueError("gradient buffer must be fp32 [layout.total]")
            self.grad_flat = buffer
        if self.grad_flat is None:
            self.grad_flat = torch.zeros(self.layout.total, dtype=torch.float32, device=self.flat.device)
        else:
            self.grad_flat.zero_()

    def named_grads(self) -> Dict[str, torch.Tensor]:
        return self.layout.named_views(self.grad_flat)

    def transposed(self) -> Dict[str, torch.Tensor]:
        """K-contiguous copies of the weights for the input-gradient GEMMs (dX = dY W as an NT GEMM against W^T), rebuilt when the parameters changed."""
        src = self._params()
        ver = (src.data_ptr(), src._version, self._epoch)
        if self._transposed is None or ver != self._transposed_version:
            names = ("w_qkv1", "attn1.to_out.0.weight", "attn2.to_q.weight", "w_kv2", "attn2.to_out.0.weight", "ffn.net.0.proj.weight", "ffn.net.2.weight")
            self._transposed = {n: ops.transpose_bf16(self.param(n)) for n in names}
            self._transposed_version = ver
        return self._transposed

    _epoch = 0

    def mark_updated(self) -> None:
        """The parameters were changed in place by the library (optimiser kernel, all-gather into the same buffer): drop the cached transposes."""
        self._epoch += 1

    # -- LoRA -----------------------------------------------------------------------------------------------------------------------------------
    def freeze_base(self) -> None:
        """Run the block with frozen base weights (input gradients only); ``add_adapter`` implies it."""
        self.frozen = True

    def add_adapter(self, rank: int = 32, lora_alpha: float = 32.0, ffn: bool = False) -> None:
        """peft ``LoraConfig(r, lora_alpha, init_lora_weights=True)`` on the eight attention projections: A kaiming-uniform(a = sqrt(5)), B zero.  Ranks that
        are not multiples of 64 are stored zero-padded; the padding stays zero (a padded row of A only receives gradient through the matching zero column
        of B and the other way round, and AdamW moves a zero parameter with zero gradient nowhere).  ``ffn``: ffn.net.0.proj and ffn.net.2 as well, with the
        same rank and scale and the same initialisation (fan_in of ffn.net.2's A is the feed-forward width)."""
        if rank <= 0 or rank > 128:
            raise ValueError(f"LoRA rank must lie in 1..128, got {rank}")
        if ffn and (self.dim < 256 or self.ffn_dim < 256):
            raise NotImplementedError("Wan block: feed-forward adapters need a width and a feed-forward width of at least 256")
        rp = -(-int(rank) // 64) * 64
        dev, D, F = self.flat.device, self.dim, self.ffn_dim
        a = torch.zeros(8, rp, D, dtype=torch.float32, device=dev)
        a[:, :rank].uniform_(-(1.0 / D) ** 0.5, (1.0 / D) ** 0.5)  # kaiming_uniform_(a = sqrt(5)) on [r, D]: bound = 1 / sqrt(fan_in)
        self.lora_A, self.lora_B = nn.Parameter(a), nn.Parameter(torch.zeros(8, D, rp, dtype=torch.float32, device=dev))
        self.lora_ffn = None
        if ffn:
            a1, a2 = torch.zeros(rp, D, dtype=torch.float32, device=dev), torch.zeros(rp, F, dtype=torch.float32, device=dev)
            a1[:rank].uniform_(-(1.0 / D) ** 0.5, (1.0 / D) ** 0.5)
            a2[:rank].uniform_(-(1.0 / F) ** 0.5, (1.0 / F) ** 0.5)
            z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
            self.lora_ffn = nn.ParameterList([nn.Parameter(a1), nn.Parameter(z(F, rp)), nn.Parameter(a2), nn.Parameter(z(D, rp))])
        self.lora_rank_user, self.lora_scale = int(rank), float(lora_alpha) / rank
        self.frozen = True

    def lora_parameters(self) -> List[nn.Parameter]:
        """The block's adapter Parameters in the order the step object lays them out: lora_A, lora_B, then the four feed-forward matrices."""
        if self.lora_A is None:
            return []
        return [self.lora_A, self.lora_B] + (list(self.lora_ffn) if self.lora_ffn is not None else [])

    def lora_named_views(self, grads: bool = False) -> Dict[str, torch.Tensor]:
        """{peft key relative to the block: view of the user's rank inside the zero-padded storage}; ``grads``: the gradients (the step object's flat views,
        or ``.grad``) under the same keys."""
        if self.lora_A is None:
            return {}
        r = self.lora_rank_user
        own = grads and self._grad_a_view is not None
        pick = (lambda p: p.grad) if grads and not own else (lambda p: p.data)
        a, b = (self._grad_a_view, self._grad_b_view) if own else (pick(self.lora_A), pick(self.lora_B))
        out = {}
        for j, n in enumerate(LORA_TARGETS):
            out[f"{n}.lora_A.weight"] = a[j, :r]
            out[f"{n}.lora_B.weight"] = b[j, :, :r]
        if self.lora_ffn is not None:
            f = self._grad_ffn_views if own else [pick(p) for p in self.lora_ffn]
            for j, n in enumerate(LORA_FFN_TARGETS):
                out[f"{n}.lora_A.weight"] = f[2 * j][:r]
                out[f"{n}.lora_B.weight"] = f[2 * j + 1][:, :r]
        return out

    def _backward_done(self) -> None:
        if self._grad_hook is not None:
            self._grad_hook(self)  # this block's adapter gradients are final: the step object may start their all-reduce

    # -- loading --------------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def load_diffusers_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """``sd``: a diffusers ``WanTransformerBlock`` state dict."""
        img = self.img_layout.entries if self.img_layout else []
        missing = [n for n, _ in self.layout.entries + img if n not in sd]
        if missing:
            raise KeyError(f"Wan block state dict lacks {missing[:4]}")
        for name, view in self.layout.named_views(self.flat.data).items():
            view.copy_(sd[name].to(bf16).reshape(view.shape))
        if self.img_layout:
            for name, view in self.img_layout.named_views(self.img_flat.data).items():
                view.copy_(sd[name].to(bf16).reshape(view.shape))
        self.mark_updated()

    def state_dict_views(self) -> Dict[str, torch.Tensor]:
        if self.flat.numel() < self.layout.total:
            raise RuntimeError("this block's parameters are sharded over the ranks: use the step object's gathered_state_dict()")
        out = self.layout.named_views(self.flat.data)
        if self.img_layout:
            out.update(self.img_layout.named_views(self.img_flat.data))
        return out

    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor, temb: torch.Tensor, rotary, encoder_hidden_states_image=None) -> torch.Tensor:
        if self._pre_forward is not None:
            self._pre_forward(self)
        if (encoder_hidden_states_image is not None) != (self.img_layout is not None):
            raise ValueError("Wan block: the image context goes with added_kv_proj_dim, and only with it")
        if self.img_layout is not None and not self.frozen:
            raise NotImplementedError("Wan image-to-video: full fine-tuning is not covered; attach adapters (add_adapter) or freeze the base (freeze_base)")
        if self.frozen:  # every LoRA configuration: adapters or none, image context or none, feed-forward adapters or none
            fn = _WanLoRABlockNativeFunction if self.native else _WanLoRABlockFunction
            img = None if encoder_hidden_states_image is None else encoder_hidden_states_image.detach().contiguous()
            ffn = (None,) * 4 if self.lora_ffn is None else tuple(self.lora_ffn)
            return fn.apply(self, hidden_states.contiguous(), encoder_hidden_states.contiguous(), temb.contiguous(), rotary[0], rotary[1], self.lora_A, self.lora_B,
                            img, *ffn)
        fn = _WanBlockNativeFunction if self.native else _WanBlockFunction
        return fn.apply(self, hidden_states.contiguous(), encoder_hidden_states.contiguous(), temb.contiguous(), rotary[0], rotary[1])
