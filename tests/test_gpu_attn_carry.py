"""The carried-softmax forward (ftmi_attn_fwd_carry) and the chunked attention built on it (attention_dispatch.chunked_attention) against a plain fp64 softmax
attention on the CPU over the concatenated keys.  B = 2, H = 3, every tensor a [B, S, H, d + 8] buffer's [B, H, S, d] view (room between the rows, NaN in it).

BOUNDS, per element, from the number formats (E = 2^-8, the unit roundoff of bf16: 8 significant bits; p = softmax weights, all sums over the reduction index):
  out  E |ref| + 2 E sum p |v|                 the bf16 result; the bf16 P in the numerator and, through l, in the denominator
  lse  (natural log) E + 2^-20 max(1, |ref|)    l sums the bf16 P: relative error E of l; fp32 slack
  dv   E |ref| + 2 E sum p |do|                 the bf16 P; p itself through the lse error
  dk   E |ref| + 3 E scale sum A |q|            A = p (|dP - delta| + D), D = sum |o| |do|: bf16 dS, p through lse, delta from the bf16 out
  dq   (n + 1) E scale sum |dS| |k| + 3 E scale sum A |k|      one bf16 rounding per chunk share and one of the fp32 sum (n = 1: the one-call backward)
ASSERTED per case and quantity, with r = largest |got - ref| / bound: r(walk) <= 1 and r(walk) <= r(one call) + MARGIN, the one call being ops.attn_fwd /
ops.attn_bwd on the concatenated keys in the same test, against the same bounds.  Nothing is rounded between the chunks, so the two are two draws of the same
rounding noise (other sum order, other running max under the lazy rescale) and must sit at the same place inside the bounds.  MEASURED on an MI355X over the
26 shape cases: r(walk) - r(one call) lies in [-0.054, +0.100] (out +0.052, lse +0.100, dq +0.039, dk +0.035, dv +0.057 at most); MARGIN = 0.15 is 1.5 x
that spread.  Largest r, walk (one call): out 0.416 (0.416)  lse 0.415 (0.415)  dq 0.174 (0.174)  dk 0.367 (0.362)  dv 0.579 (0.565); the single-chunk
cases lead out and lse; walks of two and three chunks alone: out 0.330 (0.330)  lse 0.317 (0.315)  dq 0.148 (0.109).
"""

import functools
import math

import pytest
import torch

from finetrainers_amd import ops
from finetrainers_amd.attention_dispatch import chunked_attention

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
B, E, MARGIN, NINF = 2, 2.0**-8, 0.15, float("-inf")
SHAPES = pytest.mark.parametrize("d,Sq,chunks,H", [(d, Sq, c, 3) for d in (64, 128) for Sq in (5, 129, 200) for c in ((7,), (64, 64), (1, 63, 65), (70, 130, 3))]
                                 + [(64, 200, (64, 64), 4), (128, 129, (70, 130, 3), 4)])  # H B = 8: the other block order of the kernel


def reference(q, k, v, bias=None, dout=None):
    """fp64 attention of bf16-valued CPU tensors [B, H, S, d] (bias [B, Sk]); with dout also the gradients and the magnitudes the bounds are made of."""
    q, k, v = (t.to(f64).requires_grad_(dout is not None) for t in (q, k, v))
    scale = 1.0 / math.sqrt(q.shape[-1])
    s = q @ k.transpose(-1, -2) * scale + (0.0 if bias is None else bias.to(f64)[:, None, None, :])
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    out = p @ v
    r = dict(out=out.detach(), lse=lse.detach(), out_mag=(p @ v.abs()).detach())
    if dout is not None:
        do = dout.to(f64)
        out.backward(do)
        with torch.no_grad():
            dP = do @ v.transpose(-1, -2)
            delta = (do * out).sum(-1, keepdim=True)
            dS, A = p * (dP - delta), p * ((dP - delta).abs() + (do.abs() * out.abs()).sum(-1, keepdim=True))
            r.update(dq=q.grad, dk=k.grad, dv=v.grad, dv_mag=p.transpose(-1, -2) @ do.abs(), dk_mag=scale * (A.transpose(-1, -2) @ q.abs()),
                     dq_mag=scale * (A @ k.abs()), dq_round=scale * (dS.abs() @ k.abs()))
    return r


@functools.lru_cache(maxsize=None)
def problem(d, Sq, chunks, H=3):
    g = torch.Generator().manual_seed(17 * d + Sq + 1000 * len(chunks) + H)
    q, k, v, dout = (torch.randn(B, H, S, d, generator=g).to(bf16) for S in (Sq, sum(chunks), sum(chunks), Sq))
    return q, k, v, dout, reference(q, k, v, None, dout)


def dev(t, chunks=None):
    if chunks is not None:
        return [dev(c) for c in t.split(list(chunks), dim=2)]
    buf = torch.full((t.shape[0], t.shape[2], t.shape[1], t.shape[3] + 8), float("nan"), dtype=bf16, device="cuda")
    view = buf[..., : t.shape[3]].permute(0, 2, 1, 3)
    view.copy_(t)
    return view


def walk(q, ks, vs, biases=None, start=0):
    """The chunks from `start` on through ftmi_attn_fwd_carry; returns out and the (acc, lse) state after every call."""
    acc = torch.full(q.shape, float("nan"), dtype=f32, device="cuda")
    lse = torch.full(q.shape[:3], float("nan"), dtype=f32, device="cuda")
    out, states = None, []
    for c in range(start, len(ks)):
        out = ops.attn_fwd_carry(q, ks[c], vs[c], acc, lse, key_bias=None if biases is None else biases[c], first=c == start, last=c == len(ks) - 1)
        states.append((acc.clone(), lse.clone()))
    return out, states


def worst(got, ref, bound):
    return float(((got.detach().cpu().to(f64) - ref).abs() / bound).max())


def fwd_ratios(out, lse2, r):
    return (worst(out, r["out"], E * r["out"].abs() + 2 * E * r["out_mag"]),
            worst(lse2.cpu().to(f64) * math.log(2.0), r["lse"], E + 2.0**-20 * r["lse"].abs().clamp_min(1.0)))


def check(what, got, one):
    """Inside the format bound, and no further from fp64 than the one-call kernel on the same inputs plus the margin."""
    print(f"{what}: walk {[round(g, 3) for g in got]}   one call {[round(o, 3) for o in one]}")
    assert all(g <= min(1.0, o + MARGIN) for g, o in zip(got, one)), (what, got, one)


@SHAPES
def test_forward(d, Sq, chunks, H):
    q, k, v, _, r = problem(d, Sq, chunks, H)
    out, states = walk(dev(q), dev(k, chunks), dev(v, chunks))
    assert torch.equal(out, states[-1][0].to(bf16))  # out is the bf16 of the state
    check(f"out, lse d={d} Sq={Sq} chunks={chunks} H={H}", fwd_ratios(out, states[-1][1], r), fwd_ratios(*ops.attn_fwd(dev(q), dev(k), dev(v)), r))


@pytest.mark.parametrize("kind", ["middle", "first", "one"])
@pytest.mark.parametrize("d", [64, 128])
def test_masked_chunks(d, kind):
    chunks, Sq = (70, 130, 3), 129
    q, k, v, _, _ = problem(d, Sq, chunks)
    bias = torch.zeros(B, sum(chunks))
    if kind == "middle":
        bias[:, 70:200] = NINF
    elif kind == "first":
        bias[:, :70] = NINF
    else:
        bias[:] = NINF
        bias[0, 100], bias[1, 201] = 0.0, 0.0  # one key kept per sample: in the middle chunk, in the last
    qd, ks, vs = dev(q), dev(k, chunks), dev(v, chunks)
    biases = [b.contiguous().cuda() for b in bias.split(list(chunks), dim=1)]
    if kind == "middle":
        biases[0] = None  # the walk changes between the plain and the biased kernel
    out, states = walk(qd, ks, vs, biases)
    assert not any(torch.isnan(t).any() for st in states for t in st) and not torch.isnan(out).any()
    if kind == "middle":  # a chunk of removed keys leaves the state as it was
        assert torch.equal(states[1][0], states[0][0]) and torch.equal(states[1][1], states[0][1])
    if kind == "first":  # nothing seen after the first chunk; from there on the walk is the one that starts with the second chunk
        assert (states[0][1] == NINF).all() and (states[0][0] == 0).all()
        _, late = walk(qd, ks, vs, biases, start=1)
        assert torch.equal(states[-1][0], late[-1][0]) and torch.equal(states[-1][1], late[-1][1])
    if kind == "one":  # weight exactly 1 on the kept key
        assert torch.equal(out.cpu(), torch.stack([v[0, :, 100], v[1, :, 201]])[:, :, None, :].expand_as(out))
    else:
        r = reference(q, k, v, bias)
        check(f"out, lse d={d} {kind}", fwd_ratios(out, states[-1][1], r), fwd_ratios(*ops.attn_fwd(qd, dev(k), dev(v), bias.cuda()), r))


@SHAPES
def test_backward(d, Sq, chunks, H):
    q, k, v, dout, r = problem(d, Sq, chunks, H)
    bounds = dict(dq=(len(chunks) + 1) * E * r["dq_round"] + 3 * E * r["dq_mag"], dk=E * r["dk"].abs() + 3 * E * r["dk_mag"], dv=E * r["dv"].abs() + 2 * E * r["dv_mag"])
    qd, kd, vd = dev(q).requires_grad_(), dev(k), dev(v)
    ks, vs = ([c.requires_grad_() for c in dev(t, chunks)] for t in (k, v))
    chunked_attention(qd, ks, vs).backward(dev(dout))
    got = (qd.grad, torch.cat([c.grad for c in ks], dim=2), torch.cat([c.grad for c in vs], dim=2))
    one = ops.attn_bwd(qd.detach(), kd, vd, *ops.attn_fwd(qd.detach(), kd, vd), dev(dout))
    check(f"dq, dk, dv d={d} Sq={Sq} chunks={chunks} H={H}", *([worst(g, r[t], bounds[t]) for g, t in zip(gs, bounds)] for gs in (got, one)))
