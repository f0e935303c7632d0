"""Chunk walk (n x ftmi_attn_fwd_carry) against n x ftmi_attn_fwd + fp32 merge in torch, interleaved, at the Wan bucket's per-rank problem for cp = 2."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from finetrainers_amd import ops  # noqa: E402

B, H, d, S, cp = 1, 12, 128, 21504, 2
n = S // cp
g = torch.Generator(device="cuda").manual_seed(0)


def mk(s):
    return torch.randn(B, s, H, d, generator=g, device="cuda", dtype=torch.bfloat16).permute(0, 2, 1, 3)


q = mk(n)
ks, vs = [mk(n) for _ in range(cp)], [mk(n) for _ in range(cp)]
kcat, vcat = torch.cat(ks, 2), torch.cat(vs, 2)
acc = torch.empty(B, H, n, d, device="cuda", dtype=torch.float32)
lse = torch.empty(B, H, n, device="cuda", dtype=torch.float32)


def walk():
    out = None
    for c in range(cp):
        out = ops.attn_fwd_carry(q, ks[c], vs[c], acc, lse, first=c == 0, last=c == cp - 1)
    return out


def merge():
    parts = [ops.attn_fwd(q, ks[c], vs[c]) for c in range(cp)]
    o, l = parts[0][0].float(), parts[0][1]
    for oc, lc in parts[1:]:
        new = torch.logaddexp2(l, lc)
        o = o * torch.exp2(l - new)[..., None] + oc.float() * torch.exp2(lc - new)[..., None]
        l = new
    return o.to(torch.bfloat16)


def one():
    return ops.attn_fwd(q, kcat, vcat)[0]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


fns = dict(walk=walk, merge=merge, one=one)
for _ in range(3):
    for f in fns.values():
        f()
torch.cuda.synchronize()
times = {k: [] for k in fns}
for _ in range(30):
    for k, f in fns.items():
        times[k].append(timed(f))
ref = one().float()
lines = ["# python tools/time_attn_carry.py: n x ftmi_attn_fwd_carry (walk) against n x ftmi_attn_fwd + fp32 merge in torch (merge) and one ftmi_attn_fwd over the",
         "# concatenated keys (one), interleaved in one process; device events around each forward, 3 warm-up rounds",
         f"devices visible: {torch.cuda.device_count()}",
         f"B={B} H={H} d={d} Sq={n} chunks={cp} x {n} keys (Wan bucket 21504 tokens, cp={cp}); 30 interleaved repetitions, ms per forward: median (min - max)"]
flop = 4.0 * B * H * n * S * d
for k, t in times.items():
    med = statistics.median(t)
    lines.append(f"{k:6s} {med:.3f} ({min(t):.3f} - {max(t):.3f})  {flop / med / 1e9:.0f} TFLOP/s")
lines.append(f"max |walk - one call| {float((walk().float() - ref).abs().max()):.4g}   max |merge - one call| {float((merge().float() - ref).abs().max()):.4g}")
print("\n".join(lines))
