"""ftmi_attn_fwd_q8 (pre-pass + forward), its pre-pass alone (ftmi_attn_q8_quant) and ftmi_attn_fwd (bf16), interleaved in one process, at the Wan bucket
(12 heads x 128, 10 752 tokens) and the LTX bucket (64 heads x 64, 2 688 tokens), self-attention.  The forward kernel alone is the difference of the medians."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes  # noqa: E402

from finetrainers_amd import _lib, ops  # noqa: E402
from finetrainers_amd._lib import check, ptr, stream_ptr  # noqa: E402

REPS = 30
g = torch.Generator(device="cuda").manual_seed(0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


lines = ["# python tools/time_attn_q8.py: q8 = ftmi_attn_fwd_q8 (pre-pass + forward, three launches), quant = ftmi_attn_q8_quant (the pre-pass alone, two launches),",
         "# bf16 = ftmi_attn_fwd; interleaved in one process, device events around each call, 3 warm-up rounds; the workspace comes from torch's caching allocator",
         f"devices visible: {torch.cuda.device_count()}; {REPS} interleaved repetitions, ms per call: median (min - max)"]
for name, B, H, d, S in (("Wan", 1, 12, 128, 10752), ("LTX", 1, 64, 64, 2688)):
    q, k, v = (torch.randn(B, S, H, d, generator=g, device="cuda", dtype=torch.bfloat16).permute(0, 2, 1, 3) for _ in range(3))
    _, desc, ws = ops._q8_operands("time_attn_q8", q, k, v, None)

    def quant():  # the C entry itself: ops.attn_q8_quantize would add its de-permuting gathers
        check(_lib.load().ftmi_attn_q8_quant(ctypes.byref(desc), ptr(q), ptr(k), ptr(v), 1, ptr(ws), ws.numel(), stream_ptr()), "ftmi_attn_q8_quant")

    fns = dict(q8=lambda: ops.attn_fwd_q8(q, k, v), quant=quant, bf16=lambda: ops.attn_fwd(q, k, v)[0])
    for _ in range(3):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(REPS):
        for n, f in fns.items():
            times[n].append(timed(f))
    med = {n: statistics.median(t) for n, t in times.items()}
    flop = 4.0 * B * H * S * S * d
    lines.append(f"{name}: B={B} H={H} d={d} Sq=Sk={S}")
    for n, t in times.items():
        rate = "" if n == "quant" else f"  {flop / med[n] / 1e9:.0f} TFLOP/s (4 B H Sq Sk d over the call)"
        lines.append(f"  {n:5s} {med[n]:.3f} ({min(t):.3f} - {max(t):.3f}){rate}")
    ref = ops.attn_fwd(q, k, v)[0].float()
    err = (ops.attn_fwd_q8(q, k, v).float() - ref)
    lines.append(f"  q8 / bf16 {med['q8'] / med['bf16']:.3f}   (q8 - quant) / bf16 {(med['q8'] - med['quant']) / med['bf16']:.3f}   quant / q8 {med['quant'] / med['q8']:.3f}"
                 f"   rms(q8 - bf16) / rms(bf16) {float(err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()):.4f}   max |q8 - bf16| {float(err.abs().max()):.4g}")
    del q, k, v
print("\n".join(lines))
