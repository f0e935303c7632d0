"""ftmi_gemm_nn against ftmi_gemm_nt_ex on the transposed twin, interleaved, at the four Wan2.1-14B input-gradient shapes (M = 10 752 tokens)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from finetrainers_amd import ops  # noqa: E402

M = 10752
# (N = reduction, K = output width, K2): attn1 q|k|v, a square projection, ffn.net.0.proj and ffn.net.2 (the last two also with a rank-64 adapter's extension)
SHAPES = [(15360, 5120, 0), (5120, 5120, 0), (13824, 5120, 0), (5120, 13824, 0), (13824, 5120, 192), (5120, 13824, 192)]
g = torch.Generator(device="cuda").manual_seed(0)


def mk(r, c, s=1.0):
    return (s * torch.randn(r, c, generator=g, device="cuda")).to(torch.bfloat16)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


lines = ["# python tools/time_gemm_nn.py: ftmi_gemm_nn on W [N, K] (nn) against ftmi_gemm_nt_ex on the twin W^T [K, N] (nt), interleaved in one process;",
         "# device events around each launch, 3 warm-up rounds, 30 repetitions; ms per launch: median (min - max)",
         f"devices visible: {torch.cuda.device_count()}   M = {M}"]
for N, K, K2 in SHAPES:
    dy, w = mk(M, N), mk(N, K, N ** -0.5)
    wt = w.t().contiguous()
    x2, w2 = (mk(M, K2), mk(K, K2, 0.05)) if K2 else (None, None)
    o_nn, o_nt = torch.empty(M, K, device="cuda", dtype=torch.bfloat16), torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
    ext = dict(x2=x2, w2=w2, K2=K2) if K2 else {}
    fns = dict(nn=lambda: ops.gemm_nn(dy, w, o_nn, x2=x2, w2=w2), nt=lambda: ops.gemm_nt_ex(dy, wt, o_nt, M=M, N=K, K=N, variant=8, **ext))
    for _ in range(3):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(30):
        for k, f in fns.items():
            times[k].append(timed(f))
    flop = 2.0 * M * K * (N + K2)
    med = {k: statistics.median(t) for k, t in times.items()}
    diff = float((o_nn.float() - o_nt.float()).abs().max())
    kind, variant, rows, cols = ops.gemm_nt_route(M=M, N=K, K=N, K2=K2, variant=8)  # what the NT launcher ran for the twin
    lines.append(f"N={N:5d} K={K:5d} K2={K2:3d}  " + "  ".join(f"{k} {med[k]:.3f} ({min(t):.3f} - {max(t):.3f}) {flop / med[k] / 1e9:.0f} TFLOP/s" for k, t in times.items())
                 + f"  [nt: kind {kind} variant {variant}, {rows} x {cols} tile]  nn / nt {med['nn'] / med['nt']:.2f}  max |nn - nt| {diff:.3g}  elements that differ {float((o_nn != o_nt).float().mean()):.2e}")
    del dy, w, wt, o_nn, o_nt
print("\n".join(lines))
