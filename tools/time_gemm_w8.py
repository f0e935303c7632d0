"""The fp8-weight GEMMs (ftmi_gemm_nt_w8 / ftmi_gemm_nn_w8) against what serves an fp8-stored weight without them, interleaved in one process, at M = 10 752:
forward   nt_w8(x, w8)   against  fp8_upcast(w8) + gemm_nt(x, w)             and against gemm_nt alone on a resident bf16 weight;
backward  nn_w8(dy, w8)  against  fp8_upcast(w8, transpose) + gemm_nt(dy, wt)  and against gemm_nn on the resident bf16 weight.
Shapes (N, K) of w8 [N, K]: Wan2.1-14B's projections and HunyuanVideo's 3072-wide ones.  Outputs are compared at the timed sizes."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from finetrainers_amd import ops  # noqa: E402

M, REPS = 10752, 30
SHAPES = [(15360, 5120), (5120, 5120), (13824, 5120), (5120, 13824), (9216, 3072), (3072, 3072), (12288, 3072), (3072, 12288)]
g = torch.Generator(device="cuda").manual_seed(0)
bf16 = torch.bfloat16


def mk(r, c, s=1.0):
    return (s * torch.randn(r, c, generator=g, device="cuda")).to(bf16)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


lines = ["# python tools/time_gemm_w8.py: w8 [N, K] float8_e4m3fn; fwd: x [M, K] -> [M, N]; bwd: dy [M, N] -> [M, K]; interleaved in one process, device events",
         f"# around each call (the up-cast launch included where named), 3 warm-up rounds, {REPS} repetitions; ms: median (min - max); TFLOP/s of the median",
         f"devices visible: {torch.cuda.device_count()}   M = {M}"]
for N, K in SHAPES:
    x, dy = mk(M, K), mk(M, N)
    w8 = mk(N, K, K ** -0.5).to(torch.float8_e4m3fn)
    w = ops.fp8_upcast(w8)  # the resident bf16 weight
    arena, arena_t = torch.empty(N * K, device="cuda", dtype=bf16), torch.empty(N * K, device="cuda", dtype=bf16)
    o = {k: torch.empty(M, N if k[0] == "f" else K, device="cuda", dtype=bf16) for k in ("f_w8", "f_up", "f_bf", "b_w8", "b_up", "b_bf")}
    fns = {
        "f_w8": lambda: ops.gemm_nt_w8(x, w8, None, o["f_w8"]),
        "f_up": lambda: ops.gemm_nt(x, ops.fp8_upcast(w8, out=arena), out=o["f_up"]),
        "f_bf": lambda: ops.gemm_nt(x, w, out=o["f_bf"]),
        "b_w8": lambda: ops.gemm_nn_w8(dy, w8, o["b_w8"]),
        "b_up": lambda: ops.gemm_nt(dy, ops.fp8_upcast(w8, out=arena_t, transpose=True), out=o["b_up"]),
        "b_bf": lambda: ops.gemm_nn(dy, w, o["b_bf"]),
    }
    for _ in range(3):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(REPS):
        for k, f in fns.items():
            times[k].append(timed(f))
    med = {k: statistics.median(t) for k, t in times.items()}
    flop = 2.0 * M * N * K
    cell = lambda k: f"{k} {med[k]:.3f} ({min(times[k]):.3f} - {max(times[k]):.3f}) {flop / med[k] / 1e9:.0f}"
    diff = lambda a, b: float((o[a].float() - o[b].float()).abs().max())
    lines.append(f"N={N:5d} K={K:5d}  " + "  ".join(cell(k) for k in fns) + f"  | f_w8/f_up {med['f_w8'] / med['f_up']:.2f} f_w8/f_bf {med['f_w8'] / med['f_bf']:.2f} "
                 f"b_w8/b_up {med['b_w8'] / med['b_up']:.2f} b_w8/b_bf {med['b_w8'] / med['b_bf']:.2f}  max|f_w8 - f_bf| {diff('f_w8', 'f_bf'):.3g} max|b_w8 - b_bf| {diff('b_w8', 'b_bf'):.3g}")
    del x, dy, w8, w, arena, arena_t, o
print("\n".join(lines))
