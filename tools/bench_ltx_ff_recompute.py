"""What the LTX feed-forward adapters' backward recomputes per block instead of keeping it: g = gelu(z) (ftmi_gelu_from_pre) and n2 = norm2 + modulate
(ftmi_norm_modulate_fwd), timed at BASELINE config 2's shapes (M = 2 x 2688 token rows, D = 2048, D_ff = 8192) with device events.

    python tools/bench_ltx_ff_recompute.py [--rows 5376] [--iters 50] [--blocks 28]

Each launch works on its own buffer set of a ring that is larger than the 256 MiB Infinity Cache, as the step's launches do (a block's z is 88 MB and was
written a whole forward earlier): one buffer timed in a loop would be served from the cache.  Prints one JSON line: microseconds per launch (median and
min over the rounds), algorithmic TB/s (bytes read + written over time), and the per-step total for ``--blocks`` blocks."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bf16 = torch.bfloat16


def _time(fn, sets, iters):
    for s in sets:  # warm every buffer set
        fn(s)
    torch.cuda.synchronize()
    us = []
    for r in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(sets[i % len(sets)])
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / iters)
    us.sort()
    return us[len(us) // 2], us[0]


def main():
    from finetrainers_amd import ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2 * 2688)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=28)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    M, D, F = args.rows, 2048, 8192
    g = torch.Generator(device=dev).manual_seed(0)
    ring = max(2, -(-(512 << 20) // (2 * M * F * 2)))  # sets whose z + g together exceed twice the Infinity Cache
    gelu_sets = [((torch.randn((M, F), generator=g, device=dev) * 2).to(bf16), torch.empty((M, F), dtype=bf16, device=dev)) for _ in range(ring)]
    gelu_med, gelu_min = _time(lambda s: ops.gelu_from_pre(s[0], out=s[1]), gelu_sets, args.iters)
    del gelu_sets
    ring_n = max(2, -(-(512 << 20) // (2 * M * D * 2)))
    shift = (torch.randn((2, D), generator=g, device=dev) * 0.1).to(bf16)
    onep = (1 + torch.randn((2, D), generator=g, device=dev) * 0.1).to(bf16)
    norm_sets = [(torch.randn((M, D), generator=g, device=dev).to(bf16), torch.empty((M, D), dtype=bf16, device=dev)) for _ in range(ring_n)]
    norm_med, norm_min = _time(lambda s: ops.norm_modulate_ex(s[0], shift, onep, s[1], M // 2), norm_sets, args.iters)
    gelu_bytes, norm_bytes = 2 * M * F * 2, 2 * M * D * 2
    print(json.dumps({
        "rows": M, "iters": args.iters, "ring_sets": [ring, ring_n],
        "gelu_from_pre": {"us_median": gelu_med, "us_min": gelu_min, "bytes": gelu_bytes, "tb_per_s": gelu_bytes / (gelu_med * 1e-6) / 1e12},
        "norm_modulate_fwd": {"us_median": norm_med, "us_min": norm_min, "bytes": norm_bytes, "tb_per_s": norm_bytes / (norm_med * 1e-6) / 1e12},
        "per_step_ms": {"blocks": args.blocks, "recompute": args.blocks * (gelu_med + norm_med) / 1e3},
        # the alternative: keep g and n2 per block -- written once more by nothing (the forward writes them anyway, into per-block storage instead of scratch)
        # and read from there, so what keeping saves is exactly the two launches above; what it costs is memory
        "kept_copies_gb": args.blocks * (M * F * 2 + M * D * 2) / 1e9,
    }))


if __name__ == "__main__":
    main()
