"""Kernel times of the wide second-context attention pair (``ftmi_attn_ctx2w_fwd / _dq``) at the Wan 14B first/last-frame shape -- B 1, 40 heads, S 20 280 video
queries (the 49 x 480 x 832 bucket), 514 image keys -- interleaved on one GPU with its two yardsticks (profiles/wan_flf_ctx2.txt):

  (a) the same loop with the narrow pair's single-buffered staging, ``ftmi_attn_ctx2w1_*``: a lab variant of the same template that only a library built with
      FTMI_EXPERIMENTAL=1 exports (point FTMI_LIB_PATH at such a build; without it the rows are reported as "not built");
  (b) ``ftmi_attn_fwd`` on 512 text keys with the same queries (the text branch of the same attn2).

Every arm is warmed up, then timed in ``--rounds`` alternating rounds of ``--iters`` launches between two device events; the table gives each arm's median and
its min .. max over the rounds (the run-to-run spread a difference has to clear), and the outputs of (a) and of the shipped pair are compared bit for bit.

    python tools/bench_ctx2w.py [--heads 40] [--queries 20280] [--keys 514] [--rounds 7] [--iters 20]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bf16 = torch.bfloat16


def main():
    from finetrainers_amd import _lib, ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=40)
    ap.add_argument("--queries", type=int, default=13 * 30 * 52)
    ap.add_argument("--keys", type=int, default=514)
    ap.add_argument("--text-keys", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    lab = hasattr(lib, "ftmi_attn_ctx2w1_fwd")
    H, S, Sk, T = args.heads, args.queries, args.keys, args.text_keys
    D = H * 128
    g = torch.Generator(device=dev).manual_seed(0)
    rows = lambda n, w: torch.randn(1, n, w, generator=g, device=dev).to(bf16)
    heads = lambda t: t.unflatten(2, (H, 128)).permute(0, 2, 1, 3)
    # the block's layouts: q, o, dO, dq rows of [B, S, D]; k_i | v_i the halves of [B, Sk, 2D] (text k, v likewise)
    q, o_t, do, dq_t = (heads(rows(S, D)) for _ in range(4))
    kvi, kvt = rows(Sk, 2 * D), rows(T, 2 * D)
    ki, vi, kt, vt = heads(kvi[:, :, :D]), heads(kvi[:, :, D:]), heads(kvt[:, :, :D]), heads(kvt[:, :, D:])

    _, lse = ops.attn_ctx2w_fwd(q, ki, vi, o_t)
    arms = {
        "ctx2w_fwd  two slots (shipped)": lambda: ops.attn_ctx2w_fwd(q, ki, vi, o_t),
        "ctx2w_dq   two slots (shipped)": lambda: ops.attn_ctx2w_dq(q, ki, vi, lse, do, dq_t),
        f"attn_fwd   {T} text keys (b)": lambda: ops.attn_fwd(q, kt, vt),
    }
    if lab:
        arms["ctx2w1_fwd one slot (a, lab)"] = lambda: ops._ctx2_fwd("ftmi_attn_ctx2w1_fwd", q, ki, vi, o_t, None)
        arms["ctx2w1_dq  one slot (a, lab)"] = lambda: ops._ctx2_dq("ftmi_attn_ctx2w1_dq", q, ki, vi, lse, do, dq_t, None, False)
        for name, a, b in (("o", arms["ctx2w_fwd  two slots (shipped)"]()[0], arms["ctx2w1_fwd one slot (a, lab)"]()[0]),
                           ("dq", arms["ctx2w_dq   two slots (shipped)"](), arms["ctx2w1_dq  one slot (a, lab)"]())):
            torch.cuda.synchronize()
            print(f"bits: {name} of the one-slot lab variant == shipped: {torch.equal(a, b)}")
    if Sk <= 320:
        arms["ctx2_fwd   narrow pair"] = lambda: ops.attn_ctx2_fwd(q, ki, vi, o_t)
        arms["ctx2_dq    narrow pair"] = lambda: ops.attn_ctx2_dq(q, ki, vi, lse, do, dq_t)
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in arms}
    for _ in range(args.rounds):
        for n, fn in arms.items():  # alternate the arms inside every round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / args.iters)
    print(f"B 1, H {H}, S {S}, image keys {Sk}; {args.rounds} alternating rounds x {args.iters} launches, us per launch (incl. the wrapper's allocations)")
    flop = lambda keys, mm: 2.0 * mm * S * keys * D  # mm matrix products of [S, keys, 128] per head
    work = {"fwd": flop(Sk, 2), "dq": flop(Sk, 5), "attn_fwd": flop(T, 2)}
    for n, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        kind = "attn_fwd" if n.startswith("attn_fwd") else ("dq" if "_dq" in n else "fwd")
        print(f"  {n:34s} median {med:9.1f}  min {ts[0]:9.1f}  max {ts[-1]:9.1f}   {work[kind] / med / 1e6:7.1f} TFLOP/s algorithmic")
    if not lab:
        print("  yardstick (a): not built (this library has no ftmi_attn_ctx2w1_*; build with FTMI_EXPERIMENTAL=1 and set FTMI_LIB_PATH)")


if __name__ == "__main__":
    main()
