"""Result tensors of ``MI355XWanBlock`` forward + backward over a fixed set of seeded cases, to compare two checkouts of the library bit for bit
(the C-call-vs-Python-composition tests cannot see a change made identically to both implementations).  Only the public Python API is used, so the same
file runs against an older checkout: copy it into that checkout's tools/ and run it there.

    python tools/wan_block_digest.py --out before.pt        # in the checkout to compare with
    python tools/wan_block_digest.py --against before.pt    # in this one

Modes: full fine-tune; frozen base, r = 0; r = 32 (peft's init, B = 0); r = 64 with non-zero B -- each with ``native`` on and off, at (B, S, T) = (2, 48, 16) and
(1, 200, 64) at width 256 and (1, 200, 64) at the Wan2.1-T2V-1.3B block geometry; one LoRA case with gradient checkpointing, one with the text input not
requiring grad.  The LoRA configurations beyond the eight attention adapters, each with ``native`` on and off at the two width-256 shapes: ``i2v_r32`` (an
image-to-video block, TI = 257 image tokens, r = 32 with peft's init), ``ffn_r64`` (adapters on the two feed-forward projections as well, non-zero B on all ten)
and ``i2v_ffn_r64`` (both); ``i2v_r32`` once with an empty image context (TI = 0), ``i2v_ffn_r64`` once with gradient checkpointing, ``ffn_r64`` once at the
Wan2.1-T2V-1.3B block geometry.  Output, dx and d text must be equal bit for bit; what is accumulated with fp32 atomics (flat parameter gradients, dmod, adapter
gradients) within a relative distance of 2e-6, the bound of the C-vs-Python tests for the same quantities.  The time projection goes in as fp32, so that dmod
comes back as the fp32 sums (handed back in bf16, single entries land on the other side of a rounding boundary from run to run)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

bf16 = torch.bfloat16
SMALL, REAL = (256, 2, 512), (1536, 12, 8960)
SHAPES = [(SMALL, 2, 48, 16), (SMALL, 1, 200, 64), (REAL, 1, 200, 64)]
MODES = ("full", "frozen_r0", "r32", "r64")
WIDE_MODES = ("i2v_r32", "ffn_r64", "i2v_ffn_r64")  # [i2v_][ffn_]r<rank>: image context in attn2, adapters on ffn.net.0.proj / ffn.net.2 as well
TI = 257  # tests/test_gpu_wan_i2v.py
EXACT = ("out", "dx", "denc")
ATOMIC_BOUND = 2e-6


def _block(geom, mode, dev):
    from finetrainers_amd.wan import MI355XWanBlock

    D, H, F = geom
    i2v, ffn = "i2v" in mode, "ffn" in mode
    blk = MI355XWanBlock(dim=D, heads=H, ffn_dim=F, device=dev, **(dict(added_kv_proj_dim=D) if i2v else {}))
    g = torch.Generator().manual_seed(11)
    views = blk.layout.named_views(blk.flat.data)
    if i2v:
        views.update(blk.img_layout.named_views(blk.img_flat.data))
    for name, view in views.items():
        if "norm" in name and name.endswith("weight"):
            v = 1 + 0.1 * torch.randn(view.shape, generator=g)
        elif name.endswith("bias"):
            v = 0.05 * torch.randn(view.shape, generator=g)
        else:  # weights and the scale_shift_table
            v = torch.randn(view.shape, generator=g) * view.shape[-1] ** -0.5
        view.copy_(v.to(bf16))
    blk.mark_updated()
    if mode == "frozen_r0":
        blk.freeze_base()
    elif mode != "full":
        rank = int(mode.rsplit("r", 1)[1])
        blk.add_adapter(rank, float(rank), **(dict(ffn=True) if ffn else {}))
        with torch.no_grad():
            blk.lora_A.data[:, :rank].copy_(torch.randn(8, rank, D, generator=g) * D ** -0.5)
            if rank == 64:
                blk.lora_B.data[:, :, :rank].copy_(0.02 * torch.randn(8, D, rank, generator=g))
            if ffn:  # A_1 [r, D], B_1 [F, r], A_2 [r, F], B_2 [D, r], all non-zero
                a1, b1, a2, b2 = blk.lora_ffn
                a1.data[:rank].copy_(torch.randn(rank, D, generator=g) * D ** -0.5)
                b1.data[:, :rank].copy_(0.02 * torch.randn(F, rank, generator=g))
                a2.data[:rank].copy_(torch.randn(rank, F, generator=g) * F ** -0.5)
                b2.data[:, :rank].copy_(0.02 * torch.randn(D, rank, generator=g))
    return blk


def _inputs(B, S, T, D, dev):
    g = torch.Generator().manual_seed(B * 1000 + S + 7)
    x = torch.randn(B, S, D, generator=g).to(bf16)
    enc = torch.randn(B, T, D, generator=g).to(bf16)
    temb = (0.5 * torch.randn(B, 6, D, generator=g)).to(bf16)
    dout = torch.randn(B, S, D, generator=g).to(bf16)
    ang = torch.rand(S, 64, generator=g, dtype=torch.float64) * 6.283
    return [t.to(dev) for t in (x, enc, temb, dout, torch.cos(ang).float(), torch.sin(ang).float())]


def _image(B, ti, D, dev):
    return torch.randn(B, ti, D, generator=torch.Generator().manual_seed(B * 1000 + ti + 3)).to(bf16).to(dev)


def _run(blk, inputs, enc_grad=True, img=None):
    x, enc, temb, dout, cos, sin = inputs
    xg, eg = x.clone().requires_grad_(True), enc.clone().requires_grad_(enc_grad)
    tg = temb.float().requires_grad_(not blk.frozen)  # fp32 time projection: its gradient comes back as the fp32 modulation sums, not rounded to bf16
    for p in blk.lora_parameters():
        p.grad = None
    if not blk.frozen:
        blk.zero_grad_flat()
    out = blk(xg, eg, tg, (cos, sin), **(dict(encoder_hidden_states_image=img) if img is not None else {}))
    out.backward(dout)
    torch.cuda.synchronize()
    res = {"out": out.detach(), "dx": xg.grad}
    if enc_grad:
        res["denc"] = eg.grad
    if not blk.frozen:
        res["dmod"] = tg.grad
        res.update({f"grad.{n}": v for n, v in blk.named_grads().items()})
    if blk.lora_A is not None:
        res["lora_A.grad"], res["lora_B.grad"] = blk.lora_A.grad, blk.lora_B.grad
    if blk.lora_ffn is not None:
        res.update({f"lora_ffn.{n}.grad": p.grad for n, p in zip(("A1", "B1", "A2", "B2"), blk.lora_ffn)})
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def collect():
    dev = torch.device("cuda", 0)
    results = {}
    for geom, B, S, T in SHAPES:
        inputs = _inputs(B, S, T, geom[0], dev)
        for mode in MODES + tuple(m for m in WIDE_MODES if geom == SMALL or m == "ffn_r64"):
            blk = _block(geom, mode, dev)
            img = _image(B, TI, geom[0], dev) if "i2v" in mode else None
            variants = [("", {})]
            if mode == "r64" and (geom, S) == (SMALL, 48):
                variants += [("+ckpt", dict(ckpt=True)), ("+frozen_text", dict(enc_grad=False))]
            if mode == "i2v_r32" and S == 48:
                variants += [("+ti0", dict(ti0=True))]
            if mode == "i2v_ffn_r64" and S == 48:
                variants += [("+ckpt", dict(ckpt=True))]
            for tag, kw in variants:
                for native in (True, False):
                    blk.native = native
                    blk.gradient_checkpointing = bool(kw.get("ckpt", False))
                    case = f"D{geom[0]}.B{B}.S{S}.T{T}/{mode}{tag}/{'native' if native else 'python'}"
                    for k, v in _run(blk, inputs, enc_grad=kw.get("enc_grad", True), img=img[:, :0] if kw.get("ti0") else img).items():
                        results[f"{case}/{k}"] = v
            del blk
    return results


def compare(got, want) -> int:
    bad = 0
    if set(got) != set(want):
        print(f"DIFFERENT result sets: only here {sorted(set(got) - set(want))[:4]}, only there {sorted(set(want) - set(got))[:4]}")
        bad += 1
    cases = {}
    for k in sorted(set(got) & set(want)):
        case, name = k.rsplit("/", 1)
        a, b = got[k], want[k]
        c = cases.setdefault(case, {"exact": 0, "worst": 0.0, "worst_name": "-", "fail": []})
        if name in EXACT:
            ok = torch.equal(a, b)
            c["exact"] += 1
        else:
            d = float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))
            ok = d < ATOMIC_BOUND
            if d >= c["worst"]:
                c["worst"], c["worst_name"] = d, name
        if not ok:
            c["fail"].append(name)
    for case, c in cases.items():
        bad += len(c["fail"])
        print(f"{case:56s} {c['exact']} tensors bit-equal, atomics worst {c['worst']:.2e} ({c['worst_name']}) " + (f"FAIL {c['fail']}" if c["fail"] else "ok"))
    print(f"{len(cases)} cases, {len(got)} tensors: " + ("all within bounds" if not bad else f"{bad} OUT OF BOUNDS"))
    return bad


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="save every result tensor to this file")
    ap.add_argument("--against", help="compare with a file saved by --out")
    args = ap.parse_args()
    results = collect()
    if args.out:
        torch.save(results, args.out)
        print(f"{len(results)} tensors saved to {args.out}")
    if args.against:
        sys.exit(1 if compare(results, torch.load(args.against)) else 0)


if __name__ == "__main__":
    main()
