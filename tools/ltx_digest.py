"""Result tensors of the LTX-Video DiT's C calls (forward, loss backward) over a fixed set of seeded cases, to compare two checkouts of the library bit for
bit: LTX has no Python composition next to its orchestrator, so nothing in the suite can see a change of its bits that stays inside the parity bounds.
Only the public Python API (and the repository's own oracle package, for the seeded weights and inputs) is used, so the same file runs against an older
checkout: copy it into that checkout's tools/ and run it there.

    python tools/ltx_digest.py --out before_1.pt                              # in the checkout to compare with ...
    python tools/ltx_digest.py --out before_2.pt                              # ... twice: what differs between the two is summed with fp32 atomics
    python tools/ltx_digest.py --against before_1.pt --floor before_2.pt      # in this one

Cases: the suite's smallest LTX geometry -- 2 blocks, B = 2, F x H x W = 3 x 4 x 6 (72 tokens), ragged text masks -- at rank 64, rank 128 (two K-extension
steps per plane), rank 32 (zero-padded rank-64 storage) and rank 64 with alpha = 32 (LoRA scale 0.5).  Per case: the prediction, every per-block tensor
``workspace_tensor()`` exposes, the all-block text keys / values, and ``lora_grad_views()`` after one backward.

A tensor that is bit-equal between the two older runs must be bit-equal here.  A tensor that differs between them (the adapter gradients: split-token
fp32 atomics) must lie within a relative distance of 2e-6 of the older run, the project's bound for such sums; the older run's own distance is printed."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(64, 64.0), (128, 128.0), (32, 32.0), (64, 32.0)]  # (rank, alpha)
LAYERS, B, F_, H_, W_ = 2, 2, 3, 4, 6
D = 2048
ATOMIC_BOUND = 2e-6


def _case(rank, alpha, dev):
    from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoModelSpecification
    from finetrainers_amd.trainer import sft_loss
    from oracle import ltx

    cfg = ltx.LTXConfig.production(num_layers=LAYERS)
    omodel = ltx.build_model(cfg, seed=0, rank=rank, alpha=float(alpha), lora_b_std=0.02)
    inp = ltx.synth_inputs(cfg, B, F_, H_, W_, seed=3, mask_lens=[32, 96], sigmas=[0.25, 0.7])
    spec = MI355XLTXVideoModelSpecification(transformer_config=LTXTransformerConfig(num_layers=LAYERS))
    model = spec.load_diffusion_models(state_dict=omodel.state_dict(), device=dev)["transformer"]
    model.add_adapter(r=rank, lora_alpha=alpha)
    model.load_lora_state_dict({k: v for k, v in omodel.state_dict().items() if "lora_" in k})
    pred, target, sig = spec.forward(
        transformer=model,
        condition_model_conditions={"encoder_hidden_states": inp.encoder_hidden_states.to(dev), "encoder_attention_mask": inp.encoder_attention_mask.to(dev)},
        latent_model_conditions={"latents": inp.latents.to(dev), "latents_mean": inp.latents_mean, "latents_std": inp.latents_std,
                                 "num_frames": F_, "height": H_, "width": W_},
        sigmas=inp.sigmas.view(-1, 1, 1, 1, 1).to(dev),
        noise=inp.noise.to(dev),
        first_frame_sigma=None,
        force_first_frame_branch=False,  # (left open, the specification draws the 10 % first-frame branch from the global RNG)
    )
    sft_loss(pred, target, sig, "none").backward()
    torch.cuda.synchronize()
    M, Mt = B * F_ * H_ * W_, B * cfg.text_seq_len
    res = {"pred": pred}
    shapes = {"n1": (M, D), "qkv": (M, 3 * D), "o1": (M, D), "h1": (M, D), "q2raw": (M, D), "o2": (M, D), "h2": (M, D), "z": (M, 4 * D)}
    for l in range(LAYERS):
        for name, shp in shapes.items():
            res[f"{l}.{name}"] = model.workspace_tensor(name, l, shp)
    res["kv2_all"] = model.workspace_tensor("kv2_all", 0, (Mt, LAYERS * 2 * D))
    res.update({f"grad.{k}": v for k, v in model.lora_grad_views().items()})
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def collect():
    dev = torch.device("cuda", 0)
    results = {}
    for rank, alpha in CASES:
        for k, v in _case(rank, alpha, dev).items():
            results[f"r{rank}.a{int(alpha)}/{k}"] = v
    return results


def _dist(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def compare(got, want, floor) -> int:
    bad = 0
    if set(got) != set(want) or set(floor) != set(want):
        print(f"DIFFERENT result sets: only here {sorted(set(got) - set(want))[:4]}, only there {sorted(set(want) - set(got))[:4]}")
        bad += 1
    cases = {}
    for k in sorted(set(got) & set(want) & set(floor)):
        case, name = k.split("/", 1)
        c = cases.setdefault(case, {"exact": 0, "atomic": 0, "worst": 0.0, "worst_floor": 0.0, "worst_name": "-", "fail": []})
        if torch.equal(want[k], floor[k]):  # the older checkout reproduces these bits: so must this one
            ok = torch.equal(got[k], want[k])
            c["exact"] += 1
        else:
            d = _dist(got[k], want[k])
            ok = d < ATOMIC_BOUND
            c["atomic"] += 1
            if d >= c["worst"]:
                c["worst"], c["worst_floor"], c["worst_name"] = d, _dist(floor[k], want[k]), name
        if not ok:
            c["fail"].append(name)
    for case, c in cases.items():
        bad += len(c["fail"])
        print(f"{case:10s} {c['exact']} tensors bit-equal, {c['atomic']} summed with atomics: worst {c['worst']:.2e} ({c['worst_name']}; the older checkout "
              f"against itself {c['worst_floor']:.2e}) " + (f"FAIL {c['fail']}" if c["fail"] else "ok"))
    print(f"{len(cases)} cases, {len(got)} tensors: " + ("all within bounds" if not bad else f"{bad} OUT OF BOUNDS"))
    return bad


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="save every result tensor to this file")
    ap.add_argument("--against", help="compare with a file saved by --out in the older checkout")
    ap.add_argument("--floor", help="a second file saved by the older checkout: separates what it reproduces bit for bit from what it sums with atomics")
    args = ap.parse_args()
    if args.against and not args.floor:
        ap.error("--against needs --floor")
    results = collect()
    if args.out:
        torch.save(results, args.out)
        print(f"{len(results)} tensors saved to {args.out}")
    if args.against:
        sys.exit(1 if compare(results, torch.load(args.against), torch.load(args.floor)) else 0)


if __name__ == "__main__":
    main()
