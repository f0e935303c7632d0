"""Result tensors of the LTX-Video DiT's C calls (forward, per-frame forward, loss backward, the two samplers) over a fixed set of seeded cases, to compare two checkouts of the library bit for
bit: LTX has no Python composition next to its orchestrator, so nothing in the suite can see a change of its bits that stays inside the parity bounds.
Only the public Python API (and the repository's own oracle package, for the seeded weights and inputs) is used, so the same file runs against an older
checkout: copy it into that checkout's tools/ and run it there.

    python tools/ltx_digest.py --out before_1.pt                              # in the checkout to compare with ...
    python tools/ltx_digest.py --out before_2.pt                              # ... twice: what differs between the two is summed with fp32 atomics
    python tools/ltx_digest.py --against before_1.pt --floor before_2.pt      # in this one

Cases: the suite's smallest LTX geometry -- 2 blocks, B = 2, F x H x W = 3 x 4 x 6 (72 tokens), ragged text masks -- at rank 64, rank 128 (two K-extension
steps per plane), rank 32 (zero-padded rank-64 storage) and rank 64 with alpha = 32 (LoRA scale 0.5).  Per case: the prediction, every per-block tensor
``workspace_tensor()`` exposes, the all-block text keys / values, and ``lora_grad_views()`` after one backward.  The ten-adapter model (feed-forward adapters,
seeded random values in every adapter) adds the same with its four feed-forward gradients.  Per model kind (eight / ten adapters), forward only: one
``frame_timestep`` forward, and ``MI355XLTXLatentSampler.sample`` at 3 steps, text-to-video and with the first latent frame held, with guidance 3 and without.
``tools/hy_sample_digest.py`` does the same for the HunyuanVideo sampler through this file's ``run``.

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
CONTROL = "(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|ff.net.0.proj|ff.net.2)"  # ten adapters per block
ROPE_SCALE = [1 / (25 / 8), 32, 32]


def _case(rank, alpha, dev, ten=False):
    from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoModelSpecification
    from finetrainers_amd.trainer import sft_loss
    from oracle import ltx

    cfg = ltx.LTXConfig.production(num_layers=LAYERS)
    omodel = ltx.build_model(cfg, seed=0, rank=rank, alpha=float(alpha), lora_b_std=0.02)
    inp = ltx.synth_inputs(cfg, B, F_, H_, W_, seed=3, mask_lens=[32, 96], sigmas=[0.25, 0.7])
    spec = MI355XLTXVideoModelSpecification(transformer_config=LTXTransformerConfig(num_layers=LAYERS))
    model = spec.load_diffusion_models(state_dict=omodel.state_dict(), device=dev)["transformer"]
    if ten:  # the oracle package builds the eight attention adapters only: seeded values in every adapter, the feed-forward ones included
        model.add_adapter(r=rank, lora_alpha=alpha, target_modules=CONTROL)
        with torch.no_grad():
            model.lora_flat.copy_(torch.randn(model.lora_flat.shape, generator=torch.Generator(device=dev).manual_seed(9), device=dev) * 0.01)
    else:
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
    if rank == 64 and alpha == 64.0:
        res.update(_forward_only(model, inp, dev))
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def _forward_only(model, inp, dev):
    """The per-frame forward and the two samplers over ``model`` as it stands."""
    from finetrainers_amd.ltx_video.sampler import MI355XLTXLatentSampler

    bf16 = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(17)
    S, C, T = F_ * H_ * W_, 128, inp.encoder_hidden_states.shape[1]
    res = {}
    with torch.no_grad():
        x_t = torch.randn((B, S, C), generator=g, device=dev).to(bf16)
        ft = torch.tensor([[0.0, 250.0, 250.0], [0.0, 700.0, 700.0]], device=dev)
        res["frames.pred"] = model(x_t, inp.encoder_hidden_states.to(dev), None, inp.encoder_attention_mask.to(dev), F_, H_, W_, ROPE_SCALE, frame_timestep=ft)["sample"]
        text_c = torch.randn((1, T, 4096), generator=g, device=dev).to(bf16)
        text_u = torch.randn((1, T, 4096), generator=g, device=dev).to(bf16)
        mask_c, mask_u = torch.zeros((1, T), dtype=bf16, device=dev), torch.zeros((1, T), dtype=bf16, device=dev)
        mask_c[:, :96], mask_u[:, :32] = 1, 1
        lat0 = torch.randn((1, C, F_, H_, W_), generator=g, device=dev)
        sig = [1.0, 0.71, 0.33, 0.0]
        for hold in (0, 1):
            for guidance in (3.0, 1.0):
                kw = dict(num_frames=F_, height=H_, width=W_, guidance_scale=guidance, sigmas=sig, timesteps=[1000.0 * s for s in sig[:-1]], latents=lat0)
                if hold:
                    kw["cond_frames"] = 1
                res[f"sample.hold{hold}.g{int(guidance)}"] = MI355XLTXLatentSampler(model).sample(text_c, mask_c, text_u if guidance != 1.0 else None,
                                                                                                 mask_u if guidance != 1.0 else None, **kw)
    torch.cuda.synchronize()
    return res


def collect():
    dev = torch.device("cuda", 0)
    results = {}
    for rank, alpha in CASES:
        for k, v in _case(rank, alpha, dev).items():
            results[f"r{rank}.a{int(alpha)}/{k}"] = v
    for k, v in _case(64, 64.0, dev, ten=True).items():
        results[f"ten.r64/{k}"] = v
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


def run(collect) -> None:
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
    run(collect)
