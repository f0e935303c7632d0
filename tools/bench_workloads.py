"""The workloads `bench.py --workload {ltx,cogvideox,wan,hunyuan}` can time (BASELINE.json configs[1], [2], [3], [4]), plus the Wan LoRA recipe
(`wan_lora`), control recipe (`wan_control_lora`) and latent sampling (`wan_sample`), run through this file's own command line (`python tools/bench_workloads.py --workload wan_lora`): for each one a
builder that puts a random-init model of the named architecture, its step object and one synthetic batch of the named clip shape on the GPU
and returns the step closure + the static part of the JSON line, and a `cpu_baseline` that times the oracle (CPU restatement of the reference
path, kind "port") on a bounded sample of the same workload.  Bench infrastructure: the only place outside tests/ and __graft_entry__.smoke()
that imports oracle/, and only inside the cpu_baseline functions."""

from __future__ import annotations

import os
import time
from typing import Any, Callable, Dict

import torch

bf16 = torch.bfloat16
PEAK_BF16_TFLOPS = 2500.0


def _time_block(fn: Callable[[], None], warm: int = 1, timed: int = 1):
    ts = []
    for it in range(warm + timed):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return sum(ts[warm:]) / timed, ts


# ------------------------------------------------------------------------------------------------------------------------------------------
# CogVideoX-2b LoRA (configs[2]): 49 x 480 x 720 -> latents [1, 13, 16, 60, 90], 226 text + 17 550 video tokens, 30 blocks, batch 1 per GPU
# ------------------------------------------------------------------------------------------------------------------------------------------
def build_cogvideox(args, par, dev) -> Dict[str, Any]:
    from finetrainers_amd.cogvideox import CogVideoXTransformerConfig, MI355XCogVideoXSFTStep, MI355XCogVideoXTransformer3DModel

    layers = args.layers if args.layers > 0 else 30
    cfg = CogVideoXTransformerConfig(num_layers=layers)
    model = MI355XCogVideoXTransformer3DModel(cfg, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    D = cfg.inner_dim

    def rnd(shape, fan_in):
        return (torch.randn(shape, generator=g, device=dev) / fan_in ** 0.5).to(bf16)

    def one(k, shp):
        if len(shp) == 2:
            return rnd(shp, shp[1])
        return torch.ones(shp, device=dev, dtype=bf16) if "norm" in k and k.endswith("weight") else 0.02 * rnd(shp, 1)

    sd = {k: one(k, getattr(model, name).shape) for k, name in model._KEYS.items()}
    sd["patch_embed.proj.weight"] = rnd((D, cfg.in_channels, 2, 2), 64)
    for i, blk in enumerate(model.transformer_blocks):
        for k, name in blk._KEYS.items():
            sd[f"transformer_blocks.{i}.{k}"] = one(k, getattr(blk, name).shape)
    model.load_diffusers_state_dict(sd)
    del sd
    model.add_adapter(r=args.rank, lora_alpha=float(args.rank))
    ckpt = bool(getattr(args, "gradient_checkpointing", False))
    if ckpt:
        model.apply_activation_checkpointing("full")
    with torch.no_grad():
        n = model.lora_flat.numel() // 2
        model.lora_flat[n:].normal_(0, 0.01, generator=g)  # B != 0 so every gradient path carries data
    step = MI355XCogVideoXSFTStep(model, lr=5e-5, betas=(0.9, 0.99), generator=torch.Generator(device=dev).manual_seed(1 + par.rank),
                                  parallel=par if par.world_size > 1 else None)
    g.manual_seed(100 + par.rank)  # every rank its own clip
    lat = torch.randn((1, 13, 16, 60, 90), generator=g, device=dev).to(bf16)
    text = torch.randn((1, 226, 4096), generator=g, device=dev).to(bf16)
    N = 226 + 17550
    # linears forward + dgrad, attention forward + 2.5 x backward (LoRA / embed / head terms omitted); checkpointing: the forward again without the second
    # feed-forward GEMM (8 of the 12 D x D units)
    flop = layers * (2.0 * N * D * D * (12 * 2 + (8 if ckpt else 0)) + 4.0 * N * N * D * (4.5 if ckpt else 3.5))
    return {
        "gradient_checkpointing": ckpt,
        "workspace_bytes": int(_cog_training_workspace(model, 1, N)),
        "one_step": lambda: step.step(lat, text),
        "samples_per_step": 1,
        "step_tflop": flop / 1e12,
        "metric": "train samples/sec (+ step ms) CogVideoX-2b LoRA 49x480x720 (BASELINE configs[2])",
        "data": "synthetic latents [1,13,16,60,90] + random text embeds [1,226,4096], random-init weights of the CogVideoX-2b DiT",
        "config": {"workload": f"CogVideoX-2b LoRA rank={args.rank} bf16 SFT step, 49x480x720 clip (226 text + 17550 video tokens), batch 1 per GPU, {layers} blocks (BASELINE configs[2])"
                               + ("" if layers == 30 else " -- REDUCED depth"),
                   "model": "CogVideoX-2b DiT: 30 blocks, width 1920, 30 x 64 heads, joint text + video attention", "seq_len": N,
                   "activation_checkpointing": ckpt, "orchestration": "C block stack (ftmi_cog_blocks_forward / _backward)"},
        "layers": layers,
    }


def cpu_baseline_cogvideox(args, layers: int) -> Dict[str, Any]:
    from oracle import cogvideox as cvx

    ocfg = cvx.CogVideoXConfig(num_layers=1)
    oblk = cvx.build_model(ocfg, seed=0, rank=args.rank, alpha=float(args.rank), lora_b_std=0.02).transformer_blocks[0]
    D = ocfg.inner_dim
    g = torch.Generator().manual_seed(0)
    vid, txt, temb = torch.randn(1, 17550, D, generator=g).to(bf16), torch.randn(1, 226, D, generator=g).to(bf16), torch.randn(1, 512, generator=g).to(bf16)

    def fb():
        for p_ in oblk.parameters():
            p_.grad = None
        vr, tr_ = vid.clone().requires_grad_(True), txt.clone().requires_grad_(True)
        hv, ht = oblk(vr, tr_, temb)
        torch.autograd.backward([hv, ht], [torch.ones_like(hv), torch.ones_like(ht)])

    per_block, ts = _time_block(fb)
    return {"value": 1.0 / (per_block * layers), "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle CogVideoXBlock forward + backward at the full 17776 tokens, 1 warm-up ({ts[0]:.1f} s) + 1 timed = {per_block:.1f} s, scaled x{layers} blocks "
                      f"(embed / head / optimiser are < 2 % of the step)"}


# ------------------------------------------------------------------------------------------------------------------------------------------
# Wan2.1-T2V-1.3B full fine-tune (configs[3]): 81 x 512 x 512 -> latents [1, 16, 21, 64, 64], 21 504 video + 512 text tokens, 30 blocks;
# N GPUs: parameters sharded per unit (the reference's FSDP-2 data flow), every rank its own clip
# ------------------------------------------------------------------------------------------------------------------------------------------
def build_wan(args, par, dev) -> Dict[str, Any]:
    from finetrainers_amd.wan import MI355XWanFullFinetuneStep, MI355XWanTransformer3DModel, WanTransformerConfig

    layers = args.layers if args.layers > 0 else 30
    cfg = WanTransformerConfig(num_layers=layers)
    model = MI355XWanTransformer3DModel(cfg, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    D = cfg.inner_dim
    with torch.no_grad():
        for name, v in model.state_dict_views().items():
            if name.endswith("weight") and v.dim() >= 2:
                v.copy_((torch.randn(v.shape, generator=g, device=dev) / v.shape[-1] ** 0.5).to(bf16))
            elif "norm" in name and name.endswith("weight"):
                v.fill_(1.0)
            elif "scale_shift_table" in name:
                v.copy_((torch.randn(v.shape, generator=g, device=dev) / D ** 0.5).to(bf16))
            else:
                v.copy_((0.02 * torch.randn(v.shape, generator=g, device=dev)).to(bf16))
    step = MI355XWanFullFinetuneStep(model, lr=1e-5, betas=(0.9, 0.95), weight_decay=1e-4, generator=torch.Generator(device=dev).manual_seed(1 + par.rank),
                                     parallel=par if par.world_size > 1 else None)
    g.manual_seed(100 + par.rank)
    B, C, F_, H, W, T = 1, 16, 21, 64, 64, 512
    moments = torch.randn((B, 2 * C, F_, H, W), generator=g, device=dev).to(bf16)
    moments[:, C:] = (moments[:, C:].float() * 0.3 - 2.0).to(bf16)
    text = torch.randn((B, T, cfg.text_dim), generator=g, device=dev).to(bf16)
    mean, std = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    sig = torch.tensor([0.6], device=dev)
    S, Fd = 21 * 32 * 32, cfg.ffn_dim
    lin = 2.0 * S * (6 * D * D + 2 * D * Fd) + 2.0 * T * 2 * D * D  # per block, forward: q|k|v, out, cross q, cross out, feed-forward; text k|v
    att = 4.0 * S * S * D + 4.0 * S * T * D                          # self + cross attention, forward
    flop = layers * (3.0 * lin + 3.5 * att)                          # linears: forward + input gradient + weight gradient; attention backward = 2.5 x forward
    W_ = par.world_size
    return {
        "one_step": lambda: step.step(moments, text, mean, std, sig),
        "samples_per_step": 1,
        "step_tflop": flop / 1e12,
        "metric": "train samples/sec (+ step ms) Wan-T2V-1.3B full fine-tune 81x512x512 (BASELINE configs[3])",
        "data": "synthetic posterior moments [1,32,21,64,64] + random text embeds [1,512,4096], random-init weights of the Wan2.1-T2V-1.3B DiT",
        "config": {"workload": f"Wan-T2V-1.3B full fine-tune bf16 step, 81x512x512 clip ({S} video + {T} text tokens), batch 1 per GPU, {layers} blocks (BASELINE configs[3])"
                               + ("" if layers == 30 else " -- REDUCED depth"),
                   "model": "Wan2.1-T2V-1.3B DiT: 30 blocks, width 1536, 12 x 128 heads, 1.42 B trainable bf16 parameters", "seq_len": S,
                   "parallelism_note": f"fsdp{W_}: parameters sharded per unit (bf16 all-gather / fp32 reduce-scatter)" if W_ > 1 else "one GPU: whole shards, no collective",
                   "activation_checkpointing": False, "orchestration": ("one C call per block and direction (ftmi_wan_block_forward / _backward)" if os.environ.get("FTMI_NATIVE_BLOCKS", "1") != "0" else "python, per kernel over the C ABI")},
        "layers": layers,
    }


def cpu_baseline_wan(args, layers: int) -> Dict[str, Any]:
    from oracle import wan

    ocfg = wan.WanConfig(num_layers=1)
    oblk = wan.WanTransformerBlock(ocfg).to(bf16)
    D, S, T = ocfg.num_attention_heads * ocfg.attention_head_dim, 21504, 512
    g = torch.Generator().manual_seed(0)
    xv, ev, tv = torch.randn(1, S, D, generator=g).to(bf16), torch.randn(1, T, D, generator=g).to(bf16), torch.randn(1, 6, D, generator=g).to(bf16)
    ang = torch.rand(S, 64, generator=g, dtype=torch.float64) * 6.283
    freqs = torch.polar(torch.ones_like(ang), ang).view(1, 1, S, 64)

    def fb():
        for p_ in oblk.parameters():
            p_.grad = None
        xr = xv.clone().requires_grad_(True)
        oblk(xr, ev, tv, freqs).backward(torch.ones_like(xv))

    per_block, ts = _time_block(fb)
    return {"value": 1.0 / (per_block * layers), "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle WanTransformerBlock forward + backward (every parameter gradient) at the full {S} + {T} tokens, 1 warm-up ({ts[0]:.1f} s) + 1 timed = "
                      f"{per_block:.1f} s, scaled x{layers} blocks"}


# ------------------------------------------------------------------------------------------------------------------------------------------
# Wan2.1-T2V-1.3B LoRA (the reference's Wan SFT recipes, examples/training/sft/wan/*/train.sh): rank 32 on to_q / to_k / to_v / to_out.0 of both
# attentions, 49 x 480 x 832 -> latents [1, 16, 13, 60, 104], 20 280 video + 512 text tokens, 30 blocks, batch 1 per GPU, frozen base.
# bench.py's --workload list is fixed: this row runs through this file's own command line (python tools/bench_workloads.py --workload wan_lora).
# ------------------------------------------------------------------------------------------------------------------------------------------
def build_wan_lora(args, par, dev) -> Dict[str, Any]:
    from finetrainers_amd.wan import MI355XWanLoRAStep, MI355XWanTransformer3DModel, WanTransformerConfig

    layers = args.layers if args.layers > 0 else 30
    cfg = WanTransformerConfig(num_layers=layers)
    model = MI355XWanTransformer3DModel(cfg, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    D = cfg.inner_dim
    with torch.no_grad():
        for name, v in model.state_dict_views().items():
            if name.endswith("weight") and v.dim() >= 2:
                v.copy_((torch.randn(v.shape, generator=g, device=dev) / v.shape[-1] ** 0.5).to(bf16))
            elif "norm" in name and name.endswith("weight"):
                v.fill_(1.0)
            elif "scale_shift_table" in name:
                v.copy_((torch.randn(v.shape, generator=g, device=dev) / D ** 0.5).to(bf16))
            else:
                v.copy_((0.02 * torch.randn(v.shape, generator=g, device=dev)).to(bf16))
    for blk in model.blocks:
        blk.mark_updated()
    ffn = bool(getattr(args, "ffn_adapters", False))  # --ffn-adapters: the ten-adapter set (ffn.net.0.proj and ffn.net.2 as well)
    model.add_adapter(args.rank, float(args.rank), target_modules="blocks.*(to_q|to_k|to_v|to_out.0" + ("|ffn.net.0.proj|ffn.net.2)" if ffn else ")"))
    ckpt = bool(getattr(args, "gradient_checkpointing", False))
    if ckpt:
        model.apply_activation_checkpointing("full")
    with torch.no_grad():
        for blk in model.blocks:
            blk.lora_B[:, :, :args.rank].normal_(0, 0.01, generator=g)  # B != 0 so every gradient path carries data
        for blk in model.blocks if ffn else ():
            for p in (blk.lora_ffn[1], blk.lora_ffn[3]):
                p[:, :args.rank].normal_(0, 0.01, generator=g)
    step = MI355XWanLoRAStep(model, lr=1e-4, generator=torch.Generator(device=dev).manual_seed(1 + par.rank), parallel=par if par.world_size > 1 else None)
    g.manual_seed(100 + par.rank)
    B, C, F_, H, W, T = 1, 16, 13, 60, 104, 512
    moments = torch.randn((B, 2 * C, F_, H, W), generator=g, device=dev).to(bf16)
    moments[:, C:] = (moments[:, C:].float() * 0.3 - 2.0).to(bf16)
    text = torch.randn((B, T, cfg.text_dim), generator=g, device=dev).to(bf16)
    mean, std = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    sig = torch.tensor([0.6], device=dev)
    S, Fd = 13 * 30 * 52, cfg.ffn_dim
    lin = 2.0 * S * (6 * D * D + 2 * D * Fd) + 2.0 * T * 2 * D * D
    att = 4.0 * S * S * D + 4.0 * S * T * D
    flop = layers * ((3.0 if ckpt else 2.0) * lin + (4.5 if ckpt else 3.5) * att)  # linears: forward + input gradient (no weight gradient); checkpointing: one more forward
    return {
        "one_step": lambda: step.step(moments, text, mean, std, sig),
        "samples_per_step": 1,
        "step_tflop": flop / 1e12,
        "metric": "train samples/sec (+ step ms) Wan-T2V-1.3B LoRA 49x480x832 (the reference's Wan SFT recipes)",
        "data": "synthetic posterior moments [1,32,13,60,104] + random text embeds [1,512,4096], random-init weights of the Wan2.1-T2V-1.3B DiT",
        "config": {"workload": f"Wan-T2V-1.3B LoRA rank={args.rank} bf16 SFT step over the frozen base, 49x480x832 clip ({S} video + {T} text tokens), batch 1 per GPU, {layers} blocks"
                               + ("" if layers == 30 else " -- REDUCED depth"),
                   "model": f"Wan2.1-T2V-1.3B DiT: 30 blocks, width 1536, 12 x 128 heads, frozen; {300 if ffn else 240} fp32 adapters", "seq_len": S,
                   "adapters_per_block": 10 if ffn else 8,
                   "activation_checkpointing": ckpt, "orchestration": ("one C call per block and direction (ftmi_wan_lora_ffn_block_forward / _backward)" if os.environ.get("FTMI_NATIVE_BLOCKS", "1") != "0" else "python, per kernel over the C ABI")},
        "layers": layers,
    }


# ------------------------------------------------------------------------------------------------------------------------------------------
# Wan2.1-T2V-1.3B control LoRA (examples/training/control/wan/image_condition/train.sh): rank 128 on the eight attention projections of every block (the
# recipe's target_modules as written selects those), the patch embedding widened to 32 input channels with its full-rank (r = 1536) adapter, `index` frame
# conditioning on frame 0, gradient checkpointing, one 49 x 480 x 832 bucket; the control clip has the latents' 13 frames.
# ------------------------------------------------------------------------------------------------------------------------------------------
def build_wan_control_lora(args, par, dev) -> Dict[str, Any]:
    from finetrainers_amd.wan import MI355XWanControlSpecOps, MI355XWanLoRAStep, MI355XWanTransformer3DModel, WanTransformerConfig

    layers = args.layers if args.layers > 0 else 30
    cfg = WanTransformerConfig(num_layers=layers)
    model = MI355XWanTransformer3DModel(cfg, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    D = cfg.inner_dim
    with torch.no_grad():
        for name, v in model.state_dict_views().items():
            if name.endswith("weight") and v.dim() >= 2:
                v.copy_((torch.randn(v.shape, generator=g, device=dev) / v.shape[-1] ** 0.5).to(bf16))
            elif "norm" in name and name.endswith("weight"):
                v.fill_(1.0)
            elif "scale_shift_table" in name:
                v.copy_((torch.randn(v.shape, generator=g, device=dev) / D ** 0.5).to(bf16))
            else:
                v.copy_((0.02 * torch.randn(v.shape, generator=g, device=dev)).to(bf16))
    for blk in model.blocks:
        blk.mark_updated()
    model.expand_patch_embedding(32)
    rank = args.rank
    model.add_adapter(rank, float(rank), target_modules="(^patch_embedding$)|(blocks.*(to_q|to_k|to_v|to_out.0|ff.net.0.proj|ff.net.2))",
                      rank_pattern={"patch_embedding": D}, alpha_pattern={"patch_embedding": D})
    model.apply_activation_checkpointing("full")
    with torch.no_grad():
        for blk in model.blocks:
            blk.lora_B[:, :, :rank].normal_(0, 0.01, generator=g)  # B != 0 so every gradient path carries data
        model.patch_lora_B.normal_(0, 0.01, generator=g)
    spec = MI355XWanControlSpecOps()
    spec.frame_conditioning_type, spec.frame_conditioning_index = "index", 0
    step = MI355XWanLoRAStep(model, spec=spec, lr=1e-4, generator=torch.Generator(device=dev).manual_seed(1 + par.rank), parallel=par if par.world_size > 1 else None)
    g.manual_seed(100 + par.rank)
    B, C, F_, H, W, T = 1, 16, 13, 60, 104, 512
    moments = torch.randn((B, 2 * C, F_, H, W), generator=g, device=dev).to(bf16)
    control = torch.randn((B, 2 * C, F_, H, W), generator=g, device=dev).to(bf16)
    text = torch.randn((B, T, cfg.text_dim), generator=g, device=dev).to(bf16)
    mean, std = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    sig = torch.tensor([0.6], device=dev)
    S, Fd, Kp = 13 * 30 * 52, cfg.ffn_dim, 128
    lin = 2.0 * S * (6 * D * D + 2 * D * Fd) + 2.0 * T * 2 * D * D
    att = 4.0 * S * S * D + 4.0 * S * T * D
    patch = 2.0 * S * D * 4 * Kp + 3 * 2.0 * D * D * Kp  # forward K = Kp + 2 Kp, backward Kp; the fold and its two gradients
    flop = layers * (3.0 * lin + 4.5 * att) + patch
    return {
        "one_step": lambda: step.step(moments, text, mean, std, sig, control_latents=control),
        "samples_per_step": 1,
        "step_tflop": flop / 1e12,
        "metric": "train samples/sec (+ step ms) Wan-T2V-1.3B control LoRA 49x480x832 (the reference's Wan control recipe)",
        "data": "synthetic posterior moments [1,32,13,60,104] for the clip and for the control clip + random text embeds [1,512,4096], random-init weights of the Wan2.1-T2V-1.3B DiT",
        "config": {"workload": f"Wan-T2V-1.3B control LoRA rank={rank} + full-rank patch-embedding adapter, bf16 step over the frozen base, index conditioning on frame 0, "
                               f"49x480x832 clip ({S} video + {T} text tokens), batch 1 per GPU, {layers} blocks" + ("" if layers == 30 else " -- REDUCED depth"),
                   "model": f"Wan2.1-T2V-1.3B DiT with a 32-channel patch embedding: 30 blocks, width 1536, 12 x 128 heads, frozen; 240 fp32 block adapters + patch_embedding (r = {D})",
                   "seq_len": S, "adapters_per_block": 8, "activation_checkpointing": True,
                   "orchestration": "one C call per block and direction; pack kernel + folded patch adapter at the root"},
        "layers": layers,
    }


# ------------------------------------------------------------------------------------------------------------------------------------------
# Wan2.1-I2V-14B-480P LoRA (examples/training/sft/wan_i2v/3dgs_dissolve/train.sh): the same adapters on the image-to-video model -- width 5120,
# 40 x 128 heads, feed-forward 13824, 40 blocks, 36 input channels, 257 CLIP image tokens in every block's attn2; the recipe's 49 x 480 x 832 bucket
# (20 280 video + 512 text tokens), gradient checkpointing as in the recipe.  --layers N runs fewer blocks; the row states how many ran.
# --last-frame: the first/last-frame model (Wan2.1-FLF2V-14B: pos_embed_seq_len = 514) at the same geometry -- the CLIP tokens of two images, 514 image keys in
# every block's attn2 (ftmi_attn_ctx2w_*), the last frame kept in the conditioning mask.
# ------------------------------------------------------------------------------------------------------------------------------------------
def build_wan_i2v_lora(args, par, dev) -> Dict[str, Any]:
    from finetrainers_amd.wan import MI355XWanLoRAStep, MI355XWanTransformer3DModel, WanTransformerConfig

    layers = args.layers if args.layers > 0 else 40
    last_frame = bool(getattr(args, "last_frame", False))
    cfg = WanTransformerConfig(num_layers=layers, num_attention_heads=40, ffn_dim=13824, in_channels=36, image_dim=1280, pos_embed_seq_len=514 if last_frame else None)
    model = MI355XWanTransformer3DModel(cfg, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    D = cfg.inner_dim
    with torch.no_grad():
        for name, v in model.state_dict_views().items():
            if name.endswith("weight") and v.dim() >= 2:
                v.copy_((torch.randn(v.shape, generator=g, device=dev) / v.shape[-1] ** 0.5).to(bf16))
            elif "norm" in name and name.endswith("weight"):
                v.fill_(1.0)
            elif "scale_shift_table" in name:
                v.copy_((torch.randn(v.shape, generator=g, device=dev) / D ** 0.5).to(bf16))
            else:
                v.copy_((0.02 * torch.randn(v.shape, generator=g, device=dev)).to(bf16))
    for blk in model.blocks:
        blk.mark_updated()
    model.add_adapter(args.rank, float(args.rank))
    model.apply_activation_checkpointing("full")
    with torch.no_grad():
        for p in model.lora_parameters()[1::2]:
            p[:, :, :args.rank].normal_(0, 0.01, generator=g)
    step = MI355XWanLoRAStep(model, lr=1e-4, generator=torch.Generator(device=dev).manual_seed(1 + par.rank), parallel=par if par.world_size > 1 else None)
    g.manual_seed(100 + par.rank)
    B, C, F_, H, W, T, TI = 1, 16, 13, 60, 104, 512, 514 if last_frame else 257
    mom = lambda: torch.cat([torch.randn((B, C, F_, H, W), generator=g, device=dev), 0.3 * torch.randn((B, C, F_, H, W), generator=g, device=dev) - 2.0], dim=1).to(bf16)
    moments, cond = mom(), mom()
    mask = torch.zeros((B, 4, F_, H, W), dtype=bf16, device=dev)
    mask[:, :, 0] = 1  # the first frame is the conditioning image
    if last_frame:
        mask[:, 3, -1] = 1  # ... and the last pixel frame, the last channel of the last latent frame (MI355XWanModelSpecification.condition_mask)
    text = torch.randn((B, T, cfg.text_dim), generator=g, device=dev).to(bf16)
    image = torch.randn((B, TI, cfg.image_dim), generator=g, device=dev).to(bf16)
    mean, std = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    sig = torch.tensor([0.6], device=dev)
    S, Fd = 13 * 30 * 52, cfg.ffn_dim
    lin = 2.0 * S * (6 * D * D + 2 * D * Fd) + 2.0 * (T + TI) * 2 * D * D
    att = 4.0 * S * S * D + 4.0 * S * (T + TI) * D
    flop = layers * (3.0 * lin + 4.5 * att)  # checkpointing: forward twice + input gradients (the image branch's backward is dQ only: counted slightly high)
    return {
        "one_step": lambda: step.step(moments, text, mean, std, sig, latent_condition=cond, latent_condition_mask=mask, encoder_hidden_states_image=image),
        "samples_per_step": 1,
        "step_tflop": flop / 1e12,
        "metric": "train samples/sec (+ step ms) Wan-I2V-14B LoRA 49x480x832 (the reference's wan_i2v SFT recipe)" + (", first/last-frame model" if last_frame else ""),
        "data": f"synthetic posterior moments [1,32,13,60,104] + conditioning moments + {'first/last' if last_frame else 'first'}-frame mask + random text [1,512,4096] and image [1,{TI},1280] embeds, random-init weights",
        "config": {"workload": f"Wan-{'FLF2V' if last_frame else 'I2V'}-14B LoRA rank={args.rank} bf16 SFT step over the frozen base, 49x480x832 clip ({S} video + {T} text + {TI} image tokens), batch 1 per GPU, "
                               f"{layers} blocks" + ("" if layers == 40 else " -- REDUCED depth"),
                   "model": "Wan2.1-I2V-14B DiT geometry: width 5120, 40 x 128 heads, feed-forward 13824, frozen; 8 fp32 adapters per block", "seq_len": S,
                   "activation_checkpointing": True, "orchestration": ("one C call per block and direction (ftmi_wan_lora_ffn_block_forward / _backward)" if os.environ.get("FTMI_NATIVE_BLOCKS", "1") != "0" else "python, per kernel over the C ABI")},
        "layers": layers,
    }


# ------------------------------------------------------------------------------------------------------------------------------------------
# HunyuanVideo LoRA, fp8 weight storage (configs[4]): 61 x 544 x 960 -> latents [1, 16, 16, 68, 120], 32 640 video + 256 text tokens,
# 20 dual-stream + 40 single-stream blocks (12.8 B parameters), batch 1 per GPU
# ------------------------------------------------------------------------------------------------------------------------------------------
HY_RECIPE_TARGET = "(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|add_q_proj|add_k_proj|add_v_proj|to_add_out)"


def _random_hunyuan(nd: int, ns: int, rank: int, dev, text_adapters: bool = False):
    """Random-init weights of the DiT rounded to fp8-representable values and stored as fp8 bytes (layerwise casting), with rank-``rank`` adapters whose B is
    non-zero -> (model, the generator that drew them).  ``text_adapters``: the shipped recipe's target_modules (eight adapters per dual-stream block)."""
    from finetrainers_amd import ops
    from finetrainers_amd.hunyuan_video import HunyuanVideoTransformerConfig, MI355XHunyuanVideoTransformer3DModel

    cfg = HunyuanVideoTransformerConfig(num_layers=nd, num_single_layers=ns)
    model = MI355XHunyuanVideoTransformer3DModel(cfg, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        def init(t, unit_scale):
            if t.dim() == 2:
                t.copy_((torch.randn(t.shape, generator=g, device=dev) / t.shape[1] ** 0.5).to(bf16))
            elif unit_scale:
                t.fill_(1.0)
            else:
                t.copy_((0.02 * torch.randn(t.shape, generator=g, device=dev)).to(bf16))

        for name, t in model.p.items():
            init(t, name.endswith("weight") and t.dim() == 1)  # the refiner's LayerNorm weights
        model.proj_out_w_t = ops.transpose_bf16(model.p["proj_out.weight"])
        for blk in list(model.transformer_blocks) + list(model.single_transformer_blocks):
            for name, buf in blk.named_buffers():
                if buf is not None and not name.endswith("_t") and name not in ("ones", "zeros"):
                    init(buf, name.startswith("norm_") and buf.dim() == 1)  # q / k RMSNorm weights
            for name in getattr(blk, "_TRANSPOSED", ("wq", "wk", "wv", "proj_mlp_w", "proj_out_w")):
                setattr(blk, name + "_t", ops.transpose_bf16(getattr(blk, name)))
    model.apply_layerwise_casting()
    if text_adapters:
        model.add_adapter(r=rank, lora_alpha=float(rank), target_modules=HY_RECIPE_TARGET)
    else:
        model.add_adapter(r=rank, lora_alpha=float(rank))
    with torch.no_grad():
        for p in model.lora_parameters()[1::2]:
            p.normal_(0, 0.01, generator=g)  # B != 0 so every gradient path carries data
    return model, g


def build_hunyuan(args, par, dev) -> Dict[str, Any]:
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoSFTStep

    nd, ns = (20, 40) if args.layers <= 0 else (max(1, args.layers // 3), max(1, args.layers - args.layers // 3))
    text_adapters = bool(getattr(args, "text_adapters", False))
    model, g = _random_hunyuan(nd, ns, args.rank, dev, text_adapters)
    cfg = model.config
    ckpt = bool(getattr(args, "gradient_checkpointing", False))
    if ckpt:
        model.apply_activation_checkpointing("full")
    step = MI355XHunyuanVideoSFTStep(model, lr=2e-5, guidance=1.0, generator=torch.Generator(device=dev).manual_seed(1 + par.rank),
                                     parallel=par if par.world_size > 1 else None)
    g.manual_seed(100 + par.rank)
    B, C, F_, H, W, T = 1, 16, 16, 68, 120, 256
    lat = torch.randn((B, C, F_, H, W), generator=g, device=dev).to(bf16)
    mask = torch.ones(B, T, dtype=torch.long, device=dev)
    mask[:, 200:] = 0
    cond = {"encoder_hidden_states": torch.randn((B, T, cfg.text_embed_dim), generator=g, device=dev).to(bf16), "encoder_attention_mask": mask,
            "pooled_projections": torch.randn((B, cfg.pooled_projection_dim), generator=g, device=dev).to(bf16)}
    sig = torch.tensor([0.6], device=dev)
    S, D = 16 * 34 * 60, cfg.inner_dim
    N = S + T
    mlp = int(D * cfg.mlp_ratio)
    dual = 2.0 * S * (4 * D * D + 2 * D * mlp) * 2 + 2.0 * T * (4 * D * D + 2 * D * mlp) * 2 + 4.0 * N * N * D * 3.5
    single = 2.0 * N * (3 * D * D + D * mlp + (D + mlp) * D) * 2 + 4.0 * N * N * D * 3.5
    flop = nd * dual + ns * single  # linears forward + input gradient, attention forward + 2.5 x backward (LoRA / front / head terms omitted)
    full = (nd, ns) == (20, 40)
    return {
        "one_step": lambda: step.step(lat, cond, sig),
        "samples_per_step": 1,
        "step_tflop": flop / 1e12,
        "metric": "train samples/sec (+ step ms) HunyuanVideo LoRA fp8-weight-storage 61x544x960 (BASELINE configs[4])",
        "data": "synthetic latents [1,16,16,68,120] + random text embeds [1,256,4096] (200 real tokens) + pooled [1,768], random-init weights of the HunyuanVideo DiT rounded to "
                "fp8-representable values (layerwise casting)",
        "config": {"workload": f"HunyuanVideo LoRA rank={args.rank} SFT step, fp8 weight storage / bf16 compute, 61x544x960 clip ({S} video + {T} text tokens), batch 1 per GPU, "
                               f"{nd} dual-stream + {ns} single-stream blocks (BASELINE configs[4])" + ("" if full else " -- REDUCED depth"),
                   "model": "HunyuanVideo DiT: 20 dual + 40 single blocks, width 3072, 24 x 128 heads, 12.8 B frozen parameters", "seq_len": N,
                   "activation_checkpointing": ckpt, "adapters": 8 * nd + 3 * ns if text_adapters else 4 * nd + 3 * ns, "text_stream_adapters": text_adapters,
                   "weight_storage": "float8_e4m3fn bytes in HBM, per-block up-cast into a shared bf16 arena",
                   "orchestration": ("one C call per block and direction (ftmi_hy_single_* / ftmi_hy_dual_*)" if os.environ.get("FTMI_NATIVE_BLOCKS", "1") != "0" else "python, per kernel over the C ABI")},
        "layers": nd + ns,
        "dual_single": (nd, ns, dual, single),
    }


def cpu_baseline_hunyuan(args, ctx) -> Dict[str, Any]:
    from oracle import hunyuan as hy
    from oracle import ltx

    nd, ns, dual, single = ctx["dual_single"]
    cfg = hy.HunyuanVideoConfig(num_layers=0, num_single_layers=1, num_refiner_layers=1)
    torch.manual_seed(0)
    oblk = hy.SingleStreamBlock(cfg).to(bf16)
    for p in oblk.parameters():
        p.requires_grad_(False)
    for t in ("to_q", "to_k", "to_v"):
        setattr(oblk.attn, t, ltx.LoraLinear(getattr(oblk.attn, t), args.rank, float(args.rank)))
    D, S, T = cfg.inner_dim, 32640, 256
    g = torch.Generator().manual_seed(0)
    video, text, temb = torch.randn(1, S, D, generator=g).to(bf16), torch.randn(1, T, D, generator=g).to(bf16), torch.randn(1, D, generator=g).to(bf16)
    ang = torch.rand(S, 64, generator=g) * 6.283
    rope = (ang.cos().repeat_interleave(2, dim=1).float().contiguous(), ang.sin().repeat_interleave(2, dim=1).float().contiguous())

    def fb():
        for p_ in oblk.parameters():
            p_.grad = None
        vr, tr_ = video.clone().requires_grad_(True), text.clone().requires_grad_(True)
        hv, ht = oblk(vr, tr_, temb, None, rope)
        torch.autograd.backward([hv, ht], [torch.ones_like(hv), torch.ones_like(ht)])

    per_single, ts = _time_block(fb, warm=0, timed=1)  # ~70 TFLOP per pass: one un-warmed pass keeps the sample inside the baseline's time budget
    per_step = ns * per_single + nd * per_single * (dual / single)
    return {"value": 1.0 / per_step, "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle single-stream block forward + backward at the full {S} + {T} tokens, 1 un-warmed pass = {per_single:.1f} s; step = {ns} single blocks + {nd} dual-stream "
                      f"blocks priced at {dual / single:.2f} x a single block (their algorithmic FLOP ratio) = {per_step:.0f} s per sample-step"}


# ------------------------------------------------------------------------------------------------------------------------------------------
# Wan2.1-T2V-1.3B validation sampling in latent space (finetrainers_amd/wan/sampler.py): 49 x 480 x 832 -> latents 13 x 60 x 104 = 20 280 tokens, unconditional +
# conditional rows (guidance 5), random weights with rank-`--rank` adapters.  One "step" of this workload is one ftmi_wan_sample call of `SAMPLE_STEPS`
# denoising steps; the report adds the same loop composed in Python (model.forward + ops.wan_sample_step) and the step kernel on its own.
# `--scheduler unipc`: the checkpoint's UniPCMultistepScheduler at flow_shift 3 (ftmi_wan_sample_ms, ops.wan_sample_step_unipc) instead of flow-match Euler.
# ------------------------------------------------------------------------------------------------------------------------------------------
SAMPLE_STEPS = 4


def build_wan_sample(args, par, dev) -> Dict[str, Any]:
    from finetrainers_amd import ops
    from finetrainers_amd.wan import MI355XWanLatentSampler, MI355XWanTransformer3DModel, WanTransformerConfig

    layers = args.layers if args.layers > 0 else 30
    cfg = WanTransformerConfig(num_layers=layers)
    model = MI355XWanTransformer3DModel(cfg, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    D = cfg.inner_dim
    with torch.no_grad():
        for name, v in model.state_dict_views().items():
            if name.endswith("weight") and v.dim() >= 2:
                v.copy_((torch.randn(v.shape, generator=g, device=dev) / v.shape[-1] ** 0.5).to(bf16))
            elif "norm" in name and name.endswith("weight"):
                v.fill_(1.0)
            elif "scale_shift_table" in name:
                v.copy_((torch.randn(v.shape, generator=g, device=dev) / D ** 0.5).to(bf16))
            else:
                v.copy_((0.02 * torch.randn(v.shape, generator=g, device=dev)).to(bf16))
    for blk in model.blocks:
        blk.mark_updated()
    model.add_adapter(args.rank, float(args.rank))
    with torch.no_grad():
        for blk in model.blocks:
            blk.lora_B[:, :, :args.rank].normal_(0, 0.01, generator=g)
    B, C, F_, H, W, T, guidance, n = 1, 16, 13, 60, 104, 512, 5.0, SAMPLE_STEPS
    S = F_ * (H // 2) * (W // 2)
    unipc = getattr(args, "scheduler", "euler") == "unipc"  # the checkpoint's UniPCMultistepScheduler (flow_shift 3.0): ftmi_wan_sample_ms
    sampler = MI355XWanLatentSampler(model, {"_class_name": "UniPCMultistepScheduler", "flow_shift": 3.0} if unipc else None)
    pos, neg = (torch.randn((B, T, cfg.text_dim), generator=g, device=dev).to(bf16) for _ in range(2))
    latents = torch.randn((B, C, F_, H, W), generator=g, device=dev)
    sig, ts = sampler.schedule(n, None, None)
    geo = sampler.geometry(B, F_, H, W, guidance=True)
    enc = sampler.text_rows(pos, neg)
    tproj, shift, scale = sampler.step_tables(ts, 2 * B)
    ccfg, weights, keep = sampler.c_arguments(geo, T, 0, n, guidance)
    ws_bytes = ops.wan_sample_ms_workspace_bytes(ccfg) if unipc else ops.wan_sample_workspace_bytes(ccfg)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rope, sig_dev = model._rope(F_, H, W), sig.float().to(dev)
    coef = sampler.unipc_tables(sig).to(dev) if unipc else None

    def step(i, pred, x, cols, hist):
        """The step launch of denoising step i from Python; ``hist``: [last, m1, m2] of the multistep solver, swapped here as the C loop swaps them."""
        if unipc:
            ops.wan_sample_step_unipc(geo, pred, x, hist[0], hist[1], hist[2], coef[i], sig_dev[i:i + 1], guidance, cols)
            hist[1], hist[2] = hist[2], hist[1]
        else:
            ops.wan_sample_step(geo, pred, x, sig_dev[i:i + 1].expand(B).contiguous(), sig_dev[i + 1:i + 2].expand(B).contiguous(), guidance, cols)

    def one_call():
        x, cols = ops.wan_sample_init(geo, latents)
        if unipc:
            ops.wan_sample_ms(ccfg, weights, cols, x, tproj, shift, scale, enc, None, rope, coef, sig_dev, workspace=ws)
        else:
            ops.wan_sample(ccfg, weights, cols, x, tproj, shift, scale, enc, None, rope, sig_dev, workspace=ws)
        return None

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return sorted(ms)[len(ms) // 2]

    @torch.no_grad()
    def composed():
        x, cols = ops.wan_sample_init(geo, latents)
        hist = [torch.empty_like(x) for _ in range(3)] if unipc else None
        text = torch.cat([neg, pos])
        for i in range(n):
            t = torch.full((2 * B,), float(ts[i]), dtype=torch.float32, device=dev)
            hidden = cols.view(2 * B, F_, H // 2, W // 2, C, 1, 2, 2).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(2 * B, C, F_, H, W)
            out = model(hidden, t, text)[0]
            pred = out.reshape(2 * B, C, F_, 1, H // 2, 2, W // 2, 2).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(2 * B, S, 4 * C).contiguous()
            step(i, pred, x, cols, hist)

    def report(one_call_ms: float) -> Dict[str, Any]:
        peak_one = torch.cuda.max_memory_allocated() / 1e9
        torch.cuda.reset_peak_memory_stats()
        composed()  # warm
        comp_ms = timed(composed, 3)
        peak_comp = torch.cuda.max_memory_allocated() / 1e9
        x, cols = ops.wan_sample_init(geo, latents)
        pred = torch.randn((2 * B, S, 4 * C), generator=g, device=dev).to(bf16)
        hist = [torch.zeros_like(x) for _ in range(3)] if unipc else None
        k = 2 if unipc else 0  # the multistep kernel is timed on a full order-2 row (step 2 of the run): every buffer is read
        reps = 50
        for _ in range(5):
            step(k, pred, x, cols, hist)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            step(k, pred, x, cols, hist)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        # per element of x: read u 2 + c 2 + x 4, write x 4 + 2 x 2; the multistep step reads last, m1, m2 and writes last, m on top: 20 more
        nbytes = B * S * 4 * C * (36 if unipc else 16)
        return {"ms_per_denoising_step_one_call": one_call_ms / n, "ms_per_denoising_step_python_composition": comp_ms / n,
                "peak_memory_gb_one_call": peak_one, "peak_memory_gb_python_composition": peak_comp, "workspace_gb": ws_bytes / 1e9,
                "step_kernel_us": us, "step_kernel_bytes": nbytes, "step_kernel_gbps": nbytes / (us * 1e-6) / 1e9}

    lin = 2.0 * 2 * S * (6 * D * D + 2 * D * cfg.ffn_dim) + 2.0 * 2 * T * 2 * D * D
    att = 4.0 * 2 * S * S * D + 4.0 * 2 * S * T * D
    return {
        "one_step": one_call,
        "report": report,
        "samples_per_step": 1.0 / n,
        "step_tflop": n * layers * (lin + att) / 1e12,
        "metric": f"{'ftmi_wan_sample_ms (UniPC, flow_shift 3)' if unipc else 'ftmi_wan_sample'}: one call of {n} denoising steps, Wan-T2V-1.3B 49x480x832, guidance 5 "
                  "(value: denoising steps per ms are in the report)",
        "data": "random noise [1,16,13,60,104] + random text embeds [1,512,4096] (conditional and unconditional), random-init weights of the Wan2.1-T2V-1.3B DiT",
        "config": {"workload": f"Wan-T2V-1.3B latent sampling, rank={args.rank} adapters, {S} video + {T} text tokens, 2 model rows (unconditional + conditional), {layers} blocks"
                               + ("" if layers == 30 else " -- REDUCED depth"), "seq_len": S, "denoising_steps_per_call": n, "scheduler": "unipc" if unipc else "euler"},
        "layers": layers,
    }


# ------------------------------------------------------------------------------------------------------------------------------------------
# CogVideoX-2b validation sampling in latent space (finetrainers_amd/cogvideox/sampler.py): 49 x 480 x 720 -> latents 13 x 60 x 90 = 17 550 video + 226 text
# tokens, unconditional + conditional rows (guidance 6), random weights with rank-`--rank` adapters (run with --rank 64: the recipe's rank).  One "step" of
# this workload is one ftmi_cog_sample call of `SAMPLE_STEPS` denoising steps; the report interleaves it with the same loop composed in Python (model.forward +
# ops.cog_sample_step, whose workspace keeps every block's activations) and times the step kernel on its own.
# ------------------------------------------------------------------------------------------------------------------------------------------
def _random_cogvideox(cfg, rank: int, dev):
    """Random-init weights of the DiT (the recipe of build_cogvideox) with rank-``rank`` adapters whose B is non-zero; no optimiser state."""
    from finetrainers_amd.cogvideox import MI355XCogVideoXTransformer3DModel

    model = MI355XCogVideoXTransformer3DModel(cfg, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    D = cfg.inner_dim
    rnd = lambda shape, fan_in: (torch.randn(shape, generator=g, device=dev) / fan_in ** 0.5).to(bf16)

    def one(k, shp):
        if len(shp) == 2:
            return rnd(shp, shp[1])
        return torch.ones(shp, device=dev, dtype=bf16) if "norm" in k and k.endswith("weight") else 0.02 * rnd(shp, 1)

    sd = {k: one(k, getattr(model, name).shape) for k, name in model._KEYS.items()}
    sd["patch_embed.proj.weight"] = rnd((D, cfg.in_channels, 2, 2), 64)
    for i, blk in enumerate(model.transformer_blocks):
        for k, name in blk._KEYS.items():
            sd[f"transformer_blocks.{i}.{k}"] = one(k, getattr(blk, name).shape)
    model.load_diffusers_state_dict(sd)
    del sd
    model.add_adapter(r=rank, lora_alpha=float(rank))
    with torch.no_grad():
        n = model.lora_flat.numel() // 2
        model.lora_flat[n:].normal_(0, 0.01, generator=g)
    return model


def build_cog_sample(args, par, dev) -> Dict[str, Any]:
    from finetrainers_amd import ops
    from finetrainers_amd.cogvideox import (COG_DPM_SCHEDULER_CONFIG, CogVideoXTransformerConfig, MI355XCogVideoXLatentSampler, cog_ddim_tables,
                                            cog_dpm_tables)

    dpm = getattr(args, "scheduler", "euler") == "dpm"  # the 5b / 1.5 checkpoints' CogVideoXDPMScheduler: ftmi_cog_sample_ms
    layers = args.layers if args.layers > 0 else 30
    cfg = CogVideoXTransformerConfig(num_layers=layers)
    model = _random_cogvideox(cfg, args.rank, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    B, C, F_, H, W, T, guidance, n = 1, 16, 13, 60, 90, 226, 6.0, SAMPLE_STEPS
    S, Kc, D = F_ * (H // 2) * (W // 2), 4 * C, cfg.inner_dim
    sampler = MI355XCogVideoXLatentSampler(model)
    pos, neg = (torch.randn((B, T, cfg.text_embed_dim), generator=g, device=dev).to(bf16) for _ in range(2))
    noise = torch.randn((B, F_, C, H, W), generator=g, device=dev)
    ts, coef = cog_ddim_tables(n)
    coef = coef.to(dev)
    geo = sampler.geometry(B, F_, H, W, guidance=True)
    text = torch.cat([neg, pos]).contiguous()
    temb, shift, onep = sampler.step_tables(ts, 2 * B)
    ccfg, weights, keep = sampler.c_arguments(geo, n, guidance)
    ws_bytes = ops.cog_sample_ms_workspace_bytes(ccfg) if dpm else ops.cog_sample_workspace_bytes(ccfg)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    if dpm:  # the folded rows of the checkpoints' table and the noise of every step but the last, packed once into the state's layout
        rows = cog_dpm_tables(n, COG_DPM_SCHEDULER_CONFIG, guidance)[1]
        k = max(i + 1 for i in range(n) if float(rows[i, 5]) != 0.0)
        rows = rows.to(dev)
        packed = ops.cog_sample_pack(geo, torch.randn((k, B, F_, C, H, W), generator=g, device=dev))
        old = torch.empty((B, S, Kc), dtype=torch.float32, device=dev)

    def ddim_call():
        x, cols = ops.cog_sample_init(geo, noise)
        ops.cog_sample(ccfg, weights, cols, x, text, temb, shift, onep, coef, workspace=ws)
        return None

    def dpm_call():
        x, cols = ops.cog_sample_init(geo, noise)
        ops.cog_sample_ms(ccfg, weights, cols, x, text, temb, shift, onep, rows, packed, workspace=ws)
        return None

    one_call = dpm_call if dpm else ddim_call

    @torch.no_grad()
    def composed():
        x, cols = ops.cog_sample_init(geo, noise)
        for i in range(n):
            t = torch.full((2 * B,), int(ts[i]), dtype=torch.int64, device=dev)
            hidden = ops.cog_unpatchify(cols.view(2 * B, S, Kc), F_, C, H, W, 2)
            out = model(hidden, text, t)[0]
            if dpm:
                ops.cog_sample_step_dpm(geo, ops.cog_patchify(out, 2), x, old, packed[i] if i < k else None, rows[i], cols)
            else:
                ops.cog_sample_step(geo, ops.cog_patchify(out, 2), x, coef, i, guidance, cols)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def report(one_call_ms: float) -> Dict[str, Any]:
        peak_one = torch.cuda.max_memory_allocated() / 1e9
        torch.cuda.reset_peak_memory_stats()
        composed()  # warm (allocates the training workspace)
        a_ms, b_ms, d_ms = [], [], []
        for _ in range(3):  # interleaved: the paths see the same clocks and the same neighbours
            a_ms.append(once(one_call))
            b_ms.append(once(composed))
            if dpm:  # the DDIM call on the same box, in the same workspace
                d_ms.append(once(ddim_call))
        peak_comp = torch.cuda.max_memory_allocated() / 1e9
        x, cols = ops.cog_sample_init(geo, noise)
        pred = torch.randn((2 * B, S, Kc), generator=g, device=dev).to(bf16)
        reps = 50
        if dpm:  # a full row (step 2: history and noise): per element of x read u 2 + c 2 + x 4 + old 4 + z 4, write x 4 + old 4 + 2 x 2
            step, per = (lambda: ops.cog_sample_step_dpm(geo, pred, x, old, packed[2], rows[2], cols)), 28
        else:  # per element of x: read u 2 + c 2 + x 4, write x 4 + 2 x 2
            step, per = (lambda: ops.cog_sample_step(geo, pred, x, coef, 1, guidance, cols)), 16
        for _ in range(5):
            step()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            step()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        nbytes = B * S * Kc * per
        extra = {"scheduler": "dpm", "ms_per_denoising_step_ddim_one_call": sorted(d_ms)[1] / n, "interleaved_ms_ddim_one_call": d_ms,
                 "step_noise_gb": packed.numel() * 4 / 1e9, "step_kernel_bytes_per_element": per} if dpm else {}
        return {**extra, "ms_per_denoising_step_one_call": sorted(a_ms)[1] / n, "ms_per_denoising_step_python_composition": sorted(b_ms)[1] / n,
                "ms_per_denoising_step_one_call_first_pass": one_call_ms / n, "interleaved_ms_one_call": a_ms, "interleaved_ms_python_composition": b_ms,
                "peak_memory_gb_one_call": peak_one, "peak_memory_gb_python_composition": peak_comp, "workspace_gb": ws_bytes / 1e9,
                "training_workspace_gb": int(_cog_training_workspace(model, 2 * B, T + S)) / 1e9,
                "step_kernel_us": us, "step_kernel_bytes": nbytes, "step_kernel_gbps": nbytes / (us * 1e-6) / 1e9}

    N = T + S
    flop = 2 * layers * (2.0 * N * D * D * 12 + 4.0 * N * N * D)  # two model rows: linears + joint attention, forward only
    return {
        "one_step": one_call,
        "report": report,
        "samples_per_step": 1.0 / n,
        "step_tflop": n * flop / 1e12,
        "metric": f"{'ftmi_cog_sample_ms (DPM)' if dpm else 'ftmi_cog_sample'}: one call of {n} denoising steps, CogVideoX-2b 49x480x720, guidance 6 (value: "
                  "denoising steps per ms are in the report)",
        "data": "random noise [1,13,16,60,90] + random text embeds [1,226,4096] (conditional and unconditional), random-init weights of the CogVideoX-2b DiT",
        "config": {"workload": f"CogVideoX-2b latent sampling, rank={args.rank} adapters, {S} video + {T} text tokens, 2 model rows (unconditional + conditional), {layers} blocks"
                               + ("" if layers == 30 else " -- REDUCED depth"), "seq_len": N, "denoising_steps_per_call": n, "scheduler": "dpm" if dpm else "ddim"},
        "layers": layers,
    }


# ------------------------------------------------------------------------------------------------------------------------------------------
# HunyuanVideo validation sampling in latent space (finetrainers_amd/hunyuan_video/sampler.py) at BASELINE configs[4]'s geometry: 61 x 544 x 960 -> latents
# [1, 16, 16, 68, 120] = 32 640 video + 256 text tokens (200 real), 20 dual-stream + 40 single-stream blocks, fp8 weight storage, random weights with
# rank-`--rank` adapters (run with --rank 64), embedded guidance 6, no true CFG (the pipeline's default).  One "step" of this workload is one ftmi_hy_sample_text
# call of `SAMPLE_STEPS` denoising steps; the report interleaves it with the same loop composed in Python (model.forward under no_grad + ops.hy_sample_step)
# and times the step kernel on its own.
# ------------------------------------------------------------------------------------------------------------------------------------------
def build_hy_sample(args, par, dev) -> Dict[str, Any]:
    from finetrainers_amd import ops
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoLatentSampler, hy_flow_match_sigmas

    nd, ns = (20, 40) if args.layers <= 0 else (max(1, args.layers // 3), max(1, args.layers - args.layers // 3))
    text_adapters = bool(getattr(args, "text_adapters", False))
    model, _ = _random_hunyuan(nd, ns, args.rank, dev, text_adapters)
    cfg = model.config
    g = torch.Generator(device=dev).manual_seed(3)
    B, C, F_, H, W, T, guidance_scale, n = 1, 16, 16, 68, 120, 256, 6.0, SAMPLE_STEPS
    S, Kc, D = F_ * (H // 2) * (W // 2), 4 * C, cfg.inner_dim
    sampler = MI355XHunyuanVideoLatentSampler(model)
    text = torch.randn((B, T, cfg.text_embed_dim), generator=g, device=dev).to(bf16)
    pooled = torch.randn((B, cfg.pooled_projection_dim), generator=g, device=dev).to(bf16)
    mask = torch.ones(B, T, dtype=torch.bool, device=dev)
    mask[:, 200:] = False
    noise = torch.randn((B, C, F_, H, W), generator=g, device=dev)
    sig = hy_flow_match_sigmas(n)
    sig_dev = sig.to(torch.float32).to(dev)
    geo = sampler.geometry(B, F_, H, W, true_cfg=False)
    with torch.no_grad():
        temb, enc, shift, onep = sampler.step_tables(sig, guidance_scale, text, mask, pooled)
    key_bias = sampler.key_bias(mask, geo, T)
    cos, sin = (t.contiguous() for t in model._rope(F_, H, W))
    ccfg, weights, keep = sampler.c_arguments(geo, T, n, 1.0)
    ws_bytes = ops.hy_sample_workspace_bytes(ccfg)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    guidance = torch.full((B,), guidance_scale, dtype=bf16, device=dev) * 1000.0
    ts = sampler.timesteps(sig).tolist()
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated() / 1e9  # the model, the step tables and the planned workspace: what both paths start from
    torch.cuda.reset_peak_memory_stats()  # (building the model peaks above either loop: bf16 weights and their transposes before the fp8 cast)

    def one_call():
        x, cols = ops.hy_sample_init(geo, noise)
        ops.hy_sample(ccfg, weights, cols, x, temb, enc, shift, onep, key_bias, cos, sin, sig_dev, workspace=ws)
        return None

    one_call.keep = keep  # the host arrays the weight structure points into live as long as the call does

    @torch.no_grad()
    def composed():
        x, cols = ops.hy_sample_init(geo, noise)
        for i in range(n):
            hidden = cols.view(B, F_, H // 2, W // 2, C, 1, 2, 2).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(B, C, F_, H, W)
            out = model(hidden, torch.full((B,), ts[i], dtype=torch.float32, device=dev), text, mask, pooled, guidance=guidance)[0]
            pred = out.view(B, C, F_, 1, H // 2, 2, W // 2, 2).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, S, Kc)
            ops.hy_sample_step(geo, pred, x, sig_dev, i, 1.0, cols)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def report(one_call_ms: float) -> Dict[str, Any]:
        peak_one = torch.cuda.max_memory_allocated() / 1e9
        torch.cuda.reset_peak_memory_stats()
        composed()  # warm
        a_ms, b_ms = [], []
        for _ in range(3):  # interleaved: both paths see the same clocks and the same neighbours
            a_ms.append(once(one_call))
            b_ms.append(once(composed))
        peak_comp = torch.cuda.max_memory_allocated() / 1e9
        x, cols = ops.hy_sample_init(geo, noise)
        pred = torch.randn((B, S, Kc), generator=g, device=dev).to(bf16)
        reps = 50
        for _ in range(5):
            ops.hy_sample_step(geo, pred, x, sig_dev, 1, 1.0, cols)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            ops.hy_sample_step(geo, pred, x, sig_dev, 1, 1.0, cols)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        nbytes = B * S * Kc * 10  # per element of x: read pred 2 + x 4, write x 4 + cols 2
        return {"ms_per_denoising_step_one_call": sorted(a_ms)[1] / n, "ms_per_denoising_step_python_composition": sorted(b_ms)[1] / n,
                "ms_per_denoising_step_one_call_first_pass": one_call_ms / n, "interleaved_ms_one_call": a_ms, "interleaved_ms_python_composition": b_ms,
                "peak_memory_gb_one_call": peak_one, "peak_memory_gb_python_composition": peak_comp, "resident_gb_before_either_loop": resident,
                "workspace_gb": ws_bytes / 1e9, "step_kernel_us": us, "step_kernel_bytes": nbytes, "step_kernel_gbps": nbytes / (us * 1e-6) / 1e9}

    N = T + S
    mlp = int(D * cfg.mlp_ratio)
    dual = 2.0 * S * (4 * D * D + 2 * D * mlp) + 2.0 * T * (4 * D * D + 2 * D * mlp) + 4.0 * N * N * D
    single = 2.0 * N * (3 * D * D + D * mlp + (D + mlp) * D) + 4.0 * N * N * D
    full = (nd, ns) == (20, 40)
    return {
        "one_step": one_call,
        "report": report,
        "samples_per_step": 1.0 / n,
        "step_tflop": n * (nd * dual + ns * single) / 1e12,  # linears + joint attention, forward only
        "metric": f"ftmi_hy_sample_text: one call of {n} denoising steps, HunyuanVideo 61x544x960, embedded guidance 6 (value: denoising steps per ms are in the report)",
        "data": "random noise [1,16,16,68,120] + random text embeds [1,256,4096] (200 real tokens) + pooled [1,768], random-init weights of the HunyuanVideo DiT "
                "stored as fp8 bytes",
        "config": {"workload": f"HunyuanVideo latent sampling, rank={args.rank} adapters, fp8 weight storage, {S} video + {T} text tokens, 1 model row, "
                               f"{nd} dual-stream + {ns} single-stream blocks" + ("" if full else " -- REDUCED depth"), "seq_len": N, "denoising_steps_per_call": n,
                   "text_stream_adapters": text_adapters},
        "layers": nd + ns,
    }


def _cog_training_workspace(model, B: int, N: int) -> int:
    import ctypes

    from finetrainers_amd import _lib

    return _lib.load().ftmi_cog_workspace_bytes(ctypes.byref(model._c_config(B, N)))


# ------------------------------------------------------------------------------------------------------------------------------------------
# LTX-Video LoRA at BASELINE config 2 (bench.py's flagship step: 49 x 512 x 768 clip, batch 2, rank 64 -- run with --rank 64), here so that --ffn-adapters can
# select the ten-adapter set (the control trainer's default target_modules): same weights, data and optimiser as bench.py's builder.
# ------------------------------------------------------------------------------------------------------------------------------------------
def build_ltx_lora(args, par, dev) -> Dict[str, Any]:
    import ctypes

    from finetrainers_amd import _lib
    from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoModelSpecification
    from finetrainers_amd.ltx_video.transformer import CONTROL_TARGET_MODULES, DEFAULT_TARGET_MODULES
    from finetrainers_amd.trainer import MI355XSFTStep

    layers = args.layers if args.layers > 0 else 28
    ffn = bool(getattr(args, "ffn_adapters", False))
    ckpt = bool(getattr(args, "gradient_checkpointing", False))
    tcfg = LTXTransformerConfig(num_layers=layers)
    spec = MI355XLTXVideoModelSpecification(transformer_config=tcfg)
    model = spec.load_diffusion_models(device=dev, random_init_seed=0)["transformer"]
    model.add_adapter(r=args.rank, lora_alpha=float(args.rank), target_modules=CONTROL_TARGET_MODULES if ffn else DEFAULT_TARGET_MODULES)
    if ckpt:
        model.enable_gradient_checkpointing()
    with torch.no_grad():  # B != 0 so every gradient path carries data (the [A | B] part holds bench.py's draws)
        g = torch.Generator(device=dev).manual_seed(1)
        model.lora_flat.copy_(torch.randn(model.lora_flat.shape, generator=g, device=dev) * 0.01)
    step = MI355XSFTStep(model, spec, lr=5e-5, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-4, max_grad_norm=1.0,
                         parallel=par if par.world_size > 1 else None, generator=torch.Generator(device=dev).manual_seed(1234 + par.rank))
    B, C, F_, H, W, T = 2, tcfg.in_channels, 7, 16, 24, 128
    gd = torch.Generator(device=dev).manual_seed(100 + par.rank)
    latents = torch.randn((B, C, F_, H, W), generator=gd, device=dev).to(bf16)
    text = torch.randn((B, T, tcfg.caption_channels), generator=gd, device=dev).to(bf16)
    mask = torch.zeros((B, T), dtype=bf16, device=dev)
    for i in range(B):
        mask[i, : (32 if i % 2 == 0 else 96)] = 1
    cond = {"encoder_hidden_states": text, "encoder_attention_mask": mask}
    lat = {"latents": latents, "latents_mean": torch.zeros(C, device=dev), "latents_std": torch.ones(C, device=dev), "num_frames": F_, "height": H, "width": W}
    S, D, Fd = F_ * H * W, tcfg.inner_dim, tcfg.inner_dim * tcfg.ff_mult
    lin = 2.0 * S * (5 * D * D + 2 * D * Fd) + 2.0 * T * 2 * D * D
    att = 4.0 * S * S * D + 4.0 * S * T * D
    flop = B * layers * ((3.0 if ckpt else 2.0) * lin + (4.5 if ckpt else 3.5) * att)  # linears: forward + input gradient (frozen base); checkpointing: one more forward
    cfg = model._c_config(B, S, T, checkpoint=ckpt)
    cos, sin = model.rope_tables(F_, H, W, None)
    w = model._c_weights(cos, sin)
    lib = _lib.load()
    ws = lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(cfg), ctypes.byref(w))
    return {
        "one_step": lambda: step.step(cond, lat),
        "samples_per_step": B,
        "step_tflop": flop / 1e12,
        "metric": "train samples/sec (+ step ms) LTX-Video LoRA 49x512x768 (BASELINE configs[1]), eight or ten adapters per block",
        "data": "synthetic latents [2,128,7,16,24] + random text embeds, random-init weights of the production LTX-Video DiT (bench.py's)",
        "config": {"workload": f"LTX-Video LoRA rank={args.rank} bf16 SFT step, 49x512x768 clip ({S} tokens), batch 2, {layers} blocks" + ("" if layers == 28 else " -- REDUCED depth"),
                   "adapters_per_block": 10 if ffn else 8, "lora_parameters": int(model.lora_flat.numel()), "workspace_bytes": int(ws), "seq_len": S,
                   "activation_checkpointing": ckpt},
        "layers": layers,
    }


WORKLOADS = {"cogvideox": (build_cogvideox, lambda a, c: cpu_baseline_cogvideox(a, c["layers"])),
             "wan": (build_wan, lambda a, c: cpu_baseline_wan(a, c["layers"])),
             "wan_lora": (build_wan_lora, lambda a, c: cpu_baseline_wan(a, c["layers"])),  # (yardstick on the host: the full fine-tune block, an upper bound of the LoRA block's work)
             "wan_control_lora": (build_wan_control_lora, None),  # (no host yardstick; run with --rank 128: the recipe's rank)
             "wan_i2v_lora": (build_wan_i2v_lora, None),  # (no host yardstick: this row runs through this file's own command line only)
             "wan_sample": (build_wan_sample, None),  # (validation sampling: forward only; this file's own command line only)
             "cog_sample": (build_cog_sample, None),  # (validation sampling: forward only; this file's own command line only; --rank 64)
             "hy_sample": (build_hy_sample, None),  # (validation sampling: forward only; this file's own command line only; --rank 64)
             "ltx_lora": (build_ltx_lora, None),  # (bench.py's flagship step with a choice of adapter set; this file's own command line only; --rank 64)
             "hunyuan": (build_hunyuan, cpu_baseline_hunyuan)}


def main() -> None:
    """One workload on one GPU, outside bench.py (whose --workload list is fixed): 1 JSON line with the builder's static part plus step_ms (median), every
    step's ms, samples/s, achieved TFLOP/s and the peak allocated memory.  ``python tools/bench_workloads.py --workload wan_lora --steps 5 --warmup 1
    [--gradient-checkpointing] [--ffn-adapters] [--text-adapters]``."""
    import argparse
    import json
    import sys
    import types

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="wan_lora")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--gradient-checkpointing", dest="gradient_checkpointing", action="store_true")
    ap.add_argument("--ffn-adapters", dest="ffn_adapters", action="store_true", help="wan_lora / ltx_lora: adapters on the two feed-forward projections as well (ten per block)")
    ap.add_argument("--text-adapters", dest="text_adapters", action="store_true",
                    help="hunyuan / hy_sample: the shipped recipe's target_modules -- adapters on add_q_proj / add_k_proj / add_v_proj / to_add_out of the dual-stream blocks too")
    ap.add_argument("--scheduler", choices=("euler", "unipc", "dpm"), default="euler",
                    help="wan_sample: flow-match Euler at shift 1 (ftmi_wan_sample) or the checkpoint's UniPC multistep scheduler at flow_shift 3 (ftmi_wan_sample_ms); "
                         "cog_sample: dpm = the 5b / 1.5 checkpoints' CogVideoXDPMScheduler (ftmi_cog_sample_ms) instead of DDIM (the default)")
    ap.add_argument("--last-frame", dest="last_frame", action="store_true",
                    help="wan_i2v_lora: the first/last-frame model (pos_embed_seq_len = 514: two images, 514 image keys in attn2) at the same geometry")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = WORKLOADS[args.workload][0](args, types.SimpleNamespace(world_size=1, rank=0), dev)
    one_step = ctx.pop("one_step")
    ms = []
    for it in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = one_step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    timed = sorted(ms[args.warmup:])
    med = timed[len(timed) // 2]
    ctx.pop("dual_single", None)
    report = ctx.pop("report", None)  # a forward-only workload (wan_sample) reports its own figures instead of loss and gradient norm
    ctx.update(step_ms=med, steps_ms=ms, value=ctx["samples_per_step"] / (med / 1e3), unit="samples/s", achieved_tflops=ctx["step_tflop"] / (med / 1e3),
               peak_memory_gb=torch.cuda.max_memory_allocated() / 1e9, gpus=1, steps=args.steps, warmup=args.warmup)
    ctx.update(report(med) if report else dict(loss=float(out["loss"]), grad_norm=float(out["grad_norm"])))
    print(json.dumps(ctx))


if __name__ == "__main__":
    main()
