"""Result latents of the HunyuanVideo one-call sampler over seeded cases, to compare two checkouts of the library bit for bit: the sibling of
tools/ltx_digest.py (same command line, same acceptance rule; copy both files into the older checkout's tools/ and run this one there).

Cases: the smallest geometry of tests/test_gpu_hy_sampling.py's loop tests -- 2 dual + 1 single block, width 256, (F, H, W) = (3, 8, 12): 72 video + 8 text
tokens, B = 2, a ragged text mask, 2 steps, true CFG 3 -- once with the video stream's adapters alone and once with the dual blocks' text-stream adapters as
well (rank 64, seeded non-zero B)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ltx_digest import run  # noqa: E402

bf16 = torch.bfloat16
SMALL = dict(num_attention_heads=2, attention_head_dim=128, num_refiner_layers=1, text_embed_dim=64, pooled_projection_dim=64)
TEXT_RECIPE = "(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|add_q_proj|add_k_proj|add_v_proj|to_add_out)"
GRID, T, N_STEPS, C, B = (3, 8, 12), 8, 2, 16, 2


def _diffusers_key(k):
    """oracle/hunyuan.py module names -> diffusers HunyuanVideoTransformer3DModel parameter names."""
    k = k.replace("context_embedder.refiner_blocks.", "context_embedder.token_refiner.refiner_blocks.").replace(".norm_out_linear.", ".norm_out.linear.")
    if k.startswith("norm_out_linear."):
        k = "norm_out.linear." + k[len("norm_out_linear."):]
    if k.startswith("x_embedder."):
        k = "x_embedder.proj." + k[len("x_embedder."):]
    for a in ("ff_context", "ff"):
        k = k.replace(f"{a}.proj_in.", f"{a}.net.0.proj.").replace(f"{a}.proj_out.", f"{a}.net.2.")
    return k


def _sample(target, dev):
    from finetrainers_amd.hunyuan_video import HunyuanVideoTransformerConfig, MI355XHunyuanVideoLatentSampler, MI355XHunyuanVideoTransformer3DModel
    from oracle import hunyuan as hy

    omodel = hy.build_model(hy.HunyuanVideoConfig(num_layers=2, num_single_layers=1, **SMALL), seed=0, dtype=torch.float32).to(bf16)
    model = MI355XHunyuanVideoTransformer3DModel(HunyuanVideoTransformerConfig(num_layers=2, num_single_layers=1, **SMALL), device=dev)
    model.load_diffusers_state_dict({_diffusers_key(k): v for k, v in omodel.state_dict().items()})
    model.add_adapter(r=64, lora_alpha=64.0, target_modules=target)
    g = torch.Generator(device=dev).manual_seed(7)
    with torch.no_grad():
        for blk in list(model.transformer_blocks) + list(model.single_transformer_blocks):
            blk.lora_B.copy_(torch.randn(blk.lora_B.shape, generator=g, device=dev) * 0.02)
    g = torch.Generator().manual_seed(11)
    F_, H, W = GRID
    noise = torch.randn(B, C, F_, H, W, generator=g)
    text, pooled = torch.randn(B, T, 64, generator=g).to(bf16), torch.randn(B, 64, generator=g).to(bf16)
    neg, neg_pooled = torch.randn(B, T, 64, generator=g).to(bf16), torch.randn(B, 64, generator=g).to(bf16)
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[0, 5:] = False
    out = MI355XHunyuanVideoLatentSampler(model).sample(noise, text, mask, pooled, negative_prompt_embeds=neg, negative_prompt_attention_mask=torch.ones(B, T, dtype=torch.bool),
                                                        negative_pooled_prompt_embeds=neg_pooled, num_inference_steps=N_STEPS, true_cfg_scale=3.0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    return out.detach().cpu().clone()


def collect():
    dev = torch.device("cuda", 0)
    return {"hy.video/latents": _sample(None, dev), "hy.text/latents": _sample(TEXT_RECIPE, dev)}


if __name__ == "__main__":
    run(collect)
