"""Torch restatement of CogVideoX latent sampling for the tests: the operand layout of csrc/sample_layout.hip, the step in fp64, the pipeline loop the GPU
trajectory test drives ``oracle.cogvideox.CogVideoXTransformer3DModel`` with, and the oracle / MI355X model pairs.

[upstream, unpinned] ``CogVideoXPipeline`` + ``CogVideoXDDIMScheduler`` (diffusers 0.33, neither is vendored): trailing timesteps, v-prediction, eta = 0,
``noise_pred = uncond + g (text - uncond)`` with the unconditional rows first; the scheduler step is written out literally here (``ddim_step``), NOT through
the folded (cx, cv) table of finetrainers_amd/cogvideox/sampler.py, so the two check each other."""
import copy

import torch

bf16 = torch.bfloat16
# 2b width (the GEMM tiles and the 30-head attention of BASELINE config 3), small everything else
SMALL = dict(sample_width=12, sample_height=8, sample_frames=9, max_text_seq_length=16)


# ---- layout ------------------------------------------------------------------------------------------------------------------------------------------------
def patchify(lat, p=2, pt=1):
    """[B, F, C, H, W] -> [B, (F/pt)(H/p)(W/p), C pt p p], columns (c, pt, ph, pw): CogVideoXPatchEmbed's operand and proj_out's output."""
    B, F_, C, H, W = lat.shape
    x = lat.reshape(B, F_ // pt, pt, C, H // p, p, W // p, p).permute(0, 1, 4, 6, 3, 2, 5, 7)
    return x.reshape(B, (F_ // pt) * (H // p) * (W // p), C * pt * p * p).contiguous()


def unpatchify(tokens, F_, C, H, W, p=2, pt=1):
    B = tokens.shape[0]
    x = tokens.reshape(B, F_ // pt, H // p, W // p, C, pt, p, p).permute(0, 1, 5, 4, 2, 6, 3, 7)
    return x.reshape(B, F_, C, H, W).contiguous()


def init_ref(lat, p=2, pt=1, P=2):
    """-> (x fp32 [B, S, Kc], cols bf16 [P B S, Kc])."""
    x = patchify(lat.float(), p, pt)
    return x, x.reshape(-1, x.shape[-1]).to(bf16).repeat(P, 1)


def step_ref(pred, x, cx, cv, g):
    """fp64: pred bf16 [P B, S, Kc] (P = 2 unless g == 1), x fp32 [B, S, Kc] -> cx x + cv (u + g (c - u))."""
    B = x.shape[0]
    pr = pred.double()
    v = pr if g == 1.0 else pr[:B] + g * (pr[B:] - pr[:B])
    return cx * x.double() + cv * v


def finish_ref(x, k, F_, C, H, W, p=2, pt=1, drop=0):
    """fp64 [B, F - drop, C, H, W] = x k without the first ``drop`` frames."""
    return unpatchify(x.double() * k, F_, C, H, W, p, pt)[:, drop:]


# ---- the scheduler, literally -----------------------------------------------------------------------------------------------------------------------------
def ddim_schedule(n, alphas_cumprod, N=1000):
    """-> [(t, alpha_bar_t, alpha_bar_prev)] fp64 for trailing spacing and set_alpha_to_one."""
    ac = alphas_cumprod.double()
    out = []
    for i in range(n):
        t = int(round(N - i * N / n)) - 1
        prev = t - N // n
        out.append((t, float(ac[t]), float(ac[prev]) if prev >= 0 else 1.0))
    return out


def ddim_step(x, v, a_t, a_prev):
    """CogVideoXDDIMScheduler.step, v-prediction, eta = 0, as upstream writes it."""
    x0 = a_t ** 0.5 * x - (1 - a_t) ** 0.5 * v
    a = ((1 - a_prev) / (1 - a_t)) ** 0.5
    b = a_prev ** 0.5 - a_t ** 0.5 * a
    return a * x + b * x0


def trajectory(fn, dtype, latents, text, negative_text, schedule, guidance, round_state=True, rope=None):
    """The pipeline's loop over ``fn(hidden_states, encoder_hidden_states, timestep, image_rotary_emb, return_dict)`` -> latents [B, F, C, H, W] in ``dtype``.
    The model runs in ``dtype`` on [x; x] (unconditional rows first); the combine runs on its outputs in ``dtype``; the step runs in fp32 (fp64 for a fp64
    run) and, with ``round_state``, the state is rounded to ``dtype`` after every step -- what upstream does with the prompt dtype."""
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    x = latents.to(dtype if round_state else wide)
    cfg = guidance != 1.0
    enc = (torch.cat([negative_text, text]) if cfg else text).to(dtype)
    with torch.no_grad():
        for t, a_t, a_prev in schedule:
            inp = x.to(dtype)
            inp = torch.cat([inp, inp]) if cfg else inp
            ts = torch.full((inp.shape[0],), t, dtype=torch.int64)
            out = fn(hidden_states=inp, encoder_hidden_states=enc, timestep=ts, image_rotary_emb=rope, return_dict=False)[0]
            if cfg:
                u, c = out.chunk(2)
                out = u + guidance * (c - u)
            x = ddim_step(x.to(wide), out.to(wide), a_t, a_prev)
            x = x.to(dtype) if round_state else x
    return x


# ---- models ------------------------------------------------------------------------------------------------------------------------------------------------
def kind_config(kind, layers=2):
    kw = dict(num_layers=layers, use_rotary_positional_embeddings=kind in ("rotary", "1.5"), **SMALL)
    if kind == "1.5":
        kw.update(patch_size_t=2, patch_bias=False)  # text-to-video 1.5: no ofs embedding
    return kw


def oracle_model(kind, layers=2, rank=64, seed=0):
    """``kind``: "sincos" (2b), "rotary" (5b), "1.5" (patch_size_t = 2, rotary, bias-free patch embedding), "plain" (sincos, no adapters).  Rank-``rank``
    adapters with B ~ N(0, 0.02); the LayerNorm affines are moved off (1, 0) so that they matter."""
    from oracle import cogvideox as cvx

    r = 0 if kind == "plain" else rank
    omodel = cvx.build_model(cvx.CogVideoXConfig(**kind_config(kind, layers)), seed=seed, rank=r, alpha=float(rank), lora_b_std=0.02 if r else None)
    with torch.no_grad():
        g = torch.Generator().manual_seed(7)
        for n, p in omodel.named_parameters():
            if "norm" in n and "linear" not in n and p.dim() == 1:
                p.copy_(((1.0 if n.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g)).to(p.dtype))
    return omodel


def fp32_copy(omodel):
    return copy.deepcopy(omodel).float()


def gpu_model(omodel, kind, device, layers=2, rank=64):
    from finetrainers_amd.cogvideox import CogVideoXTransformerConfig, MI355XCogVideoXTransformer3DModel

    sd = {k.replace("ff.proj_in.", "ff.net.0.proj.").replace("ff.proj_out.", "ff.net.2."): v for k, v in omodel.state_dict().items()}
    gmodel = MI355XCogVideoXTransformer3DModel(CogVideoXTransformerConfig(**kind_config(kind, layers)), device=device)
    gmodel.load_diffusers_state_dict(sd)
    if kind != "plain":
        gmodel.add_adapter(r=rank, lora_alpha=float(rank))
        gmodel.load_lora_state_dict({k: v for k, v in sd.items() if "lora_" in k})
    return gmodel


def oracle_rope(omodel, frames, height, width):
    """The rotary tables the reference hands the transformer for a LATENT grid (None for the sincos-table geometry)."""
    from oracle import cogvideox as cvx

    cfg = omodel.cfg
    if not cfg.use_rotary_positional_embeddings:
        return None
    return cvx.prepare_rotary_positional_embeddings(height * 8, width * 8, frames, 8, cfg.patch_size, cfg.patch_size_t, cfg.attention_head_dim,
                                                    cfg.sample_height * 8, cfg.sample_width * 8)
