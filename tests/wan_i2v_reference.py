"""Test reference for Wan image-to-video: oracle.wan's classes extended with what the published diffusers ``WanTransformer3DModel`` adds when
``image_dim`` / ``added_kv_proj_dim`` are set ([upstream], unpinned like the rest of oracle/wan.py; the 257-token form only):

* ``WanImageEmbedding``: FP32LayerNorm(image_dim) -> Linear -> exact GELU -> Linear(image_dim, D) -> FP32LayerNorm(D), diffusers parameter names;
* attn2 with a second key / value set (``WanAttnProcessor2_0``): k_i = norm_added_k(add_k_proj(img)), v_i = add_v_proj(img), two independent softmaxes,
  each output cast to the query's dtype, then summed;
* the 36-channel input of the specification's forward (finetrainers/models/wan/base_specification.py:457-481).

Also the fp64 / bf16-storage evaluations of the second-context attention that the kernel tests measure against."""
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import wan
from oracle.ltx import RMSNorm, native_sdpa

bf16 = torch.bfloat16
LOG2E = 1.4426950408889634


@dataclass
class WanI2VConfig(wan.WanConfig):
    in_channels: int = 36
    image_dim: int = 1280


class _Gelu(nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.proj = nn.Linear(i, o)

    def forward(self, x):
        return F.gelu(self.proj(x))


class _FeedForward(nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.net = nn.ModuleList([_Gelu(i, i), nn.Dropout(0.0), nn.Linear(i, o)])

    def forward(self, x):
        for m in self.net:
            x = m(x)
        return x


class WanImageEmbedding(nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.norm1, self.ff, self.norm2 = wan.FP32LayerNorm(i), _FeedForward(i, o), wan.FP32LayerNorm(o)

    def forward(self, x):
        return self.norm2(self.ff(self.norm1(x)))


class WanI2VAttention(wan.WanAttention):
    def __init__(self, cfg):
        super().__init__(cfg)
        d = cfg.inner_dim
        self.add_k_proj, self.add_v_proj = nn.Linear(d, d), nn.Linear(d, d)
        self.norm_added_k = RMSNorm(d, cfg.eps, elementwise_affine=True)

    def forward(self, hidden_states, encoder_hidden_states=None, encoder_hidden_states_image=None, rotary_emb=None):
        q, k, v = self.norm_q(self.to_q(hidden_states)), self.norm_k(self.to_k(encoder_hidden_states)), self.to_v(encoder_hidden_states)
        split = lambda t: t.unflatten(2, (self.heads, -1)).transpose(1, 2)
        q, k, v = split(q), split(k), split(v)
        o = native_sdpa(q, k, v, None).transpose(1, 2).flatten(2, 3).type_as(q)
        if encoder_hidden_states_image is not None and encoder_hidden_states_image.shape[1] > 0:
            ki, vi = split(self.norm_added_k(self.add_k_proj(encoder_hidden_states_image))), split(self.add_v_proj(encoder_hidden_states_image))
            o = o + native_sdpa(q, ki, vi, None).transpose(1, 2).flatten(2, 3).type_as(q)
        return self.to_out[1](self.to_out[0](o))


class WanI2VTransformerBlock(wan.WanTransformerBlock):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.attn2 = WanI2VAttention(cfg)

    def forward(self, hidden_states, encoder_hidden_states, temb, rotary_emb, encoder_hidden_states_image=None):
        shift_msa, scale_msa, gate_msa, c_shift, c_scale, c_gate = (self.scale_shift_table + temb.float()).chunk(6, dim=1)
        n = (self.norm1(hidden_states.float()) * (1 + scale_msa) + shift_msa).type_as(hidden_states)
        a = self.attn1(n, rotary_emb=rotary_emb)
        hidden_states = (hidden_states.float() + a * gate_msa).type_as(hidden_states)
        n = self.norm2(hidden_states.float()).type_as(hidden_states)
        hidden_states = hidden_states + self.attn2(n, encoder_hidden_states=encoder_hidden_states, encoder_hidden_states_image=encoder_hidden_states_image)
        n = (self.norm3(hidden_states.float()) * (1 + c_scale) + c_shift).type_as(hidden_states)
        f = self.ffn(n)
        return (hidden_states.float() + f.float() * c_gate).type_as(hidden_states)


class WanI2VTransformer3DModel(wan.WanTransformer3DModel):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.condition_embedder.image_embedder = WanImageEmbedding(cfg.image_dim, cfg.inner_dim)
        self.blocks = nn.ModuleList([WanI2VTransformerBlock(cfg) for _ in range(cfg.num_layers)])

    def forward(self, hidden_states, timestep, encoder_hidden_states, encoder_hidden_states_image=None, return_dict=True, **kwargs):
        b, _, f, h, w = hidden_states.shape
        pt, ph, pw = self.cfg.patch_size
        ppf, pph, ppw = f // pt, h // ph, w // pw
        rotary = self.rope(hidden_states)
        x = self.patch_embedding(hidden_states).flatten(2).transpose(1, 2)
        temb, tproj, enc, enc_img = self.condition_embedder(timestep, encoder_hidden_states, encoder_hidden_states_image)
        tproj = tproj.unflatten(1, (6, -1))
        for blk in self.blocks:
            x = blk(x, enc, tproj, rotary, enc_img)
        shift, scale = (self.scale_shift_table + temb.unsqueeze(1)).chunk(2, dim=1)
        x = (self.norm_out(x.float()) * (1 + scale) + shift).type_as(x)
        x = self.proj_out(x)
        x = x.reshape(b, ppf, pph, ppw, pt, ph, pw, -1).permute(0, 7, 1, 4, 2, 5, 3, 6)
        out = x.flatten(6, 7).flatten(4, 5).flatten(2, 3)
        return (out,) if not return_dict else {"sample": out}


def i2v_model_input(moments, latents_mean, latents_std, sigmas, eps, noise, latent_condition, latent_condition_mask):
    """base_specification.py:457-481 up to the model call -> (hidden_states [B, 36, F, H, W], latents, timesteps)."""
    mu, logvar = torch.chunk(moments, 2, dim=1)
    mu, logvar = wan.normalize_latents(mu, latents_mean, latents_std), wan.normalize_latents(logvar, latents_mean, latents_std)
    latents = wan.posterior_sample(torch.cat([mu, logvar], dim=1), eps)
    mu, logvar = torch.chunk(latent_condition, 2, dim=1)
    mu, logvar = wan.normalize_latents(mu, latents_mean, latents_std), wan.normalize_latents(logvar, latents_mean, latents_std)
    cond = torch.chunk(torch.cat([mu, logvar], dim=1), 2, dim=1)[0]  # DiagonalGaussianDistribution(...).mode()
    noisy = (1.0 - sigmas) * latents + sigmas * noise
    noisy = torch.cat([noisy, latent_condition_mask, cond], dim=1)
    return noisy.to(latents), latents, (sigmas.flatten() * 1000.0).long()


def spec_forward_i2v(transformer, moments, latents_mean, latents_std, encoder_hidden_states, sigmas, eps, noise, latent_condition, latent_condition_mask,
                     encoder_hidden_states_image):
    hidden, latents, timesteps = i2v_model_input(moments, latents_mean, latents_std, sigmas, eps, noise, latent_condition, latent_condition_mask)
    pred = transformer(hidden_states=hidden, encoder_hidden_states=encoder_hidden_states, encoder_hidden_states_image=encoder_hidden_states_image,
                       timestep=timesteps, return_dict=False)[0]
    return pred, noise - latents, sigmas


# ---- the second-context attention alone: [B, H, S, 128] tensors holding bf16 values ------------------------------------------------------------------
def _ctx2(q, k, v, o_t, do, dq_t, dt, rnd):
    """o = rnd(o_t + rnd(softmax(q k^T / sqrt(d)) v)), dq = rnd(dq_t + rnd(dq_i)), lse (log2 domain); everything inside the softmax in ``dt``."""
    q = q.to(dt).requires_grad_(True)
    s = (q @ k.to(dt).transpose(-1, -2)) / q.shape[-1] ** 0.5
    oi = rnd(torch.softmax(s, dim=-1) @ v.to(dt))
    (dqi,) = torch.autograd.grad(oi, q, do.to(dt))
    return rnd(o_t.to(dt) + oi.detach()), rnd(dq_t.to(dt) + rnd(dqi)), torch.logsumexp(s.detach(), dim=-1) * LOG2E


def ctx2_fp64(q, k, v, o_t, do, dq_t):
    return _ctx2(q, k, v, o_t, do, dq_t, torch.float64, lambda t: t)


def ctx2_bf16_storage(q, k, v, o_t, do, dq_t):
    """The same graph with bf16 STORAGE at the reference's rounding points (each SDPA output, the sum of the two, each gradient entering or leaving an
    SDPA backward, the sum of the two dq) and fp32 inside each fused SDPA: the yardstick whose distance from fp64 the kernel may at most double."""
    return _ctx2(q, k, v, o_t, do, dq_t, torch.float32, lambda t: t.to(bf16).float())
