"""Test reference for the Wan first/last-frame image-to-video model (Wan2.1-FLF2V: a transformer config with ``pos_embed_seq_len``): tests/wan_i2v_reference.py
extended with what the published diffusers ``WanTransformer3DModel`` adds for it ([upstream], unpinned like its parent):

* ``WanImageEmbedding`` with ``pos_embed`` [1, pos_embed_seq_len, image_dim]: the input is viewed as [-1, pos_embed_seq_len, image_dim] (upstream writes the
  view as ``(-1, 2 * seq_len, embed_dim)`` for its [2B, L, image_dim] input, the same thing there; a [B, 2L, image_dim] input passes through this form
  unchanged) and ``pos_embed`` is added in the module's dtype before the FP32LayerNorm -> Linear -> GELU -> Linear -> FP32LayerNorm chain.  Every block's
  attn2 then sees 2 x 257 = 514 image tokens: the blocks are the parent's;
* the conditioning mask of ``WanImageConditioningLatentEncodeProcessor`` (finetrainers/models/wan/base_specification.py:145-155), formulated
  independently of the specification's ``condition_mask`` (which follows the reference's lines): one keep flag per pixel frame -- the first, and with ``use_last_frame`` the last --, the first flag repeated ``temporal_downsample``
  times, the flags folded ``[F_latent, td] -> [td, F_latent]`` into channels and broadcast over batch, height and width."""
from dataclasses import dataclass

import torch
import torch.nn as nn

import wan_i2v_reference as i2v

bf16 = torch.bfloat16


@dataclass
class WanFLFConfig(i2v.WanI2VConfig):
    pos_embed_seq_len: int = 514


class WanImageEmbedding(i2v.WanImageEmbedding):
    def __init__(self, i, o, pos_embed_seq_len=None):
        super().__init__(i, o)
        self.pos_embed = nn.Parameter(torch.zeros(1, pos_embed_seq_len, i)) if pos_embed_seq_len is not None else None

    def forward(self, x):
        if self.pos_embed is not None:
            x = x.view(-1, self.pos_embed.shape[1], x.shape[-1])
            x = x + self.pos_embed
        return super().forward(x)


class WanFLFTransformer3DModel(i2v.WanI2VTransformer3DModel):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.condition_embedder.image_embedder = WanImageEmbedding(cfg.image_dim, cfg.inner_dim, cfg.pos_embed_seq_len)


def condition_mask(latents: torch.Tensor, num_frames: int, use_last_frame: bool, temporal_downsample: int = 4) -> torch.Tensor:
    """base_specification.py:145-155 (``latents`` [B, C, F_latent, h, w] gives batch, height, width and dtype; ``num_frames`` counts PIXEL frames)."""
    B, h, w = latents.shape[0], latents.shape[3], latents.shape[4]
    keep = torch.zeros(num_frames, dtype=latents.dtype)  # one flag per pixel frame: frames 1: (or 1:-1) are dropped
    keep[0] = 1
    if use_last_frame:
        keep[-1] = 1
    keep = torch.cat([keep[:1].repeat(temporal_downsample), keep[1:]])  # the first frame stands for a whole latent frame
    folded = keep.view(-1, temporal_downsample).t()  # [F_latent, td] -> [td, F_latent]: the pixel frames of a latent frame become channels
    return folded.reshape(1, temporal_downsample, -1, 1, 1).expand(B, -1, -1, h, w).to(latents.device)
