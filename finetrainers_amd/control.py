"""Frame conditioning of the control trainer (finetrainers/trainer/control_trainer/data.py:202-268), restated: which frames of the control latents the model
gets to see.  ``apply_frame_conditioning_on_latents`` is the tensor form with the reference's signature; ``frame_keep_mask`` is the same decision as one
flag per frame of the noisy latents, which is what the pack kernel (ops.wan_control_pack) consumes.

``prefix`` and ``random`` draw from Python's ``random`` module with the reference's calls in the reference's order (``randint(1, n)``; for ``random`` then
``sample(range(n), k)``), so a run seeded with ``random.seed`` keeps the same frames here and there.  Each function draws ONCE per call: use one or the
other for a batch, not both."""

from __future__ import annotations

import random
from typing import List, Optional

import torch

FRAME_CONDITIONING_TYPES = ("index", "prefix", "random", "first_and_last", "full")


def _type_name(frame_conditioning_type) -> str:
    name = getattr(frame_conditioning_type, "value", frame_conditioning_type)  # the reference's FrameConditioningType is a str enum
    if name not in FRAME_CONDITIONING_TYPES:
        raise ValueError(f"frame_conditioning_type {frame_conditioning_type!r} is not one of {FRAME_CONDITIONING_TYPES}")
    return name


def _kept_frames(num_frames: int, name: str, index: Optional[int]) -> List[int]:
    """The frames of a ``num_frames``-long control clip whose mask is 1 (before the clip is cut or padded to the latents' length)."""
    if name == "index":
        if index is None:
            raise ValueError("frame_conditioning_type 'index' needs frame_conditioning_index")
        return [min(int(index), num_frames - 1)]
    if name == "prefix":
        return list(range(random.randint(1, num_frames)))
    if name == "random":
        keep = random.randint(1, num_frames)
        return random.sample(range(num_frames), keep)
    if name == "first_and_last":
        return [0, num_frames - 1]
    return list(range(num_frames))


def frame_keep_mask(num_frames: int, expected_num_frames: int, frame_conditioning_type, frame_conditioning_index: Optional[int] = None) -> torch.Tensor:
    """-> uint8 [expected_num_frames]: 1 where the control frame is kept, 0 where it is zeroed (dropped by the conditioning, or past the control clip's
    ``num_frames``).  ``full`` multiplies nothing in the reference: every frame of the clip is kept."""
    kept = _kept_frames(num_frames, _type_name(frame_conditioning_type), frame_conditioning_index)
    mask = torch.zeros(max(num_frames, expected_num_frames), dtype=torch.uint8)
    mask[[k % num_frames for k in kept]] = 1  # (a negative index counts from the clip's end, as tensor indexing does)
    mask[num_frames:] = 0
    return mask[:expected_num_frames].clone()


def apply_frame_conditioning_on_latents(latents: torch.Tensor, expected_num_frames: int, channel_dim: int, frame_dim: int, frame_conditioning_type,
                                        frame_conditioning_index: Optional[int] = None, concatenate_mask: bool = False) -> torch.Tensor:
    name = _type_name(frame_conditioning_type)
    num_frames = latents.size(frame_dim)
    mask = torch.zeros_like(latents)
    indexing = [slice(None)] * latents.ndim
    indexing[frame_dim] = _kept_frames(num_frames, name, frame_conditioning_index)
    mask[tuple(indexing)] = 1
    if name != "full":
        latents = latents * mask
    if num_frames >= expected_num_frames:
        latents, mask = latents.narrow(frame_dim, 0, expected_num_frames), mask.narrow(frame_dim, 0, expected_num_frames)
    else:
        pad_shape = list(latents.shape)
        pad_shape[frame_dim] = expected_num_frames - num_frames
        padding = latents.new_zeros(pad_shape)
        latents, mask = torch.cat([latents, padding], dim=frame_dim), torch.cat([mask, padding], dim=frame_dim)
    if concatenate_mask:  # (the reference concatenates the whole mask -- its one-channel slice is computed and never applied, data.py:263-266)
        latents = torch.cat([latents, mask], dim=channel_dim)
    return latents
