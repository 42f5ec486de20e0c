"""What the Wan sampler (pipeline.py) and the LongCat sampler (longcat_pipeline.py) do alike: plain functions, one copy each.

Input preparation as diffusers / the two reference pipelines do it (image preprocessing, the guide mask's shape, the generator's draw
order), the CFG-groups exchange of a job split into one rank group per CFG branch, and the tail that turns final latents into frames.
"""
from __future__ import annotations

from contextlib import nullcontext
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import ops


def preprocess_image(image, height: int, width: int) -> torch.Tensor:
    """diffusers VideoProcessor.preprocess: a PIL image (resized to the target) or a tensor [3,H,W] / [1,3,H,W] in [0,1] -> [1,3,H,W]
    fp32 in [-1,1], where the input lives: the caller moves it."""
    if isinstance(image, torch.Tensor):
        t = (image if image.dim() == 4 else image.unsqueeze(0)).to(torch.float32)
    else:
        if image.size != (width, height):
            image = image.resize((width, height))
        t = torch.from_numpy(np.array(image).astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    if t.shape[-2:] != (height, width):
        raise ValueError(f"image tensor is {tuple(t.shape[-2:])}, expected {(height, width)}")
    return 2.0 * t - 1.0


def guide_mask(mask, device) -> torch.Tensor:
    """The guide mask as the scheduler's fusion takes it (Wan PIPE:541-553, LongCat PIPE:803-817): [F,H,W], one frame as
    [1,C,H,W] or [1,1,H,W], [1,C,F,H,W] or [1,1,F,H,W], tensor or array of any float type -> [1,1,F,H,W] fp32 on `device`."""
    mask = torch.from_numpy(mask) if isinstance(mask, np.ndarray) else mask
    if mask.dim() == 3:
        mask = mask.unsqueeze(0).unsqueeze(1)
    elif mask.dim() == 4 and mask.shape[1] != 1:
        mask = mask[:, 0:1, :, :].unsqueeze(0)
    elif mask.dim() == 4 and mask.shape[0] == 1:
        mask = mask.unsqueeze(1)
    elif mask.dim() == 5 and mask.shape[1] != 1:
        mask = mask[:, 0:1, :, :, :]
    return mask.to(device, torch.float32)


def randn(shape, generator, device, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """diffusers randn_tensor: a CPU generator draws on the CPU and the result moves (RNG parity with the references).  The draw is made
    IN `dtype` (None: fp32): a bf16 draw consumes the generator differently from an fp32 draw cast down."""
    if generator is not None and generator.device.type == "cpu":
        return torch.randn(shape, generator=generator, dtype=dtype).to(device)
    return torch.randn(shape, generator=generator, dtype=dtype, device=device)


def cfg_groups_exchange(split, forward_branch: Callable[[int], torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """CFG groups x sequence shards (SURVEY 8e "P = 8 = 2 x 4"; parallel.Comm.split).  split = (the whole job's communicator, this rank's
    group): the ranks of group b run CFG branch b -- ONE forward per rank and evaluation, on a token shard twice as long, with half the
    K / V^T exchange -- and every rank then takes both velocities from one small all-gather over the whole job (a rank's slot holds its
    group's full tensor: [P, ...] -> slots 0 and P / 2).  -> (branch 0's velocity, branch 1's)."""
    world_comm, branch = split
    own = forward_branch(branch).contiguous()
    both = torch.empty((world_comm.world,) + tuple(own.shape), dtype=own.dtype, device=own.device)
    world_comm.all_gather(both, own)
    return both[0], both[world_comm.world // 2]


def decode_tail(vae, latents: torch.Tensor, output_type: str, to_vae_input: Callable[[torch.Tensor], torch.Tensor],
                crop: Optional[Tuple[int, int]] = None, tracer=None):
    """Final latents -> what the call hands back: the latents themselves (output_type "latent"), or the frames [B,F,H,W,C] in [0,1]
    decoded from to_vae_input(latents), cut to frames [crop[0], crop[1]) where given, as an array ("np") or a device tensor.  Either
    way a VAE call of this job that left the fp16 operand range (vae.AutoencoderKLWan.check_range) fails here, before anything is
    handed back."""
    video = latents
    if output_type != "latent":
        z = to_vae_input(latents)
        with tracer.range("final_decode") if tracer is not None else nullcontext():
            video = vae.decode(z, return_dict=False)[0]
            video = torch.stack([ops.postprocess_video(v) for v in video])
        if crop is not None:
            video = video[:, crop[0]:crop[1]]
    if hasattr(vae, "check_range"):
        vae.check_range()
    return video.cpu().numpy() if output_type == "np" else video
