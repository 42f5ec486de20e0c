"""VGGT's aggregator, camera head and DPT depth head on this engine's own kernels: images in; aggregated tokens, `pose_enc`, extrinsics,
intrinsics, depth maps and their confidence out.

What the reference runs as `model.aggregator(images)` under bf16 autocast, then `model.camera_head(tokens)` in fp32 (vggt/run_warp.py:212-234;
AGG = vggt/models/aggregator.py, ATT = vggt/layers/attention.py, ROPE = vggt/layers/rope.py, DINO = vggt/layers/vision_transformer.py,
CAM = vggt/heads/camera_head.py).  The aggregator's linears are bf16 MFMA (wf_gemm_bf16, weights rounded once at load: what autocast does
per call) on an fp32 residual stream; LayerNorms, LayerScale, tokens and the position table are fp32.  The camera head is fp32 throughout.

    rows = wf_vit_patch_rows(images)                              (x - mean) / std in fp32, bf16 [n P, 592]
    DINOv2 (DINO:214-271), per frame T = 5 + P tokens:
    x    = [cls + pos_0; registers; pos' + wf_gemm_bf16(rows, proj)]     pos' = position table, bicubic + antialias to the patch grid (cached)
    per block:  n = wf_ln_modulate(x) -> bf16;  qkv = wf_gemm_bf16(n);  a = wf_vit_attn_fwd(qkv, nseq = S, L = T)
                x += ls1 * wf_gemm_bf16(a, proj)   WF_EPI_RESID;   h = wf_gemm_bf16(n2, fc1) f32 -> wf_act GELU-erf -> bf16;  x += ls2 * fc2
    patch tokens = rows 5.. of wf_ln_modulate(x, norm)
    aggregator (AGG:184-258): tokens = [camera_token[i]; register_token[i]; patch tokens], i = 0 for frame 0 and 1 for the others
    per depth: a frame block (nseq = S, L = T) then a global block (nseq = 1, L = S T): the same block with wf_vit_qk_norm_rope
               (per-head LayerNorm on q and k + 2D RoPE) in front of the attention; kept layers = cat(frame out, global out) [S, T, 2 C]
    camera head (CAM:73-141) on the last layer's camera tokens [S, 2 C]: wf_gemm_f32, wf_clip_attn_fwd (D = 128, L = S), wf_ln_modulate,
    the AdaLN modulate / gate and the activations as torch ops on [S, 2 C].

    depth head (DPT = vggt/heads/dpt_head.py:172-291, opt-in: `depth=True` at load), fp32 throughout like the reference's (run_warp.py:234
    calls it outside autocast), channels-last maps [n, H, W, C], per chunk of frames, for the four kept layers i = 0..3:
        rows = wf_ln_modulate(tokens[layer_i][:, 5:])                   the one LayerNorm(2 C), eps 1e-5
        y    = pos(gh, gw) ; wf_gemm_f32(rows, projects[i]) WF_EPI_F32_ACC      the 1x1 projection on top of the position embedding
        map  = ConvTranspose k = s = 4 / 2 as wf_gemm_f32 to [pixels, s s Cout] + a pixel shuffle | identity | wf_conv2d_f32 stride 2
        l_i  = wf_conv2d_f32(map, layer{i+1}_rn)                        bias-free 3x3 to `depth_features` channels
    fusion (refinenet4 .. 1): out = [out + RCU1(l_i)] ; RCU2(out) ; the 1x1 out_conv (wf_gemm_f32) ; wf_resize_bilinear_cl_f32 to the next
        map's size -- the 1x1 runs BEFORE the resize (both are linear and the bilinear weights sum to one: a quarter of its FLOPs);
        RCU(x) = conv2(relu(conv1(relu(x)))) + relu(x) in two wf_conv2d_f32 calls: the reference's ReLU is in place, so the skip is relu(x)
    head: output_conv1 ; resize to (14 gh, 14 gw) + position tables ; output_conv2.0 + ReLU ; wf_dpt_depth_out (1x1 to 2, exp / 1 + exp).
    The position embedding (vggt/heads/utils.py) is separable: a column table [w][C / 2] and a row table [h][C / 2], built on the host with
    the reference's own torch calls and cached per shape (dpt_pos_tables).

Not built: the point / track heads, DPTHead's `feature_only` and `down_ratio != 1`, `mode="pad"` of the preprocessing, images of mixed shapes.
"""
from __future__ import annotations

import json
import os
import warnings
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

WF_F32, WF_BF16 = 0, 1
EPI_BF16, EPI_F32, EPI_RESID, EPI_F32_ACC, EPI_F32_GELU = 0, 2, 3, 4, 5
PATCH_K = 592                 # 3 * 14 * 14 = 588 padded to a multiple of 8 (wf_vit_patch_rows)
MAX_FRAMES = 1024             # wf_clip_attn_fwd over the camera tokens
IGNORED = ("depth_head.", "point_head.", "track_head.", "aggregator.patch_embed.mask_token")
KEEP = (4, 11, 17, 23)


@dataclass(frozen=True)
class VGGTConfig:
    img_size: int = 518
    patch_size: int = 14
    embed_dim: int = 1024
    depth: int = 24
    num_heads: int = 16
    mlp_ratio: float = 4.0
    num_register_tokens: int = 4
    rope_freq: float = 100.0
    init_values: float = 0.01
    qk_norm: bool = True
    aa_order: Tuple[str, ...] = ("frame", "global")
    aa_block_size: int = 1
    patch_embed: str = "dinov2_vitl14_reg"
    dino_depth: int = 24
    dino_num_heads: int = 16
    dino_eps: float = 1e-6
    dino_init_values: float = 1.0
    camera_trunk_depth: int = 4
    camera_num_heads: int = 16
    camera_iterations: int = 4
    depth_features: int = 256
    depth_out_channels: Tuple[int, ...] = (256, 512, 1024, 1024)
    depth_layers: Tuple[int, ...] = (4, 11, 17, 23)

    @property
    def patch_start_idx(self) -> int:
        return 1 + self.num_register_tokens

    @property
    def hidden(self) -> int:
        return int(self.embed_dim * self.mlp_ratio)

    @property
    def pos_grid(self) -> int:
        return self.img_size // self.patch_size

    @property
    def camera_dim(self) -> int:
        return 2 * self.embed_dim

    @classmethod
    def from_dict(cls, d: dict) -> "VGGTConfig":
        d = dict(d)
        if "aa_order" in d:
            d["aa_order"] = tuple(d["aa_order"])
        for k in ("depth_out_channels", "depth_layers"):
            if k in d:
                d[k] = tuple(int(v) for v in d[k])
        cfg = cls(**{k: d[k] for k in cls.__dataclass_fields__ if k in d})
        if cfg.patch_size != 14:
            raise NotImplementedError(f"patch_size {cfg.patch_size}: wf_vit_patch_rows is built for 14")
        if cfg.embed_dim % cfg.num_heads or cfg.embed_dim // cfg.num_heads != 64:
            raise NotImplementedError(f"aggregator head width {cfg.embed_dim / cfg.num_heads:g}: wf_vit_attn_fwd is built for 64")
        if cfg.embed_dim % cfg.dino_num_heads or cfg.embed_dim // cfg.dino_num_heads != 64:
            raise NotImplementedError(f"DINOv2 head width {cfg.embed_dim / cfg.dino_num_heads:g}: wf_vit_attn_fwd is built for 64")
        if tuple(cfg.aa_order) != ("frame", "global"):
            raise NotImplementedError(f"aa_order {list(cfg.aa_order)}: built is ['frame', 'global']")
        if cfg.aa_block_size != 1:
            raise NotImplementedError(f"aa_block_size {cfg.aa_block_size}: built is 1")
        if not cfg.rope_freq > 0:
            raise NotImplementedError(f"rope_freq {cfg.rope_freq}: the blocks are built with the 2D RoPE")
        if not cfg.qk_norm:
            raise NotImplementedError("qk_norm off: the frame and global blocks are built with q_norm / k_norm")
        if not cfg.patch_embed.startswith("dinov2"):
            raise NotImplementedError(f"patch_embed {cfg.patch_embed!r}: built is the DINOv2 ViT")
        if cfg.camera_dim % cfg.camera_num_heads or not 8 <= cfg.camera_dim // cfg.camera_num_heads <= 128 or (cfg.camera_dim // cfg.camera_num_heads) % 8:
            raise NotImplementedError("camera trunk head width: wf_clip_attn_fwd takes multiples of 8 in 8..128")
        if min(cfg.depth, cfg.dino_depth, cfg.camera_trunk_depth, cfg.num_register_tokens, cfg.img_size) < 1 or cfg.img_size % 14:
            raise ValueError("depths, register tokens and img_size must be positive, img_size a multiple of 14")
        if len(cfg.depth_layers) != 4 or len(cfg.depth_out_channels) != 4:
            raise NotImplementedError(f"depth_layers {list(cfg.depth_layers)} / depth_out_channels {list(cfg.depth_out_channels)}: the DPT head "
                                      "is built for four kept layers")
        if cfg.depth_features < 8 or cfg.depth_features % 8 or any(c < 4 or c % 4 for c in cfg.depth_out_channels):
            raise NotImplementedError(f"depth_features {cfg.depth_features} / depth_out_channels {list(cfg.depth_out_channels)}: wf_conv2d_f32 "
                                      "takes channel counts that are multiples of 4 (depth_features / 2 included)")
        if "depth_layers" in d:      # a config that does not name them (no depth head in its checkpoint) is checked when the head is loaded
            cfg.check_depth_layers()
        return cfg

    def check_depth_layers(self):
        if any(not 0 <= k < self.depth for k in self.depth_layers):
            raise ValueError(f"depth_layers {list(self.depth_layers)}: layers 0..{self.depth - 1} exist")

    @classmethod
    def from_json(cls, path: str) -> "VGGTConfig":
        with open(path) as f:
            return cls.from_dict(json.load(f))


def _block_keys(prefix: str, C: int, F: int, qk_norm: bool) -> Dict[str, Tuple[int, ...]]:
    out = {}
    for n in ("norm1", "norm2"):
        out[f"{prefix}{n}.weight"], out[f"{prefix}{n}.bias"] = (C,), (C,)
    out[f"{prefix}attn.qkv.weight"], out[f"{prefix}attn.qkv.bias"] = (3 * C, C), (3 * C,)
    out[f"{prefix}attn.proj.weight"], out[f"{prefix}attn.proj.bias"] = (C, C), (C,)
    if qk_norm:
        for n in ("q_norm", "k_norm"):
            out[f"{prefix}attn.{n}.weight"], out[f"{prefix}attn.{n}.bias"] = (64,), (64,)
    out[f"{prefix}ls1.gamma"], out[f"{prefix}ls2.gamma"] = (C,), (C,)
    out[f"{prefix}mlp.fc1.weight"], out[f"{prefix}mlp.fc1.bias"] = (F, C), (F,)
    out[f"{prefix}mlp.fc2.weight"], out[f"{prefix}mlp.fc2.bias"] = (C, F), (C,)
    return out


def depth_head_keys(cfg: VGGTConfig) -> Dict[str, Tuple[int, ...]]:
    """{key: shape} of DPTHead(dim_in = 2 C, output_dim = 2, features, out_channels) under `depth_head.` (DPT:66-113, 299-341)."""
    D, f, oc, dh = cfg.camera_dim, cfg.depth_features, cfg.depth_out_channels, "depth_head."
    out: Dict[str, Tuple[int, ...]] = {dh + "norm.weight": (D,), dh + "norm.bias": (D,)}
    for i, c in enumerate(oc):
        out[f"{dh}projects.{i}.weight"], out[f"{dh}projects.{i}.bias"] = (c, D, 1, 1), (c,)
    for i, k in ((0, 4), (1, 2), (3, 3)):
        out[f"{dh}resize_layers.{i}.weight"], out[f"{dh}resize_layers.{i}.bias"] = (oc[i], oc[i], k, k), (oc[i],)
    sc = dh + "scratch."
    for i, c in enumerate(oc):
        out[f"{sc}layer{i + 1}_rn.weight"] = (f, c, 3, 3)
    for i in (1, 2, 3, 4):
        r = f"{sc}refinenet{i}."
        out[r + "out_conv.weight"], out[r + "out_conv.bias"] = (f, f, 1, 1), (f,)
        for u in (("resConfUnit1", "resConfUnit2") if i < 4 else ("resConfUnit2",)):
            for c in ("conv1", "conv2"):
                out[f"{r}{u}.{c}.weight"], out[f"{r}{u}.{c}.bias"] = (f, f, 3, 3), (f,)
    out.update({sc + "output_conv1.weight": (f // 2, f, 3, 3), sc + "output_conv1.bias": (f // 2,),
                sc + "output_conv2.0.weight": (32, f // 2, 3, 3), sc + "output_conv2.0.bias": (32,),
                sc + "output_conv2.2.weight": (2, 32, 1, 1), sc + "output_conv2.2.bias": (2,)})
    return out


def expected_state_dict(cfg: VGGTConfig, depth: bool = False) -> Dict[str, Tuple[int, ...]]:
    """{key of the reference's VGGT module: shape} of everything this engine uploads: `aggregator.*` (without the DINOv2 mask token) and
    `camera_head.*`; with `depth=True` also `depth_head.*`."""
    C, F, R, D = cfg.embed_dim, cfg.hidden, cfg.num_register_tokens, cfg.camera_dim
    out: Dict[str, Tuple[int, ...]] = {"aggregator.camera_token": (1, 2, 1, C), "aggregator.register_token": (1, 2, R, C)}
    pe = "aggregator.patch_embed."
    out.update({pe + "cls_token": (1, 1, C), pe + "pos_embed": (1, 1 + cfg.pos_grid ** 2, C), pe + "register_tokens": (1, R, C),
                pe + "patch_embed.proj.weight": (C, 3, 14, 14), pe + "patch_embed.proj.bias": (C,), pe + "norm.weight": (C,), pe + "norm.bias": (C,)})
    for i in range(cfg.dino_depth):
        out.update(_block_keys(f"{pe}blocks.{i}.", C, F, False))
    for i in range(cfg.depth):
        out.update(_block_keys(f"aggregator.frame_blocks.{i}.", C, F, True))
        out.update(_block_keys(f"aggregator.global_blocks.{i}.", C, F, True))
    ch = "camera_head."
    for i in range(cfg.camera_trunk_depth):
        out.update(_block_keys(f"{ch}trunk.{i}.", D, 4 * D, False))
    for n in ("token_norm", "trunk_norm"):
        out[f"{ch}{n}.weight"], out[f"{ch}{n}.bias"] = (D,), (D,)
    out.update({ch + "empty_pose_tokens": (1, 1, 9), ch + "embed_pose.weight": (D, 9), ch + "embed_pose.bias": (D,),
                ch + "poseLN_modulation.1.weight": (3 * D, D), ch + "poseLN_modulation.1.bias": (3 * D,),
                ch + "pose_branch.fc1.weight": (D // 2, D), ch + "pose_branch.fc1.bias": (D // 2,),
                ch + "pose_branch.fc2.weight": (9, D // 2), ch + "pose_branch.fc2.bias": (9,)})
    if depth:
        out.update(depth_head_keys(cfg))
    return out


def consumed_header(found: Dict[str, dict], where: str = "checkpoint", depth: bool = False) -> Dict[str, dict]:
    """The entries this engine uploads; the heads that are not built (or, without `depth=True`, not asked for) and the DINOv2 mask token
    are dropped with ONE warning.  With `depth=True` the `depth_head.*` entries are kept and checked like every other."""
    ignored = tuple(g for g in IGNORED if not (depth and g == "depth_head."))
    keep = {k: v for k, v in found.items() if not k.startswith(ignored)}
    if len(keep) != len(found):
        groups = sorted({g for g in ignored for k in found if k.startswith(g)})
        warnings.warn(f"{where}: {len(found) - len(keep)} tensors of {', '.join(groups)} are not consumed (heads not built here) and are ignored",
                      UserWarning, stacklevel=3)
    return keep


def _raise_on(keep: Dict[str, dict], cfg: VGGTConfig, where: str, depth: bool = False):
    from .checkpoint import compare_header
    if depth:
        cfg.check_depth_layers()
    missing, unexpected, wrong = compare_header(keep, expected_state_dict(cfg, depth))
    if missing:
        raise KeyError(f"{where}: {len(missing)} parameters of the aggregator / camera head{' / depth head' if depth else ''} are not in the "
                       f"checkpoint: {missing[:5]}")
    if wrong:
        w = wrong[0]
        raise ValueError(f"{where}: {len(wrong)} parameters have the wrong shape: {w['key']} is {w['found']}, expected {w['expected']}")
    if unexpected:
        raise ValueError(f"{where}: {len(unexpected)} checkpoint tensors are not consumed: {unexpected[:5]}")


# ---- RoPE tables and positions (ROPE:86-117, AGG:219-228) ---------------------------------------------------------------------------------
def rope_tables(max_pos: int, freq: float = 100.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos / sin f32 [max_pos + 1][16]: the reference's fp32 angles (position x 1 / freq^(2 i / 32), both fp32), their cosine and sine
    taken in float64 and rounded once."""
    exponents = torch.arange(0, 32, 2).float() / 32
    inv_freq = 1.0 / (freq ** exponents)
    angles = torch.einsum("i,j->ij", torch.arange(max_pos + 1, dtype=inv_freq.dtype), inv_freq).double()
    return angles.cos().float().contiguous(), angles.sin().float().contiguous()


def token_positions(gh: int, gw: int, n_special: int, frames: int = 1) -> torch.Tensor:
    """int32 [frames * (n_special + gh gw)][2] = (y, x): special tokens (0, 0), patch (y, x) carries (y + 1, x + 1)."""
    yx = torch.cartesian_prod(torch.arange(gh), torch.arange(gw)).reshape(gh * gw, 2) + 1
    one = torch.cat([torch.zeros(n_special, 2, dtype=yx.dtype), yx], 0)
    return one.repeat(frames, 1).to(torch.int32).contiguous()


# ---- the DPT head's position embedding (DPT:249-259, vggt/heads/utils.py) ------------------------------------------------------------------
def dpt_pos_tables(C: int, h: int, w: int, image_hw: Tuple[int, int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """_apply_pos_embed's addend for a [C, h, w] map of an image of size image_hw, as its two factors: (col f32 [w][C / 2], row f32
    [h][C / 2]); channel c < C / 2 of pixel (y, x) receives col[x][c], channel c >= C / 2 receives row[y][c - C / 2].  Built with the
    reference's own torch calls, so bit-equal to it: the coordinate is an fp32 linspace over -+span (n - 1) / n (span_x = a / sqrt(a^2 + 1),
    span_y = 1 / sqrt(a^2 + 1), a = W / H of the image), the angles coordinate x 100^(-k / (C / 4)) are float64, [sin | cos] is rounded
    to fp32 and then multiplied by 0.1 in fp32."""
    if C % 4:
        raise ValueError(f"dpt_pos_tables: {C} channels: each axis takes C / 2 channels, half sines and half cosines")
    H, W = image_hw
    aspect = W / H
    diag = (aspect ** 2 + 1.0) ** 0.5
    span_x, span_y = aspect / diag, 1.0 / diag
    xs = torch.linspace(-span_x * (w - 1) / w, span_x * (w - 1) / w, steps=w, dtype=torch.float32)
    ys = torch.linspace(-span_y * (h - 1) / h, span_y * (h - 1) / h, steps=h, dtype=torch.float32)
    omega = torch.arange(C // 4, dtype=torch.double)
    omega /= (C // 2) / 2.0
    omega = 1.0 / 100 ** omega

    def table(pos):
        out = torch.einsum("m,d->md", pos, omega)
        return (torch.cat([torch.sin(out), torch.cos(out)], dim=1).float() * 0.1).contiguous()
    return table(xs), table(ys)


def dpt_pos_embed(C: int, h: int, w: int, image_hw: Tuple[int, int]) -> torch.Tensor:
    """The two tables expanded to the reference's addend, f32 [C, h, w] (the patch grids and the tests; never the full-resolution map)."""
    col, row = dpt_pos_tables(C, h, w, image_hw)
    return torch.cat([col.t()[:, None, :].expand(C // 2, h, w), row.t()[:, :, None].expand(C // 2, h, w)], 0).contiguous()


def to_image_size(depth: torch.Tensor, depth_conf: torch.Tensor, intrinsic: torch.Tensor, model_hw: Tuple[int, int], orig_hw: Tuple[int, int]):
    """The hand-over to stage 1 (run_warp.py:273-292): depth f32 [..., H, W, 1] and depth_conf f32 [..., H, W] at the model's size ->
    the original image's size with half-pixel bilinear (cv2.INTER_LINEAR on float maps = wf_resize_bilinear2d), and the intrinsics
    [..., 3, 3] with fx, cx scaled by orig_w / model_w and fy, cy by orig_h / model_h.  -> (depth [..., h, w, 1], conf [..., h, w], K)."""
    from . import ops
    (H, W), (oh, ow) = model_hw, orig_hw
    if tuple(depth.shape[-3:]) != (H, W, 1) or tuple(depth_conf.shape[-2:]) != (H, W) or tuple(intrinsic.shape[-2:]) != (3, 3):
        raise ValueError(f"to_image_size: depth {tuple(depth.shape)}, depth_conf {tuple(depth_conf.shape)}, intrinsic {tuple(intrinsic.shape)} "
                         f"do not match the model size {(H, W)}")
    d = ops.resize_bilinear2d(depth.squeeze(-1).contiguous(), oh, ow).unsqueeze(-1)
    c = ops.resize_bilinear2d(depth_conf.contiguous(), oh, ow)
    K = intrinsic.clone()
    K[..., 0, 0] *= ow / W
    K[..., 0, 2] *= ow / W
    K[..., 1, 1] *= oh / H
    K[..., 1, 2] *= oh / H
    return d, c, K


# ---- pose encoding -> matrices (vggt/utils/pose_enc.py:62-130, rotation.py:14-44) -----------------------------------------------------------
def pose_encoding_to_extri_intri(pose_enc: torch.Tensor, image_size_hw: Tuple[int, int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """pose_enc [B, S, 9] = (T 3, quaternion xyzw 4, FoV h, FoV w) -> (extrinsic [B, S, 3, 4] = [R | T], intrinsic [B, S, 3, 3])."""
    T, quat, fov_h, fov_w = pose_enc[..., :3], pose_enc[..., 3:7], pose_enc[..., 7], pose_enc[..., 8]
    i, j, k, r = torch.unbind(quat, -1)
    two_s = 2.0 / (quat * quat).sum(-1)
    R = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1).reshape(quat.shape[:-1] + (3, 3))
    extrinsic = torch.cat([R, T[..., None]], -1)
    H, W = image_size_hw
    K = torch.zeros(pose_enc.shape[:-1] + (3, 3), dtype=pose_enc.dtype, device=pose_enc.device)
    K[..., 0, 0] = (W / 2.0) / torch.tan(fov_w / 2.0)
    K[..., 1, 1] = (H / 2.0) / torch.tan(fov_h / 2.0)
    K[..., 0, 2], K[..., 1, 2], K[..., 2, 2] = W / 2, H / 2, 1.0
    return extrinsic, K


# ---- load_and_preprocess_images on PIL images (vggt/utils/load_fn.py:97-215) -----------------------------------------------------------------
def preprocess(pil_images: Sequence, mode: str = "crop", target: int = 518) -> torch.Tensor:
    """PIL images -> fp32 [N, 3, H, W] in [0, 1]: RGBA composited over white, width `target`, height rounded to a multiple of 14, PIL
    bicubic on the uint8 image, centre crop of the height above `target`.  Refused: an empty list, `mode="pad"`, images that end with
    different shapes (the reference pads those with white)."""
    from PIL import Image
    if len(pil_images) == 0:
        raise ValueError("At least 1 image is required")
    if mode == "pad":
        raise NotImplementedError('mode="pad" is not implemented')
    if mode != "crop":
        raise ValueError("Mode must be either 'crop' or 'pad'")
    out = []
    for img in pil_images:
        if not isinstance(img, Image.Image):
            raise TypeError(f"preprocess takes PIL images, got {type(img)}")
        if img.mode == "RGBA":
            img = Image.alpha_composite(Image.new("RGBA", img.size, (255, 255, 255, 255)), img)
        img = img.convert("RGB")
        w, h = img.size
        nh = round(h * (target / w) / 14) * 14
        img = img.resize((target, nh), Image.Resampling.BICUBIC)
        x = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).to(torch.float32).div(255)
        if nh > target:
            y0 = (nh - target) // 2
            x = x[:, y0:y0 + target]
        out.append(x.contiguous())
    if len({tuple(x.shape) for x in out}) > 1:
        raise NotImplementedError(f"images of mixed shapes {sorted({tuple(x.shape[1:]) for x in out})} are not implemented")
    return torch.stack(out)


def preprocess_device(images: Sequence, device, mode: str = "crop", target: int = 518) -> torch.Tensor:
    """preprocess on the device, bit for bit: PIL images or u8 [h, w, 3] arrays / tensors (host or device) -> fp32 [N, 3, H, W] on
    `device`.  On the host stays what decoding does there (RGBA over white, convert("RGB")); the bicubic resize, the centre crop, u8 ->
    f32 and the move to planar are one entry (ops.resample_u8_window) that computes the cropped rows only, images of equal source size in
    one call.  The 256-entry table is preprocess' own expression on every byte value.  The same refusals as preprocess."""
    from PIL import Image

    from . import ops
    if len(images) == 0:
        raise ValueError("At least 1 image is required")
    if mode == "pad":
        raise NotImplementedError('mode="pad" is not implemented')
    if mode != "crop":
        raise ValueError("Mode must be either 'crop' or 'pad'")
    px = []
    for img in images:
        if isinstance(img, Image.Image):
            if img.mode == "RGBA":
                img = Image.alpha_composite(Image.new("RGBA", img.size, (255, 255, 255, 255)), img)
            img = torch.from_numpy(np.asarray(img.convert("RGB")).copy())
        elif isinstance(img, np.ndarray):
            img = torch.from_numpy(img)
        if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise TypeError(f"preprocess_device takes PIL images or uint8 [h, w, 3] arrays / tensors, got {type(img)}")
        px.append(img)
    plans = []
    for x in px:
        h, w = x.shape[:2]
        nh = round(h * (target / w) / 14) * 14
        plans.append((nh, (nh - target) // 2 if nh > target else 0, min(nh, target)))
    if len({p[2] for p in plans}) > 1:
        raise NotImplementedError(f"images of mixed shapes {sorted({(p[2], target) for p in plans})} are not implemented")
    lut = torch.tensor(np.arange(256, dtype=np.uint8)).float().div(255).expand(3, 256).contiguous().to(device)
    groups: Dict[Tuple[int, int], list] = {}
    for i, x in enumerate(px):
        groups.setdefault(tuple(x.shape[:2]), []).append(i)
    out = None
    for idx in groups.values():
        nh, y0, Hc = plans[idx[0]]
        frames = torch.stack([px[i].to(device) for i in idx])
        x = ops.resample_u8_window(frames, (nh, target), (y0, 0, Hc, target), lut)
        if len(groups) == 1:
            return x
        if out is None:
            out = torch.empty((len(px),) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
        out[idx] = x
    return out


class VGGT:
    def __init__(self, cfg: Optional[VGGTConfig] = None, device="cuda:0"):
        self.cfg = cfg or VGGTConfig()
        self.device = torch.device(device)
        self.W: Dict[str, torch.Tensor] = {}
        self._pos_cache: Dict[Tuple[int, int], torch.Tensor] = {}
        self._rope_cache: Dict[Tuple[int, int, int], tuple] = {}
        self._dpt_cache: Dict[tuple, tuple] = {}
        self.has_depth = False

    # ---- weights ---------------------------------------------------------------------------------------------------------------------------
    def _assemble(self, get, depth: bool = False):
        """get(reference key) -> CPU tensor.  Aggregator linears bf16 (rounded once), everything else fp32; the camera head fp32 with its
        LayerScale folded into proj / fc2 and the 9-wide linears zero-padded to 12; `depth`: the DPT head too (_assemble_depth)."""
        cfg, dev = self.cfg, self.device
        f = lambda k: get(k).to(torch.float32).to(dev).contiguous()                      # noqa: E731
        b = lambda k: get(k).to(torch.float32).to(torch.bfloat16).to(dev).contiguous()   # noqa: E731
        C = cfg.embed_dim
        W: Dict[str, torch.Tensor] = {}
        pe = "aggregator.patch_embed."
        pw = torch.zeros(C, PATCH_K, dtype=torch.float32)
        pw[:, :588] = get(pe + "patch_embed.proj.weight").to(torch.float32).reshape(C, 588)
        W["patch.w"], W["patch.b"] = pw.to(torch.bfloat16).to(dev), f(pe + "patch_embed.proj.bias")
        W["cls"], W["pos"], W["reg"] = f(pe + "cls_token").reshape(C), f(pe + "pos_embed")[0], f(pe + "register_tokens")[0]
        W["dnorm.w"], W["dnorm.b"] = f(pe + "norm.weight"), f(pe + "norm.bias")
        W["cam_tok"], W["reg_tok"] = f("aggregator.camera_token")[0, :, 0], f("aggregator.register_token")[0]

        def block(name, src, qk):
            for n in ("norm1", "norm2"):
                W[f"{name}.{n}.w"], W[f"{name}.{n}.b"] = f(f"{src}{n}.weight"), f(f"{src}{n}.bias")
            for n, k in (("qkv", "attn.qkv"), ("proj", "attn.proj"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
                W[f"{name}.{n}.w"], W[f"{name}.{n}.b"] = b(f"{src}{k}.weight"), f(f"{src}{k}.bias")
            W[f"{name}.ls1"], W[f"{name}.ls2"] = f(f"{src}ls1.gamma"), f(f"{src}ls2.gamma")
            if qk:
                for n in ("q_norm", "k_norm"):
                    W[f"{name}.{n}.w"], W[f"{name}.{n}.b"] = f(f"{src}attn.{n}.weight"), f(f"{src}attn.{n}.bias")

        for i in range(cfg.dino_depth):
            block(f"d{i}", f"{pe}blocks.{i}.", False)
        for i in range(cfg.depth):
            block(f"f{i}", f"aggregator.frame_blocks.{i}.", True)
            block(f"g{i}", f"aggregator.global_blocks.{i}.", True)

        ch, D = "camera_head.", cfg.camera_dim
        for i in range(cfg.camera_trunk_depth):
            src, name = f"{ch}trunk.{i}.", f"c{i}"
            for n in ("norm1", "norm2"):
                W[f"{name}.{n}.w"], W[f"{name}.{n}.b"] = f(f"{src}{n}.weight"), f(f"{src}{n}.bias")
            W[f"{name}.qkv.w"], W[f"{name}.qkv.b"] = f(f"{src}attn.qkv.weight"), f(f"{src}attn.qkv.bias")
            W[f"{name}.fc1.w"], W[f"{name}.fc1.b"] = f(f"{src}mlp.fc1.weight"), f(f"{src}mlp.fc1.bias")
            for n, k, ls in (("proj", "attn.proj", "ls1"), ("fc2", "mlp.fc2", "ls2")):       # LayerScale folded: gamma * (W x + b)
                g = f(f"{src}{ls}.gamma")
                W[f"{name}.{n}.w"], W[f"{name}.{n}.b"] = (f(f"{src}{k}.weight") * g[:, None]).contiguous(), f(f"{src}{k}.bias") * g
        for n in ("token_norm", "trunk_norm"):
            W[f"{n}.w"], W[f"{n}.b"] = f(f"{ch}{n}.weight"), f(f"{ch}{n}.bias")
        W["empty_pose"] = f(ch + "empty_pose_tokens").reshape(9)
        ew = torch.zeros(D, 12, dtype=torch.float32, device=dev)
        ew[:, :9] = f(ch + "embed_pose.weight")
        W["embed.w"], W["embed.b"] = ew, f(ch + "embed_pose.bias")
        W["mod.w"], W["mod.b"] = f(ch + "poseLN_modulation.1.weight"), f(ch + "poseLN_modulation.1.bias")
        W["pb1.w"], W["pb1.b"] = f(ch + "pose_branch.fc1.weight"), f(ch + "pose_branch.fc1.bias")
        w2, b2 = torch.zeros(12, D // 2, dtype=torch.float32, device=dev), torch.zeros(12, dtype=torch.float32, device=dev)
        w2[:9], b2[:9] = f(ch + "pose_branch.fc2.weight"), f(ch + "pose_branch.fc2.bias")
        W["pb2.w"], W["pb2.b"] = w2, b2
        if depth:
            self._assemble_depth(W, f)
        self.W = W
        self.has_depth = bool(depth)
        self._pos_cache.clear()
        self._dpt_cache.clear()
        return self

    def _assemble_depth(self, W, f):
        """The DPT head, fp32: 3x3 weights packed [3][3][Cout][Cin] for wf_conv2d_f32, 1x1 weights as [Cout, Cin], the ConvTranspose
        weights [Cin][Cout][s][s] as the GEMM operand [(ky, kx, Cout)][Cin] with the bias repeated s s times."""
        dh, sc = "depth_head.", "depth_head.scratch."
        pack = lambda k: f(k).permute(2, 3, 0, 1).contiguous()                           # noqa: E731
        flat = lambda k: f(k).flatten(1).contiguous()                                    # noqa: E731
        W["dpt.norm.w"], W["dpt.norm.b"] = f(dh + "norm.weight"), f(dh + "norm.bias")
        for i in range(4):
            W[f"dpt.proj{i}.w"], W[f"dpt.proj{i}.b"] = flat(f"{dh}projects.{i}.weight"), f(f"{dh}projects.{i}.bias")
            W[f"dpt.rn{i}.w"] = pack(f"{sc}layer{i + 1}_rn.weight")
        for i, s in ((0, 4), (1, 2)):
            w = f(f"{dh}resize_layers.{i}.weight")
            W[f"dpt.up{i}.w"] = w.permute(2, 3, 1, 0).reshape(s * s * w.shape[1], w.shape[0]).contiguous()
            W[f"dpt.up{i}.b"] = f(f"{dh}resize_layers.{i}.bias").repeat(s * s).contiguous()
        W["dpt.down.w"], W["dpt.down.b"] = pack(dh + "resize_layers.3.weight"), f(dh + "resize_layers.3.bias")
        for i in (1, 2, 3, 4):
            r = f"{sc}refinenet{i}."
            W[f"dpt.ref{i}.out.w"], W[f"dpt.ref{i}.out.b"] = flat(r + "out_conv.weight"), f(r + "out_conv.bias")
            for u, name in ((("resConfUnit1", "rcu1"), ("resConfUnit2", "rcu2")) if i < 4 else (("resConfUnit2", "rcu2"),)):
                for c, cn in (("conv1", "c1"), ("conv2", "c2")):
                    W[f"dpt.ref{i}.{name}.{cn}.w"], W[f"dpt.ref{i}.{name}.{cn}.b"] = pack(f"{r}{u}.{c}.weight"), f(f"{r}{u}.{c}.bias")
        W["dpt.oc1.w"], W["dpt.oc1.b"] = pack(sc + "output_conv1.weight"), f(sc + "output_conv1.bias")
        W["dpt.oc2.w"], W["dpt.oc2.b"] = pack(sc + "output_conv2.0.weight"), f(sc + "output_conv2.0.bias")
        W["dpt.oc3.w"], W["dpt.oc3.b"] = flat(sc + "output_conv2.2.weight"), f(sc + "output_conv2.2.bias")

    def init_random(self, seed: int = 0, depth: bool = False):
        """Synthetic weights of the configured shapes, generated tensor by tensor from one seeded generator (benchmarks and shape tests).
        The aggregator's and the camera head's are the same with and without `depth=True`: the depth head's are drawn after them."""
        g = torch.Generator().manual_seed(seed)
        if depth:
            self.cfg.check_depth_layers()
        shapes = expected_state_dict(self.cfg, depth)

        def get(k):
            s = shapes[k]
            if k.endswith(("norm.weight", "norm1.weight", "norm2.weight")):
                return 1.0 + 0.1 * torch.randn(s, generator=g)
            if k.endswith(".gamma"):
                return 0.3 + 0.05 * torch.randn(s, generator=g)
            if k.endswith(".weight") and len(s) >= 2:
                fan = int(np.prod(s[1:]))
                return torch.randn(s, generator=g) * fan ** -0.5
            if k.endswith("pose_branch.fc2.bias"):
                return torch.tensor([0.0] * 7 + [1.0, 1.0]) + 0.02 * torch.randn(s, generator=g)
            return 0.02 * torch.randn(s, generator=g) if not k.endswith(("token", "tokens")) else 0.5 * torch.randn(s, generator=g)
        return self._assemble(get, depth)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], depth: bool = False):
        """A state dict under the reference module's key names: the same rules as from_pretrained."""
        keep = consumed_header({k: {"shape": tuple(v.shape)} for k, v in sd.items()}, "state dict", depth)
        _raise_on(keep, self.cfg, "state dict", depth)
        return self._assemble(lambda k: sd[k], depth)

    @classmethod
    def from_pretrained(cls, folder: str, device="cuda:0", depth: bool = False):
        """`folder/model.safetensors` (+ an optional `config.json`; the defaults are the release).  The header is checked against
        expected_state_dict before a byte is uploaded: a missing key is a KeyError, an unexpected key or a wrong shape a ValueError.
        `depth=True` also loads the DPT depth head (`depth_head.*`, checked in the same way); without it those tensors are ignored."""
        from . import checkpoint
        cj = os.path.join(folder, "config.json")
        cfg = VGGTConfig.from_json(cj) if os.path.exists(cj) else VGGTConfig()
        path = os.path.join(folder, "model.safetensors")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{folder}: no model.safetensors")
        hdr, _ = checkpoint.read_header(path)
        keep = consumed_header({k: {"shape": tuple(int(v) for v in e["shape"])} for k, e in hdr.items()}, folder, depth)
        _raise_on(keep, cfg, folder, depth)
        sd = checkpoint.load_file(path, keep.keys())     # memory-mapped: a tensor's bytes are read when it is converted
        return cls(cfg, device)._assemble(lambda k: sd[k], depth)

    # ---- kernels ---------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _gemm(x, w, bias, out, epi, gate=None):
        from . import ops
        from ._ffi import call
        call("wf_gemm_bf16", x.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), out.data_ptr(),
             None if gate is None else gate.data_ptr(), x.shape[0], w.shape[0], w.shape[1], x.stride(0), w.stride(0), out.stride(0), epi, ops.stream())

    @staticmethod
    def _gemm32(x, w, bias, out, epi):
        from . import ops
        from ._ffi import call
        call("wf_gemm_f32", x.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), out.data_ptr(), x.shape[0], w.shape[0],
             w.shape[1], x.stride(0), w.stride(0), out.stride(0), epi, ops.stream())

    @staticmethod
    def _ln(x, w, b, out, eps):
        from . import ops
        from ._ffi import call
        call("wf_ln_modulate", x.data_ptr(), None if w is None else w.data_ptr(), None if b is None else b.data_ptr(), out.data_ptr(),
             WF_BF16 if out.dtype == torch.bfloat16 else WF_F32, x.shape[0], x.shape[1], float(eps), 1 if w is None else 0, ops.stream())

    def _block(self, x, name, nseq, L, heads, eps, rope, ws):
        """One pre-norm block with LayerScale on the fp32 residual stream x [nseq L, C], in place."""
        from . import ops
        from ._ffi import call
        W, st = self.W, ops.stream()
        M, C = x.shape
        n, qkv, att, hid, hb = ws["n"][:M], ws["qkv"][:M], ws["att"][:M], ws["hid"][:M], ws["hb"][:M]
        self._ln(x, W[f"{name}.norm1.w"], W[f"{name}.norm1.b"], n, eps)
        self._gemm(n, W[f"{name}.qkv.w"], W[f"{name}.qkv.b"], qkv, EPI_BF16)
        if rope is not None:
            cs, sn, pos, max_pos = rope
            call("wf_vit_qk_norm_rope", qkv.data_ptr(), qkv.data_ptr() + 2 * C, 3 * C, W[f"{name}.q_norm.w"].data_ptr(), W[f"{name}.q_norm.b"].data_ptr(),
                 W[f"{name}.k_norm.w"].data_ptr(), W[f"{name}.k_norm.b"].data_ptr(), 1e-5, cs.data_ptr(), sn.data_ptr(), max_pos, pos.data_ptr(),
                 nseq, L, heads, 1.0, st)
        call("wf_vit_attn_fwd", qkv.data_ptr(), qkv.data_ptr() + 2 * C, qkv.data_ptr() + 4 * C, 3 * C, att.data_ptr(), C, nseq, heads, L,
             0.125, st)
        self._gemm(att, W[f"{name}.proj.w"], W[f"{name}.proj.b"], x, EPI_RESID, W[f"{name}.ls1"])
        self._ln(x, W[f"{name}.norm2.w"], W[f"{name}.norm2.b"], n, eps)
        self._gemm(n, W[f"{name}.fc1.w"], W[f"{name}.fc1.b"], hid, EPI_F32)
        call("wf_act", hid.data_ptr(), WF_F32, None, WF_F32, hb.data_ptr(), WF_BF16, 1, hid.numel(), st)
        self._gemm(hb, W[f"{name}.fc2.w"], W[f"{name}.fc2.b"], x, EPI_RESID, W[f"{name}.ls2"])

    def _dino_base(self, gh: int, gw: int) -> torch.Tensor:
        """fp32 [5 + gh gw, C]: row 0 = cls + pos_0, rows 1..4 the registers (no position), then the position table interpolated to the
        grid (DINO:180-226: bicubic with antialias, offset 0; the table itself when the grid is the table's)."""
        if (gh, gw) not in self._pos_cache:
            cfg, W = self.cfg, self.W
            pos, M = W["pos"].cpu(), cfg.pos_grid
            patch = pos[1:]
            if (gh, gw) != (M, M):
                patch = torch.nn.functional.interpolate(patch.reshape(1, M, M, -1).permute(0, 3, 1, 2), size=(gh, gw), mode="bicubic",
                                                        antialias=True).permute(0, 2, 3, 1).reshape(gh * gw, -1)
            base = torch.cat([(W["cls"].cpu() + pos[0])[None], W["reg"].cpu(), patch], 0)
            self._pos_cache[(gh, gw)] = base.to(self.device).contiguous()
        return self._pos_cache[(gh, gw)]

    def _rope(self, gh: int, gw: int, frames: int):
        key = (gh, gw, frames)
        if key not in self._rope_cache:
            max_pos = max(gh, gw)
            cs, sn = rope_tables(max_pos, self.cfg.rope_freq)
            pos = token_positions(gh, gw, self.cfg.patch_start_idx, frames)
            self._rope_cache[key] = (cs.to(self.device), sn.to(self.device), pos.to(self.device), max_pos)
        return self._rope_cache[key]

    # ---- forward ---------------------------------------------------------------------------------------------------------------------------
    def _check_images(self, images: torch.Tensor) -> torch.Tensor:
        if not self.W:
            raise RuntimeError("VGGT has no weights: from_pretrained, load_state_dict or init_random first")
        if images.dim() == 4:
            images = images.unsqueeze(0)
        if images.dim() != 5 or images.shape[2] != 3 or images.dtype != torch.float32:
            raise ValueError(f"images must be float32 [S, 3, H, W] or [B, S, 3, H, W], got {images.dtype} {tuple(images.shape)}")
        if images.shape[0] < 1 or images.shape[1] < 1 or images.shape[3] % 14 or images.shape[4] % 14 or min(images.shape[3:]) < 14:
            raise ValueError(f"images {tuple(images.shape)}: at least one frame, H and W positive multiples of 14")
        return images

    def aggregate(self, images: torch.Tensor, keep=KEEP):
        """images fp32 [S, 3, H, W] or [B, S, 3, H, W] in [0, 1] -> ({layer: fp32 [B, S, 5 + P, 2 C]}, patch_start_idx); `keep="all"`
        returns every depth."""
        images = self._check_images(images)
        cfg = self.cfg
        layers = tuple(range(cfg.depth)) if isinstance(keep, str) and keep == "all" else tuple(int(k) for k in keep)
        if any(not 0 <= k < cfg.depth for k in layers):
            raise ValueError(f"keep {layers}: layers 0..{cfg.depth - 1} exist")
        per = [self._aggregate_one(images[b].to(self.device).contiguous(), layers) for b in range(images.shape[0])]
        return {k: torch.stack([p[k] for p in per], 0) for k in layers}, cfg.patch_start_idx

    def _aggregate_one(self, img: torch.Tensor, layers) -> Dict[int, torch.Tensor]:
        from . import ops
        from ._ffi import call
        cfg, W, dev, st = self.cfg, self.W, self.device, ops.stream()
        S, _, Hh, Ww = img.shape
        gh, gw = Hh // 14, Ww // 14
        P, C, F, R = gh * gw, cfg.embed_dim, cfg.hidden, cfg.patch_start_idx
        T = R + P
        M = S * T
        bf, f32 = torch.bfloat16, torch.float32
        ws = {"n": torch.empty(M, C, dtype=bf, device=dev), "qkv": torch.empty(M, 3 * C, dtype=bf, device=dev),
              "att": torch.empty(M, C, dtype=bf, device=dev), "hid": torch.empty(M, F, dtype=f32, device=dev),
              "hb": torch.empty(M, F, dtype=bf, device=dev)}
        rows = torch.empty(S * P, PATCH_K, dtype=bf, device=dev)
        call("wf_vit_patch_rows", img.data_ptr(), rows.data_ptr(), S, Hh, Ww, st)
        x = self._dino_base(gh, gw).unsqueeze(0).repeat(S, 1, 1)                    # [S, T, C]: a device copy
        for s in range(S):                                                          # patch rows += conv (+ bias) on top of the positions
            self._gemm(rows[s * P:(s + 1) * P], W["patch.w"], W["patch.b"], x[s, R:], EPI_F32_ACC)
        x = x.view(M, C)
        for i in range(cfg.dino_depth):
            self._block(x, f"d{i}", S, T, cfg.dino_num_heads, cfg.dino_eps, None, ws)
        xn = torch.empty(M, C, dtype=f32, device=dev)
        self._ln(x, W["dnorm.w"], W["dnorm.b"], xn, cfg.dino_eps)
        idx = torch.tensor([0] + [1] * (S - 1), device=dev)
        tok = torch.cat([W["cam_tok"][idx].unsqueeze(1), W["reg_tok"][idx], xn.view(S, T, C)[:, R:]], 1).contiguous().view(M, C)
        rope_f, rope_g = self._rope(gh, gw, 1), self._rope(gh, gw, S)
        out: Dict[int, torch.Tensor] = {}
        for i in range(cfg.depth):
            self._block(tok, f"f{i}", S, T, cfg.num_heads, 1e-5, rope_f, ws)
            fr = tok.clone() if i in layers else None
            self._block(tok, f"g{i}", 1, M, cfg.num_heads, 1e-5, rope_g, ws)
            if i in layers:
                out[i] = torch.cat([fr.view(S, T, C), tok.view(S, T, C)], -1)
            if i == max(layers):
                break
        return out

    def camera_from_tokens(self, tokens: torch.Tensor, num_iterations: Optional[int] = None) -> torch.Tensor:
        """The camera head on the last kept layer's tokens fp32 [B, S, T, 2 C] -> pose_enc fp32 [B, S, 9] of the last iteration."""
        from . import ops
        from ._ffi import call
        cfg, W, dev, st = self.cfg, self.W, self.device, ops.stream()
        if not W:
            raise RuntimeError("VGGT has no weights: from_pretrained, load_state_dict or init_random first")
        n_it = cfg.camera_iterations if num_iterations is None else int(num_iterations)
        B, S, _, D = tokens.shape
        if D != cfg.camera_dim or tokens.dtype != torch.float32 or n_it < 1:
            raise ValueError(f"tokens must be float32 [B, S, T, {cfg.camera_dim}] and num_iterations >= 1, got {tokens.dtype} {tuple(tokens.shape)}")
        if S > MAX_FRAMES:
            raise NotImplementedError(f"{S} frames: wf_clip_attn_fwd over the camera tokens takes at most {MAX_FRAMES}")
        Hc, f32 = cfg.camera_num_heads, torch.float32
        hd = D // Hc
        e = lambda *s: torch.empty(*s, dtype=f32, device=dev)  # noqa: E731
        res = []
        for bi in range(B):
            pose = e(S, D)
            self._ln(tokens[bi, :, 0].to(dev).contiguous(), W["token_norm.w"], W["token_norm.b"], pose, 1e-5)
            a = e(S, D)
            self._ln(pose, None, None, a, 1e-6)                                     # adaln_norm: no affine
            pred = None
            inp, emb, mod, n, qkv, att, hid, h2, d12 = torch.zeros(S, 12, dtype=f32, device=dev), e(S, D), e(S, 3 * D), e(S, D), e(S, 3 * D), \
                e(S, D), e(S, 4 * D), e(S, D // 2), e(S, 12)
            for _ in range(n_it):
                inp[:, :9] = W["empty_pose"] if pred is None else pred
                self._gemm32(inp, W["embed.w"], W["embed.b"], emb, EPI_F32)
                self._gemm32(torch.nn.functional.silu(emb), W["mod.w"], W["mod.b"], mod, EPI_F32)
                shift, scale, gate = mod.chunk(3, -1)
                y = (gate * (a * (1 + scale) + shift) + pose).contiguous()
                for i in range(cfg.camera_trunk_depth):
                    c = f"c{i}"
                    self._ln(y, W[f"{c}.norm1.w"], W[f"{c}.norm1.b"], n, 1e-5)
                    self._gemm32(n, W[f"{c}.qkv.w"], W[f"{c}.qkv.b"], qkv, EPI_F32)
                    call("wf_clip_attn_fwd", qkv.data_ptr(), qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, att.data_ptr(), D, Hc, S, hd,
                         float(hd) ** -0.5, st)
                    self._gemm32(att, W[f"{c}.proj.w"], W[f"{c}.proj.b"], y, EPI_F32_ACC)
                    self._ln(y, W[f"{c}.norm2.w"], W[f"{c}.norm2.b"], n, 1e-5)
                    self._gemm32(n, W[f"{c}.fc1.w"], W[f"{c}.fc1.b"], hid, EPI_F32_GELU)
                    self._gemm32(hid, W[f"{c}.fc2.w"], W[f"{c}.fc2.b"], y, EPI_F32_ACC)
                self._ln(y, W["trunk_norm.w"], W["trunk_norm.b"], n, 1e-5)
                self._gemm32(n, W["pb1.w"], W["pb1.b"], h2, EPI_F32_GELU)
                self._gemm32(h2, W["pb2.w"], W["pb2.b"], d12, EPI_F32)
                pred = d12[:, :9].clone() if pred is None else pred + d12[:, :9]
            res.append(torch.cat([pred[:, :7], torch.relu(pred[:, 7:])], -1))
        return torch.stack(res, 0)

    def camera(self, images: torch.Tensor, num_iterations: Optional[int] = None) -> torch.Tensor:
        """images -> pose_enc fp32 [B, S, 9] (absT_quaR_FoV) of the last iteration."""
        last = self.cfg.depth - 1
        toks, _ = self.aggregate(images, keep=(last,))
        return self.camera_from_tokens(toks[last], num_iterations)

    def cameras(self, images: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """images -> (extrinsic fp32 [B, S, 3, 4], intrinsic fp32 [B, S, 3, 3]) in pixels of the images' own size."""
        images = self._check_images(images)
        return pose_encoding_to_extri_intri(self.camera(images), tuple(images.shape[-2:]))

    # ---- the DPT depth head ----------------------------------------------------------------------------------------------------------------
    def _need_depth(self):
        if not self.W:
            raise RuntimeError("VGGT has no weights: from_pretrained, load_state_dict or init_random first")
        if not self.has_depth:
            raise RuntimeError("this VGGT was loaded without the depth head: load it with depth=True "
                               "(from_pretrained / load_state_dict / init_random)")

    def _conv(self, x, name, stride=1, relu_in=False, resid=None, relu_resid=False, relu_out=False):
        """wf_conv2d_f32 on a contiguous channels-last map x f32 [n, Hi, Wi, Cin] with the packed weight `name`.w (and `name`.b if any)."""
        from . import ops
        from ._ffi import call
        w, b = self.W[name + ".w"], self.W.get(name + ".b")
        n, Hi, Wi, Cin = x.shape
        out = torch.empty(n, (Hi - 1) // stride + 1, (Wi - 1) // stride + 1, w.shape[2], dtype=torch.float32, device=self.device)
        call("wf_conv2d_f32", x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), None if resid is None else resid.data_ptr(),
             out.data_ptr(), n, Hi, Wi, Cin, w.shape[2], stride, int(relu_in), int(relu_resid), int(relu_out), ops.stream())
        return out

    def _resize(self, x, Ho, Wo, tables=None):
        from . import ops
        from ._ffi import call
        n, Hi, Wi, C = x.shape
        out = torch.empty(n, Ho, Wo, C, dtype=torch.float32, device=self.device)
        col, row = tables if tables is not None else (None, None)
        call("wf_resize_bilinear_cl_f32", x.data_ptr(), out.data_ptr(), n, Hi, Wi, Ho, Wo, C, None if col is None else col.data_ptr(),
             None if row is None else row.data_ptr(), ops.stream())
        return out

    def _dpt_tables(self, C, h, w, image_hw, expanded=False):
        """The position tables on the device, cached per shape; `expanded`: the addend of a patch grid as rows f32 [h w, C]."""
        key = (C, h, w, tuple(image_hw), expanded)
        if key not in self._dpt_cache:
            if expanded:
                self._dpt_cache[key] = (dpt_pos_embed(C, h, w, image_hw).permute(1, 2, 0).reshape(h * w, C).contiguous().to(self.device),)
            else:
                self._dpt_cache[key] = tuple(t.to(self.device) for t in dpt_pos_tables(C, h, w, image_hw))
        return self._dpt_cache[key]

    def _rcu(self, x, name):
        """ResidualConvUnit (DPT:366-386) with its in-place ReLU: conv2(relu(conv1(relu(x)))) + relu(x)."""
        t = self._conv(x, name + ".c1", relu_in=True)
        return self._conv(t, name + ".c2", relu_in=True, resid=x, relu_resid=True)

    def _fuse(self, out, skip, name, size):
        """FeatureFusionBlock (DPT:432-456); the 1x1 out_conv runs before the resize (see the module docstring)."""
        if skip is not None:
            out = out + self._rcu(skip, name + ".rcu1")
        out = self._rcu(out, name + ".rcu2")
        n, h, w, f = out.shape
        o = torch.empty(n * h * w, f, dtype=torch.float32, device=self.device)
        self._gemm32(out.view(n * h * w, f), self.W[name + ".out.w"], self.W[name + ".out.b"], o, EPI_F32)
        return self._resize(o.view(n, h, w, f), size[0], size[1])

    def _depth_chunk(self, xs, gh, gw, image_hw, depth_out, conf_out):
        """DPT._forward_impl on n frames: xs = the four kept layers' patch tokens [n, P, 2 C] -> depth_out / conf_out f32 [n, H, W]."""
        from . import ops
        from ._ffi import call
        cfg, W, dev, f32 = self.cfg, self.W, self.device, torch.float32
        n, P, D = xs[0].shape
        maps = []
        for i, oc in enumerate(cfg.depth_out_channels):
            x = xs[i].to(dev).reshape(n * P, D).contiguous()
            xn = torch.empty_like(x)
            self._ln(x, W["dpt.norm.w"], W["dpt.norm.b"], xn, 1e-5)
            y = self._dpt_tables(oc, gh, gw, image_hw, expanded=True)[0].repeat(n, 1)       # the projection lands on top of the positions
            self._gemm32(xn, W[f"dpt.proj{i}.w"], W[f"dpt.proj{i}.b"], y, EPI_F32_ACC)
            if i < 2:                                                                     # ConvTranspose, kernel = stride = s
                s = 4 if i == 0 else 2
                g = torch.empty(n * P, s * s * oc, dtype=f32, device=dev)
                self._gemm32(y, W[f"dpt.up{i}.w"], W[f"dpt.up{i}.b"], g, EPI_F32)
                m = g.view(n, gh, gw, s, s, oc).permute(0, 1, 3, 2, 4, 5).reshape(n, gh * s, gw * s, oc).contiguous()
            elif i == 2:
                m = y.view(n, gh, gw, oc)
            else:
                m = self._conv(y.view(n, gh, gw, oc), "dpt.down", stride=2)
            maps.append(self._conv(m, f"dpt.rn{i}"))
        l1, l2, l3, l4 = maps
        out = self._fuse(l4, None, "dpt.ref4", l3.shape[1:3])
        out = self._fuse(out, l3, "dpt.ref3", l2.shape[1:3])
        out = self._fuse(out, l2, "dpt.ref2", l1.shape[1:3])
        out = self._fuse(out, l1, "dpt.ref1", (2 * l1.shape[1], 2 * l1.shape[2]))
        out = self._conv(out, "dpt.oc1")
        out = self._resize(out, 14 * gh, 14 * gw, self._dpt_tables(out.shape[3], 14 * gh, 14 * gw, image_hw))
        out = self._conv(out, "dpt.oc2", relu_out=True)
        call("wf_dpt_depth_out", out.data_ptr(), W["dpt.oc3.w"].data_ptr(), W["dpt.oc3.b"].data_ptr(), depth_out.data_ptr(), conf_out.data_ptr(),
             n * 14 * gh * 14 * gw, out.shape[3], ops.stream())

    def depth_from_tokens(self, tokens: Dict[int, torch.Tensor], image_hw: Tuple[int, int], frames_chunk_size: Optional[int] = 8,
                          layers: Optional[Sequence[int]] = None):
        """The depth head on the kept layers {layer: fp32 [B, S, 5 + P, 2 C]} of images of size image_hw -> (depth fp32 [B, S, H, W, 1],
        depth_conf fp32 [B, S, H, W]).  Frames are processed in chunks of frames_chunk_size (None: all at once; DPT:139-170); the result
        does not depend on the chunk size, bit for bit.  `layers`: the four keys of `tokens` in the head's order (default: the
        configuration's depth_layers, the keys aggregate() returns)."""
        self._need_depth()
        cfg, dev = self.cfg, self.device
        H, W = (int(v) for v in image_hw)
        if H < 14 or W < 14 or H % 14 or W % 14:
            raise ValueError(f"image_hw {(H, W)}: H and W are positive multiples of 14")
        gh, gw, R = H // 14, W // 14, cfg.patch_start_idx
        layers = tuple(cfg.depth_layers if layers is None else layers)
        missing = [k for k in layers if k not in tokens]
        if missing or len(layers) != 4:
            raise ValueError(f"depth_from_tokens: four layers are needed, {missing} of {list(layers)} are not in the tokens")
        B, S = tokens[layers[0]].shape[:2]
        for k in layers:
            t = tokens[k]
            if t.dtype != torch.float32 or tuple(t.shape) != (B, S, R + gh * gw, cfg.camera_dim):
                raise ValueError(f"tokens[{k}] must be float32 {(B, S, R + gh * gw, cfg.camera_dim)}, got {t.dtype} {tuple(t.shape)}")
        if frames_chunk_size is not None and int(frames_chunk_size) < 1:
            raise ValueError(f"frames_chunk_size {frames_chunk_size}: at least 1, or None")
        chunk = S if frames_chunk_size is None else min(int(frames_chunk_size), S)
        depth = torch.empty(B, S, H, W, dtype=torch.float32, device=dev)
        conf = torch.empty(B, S, H, W, dtype=torch.float32, device=dev)
        for b in range(B):
            for s0 in range(0, S, chunk):
                s1 = min(s0 + chunk, S)
                self._depth_chunk([tokens[k][b, s0:s1, R:] for k in layers], gh, gw, (H, W), depth[b, s0:s1], conf[b, s0:s1])
        return depth.unsqueeze(-1), conf

    def depth(self, images: torch.Tensor, frames_chunk_size: Optional[int] = 8) -> Tuple[torch.Tensor, torch.Tensor]:
        """images -> (depth fp32 [B, S, H, W, 1], depth_conf fp32 [B, S, H, W]): aggregate + depth head."""
        self._need_depth()
        images = self._check_images(images)
        toks, _ = self.aggregate(images, keep=self.cfg.depth_layers)
        return self.depth_from_tokens(toks, tuple(images.shape[-2:]), frames_chunk_size)

    def predict(self, images: torch.Tensor, frames_chunk_size: Optional[int] = 8) -> Dict[str, torch.Tensor]:
        """images -> {pose_enc, extrinsic, intrinsic, depth, depth_conf}: ONE aggregator pass serves the camera head and the depth head."""
        self._need_depth()
        images = self._check_images(images)
        last, hw = self.cfg.depth - 1, tuple(images.shape[-2:])
        toks, _ = self.aggregate(images, keep=tuple(self.cfg.depth_layers) + (last,))
        pose = self.camera_from_tokens(toks[last])
        ext, intr = pose_encoding_to_extri_intri(pose, hw)
        depth, conf = self.depth_from_tokens(toks, hw, frames_chunk_size)
        return {"pose_enc": pose, "extrinsic": ext, "intrinsic": intr, "depth": depth, "depth_conf": conf}


def main(argv=None) -> int:
    import argparse
    from PIL import Image
    ap = argparse.ArgumentParser(prog="python -m worldforge_amd.vggt", description="images in, cameras out (VGGT aggregator + camera head)")
    ap.add_argument("--checkpoint", required=True, help="folder with model.safetensors (+ optional config.json)")
    ap.add_argument("--images", nargs="+", required=True)
    ap.add_argument("--out", required=True, help="npz: pose_enc, extrinsic, intrinsic, image_size_hw")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--depth", action="store_true", help="load the DPT depth head too and add depth [1, S, H, W, 1], depth_conf [1, S, H, W] to the npz")
    a = ap.parse_args(argv)
    x = preprocess_device([Image.open(p) for p in a.images], a.device)
    model = VGGT.from_pretrained(a.checkpoint, device=a.device, depth=a.depth)
    extra = {}
    if a.depth:
        r = model.predict(x)
        pose, ext, intr = r["pose_enc"], r["extrinsic"], r["intrinsic"]
        extra = {"depth": r["depth"].cpu().numpy(), "depth_conf": r["depth_conf"].cpu().numpy()}
    else:
        pose = model.camera(x)
        ext, intr = pose_encoding_to_extri_intri(pose, tuple(x.shape[-2:]))
    np.savez(a.out, pose_enc=pose.cpu().numpy(), extrinsic=ext.cpu().numpy(), intrinsic=intr.cpu().numpy(),
             image_size_hw=np.array(x.shape[-2:], dtype=np.int64), **extra)
    print(f"{len(a.images)} images {tuple(x.shape[-2:])} -> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
