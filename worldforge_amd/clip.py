"""The CLIP vision encoder on this engine's own kernels, in float32: an image in, `hidden_states[-2]` out.

What the reference loads as `CLIPVisionModel.from_pretrained(..., subfolder="image_encoder", torch_dtype=torch.float32)` (INFER:179-182;
HF = transformers/models/clip/modeling_clip.py) and calls once per video (PIPE:207-211: `hidden_states[-2]`, cast to bf16 afterwards).
The reference runs this model in fp32, so this encoder is an fp32 encoder: every product is wf_gemm_f32 / wf_clip_attn_fwd on the
fp32-input MFMA (csrc/clip.hip), the residual stream, the LayerNorms and the softmax are fp32, nothing is narrower anywhere.

    rows = wf_clip_patch_rows(pixel_values)                          [(S/p)^2, 3 p^2] in the conv weight's flattening order
    x    = pos' ; x[1:] += wf_gemm_f32(rows, patch weight)           pos' = position table with class_embedding added to row 0 at load
    x    = wf_ln_modulate(x, pre_layrnorm)                           (affine LayerNorm: plus_one = 0, fp32 out)
    per layer, num_hidden_layers - 1 of them:
    n    = wf_ln_modulate(x, layer_norm1)
    qkv  = wf_gemm_f32(n, [q; k; v], bias)                           ONE stacked [3 hidden, hidden] product
    a    = wf_clip_attn_fwd(q, k, v, scale = head_dim ** -0.5)
    x   += wf_gemm_f32(a, out_proj, bias)        WF_EPI_F32_ACC
    n    = wf_ln_modulate(x, layer_norm2)
    h    = wf_gemm_f32(n, fc1, bias)             WF_EPI_F32_GELU / _QUICK_GELU
    x   += wf_gemm_f32(h, fc2, bias)             WF_EPI_F32_ACC

`hidden_states[-2]` is the residual stream after num_hidden_layers - 1 layers, without `post_layernorm`: the last layer and the final
norm are checked in the checkpoint and never uploaded.  `preprocess` restates CLIPImageProcessor's PIL path on the host; `preprocess_device`
gives the same bits on the device (ops.resample_u8_window) and is what `encode_image` uses.
Not built: position interpolation (the image must have the configured size), batches, the text tower, the projection heads.
"""
from __future__ import annotations

import json
import os
import warnings
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._ffi import call

WF_F32 = 0
WF_EPI_F32, WF_EPI_F32_ACC, WF_EPI_F32_GELU, WF_EPI_F32_QUICK_GELU = 2, 4, 5, 6
ACTIVATIONS = {"gelu": WF_EPI_F32_GELU, "quick_gelu": WF_EPI_F32_QUICK_GELU}
MAX_TOKENS = 1024         # wf_clip_attn_fwd
PREFIX = "vision_model."
DROPPED = ("text_model.", "visual_projection.", "text_projection.", "logit_scale")   # the rest of a full CLIPModel file
POSITION_IDS = "embeddings.position_ids"   # a buffer older files carry: accepted, never read


@dataclass(frozen=True)
class CLIPVisionConfig:
    hidden_size: int = 1280
    intermediate_size: int = 5120
    num_hidden_layers: int = 32
    num_attention_heads: int = 16
    image_size: int = 224
    patch_size: int = 14
    hidden_act: str = "gelu"
    layer_norm_eps: float = 1e-5

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    @property
    def num_tokens(self) -> int:
        return (self.image_size // self.patch_size) ** 2 + 1

    @property
    def patch_dim(self) -> int:
        return 3 * self.patch_size ** 2

    @classmethod
    def from_dict(cls, d: dict) -> "CLIPVisionConfig":
        d = d.get("vision_config", d) if isinstance(d.get("vision_config"), dict) else d     # a full CLIPConfig nests it
        if d.get("num_channels", 3) != 3:
            raise NotImplementedError(f"num_channels {d['num_channels']}: the patch embedding is built for RGB")
        cfg = cls(**{k: d[k] for k in cls.__dataclass_fields__ if k in d})
        if cfg.hidden_act not in ACTIVATIONS:
            raise NotImplementedError(f"hidden_act {cfg.hidden_act!r}: built are {sorted(ACTIVATIONS)}")
        if min(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.image_size, cfg.patch_size) < 1:
            raise ValueError("sizes must be positive")
        if cfg.hidden_size % cfg.num_attention_heads:
            raise ValueError(f"hidden_size {cfg.hidden_size} is no multiple of num_attention_heads {cfg.num_attention_heads}")
        if cfg.head_dim % 8 or not 8 <= cfg.head_dim <= 128:
            raise NotImplementedError(f"head width {cfg.head_dim}: wf_clip_attn_fwd takes multiples of 8 in 8..128")
        if cfg.hidden_size % 4 or cfg.intermediate_size % 4 or cfg.patch_dim % 4:
            raise ValueError(f"hidden_size {cfg.hidden_size}, intermediate_size {cfg.intermediate_size} and 3 * patch_size^2 = {cfg.patch_dim} "
                             "must be multiples of 4 (wf_gemm_f32)")
        if cfg.image_size % cfg.patch_size:
            raise ValueError(f"image_size {cfg.image_size} is no multiple of patch_size {cfg.patch_size}")
        if cfg.num_tokens > MAX_TOKENS:
            raise NotImplementedError(f"{cfg.num_tokens} tokens: wf_clip_attn_fwd takes at most {MAX_TOKENS}")
        return cfg

    @classmethod
    def from_json(cls, path: str) -> "CLIPVisionConfig":
        with open(path) as f:
            return cls.from_dict(json.load(f))


def expected_state_dict(cfg: CLIPVisionConfig) -> Dict[str, Tuple[int, ...]]:
    """{HF key without the `vision_model.` prefix: shape} of a CLIPVisionModel: every layer and `post_layernorm` included (the loader
    checks them all and uploads what `hidden_states[-2]` needs)."""
    C, F, p = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size
    out: Dict[str, Tuple[int, ...]] = {"embeddings.class_embedding": (C,), "embeddings.patch_embedding.weight": (C, 3, p, p),
                                       "embeddings.position_embedding.weight": (cfg.num_tokens, C),
                                       "pre_layrnorm.weight": (C,), "pre_layrnorm.bias": (C,)}
    for i in range(cfg.num_hidden_layers):
        b = f"encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[f"{b}self_attn.{n}.weight"], out[f"{b}self_attn.{n}.bias"] = (C, C), (C,)
        for n in ("layer_norm1", "layer_norm2"):
            out[f"{b}{n}.weight"], out[f"{b}{n}.bias"] = (C,), (C,)
        out[f"{b}mlp.fc1.weight"], out[f"{b}mlp.fc1.bias"] = (F, C), (F,)
        out[f"{b}mlp.fc2.weight"], out[f"{b}mlp.fc2.bias"] = (C, F), (C,)
    out["post_layernorm.weight"], out["post_layernorm.bias"] = (C,), (C,)
    return out


def consumed_header(found: Dict[str, dict]) -> Tuple[Dict[str, dict], int, Dict[str, str]]:
    """The entries of a checkpoint header the vision encoder looks at, under their names WITHOUT the `vision_model.` prefix (released
    files carry it, files written by a bare CLIPVisionModel of recent `transformers` do not): the text tower, the projections and
    `logit_scale` of a full CLIPModel file dropped, the `position_ids` buffer dropped -> (entries, number dropped, {name: key in file})."""
    keep, names, dropped = {}, {}, 0
    for k, v in found.items():
        if k.startswith(DROPPED):
            dropped += 1
            continue
        n = k[len(PREFIX):] if k.startswith(PREFIX) else k
        if n == POSITION_IDS:
            continue
        keep[n], names[n] = v, k
    return keep, dropped, names


def uploaded_keys(cfg: CLIPVisionConfig, n_layers: Optional[int] = None):
    """The keys whose bytes go to the device: everything but the layers from `n_layers` (default num_hidden_layers - 1) on and post_layernorm."""
    n = cfg.num_hidden_layers - 1 if n_layers is None else n_layers
    skip = tuple(f"encoder.layers.{i}." for i in range(n, cfg.num_hidden_layers)) + ("post_layernorm.",)
    return [k for k in expected_state_dict(cfg) if not k.startswith(skip)]


class CLIPVisionModel:
    def __init__(self, cfg: CLIPVisionConfig, device="cuda:0"):
        self.cfg = cfg
        self.device = torch.device(device)
        self.W: Dict[str, torch.Tensor] = {}
        self.n_layers = cfg.num_hidden_layers - 1

    # ---- weights -----------------------------------------------------------------------------------------------------------------------
    def _assemble(self, get):
        """get(key without prefix) -> the CPU tensor.  Everything becomes fp32 on the device (`torch_dtype=torch.float32`); q, k, v are
        stacked; class_embedding is added to row 0 of the position table once (the same fp32 addition HF does per call)."""
        cfg, dev = self.cfg, self.device
        f = lambda k: get(k).to(torch.float32).to(dev).contiguous()  # noqa: E731
        pos = f("embeddings.position_embedding.weight").clone()
        pos[0] += f("embeddings.class_embedding")
        W = {"pos": pos, "patch": f("embeddings.patch_embedding.weight").reshape(cfg.hidden_size, cfg.patch_dim).contiguous(),
             "pre.w": f("pre_layrnorm.weight"), "pre.b": f("pre_layrnorm.bias")}
        for i in range(self.n_layers):
            b = f"encoder.layers.{i}."
            W[f"{i}.qkv.w"] = torch.cat([f(f"{b}self_attn.{n}_proj.weight") for n in "qkv"], 0).contiguous()
            W[f"{i}.qkv.b"] = torch.cat([f(f"{b}self_attn.{n}_proj.bias") for n in "qkv"], 0).contiguous()
            W[f"{i}.o.w"], W[f"{i}.o.b"] = f(f"{b}self_attn.out_proj.weight"), f(f"{b}self_attn.out_proj.bias")
            for j, n in ((1, "layer_norm1"), (2, "layer_norm2")):
                W[f"{i}.ln{j}.w"], W[f"{i}.ln{j}.b"] = f(f"{b}{n}.weight"), f(f"{b}{n}.bias")
            W[f"{i}.fc1.w"], W[f"{i}.fc1.b"] = f(f"{b}mlp.fc1.weight"), f(f"{b}mlp.fc1.bias")
            W[f"{i}.fc2.w"], W[f"{i}.fc2.b"] = f(f"{b}mlp.fc2.weight"), f(f"{b}mlp.fc2.bias")
        self.W = W
        return self

    def init_random(self, seed: int = 0):
        """Synthetic fp32 weights of the right shapes, generated on the device (benchmarks: there are no checkpoints offline)."""
        cfg, dev = self.cfg, self.device
        g = torch.Generator(device=dev).manual_seed(seed)
        C, F = cfg.hidden_size, cfg.intermediate_size
        rn = lambda *s, std=1.0, base=0.0: torch.randn(*s, generator=g, device=dev, dtype=torch.float32) * std + base  # noqa: E731
        W = {"pos": rn(cfg.num_tokens, C, std=0.02), "patch": rn(C, cfg.patch_dim, std=cfg.patch_dim ** -0.5), "pre.w": rn(C, std=0.1, base=1.0),
             "pre.b": rn(C, std=0.02)}
        for i in range(self.n_layers):
            W[f"{i}.qkv.w"], W[f"{i}.qkv.b"] = rn(3 * C, C, std=C ** -0.5), rn(3 * C, std=0.02)
            W[f"{i}.o.w"], W[f"{i}.o.b"] = rn(C, C, std=C ** -0.5), rn(C, std=0.02)
            for j in (1, 2):
                W[f"{i}.ln{j}.w"], W[f"{i}.ln{j}.b"] = rn(C, std=0.1, base=1.0), rn(C, std=0.02)
            W[f"{i}.fc1.w"], W[f"{i}.fc1.b"] = rn(F, C, std=C ** -0.5), rn(F, std=0.02)
            W[f"{i}.fc2.w"], W[f"{i}.fc2.b"] = rn(C, F, std=F ** -0.5), rn(C, std=0.02)
        self.W = W
        return self

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        """An HF state dict (tests): the same key rules as from_pretrained."""
        keep, dropped, names = consumed_header({k: {"shape": tuple(v.shape)} for k, v in sd.items()})
        _raise_on(keep, self.cfg, "state dict", dropped)
        return self._assemble(lambda k: sd[names[k]])

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0", subfolder: Optional[str] = "image_encoder"):
        """`<path>/<subfolder>/config.json` (or `path` itself when it is the encoder's folder) + one safetensors file or an index with
        shards.  The headers are checked against expected_state_dict before a byte is uploaded: a missing key is a KeyError, an
        unexpected key or a wrong shape a ValueError; the rest of a full CLIPModel file is ignored with one warning.  The last encoder
        layer and post_layernorm are checked and never read."""
        from . import checkpoint
        folder = os.path.join(path, subfolder) if subfolder and os.path.isdir(os.path.join(path, subfolder)) else path
        cj = os.path.join(folder, "config.json")
        if not os.path.exists(cj):
            raise FileNotFoundError(f"{folder}: no config.json")
        cfg = CLIPVisionConfig.from_json(cj)
        found, info = checkpoint.dir_header(folder)
        if info["missing_shards"]:
            raise FileNotFoundError(f"{folder}: shards named by {info['index']} are missing: {info['missing_shards']}")
        keep, dropped, names = consumed_header(found)
        _raise_on(keep, cfg, folder, dropped)
        model = cls(cfg, device)
        sd = checkpoint.load_dir(folder)   # memory-mapped: a tensor's bytes are read when it is converted
        return model._assemble(lambda k: sd[names[k]])

    # ---- forward -----------------------------------------------------------------------------------------------------------------------
    def _gemm(self, x, w, bias, out, epi):
        M, K = x.shape
        call("wf_gemm_f32", x.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), out.data_ptr(), M, w.shape[0], K,
             x.stride(0), w.stride(0), out.stride(0), epi, ops.stream())

    def _ln(self, x, w, b, out):
        call("wf_ln_modulate", x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), WF_F32, x.shape[0], x.shape[1],
             float(self.cfg.layer_norm_eps), 0, ops.stream())

    def __call__(self, pixel_values: torch.Tensor, hidden_state_index: int = -2) -> torch.Tensor:
        """pixel_values fp32 [3, S, S] or [1, 3, S, S], S = image_size -> hidden_states[hidden_state_index] fp32 [tokens, hidden].
        Refused before any device work (ValueError): another shape or dtype, an index behind the layers that were uploaded."""
        if not self.W:
            raise RuntimeError("CLIPVisionModel has no weights: from_pretrained or load_state_dict first")
        cfg, dev, W = self.cfg, self.device, self.W
        S, C, F, H, T = cfg.image_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_tokens
        px = pixel_values
        if px.dim() == 4 and px.shape[0] == 1:
            px = px[0]
        if px.dtype != torch.float32 or tuple(px.shape) != (3, S, S):
            raise ValueError(f"pixel_values must be float32 [3, {S}, {S}] or [1, 3, {S}, {S}] (no position interpolation, batch 1), got "
                             f"{pixel_values.dtype} {tuple(pixel_values.shape)}")
        n_run = hidden_state_index if hidden_state_index >= 0 else cfg.num_hidden_layers + 1 + hidden_state_index
        if not 0 <= n_run <= self.n_layers:
            raise ValueError(f"hidden_state_index {hidden_state_index}: hidden states 0..{self.n_layers} are available (the layers behind "
                             "hidden_states[-2] are not uploaded)")
        st, f32 = ops.stream(), torch.float32
        px = px.to(dev).contiguous()
        rows = torch.empty(T - 1, cfg.patch_dim, dtype=f32, device=dev)
        e = torch.empty(T, C, dtype=f32, device=dev)
        x = torch.empty(T, C, dtype=f32, device=dev)
        n = torch.empty(T, C, dtype=f32, device=dev)
        qkv = torch.empty(T, 3 * C, dtype=f32, device=dev)
        att = torch.empty(T, C, dtype=f32, device=dev)
        hdn = torch.empty(T, F, dtype=f32, device=dev)
        call("wf_clip_patch_rows", px.data_ptr(), rows.data_ptr(), S, cfg.patch_size, st)
        e.copy_(W["pos"])                                                          # [class + pos 0; pos 1..]: a device copy
        self._gemm(rows, W["patch"], None, e[1:], WF_EPI_F32_ACC)                  # rows 1.. += patch embedding (the conv has no bias)
        self._ln(e, W["pre.w"], W["pre.b"], x)
        act, scale = ACTIVATIONS[cfg.hidden_act], float(cfg.head_dim) ** -0.5
        for i in range(n_run):
            self._ln(x, W[f"{i}.ln1.w"], W[f"{i}.ln1.b"], n)
            self._gemm(n, W[f"{i}.qkv.w"], W[f"{i}.qkv.b"], qkv, WF_EPI_F32)
            call("wf_clip_attn_fwd", qkv.data_ptr(), qkv.data_ptr() + 4 * C, qkv.data_ptr() + 8 * C, 3 * C, att.data_ptr(), C, H, T,
                 cfg.head_dim, scale, st)
            self._gemm(att, W[f"{i}.o.w"], W[f"{i}.o.b"], x, WF_EPI_F32_ACC)
            self._ln(x, W[f"{i}.ln2.w"], W[f"{i}.ln2.b"], n)
            self._gemm(n, W[f"{i}.fc1.w"], W[f"{i}.fc1.b"], hdn, act)
            self._gemm(hdn, W[f"{i}.fc2.w"], W[f"{i}.fc2.b"], x, WF_EPI_F32_ACC)
        return x


def _raise_on(keep: Dict[str, dict], cfg: CLIPVisionConfig, where: str, dropped: int):
    from .checkpoint import compare_header
    if dropped:
        warnings.warn(f"{where}: {dropped} text_model.* / projection / logit_scale tensors are not part of the vision encoder and are ignored",
                      UserWarning, stacklevel=3)
    missing, unexpected, wrong = compare_header(keep, expected_state_dict(cfg))
    if missing:
        raise KeyError(f"{where}: {len(missing)} parameters of the vision encoder are not in the checkpoint: {missing[:5]}")
    if wrong:
        w = wrong[0]
        raise ValueError(f"{where}: {len(wrong)} parameters have the wrong shape: {w['key']} is {w['found']}, expected {w['expected']}")
    if unexpected:
        raise ValueError(f"{where}: {len(unexpected)} checkpoint tensors are not consumed by the vision encoder: {unexpected[:5]}")


# ---- CLIPImageProcessor's PIL path on the host -------------------------------------------------------------------------------------------
_PIL_RESAMPLE = {0: "NEAREST", 1: "LANCZOS", 2: "BILINEAR", 3: "BICUBIC", 4: "BOX", 5: "HAMMING"}


def _processor_settings(c: dict):
    """The checks of preprocess / preprocess_device on a preprocessor_config -> (shortest edge, crop S, resample code, mean, std, rescale)."""
    for flag in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
        if not c.get(flag, True):
            raise NotImplementedError(f"preprocessor_config {flag}=false is not implemented")
    if not c.get("do_convert_rgb", True):
        raise NotImplementedError("preprocessor_config do_convert_rgb=false is not implemented")
    if c.get("do_pad"):
        raise NotImplementedError("preprocessor_config do_pad is not implemented")
    size = c.get("size", {"shortest_edge": 224})
    size = {"shortest_edge": size} if isinstance(size, int) else size
    if set(size) != {"shortest_edge"}:
        raise NotImplementedError(f"preprocessor_config size {size}: only a shortest_edge is implemented")
    crop = c.get("crop_size", {"height": 224, "width": 224})
    crop = {"height": crop, "width": crop} if isinstance(crop, int) else crop
    if set(crop) != {"height", "width"} or crop["height"] != crop["width"]:
        raise NotImplementedError(f"preprocessor_config crop_size {crop}: a square height / width is implemented")
    resample = int(c.get("resample", 3))
    if resample not in _PIL_RESAMPLE:
        raise NotImplementedError(f"preprocessor_config resample {resample} is no PIL filter")
    mean, std = c.get("image_mean"), c.get("image_std")
    if mean is None or std is None or len(mean) != 3 or len(std) != 3:
        raise NotImplementedError("preprocessor_config needs image_mean and image_std of 3 values")
    return size["shortest_edge"], int(crop["height"]), resample, mean, std, float(c.get("rescale_factor", 1 / 255))


def _resized_and_window(w: int, h: int, shortest_edge, S: int):
    """The shortest-edge rule and the centre crop: (nw, nh, top, left)."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = int(shortest_edge), int(shortest_edge * long / short)
    nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
    if nh < S or nw < S:
        raise NotImplementedError(f"crop {S} is larger than the resized image {nw} x {nh}: padding is not implemented")
    return nw, nh, (nh - S) // 2, (nw - S) // 2


def _rescale_normalize(a: np.ndarray, rescale: float, mean, std) -> np.ndarray:
    """uint8 [3, h, w] -> float32: float64 rescale rounded to float32, then (x - mean) / std in float32."""
    x = (a.astype(np.float64) * rescale).astype(np.float32)
    return ((x.T - np.array(mean, dtype=np.float32)) / np.array(std, dtype=np.float32)).T


def preprocess(image, processor_config: dict) -> torch.Tensor:
    """A PIL image -> pixel_values fp32 [3, S, S] as CLIPImageProcessor's PIL path computes them (image_processor/preprocessor_config.json):
    convert to RGB, resize the shortest edge on the uint8 image with the configured PIL filter (the long edge is int(size * long / short)),
    centre crop, uint8 -> float64 * rescale_factor -> float32, (x - mean) / std in float32.  Settings this does not implement raise
    NotImplementedError: any of the five steps switched off, padding, a size that is not a shortest edge (or square), a crop larger
    than the resized image."""
    from PIL import Image
    edge, S, resample, mean, std, rescale = _processor_settings(processor_config)
    if not isinstance(image, Image.Image):
        raise TypeError(f"preprocess takes a PIL image, got {type(image)}")
    img = image.convert("RGB")
    nw, nh, top, left = _resized_and_window(*img.size, edge, S)
    img = img.resize((nw, nh), resample=getattr(Image.Resampling, _PIL_RESAMPLE[resample]))
    a = np.asarray(img)[top:top + S, left:left + S].transpose(2, 0, 1)
    return torch.from_numpy(np.ascontiguousarray(_rescale_normalize(a, rescale, mean, std), dtype=np.float32))


def preprocess_device(image, processor_config: dict, device) -> torch.Tensor:
    """preprocess on the device, bit for bit: a PIL image or a u8 [h, w, 3] tensor (host or device) -> pixel_values fp32 [3, S, S] on
    `device`.  The same settings and refusals (_processor_settings); the resize with the configured filter, the centre-crop window, the
    u8 -> f32 step and the move to planar are one entry (ops.resample_u8_window) that computes the window only; the three per-channel
    tables of 256 floats are preprocess' own two expressions on every byte value.  resample 0 (NEAREST is no convolution in Pillow) raises
    NotImplementedError here; the host function serves it."""
    from . import ops
    edge, S, resample, mean, std, rescale = _processor_settings(processor_config)
    if resample == 0:
        raise NotImplementedError("preprocessor_config resample 0 (NEAREST) is not implemented on the device: use preprocess")
    if isinstance(image, torch.Tensor):
        if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
            raise TypeError(f"preprocess_device takes a PIL image or a uint8 [h, w, 3] tensor, got {image.dtype} {tuple(image.shape)}")
        px = image
    else:
        from PIL import Image
        if not isinstance(image, Image.Image):
            raise TypeError(f"preprocess_device takes a PIL image or a uint8 [h, w, 3] tensor, got {type(image)}")
        px = torch.from_numpy(np.asarray(image.convert("RGB")).copy())
    h, w = px.shape[:2]
    nw, nh, top, left = _resized_and_window(w, h, edge, S)
    table = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (3, 256, 1))
    lut = torch.from_numpy(np.ascontiguousarray(_rescale_normalize(table, rescale, mean, std)[:, :, 0], dtype=np.float32))
    out = ops.resample_u8_window(px.to(device).unsqueeze(0), (nh, nw), (top, left, S, S), lut.to(device), filter=_PIL_RESAMPLE[resample].lower())
    return out[0]


def encode_image(model_path: str, image, device, subfolder: Optional[str] = "image_encoder") -> torch.Tensor:
    """PIPE:207-211 on this engine: the folder's `image_processor/preprocessor_config.json` and `image_encoder/`, a PIL image or a u8
    [h, w, 3] tensor (a frame that is already on the device stays there) -> image_embeds bf16 [1, tokens, hidden] (hidden_states[-2], cast
    once).  The pixels go through preprocess_device.  The encoder is built for the call and freed afterwards."""
    with open(os.path.join(model_path, "image_processor", "preprocessor_config.json")) as f:
        pc = json.load(f)
    model = CLIPVisionModel.from_pretrained(model_path, device=device, subfolder=subfolder)
    out = model(preprocess_device(image, pc, device)).to(torch.bfloat16).unsqueeze(0)
    del model
    if torch.device(device).type == "cuda":
        torch.cuda.empty_cache()
    return out
