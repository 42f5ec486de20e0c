"""LongCat-Video DiT (LongCatVideoTransformer3DModel) on hand-written HIP kernels.

Speaks the call protocol of the reference sampler (longcat_video/pipeline_longcat_video.py:867-873):
    dit(hidden_states[B,16,T,H,W], timestep[B,T], encoder_hidden_states[B,1,N,4096], encoder_attention_mask[B,N],
        num_cond_latents=1) -> fp32 [B,16,T,H,W]
and follows longcat_video/modules/longcat_video_dit.py (LCD), attention.py (LCA), blocks.py (LCB), rope_3d.py (LCR); file:line
citations are on the kernels (csrc/longcat_ops.hip, gemm.hip, attention.hip) and below.  Every FLOP of the token path runs in
libwf_hip.so; PyTorch owns the buffers.  The samples of a batch (the CFG pair of pipeline:857-866) are run one after the other:
the reference's varlen / block-diagonal cross-attention (LCA:236-262) never mixes samples.

Numerics: bf16 weights, bf16 residual stream (LCD:104, 120), bf16 GEMM / attention operands with fp32 accumulation, fp32 timestep
embedding and AdaLN parameters (LCD:84-88, 310-311: the fp32 activations are fed to the bf16 MFMA GEMM as a hi + lo bf16 pair, which
keeps 16 mantissa bits), fp32 LayerNorm statistics, fp32 final projection (LCB:162-167).

Runtime LoRA (LCD:189-270): `load_lora` / `enable_loras` / `disable_all_loras` keep the adapters' bf16 factors resident and SWITCH the
weights on the GPU (csrc/lora.hip: effective = bf16(base + sum of the active adapters' scaled products), one rounding, from an untouched
base copy), so the forward still runs on plain bf16 matrices and a LoRA costs nothing per step; `fold_lora` is the host-side state-dict
route (a fold before load_state_dict, not undoable).  Block-sparse attention (LCA:57-66; `enable_bsa`, bsa.py)
and sequence parallelism (`comm`, parallel.py) are built.

Weights: `load_state_dict` (a reference-keyed state dict), `init_random`, or `from_pretrained(folder)` -- `<folder>/dit/config.json` plus
safetensors files, their headers checked against `expected_state_dict(cfg)` before anything is uploaded, every tensor rounded to bf16
first as the reference's `torch_dtype=torch.bfloat16` load does (run_longcat_worldforge_single.py:207).

Video continuation (LCA:147-181, PIPE:336-348): `cache_condition` runs the condition frames' stream once (timestep 0, no caption, no
cross-attention: it depends on neither the noise tokens, the prompt nor the step) and keeps every block's K / V^T / norm bound resident
in the attention kernel's layout (LongCatCondCache); `forward_tokens_cached` / `forward_cached` then run the noise frames only, appending
their keys behind the cached ones (wf_lc_norm_heads at a row offset, wf_v_transpose_at) in front of the one noise-query attention launch
of the uncached forward.  A cache is bound to the weights it was built with (weights version, adapters, linear_precision) and to its
latent size.  `cache_condition_blocks` / `forward_tokens_cached_blocks` / `forward_cached_blocks` are the same for a model with
block-sparse attention on (the refine pass of a continued video): a LongCatBlockCondCache holds K / V^T and the pooled key-block means
in 3D-block token order.  Not built: continuation under sequence parallelism, CPU offload of the cache.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._ffi import call
from .dit import (EPI_BF16, EPI_BF16_GELU, EPI_F32, EPI_F32_ACC, _pad64, attention, attention_exchange, gemm, head_max_norm2,
                  quantize_linears)
from .forward_common import (ForwardWorkspaces, act, bf16_latents, gather_layer_kv, layers_per_rank, run, seeded_generators,
                             wait_events)


@dataclass
class LongCatConfig:
    """LCD:138-158 defaults = the released model."""
    hidden_size: int = 4096
    depth: int = 48
    num_heads: int = 32
    in_channels: int = 16
    out_channels: int = 16
    caption_channels: int = 4096
    mlp_ratio: int = 4
    adaln_tembed_dim: int = 512
    frequency_embedding_size: int = 256
    patch_size: Tuple[int, int, int] = (1, 2, 2)
    text_tokens_zero_pad: bool = False
    eps: float = 1e-6

    @property
    def ffn_hidden(self) -> int:
        """LCB:17-29."""
        h = int(2 * int(self.hidden_size * self.mlp_ratio) / 3)
        return 256 * ((h + 255) // 256)


def expected_state_dict(cfg: LongCatConfig) -> Dict[str, Tuple[int, ...]]:
    """{reference parameter name: shape} of everything load_state_dict reads = the state dict of the reference module
    (LCD:159-189, LCB, LCA) for this configuration.  Host only: from_pretrained checks a checkpoint's header against it before
    anything is uploaded, the checkpoint audit reports against it."""
    C, Ct, Hd = cfg.hidden_size, cfg.adaln_tembed_dim, cfg.ffn_hidden
    D = C // cfg.num_heads
    E: Dict[str, Tuple[int, ...]] = {"x_embedder.proj.weight": (C, cfg.in_channels) + tuple(cfg.patch_size), "x_embedder.proj.bias": (C,)}

    def lin(name, o, i, bias=True):
        E[name + ".weight"] = (o, i)
        if bias:
            E[name + ".bias"] = (o,)

    lin("t_embedder.mlp.0", Ct, cfg.frequency_embedding_size)
    lin("t_embedder.mlp.2", Ct, Ct)
    lin("y_embedder.y_proj.0", C, cfg.caption_channels)
    lin("y_embedder.y_proj.2", C, C)
    lin("final_layer.linear", int(np.prod(cfg.patch_size)) * cfg.out_channels, C)
    lin("final_layer.adaLN_modulation.1", 2 * C, Ct)
    for i in range(cfg.depth):
        p = f"blocks.{i}."
        lin(p + "adaLN_modulation.1", 6 * C, Ct)
        E[p + "pre_crs_attn_norm.weight"] = E[p + "pre_crs_attn_norm.bias"] = (C,)
        for n, o in (("attn.qkv", 3 * C), ("attn.proj", C), ("cross_attn.q_linear", C), ("cross_attn.kv_linear", 2 * C), ("cross_attn.proj", C)):
            lin(p + n, o, C)
        for n in ("attn.q_norm", "attn.k_norm", "cross_attn.q_norm", "cross_attn.k_norm"):
            E[p + n + ".weight"] = (D,)
        lin(p + "ffn.w1", Hd, C, bias=False)
        lin(p + "ffn.w2", C, Hd, bias=False)
        lin(p + "ffn.w3", Hd, C, bias=False)
    return E


# config.json of the reference class (a diffusers ConfigMixin file, LCD:129-151): what goes into LongCatConfig, what goes to the
# constructor, and what is accepted and dropped (the attention back-ends are this engine's kernels; sequence parallelism is `comm`)
_CONFIG_FIELDS = ("in_channels", "out_channels", "hidden_size", "depth", "num_heads", "caption_channels", "mlp_ratio", "adaln_tembed_dim",
                  "frequency_embedding_size", "patch_size", "text_tokens_zero_pad")
_CONFIG_IGNORED = ("enable_flashattn2", "enable_flashattn3", "enable_xformers", "cp_split_hw")


def config_from_dict(c: dict):
    """-> (LongCatConfig, constructor keywords {enable_bsa, bsa_params}, [keys that are neither known nor ignored]).  ValueError for
    a `_class_name` of another class (someone pointing the loader at a Wan `transformer/` folder)."""
    name = c.get("_class_name")
    if name is not None and name != "LongCatVideoTransformer3DModel":
        raise ValueError(f"config.json is of class {name!r}, not LongCatVideoTransformer3DModel")
    kw = {k: c[k] for k in _CONFIG_FIELDS if k in c}
    if "patch_size" in kw:
        kw["patch_size"] = tuple(int(v) for v in kw["patch_size"])
    if "text_tokens_zero_pad" in kw:
        kw["text_tokens_zero_pad"] = bool(kw["text_tokens_zero_pad"])
    ctor = dict(enable_bsa=bool(c.get("enable_bsa", False)), bsa_params=c.get("bsa_params") or None)
    unknown = [k for k in c if k not in _CONFIG_FIELDS and k not in _CONFIG_IGNORED and k not in ("enable_bsa", "bsa_params")
               and not k.startswith("_")]
    return LongCatConfig(**kw), ctor, unknown


def timestep_embedding(ts, dim: int, max_period: float = 10000.0) -> torch.Tensor:
    """LCB:181-199 on the host in fp32: [cos | sin] -> [len(ts), dim]."""
    half = dim // 2
    freqs = np.exp(np.float32(-math.log(max_period)) * np.arange(half, dtype=np.float32) / np.float32(half)).astype(np.float32)
    args = np.asarray(ts, dtype=np.float32)[:, None] * freqs[None]
    emb = np.concatenate([np.cos(args), np.sin(args)], axis=-1).astype(np.float32)
    if dim % 2:
        emb = np.concatenate([emb, np.zeros_like(emb[:, :1])], axis=-1)
    return torch.from_numpy(emb)


def rope_tables(head_dim: int, f: int, h: int, w: int, base: float = 10000.0):
    """LCR:68-99 + 113-115: cos / sin [f*h*w, head_dim/2] fp32, one entry per rotation pair (2p, 2p+1): the first
    (head_dim - 4*(head_dim//6))/2 pairs turn with the frame index, the next head_dim//6 with the row, the last with the column."""
    d_hw = 2 * (head_dim // 6)
    d_t = head_dim - 2 * d_hw

    def axis(n, dim):
        freqs = 1.0 / (base ** (torch.arange(0, dim, 2)[: dim // 2].float() / dim))
        grid = torch.from_numpy(np.linspace(0, n, n, endpoint=False, dtype=np.float32)).float()
        return torch.outer(grid, freqs)  # [n, dim/2]

    at, ah, aw = axis(f, d_t), axis(h, d_hw), axis(w, d_hw)
    ang = torch.cat([at.view(f, 1, 1, -1).expand(f, h, w, -1), ah.view(1, h, 1, -1).expand(f, h, w, -1),
                     aw.view(1, 1, w, -1).expand(f, h, w, -1)], dim=-1).reshape(f * h * w, head_dim // 2)
    return ang.cos().contiguous(), ang.sin().contiguous()


def fold_lora(sd: Dict[str, torch.Tensor], lora_sd: Dict[str, torch.Tensor], multiplier: float = 1.0, network_dim: int = 128,
              network_alpha: float = 64.0) -> Dict[str, torch.Tensor]:
    """The reference applies LoRA at run time (LCD:189-247, lora_utils.py:27-78): every wrapped Linear returns
    org(x) + multiplier * alpha_scale * up(down(x)).  Here the update is folded into the weights once, at load (fp32 accumulate, then
    the usual bf16 storage): W' = W + multiplier * alpha_scale * U @ D, with U block-diagonal over the rank slices of D when the
    up-projection is stored as n separate blocks (fused qkv / kv).  A weight-load step, not part of the sampling path; the forward then
    costs exactly what the base model costs.  Returns a new reference-keyed state dict for load_state_dict."""
    out = dict(sd)
    for key in lora_sd:
        if not key.endswith(".lora_down.weight"):
            continue
        name = key[: -len(".lora_down.weight")]
        module = name.replace("lora___lorahyphen___", "").replace("___lorahyphen___", ".")
        wk = module + ".weight"
        if wk not in sd:
            raise KeyError(f"LoRA entry {name} has no Linear {wk} in the model")
        dev = sd[wk].device
        down = lora_sd[key].to(dev, torch.float32)
        if name + ".alpha_scale" in lora_sd:
            scale = float(lora_sd[name + ".alpha_scale"])
        else:
            scale = (network_alpha or network_dim) / network_dim
        if name + ".lora_up.weight" in lora_sd:
            delta = lora_sd[name + ".lora_up.weight"].to(dev, torch.float32) @ down
        else:
            blocks = sorted((k for k in lora_sd if k.startswith(name + ".lora_up.blocks.")), key=lambda k: int(k.split(".")[-2]))
            if not blocks:
                raise KeyError(f"LoRA entry {name} has no up-projection")
            r = down.shape[0] // len(blocks)
            delta = torch.cat([lora_sd[k].to(dev, torch.float32) @ down[i * r:(i + 1) * r] for i, k in enumerate(blocks)], dim=0)
        if tuple(delta.shape) != tuple(sd[wk].shape):
            raise ValueError(f"LoRA update for {wk} has shape {tuple(delta.shape)}, weight is {tuple(sd[wk].shape)}")
        out[wk] = sd[wk].to(torch.float32) + (multiplier * scale) * delta
    return out


_LORA_H = "___lorahyphen___"


@dataclass(eq=False)
class _CondCache:
    """What both condition caches say about themselves: their size, and the model and weights they were built with."""
    ncl: int               # condition latent frames
    nc: int                # condition tokens = ncl * tokens per frame
    latent_hw: Tuple[int, int]
    owner: object          # the model's token, and what its weights were when the cache was built:
    wver: int
    loras: Tuple[str, ...]
    linear_precision: str


@dataclass(eq=False)
class LongCatCondCache(_CondCache):
    """The condition frames' self-attention keys / values of every block (LCA:149-181 `kv_cache_dict`), resident on the GPU in the
    layout wf_attn_fwd reads, built by LongCatVideoTransformer3DModel.cache_condition.  K is normalised AND rotated: a frame's RoPE rows
    do not depend on how many frames follow (rope_tables), so the rotation of LCA:168-172 is done once."""
    k: torch.Tensor        # bf16 [depth, H, pad64(nc), 128], rows nc.. zero
    vt: torch.Tensor       # bf16 [depth, H, pad64(nc) / 64, 128, 64], keys nc.. zero
    kmax2: torch.Tensor    # f32 [depth, H]: max |k row|^2 per head over the nc cached rows (wf_head_max_norm2)


@dataclass(eq=False)
class LongCatBlockCondCache(_CondCache):
    """The condition cache of the block-sparse refine pass (cache_condition_blocks): every tensor in 3D-BLOCK token order, in which
    the condition tokens are the first nc rows of every (condition + noise) grid (bsa_interface.py:600-604 orders by frame chunk first
    and ncl is whole chunks), so nc is whole blocks and whole 64-key tiles.  Besides K / V^T it keeps the pooled key-block means
    (bsa_interface.py:169-179): the gating of every later step scores its query blocks against them."""
    k: torch.Tensor        # bf16 [depth, H, nc, 128], normalised and rotated
    vt: torch.Tensor       # bf16 [depth, H, nc / 64, 128, 64]
    kcmp: torch.Tensor     # bf16 [depth, H, nc / block, 128]: mean of every key block
    bsa_indices: list      # per DiT block the condition-query selection of the build (what last_bsa_indices held; read by tests)
    chunk: Tuple[int, int, int]
    sparsity: Optional[float]
    cdf_threshold: Optional[float]


@dataclass(eq=False)
class LoRAPart:
    """One wrapped Linear of one adapter, placed in this model's fused storage: rows [row0, row0 + U.shape[0]) of matrix `wkey`."""
    wkey: str
    row0: int
    U: torch.Tensor      # bf16 [rows, rank]: the up-projection, its separate blocks stacked (never block-diagonal)
    D: torch.Tensor      # bf16 [nsep * rank, K]: the down-projection; row block b of the slice uses rank slice b
    nsep: int
    scale: float         # multiplier * alpha_scale


@dataclass(frozen=True, eq=False)
class _ForwardPlan:
    """Everything one forward derives from its arguments (LongCatVideoTransformer3DModel._plan), fixed before its first launch.  Counts
    of the whole sequence and of this rank's rows have names of their own: without `comm` they differ by the cached keys only."""
    tag: str                                    # separates the workspaces of concurrent forwards
    T: int; Hh: int; Ww: int; tpf: int          # noqa: E702  this forward's latent frames, their size, tokens per frame
    L_tok: int                                  # this forward's tokens, over all ranks
    L_all: int; nc_all: int                     # noqa: E702  the keys a noise / a condition query sees: kc + L_tok / the condition tokens
    L: int; nc: int; lo: int                    # noqa: E702  this rank's rows, its condition rows (the first), its first row's global index
    kc: int; fc: int                            # noqa: E702  cached condition keys / frames IN FRONT of this forward's rows (0 without "use")
    Sp: int                                     # key rows of a shard = of a K workspace (whole 64-key tiles)
    blk: int                                    # tokens per attention block (64 in the dense paths)
    cos: torch.Tensor; sin: torch.Tensor        # noqa: E702  RoPE tables of this rank's rows (in block order under block-sparse attention)
    gidx: object; perm: object; pos: object     # noqa: E702  block order: frame index per row, the permutation, its inverse; else None
    shard: object                               # parallel.ShardPlan, None without `comm`
    use_bsa: bool
    build: bool; cached: bool; cache: object    # noqa: E702  vc = ("build", cache) / ("use", cache)
    prescale: bool; use_bounds: bool            # noqa: E702
    scale: float; q_scale: float; sa_scale: float  # noqa: E702  1 / sqrt(head_dim); what the query producer folds in / the kernel is told
    exchange: Optional[str]                     # the effective mode of the K / V^T exchange; None: this forward has none
    sparsity: Optional[float]; cdf_thr: Optional[float]; fused_sel: bool  # noqa: E702  the block selection rule (bsa_params, WF_BSA_TORCH_SELECT)


class LongCatVideoTransformer3DModel(ForwardWorkspaces):
    dtype = torch.bfloat16

    # the per-block token GEMMs that linear_precision="mxfp8" runs in MX-fp8 (embeddings, AdaLN, final layer and the caption K / V stay bf16)
    MX_LINEARS = ("attn.qkv.w", "attn.proj.w", "cross_attn.q_linear.w", "cross_attn.proj.w", "ffn.w13", "ffn.w2")

    def __init__(self, cfg: LongCatConfig, device="cuda:0", enable_bsa: bool = False, bsa_params: Optional[dict] = None, comm=None,
                 linear_precision: str = "bf16"):
        if linear_precision not in ("bf16", "mxfp8"):
            raise ValueError(f"linear_precision must be 'bf16' or 'mxfp8', not {linear_precision!r}")
        self.linear_precision = linear_precision
        assert cfg.hidden_size // cfg.num_heads == 128 and cfg.hidden_size % cfg.num_heads == 0, "attention kernel is built for head_dim 128"
        assert cfg.patch_size == (1, 2, 2)
        self.cfg = cfg
        self.config = SimpleNamespace(in_channels=cfg.in_channels, out_channels=cfg.out_channels, patch_size=cfg.patch_size)
        self.cp_split_hw = None
        self.comm = comm  # parallel.Comm (or a stand-in): sequence parallelism over contiguous token shards, see forward_tokens
        self.device = torch.device(device)
        # switchable LoRA adapters (LCD:189-270): lora_dict key -> [LoRAPart], active_loras the enabled keys in order; _eff holds ONE
        # effective buffer per touched matrix, allocated at its first activation and reused by every later switch
        self.lora_dict: Dict[str, list] = {}
        self.active_loras: list = []
        self._eff: Dict[str, torch.Tensor] = {}
        self.w: Dict[str, torch.Tensor] = {}
        self._ws = {}
        self._rope = {}
        self._token = object()  # what a LongCatCondCache names its model by
        self.last_kmax2 = self.last_vc_keys = None  # forward_tokens_cached: the last block's key norm bound and (working K, key count)
        # block-sparse self-attention of the 720p refine pass (LCA:57-66, LCD:270-276); bsa_params as in the reference's config:
        # sparsity, chunk_3d_shape_q, chunk_3d_shape_k (cdf_threshold is not built)
        self._bsa = bool(enable_bsa)
        self.bsa_params = dict(bsa_params) if bsa_params else dict(sparsity=0.875, chunk_3d_shape_q=[4, 4, 8], chunk_3d_shape_k=[4, 4, 8])  # bsa_interface.py:618-621 defaults
        self.last_bsa_indices = None

    @property
    def w(self) -> Dict[str, torch.Tensor]:
        """The weights the forward runs on: the base dictionary itself while no adapter is active, else the effective dictionary
        (touched matrices replaced by their effective buffers, every other tensor shared with the base)."""
        return self._w

    @w.setter
    def w(self, W: Dict[str, torch.Tensor]):
        """A new base: every adapter is deactivated (the loaded ones stay in lora_dict), the effective buffers are dropped."""
        self._base = self._w = W
        self.active_loras = []
        self._eff = {}
        self.weights_changed()

    @property
    def base_w(self) -> Dict[str, torch.Tensor]:
        """The base weights (never written by a LoRA switch)."""
        return self._base

    def weights_changed(self):
        """Call after editing (base) weight tensors IN PLACE: with adapters active the effective weights are folded again from the
        base, then the MX-fp8 copies of linear_precision="mxfp8" are re-derived (none in bf16).  Every path that changes the weights
        the forward runs on ends here (the `w` setter, load_state_dict, the LoRA switches): the version counter makes a
        LongCatCondCache built before it unusable."""
        self._wver = getattr(self, "_wver", 0) + 1
        try:
            self._w = self._fold_active() if self.active_loras else self._base
        except Exception:  # a switch that cannot be made leaves the base model, not half-folded buffers
            self.active_loras, self._w = [], self._base
            self._wl = quantize_linears(self._w, self.MX_LINEARS) if self.linear_precision == "mxfp8" else self._w
            raise
        self._wl = quantize_linears(self._w, self.MX_LINEARS) if self.linear_precision == "mxfp8" else self._w

    # ---- LoRA adapters (LCD:189-270, lora_utils.py) ---------------------------------------------------------------
    def _lora_target(self, module: str):
        """Reference module name -> (key in the fused storage, first row, rows) of its Linear; KeyError if the model has none."""
        cfg, W = self.cfg, self._base
        parts = module.split(".")
        key = row0 = rows = None
        if len(parts) == 4 and parts[0] == "blocks" and parts[1].isdigit() and parts[2] == "ffn" and parts[3] in ("w1", "w3"):
            key, rows = f"blocks.{parts[1]}.ffn.w13", cfg.ffn_hidden
            row0 = 0 if parts[3] == "w1" else rows
        elif len(parts) == 4 and parts[0] == "blocks" and parts[1].isdigit() and parts[2:] == ["adaLN_modulation", "1"]:
            key, rows = "ada.w", 6 * cfg.hidden_size
            row0 = int(parts[1]) * rows
            if int(parts[1]) >= cfg.depth:
                key = None
        elif parts[-2:] == ["ffn", "w2"]:
            key, row0 = module, 0
        elif module != "x_embedder.proj":  # (a Conv3d in the reference: not a Linear, never wrapped)
            key, row0 = module + ".w", 0
        t = W.get(key) if key is not None else None
        if t is None or t.dim() != 2 or t.dtype != torch.bfloat16:
            raise KeyError(f"LoRA entry {module} has no Linear {module}.weight in the model")
        return key, row0, (t.shape[0] if rows is None else rows)

    def _parse_lora(self, lora_sd, multiplier, network_dim, network_alpha):
        """State dict in the reference's naming -> [LoRAPart] on the device, factors rounded to bf16 (LCD:221); the naming and the
        strictness of fold_lora."""
        dev, bf = self.device, torch.bfloat16
        out = []
        for key in lora_sd:
            if not key.endswith(".lora_down.weight"):
                continue
            name = key[: -len(".lora_down.weight")]
            module = name.replace("lora" + _LORA_H, "").replace(_LORA_H, ".")
            wkey, row0, rows = self._lora_target(module)
            K = self._base[wkey].shape[1]
            down = lora_sd[key]
            if name + ".alpha_scale" in lora_sd:
                scale = float(lora_sd[name + ".alpha_scale"])
            else:
                scale = (network_alpha or network_dim) / network_dim
            if name + ".lora_up.weight" in lora_sd:
                ups = [lora_sd[name + ".lora_up.weight"]]
            else:
                ups = [lora_sd[k] for k in sorted((k for k in lora_sd if k.startswith(name + ".lora_up.blocks.")),
                                                  key=lambda k: int(k.split(".")[-2]))]
                if not ups:
                    raise KeyError(f"LoRA entry {name} has no up-projection")
            nsep = len(ups)
            rank = down.shape[0] // nsep if down.dim() == 2 else 0
            ok = (down.dim() == 2 and down.shape[1] == K and rank > 0 and down.shape[0] == nsep * rank
                  and all(u.dim() == 2 and tuple(u.shape) == (rows // nsep, rank) for u in ups) and rows % nsep == 0)
            if not ok:
                raise ValueError(f"LoRA update for {module}.weight: down {tuple(down.shape)}, up {[tuple(u.shape) for u in ups]} do not "
                                 f"give the weight's shape {(rows, K)}")
            U = torch.cat([u.to(torch.float32) for u in ups], 0).to(bf)
            D = down.to(torch.float32).to(bf)
            if rank % 8:  # the kernel takes ranks in whole 8-element operand slots: zero ranks change nothing
                pad = 8 - rank % 8
                U = torch.nn.functional.pad(U, (0, pad))
                D = torch.nn.functional.pad(D.view(nsep, rank, K), (0, 0, 0, pad)).reshape(nsep * (rank + pad), K)
            out.append(LoRAPart(wkey, row0, U.contiguous().to(dev), D.contiguous().to(dev), nsep, float(multiplier) * scale))
        return out

    def load_lora(self, lora, lora_key: str, multiplier: float = 1.0, lora_network_dim: int = 128, lora_network_alpha: float = 64):
        """LCD:194-215.  lora: a .safetensors path or a state dict in the reference's naming (`lora___lorahyphen___blocks___lorahyphen___3
        ___lorahyphen___attn___lorahyphen___qkv.lora_down.weight`, `.lora_up.weight` or `.lora_up.blocks.N.weight`, optional
        `.alpha_scale`, else alpha / dim).  The factors are rounded to bf16, uploaded once and stay resident.  KeyError for an entry
        whose Linear the model does not have, ValueError for a shape mismatch, both raised here with lora_dict unchanged.  Loading
        under an existing key replaces that adapter (the weights are folded again if it is active)."""
        if isinstance(lora, (str, os.PathLike)):
            from .checkpoint import load_file
            lora = load_file(os.fspath(lora))
        parts = self._parse_lora(lora, multiplier, lora_network_dim, lora_network_alpha)
        self.lora_dict[lora_key] = parts
        if lora_key in self.active_loras:
            self.weights_changed()

    def enable_loras(self, lora_key_list):
        """LCD:217-247: disable_all_loras(), then the listed keys become active (unknown keys are ignored, LCD:219): every touched matrix
        becomes wf_lora_fold(base, all its active adapters) in its effective buffer; the forward's cost does not change."""
        active = []
        for k in lora_key_list:
            if k in self.lora_dict and k not in active:
                active.append(k)
        self.active_loras = active
        self.weights_changed()

    def disable_all_loras(self):
        """LCD:249-268: the forward reads the base tensors again (the effective buffers are kept for the next switch)."""
        self.active_loras = []
        self.weights_changed()

    def _fold_active(self) -> Dict[str, torch.Tensor]:
        """The effective dictionary of the active adapters, folded from the base on the device."""
        touched: Dict[str, Dict[int, list]] = {}
        for key in self.active_loras:
            for part in self.lora_dict[key]:
                touched.setdefault(part.wkey, {}).setdefault(part.row0, []).append(part)
        eff = dict(self._base)
        for wkey, slices in touched.items():
            base = self._base.get(wkey)
            for row0, parts in slices.items():
                for q in parts:
                    if base is None or base.dim() != 2 or row0 + q.U.shape[0] > base.shape[0] or q.D.shape[1] != base.shape[1]:
                        raise ValueError(f"LoRA adapter for {wkey} rows {row0}..{row0 + q.U.shape[0]} does not fit the current base weights")
            buf = self._eff.get(wkey)
            if buf is None or buf.shape != base.shape or buf.device != base.device:
                buf = self._eff[wkey] = torch.empty_like(base)
            pos = 0
            for row0 in sorted(slices):  # rows no active adapter touches are the base's bits
                if row0 > pos:
                    buf[pos:row0].copy_(base[pos:row0])
                parts = slices[row0]
                rows = parts[0].U.shape[0]
                for i in range(0, len(parts), 4):  # one launch, ONE rounding for up to 4 adapters of a Linear; a fifth rounds again
                    ops.lora_fold((base if i == 0 else buf)[row0:row0 + rows], buf[row0:row0 + rows],
                                  [(q.U, q.D, q.nsep, q.scale) for q in parts[i:i + 4]])
                pos = row0 + rows
            if pos < base.shape[0]:
                buf[pos:].copy_(base[pos:])
            eff[wkey] = buf
        return eff

    def enable_bsa(self):
        """LCD:270-272."""
        self._bsa = True

    def disable_bsa(self):
        """LCD:274-276."""
        self._bsa = False

    # ------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Reference-keyed state dict (any dtype / device) -> device tensors: matrices bf16, vectors fp32; the AdaLN projections of
        all blocks stacked into one matrix, w1 | w3 fused."""
        dev = self.device
        mat = lambda k: sd[k].to(device=dev, dtype=torch.bfloat16).contiguous()  # noqa: E731
        vec = lambda k: sd[k].to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
        return self._assemble(mat, vec)

    def _assemble(self, mat, vec):
        """The fused storage from two readers of a reference key: mat -> bf16 device matrix, vec -> fp32 device vector."""
        cfg = self.cfg
        W = {}
        W["patch.w"] = mat("x_embedder.proj.weight").reshape(cfg.hidden_size, -1).contiguous()
        W["patch.b"] = vec("x_embedder.proj.bias")
        for n in ("t_embedder.mlp.0", "t_embedder.mlp.2", "y_embedder.y_proj.0", "y_embedder.y_proj.2", "final_layer.linear",
                  "final_layer.adaLN_modulation.1"):
            W[n + ".w"], W[n + ".b"] = mat(n + ".weight"), vec(n + ".bias")
        W["ada.w"] = torch.cat([mat(f"blocks.{i}.adaLN_modulation.1.weight") for i in range(cfg.depth)], 0).contiguous()
        W["ada.b"] = torch.cat([vec(f"blocks.{i}.adaLN_modulation.1.bias") for i in range(cfg.depth)], 0).contiguous()
        for i in range(cfg.depth):
            p = f"blocks.{i}."
            W[p + "norm.w"], W[p + "norm.b"] = vec(p + "pre_crs_attn_norm.weight"), vec(p + "pre_crs_attn_norm.bias")
            for n in ("attn.qkv", "attn.proj", "cross_attn.q_linear", "cross_attn.kv_linear", "cross_attn.proj"):
                W[p + n + ".w"], W[p + n + ".b"] = mat(p + n + ".weight"), vec(p + n + ".bias")
            for n in ("attn.q_norm", "attn.k_norm", "cross_attn.q_norm", "cross_attn.k_norm"):
                W[p + n] = vec(p + n + ".weight")
            W[p + "ffn.w13"] = torch.cat([mat(p + "ffn.w1.weight"), mat(p + "ffn.w3.weight")], 0).contiguous()
            W[p + "ffn.w2"] = mat(p + "ffn.w2.weight")
        self.w = W
        return self

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0", comm=None, subfolder: str = "dit", linear_precision: str = "bf16",
                        strict: bool = True):
        """`LongCatVideoTransformer3DModel.from_pretrained(checkpoint_dir, subfolder="dit", torch_dtype=torch.bfloat16)`
        (run_longcat_worldforge_single.py:207) from a local folder: `<path>/<subfolder>/config.json` (config_from_dict; an unknown key
        is ignored with one UserWarning naming it) + one safetensors file or an index with shards (checkpoint.load_dir).

        Before anything is uploaded the files' headers are checked against expected_state_dict(cfg): missing keys are a KeyError,
        keys the model does not consume a ValueError (a warning with strict=False), a wrong shape a ValueError naming key, found and
        expected.  EVERY tensor is first rounded to bf16, whatever the file's dtype -- what torch_dtype=torch.bfloat16 does to every
        parameter of the reference module -- and then stored as load_state_dict stores it (matrices bf16, vectors fp32 holding the
        bf16 values).  load_state_dict itself keeps an fp32 checkpoint's vectors unrounded; this loader must not.  The tensors go from
        the memory map to the device one at a time: no second host copy of the checkpoint is made."""
        import json
        import warnings
        from . import checkpoint
        folder = os.path.join(path, subfolder) if subfolder and os.path.isdir(os.path.join(path, subfolder)) else path
        cj = os.path.join(folder, "config.json")
        if not os.path.exists(cj):
            raise FileNotFoundError(f"{folder}: no config.json")
        with open(cj) as f:
            cfg, ctor, unknown = config_from_dict(json.load(f))
        for k in unknown:
            warnings.warn(f"{cj}: key {k!r} is not a field of LongCatVideoTransformer3DModel and is ignored", UserWarning, stacklevel=2)
        found, info = checkpoint.dir_header(folder)
        if info["missing_shards"]:
            raise FileNotFoundError(f"{folder}: shards named by {info['index']} are missing: {info['missing_shards']}")
        missing, unexpected, wrong = checkpoint.compare_header(found, expected_state_dict(cfg))
        if missing:
            raise KeyError(f"{folder}: {len(missing)} parameters of the model are not in the checkpoint: {missing[:5]}")
        if wrong:
            w = wrong[0]
            raise ValueError(f"{folder}: {len(wrong)} parameters have the wrong shape: {w['key']} is {w['found']}, expected {w['expected']}")
        if unexpected:
            msg = f"{folder}: {len(unexpected)} checkpoint tensors are not consumed by the model: {unexpected[:5]}"
            if strict:
                raise ValueError(msg)
            warnings.warn(msg, UserWarning, stacklevel=2)
        model = cls(cfg, device, comm=comm, linear_precision=linear_precision, **ctor)
        sd = checkpoint.load_dir(folder)  # memory-mapped: a tensor's bytes are read when it is converted below
        dev, bf = model.device, torch.bfloat16
        mat = lambda k: sd[k].to(bf).to(dev).contiguous()  # noqa: E731
        vec = lambda k: sd[k].to(bf).to(dev).to(torch.float32).contiguous()  # noqa: E731
        return model._assemble(mat, vec)

    def init_random(self, seed: int = 0):
        """Synthetic weights of the right shapes, generated on the device (there are no checkpoints offline)."""
        cfg = self.cfg
        mat, vec = seeded_generators(self.device, seed)
        C, Ct, Hd = cfg.hidden_size, cfg.adaln_tembed_dim, cfg.ffn_hidden
        W = {"patch.w": mat(C, cfg.in_channels * 4), "patch.b": vec(C)}
        for n, (o, i) in {"t_embedder.mlp.0": (Ct, cfg.frequency_embedding_size), "t_embedder.mlp.2": (Ct, Ct),
                          "y_embedder.y_proj.0": (C, cfg.caption_channels), "y_embedder.y_proj.2": (C, C),
                          "final_layer.linear": (4 * cfg.out_channels, C)}.items():
            W[n + ".w"], W[n + ".b"] = mat(o, i), vec(o)
        W["final_layer.adaLN_modulation.1.w"], W["final_layer.adaLN_modulation.1.b"] = mat(2 * C, Ct, 0.5 / math.sqrt(Ct)), vec(2 * C)
        W["ada.w"], W["ada.b"] = mat(cfg.depth * 6 * C, Ct, 0.5 / math.sqrt(Ct)), vec(cfg.depth * 6 * C)
        for i in range(cfg.depth):
            p = f"blocks.{i}."
            W[p + "norm.w"], W[p + "norm.b"] = vec(C, 0.05, 1.0), vec(C)
            for n, o in (("attn.qkv", 3 * C), ("attn.proj", C), ("cross_attn.q_linear", C), ("cross_attn.kv_linear", 2 * C),
                         ("cross_attn.proj", C)):
                W[p + n + ".w"], W[p + n + ".b"] = mat(o, C), vec(o)
            for n in ("attn.q_norm", "attn.k_norm", "cross_attn.q_norm", "cross_attn.k_norm"):
                W[p + n] = vec(128, 0.05, 1.0)
            W[p + "ffn.w13"], W[p + "ffn.w2"] = mat(2 * Hd, C), mat(C, Hd)
        self.w = W
        return self

    def param_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.w.values())

    # ------------------------------------------------------------------------------------------------------------
    _rope_fn = staticmethod(rope_tables)  # (_buf, _exchange, _rope_tables: forward_common.ForwardWorkspaces)

    def _gemm_f32(self, a: torch.Tensor, w, b, out):
        """out f32 = a f32 @ w^T + b with the fp32 activation split into a hi + lo bf16 pair (two MFMA GEMMs accumulating in fp32):
        what the reference's fp32 autocast regions compute from bf16-valued weights, to ~2^-17 relative."""
        hi = ops.cast(a, torch.bfloat16)
        lo = ops.cast(a - hi.float(), torch.bfloat16)
        gemm(hi, w, b, out, EPI_F32)
        gemm(lo, w, None, out, EPI_F32_ACC)
        return out

    def _ln(self, x, mul, add, mod_ld, rows_per_group, plus_one, out, row0=0, gidx=None):
        L, C = x.shape
        if L == 0:
            return
        call("wf_lc_ln_modulate", x.data_ptr(), mul.data_ptr(), add.data_ptr(), mod_ld, rows_per_group, row0,
             gidx.data_ptr() if gidx is not None else None, 1 if plus_one else 0, out.data_ptr(), L, C, float(self.cfg.eps), ops.stream())

    def _resid(self, x, y, gate, gate_ld, rows_per_group, row0=0, gidx=None):
        L, C = x.shape
        if L == 0:
            return
        call("wf_lc_gate_residual", x.data_ptr(), y.data_ptr(), y.stride(0), gate.data_ptr() if gate is not None else None, gate_ld,
             rows_per_group, row0, gidx.data_ptr() if gidx is not None and gate is not None else None, L, C, ops.stream())

    def _heads(self, src, col0, weight, cos, sin, out, r0, r1, out_scale=1.0, lout: Optional[int] = None):
        """Rows [r0, r1) of columns [col0, col0 + C) of src -> out [H, Lout, 128] rows [0, r1 - r0).  lout: rows between two heads of
        the destination when `out` is a row range of a larger [H, lout, 128] buffer (the noise keys behind the cached condition keys)."""
        if r1 <= r0:
            return
        view = src[r0:r1, col0:col0 + self.cfg.hidden_size]
        call("wf_lc_norm_heads", view.data_ptr(), src.stride(0), weight.data_ptr(),
             cos[r0:r1].data_ptr() if cos is not None else None, sin[r0:r1].data_ptr() if sin is not None else None,
             out.data_ptr(), r1 - r0, out.shape[1] if lout is None else lout, self.cfg.num_heads, float(self.cfg.eps), float(out_scale),
             ops.stream())

    def _vt(self, src, col0, out, L):
        view = src[:, col0:col0 + self.cfg.hidden_size]
        call("wf_v_transpose", view.data_ptr(), src.stride(0), out.data_ptr(), L, out.shape[1] * 64, self.cfg.num_heads, ops.stream())

    def _vt_at(self, src, col0, out, k0, L):
        """The same behind k0 resident keys of out [H, Lp / 64, 128, 64] (wf_v_transpose_at)."""
        view = src[:, col0:col0 + self.cfg.hidden_size]
        call("wf_v_transpose_at", view.data_ptr(), src.stride(0), out.data_ptr(), k0, L, out.shape[1] * 64, self.cfg.num_heads,
             ops.stream())

    # ------------------------------------------------------------------------------------------------------------
    # Exchange of a forward WITHOUT a lock-step partner (the distilled schedule has no CFG; see dit.WanTransformer3DModel for the modes);
    # the two samples of a CFG batch are advanced in lock-step with the one-event all-gather (forward_tokens_pair)
    exchange_mode = "chunked"
    exchange_chunks = 2
    pair_lockstep = True
    attn_prescale = True
    attn_track_max = False

    def forward_tokens(self, x_in: torch.Tensor, timesteps, caption: torch.Tensor, caption_mask: Optional[torch.Tensor] = None,
                       num_cond_latents: int = 0) -> torch.Tensor:
        """One sample.  x_in [16, T, Hh, Ww] bf16; timesteps: T host floats; caption [N, caption_channels] bf16; caption_mask [N]
        host / device ints (0 = padding) or None -> velocity [16, T, Hh, Ww] fp32  (LCD:279-366)."""
        out = [None]
        run(self._forward_steps(x_in, timesteps, caption, caption_mask, num_cond_latents, "", out, self.exchange_mode))
        return out[0]

    def forward_tokens_pair(self, sample_a, sample_b, num_cond_latents: int = 0):
        """The two samples of a CFG batch (pipeline_longcat_video.py:857-866: [negative, positive] concatenated on the batch axis; each
        sample = (x_in, timesteps, caption, caption_mask) as for forward_tokens).  The reference's batch is one tensor through one network
        call; here the two samples are two forwards advanced in LOCK-STEP, one layer apart, under sequence parallelism: while sample A's
        K / V^T all-gather of block i is in flight on the communication stream, sample B computes its block i-1 attention / FFN, and vice
        versa (the scheme of dit.WanTransformer3DModel.forward_tokens_pair).  Each sample issues exactly the kernels of forward_tokens in
        exchange mode "gather" on its own buffers: bit-identical to two sequential calls."""
        oa, ob = [None], [None]
        run(self._forward_steps(*sample_a, num_cond_latents, "", oa, "gather"),
                     self._forward_steps(*sample_b, num_cond_latents, "#b", ob, "gather"))
        return oa[0], ob[0]

    def _forward_steps(self, x_in, timesteps, caption, caption_mask, num_cond_latents, tag, result, mode="gather", vc=None):
        """Generator over one forward: yields once per dense block, right after that block's K / V^T exchange has been launched (where
        another forward can usefully take over the compute stream); `tag` separates the workspaces of concurrent forwards; the velocity
        lands in result[0].

        With `comm` (one process per GPU) the tokens are split into contiguous shards, weights replicated: every rank runs the row-wise
        work on its shard, K and blocked V^T shards are exchanged once per block (parallel.KVExchange) and consumed in place by the
        attention kernel (segment addressing), the 64-column output rows are gathered at the end.  The condition / noise split of
        LCA:123-138 is by GLOBAL token index: a rank's rows below the first frame boundary are condition queries (keys < nc), the rest
        noise queries.

        vc (video continuation, single GPU) = ("build", cache): x_in holds condition frames only -- the stream of
        LCA:127-131 / PIPE:336-348 (no caption, no cross-attention, no final layer), whose K / V^T / norm bound of every block are
        written straight into `cache`; nothing lands in result.  ("use", cache): x_in holds the noise frames only; the cache's keys are
        copied to the front of a working K / V^T pair, this step's keys are appended behind them, and everything else runs on the
        noise rows.  With block-sparse attention on (a LongCatBlockCondCache) both modes run in block order: the build also keeps
        the pooled key-block means and its selection, a step appends its own means behind the cached ones (wf_lc_mean_pool_blocks_at)
        and scores / selects / attends for the noise query blocks only, over all (nc + L) / block key blocks.

        The stages are methods on one plan and one set of workspaces; self-attention is one method per path (_sa_*)."""
        pl = self._plan(x_in, timesteps, num_cond_latents, tag, mode, vc)
        W, C, tpf = self._wl, self.cfg.hidden_size, pl.tpf
        emb = self._embed(pl, x_in, timesteps, caption, caption_mask)
        ws = self._workspaces(pl, emb.n_txt)
        ctx = self._shared_caption_kv(pl, ws, emb)
        x, ada, ald = emb.x, emb.ada, emb.ald
        if pl.use_bsa:
            self.last_bsa_indices = []
        for i in range(self.cfg.depth):
            p = f"blocks.{i}."
            m = ada[:, i * 6 * C:(i + 1) * 6 * C]
            shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = (m[:, j * C:(j + 1) * C] for j in range(6))
            last_of_build = pl.build and i == self.cfg.depth - 1
            # ---- self-attention (LCD:91-104, LCA:105-145) ----
            self._ln(x, scale_msa, shift_msa, ald, tpf, True, ws.hbuf, row0=pl.lo, gidx=pl.gidx)
            gemm(ws.hbuf, W[p + "attn.qkv.w"], W[p + "attn.qkv.b"], ws.qkv, EPI_BF16)
            if pl.use_bsa:
                self._sa_block_sparse(pl, ws, i)
                if last_of_build:
                    return  # the block-sparse build stops AFTER its last attention: it keeps that block's selection too
            elif pl.exchange is not None:
                yield from self._sa_dense_exchange(pl, ws, i)
            elif pl.cache is not None:
                self._sa_dense_cached(pl, ws, i, attend=not last_of_build)
                if last_of_build:
                    # the dense build stops BEFORE its last attention: the last block's keys are in the cache, nothing reads the
                    # condition stream behind them
                    return
            else:
                self._sa_dense_local(pl, ws, i)
            gemm(ws.ao, W[p + "attn.proj.w"], W[p + "attn.proj.b"], ws.ys, EPI_BF16)
            self._resid(x, ws.ys, gate_msa, ald, tpf, row0=pl.lo, gidx=pl.gidx)
            if not pl.build and pl.L - pl.nc > 0:  # (a build has condition rows only: LCA:127-131 skip_crs_attn)
                self._cross_attention(pl, ws, emb, ctx, i)
            # ---- SwiGLU FFN (LCD:113-120, LCB:36-37) ----
            self._ln(x, scale_mlp, shift_mlp, ald, tpf, True, ws.hbuf, row0=pl.lo, gidx=pl.gidx)
            gemm(ws.hbuf, W[p + "ffn.w13"], None, ws.ffh, EPI_BF16)
            call("wf_lc_swiglu", ws.ffh.data_ptr(), ws.ffh.stride(0), ws.ffg.data_ptr(), pl.L, self.cfg.ffn_hidden, ops.stream())
            gemm(ws.ffg, W[p + "ffn.w2"], None, ws.ys, EPI_BF16)
            self._resid(x, ws.ys, gate_mlp, ald, tpf, row0=pl.lo, gidx=pl.gidx)
        assert not pl.build
        result[0] = self._final_layer(pl, ws, emb)

    def _block_order(self, T, fc, kc, h2, w2, num_cond_latents, cos, sin):
        """The refine pass keeps the WHOLE network in 3D-block token order (bsa_interface.py:600-604): every row-wise op is order
        agnostic once the per-frame AdaLN kernels take a per-row frame index, the RoPE tables are permuted once, and the velocity rows
        are put back in (T, H, W) order at the end -- no per-layer permutes, and contiguous runs of blocks are the shards of the
        sequence-parallel job.  The first nc rows of the block order are the condition tokens.
        cos / sin: the (fc + T) grid's tables -> (block tokens, permuted cos, sin, per-row frame index, permutation, its inverse)."""
        from . import bsa
        dev, tpf = self.device, h2 * w2
        cq, ck = self.bsa_params["chunk_3d_shape_q"], self.bsa_params["chunk_3d_shape_k"]
        if list(cq) != list(ck):
            raise NotImplementedError("different query / key block shapes")
        ncl = int(num_cond_latents or 0)
        if ncl % cq[0] or (T - ncl) % cq[0]:
            raise ValueError(f"block-sparse attention needs the condition ({ncl}) and noise ({T - ncl}) latent frames to be "
                             f"multiples of {cq[0]} (the reference pads them: pipeline_longcat_video.py:1417-1419)")
        blk = cq[0] * cq[1] * cq[2]
        if kc:
            # a cached step: its rows are rows kc.. of the (fc + T) grid's block order -- that grid's permuted RoPE tables (sliced at kc
            # by the plan), and its permutation / frame indices / inverse permutation restricted to those rows, counted from the first
            # noise token / frame
            key = ("blk_vc", fc, T, h2, w2, tuple(cq))
            if key not in self._rope:
                pf, qf = bsa.block_permutation(fc + T, h2, w2, cq, dev)
                rows = pf.long()
                self._rope[key] = (cos[rows].contiguous(), sin[rows].contiguous(), (pf[kc:] // tpf - fc).to(torch.int32).contiguous(),
                                   (pf[kc:] - kc).contiguous(), (qf[kc:] - kc).contiguous())
            return (blk,) + tuple(self._rope[key])
        perm, pos = bsa.block_permutation(T, h2, w2, cq, dev)
        key = ("blk", T, h2, w2, tuple(cq))
        if key not in self._rope:
            rows = perm.long()
            self._rope[key] = (cos[rows].contiguous(), sin[rows].contiguous(), (perm // tpf).to(torch.int32).contiguous())
        return (blk,) + tuple(self._rope[key]) + (perm, pos)

    def _plan(self, x_in, timesteps, num_cond_latents, tag, mode, vc) -> _ForwardPlan:
        """Everything a forward derives from its arguments, before the first launch."""
        cfg, comm = self.cfg, self.comm
        Cin, T, Hh, Ww = x_in.shape
        assert Cin == cfg.in_channels and len(timesteps) == T
        h2, w2 = Hh // 2, Ww // 2
        tpf = h2 * w2
        build = vc is not None and vc[0] == "build"
        cached = vc is not None and not build
        cache = vc[1] if vc is not None else None
        kc, fc = (cache.nc, cache.ncl) if cached else (0, 0)
        L_tok = T * tpf
        nc_all = L_tok if build else int(num_cond_latents or 0) * tpf
        assert 0 <= nc_all < L_tok or build
        scale = 1.0 / math.sqrt(128.0)
        cos_thw, sin_thw = self._rope_tables(fc + T, h2, w2)
        use_bsa = self._bsa and fc + T > 1  # LCA:57: "bsa will not be used in image training / sampling"
        blk, cos_all, sin_all, gidx, perm, pos = (self._block_order(T, fc, kc, h2, w2, num_cond_latents, cos_thw, sin_thw) if use_bsa
                                                  else (64, cos_thw, sin_thw, None, None, None))
        sparsity, cdf_thr = (self.bsa_params.get("sparsity"), self.bsa_params.get("cdf_threshold")) if use_bsa else (None, None)
        if use_bsa and sparsity is None and cdf_thr is None:
            raise ValueError("bsa_params needs sparsity and / or cdf_threshold (bsa_interface.py:265-274)")
        if comm is not None:
            from .parallel import ShardPlan, shard_plan
            if use_bsa:  # whole 256-row query groups (two 128-token / four 64-token blocks) per rank
                per = (L_tok + comm.world - 1) // comm.world
                shard = ShardPlan(L=L_tok, P=comm.world, shard_len=(per + 255) // 256 * 256)
            else:
                shard = shard_plan(L_tok, comm.world)
            lo, hi = shard.bounds(comm.rank)
            L, Sp = hi - lo, shard.shard_len
            if L <= 0:
                raise ValueError(f"sequence-parallel plan leaves rank {comm.rank} of {comm.world} without tokens ({L_tok} tokens in shards "
                                 f"of {Sp}); use fewer ranks for this size")
        else:
            shard, lo, L, Sp = None, 0, L_tok, _pad64(kc + L_tok)
        # dense self-attention (no block gating on Q): as in the Wan DiT (dit.py), softmax_scale * log2(e) is folded into Q by its producer and
        # the kernel runs its exp2-domain form (softmax_scale = 0), without max tracking where the per-head norm bound allows it.  The
        # block-sparse pass keeps the in-kernel scale: its Q also feeds the gating.
        prescale = (not use_bsa) and bool(self.attn_prescale)
        q_scale, sa_scale = (scale * 1.4426950408889634, 0.0) if prescale else (1.0, scale)
        exchange = None
        if comm is not None and not use_bsa:  # (block-sparse blocks gather K / V^T densely instead)
            # part launches are built for the pre-scaled-Q form
            exchange = mode if prescale and comm.world > 1 else "gather"
        return _ForwardPlan(
            tag=tag, T=T, Hh=Hh, Ww=Ww, tpf=tpf, L_tok=L_tok, L_all=kc + L_tok, nc_all=nc_all, L=L, nc=min(max(nc_all - lo, 0), L), lo=lo,
            kc=kc, fc=fc, Sp=Sp, blk=blk, cos=cos_all[kc + lo:kc + lo + L], sin=sin_all[kc + lo:kc + lo + L], gidx=gidx, perm=perm, pos=pos,
            shard=shard, use_bsa=use_bsa, build=build, cached=cached, cache=cache, prescale=prescale,
            use_bounds=prescale and not self.attn_track_max, scale=scale, q_scale=q_scale, sa_scale=sa_scale, exchange=exchange,
            sparsity=sparsity, cdf_thr=cdf_thr,
            fused_sel=not os.environ.get("WF_BSA_TORCH_SELECT"))  # (the env switch keeps the torch selection paths testable)

    def _embed(self, pl, x_in, timesteps, caption, caption_mask):
        """Patch, timestep and caption embeddings -> (x: this rank's residual stream, ada / ald: the AdaLN parameters of all blocks and
        their row stride, fmod: the final layer's, y / n_txt: the caption tokens); a build has no caption and no final layer."""
        cfg, W, dev = self.cfg, self._wl, self.device
        bf, f32 = torch.bfloat16, torch.float32
        C, Ct, Cin, T = cfg.hidden_size, cfg.adaln_tembed_dim, cfg.in_channels, pl.T
        _buf = self._tagged_buf(pl)
        tok_thw = _buf("tok", (pl.L_tok, Cin * 4), bf)
        call("wf_patchify", x_in.data_ptr(), tok_thw.data_ptr(), Cin, T, pl.Hh, pl.Ww, ops.stream())
        tok = _buf("tokb", (pl.L_tok, Cin * 4), bf) if pl.use_bsa else tok_thw
        if pl.use_bsa:
            call("wf_gather_rows_bf16", tok_thw.data_ptr(), tok_thw.stride(0), pl.perm.data_ptr(), tok.data_ptr(), tok.stride(0), pl.L_tok,
                 Cin * 4, ops.stream())
        x = _buf("x", (pl.L, C), bf)
        gemm(tok[pl.lo:pl.lo + pl.L], W["patch.w"], W["patch.b"], x, EPI_BF16)  # LCB:112 (Conv3d with kernel = stride = patch)
        tf = timestep_embedding(timesteps, cfg.frequency_embedding_size).to(dev)  # LCB:201-206
        t0 = self._gemm_f32(tf, W["t_embedder.mlp.0.w"], W["t_embedder.mlp.0.b"], _buf("t0", (T, Ct), f32))
        t = self._gemm_f32(act(t0, None, f32, 0), W["t_embedder.mlp.2.w"], W["t_embedder.mlp.2.b"], _buf("t", (T, Ct), f32))
        st = act(t, None, f32, 0)  # SiLU(t), shared by every adaLN_modulation (LCD:40-43, LCB:156)
        ada = self._gemm_f32(st, W["ada.w"], W["ada.b"], _buf("ada", (T, W["ada.w"].shape[0]), f32))   # (all stored blocks: a run on the first cfg.depth blocks only reads its own columns)
        fmod, y, n_txt = None, None, 0
        if not pl.build:
            fmod = self._gemm_f32(st, W["final_layer.adaLN_modulation.1.w"], W["final_layer.adaLN_modulation.1.b"], _buf("fmod", (T, 2 * C), f32))
            # caption: Linear -> GELU(tanh) -> Linear (LCB:225-228), valid tokens only (LCD:319-325)
            cap = caption
            if caption_mask is not None:
                keep = torch.as_tensor(caption_mask).reshape(-1).to("cpu") != 0
                if not cfg.text_tokens_zero_pad:
                    cap = caption[keep.to(caption.device)]
            n_txt = cap.shape[0]
            assert n_txt > 0, "empty caption"
            yh = _buf("yh", (n_txt, C), bf)
            gemm(cap.contiguous(), W["y_embedder.y_proj.0.w"], W["y_embedder.y_proj.0.b"], yh, EPI_BF16_GELU)
            y = _buf("y", (n_txt, C), bf)
            gemm(yh, W["y_embedder.y_proj.2.w"], W["y_embedder.y_proj.2.b"], y, EPI_BF16)
            if caption_mask is not None and cfg.text_tokens_zero_pad:
                y[(~keep).to(dev)] = 0  # LCD:315-317
        return SimpleNamespace(x=x, ada=ada, ald=ada.stride(0), fmod=fmod, y=y, n_txt=n_txt)

    def _workspaces(self, pl, n_txt):
        """Every per-block workspace of this forward, and with it who holds the self-attention keys: `ex` (the exchange slots), or
        kh / vt / km (/ kcw, kh_all / vt_all) -- all None for a build, which writes the cache's own tensors."""
        cfg, comm = self.cfg, self.comm
        bf, f32 = torch.bfloat16, torch.float32
        C, H, Hd, L, nc, Sp = cfg.hidden_size, cfg.num_heads, cfg.ffn_hidden, pl.L, pl.nc, pl.Sp
        Ltp = _pad64(n_txt)
        _buf = self._tagged_buf(pl)
        ws = SimpleNamespace(ex=None, kh=None, vt=None, km=None, kcw=None, kh_all=None, vt_all=None)
        ws.hbuf = _buf("h", (L, C), bf)
        ws.qkv = _buf("qkv", (L, 3 * C), bf)
        ws.qh_c = _buf("qh_c", (H, max(nc, 1), 128), bf)
        ws.qh_n = _buf("qh_n", (H, max(L - nc, 1), 128), bf)  # (a rank of a sequence-parallel job may hold condition rows only)
        ws.qm_c = _buf("qmax2_c", (H,), f32) if pl.use_bounds else None
        ws.qm_n = _buf("qmax2_n", (H,), f32) if pl.use_bounds else None
        if pl.exchange is not None:
            # dense blocks: K, V^T and the norm bounds of this rank's shard go straight into its slot of the exchange buffers
            ws.ex = self._exchange(pl.tag, H, Sp, pl.exchange, int(self.exchange_chunks))
        elif pl.cached:
            # continuation: the working pair of ("use") has names of its own -- the uncached forward scans its zero-initialised K up to
            # the pad for the norm bound and must never find another forward's rows there; ("build") writes the cache's own tensors
            ws.kh = _buf("kh_vc", (H, Sp, 128), bf, zero=True)
            ws.vt = _buf("vt_vc", (H, Sp // 64, 128, 64), bf, zero=True)
            ws.km = _buf("kmax2_vc", (H,), f32) if pl.use_bounds else None
            ws.kcw = _buf("kcmp_vc", (H, Sp // pl.blk, 128), bf) if pl.use_bsa else None
        elif not pl.build:
            ws.kh = _buf("kh", (H, Sp, 128), bf, zero=True)
            ws.vt = _buf("vt", (H, Sp // 64, 128, 64), bf)
            ws.km = _buf("kmax2", (H,), f32) if pl.use_bounds else None
            if comm is not None:  # block-sparse blocks gather K / V^T densely (the sparse kernel addresses [P][H][S][128])
                ws.kh_all = _buf("kh_all", (comm.world, H, Sp, 128), bf, zero=True)
                ws.vt_all = _buf("vt_all", (comm.world, H, Sp // 64, 128, 64), bf)
        ws.ao = _buf("ao", (L, C), bf)
        ws.ys = _buf("ys", (L, C), bf)
        ws.qc = _buf("qc", (L, C), bf)
        ws.kvt = _buf("kvt", (n_txt, 2 * C), bf)
        ws.kth = _buf("kth", (H, Ltp, 128), bf, zero=True)
        ws.vtt = _buf("vtt", (H, Ltp // 64, 128, 64), bf)
        ws.ffh = _buf("ffh", (L, 2 * Hd), bf)
        ws.ffg = _buf("ffg", (L, Hd), bf)
        return ws

    def _caption_kv(self, ws, emb, i, kth, vtt):
        """Block i's caption keys / values (LCA:236-262) into kth [H, Ltp, 128] / vtt [H, Ltp / 64, 128, 64]."""
        W, p = self._wl, f"blocks.{i}."
        gemm(emb.y, W[p + "cross_attn.kv_linear.w"], W[p + "cross_attn.kv_linear.b"], ws.kvt, EPI_BF16)
        self._heads(ws.kvt, 0, W[p + "cross_attn.k_norm"], None, None, kth, 0, emb.n_txt)
        self._vt(ws.kvt, self.cfg.hidden_size, vtt, emb.n_txt)

    def _shared_caption_kv(self, pl, ws, emb):
        """Sequence-parallel jobs: the caption K / V^T of layer i are computed by rank i (mod P) only and all-gathered once per forward
        (see dit.py: work that does not shrink with the token shard).  -> None, or the gathered buffers
        (forward_common.GatheredLayerKV), whose first use by a cross-attention waits for the gathers."""
        cfg, comm = self.cfg, self.comm
        if comm is None or comm.world <= 1:
            return None
        bf, H, Ltp = torch.bfloat16, cfg.num_heads, _pad64(emb.n_txt)
        _buf = self._tagged_buf(pl)
        nl = layers_per_rank(cfg.depth, comm.world)
        loc = [_buf("ckv_loc0", (nl, H, Ltp, 128), bf, zero=True), _buf("ckv_loc1", (nl, H, Ltp // 64, 128, 64), bf)]
        allb = [_buf(f"ckv_all{j}", (comm.world,) + tuple(t.shape), bf) for j, t in enumerate(loc)]
        return gather_layer_kv(cfg.depth, comm, loc, allb, lambda i, kth, vtt: self._caption_kv(ws, emb, i, kth, vtt))

    # ---- self-attention, one method per path; each decides in ONE place whose K / V^T / bound it runs on ------------------------
    def _sa_queries(self, pl, ws, i):
        """Normalised, rotated (and in the dense paths pre-scaled) condition / noise queries of this rank's rows."""
        qn = self._wl[f"blocks.{i}.attn.q_norm"]
        self._heads(ws.qkv, 0, qn, pl.cos, pl.sin, ws.qh_c, 0, pl.nc, out_scale=pl.q_scale)
        self._heads(ws.qkv, 0, qn, pl.cos, pl.sin, ws.qh_n, pl.nc, pl.L, out_scale=pl.q_scale)

    def _sa_query_bounds(self, pl, ws):
        if pl.use_bounds and pl.nc > 0:
            head_max_norm2(ws.qh_c, pl.nc, ws.qm_c)
        if pl.use_bounds and pl.L - pl.nc > 0:
            head_max_norm2(ws.qh_n, pl.L - pl.nc, ws.qm_n)

    def _sa_keys(self, pl, ws, i, kh, vt, km):
        """This forward's L rows as the WHOLE key set: K into kh, V^T into vt, the norm bound into km (None: not wanted)."""
        self._heads(ws.qkv, self.cfg.hidden_size, self._wl[f"blocks.{i}.attn.k_norm"], pl.cos, pl.sin, kh, 0, pl.L)
        self._vt(ws.qkv, 2 * self.cfg.hidden_size, vt, pl.L)
        if km is not None:  # zero rows past L do not raise a maximum: the whole (padded) shard is scanned
            head_max_norm2(kh, pl.Sp, km)

    def _sa_attend(self, pl, ws, kh, vt, km):
        self._sa_query_bounds(pl, ws)
        if pl.nc > 0:  # condition tokens see condition tokens only (LCA:127-131)
            attention(ws.qh_c, kh, vt, ws.ao[:pl.nc], pl.nc_all, pl.sa_scale, kmax2=km, qmax2=ws.qm_c)
        if pl.L - pl.nc > 0:  # noise tokens see everything (LCA:133-134)
            attention(ws.qh_n, kh, vt, ws.ao[pl.nc:], pl.L_all, pl.sa_scale, profile=True, kmax2=km, qmax2=ws.qm_n)

    def _sa_dense_local(self, pl, ws, i):
        """One GPU, no cache: keys in this forward's own workspaces."""
        self._sa_queries(pl, ws, i)
        self._sa_keys(pl, ws, i, ws.kh, ws.vt, ws.km)
        self._sa_attend(pl, ws, ws.kh, ws.vt, ws.km)

    def _sa_dense_exchange(self, pl, ws, i):
        """Sequence parallel: K, V^T and the bounds of this rank's rows are written into its slots of the exchange buffers; yields
        once, right after the exchange has been launched."""
        ex, C, L, nc = ws.ex, self.cfg.hidden_size, pl.L, pl.nc
        kn = self._wl[f"blocks.{i}.attn.k_norm"]
        self._sa_queries(pl, ws, i)
        for g in range(ex.G):
            r0, r1 = ex.chunk_rows(g, L)
            if r1 > r0:
                self._heads(ws.qkv, C, kn, pl.cos, pl.sin, ex.own_k(g), r0, r1)
                self._vt(ws.qkv[r0:r1], 2 * C, ex.own_vt(g), r1 - r0)
                if pl.use_bounds:
                    head_max_norm2(ex.own_k(g), ex.chunk_len(g), ex.own_km(g))
        ex.launch()
        yield i
        self._sa_query_bounds(pl, ws)
        # the noise queries first: their sweep is what the exchange hides under; the condition queries see the first nc_all
        # keys only (rank 0's first rows), their windows are ready by then
        if L - nc > 0:
            attention_exchange(ws.qh_n, ex, ws.ao[nc:], pl.L_all, pl.sa_scale, ws.qm_n, use_bounds=pl.use_bounds, profile=True, release=False)
        if nc > 0:
            attention_exchange(ws.qh_c, ex, ws.ao[:nc], pl.nc_all, pl.sa_scale, ws.qm_c, use_bounds=pl.use_bounds, release=False,
                               comm_profile=L - nc <= 0)
        ex.wait_all()

    def _sa_dense_cached(self, pl, ws, i, attend):
        """Video continuation.  A build writes block i's rows of the cache in place (and always its norm bound); a step runs on the
        "_vc" working pair: the cached keys in front, its own behind them."""
        cache, C, H, L, kc, Sp = pl.cache, self.cfg.hidden_size, self.cfg.num_heads, pl.L, pl.kc, pl.Sp
        self._sa_queries(pl, ws, i)
        if pl.build:
            kh, vt, km = cache.k[i], cache.vt[i], cache.kmax2[i]
            self._sa_keys(pl, ws, i, kh, vt, km)
        else:
            kh, vt, km = ws.kh, ws.vt, ws.km
            # LCA:163-172 with the rotation already in the cache: cached keys [0, kc), this step's keys behind them
            ct = cache.vt.shape[2]
            kh[:, :kc].copy_(cache.k[i, :, :kc])
            vt[:, :ct].copy_(cache.vt[i])
            self._heads(ws.qkv, C, self._wl[f"blocks.{i}.attn.k_norm"], pl.cos, pl.sin, kh[:, kc:], 0, L, lout=Sp)
            self._vt_at(ws.qkv, 2 * C, vt, kc, L)
            if pl.use_bounds:
                # the un-tracked softmax body is only safe under a bound over ALL kc + L keys: the cached rows' maximum, raised
                # by the new rows' (wf_head_max_norm2 only ever raises `out`; its row window is offset to key kc)
                km.copy_(cache.kmax2[i])
                call("wf_head_max_norm2", kh[:, kc:].data_ptr(), H, L, Sp, km.data_ptr(), ops.stream())
            self.last_kmax2, self.last_vc_keys = km, (kh, kc + L)
        if attend:
            self._sa_attend(pl, ws, kh, vt, km)

    def _sa_block_sparse(self, pl, ws, i):
        """LCA:57-66 + bsa_interface.py:612-659 on rows that already are in block order: gating = mean-pooled q / k blocks ->
        bf16 block scores -> top-k / cdf selection per query block -> sparse attention over the selected key blocks."""
        from . import bsa
        comm, cache, C, H, L, nc, kc, Sp, blk = self.comm, pl.cache, self.cfg.hidden_size, self.cfg.num_heads, pl.L, pl.nc, pl.kc, pl.Sp, pl.blk
        kn = self._wl[f"blocks.{i}.attn.k_norm"]
        self._sa_queries(pl, ws, i)  # (q_scale is 1: this Q also feeds the gating)
        # the operands: kh / vt / kcmp_own = this rank's keys, values and pooled key blocks
        if pl.cached:
            # a step on a cache: the "_vc" working set, the cached keys, values and pooled means in front (kc is whole blocks), this
            # step's appended behind them
            kh, vt, kcmp_own = ws.kh, ws.vt, ws.kcw
            kh[:, :kc].copy_(cache.k[i])
            vt[:, :kc // 64].copy_(cache.vt[i])
            kcmp_own[:, :kc // blk].copy_(cache.kcmp[i])
            self._heads(ws.qkv, C, kn, pl.cos, pl.sin, kh[:, kc:], 0, L, lout=Sp)
            self._vt_at(ws.qkv, 2 * C, vt, kc, L)
            call("wf_lc_mean_pool_blocks_at", kh[:, kc:].data_ptr(), Sp, kcmp_own.data_ptr(), Sp // blk, kc // blk, H, L, blk, ops.stream())
        else:
            # a build writes block i's rows of the cache in place and copies the means there; else this forward's own workspaces
            kh, vt = (cache.k[i], cache.vt[i]) if pl.build else (ws.kh, ws.vt)
            self._sa_keys(pl, ws, i, kh, vt, None)
            kcmp_own = bsa.mean_pool(kh, blk)  # this rank's key blocks (zero rows past the last token pool to zero blocks)
            if pl.build:
                cache.kcmp[i].copy_(kcmp_own)
        kk, vv, kcmp_all = kh, vt, kcmp_own
        if comm is not None:  # sequence parallel: every rank's shards, gathered (kh_all / vt_all are workspaces of their own)
            evs = (comm.all_gather_async(ws.kh_all, kh), comm.all_gather_async(ws.vt_all, vt))
            kc_all = torch.empty((comm.world,) + tuple(kcmp_own.shape), dtype=torch.bfloat16, device=self.device)
            comm.all_gather(kc_all, kcmp_own)
            kk, vv, kcmp_all = ws.kh_all, ws.vt_all, kc_all.permute(1, 0, 2, 3).reshape(H, -1, 128)
            wait_events(evs)
        kcmp = kcmp_all[:, :pl.L_all // blk].contiguous()
        picked = []
        for nrows, qrows, orows, nkb in ((nc, ws.qh_c, ws.ao[:nc], pl.nc_all // blk), (L - nc, ws.qh_n, ws.ao[nc:], pl.L_all // blk)):
            if nrows == 0:
                continue
            sc = bsa.block_scores(bsa.mean_pool(qrows, blk), kcmp if nkb == pl.L_all // blk else kcmp[:, :nkb].contiguous())
            picked.append(self._bsa_select_attend(pl, qrows, kk, vv, orows, sc, nkb))
        self.last_bsa_indices.append(picked)
        if pl.build:
            cache.bsa_indices.append(picked[0])

    def _bsa_select_attend(self, pl, qrows, kk, vv, orows, sc, nkb):
        """Selection (bsa_interface.py:265-274) and sparse attention of one kind of query rows -> what last_bsa_indices keeps."""
        from . import bsa
        sparsity, cdf_thr, scale, blk = pl.sparsity, pl.cdf_thr, pl.scale, pl.blk
        if pl.fused_sel and nkb <= bsa.TOPK_MAX_BLOCKS and cdf_thr is None:  # selection + list building in one kernel
            return bsa.sparse_attention_topk(qrows, kk, vv, orows, sc, float(sparsity), scale, blk)
        if pl.fused_sel and nkb <= bsa.TOPK_MAX_BLOCKS:  # the cdf rule: counts (sort + scan in LDS), then the same list kernel
            return bsa.sparse_attention_cdf(qrows, kk, vv, orows, sc, float(cdf_thr), None if sparsity is None else float(sparsity), scale, blk)
        if cdf_thr is None:  # -> (block indices, per-row counts or None)
            idx, lens = bsa.select_topk(sc, float(sparsity)), None
        else:
            idx, lens = bsa.select_cdf(sc, float(cdf_thr), None if sparsity is None else float(sparsity))
        bsa.sparse_attention(qrows, kk, vv, orows, idx, scale, nkb, lens, blk)
        return idx if lens is None else (idx, lens)

    def _cross_attention(self, pl, ws, emb, ctx, i):
        """Cross-attention on the noise tokens (LCD:108-111, LCA:218-276); ctx: the gathered caption K / V^T of _shared_caption_kv."""
        W, p, x, nc, L = self._wl, f"blocks.{i}.", emb.x, pl.nc, pl.L
        self._ln(x[nc:], W[p + "norm.w"], W[p + "norm.b"], 0, 0, False, ws.hbuf[nc:])
        gemm(ws.hbuf[nc:], W[p + "cross_attn.q_linear.w"], W[p + "cross_attn.q_linear.b"], ws.qc[nc:], EPI_BF16)
        self._heads(ws.qc, 0, W[p + "cross_attn.q_norm"], None, None, ws.qh_n, nc, L)
        if ctx is not None:
            kth_i, vtt_i = ctx.layer(i)
        else:
            self._caption_kv(ws, emb, i, ws.kth, ws.vtt)
            kth_i, vtt_i = ws.kth, ws.vtt
        attention(ws.qh_n, kth_i, vtt_i, ws.ao[nc:], emb.n_txt, pl.scale)
        gemm(ws.ao[nc:], W[p + "cross_attn.proj.w"], W[p + "cross_attn.proj.b"], ws.ys[nc:], EPI_BF16)
        self._resid(x[nc:], ws.ys[nc:], None, 0, 0)

    def _final_layer(self, pl, ws, emb):
        """Final layer (LCB:159-168) + unpatchify (LCD:371-392) -> velocity [out_channels, T, Hh, Ww] fp32."""
        from .parallel import gather_rows
        cfg, W, fmod, C = self.cfg, self._wl, emb.fmod, self.cfg.hidden_size
        self._ln(emb.x, fmod[:, C:], fmod[:, :C], fmod.stride(0), pl.tpf, True, ws.hbuf, row0=pl.lo, gidx=pl.gidx)
        yo_own = self._tagged_buf(pl)("yo", (pl.L, 4 * cfg.out_channels), torch.float32)
        gemm(ws.hbuf, W["final_layer.linear.w"], W["final_layer.linear.b"], yo_own, EPI_F32)
        yo = yo_own if self.comm is None else gather_rows(self.comm, yo_own, pl.shard).contiguous()
        yt = torch.empty_like(yo) if pl.use_bsa else yo
        if pl.use_bsa:  # velocity rows back to (T, H, W) order: bsa_interface.py:606-610 (fp32 rows moved as 16-byte chunks)
            call("wf_gather_rows_bf16", yo.data_ptr(), 2 * yo.stride(0), pl.pos.data_ptr(), yt.data_ptr(), 2 * yt.stride(0), pl.L_tok,
                 2 * yo.shape[1], ops.stream())
        out = torch.empty((cfg.out_channels, pl.T, pl.Hh, pl.Ww), dtype=torch.float32, device=self.device)
        call("wf_unpatchify", yt.data_ptr(), out.data_ptr(), cfg.out_channels, pl.T, pl.Hh, pl.Ww, ops.stream())
        return out

    def _batch_samples(self, hidden_states, timestep, encoder_hidden_states, encoder_attention_mask):
        """The diffusers-style batch -> one (x_in, timesteps, caption, caption_mask) of forward_tokens per sample."""
        B, _, T, _, _ = hidden_states.shape
        ts = torch.as_tensor(timestep)
        if ts.dim() == 1:
            ts = ts.unsqueeze(1).expand(-1, T)  # LCD:299-301
        # LCD:304-306: the reference casts the timesteps to the model dtype (bf16) before embedding them
        ts = ts.to(self.dtype).float().cpu()
        cap = encoder_hidden_states
        if cap.dim() == 4:
            cap = cap[:, 0]
        samples = []
        for b in range(B):
            mask = encoder_attention_mask[b] if encoder_attention_mask is not None else None
            samples.append((bf16_latents(hidden_states[b]), ts[b].tolist(), cap[b].to(torch.bfloat16).contiguous(), mask))
        return samples

    # ---- video continuation on a resident condition cache (LCA:147-181, PIPE:336-348) --------------------------------------------
    def _vc_guard(self):
        if self.comm is not None:
            raise NotImplementedError("video continuation under sequence parallelism (`comm`) is not built")
        if self._bsa:
            raise NotImplementedError("the dense condition cache does not serve block-sparse attention: disable_bsa() first, or use "
                                      "cache_condition_blocks() / forward_cached_blocks()")

    def _cond_input(self, cond_latents):
        """cond_latents [16, ncl, Hh, Ww] -> (the same bf16, contiguous, on the device; ncl, Hh, Ww, condition tokens)."""
        x = cond_latents if cond_latents.dtype == torch.bfloat16 else ops.cast(cond_latents.contiguous(), torch.bfloat16)
        x = x.to(self.device).contiguous()
        _, ncl, Hh, Ww = x.shape
        return x, ncl, Hh, Ww, ncl * (Hh // 2) * (Ww // 2)

    def _check_cache_origin(self, cache: _CondCache, latent_hw, builder: str):
        """Either kind of cache is bound to the weights it was built with and to its latent size; builder: who makes a new one."""
        if cache.owner is not self._token or cache.wver != self._wver or cache.loras != tuple(self.active_loras) \
                or cache.linear_precision != self.linear_precision:
            raise ValueError("the condition cache was built with other weights (another model, a weight load / weights_changed(), a LoRA "
                             f"switch or another linear_precision since): build it again with {builder}")
        if tuple(latent_hw) != tuple(cache.latent_hw):
            raise ValueError(f"the condition cache holds {cache.latent_hw[0]} x {cache.latent_hw[1]} latent frames, the input is "
                             f"{latent_hw[0]} x {latent_hw[1]}")

    def cache_condition(self, cond_latents: torch.Tensor) -> LongCatCondCache:
        """PIPE:336-348 (`_cache_clean_latents`: timestep 0, skip_crs_attn, return_kv).  cond_latents [16, ncl, Hh, Ww] (normalised
        condition latents, bf16 or cast to it) -> the cache of their keys / values in every block.  Stays on the GPU
        (`offload_kv_cache` has no counterpart); shared by the samples of a CFG batch (LCA:163-165)."""
        self._vc_guard()
        cfg, dev = self.cfg, self.device
        x, ncl, Hh, Ww, nc = self._cond_input(cond_latents)
        assert nc > 0
        H, ncp = cfg.num_heads, _pad64(nc)
        cache = LongCatCondCache(
            k=torch.zeros((cfg.depth, H, ncp, 128), dtype=torch.bfloat16, device=dev),
            vt=torch.empty((cfg.depth, H, ncp // 64, 128, 64), dtype=torch.bfloat16, device=dev),
            kmax2=torch.zeros((cfg.depth, H), dtype=torch.float32, device=dev),
            ncl=ncl, nc=nc, latent_hw=(Hh, Ww), owner=self._token, wver=self._wver, loras=tuple(self.active_loras),
            linear_precision=self.linear_precision)
        run(self._forward_steps(x, [0.0] * ncl, None, None, ncl, "", [None], "gather", vc=("build", cache)))
        return cache

    def _check_cache(self, cache: LongCatCondCache, latent_hw):
        self._vc_guard()
        if not isinstance(cache, LongCatCondCache):
            raise ValueError("forward_cached / forward_tokens_cached take the dense LongCatCondCache of cache_condition()")
        self._check_cache_origin(cache, latent_hw, "cache_condition()")

    def forward_tokens_cached(self, x_in: torch.Tensor, timesteps, caption: torch.Tensor, caption_mask: Optional[torch.Tensor],
                              cache: LongCatCondCache) -> torch.Tensor:
        """One sample of LCA:149-181 `forward_with_kv_cache`: x_in [16, T, Hh, Ww] bf16 holds the NOISE frames only (frames cache.ncl ..
        of the video), timesteps their T host floats -> velocity [16, T, Hh, Ww] fp32.  The mathematical value of the noise frames of
        forward_tokens(concatenated latents, condition timesteps 0, num_cond_latents = cache.ncl): the condition stream does not depend
        on the noise tokens, the caption or the step."""
        self._check_cache(cache, x_in.shape[-2:])
        out = [None]
        run(self._forward_steps(x_in, timesteps, caption, caption_mask, 0, "", out, "gather", vc=("use", cache)))
        return out[0]

    def forward_cached(self, hidden_states: torch.Tensor, timestep: torch.Tensor, encoder_hidden_states: torch.Tensor,
                       encoder_attention_mask: Optional[torch.Tensor], cache: LongCatCondCache) -> torch.Tensor:
        """The batch form (the call of PIPE:1218-1225 with kv_cache_dict): hidden_states [B, 16, T, Hh, Ww] noise frames, the
        conversions of __call__; the samples run one after the other on the one cache.  -> fp32 [B, 16, T, Hh, Ww]."""
        samples = self._batch_samples(hidden_states, timestep, encoder_hidden_states, encoder_attention_mask)
        return torch.stack([self.forward_tokens_cached(*smp, cache) for smp in samples])

    # ---- the same on a block-ordered cache, for the block-sparse refine pass (PIPE:1271-1511 with a conditioning video) -----------
    def _vc_blocks_guard(self):
        if self.comm is not None:
            raise NotImplementedError("the block-ordered condition cache under sequence parallelism (`comm`) is not built")
        if not self._bsa:
            raise NotImplementedError("the block-ordered condition cache belongs to block-sparse attention (enable_bsa()); a dense "
                                      "model caches with cache_condition() / forward_cached()")
        cq, ck = self.bsa_params["chunk_3d_shape_q"], self.bsa_params["chunk_3d_shape_k"]
        if list(cq) != list(ck):
            raise NotImplementedError("different query / key block shapes")
        return tuple(int(c) for c in cq)

    def _vc_blocks_selection(self, n_key_blocks: int):
        """(sparsity, cdf_threshold) of bsa_params; the cdf rule is only built on its fused kernel."""
        from . import bsa
        sp, cdf = self.bsa_params.get("sparsity"), self.bsa_params.get("cdf_threshold")
        if cdf is not None and n_key_blocks > bsa.TOPK_MAX_BLOCKS:
            raise NotImplementedError(f"cdf_threshold over more than {bsa.TOPK_MAX_BLOCKS} key blocks on a condition cache is not built")
        return (None if sp is None else float(sp)), (None if cdf is None else float(cdf))

    def cache_condition_blocks(self, cond_latents: torch.Tensor) -> LongCatBlockCondCache:
        """cache_condition for a model with block-sparse attention on: cond_latents [16, ncl, Hh, Ww], ncl a whole number (> 1 frame)
        of chunk[0]-frame blocks.  The condition stream stays independent under block-sparse attention -- its queries see condition
        keys only (LCA:124-131), select among condition key blocks only, skip cross-attention and carry timestep 0 -- so it is run
        once, in block order, and K / V^T / the pooled block means of every DiT block stay resident."""
        cq = self._vc_blocks_guard()
        cfg, dev = self.cfg, self.device
        x, ncl, Hh, Ww, nc = self._cond_input(cond_latents)
        if ncl < 2 or ncl % cq[0]:
            raise ValueError(f"the block-ordered condition cache needs at least 2 condition latent frames in whole {cq[0]}-frame blocks, "
                             f"not {ncl} (the reference pads them: pipeline_longcat_video.py:1417-1419)")
        blk = cq[0] * cq[1] * cq[2]
        sp, cdf = self._vc_blocks_selection(nc // blk)
        H, bf = cfg.num_heads, torch.bfloat16
        cache = LongCatBlockCondCache(
            k=torch.empty((cfg.depth, H, nc, 128), dtype=bf, device=dev),
            vt=torch.empty((cfg.depth, H, nc // 64, 128, 64), dtype=bf, device=dev),
            kcmp=torch.empty((cfg.depth, H, nc // blk, 128), dtype=bf, device=dev), bsa_indices=[],
            ncl=ncl, nc=nc, latent_hw=(Hh, Ww), chunk=cq, sparsity=sp, cdf_threshold=cdf, owner=self._token, wver=self._wver,
            loras=tuple(self.active_loras), linear_precision=self.linear_precision)
        run(self._forward_steps(x, [0.0] * ncl, None, None, ncl, "", [None], "gather", vc=("build", cache)))
        return cache

    def _check_block_cache(self, cache: LongCatBlockCondCache, latent_hw, T: int):
        cq = self._vc_blocks_guard()
        if not isinstance(cache, LongCatBlockCondCache):
            raise ValueError("forward_cached_blocks / forward_tokens_cached_blocks take the LongCatBlockCondCache of cache_condition_blocks()")
        self._check_cache_origin(cache, latent_hw, "cache_condition_blocks()")
        blk = cq[0] * cq[1] * cq[2]
        tpf = (latent_hw[0] // 2) * (latent_hw[1] // 2)
        if cache.chunk != cq or (cache.sparsity, cache.cdf_threshold) != self._vc_blocks_selection((cache.nc + T * tpf) // blk):
            raise ValueError("the condition cache was built under other bsa_params (chunk shape, sparsity or cdf_threshold): its block "
                             "order and its selection are not this model's; build it again with cache_condition_blocks()")

    def forward_tokens_cached_blocks(self, x_in: torch.Tensor, timesteps, caption: torch.Tensor, caption_mask: Optional[torch.Tensor],
                                     cache: LongCatBlockCondCache) -> torch.Tensor:
        """forward_tokens_cached under block-sparse attention: x_in [16, T, Hh, Ww] bf16 NOISE frames (T whole chunk[0]-frame blocks)
        -> velocity [16, T, Hh, Ww] fp32 in (T, H, W) order: the value of the noise frames of forward_tokens(concatenated latents,
        condition timesteps 0, num_cond_latents = cache.ncl) with block-sparse attention on.  last_bsa_indices[i] then holds one entry,
        the noise-query selection over all (cache.nc + L) / block key blocks."""
        self._check_block_cache(cache, x_in.shape[-2:], x_in.shape[1])
        out = [None]
        run(self._forward_steps(x_in, timesteps, caption, caption_mask, 0, "", out, "gather", vc=("use", cache)))
        return out[0]

    def forward_cached_blocks(self, hidden_states: torch.Tensor, timestep: torch.Tensor, encoder_hidden_states: torch.Tensor,
                              encoder_attention_mask: Optional[torch.Tensor], cache: LongCatBlockCondCache) -> torch.Tensor:
        """The batch form: hidden_states [B, 16, T, Hh, Ww] noise frames, the conversions of __call__ -> fp32 [B, 16, T, Hh, Ww]."""
        samples = self._batch_samples(hidden_states, timestep, encoder_hidden_states, encoder_attention_mask)
        return torch.stack([self.forward_tokens_cached_blocks(*smp, cache) for smp in samples])

    def __call__(self, hidden_states: torch.Tensor, timestep: torch.Tensor, encoder_hidden_states: torch.Tensor,
                 encoder_attention_mask: Optional[torch.Tensor] = None, num_cond_latents: int = 0, return_kv: bool = False,
                 kv_cache_dict=None, skip_crs_attn: bool = False, offload_kv_cache: bool = False) -> torch.Tensor:
        if return_kv or kv_cache_dict or skip_crs_attn:
            raise NotImplementedError("the reference's kv_cache_dict protocol (LCA:147-181) is not spoken by __call__: build the condition "
                                      "cache with cache_condition() and run forward_cached() / forward_tokens_cached()")
        samples = self._batch_samples(hidden_states, timestep, encoder_hidden_states, encoder_attention_mask)
        B = len(samples)
        if B == 2 and self.comm is not None and self.comm.world > 1 and self.pair_lockstep:
            # the CFG batch (pipeline_longcat_video.py:857-866): two forwards in lock-step, each exchange hidden under the other's block
            return torch.stack(self.forward_tokens_pair(samples[0], samples[1], num_cond_latents))
        return torch.stack([self.forward_tokens(*smp, num_cond_latents) for smp in samples])
