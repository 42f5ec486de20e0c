"""The UMT5 text encoder on this engine's own kernels: token ids in, `last_hidden_state` out.

What the reference loads as `UMT5EncoderModel.from_pretrained(..., subfolder="text_encoder", torch_dtype=torch.bfloat16)` (RUN:203-204 of
the LongCat entry, PIPE:21 / INFER:191-197 of the Wan pipeline; HF = transformers/models/umt5/modeling_umt5.py) and calls once per prompt
(Wan PIPE:167-199, LongCat pipeline_longcat_video.py:90-124).  Per encoder layer:

    n   = wf_t5_rmsnorm(x)                                   UMT5LayerNorm (fp32 sum of squares, one rounding to bf16)
    qkv = wf_gemm_bf16(n, [q; k; v])                         ONE stacked [3 * H * 64, d_model] product, bf16 out
    a   = wf_t5_attn_fwd(q, k, v, bias table of THIS layer)  unscaled scores + bucketed relative-position bias + key padding
    x  += wf_gemm_bf16(a, o)                 WF_EPI_F32_ACC  the residual stream is fp32
    n   = wf_t5_rmsnorm(x)
    gu  = wf_gemm_bf16(n, [wi_0; wi_1])      WF_EPI_F32      ONE stacked [2 * d_ff, d_model] product, fp32 out
    hdn = wf_t5_gated_gelu(gu)                               gelu_new(g) * u, one rounding to bf16
    x  += wf_gemm_bf16(hdn, wo)              WF_EPI_F32_ACC

and `last_hidden_state = wf_t5_rmsnorm(x, final_layer_norm)` in bf16.  Every intermediate is at least as wide as the bf16 HF module's
(which keeps the residual stream, the scores and the probabilities in bf16).  No Hugging Face model code runs; the tokenizer (data plus
a host library) is out of scope and stays with the caller.  Not built: the T5 decoder, non-gated / ReLU feed-forwards, masks that are not
a prefix of ones, more than 512 tokens.
"""
from __future__ import annotations

import json
import math
import os
import warnings
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._ffi import call

WF_EPI_BF16, WF_EPI_F32, WF_EPI_F32_ACC = 0, 2, 4
MAX_TOKENS = 512          # wf_t5_attn_fwd keeps a head's whole K and V^T in LDS
HEAD_DIM = 64


def relative_position_bucket(rel: int, num_buckets: int = 32, max_distance: int = 128) -> int:
    """UMT5Attention._relative_position_bucket, the bidirectional (encoder) rule, for one `rel` = key position - query position,
    evaluated in integers and fp64.  Half of the buckets are for rel > 0; of each half, the first half holds |rel| exactly and the
    second half logarithmic bins up to max_distance."""
    half = num_buckets // 2
    out = half if rel > 0 else 0
    rel = abs(int(rel))
    max_exact = half // 2
    if rel < max_exact:
        return out + rel
    large = max_exact + int(math.log(rel / max_exact) / math.log(max_distance / max_exact) * (half - max_exact))
    return out + min(large, half - 1)


def bucket_lut(num_buckets: int = 32, max_distance: int = 128, lmax: int = MAX_TOKENS) -> np.ndarray:
    """uint8 [2 * lmax - 1]: entry (key - query) + (lmax - 1) = the bucket of that relative position (wf_t5_attn_fwd's table)."""
    if not 1 <= num_buckets <= 256:
        raise ValueError(f"relative_attention_num_buckets {num_buckets} does not fit the byte table")
    return np.array([relative_position_bucket(r, num_buckets, max_distance) for r in range(-(lmax - 1), lmax)], dtype=np.uint8)


@dataclass(frozen=True)
class UMT5Config:
    vocab_size: int = 256384
    d_model: int = 4096
    d_kv: int = 64
    d_ff: int = 10240
    num_layers: int = 24
    num_heads: int = 64
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6

    @property
    def inner_dim(self) -> int:
        return self.num_heads * self.d_kv

    @classmethod
    def from_dict(cls, d: dict) -> "UMT5Config":
        ff = d.get("feed_forward_proj", "gated-gelu")
        if ff != "gated-gelu":
            raise NotImplementedError(f"feed_forward_proj {ff!r}: only the gated-gelu feed-forward of UMT5 is built")
        if d.get("is_decoder"):
            raise NotImplementedError("is_decoder: the T5 decoder (causal self-attention, cross-attention) is not built")
        cfg = cls(**{k: d[k] for k in cls.__dataclass_fields__ if k in d})
        if cfg.d_kv != HEAD_DIM:
            raise NotImplementedError(f"d_kv {cfg.d_kv}: wf_t5_attn_fwd is built for 64-wide heads")
        if cfg.d_model % 8 or cfg.d_ff % 8 or min(cfg.vocab_size, cfg.d_model, cfg.d_ff, cfg.num_layers, cfg.num_heads) < 1:
            raise ValueError(f"d_model {cfg.d_model} and d_ff {cfg.d_ff} must be positive multiples of 8")
        if not 2 <= cfg.relative_attention_num_buckets <= 256:
            raise ValueError(f"relative_attention_num_buckets {cfg.relative_attention_num_buckets} outside 2..256")
        return cfg

    @classmethod
    def from_json(cls, path: str) -> "UMT5Config":
        with open(path) as f:
            return cls.from_dict(json.load(f))


ALIAS = "encoder.embed_tokens.weight"    # tied to shared.weight: accepted, not required, never uploaded twice


def expected_state_dict(cfg: UMT5Config) -> Dict[str, Tuple[int, ...]]:
    """{HF key: shape} of what the encoder consumes."""
    d, inner, F = cfg.d_model, cfg.inner_dim, cfg.d_ff
    out: Dict[str, Tuple[int, ...]] = {"shared.weight": (cfg.vocab_size, d)}
    for i in range(cfg.num_layers):
        b = f"encoder.block.{i}.layer."
        for n in "qkv":
            out[f"{b}0.SelfAttention.{n}.weight"] = (inner, d)
        out[f"{b}0.SelfAttention.o.weight"] = (d, inner)
        out[f"{b}0.SelfAttention.relative_attention_bias.weight"] = (cfg.relative_attention_num_buckets, cfg.num_heads)
        out[f"{b}0.layer_norm.weight"] = (d,)
        out[f"{b}1.DenseReluDense.wi_0.weight"] = (F, d)
        out[f"{b}1.DenseReluDense.wi_1.weight"] = (F, d)
        out[f"{b}1.DenseReluDense.wo.weight"] = (d, F)
        out[f"{b}1.layer_norm.weight"] = (d,)
    out["encoder.final_layer_norm.weight"] = (d,)
    return out


def consumed_header(found: Dict[str, dict]) -> Tuple[Dict[str, dict], int]:
    """The entries of a checkpoint header the encoder looks at: `decoder.*` / `lm_head.*` (a full UMT5 checkpoint) dropped, the tied
    alias folded into `shared.weight` (kept under that name when the file holds only the alias) -> (entries, number dropped)."""
    keep = {k: v for k, v in found.items() if not k.startswith(("decoder.", "lm_head."))}
    dropped = len(found) - len(keep)
    if ALIAS in keep:
        alias = keep.pop(ALIAS)
        keep.setdefault("shared.weight", alias)
    return keep, dropped


def check_mask(attention_mask: torch.Tensor) -> int:
    """The number of leading ones of a [L] mask that is ones followed by zeros with at least one 1; ValueError otherwise."""
    m = attention_mask.detach().to("cpu").reshape(-1)
    n = int((m != 0).sum())
    if n < 1 or bool((m[:n] == 0).any()) or bool(((m != 0) & (m != 1)).any()):
        raise ValueError("attention_mask must be ones followed by zeros with at least one 1 (the tokenizer's right padding)")
    return n


class UMT5EncoderModel:
    def __init__(self, cfg: UMT5Config, device="cuda:0"):
        self.cfg = cfg
        self.device = torch.device(device)
        self.W: Dict[str, torch.Tensor] = {}
        self.lut = torch.from_numpy(bucket_lut(cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance)).to(self.device)

    # ---- weights -----------------------------------------------------------------------------------------------------------------------
    def _assemble(self, get):
        """get(key) -> the CPU tensor of an HF key.  Every tensor is rounded to bf16 first (what torch_dtype=torch.bfloat16 does to the
        reference module's parameters), matrices stay bf16, vectors and the bias tables become fp32 holding the bf16 values."""
        cfg, dev, bf = self.cfg, self.device, torch.bfloat16
        mat = lambda t: t.to(bf).to(dev).contiguous()  # noqa: E731
        vec = lambda t: t.to(bf).to(dev).to(torch.float32).contiguous()  # noqa: E731
        W = {"embed": mat(get("shared.weight")), "final_ln": vec(get("encoder.final_layer_norm.weight"))}
        for i in range(cfg.num_layers):
            b = f"encoder.block.{i}.layer."
            a = b + "0.SelfAttention."
            W[f"{i}.qkv"] = torch.cat([mat(get(a + n + ".weight")) for n in "qkv"], 0).contiguous()
            W[f"{i}.o"] = mat(get(a + "o.weight"))
            W[f"{i}.bias"] = vec(get(a + "relative_attention_bias.weight")).t().contiguous()       # [H][num_buckets]
            W[f"{i}.ln0"] = vec(get(b + "0.layer_norm.weight"))
            W[f"{i}.wi"] = torch.cat([mat(get(b + "1.DenseReluDense.wi_0.weight")), mat(get(b + "1.DenseReluDense.wi_1.weight"))], 0).contiguous()
            W[f"{i}.wo"] = mat(get(b + "1.DenseReluDense.wo.weight"))
            W[f"{i}.ln1"] = vec(get(b + "1.layer_norm.weight"))
        self.W = W
        return self

    def init_random(self, seed: int = 0):
        """Synthetic weights of the right shapes, generated on the device (benchmarks: there are no checkpoints offline)."""
        cfg, dev = self.cfg, self.device
        g = torch.Generator(device=dev).manual_seed(seed)
        d, inner, F = cfg.d_model, cfg.inner_dim, cfg.d_ff

        def mat(n, k, std=None):
            return (torch.randn(n, k, generator=g, device=dev, dtype=torch.float32) * (std or k ** -0.5)).to(torch.bfloat16)

        def vec(*shape, std=0.1, base=1.0):
            return (torch.randn(*shape, generator=g, device=dev, dtype=torch.float32) * std + base).to(torch.bfloat16).float()

        W = {"embed": mat(cfg.vocab_size, d, 1.0), "final_ln": vec(d)}
        for i in range(cfg.num_layers):
            W[f"{i}.qkv"] = torch.cat([mat(inner, d, 0.7 * d ** -0.5), mat(inner, d, 0.7 * d ** -0.5), mat(inner, d)], 0)
            W[f"{i}.o"], W[f"{i}.bias"], W[f"{i}.ln0"] = mat(d, inner), vec(cfg.num_heads, cfg.relative_attention_num_buckets, std=2.0, base=0.0), vec(d)
            W[f"{i}.wi"], W[f"{i}.wo"], W[f"{i}.ln1"] = mat(2 * F, d), mat(d, F), vec(d)
        self.W = W
        return self

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        """An HF state dict (tests): the same key rules as from_pretrained."""
        found = {k: {"shape": tuple(v.shape)} for k, v in sd.items()}
        keep, dropped = consumed_header(found)
        _raise_on(keep, self.cfg, "state dict", dropped)
        src = dict(sd)
        if "shared.weight" not in src:
            src["shared.weight"] = src[ALIAS]
        return self._assemble(lambda k: src[k])

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0", subfolder: Optional[str] = "text_encoder"):
        """`<path>/<subfolder>/config.json` + one safetensors file or an index with shards.  The headers are checked against
        expected_state_dict before a byte is uploaded: a missing key is a KeyError, an unexpected key or a wrong shape a ValueError;
        `decoder.*` / `lm_head.*` are ignored with one warning.  Tensors go from the memory map to the device one at a time."""
        from . import checkpoint
        folder = os.path.join(path, subfolder) if subfolder and os.path.isdir(os.path.join(path, subfolder)) else path
        cj = os.path.join(folder, "config.json")
        if not os.path.exists(cj):
            raise FileNotFoundError(f"{folder}: no config.json")
        cfg = UMT5Config.from_json(cj)
        found, info = checkpoint.dir_header(folder)
        if info["missing_shards"]:
            raise FileNotFoundError(f"{folder}: shards named by {info['index']} are missing: {info['missing_shards']}")
        keep, dropped = consumed_header(found)
        _raise_on(keep, cfg, folder, dropped)
        model = cls(cfg, device)
        sd = checkpoint.load_dir(folder)   # memory-mapped: a tensor's bytes are read when it is converted
        return model._assemble(lambda k: sd[k] if k in sd else sd[ALIAS])

    # ---- forward -----------------------------------------------------------------------------------------------------------------------
    def _gemm(self, x, w, out, epi):
        M, K = x.shape
        call("wf_gemm_bf16", x.data_ptr(), w.data_ptr(), None, out.data_ptr(), None, M, w.shape[0], K, x.stride(0), w.stride(0),
             out.stride(0), epi, ops.stream())

    def _norm(self, x, w, out):
        call("wf_t5_rmsnorm", x.data_ptr(), w.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], float(self.cfg.layer_norm_epsilon),
             ops.stream())

    def _encode_one(self, ids: torch.Tensor, kv_len: int) -> torch.Tensor:
        cfg, dev, W = self.cfg, self.device, self.W
        L, d, inner, F, H = ids.numel(), cfg.d_model, cfg.inner_dim, cfg.d_ff, cfg.num_heads
        bf, st = torch.bfloat16, ops.stream()
        x = torch.empty(L, d, dtype=torch.float32, device=dev)
        n = torch.empty(L, d, dtype=bf, device=dev)
        qkv = torch.empty(L, 3 * inner, dtype=bf, device=dev)
        att = torch.empty(L, inner, dtype=bf, device=dev)
        gu = torch.empty(L, 2 * F, dtype=torch.float32, device=dev)
        hdn = torch.empty(L, F, dtype=bf, device=dev)
        call("wf_t5_embed", ids.data_ptr(), W["embed"].data_ptr(), x.data_ptr(), L, cfg.vocab_size, d, st)
        esz = qkv.element_size()
        for i in range(cfg.num_layers):
            self._norm(x, W[f"{i}.ln0"], n)
            self._gemm(n, W[f"{i}.qkv"], qkv, WF_EPI_BF16)
            call("wf_t5_attn_fwd", qkv.data_ptr(), qkv.data_ptr() + inner * esz, qkv.data_ptr() + 2 * inner * esz, 3 * inner,
                 att.data_ptr(), inner, W[f"{i}.bias"].data_ptr(), self.lut.data_ptr(), MAX_TOKENS, cfg.relative_attention_num_buckets,
                 H, L, kv_len, st)
            self._gemm(att, W[f"{i}.o"], x, WF_EPI_F32_ACC)
            self._norm(x, W[f"{i}.ln1"], n)
            self._gemm(n, W[f"{i}.wi"], gu, WF_EPI_F32)
            call("wf_t5_gated_gelu", gu.data_ptr(), 2 * F, hdn.data_ptr(), L, F, st)
            self._gemm(hdn, W[f"{i}.wo"], x, WF_EPI_F32_ACC)
        out = torch.empty(L, d, dtype=bf, device=dev)
        self._norm(x, W["final_ln"], out)
        return out

    def __call__(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        """input_ids / attention_mask [B, L] (or [L]) -> last_hidden_state bf16 [B, L, d_model]: all L rows, the pad rows included, as
        HF returns them.  Refused before any device work (ValueError): ids outside [0, vocab), L > 512, a mask that is not ones
        followed by zeros with at least one 1."""
        if not self.W:
            raise RuntimeError("UMT5EncoderModel has no weights: from_pretrained or load_state_dict first")
        ids = input_ids.detach().to("cpu").reshape(-1, input_ids.shape[-1]).to(torch.int64)
        mask = attention_mask.detach().to("cpu").reshape(-1, attention_mask.shape[-1])
        if ids.shape != mask.shape:
            raise ValueError(f"input_ids {tuple(ids.shape)} and attention_mask {tuple(mask.shape)} disagree")
        B, L = ids.shape
        if not 1 <= L <= MAX_TOKENS:
            raise ValueError(f"{L} tokens: the encoder takes 1..{MAX_TOKENS}")
        if int(ids.min()) < 0 or int(ids.max()) >= self.cfg.vocab_size:
            raise ValueError(f"input_ids outside [0, {self.cfg.vocab_size})")
        lens = [check_mask(mask[b]) for b in range(B)]
        ids_dev = ids.to(torch.int32).to(self.device)
        return torch.stack([self._encode_one(ids_dev[b], lens[b]) for b in range(B)], 0)


def _raise_on(keep: Dict[str, dict], cfg: UMT5Config, where: str, dropped: int):
    from .checkpoint import compare_header
    if dropped:
        warnings.warn(f"{where}: {dropped} decoder.* / lm_head.* tensors are not part of the encoder and are ignored", UserWarning, stacklevel=3)
    missing, unexpected, wrong = compare_header(keep, expected_state_dict(cfg))
    if missing:
        raise KeyError(f"{where}: {len(missing)} parameters of the encoder are not in the checkpoint: {missing[:5]}")
    if wrong:
        w = wrong[0]
        raise ValueError(f"{where}: {len(wrong)} parameters have the wrong shape: {w['key']} is {w['found']}, expected {w['expected']}")
    if unexpected:
        raise ValueError(f"{where}: {len(unexpected)} checkpoint tensors are not consumed by the encoder: {unexpected[:5]}")


# ---- the two layouts the pipelines take --------------------------------------------------------------------------------------------------
def to_longcat(h: torch.Tensor, mask: torch.Tensor):
    """pipeline_longcat_video.py:116-124: last_hidden_state [1, L, C] -> prompt_embeds [1, 1, L, C] (all rows) + the mask [1, L] int64."""
    if h.dim() != 3 or h.shape[0] != 1:
        raise ValueError(f"expected [1, L, C], got {tuple(h.shape)}")
    return h.view(1, 1, h.shape[1], h.shape[2]), mask.reshape(1, -1).to(torch.int64).to(h.device)


def to_wan(h: torch.Tensor, mask: torch.Tensor, max_sequence_length: int = MAX_TOKENS) -> torch.Tensor:
    """Wan PIPE:190-199: the rows of the prompt's own tokens, exact zeros behind them, [1, max_sequence_length, C]."""
    if h.dim() != 3 or h.shape[0] != 1:
        raise ValueError(f"expected [1, L, C], got {tuple(h.shape)}")
    n = check_mask(mask.reshape(-1))
    out = h.new_zeros(1, max_sequence_length, h.shape[2])
    out[0, :n] = h[0, :n]
    return out


def encode_prompts(folder: str, texts: Dict[str, str], device, tokenizer=None, max_sequence_length: int = MAX_TOKENS,
                   subfolder: Optional[str] = "text_encoder"):
    """{name: text} -> {name: (last_hidden_state bf16 [1, L, C], attention mask [1, L])} with the folder's tokenizer (`tokenizer/`,
    loaded with `transformers.AutoTokenizer` unless one is given: any callable with the Hugging Face tokenizer signature) and THIS
    encoder, which is built for the call and freed afterwards."""
    if tokenizer is None:
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(os.path.join(folder, "tokenizer"), local_files_only=True)
    te = UMT5EncoderModel.from_pretrained(folder, device=device, subfolder=subfolder)
    out = {}
    for name, text in texts.items():
        t = tokenizer([text], padding="max_length", max_length=max_sequence_length, truncation=True, add_special_tokens=True,
                      return_attention_mask=True, return_tensors="pt")
        out[name] = (te(t.input_ids, t.attention_mask), t.attention_mask.to(torch.int64))
    del te
    if torch.device(device).type == "cuda":
        torch.cuda.empty_cache()
    return out
