"""What the Wan DiT (dit.py) and the LongCat DiT (longcat_dit.py) forwards share on the host: a model's named workspaces, cached RoPE tables
and K / V^T exchange buffers, the small drivers of their `_forward_steps` generators, the once-per-forward gather of the prompt context's
K / V^T, the `wf_act` launcher, the seeded weight generators of `init_random` and the bf16 form of a call's latents."""
from __future__ import annotations

import math

import torch

from . import ops
from ._ffi import WF_BF16, WF_F32, call


class ForwardWorkspaces:
    """Mixin of a model with `device`, `comm`, the dictionaries `_ws` / `_rope`, and `_rope_fn` = its rope_tables function."""

    def _buf(self, name, shape, dtype, zero=False):
        """The workspace `name` of this shape and dtype: allocated once (everything stays resident in HBM), zeroed only then."""
        key = (name, tuple(shape), dtype)
        t = self._ws.get(key)
        if t is None:
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
            self._ws[key] = t
        return t

    def _tagged_buf(self, pl):
        """`_buf` under the plan's tag, which separates the workspaces of concurrent forwards."""
        return lambda name, shape, dtype, zero=False: self._buf(name + pl.tag, shape, dtype, zero)

    def _exchange(self, tag: str, H: int, shard_len: int, mode: str, chunks: int):
        """The K / V^T exchange buffers of the forward `tag` (parallel.KVExchange), allocated once per shape and mode."""
        from .parallel import KVExchange
        key = ("kvx" + tag, H, shard_len, mode, chunks, id(self.comm))
        ex = self._ws.get(key)
        if ex is None:
            ex = self._ws[key] = KVExchange(self.comm, H, shard_len, mode, chunks, self.device)
        return ex

    def _rope_tables(self, f, h, w):
        key = (f, h, w)
        if key not in self._rope:
            c, s = self._rope_fn(128, f, h, w)
            self._rope[key] = (c.to(self.device), s.to(self.device))
        return self._rope[key]


def run(*gens):
    """Run one `_forward_steps` generator to its end, or advance several in LOCK-STEP, in turn from yield to yield until all have
    ended: each forward's exchange is in flight while the next one computes."""
    live = list(gens)
    while live:
        for gen in list(live):
            try:
                next(gen)
            except StopIteration:
                live.remove(gen)


def wait_events(events):
    """The compute stream waits for every event of the asynchronous gathers (None: that gather was synchronous)."""
    for ev in events:
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)


class GatheredLayerKV:
    """Per-layer K / V^T that do not shrink with a rank's token shard (the prompt context of the cross-attention), computed once per
    forward by rank i (mod P) for layer i and all-gathered on the communication stream: allb = the [P, layers per rank, ...] key and
    V^T buffers, events = those of the two gathers."""

    def __init__(self, allb, P, events):
        self.allb, self.P, self.events, self._pending = allb, P, events, True

    def layer(self, i):
        """Layer i's (k, vt): slot [i % P][i // P].  The first use waits for the gathers."""
        if self._pending:
            wait_events(self.events)
            self._pending = False
        return tuple(a_[i % self.P, i // self.P] for a_ in self.allb)


def layers_per_rank(n_layers: int, P: int) -> int:
    return (n_layers + P - 1) // P


def gather_layer_kv(n_layers, comm, loc, allb, write) -> GatheredLayerKV:
    """write(i, k, vt) fills slot j of loc = [k [nl, ...], vt [nl, ...]] (nl = layers_per_rank) for every layer i = rank + P * j of this
    rank; the two buffers are then all-gathered into allb = [[P, nl, ...], [P, nl, ...]] without blocking the compute stream."""
    P = comm.world
    for j in range(layers_per_rank(n_layers, P)):
        i = comm.rank + P * j
        if i >= n_layers:
            break
        write(i, loc[0][j], loc[1][j])
    return GatheredLayerKV(allb, P, [comm.all_gather_async(a_, l_) for a_, l_ in zip(allb, loc)])


def act(a, b, out_dtype, mode):
    """wf_act of a (and b; None: a unary mode) into a fresh tensor of a's shape."""
    out = torch.empty(a.shape, dtype=out_dtype, device=a.device)
    dt = {torch.float32: WF_F32, torch.bfloat16: WF_BF16}
    call("wf_act", a.data_ptr(), dt[a.dtype], b.data_ptr() if b is not None else None, dt[b.dtype] if b is not None else 0,
         out.data_ptr(), dt[out_dtype], mode, a.numel(), ops.stream())
    return out


def seeded_generators(dev, seed: int):
    """(mat, vec) of an `init_random`: bf16 matrices [n, k] of std 1 / sqrt(k) unless given, bf16-valued fp32 vectors, drawn in call
    order from ONE generator seeded here (recorded tolerances and goldens depend on that order)."""
    g = torch.Generator(device=dev).manual_seed(seed)

    def mat(n, k, std=None):
        std = std if std is not None else 1.0 / math.sqrt(k)
        return (torch.randn(n, k, generator=g, device=dev, dtype=torch.float32) * std).to(torch.bfloat16)

    def vec(n, std=0.02, base=0.0):
        return (torch.randn(n, generator=g, device=dev, dtype=torch.float32) * std + base).to(torch.bfloat16).float()

    return mat, vec


def bf16_latents(x: torch.Tensor) -> torch.Tensor:
    """One sample's latents as the forward takes them: bf16, contiguous."""
    if x.dtype != torch.bfloat16:
        x = ops.cast(x.contiguous(), torch.bfloat16)
    return x.contiguous()
