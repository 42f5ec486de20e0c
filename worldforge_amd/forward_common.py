"""What the Wan DiT (dit.py) and the LongCat DiT (longcat_dit.py) forwards share on the host: a model's named workspaces, cached RoPE tables
and K / V^T exchange buffers, and the small drivers of their `_forward_steps` generators."""
from __future__ import annotations

import torch


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
