"""Pillow's 8-bit resample restated on the host: the coefficient tables `PIL.Image.resize` builds for the bicubic filter (its default for
modes RGB and L; filter_tables: for each of its five convolution filters, with that filter's kernel and support), a numpy emulation of its two passes, and the two 256-entry u8 -> f32 tables of harness.prepare_inputs.

The contract (Pillow's Resample.c, 8 bits per channel), per axis, in float64:
    scale = in / out, filterscale = max(scale, 1), support = 2 filterscale, centre_i = (i + 0.5) scale,
    first_i = max(0, int(centre_i - support + 0.5)), count_i = min(in, int(centre_i + support + 0.5)) - first_i,
    w_ij = bicubic((j + first_i - centre_i + 0.5) (1 / filterscale)) with a = -0.5, summed in index order, each divided by the sum,
    k_ij = int(w_ij 2^22 + 0.5) for w_ij >= 0, int(w_ij 2^22 - 0.5) below (truncation towards zero), zeros behind count_i;
    out = clamp(((1 << 21) + sum_j px[first + j] k_j) >> 22, 0, 255) in int32.
The horizontal pass runs first and leaves a uint8 image, the vertical pass reads that; a pass whose size does not change is skipped.
The tables feed wf_resample_u8 (ops.resample_u8) and wf_resample_u8_window_f32 (ops.resample_u8_window); the emulation is the CPU yardstick and needs no PIL."""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

PRECISION_BITS = 22     # 32 - 8 - 2
BICUBIC_SUPPORT = 2.0


def _bicubic(x: np.ndarray) -> np.ndarray:
    """Keys' cubic with a = -0.5, evaluated in Horner form."""
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    outer = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def pil_resample_tables(in_size: int, out_size: int, filter: str = "bicubic") -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 [out, 2] = (first tap, tap count), coefs int32 [out, ksize]) of one axis, ksize = ceil(support) * 2 + 1."""
    if filter != "bicubic":
        raise ValueError(f"filter {filter!r}: only bicubic is built")
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = BICUBIC_SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    centre = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    first = np.maximum(np.trunc(centre - support + 0.5).astype(np.int64), 0)
    last = np.minimum(np.trunc(centre + support + 0.5).astype(np.int64), in_size)
    count = last - first
    j = np.arange(ksize, dtype=np.int64)[None, :]
    live = j < count[:, None]
    w = np.where(live, _bicubic(((j + first[:, None]).astype(np.float64) - centre[:, None] + 0.5) * inv), 0.0)
    total = np.zeros(out_size, dtype=np.float64)
    for t in range(ksize):               # in index order, one rounding per addition (a pairwise sum would round differently)
        total = total + w[:, t]
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    w = np.where(live, w, 0.0)
    fixed = np.trunc(np.where(w < 0.0, -0.5, 0.5) + w * float(1 << PRECISION_BITS))
    bounds = np.stack([first, count], axis=1).astype(np.int32)
    return np.ascontiguousarray(bounds), np.ascontiguousarray(fixed.astype(np.int32))


def _box(x: float) -> float:
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x: float) -> float:
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# Pillow's convolution filters: (kernel of one float64, support).  Bicubic is pil_resample_tables' own array code.
FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "hamming": (_hamming, 1.0), "bicubic": (None, BICUBIC_SUPPORT),
           "lanczos": (_lanczos, 3.0)}


def filter_tables(in_size: int, out_size: int, filter: str = "bicubic") -> Tuple[np.ndarray, np.ndarray]:
    """pil_resample_tables for any of Pillow's five convolution filters: the module's contract with the filter's own kernel and support.
    The taps are evaluated one at a time with the C library's sin / cos (math.sin, math.cos), as Pillow does; "bicubic" returns
    pil_resample_tables' arrays.  NEAREST is no convolution in Pillow (it goes through the affine transform) and is refused."""
    if filter not in FILTERS:
        raise ValueError(f"filter {filter!r}: one of {sorted(FILTERS)}")
    if filter == "bicubic":
        return pil_resample_tables(in_size, out_size)
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"sizes must be positive, got {in_size} -> {out_size}")
    kernel, support = FILTERS[filter]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coefs = np.zeros((out_size, ksize), dtype=np.int32)
    for i in range(out_size):
        centre = (i + 0.5) * scale
        first = max(int(centre - support + 0.5), 0)
        count = min(int(centre + support + 0.5), in_size) - first
        w = [kernel((j + first - centre + 0.5) * inv) for j in range(count)]
        total = 0.0
        for v in w:                      # in index order, one rounding per addition
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        bounds[i] = (first, count)
        coefs[i, :count] = [int(v * float(1 << PRECISION_BITS) + (-0.5 if v < 0.0 else 0.5)) for v in w]
    return bounds, coefs


def _pass(a: np.ndarray, axis: int, bounds: np.ndarray, coefs: np.ndarray) -> np.ndarray:
    """One pass along `axis` of a uint8 array; the sum cannot leave int32 (|sum| <= 255 sum |k| < 2^31), int64 here is the same number."""
    n_in = a.shape[axis]
    shape = [1] * a.ndim
    shape[axis] = -1
    acc = np.full(a.shape[:axis] + (bounds.shape[0],) + a.shape[axis + 1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for t in range(coefs.shape[1]):
        idx = np.minimum(bounds[:, 0].astype(np.int64) + t, n_in - 1)   # behind the count the coefficient is zero
        acc += np.take(a, idx, axis=axis).astype(np.int64) * coefs[:, t].astype(np.int64).reshape(shape)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resample_u8_numpy(a: np.ndarray, size_hw, channels_last: bool = True, filter: str = "bicubic") -> np.ndarray:
    """`np.array(Image.fromarray(a).resize((W, H), filter))` per image: uint8 a [..., h, w, C] (channels_last) or [..., h, w], any leading
    axes; `filter` one of FILTERS."""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError(f"uint8 only, got {a.dtype}")
    H, W = int(size_hw[0]), int(size_hw[1])
    ay, ax = (a.ndim - 3, a.ndim - 2) if channels_last else (a.ndim - 2, a.ndim - 1)
    if a.shape[ax] != W:
        a = _pass(a, ax, *filter_tables(a.shape[ax], W, filter))
    if a.shape[ay] != H:
        a = _pass(a, ay, *filter_tables(a.shape[ay], H, filter))
    return a


def u8_to_f32_tables() -> Tuple[np.ndarray, np.ndarray]:
    """(frames table, masks table), float32 [256] each, with harness.prepare_inputs' own two expressions on all 256 inputs:
    `torch.tensor(u8).float() / 255.0` for the frames and `(u8 / 255.0).astype(float32)` (float64 division, then rounding) for the masks."""
    import torch
    u8 = np.arange(256, dtype=np.uint8)
    frames = (torch.tensor(u8).float() / 255.0).numpy()
    masks = (u8 / 255.0).astype(np.float32)
    return frames, masks
