"""Tensor-level wrappers over the C-ABI (include/wf_hip.h) for the scheduler / injection set.

PyTorch is used for device memory and streams only: every function takes CUDA(ROCm) tensors, allocates the output with
torch.empty and launches the HIP kernel on torch's current stream.  There is no CPU path here.
"""
from __future__ import annotations

from typing import Optional, Sequence

import threading

import torch

from . import _ffi
from ._ffi import WF_BF16, WF_F32, call


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return WF_F32
    if t.dtype == torch.bfloat16:
        return WF_BF16
    raise TypeError(f"unsupported dtype {t.dtype} (float32 / bfloat16 only)")


def _dev(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError("worldforge_amd ops need device tensors (there is no CPU fallback)")
    return t if t.is_contiguous() else t.contiguous()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _promote(*ts: torch.Tensor) -> torch.dtype:
    return torch.bfloat16 if all(t.dtype == torch.bfloat16 for t in ts) else torch.float32


def cfg_combine(cond: torch.Tensor, uncond: torch.Tensor, g: float) -> torch.Tensor:
    """PIPE:611."""
    cond, uncond = _dev(cond), _dev(uncond)
    assert cond.dtype == uncond.dtype and cond.shape == uncond.shape
    out = torch.empty_like(cond)
    call("wf_cfg_combine", cond.data_ptr(), uncond.data_ptr(), out.data_ptr(), _dt(cond), float(g), cond.numel(), stream())
    return out


def x0_from_v(sample: torch.Tensor, v: torch.Tensor, sigma: float) -> torch.Tensor:
    """SCHED:958."""
    sample, v = _dev(sample), _dev(v)
    assert sample.shape == v.shape
    out = torch.empty(sample.shape, dtype=_promote(sample, v), device=sample.device)
    call("wf_x0_from_v", sample.data_ptr(), _dt(sample), v.data_ptr(), _dt(v), out.data_ptr(), float(sigma), sample.numel(),
         stream())
    return out


def unipc_update(x: torch.Tensor, m0: torch.Tensor, m1: Optional[torch.Tensor], c1: float, c2: float, c3: float,
                 rk: float) -> torch.Tensor:
    """SCHED:1083-1098."""
    x, m0 = _dev(x), _dev(m0)
    out = torch.empty_like(x)
    if m1 is not None:
        m1 = _dev(m1)
        call("wf_unipc_update", x.data_ptr(), _dt(x), m0.data_ptr(), _dt(m0), m1.data_ptr(), _dt(m1), out.data_ptr(),
             float(c1), float(c2), float(c3), float(rk), x.numel(), stream())
    else:
        call("wf_unipc_update", x.data_ptr(), _dt(x), m0.data_ptr(), _dt(m0), None, 0, out.data_ptr(), float(c1), float(c2),
             float(c3), 1.0, x.numel(), stream())
    return out


def add_noise(x0: torch.Tensor, noise: torch.Tensor, one_minus_sigma: float, sigma: float) -> torch.Tensor:
    """SCHED:1584."""
    x0, noise = _dev(x0), _dev(noise)
    out = torch.empty(x0.shape, dtype=_promote(x0, noise), device=x0.device)
    call("wf_add_noise", x0.data_ptr(), _dt(x0), noise.data_ptr(), _dt(noise), out.data_ptr(), float(one_minus_sigma),
         float(sigma), x0.numel(), stream())
    return out


def _chan_consts(mean: Sequence[float], std: Sequence[float], dtype: torch.dtype):
    m = torch.tensor(list(mean)).to(dtype)
    istd = 1.0 / torch.tensor(list(std)).to(dtype)
    return _ffi.farr(m.float().tolist()), _ffi.farr(istd.float().tolist())


def latent_denorm(z: torch.Tensor, mean, std) -> torch.Tensor:
    """SCHED:1272-1282 / PIPE:742: (z / (1/std) + mean) in z's dtype, returned as fp32."""
    z = _dev(z)
    B, C = z.shape[0], z.shape[1]
    inner = z.numel() // (B * C)
    m, s = _chan_consts(mean, std, z.dtype)
    out = torch.empty(z.shape, dtype=torch.float32, device=z.device)
    call("wf_latent_affine", z.data_ptr(), _dt(z), out.data_ptr(), WF_F32, m, s, 0, B, C, inner, stream())
    return out


def latent_norm(mu: torch.Tensor, mean, std, const_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """SCHED:1385 / PIPE:351: (mu - mean) * (1/std) with constants held in `const_dtype`; mu fp32 -> fp32."""
    mu = _dev(mu)
    assert mu.dtype == torch.float32
    B, C = mu.shape[0], mu.shape[1]
    inner = mu.numel() // (B * C)
    m, s = _chan_consts(mean, std, const_dtype)
    out = torch.empty_like(mu)
    call("wf_latent_affine", mu.data_ptr(), WF_F32, out.data_ptr(), WF_F32, m, s, 1, B, C, inner, stream())
    return out


PROFILE_BLEND = None  # bench.py sets this to a list: (start, end, bytes) HIP events around every wf_blend_pixels launch (HBM GB/s)


def blend_pixels(ref: torch.Tensor, mask: torch.Tensor, dec: torch.Tensor) -> torch.Tensor:
    """SCHED:1375-1381.  ref [B,3,F,H,W] fp32, mask [B,1,F,H,W] fp32; dec fp32 -> fp32, or dec bf16 (a bf16 VAE module, the LongCat
    entry's: the statements then run in bf16, LongCat SCHED:1152-1164) -> bf16."""
    ref, mask, dec = _dev(ref), _dev(mask), _dev(dec)
    assert ref.dtype == mask.dtype == torch.float32 and dec.dtype in (torch.float32, torch.bfloat16)
    assert ref.shape == dec.shape and mask.shape[1] == 1 and mask.shape[2:] == dec.shape[2:]
    B, C = dec.shape[0], dec.shape[1]
    inner = dec.numel() // (B * C)
    out = torch.empty_like(dec)
    if dec.dtype == torch.bfloat16:
        call("wf_blend_pixels_bf16", ref.data_ptr(), mask.data_ptr(), dec.data_ptr(), out.data_ptr(), B, C, inner, stream())
        return out
    prof = PROFILE_BLEND
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    call("wf_blend_pixels", ref.data_ptr(), mask.data_ptr(), dec.data_ptr(), out.data_ptr(), B, C, inner, stream())
    if prof is not None:
        e1.record()
        # algorithmic bytes: read ref (C ch) + mask (1 ch, broadcast) + dec (C ch), write fused (C ch), fp32
        prof.append((e0, e1, 4 * B * inner * (3 * C + 1)))
    return out


def postprocess_video(x: torch.Tensor) -> torch.Tensor:
    """PIPE:744: [C,F,H,W] in [-1,1] -> [F,H,W,C] in [0,1] (fp32; a bf16 video is processed in bf16 and converted, as diffusers does)."""
    x = _dev(x)
    assert x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 4
    C, F, H, W = x.shape
    out = torch.empty((F, H, W, C), dtype=torch.float32, device=x.device)
    if x.dtype == torch.bfloat16:
        call("wf_postprocess_video_bf16", x.data_ptr(), out.data_ptr(), C, F, H, W, stream())
        return out
    call("wf_postprocess_video", x.data_ptr(), out.data_ptr(), C, F, H, W, stream())
    return out


def cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    x = _dev(x)
    if x.dtype == dtype:
        return x
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    call("wf_cast", x.data_ptr(), _dt(x), out.data_ptr(), _dt(out), x.numel(), stream())
    return out


def channel_swap_(enc: torch.Tensor, pred: torch.Tensor, channels: Sequence[int]) -> torch.Tensor:
    """SCHED:1410-1412 in place on enc."""
    if len(channels) == 0:
        return enc
    assert enc.is_contiguous() and enc.is_cuda
    pred = _dev(pred)
    B, C = enc.shape[0], enc.shape[1]
    inner = enc.numel() // (B * C)
    call("wf_channel_swap", enc.data_ptr(), _dt(enc), pred.data_ptr(), _dt(pred), _ffi.iarr(channels), len(channels), B, C,
         inner, stream())
    return enc


def resize_bilinear2d(x: torch.Tensor, Ho: int, Wo: int) -> torch.Tensor:
    """SCHED:1316-1324 on [..., Hi, Wi] fp32."""
    x = _dev(x)
    assert x.dtype == torch.float32
    Hi, Wi = x.shape[-2:]
    N = x.numel() // (Hi * Wi)
    out = torch.empty(x.shape[:-2] + (Ho, Wo), dtype=torch.float32, device=x.device)
    call("wf_resize_bilinear2d", x.data_ptr(), out.data_ptr(), N, Hi, Wi, Ho, Wo, stream())
    return out


def resize_nearest2d(x: torch.Tensor, Ho: int, Wo: int) -> torch.Tensor:
    """SCHED:1355-1362 on [..., Hi, Wi] fp32."""
    x = _dev(x)
    assert x.dtype == torch.float32
    Hi, Wi = x.shape[-2:]
    N = x.numel() // (Hi * Wi)
    out = torch.empty(x.shape[:-2] + (Ho, Wo), dtype=torch.float32, device=x.device)
    call("wf_resize_nearest2d", x.data_ptr(), out.data_ptr(), N, Hi, Wi, Ho, Wo, stream())
    return out


_WS = {}


def _workspace(key, nfloats, device):
    """Scratch buffer for the multi-launch entry points (DSG, flow metric, Farneback, split attention), one per calling thread: the
    launches of one call must not interleave with another thread's launches on the same buffer (the simulated-rank tests run several
    ranks as threads of one process; a real job has one process per GPU)."""
    k = (key, device, threading.get_ident())
    t = _WS.get(k)
    if t is None or t.numel() < nfloats:
        t = torch.empty(int(nfloats), dtype=torch.float32, device=device)
        _WS[k] = t
    return t


def dsg(good: torch.Tensor, worse: torch.Tensor, omega: float) -> torch.Tensor:
    """PIPE:669-681, one fused call, no host sync."""
    good, worse = _dev(good), _dev(worse)
    assert good.dtype == worse.dtype and good.shape == worse.shape
    ws = _workspace("dsg", _ffi.lib().wf_dsg_workspace_floats(), good.device)
    out = torch.empty_like(good)
    call("wf_dsg", good.data_ptr(), worse.data_ptr(), out.data_ptr(), _dt(good), float(omega), good.numel(), ws.data_ptr(),
         stream())
    return out


def cfg_zero(cond: torch.Tensor, uncond: torch.Tensor, guidance: float, negate: bool = False) -> torch.Tensor:
    """LongCat CFG-zero (pipeline_longcat_video.py:374-383, 875-888) for one sample, one fused call, no host sync."""
    cond, uncond = _dev(cond).contiguous(), _dev(uncond).contiguous()
    assert cond.dtype == uncond.dtype == torch.float32 and cond.shape == uncond.shape
    ws = _workspace("dsg", _ffi.lib().wf_dsg_workspace_floats(), cond.device)
    out = torch.empty_like(cond)
    call("wf_cfg_zero", cond.data_ptr(), uncond.data_ptr(), out.data_ptr(), float(guidance), 1 if negate else 0, cond.numel(),
         ws.data_ptr(), stream())
    return out


def temporal_diff(x: torch.Tensor) -> torch.Tensor:
    """SCHED:391-392: x [C,T,h,w] -> [C,T-1,h,w] fp32."""
    x = _dev(x)
    C, T, h, w = x.shape
    out = torch.empty((C, T - 1, h, w), dtype=torch.float32, device=x.device)
    call("wf_temporal_diff", x.data_ptr(), _dt(x), out.data_ptr(), C, T, h * w, stream())
    return out


_DECAY = {"linear": 0, "exponential": 1, "sine": 2, "cosine": 3}


def soften_mask(mask: torch.Tensor, transition_distance: int = 15, decay_type: str = "sine") -> torch.Tensor:
    """INFER:105-150 on the device: mask [F,H,W] fp32 -> softened [F,H,W] fp32."""
    if decay_type not in _DECAY:
        raise ValueError(f"Unsupported decay type: {decay_type}")
    mask = _dev(mask)
    assert mask.dtype == torch.float32 and mask.dim() == 3 and mask.is_contiguous()
    out = torch.empty_like(mask)
    F_, H, W = mask.shape
    call("wf_soften_mask", mask.data_ptr(), out.data_ptr(), F_, H, W, int(transition_distance), _DECAY[decay_type], stream())
    return out


_RESAMPLE_TABLES: dict = {}


def _resample_tables(n_in: int, n_out: int, device, filter: str = "bicubic"):
    """Pillow's tables of one axis on `device` (bounds, coefs, ksize), built and checked once per (in, out, filter, device): they are
    read-only."""
    from . import resample
    key = (n_in, n_out, filter, str(device))
    if key not in _RESAMPLE_TABLES:
        bounds, coefs = resample.filter_tables(n_in, n_out, filter)
        if bounds[:, 0].min() < 0 or bounds[:, 1].min() < 1 or (bounds[:, 0] + bounds[:, 1]).max() > n_in or bounds[:, 1].max() > coefs.shape[1]:
            raise ValueError(f"resample tables {n_in} -> {n_out}: a tap window leaves the axis")   # the C entry trusts what it is handed
        if len(_RESAMPLE_TABLES) >= 64:
            _RESAMPLE_TABLES.clear()
        _RESAMPLE_TABLES[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(coefs).to(device), coefs.shape[1])
    return _RESAMPLE_TABLES[key]


def _axis_tables(frames_hw, size_hw, device, filter: str):
    """[xbounds, xcoefs, xk, ybounds, ycoefs, yk] for the C entries: columns first, None / 0 for an axis whose size does not change."""
    from . import resample
    if filter not in resample.FILTERS:
        raise ValueError(f"filter {filter!r}: one of {sorted(resample.FILTERS)}")
    tabs = []
    for n_in, n_out in ((frames_hw[1], size_hw[1]), (frames_hw[0], size_hw[0])):
        tabs += [None, None, 0] if n_in == n_out else list(_resample_tables(n_in, n_out, device, filter))
    return tabs


def resample_u8(frames: torch.Tensor, size_hw, filter: str = "bicubic") -> torch.Tensor:
    """`PIL.Image.resize((W, H), filter)` (bicubic: Pillow's default for modes RGB and L) of every frame, bit for bit, on the device
    (wf_resample_u8): frames u8 [T, h, w, C] (C = 1 or 3) or [T, h, w] -> u8 of the same rank at H x W.  `filter`: one of Pillow's five
    convolution filters (resample.FILTERS).  Pillow's coefficient tables are built here on the host (resample.filter_tables; kept per
    size pair and filter) and uploaded, so the kernel only ever reads tables whose taps lie inside the image."""
    frames = _dev(frames)
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4):
        raise TypeError(f"resample_u8: uint8 [T, h, w, C] or [T, h, w], got {frames.dtype} {tuple(frames.shape)}")
    planar = frames.dim() == 3
    T, h, w = frames.shape[:3]
    C = 1 if planar else frames.shape[3]
    H, W = int(size_hw[0]), int(size_hw[1])
    if C not in (1, 3) or min(T, h, w, H, W) <= 0:
        raise ValueError(f"resample_u8: {tuple(frames.shape)} -> {(H, W)}: sizes must be positive and C 1 or 3")
    dev = frames.device
    tabs = _axis_tables((h, w), (H, W), dev, filter)
    out = torch.empty((T, H, W) if planar else (T, H, W, C), dtype=torch.uint8, device=dev)
    ws = torch.empty(int(_ffi.lib().wf_resample_u8_workspace_bytes(T, h, w, H, W, C)), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    call("wf_resample_u8", frames.data_ptr(), out.data_ptr(), T, h, w, H, W, C, ptr(tabs[0]), ptr(tabs[1]), tabs[2], ptr(tabs[3]),
         ptr(tabs[4]), tabs[5], ws.data_ptr(), stream())
    return out


def resample_u8_window(frames: torch.Tensor, size_hw, window, lut: torch.Tensor, filter: str = "bicubic") -> torch.Tensor:
    """A network's fp32 input from decoded pixels in one entry (wf_resample_u8_window_f32): frames u8 [T, h, w, C] (C = 1 or 3) or
    [T, h, w] -> f32 [T, C, Hc, Wc] = lut[c][resample_u8(frames, size_hw, filter)[:, y0:y0 + Hc, x0:x0 + Wc, c]], window = (y0, x0, Hc, Wc),
    lut f32 [C, 256] (or [256] for C = 1): the host's own u8 -> f32 expression per channel.  Only the window is computed."""
    frames, lut = _dev(frames), _dev(lut)
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4):
        raise TypeError(f"resample_u8_window: uint8 [T, h, w, C] or [T, h, w], got {frames.dtype} {tuple(frames.shape)}")
    T, h, w = frames.shape[:3]
    C = 1 if frames.dim() == 3 else frames.shape[3]
    H, W = int(size_hw[0]), int(size_hw[1])
    y0, x0, Hc, Wc = (int(v) for v in window)
    if C not in (1, 3) or min(T, h, w, H, W, Hc, Wc) <= 0:
        raise ValueError(f"resample_u8_window: {tuple(frames.shape)} -> {(H, W)}, window {(y0, x0, Hc, Wc)}: sizes must be positive and C 1 or 3")
    if y0 < 0 or x0 < 0 or y0 + Hc > H or x0 + Wc > W:
        raise ValueError(f"resample_u8_window: the window {Hc} x {Wc} at {(y0, x0)} leaves {H} x {W}")
    if lut.dtype != torch.float32 or lut.numel() != C * 256:
        raise TypeError(f"resample_u8_window: a float32 table [{C}, 256], got {lut.dtype} {tuple(lut.shape)}")
    dev = frames.device
    tabs = _axis_tables((h, w), (H, W), dev, filter)
    out = torch.empty((T, C, Hc, Wc), dtype=torch.float32, device=dev)
    ws = torch.empty(int(_ffi.lib().wf_resample_u8_window_f32_workspace_bytes(T, h, w, H, W, C, y0, x0, Hc, Wc)), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    call("wf_resample_u8_window_f32", frames.data_ptr(), out.data_ptr(), T, h, w, H, W, C, y0, x0, Hc, Wc, ptr(tabs[0]), ptr(tabs[1]), tabs[2],
         ptr(tabs[3]), ptr(tabs[4]), tabs[5], lut.data_ptr(), ws.data_ptr(), stream())
    return out


def u8_lut_planar(frames: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """frames u8 [T, h, w, C] or [T, h, w], lut f32 [256] -> f32 [C, T, h, w] = lut[frames] (wf_u8_lut_planar_f32): the u8 -> f32 step
    of harness.prepare_inputs with the host's own 256 values, channels moved in front."""
    frames, lut = _dev(frames), _dev(lut)
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or lut.dtype != torch.float32 or lut.numel() != 256:
        raise TypeError("u8_lut_planar: uint8 [T, h, w, C] or [T, h, w] and a float32 table of 256 entries")
    T, h, w = frames.shape[:3]
    C = 1 if frames.dim() == 3 else frames.shape[3]
    out = torch.empty((C, T, h, w), dtype=torch.float32, device=frames.device)
    call("wf_u8_lut_planar_f32", frames.data_ptr(), lut.data_ptr(), out.data_ptr(), T, h, w, C, stream())
    return out


def farneback_flows(x: torch.Tensor, quant_mode: int = 0) -> torch.Tensor:
    """SCHED:156-248 for every channel at once: x [C,T,h,w] (f32 / bf16) -> flows [C,T-1,2,h,w] fp32 (device).
    quant_mode 0 = the Wan scheduler's uint8 preparation (one global range), 1 = the LongCat scheduler's (a range per channel)."""
    x = _dev(x)
    C, T, h, w = x.shape
    nbytes = _ffi.lib().wf_farneback_workspace_bytes(C, T, h, w)
    ws = _workspace("farneback", (nbytes + 3) // 4, x.device)
    out = torch.empty((C, T - 1, 2, h, w), dtype=torch.float32, device=x.device)
    call("wf_farneback_flows", x.data_ptr(), _dt(x), out.data_ptr(), C, T, h, w, quant_mode, ws.data_ptr(), stream())
    return out


def flow_metrics(ref_flow: torch.Tensor, chan_flow: torch.Tensor, variant: int = 0) -> torch.Tensor:
    """SCHED:497-607 (variant 0) or the LongCat scheduler's metric (variant 1) for n channels at once.
    ref_flow [n,Tm,Cr,h,w], chan_flow [n,Tm,Cc,h,w] fp32 -> sim [n] (device)."""
    ref_flow, chan_flow = _dev(ref_flow), _dev(chan_flow)
    assert ref_flow.dtype == chan_flow.dtype == torch.float32
    n, Tm, Cr, h, w = ref_flow.shape
    Cc = chan_flow.shape[2]
    assert chan_flow.shape == (n, Tm, Cc, h, w)
    ws = _workspace("flow", _ffi.lib().wf_flow_metrics_workspace_floats(n), ref_flow.device)
    sim = torch.empty(n, dtype=torch.float32, device=ref_flow.device)
    call("wf_flow_metrics_variant", ref_flow.data_ptr(), chan_flow.data_ptr(), sim.data_ptr(), n, Tm, Cr, Cc, h * w, variant,
         ws.data_ptr(), stream())
    return sim


def mx_quant(x: torch.Tensor, q: Optional[torch.Tensor] = None, s: Optional[torch.Tensor] = None):
    """OCP MX-fp8 quantization of a bf16 matrix x [M, K] (unit column stride, any row stride): e4m3 elements q [M, K] and E8M0 block
    scales s [M, K/32] (uint8 views; one scale per 32 consecutive elements of a row) -- wf_mx_quant_e4m3."""
    assert x.dim() == 2 and x.dtype == torch.bfloat16 and x.stride(1) == 1
    M, K = x.shape
    q = torch.empty((M, K), dtype=torch.uint8, device=x.device) if q is None else q
    s = torch.empty((M, K // 32), dtype=torch.uint8, device=x.device) if s is None else s
    assert q.shape == (M, K) and q.is_contiguous() and s.shape == (M, K // 32) and s.is_contiguous()
    call("wf_mx_quant_e4m3", x.data_ptr(), q.data_ptr(), s.data_ptr(), M, K, x.stride(0), stream())
    return q, s


def gemm_mxfp8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor,
               epi: int, gate: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N] = epi(dequant(xq, xs) @ dequant(wq, ws)^T + bias) on the scaled MX MFMA (wf_gemm_mxfp8); K % 128 == 0."""
    M, K = xq.shape
    N = wq.shape[0]
    assert wq.shape[1] == K and xs.shape == (M, K // 32) and ws.shape == (N, K // 32) and out.shape[0] == M and out.shape[1] == N
    assert xs.is_contiguous() and ws.is_contiguous()
    call("wf_gemm_mxfp8", xq.data_ptr(), xs.data_ptr(), wq.data_ptr(), ws.data_ptr(), bias.data_ptr() if bias is not None else None,
         out.data_ptr(), gate.data_ptr() if gate is not None else None, M, N, K, xq.stride(0), wq.stride(0), out.stride(0), epi, stream())
    return out


def lora_fold(base: torch.Tensor, out: torch.Tensor, adapters) -> torch.Tensor:
    """out = bf16(base + sum_j scale_j * U_j @ D_j[row block's rank slice]) for one bf16 matrix [N, K] or a contiguous row slice of one
    (wf_lora_fold): adapters = 1..4 tuples (U bf16 [N, rank], D bf16 [nsep * rank, K], nsep, scale); fp32 accumulation, one rounding.
    base is only read; out may be base."""
    if not (base.is_cuda and out.is_cuda and all(U.is_cuda and D.is_cuda for U, D, _, _ in adapters)):
        raise RuntimeError("worldforge_amd ops need device tensors (there is no CPU fallback)")
    assert base.dim() == 2 and base.dtype == out.dtype == torch.bfloat16 and base.shape == out.shape
    assert base.is_contiguous() and out.is_contiguous()
    N, K = base.shape
    flat = []
    for U, D, nsep, scale in adapters:
        assert U.dtype == D.dtype == torch.bfloat16 and U.is_contiguous() and D.is_contiguous()
        assert U.shape[0] == N and D.shape == (int(nsep) * U.shape[1], K), (tuple(U.shape), tuple(D.shape), nsep, (N, K))
        flat += [U.data_ptr(), D.data_ptr(), U.shape[1], int(nsep), float(scale)]
    n = len(flat) // 5
    if not 1 <= n <= 4:
        raise ValueError(f"wf_lora_fold takes 1..4 adapters per launch, not {n}")
    flat += [None, None, 0, 0, 0.0] * (4 - n)
    call("wf_lora_fold", base.data_ptr(), out.data_ptr(), N, K, n, *flat, stream())
    return out
