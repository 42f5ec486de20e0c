"""Wan2.1 3D causal VAE (AutoencoderKLWan) on hand-written HIP kernels.

Speaks the diffusers protocol the reference uses (SCHED:1272-1285, 1384; PIPE:162-163, 348, 743):
    vae.encode(x[B,3,F,H,W]).latent_dist.mode() -> [B,16,T,h,w]      vae.decode(z[B,16,T,h,w], return_dict=False)[0]
    vae.config.{z_dim, latents_mean, latents_std}, vae.dtype, vae.temperal_downsample
The arithmetic follows /root/reference/wan_for_worldforge/wan/modules/vae.py (in-tree statement of the diffusers class).

MI355X-first design: instead of the reference's 21 sequential per-latent-frame decoder passes with a Python-side
feature cache, the WHOLE frame sequence stays resident in HBM (channels-last [T,H,W,C]; 81x480x832x96 fp32 = 12.4 GB,
trivial against 288 GB) and every layer is ONE launch over all frames with causal zero padding in time -- arithmetically
the same function (oracle/vae.py proves it against the chunked twin).  Convolutions with MFMA-sized channel counts run as
implicit GEMM (csrc/conv.hip); RMS-norm + SiLU is a fused one-pass kernel producing the bf16 conv operand; the nearest
2x upsample and the stride-2 / zero-pad of Resample are folded into the convolution's gather; the mid-block attention is
two MFMA GEMMs around a row softmax.  fp32 residual stream, fp32 accumulation.

precision (the reference loads the VAE with torch_dtype=torch.float32, INFER:185-189):
  "bf16"  -- every matrix-core operand (activation and weight) rounded to bf16: 2^-9 relative per operand.  Opt-in fast mode: over a
             guided job's 31 decode -> encode round trips this noise is enough to flip near-tied FLF gate decisions
             (tools/vae_precision_study.py).
  "fp16x3" -- DEFAULT since round 4 (alias "fp32").  The three-term split below on FP16 parts (hi = fp16(x), lo = fp16(x - hi): 22
             significand bits) on v_mfma_f32_32x32x16_f16: same kernels, same cost as the bf16 split.  Per product ~2^-22 WHERE lo IS A
             NORMAL fp16, i.e. |x| >= 2^-3; below that lo is a subnormal with an absolute floor of 2^-25.  Round 5: every weight matrix is
             stored times an exact power of two that lifts it into the normal range (undone in the kernels' epilogues, `acc_scale`), so
             the floor only remains for small ACTIVATIONS, whose absolute error 2^-25 |w| is negligible against the products of the O(1)
             ones.  Measured end to end against the fp32 goldens: see tests/test_gpu_vae.py (rel. L2) -- that, not the per-product
             figure, is the claim.  fp16 cannot hold |x| > 65504: the producers raise a device flag; it is copied to the host
             asynchronously and turned into a RuntimeError at the next check point (check_range; never a silent inf) -- such weights
             need "bf16x3".
  "fp16"  -- round 6 (alias "tf32"): ONE fp16 term per operand (hi = fp16(x): 10 explicit mantissa bits, fp32 accumulation) on the same
             *_f16 kernels with the same power-of-two weight scale and range flag -- the multiplicand width of a TF32 convolution, which
             is what an fp32 `conv3d` executes under PyTorch's defaults on the reference's stack (torch.backends.cudnn.allow_tf32 = True;
             the LongCat entry sets it explicitly, run_longcat_worldforge_single.py:144-146).  One third of "fp16x3"'s matrix work.  The
             tensors between layers stay f32 (residual stream, norm inputs, attention scores and probabilities), as in the three-term
             modes.  Opt-in for the Wan path (the headline keeps "fp16x3": BASELINE.md states an fp32 VAE and the parity target is the
             CPU eager path).
  "bf16x3" -- the default of rounds 2-3.  fp32-CLASS contractions on the bf16 matrix cores, NOT IEEE fp32: every operand x is carried as hi = bf16(x),
             lo = bf16(x - hi) and every contraction as hi.hi + lo.hi + hi.lo in fp32 accumulators (wf_split_bf16x3: activations
             [hi | lo | hi], weights [hi | hi | lo] on 3x the channels, the SAME conv / GEMM kernels; the dropped lo.lo term and the
             rounding of lo leave ~2^-16 relative per product, against 2^-24 for true fp32).  3x the MFMA work.  "fp32" is accepted as
             an alias (rounds 1-2 called the mode that) and maps to "bf16x3".
"""
from __future__ import annotations

import os

import math
from types import SimpleNamespace
from typing import Dict

import torch

from . import ops
from . import _ffi
from ._ffi import WF_BF16, WF_F32, call
from .dit import EPI_BF16, EPI_F32, EPI_F32_ACC, gemm
# (the plans, the constants, the key map and weight_operand are imported from this module by the entry points, the tools and the tests)
from .vae_weights import (BF, F32, LATENTS_MEAN, LATENTS_STD, T_DOWN, Z_DIM, decoder_plan, diffusers_key_map,  # noqa: F401
                          diffusers_to_twin_state_dict, encoder_plan, first_up, pack_state_dict, random_state_dict, weight_operand)


class _LatentDist:
    """diffusers' DiagonalGaussianDistribution surface the samplers use: mode() (Wan path, PIPE retrieve_latents "argmax") and
    sample(generator) (LongCat prepare_latents, pipeline_longcat_video.py:278: mean + std * randn, logvar clamped to [-30, 20])."""

    def __init__(self, mean, logvar=None):
        self._mean = mean
        self._logvar = logvar

    def mode(self):
        return self._mean

    def sample(self, generator=None):
        std = torch.exp(0.5 * torch.clamp(self._logvar, -30.0, 20.0))
        if generator is not None and generator.device.type != self._mean.device.type:
            noise = torch.randn(self._mean.shape, generator=generator, dtype=self._mean.dtype).to(self._mean.device)
        else:
            noise = torch.randn(self._mean.shape, generator=generator, dtype=self._mean.dtype, device=self._mean.device)
        return self._mean + std * noise


class AutoencoderKLWan:
    dtype = torch.float32

    ATTN_BATCH_BYTES = 12 << 30  # scores, probabilities and split operands of the mid-block attention's batched launches kept at a time (_attn_x3)
    crop_to_mask = True          # the IRR injection decodes only the pixel columns its blend can see (needed_columns); False: everything

    def __init__(self, device="cuda:0", comm=None, precision: str = "fp16x3", dtype: torch.dtype = torch.float32, strict_range: bool = False):
        """strict_range: check the fp16 range flag INSIDE the call that raised it (one host synchronisation per encode / decode) -- for
        callers of the bare encode / decode API who consume the result without ever calling check_range() or the VAE again.
        dtype: the MODULE dtype the protocol shows (`vae.dtype`, what `from_pretrained(torch_dtype=...)` sets): torch.float32 for the
        Wan entry (INFER:185-189), torch.bfloat16 for the LongCat entry (run_longcat_worldforge_single.py:205).  A bf16 module takes bf16
        inputs (others are rounded to bf16 on the way in, the `.to(dtype=vae.dtype)` of LongCat's fuse_latents) and returns bf16 videos /
        moments; in between, this implementation keeps its f32 stream with `precision` operands -- closer to the fp32 network than the
        eager bf16 module, whose every activation is bf16 (tests/golden/g8c)."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"dtype must be torch.float32 or torch.bfloat16, got {dtype}")
        self.dtype = dtype
        self.strict_range = bool(strict_range)
        if precision == "fp32":  # the fp32-CLASS mode of the round: three-term split operands, fp16 parts since round 4
            precision = "fp16x3"
        if precision == "tf32":  # what the mode stands for: the multiplicand width of a TF32 convolution
            precision = "fp16"
        if precision not in ("bf16", "bf16x3", "fp16x3", "fp16"):
            raise ValueError(f"precision must be 'fp16x3' (alias 'fp32'), 'bf16x3', 'fp16' (alias 'tf32') or 'bf16', got {precision!r}")
        self.precision = precision
        self.x3 = precision in ("bf16x3", "fp16x3")  # three-term split operands
        self.f16 = precision in ("fp16x3", "fp16")     # operand parts are fp16 (v_mfma_f32_32x32x16_f16) instead of bf16
        # `wide`: every tensor BETWEEN two layers is f32 and the 16-bit operand is made by a producer that checks the fp16 range (the
        # three-term modes, and the one-term fp16 mode); only "bf16" takes the 16-bit output copies of the conv / GEMM epilogues
        self.wide = self.x3 or self.f16
        self.terms = 3 if self.x3 else 1
        self.OP = torch.float16 if self.f16 else BF    # element type of every matrix-core operand tensor
        self._sfx = "_f16" if self.f16 else ""         # the C-ABI entry points of that element type
        self.device = torch.device(device)
        self.comm = comm  # row-slab sharding of the high-resolution stages over the ranks of `comm` (parallel.Comm or a stand-in)
        self.config = SimpleNamespace(z_dim=Z_DIM, latents_mean=LATENTS_MEAN, latents_std=LATENTS_STD)
        self.temperal_downsample = list(T_DOWN)
        self.w: Dict[str, torch.Tensor] = {}
        self.flops_last = 0

    # ------------------------------------------------------------------------------------------------------------
    # weights (keys as in WanVAE_.state_dict())
    # ------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        self.w = pack_state_dict(sd, self.precision, self.device)
        return self

    def load_diffusers_state_dict(self, sd: Dict[str, torch.Tensor]):
        """State dict in the layout of the class the reference executes (diffusers AutoencoderKLWan, INFER:185-189)."""
        return self.load_state_dict(diffusers_to_twin_state_dict(sd))

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0", comm=None, precision: str = "fp16x3", subfolder: str = "vae",
                        torch_dtype: torch.dtype = torch.float32):
        """`AutoencoderKLWan.from_pretrained(model_id, subfolder="vae", torch_dtype=torch.float32)` (INFER:185-189) from a local
        diffusers checkpoint directory: reads `<path>/<subfolder>/*.safetensors` (sharded or not) with checkpoint.load_dir."""
        from . import checkpoint
        folder = os.path.join(path, subfolder) if subfolder and os.path.isdir(os.path.join(path, subfolder)) else path
        return cls(device, comm=comm, precision=precision, dtype=torch_dtype).load_diffusers_state_dict(checkpoint.load_dir(folder))

    def init_random(self, seed: int = 0):
        """Synthetic weights of the real shapes, generated on the host in twin layout (127 M parameters)."""
        return self.load_state_dict(random_state_dict(seed))

    # ------------------------------------------------------------------------------------------------------------
    # kernels wrappers; activations are channels-last [T, H, W, C]
    # ------------------------------------------------------------------------------------------------------------
    def _conv(self, x, p, To, Ho, Wo, Cout, k, st=1, ss=1, pt=0, ps=0, up2=False, tsplit=False, resid=None, out_f32=True,
              out_bf16=False, out_shape=None, out_bf_tensor=None, ph=None):
        """ps: symmetric spatial padding (top = left); ph overrides the top padding (row slabs with halo rows).  x: channels-last
        [T,H,W,C], or the slice-major operand [T,H,C_stored/16,W,16] of _rms(blocked=True) (3x3x3 stride-1 layers only)."""
        layout, Cst = 0, x.shape[-1]
        if x.dim() == 5:
            Ti, Hi, nsl, Wi, _ = x.shape
            layout, Cst = 1, 16 * nsl
            Cin = Cst * 3 // 2 if self.x3 else Cst  # fp32-class: [hi | lo] stored, K = [hi | lo | hi]
        else:
            Ti, Hi, Wi, Cin = x.shape
        assert x.dtype == self.OP and x.is_contiguous()
        shape = out_shape or (To, Ho, Wo, Cout)
        of = torch.empty(shape, dtype=F32, device=x.device) if out_f32 else None
        ob = out_bf_tensor if out_bf_tensor is not None else (torch.empty(shape, dtype=self.OP, device=x.device) if out_bf16 else None)
        W = self.w
        if (tuple(k) == (3, 3, 3) and st == 1 and ss == 1 and pt == 2 and ps == 1 and not up2 and not tsplit and To == Ti and Wo == Wi
                and Cin % 32 == 0 and Cout % 32 == 0):
            # the FLOP-heavy layers: LDS-resident input patch kernel on re-packed weights (packed once per layer, cached).  Chosen by
            # layer type only, never by size: a row slab of the sharded VAE must run the same arithmetic as the whole image
            zp = self._zero_page(int(_ffi.lib().wf_conv3d_333_zero_page_bytes(Wi, Cst, layout)))
            call("wf_conv3d_333" + self._sfx, x.data_ptr(), self._packed333(p, Cout, Cin).data_ptr(), W[p + ".b"].data_ptr(),
                 resid.data_ptr() if resid is not None else None, of.data_ptr() if of is not None else None,
                 ob.data_ptr() if ob is not None else None, Ti, Hi, Wi, Cin, Ho, Cout, ps if ph is None else ph,
                 zp.data_ptr(), zp.numel() * 2, layout, Cst, *self._acc_scale(p + ".w"), ops.stream())
        else:
            assert layout == 0, "slice-major operands are for the 3x3x3 stride-1 kernel only"
            call("wf_conv3d_cl" + self._sfx, x.data_ptr(), W[p + ".w"].data_ptr(), W[p + ".b"].data_ptr(),
                 resid.data_ptr() if resid is not None else None, of.data_ptr() if of is not None else None,
                 ob.data_ptr() if ob is not None else None, Ti, Hi, Wi, Cin, To, Ho, Wo, Cout, k[0], k[1], k[2], st, ss, pt,
                 ps if ph is None else ph, ps, 1 if up2 else 0, 1 if tsplit else 0, self._zero_page().data_ptr(), *self._acc_scale(p + ".w"),
                 ops.stream())
        self.flops_last += 2 * To * Ho * Wo * Cout * k[0] * k[1] * k[2] * Cin
        return of, ob

    def _acc_scale(self, wkey: str):
        """The extra trailing argument of the *_f16 entry points that take a weight operand: () for the bf16 ones."""
        return (float(self.w.get(wkey + ".scale", 1.0)),) if self.f16 else ()

    def _packed333(self, p, Cout, Cin):
        """[Cout][27][Cin] -> [27][Cin/16][Cout][16] copy of a 3x3x3 weight for wf_conv3d_333 (keyed by the weight tensor's identity so
        that instances sharing `w` and reloaded weights stay consistent)."""
        w = self.w[p + ".w"]
        cache = self.__dict__.setdefault("_packed", {})
        hit = cache.get(p)
        if hit is None or hit[0] is not w:
            out = torch.empty((27, Cin // 16, Cout, 16), dtype=w.dtype, device=w.device)
            call("wf_conv3d_pack333", w.data_ptr(), out.data_ptr(), Cout, Cin, ops.stream())
            cache[p] = hit = (w, out)
        return hit[1]

    def _zero_page(self, nbytes: int = 128):
        """Zeros for the convolutions' padding taps.  wf_conv3d_333 reads it at the wave-uniform slice offset of its LDS-DMA pieces
        (wf_conv3d_333_zero_page_bytes: up to (Cin_stored / 16 - 1) x W x 32 bytes), so the page grows to the largest request seen."""
        z = getattr(self, "_zeros", None)
        if z is None or z.numel() * 2 < nbytes:
            z = self._zeros = torch.zeros(max(1 << 20, (nbytes + 1) // 2), dtype=BF, device=self.device)
        return z

    def _small_conv(self, x, p, To, Ho, Wo, Cout, k, pt=0, ps=0, clamp=0.0, out_dtype=F32):
        Ti, Hi, Wi, Cin = x.shape
        out = torch.empty((To, Ho, Wo, Cout), dtype=out_dtype, device=x.device)
        W = self.w
        call("wf_conv3d_small", x.data_ptr(), WF_BF16 if x.dtype == BF else WF_F32, W[p + ".w"].data_ptr(), W[p + ".b"].data_ptr(),
             out.data_ptr() if out_dtype == F32 else None, out.data_ptr() if out_dtype == BF else None, Ti, Hi, Wi, Cin, To, Ho,
             Wo, Cout, k[0], k[1], k[2], 1, 1, pt, ps, float(clamp), ops.stream())
        self.flops_last += 2 * To * Ho * Wo * Cout * k[0] * k[1] * k[2] * Cin
        return out

    def _rms(self, x, gamma, silu=True, blocked=False, halo=False):
        """RMS_norm (+ SiLU) of the f32 stream -> the next layer's matrix-core operand.  blocked: the slice-major operand of the 3x3x3
        kernel, [T,H,C/16,W,16] (fp32-class mode: [hi | lo] slices, [T,H,2C/16,W,16])."""
        C = x.shape[-1]
        if blocked and C % 32 == 0:
            T, H, Wd, _ = x.shape
            # halo: the kernel writes rows 1 .. H of a [T, H + 2, ...] slab operand directly (row slabs: _halo_fill adds the neighbours' rows)
            out = torch.empty((T, H + (2 if halo else 0), (2 if self.x3 else 1) * C // 16, Wd, 16), dtype=self.OP, device=x.device)
            call("wf_rms_silu_cl_blocked" + self._sfx, x.data_ptr(), gamma.data_ptr(), out.data_ptr(), x.numel() // C, C, 1 if silu else 0, Wd,
                 1 if self.x3 else 0, H if halo else 0, ops.stream())
            return out
        if self.x3:
            out = torch.empty(tuple(x.shape[:-1]) + (3 * C,), dtype=self.OP, device=x.device)
            call("wf_rms_silu_cl_x3" + self._sfx, x.data_ptr(), gamma.data_ptr(), out.data_ptr(), x.numel() // C, C, 1 if silu else 0, ops.stream())
            return out
        out = torch.empty(x.shape, dtype=self.OP, device=x.device)
        call("wf_rms_silu_cl" + self._sfx, x.data_ptr(), gamma.data_ptr(), out.data_ptr(), None, x.numel() // C, C, 1 if silu else 0,
             ops.stream())
        return out

    def _operand(self, x, side=0, out=None):
        """f32 [..., C] -> the matrix-core operand: bf16 [..., C], or the three-term split [..., 3C] (precision="fp32"; side 0 =
        activation, 1 = weight-side layout).  `out`: a contiguous destination of the operand's shape."""
        if not self.wide:
            y = ops.cast(x, BF)
            if out is not None:
                out.copy_(y)
                return out
            return y
        assert x.dtype == F32 and x.stride(-1) == 1
        C = x.shape[-1]
        if x.dim() > 2:
            assert x.is_contiguous()
            x2 = x.view(-1, C)
        else:
            x2 = x
        n = self.terms
        if out is None:
            out = torch.empty(tuple(x.shape[:-1]) + (n * C,), dtype=self.OP, device=x.device)
        assert out.is_contiguous() and out.numel() == n * x2.shape[0] * C and out.dtype == self.OP
        if not self.x3:   # "fp16": hi alone
            call("wf_cast_f16", x2.data_ptr(), x2.stride(0), out.data_ptr(), C, x2.shape[0], C, ops.stream())
            return out
        call("wf_split_f16x3" if self.f16 else "wf_split_bf16x3", x2.data_ptr(), x2.stride(0), out.data_ptr(), 3 * C, x2.shape[0], C, side, ops.stream())
        return out

    def _gemm(self, x, w, bias, out, epi, wkey=None):
        """out[M,N] = epi(x[M,K] @ w[N,K]^T + bias) on the operand type of this precision mode (wf_gemm_bf16 / wf_gemm_f16).  wkey: the weight
        dict key of `w` when it is a stored weight operand (its power-of-two scale is undone in the epilogue), None for activations."""
        if not self.f16:
            return gemm(x, w, bias, out, epi)
        M, K = x.shape
        N = w.shape[0]
        assert w.shape[1] == K and x.dtype == self.OP and w.dtype == self.OP and out.shape[0] == M and out.shape[1] == N
        call("wf_gemm_f16", x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(), M, N, K,
             x.stride(0), w.stride(0), out.stride(0), epi, float(self.w.get(wkey + ".scale", 1.0)) if wkey else 1.0, ops.stream())
        return out

    def _note_range(self, what: str):
        """fp16 operand formats: a producer that met a value beyond +-65504 (or a NaN) raised the sticky device flag.  Queue a 4-byte
        copy of it into pinned host memory behind this call's kernels (wf_f16_overflow_flag_async) and an event -- NO host
        synchronisation inside encode / decode (no hidden device syncs; round 4 synchronised the stream once per VAE call).
        `check_range` reads it, DETERMINISTICALLY: every encode / decode / decode_blend_encode starts by waiting for the flag
        of the call before it (by then that call's kernels have all but finished: the wait costs a launch latency, not a drain) -- on a
        sharded VAE too, where the calls are collective and every rank is at the same program point -- and the schedulers' `fuse_latents`
        and the pipelines check at their own synchronisation points (FLF gate read-back, final frames).  What remains for the caller: the
        LAST call of a job.  A caller of the bare encode / decode API must call check_range() before consuming the result, or construct the
        VAE with strict_range=True (the check then runs inside the call, one host synchronisation each)."""
        if not self.f16:
            return
        self.check_range()   # an earlier call's flag (none, when the entry point ran its own check at the start)
        if getattr(self, "_flag_host", None) is None:
            self._flag_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        call("wf_f16_overflow_flag_async", self._flag_host.data_ptr(), ops.stream())
        ev = torch.cuda.Event()
        ev.record()
        self._flag_pending = (ev, what)
        if self.strict_range:
            self.check_range()

    def check_range(self, wait: bool = True):
        """Turn a raised fp16 range flag of an earlier encode / decode into a RuntimeError -- never a silent inf.  wait=False: only if its
        copy has already landed.  With `comm` every rank takes part in one tiny all-gather of the flag first, so that all ranks fail
        together instead of one raising while its peers wait in the next collective; call it at the same program points on
        every rank (the pipelines do)."""
        pend = getattr(self, "_flag_pending", None)
        if pend is None:
            return
        ev, what = pend
        shared = self.comm is not None and getattr(self.comm, "world", 1) > 1
        if not wait and (shared or not ev.query()):
            return   # (wait=False is timing-dependent: a sharded VAE never takes it, every rank must take the same branch)
        ev.synchronize()
        self._flag_pending = None
        bad = int(self._flag_host[0])
        if shared:
            mine = torch.tensor([bad], dtype=torch.int32, device=self.device)
            allr = torch.empty((self.comm.world, 1), dtype=torch.int32, device=self.device)
            self.comm.all_gather(allr, mine)
            bad = int(allr.max())
        if bad:
            import ctypes
            flag = ctypes.c_int(0)
            call("wf_f16_overflow_flag", ctypes.byref(flag), 1, ops.stream())   # reset (synchronous: we are about to raise)
            raise RuntimeError(f"AutoencoderKLWan.{what}: an activation left the fp16 range (|x| > 65504) or was NaN under precision="
                               f"{self.precision!r}; use precision='bf16x3' (8-bit exponent) for these weights / inputs")

    def _res(self, x, p, cin, cout, k=None):
        """vae.py:186-220.  k: see _run."""
        T, H, Wd, _ = x.shape
        W = self.w
        a, ph = self._halo_operand(x, W[p + ".residual.0.gamma"], k)
        y, _ = self._conv(a, p + ".residual.2", T, H, Wd, cout, (3, 3, 3), pt=2, ps=1, ph=ph)
        del a
        a2, ph = self._halo_operand(y, W[p + ".residual.3.gamma"], k)
        del y
        if cin != cout:
            xb = self._operand(x)
            h = torch.empty((T, H, Wd, cout), dtype=F32, device=x.device)
            self._gemm(xb.view(-1, xb.shape[-1]), W[p + ".shortcut.w"], W[p + ".shortcut.b"], h.view(-1, cout), EPI_F32, wkey=p + ".shortcut.w")
            self.flops_last += 2 * T * H * Wd * xb.shape[-1] * cout
            del xb
        else:
            h = x
        out, _ = self._conv(a2, p + ".residual.6", T, H, Wd, cout, (3, 3, 3), pt=2, ps=1, ph=ph, resid=h)
        return out

    def _attn(self, x, p, rows=None):
        """vae.py:223-262: per-frame single-head attention over the H*W positions (C = 384).  rows = (r0, r1): only the query rows r0 .. r1
        of every frame are computed (keys / values: the whole frame) and the updated rows are returned as a slab [T, r1 - r0, W, C] -- the
        row-group sharded low-resolution stage; per output element the arithmetic is that of the whole-frame call."""
        T, H, Wd, C = x.shape
        hw = H * Wd
        # K / N padding for the MFMA GEMMs; padded score columns are never read by the softmax and are written as zero probabilities.  The
        # fp32-class path pads to 64 so that the batched P . V products (K = 3 hwp) qualify for the ping-pong GEMM (whole 64-wide K tiles)
        hwp = (hw + 63) // 64 * 64 if self.wide else (hw + 7) // 8 * 8
        W = self.w
        a = self._rms(x, W[p + ".norm.gamma"], silu=False)
        q0, q1 = (0, hw) if rows is None else (rows[0] * Wd, rows[1] * Wd)
        nq = q1 - q0
        if rows is not None:
            x = x[:, rows[0]:rows[1]].contiguous()
        if self.wide:
            return self._attn_x3(x, p, a, hw, hwp, q0, nq)
        qkv = torch.empty((T * hw + 8, 3 * C), dtype=BF, device=x.device)  # +8 rows: the padded K rows stay in-bounds
        qkv[T * hw:].zero_()
        self._gemm(a.view(-1, C), W[p + ".to_qkv.w"], W[p + ".to_qkv.b"], qkv[:T * hw], EPI_BF16)
        del a
        O = torch.empty((T * nq, C), dtype=BF, device=x.device)
        scale = 1.0 / math.sqrt(C)
        # all frames of a chunk in ONE launch per product (round 6; see _attn_x3): q / k are read in place from the qkv rows (row stride 3C,
        # frame stride hw rows), per frame the tiles and the K order of the single call
        tb = max(1, min(T, self.ATTN_BATCH_BYTES // (nq * hwp * 6 + C * hwp * 2)))
        S = torch.empty((tb, nq, hwp), dtype=F32, device=x.device)
        P = torch.empty((tb, nq, hwp), dtype=BF, device=x.device)
        Vt = torch.empty((tb, C, hwp), dtype=BF, device=x.device)
        for t0 in range(0, T, tb):
            n = min(tb, T - t0)
            call("wf_gemm_bf16_batched", qkv[t0 * hw + q0:].data_ptr(), qkv[t0 * hw:, C:].data_ptr(), S.data_ptr(), n, nq, hwp, C, 3 * C, 3 * C, hwp,
                 hw * 3 * C, hw * 3 * C, nq * hwp, EPI_F32, ops.stream())
            call("wf_softmax_rows", S.data_ptr(), hwp, P.data_ptr(), hwp, n * nq, hw, float(scale), ops.stream())
            for t in range(t0, t0 + n):
                call("wf_transpose_bf16", qkv[t * hw:, 2 * C:].data_ptr(), 3 * C, Vt[t - t0].data_ptr(), hwp, hw, C, ops.stream())
            call("wf_gemm_bf16_batched", P.data_ptr(), Vt.data_ptr(), O[t0 * nq:].data_ptr(), n, nq, C, hwp, hwp, hwp, C, nq * hwp, C * hwp, nq * C,
                 EPI_BF16, ops.stream())
        self._gemm(O, W[p + ".proj.w"], W[p + ".proj.b"], x.view(-1, C), EPI_F32_ACC)  # x + proj(attn)  (vae.py:262)
        self.flops_last += T * (4 * nq * hw * C) + 2 * T * hw * C * 3 * C + 2 * T * nq * C * C
        return x

    def _attn_x3(self, x, p, a, hw, hwp, q0, nq):
        """_attn with fp32-class contractions: q / k / v, the scores and the probabilities stay f32 and are split per use.  x: the rows that
        are updated ([T, rows, W, C]: the whole frames, or the query-row slab); a: the normalised WHOLE frames.  Also the one-term fp16
        mode (n = 1 operand term instead of 3): the f32 tensors between the products are the same, each operand is hi alone."""
        T, C = x.shape[0], x.shape[-1]
        W = self.w
        n3 = self.terms
        qkv = torch.zeros((T * hw + 64, 3 * C), dtype=F32, device=x.device)  # + 64 rows: the last frame's padded K rows stay in-bounds
        self._gemm(a.view(-1, n3 * C), W[p + ".to_qkv.w"], W[p + ".to_qkv.b"], qkv[:T * hw], EPI_F32, wkey=p + ".to_qkv.w")
        del a
        Of = torch.empty((T * nq, C), dtype=F32, device=x.device)
        scale = 1.0 / math.sqrt(C)
        # A frame's products are a fraction of the chip (Q . K^T: nq x hwp x n3 C = 175 workgroups of the 256 x 256 kernel at 480p, 49 on a row
        # group's query slab; P . V: 147 / 37), 21 times in a row, with a handful of small launches each.  Round 4 batched the P . V products
        # of a chunk of frames into ONE launch; round 6 does the same for Q . K^T, the softmax and the operand splits: q and k of ALL frames
        # are split once (two launches), the batched GEMM addresses frame t's rows in place (batch stride hw rows; the padded key rows of a
        # frame are the next frame's first rows, never read by the softmax), one softmax launch covers the chunk's n * nq rows, one split
        # each its probabilities and its transposed values.  Per frame the arithmetic is that of the single call (same kernels, same tiles,
        # same K order: the GEMM's results do not depend on the tile or on the batch).  The chunk is bounded by a byte budget
        # (ATTN_BATCH_BYTES: 11.8 GB at 480p = all 21 frames; 720p: 4 frames at a time): whole frames while they fit, never fewer than one.
        Q3 = self._operand(qkv[:, 0:C], 0)          # [T hw + 64, n3 C]
        K3 = self._operand(qkv[:, C:2 * C], 1)
        ld3 = n3 * C
        per_frame = nq * hwp * 8 + (nq + C) * n3 * hwp * 2 + C * hwp * 4
        tb = max(1, min(T, self.ATTN_BATCH_BYTES // per_frame))
        S = torch.empty((tb, nq, hwp), dtype=F32, device=x.device)
        P = torch.empty((tb, nq, hwp), dtype=F32, device=x.device)
        Vt = torch.empty((tb, C, hwp), dtype=F32, device=x.device)
        P3 = torch.empty((tb, nq, n3 * hwp), dtype=self.OP, device=x.device)
        V3 = torch.empty((tb, C, n3 * hwp), dtype=self.OP, device=x.device)
        batched = "wf_gemm_f16_batched" if self.f16 else "wf_gemm_bf16_batched"
        for t0 in range(0, T, tb):
            n = min(tb, T - t0)
            call(batched, Q3[t0 * hw + q0:].data_ptr(), K3[t0 * hw:].data_ptr(), S.data_ptr(), n, nq, hwp, ld3, ld3, ld3, hwp, hw * ld3, hw * ld3,
                 nq * hwp, EPI_F32, ops.stream())
            call("wf_softmax_rows_f32", S.data_ptr(), hwp, P.data_ptr(), hwp, n * nq, hw, float(scale), ops.stream())
            for t in range(t0, t0 + n):
                call("wf_transpose_f32", qkv[t * hw:, 2 * C:].data_ptr(), 3 * C, Vt[t - t0].data_ptr(), hwp, hw, C, ops.stream())
            self._operand(P[:n].view(n * nq, hwp), 0, out=P3[:n].view(n * nq, n3 * hwp))
            self._operand(Vt[:n].view(n * C, hwp), 1, out=V3[:n].view(n * C, n3 * hwp))
            call(batched, P3.data_ptr(), V3.data_ptr(), Of[t0 * nq:].data_ptr(), n, nq, C,
                 n3 * hwp, n3 * hwp, n3 * hwp, C, nq * n3 * hwp, C * n3 * hwp, nq * C, EPI_F32, ops.stream())
        del Q3, K3, S, P, Vt
        del P3, V3
        self._gemm(self._operand(Of), W[p + ".proj.w"], W[p + ".proj.b"], x.view(-1, C), EPI_F32_ACC, wkey=p + ".proj.w")
        self.flops_last += n3 * (T * (4 * nq * hw * C) + 2 * T * hw * C * 3 * C + 2 * T * nq * C * C)
        return x

    def _down(self, x, p, C, temporal, k=None):
        """vae.py:87-96, 139-159: ZeroPad2d((0,1,0,1)) + stride-2 conv (of a row slab's halo rows only the bottom one is read), then the
        stride-2 temporal conv.  k: see _run."""
        T, H, Wd, _ = x.shape
        Ho, Wo = H // 2, Wd // 2
        xb, ph = self._halo_pad_of(x, k)
        if not temporal or T == 1:
            y, _ = self._conv(xb, p + ".resample.1", T, Ho, Wo, C, (1, 3, 3), ss=2, ps=0, ph=ph)
            return y
        y, yb = self._conv(xb, p + ".resample.1", T, Ho, Wo, C, (1, 3, 3), ss=2, ps=0, ph=ph, out_f32=True, out_bf16=not self.wide)
        del xb
        if self.wide:
            yb = self._operand(y)
        To = (T - 1) // 2
        out = torch.empty((1 + To, Ho, Wo, C), dtype=F32, device=x.device)
        out[0].copy_(y[0])  # frame 0 by-passes time_conv (vae.py:146-148)
        W = self.w
        call("wf_conv3d_cl" + self._sfx, yb.data_ptr(), W[p + ".time_conv.w"].data_ptr(), W[p + ".time_conv.b"].data_ptr(), None,
             out[1:].data_ptr(), None, T, Ho, Wo, yb.shape[-1], To, Ho, Wo, C, 3, 1, 1, 2, 1, 0, 0, 0, 0, 0, None, *self._acc_scale(p + ".time_conv.w"), ops.stream())
        self.flops_last += 2 * To * Ho * Wo * C * 3 * yb.shape[-1]
        return out

    def _up(self, x, p, C, temporal):
        """vae.py:76-86, 101-141."""
        T, H, Wd, _ = x.shape
        xb = self._time_up(self._operand(x), p, C) if temporal else self._operand(x)
        Tn = xb.shape[0]
        if p + ".resample.1.ph00.w" in self.w:
            return self._up_phases(xb, p + ".resample.1", Tn, H, 2 * H, 0, C // 2)
        out, _ = self._conv(xb, p + ".resample.1", Tn, 2 * H, 2 * Wd, C // 2, (1, 3, 3), ps=1, up2=True)
        return out

    def _up_phases(self, xb, p, T, n_rows, out_rows, row_off, Cout):
        """The four phase convolutions of an upsampling conv.  xb [T, Hs, W, Cin] bf16: the whole image (Hs = n_rows, row_off = 0) or a row
        slab whose first row is source row s0 while the first output row belongs to source row y0 / 2 (row_off = s0 - y0 / 2 <= 0: halo rows
        above).  Writes out [T, out_rows, 2W, Cout] fp32: phase (py, px) computes n_rows x W outputs from source rows {y - 1 + py, y + py}
        (top padding 1 - py + row_off) and scatters them to rows 2 j + py, columns 2 x + px."""
        _, Hs, Wd, Cin = xb.shape
        out = torch.empty((T, out_rows, 2 * Wd, Cout), dtype=F32, device=xb.device)
        W = self.w
        for py in range(2):
            for px in range(2):
                call("wf_conv3d_cl_scatter" + self._sfx, xb.data_ptr(), W[f"{p}.ph{py}{px}.w"].data_ptr(), W[p + ".b"].data_ptr(), None, out.data_ptr(), None,
                     T, Hs, Wd, Cin, T, n_rows, Wd, Cout, 1, 2, 2, 1, 1, 0, 1 - py + row_off, 1 - px, self._zero_page().data_ptr(),
                     out_rows, 2 * Wd, 2, py, 2, px, *self._acc_scale(f"{p}.ph{py}{px}.w"), ops.stream())
        self.flops_last += 4 * 2 * T * n_rows * Wd * Cout * 4 * Cin
        return out

    def _run(self, x, plan, k=None, g=0):
        """The layers of `plan` on x.  k = None: x holds whole frames.  k >= 1: x is the row slab of row group g, whose k consecutive ranks
        hold the same rows (_row_groups; k = 1: every rank its own slab): a conv operand's top and bottom rows then come from the
        neighbouring groups instead of the kernel's zero padding (_halo_operand, _halo_pad_of), and the attention's keys / values are
        the gathered frame (_attn_group).  Per output element the same arithmetic either way."""
        W = self.w
        for kind, p, cin, cout in plan:
            T, H, Wd, _ = x.shape
            if kind == "conv_in":  # x arrives bf16, zero-padded to 32 channels (a slab's first conv is its caller's: its halo is cut, not exchanged)
                x, _ = self._conv(x, p, T, H, Wd, cout, (3, 3, 3), pt=2, ps=1)
            elif kind == "res":
                x = self._res(x, p, cin, cout, k)
            elif kind == "attn":
                x = self._attn(x, p) if k is None else self._attn_group(x, p, g, k)
            elif kind in ("down2d", "down3d"):
                x = self._down(x, p, cin, kind == "down3d", k)
            elif kind in ("up2d", "up3d"):  # (whole frames: a slab's source rows are its caller's, _up_slab)
                x = self._up(x, p, cin, kind == "up3d")
            elif kind == "head":
                a, ph = self._halo_operand(x, W[p + ".0.gamma"], k)
                x, _ = self._conv(a, p + ".2", T, H, Wd, (cout + 31) // 32 * 32, (3, 3, 3), pt=2, ps=1, ph=ph)
        return x

    # ------------------------------------------------------------------------------------------------------------
    # multi-GPU: row-slab sharding of the high-resolution stages.  The low-resolution stage (60 x 104 at 480p:
    # ~4 % of the FLOPs, and the only place with global spatial coupling -- the mid-block attention) is computed replicated;
    # every other layer runs on H/P rows per rank.  A 3x3 convolution needs one halo row from each neighbour: the ranks
    # all-gather their top / bottom rows of the convolution INPUT (bf16) and pick their neighbours' (zeros at the image edge).
    # Only all-gather is used.  Results are bit-identical to the unsharded path (same per-pixel accumulation order).
    # ------------------------------------------------------------------------------------------------------------
    def _halo_fill(self, out, up, down):
        """out [T,Hs+2,...] whose rows 1 .. Hs are this rank's: rows 0 and Hs+1 <- the neighbours' boundary rows `up` and `down` (None at the
        image edge: zeros), as the exchange handed them over.  Round 5: exchanged with the two neighbours only (parallel.Comm.neighbor_rows:
        all-gathers inside two-rank groups), not all-gathered over the whole job -- a rank receives the 2 rows it needs instead of 2 (P - 1)."""
        for row, src in ((0, up), (out.shape[1] - 1, down)):
            if src is not None:
                out[:, row].copy_(src)
            else:
                out[:, row].zero_()
        return out

    def _halo_pad(self, a, k):
        """a [T,Hs,W,C] (or slice-major [T,Hs,S,W,16]) bf16 -> [T,Hs+2,...] with the neighbours' boundary rows (zeros at the image
        boundary)."""
        T, Hs = a.shape[:2]
        out = torch.empty((T, Hs + 2) + tuple(a.shape[2:]), dtype=a.dtype, device=a.device)
        out[:, 1:Hs + 1].copy_(a)
        return self._halo_fill(out, *self.comm.neighbor_rows(out[:, 1], out[:, Hs], k))

    def _halo_pad_of(self, x, k):
        """The plain conv operand of the f32 stream x and the top padding `ph` its stride-2 conv (ps = 0) is told.  k = None (whole
        frames): _operand(x), the kernel pads.  k >= 1: x is a row slab [T,Hs,W,C] (k: see _run) -> [T,Hs+2,W,..] with the neighbours'
        boundary rows (zeros at the image edge), ph = -1: the top halo row is skipped.  The two border rows are produced FIRST: their operand
        rows travel to the neighbours on the communication stream (Comm.neighbor_rows_async) while the whole slab's operand is produced --
        straight into rows 1 .. Hs of the padded buffer (wf_operand_rows: round 5 produced the slab's operand and copied it in, 1-2 GB per
        full-resolution layer).  Per pixel the same arithmetic wherever the pixel sits: bit-identical to exchanging rows of the produced
        slab."""
        if k is None:
            return self._operand(x), None
        T, Hs, Wd, C = x.shape
        e_op = self._operand(torch.stack([x[:, 0], x[:, Hs - 1]], dim=1))
        pending = self.comm.neighbor_rows_async(e_op[:, 0], e_op[:, 1], k)
        nC = self.terms * C
        out = torch.empty((T, Hs + 2, Wd, nC), dtype=self.OP, device=x.device)
        fmt = (1 if self.f16 else 0) if self.x3 else (2 if self.f16 else 3)
        call("wf_operand_rows", x.data_ptr(), C, out.data_ptr(), nC, T * Hs * Wd, C, fmt, 0, Hs * Wd, 2 * Wd, Wd, ops.stream())
        return self._halo_fill(out, *pending()), -1

    def _halo_operand(self, x, gamma, k):
        """RMS_norm + SiLU of the f32 stream x as the operand of a 3x3x3 conv (ps = 1), and the top padding `ph` that conv is told.  k = None
        (whole frames): _rms(blocked=True), the kernel pads.  k >= 1: x is a row slab (k: see _run) -> the halo-padded operand, ph = 0;
        the norm kernel writes the slab's own rows in place (no copy)."""
        if k is None:
            return self._rms(x, gamma, blocked=True), None
        if x.shape[-1] % 32 == 0:
            # the two border rows first: their operand rows travel to the neighbours on the communication stream while the norm kernel
            # produces the whole slab (per pixel the same arithmetic wherever the pixel sits: bit-identical to exchanging rows of the slab)
            T, Hs = x.shape[:2]
            edge = torch.stack([x[:, 0], x[:, Hs - 1]], dim=1)                       # [T, 2, W, C] f32
            e_op = self._rms(edge, gamma, blocked=True)                              # [T, 2, S, W, 16]
            pending = self.comm.neighbor_rows_async(e_op[:, 0], e_op[:, 1], k)
            return self._halo_fill(self._rms(x, gamma, blocked=True, halo=True), *pending()), 0
        return self._halo_pad(self._rms(x, gamma, blocked=True), k), 0

    def _rows_from_full(self, x, r0, r1):
        """Rows [r0, r1) of a replicated [T,H,W,C] tensor with zero rows outside the image -> contiguous slab."""
        T, H, Wd, C = x.shape
        out = torch.zeros((T, r1 - r0, Wd, C), dtype=x.dtype, device=x.device)
        lo, hi = max(r0, 0), min(r1, H)
        out[:, lo - r0:hi - r0].copy_(x[:, lo:hi])
        return out

    def _gather_rows(self, slab, k=1):
        """[T,Hs,W,C] per rank (k consecutive ranks hold the same slab) -> full [T,(P/k)*Hs,W,C] on every rank."""
        comm = self.comm
        allr = torch.empty((comm.world,) + tuple(slab.shape), dtype=slab.dtype, device=slab.device)
        comm.all_gather(allr, slab.contiguous())
        if k > 1:  # one copy per row group
            allr = allr[::k]
        return allr.permute(1, 0, 2, 3, 4).reshape(slab.shape[0], allr.shape[0] * slab.shape[1], slab.shape[2], slab.shape[3]).contiguous()

    def _attn_group(self, x, p, g: int, reps: int):
        """The mid-block attention of row group g (x: the group's slab [T, Hg, W, C], the same on the group's `reps` ranks): keys / values are
        the whole frame (gathered), and the group's QUERY rows are divided among its replicas (round 6: each of the `reps` ranks computed all
        Hg rows before -- at 8 ranks, 4 groups x 2, every rank did a quarter of the queries instead of an eighth); the replicas' rows come back
        by one all-gather.  Per output row the arithmetic of the whole-frame call: bit-identical."""
        comm = self.comm
        T, Hg, Wd, C = x.shape
        full = self._gather_rows(x, reps)
        if reps == 1:
            return self._attn(full, p, rows=(g * Hg, (g + 1) * Hg))
        j, per = comm.rank % reps, -(-Hg // reps)
        r0, r1 = min(j * per, Hg), min((j + 1) * per, Hg)
        mine = torch.zeros((T, per, Wd, C), dtype=F32, device=x.device)
        if r1 > r0:
            mine[:, :r1 - r0].copy_(self._attn(full, p, rows=(g * Hg + r0, g * Hg + r1)))
        allr = torch.empty((comm.world,) + tuple(mine.shape), dtype=F32, device=x.device)
        comm.all_gather(allr, mine)
        parts = []
        for jj in range(reps):
            n = min((jj + 1) * per, Hg) - min(jj * per, Hg)
            if n > 0:
                parts.append(allr[g * reps + jj, :, :n])
        return torch.cat(parts, dim=1).contiguous()

    def _row_groups(self, h: int, even: bool = False) -> int:
        """Row groups for a stage of h rows: the largest divisor G of the world size with h % G == 0 (and an even number of rows per group
        if a stride-2 conv follows); world / G consecutive ranks then compute the same slab (the low-resolution stage: 60 rows on 8 ranks =
        4 groups of 15, computed twice each, instead of the whole stage on every rank)."""
        P = self.comm.world
        for G in range(P, 0, -1):
            if P % G == 0 and h % G == 0 and (not even or (h // G) % 2 == 0):
                return G
        return 1

    def _time_up(self, xb, p, C):
        """'upsample3d' temporal part (pointwise in space) on the conv operand xb of x: [T,..] -> [1+2(T-1),..] as an operand again.
        The first latent frame by-passes time_conv ('Rep', vae.py:106-108): its operand is carried over as it is.  precision="fp32":
        the interleaved frames are produced in f32 and split."""
        T, H, Wd, Cop = xb.shape
        if T == 1:
            return xb
        W = self.w
        self.flops_last += 2 * (T - 1) * H * Wd * 2 * C * 3 * Cop
        if self.wide:
            yf = torch.empty((1 + 2 * (T - 1), H, Wd, C), dtype=F32, device=xb.device)  # frame 0 is not written (tsplit: 1 + 2t + h)
            call("wf_conv3d_cl" + self._sfx, xb[1:].data_ptr(), W[p + ".time_conv.w"].data_ptr(), W[p + ".time_conv.b"].data_ptr(), None,
                 yf.data_ptr(), None, T - 1, H, Wd, Cop, T - 1, H, Wd, 2 * C, 3, 1, 1, 1, 1, 2, 0, 0, 0, 1, None, *self._acc_scale(p + ".time_conv.w"), ops.stream())
            yb = torch.empty((1 + 2 * (T - 1), H, Wd, Cop), dtype=self.OP, device=xb.device)
            yb[0].copy_(xb[0])
            self._operand(yf[1:], out=yb[1:])
            return yb
        yb = torch.empty((1 + 2 * (T - 1), H, Wd, C), dtype=BF, device=xb.device)
        yb[0].copy_(xb[0])
        call("wf_conv3d_cl" + self._sfx, xb[1:].data_ptr(), W[p + ".time_conv.w"].data_ptr(), W[p + ".time_conv.b"].data_ptr(), None,
             None, yb.data_ptr(), T - 1, H, Wd, C, T - 1, H, Wd, 2 * C, 3, 1, 1, 1, 1, 2, 0, 0, 0, 1, None, *self._acc_scale(p + ".time_conv.w"), ops.stream())
        return yb

    def _up_slab(self, xsrc_b, p, C, temporal, s0, y0, Ho, h_src):
        """Nearest-2x upsample + 3x3 conv for output rows [y0, y0+Ho) (upsampled coordinates) from a bf16 source slab that
        starts at source row s0 (may be -1: zero row) and covers (y0-1)>>1 .. (y0+Ho)>>1.  Output row j reads upsampled rows
        y0 + j - 1 + dy, i.e. slab-local upsampled row j + dy - ph with ph = 1 + 2*s0 - y0."""
        if temporal:
            xsrc_b = self._time_up(xsrc_b, p, C)
            # rows outside the image are the spatial conv's ZERO padding: the (pointwise) time_conv turned them into its bias
            if s0 < 0:
                xsrc_b[:, 0].zero_()
            if s0 + xsrc_b.shape[1] > h_src:
                xsrc_b[:, -1].zero_()
        T, _, Wd, _ = xsrc_b.shape
        if p + ".resample.1.ph00.w" in self.w:
            # output rows y0 .. y0 + Ho (both even here): phase py computes source rows y0/2 .. y0/2 + Ho/2, reading slab rows
            # (y + a - 1 + py) - s0 for its two taps a: the slab starts y0/2 - s0 rows above the first of them
            assert y0 % 2 == 0 and Ho % 2 == 0
            return self._up_phases(xsrc_b, p + ".resample.1", T, Ho // 2, Ho, s0 - y0 // 2, C // 2)
        out, _ = self._conv(xsrc_b, p + ".resample.1", T, Ho, 2 * Wd, C // 2, (1, 3, 3), ps=1, ph=1 + 2 * s0 - y0, up2=True)
        return out

    def can_shard(self, H_lat: int) -> bool:
        """Row sharding needs every sharded stage to hold an integer (even, where a stride-2 conv follows) number of rows."""
        if self.comm is None or self.comm.world == 1:
            return False
        P = self.comm.world
        return (2 * H_lat) % P == 0 and (8 * H_lat) % (4 * P) == 0

    def _decode_stage0_sharded(self, x, plan):
        """The latent-resolution stage of the sharded decoder (conv_in, 5 residual blocks, the mid-block attention at h x w) on the replicated
        operand x -> whole frames on every rank [T,h,w,384] fp32: in G row groups of h / G rows, world / G ranks per group, where h has
        such a divisor."""
        comm = self.comm
        T, h, w, _ = x.shape
        G = self._row_groups(h)
        if G == 1:
            return self._run(x, plan)
        k = comm.world // G
        g, Hg = comm.rank // k, h // G
        kind, p, cin, cout = plan[0]
        x, _ = self._conv(self._rows_from_full(x, g * Hg - 1, (g + 1) * Hg + 1), p, T, Hg, w, cout, (3, 3, 3), pt=2, ps=1, ph=0)
        return self._gather_rows(self._run(x, plan[1:], k, g), k)

    def _decode_ups_sharded(self, x, plan):
        """The decoder from its first upsampling layer on (`plan`), sharded: replicated whole frames x [T,h,w,C] f32 -> this rank's rows
        (rank * 8h/P ...) of the head's output."""
        P, rank = self.comm.world, self.comm.rank
        h = x.shape[1]
        kind, p, cin, cout = plan[0]
        Hs = 2 * h // P                                        # my rows at the next resolution
        y0 = rank * Hs
        s0, s1 = (y0 - 1) >> 1, ((y0 + Hs) >> 1) + 1               # source rows incl. halo (s0 = -1 -> zero row)
        src = self._operand(self._rows_from_full(x, s0, s1))       # (rows first: the operand of this rank's rows only; zero rows stay zero)
        x = self._up_slab(src, p, cin, kind == "up3d", s0, y0, Hs, h)
        h_cur = 2 * h                                          # full image height at the current resolution
        row0 = y0                                              # global first row of my slab at the current resolution
        ups = [i for i, e in enumerate(plan) if e[0] in ("up2d", "up3d")] + [len(plan)]
        for a, b in zip(ups, ups[1:]):                         # the layers up to the next upsampling layer, then that layer
            x = self._run(x, plan[a + 1:b], 1)
            if b < len(plan):
                kind, p, cin, cout = plan[b]
                x = self._up_slab(self._halo_pad_of(x, 1)[0], p, cin, kind == "up3d", row0 - 1, 2 * row0, 2 * x.shape[1], h_cur)
                row0 *= 2
                h_cur *= 2
        return x

    def _encode_one_sharded(self, video: torch.Tensor, slab: torch.Tensor = None) -> torch.Tensor:
        """video [3,F,H,W] replicated on every rank -- or slab [3,F,H/P,W]: only this rank's rows (rank * H/P ...), the halo rows of the
        first convolution then come from the neighbours by all-gather like every later layer's (same operand values: bit-identical)."""
        comm = self.comm
        P, rank = comm.world, comm.rank
        plan = encoder_plan()
        if slab is not None:
            C, Fr, Hs, Wd = slab.shape
            xpad = self._halo_pad(self._video_in(slab), 1)
        else:
            C, Fr, H, Wd = video.shape
            Hs = H // P
            y0 = rank * Hs
            lo, hi = max(y0 - 1, 0), min(y0 + Hs + 1, H)      # this rank's rows + halo: only those are converted (round 5: the whole video)
            xs = self._video_in(video[:, :, lo:hi].contiguous())
            xpad = self._rows_from_full(xs, y0 - 1 - lo, y0 + Hs + 1 - lo)
        kind, p, cin, cout = plan[0]
        x, _ = self._conv(xpad, p, Fr, Hs, Wd, cout, (3, 3, 3), pt=2, ps=1, ph=0)
        last_down = max(i for i, e in enumerate(plan) if e[0] in ("down2d", "down3d"))
        x = self._gather_rows(self._run(x, plan[1:last_down], 1))   # whole frames at the resolution of the last downsample
        G = self._row_groups(x.shape[1], even=True)
        if G == 1:
            return self._moments(self._run(x, plan[last_down:]))
        # the last downsample and everything after it (4 residual blocks, the mid-block attention, the head) in G row groups
        k = P // G
        g, Hg = rank // k, x.shape[1] // G
        return self._moments(self._gather_rows(self._run(x[:, g * Hg:(g + 1) * Hg].contiguous(), plan[last_down:], k, g), k))

    def _moments(self, y):
        """quant conv1 on the encoder head's output y [T,h,w,32] -> [mean | logvar] as [32,T,h,w] f32."""
        T, h, w, _ = y.shape
        q = self._small_conv(y, "conv1", T, h, w, 2 * Z_DIM, (1, 1, 1))
        out = torch.empty((2 * Z_DIM, T, h, w), dtype=F32, device=self.device)
        call("wf_cl_to_ncthw", q.data_ptr(), out.data_ptr(), 2 * Z_DIM, 2 * Z_DIM, T * h * w, 0.0, ops.stream())
        return out

    def _video_in(self, video):
        """[3,F,H,W] f32 -> channels-last conv operand [F,H,W,32 (x3)]: 3 channels zero-padded to one MFMA K slice."""
        C, Fr, H, Wd = video.shape
        if self.f16 and not self.x3:   # one-term fp16: the converting layout kernel raises the range flag itself
            x = torch.empty((Fr, H, Wd, 32), dtype=self.OP, device=self.device)
            call("wf_ncthw_to_cl_f16", video.data_ptr(), None, x.data_ptr(), 3, 32, Fr * H * Wd, ops.stream())
            return x
        if self.x3:
            xf = torch.empty((Fr, H, Wd, 32), dtype=F32, device=self.device)
            call("wf_ncthw_to_cl", video.data_ptr(), xf.data_ptr(), None, 3, 32, Fr * H * Wd, ops.stream())
            return self._operand(xf)
        x = torch.empty((Fr, H, Wd, 32), dtype=BF, device=self.device)
        call("wf_ncthw_to_cl", video.data_ptr(), None, x.data_ptr(), 3, 32, Fr * H * Wd, ops.stream())
        return x

    def _latent_in(self, x, T, h, w):
        """post-quant conv2 (vae.py:558) on the channels-last latent -> conv operand [T,h,w,32 (x3)] (16 channels + 16 zero channels)."""
        if self.wide:
            return self._operand(self._small_conv(x, "conv2", T, h, w, 32, (1, 1, 1), out_dtype=F32))
        return self._small_conv(x, "conv2", T, h, w, 32, (1, 1, 1), out_dtype=BF)

    # ------------------------------------------------------------------------------------------------------------
    # diffusers protocol
    # ------------------------------------------------------------------------------------------------------------
    def _encode_one(self, video: torch.Tensor) -> torch.Tensor:
        """[3,F,H,W] f32 -> posterior moments [32,T,h,w] f32  (vae.py:516-542 without the scale; mode() = mean half)."""
        C, Fr, H, Wd = video.shape
        if (Fr - 1) % 4 != 0:
            raise ValueError(f"number of frames must be 1 + 4k, got {Fr}")
        if H % 8 or Wd % 8:
            raise ValueError("height and width must be multiples of 8")
        self.flops_last = 0
        if self.can_shard(H // 8):
            return self._encode_one_sharded(video)
        return self._moments(self._run(self._video_in(video), encoder_plan()))

    def _decode_one(self, z: torch.Tensor, crop=None, gather: bool = True) -> torch.Tensor:
        """[16,T,h,w] f32 -> [3, 4T-3, 8h, 8w] f32 clamped to [-1,1] (vae.py:544-568, autoencoder_kl_wan.py:1222).  crop = (a0, a1): the
        latent columns decoded after the latent-resolution stage, see decode(columns=...).  Row-sharded (can_shard): gather=False returns
        this rank's row slab [3, F, 8h/P, 8w] (rows rank * 8h/P ...) instead of the gathered video."""
        C, T, h, w = z.shape
        self.flops_last = 0
        shard = self.can_shard(h)
        x = torch.empty((T, h, w, Z_DIM), dtype=F32, device=self.device)
        call("wf_ncthw_to_cl", z.data_ptr(), x.data_ptr(), None, Z_DIM, Z_DIM, T * h * w, ops.stream())
        x = self._latent_in(x, T, h, w)  # 16 channels + 16 zero channels
        plan = decoder_plan()
        up0 = first_up(plan)
        # the latent-resolution stage sees whole frames (mid-block attention)
        x = self._decode_stage0_sharded(x, plan[:up0]) if shard else self._run(x, plan[:up0])
        if crop is not None:
            x = x[:, :, crop[0]:crop[1]].contiguous()
        y = self._decode_ups_sharded(x, plan[up0:]) if shard else self._run(x, plan[up0:])
        Fo, Ho, Wo, Cy = y.shape
        out = torch.empty((3, Fo, Ho, Wo), dtype=F32, device=self.device)
        call("wf_cl_to_ncthw", y.data_ptr(), out.data_ptr(), 3, Cy, Fo * Ho * Wo, 1.0, ops.stream())
        if shard and gather:
            # one all-gather of the 3-channel slabs (round 5 gathered the padded 32-channel slabs, 4.1 GB at C2, and converted the whole video
            # on every rank)
            P = self.comm.world
            allr = torch.empty((P, 3, Fo, Ho, Wo), dtype=F32, device=self.device)
            self.comm.all_gather(allr, out)
            out = allr.permute(1, 2, 0, 3, 4).reshape(3, Fo, P * Ho, Wo).contiguous()
        return out if crop is None else self._uncrop(out, crop, w)


    # ------------------------------------------------------------------------------------------------------------
    # decoding only what an IRR injection consumes
    # ------------------------------------------------------------------------------------------------------------
    # The decoded video of fuse_latents (SCHED:1285) is consumed by ONE statement, fused = ref * m + dec * (1 - m) (SCHED:1380): wherever the
    # mask is exactly 1 the result is the reference pixel whatever (finite) value dec has there.  Real warping masks are mostly 1 (the
    # warped view covers most of the frame; the hole grows from one side: SURVEY 8d's synthetic mask ends at 65 % valid), so only the pixel
    # COLUMNS that hold a mask value != 1 -- plus the receptive field of the layers that follow -- need decoding.  Everything up to the first
    # up-sampling layer (4 % of the decoder's flops, and the only place with global spatial coupling: the mid-block attention) runs on whole
    # frames; the rest runs on the cropped columns.  Every needed pixel is computed by the same kernels on the same inputs inside its
    # receptive field, so the BLEND RESULT is bit-identical to decoding everything (tests/test_gpu_vae.py); the other columns of the
    # returned video are zeros.
    CROP_HALO = 8      # latent columns decoded beyond the needed ones on either side.  Receptive field of the layers after the crop, walking
                       # back from a needed output pixel: head conv 1 px + 3 residual blocks 6 = 7 @480 -> (+1 conv) / 2 = 4 @240 -> + 6 + 1 = 11
                       # -> 6 @120 -> + 6 + 1 = 13 -> 7 latent columns; 8 keeps the crop on the 64-pixel tile grid of the convolutions
    CROP_MIN_GAIN = 0.9  # crop only when it leaves at most this fraction of the columns

    def needed_columns(self, mask: torch.Tensor):
        """mask [1,1,F,H,W] f32 (aligned to the decoded size) -> (c0, c1): the LATENT columns whose pixels the blend can see (mask != 1
        somewhere in the column), or (0, 0) when there is none: no pixel of the decoded video reaches the result then.  Whether a range is worth
        cropping to is _crop_range's decision.  One 8-byte read-back per distinct mask tensor (the mask of a job
        is the same object for all its injections)."""
        key = (mask.data_ptr(), mask._version, tuple(mask.shape))
        cache = self.__dict__.setdefault("_cols_cache", {})
        if key not in cache:
            cache.clear()
            W = mask.shape[-1]
            md = mask.to(device=self.device, dtype=F32).contiguous()
            out = torch.empty(2, dtype=torch.int32, device=self.device)
            call("wf_mask_column_range", md.data_ptr(), md.numel() // W, W, out.data_ptr(), ops.stream())
            x0, x1 = (int(v) for v in out.cpu())
            cache[key] = (mask, None if x1 <= x0 else (x0 // 8, (x1 + 7) // 8))   # (`mask` is held: its address cannot be recycled under the key)
        cols = cache[key][1]
        if cols is None:
            return (0, 0)   # no pixel of the decoded video reaches the result
        return cols

    def _crop_range(self, columns, w: int):
        """(c0, c1) needed latent columns -> the latent columns [a0, a1) to decode after the latent-resolution stage, or None (decode all)."""
        if columns is None:
            return None
        c0, c1 = columns
        if c1 <= c0:
            c0, c1 = 0, 8   # nothing is needed: the cheapest legal crop
        a0 = max(0, (c0 - self.CROP_HALO) // 8 * 8)
        a1 = min(w, -(-(c1 + self.CROP_HALO) // 8) * 8)
        return (a0, a1) if (a1 - a0) <= self.CROP_MIN_GAIN * w else None

    def _uncrop(self, out: torch.Tensor, crop, w: int) -> torch.Tensor:
        """[3, F, H, 8 (a1 - a0)] -> [3, F, H, 8 w] with zeros in the columns that were not decoded."""
        full = torch.zeros(tuple(out.shape[:-1]) + (8 * w,), dtype=out.dtype, device=out.device)
        full[..., 8 * crop[0]:8 * crop[1]].copy_(out)
        return full

    def _row_slab_of(self, t: torch.Tensor, y0: int, Hs: int) -> torch.Tensor:
        """Rows [y0, y0 + Hs) of a [1,C,F,H,W] tensor as a contiguous slab, kept while the tensor is unchanged (the reference video and the
        mask are the same objects for all 30 injections of a job)."""
        key = (t.data_ptr(), t._version, tuple(t.shape), y0, Hs)
        cache = self.__dict__.setdefault("_slab_cache", {})
        hit = cache.get(key)
        if hit is None:
            # two live entries (the reference video and the mask); an entry whose source differs from both is dropped, so a caller that
            # hands over fresh tensors every time pins at most two stale full-resolution sources, not four
            while len(cache) >= 2:
                cache.pop(next(iter(cache)))
            hit = cache[key] = (t, t[:, :, :, y0:y0 + Hs].contiguous())  # `t` is held so that its storage cannot be recycled under the key
        return hit[1]

    @torch.no_grad()
    def decode_blend_encode(self, z: torch.Tensor, ref: torch.Tensor, mask: torch.Tensor):
        """The pixel round trip of one IRR injection: decode (SCHED:1285) -> blend the warped reference in (SCHED:1375-1381) -> encode
        (SCHED:1384) -> the posterior.  z [1,16,T,h,w]; ref [1,3,F,H,W] / mask [1,1,F,H,W] fp32, already aligned to the decoded size.
        One GPU: exactly decode(), ops.blend_pixels(), encode().  Row-sharded (comm): the decoded video is NOT gathered -- the blend is
        element-wise per pixel, so each rank blends and re-encodes its own row slab (the encoder's first halo comes from the neighbours);
        only latent-resolution tensors are gathered.  Bit-identical to the gathered form."""
        self.check_range()   # the flag of the VAE call before this one (see _note_range)
        z = self._io_in(z)
        cols = self.needed_columns(mask) if self.crop_to_mask else None
        if z.shape[0] != 1 or not self.can_shard(z.shape[3]):
            dec = self.decode(z, return_dict=False, columns=cols)[0]
            return self.encode(ops.blend_pixels(ref, mask, dec)).latent_dist
        slab = self._io_out(self._decode_one(z[0], self._crop_range(cols, z.shape[4]), gather=False))  # [3, F, Hs, W] in the module dtype
        Hs = slab.shape[2]
        y0 = self.comm.rank * Hs
        fused = ops.blend_pixels(self._row_slab_of(ref, y0, Hs), self._row_slab_of(mask, y0, Hs), slab.unsqueeze(0))
        mom = self._io_out(self._encode_one_sharded(None, slab=self._io_in(fused)[0]).unsqueeze(0))
        self._note_range("decode_blend_encode")
        return _LatentDist(mom[:, :Z_DIM].contiguous(), mom[:, Z_DIM:])

    def _io_in(self, x: torch.Tensor) -> torch.Tensor:
        """A tensor entering the module: on the device, holding values of the module dtype (rounded to bf16 for a bf16 module: the
        reference's `.to(dtype=vae.dtype)`), as the contiguous f32 the kernels read."""
        x = x.to(self.device)
        if self.dtype == torch.bfloat16 and x.dtype != torch.bfloat16:
            x = ops.cast(x.contiguous(), torch.bfloat16)
        return x.contiguous() if x.dtype == F32 else ops.cast(x.contiguous(), F32)

    def _io_out(self, y: torch.Tensor) -> torch.Tensor:
        """A result leaving the module: in the module dtype."""
        return y if self.dtype == F32 else ops.cast(y.contiguous(), self.dtype)

    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """-> the posterior (latent_dist.mode() / .sample()).  fp16 operand modes: the range flag of THIS call is checked at the next VAE
        call or check_range() -- call check_range() before consuming the result if neither follows (or use strict_range=True)."""
        self.check_range()   # the flag of the VAE call before this one (see _note_range)
        x = self._io_in(x)
        moments = self._io_out(torch.stack([self._encode_one(v) for v in x]))
        self._note_range("encode")
        post = _LatentDist(moments[:, :Z_DIM].contiguous(), moments[:, Z_DIM:])
        if not return_dict:
            return (post,)
        return SimpleNamespace(latent_dist=post)

    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = True, columns=None):
        """-> the video, clamped to [-1, 1].  fp16 operand modes: see encode() for when the range flag of this call is checked.
        columns = (c0, c1) (an extension of the diffusers protocol, used by the IRR injection only): the caller consumes the LATENT columns
        [c0, c1) of the video alone (pixel columns 8 c0 .. 8 c1, see needed_columns); those are what a full decode returns, bit for bit,
        the other columns are unspecified finite values (zeros, or decoded where they fall inside the halo)."""
        self.check_range()   # the flag of the VAE call before this one (see _note_range)
        z = self._io_in(z)
        crop = self._crop_range(columns, z.shape[4])
        out = self._io_out(torch.stack([self._decode_one(v, crop) for v in z]))
        self._note_range("decode")
        if not return_dict:
            return (out,)
        return SimpleNamespace(sample=out)
