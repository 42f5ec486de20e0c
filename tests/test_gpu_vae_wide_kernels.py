"""GPU: the kernels of the VAE's wide operand modes (precision = "fp16x3" -- the default --, "bf16x3", "fp16", "bf16") called one at a
time through the C-ABI, at the production shapes and layouts, against float64 CPU references of the same operation.

Operands are built by the production code: weights by worldforge_amd.vae.weight_operand (what AutoencoderKLWan.load_state_dict stores,
power-of-two scale included), activations by the production producers (wf_split_*, wf_cast_f16, wf_rms_silu_cl_blocked*, through
AutoencoderKLWan._operand / _rms where the VAE calls them that way).

Error model of a contraction (per output element):  |got - ref64| <= c_mode * S + tiny,  S = sum |x| |w| over the K0 products (float64).
  u = unit roundoff of an operand part (fp16 2^-11, bf16 2^-8).  One product x w made of the parts carries a relative error e:
    one term  (hi = x (1 + d), |d| <= u):  e = d_x + d_w + d_x d_w, each |d| <= u
    three terms (hi.hi + lo.hi + hi.lo, lo = rn(x - hi)): e = -(lo_x lo_w + t_x w + x t_w) / (x w), |lo| <= u |x|, tail |t| <= u^2 |x|
  The worst case of one product is 2u (one term) / 3u^2 (three terms), but the K0 products of an output carry independent, zero-mean
  errors (round-to-nearest of unrelated numbers) of rms <= u / u^2 |x w|.  Their sum stays below 6 sigma = 6 u^2 sqrt(sum (x w)^2); for
  products of roughly Gaussian x and w, sqrt(sum (x w)^2) <= 1.6 S / sqrt(K0), so 6 sigma <= u^2 S once K0 >= 100 (asserted).  The fp32
  accumulation (about K0 / 16 MFMA adds, each rounding by <= 2^-24 of a partial sum that is itself a random walk) is, by the same
  argument, below 2^-24 S; the bar allows 4 x that.  Hence
    c = u + 2^-22 (one term: bf16 2^-8, fp16 2^-11)        c = u^2 + 2^-22 (three terms: bf16x3 2^-16, fp16x3 2^-22 + 2^-22)
  tiny: the fp32 epilogue (acc * acc_scale + bias + residual: two roundings of <= 2^-24 each) and, for fp16 parts, the subnormal floor
  of a part (absolute 2^-25 per activation element: 2^-24 sum |w|).
Each three-term check runs once more with the lo parts of both operands zeroed (one-term arithmetic in disguise) and asserts that run
fails the bar by >= 8x: the bars can see a dropped term.  The measured max(|err| / bar) goes through tests._tol.within."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import vae as ovae
from tests._tol import within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, BF, H16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
MODES = ["bf16", "bf16x3", "fp16", "fp16x3"]
X3 = ("bf16x3", "fp16x3")
F16M = ("fp16", "fp16x3")
U32 = 2.0 ** -24
SENTINEL = 0x7FA5      # a NaN bit pattern in both fp16 and bf16: slots a kernel must not write are pre-filled with it
DISCRIM = 8.0          # a three-term check with its lo parts zeroed must exceed its bar by at least this factor


def _op(mode):
    return H16 if mode in F16M else BF


def _u(mode):
    return 2.0 ** -11 if mode in F16M else 2.0 ** -8


def c_mode(mode):
    """See the module docstring: u^2 (three terms) or u (one term) per |product|, plus 2^-22 for the fp32 accumulation."""
    u = _u(mode)
    return (u * u if mode in X3 else u) + 2.0 ** -22


def _vae(mode):
    from worldforge_amd.vae import AutoencoderKLWan
    return AutoencoderKLWan(DEV, precision=mode)


def _sfx(mode):
    return "_f16" if mode in F16M else ""


def _scale_args(mode, scale):
    """The trailing acc_scale of the *_f16 entry points."""
    return (float(scale if scale is not None else 1.0),) if mode in F16M else ()


def _weight(w_ck, mode):
    """f32 [Cout, taps, Cin] -> (device operand, acc_scale or None) exactly as load_state_dict stores it."""
    from worldforge_amd.vae import weight_operand
    op, scale = weight_operand(w_ck, mode, DEV)
    if mode in F16M:
        assert scale is not None and scale != 1.0          # acc_scale != 1: the epilogue's 2^-k is exercised
    return op, scale


def _zero_lo(t, C, side):
    """Three-term operand [..., 3C]: zero the lo third (side 0 [hi | lo | hi]: the middle one; side 1 [hi | hi | lo]: the last one)."""
    t = t.clone()
    if side == 0:
        t[..., C:2 * C] = 0
    else:
        t[..., 2 * C:] = 0
    return t


def _zero_page(nbytes, op):
    """A zero page of exactly `nbytes` at the start of a larger buffer whose rest is NaN: a read past the promised size shows up as NaN."""
    assert nbytes % 2 == 0
    buf = torch.full((nbytes // 2 + 8192,), float("nan"), dtype=op, device=DEV)
    buf[: nbytes // 2] = 0
    return buf


def _ratio(got, ref, bar):
    return ((got.to(F64) - ref).abs() / bar).max().item()


def _bar(mode, S, ref, extra, wabs):
    """c_mode * S + tiny (float64, broadcast over [..., Cout]); extra = |bias| + |residual| of the fp32 epilogue, wabs = sum |w| per Cout."""
    tiny = 2.0 ** -23 * (ref.abs() + extra) + (2.0 ** -24 * wabs if mode in F16M else 0.0) + 1e-30
    return c_mode(mode) * S + tiny


def _ref_conv(x, w, b, k, st, ss, pt, ph, pw, up2=False):
    """float64 reference of wf_conv3d_cl (zero padding pt in front of time, ph / pw before the rows / columns, the rest after):
    x [T,H,W,Cin], w [Cout,Cin,kt,kh,kw] -> [To,Ho,Wo,Cout]."""
    x = x.permute(3, 0, 1, 2).unsqueeze(0).to(F64)
    if up2:
        x = F.interpolate(x, scale_factor=(1.0, 2.0, 2.0), mode="nearest-exact")
    after_h = max(0, k[1] - 1 - ph) if ss == 1 else 1
    after_w = max(0, k[2] - 1 - pw) if ss == 1 else 1
    x = F.pad(x, (pw, after_w, ph, after_h, pt, 0))
    y = F.conv3d(x, w.to(F64), None if b is None else b.to(F64), stride=(st, ss, ss))
    return y[0].permute(1, 2, 3, 0)


# ---- 1. wf_conv3d_cl / wf_conv3d_cl_f16 -----------------------------------------------------------------------------------------------
CL_CASES = {
    # >= 32 768 output pixels, stride 1, 3x3x3: the 512-pixel ping-pong kernel (k_conv_pp<true> on fp16 operands); M = 35 136, ragged
    "pp_333_96": dict(T=9, H=61, W=64, cin=96, cout=96, k=(3, 3, 3), pt=2, ps=1),
    # the time conv (3,1,1) at M = 32 940 (ragged) with Cout = 384
    "pp_time_384": dict(T=9, H=60, W=61, cin=192, cout=384, k=(3, 1, 1), pt=2, ps=0),
    # Cout not a multiple of 96 (a partial second output block) on the ping-pong kernel: M = 33 000
    "pp_cout160": dict(T=3, H=110, W=100, cin=96, cout=160, k=(3, 3, 3), pt=2, ps=1),
    # nearest-2x upsample + 3x3 (the first upsample conv of the decoder): the generic kernel
    "up2": dict(T=2, H=12, W=20, cin=192, cout=96, k=(1, 3, 3), pt=0, ps=1, up2=True),
    # 'upsample3d' time conv with the frame interleave: the generic kernel
    "tsplit": dict(T=3, H=8, W=10, cin=96, cout=192, k=(3, 1, 1), pt=2, ps=0, tsplit=True),
}
_CL_REF = {}


def _cl_case(name):
    """Mode-independent part of a case: fp32 sources, float64 reference and S (cached: the four modes share them)."""
    if name not in _CL_REF:
        c = CL_CASES[name]
        g = torch.Generator().manual_seed(100 + sorted(CL_CASES).index(name))
        T, H, W, cin, cout, k = c["T"], c["H"], c["W"], c["cin"], c["cout"], c["k"]
        up2 = c.get("up2", False)
        x = torch.randn(T, H, W, cin, generator=g)
        w = torch.randn(cout, cin, *k, generator=g) / math.sqrt(cin * math.prod(k))
        b = torch.randn(cout, generator=g) * 0.1
        args = (k, 1, 1, c["pt"], c["ps"], c["ps"], up2)
        ref = _ref_conv(x, w, b, *args)
        S = _ref_conv(x.abs(), w.abs(), None, *args)
        resid = torch.randn(ref.shape, generator=g)
        wabs = w.abs().to(F64).sum(dim=(1, 2, 3, 4))
        _CL_REF[name] = (x, w, b, resid, ref, S, wabs)
    return _CL_REF[name]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CL_CASES))
def test_conv3d_cl_wide_vs_fp64(case, mode):
    from worldforge_amd import _ffi, ops
    c = CL_CASES[case]
    x, w, b, resid, ref, S, wabs = _cl_case(case)
    T, H, W, cin, cout, k = c["T"], c["H"], c["W"], c["cin"], c["cout"], c["k"]
    up2, tsplit = c.get("up2", False), c.get("tsplit", False)
    To, Ho, Wo, _ = ref.shape
    assert cin * math.prod(k) >= 100                                       # the error model's K0
    if case.startswith("pp_"):
        assert To * Ho * Wo >= 32768 and (To * Ho * Wo) % 512 != 0         # the ping-pong kernel, ragged last tile
    op = _op(mode)
    vae = _vae(mode)
    xo = vae._operand(x.to(DEV))                                           # [T,H,W,terms*Cin]: wf_split_* side 0 / wf_cast_f16 / bf16
    wo, scale = _weight(w.permute(0, 2, 3, 4, 1).reshape(cout, -1, cin), mode)
    K = xo.shape[-1]
    bd = b.to(DEV)
    zp = _zero_page(16, op)                                                # the ABI's ">= 16 bytes of zeros"

    def run(xin, win, rd, want16):
        shape = (1 + 2 * To, Ho, Wo, cout // 2) if tsplit else (To, Ho, Wo, cout)
        of = torch.full(shape, float("nan"), dtype=F32, device=DEV)
        o16 = torch.full(shape, float("nan"), dtype=op, device=DEV) if want16 else None
        _ffi.call("wf_conv3d_cl" + _sfx(mode), xin.data_ptr(), win.data_ptr(), bd.data_ptr(), rd.data_ptr() if rd is not None else None,
                  of.data_ptr(), o16.data_ptr() if o16 is not None else None, T, H, W, K, To, Ho, Wo, cout, k[0], k[1], k[2], 1, 1,
                  c["pt"], c["ps"], c["ps"], 1 if up2 else 0, 1 if tsplit else 0, zp.data_ptr(), *_scale_args(mode, scale), ops.stream())
        if tsplit:   # frame 1 + 2t + h of [1 + 2 To, Ho, Wo, Cout / 2] <- output frame t, channel half h; frame 0 is the caller's
            assert torch.isnan(of[0]).all() and (o16 is None or torch.isnan(o16[0]).all())
            of = of[1:].reshape(To, 2, Ho, Wo, cout // 2).permute(0, 2, 3, 1, 4).reshape(To, Ho, Wo, cout)
            if o16 is not None:
                o16 = o16[1:].reshape(To, 2, Ho, Wo, cout // 2).permute(0, 2, 3, 1, 4).reshape(To, Ho, Wo, cout)
        return of, o16

    babs = b.abs().to(F64)
    # (a) bias + residual, f32 output and its 16-bit copy (tsplit takes no residual: bias alone there)
    rd = None if tsplit else resid.to(DEV)
    want = ref if tsplit else ref + resid.to(F64)
    extra = babs + (0.0 if tsplit else resid.abs().to(F64))
    bar = _bar(mode, S, want, extra, wabs)
    of, o16 = run(xo, wo, rd, True)
    got = of.cpu()
    assert torch.isfinite(got).all()
    within(f"conv_cl.{mode}.bias_resid", _ratio(got, want, bar), 1.0)
    assert torch.equal(o16.cpu(), got.to(op))                              # the 16-bit copy: one round-to-nearest of the f32 value
    # (b) without the residual (f32 only: what every layer that is not a block's last conv runs)
    of, _ = run(xo, wo, None, False)
    bar0 = _bar(mode, S, ref, babs, wabs)
    within(f"conv_cl.{mode}.no_resid", _ratio(of.cpu(), ref, bar0), 1.0)
    # (c) three terms: the same launch with the lo parts zeroed must fail the bar
    if mode in X3:
        of, _ = run(_zero_lo(xo, cin, 0), _zero_lo(wo, cin, 1), None, False)
        r = _ratio(of.cpu(), ref, bar0)
        assert r >= DISCRIM, f"lo parts zeroed: max err / bar = {r:.2f} < {DISCRIM}: the bar cannot see a dropped term"


# ---- 2. wf_conv3d_cl_scatter_f16 / wf_conv3d_cl_scatter: the four-phase upsample ------------------------------------------------------
_SC_REF = {}


@pytest.mark.parametrize("mode", MODES)
def test_conv3d_cl_scatter_four_phase_vs_fp64(mode):
    """Nearest-2x + 3x3 conv as the four 2x2 phase convolutions of load_state_dict's up_phases, each on the ping-pong kernel
    (T H W = 36 864 source pixels >= 32 768), against float64 nearest-2x + conv2d.  The phase weights are sums of up to four taps, formed
    in fp32 as the VAE does (<= 2^-24 S more, inside the accumulation allowance)."""
    from worldforge_amd import _ffi, ops
    T, H, W, cin, cout = 3, 96, 128, 192, 96
    assert T * H * W >= 32768
    if not _SC_REF:
        g = torch.Generator().manual_seed(7)
        x = torch.randn(T, H, W, cin, generator=g)
        w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
        b = torch.randn(cout, generator=g) * 0.1
        xu = F.interpolate(x.to(F64).permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
        ref = F.conv2d(xu, w.to(F64), b.to(F64), padding=1).permute(0, 2, 3, 1)
        S = F.conv2d(xu.abs(), w.abs().to(F64), None, padding=1).permute(0, 2, 3, 1)
        resid = torch.randn(ref.shape, generator=g)
        _SC_REF.update(x=x, w=w, b=b, ref=ref, S=S, resid=resid)
    x, w, b, ref, S, resid = (_SC_REF[k] for k in ("x", "w", "b", "ref", "S", "resid"))
    op = _op(mode)
    xo = _vae(mode)._operand(x.to(DEV))
    K = xo.shape[-1]
    groups = (([0], [1, 2]), ([0, 1], [2]))                     # [phase][source offset] -> the 3-tap indices that read it (vae.py up_phases)
    phases = {}
    for py in range(2):
        for px in range(2):
            wp = torch.stack([torch.stack([sum(w[:, :, dy, dx] for dy in groups[py][a] for dx in groups[px][bb]) for bb in range(2)], dim=-1)
                              for a in range(2)], dim=-2)
            phases[py, px] = _weight(wp.permute(0, 2, 3, 1).reshape(cout, 4, cin), mode)
    wabs = 4 * w.abs().to(F64).sum(dim=(1, 2, 3))              # >= sum |w| of any phase
    bd = b.to(DEV)
    zp = _zero_page(16, op)

    def run(xin, rd, want16, zero_lo=False):
        of = torch.full((T, 2 * H, 2 * W, cout), float("nan"), dtype=F32, device=DEV)
        o16 = torch.full((T, 2 * H, 2 * W, cout), float("nan"), dtype=op, device=DEV) if want16 else None
        for (py, px), (wo, scale) in phases.items():
            if zero_lo:
                wo = _zero_lo(wo, cin, 1)
            _ffi.call("wf_conv3d_cl_scatter" + _sfx(mode), xin.data_ptr(), wo.data_ptr(), bd.data_ptr(),
                      rd.data_ptr() if rd is not None else None, of.data_ptr(), o16.data_ptr() if o16 is not None else None,
                      T, H, W, K, T, H, W, cout, 1, 2, 2, 1, 1, 0, 1 - py, 1 - px, zp.data_ptr(), 2 * H, 2 * W, 2, py, 2, px,
                      *_scale_args(mode, scale), ops.stream())
        return of.cpu(), (o16.cpu() if o16 is not None else None)

    babs = b.abs().to(F64)
    got, g16 = run(xo, resid.to(DEV), True)
    assert torch.isfinite(got).all() and torch.isfinite(g16).all()        # every output pixel written by exactly one phase
    want = ref + resid.to(F64)
    within(f"conv_scatter.{mode}.bias_resid", _ratio(got, want, _bar(mode, S, want, babs + resid.abs().to(F64), wabs)), 1.0)
    assert torch.equal(g16, got.to(op))
    got, _ = run(xo, None, False)
    assert torch.isfinite(got).all()
    bar0 = _bar(mode, S, ref, babs, wabs)
    within(f"conv_scatter.{mode}.no_resid", _ratio(got, ref, bar0), 1.0)
    if mode in X3:
        got, _ = run(_zero_lo(xo, cin, 0), None, False, zero_lo=True)
        r = _ratio(got, ref, bar0)
        assert r >= DISCRIM, f"lo parts zeroed: max err / bar = {r:.2f} < {DISCRIM}"


# ---- 3. wf_conv3d_333_f16 / wf_conv3d_333, layout 1, production Cin_stored --------------------------------------------------------------
C333_CASES = {
    "w200_h13_96": dict(T=2, H=13, W=200, cin=96, cout=96),         # 4 column tiles (the last 8 wide), H not a multiple of 8
    "w104_192": dict(T=2, H=12, W=104, cin=192, cout=192),          # 2 column tiles (ragged), 2 output-channel blocks (one partial)
    "w104_h9_384": dict(T=2, H=9, W=104, cin=384, cout=384),        # the 384-wide stage: 24 / 48 stored slices, 4 output blocks
    "thin_w200_32": dict(T=2, H=12, W=200, cin=96, cout=32),        # the head: Cout <= 32, k_conv_w4<0, 1, *>
    "halo_w104_96": dict(T=2, H=11, W=104, cin=96, cout=96, halo=True),   # row slab: ph = 0, Hi = Ho + 2, operand from halo_rows
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(C333_CASES))
def test_conv3d_333_layout1_vs_fp64(case, mode):
    """The operand is what _rms(blocked=True) writes: slice-major [T, Hi, Cin_stored / 16, W, 16], Cin_stored = 2/3 Cin for the three-term
    modes ([hi | lo] stored, K = [hi | lo | hi] rebuilt by the kernel).  Its fp32 source: the f32 activation of the one-term producer (same
    kernel instantiation as the blocked one, bit for bit) or, for three terms, hi + lo (exact in fp32; what those parts represent -- their
    distance from the fp64 RMS norm is test_rms_silu_producers_vs_fp64's)."""
    from worldforge_amd import _ffi, ops
    c = C333_CASES[case]
    T, Ho, W, cin, cout, halo = c["T"], c["H"], c["W"], c["cin"], c["cout"], c.get("halo", False)
    Hi = Ho + 2 if halo else Ho
    op, x3 = _op(mode), mode in X3
    g = torch.Generator().manual_seed(200 + sorted(C333_CASES).index(case))
    xpre = torch.randn(T, Hi, W, cin, generator=g) * 2 + 0.3
    gam = 1 + 0.05 * torch.randn(cin, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(cin * 27)
    b = torch.randn(cout, generator=g) * 0.1
    vae = _vae(mode)
    xd, gd = xpre.to(DEV), gam.to(DEV)
    full = vae._rms(xd, gd, silu=True, blocked=True)                          # [T, Hi, Cst/16, W, 16]
    nsl = full.shape[2]
    Cst = 16 * nsl
    assert Cst == (2 * cin if x3 else cin)
    K = Cst * 3 // 2 if x3 else Cst                                          # = 3 Cin / Cin: what _conv passes
    if halo:   # the slab's own rows from the producer's halo_rows form; rows 0 and Hi - 1 are the neighbours' (here: the same producer's)
        own = vae._rms(xd[:, 1:-1].contiguous(), gd, silu=True, blocked=True, halo=True)
        assert own.shape == full.shape
        own[:, 0], own[:, -1] = full[:, 0], full[:, -1]
        assert torch.equal(own.view(torch.int16), full.view(torch.int16))
        xop = own
    else:
        xop = full
    # the fp32 source of the operand
    sl = xop.permute(0, 1, 3, 2, 4).reshape(T, Hi, W, Cst).cpu()              # pixel-major [hi | lo] / [hi]
    if x3:
        src = sl[..., :cin].to(F64) + sl[..., cin:].to(F64)
    else:
        y32 = torch.empty((T * Hi * W, cin), dtype=F32, device=DEV)
        _ffi.call("wf_rms_silu_cl" + _sfx(mode), xd.data_ptr(), gd.data_ptr(), None, y32.data_ptr(), T * Hi * W, cin, 1, ops.stream())
        src = y32.cpu().reshape(T, Hi, W, cin).to(F64)
        assert torch.equal(src.to(op), sl)                                   # the operand is one rounding of that source
    ref = _ref_conv(src, w, b, (3, 3, 3), 1, 1, 2, 1, 1)
    S = _ref_conv(src.abs(), w.abs(), None, (3, 3, 3), 1, 1, 2, 1, 1)
    if halo:
        ref, S = ref[:, 1:-1], S[:, 1:-1]
    resid = torch.randn(ref.shape, generator=g)
    wabs = w.abs().to(F64).sum(dim=(1, 2, 3, 4))
    wo, scale = _weight(w.permute(0, 2, 3, 4, 1).reshape(cout, 27, cin), mode)

    def pack(wk):
        wp = torch.empty((27, K // 16, cout, 16), dtype=op, device=DEV)
        _ffi.call("wf_conv3d_pack333", wk.data_ptr(), wp.data_ptr(), cout, K, ops.stream())
        return wp

    wp = pack(wo)
    bd, rd = b.to(DEV), resid.to(DEV)
    ph = 0 if halo else 1

    def run(xin, wpk, rd_, want16, layout=1):
        need = int(_ffi.lib().wf_conv3d_333_zero_page_bytes(W, Cst, layout))
        zp = _zero_page(need, op)
        of = torch.full((T, Ho, W, cout), float("nan"), dtype=F32, device=DEV)
        o16 = torch.full((T, Ho, W, cout), float("nan"), dtype=op, device=DEV) if want16 else None
        _ffi.call("wf_conv3d_333" + _sfx(mode), xin.data_ptr(), wpk.data_ptr(), bd.data_ptr(), rd_.data_ptr() if rd_ is not None else None,
                  of.data_ptr(), o16.data_ptr() if o16 is not None else None, T, Hi, W, K, Ho, cout, ph, zp.data_ptr(), need, layout, Cst,
                  *_scale_args(mode, scale), ops.stream())
        return of.cpu(), (o16.cpu() if o16 is not None else None)

    babs = b.abs().to(F64)
    want = ref + resid.to(F64)
    got, g16 = run(xop, wp, rd, True)
    assert torch.isfinite(got).all()                                          # NaN here: a read past the zero page the ABI sized
    within(f"conv333.{mode}.bias_resid", _ratio(got, want, _bar(mode, S, want, babs + resid.abs().to(F64), wabs)), 1.0)
    assert torch.equal(g16, got.to(op))
    got0, _ = run(xop, wp, None, False)                                       # the ResidualBlock epilogue: bias, f32 out, no residual
    assert torch.isfinite(got0).all()
    bar0 = _bar(mode, S, ref, babs, wabs)
    within(f"conv333.{mode}.no_resid", _ratio(got0, ref, bar0), 1.0)
    # layout 0 (pixel-major, the same [hi | lo] storage) is legal for every one of these shapes: the same result within 1e-4
    xpm = xop.permute(0, 1, 3, 2, 4).reshape(T, Hi, W, Cst).contiguous()
    gotl0, _ = run(xpm, wp, rd, False, layout=0)
    assert torch.isfinite(gotl0).all()
    assert (gotl0 - got).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item())
    if x3:
        xz = xop.clone()
        xz[:, :, nsl // 2:] = 0                                               # the stored lo slices
        gz, _ = run(xz, pack(_zero_lo(wo, cin, 1)), None, False)
        r = _ratio(gz, ref, bar0)
        assert r >= DISCRIM, f"lo parts zeroed: max err / bar = {r:.2f} < {DISCRIM}"


# ---- 4. operand producers ---------------------------------------------------------------------------------------------------------------
def _rms_ref(x, gam):
    """float64 silu(rms_norm(x) * gamma) and the pre-SiLU y."""
    x = x.to(F64)
    y = F.normalize(x, dim=-1) * x.shape[-1] ** 0.5 * gam.to(F64)
    return F.silu(y), y


def _rms_bar(y, ref, C):
    """fp32 RMS norm + SiLU: the sum of squares (C / G sequential adds per lane + log2 G shuffle adds), sqrt, the division and two products
    give <= ((C / G + log2 G) / 2 + 5) 2^-24 relative on y; SiLU turns a relative error e of y into <= (1 + |y|) e of silu(y), and adds
    its own exp (__expf: error growing with |y|) and division: (2 |y| + 4) 2^-24."""
    G = 8 if C <= 128 else (16 if C <= 256 else (32 if C <= 512 else 64))
    ey = ((C / G + math.log2(G)) / 2 + 5) * U32
    return ((1 + y.abs()) * ey + (2 * y.abs() + 4) * U32) * ref.abs() + 2.0 ** -126


def _repr_bar(f16, ref):
    """hi + lo represents an fp32 value v to u^2 |v| (lo normal); fp16 lo is subnormal below 2^-14: absolute floor 2^-25 (as
    test_split_f16x3_reconstructs_fp32)."""
    return (2.0 ** -22 if f16 else 2.0 ** -16) * ref.abs() + (2.0 ** -25 if f16 else 0.0)


def _blocked_to_pixels(t, W, C, nsl):
    """[T, H, nsl, W, 16] -> [T, H, W, 16 nsl]."""
    return t.permute(0, 1, 3, 2, 4).reshape(t.shape[0], t.shape[1], W, 16 * nsl)


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("C", [32, 96, 192, 384])        # k_rms_silu<G>: G = 8, 8, 16, 32
def test_rms_silu_producers_vs_fp64(C, f16):
    """wf_rms_silu_cl{,_f16} (one term + f32), wf_rms_silu_cl_x3{,_f16} ([hi | lo | hi]) and wf_rms_silu_cl_blocked{,_f16} (split 0 / 1,
    halo_rows 0 / Hs).  Values against fp64; the blocked layout against the pixel-major producers BIT FOR BIT (split 1 and the x3 producer
    are k_rms_silu<G, true>, split 0 and the one-term producer k_rms_silu<G, false>: the same arithmetic per pixel)."""
    from worldforge_amd import _ffi, ops
    sfx, op = ("_f16", H16) if f16 else ("", BF)
    g = torch.Generator().manual_seed(300 + C + f16)
    T, Hs, W = 2, 5, 24
    npix = T * Hs * W
    x = torch.randn(T, Hs, W, C, generator=g) * torch.logspace(-2, 2, W).reshape(1, 1, W, 1)
    gam = 1 + 0.05 * torch.randn(C, generator=g)
    ref, y = _rms_ref(x, gam)
    ref, y = ref.reshape(npix, C), y.reshape(npix, C)
    xd, gd = x.to(DEV), gam.to(DEV)
    # one term
    o1 = torch.empty((npix, C), dtype=op, device=DEV)
    of = torch.empty((npix, C), dtype=F32, device=DEV)
    _ffi.call("wf_rms_silu_cl" + sfx, xd.data_ptr(), gd.data_ptr(), o1.data_ptr(), of.data_ptr(), npix, C, 1, ops.stream())
    of_c = of.cpu()
    within(f"rms_silu{sfx}.f32", _ratio(of_c, ref, _rms_bar(y, ref, C)), 1.0)
    assert torch.equal(o1.cpu(), of_c.to(op))
    # three terms, pixel-major
    o3 = torch.empty((npix, 3 * C), dtype=op, device=DEV)
    _ffi.call("wf_rms_silu_cl_x3" + sfx, xd.data_ptr(), gd.data_ptr(), o3.data_ptr(), npix, C, 1, ops.stream())
    o3c = o3.cpu()
    assert torch.equal(o3c[:, 2 * C:], o3c[:, :C])                              # [hi | lo | hi]
    hi, lo = o3c[:, :C].to(F64), o3c[:, C:2 * C].to(F64)
    within(f"rms_silu_x3{sfx}.hi_lo", _ratio(hi + lo, ref, _rms_bar(y, ref, C) + _repr_bar(f16, ref)), 1.0)
    # blocked, split 0 / 1, halo 0 / Hs
    for split in (0, 1):
        nsl = (2 if split else 1) * C // 16
        ob = torch.empty((T, Hs, nsl, W, 16), dtype=op, device=DEV)
        _ffi.call("wf_rms_silu_cl_blocked" + sfx, xd.data_ptr(), gd.data_ptr(), ob.data_ptr(), npix, C, 1, W, split, 0, ops.stream())
        pm = _blocked_to_pixels(ob.cpu(), W, C, nsl).reshape(npix, 16 * nsl)
        want = o3c[:, :2 * C] if split else o1.cpu()
        assert torch.equal(pm.view(torch.int16), want.view(torch.int16))
        oh = torch.full((T, Hs + 2, nsl, W, 16), 0, dtype=torch.int16, device=DEV)
        oh.fill_(SENTINEL)
        _ffi.call("wf_rms_silu_cl_blocked" + sfx, xd.data_ptr(), gd.data_ptr(), oh.data_ptr(), npix, C, 1, W, split, Hs, ops.stream())
        ohc = oh.cpu()
        assert (ohc[:, 0] == SENTINEL).all() and (ohc[:, Hs + 1] == SENTINEL).all()   # the halo rows are the caller's
        assert torch.equal(ohc[:, 1:Hs + 1], ob.cpu().view(torch.int16))


def test_rms_silu_producers_past_the_grid_cap():
    """npix = 530 000 > 16 384 blocks x 4 waves x 64 / G pixels (G = 8 at C = 96): the grid-stride loop of k_rms_silu runs a second lap."""
    from worldforge_amd import _ffi, ops
    C, W, f16 = 96, 100, 1
    npix = 5300 * W
    assert npix > 16384 * 4 * (64 // 8)
    g = torch.Generator().manual_seed(310)
    x = torch.randn(npix, C, generator=g)
    gam = 1 + 0.05 * torch.randn(C, generator=g)
    xd, gd = x.to(DEV), gam.to(DEV)
    o3 = torch.empty((npix, 3 * C), dtype=H16, device=DEV)
    _ffi.call("wf_rms_silu_cl_x3_f16", xd.data_ptr(), gd.data_ptr(), o3.data_ptr(), npix, C, 1, ops.stream())
    ob = torch.empty((npix // W, 2 * C // 16, W, 16), dtype=H16, device=DEV)
    _ffi.call("wf_rms_silu_cl_blocked_f16", xd.data_ptr(), gd.data_ptr(), ob.data_ptr(), npix, C, 1, W, 1, 0, ops.stream())
    assert torch.equal(ob.permute(0, 2, 1, 3).reshape(npix, 2 * C), o3[:, :2 * C])
    o3c = o3.cpu()
    del o3, ob
    ref, y = _rms_ref(x, gam)
    hi, lo = o3c[:, :C].to(F64), o3c[:, C:2 * C].to(F64)
    within("rms_silu_x3_f16.hi_lo", _ratio(hi + lo, ref, _rms_bar(y, ref, C) + _repr_bar(f16, ref)), 1.0)


# ---- 5. wf_operand_rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gaps", [True, False])
@pytest.mark.parametrize("fmt,side", [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (3, 0)])
def test_operand_rows_equals_standalone_producers(fmt, side, gaps):
    """Every written row equals the stand-alone producer's bit for bit (fmt 0 wf_split_bf16x3, 1 wf_split_f16x3, 2 wf_cast_f16, 3 bf16
    rounding); lead rows, gap rows, trailing rows and the columns past the operand's width keep their sentinel."""
    from worldforge_amd import _ffi, ops
    T, Hs, W, C, ld_src = 3, 4, 8, 96, 100
    rows = T * Hs * W
    width = 3 * C if fmt < 2 else C
    ld_dst = width + 8
    op = H16 if fmt in (1, 2) else BF
    g = torch.Generator().manual_seed(400 + 10 * fmt + side)
    src = (torch.randn(rows, ld_src, generator=g) * torch.logspace(-3, 3, rows).unsqueeze(1)).to(DEV)
    group, gap, lead = (Hs * W, 2 * W, W) if gaps else (0, 0, W)
    nrows_dst = T * (Hs + 2) * W if gaps else lead + rows + W
    dst = torch.full((nrows_dst, ld_dst), SENTINEL, dtype=torch.int16, device=DEV)
    _ffi.call("wf_operand_rows", src.data_ptr(), ld_src, dst.data_ptr(), ld_dst, rows, C, fmt, side, group, gap, lead, ops.stream())
    want = torch.empty((rows, width), dtype=op, device=DEV)
    if fmt in (0, 1):
        _ffi.call("wf_split_bf16x3" if fmt == 0 else "wf_split_f16x3", src.data_ptr(), ld_src, want.data_ptr(), width, rows, C, side,
                  ops.stream())
    elif fmt == 2:
        _ffi.call("wf_cast_f16", src.data_ptr(), ld_src, want.data_ptr(), width, rows, C, ops.stream())
    else:
        want = src[:, :C].to(BF)
    r = torch.arange(rows, device=DEV)
    drow = lead + r + ((r // group) * gap if gaps else 0)
    d = dst.cpu()
    assert torch.equal(d[drow.cpu(), :width], want.view(torch.int16).cpu())
    untouched = torch.ones(nrows_dst, dtype=torch.bool)
    untouched[drow.cpu()] = False
    assert int(untouched.sum()) == nrows_dst - rows
    assert (d[untouched] == SENTINEL).all() and (d[:, width:] == SENTINEL).all()


# ---- 6. wf_softmax_rows_f32 / wf_softmax_rows_f16 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("N", [6240, 1000])           # 6 240: the mid-block's tokens per frame at 480 x 832; 1 000: not a multiple of 64
def test_softmax_rows_vs_fp64(N, kind):
    """Rows: randn * 3, randn * 1e4 (the max subtraction), all entries equal, randn.  P[:, N:ldp] exactly 0; row sums 1 to the output
    type's precision.  Bar per element: the fp32 argument (s - max) * scale carries <= 2 |a| 2^-24 absolute, exp adds 2^-24 (x 1 + |a|
    for __expf's scaled argument), the row sum (N / 256 sequential adds + the 8-way tree) and the division (N / 256 + 10) 2^-24; the fp16
    output adds one rounding (2^-11 relative, 2^-25 absolute below the normal range)."""
    from worldforge_amd import _ffi, ops
    g = torch.Generator().manual_seed(500 + N)
    M, lds, ldp, scale = 4, N + 16, (N + 63) // 64 * 64 + 64, 384 ** -0.5
    S = torch.randn(M, lds, generator=g)
    S[0] *= 3
    S[1] *= 1e4
    S[2] = 5.0
    Sd = S.to(DEV)
    ref = torch.softmax(S[:, :N].to(F64) * scale, dim=-1)
    a = (S[:, :N].to(F64) - S[:, :N].to(F64).max(dim=-1, keepdim=True).values).abs() * scale
    bar = ((3 * a + N / 256 + 12) * U32) * ref + 2.0 ** -126
    if kind == "f32":
        P = torch.full((M, ldp), float("nan"), dtype=F32, device=DEV)
        _ffi.call("wf_softmax_rows_f32", Sd.data_ptr(), lds, P.data_ptr(), ldp, M, N, scale, ops.stream())
        u_out, floor = U32, 2.0 ** -149
    else:
        P = torch.full((M, ldp), float("nan"), dtype=H16, device=DEV)
        _ffi.call("wf_softmax_rows_f16", Sd.data_ptr(), lds, P.data_ptr(), ldp, M, N, scale, ops.stream())
        u_out, floor = 2.0 ** -11, 2.0 ** -25
        bar = bar + u_out * ref + floor
    Pc = P.cpu()
    assert (Pc[:, N:] == 0).all()
    within(f"softmax_rows_{kind}", _ratio(Pc[:, :N], ref, bar), 1.0)
    # row sums: the per-element bars summed, and the output type's own precision -- the shared 1 / sum ((N / 256 + 12) 2^-24) plus, for
    # fp16, one rounding per element (<= 2^-11 of the sum) and the subnormal floor
    sums = Pc[:, :N].to(F64).sum(dim=-1)
    err = (sums - 1).abs()
    assert (err <= bar.sum(dim=-1)).all(), err
    assert (err <= (N / 256 + 12) * U32 + (u_out if kind == "f16" else 0.0) + N * floor).all(), err
    assert torch.equal(Pc[2, :N], Pc[2, :1].expand(N))                      # all entries equal -> one value, ~1 / N
    assert abs(Pc[2, 0].item() * N - 1) <= 2 * u_out + 64 * U32


# ---- 7. wf_conv3d_small ------------------------------------------------------------------------------------------------------------------
SMALL_CASES = {
    "in3_96_f32": dict(T=5, H=12, W=14, cin=3, cout=96, k=(3, 3, 3), pt=2, ps=1, dtype="f32"),
    "in3_96_bf16": dict(T=5, H=12, W=14, cin=3, cout=96, k=(3, 3, 3), pt=2, ps=1, dtype="bf16"),
    "out96_3_clamp": dict(T=3, H=10, W=12, cin=96, cout=3, k=(3, 3, 3), pt=2, ps=1, dtype="f32", clamp=1.0),
    "q16_384": dict(T=2, H=8, W=9, cin=16, cout=384, k=(1, 1, 1), pt=0, ps=0, dtype="f32"),
    "q384_32": dict(T=2, H=8, W=9, cin=384, cout=32, k=(1, 1, 1), pt=0, ps=0, dtype="f32"),
}


@pytest.mark.parametrize("case", list(SMALL_CASES))
def test_conv3d_small_vs_fp64(case):
    """Direct fp32 convolution (one sequential fma chain per output from the bias): |err| <= (K0 + 1) 2^-24 (S + |bias|), the
    deterministic bound of K0 + 1 roundings; the clamp is 1-Lipschitz.  Weights in the header's [taps][Cin][Cout] layout."""
    from worldforge_amd import _ffi, ops
    c = SMALL_CASES[case]
    T, H, W, cin, cout, k, pt, ps = c["T"], c["H"], c["W"], c["cin"], c["cout"], c["k"], c["pt"], c["ps"]
    clamp = c.get("clamp", 0.0)
    g = torch.Generator().manual_seed(600 + sorted(SMALL_CASES).index(case))
    x = torch.randn(T, H, W, cin, generator=g)
    if c["dtype"] == "bf16":
        x = x.to(BF)
    w = torch.randn(cout, cin, *k, generator=g) / math.sqrt(cin * math.prod(k)) * (3.0 if clamp else 1.0)
    b = torch.randn(cout, generator=g) * 0.1
    ref = _ref_conv(x.float(), w, b, k, 1, 1, pt, ps, ps)
    S = _ref_conv(x.float().abs(), w.abs(), None, k, 1, 1, pt, ps, ps)
    if clamp:
        assert (ref.abs() > clamp).any()
        ref = ref.clamp(-clamp, clamp)
    To, Ho, Wo, _ = ref.shape
    wk = w.permute(2, 3, 4, 1, 0).reshape(-1, cin, cout).contiguous().to(DEV)
    of = torch.full((To, Ho, Wo, cout), float("nan"), dtype=F32, device=DEV)
    ob = torch.full((To, Ho, Wo, cout), float("nan"), dtype=BF, device=DEV)
    from worldforge_amd._ffi import WF_BF16, WF_F32
    xd, bd = x.to(DEV), b.to(DEV)
    _ffi.call("wf_conv3d_small", xd.data_ptr(), WF_BF16 if x.dtype == BF else WF_F32, wk.data_ptr(), bd.data_ptr(),
              of.data_ptr(), ob.data_ptr(), T, H, W, cin, To, Ho, Wo, cout, k[0], k[1], k[2], 1, 1, pt, ps, float(clamp), ops.stream())
    got = of.cpu()
    K0 = cin * math.prod(k)
    bar = (K0 + 1) * U32 * (S + b.abs().to(F64)) + 2.0 ** -126
    within(f"conv_small.{case}", _ratio(got, ref, bar), 1.0)
    assert torch.equal(ob.cpu(), got.to(BF))
    if clamp:
        assert got.abs().max().item() <= clamp


# ---- 8. wf_gemm_f16 with acc_scale != 1 on the VAE's operands ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp16", "fp16x3"])
@pytest.mark.parametrize("shape", ["qkv", "proj"])
def test_gemm_f16_acc_scale_vs_fp64(shape, mode):
    """The mid-block's 1x1 convolutions (to_qkv 384 -> 1152, proj 384 -> 384) at a ragged M, WF_EPI_F32 and WF_EPI_F32_ACC."""
    from worldforge_amd import _ffi, ops
    M, K0 = 2037, 384
    N = 3 * K0 if shape == "qkv" else K0
    g = torch.Generator().manual_seed(700 + N + (mode == "fp16x3"))
    x = torch.randn(M, K0, generator=g)
    w = torch.randn(N, K0, generator=g) / math.sqrt(K0)
    b = torch.randn(N, generator=g) * 0.1
    prev = torch.randn(M, N, generator=g)
    ref = x.to(F64) @ w.to(F64).t() + b.to(F64)
    S = x.abs().to(F64) @ w.abs().to(F64).t()
    wabs = w.abs().to(F64).sum(dim=1)
    xo = _vae(mode)._operand(x.to(DEV))
    wo, scale = _weight(w, mode)
    K = xo.shape[1]
    bd = b.to(DEV)

    def run(xin, win, epi, out):
        _ffi.call("wf_gemm_f16", xin.data_ptr(), win.data_ptr(), bd.data_ptr(), out.data_ptr(), M, N, K, K, K, N, epi, float(scale),
                  ops.stream())
        return out.cpu()

    babs = b.abs().to(F64)
    got = run(xo, wo, 2, torch.full((M, N), float("nan"), dtype=F32, device=DEV))      # WF_EPI_F32
    bar0 = _bar(mode, S, ref, babs, wabs)
    within(f"gemm_f16.{mode}.f32", _ratio(got, ref, bar0), 1.0)
    got = run(xo, wo, 4, prev.to(DEV))                                                    # WF_EPI_F32_ACC
    want = ref + prev.to(F64)
    within(f"gemm_f16.{mode}.f32_acc", _ratio(got, want, _bar(mode, S, want, babs + prev.abs().to(F64), wabs)), 1.0)
    if mode in X3:
        got = run(_zero_lo(xo, K0, 0), _zero_lo(wo, K0, 1), 2, torch.empty((M, N), dtype=F32, device=DEV))
        r = _ratio(got, ref, bar0)
        assert r >= DISCRIM, f"lo parts zeroed: max err / bar = {r:.2f} < {DISCRIM}"


# ---- one fp16x3 decode through the production paths, against the oracle in float64 ------------------------------------------------------
def test_fp16x3_decode_at_production_paths_vs_fp64_oracle():
    """Latent [16, 2, 12, 9] -> 5 x 96 x 72 pixels: the full-resolution stage has 34 560 pixels (the ping-pong conv kernel on fp16
    operands) and two 64-wide column tiles (the second ragged) in wf_conv3d_333_f16.  The reference is oracle/vae.py's decoder in float64
    (its decode() casts to fp32 on entry, so its body -- conv2, run_plan, clamp -- is called on float64 tensors).  Bars: the fp16x3 bars
    of the twin-golden tests."""
    from tests.test_gpu_vae import FP32_CLASS_BARS
    from worldforge_amd.vae import AutoencoderKLWan
    W = ovae.random_weights(seed=5)
    m = AutoencoderKLWan(DEV, precision="fp16x3").load_state_dict(W)
    assert m.precision == "fp16x3" and m.x3 and m.f16
    g = torch.Generator().manual_seed(800)
    z = torch.randn(1, 16, 2, 12, 9, generator=g)
    dec = m.decode(z.to(DEV), return_dict=False)[0].cpu()
    m.check_range()
    W64 = {k: v.to(F64) for k, v in W.items()}
    with torch.no_grad():
        ref = ovae.run_plan(ovae.causal_conv3d(z.to(F64), W64, "conv2"), W64, ovae.decoder_plan()).clamp(-1.0, 1.0)
    assert dec.shape == ref.shape == (1, 3, 5, 96, 72)
    rel = ((dec.to(F64) - ref).norm() / ref.norm()).item()
    mx = (dec.to(F64) - ref).abs().max().item()
    tol_rel, tol_abs = FP32_CLASS_BARS["fp16x3"]
    within("vae.fp16x3.decode_fp64.rel_l2", rel, tol_rel)
    within("vae.fp16x3.decode_fp64.max_abs", mx, tol_abs)

