"""GPU: the kernels of csrc/dpt.hip (VGGT's DPT depth head) element by element against float64 on their own fp32 inputs, with the bars
derived in tests/vggt_depth_cases.py's docstring:
    wf_conv2d_f32               (9 Cin + 4) U sum|x||w| (+ |bias| + |resid|) + U |ref|
    wf_resize_bilinear_cl_f32   8 U A + 2 U ((Hi - 1) Dy + (Wi - 1) Dx) + U |table| + 2 U |ref|, against the RECORDED float64 custom_interpolate
    wf_dpt_depth_out            |ref| ((Cin + 2) U S + 2^-22 + U)
and the refusals (WF_EINVAL, no launch) of every documented precondition.  Each test prints its worst error / bar ratio."""
import itertools

import pytest
import torch

from tests import vggt_depth_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
U = dc.U


def _conv(x, wp, bias, resid, stride, relu_in=False, relu_resid=False, relu_out=False, out=None):
    from worldforge_amd import ops
    from worldforge_amd._ffi import call
    n, Hi, Wi, Cin = x.shape
    Cout = wp.shape[2]
    if out is None:
        out = torch.full((n, (Hi - 1) // stride + 1, (Wi - 1) // stride + 1, Cout), float("nan"), dtype=F32, device=DEV)
    call("wf_conv2d_f32", x.data_ptr(), wp.data_ptr(), None if bias is None else bias.data_ptr(), None if resid is None else resid.data_ptr(),
         out.data_ptr(), n, Hi, Wi, Cin, Cout, stride, int(relu_in), int(relu_resid), int(relu_out), ops.stream())
    return out


def _check_conv(shape, bias=True, resid=False, relu_in=False, relu_resid=False, relu_out=False, planted=False, what=""):
    n, Hi, Wi, Cin, Cout, stride = shape
    x, w, b, r = dc.conv_inputs(*shape, planted=planted)
    b, r = (b if bias else None), (r if resid else None)
    ref, bar = dc.conv_reference(x, w, b, r, stride, relu_in, relu_resid, relu_out, device=DEV)
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    got = _conv(dev(x), dev(dc.pack_conv_weight(w)), dev(b), dev(r), stride, relu_in, relu_resid, relu_out)
    torch.cuda.synchronize()
    assert tuple(got.shape) == tuple(ref.shape) and bool(torch.isfinite(got).all())
    ratio = ((got.cpu().to(F64) - ref).abs() / (bar + 1e-300)).max().item()
    print(f"wf_conv2d_f32 {shape} {what} bias {bias} resid {resid} relu in/resid/out {int(relu_in)}{int(relu_resid)}{int(relu_out)}: "
          f"worst |err| / bar {ratio:.3f}")
    assert ratio <= 1.0, (shape, what, ratio)
    return got


# the combinations the head runs: layer_rn (no bias), resize_layers.3 / output_conv1 (bias), RCU conv1, RCU conv2, output_conv2.0
HEAD_COMBOS = (dict(bias=False), dict(), dict(relu_in=True), dict(relu_in=True, resid=True, relu_resid=True), dict(relu_out=True))


@pytest.mark.parametrize("shape", dc.CONV_SHAPES)
def test_conv2d_f32_against_float64_on_every_shape(shape):
    for kw in HEAD_COMBOS:
        _check_conv(shape, **kw)
    _check_conv(shape, planted=True, what="planted corners")
    _check_conv(shape, planted=True, relu_in=True, what="planted corners")


def test_conv2d_f32_every_switch_combination():
    for shape in ((2, 5, 7, 36, 68, 1), (2, 5, 7, 36, 68, 2)):
        for bias, resid, relu_in, relu_out in itertools.product((False, True), repeat=4):
            for relu_resid in ((False, True) if resid else (False,)):
                _check_conv(shape, bias, resid, relu_in, relu_resid, relu_out)


def test_conv2d_f32_is_deterministic_and_independent_of_n():
    for shape in ((2, 5, 7, 36, 68, 2), (2, 11, 15, 128, 64, 2), (2, 44, 60, 64, 32, 1), (2, 92, 90, 8, 132, 1)):
        n, Hi, Wi, Cin, Cout, stride = shape
        x, w, b, r = dc.conv_inputs(*shape)
        x, wp, b, r = x.to(DEV), dc.pack_conv_weight(w).to(DEV), b.to(DEV), r.to(DEV)
        both = _conv(x, wp, b, r, stride, True, True, False)
        again = _conv(x, wp, b, r, stride, True, True, False)
        assert torch.equal(both, again), shape
        for i in range(n):     # one frame alone: other tile edges, and for the last shape another tile shape (64 x 64 tiles where 128 x 128 ones would number 130 instead of 260)
            one = _conv(x[i:i + 1].contiguous(), wp, b, r[i:i + 1].contiguous(), stride, True, True, False)
            assert torch.equal(one[0], both[i]), (shape, i)


def _interp_abs_terms(x, size):
    """float64 [C, hi, wi] -> A (interpolated |v|), Dy, Dx (interpolated |neighbour difference| along each axis) at the output size."""
    C, hi, wi = x.shape
    dy = torch.zeros_like(x)
    dx = torch.zeros_like(x)
    if hi > 1:
        d = (x[:, 1:] - x[:, :-1]).abs()                      # a pixel carries the larger of its differences to the two neighbours
        dy[:, :-1] = d
        dy[:, 1:] = torch.maximum(dy[:, 1:], d)
    if wi > 1:
        d = (x[:, :, 1:] - x[:, :, :-1]).abs()
        dx[:, :, :-1] = d
        dx[:, :, 1:] = torch.maximum(dx[:, :, 1:], d)
    f = lambda t: dc.resize_ac(t[None], size)[0]  # noqa: E731
    return f(x.abs()), f(dy), f(dx)


@pytest.mark.parametrize("ci", range(len(dc.RESIZE_CASES)))
@pytest.mark.parametrize("C", [4, 36, 64])
def test_resize_bilinear_cl_against_the_recorded_float64_interpolation(ci, C):
    from worldforge_amd import ops, vggt
    from worldforge_amd._ffi import call
    (hi, wi), (ho, wo) = dc.RESIZE_CASES[ci]
    base, want2 = dc.fixture()["resize"][ci]                                       # fp32 [2, hi, wi], float64 [2, ho, wo]
    # channel c = recorded channel c % 2 times 2^(c // 2): exact in fp32 and in float64, so the recorded reference scales with it
    scale = torch.tensor([2.0 ** (c // 2) for c in range(C)], dtype=F64)
    idx = torch.tensor([c % 2 for c in range(C)])
    x = (base[idx].to(F64) * scale[:, None, None]).to(F32)                         # [C, hi, wi]
    assert torch.equal(x.to(F64), base[idx].to(F64) * scale[:, None, None])
    ref = want2[idx] * scale[:, None, None]
    A, Dy, Dx = _interp_abs_terms(x.to(F64), (ho, wo))
    xin = torch.stack([x, -0.5 * x], 0).permute(0, 2, 3, 1).contiguous().to(DEV)   # n = 2: the second frame is an exact multiple
    col, row = vggt.dpt_pos_tables(C, ho, wo, (14 * ho, 14 * wo))
    table = torch.cat([col.t()[:, None, :].expand(C // 2, ho, wo), row.t()[:, :, None].expand(C // 2, ho, wo)], 0).to(F64)
    for tables in (None, (col.to(DEV), row.to(DEV))):
        out = torch.full((2, ho, wo, C), float("nan"), dtype=F32, device=DEV)
        call("wf_resize_bilinear_cl_f32", xin.data_ptr(), out.data_ptr(), 2, hi, wi, ho, wo, C, None if tables is None else tables[0].data_ptr(),
             None if tables is None else tables[1].data_ptr(), ops.stream())
        torch.cuda.synchronize()
        got = out.cpu().permute(0, 3, 1, 2).to(F64)
        worst = 0.0
        for f, m in ((0, 1.0), (1, -0.5)):
            want = ref * m + (0.0 if tables is None else table)
            bar = abs(m) * (8 * U * A + 2 * U * ((hi - 1) * Dy + (wi - 1) * Dx)) + (0.0 if tables is None else U * table.abs()) + 2 * U * want.abs()
            worst = max(worst, ((got[f] - want).abs() / (bar + 1e-300)).max().item())
            if (hi, wi) == (ho, wo) and tables is None:
                assert torch.equal(out[f].cpu(), xin[f].cpu())                     # equal sizes: an exact copy
        print(f"wf_resize_bilinear_cl_f32 {(hi, wi)} -> {(ho, wo)} C {C} tables {tables is not None}: worst |err| / bar {worst:.3f}")
        assert worst <= 1.0


@pytest.mark.parametrize("npix", [1, 63, 12345])
def test_dpt_depth_out_against_float64(npix):
    from worldforge_amd import ops
    from worldforge_amd._ffi import call
    g = torch.Generator().manual_seed(npix)
    x = torch.relu(torch.randn(npix, 32, generator=g))                              # what output_conv2.0's ReLU leaves
    w, b = torch.randn(2, 32, generator=g) * 0.3, torch.tensor([0.4, -0.3])
    depth, conf = (torch.full((npix,), float("nan"), dtype=F32, device=DEV) for _ in range(2))
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)                                    # held until the kernel has run
    call("wf_dpt_depth_out", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), depth.data_ptr(), conf.data_ptr(), npix, 32, ops.stream())
    torch.cuda.synchronize()
    v = x.to(F64) @ w.to(F64).t() + b.to(F64)
    S = x.to(F64).abs() @ w.to(F64).abs().t() + b.to(F64).abs()
    rel = (32 + 2) * U * S + 2.0 ** -22 + U
    for j, (got, ref) in enumerate(((depth, v[:, 0].exp()), (conf, 1 + v[:, 1].exp()))):
        ratio = ((got.cpu().to(F64) - ref).abs() / (ref.abs() * rel[:, j])).max().item()
        print(f"wf_dpt_depth_out npix {npix} {'depth' if j == 0 else 'conf'}: worst |err| / bar {ratio:.3f}")
        assert ratio <= 1.0
    assert bool((depth > 0).all()) and bool((conf > 1).all())


def test_documented_preconditions_are_refused_without_a_launch():
    from worldforge_amd import ops
    from worldforge_amd._ffi import lib
    L, st = lib(), ops.stream()
    buf = torch.zeros(1 << 16, dtype=F32, device=DEV)
    sentinel = torch.full((1 << 12,), 7.0, dtype=F32, device=DEV)
    p, o = buf.data_ptr(), sentinel.data_ptr()
    conv = lambda *a: L.wf_conv2d_f32(*a, st)  # noqa: E731
    assert conv(p, p, None, None, o, 1, 4, 4, 8, 8, 1, 0, 0, 0) == 0                # the well-formed call goes through
    torch.cuda.synchronize()
    sentinel.fill_(7.0)
    bad = [conv(p, p, None, None, o, 1, 4, 4, 6, 8, 1, 0, 0, 0),                    # Cin % 4
           conv(p, p, None, None, o, 1, 4, 4, 8, 6, 1, 0, 0, 0),                    # Cout % 4
           conv(p, p, None, None, o, 1, 4, 4, 8, 8, 3, 0, 0, 0),                    # stride 3
           conv(p, p, None, None, o, 1, 4, 4, 8, 8, 0, 0, 0, 0),                    # stride 0
           conv(p, p, None, None, None, 1, 4, 4, 8, 8, 1, 0, 0, 0),                 # NULL output
           conv(None, p, None, None, o, 1, 4, 4, 8, 8, 1, 0, 0, 0),                 # NULL input
           conv(p, None, None, None, o, 1, 4, 4, 8, 8, 1, 0, 0, 0),                 # NULL weights
           conv(p + 4, p, None, None, o, 1, 4, 4, 8, 8, 1, 0, 0, 0),                # misaligned input
           conv(p, p + 8, None, None, o, 1, 4, 4, 8, 8, 1, 0, 0, 0),                # misaligned weights
           conv(p, p, p + 4, None, o, 1, 4, 4, 8, 8, 1, 0, 0, 0),                   # misaligned bias
           conv(p, p, None, p + 12, o, 1, 4, 4, 8, 8, 1, 0, 0, 0),                  # misaligned residual
           conv(p, p, None, None, o + 4, 1, 4, 4, 8, 8, 1, 0, 0, 0),                # misaligned output
           conv(p, p, None, None, o, 1, 4, 4, 8, 8, 1, 0, 1, 0),                    # relu_resid without a residual
           conv(p, p, None, None, o, 0, 4, 4, 8, 8, 1, 0, 0, 0),                    # n = 0
           conv(p, p, None, None, o, 1, 0, 4, 8, 8, 1, 0, 0, 0),                    # Hi = 0
           conv(p, p, None, None, o, 4096, 1024, 1024, 8, 8, 1, 0, 0, 0),           # 2^31 elements and more
           L.wf_resize_bilinear_cl_f32(p, o, 1, 2, 2, 3, 3, 6, None, None, st),     # C % 4
           L.wf_resize_bilinear_cl_f32(p, None, 1, 2, 2, 3, 3, 4, None, None, st),
           L.wf_resize_bilinear_cl_f32(p, o, 1, 2, 2, 0, 3, 4, None, None, st),
           L.wf_resize_bilinear_cl_f32(p, o, 1, 2, 2, 3, 3, 4, p, None, st),        # one table without the other
           L.wf_resize_bilinear_cl_f32(p + 4, o, 1, 2, 2, 3, 3, 4, None, None, st),
           L.wf_resize_bilinear_cl_f32(p, o + 8, 1, 2, 2, 3, 3, 4, None, None, st),
           L.wf_dpt_depth_out(p, p, p, o, o + 256, 4, 6, st),                       # Cin % 4
           L.wf_dpt_depth_out(p, p, p, None, o, 4, 32, st),
           L.wf_dpt_depth_out(p, p, p, o, o + 256, 0, 32, st),                      # npix = 0
           L.wf_dpt_depth_out(p + 4, p, p, o, o + 256, 4, 32, st),                  # misaligned rows
           L.wf_dpt_depth_out(p, p, p, o + 2, o + 256, 4, 32, st)]                  # misaligned depth
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())                                            # nothing was launched
