"""wf_resample_u8_window_f32 (ops.resample_u8_window) against the installed PIL: `PIL.Image.resize(..., filter)` -> the numpy window ->
the host table indexed per channel, compared with torch.equal.  The yardstick is PIL, never the kernel.  The shapes are the smallest at
which the entry can still go wrong: window offsets that are no multiple of 4, a row of an odd length (so that the aligned groups of four
floats start at every phase and both clipped groups are reached), tap windows clipped at both borders, a first needed source row above 0
(the column pass then runs frame by frame), the whole image, one pixel in the last row and column, an enlargement, a 117-tap column
window with the row pass skipped, the column pass skipped with a strided read of the input at x0 = 7, and the look-up alone.  T = 3 checks
the frame stride, three distinct tables show a channel mix-up, binary data puts both clamps to work under the negative lobes."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

FILTERS = {"box": Image.Resampling.BOX, "bilinear": Image.Resampling.BILINEAR, "hamming": Image.Resampling.HAMMING,
           "bicubic": Image.Resampling.BICUBIC, "lanczos": Image.Resampling.LANCZOS}
ALL, TWO = tuple(sorted(FILTERS)), ("bicubic", "lanczos")
# (h, w), (H, W), (y0, x0, Hc, Wc), filters
CASES = [((45, 83), (32, 48), (5, 3, 21, 37), ALL),
         ((45, 83), (32, 48), (0, 0, 32, 48), TWO),
         ((45, 83), (32, 48), (31, 47, 1, 1), TWO),
         ((5, 7), (48, 80), (3, 5, 41, 70), TWO),
         ((8, 200), (8, 7), (2, 1, 5, 5), TWO),
         ((90, 160), (40, 160), (4, 7, 30, 101), TWO),
         ((33, 47), (33, 47), (2, 3, 29, 41), TWO)]
KINDS = ("random", "binary", "all256")


def frames_u8(kind, T, h, w, C, seed):
    rng = np.random.default_rng(seed)
    shape = (T, h, w, C)
    if kind == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    n = T * h * w * C
    return rng.permutation(np.arange(n) % 256).astype(np.uint8).reshape(shape)      # every byte value, as far as the frame is long


def tables(C, seed=11):
    """C distinct tables of 256 floats: no two channels share a value."""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((C, 256)).astype(np.float32))


def pil_resize(a, H, W, filter):
    """a u8 [T, h, w, C] -> [T, H, W, C], every frame through PIL.Image.resize (mode L for C = 1, RGB for C = 3)."""
    f = FILTERS[filter]
    if a.shape[3] == 1:
        return np.stack([np.array(Image.fromarray(x[:, :, 0], "L").resize((W, H), f))[:, :, None] for x in a])
    return np.stack([np.array(Image.fromarray(x, "RGB").resize((W, H), f)) for x in a])


def reference(a, size, window, lut, filter):
    """PIL resize -> window -> per-channel table: f32 [T, C, Hc, Wc]."""
    y0, x0, Hc, Wc = window
    win = pil_resize(a, size[0], size[1], filter)[:, y0:y0 + Hc, x0:x0 + Wc]
    lut = lut.numpy()
    return torch.from_numpy(np.stack([lut[c][win[..., c]] for c in range(a.shape[3])], axis=1))


@pytest.mark.parametrize("src,dst,window,filters", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CASES])
def test_window_equals_pil_window_and_table_bit_for_bit(src, dst, window, filters):
    from worldforge_amd import ops
    dev = torch.device("cuda:0")
    (h, w) = src
    for C in (1, 3):
        lut = tables(C)
        for T in (1, 3):
            for n, kind in enumerate(KINDS):
                a = frames_u8(kind, T, h, w, C, seed=17 * n + T + C)
                for f in filters:
                    want = reference(a, dst, window, lut, f)
                    got = ops.resample_u8_window(torch.from_numpy(a).to(dev), dst, window, lut.to(dev), filter=f)
                    assert got.dtype == torch.float32 and tuple(got.shape) == (T, C, window[2], window[3])
                    assert torch.equal(got.cpu(), want), (src, dst, window, C, T, kind, f)
                if C == 1:       # the rank-3 form with a flat table
                    got = ops.resample_u8_window(torch.from_numpy(a[..., 0]).to(dev), dst, window, lut[0].to(dev), filter=filters[0])
                    assert torch.equal(got.cpu(), reference(a, dst, window, lut, filters[0]))


def test_two_runs_give_equal_bits_and_a_misaligned_output_is_written_in_place():
    from worldforge_amd import _ffi, ops
    dev = torch.device("cuda:0")
    a = torch.from_numpy(frames_u8("random", 3, 45, 83, 3, seed=5)).to(dev)
    lut = tables(3).to(dev)
    one, two = (ops.resample_u8_window(a, (32, 48), (5, 3, 21, 37), lut, filter="lanczos") for _ in range(2))
    assert torch.equal(one, two)
    # the C entry on an output at every phase of a 16-byte line: the floats around it stay untouched
    xb, xc, xk = ops._resample_tables(83, 48, dev, "lanczos")
    yb, yc, yk = ops._resample_tables(45, 32, dev, "lanczos")
    ws = torch.empty(int(_ffi.lib().wf_resample_u8_window_f32_workspace_bytes(3, 45, 83, 32, 48, 3, 5, 3, 21, 37)), dtype=torch.uint8, device=dev)
    n = one.numel()
    for off in (1, 2, 3):
        buf = torch.full((n + 8,), -7.0, dtype=torch.float32, device=dev)
        _ffi.call("wf_resample_u8_window_f32", a.data_ptr(), buf.data_ptr() + 4 * off, 3, 45, 83, 32, 48, 3, 5, 3, 21, 37, xb.data_ptr(),
                  xc.data_ptr(), xk, yb.data_ptr(), yc.data_ptr(), yk, lut.data_ptr(), ws.data_ptr(), ops.stream())
        assert torch.equal(buf[off:off + n], one.reshape(-1)) and bool((buf[:off] == -7.0).all()) and bool((buf[off + n:] == -7.0).all())


@pytest.mark.parametrize("filter", ALL)
def test_resample_u8_with_a_filter_equals_pil(filter):
    from worldforge_amd import ops
    dev = torch.device("cuda:0")
    for C in (1, 3):
        for n, kind in enumerate(("random", "binary")):
            a = frames_u8(kind, 2, 45, 83, C, seed=n + C)
            got = ops.resample_u8(torch.from_numpy(a).to(dev), (32, 48), filter=filter).cpu()
            assert torch.equal(got, torch.from_numpy(pil_resize(a, 32, 48, filter))), (filter, C, kind)
    a = frames_u8("random", 2, 45, 83, 3, seed=9)
    assert torch.equal(ops.resample_u8(torch.from_numpy(a).to(dev), (32, 48)).cpu(), torch.from_numpy(pil_resize(a, 32, 48, "bicubic")))


def test_bad_arguments_are_refused_before_any_launch():
    from worldforge_amd import _ffi, ops
    dev = torch.device("cuda:0")
    L = _ffi.lib()
    fn = L.wf_resample_u8_window_f32
    a = torch.zeros(2 * 8 * 8 * 3, dtype=torch.uint8, device=dev)
    o = torch.full((2 * 3 * 4 * 4,), 7.0, dtype=torch.float32, device=dev)
    t = torch.zeros(64, dtype=torch.int32, device=dev)
    lut = torch.zeros(3, 256, dtype=torch.float32, device=dev)
    ws = torch.zeros(1024, dtype=torch.uint8, device=dev)
    p, q, tp, lp, wp, st = a.data_ptr(), o.data_ptr(), t.data_ptr(), lut.data_ptr(), ws.data_ptr(), ops.stream()
    # in, out, T, h, w, H, W, C, y0, x0, Hc, Wc, xbounds, xcoefs, xk, ybounds, ycoefs, yk, lut, workspace, stream
    bad = [fn(None, q, 2, 8, 8, 4, 4, 3, 0, 0, 4, 4, tp, tp, 5, tp, tp, 5, lp, wp, st),          # null pointers
           fn(p, None, 2, 8, 8, 4, 4, 3, 0, 0, 4, 4, tp, tp, 5, tp, tp, 5, lp, wp, st),
           fn(p, q, 2, 8, 8, 4, 4, 3, 0, 0, 4, 4, tp, tp, 5, tp, tp, 5, None, wp, st),
           fn(p, q, 0, 8, 8, 4, 4, 3, 0, 0, 4, 4, tp, tp, 5, tp, tp, 5, lp, wp, st),             # non-positive sizes
           fn(p, q, 2, 8, -1, 4, 4, 3, 0, 0, 4, 4, tp, tp, 5, tp, tp, 5, lp, wp, st),
           fn(p, q, 2, 8, 8, 4, 0, 3, 0, 0, 4, 4, tp, tp, 5, tp, tp, 5, lp, wp, st),
           fn(p, q, 2, 8, 8, 4, 4, 3, 0, 0, 0, 4, tp, tp, 5, tp, tp, 5, lp, wp, st),
           fn(p, q, 2, 8, 8, 4, 4, 3, 0, 0, 4, -2, tp, tp, 5, tp, tp, 5, lp, wp, st),
           fn(p, q, 2, 8, 8, 4, 4, 2, 0, 0, 4, 4, tp, tp, 5, tp, tp, 5, lp, wp, st),             # C = 2, C = 4
           fn(p, q, 2, 8, 8, 4, 4, 4, 0, 0, 4, 4, tp, tp, 5, tp, tp, 5, lp, wp, st),
           fn(p, q, 2, 8, 8, 4, 4, 3, 1, 0, 4, 4, tp, tp, 5, tp, tp, 5, lp, wp, st),             # a window that leaves H x W
           fn(p, q, 2, 8, 8, 4, 4, 3, 0, 2, 4, 3, tp, tp, 5, tp, tp, 5, lp, wp, st),
           fn(p, q, 2, 8, 8, 4, 4, 3, -1, 0, 4, 4, tp, tp, 5, tp, tp, 5, lp, wp, st),
           fn(p, q, 2, 8, 8, 4, 4, 3, 0, -1, 4, 4, tp, tp, 5, tp, tp, 5, lp, wp, st),
           fn(p, q, 2, 8, 8, 4, 4, 3, 0, 0, 4, 4, None, tp, 5, tp, tp, 5, lp, wp, st),           # a pass that runs without its tables
           fn(p, q, 2, 8, 8, 4, 4, 3, 0, 0, 4, 4, tp, tp, 5, tp, None, 5, lp, wp, st),
           fn(p, q, 2, 8, 8, 4, 4, 3, 0, 0, 4, 4, tp, tp, 0, tp, tp, 5, lp, wp, st),             # ... or without taps
           fn(p, q, 2, 8, 8, 4, 4, 3, 0, 0, 4, 4, tp, tp, 5, tp, tp, 0, lp, wp, st),
           fn(p, q, 2, 8, 8, 4, 4, 3, 0, 0, 4, 4, tp, tp, 5, tp, tp, 5, lp, None, st),           # the column pass without the workspace
           fn(p, q, 2, 4, 8, 4, 4, 3, 0, 0, 4, 4, tp, tp, 5, None, None, 0, lp, None, st)]       # ... also when the row pass is skipped
    assert all(rc != 0 for rc in bad), bad
    assert b"wf_resample_u8_window_f32" in L.wf_last_error()
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                                                                 # nothing was launched
    wsb = L.wf_resample_u8_window_f32_workspace_bytes
    assert wsb(2, 8, 8, 4, 4, 2, 0, 0, 4, 4) == 0 and wsb(0, 8, 8, 4, 4, 3, 0, 0, 4, 4) == 0 and wsb(2, 8, 8, 4, 4, 3, 1, 0, 4, 4) == 0
    assert wsb(2, 8, 8, 4, 4, 3, 0, 1, 4, 3) >= 2 * 8 * 3 * 3
    # skipped passes take null tables, and no column pass takes no workspace: a windowed look-up
    src = (torch.arange(2 * 8 * 8 * 3, dtype=torch.int32, device=dev) % 251).to(torch.uint8)
    ramp = torch.arange(3 * 256, dtype=torch.float32, device=dev).reshape(3, 256)
    got = torch.empty(2, 3, 5, 6, dtype=torch.float32, device=dev)
    assert fn(src.data_ptr(), got.data_ptr(), 2, 8, 8, 8, 8, 3, 2, 1, 5, 6, None, None, 0, None, None, 0, ramp.data_ptr(), None, st) == 0
    win = src.reshape(2, 8, 8, 3)[:, 2:7, 1:7].permute(0, 3, 1, 2).float()
    assert torch.equal(got, win + 256.0 * torch.arange(3, device=dev).reshape(1, 3, 1, 1))
    # and the wrapper refuses what it cannot hand over
    u8 = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError):
        ops.resample_u8_window(u8.float(), (2, 2), (0, 0, 2, 2), lut)
    with pytest.raises(TypeError):
        ops.resample_u8_window(u8, (2, 2), (0, 0, 2, 2), lut[:2])
    with pytest.raises(ValueError):
        ops.resample_u8_window(u8[..., :2], (2, 2), (0, 0, 2, 2), lut)
    with pytest.raises(ValueError):
        ops.resample_u8_window(u8, (2, 2), (1, 0, 2, 2), lut)
    with pytest.raises(ValueError):
        ops.resample_u8_window(u8, (2, 2), (0, 0, 2, 0), lut)
    with pytest.raises(ValueError):
        ops.resample_u8_window(u8, (2, 2), (0, 0, 2, 2), lut, filter="nearest")
    with pytest.raises(ValueError):
        ops.resample_u8(u8, (2, 2), filter="nearest")
    with pytest.raises(RuntimeError):
        ops.resample_u8_window(u8.cpu(), (2, 2), (0, 0, 2, 2), lut)
