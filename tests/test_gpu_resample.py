"""wf_resample_u8 (ops.resample_u8) against the installed `PIL.Image.resize`, bit for bit.  The yardstick is PIL, never the kernel.
The shapes are the smallest that reach a clipped tap window at both borders and a tap count that varies along the row (45 x 83 -> 32 x 48),
an enlargement from a handful of pixels (5 x 7 -> 48 x 80), rows of an odd byte length (W = 5, 7, 47, 83 with C = 1 and 3, so that the
dword walk of the flat output crosses row ends at every phase), each skipped pass, the copy, a 1-pixel-wide source, a 117-tap window
(200 -> 7), both clamps (binary data under the negative lobes: tests/test_resample_host.py shows on the host tables that the 45 x 83 binary
case leaves 0..255 on both sides) and the frame stride (T = 3)."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

SHAPES = [((45, 83), (32, 48)), ((5, 7), (48, 80)), ((90, 160), (90, 100)), ((45, 80), (30, 80)), ((33, 47), (33, 47)), ((37, 1), (16, 5)),
          ((8, 200), (8, 7))]
KINDS = ["random", "binary", "zeros", "full"]


def frames_u8(kind, T, h, w, C, seed):
    rng = np.random.default_rng(seed)
    shape = (T, h, w, C)
    if kind == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    return np.full(shape, 0 if kind == "zeros" else 255, np.uint8)


def pil_resize(a, H, W):
    """a u8 [T, h, w, C] -> [T, H, W, C], every frame through PIL.Image.resize (mode L for C = 1, RGB for C = 3)."""
    if a.shape[3] == 1:
        return np.stack([np.array(Image.fromarray(f[:, :, 0], "L").resize((W, H)))[:, :, None] for f in a])
    return np.stack([np.array(Image.fromarray(f, "RGB").resize((W, H))) for f in a])


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resample_u8_equals_pil_bit_for_bit(src, dst):
    from worldforge_amd import ops
    (h, w), (H, W) = src, dst
    dev = torch.device("cuda:0")
    for C in (1, 3):
        for T in (1, 3):
            for n, kind in enumerate(KINDS):
                a = frames_u8(kind, T, h, w, C, seed=17 * n + T + C)
                want = torch.from_numpy(pil_resize(a, H, W))
                got = ops.resample_u8(torch.from_numpy(a).to(dev), (H, W))
                assert got.dtype == torch.uint8 and tuple(got.shape) == (T, H, W, C)
                got = got.cpu()
                assert torch.equal(got, want), (src, dst, C, T, kind, int((got.int() - want.int()).abs().max()))
                if C == 1:       # the rank-3 form the masks take
                    assert torch.equal(ops.resample_u8(torch.from_numpy(a[..., 0]).to(dev), (H, W)).cpu(), want[..., 0])


def test_two_runs_give_equal_bytes_and_a_misaligned_output_is_written_in_place():
    from worldforge_amd import _ffi, ops, resample
    dev = torch.device("cuda:0")
    a = torch.from_numpy(frames_u8("random", 3, 45, 83, 3, seed=5)).to(dev)
    one, two = ops.resample_u8(a, (32, 48)), ops.resample_u8(a, (32, 48))
    assert torch.equal(one, two)
    # the C entry on an output that starts at every offset inside a dword: the bytes around it stay untouched
    xb, xc = (torch.from_numpy(t).to(dev) for t in resample.pil_resample_tables(83, 48))
    yb, yc = (torch.from_numpy(t).to(dev) for t in resample.pil_resample_tables(45, 32))
    ws = torch.empty(int(_ffi.lib().wf_resample_u8_workspace_bytes(3, 45, 83, 32, 48, 3)), dtype=torch.uint8, device=dev)
    n = one.numel()
    for off in (1, 2, 3):
        buf = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device=dev)
        _ffi.call("wf_resample_u8", a.data_ptr(), buf.data_ptr() + off, 3, 45, 83, 32, 48, 3, xb.data_ptr(), xc.data_ptr(), xc.shape[1],
                  yb.data_ptr(), yc.data_ptr(), yc.shape[1], ws.data_ptr(), ops.stream())
        assert torch.equal(buf[off:off + n], one.reshape(-1)) and bool((buf[:off] == 0xA5).all()) and bool((buf[off + n:] == 0xA5).all())


def test_bad_arguments_are_refused_before_any_launch():
    from worldforge_amd import _ffi, ops
    dev = torch.device("cuda:0")
    L = _ffi.lib()
    a = torch.zeros(2 * 8 * 8 * 3, dtype=torch.uint8, device=dev)
    o = torch.full((2 * 4 * 4 * 3,), 7, dtype=torch.uint8, device=dev)
    t = torch.zeros(64, dtype=torch.int32, device=dev)
    ws = torch.zeros(1024, dtype=torch.uint8, device=dev)
    p, q, tp, wp, st = a.data_ptr(), o.data_ptr(), t.data_ptr(), ws.data_ptr(), ops.stream()
    bad = [L.wf_resample_u8(p, q, 0, 8, 8, 4, 4, 3, tp, tp, 5, tp, tp, 5, wp, st),          # T = 0
           L.wf_resample_u8(p, q, 2, 8, -1, 4, 4, 3, tp, tp, 5, tp, tp, 5, wp, st),         # a negative size
           L.wf_resample_u8(p, q, 2, 8, 8, 4, 0, 3, tp, tp, 5, tp, tp, 5, wp, st),
           L.wf_resample_u8(p, q, 2, 8, 8, 4, 4, 2, tp, tp, 5, tp, tp, 5, wp, st),          # C = 2
           L.wf_resample_u8(p, q, 2, 8, 8, 4, 4, 4, tp, tp, 5, tp, tp, 5, wp, st),          # C = 4
           L.wf_resample_u8(None, q, 2, 8, 8, 4, 4, 3, tp, tp, 5, tp, tp, 5, wp, st),       # null pointers
           L.wf_resample_u8(p, None, 2, 8, 8, 4, 4, 3, tp, tp, 5, tp, tp, 5, wp, st),
           L.wf_resample_u8(p, q, 2, 8, 8, 4, 4, 3, None, tp, 5, tp, tp, 5, wp, st),        # a pass that runs without its tables
           L.wf_resample_u8(p, q, 2, 8, 8, 4, 4, 3, tp, tp, 5, tp, None, 5, wp, st),
           L.wf_resample_u8(p, q, 2, 8, 8, 4, 4, 3, tp, tp, 0, tp, tp, 5, wp, st),          # ... or without taps
           L.wf_resample_u8(p, q, 2, 8, 8, 4, 4, 3, tp, tp, 5, tp, tp, 5, None, st)]        # two passes without the workspace
    assert all(rc != 0 for rc in bad), bad
    assert b"wf_resample_u8" in L.wf_last_error()
    torch.cuda.synchronize()
    assert bool((o == 7).all())                                                            # nothing was launched
    assert L.wf_resample_u8_workspace_bytes(2, 8, 8, 4, 4, 2) == 0 and L.wf_resample_u8_workspace_bytes(0, 8, 8, 4, 4, 3) == 0
    assert L.wf_resample_u8_workspace_bytes(2, 8, 8, 4, 4, 3) >= 2 * 8 * 4 * 3
    # a skipped pass takes null tables (and no workspace)
    src = (torch.arange(2 * 8 * 8 * 3, dtype=torch.int32, device=dev) % 251).to(torch.uint8)
    same = torch.empty_like(src)
    assert L.wf_resample_u8(src.data_ptr(), same.data_ptr(), 2, 8, 8, 8, 8, 3, None, None, 0, None, None, 0, None, st) == 0
    assert torch.equal(src, same)
    # and the wrapper refuses what it cannot hand over
    with pytest.raises(TypeError):
        ops.resample_u8(torch.zeros(1, 4, 4, 3, device=dev), (2, 2))
    with pytest.raises(ValueError):
        ops.resample_u8(torch.zeros(1, 4, 4, 2, dtype=torch.uint8, device=dev), (2, 2))
    with pytest.raises(ValueError):
        ops.resample_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev), (0, 2))
    with pytest.raises(RuntimeError):
        ops.resample_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), (2, 2))


def test_u8_lut_planar_indexes_the_host_tables():
    from worldforge_amd import ops, resample
    dev = torch.device("cuda:0")
    frames, masks = (torch.from_numpy(t) for t in resample.u8_to_f32_tables())
    a = torch.from_numpy(frames_u8("random", 3, 5, 7, 3, seed=2))
    a.view(-1)[:256] = torch.from_numpy(np.arange(256, dtype=np.uint8))       # every input value
    got = ops.u8_lut_planar(a.to(dev), frames.to(dev)).cpu()
    assert tuple(got.shape) == (3, 3, 5, 7) and torch.equal(got, (a.float() / 255.0).permute(3, 0, 1, 2))
    m = a[..., 0].contiguous()
    got = ops.u8_lut_planar(m.to(dev), masks.to(dev)).cpu()
    assert tuple(got.shape) == (1, 3, 5, 7) and torch.equal(got[0], torch.from_numpy((m.numpy() / 255.0).astype(np.float32)))
    L = __import__("worldforge_amd._ffi", fromlist=["lib"]).lib()
    assert L.wf_u8_lut_planar_f32(None, None, None, 1, 1, 1, 1, ops.stream()) != 0 and L.wf_u8_lut_planar_f32(1, 1, 1, 0, 1, 1, 1, ops.stream()) != 0
