"""What the Wan and the LongCat sampler share (worldforge_amd/sampler_common.py) and the LongCat prompt hand-off, on the host: neither the
library nor a device is needed."""
import pytest
import torch

from worldforge_amd import sampler_common as sc
from worldforge_amd.longcat_pipeline import prompt_batch

F, H, W = 5, 6, 8


def _mask5():
    return torch.rand(1, 1, F, H, W, generator=torch.Generator().manual_seed(1), dtype=torch.float64)


@pytest.mark.parametrize("name", ["3d", "4d_channels", "4d_batch1", "5d_channels", "5d"])
def test_guide_mask_shapes(name):
    """Every accepted layout comes out as [1, 1, F, H, W] fp32 holding the values given; an array gives what the tensor gives.  The two
    4-D layouts are one frame's, as in both references: [1, C, H, W] meets `shape[1] != 1` (channel 0 is taken), [1, 1, H, W] meets
    `shape[0] == 1`."""
    want = _mask5()
    given = {"3d": want[0, 0],                                  # [F, H, W]
             "4d_channels": want[0, :, :1].repeat(1, 3, 1, 1),  # [1, C, H, W]
             "4d_batch1": want[0, :, :1],                       # [1, 1, H, W]
             "5d_channels": want.repeat(1, 3, 1, 1, 1),         # [1, C, F, H, W]
             "5d": want}[name]
    if name.startswith("4d"):
        want = want[:, :, :1]
    got = sc.guide_mask(given, "cpu")
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) == (1, 1, want.shape[2], H, W)
    assert torch.equal(got, want.to(torch.float32))
    assert torch.equal(sc.guide_mask(given.numpy(), "cpu"), got)


@pytest.mark.parametrize("dtype", [None, torch.float32, torch.bfloat16])
def test_randn_is_the_cpu_generators_draw_in_the_dtype(dtype):
    shape = (2, 3, 5, 7)
    got = sc.randn(shape, torch.Generator().manual_seed(11), "cpu", dtype)
    want = torch.randn(shape, generator=torch.Generator().manual_seed(11), dtype=dtype)
    assert got.dtype == (dtype or torch.float32) and torch.equal(got, want)
    if dtype == torch.bfloat16:   # drawn IN bf16: another stream of the generator than an fp32 draw cast down
        cast_down = torch.randn(shape, generator=torch.Generator().manual_seed(11)).to(torch.bfloat16)
        assert not torch.equal(got, cast_down)


def test_randn_advances_the_generator_it_is_given():
    g, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    a, b = sc.randn((4,), g, "cpu"), sc.randn((4,), g, "cpu")
    a2, b2 = torch.randn((4,), generator=g2), torch.randn((4,), generator=g2)
    assert torch.equal(a, a2) and torch.equal(b, b2)


def test_prompt_batch_is_negative_then_positive():
    pe, ne = torch.full((1, 1, 4, 8), 1.0), torch.full((1, 1, 4, 8), -1.0)
    pm, nm = torch.ones(1, 4, dtype=torch.int64), torch.zeros(1, 4, dtype=torch.int64)
    e, m = prompt_batch("cpu", torch.bfloat16, pe, pm, ne, nm, do_cfg=True)
    assert e.dtype == torch.bfloat16 and tuple(e.shape) == (2, 1, 4, 8) and tuple(m.shape) == (2, 4)
    assert torch.equal(e[0], ne[0].to(torch.bfloat16)) and torch.equal(e[1], pe[0].to(torch.bfloat16))
    assert torch.equal(m[0], nm[0]) and torch.equal(m[1], pm[0])
    e, m = prompt_batch("cpu", torch.bfloat16, pe, pm, ne, nm)   # without CFG the negative pair is not used
    assert torch.equal(e, pe.to(torch.bfloat16)) and torch.equal(m, pm)


def test_prompt_batch_without_the_negative_prompt_raises():
    pe, pm = torch.zeros(1, 1, 4, 8), torch.ones(1, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"classifier-free guidance \(guidance_scale > 1\) needs the negative prompt embeddings"):
        prompt_batch("cpu", torch.bfloat16, pe, pm, None, None, do_cfg=True)


def test_preprocess_image_stays_where_the_input_is():
    img = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3))
    out = sc.preprocess_image(img, H, W)
    assert out.device.type == "cpu" and out.dtype == torch.float32 and tuple(out.shape) == (1, 3, H, W)
    assert torch.equal(out, 2.0 * img[None] - 1.0)
    with pytest.raises(ValueError):
        sc.preprocess_image(img, H + 1, W)
