"""Pillow's five convolution filters restated on the host, without a GPU: resample.filter_tables and resample_u8_numpy(filter=...) against
the installed `PIL.Image.resize(..., filter)`, bit for bit; the bicubic tables against pil_resample_tables, array for array; the refusals;
and the table invariants the device entries rely on (taps inside the axis, coefficient rows that sum to 1 << 22 within one unit per tap)."""
import numpy as np
import pytest
from PIL import Image

from worldforge_amd import resample

FILTERS = {"box": Image.Resampling.BOX, "bilinear": Image.Resampling.BILINEAR, "hamming": Image.Resampling.HAMMING,
           "bicubic": Image.Resampling.BICUBIC, "lanczos": Image.Resampling.LANCZOS}
SUPPORT = {"box": 0.5, "bilinear": 1.0, "hamming": 1.0, "bicubic": 2.0, "lanczos": 3.0}
# down with clipped windows, up from a handful of pixels, the VGGT and CLIP product sizes, a 200 -> 7 shrink with a skipped pass, a 1-pixel-wide input
SHAPES = [((45, 83), (32, 48)), ((5, 7), (48, 80)), ((720, 1280), (294, 518)), ((333, 500), (224, 336)), ((8, 200), (8, 7)), ((37, 1), (16, 5))]


def image_u8(kind, h, w, C, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w, C), dtype=np.uint8)
    return (rng.integers(0, 2, (h, w, C)) * 255).astype(np.uint8)


def pil_resize(a, H, W, filter):
    if a.shape[2] == 1:
        return np.array(Image.fromarray(a[:, :, 0], "L").resize((W, H), FILTERS[filter]))[:, :, None]
    return np.array(Image.fromarray(a, "RGB").resize((W, H), FILTERS[filter]))


@pytest.mark.parametrize("filter", sorted(FILTERS))
@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tables_and_emulation_equal_pil_for_every_filter(src, dst, filter):
    (h, w), (H, W) = src, dst
    for C in (1, 3):
        for n, kind in enumerate(("random", "binary")):
            a = image_u8(kind, h, w, C, seed=3 * n + C)
            want = pil_resize(a, H, W, filter)
            got = resample.resample_u8_numpy(a, (H, W), filter=filter)
            assert got.dtype == np.uint8 and got.shape == want.shape
            assert np.array_equal(got, want), (src, dst, filter, C, kind, int(np.abs(got.astype(int) - want).max()))


def test_the_default_filter_is_bicubic():
    a = image_u8("random", 45, 83, 3, seed=1)
    assert np.array_equal(resample.resample_u8_numpy(a, (32, 48)), resample.resample_u8_numpy(a, (32, 48), filter="bicubic"))
    assert np.array_equal(resample.resample_u8_numpy(a, (32, 48)), np.array(Image.fromarray(a, "RGB").resize((48, 32))))


@pytest.mark.parametrize("n_in,n_out", [(83, 48), (45, 32), (7, 80), (200, 7), (1, 5), (1280, 518), (720, 294), (33, 33)])
def test_bicubic_tables_are_pil_resample_tables_arrays(n_in, n_out):
    got, want = resample.filter_tables(n_in, n_out, "bicubic"), resample.pil_resample_tables(n_in, n_out)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    default = resample.filter_tables(n_in, n_out)
    assert np.array_equal(default[0], want[0]) and np.array_equal(default[1], want[1])


def test_unknown_filters_and_nearest_are_refused():
    for bad in ("nearest", "NEAREST", "cubic", "", None, 3):
        with pytest.raises(ValueError):
            resample.filter_tables(8, 4, bad)
    with pytest.raises(ValueError):
        resample.resample_u8_numpy(np.zeros((4, 4, 3), np.uint8), (2, 2), filter="nearest")
    for f in FILTERS:
        with pytest.raises(ValueError):
            resample.filter_tables(0, 4, f)
        with pytest.raises(ValueError):
            resample.filter_tables(4, -1, f)
    with pytest.raises(ValueError):                      # the bicubic-only function keeps refusing the others
        resample.pil_resample_tables(8, 4, filter="lanczos")


@pytest.mark.parametrize("filter", sorted(FILTERS))
def test_table_invariants(filter):
    for n_in, n_out in ((200, 7), (7, 200), (1, 5), (83, 48), (1280, 518), (33, 33)):
        bounds, coefs = resample.filter_tables(n_in, n_out, filter)
        ksize = int(np.ceil(SUPPORT[filter] * max(n_in / n_out, 1.0))) * 2 + 1
        assert bounds.dtype == np.int32 and coefs.dtype == np.int32 and bounds.shape == (n_out, 2) and coefs.shape == (n_out, ksize)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all()
        assert (bounds[:, 1] <= ksize).all()
        live = np.arange(ksize)[None, :] < bounds[:, 1:2]
        assert (coefs[~live] == 0).all()
        assert np.abs(coefs.sum(1).astype(np.int64) - (1 << 22)).max() <= ksize          # normalised, one rounding per tap
        # what wf_resample_u8_window_f32 takes from the geometry: no tap further than (ksize - 1) / 2 + 1 / 2 from the window's centre
        centre = (np.arange(n_out) + 0.5) * (n_in / n_out)
        half = 0.5 * (ksize - 1) + 0.5
        assert (bounds[:, 0] >= np.floor(centre - half)).all() and (bounds[:, 0] + bounds[:, 1] <= np.ceil(centre + half)).all()
        assert (np.diff(bounds[:, 0]) >= 0).all()
