"""GPU: stage 1 on the engine -- wf_select_pair_f32 + the host lerp against np.percentile (bit for bit), wf_depth_conf_filter against numpy,
wf_crack_fill_ex against the CPU restatement of tests/stage1_cases.py (masks, NaN patterns and fill decisions exact, the bars of
tests/test_gpu_warp.py for depths and colours; across tile corners and on a view wider than every capped grid with the inputs of
tests/stage1_edges.py), warp.warp_single_img against the recorded reference (tests/golden/g28_stage1_*), and
`python -m worldforge_amd.run_warp` end to end on a test-width VGGT checkpoint."""
import os
import re

import numpy as np
import pytest
import torch

from tests import stage1_cases as sc
from tests import stage1_edges as se

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FX = sc.fixture()


def _bits(x):
    return np.float32(x).view(np.uint32)


# ---- wf_select_pair_f32 -------------------------------------------------------------------------------------------------------------------
def _select_inputs(n, rng):
    conf = (1 + np.exp(rng.standard_normal(n))).astype(np.float32)
    ties = conf.copy()
    ties[rng.random(n) < 0.9] = 1.0
    signs = (3 * rng.standard_normal(n)).astype(np.float32)
    signs[signs == 0] = 1.0
    signs[n // 2] = -0.0            # ONE zero, the negative one: numpy's partition does not order -0.0 against +0.0
    inf = conf.copy()
    inf[n // 3] = np.inf
    return {"equal": np.full(n, 1.25, dtype=np.float32), "ties": ties, "signs": signs, "inf": inf,
            "ramp": (np.arange(n, 0, -1) * 0.25).astype(np.float32)}


def _gamma_zero_q(n):
    from worldforge_amd import warp
    for k in range(1, n - 1):
        q = 100.0 * k / (n - 1)
        if warp.percentile_plan(n, q) == (k, 0.0):      # float32 arithmetic lands on the integer
            return q
    return 0.0


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 48 * 64, 37 * 53])
def test_select_pair_and_host_lerp_equal_numpy_percentile_bit_for_bit(n):
    from worldforge_amd import warp
    rng = np.random.default_rng(n)
    qs = [(1 - c) * 100 for c in (0.999, 0.8, 0.5, 0.01)] + [_gamma_zero_q(n)]
    assert n <= 2 or warp.percentile_plan(n, qs[-1])[1] == 0.0      # (n <= 2 has no interior index: q = 0)
    for kind, x in _select_inputs(n, rng).items():
        xd = torch.from_numpy(x).to(DEV)
        s = np.sort(x)
        for q in qs:
            with np.errstate(invalid="ignore"):
                want = np.percentile(x.flatten(), q)
            assert want.dtype == np.float32
            k, _ = warp.percentile_plan(n, q)
            lo, hi, nans = warp.select_pair(xd, k)
            assert nans == 0 and _bits(lo) == _bits(s[k]) and _bits(hi) == _bits(s[min(k + 1, n - 1)]), (kind, n, q, k, lo, hi)
            got = warp.percentile_f32(xd, q)
            assert (np.isnan(got) and np.isnan(want)) or _bits(got) == _bits(want), (kind, n, q, got, want)


def test_select_pair_counts_nans_and_repeats_its_bits():
    from worldforge_amd import warp
    rng = np.random.default_rng(5)
    x = _select_inputs(37 * 53, rng)["ties"]
    xd = torch.from_numpy(x).to(DEV)
    a, b = warp.select_pair(xd, 1000), warp.select_pair(xd, 1000)
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1]) and a[2] == b[2] == 0
    y = x.copy()
    y[[3, 700, 1960]] = np.nan
    yd = torch.from_numpy(y).to(DEV)
    lo, hi, nans = warp.select_pair(yd, 10)
    s = np.sort(y)                                   # numpy sorts NaN last, as the kernel does
    assert nans == 3 and _bits(lo) == _bits(s[10]) and _bits(hi) == _bits(s[11])
    lo, hi, nans = warp.select_pair(yd, y.size - 1)
    assert nans == 3 and np.isnan(lo) and np.isnan(hi)
    with pytest.raises(ValueError, match="NaN"):
        warp.percentile_f32(yd, 20.0)


# ---- wf_depth_conf_filter -----------------------------------------------------------------------------------------------------------------
def _filter_case(H, W, seed):
    rng = np.random.default_rng(seed)
    depth = (2.0 + rng.standard_normal((H, W))).astype(np.float32)      # a few per cent <= 0
    depth[rng.random((H, W)) < 0.05] = np.nan
    depth[0, 0], depth[H - 1, W - 1] = 0.0, -1.5
    conf = (1 + np.exp(rng.standard_normal((H, W)))).astype(np.float32)
    conf[rng.random((H, W)) < 0.1] = 1.0
    return depth, conf


@pytest.mark.parametrize("H,W", [(5, 7), (37, 53), (300, 301)])
def test_depth_conf_filter_equals_numpy(H, W):
    from worldforge_amd import warp
    depth, conf = _filter_case(H, W, H)
    dd, cd = torch.from_numpy(depth).to(DEV), torch.from_numpy(conf).to(DEV)
    for c, use_conf in ((0.8, True), (0.3, True), (1.0, True), (0.5, False)):
        got, thr, mean, count = warp.depth_conf_filter(dd, cd if use_conf else None, c)
        want, wthr, wmean, wcount = sc.conf_filter(depth, conf if use_conf else None, c)
        if use_conf and c != 1.0:
            assert _bits(thr) == _bits(np.percentile(conf.flatten(), (1 - c) * 100)) == _bits(wthr)
        else:
            assert thr is None
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want)) and np.array_equal(g[~np.isnan(g)], want[~np.isnan(want)])
        assert count == wcount > 0
        assert abs(mean - wmean) <= sc.ulp32(wmean), (mean, wmean)       # (fp64 on both sides: the difference is ~1e-16)
    a, b = warp.depth_conf_filter(dd, cd, 0.8), warp.depth_conf_filter(dd, cd, 0.8)
    assert a[2] == b[2] and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_empty_selections_and_nan_confidence_are_refused():
    from worldforge_amd import warp
    depth, conf = _filter_case(37, 53, 1)
    dd, cd = torch.from_numpy(depth).to(DEV), torch.from_numpy(conf).to(DEV)
    got, thr, mean, count = warp.depth_conf_filter(dd, cd, 0.5, threshold=float(conf.max()))     # conf > max keeps nothing
    assert count == 0 and np.isnan(mean) and bool(torch.isnan(got).all())
    s = FX["scenes"]["s48"]
    kw = dict(extrinsic=s["E"], intrinsic=s["K"], image=s["image"], direction="left", degree=20.0, frame_num=3, device=DEV)
    with pytest.raises(ValueError, match="no pixel"):
        warp.warp_single_img(depth_map=np.full_like(s["depth"], np.nan), depth_conf=s["conf"], conf_threshold=0.8, **kw)
    with pytest.raises(ValueError, match="no pixel"):
        warp.warp_single_img(depth_map=-np.abs(s["depth"]), depth_conf=None, **kw)
    bad = s["conf"].copy()
    bad[7, 9] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        warp.warp_single_img(depth_map=s["depth"], depth_conf=bad, conf_threshold=0.8, **kw)


# ---- wf_crack_fill_ex -----------------------------------------------------------------------------------------------------------------------
MIN_NEIGHBORS = {1: 4, 2: 7, 3: 10, 4: 14}      # 10 in the 7 x 7 window is what ships; the others keep about the same share of the window


def _views(H, W, seed):
    """Six splat-like views (image u8, mask u8, depth f32 with NaN = empty): three depth layers with random holes; the same plus a far
    layer made ONLY of isolated pixels (every pixel of the farthest segment is an outlier); one depth value (min == max); an empty view;
    a view with <= 100 depths; another layered view with denser holes."""
    rng = np.random.default_rng(seed)

    def layered(p_hole):
        cells = rng.integers(0, 3, ((H + 3) // 4, (W + 3) // 4)).repeat(4, 0).repeat(4, 1)[:H, :W]
        d = (np.choose(cells, [1.0, 2.5, 6.0]) + 0.2 * rng.random((H, W))).astype(np.float32)
        m = (rng.random((H, W)) > p_hole).astype(np.uint8)
        return d, m

    def finish(d, m):
        i = (rng.random((H, W, 3)) * 255).astype(np.uint8)
        d = np.where(m > 0, d, np.float32(np.nan)).astype(np.float32)
        i[m == 0] = 0
        return i, m, d

    out = [finish(*layered(0.12))]
    d, m = layered(0.12)
    for k in range(3):                       # isolated far pixels, more than 2 * 4 + 1 apart along the long axis
        y, x = (H // 2, 5 + k * (W - 10) // 2) if W >= H else (5 + k * (H - 10) // 2, W // 2)
        d[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = 1.1
        d[y, x], m[y, x] = 20.0, 1
    out.append(finish(d, m))
    d, m = layered(0.12)
    out.append(finish(np.full((H, W), 2.0, dtype=np.float32), m))
    out.append(finish(d, np.zeros((H, W), dtype=np.uint8)))
    d, m = layered(0.1)
    keep = np.zeros((H, W), dtype=np.uint8)
    keep[:min(H, 8), :min(W, 10)] = 1        # <= 80 pixels
    out.append(finish(d, m & keep))
    out.append(finish(*layered(0.3)))
    assert int((~np.isnan(out[4][2])).sum()) <= 100 < int((~np.isnan(out[0][2])).sum())
    return [np.stack([v[j] for v in out]) for j in range(3)]


def _check_views(got, img, mask, depth, params, nseg, odepth):
    oi, om, od = (t.cpu().numpy() for t in got)
    filled = 0
    for f in range(img.shape[0]):
        wi, wm, wd = sc.warp_frame_fill(img[f], mask[f], depth[f], params, nseg, odepth, True)
        np.testing.assert_array_equal(om[f], wm)
        assert np.array_equal(np.isnan(od[f]), np.isnan(wd))
        np.testing.assert_allclose(od[f][~np.isnan(wd)], wd[~np.isnan(wd)], rtol=1e-6)
        assert np.abs(oi[f].astype(np.int32) - wi.astype(np.int32)).max() <= 1
        filled += int(((wm > 0) & (mask[f] == 0)).sum())
    return filled


@pytest.mark.parametrize("H,W", [(37, 53), (5, 70), (70, 5)])
def test_crack_fill_ex_equals_the_restatement(H, W):
    from worldforge_amd import warp
    img, mask, depth = _views(H, W, 7 * H + W)
    odepth = (2.0 + 0.05 * np.random.default_rng(3).standard_normal((H, W))).astype(np.float32)
    dev = [torch.from_numpy(a).to(DEV) for a in (img, mask, depth)]
    od = torch.from_numpy(odepth).to(DEV)
    filled = 0
    for r in (1, 2, 3, 4):
        for nseg in (1, 5, 8, 16):
            p = dict(min_neighbors=MIN_NEIGHBORS[r], neighbor_radius=r, min_valid_neighbors=2, max_crack_size=6, depth_threshold=0.1)
            for v0 in (0, 3):           # three views per call
                got = warp.crack_fill_ex(*(t[v0:v0 + 3] for t in dev), min_neighbors=p["min_neighbors"], neighbor_radius=r,
                                         min_valid_neighbors=2, num_segments=nseg, original_depth=od, has_depth_conf=True,
                                         depth_threshold=0.1, max_crack_size=6)
                filled += _check_views(got, img[v0:v0 + 3], mask[v0:v0 + 3], depth[v0:v0 + 3], p, nseg, odepth)
    assert filled > 16 * 6
    # the far layer of view 1 is all outliers under the shipped parameters: the restatement keeps none of its depths
    far = depth[1] == 20.0
    wd = sc.warp_frame_fill(img[1], mask[1], depth[1], warp.RUN_WARP_DEFAULTS, 8)[2]
    assert far.sum() == 3 and not (wd[far] == 20.0).any()


@pytest.mark.parametrize("H,W", [(37, 53), (64, 96)])
def test_crack_fill_ex_at_radius_1_and_5_segments_is_crack_fill_bit_for_bit(H, W):
    from worldforge_amd import warp
    img, mask, depth = _views(H, W, H)
    dev = [torch.from_numpy(a).to(DEV) for a in (img, mask, depth)]
    for mn, mvn, nseg in ((4, 2, 5), (4, 3, 5), (6, 2, 3)):
        a = warp.crack_fill(*dev, min_neighbors=mn, min_valid_neighbors=mvn, num_segments=nseg)
        b = warp.crack_fill_ex(*dev, min_neighbors=mn, neighbor_radius=1, min_valid_neighbors=mvn, num_segments=nseg)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
        assert bool(((a[1] > 0) & (dev[1] == 0)).any()) and bool(((a[1] == 0) & (dev[1] > 0)).any())   # cracks filled, outliers dropped
    c = warp.crack_fill_ex(*dev, min_neighbors=4, neighbor_radius=1, min_valid_neighbors=2, num_segments=5)
    d = warp.crack_fill_ex(*dev, min_neighbors=4, neighbor_radius=1, min_valid_neighbors=2, num_segments=5)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(c, d))
    with pytest.raises(RuntimeError, match="num_segments"):
        warp.crack_fill_ex(*dev, num_segments=17)
    with pytest.raises(RuntimeError, match="neighbor_radius"):
        warp.crack_fill_ex(*dev, neighbor_radius=5)


# ---- wf_crack_fill_ex / wf_crack_fill across tile corners and beyond one grid (inputs and their conditions: tests/stage1_edges.py) -------------
@pytest.mark.parametrize("H,W", se.CORNER_SHAPES)
def test_crack_fill_ex_across_tile_corners(H, W):
    """3 x 3 ragged tiles, a one-pixel overhang both ways, exactly one tile, exact multiples; radius 1..4 x {5, 8, 16} segments, the shipped
    (3, 8, 10) among them.  What a halo error would move, counted on the CPU at radius 3 / 8 segments and printed (the conditions for every
    radius and segment count are asserted in tests/test_stage1_edges_host.py): at 35 x 131, 111 outlier decisions hang on the halo beyond a
    vertical tile edge, 457 on the one beyond a horizontal edge, 34 on the diagonal tile's alone, and 241 fill decisions on the closing's
    halo (floors 8 / 8 / 4 / 4); 70 / 317 / 5 / 86 at 17 x 65, 61 / 273 / 8 / 97 at 32 x 128, none at 16 x 64 (one tile)."""
    from worldforge_amd import warp
    img, mask, depth = se.corner_views(H, W, 7 * H + W)
    fh = fv = fd = fc = 0
    for f in range(img.shape[0]):
        ids = se.segment_ids(depth[f], mask[f], 8)
        full, a, b, c = se.halo_flips(ids, 3, MIN_NEIGHBORS[3])
        fh, fv, fd, fc = fh + a, fv + b, fd + c, fc + se.closing_flips(ids, full)
    print(f"{H}x{W} r 3 / 8 segments: flips vertical {fh} horizontal {fv} diagonal-only {fd} closing {fc}")
    if (H, W) != (16, 64):
        assert fh >= 8 and fv >= 8 and fc >= 4 and fd >= (4 if (H, W) == (35, 131) else 1)
    odepth = (2.0 + 0.05 * np.random.default_rng(3).standard_normal((H, W))).astype(np.float32)
    dev = [torch.from_numpy(a).to(DEV) for a in (img, mask, depth)]
    od = torch.from_numpy(odepth).to(DEV)
    filled = 0
    for r in (1, 2, 3, 4):
        for nseg in (5, 8, 16):
            p = dict(min_neighbors=MIN_NEIGHBORS[r], neighbor_radius=r, min_valid_neighbors=2, max_crack_size=6, depth_threshold=0.1)
            got = warp.crack_fill_ex(*dev, min_neighbors=p["min_neighbors"], neighbor_radius=r, min_valid_neighbors=2, num_segments=nseg,
                                     original_depth=od, has_depth_conf=True, depth_threshold=0.1, max_crack_size=6)
            filled += _check_views(got, img, mask, depth, p, nseg, odepth)
    assert filled > 12 * 7


def test_crack_fill_on_one_wide_view_beyond_every_capped_grid():
    """17 x 15430 = 262 310 pixels in 2 x 242 = 484 tiles: more than the 1024 x 256 threads of the linear grids (k_cf_segid, k_cf_merge,
    k_cfx_merge), than the 120 x 256 of k_cfx_stats and than the 256 tiles k_cfx_order sums per step.  wf_crack_fill_ex with the shipped
    parameters and wf_crack_fill at radius 1 / 5 segments against their restatements; 18 of the 30 629 fills lie beyond pixel 262 144."""
    from oracle import crackfill as ocf
    from worldforge_amd import warp
    H, W = se.WIDE_SHAPE
    tiles = ((H + 15) // 16) * ((W + 63) // 64)
    assert H * W > 1024 * 256 and tiles > 256
    img, mask, depth = se.wide_view()
    dev = [torch.from_numpy(a).to(DEV) for a in (img, mask, depth)]
    p = dict(warp.RUN_WARP_DEFAULTS)
    got = warp.crack_fill_ex(*dev, min_neighbors=p["min_neighbors"], neighbor_radius=p["neighbor_radius"],
                             min_valid_neighbors=p["min_valid_neighbors"], num_segments=8)
    filled = _check_views(got, img, mask, depth, p, 8, None)
    tail = ((got[1][0].cpu().numpy() > 0) & (mask[0] == 0)).ravel()[1024 * 256:].sum()
    print("wide view: filled", filled, "beyond pixel 262144:", int(tail))
    assert filled > 10000 and tail >= 4
    # radius 1 / min_neighbors 3 keeps the far run of the last row: a segment whose only partial sums lie beyond k_cfx_order's first 256 tiles
    p1 = dict(p, min_neighbors=3, neighbor_radius=1)
    got = warp.crack_fill_ex(*dev, min_neighbors=3, neighbor_radius=1, min_valid_neighbors=p["min_valid_neighbors"], num_segments=8)
    _check_views(got, img, mask, depth, p1, 8, None)
    kept = np.nonzero(got[2][0].cpu().numpy() == 20.0)
    assert len(kept[0]) >= 10 and (kept[0] == H - 1).all() and kept[1].min() >= 64 * (256 - (W + 63) // 64)
    q = dict(ocf.RUN_WARP_PARAMS)
    oi, om, od = (t.cpu().numpy() for t in warp.crack_fill(*dev, min_neighbors=q["min_neighbors"], min_valid_neighbors=q["min_valid_neighbors"],
                                                           num_segments=5))
    wi, wm, wd = ocf.warp_frame_fill(img[0], mask[0], depth[0], q, 5)
    np.testing.assert_array_equal(om[0], wm)
    assert np.array_equal(np.isnan(od[0]), np.isnan(wd))
    np.testing.assert_allclose(od[0][~np.isnan(wd)], wd[~np.isnan(wd)], rtol=1e-6)
    assert np.abs(oi[0].astype(np.int32) - wi.astype(np.int32)).max() <= 1
    assert ((wm > 0) & (mask[0] == 0)).sum() > 10000 and ((wm == 0) & (mask[0] > 0)).sum() > 100


def test_small_crack_fill_on_one_wide_view():
    """wf_fill_small_cracks at 17 x 15430 (its grids are capped at 1024 x 256 threads too) against the oracle's fill_small_cracks: masks
    exact, colours within one grey level; 128 082 holes, 42 617 closed by step 1, 1566 more by the depth-guided step, 48 beyond pixel
    262 144."""
    from oracle import crackfill as ocf
    from worldforge_amd import warp
    img, mask, odepth = se.sparse_view()
    assert mask.size > 1024 * 256
    want_i, want_m = ocf.fill_small_cracks_depth_guided(img.astype(np.float32) / 255.0, mask, odepth, True, 0.1, 6, 2)
    step1 = ocf.fill_small_cracks(img.astype(np.float32) / 255.0, mask, 2)[1]
    oi, om = warp.small_crack_fill(torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV), torch.from_numpy(odepth).to(DEV), True, 0.1, 6, 2)
    om = om.cpu().numpy()
    print("small cracks, wide view: holes", int((mask == 0).sum()), "step 1", int(((step1 > 0) & (mask == 0)).sum()), "both steps",
          int(((want_m > 0) & (mask == 0)).sum()), "beyond pixel 262144:", int(((want_m > 0) & (mask == 0)).ravel()[1024 * 256:].sum()))
    assert int((want_m > step1).sum()) > 500 and ((want_m > 0) & (mask == 0)).ravel()[1024 * 256:].sum() >= 8
    assert np.array_equal(om, want_m)
    want_u8 = (want_i * 255).astype(np.uint8)
    assert np.abs(oi.cpu().numpy().astype(np.int32) - want_u8.astype(np.int32)).max() <= 1


# ---- the chain against the recorded reference -----------------------------------------------------------------------------------------------
MASK_CAP, COLOUR_CAP = 1e-3, 2e-3


@pytest.mark.parametrize("name", sorted(FX["cases"]))
def test_warp_single_img_against_the_recorded_reference(name):
    """Thresholds bit for bit, the mean depth within one fp32 ulp, infos equal; masks differ on <= 1e-3 of a case's pixels and colours by
    more than one level on <= 2e-3 of the pixels where the masks agree.  The caps are conditions: the reference's OWN reruns with the
    mean depth moved by an ulp (recorded in the meta file) must stay below a quarter of each -- they change 0 pixels on these scenes."""
    from worldforge_amd import warp
    c = FX["cases"][name]
    s = FX["scenes"][c["scene"]]
    sens = FX["meta"]["sensitivity"][name]
    assert sens["mask_changed"] / sens["pixels"] < MASK_CAP / 4 and sens["colour_changed"] / sens["pixels"] < COLOUR_CAP / 4
    p = FX["meta"]["crack_params"]
    _, thr, mean, count = warp.depth_conf_filter(torch.from_numpy(s["depth"]).to(DEV), torch.from_numpy(s["conf"]).to(DEV), c["thr"])
    print(name, "threshold", thr, c["threshold"], "mean", repr(mean), repr(float(c["mean_depth"])), "count", count)
    assert (thr is None) == (c["threshold"] is None) and (thr is None or _bits(thr) == _bits(c["threshold"]))
    assert abs(float(np.float32(mean)) - float(c["mean_depth"])) <= sc.ulp32(c["mean_depth"])
    imgs, masks, infos = warp.warp_single_img(s["E"], s["K"], torch.from_numpy(s["image"]).permute(2, 0, 1), s["depth"], depth_conf=s["conf"],
                                              direction=c["direction"], degree=c["degree"], conf_threshold=c["thr"],
                                              frame_num=FX["meta"]["frame_num"], fill_cracks=True, crack_params=p, look_at_depth=1.0,
                                              depth_segments=8, device=DEV)
    assert infos == c["infos"]
    imgs, masks = imgs.cpu().numpy(), masks.cpu().numpy()
    assert imgs.shape == c["images"].shape and masks.shape == c["masks"].shape and imgs.dtype == masks.dtype == np.uint8
    np.testing.assert_array_equal(imgs[0], c["images"][0])
    assert masks[0].all()
    dm = float((masks != c["masks"]).mean())
    same = masks == c["masks"]
    dc = float(((np.abs(imgs.astype(np.int32) - c["images"].astype(np.int32)).max(-1) > 1) & same).sum() / same.sum())
    print(name, "mask pixels that differ", dm, "colour pixels that differ by more than one level", dc)
    assert dm <= MASK_CAP and dc <= COLOUR_CAP, (dm, dc)


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def test_run_warp_main_writes_the_guidance_folder(tmp_path):
    from PIL import Image
    from tests import vggt_cases as vc, vggt_depth_cases as dc
    from worldforge_amd import harness, run_warp
    fx = dc.fixture()
    folder = vc.write_folder(str(tmp_path / "ckpt"), sd=fx["sd"], config=fx["chain_config"])
    src = vc.fixture()["preprocess"]["landscape_in"]
    os.makedirs(tmp_path / "imgs")
    for i in range(3):
        Image.fromarray(np.roll(src, 40 * i, axis=1)).save(str(tmp_path / "imgs" / f"{i}.png"))
    outs = []
    for tag in ("a", "b"):
        out = str(tmp_path / tag)
        assert run_warp.main(["--checkpoint", folder, "--image_path", str(tmp_path / "imgs"), "--output_path", out, "--camera", "1",
                              "--direction", "left", "--degree", "20", "--frame_single", "5", "--conf_single", "0.8", "--device", DEV]) == 0
        outs.append(out)
    names = sorted(os.listdir(os.path.join(outs[0], "warped_images")))
    assert len(names) == 10 and all(re.fullmatch(r"(warp|mask)_cam1_left_\d\d\.\d\d_deg\.png", n) for n in names)
    assert "warp_cam1_left_00.00_deg.png" in names and "mask_cam1_left_20.00_deg.png" in names
    frames, masks, first = harness.read_frames_from_directory(os.path.join(outs[0], "warped_images"))
    assert len(frames) == len(masks) == 5
    np.testing.assert_array_equal(np.asarray(frames[0]), np.roll(src, 40, axis=1))
    assert np.asarray(masks[0]).min() == 255 and set(np.unique(np.asarray(masks[-1]))) <= {0, 255}
    for n in names:                                  # a second run gives identical files
        with open(os.path.join(outs[0], "warped_images", n), "rb") as f, open(os.path.join(outs[1], "warped_images", n), "rb") as g:
            assert f.read() == g.read(), n
    with open(os.path.join(outs[0], "camera_info.txt"), encoding="utf-8") as f:
        txt = f.read()
    assert "Camera Index: 1" in txt and "Direction: left" in txt and "4: single_view_warped - left 20.00°" in txt
