"""GPU: the dynamic-scene stage 1 -- wf_dc_warp_frames (the whole frame loop of DepthCrafter/warp_depthcrafter.py:257-290 in one call) against
the per-frame entry points (the same kernels at T = 1), the bits all three returned before they shared kernels (g30_pointrender_parent.json)
and oracle/pointrender.py, wf_resize_bilinear_aa_f32 against torch's CPU kernel, the whole route against the
reference's recorded frames (G29, tools/make_dynamic_warp_golden.py) and the command line's hand-over to the sampler's frame reader.

The renderer's radius is fixed (0.005 NDC units) and the reference un-projects pixel (i, j) to a pixel CORNER, so below a short side of
about 283 pixels its coverage is specks (tests/dynwarp_cases.py).  Where a small case needs coverage, `K_points` = K shifted by half a pixel
un-projects to the pixel centres: the identity camera then covers every pixel with its own point, at any size."""
import os

import numpy as np
import pytest
import torch

from oracle import pointrender as opr
from tests import dynwarp_cases as dc
from tests import pointrender_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


def _K(H, W, centred=False):
    K = np.array([[525, 0, W / 2], [0, 525, H / 2], [0, 0, 1]], dtype=F32)
    if centred:
        K[:2, 2] -= F32(0.5)
    return K


def _depth(disp):
    return (F32(1.0) / (disp.astype(F32) + F32(0.1))).astype(F32)


def _quantise(x):
    return np.clip(np.rint(np.asarray(x, dtype=F32) * F32(255)), 0, 255).astype(np.uint8)


def _moved(tx, th):
    cam = np.eye(4)
    cam[0, 3], cam[1, 3] = tx, -tx / 2
    cam[:3, :3] = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    return cam


_scene = pc.scene


def _per_frame(rgb, disp, cams, K, from_, Kp=None):
    """The loop the batched call replaces: warp.render_depthcrafter_frame per frame (with K_points: the same composition from its parts)."""
    from worldforge_amd import warp
    T, H, W = disp.shape
    imgs, masks = [], []
    for t in range(T):
        d = torch.from_numpy(_depth(disp[t])).to(DEV)
        r = torch.from_numpy(rgb[t]).to(DEV)
        if Kp is None:
            img, m = warp.render_depthcrafter_frame(r, d, cams[t], K, edge_filter=t >= from_)
        else:
            ii = torch.arange(H, device=DEV, dtype=torch.float32).view(H, 1)
            jj = torch.arange(W, device=DEV, dtype=torch.float32).view(1, W)
            pts = torch.stack(((jj - float(Kp[0, 2])) * d / float(Kp[0, 0]), (ii - float(Kp[1, 2])) * d / float(Kp[1, 1]), d), dim=-1).reshape(-1, 3)
            drop = warp.depth_edge_mask(d).reshape(-1) if t >= from_ else None
            img, m = warp.points_render(pts, r.reshape(-1, 3), cams[t], K, (H, W), morph=True, drop=drop)
        imgs.append(img)
        masks.append(m[..., 0])
    return torch.stack(imgs), torch.stack(masks)


def _batched(rgb, disp, cams, K, from_, Kp=None, **kw):
    from worldforge_amd import warp
    return warp.dc_warp_frames(torch.from_numpy(rgb).to(DEV), torch.from_numpy(disp).to(DEV), cams, K, edge_filter_from=from_, return_float=True,
                               K_points=Kp, **kw)


def _sobel_max(depth):
    d = depth.astype(np.float64)
    from scipy import ndimage
    return np.sqrt(ndimage.correlate(d, opr.SOBEL_X, mode="mirror") ** 2 + ndimage.correlate(d, opr.SOBEL_X.T, mode="mirror") ** 2).max()


@pytest.mark.parametrize("H,W,centred", [(35, 131, True), (131, 35, True), (35, 131, False), (131, 35, False), (288, 300, False),
                                          (17, 15430, True)])
def test_batched_equals_per_frame(H, W, centred):
    """Masks and float images (hence the owning point of every covered pixel) of ONE wf_dc_warp_frames call are bit-identical to the loop of
    per-frame calls: edge filter off on frame 0, on for frames 1 and 2, whose Sobel maxima differ by >= 10 x (a maximum that leaked into
    the neighbouring frame would move its threshold).  17 x 15430 x 3 frames exceeds every capped grid (2048 x 256 threads), the two
    filtered frames alone as well."""
    T = 3
    rgb, disp = _scene(T, H, W, seed=H)
    m1, m2 = _sobel_max(_depth(disp[1])), _sobel_max(_depth(disp[2]))
    assert m2 >= 10 * m1 > 0
    if H == 17:
        assert (T - 1) * H * W > 2048 * 256
    K = _K(H, W)
    Kp = _K(H, W, centred=True) if centred else None
    cams = [np.eye(4), np.eye(4), np.eye(4) if centred else _moved(0.01, 0.004)]
    if not centred:
        cams[1] = _moved(-0.006, 0.0)
    want_img, want_mask = _per_frame(rgb, disp, cams, K, 1, Kp)
    img8, mask, fimg = _batched(rgb, disp, cams, K, 1, Kp)
    assert torch.equal(mask, want_mask)
    assert torch.equal(fimg.view(torch.int32), want_img.view(torch.int32))
    np.testing.assert_array_equal(img8.cpu().numpy(), _quantise(fimg.cpu().numpy()))
    cover = mask.float().mean(dim=(1, 2)).cpu().numpy()
    if centred:  # frame 0 fully covered; the filtered frames lose the surroundings of their edges
        assert cover[0] == 1.0 and 0.1 < cover[1] < 1.0 and 0.1 < cover[2] < 1.0, cover
    elif min(H, W) >= 283:
        assert (cover > 0.5).all() and (cover[1:] < 1.0).all(), cover


@pytest.fixture(scope="module")
def recorder():
    import importlib.util
    spec = importlib.util.spec_from_file_location("record_pointrender_digests", os.path.join(os.path.dirname(GOLD), os.pardir, "tools",
                                                                                             "record_pointrender_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("kind", ["points", "edge", "batch"])
def test_entry_points_repeat_the_parent(kind, recorder):
    """Every output bit of wf_points_render, wf_depth_edge_mask and wf_dc_warp_frames on tests/pointrender_cases.py equals what the commit
    named in g30_pointrender_parent.json returned (sha256 of the bytes, recorded by tools/record_pointrender_digests.py from that commit's
    build: its per-frame entry points still had kernels of their own).  So that the recorded bits are not merely repeated but right: at
    radius 0.05 with dropped points the masks equal oracle.pointrender's on the live points and the images equal it on the pixels whose
    nearest point has a live exact copy (the smaller index wins); the default edge filter equals the oracle's exactly."""
    import json
    from worldforge_amd import warp
    with open(os.path.join(GOLD, "g30_pointrender_parent.json")) as f:
        want = {k: v for k, v in json.load(f)["digests"].items() if k.startswith({"points": "pts_", "edge": "edge_", "batch": "batch_"}[kind])}
    got = recorder.compute(DEV, kinds=(kind,))
    assert set(got) == set(want) and len(want) >= {"points": 25, "edge": 60, "batch": 5}[kind]
    moved = sorted(k for k in want if got[k] != want[k])
    assert not moved, moved
    if kind == "points":
        from tests.test_pointrender_cases_host import owners, tie_pixels
        for H, W in pc.POINT_SHAPES:
            c = pc.points(H, W)
            live = c["drop"] == 0
            ties, _ = tie_pixels(c, owners(c, live), live)
            assert ties.sum() >= 100
            for morph in (True, False):
                img, mask = recorder.render_points(c, dict(radius=0.05, morph=morph, use_drop=True), DEV)
                with np.errstate(all="ignore"):
                    wimg, wmask = opr.project_points_to_image(c["pts"][live], c["feats"][live], c["cam"], c["K"], (H, W), morph=morph, radius=0.05)
                np.testing.assert_array_equal(mask, wmask[..., 0])
                np.testing.assert_array_equal(img[ties], wimg[ties])
                assert morph or mask[ties].all()
    if kind == "edge":
        for H, W in ((40, 56), (57, 33)):
            depth = pc.edge_depths(H, W)
            for t in range(3):
                got_drop = warp.depth_edge_mask(torch.from_numpy(depth[t]).to(DEV)).cpu().numpy()
                np.testing.assert_array_equal(got_drop.astype(bool), opr.edge_filter_mask(depth[t]))


def _border_counts(diff):
    return [int(diff[0].sum()), int(diff[-1].sum()), int(diff[:, 0].sum()), int(diff[:, -1].sum())]


@pytest.mark.parametrize("H,W", [(40, 56), (57, 33)])
def test_separable_edge_filter_equals_the_oracle(H, W):
    """Identity cameras, centred points, no opening: the mask of a filtered frame is exactly the complement of its drop mask.  Compared
    exactly with oracle.pointrender.edge_filter_mask per frame; a border-blind variant (zero padding instead of reflect-101 / reflect)
    changes >= 8 pixels on each of the four borders, so the borders are under test."""
    from scipy import ndimage
    T = 3
    rgb, disp = _scene(T, H, W, seed=7 * H, steps=(0.3, 0.05, 0.45))
    want = np.stack([opr.edge_filter_mask(_depth(disp[t])) for t in range(T)])
    for t in range(T):
        d = _depth(disp[t]).astype(np.float64)
        mag = np.sqrt(ndimage.correlate(d, opr.SOBEL_X, mode="constant") ** 2 + ndimage.correlate(d, opr.SOBEL_X.T, mode="constant") ** 2)
        blind = ndimage.maximum_filter(((mag / mag.max()) > 0.1).astype(np.uint8), size=7, mode="constant").astype(bool)
        blind |= (ndimage.maximum_filter(_depth(disp[t]), size=5, mode="constant") - ndimage.minimum_filter(_depth(disp[t]), size=5, mode="constant")) > 0.3
        assert min(_border_counts(blind != want[t])) >= 8, _border_counts(blind != want[t])
        assert 0 < want[t].sum() < want[t].size
    _, mask, _ = _batched(rgb, disp, [np.eye(4)] * T, _K(H, W), 0, _K(H, W, centred=True), morph=False)
    np.testing.assert_array_equal(mask.cpu().numpy().astype(bool), ~want)


@pytest.mark.parametrize("H,W", [(40, 56), (57, 33)])
def test_separable_opening_equals_the_oracle(H, W):
    """Identity cameras, centred points, no filter: the raw coverage is the pattern of disparities whose depth is not behind the camera, so
    the 5 x 5 opening is tested on a designed mask with a 3-pixel strip along every border and slivers thinner than 5 pixels.  An opening that treats the
    outside as empty changes >= 8 pixels on each border."""
    from scipy import ndimage
    T = 2
    rng = np.random.default_rng(H)
    pattern = np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        p = (ndimage.uniform_filter(rng.random((H, W)), size=5) > 0.5 - 0.03 * t).astype(np.uint8)
        p[:8, 9:W - 9], p[H - 8:, 10:W - 10], p[9:H - 9, :8], p[10:H - 10, W - 8:] = 0, 0, 0, 0
        # strips 3 pixels thick along each border: kept only by an opening that ignores the outside
        p[:3, 9:W - 9], p[H - 3:, 10:W - 10], p[9:H - 9, :3], p[10:H - 10, W - 3:] = 1, 1, 1, 1
        p[H // 2, :] = 0
        p[:, W // 2 - 1:W // 2 + 1] = 0
        pattern[t] = p
    want = np.stack([opr.morph_open5(p) for p in pattern])
    for t in range(T):
        blind = ndimage.maximum_filter(ndimage.minimum_filter(pattern[t], size=5, mode="constant", cval=0), size=5, mode="constant", cval=0)
        assert min(_border_counts(blind != want[t])) >= 8, _border_counts(blind != want[t])
        assert (want[t] != pattern[t]).sum() >= 8
    rgb = rng.random((T, H, W, 3)).astype(F32)
    disp = np.where(pattern == 1, F32(0.4), F32(-1.0)).astype(F32)  # 1 / (-1 + 0.1) < 0: behind the camera, never splatted
    _, mask, fimg = _batched(rgb, disp, [np.eye(4)] * T, _K(H, W), T, _K(H, W, centred=True))
    np.testing.assert_array_equal(mask.cpu().numpy(), want)
    np.testing.assert_array_equal(fimg.cpu().numpy(), rgb * want[..., None])


def test_quantisation_is_round_half_even_then_saturate():
    """k / 255, (k + 0.5) / 255 on both parities of k, 0, 1 and values slightly above 1, against rint(float32(x) * float32(255)).clip(0, 255)."""
    k = np.arange(256, dtype=np.float64)
    vals = np.concatenate([k / 255, (k + 0.5) / 255, [0.0, 1.0, 1.0000001, 1.001, 1.0019, 1.002, 1.5, 1e-9, 0.0019, 0.00197]]).astype(F32)
    H = W = 16
    assert vals.size <= H * W * 3
    rgb = np.zeros((1, H, W, 3), dtype=F32)
    rgb.reshape(-1)[:vals.size] = vals
    prod = vals * F32(255)
    ties = prod[np.abs(prod - np.floor(prod) - 0.5) == 0]
    assert (np.floor(ties) % 2 == 0).sum() >= 20 and (np.floor(ties) % 2 == 1).sum() >= 20  # exact ties of the float32 product, both parities
    img8, mask, _ = _batched(rgb, np.full((1, H, W), 0.4, dtype=F32), [np.eye(4)], _K(H, W), 1, _K(H, W, centred=True), morph=False)
    assert bool(mask.all())
    want = np.rint(F32(rgb) * F32(255)).clip(0, 255).astype(np.uint8)
    np.testing.assert_array_equal(img8.cpu().numpy(), want)


RESIZE_CASES = [(60, 100, 48, 80), (40, 24, 80, 48), (7, 5, 3, 2), (48, 80, 48, 80)]


@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("h,w,H,W", RESIZE_CASES)
def test_resize_matches_torch_cpu(h, w, H, W, aa):
    """Against F.interpolate(mode="bilinear", align_corners=False, antialias=aa) on the CPU in float32.  Bars: dynwarp_cases.RESIZE_BARS,
    2 x the measured maximum absolute error per case; equal sizes must return the input bits; above 1e-5 the tap rule would be wrong."""
    from worldforge_amd import warp
    x = torch.from_numpy(np.random.default_rng(h * W).random((3, h, w, 3)).astype(F32))
    want = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False, antialias=aa).permute(0, 2, 3, 1)
    got = warp.resize_bilinear(x.to(DEV), (H, W), antialias=aa).cpu()
    assert got.shape == want.shape == (3, H, W, 3)
    err = float((got - want).abs().max())
    print(f"resize {h}x{w}->{H}x{W} antialias={aa}: max abs err {err:.3e}")
    if (h, w) == (H, W):
        assert torch.equal(got.view(torch.int32), x.view(torch.int32))
        return
    assert err <= 1e-5
    assert err <= dc.RESIZE_BARS[(h, w, H, W, aa)]


# Share of the pixels of a case whose 8-bit colour may differ (by one code) from the recorded frame where the resize is not the identity.
# Measured: 0 on scenes a and b (their masks are empty), 0.00021 on c_up_edge; the cap is 2 x that, far below the 1 % ceiling, and the
# recorder checks that the reference's own colours perturbed by the largest resize bar change fewer pixels than the ceiling.
COLOUR_SHARE_CAP = 0.00044


@pytest.fixture(scope="module")
def scenes():
    return {n: dc.scene(n) for n in dc.SCENES}


@pytest.mark.parametrize("case", list(dc.CASES))
def test_whole_route_equals_the_recorded_frames(case, scenes):
    """warp.warp_depthcrafter_frames on the recorded scenes: masks exact; native-size frames: 8-bit images exact; resized frames: colours
    within one code on at most COLOUR_SHARE_CAP of the pixels; the float image where recorded (ownership) within the resize bar."""
    from worldforge_amd import warp
    c, s = dc.CASES[case], scenes[dc.CASES[case]["scene"]]
    rec = np.load(os.path.join(GOLD, f"g29_dynwarp_{case}.npz"))
    imgs, masks, cams, fimg = warp.warp_depthcrafter_frames(s["frames_native" if c["native"] else "frames"], s["disparity"], device=DEV,
                                                            return_float=True, **dc.options(case))
    imgs, masks, fimg = imgs.cpu().numpy(), masks.cpu().numpy(), fimg.cpu().numpy()
    assert len(cams) == masks.shape[0]
    np.testing.assert_array_equal(masks, rec["masks"])
    if c["scene"] == "c":
        assert 0.3 < masks[1:].mean() < 1.0
    if c["native"]:
        np.testing.assert_array_equal(imgs, rec["images"])
    else:
        diff = np.abs(imgs.astype(np.int16) - rec["images"].astype(np.int16))
        share = float((diff > 0).any(-1).mean())
        print(f"{case}: colour pixels that differ {share:.5f}, max code difference {diff.max()}")
        assert diff.max() <= 1 and share <= COLOUR_SHARE_CAP
    if "float_images" in rec:
        assert np.abs(fimg - rec["float_images"]).max() <= (0.0 if c["native"] else dc.RESIZE_BAR_MAX)


def test_command_line_hands_over_to_the_frame_reader(tmp_path, scenes):
    """python -m worldforge_amd.warp_depthcrafter on a fixture folder -> OUT/warped/imgs, read back by harness.read_frames_from_directory (what
    both infer command lines read --video-ref with): counts and values equal what the call returned."""
    from PIL import Image
    from worldforge_amd import harness, warp, warp_depthcrafter as wd
    s, opt = scenes["c"], dc.options("c_native_left_edge")
    seq = tmp_path / "clip"
    seq.mkdir()
    for i, f in enumerate(s["frames_native"]):
        Image.fromarray(f, "RGB").save(seq / f"frame_{i:03d}.png")
    npz = tmp_path / "depth.npz"
    np.savez_compressed(npz, depth=s["disparity"])
    out = tmp_path / "out"
    assert wd.main(["--video_path", str(seq), "--depth_npz", str(npz), "--output_path", str(out), "--direction", opt["direction"], "--degree",
                    str(opt["degree"]), "--enable_edge_filter", "--device", DEV]) == 0
    imgs, masks, _ = warp.warp_depthcrafter_frames(s["frames_native"], s["disparity"], device=DEV, **opt)
    frames, fmasks, first = harness.read_frames_from_directory(str(out / "warped" / "imgs"))
    assert len(frames) == len(fmasks) == imgs.shape[0] and first is frames[0]
    np.testing.assert_array_equal(np.stack([np.array(f) for f in frames]), imgs.cpu().numpy())
    np.testing.assert_array_equal(np.stack([np.array(m) for m in fmasks]), masks.cpu().numpy() * 255)
    assert sorted(os.listdir(out / "warped" / "imgs")) == sorted([f"rendered_image_{i:02d}.png" for i in range(2)] + [f"mask_{i:02d}.png" for i in range(2)])


def test_three_calls_repeat_their_bits():
    outs = []
    for _ in range(3):
        per = []
        for H, W in ((35, 131), (131, 35), (288, 300)):
            rgb, disp = _scene(3, H, W, seed=H)
            per.append(_batched(rgb, disp, [np.eye(4), _moved(-0.006, 0.0), _moved(0.01, 0.004)], _K(H, W), 1))
        outs.append(per)
    for per in outs[1:]:
        for a, b in zip(outs[0], per):
            assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_refusals_and_chunking():
    from worldforge_amd import _ffi, warp
    lib = _ffi.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    for T, H, W, radius, dil, nr in ((0, 8, 8, 0.005, 3, 2), (1, 1, 8, 0.005, 3, 2), (1, 8, 1, 0.005, 3, 2), (1, 8, 0, 0.005, 3, 2),
                                     (1, 8, 8, 0.0, 3, 2), (1, 8, 8, 0.06, 3, 2), (1, 8, 8, 0.005, 16, 2), (1, 8, 8, 0.005, 3, 16)):
        assert lib.wf_dc_warp_frames(p, p, p, 525.0, 525.0, 4.0, 4.0, 0.1, dil, 0.3, nr, 1, radius, 1, T, H, W, p, p, None, p, None) != 0
    rgb, disp = _scene(3, 35, 131, seed=1)
    cams = [np.eye(4)] * 3
    one = _batched(rgb, disp, cams, _K(35, 131), 1, _K(35, 131, centred=True))
    per_frame_ws = int(lib.wf_dc_warp_frames_workspace_bytes(1, 35, 131))
    two = _batched(rgb, disp, cams, _K(35, 131), 1, _K(35, 131, centred=True), workspace_budget=per_frame_ws)  # one frame per call
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    with pytest.raises(ValueError, match="NaN"):
        bad = disp.copy()
        bad[0, 3, 3] = np.nan
        warp.warp_depthcrafter_frames(np.zeros((3, 35, 131, 3), np.uint8), bad, device=DEV)
