"""G29: stage 1 for dynamic scenes as the reference ships it -- DepthCrafter/warp_depthcrafter.py run_warping and the camera-sequence
functions of DepthCrafter/utils.py, both UNMODIFIED, on the CPU.  Usage:  python tools/make_dynamic_warp_golden.py REFERENCE_ROOT

Stand-in modules serve the imports the image lacks (their real behaviour stays unpinned, as oracle/pointrender.py says):
  cv2          imread through PIL (BGR, as cv2 returns it), cvtColor = channel swap, Sobel / dilate / morphologyEx = oracle/pointrender.py's
               restatements, imwrite captures the array it is given
  pytorch3d    Pointclouds, PointsRasterizationSettings, PointsRasterizer and the camera object of
               camera_conversions._cameras_from_opencv_projection, over oracle/pointrender.py's cameras_from_opencv / to_ndc / rasterize_nearest
  torchvision  transforms.functional.resize = F.interpolate(mode="bilinear", align_corners=False, antialias=True)
  diffusers, tqdm, depthcrafter.*   inert (export_to_video captures the float frames it is handed)
Written to tests/golden/:
  g29_dynwarp_meta.json      the parser's option table, the camera cases, per scene case its options and what the recorder checked
  g29_dynwarp_cameras.npz    one [frame_num, 4, 4] float64 array per camera case
  g29_dynwarp_<case>.npz     images u8 [T, H, W, 3] (the captured imwrite arrays as a PNG reader returns them: RGB, saturate(rint(x))),
                             masks u8 [T, H, W] (0 / 1), float_images f32 [T, H, W, 3] (before x 255; not for scene `c`: its size),
                             look_at (the float32 look-at depth)
The inputs are rebuilt from tests/dynwarp_cases.py, which also says why the two small scenes render as specks.  The recorder asserts that
the edge filter drops points in every filtered frame, that the opening removes pixels in every warped frame of the scene with real coverage
(`c`) and in at least one case of each small scene, and that perturbing the float colours by the largest resize bar of the tests
(tests/dynwarp_cases.py RESIZE_BAR_MAX) changes the 8-bit colour of fewer than 1 % of the pixels."""
import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pointrender as opr  # noqa: E402
from tests import dynwarp_cases as dc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
RESIZE_BAR_CEILING = dc.RESIZE_BAR_MAX


class Capture:
    def __init__(self):
        self.written, self.videos, self.dropped, self.opened = [], [], [], []


def install_stand_ins(cap: Capture):
    cv2 = types.ModuleType("cv2")
    cv2.CV_64F, cv2.MORPH_OPEN, cv2.MORPH_CLOSE, cv2.COLOR_BGR2RGB, cv2.COLOR_RGB2BGR, cv2.COLOR_BGR2GRAY = 6, 2, 3, 4, 4, 6
    cv2.imread = lambda path: np.ascontiguousarray(np.array(Image.open(path).convert("RGB"))[..., ::-1])
    cv2.cvtColor = lambda im, code: np.ascontiguousarray(im[..., ::-1])
    cv2.Sobel = lambda d, ddepth, dx, dy, ksize=3: ndimage.correlate(d.astype(np.float64), opr.SOBEL_X if dx else opr.SOBEL_X.T, mode="mirror")

    def dilate(mask, kernel, iterations=1):
        out = ndimage.maximum_filter(mask, size=kernel.shape[0], mode="constant", cval=0)
        cap.dropped.append(int(out.sum()))
        return out

    def morphology_ex(mask, op, kernel):
        assert op == cv2.MORPH_OPEN and kernel.shape == (5, 5)
        out = opr.morph_open5(mask)
        cap.opened.append(int(mask.sum()) - int(out.sum()))
        return out

    cv2.dilate, cv2.morphologyEx = dilate, morphology_ex
    cv2.imwrite = lambda path, im: cap.written.append((os.path.basename(path), np.array(im))) or True
    sys.modules["cv2"] = cv2

    class Pointclouds:
        def __init__(self, points, features):
            self.points, self.features = points[0], features[0]

    class OpenCVCameras:
        def __init__(self, R, tvec, camera_matrix, image_size):
            E = np.eye(4)
            E[:3, :3], E[:3, 3] = R[0].cpu().numpy(), tvec[0].cpu().numpy()
            hw = [int(v) for v in image_size[0]]
            self.params = opr.cameras_from_opencv(E, camera_matrix[0].cpu().numpy(), hw)

    class PointsRasterizationSettings:
        def __init__(self, image_size, radius, points_per_pixel):
            self.image_size, self.radius, self.points_per_pixel = image_size, radius, points_per_pixel

    class PointsRasterizer:
        def __init__(self, cameras, raster_settings):
            self.cameras, self.settings = cameras, raster_settings

        def __call__(self, cloud):
            x, y, z = opr.to_ndc(cloud.points.cpu().numpy(), *self.cameras.params)
            idx = opr.rasterize_nearest(x, y, z, self.settings.image_size, self.settings.radius)
            return types.SimpleNamespace(idx=torch.from_numpy(idx)[None, :, :, None])

    p3d, st, rd = types.ModuleType("pytorch3d"), types.ModuleType("pytorch3d.structures"), types.ModuleType("pytorch3d.renderer")
    p3d.__path__ = []
    st.Pointclouds = Pointclouds
    rd.PointsRasterizationSettings, rd.PointsRasterizer = PointsRasterizationSettings, PointsRasterizer
    rd.camera_conversions = types.SimpleNamespace(_cameras_from_opencv_projection=lambda R, tvec, camera_matrix, image_size: OpenCVCameras(
        R, tvec, camera_matrix, image_size))
    for n in ("PerspectiveCameras", "PointsRenderer", "AlphaCompositor", "NormWeightedCompositor", "look_at_view_transform",
              "FoVOrthographicCameras"):
        setattr(rd, n, None)
    sys.modules.update({"pytorch3d": p3d, "pytorch3d.structures": st, "pytorch3d.renderer": rd})

    tv, tvt, tvf = (types.ModuleType(n) for n in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"))
    tv.__path__, tvt.__path__ = [], []
    tvf.resize = lambda x, size: torch.nn.functional.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False, antialias=True)
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})

    inert = {"diffusers": (), "diffusers.training_utils": ("set_seed",), "diffusers.utils": (), "tqdm": (), "depthcrafter": (),
             "depthcrafter.depth_crafter_ppl": ("DepthCrafterPipeline",), "depthcrafter.unet": ("DiffusersUNetSpatioTemporalConditionModelDepthCrafter",),
             "depthcrafter.utils": ("read_video_frames",)}
    for name, attrs in inert.items():
        m = types.ModuleType(name)
        m.__path__ = []
        for a in attrs:
            setattr(m, a, None)
        sys.modules[name] = m
    sys.modules["tqdm"].tqdm = lambda it, **kw: it
    sys.modules["diffusers.utils"].export_to_video = lambda frames, path, fps=6: cap.videos.append([np.array(f) for f in frames])


def parser_table(WD):
    """main() builds its parser inside: take the table from the parser object as parse_args sees it, and stop there."""
    seen = {}
    orig = argparse.ArgumentParser.parse_args

    class Stop(Exception):
        pass

    def spy(self, *a, **k):
        seen["table"] = [dict(name=x.option_strings[0], dest=x.dest, default=x.default, choices=list(x.choices) if x.choices else None,
                              type=x.type.__name__ if x.type else None, required=bool(x.required), flag=x.nargs == 0)
                         for x in self._actions if x.option_strings and x.dest != "help"]
        raise Stop

    argparse.ArgumentParser.parse_args = spy
    try:
        WD.main()
    except Stop:
        pass
    finally:
        argparse.ArgumentParser.parse_args = orig
    return seen["table"]


def quantise(x255):
    """What a reader gets back from cv2.imwrite of a float32 image (restated: convertTo(CV_8U) = saturate(round half to even))."""
    return np.clip(np.rint(np.asarray(x255, dtype=np.float32)), 0, 255).astype(np.uint8)


def camera_cases(U):
    seqs = {("up", False): (U.get_look_up_camera_seq, 1), ("down", False): (U.get_look_up_camera_seq, -1),
            ("right", False): (U.get_look_right_camera_seq, 1), ("left", False): (U.get_look_right_camera_seq, -1),
            ("up", True): (U.get_stable_look_up_camera_seq, 1), ("down", True): (U.get_stable_look_up_camera_seq, -1),
            ("right", True): (U.get_stable_look_right_camera_seq, 1), ("left", True): (U.get_stable_look_right_camera_seq, -1)}
    look = np.float32(1.7320508)
    cases, arrays = [], {}
    for frame_num in (5, 1):
        for direction in ("up", "down", "left", "right"):
            for stable, stable_frame in ((False, 17), (True, 1), (True, 3), (True, 5), (True, 8)):
                if frame_num == 1 and stable_frame not in (17, 3):
                    continue
                for zoom in ("none", "zoom_in", "zoom_out"):
                    fn, sign = seqs[(direction, stable)]
                    degree, rate = 12.5, 0.7
                    if stable:
                        cams = fn(np.eye(4), sign * degree, frame_num, look, stable_frame)
                        if zoom != "none":
                            cams = U.apply_stable_zoom_to_camera_seq(cams, zoom, rate, look, stable_frame)
                    else:
                        cams = fn(np.eye(4), sign * degree, frame_num, look)
                        if zoom != "none":
                            cams = U.apply_zoom_to_camera_seq(cams, zoom, rate, look)
                    key = f"c{len(cases):03d}"
                    cases.append(dict(key=key, direction=direction, degree=degree, frame_num=frame_num, look_at_depth_value=float(look),
                                      zoom=zoom, rate=rate, stable=stable, stable_frame=stable_frame))
                    arrays[key] = np.stack(cams).astype(np.float64)
    return cases, arrays


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = os.path.join(sys.argv[1], "DepthCrafter")
    cap = Capture()
    install_stand_ins(cap)
    sys.path.insert(0, ref)
    import utils as U
    import warp_depthcrafter as WD
    argv = sys.argv
    sys.argv = ["warp_depthcrafter.py", "--video_path", "frames"]
    try:
        table = parser_table(WD)
    finally:
        sys.argv = argv
    cases, arrays = camera_cases(U)
    np.savez_compressed(os.path.join(OUT, "g29_dynwarp_cameras.npz"), **arrays)
    meta = dict(numpy=np.__version__, torch=torch.__version__, parser=table, cameras=cases, scenes=dc.SCENES, cases={},
                resize_bar_ceiling=RESIZE_BAR_CEILING)
    scenes = {n: dc.scene(n) for n in dc.SCENES}
    opened_in = {n: 0 for n in dc.SCENES}
    for cn, c in dc.CASES.items():
        s, opt = scenes[c["scene"]], dc.options(cn)
        frames = s["frames_native" if c["native"] else "frames"]
        T = frames.shape[0]
        rec = {}
        med = np.median
        np.median = lambda *a, **k: rec.setdefault("median", med(*a, **k))
        del cap.written[:], cap.videos[:], cap.dropped[:], cap.opened[:]
        with tempfile.TemporaryDirectory() as tmp:
            vid, dep = os.path.join(tmp, "seq"), os.path.join(tmp, "depth")
            os.makedirs(vid), os.makedirs(dep)
            for i, f in enumerate(frames):
                Image.fromarray(f, "RGB").save(os.path.join(vid, f"frame_{i:03d}.png"))
            np.savez_compressed(os.path.join(dep, "depth.npz"), depth=s["disparity"])
            try:
                WD.run_warping(video_path=vid, depth_folder=dep, output_path=os.path.join(tmp, "warped"), **opt)
            finally:
                np.median = med
        assert rec["median"].dtype == np.float32, rec["median"].dtype
        imgs = np.stack([quantise(a[..., ::-1]) for nme, a in cap.written if nme.startswith("rendered_image_")])
        masks = np.stack([(a[..., 0] // 255).astype(np.uint8) for nme, a in cap.written if nme.startswith("mask_")])
        fimgs = np.stack(cap.videos[0]).astype(np.float32)
        vmasks = np.stack(cap.videos[1])[..., 0].astype(np.uint8)
        assert imgs.shape == (T,) + s["disparity"].shape[1:] + (3,) and masks.shape == s["disparity"].shape and (masks == vmasks).all()
        assert set(np.unique(masks)) <= {0, 1} and (imgs == quantise(fimgs * np.float32(255))).all()
        assert len(cap.opened) == T
        opened_in[c["scene"]] += sum(cap.opened)
        if c["scene"] == "c":
            assert all(v > 0 for v in cap.opened[1:]) and 0.3 < masks[1:].mean() < 1.0, ("the opening must remove pixels", cap.opened)
        if opt["enable_edge_filter"]:
            assert len(cap.dropped) == T - 1 and all(v > 0 for v in cap.dropped), ("the edge filter must drop points", cap.dropped)
        else:
            assert not cap.dropped
        changed = 0
        for eps in (RESIZE_BAR_CEILING, -RESIZE_BAR_CEILING):
            q = quantise((fimgs + np.float32(eps)).astype(np.float32) * np.float32(255))
            changed = max(changed, int((q != imgs).any(-1)[masks == 1].sum()))
        share = changed / masks.size
        assert share < 0.01, share
        look = np.float32(rec["median"] * opt["look_at_depth"])
        keep = dict(images=imgs, masks=masks, look_at=look)
        if c["scene"] != "c":  # (at scene c's size the float images would outweigh every other fixture; its frames are native: u8 exact)
            keep["float_images"] = fimgs
        np.savez_compressed(os.path.join(OUT, f"g29_dynwarp_{cn}.npz"), **keep)
        meta["cases"][cn] = dict(scene=c["scene"], native=c["native"], options=opt, mask_mean=float(masks.mean()), opened=list(cap.opened),
                                 edge_dropped=list(cap.dropped), look_at_bits=int(look.view(np.uint32)),
                                 perturbed_colour_pixels=changed, perturbed_colour_share=share)
        print("g29", cn, "mask", round(float(masks.mean()), 3), "opened", cap.opened, "dropped", cap.dropped, "perturbed share", share)
    assert all(v > 0 for v in opened_in.values()), opened_in
    with open(os.path.join(OUT, "g29_dynwarp_meta.json"), "w", encoding="utf-8") as f:
        json.dump(meta, f, indent=1)
    print("g29 meta:", len(meta["cases"]), "scene cases,", len(cases), "camera cases")


if __name__ == "__main__":
    main()
