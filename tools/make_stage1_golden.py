"""G28: stage 1 as the reference ships it -- vggt/run_warp.py's parser and vggt/modules/utils_warp.py warp_single_img, both UNMODIFIED, with
the parser's defaults (outlier_min_neighbors 10, outlier_neighbor_radius 3, depth_segments 8, crack_min_neighbors 2, crack_max_size 6).
CPU only.  Usage:  python tools/make_stage1_golden.py REFERENCE_ROOT

`import cv2` is served by a stand-in whose filter2D / morphologyEx are oracle/crackfill.py's restatements (OpenCV is absent; its real
stencils stay unpinned) and whose imwrite only records the file name; the VGGT model modules run_warp.py imports at its top are empty
placeholders (no model runs here).  Written to tests/golden/:
  g28_stage1_meta.json           the parser's option table, create_default_crack_params(args), per case the threshold and the mean depth the
                                 reference computed (np.percentile / np.nanmean are wrapped to record them), its `infos`, the file names and
                                 camera_info.txt of save_warped_results for one case, and the reference's own sensitivity (below)
  g28_stage1_<scene>_inputs.npz  image, depth, conf, K, E of tests/stage1_cases.scene
  g28_stage1_<case>.npz          images u8 [5, H, W, 3], masks u8 [5, H, W] of warp_single_img(depth_conf given, fill_cracks=True)
Sensitivity: every case is run again with look_at_depth one fp32 ulp above and below 1, which moves the one quantity this engine rounds
differently (the mean depth: fp64 here, numpy's fp32 pairwise sum there) by about an ulp; the number of mask / colour pixels that change
between the REFERENCE's runs is recorded, and tests/test_gpu_stage1.py holds its caps to four times that."""
import argparse
import copy
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import crackfill as ocf  # noqa: E402
from tests import stage1_cases as sc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def install_stand_ins(written):
    cv2 = types.ModuleType("cv2")
    cv2.MORPH_CLOSE, cv2.COLOR_RGB2BGR, cv2.COLOR_GRAY2RGB, cv2.BORDER_REFLECT = 3, 4, 8, 2
    cv2.morphologyEx = lambda m, op, k: ocf.close3(m)
    cv2.filter2D = lambda im, dd, k, **kw: ocf.filter2d(im, k, "reflect" if kw.get("borderType") else "reflect101")
    cv2.cvtColor = lambda im, code: im
    cv2.imwrite = lambda path, im: written.append((os.path.basename(path), tuple(im.shape), str(im.dtype), int(im.max()))) or True
    sys.modules["cv2"] = cv2
    for name, attrs in (("vggt", ()), ("vggt.models", ()), ("vggt.models.vggt", ("VGGT",)), ("vggt.utils", ()),
                        ("vggt.utils.load_fn", ("load_and_preprocess_images",)), ("vggt.utils.pose_enc", ("pose_encoding_to_extri_intri",))):
        m = types.ModuleType(name)
        m.__path__ = []
        for a in attrs:
            setattr(m, a, None)
        sys.modules[name] = m


def parser_table(RW):
    """run_warp.parse_arguments builds its parser inside: take the table from the parser object as parse_args sees it."""
    seen = {}
    orig = argparse.ArgumentParser.parse_args

    def spy(self, *a, **k):
        seen["table"] = [dict(name=x.option_strings[0], dest=x.dest, default=x.default, choices=list(x.choices) if x.choices else None,
                              type=x.type.__name__ if x.type else None, required=bool(x.required))
                         for x in self._actions if x.option_strings and x.dest != "help"]
        return orig(self, *a, **k)

    argparse.ArgumentParser.parse_args = spy
    argv = sys.argv
    sys.argv = ["run_warp.py", "--image_path", "images"]
    try:
        args = RW.parse_arguments()
    finally:
        argparse.ArgumentParser.parse_args = orig
        sys.argv = argv
    return seen["table"], RW.validate_args(args)


def run(UW, args, s, thr, direction, degree, look_at_depth=None):
    """One unmodified warp_single_img call; -> (images, masks, infos, threshold, mean depth) with the last two as the reference computed them."""
    a = copy.copy(args)
    if look_at_depth is not None:
        a.look_at_depth = look_at_depth
    rec = {}
    pct, nmean = np.percentile, np.nanmean
    np.percentile = lambda *x, **k: rec.setdefault("threshold", pct(*x, **k))
    np.nanmean = lambda *x, **k: rec.setdefault("mean", nmean(*x, **k))
    try:
        imgs, masks, infos = UW.warp_single_img(s["E"], s["K"], torch.from_numpy(s["image"]).permute(2, 0, 1), s["depth"].copy(),
                                                depth_conf=s["conf"].copy(), direction=direction, degree=degree, conf_threshold=thr,
                                                frame_num=sc.FRAME_NUM, use_backward=False, fill_cracks=a.fill_cracks,
                                                crack_params=UW.create_default_crack_params(a), args=a)
    finally:
        np.percentile, np.nanmean = pct, nmean
    return np.stack(imgs), np.stack([m.astype(np.uint8) for m in masks]), infos, rec.get("threshold"), rec["mean"]


def bits(x):
    return None if x is None else int(np.float32(x).view(np.uint32))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    written = []
    install_stand_ins(written)
    sys.path.insert(0, os.path.join(ref, "vggt"))
    from modules import utils_warp as UW
    import run_warp as RW
    table, args = parser_table(RW)
    meta = dict(numpy=np.__version__, parser=table, crack_params=UW.create_default_crack_params(args), frame_num=sc.FRAME_NUM,
                fixed=dict(fill_cracks=args.fill_cracks, disable_depth_aware_fill=args.disable_depth_aware_fill,
                           skip_outlier_detection=args.skip_outlier_detection, use_fast_outlier_detection=args.use_fast_outlier_detection),
                cases={}, sensitivity={})
    up, down = float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(1), np.float32(0)))
    for name in sc.SCENES:
        image, depth, conf, K, E = sc.scene(name)
        s = dict(image=image, depth=depth, conf=conf, K=K, E=E)
        np.savez_compressed(os.path.join(OUT, f"g28_stage1_{name}_inputs.npz"), **s)
        for thr, direction, degree in sc.CASES:
            cn = sc.case_name(name, thr, direction)
            imgs, masks, infos, t, mean = run(UW, args, s, thr, direction, degree)
            assert mean.dtype == np.float32 and (t is None or t.dtype == np.float32), (mean.dtype, None if t is None else t.dtype)
            np.savez_compressed(os.path.join(OUT, f"g28_stage1_{cn}.npz"), images=imgs, masks=masks)
            meta["cases"][cn] = dict(threshold_bits=bits(t), mean_depth_bits=bits(mean), infos=infos, mask_mean=float(masks[1:].mean()))
            dm = dc = 0
            for lad in (up, down):
                i2, m2, _, _, _ = run(UW, args, s, thr, direction, degree, lad)
                dm = max(dm, int((m2 != masks).sum()))
                dc = max(dc, int(((i2 != imgs).any(-1) & (m2 == masks)).sum()))
            meta["sensitivity"][cn] = dict(pixels=int(masks.size), mask_changed=dm, colour_changed=dc)
            print("g28", cn, "threshold", t, "mean", mean, "mask", round(float(masks[1:].mean()), 3), "one-ulp rerun:", dm, "mask /", dc,
                  "colour pixels of", masks.size)
    # save_warped_results: the file names and camera_info.txt of one case
    name, (thr, direction, degree) = "s48", sc.CASES[0]
    image, depth, conf, K, E = sc.scene(name)
    a = copy.copy(args)
    a.direction, a.degree, a.frame_single, a.conf_single = direction, degree, sc.FRAME_NUM, thr
    imgs, masks, infos, _, _ = run(UW, a, dict(image=image, depth=depth, conf=conf, K=K, E=E), thr, direction, degree)
    del written[:]
    with tempfile.TemporaryDirectory() as tmp:
        RW.save_warped_results(list(imgs), list(masks), infos, tmp, 2, a)
        with open(os.path.join(tmp, "camera_info.txt"), encoding="utf-8") as f:
            info_txt = f.read()
    meta["save"] = dict(case=sc.case_name(name, thr, direction), camera_idx=2, files=[list(w) for w in written], camera_info=info_txt)
    with open(os.path.join(OUT, "g28_stage1_meta.json"), "w", encoding="utf-8") as f:
        json.dump(meta, f, indent=1, ensure_ascii=False)
    print("g28 meta:", len(meta["cases"]), "cases; crack_params", meta["crack_params"])


if __name__ == "__main__":
    main()
