"""Stage-1 depth-guided forward warping on the GPU (vggt/modules/utils_warp.py warp_single_img :724-1001).

`forward_splat` (:863-945) and `crack_fill` / `crack_fill_ex` (:954-985 -> :386-706) are the tensor-sized parts of the stage-1 warper: one
image + depth map -> n warped views with validity masks (the `warp_*` / `mask_*` frames the guided sampler consumes), cracks closed.  The
camera paths (:64-383) are 4x4 host math (`camera_path`); the confidence filter (:774-808) is `depth_conf_filter` (np.percentile's
threshold from an exact select on the device, the mean in fp64); `warp_single_img` joins them as the reference does, and
`python -m worldforge_amd.run_warp` is its command line.

Dynamic scenes (DepthCrafter/warp_depthcrafter.py run_warping :140-301: every frame of a clip warped to its own camera) are at the end of
the file: the camera sequences, `warp_depthcrafter_frames` and the batched `dc_warp_frames`; `python -m worldforge_amd.warp_depthcrafter`
is their command line.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._ffi import call


def forward_splat(image: torch.Tensor, depth: torch.Tensor, intrinsic, extrinsic, cameras, device="cuda:0"):
    """image [H,W,3] float in [0,1]; depth [H,W] float (NaN / <= 0 = invalid); intrinsic 3x3; extrinsic 4x4 or 3x4 (world -> source
    camera); cameras: sequence of 4x4 (world -> new camera).  Returns (images u8 [n,H,W,3], masks u8 [n,H,W], depths f32 [n,H,W]) on the
    device."""
    dev = torch.device(device)
    img = torch.as_tensor(image, dtype=torch.float32).to(dev).contiguous()
    dep = torch.as_tensor(depth, dtype=torch.float32).to(dev).contiguous()
    H, W, C = img.shape
    if C != 3 or tuple(dep.shape) != (H, W):
        raise ValueError("image must be [H, W, 3] and depth [H, W]")
    K = np.asarray(intrinsic, dtype=np.float64)
    E = np.eye(4)
    ext = np.asarray(extrinsic, dtype=np.float64)
    E[:ext.shape[0], :] = ext
    R, t = E[:3, :3], E[:3, 3]
    geom = np.concatenate([np.linalg.inv(K).ravel(), K.ravel(), R.T.ravel(), (-R.T @ t).ravel()])
    cams = np.stack([np.asarray(c, dtype=np.float64)[:3, :4].ravel() for c in cameras])
    n = cams.shape[0]
    geom_d = torch.from_numpy(geom).to(dev)
    cams_d = torch.from_numpy(cams).contiguous().to(dev)
    out_img = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    out_mask = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    out_depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    zbuf = torch.empty((3 * n * H * W + 1) // 2, dtype=torch.int64, device=dev)  # 12 bytes per target: 64-bit depth key + 32-bit owner
    call("wf_warp_splat", img.data_ptr(), dep.data_ptr(), geom_d.data_ptr(), cams_d.data_ptr(), out_img.data_ptr(), out_mask.data_ptr(),
         out_depth.data_ptr(), zbuf.data_ptr(), n, H, W, ops.stream())
    return out_img, out_mask, out_depth


# ---- camera paths (vggt/modules/utils_warp.py:64-383 + the dispatch of warp_single_img :818-839): 4x4 host math, float64 ------------
def _rot(axis: str, rad: float) -> np.ndarray:
    c, s = np.cos(rad), np.sin(rad)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _look_at(R0: np.ndarray, cam_pos: np.ndarray, target: np.ndarray, guarded: bool):
    """Camera at cam_pos looking at target, up vector = the source camera's y axis made orthogonal to the view direction."""
    z = target - cam_pos
    n = np.linalg.norm(z)
    if guarded and not n > 1e-6:
        return None
    z = z / n
    y0 = R0.T @ np.array([0, 1, 0])
    y = y0 - np.dot(y0, z) * z
    yn = np.linalg.norm(y)
    if guarded and not yn > 1e-6:
        y = np.array([0, 1, 0]) if abs(z[1]) < 0.9 else np.array([1, 0, 0])
        y = y - np.dot(y, z) * z
        yn = np.linalg.norm(y)
    y = y / yn
    x = np.cross(y, z)
    x = x / np.linalg.norm(x)
    return np.column_stack([x, y, z]).T


def camera_path(direction: str, extrinsic, degree: float, frame_num: int, look_at_depth: float):
    """The reference's camera sequences: `up` / `down` / `left` / `right` orbit the point `look_at_depth` in front of the camera by up
    to +-degree about the x / y axis and re-aim at it; `forward` / `backward` dolly along the view direction by degree % of that depth;
    `*_pan` rotate in place.  Returns frame_num 4x4 world -> camera matrices, the first being the source camera."""
    E = np.eye(4)
    ext = np.asarray(extrinsic, dtype=np.float64)
    E[:ext.shape[0], :] = ext
    R, t = E[:3, :3], E[:3, 3]
    cam_pos = -R.T @ t
    d = direction.lower()
    out = []
    if d in ("up", "down", "left", "right"):
        axis = "x" if d in ("up", "down") else "y"
        sign = 1.0 if d in ("up", "right") else -1.0
        look_at = cam_pos + R.T @ np.array([0, 0, look_at_depth])
        for deg in np.linspace(0, sign * degree, frame_num):
            new_pos = look_at - _rot(axis, np.deg2rad(deg)) @ (look_at - cam_pos)
            nR = _look_at(R, new_pos, look_at, guarded=False)
            out.append((nR, new_pos))
    elif d in ("forward", "backward"):
        centre = cam_pos + R.T @ np.array([0, 0, look_at_depth])
        to_c = centre - cam_pos
        radius = np.linalg.norm(to_c)
        step = (to_c / radius) if d == "forward" else (-to_c / radius)
        for prog in np.linspace(0, degree / 100.0, frame_num):
            new_pos = cam_pos + step * (radius * prog)
            nR = _look_at(R, new_pos, centre, guarded=True)
            out.append((R.copy() if nR is None else nR, new_pos))
    elif d in ("up_pan", "down_pan", "left_pan", "right_pan"):
        axis = "x" if d in ("up_pan", "down_pan") else "y"
        sign = 1.0 if d in ("up_pan", "right_pan") else -1.0
        for deg in np.linspace(0, degree, frame_num):
            out.append((R @ _rot(axis, np.deg2rad(sign * deg)), cam_pos))
    else:
        raise ValueError(f"Unsupported direction: {direction}")
    cams = []
    for nR, pos in out:
        c = E.copy()
        c[:3, :3] = nR
        c[:3, 3] = -nR @ pos
        cams.append(c)
    return cams


def crack_fill(images: torch.Tensor, masks: torch.Tensor, depths: torch.Tensor, min_neighbors: int = 4, min_valid_neighbors: int = 3,
               num_segments: int = 5, original_depth: torch.Tensor = None, has_depth_conf: bool = False, depth_threshold: float = 0.1,
               max_crack_size: int = 5):
    """Crack filling of splatted views as warp_single_img applies it per view (utils_warp.py:954-985): images u8 [n,H,W,3], masks u8
    [n,H,W], depths f32 [n,H,W] (NaN = empty), as forward_splat returns them -> the same three, filled.  Views with more than 100 splatted
    depths take depth_aware_crack_filling (:647-691); the others fill_small_cracks (:386-455, `small_crack_fill` below) with the SOURCE
    view's filtered depth map `original_depth` [H,W] and `has_depth_conf` (whether the caller has a confidence map: only its presence
    matters, :433) -- their depth is returned unchanged, as in the reference.  Defaults = create_default_crack_params(None) (:694-704);
    run_warp.py passes min_valid_neighbors = 2, max_crack_size = 6 (:50-59, 294)."""
    n, H, W, _ = images.shape
    assert images.dtype == torch.uint8 and masks.dtype == torch.uint8 and depths.dtype == torch.float32
    images, masks, depths = images.contiguous(), masks.contiguous(), depths.contiguous()
    from ._ffi import lib
    ws = torch.empty(int(lib().wf_crack_fill_workspace_bytes(n, H, W)), dtype=torch.uint8, device=images.device)
    oi, om, od = torch.empty_like(images), torch.empty_like(masks), torch.empty_like(depths)
    call("wf_crack_fill", images.data_ptr(), masks.data_ptr(), depths.data_ptr(), oi.data_ptr(), om.data_ptr(), od.data_ptr(), n, H, W,
         int(min_neighbors), int(min_valid_neighbors), int(num_segments), ws.data_ptr(), ops.stream())
    return _route_sparse_views(images, masks, depths, oi, om, od, original_depth, has_depth_conf, depth_threshold, max_crack_size,
                               min_valid_neighbors)


def _route_sparse_views(images, masks, depths, oi, om, od, original_depth, has_depth_conf, depth_threshold, max_crack_size,
                        min_valid_neighbors):
    """Views with <= 100 splatted depths take fill_small_cracks instead (utils_warp.py:957-962, 973-981), their depth unchanged."""
    few = (~torch.isnan(depths)).flatten(1).sum(1) <= 100
    if bool(few.any()):  # once per camera path, outside any loop
        for i in torch.nonzero(few).flatten().tolist():
            oi[i], om[i] = small_crack_fill(images[i], masks[i], original_depth, has_depth_conf, depth_threshold, max_crack_size,
                                            min_valid_neighbors)
            od[i] = depths[i]
    return oi, om, od


def crack_fill_ex(images: torch.Tensor, masks: torch.Tensor, depths: torch.Tensor, min_neighbors: int = 4, neighbor_radius: int = 1,
                  min_valid_neighbors: int = 3, num_segments: int = 5, original_depth: torch.Tensor = None, has_depth_conf: bool = False,
                  depth_threshold: float = 0.1, max_crack_size: int = 5):
    """`crack_fill` with the outlier window radius (1..4) and the number of depth segments (1..16) as parameters (wf_crack_fill_ex): what
    run_warp.py ships is min_neighbors 10 in a 7 x 7 window (radius 3) over 8 segments.  At (radius 1, <= 5 segments) it returns
    `crack_fill`'s bits."""
    n, H, W, _ = images.shape
    assert images.dtype == torch.uint8 and masks.dtype == torch.uint8 and depths.dtype == torch.float32
    images, masks, depths = images.contiguous(), masks.contiguous(), depths.contiguous()
    from ._ffi import lib
    ws = torch.empty(int(lib().wf_crack_fill_ex_workspace_bytes(n, H, W)), dtype=torch.uint8, device=images.device)
    oi, om, od = torch.empty_like(images), torch.empty_like(masks), torch.empty_like(depths)
    call("wf_crack_fill_ex", images.data_ptr(), masks.data_ptr(), depths.data_ptr(), oi.data_ptr(), om.data_ptr(), od.data_ptr(), n, H, W,
         int(min_neighbors), int(min_valid_neighbors), int(num_segments), int(neighbor_radius), ws.data_ptr(), ops.stream())
    return _route_sparse_views(images, masks, depths, oi, om, od, original_depth, has_depth_conf, depth_threshold, max_crack_size,
                               min_valid_neighbors)


# ---- the confidence filter of warp_single_img (utils_warp.py:774-808) -----------------------------------------------------------------------
def percentile_plan(n: int, q: float):
    """Where np.percentile(a, q) (method "linear") looks in the sorted float32 array of n values: (k, gamma) with the result
    lerp(sorted[k], sorted[min(k + 1, n - 1)], gamma).  numpy divides q by 100 IN THE ARRAY'S DTYPE and multiplies by n - 1 there, so
    the virtual index and gamma are float32 (numpy/lib/_function_base_impl.py: percentile, _quantile, _get_indexes, _get_gamma)."""
    q32 = np.float32(q) / np.float32(100)
    if not (0.0 <= q32 <= 1.0):
        raise ValueError("Percentiles must be in the range [0, 100]")
    v = np.float32(n - 1) * q32
    if v >= n - 1:  # numpy indexes the last element as -1 and takes gamma = v - (-1): both neighbours are the maximum
        return n - 1, np.float32(np.float64(v) + 1.0)
    return int(np.floor(v)), np.float32(v - np.floor(v))


def lerp_f32(a, b, gamma) -> np.float32:
    """numpy's _lerp on float32 scalars: a + (b - a) gamma, replaced by b - (b - a) (1 - gamma) where gamma >= 0.5."""
    a, b, g = np.float32(a), np.float32(b), np.float32(gamma)
    with np.errstate(invalid="ignore"):  # inf - inf, inf * 0: NaN, as in numpy
        d = np.float32(b - a)
        return np.float32(b - d * np.float32(np.float32(1) - g)) if g >= 0.5 else np.float32(a + d * g)


def select_pair(x: torch.Tensor, k: int):
    """wf_select_pair_f32: the k-th and min(k + 1, n - 1)-th smallest of the fp32 device tensor x (exact; a NaN sorts last) and the number
    of NaNs -> (lo, hi, nan_count) as np.float32, np.float32, int.  One host synchronisation (12 bytes)."""
    from ._ffi import lib
    x = x.to(torch.float32).contiguous().flatten()
    ws = torch.empty(int(lib().wf_select_pair_f32_workspace_bytes()), dtype=torch.uint8, device=x.device)
    out = torch.empty(3, dtype=torch.float32, device=x.device)
    call("wf_select_pair_f32", x.data_ptr(), x.numel(), int(k), out.data_ptr(), ws.data_ptr(), ops.stream())
    h = out.cpu().numpy()
    return h[0], h[1], int(h[2:3].view(np.uint32)[0])


def percentile_f32(x: torch.Tensor, q: float) -> np.float32:
    """np.percentile(x.flatten(), q) of an fp32 device tensor, bit for bit as an fp32 value; a NaN in x is a ValueError (numpy would return
    NaN, and a NaN threshold keeps no pixel)."""
    k, gamma = percentile_plan(x.numel(), q)
    lo, hi, nans = select_pair(x, k)
    if nans:
        raise ValueError(f"percentile_f32: {nans} NaN value(s) in the input (numpy's percentile would be NaN)")
    return lerp_f32(lo, hi, gamma)


def depth_conf_filter(depth: torch.Tensor, depth_conf: torch.Tensor = None, conf_threshold: float = 0.5, threshold=None):
    """The filter of utils_warp.py:774-808 on the device: depth f32 [H, W], depth_conf f32 [H, W] or None -> (filtered depth f32 [H, W] on
    the device, threshold (np.float32 or None), mean depth (float: a fixed-order fp64 mean), count).  With a confidence map and
    conf_threshold != 1.0 the threshold is np.percentile(conf, (1 - conf_threshold) * 100) (or `threshold`, if given), the kept pixels
    are conf > threshold and the mean runs over their non-NaN depths; with conf_threshold == 1.0 the map passes through and without a map
    the invalid depths become NaN -- the mean then runs over the depths that are not NaN and > 0.  Two host synchronisations: the
    selected pair and the (mean, count) pair."""
    from ._ffi import lib
    depth = depth.to(torch.float32).contiguous()
    thr, mode, conf = None, 2, None
    if depth_conf is not None:
        conf = depth_conf.to(device=depth.device, dtype=torch.float32).contiguous()
        if tuple(conf.shape) != tuple(depth.shape):
            raise ValueError(f"depth_conf {tuple(conf.shape)} does not match depth {tuple(depth.shape)}")
        mode = 1
        if conf_threshold != 1.0:
            thr = np.float32(threshold) if threshold is not None else percentile_f32(conf, (1 - conf_threshold) * 100)
            mode = 0
    out = torch.empty_like(depth)
    stats = torch.empty(2, dtype=torch.float64, device=depth.device)
    ws = torch.empty(int(lib().wf_depth_conf_filter_workspace_bytes()), dtype=torch.uint8, device=depth.device)
    call("wf_depth_conf_filter", depth.data_ptr(), conf.data_ptr() if mode == 0 else None, float(thr) if thr is not None else 0.0, mode,
         out.data_ptr(), stats.data_ptr(), depth.numel(), ws.data_ptr(), ops.stream())
    mean, count = stats.cpu().tolist()
    return out, thr, mean, int(count)


# ---- warp_single_img (utils_warp.py:724-1001) and the parameters run_warp.py hands it --------------------------------------------------------
RUN_WARP_DEFAULTS = dict(depth_threshold=0.1, max_crack_size=6, min_valid_neighbors=2, min_neighbors=10, neighbor_radius=3,
                         skip_outlier_detection=False, use_fast_outlier_detection=True)  # create_default_crack_params(run_warp.py's parser)


def crack_params_from_args(args=None) -> dict:
    """create_default_crack_params (utils_warp.py:707-717), line for line."""
    return {
        "depth_threshold": getattr(args, "crack_depth_threshold", 0.1) if args is not None else 0.1,
        "max_crack_size": getattr(args, "crack_max_size", 5) if args is not None else 5,
        "min_valid_neighbors": getattr(args, "crack_min_neighbors", 3) if args is not None else 3,
        "min_neighbors": getattr(args, "outlier_min_neighbors", 4) if args is not None else 4,
        "neighbor_radius": getattr(args, "outlier_neighbor_radius", 1) if args is not None else 1,
        "skip_outlier_detection": getattr(args, "skip_outlier_detection", False) if args is not None else False,
        "use_fast_outlier_detection": getattr(args, "use_fast_outlier_detection", True) if args is not None else True,
    }


def frame_infos(direction: str, degree: float, frame_num: int):
    """The reference's list of dicts (utils_warp.py:851-856, 991-997).  `angle` is its LABEL degree (i + 1) / frame_num, not the angle of
    the camera (that is degree i / (frame_num - 1)): the file names are built from it."""
    out = [{"type": "original", "camera_name": "original", "direction": direction, "angle": 0.0}]
    for i in range(1, frame_num):
        angle = degree * (i + 1) / frame_num
        out.append({"type": "single_view_warped", "direction": direction, "angle": angle, "camera_name": f"{direction}_{angle:.2f}_deg"})
    return out


def warp_single_img(extrinsic, intrinsic, image, depth_map, depth_conf=None, direction="right", degree=15.0, conf_threshold=0.5,
                    frame_num=24, fill_cracks=True, crack_params=None, look_at_depth=1.0, depth_segments=5, device="cuda:0",
                    use_backward=False, disable_depth_aware_fill=False):
    """The reference's warp_single_img on the device.  extrinsic 3x4 / 4x4, intrinsic 3x3 (host); image [3, H, W] (or [1, 3, H, W]) tensor
    or [H, W, 3] array, float in [0, 1]; depth_map, depth_conf [H, W] (singleton axes are squeezed), host or device.  look_at_depth and
    depth_segments are the two fields the reference reads from its `args`; crack_params is laid over crack_params_from_args(None).
    -> (images u8 [frame_num, H, W, 3], masks u8 [frame_num, H, W]) on the device and the reference's list of dicts.  Frame 0 is the
    source image with a mask of ones.
    ValueError: a NaN in the confidence map; no pixel left by the filter (the reference goes on with a NaN camera); an image above 1.0
    (the reference then casts instead of scaling); use_backward, disable_depth_aware_fill, crack_params' skip_outlier_detection or
    use_fast_outlier_detection=False (run_warp.py's validate_args fixes all four); a radius or segment count wf_crack_fill_ex refuses."""
    if use_backward or disable_depth_aware_fill:
        raise ValueError("warp_single_img: use_backward / disable_depth_aware_fill are not implemented (run_warp.py fixes both to False)")
    params = crack_params_from_args(None)
    params.update(crack_params or {})
    if params.get("skip_outlier_detection", False) or not params.get("use_fast_outlier_detection", True):
        raise ValueError("warp_single_img: skip_outlier_detection and the scipy remove_outliers route (use_fast_outlier_detection=False) "
                         "are not implemented (run_warp.py fixes them to False / True)")
    radius, nseg = int(params["neighbor_radius"]), int(depth_segments)
    if fill_cracks and not (1 <= radius <= 4 and 1 <= nseg <= 16):
        raise ValueError(f"warp_single_img: neighbor_radius {radius} must be 1..4 and depth_segments {nseg} 1..16")
    dev = torch.device(device)
    img = torch.as_tensor(image, dtype=torch.float32)
    if img.dim() == 4:
        img = img[0]
    if img.dim() != 3:
        raise ValueError(f"image must be [3, H, W] or [H, W, 3], got {tuple(img.shape)}")
    if isinstance(image, torch.Tensor):
        img = img.permute(1, 2, 0)
    if img.shape[2] != 3:
        raise ValueError(f"image must have 3 channels, got {tuple(img.shape)}")
    if img.device.type == "cpu" and float(img.max()) > 1.0:  # (a device image is taken at its word: no synchronisation for this)
        raise ValueError("warp_single_img: the image must be in [0, 1]")
    img = img.to(dev).contiguous()
    H, W, _ = img.shape
    depth = torch.as_tensor(depth_map, dtype=torch.float32).to(dev).squeeze()
    conf = torch.as_tensor(depth_conf, dtype=torch.float32).to(dev).squeeze() if depth_conf is not None else None
    if tuple(depth.shape) != (H, W):
        raise ValueError(f"depth_map {tuple(depth.shape)} does not match the image {(H, W)}")
    filtered, _, mean, count = depth_conf_filter(depth, conf, conf_threshold)
    if count == 0:
        raise ValueError("warp_single_img: no pixel survives the depth / confidence filter")
    adjusted = float(np.float32(np.float32(mean) * np.float32(look_at_depth)))  # fp32 as the reference's np.float32 * float
    cams = camera_path(direction, extrinsic, degree, frame_num, adjusted)
    images = torch.empty((frame_num, H, W, 3), dtype=torch.uint8, device=dev)
    masks = torch.ones((frame_num, H, W), dtype=torch.uint8, device=dev)
    images[0] = (img * 255).to(torch.uint8)
    if frame_num > 1:
        wi, wm, wd = forward_splat(img, filtered, intrinsic, extrinsic, cams[1:], device=dev)
        if fill_cracks:
            wi, wm, _ = crack_fill_ex(wi, wm, wd, min_neighbors=params["min_neighbors"], neighbor_radius=radius,
                                      min_valid_neighbors=params["min_valid_neighbors"], num_segments=nseg, original_depth=filtered,
                                      has_depth_conf=conf is not None, depth_threshold=params["depth_threshold"],
                                      max_crack_size=params["max_crack_size"])
        images[1:], masks[1:] = wi, wm
    return images, masks, frame_infos(direction, degree, frame_num)


def small_crack_fill(image: torch.Tensor, mask: torch.Tensor, original_depth: torch.Tensor = None, has_depth_conf: bool = False,
                     depth_threshold: float = 0.1, max_crack_size: int = 5, min_valid_neighbors: int = 3):
    """fill_small_cracks (utils_warp.py:386-455) of ONE view: image u8 [H,W,3], mask u8 [H,W]; original_depth f32 [H,W] (the source view's
    filtered depth) is read by the depth-guided second step, which runs only when a confidence map exists (has_depth_conf)."""
    from ._ffi import lib
    H, W, _ = image.shape
    if has_depth_conf and original_depth is None:
        raise ValueError("small_crack_fill: has_depth_conf needs original_depth (the source view's filtered depth map)")
    image, mask = image.contiguous(), mask.contiguous()
    od = original_depth.to(torch.float32).contiguous() if original_depth is not None else None
    ws = torch.empty(int(lib().wf_fill_small_cracks_workspace_bytes(H, W)), dtype=torch.uint8, device=image.device)
    oi, om = torch.empty_like(image), torch.empty_like(mask)
    call("wf_fill_small_cracks", image.data_ptr(), mask.data_ptr(), od.data_ptr() if od is not None else None, 1 if has_depth_conf else 0,
         oi.data_ptr(), om.data_ptr(), H, W, float(depth_threshold), int(max_crack_size), int(min_valid_neighbors), ws.data_ptr(), ops.stream())
    return oi, om


# ---- dynamic scenes: the DepthCrafter warper's per-frame point-cloud render (DepthCrafter/warp_depthcrafter.py:255-288) ------------------
# (depth_edge_mask and points_render run the kernels of dc_warp_frames, further down, on one frame's stored depth plane / point array)
def pytorch3d_camera(extrinsic, K, size_hw) -> np.ndarray:
    """The 16 floats wf_points_render takes: pytorch3d's view of the reference's (extrinsic, K, image size), i.e. what
    pytorch3d.utils.camera_conversions._cameras_from_opencv_projection builds at DepthCrafter/utils.py:119-124 -- R' = R^T with its first two
    columns negated, T' = (-tx, -ty, tz), focal / s, -(principal - (W, H) / 2) / s with s = min(W, H) / 2, all float32."""
    H, W = int(size_hw[0]), int(size_hw[1])
    E = np.asarray(extrinsic, dtype=np.float64)
    R, t = E[:3, :3].astype(np.float32), E[:3, 3].astype(np.float32)
    Kf = np.asarray(K, dtype=np.float32)
    s = np.float32(min(W, H)) / np.float32(2.0)
    Rp = R.T.copy()
    Rp[:, :2] *= np.float32(-1)
    Tp = t.copy()
    Tp[:2] *= np.float32(-1)
    focal = np.array([Kf[0, 0], Kf[1, 1]], dtype=np.float32) / s
    p0 = -(np.array([Kf[0, 2], Kf[1, 2]], dtype=np.float32) - np.array([W, H], dtype=np.float32) / np.float32(2.0)) / s
    return np.concatenate([Rp.reshape(-1), Tp, focal, p0]).astype(np.float32)


def depth_edge_mask(depth: torch.Tensor, edge_threshold: float = 0.1, edge_dilation: int = 3, depth_jump_threshold: float = 0.3,
                    neighbor_check_radius: int = 2) -> torch.Tensor:
    """filter_edge_points (DepthCrafter/utils.py:523-567): depth f32 [H, W] (device) -> u8 [H, W], 1 = the pixel's point is dropped."""
    from ._ffi import lib
    H, W = depth.shape
    depth = depth.to(torch.float32).contiguous()
    ws = torch.empty(int(lib().wf_depth_edge_mask_workspace_bytes(H, W)), dtype=torch.uint8, device=depth.device)
    out = torch.empty((H, W), dtype=torch.uint8, device=depth.device)
    call("wf_depth_edge_mask", depth.data_ptr(), H, W, float(edge_threshold), int(edge_dilation), float(depth_jump_threshold),
         int(neighbor_check_radius), out.data_ptr(), ws.data_ptr(), ops.stream())
    return out


def points_render(points: torch.Tensor, features: torch.Tensor, extrinsic, K, size_hw, morph: bool = True, radius: float = 0.005,
                  drop: torch.Tensor = None):
    """project_points_to_image_pytorch (DepthCrafter/utils.py:103-171): points f32 [n, 3], features f32 [n, F] (device), extrinsic 4x4 and K
    3x3 (host), -> (image f32 [H, W, F], mask u8 [H, W, 1]) on the device.  drop: u8 [n], 1 = point removed beforehand (edge filter)."""
    from ._ffi import lib
    H, W = int(size_hw[0]), int(size_hw[1])
    points, features = points.to(torch.float32).contiguous(), features.to(torch.float32).contiguous()
    n, F = features.shape
    assert tuple(points.shape) == (n, 3)
    cam = pytorch3d_camera(extrinsic, K, (H, W))
    ws = torch.empty(int(lib().wf_points_render_workspace_bytes(H, W)), dtype=torch.uint8, device=points.device)
    img = torch.empty((H, W, F), dtype=torch.float32, device=points.device)
    mask = torch.empty((H, W), dtype=torch.uint8, device=points.device)
    call("wf_points_render", points.data_ptr(), features.data_ptr(), drop.contiguous().data_ptr() if drop is not None else None, n, F,
         cam.ctypes.data, H, W, float(radius), 1 if morph else 0, img.data_ptr(), mask.data_ptr(), ws.data_ptr(), ops.stream())
    return img, mask.unsqueeze(-1)


def render_depthcrafter_frame(rgb: torch.Tensor, depth_frame: torch.Tensor, cam, K, edge_filter: bool = True, **edge_kw):
    """One iteration of warp_depthcrafter.py:255-288: rgb f32 [H, W, 3] in [0, 1], depth_frame f32 [H, W] (= 1 / (disparity + 0.1)),
    cam 4x4, K 3x3 -> (rendered image f32 [H, W, 3], mask u8 [H, W, 1]); the reference skips the edge filter for frame 0."""
    H, W = depth_frame.shape
    Kf = np.asarray(K, dtype=np.float32)
    d = depth_frame.to(torch.float32)
    ii = torch.arange(H, device=d.device, dtype=torch.float32).view(H, 1)
    jj = torch.arange(W, device=d.device, dtype=torch.float32).view(1, W)
    pts = torch.stack(((jj - float(Kf[0, 2])) * d / float(Kf[0, 0]), (ii - float(Kf[1, 2])) * d / float(Kf[1, 1]), d), dim=-1).reshape(-1, 3)
    drop = depth_edge_mask(d, **edge_kw).reshape(-1) if edge_filter else None
    return points_render(pts, rgb.reshape(-1, 3), cam, K, (H, W), morph=True, drop=drop)


# ---- dynamic scenes, the whole route: DepthCrafter/warp_depthcrafter.py run_warping (:140-301) ---------------------------------------------
# Camera sequences (DepthCrafter/utils.py:240-492): float64 host math.  A "camera" here is what the reference builds -- a 4x4 whose rotation
# block is look_at's matrix and whose last column is the camera POSITION -- and hands to the renderer as the extrinsic, unchanged.
def dc_look_at(camera_pos, target, up) -> np.ndarray:
    """utils.py:240-250: the columns are right, up, forward of a camera at camera_pos aimed at target."""
    forward = np.asarray(target, dtype=np.float64) - np.asarray(camera_pos, dtype=np.float64)
    forward = forward / np.linalg.norm(forward)
    right = np.cross(up, forward)
    right = right / np.linalg.norm(right)
    return np.vstack([right, np.cross(forward, right), forward]).T


def _dc_orbit_camera(extrinsic, degree: float, depth: float, axis: int) -> np.ndarray:
    """get_look_up_camera (axis 1, :253-278) / get_look_right_camera (axis 0, with the angle negated, :281-306).  The target is taken from
    the position BEFORE it moves: the reference moves `t` in place after it has formed look_at_point."""
    E = np.asarray(extrinsic, dtype=np.float64)
    pos, R = E[:3, 3].copy(), E[:3, :3].copy()
    target = pos + R @ np.array([0, 0, depth], dtype=np.float64)
    rad = np.deg2rad(degree if axis == 1 else -degree)
    pos[axis] = pos[axis] + np.sin(rad) * depth
    pos[2] = pos[2] + (1 - np.cos(rad)) * depth
    cam = np.eye(4)
    cam[:3, :3] = dc_look_at(pos, target, np.array([0, 1, 0]))
    cam[:3, 3] = pos
    return cam


def _dc_stable_degrees(max_degree: float, frame_num: int, stable_frame: int):
    """:412-447: the angle reaches max_degree at frame stable_frame - 1 and stays there."""
    sf = min(stable_frame, frame_num)
    return [(i / (sf - 1)) * max_degree if (i < sf and sf > 1) else max_degree for i in range(frame_num)]


def dc_look_up_camera_seq(extrinsics, max_degree, frame_num, look_at_depth):
    """get_look_up_camera_seq (:309-319)."""
    return [_dc_orbit_camera(extrinsics, d, float(look_at_depth), 1) for d in np.linspace(0, max_degree, frame_num)]


def dc_look_right_camera_seq(extrinsics, max_degree, frame_num, look_at_depth):
    """get_look_right_camera_seq (:322-332)."""
    return [_dc_orbit_camera(extrinsics, d, float(look_at_depth), 0) for d in np.linspace(0, max_degree, frame_num)]


def dc_stable_look_up_camera_seq(extrinsics, max_degree, frame_num, look_at_depth, stable_frame=17):
    """get_stable_look_up_camera_seq (:412-428)."""
    return [_dc_orbit_camera(extrinsics, d, float(look_at_depth), 1) for d in _dc_stable_degrees(max_degree, frame_num, stable_frame)]


def dc_stable_look_right_camera_seq(extrinsics, max_degree, frame_num, look_at_depth, stable_frame=17):
    """get_stable_look_right_camera_seq (:431-447)."""
    return [_dc_orbit_camera(extrinsics, d, float(look_at_depth), 0) for d in _dc_stable_degrees(max_degree, frame_num, stable_frame)]


def _dc_zoom(cams, zoom_mode, rate, look_at_depth, progress):
    if zoom_mode == "none":
        return cams
    if not (0.0 < rate <= 1.0):
        raise ValueError("rate must be between 0.0 and 1.0")
    out = []
    for i, cam in enumerate(cams):
        pos, R = cam[:3, 3].copy(), cam[:3, :3].copy()
        target = pos + R @ np.array([0, 0, float(look_at_depth)], dtype=np.float64)
        away = pos - target
        p = progress(i)
        factor = 1.0 - p * (1.0 - rate) if zoom_mode == "zoom_out" else (1.0 + p * (1.0 / rate - 1.0) if zoom_mode == "zoom_in" else 1.0)
        new_pos = target + away * factor
        new = np.eye(4)
        new[:3, :3] = dc_look_at(new_pos, target, np.array([0, 1, 0]))
        new[:3, 3] = new_pos
        out.append(new)
    return out


def dc_apply_zoom_to_camera_seq(cams, zoom_mode, rate, look_at_depth):
    """apply_zoom_to_camera_seq (:371-409): every camera moves along its line to the point look_at_depth in front of it, to `rate` times
    the distance (zoom_out) or 1 / rate times (zoom_in) at the last frame."""
    n = len(cams)
    return _dc_zoom(cams, zoom_mode, rate, look_at_depth, lambda i: i / (n - 1) if n > 1 else 0.0)


def dc_apply_stable_zoom_to_camera_seq(cams, zoom_mode, rate, look_at_depth, stable_frame=17):
    """apply_stable_zoom_to_camera_seq (:450-492): the same, complete at frame stable_frame - 1."""
    sf = min(stable_frame, len(cams))
    return _dc_zoom(cams, zoom_mode, rate, look_at_depth, lambda i: i / (sf - 1) if (i < sf and sf > 1) else 1.0)


def depthcrafter_cameras(direction, degree, frame_num, look_at_depth_value, zoom="none", rate=0.8, stable=False, stable_frame=17):
    """The dispatch of run_warping (:211-247) from the identity extrinsic: `down` and `left` negate the angle; zoom, if any, is laid over the
    sequence; the rate check is main()'s (:374-375).  -> frame_num 4x4 float64 arrays."""
    if zoom not in ("zoom_in", "zoom_out", "none"):
        raise ValueError(f"Unsupported zoom: {zoom}")
    if zoom != "none" and not (0.0 < rate <= 1.0):
        raise ValueError(f"Rate must be between 0.0 and 1.0, got {rate}")
    if direction not in ("up", "down", "left", "right"):
        raise ValueError(f"Unsupported direction: {direction}")
    E = np.eye(4)
    deg = degree if direction in ("up", "right") else -degree
    if stable:
        seq = dc_stable_look_up_camera_seq if direction in ("up", "down") else dc_stable_look_right_camera_seq
        cams = seq(E, deg, frame_num, look_at_depth_value, stable_frame)
        if zoom != "none":
            cams = dc_apply_stable_zoom_to_camera_seq(cams, zoom, rate, look_at_depth_value, stable_frame)
    else:
        seq = dc_look_up_camera_seq if direction in ("up", "down") else dc_look_right_camera_seq
        cams = seq(E, deg, frame_num, look_at_depth_value)
        if zoom != "none":
            cams = dc_apply_zoom_to_camera_seq(cams, zoom, rate, look_at_depth_value)
    return cams


def median_index(n: int) -> int:
    """The k of wf_select_pair_f32 whose pair np.median(a) of n values needs: sorted[(n - 1) // 2] and its successor."""
    return (int(n) - 1) // 2


def median_from_pair(lo, hi, n: int) -> np.float32:
    """np.median of n float32 values from (sorted[k], sorted[k + 1]), k = median_index(n): the lower value itself for odd n, for even n the
    float32 mean as numpy forms it (the float32 sum, divided by 2)."""
    lo, hi = np.float32(lo), np.float32(hi)
    return lo if n % 2 else np.float32(np.float32(lo + hi) / np.float32(2))


def median_f32(x: torch.Tensor) -> np.float32:
    """np.median(x) of an fp32 device tensor, bit for bit; a NaN in x is a ValueError (numpy would return NaN)."""
    n = x.numel()
    lo, hi, nans = select_pair(x, median_index(n))
    if nans:
        raise ValueError(f"median_f32: {nans} NaN value(s) in the input (numpy's median would be NaN)")
    return median_from_pair(lo, hi, n)


def resize_bilinear(frames: torch.Tensor, size_hw, antialias: bool = True) -> torch.Tensor:
    """torchvision.transforms.functional.resize(frames, (H, W)) of float frames, channels-last: f32 [T, h, w, 3] (device) -> [T, H, W, 3]
    (wf_resize_bilinear_aa_f32).  antialias=True is torchvision's default on tensors since 0.17; older releases default to False (plain
    bilinear, which differs when the frames shrink).  Which release the reference's users run is unpinned."""
    from ._ffi import lib
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames must be [T, h, w, 3], got {tuple(frames.shape)}")
    frames = frames.to(torch.float32).contiguous()
    T, h, w, _ = frames.shape
    H, W = int(size_hw[0]), int(size_hw[1])
    aa = 1 if antialias else 0
    ws = torch.empty(int(lib().wf_resize_bilinear_aa_f32_workspace_bytes(T, h, w, H, W, aa)), dtype=torch.uint8, device=frames.device)
    out = torch.empty((T, H, W, 3), dtype=torch.float32, device=frames.device)
    call("wf_resize_bilinear_aa_f32", frames.data_ptr(), out.data_ptr(), T, h, w, H, W, aa, ws.data_ptr(), ops.stream())
    return out


DC_WORKSPACE_BUDGET = 2 << 30  # bytes of wf_dc_warp_frames workspace above which warp_depthcrafter_frames splits the frames into chunks


def dc_warp_frames(rgb: torch.Tensor, disparity: torch.Tensor, cams, K, edge_filter_from: int = 1, edge_threshold: float = 0.1,
                   edge_dilation: int = 3, depth_jump_threshold: float = 0.3, neighbor_check_radius: int = 2, radius: float = 0.005,
                   morph: bool = True, return_float: bool = False, workspace_budget: int = None, K_points=None):
    """wf_dc_warp_frames: rgb f32 [T, H, W, 3] in [0, 1], disparity f32 [T, H, W] (device), cams T 4x4 (host), K 3x3 -> (images u8
    [T, H, W, 3], masks u8 [T, H, W][, float images f32 [T, H, W, 3]]).  Frames t >= edge_filter_from get the edge filter.  One call, unless
    its workspace (11 bytes per pixel) exceeds workspace_budget (default DC_WORKSPACE_BUDGET): then one call per chunk of frames.
    K_points: the intrinsics the pixels are un-projected with, where they differ from the camera's K (the reference uses one K for both)."""
    from ._ffi import lib
    rgb, disparity = rgb.to(torch.float32).contiguous(), disparity.to(torch.float32).contiguous()
    T, H, W = disparity.shape
    if tuple(rgb.shape) != (T, H, W, 3) or len(cams) != T:
        raise ValueError(f"rgb {tuple(rgb.shape)}, disparity {tuple(disparity.shape)} and {len(cams)} cameras do not match")
    dev = disparity.device
    Kf = np.asarray(K, dtype=np.float32)
    cam16 = torch.from_numpy(np.stack([pytorch3d_camera(c, Kf, (H, W)) for c in cams])).to(dev)
    Kp = Kf if K_points is None else np.asarray(K_points, dtype=np.float32)
    images = torch.empty((T, H, W, 3), dtype=torch.uint8, device=dev)
    masks = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    fimg = torch.empty((T, H, W, 3), dtype=torch.float32, device=dev) if return_float else None
    budget = DC_WORKSPACE_BUDGET if workspace_budget is None else int(workspace_budget)
    chunk = min(T, max(1, budget // max(1, int(lib().wf_dc_warp_frames_workspace_bytes(1, H, W)))))
    ws = torch.empty(int(lib().wf_dc_warp_frames_workspace_bytes(chunk, H, W)), dtype=torch.uint8, device=dev)
    for t0 in range(0, T, chunk):
        n = min(chunk, T - t0)
        call("wf_dc_warp_frames", rgb[t0:].data_ptr(), disparity[t0:].data_ptr(), cam16[t0:].data_ptr(), float(Kp[0, 0]), float(Kp[1, 1]),
             float(Kp[0, 2]), float(Kp[1, 2]), float(edge_threshold), int(edge_dilation), float(depth_jump_threshold),
             int(neighbor_check_radius), max(0, int(edge_filter_from) - t0), float(radius), 1 if morph else 0, n, H, W,
             images[t0:].data_ptr(), masks[t0:].data_ptr(), fimg[t0:].data_ptr() if return_float else None, ws.data_ptr(), ops.stream())
    return (images, masks, fimg) if return_float else (images, masks)


def warp_depthcrafter_frames(frames, disparity, direction="left", degree=15.0, look_at_depth=1.0, zoom="none", rate=0.8, stable=False,
                             stable_frame=17, enable_edge_filter=False, edge_threshold=0.1, edge_dilation=3, depth_jump_threshold=0.3,
                             neighbor_check_radius=2, antialias=True, return_float=False, device="cuda:0"):
    """run_warping (warp_depthcrafter.py:201-290) on the device: frames [T, h, w, 3], u8 or float holding 0..255 (what an image reader
    returns); disparity [T, H, W] (the `depth` of depth.npz).  frames / 255 -> resize to H x W (resize_bilinear; `antialias` as there) ->
    K = [[525, 0, W / 2], [0, 525, H / 2]] in float32 -> look-at depth = np.median(1 / (disparity[0] + 0.1)) * look_at_depth in float32 ->
    depthcrafter_cameras -> dc_warp_frames (frame 0 never gets the edge filter).  -> (images u8 [T, H, W, 3], masks u8 [T, H, W], cams
    [, float images]) with images and masks on the device.
    ValueError: shapes other than [T, h, w, 3] / [T, H, W]; a frame count that differs from the depth's; a NaN in frame 0's depth."""
    dev = torch.device(device)
    fr, disp = torch.as_tensor(frames), torch.as_tensor(disparity)
    if fr.dim() != 4 or fr.shape[3] != 3:
        raise ValueError(f"frames must be [T, h, w, 3], got {tuple(fr.shape)}")
    if disp.dim() != 3:
        raise ValueError(f"disparity must be [T, H, W], got {tuple(disp.shape)}")
    if fr.shape[0] != disp.shape[0]:
        raise ValueError(f"{fr.shape[0]} frames but {disp.shape[0]} depth maps")
    T, H, W = disp.shape
    disp = disp.to(dev).to(torch.float32).contiguous()
    rgb = resize_bilinear(fr.to(dev) / 255.0, (H, W), antialias=antialias)
    K = np.array([[525.0, 0, 0.5 * W], [0, 525.0, 0.5 * H], [0, 0, 1]], dtype=np.float32)
    try:
        med = median_f32(1.0 / (disp[0] + 0.1))
    except ValueError as e:
        raise ValueError(f"warp_depthcrafter_frames: NaN in the depth of frame 0 ({e})") from None
    look = float(np.float32(med * np.float32(look_at_depth)))  # np.float32 * float stays float32, as in the reference
    cams = depthcrafter_cameras(direction, degree, T, look, zoom, rate, stable, stable_frame)
    out = dc_warp_frames(rgb, disp, cams, K, edge_filter_from=1 if enable_edge_filter else T, edge_threshold=edge_threshold,
                         edge_dilation=edge_dilation, depth_jump_threshold=depth_jump_threshold, neighbor_check_radius=neighbor_check_radius,
                         return_float=return_float)
    return (out[0], out[1], cams) + tuple(out[2:])
