"""Inputs of the point renderer's recorded-output test (tests/golden/g30_pointrender_parent.json): numpy only, importable without a GPU.

Three families, each a dict of case id -> a function that builds the call's arguments:
  POINT_CASES   wf_points_render on arbitrary point arrays: exact z ties between different points, exact duplicates, points far outside the
                image, behind the camera, NaN, at the origin; both NDC orientations and a square; one case with more points than one grid
  EDGE_CASES    wf_depth_edge_mask on the depths of `scene`, down to 2 x 2, with each stage switched off in turn and at the largest radii
  BATCH_SCENES  wf_dc_warp_frames on the scenes of test_batched_equals_per_frame (the 17-row one aside)
tests/test_pointrender_cases_host.py asserts on the CPU oracle what makes the point cases worth running; tools/record_pointrender_digests.py
records the digests."""
import hashlib

import numpy as np

F32 = np.float32
POINT_SHAPES = [(40, 56), (56, 40), (33, 33)]
N_POINTS = 3000
BIG_N, BIG_DEAD = 600_000, 590_000  # more points than 2048 x 256 threads; the first BIG_DEAD are behind the camera
EDGE_SHAPES = [(40, 56), (57, 33), (2, 2), (2, 37)]
EDGE_DEFAULT = (0.1, 3, 0.3, 2)  # edge_threshold, edge_dilation, depth_jump_threshold, neighbor_check_radius
EDGE_PARAMS = {"default": EDGE_DEFAULT, "dil0": (0.1, 0, 0.3, 2), "jump0": (0.1, 3, 0.0, 2), "nr0": (0.1, 3, 0.3, 0), "r15": (0.1, 15, 0.3, 15)}
BATCH_SHAPES = [(35, 131, True), (131, 35, True), (35, 131, False), (131, 35, False), (288, 300, False)]


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def intrinsics(H, W, centred=False):
    K = np.array([[525, 0, W / 2], [0, 525, H / 2], [0, 0, 1]], dtype=F32)
    if centred:
        K[:2, 2] -= F32(0.5)
    return K


def moved(tx, th):
    cam = np.eye(4)
    cam[0, 3], cam[1, 3] = tx, -tx / 2
    cam[:3, :3] = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    return cam


def scene(T, H, W, seed, steps=(0.0, 0.02, 0.45)):
    """rgb f32 [T, H, W, 3], disparity f32 [T, H, W]: frame t carries a box whose disparity step is steps[t] -- frames 1 and 2 differ in
    their Sobel maximum by far more than 10 x -- over a gentle ripple, with features on every border."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    disp = np.empty((T, H, W), dtype=F32)
    for t in range(T):
        d = 0.3 + 0.004 * np.sin(xx / 9.0) + 0.004 * np.cos(yy / 11.0) + 0.0001 * rng.random((H, W))
        d[H // 4:H // 4 + max(6, H // 3), W // 4:W // 4 + max(6, W // 3)] += steps[t % len(steps)]
        d[:2, : W // 2] += steps[t % len(steps)]
        d[H // 2:, W - 2:] += steps[t % len(steps)]
        disp[t] = d
    return rng.random((T, H, W, 3)).astype(F32), disp


def depth_of(disp):
    return (F32(1.0) / (disp.astype(F32) + F32(0.1))).astype(F32)


def points(H, W, n=N_POINTS, F=5):
    """-> dict(pts f32 [n, 3], feats f32 [n, F], drop u8 [n], K, cam, size): few distinct depths (exact z ties between different points),
    the points [n // 2, n // 2 + n // 8) exact copies of [0, n // 8), a margin of 4 pixels around the image, six degenerate points last."""
    rng = np.random.default_rng(H * W)
    z = np.round((1.5 + rng.random(n)) * 8) / 8
    u, v = rng.random(n) * (W + 8) - 4, rng.random(n) * (H + 8) - 4
    pts = np.stack([(u - W / 2) * z / 525, (v - H / 2) * z / 525, z], axis=-1).astype(F32)
    pts[n // 2:n // 2 + n // 8] = pts[:n // 8]
    pts[-6:] = np.array([[1e30, 0, 1], [0, -1e30, 1], [0, 0, -1], [np.nan, 0, 1], [0, 0, 0], [1e-30, 1e-30, 1e-38]], dtype=F32)
    feats = rng.random((n, F)).astype(F32)
    drop = (rng.random(n) < 0.2).astype(np.uint8)
    cam = np.eye(4)
    cam[0, 3] = 0.01
    return dict(pts=pts, feats=feats, drop=drop, K=intrinsics(H, W), cam=cam, size=(H, W))


def big_points():
    """(40, 56), BIG_N points, F = 1: the first BIG_DEAD at z = -1, the rest the recipe of `points`."""
    c = points(40, 56, n=BIG_N - BIG_DEAD, F=1)
    dead = np.zeros((BIG_DEAD, 3), dtype=F32)
    dead[:, 2] = -1
    rng = np.random.default_rng(BIG_N)
    c["pts"] = np.concatenate([dead, c["pts"]])
    c["feats"] = np.concatenate([rng.random((BIG_DEAD, 1)).astype(F32), c["feats"]])
    c["drop"] = np.concatenate([(rng.random(BIG_DEAD) < 0.2).astype(np.uint8), c["drop"]])
    return c


def point_cases():
    """-> {id: (scene key, dict(radius, morph, use_drop))}; the scene is points(*key) or big_points() for key == "big"."""
    out = {}
    for H, W in POINT_SHAPES:
        for radius in (0.05, 0.005):
            for morph in (True, False):
                for use_drop in (True, False):
                    out[f"pts_{H}x{W}_r{radius}_{'open' if morph else 'raw'}_{'drop' if use_drop else 'all'}"] = \
                        ((H, W), dict(radius=radius, morph=morph, use_drop=use_drop))
    out["pts_big_r0.05_open_drop"] = ("big", dict(radius=0.05, morph=True, use_drop=True))
    return out


def point_scene(key):
    return big_points() if key == "big" else points(*key)


def edge_cases():
    """-> {id: ((H, W), frame, (edge_threshold, edge_dilation, depth_jump_threshold, neighbor_check_radius))}."""
    return {f"edge_{H}x{W}_f{t}_{name}": ((H, W), t, p) for H, W in EDGE_SHAPES for t in range(3) for name, p in EDGE_PARAMS.items()}


def edge_depths(H, W):
    """depth f32 [3, H, W] of the edge-filter scene (the one of test_separable_edge_filter_equals_the_oracle)."""
    return depth_of(scene(3, H, W, seed=7 * H, steps=(0.3, 0.05, 0.45))[1])


def batch_scene(H, W, centred):
    """The arguments of test_batched_equals_per_frame: -> rgb, disparity, cams, K, K_points (None = K), edge_filter_from."""
    rgb, disp = scene(3, H, W, seed=H)
    cams = [np.eye(4), np.eye(4), np.eye(4) if centred else moved(0.01, 0.004)]
    if not centred:
        cams[1] = moved(-0.006, 0.0)
    return rgb, disp, cams, intrinsics(H, W), intrinsics(H, W, centred=True) if centred else None, 1


def batch_id(H, W, centred):
    return f"batch_{H}x{W}_{'centred' if centred else 'corner'}"
