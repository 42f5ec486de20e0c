"""Scenes and cases of the dynamic-scene stage-1 fixtures (G29), shared by tools/make_dynamic_warp_golden.py and the tests: seeded inputs
are rebuilt from here, only what the reference made of them is stored under tests/golden/.

The reference's renderer has a fixed radius of 0.005 NDC units (the short side spans 2), and a source pixel (i, j) un-projects through
K = [[525, 0, W / 2], [0, 525, H / 2]] to the CORNER between four target pixels.  Below a short side of about 2 / (0.005 sqrt 2) = 283
pixels a point therefore reaches a pixel centre only by chance: scenes `a` and `b` (the two small orientations) come out as sparse specks
that the opening removes, and show the camera, resize, filter and quantisation plumbing.  Scene `c` (short side 288) is the one with real
coverage, cracks and opened slivers."""
import numpy as np

SCENES = {"a": dict(T=5, H=48, W=80, h=60, w=100, seed=29), "b": dict(T=4, H=80, W=48, h=40, w=24, seed=30),
          "c": dict(T=2, H=288, W=304, h=200, w=212, seed=31)}
CASES = {
    "a_left_edge": dict(scene="a", native=False, direction="left", degree=9.0, enable_edge_filter=True),
    "a_up_zoom_in": dict(scene="a", native=False, direction="up", degree=7.0, zoom="zoom_in", rate=0.8, enable_edge_filter=False),
    "a_native_right_edge": dict(scene="a", native=True, direction="right", degree=9.0, enable_edge_filter=True),
    "b_down_stable_edge": dict(scene="b", native=False, direction="down", degree=8.0, stable=True, stable_frame=3, enable_edge_filter=True),
    "b_right": dict(scene="b", native=False, direction="right", degree=9.0, enable_edge_filter=False),
    "b_native_left_edge": dict(scene="b", native=True, direction="left", degree=8.0, zoom="zoom_out", rate=0.9, enable_edge_filter=True),
    "c_native_left_edge": dict(scene="c", native=True, direction="left", degree=1.5, enable_edge_filter=True),
    "c_up_edge": dict(scene="c", native=False, direction="up", degree=1.0, enable_edge_filter=True),
}
DEFAULTS = dict(look_at_depth=1.0, zoom="none", rate=0.8, stable=False, stable_frame=17, edge_threshold=0.1, edge_dilation=3,
                depth_jump_threshold=0.3, neighbor_check_radius=2)


def options(case: str) -> dict:
    opt = dict(DEFAULTS)
    opt.update({k: v for k, v in CASES[case].items() if k not in ("scene", "native")})
    return opt


def scene(name: str) -> dict:
    """-> frames u8 [T, h, w, 3] (source size), frames_native u8 [T, H, W, 3], disparity f32 [T, H, W]: a near box that moves across a
    sloped background, a far strip on the left border, a near strip on the bottom border."""
    s = SCENES[name]
    T, H, W, h, w = s["T"], s["H"], s["W"], s["h"], s["w"]
    rng = np.random.default_rng(s["seed"])
    yy, xx = np.mgrid[0:H, 0:W]
    disp = np.empty((T, H, W), dtype=np.float32)
    for t in range(T):
        d = 0.2 + 0.25 * xx / W + 0.15 * yy / H + 0.05 * np.sin(yy / 7.0) + 0.01 * rng.random((H, W))
        x0, y0 = W // 5 + 3 * t, H // 4 + t
        d[y0:y0 + H // 3, x0:x0 + W // 3] += 0.45
        d[:, :3] -= 0.12
        d[H - 4:, W // 2:] += 0.3
        disp[t] = d

    def frames(hh, ww):
        y, x = np.mgrid[0:hh, 0:ww]
        out = np.empty((T, hh, ww, 3), dtype=np.uint8)
        for t in range(T):
            base = np.stack([128 + 100 * np.sin(x / ww * 6 + t), 128 + 100 * np.cos(y / hh * 5 - t), 255.0 * ((x + y + 3 * t) % 17) / 16], -1)
            out[t] = np.clip(base + rng.integers(-6, 7, size=(hh, ww, 3)), 0, 255).astype(np.uint8)
        return out

    return dict(frames=frames(h, w), frames_native=frames(H, W), disparity=disp)


# Bars of wf_resize_bilinear_aa_f32 against torch's CPU kernel in float32 (maximum absolute error on data in [0, 1]): 2 x the measured
# value per case, the rule of tolerances_mi355x.json; the measurements (in the comments) are in profiles/stage1_dynamic_warp.md: one to
# three float32 ulps of values below 1, i.e. rounding.  Keys: (h, w, H, W, antialias).
RESIZE_BARS = {
    (60, 100, 48, 80, True): 2 * 1.788e-07, (60, 100, 48, 80, False): 2 * 1.192e-07,  # measured 1.788e-07, 1.192e-07
    (40, 24, 80, 48, True): 2 * 1.192e-07, (40, 24, 80, 48, False): 2 * 1.192e-07,    # measured 1.192e-07, 1.192e-07
    (7, 5, 3, 2, True): 2 * 5.960e-08, (7, 5, 3, 2, False): 2 * 5.960e-08,            # measured 5.960e-08, 5.960e-08
}
RESIZE_BAR_MAX = max(RESIZE_BARS.values())  # what the recorder perturbs the colours by
