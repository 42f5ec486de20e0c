"""Stage 1 after the networks, timed per stage on the GPU: a synthetic 1280 x 720 scene, 25 warped views, run_warp.py's shipped parameters
(outlier window 7 x 7 / min_neighbors 10, 8 depth segments).  HIP events, the median of 9 after a warm-up.  Writes a markdown table:

    python tools/stage1_bench.py [--out profiles/stage1_warp.md] [--height 720 --width 1280 --views 25]

Stages: select (wf_select_pair_f32 + the 12-byte read), filter (wf_depth_conf_filter + the 16-byte read), splat (wf_warp_splat), crack
fill (wf_crack_fill_ex at radius 3 / 8 segments, beside wf_crack_fill at radius 1 / 5 segments on the same views).  The crack fill's
algorithmic traffic is what any implementation must move: the splatted image, mask and depth in, the filled ones out, 16 bytes a pixel;
its time is set against that at 8 TB/s.  No CPU fallback: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from worldforge_amd import warp  # noqa: E402

HBM_BYTES_PER_S = 8e12


def scene(H, W, seed=0):
    g = np.random.default_rng(seed)
    s = W / 64.0
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = (2.0 + 0.6 * np.sin(xx / (9.0 * s)) + 0.4 * np.cos(yy / (7.0 * s)) + 0.05 * g.standard_normal((H, W))).astype(np.float32)
    near = (xx > 40 * s) & (yy < 20 * s)
    depth[near] = (1.1 + 0.01 * g.standard_normal((H, W))).astype(np.float32)[near]
    image = g.random((H, W, 3)).astype(np.float32)
    K = np.array([[55.0 * s, 0, W / 2 - 0.5], [0, 55.0 * s, H / 2 - 0.5], [0, 0, 1]])
    conf = (1.0 + np.exp(1.5 * g.standard_normal((H, W)))).astype(np.float32)
    conf[g.random((H, W)) < 0.1] = 1.0
    return image, depth, conf, K, np.eye(4)


def timed(fn, reps=9, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage1_warp.md"))
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--views", type=int, default=25)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("stage1_bench: no GPU (there is no CPU path to time)")
    H, W, n, dev = a.height, a.width, a.views, a.device
    image, depth, conf, K, E = scene(H, W)
    img_d, dep_d, conf_d = (torch.from_numpy(x).to(dev) for x in (image, depth, conf))
    p = warp.RUN_WARP_DEFAULTS
    filtered, thr, mean, count = warp.depth_conf_filter(dep_d, conf_d, 0.8)
    cams = warp.camera_path("left", E, 20.0, n + 1, float(np.float32(mean)))[1:]
    wi, wm, wd = warp.forward_splat(img_d, filtered, K, E, cams, device=dev)
    rows = [("select (np.percentile's pair, 20th percentile of conf)", timed(lambda: warp.percentile_f32(conf_d, 20.0))),
            ("filter (conf > threshold, fp64 mean)", timed(lambda: warp.depth_conf_filter(dep_d, conf_d, 0.8, threshold=thr))),
            (f"splat, {n} views", timed(lambda: warp.forward_splat(img_d, filtered, K, E, cams, device=dev))),
            (f"wf_crack_fill_ex, radius 3 / 8 segments / min_neighbors 10, {n} views",
             timed(lambda: warp.crack_fill_ex(wi, wm, wd, min_neighbors=p["min_neighbors"], neighbor_radius=p["neighbor_radius"],
                                              min_valid_neighbors=p["min_valid_neighbors"], num_segments=8, original_depth=filtered,
                                              has_depth_conf=True, depth_threshold=p["depth_threshold"], max_crack_size=p["max_crack_size"]))),
            (f"wf_crack_fill, radius 1 / 5 segments / min_neighbors 4, {n} views",
             timed(lambda: warp.crack_fill(wi, wm, wd, min_neighbors=4, min_valid_neighbors=p["min_valid_neighbors"], num_segments=5,
                                           original_depth=filtered, has_depth_conf=True))),
            (f"wf_crack_fill_ex, radius 1 / 5 segments / min_neighbors 4, {n} views",
             timed(lambda: warp.crack_fill_ex(wi, wm, wd, min_neighbors=4, neighbor_radius=1, min_valid_neighbors=p["min_valid_neighbors"],
                                              num_segments=5, original_depth=filtered, has_depth_conf=True)))]
    whole = timed(lambda: warp.warp_single_img(E, K, torch.from_numpy(image).permute(2, 0, 1), dep_d, conf_d, "left", 20.0, 0.8, n + 1, True,
                                               dict(p), 1.0, 8, dev), reps=5, warmup=1)
    pix = n * H * W
    algo = 16 * pix
    lines = ["# Stage 1 after the networks: select, filter, splat, crack fill", "",
             f"`python tools/stage1_bench.py` on {torch.cuda.get_device_name(0)}: synthetic {W} x {H} scene, {n} warped views, run_warp.py's",
             "shipped parameters; HIP events around each call (launches, workspace allocation and, for select / filter, the small host read",
             "included), median of 9 after 2 warm-up calls.  Kept fraction of the confidence filter: "
             f"{count / (H * W):.3f}; splatted coverage {float(wm.float().mean()):.3f}.", "",
             "| stage | median ms | min | max |", "|---|---|---|---|"]
    lines += [f"| {name} | {m:.3f} | {lo:.3f} | {hi:.3f} |" for name, (m, lo, hi) in rows]
    lines += [f"| warp_single_img, whole call (upload of the image, 2 host reads, {n} views) | {whole[0]:.3f} | {whole[1]:.3f} | {whole[2]:.3f} |", ""]
    ex = rows[3][1][0]
    lines += [f"Crack fill, algorithmic traffic: image + mask + depth in and out = 16 bytes a pixel x {pix} pixels = {algo / 1e6:.1f} MB.",
              f"At {ex:.3f} ms that is {algo / ex / 1e9:.3f} TB/s, {100 * algo / (ex * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s (bound: memory; the kernels",
              "themselves move about 37 bytes a pixel through the segment-id and fill-set workspaces).", "",
              "The VGGT part of stage 1 at the released size is in profiles/vggt_encode.md and profiles/vggt_depth.md; it is not re-measured here.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
