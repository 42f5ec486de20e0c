"""Stage 1 for dynamic scenes, timed on the GPU: 49 frames of 576 x 1024 from 720 x 1280 sources, seeded, edge filter on.  HIP events, the
median of 9 after a warm-up, both arms in one process on one box.  Writes a markdown table:

    python tools/dynamic_warp_bench.py [--out profiles/stage1_dynamic_warp.md] [--frames 49]

Rows: the batched call (wf_dc_warp_frames, one call for all frames), the loop of per-frame calls (warp.render_depthcrafter_frame per
frame: the same kernels at T = 1 on a stored depth plane and point array, the depth 1 / (d + 0.1) included as the loop computes it), the resize
(wf_resize_bilinear_aa_f32, antialias on) and the median of frame 0 (wf_select_pair_f32 + the 12-byte read).  Below them the resize's
measured error against torch's CPU kernel on the test sizes (the bars of tests/dynwarp_cases.py are twice these).  No CPU fallback:
without a GPU the tool fails."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from worldforge_amd import warp  # noqa: E402

RESIZE_CASES = [(60, 100, 48, 80), (40, 24, 80, 48), (7, 5, 3, 2), (48, 80, 48, 80)]


def scene(T, H, W, h, w, seed=0):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    disp = np.empty((T, H, W), dtype=np.float32)
    for t in range(T):
        d = 0.25 + 0.2 * np.sin(xx / 160.0 + 0.05 * t) * np.cos(yy / 120.0) + 0.2 * xx / W + 0.005 * g.random((H, W))
        x0 = W // 6 + 6 * t
        d[H // 4:H // 4 + H // 3, x0:x0 + W // 4] += 0.35
        disp[t] = d
    frames = g.integers(0, 256, size=(T, h, w, 3), dtype=np.uint8)
    return frames, disp


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


def resize_errors(dev):
    out = []
    for h, w, H, W in RESIZE_CASES:
        x = torch.from_numpy(np.random.default_rng(h * W).random((3, h, w, 3)).astype(np.float32))
        for aa in (True, False):
            want = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False,
                                                   antialias=aa).permute(0, 2, 3, 1)
            got = warp.resize_bilinear(x.to(dev), (H, W), antialias=aa).cpu()
            out.append(((h, w, H, W, aa), float((got - want).abs().max())))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage1_dynamic_warp.md"))
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--src-height", type=int, default=720)
    ap.add_argument("--src-width", type=int, default=1280)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("dynamic_warp_bench: no GPU (there is no CPU path to time)")
    T, H, W, h, w, dev = a.frames, a.height, a.width, a.src_height, a.src_width, a.device
    frames, disp = scene(T, H, W, h, w)
    src = torch.from_numpy(frames).to(dev) / 255.0
    disp_d = torch.from_numpy(disp).to(dev)
    rgb = warp.resize_bilinear(src, (H, W))
    K = np.array([[525.0, 0, 0.5 * W], [0, 525.0, 0.5 * H], [0, 0, 1]], dtype=np.float32)
    look = float(warp.median_f32(1.0 / (disp_d[0] + 0.1)))
    cams = warp.depthcrafter_cameras("left", 15.0, T, look)

    def loop():
        out = []
        for t in range(T):
            out.append(warp.render_depthcrafter_frame(rgb[t], 1.0 / (disp_d[t] + 0.1), cams[t], K, edge_filter=t > 0))
        return out

    images, masks = warp.dc_warp_frames(rgb, disp_d, cams, K)
    ref = loop()
    same = all(torch.equal(masks[t], ref[t][1][..., 0]) for t in range(T))
    rows = [(f"batched: wf_dc_warp_frames, {T} frames in one call (u8 frames and masks out)", timed(lambda: warp.dc_warp_frames(rgb, disp_d, cams, K))),
            (f"per-frame loop: render_depthcrafter_frame x {T} (fp32 frames out)", timed(loop)),
            (f"resize {h} x {w} -> {H} x {W}, {T} frames, antialias", timed(lambda: warp.resize_bilinear(src, (H, W)))),
            ("median of frame 0 (select pair + 12-byte read)", timed(lambda: warp.median_f32(1.0 / (disp_d[0] + 0.1))))]
    b, l = rows[0][1][0], rows[1][1][0]
    lines = ["# Stage 1 for dynamic scenes: batched warp, per-frame loop, resize, median", "",
             f"`python tools/dynamic_warp_bench.py` on {torch.cuda.get_device_name(0)}: {T} frames of {H} x {W} from {h} x {w} sources, seeded,",
             "direction left 15 degrees, edge filter on (frames 1..); HIP events around each call (launches, workspace and output allocation",
             "included), median of 9 after 2 warm-up calls, both arms in this process.  Coverage of the warped frames: "
             f"{float(masks[1:].float().mean()):.3f}; masks of the two arms equal: {same}.", "",
             "| call | median ms | min | max |", "|---|---|---|---|"]
    lines += [f"| {name} | {m:.3f} | {lo:.3f} | {hi:.3f} |" for name, (m, lo, hi) in rows]
    lines += ["", f"Batched against loop: {l / b:.2f} x ({'faster' if b < l else 'NOT faster'}).", "",
              "## Resize against torch's CPU kernel (float32, data in [0, 1])", "",
              "Maximum absolute error of wf_resize_bilinear_aa_f32 against `F.interpolate(mode=\"bilinear\", align_corners=False, antialias=...)`",
              "on the CPU, 3 frames per size.  tests/dynwarp_cases.py sets each bar to twice the value measured here.", "",
              "| h x w -> H x W | antialias | max abs error |", "|---|---|---|"]
    lines += [f"| {k[0]} x {k[1]} -> {k[2]} x {k[3]} | {k[4]} | {e:.3e} |" for k, e in resize_errors(dev)]
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
