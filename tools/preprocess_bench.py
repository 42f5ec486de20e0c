"""Device image preprocessing for VGGT and CLIP, timed: decoded u8 pixels to the network's fp32 input.

    python tools/preprocess_bench.py [--out profiles/device_preprocess.md]

Two cases, each in one process on one box: VGGT, 8 frames of 720 x 1280 -> 294 x 518 (bicubic, no crop at this aspect ratio), and CLIP,
one frame of 480 x 832 -> shortest edge 224 -> the centre 224 x 224 (bicubic).  For each:
(a) the host function (vggt.preprocess / clip.preprocess on PIL images) -- wall clock, median of 5; its result stays on the host;
(b) the device route's GPU work, ops.resample_u8_window on u8 frames that are already on the device (wf_resample_u8_window_f32: the
    column pass over the rows and columns the window needs, then row taps + table + planar store in one kernel) -- HIP events around
    20 calls, 15 samples after 3 warm-ups, median / min / max of the per-call time;
(c) the same tensor composed from the entry points that existed before it: ops.resample_u8 of the whole frame, the window as a slice,
    ops.u8_lut_planar (one call per distinct channel table), channels moved behind the frame axis -- timed as (b), samples of (b) and (c)
    alternating.
The three results are compared (torch.equal) before anything is timed.  Event times include the wrappers' allocations; the tables are
built and uploaded in the warm-up.  No CPU fallback: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from worldforge_amd import clip, ops, vggt  # noqa: E402

CLIP_CONFIG = {"size": {"shortest_edge": 224}, "crop_size": {"height": 224, "width": 224}, "resample": 3, "rescale_factor": 1 / 255,
               "image_mean": [0.48145466, 0.4578275, 0.40821073], "image_std": [0.26862954, 0.26130258, 0.27577711]}
INNER, SAMPLES, WARMUP = 20, 15, 3


def scene(T, h, w, seed=0):
    """Smooth colour frames with noise, as photographs are, not white noise."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    frames = np.empty((T, h, w, 3), np.uint8)
    for t in range(T):
        base = 127 + 100 * np.sin(xx / 90.0 + 0.1 * t)[..., None] * np.cos(yy / 70.0)[..., None] * np.array([1.0, 0.8, 0.6])
        frames[t] = np.clip(base + g.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
    return frames


def composed(frames, size, window, lut):
    """The window entry's tensor from ops.resample_u8, a slice and ops.u8_lut_planar."""
    y0, x0, Hc, Wc = window
    win = ops.resample_u8(frames, size)[:, y0:y0 + Hc, x0:x0 + Wc]
    if bool((lut == lut[:1]).all()):
        return ops.u8_lut_planar(win.contiguous(), lut[0].contiguous()).permute(1, 0, 2, 3).contiguous()
    return torch.cat([ops.u8_lut_planar(win[..., c].contiguous(), lut[c].contiguous()) for c in range(lut.shape[0])]).permute(1, 0, 2, 3).contiguous()


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


def alternating(f, g):
    for _ in range(WARMUP):
        f()
        g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(SAMPLES):
        tf.append(sample(f))
        tg.append(sample(g))
    return tuple((statistics.median(t), min(t), max(t)) for t in (tf, tg))


def wall(fn, reps=5):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def verdict(b, c):
    if b[2] < c[1]:
        return f"(b) is faster than (c) beyond the measured spread: {c[0] / b[0]:.2f} x by the medians, every sample of (b) below every sample of (c)."
    if b[0] < c[0]:
        return (f"(b) is NOT faster than (c) beyond the measured spread: the medians differ by {c[0] / b[0]:.2f} x in favour of (b), but the "
                "samples of the two overlap.")
    return f"(b) is NOT faster than (c): the composed route's median is {b[0] / c[0]:.2f} x lower."


def main(argv=None) -> int:
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_preprocess.md"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench: no GPU (there is no CPU path to time)")
    dev = torch.device(a.device)
    rows, notes = [], []

    # VGGT: 8 frames of 720 x 1280
    frames = scene(8, 720, 1280)
    pil = [Image.fromarray(f) for f in frames]
    want = vggt.preprocess(pil)
    nh, tw = int(want.shape[2]), int(want.shape[3])
    fd = torch.from_numpy(frames).to(dev)
    lut = torch.tensor(np.arange(256, dtype=np.uint8)).float().div(255).expand(3, 256).contiguous().to(dev)
    size, window = (nh, tw), (0, 0, nh, tw)
    same = (torch.equal(vggt.preprocess_device(pil, dev).cpu(), want) and torch.equal(ops.resample_u8_window(fd, size, window, lut).cpu(), want) and
            torch.equal(composed(fd, size, window, lut).cpu(), want))
    t_host = wall(lambda: vggt.preprocess(pil))
    t_b, t_c = alternating(lambda: ops.resample_u8_window(fd, size, window, lut), lambda: composed(fd, size, window, lut))
    rows.append((f"VGGT, 8 x 720 x 1280 -> {nh} x {tw}", same, t_host, t_b, t_c))

    # CLIP: one frame of 480 x 832
    frame = scene(1, 480, 832, seed=1)
    pil1 = Image.fromarray(frame[0])
    want = clip.preprocess(pil1, CLIP_CONFIG)
    f1 = torch.from_numpy(frame).to(dev)
    nw, nh1, top, left = clip._resized_and_window(832, 480, 224, 224)
    table = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (3, 256, 1))
    lut1 = torch.from_numpy(np.ascontiguousarray(clip._rescale_normalize(table, 1 / 255, CLIP_CONFIG["image_mean"], CLIP_CONFIG["image_std"])[:, :, 0])).to(dev)
    size1, window1 = (nh1, nw), (top, left, 224, 224)
    same1 = (torch.equal(clip.preprocess_device(pil1, CLIP_CONFIG, dev).cpu(), want) and
             torch.equal(ops.resample_u8_window(f1, size1, window1, lut1)[0].cpu(), want) and torch.equal(composed(f1, size1, window1, lut1)[0].cpu(), want))
    t_host1 = wall(lambda: clip.preprocess(pil1, CLIP_CONFIG))
    t_b1, t_c1 = alternating(lambda: ops.resample_u8_window(f1, size1, window1, lut1), lambda: composed(f1, size1, window1, lut1))
    rows.append((f"CLIP, 1 x 480 x 832 -> {nh1} x {nw} -> the 224 x 224 at ({top}, {left})", same1, t_host1, t_b1, t_c1))

    lines = ["# Device image preprocessing: the host functions, the window entry, and the earlier entry points composed", "",
             f"`python tools/preprocess_bench.py` on {torch.cuda.get_device_name(0)}, one process.  (a) is wall clock on the host, median of 5 after 1;",
             f"(b) and (c) are HIP events around {INNER} calls, {SAMPLES} samples each after {WARMUP} warm-ups, alternating, per-call milliseconds as median",
             "(min .. max); the u8 frames are on the device before the clock starts and the wrappers' allocations are inside it.", "",
             "| case | results equal | (a) host function | (b) ops.resample_u8_window | (c) resample_u8 + slice + u8_lut_planar |", "|---|---|---|---|---|"]
    for name, ok, h, b, c in rows:
        lines.append(f"| {name} | **{ok}** | {h[0]:.2f} ({h[1]:.2f} .. {h[2]:.2f}) | {b[0]:.4f} ({b[1]:.4f} .. {b[2]:.4f}) | {c[0]:.4f} ({c[1]:.4f} .. {c[2]:.4f}) |")
        notes.append(f"- {name}: {verdict(b, c)}  Host function / (b): {h[0] / b[0]:.0f} x (the host figure has no upload in it, (b) no decode).")
    lines += ["", *notes, "",
              "These are times of whole wrapper calls (allocation and launches included); kernel-only times were not measured.  No speed is gated",
              "on these figures.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
