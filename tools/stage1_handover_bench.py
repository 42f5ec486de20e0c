"""The hand-over from stage 1 to the sampler, timed: 81 frames of 720 x 1280 (u8 frames and 0 / 1 masks on the device, as stage 1 returns
them) to the 480p size the size rule gives.  Both routes in one process on one box:

    python tools/stage1_handover_bench.py [--out profiles/stage1_handover.md] [--frames 81]

(a) the file route: the stage-1 PNG writer (device -> host, PIL encode, disk), then harness.prepare_inputs on the folder (PIL decode, 2 F
    PIL resizes on the host, upload, wf_soften_mask) -- wall clock, median of 3 (it takes seconds);
(b) harness.prepare_inputs_device on the same tensors -- wall clock with a device synchronisation, median of 9 after 2 warm-ups;
and ops.resample_u8 alone (HIP events, median of 9 after 2 warm-ups) against its byte count: it reads the input and writes and re-reads the
u8 intermediate and writes the output once each, compared with the same buffers moved by a device copy in the same run.  The outputs
of the two routes are compared (torch.equal) before anything is timed.  No CPU fallback: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from worldforge_amd import harness, ops, warp_depthcrafter  # noqa: E402


def scene(T, h, w, seed=0):
    """Smooth colour frames with noise and masks with a moving hole: PNG sizes and mask softening as on warped frames, not on noise."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    frames = np.empty((T, h, w, 3), np.uint8)
    masks = np.ones((T, h, w), np.uint8)
    for t in range(T):
        base = 127 + 100 * np.sin(xx / 90.0 + 0.1 * t)[..., None] * np.cos(yy / 70.0)[..., None] * np.array([1.0, 0.8, 0.6])
        frames[t] = np.clip(base + g.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
        x0 = w // 8 + 4 * t
        masks[t, h // 5:h // 5 + h // 3, x0:x0 + w // 5] = 0
        masks[t, :, : 2 * t] = 0
        frames[t][masks[t] == 0] = 0
    return frames, masks


def events(fn, reps=9, warmup=2):
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


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage1_handover.md"))
    ap.add_argument("--frames", type=int, default=81)
    ap.add_argument("--src-height", type=int, default=720)
    ap.add_argument("--src-width", type=int, default=1280)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("stage1_handover_bench: no GPU (there is no CPU path to time)")
    T, h, w, dev = a.frames, a.src_height, a.src_width, torch.device(a.device)
    frames, masks = scene(T, h, w)
    fd, md = torch.from_numpy(frames).to(dev), torch.from_numpy(masks).to(dev)
    H, W = harness.target_size(h, w, 480 * 832)
    kw = dict(model="480p", soften=True, device=dev)

    with tempfile.TemporaryDirectory() as tmp:
        def write():
            return warp_depthcrafter.save_frames(fd.cpu().numpy(), md.cpu().numpy(), os.path.join(tmp, "imgs"))

        folder = write()
        want = harness.prepare_inputs(folder, **kw)
        got = harness.prepare_inputs_device(fd, md, **kw)
        same = (torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]) and got[3:] == want[3:] and
                np.array_equal(np.asarray(got[0]), np.asarray(want[0])))
        png_mb = sum(os.path.getsize(os.path.join(folder, n)) for n in os.listdir(folder)) / 1e6
        t_write = wall(write, 3, 0)
        t_read = wall(lambda: harness.prepare_inputs(folder, **kw), 3, 0)
    t_dev = wall(lambda: harness.prepare_inputs_device(fd, md, **kw), 9, 2)
    t_k3 = events(lambda: ops.resample_u8(fd, (H, W)))
    t_k1 = events(lambda: ops.resample_u8(md, (H, W)))
    # what the kernel moves, and the same number of bytes through a device copy in this run (read + write = 2 x the buffer)
    moved = lambda C: T * C * (h * w + 2 * h * W + H * W)  # noqa: E731
    buf = torch.empty(moved(3) // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(buf)
    t_copy = events(lambda: dst.copy_(buf))
    gbs = lambda nbytes, ms: nbytes / ms / 1e6  # noqa: E731

    lines = ["# Stage 1 to the sampler: the file route against the device route", "",
             f"`python tools/stage1_handover_bench.py` on {torch.cuda.get_device_name(0)}: {T} frames of {h} x {w} (u8 frames, 0 / 1 masks, on the",
             f"device) to {H} x {W}, masks softened; both routes in this process.  Outputs of the two routes equal (video_ref, mask, size, image):",
             f"**{same}**.  PNG files of route (a): {png_mb:.1f} MB.", "",
             "| step | median ms | min | max | how |", "|---|---|---|---|---|",
             "| (a) write: device -> host, {0} PNG files | {1:.1f} | {2:.1f} | {3:.1f} | wall clock, 3 runs |".format(2 * T, *t_write),
             "| (a) harness.prepare_inputs(folder): decode, {0} PIL resizes, upload, soften | {1:.1f} | {2:.1f} | {3:.1f} | wall clock, 3 runs |".format(2 * T, *t_read),
             "| (a) total | {0:.1f} | | | sum of the two medians |".format(t_write[0] + t_read[0]),
             "| (b) harness.prepare_inputs_device (tables, 2 x wf_resample_u8, 2 x look-up, soften, first frame to the host) | {0:.2f} | {1:.2f} | {2:.2f} | wall clock + synchronise, 9 runs after 2 |".format(*t_dev),
             "| ops.resample_u8 (wf_resample_u8), frames (C = 3), allocation included | {0:.3f} | {1:.3f} | {2:.3f} | HIP events, 9 runs after 2 |".format(*t_k3),
             "| wf_resample_u8, masks (C = 1) | {0:.3f} | {1:.3f} | {2:.3f} | HIP events, 9 runs after 2 |".format(*t_k1),
             "| device copy of {0:.0f} MB (reads + writes = the frames' byte count) | {1:.3f} | {2:.3f} | {3:.3f} | HIP events, 9 runs after 2 |".format(moved(3) / 2 / 1e6, *t_copy),
             "",
             f"Route (a) / route (b): {(t_write[0] + t_read[0]) / t_dev[0]:.0f} x.",
             f"Bytes wf_resample_u8 moves on the frames (input read, u8 intermediate written and read, output written): {moved(3) / 1e6:.0f} MB -> "
             f"{gbs(moved(3), t_k3[0]):.0f} GB/s; the device copy of the same byte count in this run: {gbs(moved(3), t_copy[0]):.0f} GB/s "
             f"(the kernel reaches {100 * t_copy[0] / t_k3[0]:.0f} % of the copy's rate).  Masks: {moved(1) / 1e6:.0f} MB -> {gbs(moved(1), t_k1[0]):.0f} GB/s.",
             "The kernel loads bytes and stores aligned dwords, one thread per output dword; the event times include the output / workspace allocation",
             "of ops.resample_u8 (the tables are built and uploaded on the first call of a size pair, in the warm-up).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
