"""Stage 1 for dynamic scenes from the command line: a frame folder and its depth in, warped guidance frames out
(DepthCrafter/warp_depthcrafter.py on this engine).

    python -m worldforge_amd.warp_depthcrafter --video_path FRAMES --depth_npz D.npz --output_path OUT --direction left --degree 15 \
        --enable_edge_filter
    python -m worldforge_amd.infer ... --video-ref OUT/warped/imgs

Every option of the reference's parser (:305-369) keeps its name, default and choices; --device and --depth_npz are added.  Flow
(:371-429, :140-301): the depth comes from --depth_npz or, as in the reference, from OUT/depth_estimation/<name>/*.npz (key `depth`, f32
[T, H, W]) -> the sorted images of --video_path -> warp.warp_depthcrafter_frames -> OUT/warped/imgs/rendered_image_XX.png, mask_XX.png.

Deviations from the reference:
  * the DepthCrafter depth network is not built here: without a depth file the run ends with a message, and the depth-estimation options
    (--unet_path ... --cpu_offload) are accepted for compatibility only;
  * --video_path must be an image folder: a video file is refused (no decoder here);
  * images are read with PIL as RGB (the reference: cv2.imread, PIL only where that fails) and the PNGs are written with PIL; the 8-bit
    conversion of the float image is restated (round half to even of x * 255, saturated);
  * the image files are de-duplicated before they are sorted (on a case-insensitive file system the reference's two globs per extension
    return every file twice), and of several *.npz in the depth folder the first in sorted order is taken (the reference: glob order);
  * video.mp4 and mask.mp4 are not written;
  * --no_antialias selects the resize of torchvision releases before 0.17 (see warp.resize_bilinear)."""
from __future__ import annotations

import argparse
import glob
import os
from typing import List, Optional

import numpy as np

IMAGE_EXTENSIONS = ["*.png", "*.jpg", "*.jpeg", "*.bmp"]
NO_DEPTH = ("no depth file: give --depth_npz PATH or put depth.npz into {folder}.  The DepthCrafter depth network is not built on this "
            "engine; the depth-estimation options (--unet_path, --pre_train_path, --num_inference_steps, --guidance_scale, --window_size, "
            "--overlap, --max_res, --process_length, --target_fps, --seed, --cpu_offload) are accepted for compatibility only.")
NO_VIDEO = "--video_path {path} is not a folder: video files are not read here (no decoder); extract the frames into a folder of images."


def add_arguments(p: argparse.ArgumentParser) -> argparse.ArgumentParser:
    """The warp options (the reference's names, defaults and choices, plus --no_antialias), for this command's parser and for any other
    that carries them."""
    p.add_argument("--direction", type=str, choices=["up", "down", "left", "right"], default="left", help="Warping direction")
    p.add_argument("--degree", type=float, default=15, help="Warping angle in degrees")
    p.add_argument("--look_at_depth", type=float, default=1.0, help="Look at depth multiplier")
    p.add_argument("--zoom", type=str, choices=["zoom_in", "zoom_out", "none"], default="none", help="Zoom mode")
    p.add_argument("--rate", type=float, default=0.8, help="Zoom rate (0.0-1.0)")
    p.add_argument("--stable", action="store_true", help="Enable stable warping (complete transformation in first N frames)")
    p.add_argument("--stable_frame", type=int, default=17, help="Number of frames to complete stable transformation (default: 17)")
    p.add_argument("--enable_edge_filter", action="store_true", help="Enable depth edge filtering to reduce warping artifacts")
    p.add_argument("--edge_threshold", type=float, default=0.1, help="Edge detection threshold (0.0-1.0)")
    p.add_argument("--edge_dilation", type=int, default=3, help="Edge region dilation in pixels")
    p.add_argument("--depth_jump_threshold", type=float, default=0.3, help="Depth discontinuity threshold")
    p.add_argument("--neighbor_check_radius", type=int, default=2, help="Neighbor depth check radius")
    p.add_argument("--no_antialias", action="store_true", help="Resize as torchvision releases before 0.17 do (no antialiasing)")
    return p


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m worldforge_amd.warp_depthcrafter", description="DepthCrafter + 3D Warping Pipeline")
    p.add_argument("--video_path", type=str, required=True, help="Input image sequence directory")
    p.add_argument("--output_path", type=str, default="output", help="Output folder path")
    p.add_argument("--unet_path", type=str, default="tencent/DepthCrafter", help="(compatibility only) DepthCrafter UNet model path")
    p.add_argument("--pre_train_path", type=str, default="stabilityai/stable-video-diffusion-img2vid-xt",
                   help="(compatibility only) Pre-trained model path")
    p.add_argument("--num_inference_steps", type=int, default=5, help="(compatibility only) Number of denoising steps")
    p.add_argument("--guidance_scale", type=float, default=1.0, help="(compatibility only) Guidance scale for inference")
    p.add_argument("--window_size", type=int, default=110, help="(compatibility only) Sliding window size")
    p.add_argument("--overlap", type=int, default=25, help="(compatibility only) Overlap between windows")
    p.add_argument("--max_res", type=int, default=1024, help="(compatibility only) Maximum resolution")
    p.add_argument("--process_length", type=int, default=-1, help="(compatibility only) Process length (-1 for full video)")
    p.add_argument("--target_fps", type=int, default=-1, help="(compatibility only) Target FPS (-1 for original)")
    p.add_argument("--seed", type=int, default=42, help="(compatibility only) Random seed")
    p.add_argument("--cpu_offload", type=str, default="model", choices=["model", "sequential", "none"],
                   help="(compatibility only) CPU offload mode")
    add_arguments(p)
    p.add_argument("--depth_npz", type=str, default=None, help="depth.npz (key `depth`, [T, H, W]) to use instead of OUT/depth_estimation/<name>")
    p.add_argument("--device", type=str, default="cuda:0")
    return p


def find_depth(args) -> str:
    """:377-393 and :156-160, with --depth_npz in front."""
    if args.depth_npz:
        if not os.path.exists(args.depth_npz):
            raise SystemExit(f"--depth_npz {args.depth_npz} does not exist")
        return args.depth_npz
    name = os.path.basename(args.video_path.rstrip("/"))
    folder = os.path.join(args.output_path, "depth_estimation", name)
    found = sorted(glob.glob(os.path.join(folder, "*.npz")))
    if not found:
        raise SystemExit(NO_DEPTH.format(folder=folder))
    return found[0]


def list_frames(video_path: str) -> List[str]:
    """:166-177: the reference's extension list in both cases, de-duplicated, sorted."""
    if not os.path.isdir(video_path):
        raise SystemExit(NO_VIDEO.format(path=video_path))
    names = set()
    for ext in IMAGE_EXTENSIONS:
        names.update(glob.glob(os.path.join(video_path, ext)))
        names.update(glob.glob(os.path.join(video_path, ext.upper())))
    if not names:
        raise FileNotFoundError(f"No images found in {video_path}")
    return sorted(names)


def read_frames(names: List[str]) -> np.ndarray:
    from PIL import Image
    frames = [np.array(Image.open(p).convert("RGB")) for p in names]
    if len({f.shape for f in frames}) != 1:
        raise ValueError(f"the images of a sequence must share one size, got {sorted({f.shape[:2] for f in frames})}")
    return np.stack(frames)


def save_frames(images, masks, folder: str) -> str:
    """:292-294 with PIL as the PNG writer: images u8 [T, H, W, 3] (RGB), masks u8 [T, H, W] (0 / 1, written as 0 / 255)."""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for idx, (img, mask) in enumerate(zip(np.asarray(images), np.asarray(masks))):
        Image.fromarray(img, "RGB").save(os.path.join(folder, f"rendered_image_{idx:02d}.png"))
        Image.fromarray((mask * 255).astype(np.uint8), "L").save(os.path.join(folder, f"mask_{idx:02d}.png"))
    return folder


def warp_frames(args, device=None):
    """:371-429 and :140-291 without the output files: parsed arguments (video_path, depth_npz / output_path, the warp options;
    `device` overrides args.device) -> (images u8 [T, H, W, 3], masks u8 [T, H, W] (0 / 1), infos), the tensors on the device."""
    if args.zoom != "none" and not (0.0 < args.rate <= 1.0):
        raise ValueError(f"Rate must be between 0.0 and 1.0, got {args.rate}")
    names = list_frames(args.video_path)
    depth_path = find_depth(args)
    print(f"Loading depth from: {depth_path}")
    depth = np.load(depth_path)["depth"]
    frames = read_frames(names)
    if frames.shape[0] != depth.shape[0]:
        raise ValueError(f"{frames.shape[0]} images in {args.video_path} but {depth.shape[0]} depth maps in {depth_path}")
    from . import warp
    print(f"Warping {frames.shape[0]} frames...")
    return warp.warp_depthcrafter_frames(
        frames, depth, direction=args.direction, degree=args.degree, look_at_depth=args.look_at_depth, zoom=args.zoom, rate=args.rate,
        stable=args.stable, stable_frame=args.stable_frame, enable_edge_filter=args.enable_edge_filter, edge_threshold=args.edge_threshold,
        edge_dilation=args.edge_dilation, depth_jump_threshold=args.depth_jump_threshold, neighbor_check_radius=args.neighbor_check_radius,
        antialias=not args.no_antialias, device=args.device if device is None else device)


def main(argv: Optional[List[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    images, masks, _ = warp_frames(args)
    folder = save_frames(images.cpu().numpy(), masks.cpu().numpy(), os.path.join(args.output_path, "warped", "imgs"))
    print(f"\nWarping completed!\nResults saved to: {folder}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
