"""Stage 1 from the command line: an image folder in, the warped guidance frames out (vggt/run_warp.py on this engine).

    python -m worldforge_amd.run_warp --checkpoint VGGT_DIR --image_path IMAGES --output_path OUT --direction left --degree 20
    python -m worldforge_amd.infer ... --video-ref OUT/warped_images

Every option of the reference's parser keeps its name, default and choices (--conf_single is clamped to [0, 1]); --checkpoint (a folder
with model.safetensors, instead of the Hugging Face download) and --device are added.  Flow (run_warp.py:199-322): the sorted images of
--image_path -> vggt.preprocess -> ONE VGGT.predict -> camera --camera -> its original image through PIL -> vggt.to_image_size ->
warp.warp_single_img -> OUT/warped_images/{warp,mask}_cam{idx}_{direction}_{angle:05.2f}_deg.png + OUT/camera_info.txt.  PNGs are written
with PIL; the reference's warping_video.mp4 is not written."""
from __future__ import annotations

import argparse
import glob
import os
from typing import List, Optional

import numpy as np

DIRECTIONS = ["up", "down", "left", "right", "forward", "backward"]


def add_arguments(p: argparse.ArgumentParser) -> argparse.ArgumentParser:
    """The warp options (run_warp.py's names, defaults and choices), for this command's parser and for any other that carries them."""
    p.add_argument("--camera", type=int, default=0, help="Camera index for single-view warping")
    p.add_argument("--direction", type=str, default="right", choices=DIRECTIONS,
                   help="Camera motion direction: up/down/left/right (orbit around focus point), forward/backward (dolly)")
    p.add_argument("--degree", type=float, default=15.0,
                   help="Rotation angle in degrees (for orbit/pan), or movement percentage (for forward/backward)")
    p.add_argument("--frame_single", type=int, default=24, help="Number of frames to generate")
    p.add_argument("--look_at_depth", type=float, default=1.0,
                   help="Focus depth coefficient (1.0=scene mean depth, <1 closer, >1 farther)")
    p.add_argument("--conf_single", type=float, default=1.0,
                   help="Depth confidence percentile threshold (1.0=use all, 0.8=keep top 80%%)")
    p.add_argument("--crack_depth_threshold", type=float, default=0.1, help="Depth difference threshold for depth-guided crack filling")
    p.add_argument("--crack_max_size", type=int, default=6, help="Maximum crack size to fill (pixels)")
    p.add_argument("--crack_min_neighbors", type=int, default=2, help="Minimum valid neighbors required for crack filling")
    p.add_argument("--depth_segments", type=int, default=8, help="Number of depth segments for layered crack filling")
    p.add_argument("--outlier_min_neighbors", type=int, default=10, help="Minimum neighbors to keep a pixel (fewer = outlier)")
    p.add_argument("--outlier_neighbor_radius", type=int, default=3, help="Search radius for counting neighbors")
    return p


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m worldforge_amd.run_warp", description="Single-View Warping with VGGT")
    p.add_argument("--image_path", type=str, required=True, help="Path to input image directory")
    p.add_argument("--output_path", type=str, default="output_warp", help="Path to output directory")
    add_arguments(p)
    p.add_argument("--checkpoint", type=str, required=True, help="VGGT checkpoint folder: model.safetensors (+ optional config.json)")
    p.add_argument("--device", type=str, default="cuda:0")
    return p


def validate_args(args):
    """run_warp.py:70-80."""
    args.conf_single = max(0.0, min(1.0, args.conf_single))
    args.fill_cracks = True
    args.disable_depth_aware_fill = False
    args.skip_outlier_detection = False
    args.use_fast_outlier_detection = True
    return args


def load_images_from_path(image_path: str) -> List[str]:
    """run_warp.py:83-100."""
    names: List[str] = []
    if not (os.path.exists(image_path) and os.path.isdir(image_path)):
        raise ValueError(f"Directory not found: {image_path}")
    for ext in (".jpg", ".jpeg", ".JPG", ".JPEG", ".PNG", ".png"):
        names.extend(glob.glob(os.path.join(image_path, f"*{ext}")))
    if not names:
        raise ValueError(f"No images found in {image_path}")
    names.sort()
    print(f"Found {len(names)} images")
    return names


def frame_file_names(camera_idx: int, infos) -> List[tuple]:
    """run_warp.py:127-135: (image name, mask name) per frame."""
    out = []
    for info in infos:
        if info["type"] == "original":
            tag = f"cam{camera_idx}_{info.get('direction', 'original')}_00.00_deg.png"
        else:
            tag = f"cam{camera_idx}_{info['direction']}_{info['angle']:05.2f}_deg.png"
        out.append(("warp_" + tag, "mask_" + tag))
    return out


def camera_info_text(camera_idx: int, infos, args) -> str:
    """run_warp.py:111-124."""
    lines = ["Single-View Warping Info:\n", f"Camera Index: {camera_idx}\n", f"Direction: {args.direction}\n",
             f"Angle: {args.degree} degrees\n", f"Frames: {args.frame_single}\n", f"Confidence Threshold: {args.conf_single}\n",
             f"Crack Filling: {'Enabled' if args.fill_cracks else 'Disabled'}\n", "\nFrame List:\n"]
    for i, info in enumerate(infos):
        line = f"{i}: {info['type']}"
        if info["type"] == "single_view_warped":
            line += f" - {info['direction']} {info['angle']:.2f}°"
        lines.append(line + "\n")
    return "".join(lines)


def save_warped_results(images, masks, infos, output_folder: str, camera_idx: int, args) -> str:
    """run_warp.py:103-162 with PIL as the PNG writer: images u8 [F, H, W, 3] (RGB), masks u8 [F, H, W] (0 / 1, written as 0 / 255)."""
    from PIL import Image
    folder = os.path.join(output_folder, "warped_images")
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(output_folder, "camera_info.txt"), "w", encoding="utf-8") as f:
        f.write(camera_info_text(camera_idx, infos, args))
    images, masks = np.asarray(images), np.asarray(masks)
    for img, mask, (iname, mname) in zip(images, masks, frame_file_names(camera_idx, infos)):
        Image.fromarray(img[:, :, :3], "RGB").save(os.path.join(folder, iname))
        Image.fromarray((mask.astype(np.float32) * 255).astype(np.uint8), "L").save(os.path.join(folder, mname))
    print(f"Saved {len(images)} warped views to: {folder}")
    return folder


def warp_frames(args, device=None):
    """run_warp.py:199-300 without the files: validated arguments (image_path, checkpoint, the warp options; `device` overrides
    args.device) -> (images u8 [F, H, W, 3], masks u8 [F, H, W] (0 / 1), infos), the tensors on the device.  args.camera is set to the
    camera actually used.  The VGGT model lives only inside this call."""
    import torch
    from PIL import Image

    from . import vggt, warp
    device = args.device if device is None else device
    print("Loading VGGT model...")
    model = vggt.VGGT.from_pretrained(args.checkpoint, device=device, depth=True)
    names = load_images_from_path(args.image_path)
    if args.camera >= len(names):
        print(f"Warning: camera index {args.camera} out of range, using 0")
        args.camera = 0
    x = vggt.preprocess_device([Image.open(p) for p in names], device)
    print("Running model inference...")
    r = model.predict(x)
    idx = args.camera
    original = np.array(Image.open(names[idx]))
    if original.ndim == 2:
        original = np.stack([original] * 3, -1)
    if original.shape[-1] == 4:
        original = original[..., :3]
    if original.dtype == np.uint8:
        original = original.astype(np.float32) / 255.0
    oh, ow = original.shape[:2]
    depth, conf, K = vggt.to_image_size(r["depth"][0, idx], r["depth_conf"][0, idx], r["intrinsic"][0, idx], tuple(x.shape[-2:]), (oh, ow))
    print(f"Warping camera {idx} in {args.direction} direction...")
    return warp.warp_single_img(
        extrinsic=r["extrinsic"][0, idx].double().cpu().numpy(), intrinsic=K.double().cpu().numpy(),
        image=torch.from_numpy(original.transpose(2, 0, 1)).float(), depth_map=depth.squeeze(-1), depth_conf=conf,
        direction=args.direction, degree=args.degree, conf_threshold=args.conf_single, frame_num=args.frame_single,
        fill_cracks=args.fill_cracks, crack_params=warp.crack_params_from_args(args), look_at_depth=args.look_at_depth,
        depth_segments=args.depth_segments, device=device)


def main(argv: Optional[List[str]] = None) -> int:
    args = validate_args(build_parser().parse_args(argv))
    os.makedirs(args.output_path, exist_ok=True)
    images, masks, infos = warp_frames(args)
    save_warped_results(images.cpu().numpy(), masks.cpu().numpy(), infos, args.output_path, args.camera, args)
    print(f"\nComplete! Results saved to: {args.output_path}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
