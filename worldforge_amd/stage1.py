"""Stage 1 inside the `infer` processes: `--stage1 vggt` (run_warp) and `--stage1 depthcrafter` (warp_depthcrafter) hand their warped
frames and masks to the sampler as device tensors -- no PNG files in between, no second process.  The two-command route
(`--stage1 files`, the default: `--video-ref DIR` holds the files a stage-1 command wrote) stays as it is, and the tensors of the two
routes are bit-identical (harness.prepare_inputs_device).

The options of the two stage-1 commands come in under their own names.  Where both commands have an option of one name (--direction,
--degree, --look_at_depth) the carrying parser holds it once, accepts either command's choices, and the chosen --stage1 supplies the
default and checks the choice.  --frame_single defaults to the frame count the sampler decodes.
Stated deviation: the in-process route keeps stage 1's frame order; the file route sorts the file names, which is the same order for
fewer than 100 frames and label angles below 100 degrees."""
from __future__ import annotations

import argparse
import os
from typing import Dict, Optional

from . import run_warp, warp_depthcrafter

MODES = ("files", "vggt", "depthcrafter")
_COMMANDS = {"vggt": run_warp, "depthcrafter": warp_depthcrafter}
# options of this module's own
_OWN = ("vggt_checkpoint", "image_path", "video_path", "depth_npz")
# The warp options of the two commands as the carrying parser needs them: (name, type -- None for a store_true flag, choices).  Names,
# types and choices repeat the commands' add_arguments; the defaults are NOT repeated, they are read from the command's own parser
# (_defaults).  tests/test_resample_host.py holds this table to the commands' parsers.
_DC_DIRECTIONS = ["up", "down", "left", "right"]
OPTIONS = {
    "vggt": [("camera", int, None), ("direction", str, run_warp.DIRECTIONS), ("degree", float, None), ("frame_single", int, None),
             ("look_at_depth", float, None), ("conf_single", float, None), ("crack_depth_threshold", float, None), ("crack_max_size", int, None),
             ("crack_min_neighbors", int, None), ("depth_segments", int, None), ("outlier_min_neighbors", int, None),
             ("outlier_neighbor_radius", int, None)],
    "depthcrafter": [("direction", str, _DC_DIRECTIONS), ("degree", float, None), ("look_at_depth", float, None),
                     ("zoom", str, ["zoom_in", "zoom_out", "none"]), ("rate", float, None), ("stable", None, None), ("stable_frame", int, None),
                     ("enable_edge_filter", None, None), ("edge_threshold", float, None), ("edge_dilation", int, None),
                     ("depth_jump_threshold", float, None), ("neighbor_check_radius", int, None), ("no_antialias", None, None)],
}


def _defaults(mode: str) -> argparse.Namespace:
    """What the command's own parser gives its warp options when none is passed."""
    return _COMMANDS[mode].add_arguments(argparse.ArgumentParser(add_help=False)).parse_args([])


def option_names(mode: Optional[str] = None):
    """The names of the stage-1 options: of one mode, or of all."""
    names = list(_OWN)
    for m in ([mode] if mode else list(OPTIONS)):
        names += [name for name, _, _ in OPTIONS[m] if name not in names]
    return names


def add_arguments(ap: argparse.ArgumentParser) -> argparse.ArgumentParser:
    """--stage1, --save-stage1, the inputs of the two commands and their warp options (defaults None = the chosen command's own)."""
    ap.add_argument("--stage1", choices=MODES, default="files",
                    help="where the guidance frames come from: the files of --video-ref (default), or stage 1 run in this process: vggt "
                         "(run_warp: --vggt-checkpoint, --image_path) or depthcrafter (warp_depthcrafter: --video_path, --depth_npz)")
    ap.add_argument("--save-stage1", default=None, help="also write the in-process stage-1 frames as PNG files here (inspection only)")
    ap.add_argument("--vggt-checkpoint", default=None, help="--stage1 vggt: VGGT checkpoint folder (run_warp's --checkpoint)")
    ap.add_argument("--image_path", default=None, help="--stage1 vggt: input image directory")
    ap.add_argument("--video_path", default=None, help="--stage1 depthcrafter: input image sequence directory")
    ap.add_argument("--depth_npz", default=None, help="--stage1 depthcrafter: depth.npz (key `depth`, [T, H, W])")
    merged: Dict[str, tuple] = {}
    for mode, table in OPTIONS.items():
        for name, kind, choices in table:
            if name in merged:      # an option both commands have: either command's choices, resolve() checks the chosen one's
                first_mode, _, first = merged[name]
                merged[name] = (f"{first_mode} / {mode}", kind, None if first is None else first + [c for c in choices or [] if c not in first])
            else:
                merged[name] = (mode, kind, None if choices is None else list(choices))
    for name, (modes, kind, choices) in merged.items():
        text = f"--stage1 {modes}: as that command's --{name} (default: the command's own)"
        if kind is None:
            ap.add_argument("--" + name, action="store_true", default=None, help=text)
        else:
            ap.add_argument("--" + name, type=kind, default=None, choices=choices, help=text)
    return ap


def options_from_args(a) -> dict:
    """The stage-1 keywords of run() out of a parsed command line (only what was given)."""
    return {k: getattr(a, k) for k in option_names() if getattr(a, k, None) is not None}


def resolve(mode: str, options: dict, eff_frames: int) -> argparse.Namespace:
    """The argument namespace the chosen stage-1 command would have parsed: its own defaults under the given options; options of the
    other command, unknown names and choices the command does not have are errors."""
    if mode not in _COMMANDS:
        raise ValueError(f"--stage1 {mode!r}: one of {MODES}")
    known = option_names(mode)
    wrong = [k for k in options if k not in known]
    if wrong:
        raise TypeError(f"--stage1 {mode} does not take {wrong} (it takes {known})")
    ns = _defaults(mode)
    for name, _, choices in OPTIONS[mode]:
        v = options.get(name)
        if v is None:
            continue
        if choices is not None and v not in choices:
            raise ValueError(f"--{name} {v!r} with --stage1 {mode}: one of {list(choices)}")
        setattr(ns, name, v)
    if mode == "vggt":
        for need, flag in (("vggt_checkpoint", "--vggt-checkpoint"), ("image_path", "--image_path")):
            if not options.get(need):
                raise ValueError(f"--stage1 vggt needs {flag}")
        ns.checkpoint, ns.image_path = options["vggt_checkpoint"], options["image_path"]
        if options.get("frame_single") is None:
            ns.frame_single = eff_frames
        ns = run_warp.validate_args(ns)
    else:
        for need in ("video_path", "depth_npz"):
            if not options.get(need):
                raise ValueError(f"--stage1 depthcrafter needs --{need} (the DepthCrafter depth network is not built on this engine)")
        ns.video_path, ns.depth_npz, ns.output_path = options["video_path"], options["depth_npz"], None
    return ns


def run(mode: str, options: dict, eff_frames: int, device, save_dir: Optional[str] = None):
    """Run the chosen stage 1 on `device` -> (images u8 [F, H, W, 3], masks u8 [F, H, W] (0 / 1)) on the device.  save_dir: also write
    the PNG files through the command's own writer (nothing reads them back).  The VGGT model is gone when this returns."""
    import torch
    ns = resolve(mode, options, eff_frames)
    ns.device = str(device)
    images, masks, infos = _COMMANDS[mode].warp_frames(ns, device=str(device))
    if save_dir is not None:
        if mode == "vggt":
            ns.output_path = save_dir
            os.makedirs(save_dir, exist_ok=True)
            run_warp.save_warped_results(images.cpu().numpy(), masks.cpu().numpy(), infos, save_dir, ns.camera, ns)
        else:
            warp_depthcrafter.save_frames(images.cpu().numpy(), masks.cpu().numpy(), os.path.join(save_dir, "warped", "imgs"))
    if torch.device(device).type == "cuda":
        torch.cuda.empty_cache()
    return images, masks


def frames_for(mode: str, options: dict, eff_frames: int, device, stage1_frames=None, save_dir: Optional[str] = None):
    """What run() of the two entry points calls: `stage1_frames` = (images_u8, masks_u8) from a caller that already holds the tensors,
    else run(mode, ...)."""
    if stage1_frames is not None:
        if options:
            raise TypeError(f"stage1_frames given: the stage-1 options {sorted(options)} would be ignored")
        images, masks = stage1_frames
        return images, masks
    return run(mode, options, eff_frames, device, save_dir=save_dir)
