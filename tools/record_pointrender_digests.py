"""Record sha256 digests of what the three point-renderer entry points return on tests/pointrender_cases.py:

    python tools/record_pointrender_digests.py --commit <hash of the checkout> [--out tests/golden/g30_pointrender_parent.json]

Uses only warp.points_render, warp.depth_edge_mask, warp.dc_warp_frames and the cases module, so the same file runs on any checkout that has
those three; tests/test_gpu_dynamic_warp.py::test_entry_points_repeat_the_parent recomputes the digests with `compute` and requires
equality with the file recorded from the commit before the entry points came to share their kernels.  No CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pointrender_cases as pc  # noqa: E402


def render_points(c, opt, dev):
    """One POINT_CASES call -> (image f32 [H, W, F], mask u8 [H, W]) as numpy."""
    from worldforge_amd import warp
    drop = torch.from_numpy(c["drop"]).to(dev) if opt["use_drop"] else None
    img, mask = warp.points_render(torch.from_numpy(c["pts"]).to(dev), torch.from_numpy(c["feats"]).to(dev), c["cam"], c["K"], c["size"],
                                   morph=opt["morph"], radius=opt["radius"], drop=drop)
    return img.cpu().numpy(), mask[..., 0].cpu().numpy()


def compute(dev="cuda:0", kinds=("points", "edge", "batch")):
    """-> {case id: {name: sha256}} for the case families in `kinds`."""
    from worldforge_amd import warp
    out = {}
    if "points" in kinds:
        scenes = {}
        for cid, (key, opt) in pc.point_cases().items():
            if key not in scenes:
                scenes[key] = pc.point_scene(key)
            img, mask = render_points(scenes[key], opt, dev)
            out[cid] = {"mask": pc.digest(mask), "image": pc.digest(img)}
    if "edge" in kinds:
        depths = {}
        for cid, (hw, t, p) in pc.edge_cases().items():
            if hw not in depths:
                depths[hw] = torch.from_numpy(pc.edge_depths(*hw)).to(dev)
            out[cid] = {"drop": pc.digest(warp.depth_edge_mask(depths[hw][t], *p).cpu().numpy())}
    if "batch" in kinds:
        for H, W, centred in pc.BATCH_SHAPES:
            rgb, disp, cams, K, Kp, from_ = pc.batch_scene(H, W, centred)
            img8, mask, fimg = warp.dc_warp_frames(torch.from_numpy(rgb).to(dev), torch.from_numpy(disp).to(dev), cams, K, edge_filter_from=from_,
                                                   return_float=True, K_points=Kp)
            out[pc.batch_id(H, W, centred)] = {"image_u8": pc.digest(img8.cpu().numpy()), "mask": pc.digest(mask.cpu().numpy()),
                                               "image_f32": pc.digest(fimg.cpu().numpy())}
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose build is recorded")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g30_pointrender_parent.json"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("record_pointrender_digests: no GPU (the entry points have no CPU path)")
    rec = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "numpy": np.__version__, "digests": compute(a.device)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec['digests'])} cases from {a.commit} -> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
