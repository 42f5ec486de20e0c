"""Recorder of the VGGT fixtures (tests/golden/g26_vggt_*): run on a build machine that has the reference's `vggt` package, never by a test.

    python tools/make_vggt_golden.py --reference <folder that holds the vggt package> [--out tests/golden]

This is the only file that imports the reference's `vggt` package; the tests read its files.  It composes the reference's own classes at
test width -- Aggregator(embed_dim 128, depth 2, 2 heads) whose patch_embed is a DinoVisionTransformer(embed_dim 128, depth 1, 2 heads,
4 registers, LayerScale 1.0, antialiased interpolation, offset 0, block_chunks 0 as the aggregator builds it) on the released position
table size (518 / 14), and CameraHead(dim_in 256, trunk_depth 1, 2 heads = 128-wide heads as released) -- with seeded, non-trivial,
bf16-representable weights, and records per case (S, H, W):
    the images (uint8; the model input is uint8 / 255 in fp32), the kept token tensors of the float64 module (one file per layer),
    the rel-L2 against them of the same module under torch.autocast("cpu", bfloat16) and in float32,
    pose_enc in float64, from the fp32 head on the bf16-autocast tokens (the chain run_warp.py runs) and from the fp32 head on the
    float64 tokens, and the matrices pose_encoding_to_extri_intri returns for the chain's pose_enc.
For `preprocess`: two uint8 images and what load_and_preprocess_images returns for them (stored as round(255 x): ToTensor's output is
uint8 / 255).  torchvision is not needed: where it is absent, `torchvision.transforms.ToTensor` is replaced by its definition for uint8
HWC images.  And the key names and shapes of VGGT(enable_point=False, enable_track=False).state_dict() at the released size.
"""
import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

CASES = ((1, 56, 84), (3, 56, 84), (2, 154, 210))
LIMIT = 900 * 1024


def bits(t):
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def seeded(module, g, fov_bias=None):
    for name, p in module.named_parameters():
        s, parts = p.shape, [""] + name.split(".")
        if parts[-1] == "gamma":
            v = 0.3 + 0.05 * torch.randn(s, generator=g)
        elif "norm" in parts[-2] and parts[-1] == "weight":
            v = 1.0 + 0.1 * torch.randn(s, generator=g)
        elif name.endswith("weight") and p.dim() >= 2:
            v = torch.randn(s, generator=g) * (p[0].numel() ** -0.5)
        elif name.endswith("pos_embed"):
            v = 0.2 * torch.randn(s, generator=g)
        elif "token" in parts[-1]:
            v = 0.5 * torch.randn(s, generator=g)
        else:
            v = 0.1 * torch.randn(s, generator=g)
        if fov_bias is not None and name == "pose_branch.fc2.bias":
            v[7:] += fov_bias
        p.data = v.to(torch.bfloat16).to(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    try:
        import torchvision  # noqa: F401
    except ImportError:
        tv, tf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")

        class ToTensor:
            def __call__(self, img):
                return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).to(torch.float32).div(255)
        tf.ToTensor, tv.transforms = ToTensor, tf
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tf
    from vggt.heads.camera_head import CameraHead
    from vggt.layers.vision_transformer import DinoVisionTransformer
    from vggt.models.aggregator import Aggregator
    from vggt.models.vggt import VGGT
    from vggt.utils.load_fn import load_and_preprocess_images
    from vggt.utils.pose_enc import pose_encoding_to_extri_intri

    out = a.out
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(26)
    agg = Aggregator(embed_dim=128, depth=2, num_heads=2, patch_embed="conv")
    agg.patch_embed = DinoVisionTransformer(img_size=518, patch_size=14, embed_dim=128, depth=1, num_heads=2, num_register_tokens=4, init_values=1.0,
                                            interpolate_antialias=True, interpolate_offset=0.0, block_chunks=0)
    head = CameraHead(dim_in=256, trunk_depth=1, num_heads=2)
    seeded(agg, g)
    seeded(head, g, fov_bias=1.0)
    agg.eval(), head.eval()
    config = {"embed_dim": 128, "depth": 2, "num_heads": 2, "dino_depth": 1, "dino_num_heads": 2, "camera_trunk_depth": 1, "camera_num_heads": 2}
    sd = {"aggregator." + k: v for k, v in agg.state_dict().items() if k != "patch_embed.mask_token"}
    sd.update({"camera_head." + k: v for k, v in head.state_dict().items()})
    part, size, parts = {}, 0, []
    for k in sorted(sd):
        n = sd[k].numel() * 2
        if size + n > LIMIT and part:
            parts.append(part)
            part, size = {}, 0
        part["sd." + k], size = bits(sd[k]), size + n
    parts.append(part)
    for i, p in enumerate(parts):
        np.savez(os.path.join(out, f"g26_vggt_weights{i}.npz"), **p)

    meta = {"config": config, "weight_files": len(parts), "cases": []}
    import copy
    agg64, head64 = copy.deepcopy(agg).double(), copy.deepcopy(head).double()
    with torch.no_grad():
        for ci, (S, H, W) in enumerate(CASES):
            u8 = torch.randint(0, 256, (S, 3, H, W), generator=g, dtype=torch.uint8)
            # smooth structure under the noise, so that frames differ in more than noise
            yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
            for s in range(S):
                for c in range(3):
                    base = 127 + 100 * torch.sin(0.05 * (c + 1) * yy + 0.03 * (s + 1) * xx)
                    u8[s, c] = (0.7 * base + 0.3 * u8[s, c].float()).clamp(0, 255).to(torch.uint8)
            img = u8.to(torch.float32).div(255)[None]
            t64, _ = agg64(img.double())
            t32, _ = agg(img)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                tbf, _ = agg(img)
            tbf = [t.float() for t in tbf]
            p64 = head64(t64)[-1]
            p_chain = head([tbf[-1]])[-1]
            p_head32 = head([t64[-1].float()])[-1]
            ext, intr = pose_encoding_to_extri_intri(p_chain, (H, W))
            for li, t in enumerate(t64):
                np.savez(os.path.join(out, f"g26_vggt_case{ci}_layer{li}.npz"), tokens=t.numpy())
            np.savez(os.path.join(out, f"g26_vggt_case{ci}.npz"), images=u8.numpy(), pose64=p64.numpy(), pose_chain=p_chain.numpy(),
                     pose_head32=p_head32.numpy(), extrinsic=ext.numpy(), intrinsic=intr.numpy())
            meta["cases"].append({"S": S, "H": H, "W": W, "rel_bf16": [rel(x, y) for x, y in zip(tbf, t64)],
                                  "rel_f32": [rel(x, y) for x, y in zip(t32, t64)], "pose_rel_chain": rel(p_chain, p64),
                                  "pose_rel_head32": rel(p_head32, p64), "pose_rel_f32": rel(head([t32[-1]])[-1], p64)})
            print(meta["cases"][-1])

    # preprocess: a landscape and a portrait that triggers the crop
    from PIL import Image
    pre = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (w, h) in (("landscape", (500, 300)), ("portrait", (250, 400))):
            yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
            rgb = np.stack([127 + 120 * np.sin(0.04 * xx + 0.02 * yy), 127 + 120 * np.cos(0.03 * yy), (xx * 7 + yy * 3) % 256], -1)
            u8 = rgb.clip(0, 255).astype(np.uint8)
            p = os.path.join(tmp, name + ".png")
            Image.fromarray(u8).save(p)
            y = load_and_preprocess_images([p])
            q = (y * 255).round()
            assert float((q / 255 - y).abs().max()) == 0.0
            pre[name + "_in"], pre[name + "_out"] = u8, q.to(torch.uint8).numpy()
            print(name, tuple(y.shape))
    np.savez_compressed(os.path.join(out, "g26_vggt_preprocess.npz"), **pre)

    # the reference's 2D RoPE on a float64 sample, with the aggregator's positions (special tokens 0, patches + 1) on a 4 x 6 grid
    from vggt.layers.rope import PositionGetter, RotaryPositionEmbedding2D
    g2 = torch.Generator().manual_seed(27)
    x = torch.randn(1, 2, 5 + 24, 64, generator=g2, dtype=torch.float64)
    pos = torch.cat([torch.zeros(1, 5, 2, dtype=torch.long), PositionGetter()(1, 4, 6, device=torch.device("cpu")) + 1], 1)
    np.savez(os.path.join(out, "g26_vggt_rope.npz"), x=x.numpy(), y=RotaryPositionEmbedding2D(frequency=100)(x, pos).numpy(), grid=np.array([4, 6]))

    full = VGGT(enable_point=False, enable_track=False)
    meta["released"] = {k: list(v.shape) for k, v in full.state_dict().items()}
    import PIL
    meta["versions"] = {"torch": torch.__version__, "PIL": PIL.__version__}
    with open(os.path.join(out, "g26_vggt_meta.json"), "w") as f:
        json.dump(meta, f, indent=0)
    for fn in sorted(os.listdir(out)):
        if fn.startswith("g26_vggt_"):
            n = os.path.getsize(os.path.join(out, fn))
            assert n < 1 << 20, (fn, n)
            print(fn, n)


if __name__ == "__main__":
    main()
