"""Recorder of the VGGT depth-head fixtures (tests/golden/g27_vggt_depth_*): run on a build machine that has the reference's `vggt` package,
never by a test.

    python tools/make_vggt_depth_golden.py --reference <folder that holds the vggt package> [--out tests/golden]

This is the only file of the depth head that imports the reference's `vggt` package; the tests read its files (tests/vggt_depth_cases.py).
It composes the reference's own DPTHead at test width -- DPTHead(dim_in=256, output_dim=2, activation="exp", conf_activation="expp1",
features=64, out_channels=[32, 64, 128, 128]) -- with seeded, bf16-representable weights (dim >= 2: randn x fan_in^-0.5; norm.weight:
1 + 0.1 randn; other 1-D tensors: 0.1 randn) and records
  head-alone cases (S, H, W) = (1, 14, 14), (1, 14, 28), (2, 42, 70), (2, 154, 210) with intermediate_layer_idx = [0, 1, 2, 3]: four
    DISTINCT seeded bf16-representable token tensors (stored as bits), the float64 module's depth and conf, and the rel-L2 against them of
    the float32 module on the same tokens (rel_f32_depth, rel_f32_conf);
  chain cases on the g26 aggregator (tests/golden/g26_vggt_weights*, composed as tools/make_vggt_golden.py composes it) with
    intermediate_layer_idx = [0, 1, 1, 0] on the g26 images of cases 1 and 2: the float64 chain's depth and conf and the rel-L2 of the
    reference's own chain (bf16-autocast aggregator tokens into the float32 head: what run_warp.py runs);
  pieces: _apply_pos_embed on zeros for (C, h, w, W, H) = (32, 1, 1, 14, 14), (32, 3, 5, 70, 42), (64, 154, 210, 210, 154);
    custom_interpolate(align_corners=True) in float64 of a seeded fp32 two-channel map for the size pairs of the resize test; one
    ResidualConvUnit (width 8, 5 x 7, with the in-place ReLU the head builds it with) and one whole FeatureFusionBlock call in float64.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

HEAD_CASES = ((1, 14, 14), (1, 14, 28), (2, 42, 70), (2, 154, 210))
CHAIN_CASES = (1, 2)                      # indices into the g26 cases
POS_CASES = ((32, 1, 1, 14, 14), (32, 3, 5, 70, 42), (64, 154, 210, 210, 154))
RESIZE_CASES = (((1, 1), (1, 2)), ((1, 2), (2, 3)), ((2, 3), (4, 6)), ((6, 8), (11, 15)), ((11, 15), (11, 15)), ((22, 30), (154, 210)))
LIMIT = 900 * 1024
WIDTH = dict(features=64, out_channels=[32, 64, 128, 128])


def bits(t):
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def of_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def seeded(module, g):
    for name, p in module.named_parameters():
        if p.dim() >= 2:
            v = torch.randn(p.shape, generator=g) * (p[0].numel() ** -0.5)
        elif name == "norm.weight":
            v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
        else:
            v = 0.1 * torch.randn(p.shape, generator=g)
        p.data = v.to(torch.bfloat16).to(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from vggt.heads.dpt_head import DPTHead, FeatureFusionBlock, ResidualConvUnit, custom_interpolate
    from vggt.layers.vision_transformer import DinoVisionTransformer
    from vggt.models.aggregator import Aggregator

    out = a.out
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(27)
    head = DPTHead(dim_in=256, output_dim=2, activation="exp", conf_activation="expp1", intermediate_layer_idx=[0, 1, 2, 3], **WIDTH)
    seeded(head, g)
    head.eval()
    head64 = copy.deepcopy(head).double()
    sd = {"depth_head." + k: v for k, v in head.state_dict().items()}
    part, size, parts = {}, 0, []
    for k in sorted(sd):
        n = sd[k].numel() * 2
        if size + n > LIMIT and part:
            parts.append(part)
            part, size = {}, 0
        part["sd." + k], size = bits(sd[k]), size + n
    parts.append(part)
    for i, p in enumerate(parts):
        np.savez(os.path.join(out, f"g27_vggt_depth_weights{i}.npz"), **p)
    meta = {"config": {"depth_features": 64, "depth_out_channels": WIDTH["out_channels"]}, "weight_files": len(parts), "head_cases": [],
            "chain_cases": [], "chain_depth_layers": [0, 1, 1, 0]}

    with torch.no_grad():
        for ci, (S, H, W) in enumerate(HEAD_CASES):
            P = (H // 14) * (W // 14)
            toks = [(torch.randn(1, S, 5 + P, 256, generator=g) * (1.0 + 0.5 * li) + 0.1 * li).to(torch.bfloat16) for li in range(4)]
            img = torch.zeros(1, S, 3, H, W)
            d64, c64 = head64([t.double() for t in toks], img.double(), 5)
            d32, c32 = head([t.float() for t in toks], img, 5)
            np.savez(os.path.join(out, f"g27_vggt_depth_head{ci}_tokens.npz"), **{f"layer{li}": bits(t) for li, t in enumerate(toks)})
            np.savez(os.path.join(out, f"g27_vggt_depth_head{ci}_depth.npz"), depth=d64.numpy())
            np.savez(os.path.join(out, f"g27_vggt_depth_head{ci}_conf.npz"), conf=c64.numpy())
            meta["head_cases"].append({"S": S, "H": H, "W": W, "rel_f32_depth": rel(d32, d64), "rel_f32_conf": rel(c32, c64),
                                       "depth_range": [float(d64.min()), float(d64.max())], "conf_range": [float(c64.min()), float(c64.max())],
                                       "rel_swap_1_2": rel(head64([toks[i].double() for i in (0, 2, 1, 3)], img.double(), 5)[0], d64)})
            print(meta["head_cases"][-1])

        # the chain: the g26 aggregator as tools/make_vggt_golden.py composes it, its recorded weights, kept layers [0, 1, 1, 0]
        with open(os.path.join(out, "g26_vggt_meta.json")) as f:
            m26 = json.load(f)
        sd26 = {}
        for i in range(m26["weight_files"]):
            z = np.load(os.path.join(out, f"g26_vggt_weights{i}.npz"))
            sd26.update({k[3:]: of_bits(z[k]).float() for k in z.files})
        agg = Aggregator(embed_dim=128, depth=2, num_heads=2, patch_embed="conv")
        agg.patch_embed = DinoVisionTransformer(img_size=518, patch_size=14, embed_dim=128, depth=1, num_heads=2, num_register_tokens=4, init_values=1.0,
                                                interpolate_antialias=True, interpolate_offset=0.0, block_chunks=0)
        own = agg.state_dict()
        load = {k[len("aggregator."):]: v for k, v in sd26.items() if k.startswith("aggregator.")}
        load["patch_embed.mask_token"] = own["patch_embed.mask_token"]
        agg.load_state_dict(load, strict=True)
        agg.eval()
        agg64 = copy.deepcopy(agg).double()
        chain, chain64 = copy.deepcopy(head), copy.deepcopy(head64)
        chain.intermediate_layer_idx = chain64.intermediate_layer_idx = [0, 1, 1, 0]
        for ci in CHAIN_CASES:
            u8 = torch.from_numpy(np.load(os.path.join(out, f"g26_vggt_case{ci}.npz"))["images"])
            img = u8.to(torch.float32).div(255)[None]
            t64, start = agg64(img.double())
            with torch.autocast("cpu", dtype=torch.bfloat16):
                tbf, _ = agg(img)
            d64, c64 = chain64(t64, img.double(), start)
            dch, cch = chain([t.float() for t in tbf], img, start)
            np.savez(os.path.join(out, f"g27_vggt_depth_chain{ci}_depth.npz"), depth=d64.numpy())
            np.savez(os.path.join(out, f"g27_vggt_depth_chain{ci}_conf.npz"), conf=c64.numpy())
            meta["chain_cases"].append({"g26_case": ci, "rel_chain_depth": rel(dch, d64), "rel_chain_conf": rel(cch, c64),
                                        "depth_range": [float(d64.min()), float(d64.max())], "conf_range": [float(c64.min()), float(c64.max())]})
            print(meta["chain_cases"][-1])

        pieces = {}
        for i, (C, h, w, W, H) in enumerate(POS_CASES):
            pieces[f"pos{i}"] = head._apply_pos_embed(torch.zeros(1, C, h, w), W, H)[0].numpy()
            pieces[f"pos{i}_shape"] = np.array([C, h, w, W, H])
        np.savez_compressed(os.path.join(out, "g27_vggt_depth_pos.npz"), **pieces)
        pieces = {}
        for i, ((hi, wi), (ho, wo)) in enumerate(RESIZE_CASES):
            x = torch.randn(1, 2, hi, wi, generator=g)
            pieces[f"in{i}"] = x.numpy()
            pieces[f"out{i}"] = custom_interpolate(x.double(), (ho, wo), mode="bilinear", align_corners=True).numpy()
        np.savez(os.path.join(out, "g27_vggt_depth_resize.npz"), **pieces)

        g2 = torch.Generator().manual_seed(28)
        rcu = ResidualConvUnit(8, torch.nn.ReLU(inplace=True), False).double()
        ffb = FeatureFusionBlock(8, torch.nn.ReLU(inplace=True), deconv=False, bn=False, expand=False, align_corners=True, size=None,
                                 has_residual=True).double()
        pieces = {}
        for name, mod in (("rcu", rcu), ("ffb", ffb)):
            for k, p in mod.named_parameters():
                p.data = torch.randn(p.shape, generator=g2, dtype=torch.float64) * (0.3 if p.dim() >= 2 else 0.1)
                pieces[f"{name}.{k}"] = p.data.numpy().copy()
        x = torch.randn(1, 8, 5, 7, generator=g2, dtype=torch.float64)
        pieces["rcu_in"], pieces["rcu_out"] = x.numpy().copy(), rcu(x.clone()).numpy()
        x0, x1 = torch.randn(1, 8, 5, 7, generator=g2, dtype=torch.float64), torch.randn(1, 8, 5, 7, generator=g2, dtype=torch.float64)
        pieces["ffb_in0"], pieces["ffb_in1"] = x0.numpy().copy(), x1.numpy().copy()
        pieces["ffb_out"] = ffb(x0.clone(), x1.clone(), size=(9, 12)).numpy()
        pieces["ffb_size"] = np.array([9, 12])
        np.savez(os.path.join(out, "g27_vggt_depth_units.npz"), **pieces)

    meta["versions"] = {"torch": torch.__version__}
    with open(os.path.join(out, "g27_vggt_depth_meta.json"), "w") as f:
        json.dump(meta, f, indent=0)
    for fn in sorted(os.listdir(out)):
        if fn.startswith("g27_vggt_depth_"):
            n = os.path.getsize(os.path.join(out, fn))
            assert n < 1 << 20, (fn, n)
            print(fn, n)


if __name__ == "__main__":
    main()
