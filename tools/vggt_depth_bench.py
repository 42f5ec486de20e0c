"""Time the native VGGT depth head (worldforge_amd/vggt.py, csrc/dpt.hip) at the released size and write profiles/vggt_depth.md.

    python tools/vggt_depth_bench.py [--iters 9] [--warmup 2] [--out profiles/vggt_depth.md]

VGGT-1B shapes (aggregator width 1024, DPTHead(dim_in 2048, features 256, out_channels 256 / 512 / 1024 / 1024)), `init_random(depth=True)`
weights, 518 x 294, S = 1 and S = 8 (one chunk of 8 frames).  The parent starts ONE fresh child process under its own time limit; the child
times, with HIP events after warm-up, median of --iters: `aggregate(images, keep=depth_layers)` and `depth_from_tokens(tokens)` on its
result (the head's time beside the aggregator's, from the same run), then every wf_conv2d_f32 layer of the head alone at its shape
(back-to-back launches on warm inputs) with its FLOP count (2 x 9 Cin Cout per output pixel) and TFLOP/s, and the other kernel families
of the head.  There is no parent-commit figure for a new capability; nothing here is a pass condition.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.vggt_bench import per_launch_us, timed  # noqa: E402

CASES = ((1, 294, 518), (8, 294, 518))
PEAK_F32_TF = 157.3      # fp32-input MFMA, dense, MI355X


def conv_layers(cfg, gh, gw):
    """[(name, calls per head, Hi, Wi, Cin, Cout, stride, weight key)] of every wf_conv2d_f32 launch of one head."""
    f, oc = cfg.depth_features, cfg.depth_out_channels
    h4, w4 = (gh - 1) // 2 + 1, (gw - 1) // 2 + 1
    sizes = [(4 * gh, 4 * gw), (2 * gh, 2 * gw), (gh, gw), (h4, w4)]
    out = [("resize_layers.3 (stride 2)", 1, gh, gw, oc[3], oc[3], 2, "dpt.down")]
    out += [(f"layer{i + 1}_rn", 1, sizes[i][0], sizes[i][1], oc[i], f, 1, f"dpt.rn{i}") for i in range(4)]
    for i, n in ((3, 2), (2, 4), (1, 4), (0, 4)):
        out.append((f"refinenet{i + 1} RCU convs", n, sizes[i][0], sizes[i][1], f, f, 1, f"dpt.ref{i + 1}.rcu2.c1"))
    out.append(("output_conv1", 1, 8 * gh, 8 * gw, f, f // 2, 1, "dpt.oc1"))
    out.append(("output_conv2.0 + ReLU", 1, 14 * gh, 14 * gw, f // 2, 32, 1, "dpt.oc2"))
    return out


def child(a):
    import torch
    from worldforge_amd import ops, vggt
    from worldforge_amd._ffi import call
    dev = torch.device("cuda:0")
    m = vggt.VGGT(vggt.VGGTConfig(), dev).init_random(0, depth=True)
    cfg, W, st = m.cfg, m.W, ops.stream()
    res = {"device": torch.cuda.get_device_name(0), "weights_gib": torch.cuda.memory_allocated() / 2 ** 30, "cases": []}
    for S, Hh, Ww in CASES:
        gh, gw = Hh // 14, Ww // 14
        img = torch.rand(S, 3, Hh, Ww, generator=torch.Generator().manual_seed(S)).to(dev)
        for _ in range(a.warmup):
            toks, _ = m.aggregate(img, keep=cfg.depth_layers)
            d, c = m.depth_from_tokens(toks, (Hh, Ww))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(d).all()) and bool((c > 1).all())
        t_agg = [timed(lambda: m.aggregate(img, keep=cfg.depth_layers))[0] for _ in range(a.iters)]
        t_head = [timed(lambda: m.depth_from_tokens(toks, (Hh, Ww)))[0] for _ in range(a.iters)]
        t_all = [timed(lambda: m.predict(img))[0] for _ in range(a.iters)]
        convs = []
        for name, count, Hi, Wi, Cin, Cout, stride, key in conv_layers(cfg, gh, gw):
            x = torch.randn(S, Hi, Wi, Cin, device=dev)
            Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
            r = torch.randn(S, Ho, Wo, Cout, device=dev)
            o = torch.empty(S, Ho, Wo, Cout, device=dev)
            b = W.get(key + ".b")
            us = per_launch_us(lambda: call("wf_conv2d_f32", x.data_ptr(), W[key + ".w"].data_ptr(), None if b is None else b.data_ptr(), r.data_ptr(),
                                            o.data_ptr(), S, Hi, Wi, Cin, Cout, stride, 1, 1, 0, st))
            flop = 2.0 * 9 * Cin * Cout * S * Ho * Wo
            convs.append({"name": name, "count": count, "shape": f"{Hi} x {Wi}, {Cin} -> {Cout}", "us": us, "gflop": flop / 1e9, "tf": flop / us / 1e6})
            del x, r, o
        P, D, f = gh * gw, cfg.camera_dim, cfg.depth_features
        x, xn = torch.randn(S * P, D, device=dev), torch.empty(S * P, D, device=dev)
        y = torch.empty(S * P, cfg.depth_out_channels[2], device=dev)
        g0 = torch.empty(S * P, 16 * cfg.depth_out_channels[0], device=dev)
        y0 = torch.randn(S * P, cfg.depth_out_channels[0], device=dev)
        m1 = torch.randn(S, 4 * gh, 4 * gw, f, device=dev)
        o1 = torch.randn(S, 8 * gh, 8 * gw, f // 2, device=dev)
        h2 = torch.randn(S * 14 * gh * 14 * gw, 32, device=dev)
        dd, cc = torch.empty(S * 14 * gh * 14 * gw, device=dev), torch.empty(S * 14 * gh * 14 * gw, device=dev)
        o2 = torch.empty(S * 16 * gh * gw, f, device=dev)

        def tail():
            m._gemm32(m1.view(-1, f), W["dpt.ref1.out.w"], W["dpt.ref1.out.b"], o2, 2)
            m._resize(o2.view(S, 4 * gh, 4 * gw, f), 8 * gh, 8 * gw)
        tabs = m._dpt_tables(f // 2, 14 * gh, 14 * gw, (Hh, Ww))
        fam = [("LayerNorm (wf_ln_modulate) on the patch rows", 4, per_launch_us(lambda: m._ln(x, W["dpt.norm.w"], W["dpt.norm.b"], xn, 1e-5))),
               ("projects[2] (wf_gemm_f32, 2048 -> 1024)", 1, per_launch_us(lambda: m._gemm32(xn, W["dpt.proj2.w"], W["dpt.proj2.b"], y, 4))),
               ("resize_layers[0] ConvTranspose as wf_gemm_f32 (256 -> 16 x 256)", 1,
                per_launch_us(lambda: m._gemm32(y0, W["dpt.up0.w"], W["dpt.up0.b"], g0, 2))),
               ("refinenet1 out_conv (wf_gemm_f32) + resize x 2", 1, per_launch_us(tail)),
               ("resize to 14 gh x 14 gw + position tables", 1, per_launch_us(lambda: m._resize(o1, 14 * gh, 14 * gw, tabs))),
               ("wf_dpt_depth_out", 1, per_launch_us(lambda: call("wf_dpt_depth_out", h2.data_ptr(), W["dpt.oc3.w"].data_ptr(), W["dpt.oc3.b"].data_ptr(),
                                                                  dd.data_ptr(), cc.data_ptr(), h2.shape[0], 32, st)))]
        res["cases"].append({"S": S, "H": Hh, "W": Ww, "agg_ms": t_agg, "head_ms": t_head, "predict_ms": t_all, "convs": convs, "families": fam,
                             "peak_gib": torch.cuda.max_memory_allocated() / 2 ** 30})
        del x, xn, y, g0, y0, m1, o1, o2, h2, dd, cc, toks
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vggt_depth.md"))
    a = ap.parse_args()
    if a.child:
        with open(a.json, "w") as f:
            json.dump(child(a), f)
        return 0
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "depth.json")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--json", p, "--iters", str(a.iters), "--warmup", str(a.warmup)],
                           timeout=420)
        if r.returncode != 0:
            print(f"the timing child failed with status {r.returncode}", file=sys.stderr)
            return 1
        with open(p) as f:
            res = json.load(f)
    med = statistics.median
    lines = ["# VGGT depth head: tokens in, depth and confidence out, at the released size", "",
             f"`python tools/vggt_depth_bench.py --iters {a.iters} --warmup {a.warmup}` on {res['device']}.  VGGT-1B shapes, `init_random(depth=True)` "
             f"weights ({res['weights_gib']:.2f} GiB on the device; the depth head is fp32).  HIP events after {a.warmup} warm-up calls, median of "
             f"{a.iters}; aggregator and head are timed in the same process on the same images, S = 8 as one chunk of 8 frames.  No parent-commit "
             "figure exists for a new capability; nothing here is a pass condition.", "",
             "| S | H x W | aggregate ms | depth head ms | head ms per frame | predict() ms (aggregator + both heads) | peak GiB |", "|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        lines.append(f"| {c['S']} | {c['H']} x {c['W']} | {med(c['agg_ms']):.1f} | {med(c['head_ms']):.2f} (min {min(c['head_ms']):.2f}, max "
                     f"{max(c['head_ms']):.2f}) | {med(c['head_ms']) / c['S']:.2f} | {med(c['predict_ms']):.1f} | {c['peak_gib']:.2f} |")
    for c in res["cases"]:
        lines += ["", f"## wf_conv2d_f32 layer by layer at S = {c['S']} (each alone at its shape, back-to-back launches, with relu_in and a residual)", "",
                  f"TFLOP/s = 2 x 9 Cin Cout x output pixels over the launch time; the fp32-input MFMA peak is {PEAK_F32_TF} TFLOP/s.", "",
                  "| layer | launches per head | map, channels | GFLOP per launch | us per launch | TFLOP/s | share of peak | ms per head |",
                  "|---|---|---|---|---|---|---|---|"]
        tot = gf = 0.0
        for v in c["convs"]:
            tot, gf = tot + v["us"] * v["count"] / 1e3, gf + v["gflop"] * v["count"]
            lines.append(f"| {v['name']} | {v['count']} | {v['shape']} | {v['gflop']:.2f} | {v['us']:.1f} | {v['tf']:.1f} | {100 * v['tf'] / PEAK_F32_TF:.0f} % | "
                         f"{v['us'] * v['count'] / 1e3:.2f} |")
        lines += ["", f"The 3 x 3 convolutions: {gf:.1f} GFLOP and {tot:.2f} ms per head call = {gf / tot:.1f} TFLOP/s over their own time.", "",
                  "| other kernels of the head | launches per head | us per launch |", "|---|---|---|"]
        rest = 0.0
        for name, count, us in c["families"]:
            rest += us * count / 1e3
            lines.append(f"| {name} | {count} | {us:.1f} |")
        lines.append(f"\nThese: {rest:.2f} ms; convolutions + these = {tot + rest:.2f} ms of the head's {med(c['head_ms']):.2f} ms (the rest: the other "
                     "projections, ConvTransposes, out_convs and resizes, the pixel shuffles and adds in torch, launch gaps and the host).")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
