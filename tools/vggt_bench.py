"""Time the native VGGT aggregator + camera head (worldforge_amd/vggt.py) at the released size and write profiles/vggt_encode.md.

    python tools/vggt_bench.py [--iters 5] [--warmup 2]

VGGT-1B (DINOv2 ViT-L/14 with 24 blocks, 24 frame + 24 global blocks at width 1024 = 16 x 64, camera trunk of 4 blocks at width 2048),
`init_random` weights.  S = 1 at 518 x 294 and 518 x 518, S = 8 at 518 x 294.  The parent starts one fresh child process per GPU step, each
under its own time limit, and stops at the first one that fails: (1) the model calls, HIP events around `camera(images)` after warm-up,
median, with each kernel family timed alone at its shape (back-to-back launches on warm inputs); (2) wf_vit_attn_fwd alone at the frame
shape and the global shape with its TFLOP/s (4 nseq H L^2 64 flop) beside F.scaled_dot_product_attention on the same bf16 tensors in the
same process.  There is no parent-commit figure for a new capability; nothing here is a pass condition.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ((1, 294, 518), (1, 518, 518), (8, 294, 518))


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def per_launch_us(fn, reps=10, rounds=3):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t, _ = timed(lambda: [fn() for _ in range(reps)])
        out.append(t * 1e3 / reps)
    return statistics.median(out)


def child_model(a):
    import torch
    from worldforge_amd import ops, vggt
    from worldforge_amd._ffi import call
    dev = torch.device("cuda:0")
    m = vggt.VGGT(vggt.VGGTConfig(), dev).init_random(0)
    cfg, W, st = m.cfg, m.W, ops.stream()
    res = {"device": torch.cuda.get_device_name(0), "weights_gib": torch.cuda.memory_allocated() / 2 ** 30, "cases": []}
    C, F, H = cfg.embed_dim, cfg.hidden, cfg.num_heads
    for S, Hh, Ww in CASES:
        img = torch.rand(S, 3, Hh, Ww, generator=torch.Generator().manual_seed(S)).to(dev)
        for _ in range(a.warmup):
            m.camera(img)
        torch.cuda.synchronize()
        ts = [timed(lambda: m.camera(img))[0] for _ in range(a.iters)]
        gh, gw = Hh // 14, Ww // 14
        T = 5 + gh * gw
        M = S * T
        bf = torch.bfloat16
        n, qkv, att = (torch.randn(M, k * C, device=dev).to(bf) for k in (1, 3, 1))
        hid, hb, x = torch.randn(M, F, device=dev), torch.randn(M, F, device=dev).to(bf), torch.randn(M, C, device=dev)
        rows = torch.empty(S * gh * gw, vggt.PATCH_K, dtype=bf, device=dev)
        cs, sn, pos, mp = m._rope(gh, gw, S)
        attn = lambda nseq, L: call("wf_vit_attn_fwd", qkv.data_ptr(), qkv.data_ptr() + 2 * C, qkv.data_ptr() + 4 * C, 3 * C, att.data_ptr(), C,  # noqa: E731
                                    nseq, H, L, 0.125, st)
        nb = cfg.dino_depth + 2 * cfg.depth
        parts = [("qkv GEMM", nb, lambda: m._gemm(n, W["f0.qkv.w"], W["f0.qkv.b"], qkv, 0)),
                 ("proj GEMM + LayerScale residual", nb, lambda: m._gemm(att, W["f0.proj.w"], W["f0.proj.b"], x, 3, W["f0.ls1"])),
                 ("fc1 GEMM (f32 out)", nb, lambda: m._gemm(n, W["f0.fc1.w"], W["f0.fc1.b"], hid, 2)),
                 ("GELU-erf (wf_act)", nb, lambda: call("wf_act", hid.data_ptr(), 0, None, 0, hb.data_ptr(), 1, 1, hid.numel(), st)),
                 ("fc2 GEMM + LayerScale residual", nb, lambda: m._gemm(hb, W["f0.fc2.w"], W["f0.fc2.b"], x, 3, W["f0.ls2"])),
                 ("LayerNorm (wf_ln_modulate)", 2 * nb + 1, lambda: m._ln(x, W["f0.norm1.w"], W["f0.norm1.b"], n, 1e-5)),
                 ("wf_vit_attn_fwd, per frame", cfg.dino_depth + cfg.depth, lambda: attn(S, T)),
                 ("wf_vit_attn_fwd, global", cfg.depth, lambda: attn(1, M)),
                 ("wf_vit_qk_norm_rope", 2 * cfg.depth, lambda: call("wf_vit_qk_norm_rope", qkv.data_ptr(), qkv.data_ptr() + 2 * C, 3 * C,
                                                                     W["f0.q_norm.w"].data_ptr(), W["f0.q_norm.b"].data_ptr(), W["f0.k_norm.w"].data_ptr(),
                                                                     W["f0.k_norm.b"].data_ptr(), 1e-5, cs.data_ptr(), sn.data_ptr(), mp, pos.data_ptr(), 1, M, H, 1.0, st)),
                 ("wf_vit_patch_rows", 1, lambda: call("wf_vit_patch_rows", img.data_ptr(), rows.data_ptr(), S, Hh, Ww, st))]
        fam = [(name, count, per_launch_us(fn)) for name, count, fn in parts]
        res["cases"].append({"S": S, "H": Hh, "W": Ww, "tokens": T, "ms": ts, "families": fam, "peak_gib": torch.cuda.max_memory_allocated() / 2 ** 30})
        del n, qkv, att, hid, hb, x
    return res


def child_attn(a):
    import torch
    from worldforge_amd import ops
    from worldforge_amd._ffi import call
    dev, H, C, st = torch.device("cuda:0"), 16, 1024, ops.stream()
    out = []
    for name, nseq, L in (("frame, S = 8 at 518 x 294", 8, 782), ("frame, 518 x 518", 1, 1374), ("global, S = 8 at 518 x 294", 1, 8 * 782)):
        qkv = torch.randn(nseq * L, 3 * C, device=dev).to(torch.bfloat16)
        o = torch.empty(nseq * L, C, dtype=torch.bfloat16, device=dev)
        us = per_launch_us(lambda: call("wf_vit_attn_fwd", qkv.data_ptr(), qkv.data_ptr() + 2 * C, qkv.data_ptr() + 4 * C, 3 * C, o.data_ptr(), C, nseq, H, L, 0.125, st))
        q, k, v = (qkv.view(nseq, L, 3, H, 64)[:, :, i].transpose(1, 2) for i in range(3))
        us_sdpa = per_launch_us(lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v))
        y = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(nseq * L, C)
        rel = ((o.double() - y.double()).norm() / y.double().norm()).item()
        flop = 4.0 * nseq * H * L * L * 64
        out.append({"name": name, "nseq": nseq, "L": L, "us": us, "tf": flop / us / 1e6, "us_sdpa": us_sdpa, "tf_sdpa": flop / us_sdpa / 1e6, "rel": rel})
    return {"attn": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vggt_encode.md"))
    a = ap.parse_args()
    if a.child:
        res = {"model": child_model, "attn": child_attn}[a.child](a)
        with open(a.json, "w") as f:
            json.dump(res, f)
        return 0
    import tempfile
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in (("attn", 180), ("model", 600)):
            p = os.path.join(tmp, step + ".json")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, "--json", p, "--iters", str(a.iters), "--warmup", str(a.warmup)],
                               timeout=limit)
            if r.returncode != 0:
                print(f"step {step} failed with status {r.returncode}: nothing more is started", file=sys.stderr)
                return 1
            with open(p) as f:
                res.update(json.load(f))
    lines = ["# VGGT aggregator + camera head: images in, pose_enc out, at the released size", "",
             f"`python tools/vggt_bench.py --iters {a.iters} --warmup {a.warmup}` on {res['device']}.  VGGT-1B shapes, `init_random` weights "
             f"({res['weights_gib']:.2f} GiB on the device: aggregator linears bf16, the rest fp32).  HIP events around `camera(images)` after "
             f"{a.warmup} warm-up calls, median of {a.iters}.  No parent-commit figure exists for a new capability; nothing here is a pass condition.", "",
             "| S | H x W | tokens per frame | median ms | min ms | max ms | peak GiB |", "|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        lines.append(f"| {c['S']} | {c['H']} x {c['W']} | {c['tokens']} | {statistics.median(c['ms']):.1f} | {min(c['ms']):.1f} | {max(c['ms']):.1f} | {c['peak_gib']:.2f} |")
    for c in res["cases"]:
        lines += ["", f"## Kernel families at S = {c['S']}, {c['H']} x {c['W']} (each alone at its shape, back-to-back launches)", "",
                  "| family | launches per call | us per launch | ms per call |", "|---|---|---|---|"]
        tot = 0.0
        for name, count, us in c["families"]:
            tot += us * count / 1e3
            lines.append(f"| {name} | {count} | {us:.1f} | {us * count / 1e3:.2f} |")
        lines.append(f"\nSum of the parts: {tot:.1f} ms (the call: {statistics.median(c['ms']):.1f} ms; the rest is the camera head, launch gaps and the host).")
    lines += ["", "## wf_vit_attn_fwd alone (16 heads x 64, bf16) beside F.scaled_dot_product_attention on the same tensors, same process", "",
              "| shape | nseq | L | wf_vit_attn_fwd us | TFLOP/s | SDPA us | SDPA TFLOP/s | rel-L2 between the two |", "|---|---|---|---|---|---|---|---|"]
    for r in res["attn"]:
        lines.append(f"| {r['name']} | {r['nseq']} | {r['L']} | {r['us']:.1f} | {r['tf']:.1f} | {r['us_sdpa']:.1f} | {r['tf_sdpa']:.1f} | {r['rel']:.2e} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
