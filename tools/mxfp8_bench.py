"""bf16 against the opt-in MX-fp8 linear layers on one MI355X, HIP events throughout.

  1. every DiT block GEMM shape: C2 (M = 32 760 tokens, one GPU), the same at M = 4 095 (one of 8 sequence-parallel ranks) and
     LongCat's block shapes (M = 8 190): wf_gemm_bf16 against wf_mx_quant_e4m3 (the activation) + wf_gemm_mxfp8, and the quantizer
     alone in GB/s against the 8 TB/s HBM roofline;
  2. the DiT part of one plain C2 step (a CFG pair of full-depth Wan2.1-I2V-14B forwards, 40 layers, synthetic weights) in both modes.
Prints one line per shape and, last, one JSON line.
Usage:  python tools/mxfp8_bench.py [--reps 20] [--no-step]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from worldforge_amd import dit as wdit, ops  # noqa: E402

DEV = torch.device("cuda:0")
C2 = [("qkv", 15360, 5120), ("o", 5120, 5120), ("ffn.0", 14080, 5120), ("ffn.2", 5120, 13824)]
LONGCAT = [("qkv", 12288, 4096), ("proj", 4096, 4096), ("w13", 22016, 4096), ("w2", 4096, 11008)]
SHAPES = [("C2", 32760, C2), ("C2/8 ranks", 4095, C2), ("LongCat", 8190, LONGCAT)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def gemm_rows(reps):
    rows = []
    for tag, M, shapes in SHAPES:
        for name, N, K in shapes:
            g = torch.Generator(device=DEV).manual_seed(N + K)
            x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
            w = (torch.randn(N, K, generator=g, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
            b = torch.zeros(N, device=DEV)
            out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            mw = wdit.MXWeight.quantize(w)
            xq, xs = ops.mx_quant(x)
            t_bf = timed(lambda: wdit.gemm(x, w, b, out, wdit.EPI_BF16), reps)
            t_mx = timed(lambda: wdit.gemm(x, mw, b, out, wdit.EPI_BF16), reps)  # quantizer + MX GEMM
            t_q = timed(lambda: ops.mx_quant(x, xq, xs), reps)
            t_g = timed(lambda: ops.gemm_mxfp8(xq, xs, mw.q, mw.s, b, out, wdit.EPI_BF16), reps)
            fl = 2.0 * M * N * K
            qbytes = M * K * 2 + M * K + M * K // 32
            r = dict(set=tag, layer=name, M=M, N=N, K=K, bf16_ms=round(t_bf, 4), mxfp8_ms=round(t_mx, 4), quant_ms=round(t_q, 4),
                     mx_gemm_ms=round(t_g, 4), bf16_tflops=round(fl / t_bf / 1e9, 1), mx_gemm_tflops=round(fl / t_g / 1e9, 1),
                     speedup=round(t_bf / t_mx, 3), quant_gbps=round(qbytes / t_q / 1e6, 1))
            print(f"{tag:11s} {name:6s} M={M:6d} N={N:6d} K={K:6d}  bf16 {t_bf:7.3f} ms ({r['bf16_tflops']:6.1f} TF)  mxfp8 {t_mx:7.3f} ms "
                  f"(quant {t_q:6.3f} ms = {r['quant_gbps']:6.0f} GB/s, GEMM {t_g:7.3f} ms = {r['mx_gemm_tflops']:6.1f} TF)  x{r['speedup']:.3f}",
                  flush=True)
            rows.append(r)
            del x, w, out, mw, xq, xs
            torch.cuda.empty_cache()
    return rows


def step_ms(reps):
    """one CFG pair of full-depth forwards at C2 (the DiT work of a plain sampler step) per linear precision"""
    cfg = wdit.DiTConfig.wan_i2v_14b()
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((36, 21, 60, 104), generator=g, device=DEV).bfloat16()
    text, neg = (torch.randn((512, 4096), generator=g, device=DEV).bfloat16() for _ in range(2))
    clip = torch.randn((257, 1280), generator=g, device=DEV).bfloat16()
    res = {}
    bf = wdit.WanTransformer3DModel(cfg, DEV).init_random(seed=0)
    for prec in ("bf16", "mxfp8"):
        m = bf if prec == "bf16" else wdit.WanTransformer3DModel(cfg, DEV, linear_precision="mxfp8")
        if prec == "mxfp8":
            m.w = bf.w  # the same bf16 weights, quantized by the setter
        res[prec] = timed(lambda: m.forward_tokens_pair(x, 500.0, text, neg, clip), reps)
        print(f"C2 plain step (CFG pair of 40-layer forwards), {prec}: {res[prec]:.1f} ms", flush=True)
        if prec == "mxfp8":
            del m
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    rows = gemm_rows(a.reps)
    out = dict(tool="mxfp8_bench", device=torch.cuda.get_device_name(0), gemm=rows,
               c2_speedup_min=min(r["speedup"] for r in rows if r["set"] == "C2"))
    if not a.no_step:
        st = step_ms(a.step_reps)
        out.update(step_bf16_ms=round(st["bf16"], 2), step_mxfp8_ms=round(st["mxfp8"], 2), step_speedup=round(st["bf16"] / st["mxfp8"], 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
