"""The cost of a LoRA switch on a resident LongCat DiT at the released width (hidden 4096, rank 128), on one MI355X, HIP events throughout.

  1. wf_lora_fold per matrix shape of a block (qkv with 3 and kv_linear with 2 up-blocks, proj / q_linear, the w1 / w3 halves of w13,
     w2, a block's slice of the stacked AdaLN matrix), beside a plain torch.Tensor.copy_ of the same bf16 matrix into a second buffer:
     the copy reads and writes the same bytes and does no arithmetic, so the ratio to it is what the products cost;
  2. one whole enable_loras() over a model of `--depth` blocks (every wrapped Linear of every block carries an adapter), beside copying
     the same matrices.
Every launch is timed on its own (an event pair), after warm-up; the median and the minimum of `--reps` launches are reported.  The
operands of consecutive launches rotate over enough buffers to exceed the 256 MiB Infinity Cache, so that each launch streams from HBM.
Writes the table and the box's identity to profiles/lora_switch.md (or --out) and prints one JSON line.
Usage:  python tools/lora_switch_bench.py [--reps 30] [--depth 4] [--out profiles/lora_switch.md]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from worldforge_amd import ops  # noqa: E402
from worldforge_amd.longcat_dit import LongCatConfig, LongCatVideoTransformer3DModel  # noqa: E402

DEV = torch.device("cuda:0")
C, HD, CT, RANK = 4096, 11008, 512, 128
# (name, rows N, columns K, up-blocks)
SHAPES = [("attn.qkv", 3 * C, C, 3), ("cross_attn.kv_linear", 2 * C, C, 2), ("attn.proj / q_linear / proj", C, C, 1),
          ("ffn.w1 (half of w13)", HD, C, 1), ("ffn.w2", C, HD, 1), ("adaLN_modulation.1 (slice of ada.w)", 6 * C, CT, 1)]
MODULES = [("attn.qkv", 3 * C, C, 3), ("attn.proj", C, C, 1), ("cross_attn.q_linear", C, C, 1), ("cross_attn.kv_linear", 2 * C, C, 2),
           ("cross_attn.proj", C, C, 1), ("ffn.w1", HD, C, 1), ("ffn.w3", HD, C, 1), ("ffn.w2", C, HD, 1), ("adaLN_modulation.1", 6 * C, CT, 1)]
H = "___lorahyphen___"


def each_timed(fns, reps, warmup=3):
    """Median / minimum ms of `reps` launches, each between its own event pair; launch i runs fns[i % len(fns)]."""
    for i in range(warmup * len(fns)):
        fns[i % len(fns)]()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (s, e) in enumerate(ev):
        s.record()
        fns[i % len(fns)]()
        e.record()
    torch.cuda.synchronize()
    ts = [s.elapsed_time(e) for s, e in ev]
    return statistics.median(ts), min(ts)


def shape_rows(reps):
    rows = []
    for name, N, K, nsep in SHAPES:
        nbuf = max(2, (320 << 20) // (4 * N * K) + 1)   # base + out of all buffers together exceed the Infinity Cache
        g = torch.Generator(device=DEV).manual_seed(N + K)
        bases = [(torch.randn(N, K, generator=g, device=DEV) / K ** 0.5).to(torch.bfloat16) for _ in range(nbuf)]
        outs = [torch.empty_like(b) for b in bases]
        U = (torch.randn(N, RANK, generator=g, device=DEV) * 0.3).to(torch.bfloat16)
        D = (torch.randn(nsep * RANK, K, generator=g, device=DEV) / K ** 0.5).to(torch.bfloat16)
        ad = [(U, D, nsep, 0.5)]
        t_f, t_fmin = each_timed([lambda b=b, o=o: ops.lora_fold(b, o, ad) for b, o in zip(bases, outs)], reps)
        t_c, t_cmin = each_timed([lambda b=b, o=o: o.copy_(b) for b, o in zip(bases, outs)], reps)
        byts = 4.0 * N * K
        rows.append(dict(shape=name, N=N, K=K, nsep=nsep, rank=RANK, fold_ms=round(t_f, 4), fold_min_ms=round(t_fmin, 4), copy_ms=round(t_c, 4),
                         copy_min_ms=round(t_cmin, 4), ratio=round(t_f / t_c, 3), fold_gbps=round(byts / t_f / 1e6, 1),
                         copy_gbps=round(byts / t_c / 1e6, 1), fold_tflops=round(2.0 * N * K * RANK / t_f / 1e9, 1)))
        print(f"{name:36s} [{N:6d} x {K:5d}] nsep {nsep}  fold {t_f:7.4f} ms ({rows[-1]['fold_gbps']:6.0f} GB/s)  copy {t_c:7.4f} ms "
              f"({rows[-1]['copy_gbps']:6.0f} GB/s)  ratio {rows[-1]['ratio']:.3f}", flush=True)
        del bases, outs
    return rows


def lora_state(depth, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    sd = {}
    for i in range(depth):
        for mod, o, k, nsep in MODULES:
            n = "lora" + H + f"blocks.{i}.{mod}".replace(".", H)
            sd[n + ".lora_down.weight"] = torch.randn(nsep * RANK, k, generator=g, device=DEV) / k ** 0.5
            if nsep == 1:
                sd[n + ".lora_up.weight"] = torch.randn(o, RANK, generator=g, device=DEV) * 0.3
            else:
                for b in range(nsep):
                    sd[n + f".lora_up.blocks.{b}.weight"] = torch.randn(o // nsep, RANK, generator=g, device=DEV) * 0.3
    return sd


def model_row(depth, reps):
    m = LongCatVideoTransformer3DModel(LongCatConfig(depth=depth), DEV).init_random(seed=1)
    m.load_lora(lora_state(depth, 1), "A")
    m.load_lora(lora_state(depth, 2), "B")
    t_e, t_emin = each_timed([lambda: m.enable_loras(["A"]), lambda: m.enable_loras(["B"])], reps)
    touched = [k for k in m.w if m.w[k] is not m.base_w[k]]
    pairs = [(m.base_w[k], torch.empty_like(m.base_w[k])) for k in touched]

    def copy_all():
        for b, o in pairs:
            o.copy_(b)

    t_c, t_cmin = each_timed([copy_all], reps)
    byts = sum(b.numel() * 2 for b, _ in pairs)
    r = dict(depth=depth, matrices=len(touched), weight_mb=round(byts / 2 ** 20, 1), enable_ms=round(t_e, 3), enable_min_ms=round(t_emin, 3),
             copy_ms=round(t_c, 3), copy_min_ms=round(t_cmin, 3), ratio=round(t_e / t_c, 3), per_block_ms=round(t_e / depth, 3))
    print(f"enable_loras over {depth} blocks ({len(touched)} matrices, {r['weight_mb']} MiB): {t_e:.3f} ms, copies {t_c:.3f} ms, "
          f"ratio {r['ratio']:.3f}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--out", default=os.path.join("profiles", "lora_switch.md"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a switch time is not measured on the CPU")
    props = torch.cuda.get_device_properties(0)
    box = dict(device=props.name, arch=getattr(props, "gcnArchName", ""), cus=props.multi_processor_count, hbm_gib=round(props.total_memory / 2 ** 30),
               torch=torch.__version__, hip=torch.version.hip)
    rows = shape_rows(a.reps)
    mr = model_row(a.depth, a.reps)
    lines = ["# LoRA switch on a resident LongCat DiT: wf_lora_fold against a plain copy (tools/lora_switch_bench.py)", "",
             f"Box: {box['device']} ({box['arch']}, {box['cus']} CUs, {box['hbm_gib']} GiB), torch {box['torch']}, HIP {box['hip']}.  "
             f"Median (minimum) of {a.reps} launches, each between its own HIP events, after warm-up; rank {RANK}; the buffers of "
             "consecutive launches rotate over more than the 256 MiB Infinity Cache.  GB/s = 4 bytes per weight element (2 read, 2 written).", "",
             "| matrix | N x K | up-blocks | fold ms | GB/s | copy_ ms | GB/s | fold / copy | MFMA TFLOP/s |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} | {r['N']} x {r['K']} | {r['nsep']} | {r['fold_ms']:.4f} ({r['fold_min_ms']:.4f}) | {r['fold_gbps']:.0f} | "
                     f"{r['copy_ms']:.4f} ({r['copy_min_ms']:.4f}) | {r['copy_gbps']:.0f} | {r['ratio']:.2f} | {r['fold_tflops']:.0f} |")
    lines += ["", f"One whole `enable_loras` over {mr['depth']} blocks at hidden 4096 ({mr['matrices']} matrices, {mr['weight_mb']} MiB of weights, every "
              f"wrapped Linear with an adapter): {mr['enable_ms']:.3f} ms ({mr['enable_min_ms']:.3f}), {mr['per_block_ms']:.3f} ms per block; copying the same "
              f"matrices with copy_: {mr['copy_ms']:.3f} ms ({mr['copy_min_ms']:.3f}); ratio {mr['ratio']:.2f}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(dict(box=box, shapes=rows, model=mr)))


if __name__ == "__main__":
    main()
