"""Time the native fp32 CLIP vision encoder (worldforge_amd/clip.py) at the released size and write profiles/clip_encode.md.

    python tools/clip_bench.py [--iters 9] [--warmup 3] [--no-hf] [--accuracy-from FILE]

ViT-H/14: 32 layers of which 31 run, hidden 1280 = 16 x 80, intermediate 5120, 257 tokens, seeded fp32 weights generated on the device,
one 224 x 224 image.  HIP events around one call after warm-up, median; the box's wf_calib_mfma figure beside it (what this box sustains
on the matrix pipe, a diagnostic that makes lines from different boxes comparable).  The split by kernel times each kernel alone at its
shape in the encoder (back-to-back launches on warm inputs, median of the per-launch mean), and gives each GEMM shape's share of the
157 TF fp32 matrix peak.  When `transformers` imports, the Hugging Face module in float32 on the device with the SAME weights is timed
in the same process, the two alternating call by call.  Nothing here is a pass condition.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PEAK_TF = 157.0


def hf_module(model, dev):
    """The Hugging Face CLIPVisionModel in fp32 on the device holding the native model's weights (the unused last layer stays at its init)."""
    from transformers import CLIPVisionConfig, CLIPVisionModel
    c = model.cfg
    cfg = CLIPVisionConfig(hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
                           num_attention_heads=c.num_attention_heads, image_size=c.image_size, patch_size=c.patch_size,
                           hidden_act=c.hidden_act, layer_norm_eps=c.layer_norm_eps)
    hf = CLIPVisionModel(cfg).to(torch.float32).to(dev).eval()
    W, C = model.W, c.hidden_size
    own = hf.state_dict()
    pre = "vision_model." if any(k.startswith("vision_model.") for k in own) else ""
    pos = W["pos"].clone()
    cls = own[pre + "embeddings.class_embedding"].to(dev)
    pos[0] -= cls                                   # the native table has the class embedding folded into row 0
    sd = {"embeddings.position_embedding.weight": pos, "embeddings.patch_embedding.weight": W["patch"].view(C, 3, c.patch_size, c.patch_size),
          "pre_layrnorm.weight": W["pre.w"], "pre_layrnorm.bias": W["pre.b"]}
    for i in range(model.n_layers):
        b = f"encoder.layers.{i}."
        for j, n in enumerate("qkv"):
            sd[f"{b}self_attn.{n}_proj.weight"], sd[f"{b}self_attn.{n}_proj.bias"] = W[f"{i}.qkv.w"][j * C:(j + 1) * C], W[f"{i}.qkv.b"][j * C:(j + 1) * C]
        sd[f"{b}self_attn.out_proj.weight"], sd[f"{b}self_attn.out_proj.bias"] = W[f"{i}.o.w"], W[f"{i}.o.b"]
        for j in (1, 2):
            sd[f"{b}layer_norm{j}.weight"], sd[f"{b}layer_norm{j}.bias"] = W[f"{i}.ln{j}.w"], W[f"{i}.ln{j}.b"]
        sd[f"{b}mlp.fc1.weight"], sd[f"{b}mlp.fc1.bias"] = W[f"{i}.fc1.w"], W[f"{i}.fc1.b"]
        sd[f"{b}mlp.fc2.weight"], sd[f"{b}mlp.fc2.bias"] = W[f"{i}.fc2.w"], W[f"{i}.fc2.b"]
    hf.load_state_dict({pre + k: v for k, v in sd.items()}, strict=False)
    return hf


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def per_launch_us(fn, reps=20, rounds=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t, _ = timed(lambda: [fn() for _ in range(reps)])
        out.append(t * 1e3 / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-hf", action="store_true")
    ap.add_argument("--accuracy-from", default=None, help="a text file whose lines are copied into the accuracy section (the GPU tests' printed figures)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_encode.md"))
    a = ap.parse_args()
    from benchlib.measure import box_calib_tflops
    from worldforge_amd import clip, ops
    from worldforge_amd._ffi import call
    dev = torch.device("cuda:0")
    cfg = clip.CLIPVisionConfig()
    torch.cuda.reset_peak_memory_stats()
    model = clip.CLIPVisionModel(cfg, dev).init_random(0)
    weights_gib = torch.cuda.memory_allocated() / 2 ** 30
    px = torch.randn(3, 224, 224, generator=torch.Generator().manual_seed(1)).to(dev)
    native = lambda: model(px)  # noqa: E731
    for _ in range(a.warmup):
        native()
    torch.cuda.synchronize()
    peak_native = torch.cuda.max_memory_allocated() / 2 ** 30
    calib = box_calib_tflops(dev)

    hf, hf_note, hf_call = None, None, None
    if not a.no_hf:
        try:
            hf = hf_module(model, dev)

            def hf_call():
                with torch.no_grad():
                    return hf(pixel_values=px[None], output_hidden_states=True).hidden_states[-2][0]
            for _ in range(a.warmup):
                hf_call()
            torch.cuda.synchronize()
        except Exception as e:   # a measurement aid: say why the comparison is absent and go on
            hf, hf_note = None, f"{type(e).__name__}: {e}"
    t_nat, t_hf, y_nat, y_hf = [], [], None, None
    for _ in range(a.iters):          # alternating, so that clocks and temperature are shared
        t, y_nat = timed(native)
        t_nat.append(t)
        if hf is not None:
            t, y_hf = timed(hf_call)
            t_hf.append(t)
    peak_all = torch.cuda.max_memory_allocated() / 2 ** 30

    # ---- the split by kernel: each kernel alone at its shape
    T, C, F, H, D = cfg.num_tokens, cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.head_dim
    st, W, L = ops.stream(), model.W, model.n_layers
    buf = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    n, qkv, att, hdn, x, rows = buf(T, C), buf(T, 3 * C), buf(T, C), buf(T, F), buf(T, C), buf(T - 1, cfg.patch_dim)
    gemm = lambda xin, w, b, out, epi: model._gemm(xin, w, b, out, epi)  # noqa: E731
    parts = [
        ("patch embedding GEMM", (T - 1, C, cfg.patch_dim), 1, lambda: gemm(rows, W["patch"], None, x[1:], 4)),
        ("q, k, v GEMM (stacked)", (T, 3 * C, C), L, lambda: gemm(n, W["0.qkv.w"], W["0.qkv.b"], qkv, 2)),
        ("out-proj GEMM, F32_ACC", (T, C, C), L, lambda: gemm(att, W["0.o.w"], W["0.o.b"], x, 4)),
        ("fc1 GEMM, GELU", (T, F, C), L, lambda: gemm(n, W["0.fc1.w"], W["0.fc1.b"], hdn, 5)),
        ("fc2 GEMM, F32_ACC", (T, C, F), L, lambda: gemm(hdn, W["0.fc2.w"], W["0.fc2.b"], x, 4)),
        ("attention 16 x 80, L 257", None, L, lambda: call("wf_clip_attn_fwd", qkv.data_ptr(), qkv.data_ptr() + 4 * C, qkv.data_ptr() + 8 * C,
                                                           3 * C, att.data_ptr(), C, H, T, D, D ** -0.5, st)),
        ("LayerNorm C 1280", None, 2 * L + 1, lambda: model._ln(x, W["0.ln1.w"], W["0.ln1.b"], n)),
        ("patch rows", None, 1, lambda: call("wf_clip_patch_rows", px.data_ptr(), rows.data_ptr(), 224, 14, st)),
    ]
    table, total_us = [], 0.0
    for name, shape, count, fn in parts:
        us = per_launch_us(fn)
        total_us += us * count
        tf = 2.0 * shape[0] * shape[1] * shape[2] / (us * 1e-6) / 1e12 if shape else None
        table.append((name, shape, count, us, tf))

    name = torch.cuda.get_device_name(0)
    flop = sum(2.0 * s[0] * s[1] * s[2] * c for _, s, c, _, _ in table if s) + 4.0 * T * T * D * H * L
    med = statistics.median(t_nat)
    lines = ["# CLIP vision encoder (fp32): one image at the released size", "",
             f"`python tools/clip_bench.py --iters {a.iters} --warmup {a.warmup}` on {name}.",
             f"ViT-H/14, {L} of {cfg.num_hidden_layers} layers run (hidden_states[-2]), hidden {C} = {H} x {D}, intermediate {F}, {T} tokens, seeded fp32 "
             f"weights ({weights_gib:.2f} GiB on the device).  Everything is fp32 on v_mfma_f32_32x32x2_f32 (the reference loads this model with "
             f"torch_dtype=float32).  HIP events around one call after {a.warmup} warm-up calls, median of {a.iters}; {flop / 1e12:.3f} TFLOP per image.",
             f"wf_calib_mfma on this box during the run: {calib:.0f} TF (bf16 matrix pipe, register-only stream).", "",
             "| route | median ms | min ms | max ms | calls |", "|---|---|---|---|---|",
             f"| native (worldforge_amd/clip.py) | {med:.3f} | {min(t_nat):.3f} | {max(t_nat):.3f} | {len(t_nat)} |"]
    if t_hf:
        mh = statistics.median(t_hf)
        lines.append(f"| transformers CLIPVisionModel, fp32, same weights, same process, alternating | {mh:.3f} | {min(t_hf):.3f} | {max(t_hf):.3f} | {len(t_hf)} |")
        rel = ((y_nat.double() - y_hf.double()).norm() / y_hf.double().norm()).item()
        lines += ["", f"native / transformers = {med / mh:.2f}.  rel-L2 between the two outputs: {rel:.3e} (two fp32 evaluations of random weights; the "
                  "pinned accuracy statement is tests/test_gpu_clip.py)."]
    else:
        lines += ["", f"transformers route: not run ({hf_note or '--no-hf'})."]
    lines += ["", f"The whole call at {flop / 1e12 / (med * 1e-3):.1f} TF = {100 * flop / 1e12 / (med * 1e-3) / PEAK_TF:.0f} % of the {PEAK_TF:.0f} TF fp32 matrix peak.", "",
              "## Split by kernel (each kernel alone at its shape, back-to-back launches)", "",
              "| kernel | M x N x K | launches per image | us per launch | us per image | TF | share of the 157 TF peak |", "|---|---|---|---|---|---|---|"]
    for nm, shape, count, us, tf in table:
        sh = " x ".join(str(v) for v in shape) if shape else "-"
        lines.append(f"| {nm} | {sh} | {count} | {us:.1f} | {us * count:.0f} | {'-' if tf is None else f'{tf:.1f}'} | {'-' if tf is None else f'{100 * tf / PEAK_TF:.0f} %'} |")
    lines += ["", f"Sum of the parts: {total_us / 1e3:.3f} ms per image (the call itself: {med:.3f} ms; the difference is launch gaps and the host).",
              "", f"Peak device memory: {peak_native:.2f} GiB with the native encoder alone (weights + one call's workspaces); {peak_all:.2f} GiB by the end of "
              "the run" + (" with the Hugging Face copy of the weights resident too." if hf is not None else "."),
              "", "Accuracy on released weights: NOT MEASURED (no checkpoint is available offline).  Nothing here is a pass condition: the encoder "
              "runs once per video."]
    if a.accuracy_from and os.path.exists(a.accuracy_from):
        with open(a.accuracy_from) as f:
            lines += ["", "## Accuracy on the recorded fixture (tests/test_gpu_clip.py, this box)", ""] + ["    " + ln.rstrip() for ln in f if ln.strip()]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
