"""Time the native UMT5 encoder (worldforge_amd/umt5.py) at the released size and write profiles/umt5_encode.md.

    python tools/umt5_bench.py [--tokens 512] [--kv-len 512] [--iters 5] [--warmup 2] [--no-hf]

24 layers, d_model 4096, 64 heads x 64, d_ff 10240, vocab 256384, random bf16 weights generated on the device, one 512-token prompt.
Timed with HIP events after warm-up; peak device memory from the allocator.  When `transformers` imports, the route of
encode_with_transformers (the Hugging Face module in bfloat16 on the device, the SAME weights) is timed on the same box, the two
alternating call by call, and the rel-L2 between the two outputs is reported.  Nothing here is a pass condition.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hf_module(model, dev):
    """The Hugging Face UMT5EncoderModel in bf16 on the device holding the native model's weights (no second random init)."""
    from transformers import UMT5Config, UMT5EncoderModel
    c = model.cfg
    cfg = UMT5Config(vocab_size=c.vocab_size, d_model=c.d_model, d_kv=c.d_kv, d_ff=c.d_ff, num_layers=c.num_layers, num_heads=c.num_heads,
                     relative_attention_num_buckets=c.relative_attention_num_buckets,
                     relative_attention_max_distance=c.relative_attention_max_distance, feed_forward_proj="gated-gelu",
                     layer_norm_epsilon=c.layer_norm_epsilon, dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)
    with torch.device("meta"):
        hf = UMT5EncoderModel(cfg)
    hf = hf.to(torch.bfloat16).to_empty(device=dev).eval()
    W, inner, F = model.W, c.inner_dim, c.d_ff
    sd = {"shared.weight": W["embed"], "encoder.embed_tokens.weight": W["embed"], "encoder.final_layer_norm.weight": W["final_ln"]}
    for i in range(c.num_layers):
        b = f"encoder.block.{i}.layer."
        for j, n in enumerate("qkv"):
            sd[f"{b}0.SelfAttention.{n}.weight"] = W[f"{i}.qkv"][j * inner:(j + 1) * inner]
        sd[f"{b}0.SelfAttention.o.weight"] = W[f"{i}.o"]
        sd[f"{b}0.SelfAttention.relative_attention_bias.weight"] = W[f"{i}.bias"].t()
        sd[f"{b}0.layer_norm.weight"], sd[f"{b}1.layer_norm.weight"] = W[f"{i}.ln0"], W[f"{i}.ln1"]
        sd[f"{b}1.DenseReluDense.wi_0.weight"], sd[f"{b}1.DenseReluDense.wi_1.weight"] = W[f"{i}.wi"][:F], W[f"{i}.wi"][F:]
        sd[f"{b}1.DenseReluDense.wo.weight"] = W[f"{i}.wo"]
    own = hf.state_dict()
    hf.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items() if k in own}, strict=True)
    return hf


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--kv-len", type=int, default=512)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--no-hf", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umt5_encode.md"))
    a = ap.parse_args()
    from worldforge_amd import umt5
    dev = torch.device("cuda:0")
    cfg = umt5.UMT5Config(num_layers=a.layers)
    torch.cuda.reset_peak_memory_stats()
    model = umt5.UMT5EncoderModel(cfg, dev).init_random(0)
    weights_gib = torch.cuda.memory_allocated() / 2 ** 30
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, cfg.vocab_size, (1, a.tokens), generator=g)
    mask = torch.zeros(1, a.tokens, dtype=torch.int64)
    mask[0, :a.kv_len] = 1
    ids[0, a.kv_len:] = 0
    native = lambda: model(ids, mask)  # noqa: E731
    for _ in range(a.warmup):
        native()
    torch.cuda.synchronize()
    peak_native = torch.cuda.max_memory_allocated() / 2 ** 30

    hf, hf_note, hf_call = None, None, None
    if not a.no_hf:
        try:
            hf = hf_module(model, dev)
            ids_d, mask_d = ids.to(dev), mask.to(dev)

            def hf_call():
                with torch.no_grad():
                    return hf(ids_d, mask_d).last_hidden_state
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
    name = torch.cuda.get_device_name(0)
    lines = ["# UMT5 text encoder: one prompt at the released size", "",
             f"`python tools/umt5_bench.py --tokens {a.tokens} --kv-len {a.kv_len} --iters {a.iters} --warmup {a.warmup} --layers {a.layers}` on {name}.",
             f"{a.layers} layers, d_model 4096, 64 heads x 64, d_ff 10240, vocab 256384, random bf16 weights ({weights_gib:.2f} GiB on the device), "
             f"{a.tokens} tokens of which {a.kv_len} are not padding.  HIP events around one call, after {a.warmup} warm-up calls; the time includes "
             "the host-side checks of the ids and the mask and the upload of the ids.", "",
             "| route | median ms | min ms | max ms | calls |", "|---|---|---|---|---|",
             f"| native (worldforge_amd/umt5.py) | {statistics.median(t_nat):.2f} | {min(t_nat):.2f} | {max(t_nat):.2f} | {len(t_nat)} |"]
    if t_hf:
        lines.append(f"| transformers UMT5EncoderModel, bf16, same weights, same box, alternating | {statistics.median(t_hf):.2f} | {min(t_hf):.2f} | "
                     f"{max(t_hf):.2f} | {len(t_hf)} |")
        rel = ((y_nat.double() - y_hf.double()).norm() / y_hf.double().norm()).item()
        lines += ["", f"rel-L2 between the two outputs over all {a.tokens} rows: {rel:.3e} (two bf16 evaluations of random weights; the pinned "
                  "accuracy statement is tests/test_gpu_umt5.py)."]
    else:
        lines += ["", f"transformers route: not run ({hf_note or '--no-hf'})."]
    lines += ["", f"Peak device memory: {peak_native:.2f} GiB with the native encoder alone (weights + one call's workspaces); "
              f"{peak_all:.2f} GiB by the end of the run" + (" with the Hugging Face copy of the weights resident too." if hf is not None else "."),
              "", "No ratio is promised and nothing here is a pass condition: the encoder runs once per video."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
