"""Record tests/golden/g24_umt5.npz (+ g24_umt5_y64.npz): a tiny UMT5 encoder as Hugging Face `transformers` evaluates it on the CPU.

    python tools/make_umt5_golden.py

The only place of this repository that imports `transformers`' UMT5 model class for a check: the GPU tests read the file and never
import the package.  Contents: the state dict (bf16 values as their 16 bits), three (ids, mask) cases, the outputs of the module in
bfloat16 (bits; the bar of tests/test_gpu_umt5.py: rel-L2 against the float64 output), `_relative_position_bucket` for rel in
[-600, 600] and the key list of the state dict.  The `UMT5EncoderModel(...).double()` outputs (the yardstick) are float64 and go to
g24_umt5_y64.npz beside it: together the two would pass the 1 MiB a committed file may have.
"""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g24_umt5.npz")
OUT64 = os.path.join(ROOT, "tests", "golden", "g24_umt5_y64.npz")


def bits(t):
    """bf16 values -> their 16 bits (numpy has no bfloat16)."""
    return t.to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


CONFIG = dict(vocab_size=97, d_model=128, d_kv=64, d_ff=192, num_layers=2, num_heads=2, relative_attention_num_buckets=32,
              relative_attention_max_distance=128, feed_forward_proj="gated-gelu", layer_norm_epsilon=1e-6, dropout_rate=0.0,
              is_encoder_decoder=False, use_cache=False, tie_word_embeddings=True)
CASES = ((70, 45), (200, 173), (512, 512))    # (L, kv_len)


def main():
    from transformers import UMT5Config, UMT5EncoderModel
    cfg = UMT5Config(**CONFIG)
    g = torch.Generator().manual_seed(24)
    model = UMT5EncoderModel(cfg).eval()
    sd = {}
    for k, v in model.state_dict().items():
        if k.endswith("relative_attention_bias.weight"):
            t = torch.randn(v.shape, generator=g) * 2.0                     # std ~2: the bias decides who attends to whom
        elif k.endswith("layer_norm.weight"):
            t = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith(("shared.weight", "embed_tokens.weight")):
            t = torch.randn(v.shape, generator=g)
        elif ".SelfAttention." in k and k.endswith((".q.weight", ".k.weight")):
            t = torch.randn(v.shape, generator=g) * (v.shape[1] ** -0.5) * 0.7   # |q.k| of a few units: softmax neither flat nor one-hot
        else:
            t = torch.randn(v.shape, generator=g) * (v.shape[1] ** -0.5)
        sd[k] = t.to(torch.bfloat16).float()
    if "encoder.embed_tokens.weight" in sd:
        sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    model.load_state_dict(sd)
    out = {"config": np.frombuffer(json.dumps(CONFIG).encode(), dtype=np.uint8)}
    out64 = {}
    keys = sorted(k for k in sd if k != "encoder.embed_tokens.weight")
    out["keys"] = np.array(keys)
    for k in keys:
        out["sd." + k] = bits(sd[k])
    m64 = UMT5EncoderModel(cfg).eval().double()
    m64.load_state_dict({k: v.double() for k, v in sd.items()})
    mbf = UMT5EncoderModel(cfg).eval().to(torch.bfloat16)
    mbf.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()})
    for i, (L, n) in enumerate(CASES):
        ids = torch.randint(0, CONFIG["vocab_size"], (1, L), generator=g)
        mask = torch.zeros(1, L, dtype=torch.int64)
        mask[0, :n] = 1
        ids[0, n:] = 0                                                      # the pad id
        with torch.no_grad():
            y64 = m64(ids, mask).last_hidden_state[0]
            ybf = mbf(ids, mask).last_hidden_state[0]
        out[f"ids{i}"], out[f"mask{i}"] = ids[0].numpy().astype(np.int32), mask[0].numpy().astype(np.int32)
        out64[f"y64_{i}"] = y64.numpy()
        out[f"ybf_{i}"] = bits(ybf)
        rel = ((ybf.double() - y64).norm() / y64.norm()).item()
        print(f"case {i}: L {L} kv_len {n}  rel-L2 of the bf16 HF module vs float64: {rel:.4e}")
    attn = m64.encoder.block[0].layer[0].SelfAttention
    rel = torch.arange(-600, 601)
    out["bucket_rel"] = rel.numpy().astype(np.int32)
    out["bucket"] = attn._relative_position_bucket(rel).numpy().astype(np.int32)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    np.savez_compressed(OUT64, **out64)
    for p in (OUT, OUT64):
        print(f"wrote {p} ({os.path.getsize(p)} bytes)")


if __name__ == "__main__":
    main()
