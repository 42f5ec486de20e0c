"""Record the CLIP vision fixtures under tests/golden/: a tiny CLIPVisionModel and the CLIP image processor as Hugging Face
`transformers` evaluates them on the CPU.

    python tools/make_clip_golden.py

The only place of this repository that imports `transformers`' CLIP classes: the tests read the files and never import the package.

The model keeps the released ViT-H/14's edges at a size that fits the files: hidden 160 = 2 heads x 80, intermediate 320, 3 layers (two
of which `hidden_states[-2]` runs), patch 4 on 64 x 64 = 256 patches + class = 257 tokens; `gelu` and, with the same weights, `quick_gelu`.
Weights are bf16-representable and stored as their 16 bits; the LAST layer and post_layernorm are not stored at all (hidden_states[-2]
does not depend on them; the tests fill them with seeded values).  Files, each below 1 MiB:
    g25_clip_w0.npz       config, key list, embeddings, pre_layrnorm, layer 0
    g25_clip_w1.npz       layer 1
    g25_clip_gelu.npz     pixel_values (fp32, full-precision values), hidden_states[-2] of the module in float64 (the yardstick), the rel-L2
    g25_clip_quick.npz    of the SAME module in float32 and in bfloat16 against it; one file per activation
    g25_clip_pre_img.npz  two uint8 images (300 x 500 and a 400 x 250 portrait; seeded noise on a gradient) + the processor settings
    g25_clip_pre_pv0.npz  the pixel_values CLIPImageProcessorPil returns for them (fp32 [3, 224, 224])
    g25_clip_pre_pv1.npz
"""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PREFIX = "vision_model."

CONFIG = dict(hidden_size=160, intermediate_size=320, num_hidden_layers=3, num_attention_heads=2, image_size=64, patch_size=4,
              hidden_act="gelu", layer_norm_eps=1e-5, num_channels=3, attention_dropout=0.0)
# image_processor/preprocessor_config.json of the released Wan2.1 I2V folders (a CLIPImageProcessor with the OpenAI statistics)
PROCESSOR = dict(crop_size={"height": 224, "width": 224}, do_center_crop=True, do_convert_rgb=True, do_normalize=True, do_rescale=True,
                 do_resize=True, image_mean=[0.48145466, 0.4578275, 0.40821073], image_std=[0.26862954, 0.26130258, 0.27577711],
                 resample=3, rescale_factor=0.00392156862745098, size={"shortest_edge": 224})


def bits(t):
    """bf16 values -> their 16 bits (numpy has no bfloat16)."""
    return t.to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def strip(k):
    return k[len(PREFIX):] if k.startswith(PREFIX) else k


def weights(model, g):
    sd = {}
    for k, v in model.state_dict().items():
        n = strip(k)
        if not v.dtype.is_floating_point:
            continue
        if "layer_norm" in n or "layrnorm" in n or "layernorm" in n:
            t = (1.0 if n.endswith("weight") else 0.0) + 0.1 * torch.randn(v.shape, generator=g)
        elif n.endswith(".bias"):
            t = 0.05 * torch.randn(v.shape, generator=g)
        elif n == "embeddings.class_embedding":
            t = torch.randn(v.shape, generator=g)
        elif n == "embeddings.position_embedding.weight":
            t = 0.5 * torch.randn(v.shape, generator=g)
        elif n == "embeddings.patch_embedding.weight":
            t = torch.randn(v.shape, generator=g) * (v[0].numel() ** -0.5)
        elif n.endswith(("q_proj.weight", "k_proj.weight")):
            t = torch.randn(v.shape, generator=g) * (v.shape[1] ** -0.5) * 2.0     # scores of a few units: softmax neither flat nor one-hot
        else:
            t = torch.randn(v.shape, generator=g) * (v.shape[1] ** -0.5)
        sd[k] = t.to(torch.bfloat16).float()
    return sd


def image(h, w, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([255.0 * xx / (w - 1), 255.0 * yy / (h - 1), 255.0 * (xx + yy) / (h + w - 2)], -1)
    return np.clip(0.7 * base + g.normal(0.0, 30.0, (h, w, 3)) + 20.0, 0, 255).astype(np.uint8)


def main():
    from PIL import Image
    from transformers import CLIPVisionConfig, CLIPVisionModel
    from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil
    os.makedirs(GOLD, exist_ok=True)
    g = torch.Generator().manual_seed(25)
    sd = weights(CLIPVisionModel(CLIPVisionConfig(**CONFIG)).eval(), g)
    last = f"encoder.layers.{CONFIG['num_hidden_layers'] - 1}."
    stored = sorted(strip(k) for k in sd if not strip(k).startswith((last, "post_layernorm.")))
    by = {strip(k): v for k, v in sd.items()}
    w0 = {"config": np.frombuffer(json.dumps(CONFIG).encode(), dtype=np.uint8), "keys": np.array(stored)}
    w1 = {}
    for k in stored:
        (w1 if k.startswith("encoder.layers.1.") else w0)["sd." + k] = bits(by[k])
    np.savez_compressed(os.path.join(GOLD, "g25_clip_w0.npz"), **w0)
    np.savez_compressed(os.path.join(GOLD, "g25_clip_w1.npz"), **w1)

    for name, act in (("gelu", "gelu"), ("quick", "quick_gelu")):
        cfg = CLIPVisionConfig(**{**CONFIG, "hidden_act": act})
        px = torch.randn(1, 3, CONFIG["image_size"], CONFIG["image_size"], generator=g) * 1.2
        outs = {}
        for tag, dt in (("f64", torch.float64), ("f32", torch.float32), ("bf16", torch.bfloat16)):
            m = CLIPVisionModel(cfg).eval().to(dt)
            m.load_state_dict({k: v.to(dt) for k, v in sd.items()}, strict=False)
            with torch.no_grad():
                outs[tag] = m(pixel_values=px.to(dt), output_hidden_states=True).hidden_states[-2][0].double()
        y64 = outs["f64"]
        rel = {t: ((outs[t] - y64).norm() / y64.norm()).item() for t in ("f32", "bf16")}
        print(f"{act}: rel-L2 vs float64: fp32 HF module {rel['f32']:.4e}, bf16 HF module {rel['bf16']:.4e}")
        np.savez_compressed(os.path.join(GOLD, f"g25_clip_{name}.npz"), pixel_values=px[0].numpy(), y64=y64.numpy(),
                            rel_f32=np.float64(rel["f32"]), rel_bf16=np.float64(rel["bf16"]), hidden_act=np.array(act))

    proc = CLIPImageProcessorPil(**PROCESSOR)
    imgs = [image(300, 500, 1), image(400, 250, 2)]
    np.savez_compressed(os.path.join(GOLD, "g25_clip_pre_img.npz"), img0=imgs[0], img1=imgs[1],
                        processor=np.frombuffer(json.dumps(PROCESSOR).encode(), dtype=np.uint8))
    for i, a in enumerate(imgs):
        pv = proc(images=Image.fromarray(a), return_tensors="np")["pixel_values"][0]
        assert pv.dtype == np.float32 and pv.shape == (3, 224, 224), (pv.dtype, pv.shape)
        np.savez_compressed(os.path.join(GOLD, f"g25_clip_pre_pv{i}.npz"), pixel_values=pv)
    for f in sorted(os.listdir(GOLD)):
        if f.startswith("g25_clip"):
            n = os.path.getsize(os.path.join(GOLD, f))
            assert n < 2 ** 20, (f, n)
            print(f"wrote tests/golden/{f} ({n} bytes)")


if __name__ == "__main__":
    main()
