"""Synthetic LongCat checkpoint folders for the loader / audit / entry-point tests: the layout of the released folder (dit/ with a
diffusers config.json and safetensors weights, scheduler/scheduler_config.json, lora/*.safetensors) around the tiny model of the
continuation tests, reference-keyed weights from oracle.longcat_dit.random_weights, the `safetensors` package as the writer."""
import json
import os

import torch

from oracle import longcat_dit as olc

KW = dict(hidden_size=256, depth=2, num_heads=2, caption_channels=64, adaln_tembed_dim=32)
# 64-token blocks: the 4 x 8 tokens of a 64 x 128 frame are two blocks per 4 latent frames, so that sparsity 0.5 keeps one of the two
# condition key blocks (one 128-token block would leave int(0.5 * 1) = 0 to select)
BSA = dict(sparsity=0.5, chunk_3d_shape_q=[4, 4, 4], chunk_3d_shape_k=[4, 4, 4])
# what diffusers' ConfigMixin writes around the fields, and the attention switches of the reference class
CONFIG_EXTRA = {"_class_name": "LongCatVideoTransformer3DModel", "_diffusers_version": "0.35.1", "enable_flashattn2": False,
                "enable_flashattn3": True, "enable_xformers": False, "cp_split_hw": None}
SCHEDULER = {"_class_name": "FlowMatchEulerDiscreteScheduler", "_diffusers_version": "0.35.1", "num_train_timesteps": 1000, "shift": 3.0,
             "use_dynamic_shifting": False, "base_shift": 0.5, "max_shift": 1.15, "invert_sigmas": False, "shift_terminal": None,
             "use_karras_sigmas": False, "use_exponential_sigmas": False, "use_beta_sigmas": False, "time_shift_type": "exponential",
             "stochastic_sampling": False}


def weights(seed=3, kw=KW):
    return olc.random_weights(olc.LongCatConfig(**kw), seed=seed)


def write_weights(folder, W, shards=1, stem="diffusion_pytorch_model"):
    """One file, or `shards` files of interleaved keys plus the index."""
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    W = {k: v.contiguous() for k, v in W.items()}
    if shards == 1:
        save_file(W, os.path.join(folder, stem + ".safetensors"), metadata={"format": "pt"})
        return
    names, wm = sorted(W), {}
    for s in range(shards):
        fn = f"{stem}-{s + 1:05d}-of-{shards:05d}.safetensors"
        part = names[s::shards]
        save_file({n: W[n] for n in part}, os.path.join(folder, fn), metadata={"format": "pt"})
        wm.update({n: fn for n in part})
    with open(os.path.join(folder, stem + ".safetensors.index.json"), "w") as f:
        json.dump({"metadata": {"total_size": sum(v.numel() * v.element_size() for v in W.values())}, "weight_map": wm}, f)


def write_dit(root, W, kw=KW, shards=1, config=None, subfolder="dit"):
    folder = os.path.join(root, subfolder)
    write_weights(folder, W, shards)
    cfg = {**CONFIG_EXTRA, "in_channels": 16, "out_channels": 16, "mlp_ratio": 4, "frequency_embedding_size": 256, "patch_size": [1, 2, 2],
           "enable_bsa": False, "bsa_params": None, "text_tokens_zero_pad": False, **kw, **(config or {})}
    with open(os.path.join(folder, "config.json"), "w") as f:
        json.dump(cfg, f)
    return folder


def write_scheduler(root, **over):
    folder = os.path.join(root, "scheduler")
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "scheduler_config.json"), "w") as f:
        json.dump({**SCHEDULER, **over}, f)
    return folder


def write_lora(root, name, sd):
    from safetensors.torch import save_file
    os.makedirs(os.path.join(root, "lora"), exist_ok=True)
    path = os.path.join(root, "lora", name + ".safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, path)
    return path


def bf16_rounded(W):
    return {k: v.to(torch.bfloat16) for k, v in W.items()}
