"""The LongCat entry point: `python -m worldforge_amd.longcat_infer ...` = the reference's `run_longcat_worldforge_single.py` (RUN:170-500)
on this engine, followed by the chain the engine was built for: guided image-to-video, continuation windows on the resident condition KV
cache, and the block-sparse 720p refine pass with switched LoRAs, all on ONE resident DiT.

    RUN:203-226  tokenizer, UMT5, VAE bf16, scheduler, DiT bf16; the distill LoRA  -> LongCatVideoPipeline.from_pretrained (own safetensors reader,
                                                                                      header check before upload, bf16-first rule), dit.load_lora / enable_loras
    RUN:231-282  warped frames / masks, the input image, size, optional softening  -> harness.read_frames_from_directory / prepare_inputs (wf_soften_mask
                                                                                      on the device); or --stage1 vggt / depthcrafter: stage 1 in this
                                                                                      process (stage1.py) and harness.prepare_inputs_device, no files between
    RUN:284-332  prompts, CPU generator seeded --seed                              -> --embeds, or the folder's tokenizer / text_encoder run once and freed
    RUN:362-385  pipe.generate_i2v(...)                                            -> LongCatVideoPipeline.generate_i2v
    (engine)     --extend-windows N                                                -> N x generate_vc on the previous window's last --num-cond-frames frames
    RUN:441-500  --enable-upscale: refinement LoRA + block-sparse attention        -> dit.load_lora / enable_loras / enable_bsa, generate_refine, then
                                                                                      disable_all_loras / disable_bsa
    RUN:387-436  export                                                            -> harness.save_png_frames (the mp4 container is an external encoder)

Same argument names, defaults and meaning as RUN:503-556.  Stated deviations:
  * Size: the reference looks the size up in a resolution-bucket table by aspect ratio (PIPE:358-372); that table is a settings file of
    the reference and is not copied.  Here the size is --height x --width if given, else harness.prepare_inputs' area rule with the
    480p / 720p pixel budget and multiples of 16 (pick_size).  The two differ on the commonest input: a 16:9 image at 480p gives
    464 x 832 here (round(sqrt(480 * 832 * 9 / 16)) = 474, floored to a multiple of 16) where the reference's table gives 480 x 832;
    `--height 480 --width 832` reproduces the reference.  At 720p a 16:9 image gives 720 x 1280.
  * The scene -> prompt table (--scene) is text of the reference and is not shipped: pass --prompt.  --enable_compile and --fps are
    accepted and do nothing (there is no graph compiler and no video container here); --context_parallel_size must be 1 (sequence
    parallelism is the `comm` of the modules, not wired into this entry).
  * The warped sequence must hold exactly the decoded frame count (as worldforge_amd.infer: the reference blends frame by frame); a
    mismatch is an error before any GPU work.
  * The refine pass is handed `(x * 255).astype(uint8)` of the stage-1 frames (RUN:398) directly, WITHOUT the reference's H.264
    write (RUN:401, crf 10) and read (RUN:454) in between, which is lossy.
  * --extend-windows runs generate_vc with enhance_hf=False: enhance_hf (the reference pipeline's default tail, PIPE:1157-1166) and
    offload_kv_cache are not built, so the reference's default continuation tail is absent.
  * prompt_clean (PIPE:101) uses ftfy when it is importable, else only the HTML-unescape and white-space steps.
Load time and peak host memory on a real checkpoint are NOT MEASURED: no real checkpoint has been available to this project.  For the
same reason the default route through the folder's own tokenizer / text_encoder with the Hugging Face model class
(--text-encoder transformers, encode_with_transformers) has never been run.  --text-encoder native (encode_native) runs the folder's
UMT5 weights on this engine's own kernels instead (worldforge_amd/umt5.py; pinned against the Hugging Face module at test size by
tests/test_gpu_umt5.py); only the tokenizer, data plus a host library, still comes from `transformers`.  Either route encodes BEFORE
the DiT and the VAE are loaded, so that UMT5 and the models are never resident together.
"""
from __future__ import annotations

import argparse
import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from . import harness
from .infer import NEGATIVE_PROMPT_DYNAMIC, NEGATIVE_PROMPT_STATIC

DEFAULT_PROMPT = "A high-quality video with smooth motion and clear details"   # RUN:291


@dataclass
class LongCatRun:
    """What run() hands back: float32 frames in [0, 1] and the PNG directories."""
    frames: np.ndarray                      # [F, H, W, 3]: window 0 followed by every later window's new frames
    png_dir: str
    windows: List[np.ndarray]               # the stage-1 windows as generated, each [num_frames, H, W, 3]
    refined: Optional[np.ndarray] = None    # [F, H', W', 3] with --enable-upscale
    refined_png_dir: Optional[str] = None
    refined_windows: Optional[List[np.ndarray]] = None


def load_embeds(path: str, device, negative: bool) -> Dict[str, torch.Tensor]:
    """`prompt_embeds` [1,1,L,C] + `prompt_attention_mask` [1,L] (and the `negative_` pair when the guidance scale is above 1) from a
    .npz or .safetensors file -> bf16 embeddings and int64 masks on the device."""
    if path.endswith(".npz"):
        z = np.load(path)
        d = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
    else:
        from .checkpoint import load_file
        d = dict(load_file(path))
    need = ["prompt_embeds", "prompt_attention_mask"] + (["negative_prompt_embeds", "negative_prompt_attention_mask"] if negative else [])
    missing = [k for k in need if k not in d]
    if missing:
        raise ValueError(f"{path}: missing {missing} (need {need})")
    out = {}
    for k in need:
        emb = k.endswith("_embeds")
        t = d[k].to(torch.float32).to(torch.bfloat16) if emb else d[k].to(torch.int64)
        if t.dim() != (4 if emb else 2) or t.shape[0] != 1:
            raise ValueError(f"{path}: {k} is {tuple(t.shape)}, expected {'[1, 1, L, C]' if emb else '[1, L]'}")
        out[k] = t.to(device)
    for p in ("", "negative_")[: 2 if negative else 1]:
        if out[p + "prompt_embeds"].shape[2] != out[p + "prompt_attention_mask"].shape[1]:
            raise ValueError(f"{path}: {p}prompt_embeds and {p}prompt_attention_mask disagree on the token count")
    return out


def _prompt_clean(text: str) -> str:
    """PIPE:101 (basic_clean + whitespace_clean)."""
    import html
    import re
    try:
        import ftfy
        text = ftfy.fix_text(text)
    except ImportError:
        pass
    text = html.unescape(html.unescape(text)).strip()
    return re.sub(r"\s+", " ", text).strip()


def encode_with_transformers(checkpoint_dir: str, prompt: str, negative_prompt: Optional[str], device, max_sequence_length: int = 512):
    """PIPE:90-187 with the Hugging Face classes the reference itself loads (RUN:203-204), outside the hot path, once per video:
    the padded UMT5 last_hidden_state as [1, 1, 512, C] bf16 plus the tokenizer's attention mask; the encoder is freed afterwards."""
    from transformers import AutoTokenizer, UMT5EncoderModel
    tok = AutoTokenizer.from_pretrained(os.path.join(checkpoint_dir, "tokenizer"), local_files_only=True)
    te = UMT5EncoderModel.from_pretrained(os.path.join(checkpoint_dir, "text_encoder"), torch_dtype=torch.bfloat16, local_files_only=True).to(device)
    out = {}
    for key, text in (("prompt", prompt), ("negative_prompt", negative_prompt)):
        if text is None:
            continue
        t = tok([_prompt_clean(text)], padding="max_length", max_length=max_sequence_length, truncation=True, add_special_tokens=True,
                return_attention_mask=True, return_tensors="pt")
        with torch.no_grad():
            h = te(t.input_ids.to(device), t.attention_mask.to(device)).last_hidden_state.to(torch.bfloat16)
        out[key + "_embeds"] = h.view(1, 1, h.shape[1], -1)
        out[key + "_attention_mask"] = t.attention_mask.to(device)
    del te
    if torch.device(device).type == "cuda":
        torch.cuda.empty_cache()
    return out


def encode_native(checkpoint_dir: str, prompt: str, negative_prompt: Optional[str], device, max_sequence_length: int = 512, tokenizer=None):
    """encode_with_transformers with the encoder of worldforge_amd/umt5.py in place of the Hugging Face model class: the same keys,
    shapes and dtypes ([1, 1, 512, C] bf16 embeddings, all rows, plus the tokenizer's mask), every tensor operation in libwf_hip.so.
    tokenizer: a callable with the Hugging Face tokenizer signature to use instead of the folder's `tokenizer/` (tests)."""
    from . import umt5
    texts = {k: _prompt_clean(v) for k, v in (("prompt", prompt), ("negative_prompt", negative_prompt)) if v is not None}
    out = {}
    for key, (h, mask) in umt5.encode_prompts(checkpoint_dir, texts, device, tokenizer=tokenizer, max_sequence_length=max_sequence_length).items():
        out[key + "_embeds"], out[key + "_attention_mask"] = umt5.to_longcat(h, mask)
    return out


def pick_size(image_height: int, image_width: int, resolution: str = "480p", height: Optional[int] = None, width: Optional[int] = None):
    """(height, width) of stage 1: --height x --width if given, else harness.target_size on the image's aspect ratio with the pixel
    budget of --resolution (480 * 832 or 720 * 1280).  A 16:9 image gives 464 x 832 at 480p (the reference's bucket table: 480 x 832)
    and 720 x 1280 at 720p; see the module docstring."""
    if (height is None) != (width is None):
        raise ValueError("--height and --width go together")
    if height is not None:
        return int(height), int(width)
    return harness.target_size(image_height, image_width, 480 * 832 if resolution == "480p" else 720 * 1280)


def _u8(frames: np.ndarray) -> np.ndarray:
    """RUN:398."""
    return (frames * 255).astype(np.uint8)


def run(checkpoint_dir: Optional[str], video_ref: str, output: str = "output_i2v.mp4", image: Optional[str] = None,
        prompt: Optional[str] = None, negative_prompt: Optional[str] = None, embeds: Optional[str] = None, use_distill: bool = False,
        resolution: str = "480p", height: Optional[int] = None, width: Optional[int] = None, num_frames: int = 93,
        num_inference_steps: int = 50, guidance_scale: float = 4.0, seed: int = 42, guided: bool = False, resample_steps: int = 3,
        guide_steps: int = 20, resample_round: int = 20, omega: float = 1.8, omega_resample: float = 1.0, soften_mask: bool = False,
        transition_distance: int = 15, decay_type: str = "sine", use_pca_channel_selection: bool = False, static: bool = False,
        max_replace: Optional[int] = None, save_png: bool = False, enable_upscale: bool = False, t_thresh: float = 0.6,
        upscale_height: int = 704, upscale_width: int = 1280, refine_num_inference_steps: int = 50, extend_windows: int = 0,
        num_cond_frames: int = 13, no_kv_cache: bool = False, refine_kv_cache: bool = False, context_parallel_size: int = 1,
        device: str = "cuda:0", dit_precision: str = "bf16", vae_precision: str = "bf16", flow_backend: str = "farneback",
        components: Optional[dict] = None, text_encoder: str = "transformers", stage1: str = "files", stage1_frames=None,
        save_stage1: Optional[str] = None, **stage1_options) -> LongCatRun:
    """RUN:170-500 plus the continuation chain; see the module docstring.  components: any of {"vae", "scheduler", "dit"} to use
    instead of loading it from `checkpoint_dir` (tests: a synthetic DiT folder beside an injected VAE).  refine_num_inference_steps:
    the reference's fixed 50 (RUN:484), a keyword here so that the chain can be exercised at test sizes.
    stage1 "vggt" / "depthcrafter" (video_ref None), stage1_frames, save_stage1 and the stage-1 options as keywords: as
    worldforge_amd.infer.run -- stage 1 runs in this process before UMT5, the DiT and the VAE are loaded and its frames reach the sampler
    through harness.prepare_inputs_device, bit-identical to the file route's.  Stated deviation: the in-process route keeps stage 1's
    frame order; the file route sorts the file names, which is the same order for fewer than 100 frames and label angles below 100
    degrees."""
    from . import stage1 as stage1_mod
    from .longcat_pipeline import LongCatVideoPipeline

    # ---- everything that can be refused without a device --------------------------------------------------------------------------
    if context_parallel_size != 1:
        raise ValueError("--context_parallel_size must be 1: sequence parallelism is the `comm` of the modules and is not wired into this entry")
    if extend_windows < 0:
        raise ValueError("--extend-windows must be >= 0")
    if text_encoder not in ("transformers", "native"):
        raise ValueError(f"--text-encoder {text_encoder!r}: transformers or native")
    given = dict(components or {})
    if not {"vae", "scheduler", "dit"} <= set(given) or use_distill or enable_upscale:
        if checkpoint_dir is None or not os.path.isdir(checkpoint_dir):
            raise ValueError(f"Checkpoint directory does not exist: {checkpoint_dir}")
    lora_files = {}
    for wanted, key in ((use_distill, "cfg_step_lora"), (enable_upscale, "refinement_lora")):   # RUN:212, 448
        if wanted:
            lora_files[key] = os.path.join(checkpoint_dir, "lora", key + ".safetensors")
            if not os.path.isfile(lora_files[key]):
                raise ValueError(f"LoRA file does not exist: {lora_files[key]}")
    eff_frames = max(num_frames // 4 * 4 + 1 if num_frames % 4 != 1 else num_frames, 1)     # PIPE:700-704
    in_process = stage1 != "files" or stage1_frames is not None
    if in_process:   # the one step up here that needs the device: stage 1 itself, before anything else is loaded
        from PIL import Image
        images_u8, masks_u8 = stage1_mod.frames_for(stage1, stage1_options, eff_frames, torch.device(device), stage1_frames=stage1_frames,
                                                    save_dir=save_stage1)
        n_warped, source = images_u8.shape[0], "stage1_frames" if stage1_frames is not None else f"--stage1 {stage1}"
        first_frame = Image.fromarray(images_u8[0].cpu().numpy(), "RGB") if n_warped else None
    elif stage1_options:
        raise TypeError(f"--stage1 files does not take {sorted(stage1_options)}")
    elif video_ref is None:
        raise ValueError("--stage1 files needs --video-ref")
    else:
        warped, _, first_frame = harness.read_frames_from_directory(video_ref)
        n_warped, source = len(warped), "--video-ref"
    if n_warped != eff_frames:
        raise ValueError(f"{source} holds {n_warped} frames but --num-frames {num_frames} decodes {eff_frames}: the reference blends "
                         "frame by frame")
    if image is not None:
        from PIL import Image
        image = Image.open(image).convert("RGB") if isinstance(image, (str, os.PathLike)) else image
    height, width = pick_size((image or first_frame).height, (image or first_frame).width, resolution, height, width)
    if extend_windows and not 1 <= num_cond_frames < eff_frames:
        raise ValueError(f"--num-cond-frames {num_cond_frames} must leave some of the {eff_frames} frames of a window to generate")
    if use_distill:
        guidance_scale = 1.0                                                                  # RUN:370
    do_cfg = guidance_scale > 1.0
    if negative_prompt is None:                                                               # RUN:321-326
        negative_prompt = NEGATIVE_PROMPT_STATIC if static else NEGATIVE_PROMPT_DYNAMIC
    have_encoder = checkpoint_dir is not None and all(os.path.isdir(os.path.join(checkpoint_dir, d)) for d in ("text_encoder", "tokenizer"))
    if embeds is None and not have_encoder:
        raise ValueError("no --embeds file and no text_encoder / tokenizer folders to compute the prompt embeddings from")

    # ---- prompt (PIPE:90-187), before the models: an --embeds file is read on the host, UMT5 is freed before they are loaded ------
    if embeds is not None:
        emb = load_embeds(embeds, "cpu", negative=do_cfg)
    else:
        try:
            import transformers  # noqa: F401
        except ImportError as e:
            raise ValueError("no --embeds file, and `transformers` is not importable to run the folder's " +
                             ("tokenizer" if text_encoder == "native" else "text encoder")) from e
        encode = encode_native if text_encoder == "native" else encode_with_transformers
        emb = encode(checkpoint_dir, prompt or DEFAULT_PROMPT, negative_prompt if do_cfg else None, torch.device(device))
    text = dict(prompt_embeds=emb["prompt_embeds"], prompt_attention_mask=emb["prompt_attention_mask"],
                negative_prompt_embeds=emb.get("negative_prompt_embeds") if do_cfg else None,
                negative_prompt_attention_mask=emb.get("negative_prompt_attention_mask") if do_cfg else None)

    # ---- models (RUN:203-226) -------------------------------------------------------------------------------------------------------
    dev = torch.device(device)
    pipe = LongCatVideoPipeline.from_pretrained(checkpoint_dir, device=dev, vae_precision=vae_precision, dit_precision=dit_precision,
                                                flow_backend=flow_backend, components=given)
    dit = pipe.dit
    text = {k: (v.to(dev) if v is not None else None) for k, v in text.items()}
    if use_distill:
        dit.load_lora(lora_files["cfg_step_lora"], "cfg_step_lora")
        dit.enable_loras(["cfg_step_lora"])

    # ---- inputs (RUN:231-282) -------------------------------------------------------------------------------------------------------
    prep = dict(model=resolution, num_frames=None, soften=soften_mask, transition_distance=transition_distance, decay_type=decay_type,
                device=dev, image=image, size=(height, width))
    if in_process:
        pil, video, mask, height, width = harness.prepare_inputs_device(images_u8, masks_u8, **prep)
        del images_u8, masks_u8
    else:
        pil, video, mask, height, width = harness.prepare_inputs(video_ref, **prep)
    # ---- stage 1 (RUN:328-385) -------------------------------------------------------------------------------------------------------
    generator = torch.Generator(device="cpu")
    generator.manual_seed(seed)
    sampling = dict(num_frames=num_frames, num_inference_steps=num_inference_steps, use_distill=use_distill, guidance_scale=guidance_scale,
                    generator=generator)
    windows = [pipe.generate_i2v(image=pil, height=height, width=width, **text, **sampling, video_ref=video, mask=mask, guided=guided,
                                 resample_steps=resample_steps, guide_steps=guide_steps, resample_round=resample_round, omega=omega,
                                 omega_resample=omega_resample, use_pca_channel_selection=use_pca_channel_selection, static=static,
                                 max_replace_threshold=max_replace)[0]]
    for _ in range(extend_windows):   # each window continues the last num_cond_frames frames of the one before it
        windows.append(pipe.generate_vc(video=_u8(windows[-1]), height=height, width=width, **text, **sampling,
                                        num_cond_frames=num_cond_frames, use_kv_cache=not no_kv_cache, enhance_hf=False)[0])
    frames = np.concatenate([windows[0]] + [w[num_cond_frames:] for w in windows[1:]], axis=0)

    # ---- export (RUN:387-436) -----------------------------------------------------------------------------------------------------------
    if os.path.isdir(output) or not os.path.splitext(output)[1]:                              # RUN:389-391
        output = os.path.join(output, "output.mp4")
    out_dir = os.path.dirname(output)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    # the mp4 container (RUN:401) is an external encoder: the lossless PNG frames (--save-png in the reference) are this engine's output
    # format and are always written
    result = LongCatRun(frames=frames, png_dir=harness.save_png_frames(frames, output), windows=windows)
    if not enable_upscale:
        return result

    # ---- 720p refine on the same resident DiT (RUN:441-500) ----------------------------------------------------------------------------------
    dit.load_lora(lora_files["refinement_lora"], "refinement_lora")
    dit.enable_loras(["refinement_lora"])
    dit.enable_bsa()
    try:
        first = first_frame.resize((upscale_width, upscale_height))                          # RUN:461-472 (the first warped frame, not --image)
        gen_up = torch.Generator(device="cpu")
        gen_up.manual_seed(seed)                                                              # RUN:475-476
        refine = dict(height=upscale_height, width=upscale_width, prompt_embeds=text["prompt_embeds"],
                      prompt_attention_mask=text["prompt_attention_mask"], num_inference_steps=refine_num_inference_steps, generator=gen_up,
                      spatial_refine_only=True, t_thresh=t_thresh)
        refined = [pipe.generate_refine(stage1_video=_u8(windows[0]), image=first, num_cond_frames=1, **refine)[0]]
        for w in windows[1:]:   # a later window is conditioned on the refined frames before it, as its stage 1 was on the stage-1 frames
            refined.append(pipe.generate_refine(stage1_video=_u8(w), video=_u8(refined[-1]), num_cond_frames=num_cond_frames,
                                                use_kv_cache=refine_kv_cache, **refine)[0])
    finally:
        dit.disable_all_loras()                                                               # RUN:490-491
        dit.disable_bsa()
    result.refined_windows = refined
    result.refined = np.concatenate([refined[0]] + [r[num_cond_frames:] for r in refined[1:]], axis=0)
    base, ext = os.path.splitext(output)
    result.refined_png_dir = harness.save_png_frames(result.refined, f"{base}_720p{ext}")      # RUN:444-445
    return result


def build_parser(video_ref_required: bool = True) -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m worldforge_amd.longcat_infer",
                                 description="WorldForge LongCat-Video guided image-to-video, continuation and 720p refine on MI355X "
                                             "(the reference's run_longcat_worldforge_single.py arguments)")
    # RUN:506-556, same names and defaults
    ap.add_argument("--checkpoint_dir", required=True)
    ap.add_argument("--context_parallel_size", type=int, default=1, help="must be 1")
    ap.add_argument("--enable_compile", action="store_true", help="accepted and ignored")
    ap.add_argument("--use_distill", action="store_true")
    ap.add_argument("--video-ref", required=video_ref_required, default=None)
    ap.add_argument("--image", default=None)
    ap.add_argument("--prompt", default=None)
    ap.add_argument("--scene", default=None, help="accepted and ignored: the reference's scene -> prompt table is not shipped, pass --prompt")
    ap.add_argument("--negative_prompt", default=None)
    ap.add_argument("--resolution", choices=["480p", "720p"], default="480p")
    ap.add_argument("--num-frames", type=int, default=93)
    ap.add_argument("--num-inference-steps", type=int, default=50)
    ap.add_argument("--guidance-scale", type=float, default=4.0)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--fps", type=int, default=15, help="accepted and ignored: PNG frames carry no frame rate")
    ap.add_argument("--guided", action="store_true")
    ap.add_argument("--resample-steps", type=int, default=3)
    ap.add_argument("--guide-steps", type=int, default=20)
    ap.add_argument("--resample-round", type=int, default=20)
    ap.add_argument("--omega", type=float, default=1.8)
    ap.add_argument("--omega_resample", type=float, default=1.0)
    ap.add_argument("--soften-mask", action="store_true")
    ap.add_argument("--transition-distance", type=int, default=15)
    ap.add_argument("--decay-type", choices=["linear", "exponential", "sine", "cosine"], default="sine")
    ap.add_argument("--use-pca-channel-selection", action="store_true")
    ap.add_argument("--static", choices=["True", "False"], default="False")
    ap.add_argument("--max-replace", type=int, default=None)
    ap.add_argument("--output", default="output_i2v.mp4")
    ap.add_argument("--save-png", action="store_true", help="accepted for CLI compatibility: the PNG frames are ALWAYS written")
    ap.add_argument("--enable-upscale", action="store_true")
    ap.add_argument("--t-thresh", type=float, default=0.6)
    # this engine's own
    ap.add_argument("--embeds", default=None, help=".npz / .safetensors with prompt_embeds [1,1,L,C], prompt_attention_mask [1,L] and, for a "
                                                   "guidance scale above 1, the negative_ pair")
    ap.add_argument("--height", type=int, default=None, help="with --width: the size outright instead of the --resolution area rule")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--upscale-height", type=int, default=704)
    ap.add_argument("--upscale-width", type=int, default=1280)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--dit-precision", choices=["bf16", "mxfp8"], default="bf16")
    ap.add_argument("--vae-precision", default="bf16")
    ap.add_argument("--extend-windows", type=int, default=0, help="continue the video by N windows of --num-frames frames (generate_vc)")
    ap.add_argument("--num-cond-frames", type=int, default=13, help="frames of the previous window that condition the next one")
    ap.add_argument("--no-kv-cache", action="store_true", help="continuation without the resident condition KV cache")
    ap.add_argument("--refine-kv-cache", action="store_true", help="refine continued windows on the block-ordered condition cache")
    return ap


def cli_parser() -> argparse.ArgumentParser:
    """build_parser() (the reference's arguments and the engine's own, pinned as a set by tests/test_longcat_checkpoint.py) plus
    --text-encoder and the in-process stage 1 (--stage1, --save-stage1 and the stage-1 commands' options, stage1.py): what the command
    line parses."""
    from . import stage1 as stage1_mod
    ap = build_parser(video_ref_required=False)   # --video-ref is required only with --stage1 files (main checks that)
    stage1_mod.add_arguments(ap)
    ap.add_argument("--text-encoder", choices=["transformers", "native"], default="transformers",
                    help="without --embeds: run the folder's UMT5 through the Hugging Face class (default) or on this engine's own kernels "
                         "(worldforge_amd/umt5.py; the tokenizer still comes from transformers)")
    return ap


def main(argv=None):
    from . import stage1 as stage1_mod
    ap = cli_parser()
    a = ap.parse_args(argv)
    if a.stage1 == "files" and a.video_ref is None:
        ap.error("--stage1 files needs --video-ref")
    for flag, on in (("--enable_compile", a.enable_compile), ("--fps", a.fps != 15), ("--scene", a.scene is not None)):
        if on:
            print(f"note: {flag} is accepted and ignored" + (" (pass --prompt)" if flag == "--scene" else ""))
    r = run(a.checkpoint_dir, a.video_ref, output=a.output, image=a.image, prompt=a.prompt, negative_prompt=a.negative_prompt, embeds=a.embeds,
            use_distill=a.use_distill, resolution=a.resolution, height=a.height, width=a.width, num_frames=a.num_frames,
            num_inference_steps=a.num_inference_steps, guidance_scale=a.guidance_scale, seed=a.seed, guided=a.guided,
            resample_steps=a.resample_steps, guide_steps=a.guide_steps, resample_round=a.resample_round, omega=a.omega,
            omega_resample=a.omega_resample, soften_mask=a.soften_mask, transition_distance=a.transition_distance, decay_type=a.decay_type,
            use_pca_channel_selection=a.use_pca_channel_selection, static=a.static == "True", max_replace=a.max_replace, save_png=a.save_png,
            enable_upscale=a.enable_upscale, t_thresh=a.t_thresh, upscale_height=a.upscale_height, upscale_width=a.upscale_width,
            extend_windows=a.extend_windows, num_cond_frames=a.num_cond_frames, no_kv_cache=a.no_kv_cache, refine_kv_cache=a.refine_kv_cache,
            context_parallel_size=a.context_parallel_size, device=a.device, dit_precision=a.dit_precision, vae_precision=a.vae_precision,
            text_encoder=a.text_encoder, stage1=a.stage1, save_stage1=a.save_stage1, **stage1_mod.options_from_args(a))
    print(f"{len(r.frames)} frames -> {r.png_dir}")
    if r.refined is not None:
        print(f"{len(r.refined)} refined frames -> {r.refined_png_dir}")


if __name__ == "__main__":
    main()
