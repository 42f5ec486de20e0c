"""The entry point of the hot path: `python -m worldforge_amd.infer ...` = the reference's `infer_worldforge.py` (INFER:153-339) on this engine.

    INFER:153-156  read the warped frames / masks of --video-ref            -> harness.read_frames_from_directory
                   or --stage1 vggt / depthcrafter: stage 1 in this process  -> stage1.py, harness.prepare_inputs_device (no files between)
    INFER:158-202  model folder, VAE fp32, pipeline bf16, clean scheduler   -> AutoencoderKLWan / WanTransformer3DModel.from_pretrained (own
                                                                               safetensors reader, checkpoint.py), UniPCMultistepScheduler.from_config
    INFER:206-254  size rule, frame / mask resize, optional mask softening  -> harness.prepare_inputs (wf_soften_mask on the device)
    INFER:256-309  prompts, seed 42, pipe(...)                              -> WanImageToVideoPipeline.__call__ (every tensor op in libwf_hip.so)
    INFER:311-339  export                                                   -> harness.save_png_frames (the mp4 container is an external encoder)

Same argument names, defaults and meaning as the reference's CLI.  The UMT5 text encoder and the CLIP vision encoder run once per video and the
loop consumes their outputs.  Those come in through --embeds (a .npz / .safetensors with `prompt_embeds` [1,L,4096], `negative_prompt_embeds`,
`image_embeds` [1,257,1280]) or, when the checkpoint folder holds `text_encoder/`, `tokenizer/`, `image_encoder/`, `image_processor/` and
`transformers` is importable, are computed with those classes exactly as PIPE:166-214 does (--text-encoder transformers --image-encoder
transformers, the defaults).  --text-encoder native runs the UMT5 weights on this engine's own kernels instead (worldforge_amd/umt5.py) and
--image-encoder native the CLIP vision weights, in float32 as the reference loads them (worldforge_amd/clip.py, with the image processor's PIL
path restated bit for bit on the device).  With both native, the only thing of `transformers` that is touched is the tokenizer (data plus a host library).
The reference's scene -> prompt table (utils/prompts.py) is text data of the reference and is not shipped: pass --prompt; the negative
prompt defaults to the entry point's own two literals (INFER:277-285, by --static).
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import harness


# INFER:277-278: the entry point's two negative prompts (protocol constants of the CLI, selected by --static at INFER:280-285)
NEGATIVE_PROMPT_STATIC = "Blink, twinkle, waggle, speak, wind, windy, leaves shaking, leaves tremble, sighboard, background dynamics, dynamic imagery, gray sky, hazy sky, overcast, gloomy sky, dim, murky, smoggy, shake, object motion blur, streaking objects, object jitter, camera shake, time flow, illogical composition, bright tones, overexposed, blurred details, subtitles, text, logo, overall gray, worst quality, low quality, JPEG compression residue, ugly, incomplete, sudden scene shift, incoherent scene jump, extra fingers, poorly drawn hands, poorly drawn faces, deformed, disfigured, misshapen limbs, fused fingers, any movement, character motion, slight object movement, object swaying, character micro-movements, subtle object rotation, object vibration, messy background, three legs, many people in the background, walking, scene changes, visual detail movement, object disintegration, object breakage."
NEGATIVE_PROMPT_DYNAMIC = "Streaking objects, mosaic, grainy, pixelated, noise, flickering, cropped, glitch, fragmented, broken, artifacts, chromatic aberration, micro camera shake, grid, tiling, blurry, camera shake, sudden scene shift, incoherent scene jump, sudden object appearance, blinking, object jitter, camera shake, illogical composition, bright tones, overexposed, blurred details, subtitles, overall gray, solid color, worst quality, low quality, JPEG compression residue, ugly, incomplete, extra fingers, poorly drawn hands, poorly drawn faces, deformed, disfigured, misshapen limbs, fused fingers, messy background, three legs, many people in the background, walking backwards"


def load_embeds(path: str, device) -> Dict[str, torch.Tensor]:
    """prompt_embeds / negative_prompt_embeds / image_embeds from a .npz or .safetensors file -> bf16 device tensors."""
    if path.endswith(".npz"):
        z = np.load(path)
        d = {k: torch.from_numpy(np.asarray(z[k], dtype=np.float32)) for k in z.files}
    else:
        from .checkpoint import load_file
        d = {k: v.float() for k, v in load_file(path).items()}
    need = ("prompt_embeds", "negative_prompt_embeds", "image_embeds")
    missing = [k for k in need if k not in d]
    if missing:
        raise ValueError(f"{path}: missing {missing} (need {need})")
    return {k: d[k].to(torch.bfloat16).to(device) for k in need}


def encode_text_native(model_path: str, prompt: str, negative_prompt: str, device, max_sequence_length: int = 512, tokenizer=None):
    """The text half of encode_with_transformers on this engine's own UMT5 (worldforge_amd/umt5.py): PIPE:167-199, each prompt's own rows
    with exact zeros behind them, [1, 512, C] bf16.  tokenizer: a callable to use instead of the folder's `tokenizer/` (tests)."""
    from . import umt5
    enc = umt5.encode_prompts(model_path, {"prompt_embeds": prompt, "negative_prompt_embeds": negative_prompt}, device, tokenizer=tokenizer,
                              max_sequence_length=max_sequence_length)
    return {k: umt5.to_wan(h, mask, max_sequence_length) for k, (h, mask) in enc.items()}


def encode_with_transformers(model_path: str, prompt: str, negative_prompt: str, image, device, max_sequence_length: int = 512,
                             text_encoder: str = "transformers", image_encoder: str = "transformers"):
    """PIPE:166-214 with the Hugging Face classes the reference itself uses (outside the hot path, once per video): UMT5 last_hidden_state
    truncated to each prompt's length and zero-padded to 512 rows (PIPE:190-199); CLIP vision hidden_states[-2] (PIPE:209-211).
    text_encoder="native": the text half comes from encode_text_native.  image_encoder="native": image_embeds come from clip.encode_image
    and neither CLIPVisionModel nor CLIPImageProcessor is imported; with both native only the tokenizer of `transformers` is used."""
    if text_encoder == "native":
        out = encode_text_native(model_path, prompt, negative_prompt, device, max_sequence_length)
    else:
        from transformers import AutoTokenizer, UMT5EncoderModel
        tok = AutoTokenizer.from_pretrained(os.path.join(model_path, "tokenizer"), local_files_only=True)
        te = UMT5EncoderModel.from_pretrained(os.path.join(model_path, "text_encoder"), torch_dtype=torch.bfloat16, local_files_only=True).to(device)
        out = {}
        for key, text in (("prompt_embeds", prompt), ("negative_prompt_embeds", negative_prompt)):
            t = tok([text], padding="max_length", max_length=max_sequence_length, truncation=True, add_special_tokens=True,
                    return_attention_mask=True, return_tensors="pt")
            n = int(t.attention_mask.gt(0).sum(dim=1)[0])
            with torch.no_grad():
                h = te(t.input_ids.to(device), t.attention_mask.to(device)).last_hidden_state.to(torch.bfloat16)[0, :n]
            out[key] = torch.cat([h, h.new_zeros(max_sequence_length - n, h.shape[1])]).unsqueeze(0)
        del te
    if image_encoder == "native":
        from . import clip
        out["image_embeds"] = clip.encode_image(model_path, image, device)
        return out
    from transformers import CLIPImageProcessor, CLIPVisionModel
    proc = CLIPImageProcessor.from_pretrained(os.path.join(model_path, "image_processor"), local_files_only=True)
    ie = CLIPVisionModel.from_pretrained(os.path.join(model_path, "image_encoder"), torch_dtype=torch.float32, local_files_only=True).to(device)
    with torch.no_grad():
        px = proc(images=image, return_tensors="pt").to(device)
        out["image_embeds"] = ie(**px, output_hidden_states=True).hidden_states[-2].to(torch.bfloat16)
    return out


def run(models_dir: Optional[str], video_ref: str, model: str = "720p", output: str = "output.mp4", image: Optional[str] = None,
        guided: bool = False, resample_steps: int = 3, guide_steps: int = 20, omega: float = 1.8, omega_resample: float = 1.0,
        num_frames: int = 25, num_inference_steps: int = 50, guidance_scale: float = 5.0, resample_round: int = 20, static: bool = False,
        prompt: Optional[str] = None, negative_prompt: Optional[str] = None, embeds: Optional[str] = None,
        use_pca_channel_selection: bool = False, soften_mask: bool = False, transition_distance: int = 15, decay_type: str = "sine",
        save_png: bool = False, device: str = "cuda:0", components: Optional[dict] = None, max_area: Optional[int] = None, seed: int = 42,
        vae_precision: str = "fp16x3", flow_backend: str = "farneback", dit_precision: str = "bf16", text_encoder: str = "transformers",
        image_encoder: str = "transformers", stage1: str = "files", stage1_frames=None, save_stage1: Optional[str] = None,
        **stage1_options):
    """INFER:153-339.  Returns (frames float32 [F,H,W,3] in [0,1], output directory of the PNG frames or None).
    components: {"transformer", "vae", "scheduler"} to use instead of loading `models_dir` (tests; synthetic weights); max_area overrides the
    model's pixel budget the same way harness.prepare_inputs documents.
    stage1 "vggt" / "depthcrafter" (video_ref None): stage 1 runs in this process BEFORE the DiT and the VAE are loaded, its options come
    as keywords under the stage-1 commands' own names (vggt_checkpoint, image_path, direction, ... / video_path, depth_npz, ...; see
    stage1.py), and its frames reach the sampler through harness.prepare_inputs_device without leaving the device; save_stage1 also writes
    them as PNG files.  stage1_frames = (images u8 [F,H,W,3], masks u8 [F,H,W] 0 / 1) hands over tensors a caller already holds.  The
    tensors are bit-identical to the file route's.  With image_encoder="native" and no `image`, clip.encode_image is handed the first
    frame at the sampler's size as a device tensor (the PIL image's bits) and preprocesses it there.  Stated deviation: the in-process
    route keeps stage 1's frame order; the file route sorts the file names, which is the same order for fewer than 100 frames and label
    angles below 100 degrees."""
    from . import stage1 as stage1_mod
    from .dit import WanTransformer3DModel
    from .pipeline import WanImageToVideoPipeline
    from .scheduler import UniPCMultistepScheduler
    from .vae import AutoencoderKLWan

    if text_encoder not in ("transformers", "native"):
        raise ValueError(f"--text-encoder {text_encoder!r}: transformers or native")
    if image_encoder not in ("transformers", "native"):
        raise ValueError(f"--image-encoder {image_encoder!r}: transformers or native")
    dev = torch.device(device)
    eff_frames = max(num_frames // 4 * 4 + 1 if num_frames % 4 != 1 else num_frames, 1)     # PIPE:475-478
    mismatch = ("{src} holds {n} frames but --num-frames {num} decodes {eff}: the reference blends "
                "frame by frame (scheduling_unipc_multistep_clean.py:1326 raises on a mismatch)")
    in_process = stage1 != "files" or stage1_frames is not None
    if in_process:   # stage 1 first: VGGT and the DiT / VAE are never resident together, and a wrong frame count is refused before they load
        images_u8, masks_u8 = stage1_mod.frames_for(stage1, stage1_options, eff_frames, dev, stage1_frames=stage1_frames, save_dir=save_stage1)
        if images_u8.shape[0] != eff_frames:
            raise ValueError(mismatch.format(src="stage1_frames" if stage1_frames is not None else f"--stage1 {stage1}", n=images_u8.shape[0], num=num_frames, eff=eff_frames))
    elif stage1_options:
        raise TypeError(f"--stage1 files does not take {sorted(stage1_options)}")
    elif video_ref is None:
        raise ValueError("--stage1 files needs --video-ref")
    model_path = None
    if components is None:
        model_path = os.path.join(models_dir, "wan2.1_480p_model_local" if model == "480p" else "wan2.1_720p_model_local")   # INFER:160-168
        if not os.path.exists(model_path):
            raise ValueError(f"Model path does not exist: {model_path}")
        vae = AutoencoderKLWan.from_pretrained(model_path, device=dev, precision=vae_precision)                              # INFER:185-189
        transformer = WanTransformer3DModel.from_pretrained(model_path, device=dev, linear_precision=dit_precision)                # INFER:191-197
        cfg_file = os.path.join(model_path, "scheduler", "scheduler_config.json")
        sconf = json.load(open(cfg_file)) if os.path.exists(cfg_file) else {"flow_shift": 3.0 if model == "480p" else 5.0}
        scheduler = UniPCMultistepScheduler.from_config(sconf, flow_backend=flow_backend)                                    # INFER:200-202
    else:
        transformer, vae, scheduler = components["transformer"], components["vae"], components["scheduler"]
    pipe = WanImageToVideoPipeline(transformer, vae, scheduler, device=dev)

    # INFER:206-254 (the first frame of the warped sequence is the input image unless --image is given)
    # --image given: the size rule takes the IMAGE's aspect ratio and the warped frames / masks are resized to it (INFER:209-241).  The
    # warped sequence is NOT truncated to --num-frames: the reference blends frame by frame and its resize of a sequence of another length
    # raises (scheduling_unipc_multistep_clean.py:1326), so a mismatch is an error here too, before any GPU work.
    prep = dict(model=model, num_frames=None, soften=soften_mask, transition_distance=transition_distance, decay_type=decay_type, device=dev,
                max_area=max_area, image=image)
    clip_image = None
    if in_process:
        pil, video, mask, height, width = harness.prepare_inputs_device(images_u8, masks_u8, **prep)
        if image_encoder == "native" and image is None and embeds is None:
            # the native image encoder takes the frame where it is: `pil` is images_u8[0] resized to (height, width), and so is this
            from . import ops
            clip_image = ops.resample_u8(images_u8[:1].contiguous(), (height, width))[0]
        del images_u8, masks_u8
    else:
        pil, video, mask, height, width = harness.prepare_inputs(video_ref, **prep)
    if video.shape[2] != eff_frames:
        raise ValueError(mismatch.format(src="--video-ref", n=video.shape[2], num=num_frames, eff=eff_frames))
    if negative_prompt is None:   # INFER:277-284: the two negative prompts are literals of the entry point, chosen by --static
        negative_prompt = NEGATIVE_PROMPT_STATIC if static else NEGATIVE_PROMPT_DYNAMIC

    if embeds is not None:
        emb = load_embeds(embeds, dev)
    elif model_path is not None and all(os.path.isdir(os.path.join(model_path, d)) for d in ("text_encoder", "tokenizer", "image_encoder", "image_processor")):
        if prompt is None:
            raise ValueError("pass --prompt (the reference's scene -> prompt table utils/prompts.py is not shipped)")
        emb = encode_with_transformers(model_path, prompt, negative_prompt, pil if clip_image is None else clip_image, dev,
                                       text_encoder=text_encoder, image_encoder=image_encoder)
    else:
        raise ValueError("no --embeds file and no text_encoder / image_encoder folders to compute them from")

    out = pipe(image=pil, height=height, width=width, num_frames=num_frames, num_inference_steps=num_inference_steps,
               guidance_scale=guidance_scale, generator=torch.manual_seed(seed), prompt_embeds=emb["prompt_embeds"],
               negative_prompt_embeds=emb["negative_prompt_embeds"], image_embeds=emb["image_embeds"], output_type="np", video_ref=video,
               mask=mask, guided=guided, resample_steps=resample_steps, guide_steps=guide_steps, omega=omega, omega_resample=omega_resample,
               resample_round=resample_round, use_pca_channel_selection=use_pca_channel_selection, static=static)
    frames = out.frames[0]
    png_dir = None
    out_dir = os.path.dirname(output)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    # the mp4 container (diffusers' export_to_video, INFER:317) is an external encoder, so the lossless PNG frames (--save-png in the
    # reference, INFER:323-339) are this engine's output format and are always written
    png_dir = harness.save_png_frames(frames, output)
    return frames, png_dir


def main(argv=None):
    ap = argparse.ArgumentParser(description="WorldForge guided image-to-video on MI355X (the reference's infer_worldforge.py arguments)")
    ap.add_argument("--model", choices=["480p", "720p"], default="720p")
    ap.add_argument("--models-dir", required=True)
    ap.add_argument("--output", default="output.mp4")
    ap.add_argument("--image", default=None)
    ap.add_argument("--video-ref", default=None, help="the warped frames / masks of a stage-1 command (required with --stage1 files)")
    ap.add_argument("--guided", action="store_true")
    ap.add_argument("--resample-steps", type=int, default=3)
    ap.add_argument("--guide-steps", type=int, default=20)
    ap.add_argument("--omega", type=float, default=1.8)
    ap.add_argument("--omega_resample", type=float, default=1.0)
    ap.add_argument("--num-frames", type=int, default=25)
    ap.add_argument("--num-inference-steps", type=int, default=50)
    ap.add_argument("--guidance-scale", type=float, default=5.0)
    ap.add_argument("--resample-round", type=int, default=20)
    ap.add_argument("--static", choices=["True", "False"], default="False")
    ap.add_argument("--use-pca-channel-selection", action="store_true")
    ap.add_argument("--soften-mask", action="store_true")
    ap.add_argument("--transition-distance", type=int, default=15)
    ap.add_argument("--decay-type", choices=["linear", "exponential", "sine", "cosine"], default="sine")
    ap.add_argument("--save-png", action="store_true",
                    help="accepted for CLI compatibility: the lossless PNG frames are ALWAYS written (this engine has no mp4 encoder, INFER:317)")
    ap.add_argument("--prompt", default=None, help="instead of the reference's --scene lookup in utils/prompts.py")
    ap.add_argument("--negative-prompt", default=None, help="default: the reference's static / dynamic negative prompt by --static (INFER:277-285)")
    ap.add_argument("--embeds", default=None, help=".npz / .safetensors with prompt_embeds, negative_prompt_embeds, image_embeds")
    ap.add_argument("--text-encoder", choices=["transformers", "native"], default="transformers",
                    help="without --embeds: run the folder's UMT5 through the Hugging Face class (default) or on this engine's own kernels")
    ap.add_argument("--image-encoder", choices=["transformers", "native"], default="transformers",
                    help="without --embeds: run the folder's CLIP vision encoder through the Hugging Face class (default) or on this engine's own "
                         "fp32 kernels")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--dit-precision", choices=["bf16", "mxfp8"], default="bf16",
                    help="DiT block linears: bf16 (default) or the opt-in MX-fp8 GEMMs (lower precision, faster)")
    from . import stage1 as stage1_mod
    stage1_mod.add_arguments(ap)
    a = ap.parse_args(argv)
    if a.stage1 == "files" and a.video_ref is None:
        ap.error("--stage1 files needs --video-ref")
    frames, png_dir = run(a.models_dir, a.video_ref, model=a.model, output=a.output, image=a.image, guided=a.guided,
                          resample_steps=a.resample_steps, guide_steps=a.guide_steps, omega=a.omega, omega_resample=a.omega_resample,
                          num_frames=a.num_frames, num_inference_steps=a.num_inference_steps, guidance_scale=a.guidance_scale,
                          resample_round=a.resample_round, static=a.static == "True", prompt=a.prompt, negative_prompt=a.negative_prompt,
                          embeds=a.embeds, use_pca_channel_selection=a.use_pca_channel_selection, soften_mask=a.soften_mask,
                          transition_distance=a.transition_distance, decay_type=a.decay_type, save_png=a.save_png, device=a.device,
                          dit_precision=a.dit_precision, text_encoder=a.text_encoder, image_encoder=a.image_encoder,
                          stage1=a.stage1, save_stage1=a.save_stage1, **stage1_mod.options_from_args(a))
    print(f"{len(frames)} frames -> {png_dir}")


if __name__ == "__main__":
    main()
