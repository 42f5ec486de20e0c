"""The IRR / FLF / DSG guided sampler, HIP-backed.

Host-side mirror of `WanImageToVideoPipeline` (PIPE = /root/reference/wan_for_worldforge/utils/pipeline_wan_i2v_clean.py):
same call signature for the sampling knobs (PIPE:390-424), same control flow (PIPE:562-728), same RNG draw order (CPU
generator, PIPE:323 and :644), same dtype hand-offs (latents become bf16 after a DSG step, PIPE:708).  The transformer,
the VAE and the scheduler are passed in as objects speaking the reference's (diffusers') call protocol, so the
MI355X-native modules of this package (dit.WanTransformer3DModel, vae.AutoencoderKLWan, scheduler.UniPCMultistepScheduler)
and test doubles are interchangeable.  Text / image encoders run once per video outside the loop and are out of scope
(SURVEY 2 #6): their outputs are taken as tensors (`prompt_embeds`, `negative_prompt_embeds`, `image_embeds`).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Union

import torch

from . import ops, trace
from . import sampler_common as sc


@dataclass
class WanPipelineOutput:
    frames: Any


class WanImageToVideoPipeline:
    def __init__(self, transformer, vae, scheduler, device: Union[str, torch.device] = "cuda:0"):
        self.transformer = transformer
        self.vae = vae
        self.scheduler = scheduler
        self.device = torch.device(device)
        tds = getattr(vae, "temperal_downsample", [False, True, True])
        self.vae_scale_factor_temporal = 2 ** sum(tds)  # PIPE:162
        self.vae_scale_factor_spatial = 2 ** len(tds)   # PIPE:163
        self._guidance_scale = 1.0
        self.tracer = trace.Tracer.from_env()  # WF_TRACE=<file.json>: roctx ranges + per-phase GPU time log (trace.py)
        self.timing: Dict[str, Dict[str, float]] = {}  # {phase: {count, total_ms, mean_ms}} of the last call when tracing is on

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1

    # ---- PIPE:262-299 ---------------------------------------------------------------------------------------
    def check_inputs(self, image, height, width, prompt_embeds, negative_prompt_embeds, image_embeds):
        if image is None:
            raise ValueError("Must provide `image` (the first frame) -- it conditions the latents (PIPE:327-351)")
        if not isinstance(image, torch.Tensor) and not hasattr(image, "resize"):
            raise ValueError(f"`image` must be torch.Tensor or PIL.Image, got {type(image)}")
        if height % 16 != 0 or width % 16 != 0:
            raise ValueError(f"`height` and `width` must be divisible by 16, got {height} and {width}")
        if prompt_embeds is None:
            raise ValueError("Must provide `prompt_embeds` (text encoder output [B,512,4096]); the encoder is out of scope")
        if image_embeds is None:
            raise ValueError("Must provide `image_embeds` (CLIP penultimate hidden states [B,257,1280])")

    # ---- PIPE:301-362 ---------------------------------------------------------------------------------------
    def prepare_latents(self, image: torch.Tensor, batch_size: int, num_channels_latents: int, height: int, width: int,
                        num_frames: int, generator=None, latents: Optional[torch.Tensor] = None):
        ts, ss = self.vae_scale_factor_temporal, self.vae_scale_factor_spatial
        T = (num_frames - 1) // ts + 1
        h, w = height // ss, width // ss
        shape = (batch_size, num_channels_latents, T, h, w)
        if latents is None:
            latents = sc.randn(shape, generator, self.device, torch.float32)  # PIPE:323
        else:
            latents = latents.to(device=self.device, dtype=torch.float32)
        video_condition = torch.zeros((image.shape[0], image.shape[1], num_frames, height, width), dtype=torch.float32,
                                      device=self.device)
        video_condition[:, :, 0] = image
        mu = self.vae.encode(video_condition).latent_dist.mode()
        latent_condition = ops.latent_norm(mu, self.vae.config.latents_mean, self.vae.config.latents_std)
        if batch_size != latent_condition.shape[0]:
            latent_condition = latent_condition.repeat(batch_size, 1, 1, 1, 1)
        # PIPE:353-360: first latent frame is "given" in all 4 temporal sub-slots
        mask_lat = torch.zeros((batch_size, ts, T, h, w), dtype=torch.float32, device=self.device)
        mask_lat[:, :, 0] = 1.0
        return latents, torch.cat([mask_lat, latent_condition], dim=1)

    def _prepare_embeds(self, prompt_embeds, negative_prompt_embeds, image_embeds):
        """-> (prompt, negative prompt or None, image) embeddings on the device in the transformer dtype, the image's once per prompt."""
        device, dtype = self.device, self.transformer.dtype
        prompt_embeds = prompt_embeds.to(device=device, dtype=dtype)
        if self.do_classifier_free_guidance:
            if negative_prompt_embeds is None:
                raise ValueError("classifier-free guidance needs `negative_prompt_embeds`")
            negative_prompt_embeds = negative_prompt_embeds.to(device=device, dtype=dtype)
        image_embeds = image_embeds.to(device=device, dtype=dtype)
        if image_embeds.shape[0] != prompt_embeds.shape[0]:
            image_embeds = image_embeds.repeat(prompt_embeds.shape[0], 1, 1)
        return prompt_embeds, negative_prompt_embeds, image_embeds

    # ---- PIPE:593-614 ---------------------------------------------------------------------------------------
    def _velocity(self, x, timestep, prompt_embeds, negative_prompt_embeds, image_embeds, attention_kwargs):
        """The transformer's velocity for model input x; under CFG, both branches by one of three routes, combined."""
        def forward(text_embeds):
            return self.transformer(hidden_states=x, timestep=timestep, encoder_hidden_states=text_embeds,
                                    encoder_hidden_states_image=image_embeds, attention_kwargs=attention_kwargs, return_dict=False)[0]

        if not self.do_classifier_free_guidance:
            return forward(prompt_embeds)
        split = getattr(self, "cfg_split", None)
        pair = getattr(self.transformer, "forward_cfg_pair", None)
        if split is not None:
            # group 0 runs the positive-prompt forward, group 1 the negative one
            cond, uncond = sc.cfg_groups_exchange(split, lambda branch: forward(prompt_embeds if branch == 0 else negative_prompt_embeds))
        elif pair is not None:
            # same two calls as below, advanced in lock-step so that under sequence parallelism each branch's K / V
            # exchange overlaps the other branch's compute (dit.forward_tokens_pair); identical results
            cond, uncond = pair(hidden_states=x, timestep=timestep, encoder_hidden_states=prompt_embeds,
                                negative_encoder_hidden_states=negative_prompt_embeds, encoder_hidden_states_image=image_embeds)
        else:
            cond, uncond = forward(prompt_embeds), forward(negative_prompt_embeds)
        return ops.cfg_combine(cond, uncond, self.guidance_scale)

    @staticmethod
    def _rewind(sch):
        """Take back the step counter and the order warm-up of the UniPC step just made: the same step is taken again."""
        sch._step_index -= 1
        if sch.lower_order_nums > 0 and sch.last_lower_order_nums < sch.config.solver_order:
            sch.lower_order_nums -= 1

    # ---- PIPE:569-660 ---------------------------------------------------------------------------------------
    def _step_rounds(self, i, t, latents, condition, embeds, attention_kwargs, generator, resample_steps, resample_round, step_kw):
        """Step i's rounds: the velocity and the scheduler's step; then, before step resample_round, resample_steps - 1 times over, the
        predicted clean sample re-noised to this step's level and the same step taken again from there.  step_kw: what sch.step is
        given alike in every round.  -> (the latents the last round started from, its scheduler output)."""
        sch, tr = self.scheduler, self.tracer
        scheduler_output = None
        for r in range(resample_steps):
            sch.set_resample_mode(r > 0)
            if r > 0:
                self._rewind(sch)
                sch.this_order = sch.last_this_order
            timestep_for_transformer = (sch.get_resample_timestep(i) if r > 0 else t).expand(latents.shape[0])
            latent_model_input = self._model_input(latents, condition, self.transformer.dtype)
            with tr.range("dit_cfg", step=i, round=r):
                noise_pred = self._velocity(latent_model_input, timestep_for_transformer, *embeds, attention_kwargs)
                if self.do_classifier_free_guidance and r < 1:
                    sch.derivative_history.append(noise_pred)
            with tr.range("scheduler_step", step=i, round=r):
                scheduler_output = sch.step(noise_pred, t, latents, resampling=r > 0, return_dict=True, current_step=i,
                                            resample_count=resample_steps, is_resample_round=i < resample_round, **step_kw)
            pred_original_sample = scheduler_output.pred_x0
            if i >= resample_round:
                break
            if r < resample_steps - 1 and pred_original_sample is not None:
                noise = sc.randn(pred_original_sample.shape, generator, self.device)  # PIPE:644
                with tr.range("renoise", step=i, round=r):
                    latents = sch.add_noise(pred_original_sample, noise, sch.get_resample_timestep(i), r,
                                            use_resample_sigma=True)
        return latents, scheduler_output

    # ---- PIPE:664-708 ---------------------------------------------------------------------------------------
    def _dsg_step(self, latents, omega, step):
        """DSG: extrapolate from the first to the last velocity of this step's rounds and take the step again with the result, the
        UniPC state put back by hand; the latents come out in the transformer dtype (PIPE:708)."""
        sch = self.scheduler
        with self.tracer.range("dsg", step=step):
            better = ops.dsg(sch.derivative_history[-1], sch.derivative_history[0], omega)
        self._rewind(sch)
        converted = sch.convert_model_output(better, sample=latents)
        sch.last_sample = latents
        sch.model_outputs[-1] = converted
        latents = sch.multistep_uni_p_bh_update(model_output=better, sample=latents, order=sch.this_order)
        sch._step_index += 1
        if 0 <= sch.lower_order_nums < sch.config.solver_order:
            sch.lower_order_nums += 1
        return ops.cast(latents, self.transformer.dtype)

    # ---- PIPE:388-753 ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, image, prompt=None, negative_prompt=None, height: int = 480, width: int = 832, num_frames: int = 81,
                 num_inference_steps: int = 50, guidance_scale: float = 5.0, num_videos_per_prompt: int = 1,
                 generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                 image_embeds: Optional[torch.Tensor] = None, output_type: str = "np", return_dict: bool = True,
                 attention_kwargs=None, callback_on_step_end: Optional[Callable] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], max_sequence_length: int = 512,
                 video_ref: Optional[torch.Tensor] = None, mask=None, guided: bool = False, resample_steps: int = 1,
                 guide_steps: int = 20, omega: float = 1.8, omega_resample: float = 1.0, resample_round: int = 20,
                 use_pca_channel_selection: bool = False, static: bool = False, start_step: int = 0,
                 max_steps: Optional[int] = None, step_hook: Optional[Callable] = None):
        """Extra (non-reference) arguments: `start_step` / `max_steps` run a window of the schedule (used by bench.py);
        `step_hook(i, phase)` is called at outer-step boundaries for timing."""
        if prompt is not None:
            raise ValueError("text encoding is out of scope: pass `prompt_embeds` / `negative_prompt_embeds`")
        self.check_inputs(image, height, width, prompt_embeds, negative_prompt_embeds, image_embeds)
        ts = self.vae_scale_factor_temporal
        if num_frames % ts != 1:
            num_frames = num_frames // ts * ts + 1  # PIPE:475-477
        num_frames = max(num_frames, 1)
        self._guidance_scale = guidance_scale
        device, sch = self.device, self.scheduler
        batch_size = prompt_embeds.shape[0]
        embeds = self._prepare_embeds(prompt_embeds, negative_prompt_embeds, image_embeds)
        sch.set_timesteps(num_inference_steps, device=device)
        timesteps = sch.timesteps
        img = sc.preprocess_image(image, height, width).to(device)
        latents, condition = self.prepare_latents(img, batch_size * num_videos_per_prompt, self.vae.config.z_dim, height,
                                                  width, num_frames, generator, latents)
        if video_ref is not None and guided:
            if not isinstance(video_ref, torch.Tensor):
                video_ref = torch.tensor(video_ref)
            video_ref = video_ref.to(dtype=torch.float32).to(device=device)
        if mask is not None and guided:
            mask = sc.guide_mask(mask, device).contiguous()  # fp64 -> fp32 is what SCHED:1374 does per call
        if not hasattr(sch, "derivative_history"):
            sch.derivative_history = []

        tr = self.tracer
        tr.reset()  # `self.timing` and the WF_TRACE log describe THIS call only
        sch.tracer = tr
        if start_step:
            # bench window: enter the schedule at `start_step` (UniPC restarts at order 1 there, like step 0)
            sch._step_index = start_step
        n_done = 0
        for i, t in enumerate(timesteps):
            if i < start_step:
                continue
            if max_steps is not None and n_done >= max_steps:
                break
            if step_hook is not None:
                step_hook(i, "begin")
            sch.derivative_history = []
            step_kw = dict(mask=mask, guided=guided and i < guide_steps, video_latents=video_ref, vae=self.vae,
                           use_pca_channel_selection=use_pca_channel_selection, static=static)
            latents, scheduler_output = self._step_rounds(i, t, latents, condition, embeds, attention_kwargs, generator,
                                                          resample_steps, resample_round, step_kw)
            if len(sch.derivative_history) > 1:
                latents = self._dsg_step(latents, omega_resample if i >= guide_steps else omega, i)
            else:
                latents = scheduler_output.prev_sample
            sch.set_resample_mode(False)
            if callback_on_step_end is not None:
                cb_out = callback_on_step_end(self, i, t, {"latents": latents}) or {}
                latents = cb_out.pop("latents", latents)
            n_done += 1
            if step_hook is not None:
                step_hook(i, "end")

        video = sc.decode_tail(self.vae, latents, output_type, self._vae_input, tracer=tr)
        if tr.enabled:
            self.timing = tr.summary()
            if getattr(tr, "path", None):
                tr.finish()
        if not return_dict:
            return (video,)
        return WanPipelineOutput(frames=video)

    def _model_input(self, latents, condition, dtype):
        """PIPE:590: cat([latents, condition], 1).to(transformer_dtype)."""
        x = torch.cat([latents.to(torch.float32), condition], dim=1)
        return ops.cast(x, dtype)

    def _vae_input(self, latents):
        """PIPE:733-742: the final latents in fp32, de-normalised."""
        return ops.latent_denorm(ops.cast(latents, torch.float32), self.vae.config.latents_mean, self.vae.config.latents_std)

