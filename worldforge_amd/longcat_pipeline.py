"""The LongCat-Video guided image-to-video sampler (IRR re-noising, FLF gate, DSG auto-guidance, CFG-zero), HIP-backed.

Host-side mirror of `LongCatVideoPipeline.generate_i2v` (PIPE = longcat_for_worldforge/longcat_video/pipeline_longcat_video.py:619-1006)
of `generate_vc` (PIPE:1010-1267, video continuation from the last frames of a video, on the DiT's resident condition KV cache)
and of `generate_refine` (PIPE:1271-1511, the 720p refine pass):
same sampling knobs, same control flow (PIPE:823-994), same RNG draw order (CPU generator: noise latents PIPE:256, the posterior sample
of the conditioning frame PIPE:278, the re-noise draws PIPE:925), same dtype hand-offs (fp32 latents, DiT input / timesteps in the
DiT dtype).  The DiT, the VAE and the scheduler are objects speaking the reference's call protocol, so the MI355X-native modules of
this package (longcat_dit.LongCatVideoTransformer3DModel, vae.AutoencoderKLWan, longcat_scheduler.FlowMatchEulerDiscreteScheduler)
and test doubles are interchangeable.  The UMT5 text encoder runs once per video outside the loop and is out of scope: its outputs
are taken as tensors (`prompt_embeds` [1,1,N,C] + `prompt_attention_mask` [1,N], and the negative pair).  The target size is given
explicitly (`height`, `width`): the resolution-bucket lookup of PIPE:358-372 belongs to the front-end.
"""
from __future__ import annotations

from typing import Optional, Union

import numpy as np
import torch

from . import ops
from . import sampler_common as sc


def prompt_batch(device, dtype, prompt_embeds, prompt_attention_mask, negative_prompt_embeds=None, negative_prompt_attention_mask=None,
                 do_cfg: bool = False):
    """The prompt hand-off: -> (embeddings in `dtype`, attention masks) on `device`; under CFG the batch [negative, positive] of both
    (PIPE:760-762 / 1148-1150)."""
    pe, pm = prompt_embeds.to(device, dtype), prompt_attention_mask.to(device)
    if do_cfg:
        if negative_prompt_embeds is None:
            raise ValueError("classifier-free guidance (guidance_scale > 1) needs the negative prompt embeddings")
        pe = torch.cat([negative_prompt_embeds.to(device, dtype), pe], dim=0)
        pm = torch.cat([negative_prompt_attention_mask.to(device), pm], dim=0)
    return pe, pm


class LongCatVideoPipeline:
    def __init__(self, vae, scheduler, dit, device: Union[str, torch.device] = "cuda:0"):
        self.vae, self.scheduler, self.dit = vae, scheduler, dit
        self.device = torch.device(device)
        cfg = getattr(vae, "config", None)
        self.vae_scale_factor_temporal = getattr(cfg, "scale_factor_temporal", 4)  # PIPE:83-84
        self.vae_scale_factor_spatial = getattr(cfg, "scale_factor_spatial", 8)
        self._num_timesteps = 1000
        self._num_distill_sample_steps = 50
        self._guidance_scale = 1.0

    @classmethod
    def from_pretrained(cls, path: str, device: Union[str, torch.device] = "cuda:0", vae_precision: str = "bf16", dit_precision: str = "bf16",
                        flow_backend: str = "farneback", components: Optional[dict] = None):
        """The three modules of run_longcat_worldforge_single.py:205-207 from one checkpoint folder: `vae/` as a bf16 module
        (AutoencoderKLWan.from_pretrained(..., torch_dtype=torch.bfloat16)), `scheduler/` and `dit/`.  components: any of "vae",
        "scheduler", "dit" to use instead of loading it.  The tokenizer and the UMT5 text encoder are not part of this pipeline (see
        the module docstring): longcat_infer runs them once and frees them."""
        from .longcat_dit import LongCatVideoTransformer3DModel
        from .longcat_scheduler import FlowMatchEulerDiscreteScheduler
        from .vae import AutoencoderKLWan
        given = dict(components or {})
        unknown = set(given) - {"vae", "scheduler", "dit"}
        if unknown:
            raise ValueError(f"components may hold 'vae', 'scheduler', 'dit', not {sorted(unknown)}")
        vae = given["vae"] if "vae" in given else AutoencoderKLWan.from_pretrained(path, device=device, precision=vae_precision,
                                                                                   torch_dtype=torch.bfloat16)
        scheduler = given["scheduler"] if "scheduler" in given else FlowMatchEulerDiscreteScheduler.from_pretrained(path, flow_backend=flow_backend)
        dit = given["dit"] if "dit" in given else LongCatVideoTransformer3DModel.from_pretrained(path, device=device, linear_precision=dit_precision)
        return cls(vae, scheduler, dit, device=device)

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1.0

    # ---- PIPE:317-331 ---------------------------------------------------------------------------------------------------
    def get_timesteps_sigmas(self, sampling_steps: int, use_distill: bool = False) -> torch.Tensor:
        if use_distill:
            idx = torch.arange(1, self._num_distill_sample_steps + 1, dtype=torch.float32)
            idx = (idx * (self._num_timesteps // self._num_distill_sample_steps)).round().long()
            inf = np.floor(np.linspace(0, self._num_distill_sample_steps, num=sampling_steps, endpoint=False)).astype(np.int64)
            sigmas = torch.flip(idx, [0])[inf].float() / self._num_timesteps
            sigmas = sigmas - sigmas[-1]
        else:
            sigmas = torch.linspace(0.999, 0.000, sampling_steps)
        return sigmas.to(torch.float32)

    def _check_size(self, height: int, width: int, blocks: int = 1):
        """PIPE:199-201 (and :1336, the refine pass: blocks = 4)."""
        ssp = self.vae_scale_factor_spatial * 2 * blocks
        if height % ssp != 0 or width % ssp != 0:
            raise ValueError(f"`height and width` have to be divisible by {ssp} but are {height} and {width}.")

    def _snap_frames(self, num_frames: int) -> int:
        """PIPE:700-704 / 1092-1096: down to 4k + 1 frames."""
        if num_frames % self.vae_scale_factor_temporal != 1:
            num_frames = num_frames // self.vae_scale_factor_temporal * self.vae_scale_factor_temporal + 1
        return max(num_frames, 1)

    def _set_timesteps(self, num_inference_steps: int, use_distill: bool = False) -> torch.Tensor:
        """PIPE:764-767 / 1152-1155 / 1394-1395."""
        sigmas = self.get_timesteps_sigmas(num_inference_steps, use_distill=use_distill)
        self.scheduler.set_timesteps(num_inference_steps, sigmas=sigmas, device=self.device)
        return self.scheduler.timesteps

    def _noise_latents(self, batch_size, num_channels_latents, height, width, num_frames, generator, latents):
        """PIPE:214-256: the given latents on the device, or noise of the latent shape drawn in fp32."""
        T = (num_frames - 1) // self.vae_scale_factor_temporal + 1
        shape = (batch_size, num_channels_latents, T, height // self.vae_scale_factor_spatial, width // self.vae_scale_factor_spatial)
        return sc.randn(shape, generator, self.device) if latents is None else latents.to(self.device)

    def _norm_in_own_dtype(self, x: torch.Tensor) -> torch.Tensor:
        """PIPE:385-394 as the reference writes it: the constants and both statements in x's dtype (ops.latent_norm is the fp32 form)."""
        mean = torch.tensor(self.vae.config.latents_mean).view(1, -1, 1, 1, 1).to(self.device, x.dtype)
        istd = 1.0 / torch.tensor(self.vae.config.latents_std).view(1, -1, 1, 1, 1).to(self.device, x.dtype)
        return (x - mean) * istd

    # ---- PIPE:214-286 with num_cond_frames = 1 ----------------------------------------------------------------------------
    def prepare_latents(self, image: torch.Tensor, batch_size: int, num_channels_latents: int, height: int, width: int,
                        num_frames: int, generator=None, latents: Optional[torch.Tensor] = None) -> torch.Tensor:
        latents = self._noise_latents(batch_size, num_channels_latents, height, width, num_frames, generator, latents).to(torch.float32)
        cond = []
        for i in range(batch_size):
            post = self.vae.encode(image[i].unsqueeze(0).unsqueeze(2)).latent_dist
            cond.append(post.sample(generator))  # PIPE:278 retrieve_latents(..., sample_mode="sample")
        cond = torch.cat(cond, dim=0).to(self.device, torch.float32)
        latents[:, :, :1] = ops.latent_norm(cond, self.vae.config.latents_mean, self.vae.config.latents_std)
        return latents

    # ---- PIPE:214-286 with a conditioning video -----------------------------------------------------------------------------
    def prepare_latents_video(self, video: torch.Tensor, batch_size: int, num_channels_latents: int, height: int, width: int,
                              num_frames: int, num_cond_frames: int, dtype: torch.dtype, generator=None,
                              latents: Optional[torch.Tensor] = None) -> torch.Tensor:
        """video [B, 3, F, H, W] in [-1, 1]: its LAST num_cond_frames frames are encoded (PIPE:272), sampled, normalised in `dtype`
        (PIPE:280-281: generate_vc holds its latents in the DiT dtype) and written over the first latent frames of the noise."""
        latents = self._noise_latents(batch_size, num_channels_latents, height, width, num_frames, generator, latents).to(dtype)  # PIPE:234, 252
        cond = []
        for i in range(batch_size):
            enc_in = video[i][:, -num_cond_frames:].unsqueeze(0)
            assert enc_in.shape[2] == num_cond_frames, "the video has fewer frames than num_cond_frames"  # PIPE:276
            cond.append(self.vae.encode(enc_in).latent_dist.sample(generator))
        ncl = 1 + (num_cond_frames - 1) // self.vae_scale_factor_temporal
        latents[:, :, :ncl] = self._norm_in_own_dtype(torch.cat(cond, dim=0).to(self.device, dtype))
        return latents

    def _preprocess_video(self, video, height, width) -> torch.Tensor:
        """diffusers VideoProcessor.preprocess_video without the resize: uint8 frames [F, H, W, 3] (tensor / array / list of arrays, what
        this pipeline's own output is times 255) or a float video [3, F, H, W] / [1, 3, F, H, W] in [0, 1] -> [1, 3, F, H, W] fp32 in [-1, 1]."""
        v = torch.as_tensor(np.array(video)) if not isinstance(video, torch.Tensor) else video
        if v.dtype == torch.uint8:
            if v.dim() != 4 or v.shape[-1] != 3:
                raise ValueError("uint8 video must be frames [F, H, W, 3]")
            v = v.permute(3, 0, 1, 2).to(torch.float32) / 255.0
        v = (v if v.dim() == 5 else v.unsqueeze(0)).to(torch.float32)
        if v.dim() != 5 or v.shape[1] != 3 or tuple(v.shape[-2:]) != (height, width):
            raise ValueError(f"video is {tuple(v.shape)}, expected [1, 3, F, {height}, {width}] (resizing to the bucket belongs to the front-end)")
        return 2.0 * v - 1.0

    # ---- the stages the three passes share -------------------------------------------------------------------------------------
    def _dit_forward(self, num_cond_latents: int, split=None):
        """-> forward(x, ts, pe, pm) for _velocity: the DiT's plain call on all frames, the first num_cond_latents of them clean.  With
        split (generate_i2v's `cfg_split`): the CFG batch [negative, positive] of PIPE:857-866 is two samples, and group b of the job's
        ranks runs sample b as ONE such call (sampler_common.cfg_groups_exchange)."""
        def plain(x, ts, pe, pm):
            return self.dit(hidden_states=x, timestep=ts, encoder_hidden_states=pe, encoder_attention_mask=pm,
                            num_cond_latents=num_cond_latents)

        def grouped(x, ts, pe, pm):
            if x.shape[0] != 2:
                return plain(x, ts, pe, pm)
            return torch.cat(sc.cfg_groups_exchange(split, lambda b: plain(x[b:b + 1], ts[b:b + 1], pe[b:b + 1], pm[b:b + 1])))

        return plain if split is None else grouped

    def _velocity(self, forward, latents, t, pe, pm, cfg_scale: Optional[float], num_clean: int) -> torch.Tensor:
        """PIPE:852-888 / 1206-1242 / 1466-1489: what the scheduler steps along.  The latents go to the DiT in its dtype, twice under CFG
        (cfg_scale is not None: pe / pm are then the batch [negative, positive]), with the timestep in that dtype, one per latent
        frame and t = 0 on the first num_clean frames; forward(x, ts, pe, pm) is the DiT call (_dit_forward, or a cached forward bound
        to its cache).  Then CFG-zero (PIPE:875-885) and the sign flip of PIPE:888 in one launch per sample, or the plain negation."""
        dit_dtype = self.dit.dtype
        x_in = ops.cast(latents, dit_dtype)
        if cfg_scale is not None:
            x_in = torch.cat([x_in] * 2)
        ts = t.expand(x_in.shape[0]).to(dit_dtype).unsqueeze(-1).repeat(1, x_in.shape[2])
        if num_clean:
            ts[:, :num_clean] = 0
        noise_pred = forward(x_in, ts, pe, pm)
        if cfg_scale is None:
            return -noise_pred
        u, c = noise_pred.chunk(2)
        return torch.stack([ops.cfg_zero(c[b], u[b], cfg_scale, negate=True) for b in range(c.shape[0])])

    def _denoise_window(self, latents, ncl: int, timesteps, pe, pm, cfg_scale, step_hook, cached=None) -> torch.Tensor:
        """The loop of generate_vc (PIPE:1195-1255) and generate_refine (PIPE:1464-1497): the first ncl latent frames are the clean
        condition, the rest are denoised.  cached = (build, forward), the DiT's cache_condition / forward_cached or their _blocks
        forms: the condition frames go through the DiT once (one video per call: a CFG pair shares the cache, LCA:163-165), every
        step runs and steps the noise frames only (PIPE:1246), and the condition is put back in front (PIPE:1254-1255).  cached =
        None: every step runs all frames through the plain call (PIPE:1215-1216) and steps the noise frames in place (PIPE:1248),
        which rounds them to the dtype the latents are held in."""
        sch = self.scheduler
        cond_latents = None
        if cached is None:
            forward = self._dit_forward(ncl)
        else:
            build, cached_forward = cached
            cond_latents = latents[:, :, :ncl]
            cache = build(cond_latents[0])
            latents = latents[:, :, ncl:].contiguous()

            def forward(x, ts, pe, pm):
                return cached_forward(x, ts, pe, pm, cache)
        for i, t in enumerate(timesteps):
            if step_hook is not None:
                step_hook(i, "start")
            sch.derivative_history = []  # (the scheduler notes every velocity it steps along; only generate_i2v reads them)
            noise_pred = self._velocity(forward, latents, t, pe, pm, cfg_scale, 0 if cached else ncl)
            if cached:
                latents = sch.step(noise_pred, t, latents, return_dict=False)[0]
            else:
                latents[:, :, ncl:] = sch.step(noise_pred[:, :, ncl:], t, latents[:, :, ncl:], return_dict=False)[0]
            if step_hook is not None:
                step_hook(i, "end")
        return latents if cond_latents is None else torch.cat([cond_latents, latents], dim=2)

    def _final_latents(self, latents: torch.Tensor) -> torch.Tensor:
        """PIPE:999-1000: `latents.to(self.vae.dtype)` and the de-normalisation IN THAT DTYPE (a bf16 VAE module, the LongCat entry's
        run_longcat_worldforge_single.py:205: constants and both statements in bf16), handed to decode in the module dtype."""
        vdt = getattr(self.vae, "dtype", torch.float32)
        z = ops.latent_denorm(ops.cast(latents, vdt), self.vae.config.latents_mean, self.vae.config.latents_std)  # f32 holding vdt values
        return z if vdt == torch.float32 else ops.cast(z, vdt)

    def _finish(self, latents: torch.Tensor, output_type: str, crop=None):
        """PIPE:996-1006: the latents, or the decoded frames [B,F,H,W,C] in [0,1]."""
        return sc.decode_tail(self.vae, latents, output_type, self._final_latents, crop=crop)

    # ---- PIPE:1010-1267 ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate_vc(self, video, height: int, width: int, prompt_embeds: torch.Tensor, prompt_attention_mask: torch.Tensor,
                    negative_prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_attention_mask: Optional[torch.Tensor] = None,
                    num_frames: int = 93, num_cond_frames: int = 13, num_inference_steps: int = 50, use_distill: bool = False,
                    guidance_scale: float = 4.0, generator=None, latents: Optional[torch.Tensor] = None, output_type: str = "np",
                    use_kv_cache: bool = True, offload_kv_cache: bool = False, enhance_hf: bool = False, step_hook=None):
        """Video continuation: the last num_cond_frames frames of `video` become the first num_cond_latents = 1 + (num_cond_frames - 1)
        // 4 latent frames, kept clean (timestep 0) while the remaining frames are denoised; the result is a num_frames video that
        starts with them.  use_kv_cache (the default, PIPE:1195-1199): the loop runs on the DiT's resident condition cache
        (dit.cache_condition / dit.forward_cached, see _denoise_window); use_kv_cache=False: on all frames.  CFG-zero and the
        distilled schedule as in generate_i2v.  The latents are held in the DiT dtype as the reference's are (PIPE:1181), so the
        uncached loop rounds them to it after every step (PIPE:1248 writes into them) while the cached loop carries the scheduler's
        fp32 result (PIPE:1246).
        Not built: offload_kv_cache (the cache stays on the GPU), enhance_hf (the 10-step uniform tail of PIPE:1157-1166; the
        reference's default), several videos per prompt."""
        if offload_kv_cache:
            raise NotImplementedError("offload_kv_cache: the condition cache stays on the GPU")
        if enhance_hf:
            raise NotImplementedError("enhance_hf (PIPE:1157-1166) is not built")
        self._check_size(height, width)
        num_frames = self._snap_frames(num_frames)
        ncl = 1 + (num_cond_frames - 1) // self.vae_scale_factor_temporal  # PIPE:1189
        if num_cond_frames < 1 or ncl >= (num_frames - 1) // self.vae_scale_factor_temporal + 1:
            raise ValueError(f"num_cond_frames = {num_cond_frames} must be >= 1 and leave at least one of the {num_frames} frames to generate")
        self._guidance_scale = guidance_scale
        do_cfg = self.do_classifier_free_guidance
        dit_dtype = self.dit.dtype
        pe, pm = prompt_batch(self.device, dit_dtype, prompt_embeds, prompt_attention_mask, negative_prompt_embeds,
                              negative_prompt_attention_mask, do_cfg)
        timesteps = self._set_timesteps(num_inference_steps, use_distill)
        # PIPE:1168-1185
        vid = self._preprocess_video(video, height, width).to(self.device, dit_dtype)
        latents = self.prepare_latents_video(vid, 1, self.dit.config.in_channels, height, width, num_frames, num_cond_frames, dit_dtype,
                                             generator, latents)
        latents = self._denoise_window(latents, ncl, timesteps, pe, pm, guidance_scale if do_cfg else None, step_hook,
                                       (self.dit.cache_condition, self.dit.forward_cached) if use_kv_cache else None)
        return self._finish(latents, output_type)

    # ---- PIPE:1271-1511 ---------------------------------------------------------------------------------------------------
    @staticmethod
    def refine_padding(num_cond_frames: int, new_frame_size: int, temporal_scale: int = 4, granularity: int = 4):
        """PIPE:1414-1424: the refine pass pads the condition and the noise frames to whole blocks of `granularity` latent frames (what
        block-sparse attention takes).  -> (condition latent frames, frames repeated in front, noise latent frames, frames repeated
        behind); the condition count is 0 / 0 without condition frames."""
        import math
        tsc, gran = temporal_scale, granularity
        num_noise_frames = new_frame_size - num_cond_frames
        ncl = added_c = 0
        if num_cond_frames > 0:
            ncl = 1 + math.ceil((num_cond_frames - 1) / tsc)
            ncl = math.ceil(ncl / gran) * gran
            added_c = 1 + (ncl - 1) * tsc - num_cond_frames
        nnl = math.ceil(math.ceil(num_noise_frames / tsc) / gran) * gran
        added_n = nnl * tsc - num_noise_frames
        return ncl, added_c, nnl, added_n

    @staticmethod
    def refine_condition_frames(video: torch.Tensor, num_cond_frames: int, added_c: int) -> torch.Tensor:
        """PIPE:272-276: video [1, 3, F, H, W] -> its last (num_cond_frames - added_c) frames with the first of them repeated added_c
        times in front: [1, 3, num_cond_frames, H, W], num_cond_frames being the PADDED count."""
        take = num_cond_frames - added_c
        if take < 1 or video.shape[2] < take:
            raise ValueError(f"the conditioning video has {video.shape[2]} frames, num_cond_frames asks for its last {take}")
        enc_in = video[0][:, -take:].unsqueeze(0)
        enc_in = torch.cat([enc_in[:, :, 0:1].repeat(1, 1, added_c, 1, 1), enc_in], dim=2)
        assert enc_in.shape[2] == num_cond_frames
        return enc_in

    def _cut_schedule(self, timesteps: torch.Tensor, t_thresh: float) -> torch.Tensor:
        """PIPE:1396-1402: the schedule entered at t_thresh."""
        sch = self.scheduler
        tt = torch.tensor(t_thresh * 1000, dtype=timesteps.dtype)
        timesteps = torch.cat([tt.unsqueeze(0), timesteps[timesteps < tt]])
        sch.timesteps = timesteps
        sch.sigmas = torch.cat([timesteps / 1000, torch.zeros(1)])
        return timesteps

    def _upsample_stage1(self, stage1_video, height: int, width: int, spatial_refine_only: bool) -> torch.Tensor:
        """PIPE:1404-1413: the up-sampling chain in the DiT dtype, one kernel.  uint8 frames [F, H0, W0, 3] -> [1, 3, F or 2 F, height,
        width] fp32 in [-1, 1]."""
        from ._ffi import call
        frames = torch.as_tensor(np.array(stage1_video)) if not isinstance(stage1_video, torch.Tensor) else stage1_video
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError("stage1_video must be uint8 frames [F, H, W, 3]")
        if self.dit.dtype != torch.bfloat16:
            raise NotImplementedError("the up-sampling kernel rounds as a bf16 model does")
        frames = frames.to(self.device).contiguous()
        nf, H0, W0, _ = frames.shape
        new_frame_size = nf if spatial_refine_only else 2 * nf
        up = torch.empty((1, 3, new_frame_size, height, width), dtype=torch.float32, device=self.device)
        call("wf_refine_upsample_u8", frames.data_ptr(), up.data_ptr(), nf, H0, W0, new_frame_size, height, width, ops.stream())
        return up

    def _noised_latents(self, up: torch.Tensor, t_thresh: float, generator) -> torch.Tensor:
        """PIPE:1426-1435: the up-sampled video encoded (posterior sample), normalised and mixed with noise: (1 - t) * latent + t * noise,
        in fp32."""
        dev = self.device
        samp = self.vae.encode(up if getattr(self.vae, "dtype", torch.float32) == torch.float32 else ops.cast(up, self.vae.dtype)) \
            .latent_dist.sample(generator).to(dev)
        if samp.dtype == torch.float32:
            lat = ops.latent_norm(samp, self.vae.config.latents_mean, self.vae.config.latents_std)
            noise = sc.randn(tuple(lat.shape), generator, dev).to(lat.dtype)
            return ops.add_noise(lat, noise, 1 - t_thresh, t_thresh)
        # a bf16 VAE module hands back a bf16 sample: PIPE:1431-1433 then normalise in bf16 (constants in bf16), draw the noise IN BF16
        # (a different stream of the generator than an fp32 draw) and mix in bf16; prepare_latents casts the result to fp32 (PIPE:234)
        lat = self._norm_in_own_dtype(samp)
        noise = sc.randn(lat.shape, generator, dev, lat.dtype)
        return ((1 - t_thresh) * lat + t_thresh * noise).to(torch.float32)

    @torch.no_grad()
    def generate_refine(self, stage1_video, height: int, width: int, prompt_embeds: torch.Tensor, prompt_attention_mask: torch.Tensor,
                        image=None, num_cond_frames: int = 0, num_inference_steps: int = 50, generator=None, output_type: str = "np",
                        t_thresh: float = 0.5, spatial_refine_only: bool = False, step_hook=None, video=None,
                        use_kv_cache: bool = False):
        """The 720p refine pass: the stage-1 (480p) video is up-sampled, encoded, mixed with noise at t_thresh and denoised from there
        without CFG, the DiT running with block-sparse self-attention and the refinement LoRA, as
        run_longcat_worldforge_single.py:447-451 does: `dit.enable_loras(["refinement_lora"])` and `dit.enable_bsa()` on the resident
        model that ran stage 1 (longcat_dit.load_lora / enable_loras; or a model built with the adapter folded in by fold_lora).  stage1_video: uint8 frames [F, H0, W0, 3] (tensor / array / list of arrays);
        image: the conditioning first frame at the target size or None.  video: the already refined frames of the previous window
        (uint8 [F, H, W, 3] or float [3, F, H, W] at the target size): its last num_cond_frames frames condition this one (PIPE:272),
        front-padded to whole 4-latent-frame blocks by repeating their first frame (PIPE:1417-1419, 274-275).  use_kv_cache (off by
        default: the reference does not cache here): the condition latents go through the block-sparse DiT once
        (dit.cache_condition_blocks), every step runs the noise frames only (dit.forward_cached_blocks), and the condition latents
        are put back in front before decoding.  Returns frames [1, F', H, W, 3] in [0, 1]."""
        if image is not None and video is not None:  # PIPE:1332
            raise ValueError("Cannot provide both `image and video` at the same time. Please provide only one.")
        if video is not None and num_cond_frames <= 0:
            raise ValueError("a conditioning video needs num_cond_frames > 0 (how many of its last frames condition the window)")
        if use_kv_cache and num_cond_frames <= 0:
            raise ValueError("use_kv_cache caches the condition frames' stream: it needs num_cond_frames > 0 and an image or a video")
        self._check_size(height, width, blocks=4)
        dev, dit_dtype = self.device, self.dit.dtype
        pe, pm = prompt_batch(dev,dit_dtype, prompt_embeds, prompt_attention_mask)
        timesteps = self._set_timesteps(num_inference_steps)
        if t_thresh:
            timesteps = self._cut_schedule(timesteps, t_thresh)
        up = self._upsample_stage1(stage1_video, height, width, spatial_refine_only)
        new_frame_size = up.shape[2]
        # PIPE:1415-1435: pad to the block-sparse granularity (4 latent frames), encode, mix with noise
        ncl, added_c, nnl, added_n = self.refine_padding(num_cond_frames, new_frame_size, self.vae_scale_factor_temporal)
        num_cond_frames = num_cond_frames + added_c
        up = torch.cat([up[:, :, 0:1].repeat(1, 1, added_c, 1, 1), up, up[:, :, -1:].repeat(1, 1, added_n, 1, 1)], dim=2)
        latents = self._noised_latents(up, t_thresh, generator)
        del up
        enc_in = None
        if image is not None:  # PIPE:262-284: the condition frame, front-padded
            img = sc.preprocess_image(image, height, width).to(dev, dit_dtype)
            enc_in = img[0].unsqueeze(0).unsqueeze(2)
            enc_in = torch.cat([enc_in[:, :, 0:1].repeat(1, 1, added_c, 1, 1), enc_in], dim=2)
            assert enc_in.shape[2] == num_cond_frames
        elif video is not None:  # PIPE:272-284: the last frames of the video, front-padded likewise
            vid = self._preprocess_video(video, height, width).to(dev, dit_dtype)
            enc_in = self.refine_condition_frames(vid, num_cond_frames, added_c)
        elif num_cond_frames > 0:
            raise ValueError("num_cond_frames > 0 needs the conditioning image or the conditioning video")
        if enc_in is not None:  # encoded (posterior sample) and normalised
            cond = self.vae.encode(enc_in).latent_dist.sample(generator).to(dev, torch.float32)
            latents[:, :, :ncl] = ops.latent_norm(cond, self.vae.config.latents_mean, self.vae.config.latents_std)
        latents = self._denoise_window(latents, ncl, timesteps, pe, pm, None, step_hook,
                                       (self.dit.cache_condition_blocks, self.dit.forward_cached_blocks) if use_kv_cache else None)
        return self._finish(latents, output_type, crop=(added_c, new_frame_size + added_c))  # PIPE:1507

    # ---- PIPE:619-1006 ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate_i2v(self, image, height: int, width: int, prompt_embeds: torch.Tensor, prompt_attention_mask: torch.Tensor,
                     negative_prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_attention_mask: Optional[torch.Tensor] = None,
                     num_frames: int = 93, num_inference_steps: int = 50, use_distill: bool = False, guidance_scale: float = 4.0,
                     generator=None, latents: Optional[torch.Tensor] = None, output_type: str = "np",
                     video_ref: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, guided: bool = False,
                     resample_steps: int = 3, guide_steps: int = 20, resample_round: int = 20, omega: float = 1.8,
                     omega_resample: float = 1.0, use_pca_channel_selection: bool = False, static: bool = False,
                     max_replace_threshold: Optional[int] = None, step_hook=None):
        dev, sch = self.device, self.scheduler
        self._check_size(height, width)
        num_frames = self._snap_frames(num_frames)
        self._guidance_scale = guidance_scale
        do_cfg = self.do_classifier_free_guidance
        dit_dtype = self.dit.dtype
        pe, pm = prompt_batch(dev, dit_dtype, prompt_embeds, prompt_attention_mask, negative_prompt_embeds,
                              negative_prompt_attention_mask, do_cfg)
        timesteps = self._set_timesteps(num_inference_steps, use_distill)
        # PIPE:769-789
        img = sc.preprocess_image(image, height, width).to(dev, dit_dtype)
        latents = self.prepare_latents(img, 1, self.dit.config.in_channels, height, width, num_frames, generator, latents)
        if video_ref is not None and guided:
            video_ref = torch.as_tensor(video_ref).to(dev, torch.float32)  # PIPE:792-801
        if mask is not None and guided:
            mask = sc.guide_mask(mask, dev)  # PIPE:803-817
        # the condition frame is clean (PIPE:865); under `cfg_split` the two CFG samples run on one group of the job's ranks each
        forward = self._dit_forward(1, getattr(self, "cfg_split", None) if do_cfg else None)
        for i, t in enumerate(timesteps):
            if step_hook is not None:
                step_hook(i, "start")
            sch.derivative_history = []
            pred_x0 = None
            scheduler_output = None
            for r in range(resample_steps if (guided and i < resample_round) else 1):
                sch.set_resample_mode(r > 0)
                if r > 0:
                    sch._step_index -= 1
                noise_pred = self._velocity(forward, latents, t, pe, pm, guidance_scale if do_cfg else None, 1)
                scheduler_output = sch.step(
                    noise_pred[:, :, 1:], t, latents[:, :, 1:], video_ref=video_ref, mask=mask, guided=guided and i < guide_steps,
                    resampling=r > 0, vae=self.vae, use_pca_channel_selection=use_pca_channel_selection, static=static,
                    current_step=i, total_steps=len(timesteps), sample_full=latents, use_distill=use_distill,
                    max_replace_threshold=max_replace_threshold, return_dict=True)
                if scheduler_output.pred_x0 is not None:
                    pred_x0 = scheduler_output.pred_x0
                if i >= resample_round:
                    break
                if r < resample_steps - 1 and pred_x0 is not None:
                    noise = sc.randn(tuple(pred_x0.shape), generator, dev).to(pred_x0.dtype)  # PIPE:925
                    latents[:, :, 1:] = sch.add_noise(pred_x0, noise, t.expand(pred_x0.shape[0]), use_resample_sigma=False)
            sch.set_resample_mode(False)
            if i < resample_round and len(sch.derivative_history) > 1 and guided:
                latents[:, :, 1:] = self._dsg_step(latents, t, omega_resample if i >= guide_steps else omega, use_distill)
            elif scheduler_output is not None:
                latents[:, :, 1:] = scheduler_output.prev_sample
            if step_hook is not None:
                step_hook(i, "end")
        return self._finish(latents, output_type)

    def _dsg_step(self, latents, t, omega, use_distill):
        """DSG (PIPE:945-976): cosine-corrected extrapolation from the first to the last velocity of this step's rounds, and the step
        taken again along it.  -> the stepped frames 1.."""
        sch = self.scheduler
        better = ops.dsg(sch.derivative_history[-1].contiguous(), sch.derivative_history[0].contiguous(), omega)
        sch._step_index -= 1
        out = sch.step(better, t, latents[:, :, 1:], guided=False, resampling=False, vae=self.vae, sample_full=latents,
                       use_distill=use_distill, return_dict=True)
        return out.prev_sample
