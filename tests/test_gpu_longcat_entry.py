"""GPU: LongCat-Video from a checkpoint folder -- LongCatVideoTransformer3DModel.from_pretrained against load_state_dict, and the entry
point worldforge_amd.longcat_infer (guided i2v, the distill LoRA, continuation windows, the refine pass with switched LoRAs) against the
same calls wired by hand.

No kernel is added by this feature: both sides of every comparison run the same kernels on the same tensors, so every comparison is
torch.equal / np.array_equal and there is no tolerance.

Sizes: the tiny model of the continuation tests (hidden 256, 2 heads, depth 2, caption 64, adaln_tembed_dim 32), 64 x 96 pixels, 3
steps; continuation num_cond_frames 5, 2 steps; refine 64 x 128, 2 steps.  A window is 9 frames, not 13: the truck fixture holds 9
warped frames and the entry refuses a sequence of another length than the decoded frame count, so `--extend-windows 2` gives
9 + 2 * (9 - 5) = 17 frames."""
import functools
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import longcat_dit as olc
from tests import longcat_ckpt as ck
from tests.fakes import FakeVAE, lora_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUCK = os.path.join(ROOT, "tests", "golden", "truck")


def _model_cls():
    from worldforge_amd.longcat_dit import LongCatConfig, LongCatVideoTransformer3DModel
    return LongCatConfig, LongCatVideoTransformer3DModel


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _weights():
    return ck.weights(seed=3)


def _forward(m, T=3, w=12, ncl=1):
    """One forward on [16, T, 8, w] with a padded caption: what every loader comparison runs on both models."""
    x = _rand((16, T, 8, w), 11).to(BF).to(DEV)
    cap = _rand((24, 64), 12).to(BF).to(DEV)
    mask = torch.zeros(24, dtype=torch.int64)
    mask[:19] = 1
    return m.forward_tokens(x, [0.0] * ncl + [500.0] * (T - ncl), cap, mask, ncl)


def _same_weights(a, b):
    assert set(a.w) == set(b.w)
    for k in a.w:
        assert a.w[k].dtype == b.w[k].dtype and a.w[k].shape == b.w[k].shape and torch.equal(a.w[k], b.w[k]), k


# ---- the loader ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 2])
def test_from_pretrained_equals_load_state_dict(tmp_path, shards):
    LongCatConfig, Model = _model_cls()
    W = _weights()
    ck.write_dit(str(tmp_path), W, shards=shards)
    got = Model.from_pretrained(str(tmp_path), device=DEV)
    want = Model(LongCatConfig(**ck.KW), DEV).load_state_dict(ck.bf16_rounded(W))
    assert got.cfg == want.cfg and got.linear_precision == "bf16" and not got._bsa and got.device == torch.device(DEV)
    _same_weights(got, want)
    a, b = _forward(got), _forward(want)
    assert a.shape == (16, 3, 8, 12) and torch.isfinite(a).all() and torch.equal(a, b)
    # the folder itself instead of its parent
    _same_weights(Model.from_pretrained(str(tmp_path / "dit"), device=DEV), want)


def test_every_tensor_is_rounded_to_bf16_first(tmp_path):
    """An fp32 folder whose vectors (and matrices) are NOT bf16 values loads to the bits of the same folder rounded to bf16 beforehand;
    load_state_dict of the unrounded weights keeps its own behaviour (fp32 vectors as they are)."""
    LongCatConfig, Model = _model_cls()
    W = {k: v * (1 + 2.0 ** -10) + 2.0 ** -13 for k, v in _weights().items()}
    vectors = [k for k, v in W.items() if v.dim() == 1]
    assert vectors and all(not torch.equal(W[k].to(BF).float(), W[k]) for k in vectors)
    ck.write_dit(str(tmp_path / "f32"), W)
    ck.write_dit(str(tmp_path / "bf16"), ck.bf16_rounded(W), shards=2)
    a = Model.from_pretrained(str(tmp_path / "f32"), device=DEV)
    b = Model.from_pretrained(str(tmp_path / "bf16"), device=DEV)
    _same_weights(a, b)
    for k, t in a.w.items():
        assert t.dtype in (BF, torch.float32) and torch.equal(t.to(BF).to(t.dtype), t), k   # fp32 vectors hold bf16 values
    fa = _forward(a)
    assert torch.equal(fa, _forward(b))
    assert torch.equal(fa, _forward(Model(LongCatConfig(**ck.KW), DEV).load_state_dict(ck.bf16_rounded(W))))
    plain = Model(LongCatConfig(**ck.KW), DEV).load_state_dict(W)
    assert torch.equal(plain.w["patch.b"].cpu(), W["x_embedder.proj.bias"]) and not torch.equal(plain.w["patch.b"], a.w["patch.b"])
    assert not torch.equal(_forward(plain), fa)


def test_config_json_is_honoured(tmp_path):
    LongCatConfig, Model = _model_cls()
    W = _weights()
    ck.write_dit(str(tmp_path), W, config={"enable_bsa": True, "bsa_params": ck.BSA, "text_tokens_zero_pad": True, "some_new_field": 3})
    with pytest.warns(UserWarning, match="some_new_field") as rec:
        got = Model.from_pretrained(str(tmp_path), device=DEV)
    assert len([r for r in rec if "some_new_field" in str(r.message)]) == 1
    assert got._bsa and got.bsa_params == ck.BSA and got.cfg.text_tokens_zero_pad is True
    want = Model(LongCatConfig(**ck.KW, text_tokens_zero_pad=True), DEV, enable_bsa=True, bsa_params=ck.BSA).load_state_dict(ck.bf16_rounded(W))
    a, b = _forward(got, T=8, w=16, ncl=4), _forward(want, T=8, w=16, ncl=4)     # 4 + 4 latent frames of 4 x 8 tokens: two 64-token blocks each
    assert torch.equal(a, b) and got.last_bsa_indices is not None
    dense = Model(LongCatConfig(**ck.KW), DEV).load_state_dict(ck.bf16_rounded(W))
    assert not torch.equal(a, _forward(dense, T=8, w=16, ncl=4))
    # the ignored keys raise no warning; another class's folder is refused
    ck.write_dit(str(tmp_path / "plain"), W)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        Model.from_pretrained(str(tmp_path / "plain"), device=DEV)
    ck.write_dit(str(tmp_path / "wan"), W, config={"_class_name": "WanTransformer3DModel"}, subfolder="transformer")
    with pytest.raises(ValueError, match="WanTransformer3DModel"):
        Model.from_pretrained(str(tmp_path / "wan"), device=DEV, subfolder="transformer")


def test_linear_precision_passes_through(tmp_path):
    LongCatConfig, Model = _model_cls()
    W = _weights()
    ck.write_dit(str(tmp_path), W)
    got = Model.from_pretrained(str(tmp_path), device=DEV, linear_precision="mxfp8")
    want = Model(LongCatConfig(**ck.KW), DEV, linear_precision="mxfp8").load_state_dict(ck.bf16_rounded(W))
    assert got.linear_precision == "mxfp8"
    a = _forward(got)
    assert torch.equal(a, _forward(want)) and not torch.equal(a, _forward(Model.from_pretrained(str(tmp_path), device=DEV)))
    with pytest.raises(ValueError):
        Model.from_pretrained(str(tmp_path), device=DEV, linear_precision="fp4")


def test_bad_checkpoints_are_refused_before_any_upload(tmp_path, monkeypatch):
    LongCatConfig, Model = _model_cls()
    W = _weights()
    want = Model(LongCatConfig(**ck.KW), DEV).load_state_dict(ck.bf16_rounded(W))
    uploads = []
    monkeypatch.setattr(Model, "_assemble", lambda self, mat, vec, _orig=Model._assemble: (uploads.append(1), _orig(self, mat, vec))[1])
    missing = {k: v for k, v in W.items() if k != "blocks.1.ffn.w3.weight"}
    ck.write_dit(str(tmp_path / "missing"), missing, shards=2)
    with pytest.raises(KeyError, match="blocks.1.ffn.w3.weight"):
        Model.from_pretrained(str(tmp_path / "missing"), device=DEV)
    shaped = {**W, "blocks.0.attn.proj.bias": torch.zeros(128)}
    ck.write_dit(str(tmp_path / "shaped"), shaped)
    with pytest.raises(ValueError, match=r"blocks.0.attn.proj.bias is \[128\], expected \[256\]"):
        Model.from_pretrained(str(tmp_path / "shaped"), device=DEV)
    extra = {**W, "blocks.0.attn.rope.freqs": torch.zeros(8)}
    ck.write_dit(str(tmp_path / "extra"), extra)
    with pytest.raises(ValueError, match="blocks.0.attn.rope.freqs"):
        Model.from_pretrained(str(tmp_path / "extra"), device=DEV)
    ck.write_dit(str(tmp_path / "gone"), W, shards=2)
    os.remove(tmp_path / "gone" / "dit" / "diffusion_pytorch_model-00002-of-00002.safetensors")
    with pytest.raises(FileNotFoundError):
        Model.from_pretrained(str(tmp_path / "gone"), device=DEV)
    assert uploads == []
    with pytest.warns(UserWarning, match="blocks.0.attn.rope.freqs"):
        loose = Model.from_pretrained(str(tmp_path / "extra"), device=DEV, strict=False)
    assert uploads == [1]
    _same_weights(loose, want)
    assert torch.equal(_forward(loose), _forward(want))


# ---- the entry point -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """dit/ (bsa_params of the tiny refine tests, block-sparse attention off), scheduler/ (shift 3), the two LoRA files, and the
    embedding files."""
    root = str(tmp_path_factory.mktemp("longcat_ckpt"))
    ck.write_dit(root, _weights(), config={"bsa_params": ck.BSA})
    ck.write_scheduler(root, shift=3.0)
    ocfg = olc.LongCatConfig(**ck.KW)
    ck.write_lora(root, "cfg_step_lora", lora_state(ocfg, seed=33))
    ck.write_lora(root, "refinement_lora", lora_state(ocfg, seed=34))
    g = torch.Generator().manual_seed(7)
    pe, ne = (torch.randn(1, 1, 24, 64, generator=g) * 0.5).to(BF), (torch.randn(1, 1, 24, 64, generator=g) * 0.5).to(BF)
    pm, nm = torch.zeros(1, 24, dtype=torch.int64), torch.zeros(1, 24, dtype=torch.int64)
    pm[:, :19] = 1
    nm[:, :7] = 1
    np.savez(os.path.join(root, "embeds.npz"), prompt_embeds=pe.float().numpy(), prompt_attention_mask=pm.numpy(),
             negative_prompt_embeds=ne.float().numpy(), negative_prompt_attention_mask=nm.numpy())
    from safetensors.torch import save_file
    save_file({"prompt_embeds": pe, "prompt_attention_mask": pm}, os.path.join(root, "embeds_positive.safetensors"))
    text = dict(prompt_embeds=pe, prompt_attention_mask=pm, negative_prompt_embeds=ne, negative_prompt_attention_mask=nm)
    return root, text


def _positive(text):
    return dict(prompt_embeds=text["prompt_embeds"], prompt_attention_mask=text["prompt_attention_mask"])


def _pipe(vae, dit):
    from worldforge_amd.longcat_pipeline import LongCatVideoPipeline
    from worldforge_amd.longcat_scheduler import FlowMatchEulerDiscreteScheduler
    return LongCatVideoPipeline(vae, FlowMatchEulerDiscreteScheduler(shift=3.0), dit, device=DEV)


def _dit(root):
    return _model_cls()[1].from_pretrained(root, device=DEV)


def _gen(seed=42):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _u8(x):
    return (x * 255).astype(np.uint8)


SIZE = dict(height=64, width=96, num_frames=9)


@functools.lru_cache(maxsize=None)
def _real_vae():
    """The real-config VAE as the bf16 module the entry loads (synthetic weights; never written to disk)."""
    from oracle import vae as ovae
    from worldforge_amd.vae import AutoencoderKLWan
    return AutoencoderKLWan(DEV, precision="bf16", dtype=BF).load_state_dict(ovae.random_weights(seed=4))


@pytest.mark.parametrize("guided", [True, False])
def test_run_on_the_truck_fixture_equals_the_direct_generate_i2v_call(folder, tmp_path, guided):
    """DiT and scheduler from the folder, the VAE injected: guided (CFG 4, IRR, FLF, DSG, softened masks) and plain (no CFG)."""
    from worldforge_amd import harness, longcat_infer
    root, text = folder
    vae = _real_vae()
    kw = dict(guided=True, resample_steps=2, guide_steps=3, resample_round=3, use_pca_channel_selection=True, static=True) if guided else {}
    scale = 4.0 if guided else 1.0
    r = longcat_infer.run(root, TRUCK, output=str(tmp_path / "out" / "truck.mp4"), embeds=os.path.join(root, "embeds.npz"),
                          num_inference_steps=3, guidance_scale=scale, soften_mask=guided, max_replace=2 if guided else None,
                          components={"vae": vae}, device=DEV, **SIZE, **kw)
    assert r.frames.shape == (9, 64, 96, 3) and r.frames.dtype == np.float32 and np.isfinite(r.frames).all()
    assert r.refined is None and r.refined_png_dir is None and len(r.windows) == 1
    files = sorted(os.listdir(r.png_dir))
    assert files == [f"frame_{i:04d}.png" for i in range(9)] and r.png_dir.endswith("truck_frames")
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(os.path.join(r.png_dir, files[4]))), (r.frames[4] * 255).clip(0, 255).astype(np.uint8))
    # the same job wired by hand
    image, ref, mask, h, w = harness.prepare_inputs(TRUCK, soften=guided, device=torch.device(DEV), size=(64, 96))
    assert (h, w) == (64, 96)
    t = text if guided else _positive(text)
    want = _pipe(vae, _dit(root)).generate_i2v(image=image, height=h, width=w, **t, num_frames=9, num_inference_steps=3, guidance_scale=scale,
                                               generator=_gen(), video_ref=ref, mask=mask, max_replace_threshold=2 if guided else None, **kw)[0]
    assert np.array_equal(r.frames, want)
    if guided:   # the guidance is in the result: the plain job differs
        plain = _pipe(vae, _dit(root)).generate_i2v(image=image, height=h, width=w, **t, num_frames=9, num_inference_steps=3,
                                                    guidance_scale=scale, generator=_gen())[0]
        assert not np.array_equal(plain, want)


def test_use_distill_equals_the_manual_lora_switch_and_embeds_round_trip(folder, tmp_path):
    from worldforge_amd import harness, longcat_infer
    root, text = folder
    common = dict(num_inference_steps=3, components={"vae": FakeVAE()}, device=DEV, **SIZE)
    r = longcat_infer.run(root, TRUCK, output=str(tmp_path / "d.mp4"), embeds=os.path.join(root, "embeds.npz"), use_distill=True,
                          guidance_scale=4.0, **common)      # the guidance scale is forced to 1.0: no negative pass
    image, ref, mask, h, w = harness.prepare_inputs(TRUCK, soften=False, device=torch.device(DEV), size=(64, 96))
    dit = _dit(root)
    dit.load_lora(os.path.join(root, "lora", "cfg_step_lora.safetensors"), "cfg_step_lora")
    dit.enable_loras(["cfg_step_lora"])
    assert dit.active_loras == ["cfg_step_lora"]
    job = dict(image=image, height=h, width=w, **_positive(text), num_frames=9, num_inference_steps=3, guidance_scale=1.0, video_ref=ref, mask=mask)
    want = _pipe(FakeVAE(), dit).generate_i2v(use_distill=True, generator=_gen(), **job)[0]
    assert np.array_equal(r.frames, want)
    dit.disable_all_loras()
    base = _pipe(FakeVAE(), dit).generate_i2v(use_distill=True, generator=_gen(), **job)[0]
    assert not np.array_equal(base, want)                   # the adapter is in the result
    # --embeds: the positive pair alone serves a guidance scale of 1, from either container; above 1 the negative pair is required
    plain = _pipe(FakeVAE(), dit).generate_i2v(generator=_gen(), **job)[0]
    for name in ("embeds.npz", "embeds_positive.safetensors"):
        got = longcat_infer.run(root, TRUCK, output=str(tmp_path / "e.mp4"), embeds=os.path.join(root, name), guidance_scale=1.0, **common)
        assert np.array_equal(got.frames, plain), name
    with pytest.raises(ValueError, match="negative_prompt_embeds"):
        longcat_infer.run(root, TRUCK, output=str(tmp_path / "e.mp4"), embeds=os.path.join(root, "embeds_positive.safetensors"),
                          guidance_scale=4.0, **common)
    # another seed is another video
    other = longcat_infer.run(root, TRUCK, output=str(tmp_path / "e.mp4"), embeds=os.path.join(root, "embeds.npz"), guidance_scale=1.0,
                              seed=43, **common)
    assert not np.array_equal(other.frames, plain)


@pytest.mark.parametrize("no_kv_cache", [False, True])
def test_extend_windows_equals_the_hand_written_generate_vc_loop(folder, tmp_path, no_kv_cache):
    from worldforge_amd import harness, longcat_infer
    root, text = folder
    dit = _dit(root)
    builds = []
    cache_condition = dit.cache_condition
    dit.cache_condition = lambda *a, **k: (builds.append(1), cache_condition(*a, **k))[1]
    r = longcat_infer.run(root, TRUCK, output=str(tmp_path / "x.mp4"), embeds=os.path.join(root, "embeds.npz"), num_inference_steps=2,
                          guidance_scale=4.0, extend_windows=2, num_cond_frames=5, no_kv_cache=no_kv_cache,
                          components={"vae": FakeVAE(), "dit": dit}, device=DEV, **SIZE)
    assert len(builds) == (0 if no_kv_cache else 2)          # one condition cache per continued window, or the uncached route
    assert r.frames.shape == (9 + 2 * (9 - 5), 64, 96, 3) and len(r.windows) == 3 and all(w.shape == (9, 64, 96, 3) for w in r.windows)
    assert sorted(os.listdir(r.png_dir)) == [f"frame_{i:04d}.png" for i in range(17)]
    # by hand
    image, ref, mask, h, w = harness.prepare_inputs(TRUCK, soften=False, device=torch.device(DEV), size=(64, 96))
    pipe, g = _pipe(FakeVAE(), dit), _gen()
    job = dict(height=h, width=w, **text, num_frames=9, num_inference_steps=2, guidance_scale=4.0, generator=g)
    wins = [pipe.generate_i2v(image=image, video_ref=ref, mask=mask, **job)[0]]
    for _ in range(2):
        wins.append(pipe.generate_vc(video=_u8(wins[-1]), num_cond_frames=5, use_kv_cache=not no_kv_cache, enhance_hf=False, **job)[0])
    for got, want in zip(r.windows, wins):
        assert np.array_equal(got, want)
    assert np.array_equal(r.frames, np.concatenate([wins[0], wins[1][5:], wins[2][5:]]))
    assert not np.array_equal(wins[1], wins[2])


@pytest.mark.parametrize("extend,refine_kv_cache", [(0, False), (1, False), (1, True)])
def test_enable_upscale_equals_the_direct_lora_switch_and_generate_refine(folder, tmp_path, extend, refine_kv_cache):
    from worldforge_amd import harness, longcat_infer
    root, text = folder
    dit = _dit(root)
    assert dit.bsa_params == ck.BSA and not dit._bsa
    builds = []
    cache_condition_blocks = dit.cache_condition_blocks
    dit.cache_condition_blocks = lambda *a, **k: (builds.append(1), cache_condition_blocks(*a, **k))[1]
    r = longcat_infer.run(root, TRUCK, output=str(tmp_path / "u.mp4"), embeds=os.path.join(root, "embeds.npz"), num_inference_steps=2,
                          guidance_scale=1.0, enable_upscale=True, upscale_height=64, upscale_width=128, refine_num_inference_steps=2,
                          extend_windows=extend, num_cond_frames=5, refine_kv_cache=refine_kv_cache,
                          components={"vae": FakeVAE(), "dit": dit}, device=DEV, **SIZE)
    assert dit.active_loras == [] and not dit._bsa and set(dit.lora_dict) == {"refinement_lora"}
    assert len(builds) == (1 if refine_kv_cache else 0)      # the block-ordered condition cache of the continued window, or none
    dit.cache_condition_blocks = cache_condition_blocks
    n = 9 + extend * 4
    assert r.frames.shape == (n, 64, 96, 3) and r.refined.shape == (n, 64, 128, 3) and np.isfinite(r.refined).all()
    assert r.refined_png_dir.endswith("u_720p_frames") and sorted(os.listdir(r.refined_png_dir)) == [f"frame_{i:04d}.png" for i in range(n)]
    assert r.png_dir.endswith("u_frames") and len(os.listdir(r.png_dir)) == n
    # by hand
    image, ref, mask, h, w = harness.prepare_inputs(TRUCK, soften=False, device=torch.device(DEV), size=(64, 96))
    first = harness.read_frames_from_directory(TRUCK)[2].resize((128, 64))
    pipe, g = _pipe(FakeVAE(), dit), _gen()
    job = dict(height=h, width=w, **_positive(text), num_frames=9, num_inference_steps=2, guidance_scale=1.0, generator=g)
    wins = [pipe.generate_i2v(image=image, video_ref=ref, mask=mask, **job)[0]]
    for _ in range(extend):
        wins.append(pipe.generate_vc(video=_u8(wins[-1]), num_cond_frames=5, use_kv_cache=True, enhance_hf=False, **job)[0])
    dit.load_lora(os.path.join(root, "lora", "refinement_lora.safetensors"), "refinement_lora")
    dit.enable_loras(["refinement_lora"])
    dit.enable_bsa()
    refine = dict(height=64, width=128, **_positive(text), num_inference_steps=2, generator=_gen(), spatial_refine_only=True, t_thresh=0.6)
    ref0 = pipe.generate_refine(stage1_video=_u8(wins[0]), image=first, num_cond_frames=1, **refine)[0]
    refs = [ref0]
    if extend:
        refs.append(pipe.generate_refine(stage1_video=_u8(wins[1]), video=_u8(ref0), num_cond_frames=5, use_kv_cache=refine_kv_cache, **refine)[0])
    unswitched = None
    dit.disable_all_loras()
    if not extend:   # the adapter is in the result
        unswitched = pipe.generate_refine(stage1_video=_u8(wins[0]), image=first, num_cond_frames=1, **{**refine, "generator": _gen()})[0]
    dit.disable_bsa()
    for got, want in zip(r.windows + r.refined_windows, wins + refs):
        assert np.array_equal(got, want)
    assert len(r.refined_windows) == 1 + extend
    assert np.array_equal(r.refined, np.concatenate([refs[0]] + [x[5:] for x in refs[1:]]))
    if unswitched is not None:
        assert not np.array_equal(unswitched, ref0)


def test_pipeline_from_pretrained_takes_components_and_loads_the_rest(folder):
    from worldforge_amd.longcat_pipeline import LongCatVideoPipeline
    root, _ = folder
    vae = FakeVAE()
    pipe = LongCatVideoPipeline.from_pretrained(root, device=DEV, components={"vae": vae}, dit_precision="mxfp8", flow_backend="tdiff")
    assert pipe.vae is vae and pipe.dit.linear_precision == "mxfp8" and pipe.scheduler.flow_backend == "tdiff"
    assert pipe.scheduler.config.shift == 3.0 and pipe.dit.cfg.adaln_tembed_dim == 32
    with pytest.raises(ValueError, match="components"):
        LongCatVideoPipeline.from_pretrained(root, device=DEV, components={"transformer": None})
    with open(os.path.join(root, "dit", "config.json")) as f:
        assert json.load(f)["_class_name"] == "LongCatVideoTransformer3DModel"
