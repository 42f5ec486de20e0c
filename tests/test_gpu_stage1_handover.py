"""Stage 1 handed to the sampler on the device against the two-command route through PNG files.

(a) harness.prepare_inputs_device on the tensors of warp.warp_single_img (a recorded g28 scene) and warp.warp_depthcrafter_frames (a g29
    case) against harness.prepare_inputs on the files the stage-1 writers make of the same tensors: video_ref, mask, height, width and
    the PIL image are EQUAL (torch.equal) -- with softening on and off, with and without `image=`, shrinking (max_area) and enlarging
    (size=).
(b) infer.run / longcat_infer.run with --stage1 vggt and --stage1 depthcrafter against the stage-1 command followed by run(video_ref=...)
    on the same inputs: np.array_equal frames.  Both sides run the same kernels on equal tensors, so there is no tolerance.
(c) a frame-count mismatch raises the entry's ValueError before the DiT is loaded."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import dynwarp_cases as dc
from tests import stage1_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


# ---- (a) the tensors --------------------------------------------------------------------------------------------------------------------
G28 = "s90_c080_left"          # 5 frames of 90 x 160 with holes, confidence filter on
G29 = "c_native_left_edge"     # 2 frames of 288 x 304, the scene with real masks


@functools.lru_cache(maxsize=None)
def _g28():
    from worldforge_amd import warp
    fx = sc.fixture()
    c = fx["cases"][G28]
    s = fx["scenes"][c["scene"]]
    imgs, masks, infos = warp.warp_single_img(s["E"], s["K"], torch.from_numpy(s["image"]).permute(2, 0, 1), s["depth"], depth_conf=s["conf"],
                                              direction=c["direction"], degree=c["degree"], conf_threshold=c["thr"],
                                              frame_num=fx["meta"]["frame_num"], fill_cracks=True, crack_params=fx["meta"]["crack_params"],
                                              look_at_depth=1.0, depth_segments=8, device=DEV)
    args = argparse.Namespace(direction=c["direction"], degree=c["degree"], frame_single=fx["meta"]["frame_num"], conf_single=c["thr"],
                              fill_cracks=True)
    return imgs, masks, infos, args


@functools.lru_cache(maxsize=None)
def _g29():
    from worldforge_amd import warp
    s = dc.scene(dc.CASES[G29]["scene"])
    imgs, masks, _ = warp.warp_depthcrafter_frames(s["frames_native"], s["disparity"], device=DEV, **dc.options(G29))
    return imgs, masks


def _write(source, folder):
    """The tensors through the stage-1 command's own PNG writer -> the folder --video-ref would name."""
    from worldforge_amd import run_warp, warp_depthcrafter
    if source == "g28":
        imgs, masks, infos, args = _g28()
        return imgs, masks, run_warp.save_warped_results(imgs.cpu().numpy(), masks.cpu().numpy(), infos, str(folder), 0, args)
    imgs, masks = _g29()
    return imgs, masks, warp_depthcrafter.save_frames(imgs.cpu().numpy(), masks.cpu().numpy(), str(folder / "warped" / "imgs"))


def _other_image():
    """An input image of another aspect ratio than the warped frames: the size rule follows IT."""
    return Image.fromarray(np.random.default_rng(3).integers(0, 256, (60, 100, 3), dtype=np.uint8), "RGB")


def _same(a, b):
    ia, va, ma, ha, wa = a
    ib, vb, mb, hb, wb = b
    assert (ha, wa) == (hb, wb) and ia.size == ib.size and ia.mode == ib.mode and np.array_equal(np.asarray(ia), np.asarray(ib))
    assert va.dtype == vb.dtype == torch.float32 and va.shape == vb.shape and va.device == vb.device and torch.equal(va, vb)
    assert ma.dtype == mb.dtype == torch.float32 and ma.shape == mb.shape and ma.device == mb.device and torch.equal(ma, mb)


@pytest.mark.parametrize("with_image", [False, True], ids=["first_frame", "image"])
@pytest.mark.parametrize("soften", [True, False], ids=["soften", "plain"])
@pytest.mark.parametrize("source", ["g28", "g29"])
def test_prepare_inputs_device_equals_the_file_route(source, soften, with_image, tmp_path):
    from worldforge_amd import harness
    imgs, masks, folder = _write(source, tmp_path)
    assert set(np.unique(masks.cpu().numpy())) == {0, 1}                      # real holes: the masks are not constant
    kw = dict(soften=soften, transition_distance=5, decay_type="sine", device=torch.device(DEV), max_area=64 * 96,
              image=_other_image() if with_image else None)
    want = harness.prepare_inputs(folder, **kw)
    got = harness.prepare_inputs_device(imgs, masks, **kw)
    _same(got, want)
    F, H, W = masks.shape
    assert got[3] < H and got[4] < W and tuple(got[1].shape) == (1, 3, F, got[3], got[4]) and tuple(got[2].shape) == (1, 1, F, got[3], got[4])
    if with_image:                                                              # a path is read like the PIL image
        path = tmp_path / "input.png"
        _other_image().save(path)
        _same(harness.prepare_inputs_device(imgs, masks, **{**kw, "image": str(path)}), want)


@pytest.mark.parametrize("source,size", [("g28", (112, 192)), ("g29", (304, 320))])
def test_prepare_inputs_device_enlarges_like_the_file_route(source, size, tmp_path):
    from worldforge_amd import harness
    imgs, masks, folder = _write(source, tmp_path)
    kw = dict(soften=True, decay_type="linear", device=torch.device(DEV), size=size)
    got = harness.prepare_inputs_device(imgs, masks, **kw)
    _same(got, harness.prepare_inputs(folder, **kw))
    assert (got[3], got[4]) == size and size[0] > masks.shape[1] and size[1] > masks.shape[2]


def test_prepare_inputs_device_refuses_what_it_cannot_take():
    from worldforge_amd import harness
    imgs, masks = _g29()
    with pytest.raises(RuntimeError, match="GPU"):
        harness.prepare_inputs_device(imgs.cpu(), masks.cpu())
    with pytest.raises(TypeError, match="images_u8"):
        harness.prepare_inputs_device(imgs.float(), masks)
    with pytest.raises(TypeError, match="masks_u8"):
        harness.prepare_inputs_device(imgs, masks[:1])
    with pytest.raises(ValueError, match="0 / 1"):              # 0 / 255 masks would wrap in the uint8 scaling
        harness.prepare_inputs_device(imgs, masks * 255)


# ---- (b) the entry points ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vggt_inputs(tmp_path_factory):
    """The synthetic VGGT checkpoint folder and three views of one image, as tests/test_gpu_stage1.py feeds run_warp.main."""
    from tests import vggt_cases as vc, vggt_depth_cases as vd
    root = tmp_path_factory.mktemp("stage1_vggt")
    fx = vd.fixture()
    ckpt = vc.write_folder(str(root / "ckpt"), sd=fx["sd"], config=fx["chain_config"])
    src = vc.fixture()["preprocess"]["landscape_in"]
    os.makedirs(root / "imgs")
    for i in range(3):
        Image.fromarray(np.roll(src, 40 * i, axis=1)).save(str(root / "imgs" / f"{i}.png"))
    return ckpt, str(root / "imgs")


@pytest.fixture(scope="module")
def dc_inputs(tmp_path_factory):
    """A frame folder and its depth file: the five native frames of g29's scene a."""
    root = tmp_path_factory.mktemp("stage1_dc")
    s = dc.scene("a")
    os.makedirs(root / "clip")
    for i, f in enumerate(s["frames_native"]):
        Image.fromarray(f, "RGB").save(root / "clip" / f"frame_{i:03d}.png")
    np.savez_compressed(root / "depth.npz", depth=s["disparity"])
    return str(root / "clip"), str(root / "depth.npz")


VGGT_OPTS = dict(camera=1, direction="left", degree=20.0, conf_single=0.8)
VGGT_ARGV = ["--camera", "1", "--direction", "left", "--degree", "20", "--conf_single", "0.8", "--frame_single", "5"]
DC_OPTS = dict(direction="right", degree=9.0, enable_edge_filter=True)
DC_ARGV = ["--direction", "right", "--degree", "9.0", "--enable_edge_filter"]


@functools.lru_cache(maxsize=None)
def _wan():
    from oracle import dit as odit
    from oracle import vae as ovae
    from worldforge_amd import dit
    from worldforge_amd.vae import AutoencoderKLWan
    cfg = dict(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    model = dit.WanTransformer3DModel(dit.DiTConfig(**cfg), torch.device(DEV)).load_state_dict(odit.random_weights(odit.DiTConfig(**cfg), seed=3))
    return model, AutoencoderKLWan(torch.device(DEV)).load_state_dict(ovae.random_weights(seed=4))


def _wan_run(tmp_path, tag, video_ref, **more):
    from worldforge_amd import infer
    from worldforge_amd.scheduler import UniPCMultistepScheduler
    emb = tmp_path / "embeds.npz"
    if not emb.exists():
        g = torch.Generator().manual_seed(1)
        np.savez(emb, prompt_embeds=(torch.randn(1, 24, 64, generator=g) * 0.5).numpy(),
                 negative_prompt_embeds=(torch.randn(1, 24, 64, generator=g) * 0.5).numpy(), image_embeds=torch.randn(1, 257, 1280, generator=g).numpy())
    model, vae = _wan()
    kw = dict(guided=True, resample_steps=2, guide_steps=2, resample_round=2, omega=4.0, omega_resample=4.0, num_frames=5, num_inference_steps=3,
              guidance_scale=4.0, use_pca_channel_selection=True, soften_mask=True, static=True)
    kw.update(more)
    return infer.run(None, video_ref, model="480p", output=str(tmp_path / tag / "out.mp4"), embeds=str(emb), device=DEV, max_area=64 * 112,
                     components=dict(transformer=model, vae=vae, scheduler=UniPCMultistepScheduler(flow_shift=3.0)), **kw)[0]


def _files(folder):
    out = {}
    for n in sorted(os.listdir(folder)):
        with open(os.path.join(folder, n), "rb") as f:
            out[n] = f.read()
    return out


def test_infer_run_with_stage1_vggt_equals_run_warp_then_infer(vggt_inputs, tmp_path):
    from worldforge_amd import run_warp
    ckpt, imgs = vggt_inputs
    out = str(tmp_path / "warp")
    assert run_warp.main(["--checkpoint", ckpt, "--image_path", imgs, "--output_path", out, "--device", DEV] + VGGT_ARGV) == 0
    want = _wan_run(tmp_path, "files", os.path.join(out, "warped_images"))
    # --frame_single is not given: it defaults to the 5 frames that --num-frames 5 decodes
    got = _wan_run(tmp_path, "vggt", None, stage1="vggt", vggt_checkpoint=ckpt, image_path=imgs, save_stage1=str(tmp_path / "saved"), **VGGT_OPTS)
    assert got.shape[0] == 5 and got.shape[1] < 300 and np.isfinite(got).all() and np.array_equal(got, want)
    # --save-stage1 writes what the stage-1 command writes
    assert _files(os.path.join(out, "warped_images")) == _files(str(tmp_path / "saved" / "warped_images"))
    with open(os.path.join(out, "camera_info.txt"), "rb") as f, open(tmp_path / "saved" / "camera_info.txt", "rb") as g:
        assert f.read() == g.read()


def test_infer_run_with_stage1_depthcrafter_equals_the_command_then_infer(dc_inputs, tmp_path):
    from worldforge_amd import warp_depthcrafter as wd
    clip, npz = dc_inputs
    out = tmp_path / "dc"
    assert wd.main(["--video_path", clip, "--depth_npz", npz, "--output_path", str(out), "--device", DEV] + DC_ARGV) == 0
    want = _wan_run(tmp_path, "files", str(out / "warped" / "imgs"))
    got = _wan_run(tmp_path, "dc", None, stage1="depthcrafter", video_path=clip, depth_npz=npz, save_stage1=str(tmp_path / "saved"), **DC_OPTS)
    assert got.shape == (5, 64, 96, 3) and np.array_equal(got, want)                     # 48 x 80 frames, enlarged by the size rule
    assert _files(str(out / "warped" / "imgs")) == _files(str(tmp_path / "saved" / "warped" / "imgs"))


@pytest.fixture(scope="module")
def longcat_folder(tmp_path_factory):
    """dit/ and scheduler/ of the tiny LongCat model plus an embedding file (as tests/test_gpu_longcat_entry.py's folder)."""
    from tests import longcat_ckpt as ck
    root = str(tmp_path_factory.mktemp("stage1_longcat"))
    ck.write_dit(root, ck.weights(seed=3), config={"bsa_params": ck.BSA})
    ck.write_scheduler(root, shift=3.0)
    g = torch.Generator().manual_seed(7)
    pe = (torch.randn(1, 1, 24, 64, generator=g) * 0.5).to(BF)
    pm = torch.zeros(1, 24, dtype=torch.int64)
    pm[:, :19] = 1
    np.savez(os.path.join(root, "embeds.npz"), prompt_embeds=pe.float().numpy(), prompt_attention_mask=pm.numpy())
    return root


@functools.lru_cache(maxsize=None)
def _bf16_vae():
    from oracle import vae as ovae
    from worldforge_amd.vae import AutoencoderKLWan
    return AutoencoderKLWan(DEV, precision="bf16", dtype=BF).load_state_dict(ovae.random_weights(seed=4))


def _longcat_run(root, tmp_path, tag, video_ref, **more):
    from worldforge_amd import longcat_infer
    kw = dict(height=64, width=96, num_frames=5, num_inference_steps=2, guidance_scale=1.0, guided=True, resample_steps=2, guide_steps=2,
              resample_round=2, use_pca_channel_selection=True, static=True, soften_mask=True)
    kw.update(more)
    return longcat_infer.run(root, video_ref, output=str(tmp_path / tag / "out.mp4"), embeds=os.path.join(root, "embeds.npz"),
                             components={"vae": _bf16_vae()}, device=DEV, **kw)


@pytest.mark.parametrize("mode", ["vggt", "depthcrafter"])
def test_longcat_run_with_stage1_equals_the_command_then_run(mode, vggt_inputs, dc_inputs, longcat_folder, tmp_path):
    from worldforge_amd import run_warp, warp_depthcrafter as wd
    out = tmp_path / "stage1"
    if mode == "vggt":
        ckpt, imgs = vggt_inputs
        assert run_warp.main(["--checkpoint", ckpt, "--image_path", imgs, "--output_path", str(out), "--device", DEV] + VGGT_ARGV) == 0
        folder, opts = str(out / "warped_images"), dict(vggt_checkpoint=ckpt, image_path=imgs, **VGGT_OPTS)
    else:
        clip, npz = dc_inputs
        assert wd.main(["--video_path", clip, "--depth_npz", npz, "--output_path", str(out), "--device", DEV] + DC_ARGV) == 0
        folder, opts = str(out / "warped" / "imgs"), dict(video_path=clip, depth_npz=npz, **DC_OPTS)
    want = _longcat_run(longcat_folder, tmp_path, "files", folder)
    got = _longcat_run(longcat_folder, tmp_path, mode, None, stage1=mode, **opts)
    assert got.frames.shape == (5, 64, 96, 3) and np.isfinite(got.frames).all() and np.array_equal(got.frames, want.frames)


# ---- (c) refusals before the models ----------------------------------------------------------------------------------------------------
def test_a_frame_count_mismatch_is_refused_before_the_dit_is_loaded(dc_inputs, longcat_folder, tmp_path, monkeypatch):
    from worldforge_amd import infer, longcat_infer
    from worldforge_amd.longcat_pipeline import LongCatVideoPipeline
    clip, npz = dc_inputs
    imgs, masks = _g29()                                                               # 2 frames
    nowhere = str(tmp_path / "nowhere")                                                # loading from it would raise "Model path does not exist"
    for opts in (dict(stage1="depthcrafter", video_path=clip, depth_npz=npz, **DC_OPTS), dict(stage1_frames=(imgs, masks))):
        with pytest.raises(ValueError, match=r"holds \d frames but --num-frames 9 decodes 9"):
            infer.run(nowhere, None, model="480p", num_frames=9, device=DEV, **opts)

    def no_loading(cls, *a, **k):
        raise AssertionError("loaded")

    monkeypatch.setattr(LongCatVideoPipeline, "from_pretrained", classmethod(no_loading))
    emb = os.path.join(longcat_folder, "embeds.npz")
    for opts in (dict(stage1="depthcrafter", video_path=clip, depth_npz=npz, **DC_OPTS), dict(stage1_frames=(imgs, masks))):
        with pytest.raises(ValueError, match=r"holds \d frames but --num-frames 9 decodes 9"):
            longcat_infer.run(longcat_folder, None, embeds=emb, guidance_scale=1.0, num_frames=9, device=DEV, **opts)
    with pytest.raises(AssertionError, match="loaded"):                                 # with the right count, loading is what comes next
        longcat_infer.run(longcat_folder, None, embeds=emb, guidance_scale=1.0, num_frames=5, device=DEV, stage1="depthcrafter",
                          video_path=clip, depth_npz=npz, **DC_OPTS)
    with pytest.raises(TypeError, match="ignored"):                                     # tensors AND options: one of them would be ignored
        infer.run(nowhere, None, stage1_frames=(imgs, masks), direction="left", device=DEV)
