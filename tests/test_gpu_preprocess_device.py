"""The two front ends' device preprocessing against their host functions, torch.equal: vggt.preprocess_device against vggt.preprocess on
the recorded inputs of g26_vggt_preprocess.npz (the portrait one takes the crop), clip.preprocess_device against clip.preprocess on the
recorded inputs of g25_clip_pre_* under each of Pillow's five convolution filters.  The yardstick is the host function, which the host
suites pin to the recordings; the refusals are the host functions' own."""
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

from tests import clip_cases as cc
from tests import vggt_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pre():
    return vc.fixture()["preprocess"]


# ---- VGGT -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hw", [("landscape", (308, 518)), ("portrait", (518, 518))])
def test_vggt_preprocess_device_equals_the_host_function(pre, name, hw):
    from worldforge_amd import vggt
    img = Image.fromarray(pre[name + "_in"])
    want = vggt.preprocess([img])
    got = vggt.preprocess_device([img], DEV)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (1, 3) + hw == tuple(want.shape)
    assert torch.equal(got.cpu(), want)
    # N = 2 through one call (equal source sizes), and a u8 array / a u8 tensor that is already on the device in place of the PIL image
    two = vggt.preprocess_device([img, img], DEV)
    assert tuple(two.shape) == (2, 3) + hw and torch.equal(two.cpu(), want.expand(2, -1, -1, -1))
    dev_u8 = torch.from_numpy(pre[name + "_in"]).to(DEV)
    assert torch.equal(vggt.preprocess_device([dev_u8], DEV).cpu(), want)
    assert torch.equal(vggt.preprocess_device([pre[name + "_in"], dev_u8.cpu()], DEV).cpu(), want.expand(2, -1, -1, -1))


def test_vggt_images_of_two_source_sizes_and_an_rgba_image(pre):
    from worldforge_amd import vggt
    a = Image.fromarray(pre["landscape_in"])
    b = a.resize((a.width // 2, a.height // 2))                  # another source size that ends with the same shape
    want = vggt.preprocess([a, b, a])
    got = vggt.preprocess_device([a, b, a], DEV)
    assert tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want)
    rgba = np.concatenate([pre["landscape_in"], np.full(pre["landscape_in"].shape[:2] + (1,), 255, np.uint8)], -1)
    rgba[:10, :, 3] = 0                                          # transparent rows become white
    rgba[10:20, :, 3] = 128                                      # and half-transparent ones blend
    img = Image.fromarray(rgba, "RGBA")
    want = vggt.preprocess([img])
    assert bool((want[0, :, 0] == 1.0).all())
    assert torch.equal(vggt.preprocess_device([img], DEV).cpu(), want)
    grey = Image.fromarray(pre["landscape_in"][..., 0])          # mode L is converted to RGB on the host, as in preprocess
    assert torch.equal(vggt.preprocess_device([grey], DEV).cpu(), vggt.preprocess([grey]))


def test_vggt_refusals_are_the_host_functions(pre):
    from worldforge_amd import vggt
    land, port = Image.fromarray(pre["landscape_in"]), Image.fromarray(pre["portrait_in"])
    for fn in (vggt.preprocess, lambda images, **kw: vggt.preprocess_device(images, DEV, **kw)):
        with pytest.raises(NotImplementedError, match="pad"):
            fn([land], mode="pad")
        with pytest.raises(NotImplementedError, match="mixed shapes"):
            fn([land, port])
        with pytest.raises(ValueError):
            fn([])
        with pytest.raises(ValueError):
            fn([land], mode="stretch")
    with pytest.raises(TypeError):
        vggt.preprocess_device([torch.zeros(4, 4, 3)], DEV)
    with pytest.raises(TypeError):
        vggt.preprocess_device(["a.png"], DEV)


# ---- CLIP -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", [1, 2, 3, 4, 5])
def test_clip_preprocess_device_equals_the_host_function(resample):
    from worldforge_amd import clip
    pc, cases = cc.preprocess_fixture()
    pc = {**pc, "resample": resample}
    for img, _ in cases:
        pil = Image.fromarray(img)
        want = clip.preprocess(pil, pc)
        got = clip.preprocess_device(pil, pc, DEV)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, 224, 224)
        assert torch.equal(got.cpu(), want), (resample, float((got.cpu() - want).abs().max()))
        assert torch.equal(clip.preprocess_device(torch.from_numpy(img).to(DEV), pc, DEV).cpu(), want)
        assert torch.equal(clip.preprocess_device(torch.from_numpy(img), pc, DEV).cpu(), want)


def test_clip_recorded_pixel_values_a_grey_image_and_another_crop():
    from worldforge_amd import clip
    pc, cases = cc.preprocess_fixture()
    for img, recorded in cases:
        assert np.array_equal(clip.preprocess_device(Image.fromarray(img), pc, DEV).cpu().numpy(), recorded)
    grey = Image.fromarray(cases[0][0][..., 0])
    assert torch.equal(clip.preprocess_device(grey, pc, DEV).cpu(), clip.preprocess(grey, pc))
    small = {**pc, "size": {"shortest_edge": 96}, "crop_size": 64, "rescale_factor": 0.004, "image_mean": [0.1, 0.5, 0.9], "image_std": [0.3, 0.2, 0.1]}
    for img, _ in cases:
        assert torch.equal(clip.preprocess_device(Image.fromarray(img), small, DEV).cpu(), clip.preprocess(Image.fromarray(img), small))


def test_clip_refusals_match_the_host_functions():
    from worldforge_amd import clip
    pc, cases = cc.preprocess_fixture()
    pil = Image.fromarray(cases[0][0])
    with pytest.raises(NotImplementedError, match="NEAREST"):
        clip.preprocess_device(pil, {**pc, "resample": 0}, DEV)
    assert tuple(clip.preprocess(pil, {**pc, "resample": 0}).shape) == (3, 224, 224)      # the host route keeps serving it
    for bad in ({"do_center_crop": False}, {"do_normalize": False}, {"do_resize": False}, {"do_rescale": False}, {"do_convert_rgb": False},
                {"size": {"height": 224, "width": 224}}, {"do_pad": True}, {"resample": 9}, {"crop_size": {"height": 224, "width": 200}},
                {"size": {"shortest_edge": 100}}, {"image_mean": None}, {"image_std": [0.5]}):
        messages = []
        for fn in (lambda c: clip.preprocess(pil, c), lambda c: clip.preprocess_device(pil, c, DEV)):
            with pytest.raises(NotImplementedError) as e:
                fn({**pc, **bad})
            messages.append(str(e.value))
        assert messages[0] == messages[1], bad
    with pytest.raises(TypeError):
        clip.preprocess_device("a.png", pc, DEV)
    with pytest.raises(TypeError):
        clip.preprocess_device(torch.zeros(8, 8, 3), pc, DEV)


# ---- wiring -----------------------------------------------------------------------------------------------------------------------------
def test_infer_run_in_process_hands_encode_image_the_device_frame(tmp_path, monkeypatch):
    """infer.run with stage-1 tensors, --image-encoder native and no --image: clip.encode_image gets the first frame at the sampler's size
    as a u8 tensor on the device, with the bits of the PIL image the pipeline gets; with --image it gets that PIL image."""
    from worldforge_amd import clip, dit, harness, infer, pipeline, vae
    mp = tmp_path / "wan2.1_480p_model_local"
    for d in ("text_encoder", "tokenizer", "image_encoder", "image_processor"):
        os.makedirs(mp / d)
    monkeypatch.setattr(vae.AutoencoderKLWan, "from_pretrained", classmethod(lambda cls, *a, **k: "vae"))
    monkeypatch.setattr(dit.WanTransformer3DModel, "from_pretrained", classmethod(lambda cls, *a, **k: "dit"))
    monkeypatch.setattr(harness, "save_png_frames", lambda frames, output: "png")
    calls = {}

    def fake_text(model_path, prompt, negative_prompt, device, max_sequence_length=512, tokenizer=None):
        return {"prompt_embeds": torch.zeros(1, 512, 8), "negative_prompt_embeds": torch.ones(1, 512, 8)}

    def fake_image(model_path, image, device, subfolder="image_encoder"):
        calls["image"] = image
        return torch.full((1, 257, 4), 0.5, dtype=torch.bfloat16)

    class Pipe:
        def __init__(self, *a, **k):
            pass

        def __call__(self, **kw):
            calls["pipe"] = kw
            return types.SimpleNamespace(frames=[np.zeros((5, 8, 8, 3), np.float32)])

    monkeypatch.setattr(infer, "encode_text_native", fake_text)
    monkeypatch.setattr(clip, "encode_image", fake_image)
    monkeypatch.setattr(pipeline, "WanImageToVideoPipeline", Pipe)
    g = torch.Generator().manual_seed(3)
    images = torch.randint(0, 256, (5, 45, 83, 3), generator=g, dtype=torch.uint8).to(DEV)
    masks = torch.randint(0, 2, (5, 45, 83), generator=g, dtype=torch.uint8).to(DEV)
    kw = dict(model="480p", num_frames=5, prompt="a truck", device=DEV, text_encoder="native", image_encoder="native", max_area=64 * 96,
              output=str(tmp_path / "out.mp4"))
    infer.run(str(tmp_path), None, stage1_frames=(images, masks), **kw)
    pil = calls["pipe"]["image"]
    got = calls["image"]
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (pil.height, pil.width, 3)
    assert (pil.height, pil.width) != (45, 83) and np.array_equal(got.cpu().numpy(), np.asarray(pil))
    other = Image.fromarray(images[1].cpu().numpy())
    infer.run(str(tmp_path), None, stage1_frames=(images, masks), image=other, **kw)
    assert calls["image"] is calls["pipe"]["image"] and isinstance(calls["image"], Image.Image)
