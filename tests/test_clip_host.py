"""CPU: the host half of the native CLIP vision encoder (worldforge_amd/clip.py): config rules, the key table, prefix handling, the loader's
errors, the audit component, the --image-encoder flag and its dispatch, the restated image preprocessing against the recorded
`CLIPImageProcessorPil` output -- and that every GPU case of tests/clip_cases.py can see a narrowed operand.  `transformers` is never
imported here."""
import json
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch

from tests import clip_cases as cc

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUCK = os.path.join(ROOT, "tests", "golden", "truck")


# ---- host rules ------------------------------------------------------------------------------------------------------------------------------
def test_config_defaults_are_vit_h_14_and_refusals():
    from worldforge_amd import clip
    c = clip.CLIPVisionConfig.from_dict({})
    assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.image_size, c.patch_size, c.hidden_act,
            c.layer_norm_eps) == (1280, 5120, 32, 16, 224, 14, "gelu", 1e-5)
    assert (c.head_dim, c.num_tokens, c.patch_dim) == (80, 257, 588)
    assert clip.CLIPVisionConfig.from_dict({"vision_config": {"hidden_act": "quick_gelu"}, "projection_dim": 512}).hidden_act == "quick_gelu"
    with pytest.raises(NotImplementedError, match="hidden_act"):
        clip.CLIPVisionConfig.from_dict({"hidden_act": "gelu_new"})
    with pytest.raises(NotImplementedError, match="head width"):
        clip.CLIPVisionConfig.from_dict({"hidden_size": 1152, "num_attention_heads": 8})        # 144-wide heads
    with pytest.raises(NotImplementedError, match="head width"):
        clip.CLIPVisionConfig.from_dict({"hidden_size": 1200, "num_attention_heads": 100})      # 12-wide heads
    with pytest.raises(ValueError, match="multiple"):
        clip.CLIPVisionConfig.from_dict({"patch_size": 15, "image_size": 225})                  # 3 * 225 = 675: K % 4 != 0
    with pytest.raises(ValueError, match="image_size"):
        clip.CLIPVisionConfig.from_dict({"image_size": 225})
    with pytest.raises(ValueError):
        clip.CLIPVisionConfig.from_dict({"hidden_size": 1290})
    with pytest.raises(NotImplementedError, match="tokens"):
        clip.CLIPVisionConfig.from_dict({"image_size": 448})                           # 1025 tokens
    with pytest.raises(NotImplementedError, match="num_channels"):
        clip.CLIPVisionConfig.from_dict({"num_channels": 1})


def test_key_table_at_the_released_size():
    from worldforge_amd import clip
    cfg = clip.CLIPVisionConfig()
    e = clip.expected_state_dict(cfg)
    assert len(e) == 5 + 32 * 16 + 2
    assert e["embeddings.patch_embedding.weight"] == (1280, 3, 14, 14) and e["embeddings.position_embedding.weight"] == (257, 1280)
    assert e["embeddings.class_embedding"] == (1280,) and e["pre_layrnorm.bias"] == (1280,)
    assert e["encoder.layers.31.mlp.fc1.weight"] == (5120, 1280) and e["encoder.layers.0.mlp.fc2.weight"] == (1280, 5120)
    assert e["encoder.layers.7.self_attn.k_proj.weight"] == (1280, 1280) and e["encoder.layers.7.self_attn.out_proj.bias"] == (1280,)
    up = clip.uploaded_keys(cfg)
    assert len(up) == 5 + 31 * 16 and not any(k.startswith(("encoder.layers.31.", "post_layernorm.")) for k in up)


def test_prefix_and_the_rest_of_a_full_clip_model_file():
    from worldforge_amd import clip
    cfg = clip.CLIPVisionConfig.from_dict(cc.fixture()["config"])
    e = clip.expected_state_dict(cfg)
    bare = {k: {"shape": s} for k, s in e.items()}
    pref = {"vision_model." + k: {"shape": s} for k, s in e.items()}
    for found in (bare, pref):
        keep, dropped, names = clip.consumed_header(found)
        assert dropped == 0 and set(keep) == set(e) and all(names[k] in found for k in keep)
    full = dict(pref)
    full.update({"text_model.embeddings.token_embedding.weight": {"shape": (9, 4)}, "visual_projection.weight": {"shape": (4, 160)},
                 "text_projection.weight": {"shape": (4, 4)}, "logit_scale": {"shape": ()},
                 "vision_model.embeddings.position_ids": {"shape": (1, 257)}})
    keep, dropped, _ = clip.consumed_header(full)
    assert dropped == 4 and set(keep) == set(e)


def test_loader_checks_headers_and_never_uploads_the_last_layer(tmp_path):
    from worldforge_amd import clip
    fx = cc.fixture()
    ok = cc.write_folder(str(tmp_path / "ok" / "image_encoder"), prefix="vision_model.")
    m = clip.CLIPVisionModel.from_pretrained(str(tmp_path / "ok"), device="cpu")
    assert m.n_layers == 2 and not any(k.startswith("2.") for k in m.W) and "0.qkv.w" in m.W and "1.fc2.b" in m.W
    assert tuple(m.W["0.qkv.w"].shape) == (480, 160) and tuple(m.W["0.qkv.b"].shape) == (480,) and m.W["pos"].dtype == F32
    assert torch.equal(m.W["0.qkv.w"][160:320], fx["sd"]["encoder.layers.0.self_attn.k_proj.weight"])
    assert torch.equal(m.W["pos"][0], fx["sd"]["embeddings.position_embedding.weight"][0] + fx["sd"]["embeddings.class_embedding"])
    assert torch.equal(m.W["pos"][1:], fx["sd"]["embeddings.position_embedding.weight"][1:])
    assert torch.equal(m.W["patch"], fx["sd"]["embeddings.patch_embedding.weight"].reshape(160, 48))
    m2 = clip.CLIPVisionModel.from_pretrained(ok, device="cpu")                                  # the encoder's own folder works too
    assert all(torch.equal(m.W[k], m2.W[k]) for k in m.W)
    cc.write_folder(str(tmp_path / "miss" / "image_encoder"), drop=("post_layernorm.bias",))       # checked although never uploaded
    with pytest.raises(KeyError, match="post_layernorm.bias"):
        clip.CLIPVisionModel.from_pretrained(str(tmp_path / "miss"), device="cpu")
    cc.write_folder(str(tmp_path / "extra" / "image_encoder"), extra={"encoder.stray": torch.zeros(2)})
    with pytest.raises(ValueError, match="not consumed"):
        clip.CLIPVisionModel.from_pretrained(str(tmp_path / "extra"), device="cpu")
    bad = dict(fx["sd"])
    bad["encoder.layers.2.mlp.fc1.bias"] = torch.zeros(321)
    cc.write_folder(str(tmp_path / "shape" / "image_encoder"), sd=bad)
    with pytest.raises(ValueError, match="wrong shape"):
        clip.CLIPVisionModel.from_pretrained(str(tmp_path / "shape"), device="cpu")
    cc.write_folder(str(tmp_path / "full" / "image_encoder"), prefix="vision_model.",
                    extra={"text_model.final_layer_norm.weight": torch.zeros(4), "logit_scale": torch.zeros(())})
    with pytest.warns(UserWarning, match="ignored"):
        clip.CLIPVisionModel.from_pretrained(str(tmp_path / "full"), device="cpu")
    with pytest.raises(FileNotFoundError):
        clip.CLIPVisionModel.from_pretrained(str(tmp_path / "nothing"), device="cpu")


def test_call_refuses_other_inputs_before_any_device_work():
    from worldforge_amd import clip
    fx = cc.fixture()
    m = clip.CLIPVisionModel(clip.CLIPVisionConfig.from_dict(fx["config"]), "cpu").load_state_dict(fx["sd"])
    for bad in (torch.zeros(3, 64, 60), torch.zeros(2, 3, 64, 64), torch.zeros(3, 64, 64, dtype=torch.float64), torch.zeros(3, 224, 224)):
        with pytest.raises(ValueError, match="pixel_values"):
            m(bad)
    for idx in (-1, 3, -5):
        with pytest.raises(ValueError, match="hidden_state_index"):
            m(torch.zeros(3, 64, 64), hidden_state_index=idx)
    with pytest.raises(RuntimeError, match="no weights"):
        clip.CLIPVisionModel(clip.CLIPVisionConfig.from_dict(fx["config"]), "cpu")(torch.zeros(3, 64, 64))


def test_audit_reports_the_image_encoder_only_when_the_folder_exists(tmp_path):
    from worldforge_amd import checkpoint
    root = tmp_path / "ckpt"
    os.makedirs(root / "scheduler")
    with open(root / "scheduler" / "scheduler_config.json", "w") as f:
        json.dump({"_class_name": "UniPCMultistepScheduler", "flow_shift": 3.0}, f)
    assert "image_encoder" not in checkpoint.audit(str(root))["components"]
    cc.write_folder(str(root / "image_encoder"), prefix="vision_model.", extra={"logit_scale": torch.zeros(())})
    rep = checkpoint.audit(str(root))
    c = rep["components"]["image_encoder"]
    assert c["kind"] == "CLIPVisionModel" and not (c["missing"] or c["unexpected"] or c["wrong_shape"] or c["refused"])
    assert sum(c["dtypes"].values()) == 5 + 3 * 16 + 2 + 1 and any("ignored" in n for n in c["notes"])
    assert "image_encoder (CLIPVisionModel)" in checkpoint.format_report(rep)
    cc.write_folder(str(root / "image_encoder"), drop=("pre_layrnorm.weight",), config={**cc.fixture()["config"], "hidden_act": "relu"})
    c = checkpoint.audit(str(root))["components"]["image_encoder"]
    assert c["refused"] and "hidden_act" in c["refused"][0]
    cc.write_folder(str(root / "image_encoder"), drop=("pre_layrnorm.weight",))
    rep = checkpoint.audit(str(root))
    assert rep["components"]["image_encoder"]["missing"] == ["pre_layrnorm.weight"] and not rep["ok"]


def test_cli_flag_parses_and_defaults_to_transformers():
    import argparse
    from worldforge_amd import infer
    seen = {}
    real = argparse.ArgumentParser.parse_args

    def grab(self, argv=None):
        ns = real(self, argv)
        seen.update(vars(ns))
        raise SystemExit(0)

    for extra, want in (([], "transformers"), (["--image-encoder", "native"], "native")):
        argparse.ArgumentParser.parse_args = grab
        try:
            with pytest.raises(SystemExit):
                infer.main(["--models-dir", "/nowhere", "--video-ref", TRUCK] + extra)
        finally:
            argparse.ArgumentParser.parse_args = real
        assert seen["image_encoder"] == want and seen["text_encoder"] == "transformers"
    with pytest.raises(ValueError, match="image-encoder"):
        infer.run("/nowhere", TRUCK, image_encoder="hf")


# ---- dispatch --------------------------------------------------------------------------------------------------------------------------------
def test_run_with_native_encoders_never_touches_the_hf_vision_classes(tmp_path, monkeypatch):
    """infer.run(..., text_encoder="native", image_encoder="native") on a folder with the four encoder directories: image_embeds come from
    clip.encode_image; a stand-in `transformers` whose every attribute raises proves that no Hugging Face class is imported."""
    from worldforge_amd import clip, dit, harness, infer, pipeline, vae

    class Poison(types.ModuleType):
        def __getattr__(self, name):
            raise AssertionError(f"transformers.{name} was touched")

    monkeypatch.setitem(sys.modules, "transformers", Poison("transformers"))
    mp = tmp_path / "wan2.1_480p_model_local"
    for d in ("text_encoder", "tokenizer", "image_encoder", "image_processor"):
        os.makedirs(mp / d)
    monkeypatch.setattr(vae.AutoencoderKLWan, "from_pretrained", classmethod(lambda cls, *a, **k: "vae"))
    monkeypatch.setattr(dit.WanTransformer3DModel, "from_pretrained", classmethod(lambda cls, *a, **k: "dit"))
    pil = object()
    monkeypatch.setattr(harness, "prepare_inputs", lambda *a, **k: (pil, torch.zeros(1, 3, 5, 8, 8), torch.zeros(1, 1, 5, 8, 8), 8, 8))
    monkeypatch.setattr(harness, "save_png_frames", lambda frames, output: "png")
    calls = {}

    def fake_text(model_path, prompt, negative_prompt, device, max_sequence_length=512, tokenizer=None):
        calls["text"] = (model_path, prompt)
        return {"prompt_embeds": torch.zeros(1, 512, 8), "negative_prompt_embeds": torch.ones(1, 512, 8)}

    def fake_image(model_path, image, device, subfolder="image_encoder"):
        calls["image"] = (model_path, image)
        return torch.full((1, 257, 4), 0.5, dtype=torch.bfloat16)

    monkeypatch.setattr(infer, "encode_text_native", fake_text)
    monkeypatch.setattr(clip, "encode_image", fake_image)

    class Pipe:
        def __init__(self, *a, **k):
            pass

        def __call__(self, **kw):
            calls["pipe"] = kw
            return types.SimpleNamespace(frames=[np.zeros((5, 8, 8, 3), np.float32)])

    monkeypatch.setattr(pipeline, "WanImageToVideoPipeline", Pipe)
    frames, png = infer.run(str(tmp_path), TRUCK, model="480p", num_frames=5, prompt="a truck", device="cpu", text_encoder="native",
                            image_encoder="native")
    assert png == "png" and frames.shape == (5, 8, 8, 3)
    assert calls["image"] == (str(mp), pil) and calls["text"] == (str(mp), "a truck")
    assert calls["pipe"]["image_embeds"].dtype == torch.bfloat16 and tuple(calls["pipe"]["image_embeds"].shape) == (1, 257, 4)
    # the default route does go to the Hugging Face classes (and therefore trips the stand-in)
    with pytest.raises(AssertionError, match="transformers.* was touched"):
        infer.run(str(tmp_path), TRUCK, model="480p", num_frames=5, prompt="a truck", device="cpu", text_encoder="native")


# ---- preprocessing ---------------------------------------------------------------------------------------------------------------------------
def test_preprocess_equals_the_recorded_clip_image_processor_output():
    from PIL import Image
    from worldforge_amd import clip
    pc, cases = cc.preprocess_fixture()
    assert pc["resample"] == 3 and pc["size"] == {"shortest_edge": 224}
    for img, want in cases:
        got = clip.preprocess(Image.fromarray(img), pc)
        assert got.dtype == F32 and tuple(got.shape) == (3, 224, 224)
        assert np.array_equal(got.numpy(), want), float(np.abs(got.numpy() - want).max())
    # a greyscale image is converted to RGB first; other settings are refused
    grey = clip.preprocess(Image.fromarray(cases[0][0][..., 0]), pc)
    assert tuple(grey.shape) == (3, 224, 224)
    back = [grey[c].double() * pc["image_std"][c] + pc["image_mean"][c] for c in range(3)]          # the same grey level in every channel
    assert float((back[0] - back[1]).abs().max()) < 1e-6 and float((back[0] - back[2]).abs().max()) < 1e-6
    for bad in ({"do_center_crop": False}, {"do_normalize": False}, {"size": {"height": 224, "width": 224}}, {"do_pad": True}, {"resample": 9},
                {"crop_size": {"height": 224, "width": 200}}, {"size": {"shortest_edge": 100}}):
        with pytest.raises(NotImplementedError):
            clip.preprocess(Image.fromarray(cases[0][0]), {**pc, **bad})


# ---- the cases can see what they are for ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,L,D", cc.ATTN_SHAPES, ids=lambda v: str(v))
def test_attention_cases_see_a_p_rounded_to_bf16(H, L, D):
    c = cc.AttnCase(H, L, D)
    if L == 1:      # one key: P = 1 exactly, there is nothing to round; the case is there for the shape
        assert torch.equal(c.ref, c.qkv.view(1, 3, H, D)[:, 2].to(F64))
        return
    bad, _ = c.reference(round_p=BF)
    r = ((bad - c.ref).abs() / c.bar).max().item()
    assert r > 1.0, r
    assert c.peak_margin() > cc.AHEAD - 1e-3
    x = c.qkv.view(L, 3, H, D)
    assert bool((x[c.flat_row, 0] == 0).all())
    assert torch.allclose(c.ref[c.flat_row], x[:, 2].to(F64).mean(0), rtol=0, atol=1e-12)     # equal scores: the mean of V


@pytest.mark.parametrize("i", range(len(cc.RANDOM_CASES)))
def test_random_gemm_cases_see_an_operand_rounded_to_bf16(i):
    c = cc.GemmCase(*cc.RANDOM_CASES[i])
    for X, W in ((c.X.to(BF).to(F32), c.W), (c.X, c.W.to(BF).to(F32))):
        bad, _ = c.reference(X, W)
        r = ((bad - c.ref).abs() / c.bar).max().item()
        assert r > 1.0, r


@pytest.mark.parametrize("kind,M,N,K", cc.exact_case_list(), ids=lambda v: str(v))
def test_exact_gemm_cases_see_a_narrowed_operand(kind, M, N, K):
    """bf16 (8 significant bits) moves the 11-bit integers: the product changes.  An fp16 three-term split represents an integer up to
    2047 in its FIRST term alone, so dropping the first term changes the product while dropping a later one cannot: these cases see
    a narrowing to fewer than 11 bits, nothing finer (the random-valued cases' bars are the finer check)."""
    X, W = cc.exact_inputs(kind, M, N, K)
    cols = cc.columns(N, K)
    big = X if kind == "a" else W
    assert float(big.abs().max()) <= 2047 and float((W if kind == "a" else X).abs().max()) == 1
    x, w = X.to(F64), W[cols].to(F64)
    ref = x @ w.T
    assert float((x.abs() @ w.abs().T).max()) < 2 ** 24
    nb = big.to(BF).to(F64)
    assert not torch.equal((nb @ w.T) if kind == "a" else (x @ nb[cols].T), ref)
    s0 = cc.split_f16x3_drop(big, 0)
    assert not torch.equal((s0 @ w.T) if kind == "a" else (x @ s0[cols].T), ref)
    assert torch.equal(cc.split_f16x3_drop(big, 2), big.to(F64))
