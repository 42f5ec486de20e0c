"""GPU: the native fp32 CLIP vision encoder (worldforge_amd/clip.py) on the recorded Hugging Face fixture tests/golden/g25_clip_*.npz:
hidden 160 = 2 heads x 80, intermediate 320, 3 layers (2 run), patch 4 on 64 x 64 = 257 tokens, `gelu` and `quick_gelu` on the same
weights.  `transformers` is never imported here.

Bar: the rel-L2 of `hidden_states[-2]` against the float64 Hugging Face module must be at most C x the rel-L2 of the SAME module in
float32 (on the CPU), recorded beside it: both are fp32 evaluations that differ only in the order of their sums, so the reference
module's own error is the measure, not a number fixed here.  C = C_BAR = 2 is the smallest of 2, 4, 8 that held at the first measurement
on an MI355X; more than 8 at K <= 320 would mean that something is evaluated below fp32.
    recorded fp32 HF module: gelu 9.4544e-07, quick_gelu 9.4302e-07   (bf16 HF module: 1.07e-02, 1.03e-02)
    this encoder, MI355X:    gelu 7.2021e-07, quick_gelu 7.0187e-07 (ratios 0.76, 0.74)  -> C = 2          (profiles/clip_encode.md)

The released shape (hidden 1280 = 16 x 80, intermediate 5120, 257 tokens; one layer, seeded weights) is checked on sampled rows against
a float64 evaluation of the same layer with the same rule: 4.6472e-07 against 3.3003e-07 of fp32 torch on the CPU (ratio 1.41)."""
import pytest
import torch

from tests import clip_cases as cc
from tests._tol import within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
C_BAR = 2.0


def _model(act, sd=None):
    from worldforge_amd import clip
    fx = cc.fixture()
    return clip.CLIPVisionModel(clip.CLIPVisionConfig.from_dict({**fx["config"], "hidden_act": act}), DEV).load_state_dict(sd or fx["sd"])


@pytest.fixture(scope="module")
def outputs():
    """Both cases, computed once and left unchanged."""
    return {name: _model(act)(px) for name, (act, px, _, _, _) in cc.fixture()["cases"].items()}


@pytest.mark.parametrize("name", ["gelu", "quick"])
def test_encoder_is_as_close_to_fp64_as_the_fp32_hf_module(outputs, name):
    act, px, y64, rel_f32, rel_bf16 = cc.fixture()["cases"][name]
    got = outputs[name]
    assert got.dtype == F32 and tuple(got.shape) == (257, 160)
    y = got.cpu().to(F64)
    assert bool(torch.isfinite(y).all())
    rel = ((y - y64).norm() / y64.norm()).item()
    print(f"clip {act}: rel-L2 {rel:.4e}, fp32 HF module {rel_f32:.4e} (ratio {rel / rel_f32:.2f}), bf16 HF module {rel_bf16:.4e}")
    within("clip_rel_l2", rel, C_BAR * rel_f32)


def test_two_runs_are_bit_equal_and_other_hidden_states(outputs):
    act, px, _, _, _ = cc.fixture()["cases"]["gelu"]
    m = _model(act)
    assert torch.equal(m(px[None]), outputs["gelu"])                     # [1, 3, S, S] is taken too
    h0, h1 = m(px, hidden_state_index=0), m(px, hidden_state_index=1)
    assert not torch.equal(h0, h1) and not torch.equal(h1, outputs["gelu"]) and torch.equal(m(px, hidden_state_index=2), outputs["gelu"])


def test_the_last_layer_and_post_layernorm_do_not_matter(outputs):
    fx = cc.fixture()
    act, px, _, _, _ = fx["cases"]["gelu"]
    sd = dict(fx["sd"])
    other = cc.last_layer_fill(fx["config"], 2)
    assert set(other) == set(sd) - set(fx["stored"]) and any(not torch.equal(other[k], sd[k]) for k in other)
    sd.update(other)
    assert torch.equal(_model(act, sd)(px), outputs["gelu"])


def test_a_prefixed_file_loads_to_the_same_output_and_encode_image_is_its_bf16_cast(tmp_path, outputs):
    import json
    import os
    from PIL import Image
    from worldforge_amd import clip
    fx = cc.fixture()
    act, px, _, _, _ = fx["cases"]["gelu"]
    root = str(tmp_path / "ckpt")
    cc.write_folder(os.path.join(root, "image_encoder"), prefix="vision_model.", extra={"logit_scale": torch.zeros(())})
    with pytest.warns(UserWarning, match="ignored"):
        m = clip.CLIPVisionModel.from_pretrained(root, DEV)
    assert torch.equal(m(px), outputs["gelu"])
    # encode_image: the folder's processor settings (crop 64 here), this encoder, one cast to bf16
    pc, cases = cc.preprocess_fixture()
    pc = {**pc, "size": {"shortest_edge": 64}, "crop_size": {"height": 64, "width": 64}}
    os.makedirs(os.path.join(root, "image_processor"))
    with open(os.path.join(root, "image_processor", "preprocessor_config.json"), "w") as f:
        json.dump(pc, f)
    pil = Image.fromarray(cases[1][0])
    with pytest.warns(UserWarning, match="ignored"):
        emb = clip.encode_image(root, pil, torch.device(DEV))
    assert emb.dtype == torch.bfloat16 and tuple(emb.shape) == (1, 257, 160) and emb.device.type == "cuda"
    assert torch.equal(emb[0], m(clip.preprocess(pil, pc)).to(torch.bfloat16))


def _layer_on_the_cpu(W, px, dt):
    """hidden_states[1] of the released-shape model in plain torch on the CPU in dtype `dt`, written out from modeling_clip.py."""
    W = {k: v.cpu().to(dt) for k, v in W.items()}
    C, H, D, G, T = 1280, 16, 80, 16, 257
    ln = lambda x, n: torch.nn.functional.layer_norm(x, (C,), W[n + ".w"], W[n + ".b"], 1e-5)  # noqa: E731
    r = px.to(dt).view(3, G, 14, G, 14).permute(1, 3, 0, 2, 4).reshape(G * G, 588)
    e = W["pos"].clone()
    e[1:] += r @ W["patch"].T
    x = ln(e, "pre")
    qkv = (ln(x, "0.ln1") @ W["0.qkv.w"].T + W["0.qkv.b"]).view(T, 3, H, D)
    s = torch.einsum("ihd,jhd->hij", qkv[:, 0], qkv[:, 1]) * D ** -0.5
    a = torch.einsum("hij,jhd->ihd", torch.softmax(s, -1), qkv[:, 2]).reshape(T, C)
    x = x + (a @ W["0.o.w"].T + W["0.o.b"])
    h = torch.nn.functional.gelu(ln(x, "0.ln2") @ W["0.fc1.w"].T + W["0.fc1.b"])
    return x + (h @ W["0.fc2.w"].T + W["0.fc2.b"])


def test_one_layer_at_the_released_shape_vs_fp64_on_sampled_rows():
    """hidden 1280 = 16 heads x 80, intermediate 5120, 257 tokens, patch 14 on 224 x 224, ONE layer run (num_hidden_layers 2), seeded
    fp32 weights: hidden_states[1] on 8 sampled token rows (the class row and the last row among them) against a float64 evaluation of
    the same layer.  The bar follows the rule of the fixture cases: C_BAR x the rel-L2 of an fp32 evaluation of the same layer in plain
    torch on the CPU over the same rows, computed here -- two fp32 evaluations that differ only in the order of their sums."""
    from worldforge_amd import clip
    m = clip.CLIPVisionModel(clip.CLIPVisionConfig.from_dict({"num_hidden_layers": 2}), DEV).init_random(3)
    px = torch.randn(3, 224, 224, generator=torch.Generator().manual_seed(4))
    got = m(px, hidden_state_index=1).cpu().to(F64)
    assert tuple(got.shape) == (257, 1280) and bool(torch.isfinite(got).all())
    rows = torch.tensor([0, 1, 37, 128, 129, 200, 255, 256])
    y64 = _layer_on_the_cpu(m.W, px, F64)[rows]
    y32 = _layer_on_the_cpu(m.W, px, F32)[rows].to(F64)
    rel = ((got[rows] - y64).norm() / y64.norm()).item()
    rel32 = ((y32 - y64).norm() / y64.norm()).item()
    print(f"clip layer at the released shape: rel-L2 {rel:.4e}, fp32 torch on the CPU {rel32:.4e} (ratio {rel / rel32:.2f})")
    within("clip_layer_released", rel, C_BAR * rel32)


