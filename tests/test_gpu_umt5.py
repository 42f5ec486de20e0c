"""GPU: the native UMT5 encoder (worldforge_amd/umt5.py) on the recorded Hugging Face fixture tests/golden/g24_umt5.npz (+ _y64):
2 layers, d_model 128, 2 heads x 64, d_ff 192, vocab 97; three (L, kv_len) cases (70, 45), (200, 173), (512, 512).  `transformers` is
never imported here.

Bar: the rel-L2 of every case over ALL L rows against `UMT5EncoderModel(...).double()` must be at most the rel-L2 of the same Hugging
Face module in bfloat16 stored beside it, margin x 1.0: every intermediate of this encoder is at least as wide as the bf16 module's
(fp32 residual stream, fp32 scores and softmax, one rounding per bf16 tensor).  Measured on an MI355X: see DESIGN.md section 4j."""
import os

import numpy as np
import pytest
import torch

from tests import umt5_cases as uc
from tests._tol import within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


@pytest.fixture(scope="module")
def model():
    from worldforge_amd import umt5
    fx = uc.fixture()
    return umt5.UMT5EncoderModel(umt5.UMT5Config.from_dict(fx["config"]), DEV).load_state_dict(fx["sd"])


@pytest.fixture(scope="module")
def outputs(model):
    """The three cases, computed once and left unchanged."""
    return [model(ids[None], mask[None]) for ids, mask, _, _ in uc.fixture()["cases"]]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_encoder_is_at_least_as_close_to_fp64_as_the_bf16_hf_module(outputs, i):
    ids, mask, y64, ybf = uc.fixture()["cases"][i]
    got = outputs[i]
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (1, ids.numel(), 128)
    y = got[0].cpu().to(F64)
    assert bool(torch.isfinite(y).all())
    rel = ((y - y64).norm() / y64.norm()).item()
    rel_hf = ((ybf.to(F64) - y64).norm() / y64.norm()).item()
    print(f"umt5 case {i} (L {ids.numel()}, kv_len {int(mask.sum())}): rel-L2 {rel:.4e}, bf16 HF module {rel_hf:.4e}")
    within("umt5_rel_l2", rel, rel_hf)


def test_two_runs_are_bit_equal(model, outputs):
    ids, mask, _, _ = uc.fixture()["cases"][1]
    assert torch.equal(model(ids[None], mask[None]), outputs[1])


def test_a_batch_of_two_equals_two_single_calls(model):
    ids, mask, _, _ = uc.fixture()["cases"][0]
    ids2 = torch.stack([ids, ids.flip(0).clamp(min=1)])
    mask2 = torch.stack([mask, torch.cat([torch.ones(70 - 9, dtype=mask.dtype), torch.zeros(9, dtype=mask.dtype)])])
    both = model(ids2, mask2)
    assert tuple(both.shape) == (2, 70, 128)
    for b in range(2):
        assert torch.equal(both[b], model(ids2[b:b + 1], mask2[b:b + 1])[0])
    assert not torch.equal(both[0], both[1])


def test_layout_helpers(outputs):
    from worldforge_amd import umt5
    ids, mask, _, _ = uc.fixture()["cases"][0]
    h = outputs[0]
    e, m = umt5.to_longcat(h, mask[None])
    assert tuple(e.shape) == (1, 1, 70, 128) and e.dtype == torch.bfloat16 and torch.equal(e[0, 0], h[0])
    assert tuple(m.shape) == (1, 70) and m.dtype == torch.int64 and int(m.sum()) == 45
    w = umt5.to_wan(h, mask[None])
    assert tuple(w.shape) == (1, 512, 128) and w.dtype == torch.bfloat16
    assert torch.equal(w[0, :45], h[0, :45])
    assert bool((w[0, 45:].view(torch.int16) == 0).all()), "pad rows must be exact zeros"


class _Tok:
    """A stand-in with the Hugging Face tokenizer's call signature: bytes mod 96 + 1, right-padded with the pad id 0."""

    def __call__(self, texts, padding, max_length, truncation, add_special_tokens, return_attention_mask, return_tensors):
        assert padding == "max_length" and return_tensors == "pt" and len(texts) == 1
        ids = [b % 96 + 1 for b in texts[0].encode()][:max_length - 1] + [1]
        out = type("Enc", (), {})()
        out.input_ids = torch.tensor([ids + [0] * (max_length - len(ids))])
        out.attention_mask = torch.tensor([[1] * len(ids) + [0] * (max_length - len(ids))])
        return out


def test_cli_helpers_return_what_load_embeds_returns(tmp_path):
    """encode_native / encode_text_native on a synthetic checkpoint folder: the keys, shapes and dtypes of the --embeds route, from a
    folder loaded through from_pretrained (header check, memory map) -- and the same values as the model built from the state dict."""
    from worldforge_amd import infer, longcat_infer, umt5
    folder = str(tmp_path / "ckpt")
    uc.write_folder(os.path.join(folder, "text_encoder"))
    emb = longcat_infer.encode_native(folder, "a  red &amp; blue kite", "blurry", torch.device(DEV), tokenizer=_Tok())
    np.savez(str(tmp_path / "e.npz"), **{k: (v.float() if v.dtype == torch.bfloat16 else v).cpu().numpy() for k, v in emb.items()})
    ref = longcat_infer.load_embeds(str(tmp_path / "e.npz"), torch.device(DEV), negative=True)
    assert sorted(emb) == sorted(ref)
    for k in ref:
        assert emb[k].dtype == ref[k].dtype and emb[k].shape == ref[k].shape and emb[k].device == ref[k].device, k
        assert torch.equal(emb[k], ref[k]), k
    assert tuple(emb["prompt_embeds"].shape) == (1, 1, 512, 128) and tuple(emb["prompt_attention_mask"].shape) == (1, 512)
    n = int(emb["prompt_attention_mask"].sum())
    assert n == len("a red & blue kite") + 1                                   # prompt_clean ran
    wan = infer.encode_text_native(folder, "a red & blue kite", "blurry", torch.device(DEV), tokenizer=_Tok())
    assert tuple(wan["prompt_embeds"].shape) == (1, 512, 128) and wan["prompt_embeds"].dtype == torch.bfloat16
    assert torch.equal(wan["prompt_embeds"][0, :n], emb["prompt_embeds"][0, 0, :n])
    assert bool((wan["prompt_embeds"][0, n:].view(torch.int16) == 0).all())
    assert tuple(wan["negative_prompt_embeds"].shape) == (1, 512, 128)
    # refusals of from_pretrained: a missing key, an unexpected key
    ln = "encoder.final_layer_norm.weight"
    uc.write_folder(os.path.join(str(tmp_path / "m"), "text_encoder"), rename={ln: "encoder.final_norm.weight"})
    with pytest.raises(KeyError):
        umt5.UMT5EncoderModel.from_pretrained(str(tmp_path / "m"), DEV)
    uc.write_folder(os.path.join(str(tmp_path / "x"), "text_encoder"), extra={"encoder.stray": torch.zeros(2)})
    with pytest.raises(ValueError):
        umt5.UMT5EncoderModel.from_pretrained(str(tmp_path / "x"), DEV)
