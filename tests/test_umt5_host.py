"""CPU: the host side of the native UMT5 encoder (worldforge_amd/umt5.py) -- the bucket rule against the recorded Hugging Face values and
the threshold table, the key table, every refusal that needs no device, the tied-embedding alias, the audit of a `text_encoder/` folder,
and the sharpness of the attention cases of tests/test_gpu_umt5_kernels_fp64.py (a bucket boundary moved by one must show)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests import umt5_cases as uc
from worldforge_amd import checkpoint, umt5

# |rel| -> bucket (plus 16 when rel > 0) of the released settings (32 buckets, max distance 128)
TABLE = [(0, 7, None), (8, 11, 8), (12, 15, 9), (16, 22, 10), (23, 31, 11), (32, 45, 12), (46, 63, 13), (64, 90, 14), (91, 600, 15)]


def test_bucket_rule_matches_the_recorded_hf_values():
    fx = uc.fixture()
    got = [umt5.relative_position_bucket(int(r)) for r in fx["bucket_rel"]]
    assert got == [int(b) for b in fx["bucket"]]
    assert int(fx["bucket_rel"][0]) == -600 and int(fx["bucket_rel"][-1]) == 600


def test_bucket_rule_matches_the_threshold_table():
    for lo, hi, b in TABLE:
        for a in range(lo, hi + 1):
            want = a if b is None else b
            assert umt5.relative_position_bucket(-a) == want, a
            assert umt5.relative_position_bucket(a) == want + (16 if a > 0 else 0), a
    lut = umt5.bucket_lut()
    assert lut.dtype == np.uint8 and lut.shape == (1023,)
    assert [int(lut[r + 511]) for r in (-511, -8, -7, 0, 7, 8, 511)] == [15, 8, 7, 0, 23, 24, 31]
    # every boundary the GPU cases plant keys at is a boundary of the rule
    for d in uc.BOUNDARIES:
        assert umt5.relative_position_bucket(d) + 1 == umt5.relative_position_bucket(d + 1)


def test_expected_state_dict_is_the_hf_key_list():
    fx = uc.fixture()
    cfg = umt5.UMT5Config.from_dict(fx["config"])
    exp = umt5.expected_state_dict(cfg)
    assert sorted(exp) == fx["keys"]
    for k in fx["keys"]:
        assert tuple(fx["sd"][k].shape) == tuple(exp[k]), k
    full = umt5.expected_state_dict(umt5.UMT5Config())
    assert len(full) == 2 + 24 * 10 and full["shared.weight"] == (256384, 4096)
    assert full["encoder.block.23.layer.1.DenseReluDense.wi_1.weight"] == (10240, 4096)


def test_config_refusals(tmp_path):
    base = uc.fixture()["config"]
    for bad in ({"feed_forward_proj": "relu"}, {"feed_forward_proj": "gated-silu"}, {"is_decoder": True}, {"d_kv": 128}):
        with pytest.raises(NotImplementedError):
            umt5.UMT5Config.from_dict({**base, **bad})
    p = tmp_path / "config.json"
    p.write_text(json.dumps({**base, "feed_forward_proj": "relu"}))
    with pytest.raises(NotImplementedError):
        umt5.UMT5Config.from_json(str(p))
    p.write_text(json.dumps(base))
    cfg = umt5.UMT5Config.from_json(str(p))
    assert (cfg.vocab_size, cfg.d_model, cfg.num_heads, cfg.d_ff, cfg.num_layers) == (97, 128, 2, 192, 2)


def _model_without_device():
    m = umt5.UMT5EncoderModel.__new__(umt5.UMT5EncoderModel)
    m.cfg, m.device, m.W = umt5.UMT5Config.from_dict(uc.fixture()["config"]), torch.device("cpu"), {"loaded": True}
    return m


@pytest.mark.parametrize("mask", [[0, 0, 0, 0], [0, 1, 1, 1], [1, 0, 1, 0], [1, 1, 0, 1], [1, 2, 0, 0]])
def test_mask_shapes_are_refused(mask):
    with pytest.raises(ValueError, match="ones followed by zeros"):
        _model_without_device()(torch.zeros(1, 4, dtype=torch.int64), torch.tensor([mask]))
    with pytest.raises(ValueError):
        umt5.check_mask(torch.tensor(mask))


def test_mask_prefix_lengths():
    assert umt5.check_mask(torch.tensor([1, 1, 1, 0, 0])) == 3 and umt5.check_mask(torch.tensor([1])) == 1
    assert umt5.check_mask(torch.ones(512, dtype=torch.int64)) == 512


@pytest.mark.parametrize("ids", [[0, 97, 1], [0, -1, 1]])
def test_id_range_is_refused(ids):
    with pytest.raises(ValueError, match="input_ids outside"):
        _model_without_device()(torch.tensor([ids]), torch.ones(1, 3, dtype=torch.int64))


def test_more_than_512_tokens_are_refused():
    with pytest.raises(ValueError, match="512"):
        _model_without_device()(torch.zeros(1, 513, dtype=torch.int64), torch.ones(1, 513, dtype=torch.int64))
    with pytest.raises(ValueError, match="disagree"):
        _model_without_device()(torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 5, dtype=torch.int64))


def test_tied_alias_decoder_keys_and_key_errors():
    fx = uc.fixture()
    cfg = umt5.UMT5Config.from_dict(fx["config"])
    hdr = {k: {"shape": tuple(v.shape)} for k, v in fx["sd"].items()}
    # the alias beside shared.weight: accepted, folded away
    keep, dropped = umt5.consumed_header({**hdr, umt5.ALIAS: hdr["shared.weight"]})
    assert sorted(keep) == fx["keys"] and dropped == 0
    # the alias alone: it stands in for shared.weight
    only = {k: v for k, v in hdr.items() if k != "shared.weight"}
    keep, _ = umt5.consumed_header({**only, umt5.ALIAS: hdr["shared.weight"]})
    assert sorted(keep) == fx["keys"]
    # decoder.* / lm_head.*: ignored with ONE warning
    keep, dropped = umt5.consumed_header({**hdr, "decoder.block.0.layer.0.SelfAttention.q.weight": {"shape": (128, 128)},
                                          "lm_head.weight": {"shape": (97, 128)}})
    assert sorted(keep) == fx["keys"] and dropped == 2
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        umt5._raise_on(keep, cfg, "here", dropped)
    assert len(w) == 1 and "decoder" in str(w[0].message)
    with pytest.raises(KeyError, match="final_layer_norm"):
        umt5._raise_on({k: v for k, v in hdr.items() if k != "encoder.final_layer_norm.weight"}, cfg, "here", 0)
    with pytest.raises(ValueError, match="not consumed"):
        umt5._raise_on({**hdr, "encoder.extra.weight": {"shape": (1,)}}, cfg, "here", 0)
    with pytest.raises(ValueError, match="wrong shape"):
        umt5._raise_on({**hdr, "shared.weight": {"shape": (96, 128)}}, cfg, "here", 0)


def test_audit_reports_the_text_encoder_component(tmp_path):
    fx = uc.fixture()
    ln = "encoder.block.1.layer.1.layer_norm.weight"
    uc.write_folder(str(tmp_path / "good" / "text_encoder"), extra={umt5.ALIAS: fx["sd"]["shared.weight"]})
    rep = checkpoint.audit(str(tmp_path / "good"))
    c = rep["components"]["text_encoder"]
    assert rep["ok"] and c["kind"] == "UMT5EncoderModel" and not (c["missing"] or c["unexpected"] or c["wrong_shape"])
    assert c["dtypes"] == {"BF16": len(fx["keys"]) + 1}
    assert c["bytes"] == 2 * (sum(v.numel() for v in fx["sd"].values()) + fx["sd"]["shared.weight"].numel())
    uc.write_folder(str(tmp_path / "bad" / "text_encoder"), rename={ln: ln.replace("layer_norm", "norm")},
                    extra={"encoder.stray.weight": torch.zeros(3, dtype=torch.bfloat16),
                           "encoder.final_layer_norm.weight": torch.ones(64, dtype=torch.bfloat16)})
    rep = checkpoint.audit(str(tmp_path / "bad"))
    c = rep["components"]["text_encoder"]
    assert not rep["ok"]
    assert c["missing"] == [ln]
    assert c["unexpected"] == sorted(["encoder.stray.weight", ln.replace("layer_norm", "norm")])
    assert c["wrong_shape"] == [{"key": "encoder.final_layer_norm.weight", "found": [64], "expected": [128]}]
    assert "text_encoder (UMT5EncoderModel)" in checkpoint.format_report(rep)
    # a refused config is reported, not raised
    uc.write_folder(str(tmp_path / "relu" / "text_encoder"), config={**fx["config"], "feed_forward_proj": "relu"})
    c = checkpoint.audit(str(tmp_path / "relu"))["components"]["text_encoder"]
    assert c["refused"] and "gated-gelu" in c["refused"][0]


def test_cli_flag_defaults_to_transformers():
    from worldforge_amd import longcat_infer
    ap = longcat_infer.cli_parser()
    base = ["--checkpoint_dir", "c", "--video-ref", "v"]
    assert ap.parse_args(base).text_encoder == "transformers"
    assert ap.parse_args(base + ["--text-encoder", "native"]).text_encoder == "native"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--text-encoder", "other"])


# ---- sharpness of the attention cases ------------------------------------------------------------------------------------------------------
SHARP = 3.0
_BOUNDARY_CASES = [c for c in uc.case_list() if c[0] == 3 and uc.plant_plan(c[1], c[2])]


def test_the_attention_cases_cover_every_boundary_on_both_sides():
    seen = set()
    for H, L, kv in uc.case_list():
        seen.update((d, side) for d, side, *_ in uc.plant_plan(L, kv))
    assert seen == {(d, s) for d in uc.BOUNDARIES for s in (1, -1)}
    assert len(_BOUNDARY_CASES) >= 8


@pytest.mark.parametrize("L,kv", [(c[1], c[2]) for c in _BOUNDARY_CASES], ids=lambda v: str(v))
def test_a_boundary_moved_by_one_moves_the_reference_by_more_than_three_bars(L, kv):
    """Every boundary a case plants, moved up or down by one: the float64 reference of the planted row must move some output element of
    EVERY head by more than 3 bars (the same inputs serve H = 3 and the first heads' construction of H = 64)."""
    c = uc.AttnCase(3, L, kv, umt5.relative_position_bucket)
    assert c.plan
    for d, side, r, j1, j2 in c.plan:
        for up in (True, False):
            ref2, _, _ = c.reference(uc.lut_of(uc.shifted(umt5.relative_position_bucket, d, up)), rows=[r])
            ratio = ((ref2[0] - c.ref[r]).abs() / c.bar[r]).amax(-1).min().item()
            assert ratio > SHARP, f"L {L} kv {kv}: boundary {d}|{d + 1} side {side} moved {'up' if up else 'down'}: {ratio:.2f} bars"


def test_the_entry_hands_the_prompt_to_the_native_encoder_before_any_model_is_loaded(tmp_path, monkeypatch):
    """--text-encoder native: run() calls encode_native (not the Hugging Face model class) with the prompt, and does so before the
    DiT and the VAE are loaded."""
    pytest.importorskip("transformers")       # run() asks for it: the folder's tokenizer is a transformers object
    from worldforge_amd import longcat_infer
    from worldforge_amd.longcat_pipeline import LongCatVideoPipeline
    truck = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "truck")

    class Reached(Exception):
        pass

    def native(checkpoint_dir, prompt, negative_prompt, device, **kw):
        raise Reached(f"{prompt}|{negative_prompt is not None}")

    def never(*a, **k):
        raise AssertionError("must not be reached")

    monkeypatch.setattr(longcat_infer, "encode_native", native)
    monkeypatch.setattr(longcat_infer, "encode_with_transformers", never)
    monkeypatch.setattr(LongCatVideoPipeline, "from_pretrained", classmethod(never))
    for d in ("text_encoder", "tokenizer"):
        os.makedirs(tmp_path / d)
    base = ["--checkpoint_dir", str(tmp_path), "--video-ref", truck, "--num-frames", "9", "--prompt", "a kite"]
    with pytest.raises(Reached, match=r"a kite\|True"):
        longcat_infer.main(base + ["--text-encoder", "native"])
    with pytest.raises(Reached, match=r"a kite\|False"):
        longcat_infer.main(base + ["--text-encoder", "native", "--guidance-scale", "1.0"])
    with pytest.raises(AssertionError, match="must not be reached"):
        longcat_infer.main(base)              # the default is today's route
