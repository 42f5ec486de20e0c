"""CPU: the host side of the VGGT depth head (worldforge_amd/vggt.py) -- key sets, header rules, config refusals, the position tables --
and the float64 restatement of the head in tests/vggt_depth_cases.py against the recorded outputs of the reference's own units
(tests/golden/g27_vggt_depth_*).  No GPU, and the reference package is never imported."""
import warnings

import pytest
import torch

from tests import vggt_depth_cases as dc
from tests.vggt_cases import fixture as g26_fixture
from worldforge_amd import vggt

F64 = torch.float64


def test_depth_key_set_is_the_released_modules():
    released = g26_fixture()["released"]
    want = {k: tuple(v) for k, v in released.items() if k.startswith(("aggregator.", "camera_head.", "depth_head.")) and not k.endswith("mask_token")}
    got = vggt.expected_state_dict(vggt.VGGTConfig(), depth=True)
    assert set(got) == set(want)
    assert [k for k in got if tuple(got[k]) != want[k]] == []
    assert sum(k.startswith("depth_head.") for k in got) == 62


def test_without_depth_the_key_set_is_unchanged():
    cfg = vggt.VGGTConfig()
    base = vggt.expected_state_dict(cfg)
    assert base == vggt.expected_state_dict(cfg, depth=False)
    assert not any(k.startswith("depth_head.") for k in base)
    with_depth = vggt.expected_state_dict(cfg, depth=True)
    assert {k: v for k, v in with_depth.items() if not k.startswith("depth_head.")} == base
    assert "depth_head." in vggt.IGNORED


def _header(cfg, **change):
    hdr = {k: {"shape": tuple(v)} for k, v in vggt.expected_state_dict(cfg, depth=True).items()}
    hdr.update(change)
    return hdr


def test_header_rules_with_depth():
    cfg = vggt.VGGTConfig.from_dict(dc.fixture()["chain_config"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        keep = vggt.consumed_header(_header(cfg), "t", depth=True)
        vggt._raise_on(keep, cfg, "t", depth=True)                                 # complete: no warning, no error
    missing = _header(cfg)
    missing.pop("depth_head.norm.bias")
    with pytest.raises(KeyError, match="depth_head.norm.bias"):
        vggt._raise_on(vggt.consumed_header(missing, "t", depth=True), cfg, "t", depth=True)
    shaped = _header(cfg, **{"depth_head.projects.0.weight": {"shape": (32, 256)}})
    with pytest.raises(ValueError, match="shape"):
        vggt._raise_on(vggt.consumed_header(shaped, "t", depth=True), cfg, "t", depth=True)
    extra = _header(cfg, **{"depth_head.scratch.stem.weight": {"shape": (4,)}})
    with pytest.raises(ValueError, match="not consumed"):
        vggt._raise_on(vggt.consumed_header(extra, "t", depth=True), cfg, "t", depth=True)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        keep = vggt.consumed_header(_header(cfg, **{"point_head.x": {"shape": (2,)}, "track_head.y": {"shape": (2,)}}), "t", depth=True)
    assert len(rec) == 1 and "point_head." in str(rec[0].message) and "depth_head." not in str(rec[0].message)
    assert "point_head.x" not in keep and "depth_head.norm.bias" in keep
    vggt._raise_on(keep, cfg, "t", depth=True)


def test_header_rules_without_depth_still_ignore_the_depth_head():
    cfg = vggt.VGGTConfig.from_dict(dc.fixture()["config"])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        keep = vggt.consumed_header(_header(cfg), "t")
    assert len(rec) == 1 and "depth_head." in str(rec[0].message)
    assert not any(k.startswith("depth_head.") for k in keep)
    vggt._raise_on(keep, cfg, "t")


def test_config_refusals():
    base = dc.fixture()["config"]
    cfg = vggt.VGGTConfig.from_dict(base)
    assert cfg.depth_features == 64 and cfg.depth_out_channels == (32, 64, 128, 128) and cfg.depth_layers == (4, 11, 17, 23)
    rel = vggt.VGGTConfig()
    assert rel.depth_features == 256 and rel.depth_out_channels == (256, 512, 1024, 1024) and rel.depth_layers == (4, 11, 17, 23)
    assert vggt.VGGTConfig.from_dict(dc.fixture()["chain_config"]).depth_layers == (0, 1, 1, 0)
    with pytest.raises(NotImplementedError):
        vggt.VGGTConfig.from_dict(dict(base, depth_layers=[0, 1, 1]))
    with pytest.raises(NotImplementedError):
        vggt.VGGTConfig.from_dict(dict(base, depth_out_channels=[32, 64, 128]))
    with pytest.raises(NotImplementedError):
        vggt.VGGTConfig.from_dict(dict(base, depth_out_channels=[32, 64, 126, 128]))
    with pytest.raises(NotImplementedError):
        vggt.VGGTConfig.from_dict(dict(base, depth_features=12))                   # features / 2 must be a multiple of 4
    with pytest.raises(ValueError):
        vggt.VGGTConfig.from_dict(dict(base, depth_layers=[0, 1, 2, 1]))           # the fixture's aggregator has layers 0 and 1
    with pytest.raises(ValueError):
        vggt.VGGTConfig.from_dict(dict(base, depth_layers=[-1, 0, 1, 1]))
    # a config that does not name depth_layers (no depth head in its folder) loads as before; the layers are checked when the head is asked for
    with pytest.raises(ValueError, match="depth_layers"):
        vggt._raise_on({}, cfg, "t", depth=True)


def test_position_tables_equal_the_recorded_embedding_bit_for_bit():
    for C, h, w, W, H, want in dc.fixture()["pos"]:
        col, row = vggt.dpt_pos_tables(C, h, w, (H, W))
        assert col.dtype == torch.float32 and tuple(col.shape) == (w, C // 2) and tuple(row.shape) == (h, C // 2)
        got = vggt.dpt_pos_embed(C, h, w, (H, W))
        assert tuple(got.shape) == (C, h, w) and torch.equal(got, want), (C, h, w)
        assert torch.equal(dc.pos_embed(C, h, w, (H, W), torch.float32), want)     # the test module's own statement of it
        assert torch.equal(got[:C // 2, 0], got[:C // 2, h - 1]) and torch.equal(got[C // 2:, :, 0], got[C // 2:, :, w - 1])   # separable
    with pytest.raises(ValueError):
        vggt.dpt_pos_tables(6, 2, 2, (28, 28))


def test_restated_units_reproduce_the_recorded_ones_and_see_the_in_place_relu():
    u = dc.fixture()["units"]
    got = dc.rcu(u["rcu_in"], u, "rcu.")
    assert float((got - u["rcu_out"]).abs().max()) <= 1e-12
    wrong = dc.rcu(u["rcu_in"], u, "rcu.", skip_is_input=True)
    assert float((wrong - u["rcu_out"]).abs().max()) > 0.1                         # the residual taken as x: the fault is seen
    size = tuple(int(v) for v in u["ffb_size"])
    got = dc.fusion(u["ffb_in0"], u["ffb_in1"], u, "ffb.", size)
    assert tuple(got.shape) == (1, 8) + size and float((got - u["ffb_out"]).abs().max()) <= 1e-12
    wrong = dc.fusion(u["ffb_in0"], u["ffb_in1"], u, "ffb.", size, skip_is_input=True)
    assert float((wrong - u["ffb_out"]).abs().max()) > 0.1


def test_restated_resize_is_the_recorded_interpolation():
    for (x, want), ((hi, wi), (ho, wo)) in zip(dc.fixture()["resize"], dc.RESIZE_CASES):
        assert tuple(x.shape) == (2, hi, wi) and tuple(want.shape) == (2, ho, wo)
        assert float((dc.resize_ac(x.to(F64)[None], (ho, wo))[0] - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_restated_head_reproduces_the_recorded_float64_module(ci):
    fx = dc.fixture()
    c = fx["head_cases"][ci]
    # the recorded module is the float64 copy, whose position coordinates are a float64 linspace
    depth, conf = dc.head64(fx["sd"], [t[0] for t in c["tokens"]], (c["H"], c["W"]), coord_dtype=F64)
    assert tuple(depth.shape) == (c["S"], c["H"], c["W"])
    assert float((depth - c["depth"][0, ..., 0]).abs().max()) <= 1e-11 and float((conf - c["conf"][0]).abs().max()) <= 1e-11
    # with the released module's fp32 coordinates (the kernel tests' reference) the head moves by far less than the fp32 module's own error
    d32, _ = dc.head64(fx["sd"], [t[0] for t in c["tokens"]], (c["H"], c["W"]))
    assert float((d32 - depth).norm() / depth.norm()) <= 0.5 * c["rel_f32_depth"]
    swapped, _ = dc.head64(fx["sd"], [c["tokens"][i][0] for i in (0, 2, 1, 3)], (c["H"], c["W"]))
    assert float((swapped - c["depth"][0, ..., 0]).norm() / c["depth"].norm()) > 0.05     # the layer order is visible


def test_depth_methods_without_the_head_say_how_to_load_it():
    m = vggt.VGGT(vggt.VGGTConfig.from_dict(dc.fixture()["config"]), "cpu")
    m.W, m.has_depth = {"placeholder": torch.zeros(1)}, False
    for call in (lambda: m.depth(torch.zeros(1, 3, 14, 14)), lambda: m.predict(torch.zeros(1, 3, 14, 14)),
                 lambda: m.depth_from_tokens({}, (14, 14))):
        with pytest.raises(RuntimeError, match="depth=True"):
            call()


def test_to_image_size_refuses_mismatched_shapes():
    with pytest.raises(ValueError):
        vggt.to_image_size(torch.zeros(1, 1, 14, 14), torch.zeros(1, 1, 14, 14), torch.zeros(1, 1, 3, 3), (14, 14), (28, 28))
