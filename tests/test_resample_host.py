"""The host half of the stage-1 hand-over, without a GPU: Pillow's bicubic coefficient tables and the numpy emulation of its two 8-bit
passes (worldforge_amd/resample.py) against the installed `PIL.Image.resize`, bit for bit; the two 256-entry u8 -> f32 tables against
harness.prepare_inputs' two expressions, exhaustively; and the command lines that carry the stage-1 options."""
import argparse

import numpy as np
import pytest
import torch
from PIL import Image

from worldforge_amd import resample

# (h, w) -> (H, W): down, up, each pass skipped, the product size, a square, a tiny source, a 200 -> 7 shrink (117 taps), a 1-pixel-wide input
SHAPES = [((72, 128), (48, 80)), ((37, 53), (64, 96)), ((90, 160), (90, 100)), ((45, 80), (30, 80)), ((720, 1280), (480, 832)),
          ((33, 47), (16, 16)), ((5, 7), (48, 80)), ((8, 200), (8, 7)), ((200, 8), (7, 8)), ((37, 1), (16, 5))]
KINDS = ["random", "binary", "zeros", "full", "checkerboard"]


def image_u8(kind, h, w, C, seed=0):
    rng = np.random.default_rng(seed)
    shape = (h, w, C)
    if kind == "random":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
    elif kind == "binary":
        a = (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    elif kind == "zeros":
        a = np.zeros(shape, np.uint8)
    elif kind == "full":
        a = np.full(shape, 255, np.uint8)
    else:
        yy, xx = np.mgrid[:h, :w]
        a = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], C, axis=2)
    return a


def pil_resize(a, H, W):
    """a u8 [h, w, C] (C = 1: mode L, C = 3: mode RGB) through PIL.Image.resize with its default filter."""
    if a.shape[2] == 1:
        return np.array(Image.fromarray(a[:, :, 0], "L").resize((W, H)))[:, :, None]
    return np.array(Image.fromarray(a, "RGB").resize((W, H)))


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tables_and_emulation_equal_pil_bit_for_bit(src, dst):
    (h, w), (H, W) = src, dst
    for C in (1, 3):
        for kind in KINDS:
            a = image_u8(kind, h, w, C)
            want = pil_resize(a, H, W)
            got = resample.resample_u8_numpy(a, (H, W))
            assert got.dtype == np.uint8 and got.shape == want.shape
            assert np.array_equal(got, want), (src, dst, C, kind, int(np.abs(got.astype(int) - want).max()))


def test_table_shapes_bounds_and_the_117_taps():
    bounds, coefs = resample.pil_resample_tables(200, 7)
    assert bounds.dtype == np.int32 and coefs.dtype == np.int32 and bounds.shape == (7, 2) and coefs.shape == (7, 117)
    assert bounds[:, 1].max() > 100                       # the window is really that long
    for n_in, n_out in ((200, 7), (7, 200), (1, 5), (83, 48), (1280, 832)):
        bounds, coefs = resample.pil_resample_tables(n_in, n_out)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all()
        assert (bounds[:, 1] <= coefs.shape[1]).all()
        live = np.arange(coefs.shape[1])[None, :] < bounds[:, 1:2]
        assert (coefs[~live] == 0).all()
        assert np.abs(coefs.sum(1).astype(np.int64) - (1 << 22)).max() <= coefs.shape[1]     # normalised, one rounding per tap
    assert (resample.pil_resample_tables(83, 48)[0][:, 1].min() < resample.pil_resample_tables(83, 48)[0][:, 1].max())   # clipped at the borders
    with pytest.raises(ValueError):
        resample.pil_resample_tables(8, 4, filter="lanczos")
    with pytest.raises(ValueError):
        resample.pil_resample_tables(0, 4)


def test_both_clamps_are_live_on_binary_data():
    """The negative lobes overshoot: the unclamped sums leave 0..255 on both sides, so neither clamp is dead code."""
    a = image_u8("binary", 45, 83, 1)[:, :, 0]
    bounds, coefs = resample.pil_resample_tables(83, 48)
    acc = np.full((45, 48), 1 << 21, np.int64)
    for t in range(coefs.shape[1]):
        acc += a[:, np.minimum(bounds[:, 0] + t, 82)].astype(np.int64) * coefs[:, t]
    assert (acc >> 22).min() < 0 and (acc >> 22).max() > 255


def test_the_two_u8_to_f32_tables_equal_the_host_expressions_on_all_256_values():
    frames, masks = resample.u8_to_f32_tables()
    assert frames.dtype == np.float32 and masks.dtype == np.float32 and frames.shape == masks.shape == (256,)
    u8 = np.arange(256, dtype=np.uint8)
    # harness.prepare_inputs: torch.tensor(np.array(f.resize(...))).permute(2, 0, 1).float() / 255.0
    want_frames = (torch.tensor(u8.reshape(16, 16, 1).repeat(3, 2)).permute(2, 0, 1).float() / 255.0)[0].reshape(-1).numpy()
    # harness.prepare_inputs: np.array(m.resize(...)) / 255.0 (float64), then .astype(np.float32)
    want_masks = np.stack([u8.reshape(16, 16) / 255.0]).astype(np.float32).reshape(-1)
    assert np.array_equal(frames.view(np.uint32), want_frames.view(np.uint32))
    assert np.array_equal(masks.view(np.uint32), want_masks.view(np.uint32))
    assert frames[0] == 0.0 and frames[255] == 1.0 and masks[255] == 1.0


# ---- the command lines -----------------------------------------------------------------------------------------------------------------
def _defaults(add):
    return vars(add(argparse.ArgumentParser()).parse_args([]))


def test_add_arguments_carry_the_commands_own_options():
    from worldforge_amd import run_warp, warp_depthcrafter
    a = _defaults(run_warp.add_arguments)
    full = vars(run_warp.build_parser().parse_args(["--image_path", "i", "--checkpoint", "c"]))
    assert a == {k: full[k] for k in a} and set(full) - set(a) == {"image_path", "output_path", "checkpoint", "device"}
    assert a == dict(camera=0, direction="right", degree=15.0, frame_single=24, look_at_depth=1.0, conf_single=1.0, crack_depth_threshold=0.1,
                     crack_max_size=6, crack_min_neighbors=2, depth_segments=8, outlier_min_neighbors=10, outlier_neighbor_radius=3)
    b = _defaults(warp_depthcrafter.add_arguments)
    full = vars(warp_depthcrafter.build_parser().parse_args(["--video_path", "v"]))
    assert b == {k: full[k] for k in b}
    assert b == dict(direction="left", degree=15, look_at_depth=1.0, zoom="none", rate=0.8, stable=False, stable_frame=17,
                     enable_edge_filter=False, edge_threshold=0.1, edge_dilation=3, depth_jump_threshold=0.3, neighbor_check_radius=2,
                     no_antialias=False)


def test_the_stage1_option_table_is_the_commands_own_parsers():
    """stage1.OPTIONS repeats names, types and choices: every command option is in it, under the command's type, and a value outside the
    command's choices is refused by the command's parser and by resolve() alike."""
    from worldforge_amd import run_warp, stage1, warp_depthcrafter
    for mode, module in (("vggt", run_warp), ("depthcrafter", warp_depthcrafter)):
        defaults = _defaults(module.add_arguments)
        assert [n for n, _, _ in stage1.OPTIONS[mode]] == list(defaults)
        for name, kind, choices in stage1.OPTIONS[mode]:
            parser = module.add_arguments(argparse.ArgumentParser())
            if kind is None:
                assert defaults[name] is False and getattr(parser.parse_args(["--" + name]), name) is True
                continue
            assert isinstance(defaults[name], (kind, int) if kind is float else kind), name
            for c in choices or []:
                assert getattr(parser.parse_args(["--" + name, c]), name) == c
            if choices is not None:
                with pytest.raises(SystemExit):
                    parser.parse_args(["--" + name, "no-such-choice"])
            if kind is not str:
                with pytest.raises(SystemExit):
                    parser.parse_args(["--" + name, "not-a-number"])
                assert type(getattr(parser.parse_args(["--" + name, "3"]), name)) is kind


@pytest.mark.parametrize("mode", ["vggt", "depthcrafter"])
def test_every_stage1_option_resolves_to_its_originals_default(mode):
    from worldforge_amd import run_warp, stage1, warp_depthcrafter
    own = dict(vggt=dict(vggt_checkpoint="c", image_path="i"), depthcrafter=dict(video_path="v", depth_npz="d.npz"))[mode]
    ns = vars(stage1.resolve(mode, dict(own), eff_frames=25))
    want = _defaults({"vggt": run_warp.add_arguments, "depthcrafter": warp_depthcrafter.add_arguments}[mode])
    if mode == "vggt":
        want["frame_single"] = 25           # the one stated exception: the frame count the sampler decodes
        assert ns["checkpoint"] == "c" and ns["image_path"] == "i" and ns["fill_cracks"] is True
    for k, v in want.items():
        assert ns[k] == v, (k, ns[k], v)
    assert stage1.resolve(mode, dict(own, degree=7.5, direction="up"), 25).degree == 7.5
    if mode == "vggt":
        assert stage1.resolve(mode, dict(own, frame_single=9, direction="forward", conf_single=3.0), 25).frame_single == 9
        assert stage1.resolve(mode, dict(own, conf_single=3.0), 25).conf_single == 1.0          # validate_args' clamp
        with pytest.raises(TypeError, match="zoom"):
            stage1.resolve(mode, dict(own, zoom="zoom_in"), 25)
    else:
        with pytest.raises(ValueError, match="direction"):      # run_warp's choice, not this command's
            stage1.resolve(mode, dict(own, direction="forward"), 25)
        with pytest.raises(TypeError, match="camera"):
            stage1.resolve(mode, dict(own, camera=1), 25)
    with pytest.raises(ValueError, match="needs"):
        stage1.resolve(mode, {}, 25)


def _grab_main_args(module, argv):
    got = {}
    real = argparse.ArgumentParser.parse_args

    def grab(self, args=None, namespace=None):
        ns = real(self, args, namespace)
        if args is argv:
            got.update(vars(ns))
            raise SystemExit(0)
        return ns

    argparse.ArgumentParser.parse_args = grab
    try:
        with pytest.raises(SystemExit):
            module.main(argv)
    finally:
        argparse.ArgumentParser.parse_args = real
    return got


@pytest.mark.parametrize("name", ["infer", "longcat_infer"])
def test_the_two_command_lines_carry_stage1(name, capsys):
    import importlib

    from worldforge_amd import stage1
    module = importlib.import_module(f"worldforge_amd.{name}")
    base = ["--models-dir", "/nowhere"] if name == "infer" else ["--checkpoint_dir", "/nowhere"]
    a = _grab_main_args(module, base + ["--video-ref", "/frames"])
    assert a["stage1"] == "files" and a["save_stage1"] is None and a["video_ref"] == "/frames"
    assert stage1.options_from_args(argparse.Namespace(**a)) == {}          # nothing given: every default is the chosen command's own
    with pytest.raises(SystemExit) as e:                                     # --stage1 files without --video-ref
        module.main(base)
    assert e.value.code == 2 and "--video-ref" in capsys.readouterr().err
    a = _grab_main_args(module, base + ["--stage1", "vggt", "--vggt-checkpoint", "V", "--image_path", "I", "--direction", "forward",
                                        "--degree", "20", "--crack_max_size", "4", "--save-stage1", "S"])
    assert a["video_ref"] is None and a["save_stage1"] == "S"
    assert stage1.options_from_args(argparse.Namespace(**a)) == dict(vggt_checkpoint="V", image_path="I", direction="forward", degree=20.0,
                                                                     crack_max_size=4)
    a = _grab_main_args(module, base + ["--stage1", "depthcrafter", "--video_path", "F", "--depth_npz", "D.npz", "--stable", "--zoom", "zoom_in"])
    assert stage1.options_from_args(argparse.Namespace(**a)) == dict(video_path="F", depth_npz="D.npz", stable=True, zoom="zoom_in")
    for dest in stage1.option_names():
        assert dest in a


def test_run_refuses_stage1_files_without_a_folder_and_stray_options():
    from worldforge_amd import infer, longcat_infer
    with pytest.raises(ValueError, match="video-ref"):
        infer.run(None, None, components={})
    with pytest.raises(TypeError, match="direction"):
        infer.run(None, "/frames", direction="left")
    with pytest.raises(ValueError, match="video-ref"):
        longcat_infer.run(None, None, embeds="e.npz", components=dict(vae=0, scheduler=0, dit=0))
    with pytest.raises(ValueError, match="vggt-checkpoint"):
        infer.run(None, None, stage1="vggt", image_path="I", device="cpu")
