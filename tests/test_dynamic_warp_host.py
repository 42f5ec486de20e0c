"""CPU: the host side of the dynamic-scene stage 1 (DepthCrafter/warp_depthcrafter.py on this engine) -- camera sequences against the
reference's own (G29, tools/make_dynamic_warp_golden.py), the median rule, the command line's option table and its refusals."""
import json
import os

import numpy as np
import pytest

from worldforge_amd import warp, warp_depthcrafter as wd

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _meta():
    with open(os.path.join(GOLD, "g29_dynwarp_meta.json"), encoding="utf-8") as f:
        return json.load(f)


def test_camera_sequences_equal_the_recorded_ones():
    """Same float64 operation sequence as DepthCrafter/utils.py:240-492: equal to round-off (rtol 1e-12).  Every direction, both stable
    settings (stable_frame 1, below, equal to and above frame_num), each zoom, frame_num 1."""
    meta, rec = _meta(), np.load(os.path.join(GOLD, "g29_dynwarp_cameras.npz"))
    seen = set()
    for c in meta["cameras"]:
        got = np.stack(warp.depthcrafter_cameras(c["direction"], c["degree"], c["frame_num"], np.float32(c["look_at_depth_value"]), c["zoom"],
                                                 c["rate"], c["stable"], c["stable_frame"]))
        want = rec[c["key"]]
        assert got.shape == want.shape == (c["frame_num"], 4, 4) and got.dtype == np.float64
        assert np.allclose(got, want, rtol=1e-12, atol=0.0), (c, np.abs(got - want).max())
        seen.add((c["direction"], c["stable"], c["zoom"], c["frame_num"], c["stable_frame"]))
    assert {s[0] for s in seen} == {"up", "down", "left", "right"} and {s[2] for s in seen} == {"none", "zoom_in", "zoom_out"}
    assert {s[4] for s in seen if s[1] and s[3] == 5} == {1, 3, 5, 8} and any(s[3] == 1 for s in seen)


def test_camera_dispatch_refuses_what_the_reference_refuses():
    with pytest.raises(ValueError):
        warp.depthcrafter_cameras("left", 10.0, 4, 1.0, zoom="zoom_in", rate=0.0)
    with pytest.raises(ValueError):
        warp.depthcrafter_cameras("left", 10.0, 4, 1.0, zoom="zoom_out", rate=1.5)
    with pytest.raises(ValueError):
        warp.depthcrafter_cameras("forward", 10.0, 4, 1.0)
    assert len(warp.depthcrafter_cameras("left", 10.0, 4, 1.0, zoom="none", rate=7.0)) == 4  # the rate is read only with a zoom


def test_the_target_is_taken_before_the_position_moves():
    """utils.py:260-269: look_at_point comes from the unmoved t.  From a non-identity extrinsic the two orders differ."""
    E = np.eye(4)
    E[:3, 3] = [0.3, -0.2, 0.5]
    cam = warp.dc_look_up_camera_seq(E, 20.0, 2, 2.0)[1]
    target = E[:3, 3] + np.array([0, 0, 2.0])
    fwd = target - cam[:3, 3]
    assert np.allclose(cam[:3, 2], fwd / np.linalg.norm(fwd), rtol=1e-12)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 9, 10, 3840, 3841])
def test_median_rule_matches_numpy(n):
    rng = np.random.default_rng(n)
    for ties in (False, True):
        a = rng.random(n).astype(np.float32) + np.float32(0.3)
        if ties:
            a = np.round(a * 4) / np.float32(4)  # a handful of distinct values: the middle pair is usually a tie
        s = np.sort(a)
        k = warp.median_index(n)
        got = warp.median_from_pair(s[k], s[min(k + 1, n - 1)], n)
        want = np.median(a)
        assert got.dtype == want.dtype == np.float32 and got.view(np.uint32) == want.view(np.uint32), (n, ties, got, want)


def test_parser_takes_every_option_of_the_reference():
    table = {a.option_strings[0]: a for a in wd.build_parser()._actions if a.option_strings and a.dest != "help"}
    rec = _meta()["parser"]
    assert len(rec) == 25
    for o in rec:
        a = table[o["name"]]
        assert a.dest == o["dest"] and a.default == o["default"] and (list(a.choices) if a.choices else None) == o["choices"], o
        assert (a.type.__name__ if a.type else None) == o["type"] and bool(a.required) == o["required"] and (a.nargs == 0) == o["flag"], o
    assert set(table) - {o["name"] for o in rec} == {"--device", "--depth_npz", "--no_antialias"}


def _frames_folder(tmp_path, n=3):
    from PIL import Image
    d = tmp_path / "seq"
    d.mkdir()
    for i in range(n):
        Image.fromarray(np.full((6, 8, 3), 40 * i, dtype=np.uint8), "RGB").save(d / f"f_{i:02d}.png")
    return str(d)


def test_refuses_a_run_without_a_depth_file(tmp_path):
    with pytest.raises(SystemExit) as e:
        wd.main(["--video_path", _frames_folder(tmp_path), "--output_path", str(tmp_path / "out")])
    msg = str(e.value)
    assert "DepthCrafter depth network is not built" in msg and "compatibility only" in msg and "--depth_npz" in msg


def test_refuses_a_video_file(tmp_path):
    v = tmp_path / "clip.mp4"
    v.write_bytes(b"\x00" * 16)
    with pytest.raises(SystemExit) as e:
        wd.main(["--video_path", str(v), "--output_path", str(tmp_path / "out")])
    assert "no decoder" in str(e.value)


def test_refuses_a_frame_count_that_differs_from_the_depth(tmp_path):
    npz = tmp_path / "depth.npz"
    np.savez_compressed(npz, depth=np.full((4, 6, 8), 0.5, dtype=np.float32))
    with pytest.raises(ValueError, match="3 images .* 4 depth maps"):
        wd.main(["--video_path", _frames_folder(tmp_path, 3), "--depth_npz", str(npz), "--output_path", str(tmp_path / "out")])
    with pytest.raises(ValueError, match="3 frames but 4 depth maps"):
        warp.warp_depthcrafter_frames(np.zeros((3, 6, 8, 3), np.uint8), np.zeros((4, 6, 8), np.float32), device="cpu")
    with pytest.raises(ValueError, match=r"\[T, h, w, 3\]"):
        warp.warp_depthcrafter_frames(np.zeros((3, 6, 8), np.uint8), np.zeros((3, 6, 8), np.float32), device="cpu")
    with pytest.raises(ValueError, match=r"\[T, H, W\]"):
        warp.warp_depthcrafter_frames(np.zeros((3, 6, 8, 3), np.uint8), np.zeros((6, 8), np.float32), device="cpu")


def test_depth_lookup_order_and_frame_listing(tmp_path):
    frames = _frames_folder(tmp_path)
    out = tmp_path / "out"
    folder = out / "depth_estimation" / "seq"
    folder.mkdir(parents=True)
    np.savez_compressed(folder / "depth.npz", depth=np.zeros((3, 6, 8), np.float32))
    other = tmp_path / "other.npz"
    np.savez_compressed(other, depth=np.zeros((3, 6, 8), np.float32))
    args = wd.build_parser().parse_args(["--video_path", frames + "/", "--output_path", str(out)])
    assert wd.find_depth(args) == str(folder / "depth.npz")
    args = wd.build_parser().parse_args(["--video_path", frames, "--output_path", str(out), "--depth_npz", str(other)])
    assert wd.find_depth(args) == str(other)
    names = wd.list_frames(frames)
    assert [os.path.basename(n) for n in names] == ["f_00.png", "f_01.png", "f_02.png"] and wd.read_frames(names).shape == (3, 6, 8, 3)
