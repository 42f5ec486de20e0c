"""CPU: stage 1's host side -- the restatement of tests/stage1_cases.py against the oracle and against the recorded reference
(tests/golden/g28_stage1_*: the unmodified warp_single_img with run_warp.py's shipped parameters), the parameters and the command line of
worldforge_amd.run_warp against the recorded parser, the file names, the percentile arithmetic, the refusals that need no device."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import crackfill as ocf
from oracle import warp as owarp
from tests import stage1_cases as sc
from worldforge_amd import warp

FX = sc.fixture()


def _splat_views(name="s48"):
    s = FX["scenes"][name]
    E = np.eye(4)
    E[:3] = s["E"]
    cams = warp.camera_path("left", E, 20.0, 4, 1.9)[1:]
    return owarp.splat(s["image"], s["depth"], s["K"], E, cams)


def test_restatement_at_radius_1_and_5_segments_is_the_oracle():
    wi, wm, wd = _splat_views()
    for p in (ocf.RUN_WARP_PARAMS, ocf.DEFAULT_PARAMS):
        for f in range(wi.shape[0]):
            want = ocf.warp_frame_fill(wi[f], wm[f], wd[f], p)
            got = sc.warp_frame_fill(wi[f], wm[f], wd[f], dict(p, neighbor_radius=1), 5)
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w)
    # and the window matters: the shipped parameters fill other pixels than the oracle's
    a = sc.warp_frame_fill(wi[0], wm[0], wd[0], warp.RUN_WARP_DEFAULTS, 8)[1]
    b = ocf.warp_frame_fill(wi[0], wm[0], wd[0], ocf.RUN_WARP_PARAMS)[1]
    assert (a != b).any()


@pytest.mark.parametrize("name", sorted(FX["cases"]))
def test_restated_chain_equals_the_recorded_reference(name):
    c = FX["cases"][name]
    s = FX["scenes"][c["scene"]]
    imgs, masks, thr, mean = sc.chain(s["E"], s["K"], s["image"], s["depth"], s["conf"], c["direction"], c["degree"], c["thr"],
                                      FX["meta"]["frame_num"], FX["meta"]["crack_params"], 1.0, 8)
    assert (thr is None) == (c["threshold"] is None)
    if thr is not None:
        assert np.float32(thr).view(np.uint32) == np.float32(c["threshold"]).view(np.uint32)
    assert np.float32(mean).view(np.uint32) == np.float32(c["mean_depth"]).view(np.uint32)
    np.testing.assert_array_equal(masks, c["masks"])
    np.testing.assert_array_equal(imgs, c["images"])
    assert sc.infos(c["direction"], c["degree"], FX["meta"]["frame_num"]) == c["infos"] == warp.frame_infos(c["direction"], c["degree"], 5)
    # the fp64 mean this engine uses is within one fp32 ulp of numpy's fp32 pairwise mean
    _, _, mean64, cnt = sc.conf_filter(s["depth"], s["conf"], c["thr"])
    assert cnt > 0 and abs(mean64 - float(c["mean_depth"])) <= sc.ulp32(c["mean_depth"])


def _recorded_namespace():
    ns = argparse.Namespace(**{o["dest"]: o["default"] for o in FX["meta"]["parser"]})
    for k, v in FX["meta"]["fixed"].items():
        setattr(ns, k, v)
    return ns


def test_crack_parameters_are_the_shipped_ones():
    rec = FX["meta"]["crack_params"]
    assert rec["min_neighbors"] == 10 and rec["neighbor_radius"] == 3 and rec["min_valid_neighbors"] == 2 and rec["max_crack_size"] == 6
    assert warp.RUN_WARP_DEFAULTS == rec
    assert warp.crack_params_from_args(_recorded_namespace()) == rec
    assert warp.crack_params_from_args(None) == dict(ocf.DEFAULT_PARAMS, skip_outlier_detection=False, use_fast_outlier_detection=True)
    from worldforge_amd import run_warp
    ours = run_warp.validate_args(run_warp.build_parser().parse_args(["--image_path", "x", "--checkpoint", "c"]))
    assert warp.crack_params_from_args(ours) == rec and ours.depth_segments == 8 and ours.look_at_depth == 1.0


def test_parser_is_the_recorded_one_plus_checkpoint_and_device():
    from worldforge_amd import run_warp
    acts = [a for a in run_warp.build_parser()._actions if a.option_strings and a.dest != "help"]
    table = [dict(name=a.option_strings[0], dest=a.dest, default=a.default, choices=list(a.choices) if a.choices else None,
                  type=a.type.__name__ if a.type else None, required=bool(a.required)) for a in acts]
    added = [t for t in table if t["name"] in ("--checkpoint", "--device")]
    assert [t for t in table if t not in added] == FX["meta"]["parser"]
    assert [t["name"] for t in added] == ["--checkpoint", "--device"] and added[0]["required"]
    a = run_warp.validate_args(run_warp.build_parser().parse_args(["--image_path", "x", "--checkpoint", "c", "--conf_single", "1.7"]))
    assert a.conf_single == 1.0 and a.fill_cracks and not a.disable_depth_aware_fill
    a = run_warp.validate_args(run_warp.build_parser().parse_args(["--image_path", "x", "--checkpoint", "c", "--conf_single", "-3"]))
    assert a.conf_single == 0.0
    with pytest.raises(SystemExit):
        run_warp.build_parser().parse_args(["--image_path", "x", "--checkpoint", "c", "--direction", "left_pan"])


def test_file_names_and_camera_info_are_the_recorded_ones(tmp_path):
    from worldforge_amd import harness, run_warp
    rec = FX["meta"]["save"]
    c = FX["cases"][rec["case"]]
    ns = _recorded_namespace()
    ns.direction, ns.degree, ns.frame_single, ns.conf_single = c["direction"], c["degree"], FX["meta"]["frame_num"], c["thr"]
    infos = warp.frame_infos(c["direction"], c["degree"], ns.frame_single)
    names = run_warp.frame_file_names(rec["camera_idx"], infos)
    assert [n for pair in names for n in pair] == [f[0] for f in rec["files"]]
    assert names[0][0].endswith("_00.00_deg.png")
    assert run_warp.camera_info_text(rec["camera_idx"], infos, ns) == rec["camera_info"]
    folder = run_warp.save_warped_results(c["images"], c["masks"], infos, str(tmp_path), rec["camera_idx"], ns)
    with open(tmp_path / "camera_info.txt", encoding="utf-8") as f:
        assert f.read() == rec["camera_info"]
    assert sorted(os.listdir(folder)) == sorted(f[0] for f in rec["files"])
    assert all(f[3] in (0, 255) or f[0].startswith("warp_") for f in rec["files"])
    frames, masks, first = harness.read_frames_from_directory(folder)   # the hand-over: infer --video-ref reads this folder
    assert len(frames) == len(masks) == ns.frame_single
    for i in range(ns.frame_single):    # (sorted by name = by angle label)
        np.testing.assert_array_equal(np.asarray(frames[i]), c["images"][i])
        np.testing.assert_array_equal(np.asarray(masks[i]), c["masks"][i] * 255)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000, 48 * 64])
def test_percentile_plan_and_lerp_equal_numpy(n):
    rng = np.random.default_rng(n)
    x = (1 + np.exp(rng.standard_normal(n))).astype(np.float32)
    x[rng.random(n) < 0.3] = 1.0
    s = np.sort(x)
    qs = [0.0, 100.0, 50.0, 20.0, (1 - 0.8) * 100, (1 - 0.999) * 100, (1 - 0.01) * 100, 37.3] + [100.0 * k / (n - 1) for k in range(min(n - 1, 4))]
    for q in qs:
        k, g = warp.percentile_plan(n, q)
        got = warp.lerp_f32(s[k], s[min(k + 1, n - 1)], g)
        want = np.percentile(x, q)
        assert want.dtype == np.float32
        assert got.view(np.uint32) == want.view(np.uint32), (n, q, k, g, got, want)
        assert sc.percentile_restated(x, q).view(np.uint32) == want.view(np.uint32)
    with pytest.raises(ValueError):
        warp.percentile_plan(n, 101.0)


def test_refusals_that_need_no_device():
    s = FX["scenes"]["s48"]
    kw = dict(extrinsic=s["E"], intrinsic=s["K"], image=s["image"], depth_map=s["depth"], depth_conf=s["conf"])
    for bad in (dict(use_backward=True), dict(disable_depth_aware_fill=True), dict(crack_params=dict(skip_outlier_detection=True)),
                dict(crack_params=dict(use_fast_outlier_detection=False)), dict(crack_params=dict(neighbor_radius=5)),
                dict(depth_segments=17), dict(depth_segments=0)):
        with pytest.raises(ValueError):
            warp.warp_single_img(**kw, **bad)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        warp.warp_single_img(**dict(kw, image=s["image"] * 255.0))
    with pytest.raises(ValueError, match="3 channels|must be"):
        warp.warp_single_img(**dict(kw, image=s["image"][..., :2]))


def test_new_prototypes_are_declared_and_exported():
    from worldforge_amd import _ffi, build
    dll = ctypes.CDLL(build.build(verbose=False))
    protos = _ffi.parse_header()
    for name, nargs in (("wf_crack_fill_ex", 15), ("wf_crack_fill_ex_workspace_bytes", 3), ("wf_select_pair_f32", 6),
                        ("wf_select_pair_f32_workspace_bytes", 0), ("wf_depth_conf_filter", 9), ("wf_depth_conf_filter_workspace_bytes", 0)):
        assert name in protos and len(protos[name][1]) == nargs and hasattr(dll, name), name
    assert protos["wf_crack_fill"][1] == protos["wf_crack_fill_ex"][1][:12] + protos["wf_crack_fill_ex"][1][13:]
    lib = _ffi.lib()
    assert lib.wf_crack_fill_ex_workspace_bytes(3, 37, 53) >= 4 * 3 * 37 * 53 and lib.wf_crack_fill_ex_workspace_bytes(0, 4, 4) == 0
    assert lib.wf_select_pair_f32_workspace_bytes() >= 4 * 2 * 256 * 4 and lib.wf_depth_conf_filter_workspace_bytes() > 0
    # argument checks come before any device work
    one = ctypes.c_void_p(16)
    args = lambda H, W, seg, r: (one, one, one, one, one, one, 1, H, W, 10, 2, seg, r, one, None)  # noqa: E731
    for H, W, seg, r, word in ((8, 8, 17, 1, "num_segments"), (8, 8, 0, 1, "num_segments"), (8, 8, 8, 5, "neighbor_radius"),
                               (8, 8, 8, 0, "neighbor_radius"), (4, 70, 8, 4, "exceed"), (70, 3, 8, 3, "exceed")):
        assert lib.wf_crack_fill_ex(*args(H, W, seg, r)) != 0 and word.encode() in lib.wf_last_error()
    assert lib.wf_select_pair_f32(one, 4, 4, one, one, None) != 0 and lib.wf_select_pair_f32(one, 0, 0, one, one, None) != 0
    assert lib.wf_depth_conf_filter(one, None, 0.5, 0, one, one, 4, one, None) != 0 and b"confidence" in lib.wf_last_error()
    assert lib.wf_depth_conf_filter(one, one, 0.5, 3, one, one, 4, one, None) != 0


def test_audit_vggt_reads_headers_only(tmp_path, capsys):
    import torch
    from tests import vggt_cases as vc, vggt_depth_cases as dc
    from worldforge_amd import checkpoint
    fx = dc.fixture()
    ok = vc.write_folder(str(tmp_path / "ok"), sd=fx["sd"], config=fx["chain_config"], extra={"point_head.x": torch.zeros(4, dtype=torch.bfloat16)})
    rep = checkpoint.audit_vggt(ok, depth=True)
    c = rep["components"]["vggt"]
    assert rep["ok"] and not c["missing"] and not c["unexpected"] and c["bytes"] > 0 and any("ignored" in n for n in c["notes"])
    bad = vc.write_folder(str(tmp_path / "bad"), sd=fx["sd"], config=fx["chain_config"], drop=("depth_head.norm.bias",),
                          reshape={"depth_head.projects.0.weight": (32, 256)})
    rep = checkpoint.audit_vggt(bad, depth=True)
    c = rep["components"]["vggt"]
    assert not rep["ok"] and c["missing"] == ["depth_head.norm.bias"] and c["wrong_shape"][0]["key"] == "depth_head.projects.0.weight"
    assert checkpoint.main([ok, "--vggt"]) == 0 and "vggt (VGGT)" in capsys.readouterr().out
    assert checkpoint.main([bad, "--vggt", "--json"]) == 1 and json.loads(capsys.readouterr().out)["ok"] is False
    assert checkpoint.main([ok]) == 1     # without the flag the folder holds no component of the video pipelines, as before
    with pytest.raises(FileNotFoundError):
        checkpoint.audit_vggt(str(tmp_path / "nope"))
