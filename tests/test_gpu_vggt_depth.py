"""GPU: the native VGGT depth head (worldforge_amd/vggt.py, csrc/dpt.hip) on the recorded fixtures tests/golden/g27_vggt_depth_*: the
reference's own DPTHead(dim_in 256, features 64, out_channels 32 / 64 / 128 / 128) at test width.  The reference package is never imported.

Head alone, cases (S, H, W) = (1, 14, 14), (1, 14, 28), (2, 42, 70), (2, 154, 210), four distinct recorded token tensors: rel-L2 of depth
and of depth_conf against the float64 module <= C_DEPTH x the recorded rel-L2 of the float32 module on the same tokens.  Both are fp32
evaluations that differ in the order of their sums (the reasoning behind C_HEAD in tests/test_gpu_vggt.py); C_DEPTH is the smallest of
2, 4, 8 that held at the first run on an MI355X, and a ratio above 8 would mean that something runs below fp32 width.
Chain, depth(images) on the g26 aggregator with depth_layers (0, 1, 1, 0) against the float64 chain <= C_AGG x the recorded error of the
reference's own chain (bf16-autocast tokens into the fp32 head); C_AGG = 1 is tests/test_gpu_vggt.py's, not re-measured.
Released shape: wf_conv2d_f32 at 84 x 148, 256 -> 256 with relu_in + relu_resid (the layer that dominates the FLOPs) and at 294 x 518,
128 -> 32 with relu_out, seeded data, a few hundred sampled output elements against float64 with the conv bar of tests/vggt_depth_cases.py.

Measured on an MI355X at the first run (rel-L2 against float64; ratio = this engine / the recorded reference error):
    head alone, depth     (1, 14, 14) 1.136e-07, (1, 14, 28) 1.402e-07, (2, 42, 70) 2.716e-07, (2, 154, 210) 5.620e-07 against the fp32 module's
                          9.464e-08, 1.117e-07, 3.192e-07, 6.380e-07                                  (ratios 1.20, 1.26, 0.85, 0.88)
    head alone, conf      7.783e-08, 9.607e-08, 1.619e-07, 2.954e-07 against 6.423e-08, 7.324e-08, 1.653e-07, 3.150e-07
                                                                                                      (ratios 1.21, 1.31, 0.98, 0.94)   -> C_DEPTH = 2
    chain, depth          g26 case 1 6.644e-04, case 2 7.023e-04 against the reference's chain 7.103e-04, 9.018e-04   (ratios 0.94, 0.78)
    chain, conf           2.549e-04, 3.145e-04 against 3.391e-04, 4.557e-04                                           (ratios 0.75, 0.69)
    released shape        worst |err| / bar 0.001 (84 x 148, 256 -> 256) and 0.002 (294 x 518, 128 -> 32) over 300 sampled elements each
The new cases have no entries in tests/golden/tolerances_mi355x.json yet."""
import numpy as np
import pytest
import torch

from tests import vggt_cases as vc
from tests import vggt_depth_cases as dc
from tests._tol import within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
C_AGG = 1.0
C_DEPTH = 2.0
HEAD_LAYERS = (0, 1, 2, 3)


def rel(a, b):
    return ((a.cpu().to(F64) - b.to(F64)).norm() / b.to(F64).norm()).item()


def _model(key="chain_config", depth=True):
    from worldforge_amd import vggt
    fx = dc.fixture()
    return vggt.VGGT(vggt.VGGTConfig.from_dict(fx[key]), DEV).load_state_dict(fx["sd"], depth=depth)


@pytest.fixture(scope="module")
def model():
    return _model()


def _head_tokens(c):
    return {k: c["tokens"][k].to(F32).to(DEV) for k in HEAD_LAYERS}


@pytest.fixture(scope="module")
def head_runs(model):
    """The head alone on every recorded case, once; left unchanged."""
    return [model.depth_from_tokens(_head_tokens(c), (c["H"], c["W"]), layers=HEAD_LAYERS) for c in dc.fixture()["head_cases"]]


@pytest.fixture(scope="module")
def chain_runs(model):
    return [model.depth(c["images"]) for c in dc.fixture()["chain_cases"]]


@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_head_alone_is_as_close_to_fp64_as_the_fp32_module(head_runs, ci):
    c = dc.fixture()["head_cases"][ci]
    depth, conf = head_runs[ci]
    assert depth.dtype == F32 and conf.dtype == F32
    assert tuple(depth.shape) == (1, c["S"], c["H"], c["W"], 1) and tuple(conf.shape) == (1, c["S"], c["H"], c["W"])
    assert bool(torch.isfinite(depth).all()) and bool((depth > 0).all()) and bool((conf > 1).all())
    rd, rc = rel(depth, c["depth"]), rel(conf, c["conf"])
    print(f"vggt depth head case {ci} (S {c['S']} {c['H']}x{c['W']}): depth rel-L2 {rd:.4e}, fp32 module {c['rel_f32_depth']:.4e} (ratio "
          f"{rd / c['rel_f32_depth']:.3f}); conf {rc:.4e}, fp32 module {c['rel_f32_conf']:.4e} (ratio {rc / c['rel_f32_conf']:.3f})")
    within("vggt_depth_head", rd, C_DEPTH * c["rel_f32_depth"])
    within("vggt_depth_head_conf", rc, C_DEPTH * c["rel_f32_conf"])


@pytest.mark.parametrize("ci", [0, 1])
def test_depth_end_to_end_against_the_float64_chain(model, chain_runs, ci):
    c = dc.fixture()["chain_cases"][ci]
    depth, conf = chain_runs[ci]
    S, H, W = c["images"].shape[1], c["images"].shape[3], c["images"].shape[4]
    assert depth.dtype == F32 and tuple(depth.shape) == (1, S, H, W, 1) and tuple(conf.shape) == (1, S, H, W)
    assert bool((depth > 0).all()) and bool((conf > 1).all())
    rd, rc = rel(depth, c["depth"]), rel(conf, c["conf"])
    print(f"vggt depth chain g26 case {c['g26_case']}: depth rel-L2 {rd:.4e}, the reference's chain {c['rel_chain_depth']:.4e} (ratio "
          f"{rd / c['rel_chain_depth']:.3f}); conf {rc:.4e}, the reference's chain {c['rel_chain_conf']:.4e} (ratio {rc / c['rel_chain_conf']:.3f})")
    within("vggt_depth_chain", rd, C_AGG * c["rel_chain_depth"])
    within("vggt_depth_chain_conf", rc, C_AGG * c["rel_chain_conf"])
    d2, c2 = model.depth(c["images"][0])                                          # [S, 3, H, W] without the batch dimension; two runs bit-equal
    assert torch.equal(d2, depth) and torch.equal(c2, conf)


def test_frames_chunk_sizes_are_bit_equal(model, head_runs):
    c = dc.fixture()["head_cases"][2]
    toks = _head_tokens(c)
    for chunk in (1, 2, None):
        d, cf = model.depth_from_tokens(toks, (c["H"], c["W"]), frames_chunk_size=chunk, layers=HEAD_LAYERS)
        assert torch.equal(d, head_runs[2][0]) and torch.equal(cf, head_runs[2][1]), chunk
    with pytest.raises(ValueError):
        model.depth_from_tokens(toks, (c["H"], c["W"]), frames_chunk_size=0, layers=HEAD_LAYERS)
    with pytest.raises(ValueError):
        model.depth_from_tokens(toks, (c["H"], c["W"] + 14), layers=HEAD_LAYERS)
    with pytest.raises(ValueError):
        model.depth_from_tokens({k: toks[k] for k in (0, 1, 2)}, (c["H"], c["W"]), layers=HEAD_LAYERS)      # a kept layer is missing
    with pytest.raises(ValueError):
        model.depth_from_tokens({k: v.double() for k, v in toks.items()}, (c["H"], c["W"]), layers=HEAD_LAYERS)


def test_batch_of_two_equals_two_single_calls(model, chain_runs):
    c = dc.fixture()["chain_cases"][0]
    other = c["images"].flip(1)
    d, cf = model.depth(torch.cat([c["images"], other], 0))
    d1, c1 = model.depth(other)
    assert tuple(d.shape)[0] == 2 and torch.equal(d[:1], chain_runs[0][0]) and torch.equal(cf[:1], chain_runs[0][1])
    assert torch.equal(d[1:], d1) and torch.equal(cf[1:], c1)


def test_predict_is_cameras_plus_depth_on_one_aggregator_pass(model, chain_runs, monkeypatch):
    c = dc.fixture()["chain_cases"][0]
    ext, intr = model.cameras(c["images"])
    pose = model.camera(c["images"])
    calls = []
    inner = model._aggregate_one
    monkeypatch.setattr(model, "_aggregate_one", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    r = model.predict(c["images"])
    assert len(calls) == 1
    assert sorted(r) == ["depth", "depth_conf", "extrinsic", "intrinsic", "pose_enc"]
    assert torch.equal(r["pose_enc"], pose) and torch.equal(r["extrinsic"], ext) and torch.equal(r["intrinsic"], intr)
    assert torch.equal(r["depth"], chain_runs[0][0]) and torch.equal(r["depth_conf"], chain_runs[0][1])


def test_a_model_loaded_without_the_head_refuses_the_depth_methods(head_runs):
    m = _model(depth=False)
    c = dc.fixture()["chain_cases"][0]
    h = dc.fixture()["head_cases"][0]
    assert not m.has_depth and not any(k.startswith("dpt.") for k in m.W)
    for call in (lambda: m.depth(c["images"]), lambda: m.predict(c["images"]),
                 lambda: m.depth_from_tokens(_head_tokens(h), (h["H"], h["W"]), layers=HEAD_LAYERS)):
        with pytest.raises(RuntimeError, match="depth=True"):
            call()
    assert tuple(m.camera(c["images"]).shape) == (1, 3, 9)                          # the cameras are served as before


def test_from_pretrained_with_depth_reproduces_load_state_dict(chain_runs, tmp_path, monkeypatch):
    import warnings
    from worldforge_amd import checkpoint, vggt
    fx = dc.fixture()
    c = fx["chain_cases"][0]
    folder = vc.write_folder(str(tmp_path / "ok"), sd=fx["sd"], config=fx["chain_config"], extra={"point_head.x": torch.zeros(4, dtype=BF)})
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        m = vggt.VGGT.from_pretrained(folder, device=DEV, depth=True)
    assert len([w for w in rec if "not consumed" in str(w.message)]) == 1
    d, cf = m.depth(c["images"])
    assert torch.equal(d, chain_runs[0][0]) and torch.equal(cf, chain_runs[0][1])
    with warnings.catch_warnings(record=True) as rec:                               # without depth=True the same folder loads as before
        warnings.simplefilter("always")
        m0 = vggt.VGGT.from_pretrained(folder, device=DEV)
    assert len([w for w in rec if "not consumed" in str(w.message)]) == 1 and not m0.has_depth

    def no_upload(*a, **k):
        raise AssertionError("tensor bytes were read although the header is wrong")
    monkeypatch.setattr(checkpoint, "load_file", no_upload)
    mk = lambda name, **kw: vc.write_folder(str(tmp_path / name), sd=fx["sd"], config=fx["chain_config"], **kw)  # noqa: E731
    with pytest.raises(KeyError):
        vggt.VGGT.from_pretrained(mk("missing", drop=("depth_head.norm.bias",)), device=DEV, depth=True)
    with pytest.raises(ValueError, match="shape"):
        vggt.VGGT.from_pretrained(mk("shape", reshape={"depth_head.projects.0.weight": (32, 256)}), device=DEV, depth=True)
    with pytest.raises(ValueError, match="not consumed"):
        vggt.VGGT.from_pretrained(mk("extra", extra={"depth_head.extra": torch.zeros(2, dtype=BF)}), device=DEV, depth=True)


def test_command_line_with_depth_writes_the_maps(tmp_path):
    from PIL import Image
    from worldforge_amd import vggt
    fx = dc.fixture()
    pre = vc.fixture()["preprocess"]
    folder = vc.write_folder(str(tmp_path / "ckpt"), sd=fx["sd"], config=fx["chain_config"])
    paths = []
    for i in range(2):
        paths.append(str(tmp_path / f"{i}.png"))
        Image.fromarray(np.roll(pre["landscape_in"], 40 * i, axis=1)).save(paths[-1])
    out, out0 = str(tmp_path / "d.npz"), str(tmp_path / "c.npz")
    assert vggt.main(["--checkpoint", folder, "--images", *paths, "--out", out0, "--device", DEV]) == 0
    assert vggt.main(["--checkpoint", folder, "--images", *paths, "--out", out, "--device", DEV, "--depth"]) == 0
    z, z0 = np.load(out), np.load(out0)
    assert sorted(z0.files) == ["extrinsic", "image_size_hw", "intrinsic", "pose_enc"]
    assert sorted(z.files) == ["depth", "depth_conf", "extrinsic", "image_size_hw", "intrinsic", "pose_enc"]
    x = vggt.preprocess([Image.open(p) for p in paths])
    m = vggt.VGGT.from_pretrained(folder, device=DEV, depth=True)
    d, cf = m.depth(x)
    H, W = z["image_size_hw"].tolist()
    assert tuple(z["depth"].shape) == (1, 2, H, W, 1) and tuple(z["depth_conf"].shape) == (1, 2, H, W)
    assert np.array_equal(z["depth"], d.cpu().numpy()) and np.array_equal(z["depth_conf"], cf.cpu().numpy())
    assert np.array_equal(z["pose_enc"], z0["pose_enc"]) and np.array_equal(z["intrinsic"], z0["intrinsic"])


def test_to_image_size_is_half_pixel_bilinear_and_scales_the_intrinsics(chain_runs):
    from worldforge_amd import vggt
    c = dc.fixture()["chain_cases"][0]
    depth, conf = chain_runs[0]
    H, W = depth.shape[2:4]
    intr = torch.tensor([[300.0, 0, W / 2], [0, 280.0, H / 2], [0, 0, 1]], device=DEV).expand(1, depth.shape[1], 3, 3).contiguous()
    oh, ow = 97, 161
    d, cf, K = vggt.to_image_size(depth, conf, intr, (H, W), (oh, ow))
    assert tuple(d.shape) == (1, depth.shape[1], oh, ow, 1) and tuple(cf.shape) == (1, depth.shape[1], oh, ow) and d.dtype == F32
    Fn = torch.nn.functional
    want_d = Fn.interpolate(depth.cpu().to(F64)[0, ..., 0][:, None], size=(oh, ow), mode="bilinear", align_corners=False)[:, 0]
    want_c = Fn.interpolate(conf.cpu().to(F64)[0][:, None], size=(oh, ow), mode="bilinear", align_corners=False)[:, 0]
    # fp32: src = (dst + 0.5) * (in / out) - 0.5 carries three roundings on magnitudes <= in, so the weights are off by <= 3 U in and
    # the value by that times the largest neighbour difference along the axis; then four products and three sums: 8 U max|v|
    def tol(v):
        v = v.cpu().to(F64)
        dy, dx = (v[..., 1:, :] - v[..., :-1, :]).abs().max().item(), (v[..., :, 1:] - v[..., :, :-1]).abs().max().item()
        return 8 * dc.U * v.abs().max().item() + 3 * dc.U * (H * dy + W * dx)
    tol_d, tol_c = tol(depth[..., 0]), tol(conf)
    assert float((d.cpu().to(F64)[0, ..., 0] - want_d).abs().max()) <= tol_d and float((cf.cpu().to(F64)[0] - want_c).abs().max()) <= tol_c
    want_K = intr.cpu().clone()
    want_K[..., 0, 0] *= ow / W
    want_K[..., 0, 2] *= ow / W
    want_K[..., 1, 1] *= oh / H
    want_K[..., 1, 2] *= oh / H
    assert torch.equal(K.cpu(), want_K) and torch.equal(intr.cpu()[..., 0, 0], torch.full((1, depth.shape[1]), 300.0))   # the input is not modified


# ---- the released shape ---------------------------------------------------------------------------------------------------------------------
def _sampled_conv(Hi, Wi, Cin, Cout, relu_in, with_resid, relu_out, seed):
    """One wf_conv2d_f32 call at a released shape; a few hundred output elements (the four corners, the edges, the tile seams and a seeded
    scatter) against float64 computed for those elements alone, with the conv bar."""
    from worldforge_amd import ops
    from worldforge_amd._ffi import call
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, Hi, Wi, Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
    b = 0.1 * torch.randn(Cout, generator=g)
    r = torch.randn(1, Hi, Wi, Cout, generator=g) if with_resid else None
    xd, wp, bd = x.to(DEV), dc.pack_conv_weight(w).to(DEV), b.to(DEV)
    rd = None if r is None else r.to(DEV)
    out = torch.full((1, Hi, Wi, Cout), float("nan"), dtype=F32, device=DEV)
    call("wf_conv2d_f32", xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), None if rd is None else rd.data_ptr(), out.data_ptr(), 1, Hi, Wi, Cin, Cout,
         1, int(relu_in), int(with_resid), int(relu_out), ops.stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    ys = torch.cat([torch.tensor([0, 0, Hi - 1, Hi - 1, 0, Hi - 1, Hi // 2, Hi // 2]), torch.randint(0, Hi, (292,), generator=g)])
    xs = torch.cat([torch.tensor([0, Wi - 1, 0, Wi - 1, Wi // 2, Wi // 2, 0, Wi - 1]), torch.randint(0, Wi, (292,), generator=g)])
    cs = torch.randint(0, Cout, (300,), generator=g)
    cs[:4] = torch.tensor([0, Cout - 1, min(127, Cout - 1), min(128, Cout - 1)])
    xp = torch.zeros(Hi + 2, Wi + 2, Cin, dtype=F64)
    xp[1:-1, 1:-1] = torch.relu(x[0].to(F64)) if relu_in else x[0].to(F64)
    patch = torch.stack([xp[y:y + 3, xx:xx + 3] for y, xx in zip(ys.tolist(), xs.tolist())])           # [300, 3, 3, Cin]
    wk = w.to(F64)[cs].permute(0, 2, 3, 1)                                                          # [300, 3, 3, Cin]
    ref, S = (patch * wk).sum((1, 2, 3)) + b.to(F64)[cs], (patch.abs() * wk.abs()).sum((1, 2, 3)) + b.to(F64)[cs].abs()
    if r is not None:
        rr = torch.relu(r[0, ys, xs, cs].to(F64))
        ref, S = ref + rr, S + rr
    if relu_out:
        ref = torch.relu(ref)
    bar = (9 * Cin + 4) * dc.U * S + dc.U * ref.abs()
    ratio = ((out[0, ys, xs, cs].cpu().to(F64) - ref).abs() / bar).max().item()
    print(f"wf_conv2d_f32 released shape {Hi}x{Wi} {Cin}->{Cout}: worst |err| / bar over {len(cs)} sampled elements {ratio:.3f}")
    assert ratio <= 1.0


def test_released_shape_residual_unit_conv():
    _sampled_conv(84, 148, 256, 256, relu_in=True, with_resid=True, relu_out=False, seed=31)


def test_released_shape_output_conv2():
    _sampled_conv(294, 518, 128, 32, relu_in=False, with_resid=False, relu_out=True, seed=32)
