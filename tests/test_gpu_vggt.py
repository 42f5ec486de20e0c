"""GPU: the native VGGT aggregator and camera head (worldforge_amd/vggt.py) on the recorded fixture tests/golden/g26_vggt_*: the
reference's own Aggregator / DinoVisionTransformer / CameraHead at width 128 (2 heads x 64, depth 2, one DINOv2 block, one trunk block of
2 x 128-wide heads), cases (S, H, W) = (1, 56, 84), (3, 56, 84), (2, 154, 210).  The reference package is never imported here.

Aggregator bar: for every case and kept layer, rel-L2 of the tokens against the float64 module <= C_AGG x the recorded rel-L2 of the
reference's bf16-autocast module.  This engine is at least as wide at every point (fp32 residual stream, LayerNorms, softmax, GELU input),
except that P is bf16 as in any fused kernel.  C_AGG is the smallest of 1, 2, 4 that held at the first measurement on an MI355X; a ratio
above 4 would mean something is evaluated below the module's width.
Camera head bar: the head alone on the recorded float64 tokens against the float64 pose_enc <= C_HEAD x the recorded error of the fp32
module on the same tokens: both are fp32 evaluations that differ in the order of their sums (the reasoning of tests/test_gpu_clip.py);
C_HEAD is the smallest of 2, 4, 8 that held.
End to end: pose_enc against float64 <= C_AGG x the recorded error of the reference's own chain (bf16-autocast tokens into the fp32 head).
The released shape (width 1024, 16 heads, S = 2 at 518 x 294 = 782 tokens per frame; one frame block and one global block, seeded
weights) is checked on sampled rows against a float64 evaluation of the same two blocks written out in torch below; bar: the rel-L2 of
the same restatement evaluated in bfloat16 on the CPU, x C_AGG.

Measured on an MI355X at the first run (rel-L2 against float64; ratio = this engine / the recorded reference error):
    tokens, layer 0 / 1   (1, 56, 84): 1.830e-03 / 2.036e-03 against bf16 autocast 2.657e-03 / 2.928e-03   (ratios 0.689 / 0.695)
                          (3, 56, 84): 1.879e-03 / 2.092e-03 against 2.632e-03 / 2.890e-03                 (ratios 0.714 / 0.724)
                          (2, 154, 210): 1.837e-03 / 1.985e-03 against 2.626e-03 / 2.845e-03               (ratios 0.700 / 0.698)   -> C_AGG = 1
    camera head alone     6.961e-08, 1.401e-07, 1.181e-07 against the fp32 module's 1.550e-07, 1.011e-07, 8.946e-08 (ratios 0.45, 1.39, 1.32) -> C_HEAD = 2
    pose_enc end to end   1.370e-03, 1.318e-03, 1.359e-03 against the reference's chain 1.914e-03, 2.156e-03, 1.692e-03 (ratios 0.72, 0.61, 0.80)
    released shape        2.400e-03 against 1.437e-02 of the bfloat16 restatement (ratio 0.17; both relative to the update the two blocks make)
(The recorded fp32 module is 4.5e-07 - 4.8e-07 from float64 on the tokens: the distance above is the bf16 operands', as in the reference.)
The new cases have no entries in tests/golden/tolerances_mi355x.json yet."""
import warnings

import numpy as np
import pytest
import torch

from tests import vggt_cases as vc
from tests._tol import within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
C_AGG = 1.0
C_HEAD = 2.0


def _model(sd=None):
    from worldforge_amd import vggt
    fx = vc.fixture()
    return vggt.VGGT(vggt.VGGTConfig.from_dict(fx["config"]), DEV).load_state_dict(sd or fx["sd"])


def rel(a, b):
    return ((a.cpu().to(F64) - b.to(F64)).norm() / b.to(F64).norm()).item()


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def runs(model):
    """Every case once: ({layer: tokens}, pose_enc); left unchanged."""
    out = []
    for c in vc.fixture()["cases"]:
        toks, start = model.aggregate(c["images"], keep="all")
        assert start == 5
        out.append((toks, model.camera_from_tokens(toks[1])))
    return out


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_aggregated_tokens_are_as_close_to_fp64_as_the_bf16_autocast_module(runs, ci):
    c = vc.fixture()["cases"][ci]
    toks, _ = runs[ci]
    P = (c["H"] // 14) * (c["W"] // 14)
    assert sorted(toks) == [0, 1]
    for k in (0, 1):
        assert toks[k].dtype == F32 and tuple(toks[k].shape) == (1, c["S"], 5 + P, 256) and bool(torch.isfinite(toks[k]).all())
        r = rel(toks[k], c["tokens"][k])
        print(f"vggt tokens case {ci} (S {c['S']} {c['H']}x{c['W']}) layer {k}: rel-L2 {r:.4e}, bf16-autocast module {c['rel_bf16'][k]:.4e} "
              f"(ratio {r / c['rel_bf16'][k]:.3f}), fp32 module {c['rel_f32'][k]:.4e}")
        within("vggt_tokens", r, C_AGG * c["rel_bf16"][k])


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_camera_head_alone_is_as_close_as_the_fp32_module(model, ci):
    c = vc.fixture()["cases"][ci]
    got = model.camera_from_tokens(c["tokens"][1].to(F32).to(DEV))
    assert got.dtype == F32 and tuple(got.shape) == (1, c["S"], 9)
    r = rel(got, c["pose64"])
    print(f"vggt head case {ci}: rel-L2 {r:.4e}, fp32 module {c['pose_rel_head32']:.4e} (ratio {r / c['pose_rel_head32']:.3f})")
    within("vggt_head", r, C_HEAD * c["pose_rel_head32"])


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_pose_enc_end_to_end(model, runs, ci):
    c = vc.fixture()["cases"][ci]
    pose = runs[ci][1]
    r = rel(pose, c["pose64"])
    print(f"vggt pose_enc case {ci}: rel-L2 {r:.4e}, the reference's chain {c['pose_rel_chain']:.4e} (ratio {r / c['pose_rel_chain']:.3f})")
    within("vggt_pose", r, C_AGG * c["pose_rel_chain"])
    assert bool((pose[..., 7:] > 0).all())
    assert torch.equal(model.camera(c["images"]), pose)                           # camera() = aggregate + head, and two runs are bit-equal
    ext, intr = model.cameras(c["images"][0])                                     # [S, 3, H, W] without the batch dimension
    from worldforge_amd import vggt
    e2, i2 = vggt.pose_encoding_to_extri_intri(pose, (c["H"], c["W"]))
    assert torch.equal(ext, e2) and torch.equal(intr, i2) and tuple(ext.shape) == (1, c["S"], 3, 4) and tuple(intr.shape) == (1, c["S"], 3, 3)


def test_runs_are_bit_equal_and_keep_subsets(model, runs):
    c = vc.fixture()["cases"][1]
    toks, _ = runs[1]
    again, _ = model.aggregate(c["images"], keep="all")
    assert len(again) == 2 and all(torch.equal(again[k], toks[k]) for k in (0, 1))
    for k in (0, 1):
        sub, _ = model.aggregate(c["images"], keep=(k,))
        assert list(sub) == [k] and torch.equal(sub[k], toks[k])
    with pytest.raises(ValueError):
        model.aggregate(c["images"], keep=(2,))
    with pytest.raises(ValueError):
        model.aggregate(c["images"][..., :50])
    with pytest.raises(ValueError):
        model.aggregate(c["images"].double())


def test_first_frame_tokens_and_global_attention(model, runs):
    c = vc.fixture()["cases"][1]
    toks3 = runs[1][0][1]
    one, _ = model.aggregate(c["images"][:, :1], keep=(1,))
    d = rel(toks3[:, :1], one[1].cpu())
    assert d > 1e-2, d                                                           # frame 0 of S = 3 saw the other frames
    same, _ = model.aggregate(c["images"][:, :1].repeat(1, 3, 1, 1, 1), keep=(0,))
    t = same[0][0]                                                               # layer 0, frame half = columns 0..127: frame attention only
    assert rel(t[0, :, :128], t[1, :, :128].cpu()) > 1e-2                        # frame 0 carries the first-frame camera / register tokens
    assert rel(t[2, :, :128], t[1, :, :128].cpu()) < 1e-6                        # the later frames share theirs


def test_batch_of_two_equals_two_single_calls(model, runs):
    c = vc.fixture()["cases"][1]
    other = c["images"].flip(1)
    both, _ = model.aggregate(torch.cat([c["images"], other], 0), keep=(1,))
    single, _ = model.aggregate(other, keep=(1,))
    assert tuple(both[1].shape)[0] == 2 and torch.equal(both[1][:1], runs[1][0][1]) and torch.equal(both[1][1:], single[1])
    p = model.camera(torch.cat([c["images"], other], 0))
    assert torch.equal(p[:1], runs[1][1]) and torch.equal(p[1:], model.camera(other))


def test_from_pretrained_rules(model, runs, tmp_path, monkeypatch):
    from worldforge_amd import checkpoint, vggt
    fx = vc.fixture()
    c = fx["cases"][0]
    folder = vc.write_folder(str(tmp_path / "ok"), extra={"depth_head.scratch.weight": torch.zeros(4, 4, dtype=BF),
                                                          "aggregator.patch_embed.mask_token": torch.zeros(1, 128, dtype=BF)})
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        m = vggt.VGGT.from_pretrained(folder, device=DEV)
    assert len([w for w in rec if "not consumed" in str(w.message)]) == 1
    assert torch.equal(m.camera(c["images"]), runs[0][1])

    def no_upload(*a, **k):
        raise AssertionError("tensor bytes were read although the header is wrong")
    monkeypatch.setattr(checkpoint, "load_file", no_upload)
    with pytest.raises(KeyError):
        vggt.VGGT.from_pretrained(vc.write_folder(str(tmp_path / "missing"), drop=("camera_head.trunk_norm.weight",)), device=DEV)
    with pytest.raises(ValueError, match="shape"):
        vggt.VGGT.from_pretrained(vc.write_folder(str(tmp_path / "shape"), reshape={"aggregator.register_token": (1, 2, 2, 256)}), device=DEV)
    with pytest.raises(ValueError, match="not consumed"):
        vggt.VGGT.from_pretrained(vc.write_folder(str(tmp_path / "extra"), extra={"aggregator.extra": torch.zeros(2, dtype=BF)}), device=DEV)


def test_command_line_writes_the_cameras(tmp_path):
    from PIL import Image
    from worldforge_amd import vggt
    pre = vc.fixture()["preprocess"]
    folder = vc.write_folder(str(tmp_path / "ckpt"))
    paths = []
    for i in range(2):
        paths.append(str(tmp_path / f"{i}.png"))
        Image.fromarray(np.roll(pre["landscape_in"], 40 * i, axis=1)).save(paths[-1])
    out = str(tmp_path / "cams.npz")
    assert vggt.main(["--checkpoint", folder, "--images", *paths, "--out", out, "--device", DEV]) == 0
    z = np.load(out)
    x = vggt.preprocess([Image.open(p) for p in paths])
    m = vggt.VGGT.from_pretrained(folder, device=DEV)
    ext, intr = m.cameras(x)
    assert z["image_size_hw"].tolist() == [308, 518] and tuple(z["pose_enc"].shape) == (1, 2, 9)
    assert np.array_equal(z["extrinsic"], ext.cpu().numpy()) and np.array_equal(z["intrinsic"], intr.cpu().numpy())
    assert np.array_equal(z["pose_enc"], m.camera(x).cpu().numpy())


# ---- the released shape ---------------------------------------------------------------------------------------------------------------------
def _two_blocks(x, W, S, T, dt, dev):
    """A frame block then a global block (AGG:260-305, the Block of vggt/layers/block.py with q_norm / k_norm and the 2D RoPE) in plain
    torch at dtype dt on device dev: x [S T, C] -> [S T, C].  Every tensor, the tables included, is dt."""
    from worldforge_amd import vggt
    Fn = torch.nn.functional
    C, H = x.shape[1], x.shape[1] // 64
    cs, sn = vggt.rope_tables(37, 100.0)
    pos = vggt.token_positions(21, 37, 5).long()
    w = lambda k: W[k].to(dev).to(dt)  # noqa: E731
    cos = [torch.cat([cs, cs], -1).to(dev).to(dt)[pos[:, a].to(dev)] for a in (0, 1)]     # [T, 32] per axis
    sin = [torch.cat([sn, sn], -1).to(dev).to(dt)[pos[:, a].to(dev)] for a in (0, 1)]
    x = x.to(dev).to(dt)

    def rope(t):                                                                  # t [n, H, L, 64], L a multiple of T
        rep = t.shape[2] // T
        out = []
        for a, blk in enumerate(t.chunk(2, -1)):
            c, s = cos[a].repeat(rep, 1), sin[a].repeat(rep, 1)
            out.append(blk * c + torch.cat([-blk[..., 16:], blk[..., :16]], -1) * s)
        return torch.cat(out, -1)

    for name, nseq in (("f0", S), ("g0", 1)):
        L = x.shape[0] // nseq
        n = Fn.layer_norm(x, (C,), w(f"{name}.norm1.w"), w(f"{name}.norm1.b"), 1e-5)
        qkv = Fn.linear(n, w(f"{name}.qkv.w"), w(f"{name}.qkv.b")).view(nseq, L, 3, H, 64).permute(2, 0, 3, 1, 4)
        q = rope(Fn.layer_norm(qkv[0], (64,), w(f"{name}.q_norm.w"), w(f"{name}.q_norm.b"), 1e-5))
        k = rope(Fn.layer_norm(qkv[1], (64,), w(f"{name}.k_norm.w"), w(f"{name}.k_norm.b"), 1e-5))
        a = torch.softmax((q @ k.transpose(-1, -2)) * 0.125, -1) @ qkv[2]
        a = a.transpose(1, 2).reshape(nseq * L, C)
        x = x + w(f"{name}.ls1") * Fn.linear(a, w(f"{name}.proj.w"), w(f"{name}.proj.b"))
        n = Fn.layer_norm(x, (C,), w(f"{name}.norm2.w"), w(f"{name}.norm2.b"), 1e-5)
        x = x + w(f"{name}.ls2") * Fn.linear(Fn.gelu(Fn.linear(n, w(f"{name}.fc1.w"), w(f"{name}.fc1.b"))), w(f"{name}.fc2.w"), w(f"{name}.fc2.b"))
    return x


def test_released_shape_frame_and_global_block():
    from worldforge_amd import vggt
    cfg = vggt.VGGTConfig.from_dict({"depth": 1, "dino_depth": 1, "camera_trunk_depth": 1})
    m = vggt.VGGT(cfg, DEV).init_random(5)
    S, gh, gw, C = 2, 21, 37, 1024
    T = 5 + gh * gw
    M = S * T
    x0 = torch.randn(M, C, generator=torch.Generator().manual_seed(9))
    ws = {"n": torch.empty(M, C, dtype=BF, device=DEV), "qkv": torch.empty(M, 3 * C, dtype=BF, device=DEV), "att": torch.empty(M, C, dtype=BF, device=DEV),
          "hid": torch.empty(M, 4 * C, dtype=F32, device=DEV), "hb": torch.empty(M, 4 * C, dtype=BF, device=DEV)}
    x = x0.to(DEV)
    m._block(x, "f0", S, T, 16, 1e-5, m._rope(gh, gw, 1), ws)
    m._block(x, "g0", 1, M, 16, 1e-5, m._rope(gh, gw, S), ws)
    torch.cuda.synchronize()
    rows = torch.tensor(sorted(set(range(0, M, 29)) | set(range(6)) | set(range(T - 2, T + 7)) | {M - 1}))
    y64 = _two_blocks(x0, m.W, S, T, F64, DEV).cpu()[rows]
    ybf = _two_blocks(x0, m.W, S, T, BF, "cpu")[rows]
    assert bool(torch.isfinite(x).all())
    # the residual stream is dominated by x0 itself: judge the UPDATE the two blocks made
    upd64 = y64 - x0[rows].to(F64)
    r = ((x.cpu()[rows].to(F64) - y64).norm() / upd64.norm()).item()
    rbf = ((ybf.to(F64) - y64).norm() / upd64.norm()).item()
    print(f"vggt released shape: rel-L2 of the update {r:.4e}, the bfloat16 restatement on the CPU {rbf:.4e} (ratio {r / rbf:.3f})")
    within("vggt_released_blocks", r, C_AGG * rbf)
