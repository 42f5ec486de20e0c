"""CPU: the VAE's weight packing (worldforge_amd/vae_weights.py) -- state dict -> matrix-core operands, on device="cpu", no kernel library.

Bounds (derived from the fp16 format, nothing measured): fp16 carries 11 significand bits, so hi = fp16(v) has |v - hi| <= 2^-11 |v| while hi is
a normal number and <= 2^-25 (half the subnormal spacing 2^-24) below that.  The weight is stored as v = w * 2^k (exact in fp32) with the
matrix's largest |v| in [2^13, 2^14).  One term ("fp16"): |hi * 2^-k - w| <= max(2^-11 |w|, 2^-25 * 2^-k).  Two terms ("fp16x3": lo =
fp16(v - hi), the difference is exact in fp32): |v - hi - lo| <= 2^-11 |v - hi| <= 2^-22 |v|, or 2^-25 where lo is subnormal, so
|(hi + lo) * 2^-k - w| <= max(2^-22 |w|, 2^-25 * 2^-k)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vae as ovae
from worldforge_amd.vae_weights import (decoder_plan, diffusers_key_map, diffusers_to_twin_state_dict, encoder_plan, pack_state_dict,
                                        weight_operand)

F32, F64 = torch.float32, torch.float64
PRECISIONS = ["bf16", "fp16x3", "bf16x3", "fp16"]
_CACHE = {}


def _sd():
    if "sd" not in _CACHE:
        _CACHE["sd"] = ovae.random_weights(seed=5)
    return _CACHE["sd"]


def _packed(precision):
    if precision not in _CACHE:
        _CACHE[precision] = pack_state_dict(_sd(), precision, "cpu")
    return _CACHE[precision]


def _operand_layers():
    """What the plans imply: {key: (kind, Cout, taps, Cin)} of every matrix-core weight operand (kind "lin": 2-D, no taps), {key: length}
    of every f32 vector (gammas, biases)."""
    ops, vecs = {}, {}

    def conv(p, cout, taps, cin, kind="conv", bias=True):
        ops[p] = (kind, cout, taps, cin)
        if bias:
            vecs[p + ".b"] = cout

    seen_up = False
    for plan in (encoder_plan(), decoder_plan()):
        for kind, p, cin, cout in plan:
            if kind == "conv_in":
                conv(p, cout, 27, 32)                                   # Cin zero-padded to one 32-channel K slice
            elif kind == "res":
                vecs[p + ".residual.0.gamma"], vecs[p + ".residual.3.gamma"] = cin, cout
                conv(p + ".residual.2", cout, 27, cin)
                conv(p + ".residual.6", cout, 27, cout)
                if cin != cout:
                    conv(p + ".shortcut", cout, 1, cin, "lin")
            elif kind == "attn":
                vecs[p + ".norm.gamma"] = cin
                conv(p + ".to_qkv", 3 * cin, 1, cin, "lin")
                conv(p + ".proj", cin, 1, cin, "lin")
            elif kind in ("down2d", "down3d"):
                conv(p + ".resample.1", cin, 9, cin)
                if kind == "down3d":
                    conv(p + ".time_conv", cin, 3, cin)
            elif kind in ("up2d", "up3d"):
                conv(p + ".resample.1", cin // 2, 9, cin)
                if seen_up:                                             # every upsampling conv but the first has its four phase operands
                    for ph in ("ph00", "ph01", "ph10", "ph11"):
                        conv(f"{p}.resample.1.{ph}", cin // 2, 4, cin, bias=False)
                seen_up = True
                if kind == "up3d":
                    conv(p + ".time_conv", 2 * cin, 3, cin)
            elif kind == "head":
                vecs[p + ".0.gamma"] = cin
                conv(p + ".2", (cout + 31) // 32 * 32, 27, cin)         # Cout zero-padded to one 32-channel output block
    return ops, vecs


def _ref_operand(p, kind, cout, taps, cin):
    """The f32 weight of layer p in the operand's layout [Cout, taps, Cin] (zero-padded), or [Cout, Cin] for "lin"."""
    w = _sd()[p + ".weight"].to(F32)
    if kind == "lin":
        return w.reshape(cout, cin)
    if w.dim() == 4:
        w = w.unsqueeze(2)
    w = w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], taps, w.shape[1])
    out = torch.zeros(cout, taps, cin)
    out[:w.shape[0], :, :w.shape[2]] = w
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
def test_keys_shapes_and_dtypes_are_what_the_plans_imply(precision):
    W = _packed(precision)
    ops, vecs = _operand_layers()
    terms = 3 if precision in ("bf16x3", "fp16x3") else 1
    op_dtype = torch.float16 if precision in ("fp16x3", "fp16") else torch.bfloat16
    want = {}
    for p, (kind, cout, taps, cin) in ops.items():
        want[p + ".w"] = ((cout, terms * cin) if kind == "lin" else (cout, taps, terms * cin), op_dtype)
        if op_dtype == torch.float16:
            want[p + ".w.scale"] = float
    for key, n in vecs.items():
        want[key] = ((n,), F32)
    want.update({"conv1.w": ((1, 32, 32), F32), "conv1.b": ((32,), F32), "conv2.w": ((1, 16, 32), F32), "conv2.b": ((32,), F32)})
    assert set(W) == set(want), sorted(set(W) ^ set(want))
    for key, spec in want.items():
        if spec is float:
            assert isinstance(W[key], float), key
        else:
            assert (tuple(W[key].shape), W[key].dtype) == spec and W[key].is_contiguous(), (key, W[key].shape, W[key].dtype)
    assert sum(k.endswith(".ph00.w") for k in W) == 2 and "decoder.upsamples.3.resample.1.ph00.w" not in W


def _rebuilt(W, key, cin, precision):
    """The weight operand `key` back in f64: (hi + lo) * scale, or hi * scale for the one-term mode -> (value, hi, scale)."""
    op, scale = W[key].to(F64), W[key + ".scale"]
    if precision == "fp16":
        return op * scale, op, scale
    hi, hi2, lo = op[..., :cin], op[..., cin:2 * cin], op[..., 2 * cin:]
    assert torch.equal(hi, hi2)                                          # [hi | hi | lo]: the weight side of the three-term split
    return (hi + lo) * scale, hi, scale


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_fp16_operands_are_scaled_into_the_normal_range_and_carry_their_bits(precision):
    W = _packed(precision)
    rel = 2.0 ** -22 if precision == "fp16x3" else 2.0 ** -11            # (module docstring)
    ops, _ = _operand_layers()
    for p, (kind, cout, taps, cin) in ops.items():
        if ".ph" in p:
            continue                                                      # (pre-summed taps: test_phase_operands_...)
        got, hi, scale = _rebuilt(W, p + ".w", cin, precision)
        assert math.frexp(scale)[0] == 0.5, (p, scale)                    # an exact power of two
        assert 2.0 ** 13 <= float(hi.abs().max()) < 2.0 ** 14, (p, float(hi.abs().max()))
        ref = _ref_operand(p, kind, cout, taps, cin).to(F64)
        bound = torch.maximum(rel * ref.abs(), torch.full_like(ref, 2.0 ** -25 * scale))
        assert bool(((got - ref).abs() <= bound).all()), (p, float(((got - ref).abs() / bound).max()))


def test_weight_operand_of_an_all_zero_and_a_non_finite_matrix():
    op, scale = weight_operand(torch.zeros(4, 8), "fp16x3", "cpu")
    assert scale is None and tuple(op.shape) == (4, 24) and not op.any()
    with pytest.raises(ValueError):
        weight_operand(torch.full((2, 2), float("inf")), "fp16", "cpu")


@pytest.mark.parametrize("p,cin", [("decoder.upsamples.7", 384), ("decoder.upsamples.11", 192)])
def test_phase_operands_equal_the_upsampled_3x3_conv(p, cin):
    """The four phase operands, rebuilt to f32 values from "fp16x3" and applied in f64 as 2 x 2 convolutions scattered to (2y + py, 2x + px),
    against conv2d(nearest-2x(x), w, padding=1) in f64.  Tolerance per output: every product x * w of the 9-tap sum carries the split's
    2^-22 |w| (module docstring; |sum of taps| <= sum of |taps|) plus the f32 pre-summation of up to 4 taps (3 additions of 2^-24 each
    < 2^-22): 2^-21 * sum |x| |w|; plus the subnormal floor 2^-25 * scale for each of the 4 Cin products of a phase."""
    W = _packed("fp16x3")
    w = _sd()[p + ".resample.1.weight"].to(F64)                           # [Cout, Cin, 3, 3]
    cout = w.shape[0]
    assert w.shape[1] == cin
    x = torch.randn(1, cin, 5, 7, generator=torch.Generator().manual_seed(7), dtype=F64)
    xu = F.interpolate(x, scale_factor=2, mode="nearest")
    ref = F.conv2d(xu, w, padding=1)
    got = torch.full_like(ref, float("nan"))
    floor = torch.zeros_like(ref)
    for py in range(2):
        for px in range(2):
            key = f"{p}.resample.1.ph{py}{px}.w"
            wp, _, scale = _rebuilt(W, key, cin, "fp16x3")                # [Cout, 4, Cin], tap = 2 a + b
            wp = wp.reshape(cout, 2, 2, cin).permute(0, 3, 1, 2)          # [Cout, Cin, a, b]: source (y - 1 + py + a, x - 1 + px + b)
            full = F.conv2d(x, wp, padding=1)                             # [.., 6, 8]: output i reads source rows {i - 1, i}
            got[:, :, py::2, px::2] = full[:, :, py:py + 5, px:px + 7]
            floor[:, :, py::2, px::2] = (2.0 ** -25 * scale) * F.conv2d(x.abs(), torch.ones_like(wp), padding=1)[:, :, py:py + 5, px:px + 7]
    assert torch.isfinite(got).all()                                      # every output pixel written by exactly one phase
    tol = 2.0 ** -21 * F.conv2d(xu.abs(), w.abs(), padding=1) + floor
    assert bool(((got - ref).abs() <= tol).all()), float(((got - ref).abs() / tol).max())


@pytest.mark.parametrize("precision", ["fp16x3", "bf16"])
def test_diffusers_names_pack_to_the_same_tensors(precision, golden_dir):
    """The mapped names and shapes are those the executed class recorded (g8b: loads without a device)."""
    b = np.load(os.path.join(golden_dir, "g8b_vae_akw.npz"))
    shapes = {str(n): tuple(int(v) for v in str(s).split(",")) for n, s in zip(b["param_names"], b["param_shapes"])}
    inv = {v: k for k, v in diffusers_key_map().items()}
    sd = {}
    for k, v in _sd().items():
        base, _, leaf = k.rpartition(".")
        sd[f"{inv[base]}.{leaf}"] = v.reshape(shapes[f"{inv[base]}.{leaf}"]).contiguous()
    assert set(sd) == set(shapes)
    got, want = pack_state_dict(diffusers_to_twin_state_dict(sd), precision, "cpu"), _packed(precision)
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v, k
    with pytest.raises(KeyError):
        diffusers_to_twin_state_dict({"encoder.not_a_layer.weight": torch.zeros(1)})
