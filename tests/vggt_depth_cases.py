"""Reader of the VGGT depth-head fixtures (tests/golden/g27_vggt_depth_*, written by tools/make_vggt_depth_golden.py), a float64 torch
restatement of the DPT head written from its data flow (NCHW, plain torch.nn.functional: the kernel tests' reference and the CPU tests'
subject) and the per-element bars of the kernels of csrc/dpt.hip.  The reference package is never imported here.

Bars (U = 2^-24, the unit roundoff of fp32; every bar is evaluated in float64 on the kernel's own fp32 inputs):
wf_conv2d_f32.  An output element is ONE chain of K = 9 Cin fp32 fma (one rounding each), then + bias, + residual (one rounding each) and
  the store is the last of those.  The standard bound of a chain of K + 2 roundings is gamma_{K+2} sum|terms|; with the padding taps being
  exact zeros it reads  bar = (9 Cin + 4) U S + U |ref|,  S = sum|x||w| + |bias| + |resid|  (the + 4 and the U |ref| cover the two epilogue
  adds, gamma's second-order term and the final rounding with room to spare: (K + 2) U / (1 - (K + 2) U) < (K + 4) U for K < 2^20).
wf_resize_bilinear_cl_f32.  fp32: scale = (in - 1) / (out - 1) (one rounding), src = scale * dst (one more: src is off by <= 2 U src <=
  2 U (in - 1) absolute, which moves the weights l1, l0 by that much: the result moves by <= 2 U (in - 1) |v_1 - v_0| per axis), l1 = src - i0
  exact (Sterbenz-like: both in [i0, i0 + 1)), l0 = 1 - l1 one rounding; then four products and three sums: <= 4 roundings deep on values
  bounded by A = sum of the four |weights| |values| (= the bilinear interpolation of |v|).  So
  bar = 8 U A + 2 U ((Hi - 1) Dy + (Wi - 1) Dx) + U |table| + 2 U |ref|,  Dy / Dx = the interpolated |difference| along the axis.  The test
  evaluates A, Dy, Dx with the same float64 interpolation (of |v| and of the neighbour differences).
wf_dpt_depth_out.  v = b + sum of Cin fma: |dv| <= (Cin + 2) U S, S = |b| + sum|x||w|; exp turns an absolute error dv into the relative
  error dv (first order, dv << 1) and expf itself is good to 2^-22 relative (2 ulp: the device library's documented bound is 1 ulp),
  the + 1 of conf adds one rounding:  bar = |ref| ((Cin + 2) U S + 2^-22 + U)  (for conf |ref - 1| carries the first two terms, and |ref|
  >= |ref - 1|).
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as Fn

from tests.vggt_cases import GOLDEN, bf16_of_bits, fixture as g26_fixture

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
RESIZE_CASES = (((1, 1), (1, 2)), ((1, 2), (2, 3)), ((2, 3), (4, 6)), ((6, 8), (11, 15)), ((11, 15), (11, 15)), ((22, 30), (154, 210)))

_FIX = None


def fixture():
    """{config (g26's + the depth head's width), chain_config (the same with depth_layers (0, 1, 1, 0)), sd (g26's aggregator and camera
    head + `depth_head.*`, bf16 tensors under the reference's key names), head_cases [{S, H, W, tokens [4 x bf16 [1, S, 5 + P, 256]],
    depth, conf (float64), rel_f32_depth, rel_f32_conf}], chain_cases [{images, depth, conf, rel_chain_depth, rel_chain_conf}],
    pos [(C, h, w, W, H, fp32 [C, h, w])], resize [(in fp32 [2, hi, wi], out float64 [2, ho, wo])], units {name: float64 tensor}}."""
    global _FIX
    if _FIX is None:
        g26 = g26_fixture()
        with open(os.path.join(GOLDEN, "g27_vggt_depth_meta.json")) as f:
            meta = json.load(f)
        ld = lambda name: np.load(os.path.join(GOLDEN, f"g27_vggt_depth_{name}.npz"))  # noqa: E731
        sd = dict(g26["sd"])
        for i in range(meta["weight_files"]):
            z = ld(f"weights{i}")
            sd.update({k[3:]: bf16_of_bits(z[k]) for k in z.files})
        heads = []
        for i, c in enumerate(meta["head_cases"]):
            d, z = dict(c), ld(f"head{i}_tokens")
            d["tokens"] = [bf16_of_bits(z[f"layer{k}"]) for k in range(4)]
            d["depth"], d["conf"] = torch.from_numpy(ld(f"head{i}_depth")["depth"]), torch.from_numpy(ld(f"head{i}_conf")["conf"])
            heads.append(d)
        chains = []
        for c in meta["chain_cases"]:
            d, i = dict(c), c["g26_case"]
            d["images"] = g26["cases"][i]["images"]
            d["depth"], d["conf"] = torch.from_numpy(ld(f"chain{i}_depth")["depth"]), torch.from_numpy(ld(f"chain{i}_conf")["conf"])
            chains.append(d)
        z = ld("pos")
        pos = [tuple(int(v) for v in z[f"pos{i}_shape"]) + (torch.from_numpy(z[f"pos{i}"]),) for i in range(len(z.files) // 2)]
        z = ld("resize")
        resize = [(torch.from_numpy(z[f"in{i}"])[0], torch.from_numpy(z[f"out{i}"])[0]) for i in range(len(RESIZE_CASES))]
        z = ld("units")
        config = dict(g26["config"], **meta["config"])
        _FIX = dict(config=config, chain_config=dict(config, depth_layers=meta["chain_depth_layers"]), sd=sd, head_cases=heads, chain_cases=chains,
                    pos=pos, resize=resize, units={k: torch.from_numpy(z[k]) for k in z.files})
    return _FIX


# ---- the head in float64, from its data flow -------------------------------------------------------------------------------------------------
def pos_embed(C, h, w, image_hw, dtype=F64, coord_dtype=F32):
    """[C, h, w] at `dtype`: the position embedding from its definition.  Channels 0 .. C/2 - 1 depend on the column, C/2 .. C - 1 on the row;
    per axis [sin(p w_k), cos(p w_k)], w_k = 100^(-k / (C / 4)), k < C / 4, angles in float64, rounded to fp32, then x 0.1 in fp32.  The
    coordinate p is a linspace over -+span (n - 1) / n AT THE MODULE'S DTYPE: fp32 in the module as released (coord_dtype = F32: what the
    host's tables hold, bit for bit), float64 in the float64 copy of the module that the fixtures' references were recorded from."""
    H, W = image_hw
    a = W / H
    span = (a / (a * a + 1.0) ** 0.5, 1.0 / (a * a + 1.0) ** 0.5)
    omega = 1.0 / 100 ** (torch.arange(C // 4, dtype=F64) / (C / 4))
    axes = []
    for n, s in ((w, span[0]), (h, span[1])):
        ang = torch.linspace(-s * (n - 1) / n, s * (n - 1) / n, n, dtype=coord_dtype).to(F64)[:, None] * omega[None, :]
        axes.append((torch.cat([ang.sin(), ang.cos()], 1).to(F32) * 0.1).to(dtype))          # [n, C / 2]
    return torch.cat([axes[0].t()[:, None, :].expand(C // 2, h, w), axes[1].t()[:, :, None].expand(C // 2, h, w)], 0)


def resize_ac(x, size):
    return Fn.interpolate(x, size=tuple(int(s) for s in size), mode="bilinear", align_corners=True)


def rcu(x, p, prefix, skip_is_input=False):
    """conv2(relu(conv1(relu(x)))) + relu(x): the head builds the unit with an IN-PLACE ReLU, so the skip connection sees relu(x).
    skip_is_input: the fault (the unit as it reads on paper, + x) that tests/test_vggt_depth_host.py must see."""
    r = torch.relu(x)
    t = Fn.conv2d(r, p[prefix + "conv1.weight"], p[prefix + "conv1.bias"], padding=1)
    t = Fn.conv2d(torch.relu(t), p[prefix + "conv2.weight"], p[prefix + "conv2.bias"], padding=1)
    return t + (x if skip_is_input else r)


def fusion(out, skip, p, prefix, size, **fault):
    if skip is not None:
        out = out + rcu(skip, p, prefix + "resConfUnit1.", **fault)
    out = rcu(out, p, prefix + "resConfUnit2.", **fault)
    return Fn.conv2d(resize_ac(out, size), p[prefix + "out_conv.weight"], p[prefix + "out_conv.bias"])


def head64(sd, tokens, image_hw, patch_start=5, prefix="depth_head.", dtype=F64, coord_dtype=F32):
    """tokens: the four kept layers [n, 5 + P, D] in head order -> (depth [n, H, W], conf [n, H, W]) at `dtype`; coord_dtype: pos_embed's."""
    p = {k[len(prefix):]: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    H, W = image_hw
    gh, gw = H // 14, W // 14
    maps = []
    for i, t in enumerate(tokens):
        x = t[:, patch_start:].to(dtype)
        n, P, D = x.shape
        x = Fn.layer_norm(x, (D,), p["norm.weight"], p["norm.bias"], 1e-5).transpose(1, 2).reshape(n, D, gh, gw)
        x = Fn.conv2d(x, p[f"projects.{i}.weight"], p[f"projects.{i}.bias"])
        x = x + pos_embed(x.shape[1], gh, gw, image_hw, dtype, coord_dtype)
        if i < 2:
            x = Fn.conv_transpose2d(x, p[f"resize_layers.{i}.weight"], p[f"resize_layers.{i}.bias"], stride=4 if i == 0 else 2)
        elif i == 3:
            x = Fn.conv2d(x, p["resize_layers.3.weight"], p["resize_layers.3.bias"], stride=2, padding=1)
        maps.append(Fn.conv2d(x, p[f"scratch.layer{i + 1}_rn.weight"], None, padding=1))
    l1, l2, l3, l4 = maps
    out = fusion(l4, None, p, "scratch.refinenet4.", l3.shape[2:])
    out = fusion(out, l3, p, "scratch.refinenet3.", l2.shape[2:])
    out = fusion(out, l2, p, "scratch.refinenet2.", l1.shape[2:])
    out = fusion(out, l1, p, "scratch.refinenet1.", (2 * l1.shape[2], 2 * l1.shape[3]))
    out = Fn.conv2d(out, p["scratch.output_conv1.weight"], p["scratch.output_conv1.bias"], padding=1)
    out = resize_ac(out, (14 * gh, 14 * gw))
    out = out + pos_embed(out.shape[1], 14 * gh, 14 * gw, image_hw, dtype, coord_dtype)
    out = torch.relu(Fn.conv2d(out, p["scratch.output_conv2.0.weight"], p["scratch.output_conv2.0.bias"], padding=1))
    out = Fn.conv2d(out, p["scratch.output_conv2.2.weight"], p["scratch.output_conv2.2.bias"])
    return torch.exp(out[:, 0]), 1 + torch.exp(out[:, 1])


# ---- wf_conv2d_f32 ------------------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = ((1, 1, 1, 4, 4, 1), (1, 1, 2, 32, 32, 2), (2, 5, 7, 36, 68, 1), (2, 5, 7, 36, 68, 2), (2, 11, 15, 128, 64, 2),
               (1, 44, 60, 64, 32, 1), (1, 9, 16, 8, 132, 1))   # (n, Hi, Wi, Cin, Cout, stride); the last: two channel tiles, the second ragged


def conv_inputs(n, Hi, Wi, Cin, Cout, stride, planted=False, seed=0):
    """x f32 [n, Hi, Wi, Cin] (channels-last), w f32 [Cout, Cin, 3, 3], bias f32 [Cout], resid f32 [n, Ho, Wo, Cout].  planted: x is zero
    except the four corner pixels and one interior pixel (negative values among them): padding or stride off by one moves them."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Hi + 13 * Wi + Cin + 3 * Cout + stride)
    x = torch.randn(n, Hi, Wi, Cin, generator=g)
    if planted:
        keep = torch.zeros(n, Hi, Wi, 1)
        for y, xx in ((0, 0), (0, Wi - 1), (Hi - 1, 0), (Hi - 1, Wi - 1), (Hi // 2, Wi // 2)):
            keep[:, y, xx] = 1.0
        x = x * keep
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    return x, w, 0.1 * torch.randn(Cout, generator=g), torch.randn(n, Ho, Wo, Cout, generator=g)


def conv_reference(x, w, bias, resid, stride, relu_in=False, relu_resid=False, relu_out=False, device="cpu"):
    """float64 on the kernel's fp32 inputs -> (ref, bar) channels-last [n, Ho, Wo, Cout] on the CPU."""
    xd, wd = x.to(device).to(F64).permute(0, 3, 1, 2), w.to(device).to(F64)
    if relu_in:
        xd = torch.relu(xd)
    ref = Fn.conv2d(xd, wd, None, stride=stride, padding=1)
    S = Fn.conv2d(xd.abs(), wd.abs(), None, stride=stride, padding=1)
    if bias is not None:
        b = bias.to(device).to(F64).view(1, -1, 1, 1)
        ref, S = ref + b, S + b.abs()
    if resid is not None:
        r = resid.to(device).to(F64).permute(0, 3, 1, 2)
        r = torch.relu(r) if relu_resid else r
        ref, S = ref + r, S + r.abs()
    if relu_out:
        ref = torch.relu(ref)
    bar = (9 * x.shape[3] + 4) * U * S + U * ref.abs()
    return ref.permute(0, 2, 3, 1).contiguous().cpu(), bar.permute(0, 2, 3, 1).contiguous().cpu()


def pack_conv_weight(w):
    """[Cout, Cin, 3, 3] -> the kernel's [3][3][Cout][Cin]."""
    return w.permute(2, 3, 0, 1).contiguous()
