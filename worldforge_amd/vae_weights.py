"""The Wan2.1 VAE's architecture plans, constants and weights: state dict (twin or diffusers names) -> the matrix-core operands that
vae.AutoencoderKLWan's kernels read.  Host code on torch alone: nothing here loads the kernel library, everything runs on device="cpu"
(tests/test_vae_host.py)."""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch

DIM, Z_DIM = 96, 16
DIM_MULT = [1, 2, 4, 4]
NUM_RES = 2
T_DOWN = [False, True, True]
LATENTS_MEAN = [-0.7571, -0.7089, -0.9113, 0.1075, -0.1745, 0.9653, -0.1517, 1.5508, 0.4134, -0.0715, 0.5517, -0.3632,
                -0.1922, -0.9497, 0.2503, -0.2921]  # vae.py:629-632
LATENTS_STD = [2.8184, 1.4541, 2.3275, 2.6558, 1.2196, 1.7708, 2.6052, 2.0743, 3.2687, 2.1526, 2.8652, 1.5579, 1.6382,
               1.1253, 2.8251, 1.9160]  # vae.py:633-636

BF, F32 = torch.bfloat16, torch.float32


def encoder_plan() -> List[Tuple]:
    """vae.py:283-316."""
    dims = [DIM * u for u in [1] + DIM_MULT]
    plan = [("conv_in", "encoder.conv1", 3, dims[0])]
    idx = 0
    for i, (cin, cout) in enumerate(zip(dims[:-1], dims[1:])):
        for _ in range(NUM_RES):
            plan.append(("res", f"encoder.downsamples.{idx}", cin, cout))
            idx += 1
            cin = cout
        if i != len(DIM_MULT) - 1:
            plan.append(("down3d" if T_DOWN[i] else "down2d", f"encoder.downsamples.{idx}", cout, cout))
            idx += 1
    c = dims[-1]
    plan += [("res", "encoder.middle.0", c, c), ("attn", "encoder.middle.1", c, c), ("res", "encoder.middle.2", c, c),
             ("head", "encoder.head", c, 2 * Z_DIM)]
    return plan


def decoder_plan() -> List[Tuple]:
    """vae.py:387-421."""
    dims = [DIM * u for u in [DIM_MULT[-1]] + DIM_MULT[::-1]]
    t_up = T_DOWN[::-1]
    plan = [("conv_in", "decoder.conv1", Z_DIM, dims[0]), ("res", "decoder.middle.0", dims[0], dims[0]),
            ("attn", "decoder.middle.1", dims[0], dims[0]), ("res", "decoder.middle.2", dims[0], dims[0])]
    idx = 0
    for i, (cin, cout) in enumerate(zip(dims[:-1], dims[1:])):
        if i in (1, 2, 3):
            cin = cin // 2
        for _ in range(NUM_RES + 1):
            plan.append(("res", f"decoder.upsamples.{idx}", cin, cout))
            idx += 1
            cin = cout
        if i != len(DIM_MULT) - 1:
            plan.append(("up3d" if t_up[i] else "up2d", f"decoder.upsamples.{idx}", cout, cout // 2))
            idx += 1
    plan.append(("head", "decoder.head", dims[-1], 3))
    return plan


def first_up(plan: List[Tuple]) -> int:
    """Index of the decoder plan's first upsampling entry: everything before it is the latent-resolution stage (the only one with global
    spatial coupling, the mid-block attention), which always sees whole frames."""
    return next(i for i, e in enumerate(plan) if e[0] in ("up2d", "up3d"))


def diffusers_key_map() -> Dict[str, str]:
    """diffusers `AutoencoderKLWan` module name -> in-tree twin (`WanVAE_`) module name, for the Wan 2.1 configuration
    (is_residual=False).  The diffusers class is what the reference executes (INFER:185-189 `AutoencoderKLWan.from_pretrained`; a
    vendored copy is longcat_video/modules/autoencoder_kl_wan.py: encoder :505-584, decoder :783-872, mid block :430-451, up block
    :714-753, residual block :311-340, top level :1029-1052).  Leaves (.weight / .bias / .gamma) are appended by the caller."""
    m = {"encoder.conv_in": "encoder.conv1", "encoder.norm_out": "encoder.head.0", "encoder.conv_out": "encoder.head.2",
         "decoder.conv_in": "decoder.conv1", "decoder.norm_out": "decoder.head.0", "decoder.conv_out": "decoder.head.2",
         "quant_conv": "conv1", "post_quant_conv": "conv2"}
    res = {"norm1": "residual.0", "conv1": "residual.2", "norm2": "residual.3", "conv2": "residual.6", "conv_shortcut": "shortcut"}
    for side in ("encoder", "decoder"):
        for j, name in ((0, "resnets.0"), (1, "attentions.0"), (2, "resnets.1")):
            d, t = f"{side}.mid_block.{name}", f"{side}.middle.{j}"
            if j == 1:
                for leaf in ("norm", "to_qkv", "proj"):
                    m[f"{d}.{leaf}"] = f"{t}.{leaf}"
            else:
                for a, b in res.items():
                    m[f"{d}.{a}"] = f"{t}.{b}"
    # encoder: down_blocks is the same flat list as the twin's downsamples
    for kind, p, cin, cout in encoder_plan():
        if not p.startswith("encoder.downsamples."):
            continue
        d = p.replace("encoder.downsamples.", "encoder.down_blocks.")
        if kind == "res":
            for a, b in res.items():
                if a != "conv_shortcut" or cin != cout:
                    m[f"{d}.{a}"] = f"{p}.{b}"
        else:
            m[f"{d}.resample.1"] = f"{p}.resample.1"
            if kind.endswith("3d"):
                m[f"{d}.time_conv"] = f"{p}.time_conv"
    # decoder: up_blocks[i] = {resnets[0..2], upsamplers[0]} against the twin's flat upsamples list
    blk, j = 0, 0
    for kind, p, cin, cout in decoder_plan():
        if not p.startswith("decoder.upsamples."):
            continue
        if kind == "res":
            d = f"decoder.up_blocks.{blk}.resnets.{j}"
            for a, b in res.items():
                if a != "conv_shortcut" or cin != cout:
                    m[f"{d}.{a}"] = f"{p}.{b}"
            j += 1
            if j == NUM_RES + 1 and blk == len(DIM_MULT) - 1:
                blk, j = blk + 1, 0
        else:
            d = f"decoder.up_blocks.{blk}.upsamplers.0"
            m[f"{d}.resample.1"] = f"{p}.resample.1"
            if kind.endswith("3d"):
                m[f"{d}.time_conv"] = f"{p}.time_conv"
            blk, j = blk + 1, 0
    return m


def diffusers_to_twin_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Rename a diffusers-layout AutoencoderKLWan state dict to the twin's names (tensors are shared, shapes are the same up to the
    trailing singleton dims of the RMS-norm gammas, which the loader flattens).  Unknown or missing parameters raise KeyError."""
    km = diffusers_key_map()
    out = {}
    for k, v in sd.items():
        base, _, leaf = k.rpartition(".")
        if base not in km:
            raise KeyError(f"unmapped diffusers AutoencoderKLWan parameter {k!r}")
        out[f"{km[base]}.{leaf}"] = v
    return out


def weight_operand(w: torch.Tensor, precision: str, device):
    """f32 [..., Cin] weight (host) -> (the matrix-core weight operand of `precision` on `device`, acc_scale or None).  acc_scale (fp16
    operand modes only; None = 1): the operand is stored times 2^k and the kernels multiply their accumulators by 2^-k."""
    w = w.to(F32)
    if precision not in ("bf16x3", "fp16x3", "fp16"):
        return w.to(device=device, dtype=BF).contiguous(), None
    op = torch.float16 if precision in ("fp16x3", "fp16") else BF
    scale = None
    if op == torch.float16:
        # hi = fp16(w), lo = fp16(w - hi): lo is an fp16 SUBNORMAL (absolute floor 2^-25) for |w| < 2^-3 -- VAE weights are ~0.02, so the
        # split carried them to ~2^-18 relative, not the 2^-22 of its normal range.  Store the matrix times an exact
        # power of two that puts its largest magnitude into [2^13, 2^14) (every weight above 2^-17 of it then has a normal lo; fp16 tops
        # out at 2^16) and hand the kernels acc_scale = 2^-k: out = acc * 2^-k + bias, exact.
        mx = float(w.abs().max())
        if not math.isfinite(mx):
            raise ValueError("a VAE weight is not finite")
        if mx > 0.0:
            k = 13 - math.floor(math.log2(mx))
            k = max(-126, min(126, k))
            w = w * (2.0 ** k)
            scale = 2.0 ** -k
    hi = w.to(op)
    if precision == "fp16":   # the one-term operand (the scaled weight can no longer leave the fp16 range)
        return hi.to(device).contiguous(), scale
    lo = (w - hi.to(F32)).to(op)
    return torch.cat([hi, hi, lo], dim=-1).to(device).contiguous(), scale  # weight side of wf_split_bf16x3 / wf_split_f16x3


# ------------------------------------------------------------------------------------------------------------
# the packers: one layer's parameters of the state dict `sd` (keys as in WanVAE_.state_dict()) -> its entries of the weight dict.
# key + ".scale" (a Python float, fp16 operand modes only; absent = 1): acc_scale = 2^-k of a weight operand stored scaled by 2^k -- kept in
# the weight dict so that instances sharing `w` share it
# ------------------------------------------------------------------------------------------------------------
def _operand_entries(key, w, precision, device, bias=None):
    op, scale = weight_operand(w, precision, device)
    out = {key + ".w": op} if scale is None else {key + ".w": op, key + ".w.scale": scale}
    if bias is not None:
        out[key + ".b"] = bias.to(device=device, dtype=F32).contiguous()
    return out


def _zero_padded(sd, p, cin_pad=None, cout_pad=None):
    """(weight, bias) of layer p in f32 with Cin / Cout zero-padded."""
    w, b = sd[p + ".weight"].to(F32), sd[p + ".bias"].to(F32)
    co, ci = w.shape[:2]
    wp = torch.zeros((cout_pad or co, cin_pad or ci) + tuple(w.shape[2:]), dtype=F32)
    wp[:co, :ci] = w
    bp = torch.zeros(cout_pad or co, dtype=F32)
    bp[:co] = b
    return wp, bp


def mfma_conv(sd, p, precision, device):  # [Cout,Cin,kt,kh,kw] -> [Cout, taps, terms * Cin]
    w = sd[p + ".weight"]
    if w.dim() == 4:
        w = w.unsqueeze(2)
    co, ci = w.shape[:2]
    return _operand_entries(p, w.permute(0, 2, 3, 4, 1).reshape(co, -1, ci), precision, device, sd[p + ".bias"])


def mfma_conv_padded(sd, p, precision, device, cin_pad=None, cout_pad=None):
    """Thin layers on the MFMA path: zero-pad Cin to a 32-channel K slice / Cout to a multiple of 4 (the kernel
    computes a 96-wide tile anyway and only stores Cout columns)."""
    wp, bp = _zero_padded(sd, p, cin_pad, cout_pad)
    return _operand_entries(p, wp.permute(0, 2, 3, 4, 1).reshape(wp.shape[0], -1, wp.shape[1]), precision, device, bp)


def small_conv(sd, p, device, cout_pad=None):  # -> f32 [taps, Cin, Cout]
    wp, bp = _zero_padded(sd, p, cout_pad=cout_pad)
    return {p + ".w": wp.permute(2, 3, 4, 1, 0).reshape(-1, wp.shape[1], wp.shape[0]).to(device).contiguous(), p + ".b": bp.to(device)}


def lin(sd, p, precision, device):  # 1x1(x1) conv as GEMM weight [Cout, terms * Cin]
    w = sd[p + ".weight"]
    return _operand_entries(p, w.reshape(w.shape[0], w.shape[1]), precision, device, sd[p + ".bias"])


def gamma(sd, p, device):
    return {p: sd[p].reshape(-1).to(device=device, dtype=F32).contiguous()}


def up_phases(sd, p, precision, device):
    """Nearest-2x upsample + 3 x 3 conv (vae.py:76-86) as four 2 x 2 convolutions on the source grid: output (2y + py, 2x + px) reads
    source rows {y - 1 + py, y + py}; the 3 x 3 taps landing on the same source pixel are summed here, in fp32, before the operand
    split -- 4 / 9 of the multiply-adds, same result up to fp32 re-association."""
    w = sd[p + ".weight"].to(F32)
    if w.dim() == 5:
        w = w[:, :, 0]
    groups = (([0], [1, 2]), ([0, 1], [2]))  # [phase][source offset] -> the 3-tap indices that read it
    out = {}
    for py in range(2):
        for px in range(2):
            wp = torch.stack([torch.stack([sum(w[:, :, dy, dx] for dy in groups[py][a] for dx in groups[px][b]) for b in range(2)], dim=-1)
                              for a in range(2)], dim=-2)  # [Cout, Cin, 2, 2]
            out.update(_operand_entries(f"{p}.ph{py}{px}", wp.permute(0, 2, 3, 1).reshape(wp.shape[0], 4, wp.shape[1]), precision, device))
    return out


def pack_state_dict(sd: Dict[str, torch.Tensor], precision: str, device) -> Dict[str, torch.Tensor]:
    """Twin-layout state dict -> the weight dict of AutoencoderKLWan (`w`) for the operand format of `precision`, on `device`."""
    W: Dict[str, torch.Tensor] = {}
    seen_up = False
    for plan in (encoder_plan(), decoder_plan()):
        for kind, p, cin, cout in plan:
            if kind == "conv_in":
                W.update(mfma_conv_padded(sd, p, precision, device, cin_pad=32))
            elif kind == "res":
                W.update(gamma(sd, p + ".residual.0.gamma", device))
                W.update(mfma_conv(sd, p + ".residual.2", precision, device))
                W.update(gamma(sd, p + ".residual.3.gamma", device))
                W.update(mfma_conv(sd, p + ".residual.6", precision, device))
                if cin != cout:
                    W.update(lin(sd, p + ".shortcut", precision, device))
            elif kind == "attn":
                W.update(gamma(sd, p + ".norm.gamma", device))
                W.update(lin(sd, p + ".to_qkv", precision, device))
                W.update(lin(sd, p + ".proj", precision, device))
            elif kind in ("down2d", "down3d", "up2d", "up3d"):
                W.update(mfma_conv(sd, p + ".resample.1", precision, device))
                if kind.startswith("up"):
                    # every upsampling conv but the first (small, and its row slabs of the sharded decoder may start on an odd row) runs
                    # as four phase convolutions
                    if seen_up:
                        W.update(up_phases(sd, p + ".resample.1", precision, device))
                    seen_up = True
                if kind.endswith("3d"):
                    W.update(mfma_conv(sd, p + ".time_conv", precision, device))
            elif kind == "head":
                W.update(gamma(sd, p + ".0.gamma", device))
                # one 32-channel output block of the 3x3x3 kernel
                W.update(mfma_conv_padded(sd, p + ".2", precision, device, cout_pad=(cout + 31) // 32 * 32))
    W.update(small_conv(sd, "conv1", device))
    W.update(small_conv(sd, "conv2", device, cout_pad=32))  # decoder input, zero-padded to one 32-channel MFMA K slice
    return W


def random_state_dict(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Synthetic weights of the real shapes, generated on the host in twin layout (127 M parameters)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(p, cin, cout, k):
        sd[p + ".weight"] = torch.randn((cout, cin) + k, generator=g) / math.sqrt(cin * math.prod(k))
        sd[p + ".bias"] = 0.02 * torch.randn(cout, generator=g)

    for plan in (encoder_plan(), decoder_plan()):
        for kind, p, cin, cout in plan:
            if kind == "conv_in":
                conv(p, cin, cout, (3, 3, 3))
            elif kind == "res":
                sd[p + ".residual.0.gamma"] = 1 + 0.05 * torch.randn(cin, generator=g)
                conv(p + ".residual.2", cin, cout, (3, 3, 3))
                sd[p + ".residual.3.gamma"] = 1 + 0.05 * torch.randn(cout, generator=g)
                conv(p + ".residual.6", cout, cout, (3, 3, 3))
                if cin != cout:
                    conv(p + ".shortcut", cin, cout, (1, 1, 1))
            elif kind == "attn":
                sd[p + ".norm.gamma"] = 1 + 0.05 * torch.randn(cin, generator=g)
                conv(p + ".to_qkv", cin, 3 * cin, (1, 1))
                conv(p + ".proj", cin, cin, (1, 1))
            elif kind in ("down2d", "down3d"):
                conv(p + ".resample.1", cin, cin, (3, 3))
                if kind == "down3d":
                    conv(p + ".time_conv", cin, cin, (3, 1, 1))
            elif kind in ("up2d", "up3d"):
                conv(p + ".resample.1", cin, cin // 2, (3, 3))
                if kind == "up3d":
                    conv(p + ".time_conv", cin, cin * 2, (3, 1, 1))
            elif kind == "head":
                sd[p + ".0.gamma"] = 1 + 0.05 * torch.randn(cin, generator=g)
                conv(p + ".2", cin, cout, (3, 3, 3))
    conv("conv1", 2 * Z_DIM, 2 * Z_DIM, (1, 1, 1))
    conv("conv2", Z_DIM, Z_DIM, (1, 1, 1))
    return sd
