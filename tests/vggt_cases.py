"""GPU-free inputs, float64 references and per-element bars for the kernels of csrc/vit.hip, the reader of the VGGT fixtures
(tests/golden/g26_vggt_*, written by tools/make_vggt_golden.py) and a `write_folder` helper.

wf_vit_attn_fwd.  The kernel keeps its scores in exp2 units (one fp32 product acc * (scale log2 e)), streams the keys in 64-key tiles with
an online softmax (per tile o, l *= exp2(m - m'), p = exp2(s - m'), l += p un-rounded, P rounded once to bf16, PV on bf16 MFMA, fp32
accumulation) and rounds O = o / l once.  That is the structure tests/attn_cases.py models for the DiT kernels, so the bar is its make_bar
with n = L keys: with W = sum_j P_j |v_j| and S_row = max_j sum_d |q_d k_jd| scale log2 e,
    e = 2^-8 W + 2 eps_s W + gamma (W + |ref|),  eps_s = ln 2 * 24 U S_row + 2^-22,  gamma = (L / 8 + 64) U + 2^-22,  bar = e + 2^-8 (|ref| + e).
Planted in every (sequence, head): a row with q = 0 (uniform softmax over all L keys: a lost tile moves it), a row whose dominant key
(score T_PLANT above the rest) sits in the first tile and a row whose dominant key is the LAST key, so that the running maximum jumps in
the last, partial tile.  `online(case, fault)` restates the tile loop in float64 with one fault switched on, for tests/test_vggt_host.py.

wf_vit_qk_norm_rope.  fp32: the mean of 64 values (3 in-lane levels, 3 shuffles: <= 8 U amax|x| absolute), the centred values (1 U), the
variance of 64 non-negative terms (<= 10 U relative), + eps, rsqrtf (2^-22), halved by the root; two products and the affine: the normalised
value n = (x - mean) r carries |n| (12 U + 2^-22) + 9 U amax|x| r, y = n w + b adds 2 U (|n w| + |b|); the rotation two products and one
sum: e_out = |c| e_1 + |s| e_2 + 3 U (|y_1 c| + |y_2 s|).  One rounding (bf16 keeps 8 significant bits: unit roundoff 2^-8): bar = 2^-8 |ref| + e_out (1 + 2^-8).
wf_vit_patch_rows.  (x - m) / s in fp32 on fp32 constants: 2 U (|x| + m) / s, one rounding: bar = 2^-8 |ref| + 2 U (|x| + m) / s (1 + 2^-8).
"""
import json
import math
import os

import numpy as np
import torch

from tests.attn_cases import LOG2E, make_bar

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U, U_BF = 2.0 ** -24, 2.0 ** -8
D = 64
SCALE = 0.125
T_PLANT = 24.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ATTN_SHAPES = ((1, 1, 1), (2, 2, 31), (1, 2, 64), (3, 2, 65), (1, 2, 129), (2, 2, 782), (1, 2, 4122))   # (nseq, H, L)
SAMPLED = (1, 16, 1374)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---- wf_vit_attn_fwd ------------------------------------------------------------------------------------------------------------------------
def planted_rows(L):
    """{name: (row, dominant key or None)}; rows coincide for the smallest L (then the later entry wins)."""
    if L == 1:
        return {"last": (0, 0)}
    if L == 2:
        return {"zero": (1, None), "last": (0, 1)}
    return {"zero": (L // 2, None), "first": (0, min(3, L - 2)), "last": (L - 1, L - 1)}


class AttnCase:
    def __init__(self, nseq, H, L, rows=None, device="cpu"):
        """rows: the query rows (inside each sequence) the reference is computed for (None = all); device: where the float64 reference
        is evaluated (the GPU tests hand over the device: torch float64 there is the same arithmetic, only faster)."""
        self.nseq, self.H, self.L, self.device = nseq, H, L, device
        g = torch.Generator().manual_seed(100000 * nseq + 1000 * H + L)
        qkv = torch.randn(nseq, L, 3, H, D, generator=g).to(BF)
        self.plan = planted_rows(L)
        for name, (r, j) in self.plan.items():
            if j is None:
                qkv[:, r, 0] = 0.0
            else:
                q = qkv[:, r, 0].to(F64)                                                   # [nseq, H, 64]
                qkv[:, j, 1] = (q * (T_PLANT / SCALE / q.pow(2).sum(-1, keepdim=True))).to(BF)
        self.qkv = qkv.reshape(nseq * L, 3 * H * D).contiguous()
        self.rows = torch.arange(L) if rows is None else torch.as_tensor(sorted(set(int(r) for r in rows) | {r for r, _ in self.plan.values()}))
        self.ref, self.W, self.S_row = self.reference()
        self.e, self.bar = make_bar(self.W, self.ref, self.S_row, L)

    def _qkv(self):
        x = self.qkv.view(self.nseq, self.L, 3, self.H, D).to(self.device).to(F64)
        return x[:, self.rows.to(self.device), 0], x[:, :, 1], x[:, :, 2]

    def reference(self):
        """float64 on the kernel's own bf16 inputs -> ref, W [nseq, rows, H, 64], S_row [nseq, rows, H, 1] in exp2 units."""
        q, k, v = self._qkv()
        ref, W, S = [], [], []
        for h in range(self.H):                                                            # head by head: the scores of one head at a time
            s = torch.einsum("nrd,njd->nrj", q[:, :, h], k[:, :, h]) * SCALE
            S.append((torch.einsum("nrd,njd->nrj", q[:, :, h].abs(), k[:, :, h].abs()) * SCALE).amax(-1, keepdim=True) * LOG2E)
            P = torch.softmax(s, -1)
            ref.append(torch.einsum("nrj,njd->nrd", P, v[:, :, h]))
            W.append(torch.einsum("nrj,njd->nrd", P, v[:, :, h].abs()))
        return torch.stack(ref, 2).cpu(), torch.stack(W, 2).cpu(), torch.stack(S, 2).cpu()

    def online(self, fault=None):
        """The kernel's tile loop in float64 (no rounding anywhere) on self.rows -> [nseq, rows, H, 64].  fault: None (equals the
        reference), "drop_last" (the last, partial tile is never visited) or "skip_rescale" (o and l keep their old unit when the
        running maximum moves in the last tile)."""
        q, k, v = self._qkv()
        L, nt = self.L, (self.L + 63) // 64
        m = torch.full(q.shape[:-1] + (1,), -math.inf, dtype=F64, device=q.device)        # [nseq, rows, H, 1]
        l, o = torch.zeros_like(m), torch.zeros_like(q)
        for t in range(nt):
            if fault == "drop_last" and t == nt - 1 and L % 64 and nt > 1:
                break
            kt, vt = k[:, 64 * t:64 * t + 64], v[:, 64 * t:64 * t + 64]
            s = torch.einsum("nrhd,njhd->nrhj", q, kt) * SCALE
            mn = torch.maximum(m, s.amax(-1, keepdim=True))
            alpha = torch.exp(m - mn)
            if fault == "skip_rescale" and t == nt - 1 and nt > 1:
                alpha = torch.ones_like(alpha)
            p = torch.exp(s - mn)
            l = l * alpha + p.sum(-1, keepdim=True)
            o = o * alpha + torch.einsum("nrhj,njhd->nrhd", p, vt)
            m = mn
        return (o / l).cpu()


# ---- wf_vit_qk_norm_rope ---------------------------------------------------------------------------------------------------------------------
def rope_apply(y, cs, sn, pos, pairing=16, special_shift=0):
    """float64: y [rows, H, 64], cs / sn [max_pos + 1, 16], pos [rows, 2] -> rotated.  pairing 16 is the reference's rotate-half inside
    each 32-channel half; pairing 1 (interleaved neighbours) and special_shift (positions moved by one: position 0 becomes a rotation)
    are the faults tests/test_vggt_host.py must see."""
    out = y.clone()
    p = (pos.long() + special_shift).clamp(0, cs.shape[0] - 1)
    for hf in range(2):
        c, s = cs.to(F64)[p[:, hf]][:, None, :], sn.to(F64)[p[:, hf]][:, None, :]          # [rows, 1, 16]
        blk = y[..., 32 * hf:32 * hf + 32]
        if pairing == 16:
            x1, x2 = blk[..., :16], blk[..., 16:]
            out[..., 32 * hf:32 * hf + 16], out[..., 32 * hf + 16:32 * hf + 32] = x1 * c - x2 * s, x2 * c + x1 * s
        else:
            x1, x2 = blk[..., 0::2], blk[..., 1::2]
            out[..., 32 * hf:32 * hf + 32:2], out[..., 32 * hf + 1:32 * hf + 32:2] = x1 * c - x2 * s, x2 * c + x1 * s
    return out


def norm_rope_reference(x, w, b, eps, cs, sn, pos, **fault):
    """x [rows, H, 64] (the bf16 values in float64), w / b [64] or None -> (ref, e_out): the float64 result and the fp32 error model of
    the docstring."""
    amax = x.abs().amax(-1, keepdim=True)
    if w is not None:
        mean = x.mean(-1, keepdim=True)
        r = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
        n = (x - mean) * r
        y = n * w.to(F64) + b.to(F64)
        e_y = w.to(F64).abs() * (n.abs() * (12 * U + 2.0 ** -22) + 9 * U * amax * r) + 2 * U * ((n * w.to(F64)).abs() + b.to(F64).abs())
    else:
        y, e_y = x, torch.zeros_like(x)
    if cs is None:
        return y, e_y
    ref = rope_apply(y, cs, sn, pos, **fault)
    p = pos.long().clamp(0, cs.shape[0] - 1)
    e = torch.zeros_like(y)
    for hf in range(2):
        c, s = cs.to(F64)[p[:, hf]][:, None, :].abs(), sn.to(F64)[p[:, hf]][:, None, :].abs()
        y1, y2 = y[..., 32 * hf:32 * hf + 16].abs(), y[..., 32 * hf + 16:32 * hf + 32].abs()
        e1, e2 = e_y[..., 32 * hf:32 * hf + 16], e_y[..., 32 * hf + 16:32 * hf + 32]
        e[..., 32 * hf:32 * hf + 16] = c * e1 + s * e2 + 3 * U * (y1 * c + y2 * s)
        e[..., 32 * hf + 16:32 * hf + 32] = c * e2 + s * e1 + 3 * U * (y2 * c + y1 * s)
    return ref, e


def norm_rope_bar(ref, e):
    return U_BF * ref.abs() + e * (1 + U_BF) + 1e-30


class NormRopeCase:
    """nseq sequences of 5 special tokens + a gh x gw grid, H heads: the stacked bf16 buffer, norm parameters, tables, positions."""

    def __init__(self, nseq, H, gh, gw, norm=True, rope=True, seed=0):
        from worldforge_amd import vggt
        self.nseq, self.H, self.L = nseq, H, 5 + gh * gw
        g = torch.Generator().manual_seed(seed + 17 * gh + gw)
        self.qkv = (torch.randn(nseq * self.L, 3 * H * D, generator=g) * 2.0 + 0.3).to(BF)
        mk = lambda base: (base + 0.2 * torch.randn(D, generator=g)).to(F32)  # noqa: E731
        self.qw, self.qb, self.kw, self.kb = (mk(1.0), mk(0.0), mk(1.0), mk(0.0)) if norm else (None,) * 4
        self.max_pos = max(gh, gw)
        self.cs, self.sn = vggt.rope_tables(self.max_pos, 100.0) if rope else (None, None)
        self.pos = vggt.token_positions(gh, gw, 5) if rope else None
        self.eps = 1e-5

    def reference(self, **fault):
        """-> (ref_q, bar_q, ref_k, bar_k) [nseq * L, H, 64] float64."""
        x = self.qkv.view(self.nseq * self.L, 3, self.H, D).to(F64)
        pos = None if self.pos is None else self.pos.repeat(self.nseq, 1)
        out = []
        for i, (w, b) in enumerate(((self.qw, self.qb), (self.kw, self.kb))):
            ref, e = norm_rope_reference(x[:, i], w, b, self.eps, self.cs, self.sn, pos, **fault)
            out += [ref, norm_rope_bar(ref, e)]
        return out


# ---- wf_vit_patch_rows ------------------------------------------------------------------------------------------------------------------------
def patch_rows_reference(img):
    """img fp32 [n, 3, H, W] -> (ref, bar) float64 [n (H/14) (W/14), 592]."""
    n, _, H, W = img.shape
    m = torch.tensor(MEAN, dtype=F32).to(F64).view(1, 3, 1, 1)
    s = torch.tensor(STD, dtype=F32).to(F64).view(1, 3, 1, 1)
    x = img.to(F64)
    y, e = (x - m) / s, 2 * U * (x.abs() + m) / s
    rows = lambda t: t.reshape(n, 3, H // 14, 14, W // 14, 14).permute(0, 2, 4, 1, 3, 5).reshape(-1, 588)  # noqa: E731
    ref, err = torch.zeros(n * (H // 14) * (W // 14), 592, dtype=F64), torch.zeros(n * (H // 14) * (W // 14), 592, dtype=F64)
    ref[:, :588], err[:, :588] = rows(y), rows(e)
    return ref, U_BF * ref.abs() + err * (1 + U_BF)


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------------
def bf16_of_bits(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(BF)


_FIX = None


def fixture():
    """{config, sd (bf16 tensors under the reference's key names), cases [{S, H, W, images fp32 [1, S, 3, H, W], tokens [float64 per layer],
    pose64, pose_chain, pose_head32, extrinsic, intrinsic, rel_bf16, rel_f32, pose_rel_chain, pose_rel_head32}], released, rope, preprocess}."""
    global _FIX
    if _FIX is None:
        with open(os.path.join(GOLDEN, "g26_vggt_meta.json")) as f:
            meta = json.load(f)
        sd = {}
        for i in range(meta["weight_files"]):
            z = np.load(os.path.join(GOLDEN, f"g26_vggt_weights{i}.npz"))
            sd.update({k[3:]: bf16_of_bits(z[k]) for k in z.files})
        cases = []
        for i, c in enumerate(meta["cases"]):
            z = np.load(os.path.join(GOLDEN, f"g26_vggt_case{i}.npz"))
            d = dict(c)
            d["images"] = torch.from_numpy(z["images"]).to(F32).div(255).unsqueeze(0)
            d["tokens"] = [torch.from_numpy(np.load(os.path.join(GOLDEN, f"g26_vggt_case{i}_layer{k}.npz"))["tokens"])
                           for k in range(meta["config"]["depth"])]
            for k in ("pose64", "pose_chain", "pose_head32", "extrinsic", "intrinsic"):
                d[k] = torch.from_numpy(z[k])
            cases.append(d)
        _FIX = dict(config=meta["config"], sd=sd, cases=cases, released={k: tuple(v) for k, v in meta["released"].items()},
                    rope=dict(np.load(os.path.join(GOLDEN, "g26_vggt_rope.npz"))), preprocess=dict(np.load(os.path.join(GOLDEN, "g26_vggt_preprocess.npz"))))
    return _FIX


def write_folder(path, sd=None, config=None, extra=None, drop=(), reshape=None):
    """A synthetic checkpoint folder (config.json + model.safetensors) from the fixture's state dict; `extra` tensors are added, `drop`
    keys removed, `reshape` {key: shape} stored under another shape."""
    from safetensors.torch import save_file
    fx = fixture()
    sd = dict(fx["sd"] if sd is None else sd)
    sd.update(extra or {})
    for k in drop:
        sd.pop(k)
    for k, s in (reshape or {}).items():
        sd[k] = sd[k].reshape(s)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(fx["config"] if config is None else config, f)
    save_file({k: v.contiguous().clone() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))
    return path
