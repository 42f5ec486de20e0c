"""GPU-free case tables, inputs, float64 references and per-element error bars for testing the LongCat DiT's non-GEMM kernels
(csrc/longcat_ops.hip: wf_lc_ln_modulate, wf_lc_norm_heads, wf_lc_swiglu, wf_lc_gate_residual, wf_lc_mean_pool_blocks, the block
scores of bsa.block_scores, wf_gather_rows_bf16 and the block selection wf_bsa_topk_lists / wf_bsa_cdf_lists) element by element.
tests/test_longcat_cases.py asserts on the references alone that every bar holds for the project's CPU restatement of the operation and
that every perturbed reference lies >= DISCRIM bars away, before a GPU sees a case; tests/test_gpu_longcat_kernels_fp64.py launches them
and carries the error models.  Every function here works on the device its inputs live on: the two grid-stride loop cases (33 M
elements each) are generated and referenced in float64 on the GPU, in row chunks; the CPU test runs the same functions on a few rows."""
import math

import numpy as np
import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
U_BF = 2.0 ** -8
C_ACC = 2.0 ** -22       # the GEMM accumulation model of tests/test_gpu_dit_kernels_fp64.py
DISCRIM = 8.0
SENT16 = 0x7FA5          # NaN bit pattern (bf16) of the guard cells of 16-bit outputs
SENT32 = 0x7FC0A5A5      # NaN bit pattern (fp32); as int32, the guard value of integer outputs too
EPS = 1e-6
LOG2E = 1.4426950408889634
PASS_CHUNKS = 8192 * 256  # 16-byte chunks one pass of a grid_for(n8, 256, 8192) launch covers


def _gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


def _randn(shape, seed, device="cpu"):
    return torch.randn(shape, generator=_gen(seed, device), device=device, dtype=F32)


def ratio(got, ref, bar):
    return ((got - ref).abs() / bar).max().item()


# ---- wf_lc_ln_modulate ---------------------------------------------------------------------------------------------------------------
LN_C = (8, 2048, 2056, 4096, 4104, 8192)          # both sides of k_lc_ln<1> / <2> / <4>, the smallest and the largest row
LN_L, LN_RPG, LN_ROW0, LN_OFFSET = 12, 4, 5, 12.0
LN_MODES = ("adaln", "gidx", "row0", "affine")


def ln_vpt(C):
    """wf_lc_ln_modulate's template choice: 16-byte chunks per thread."""
    return 1 if C <= 2048 else 2 if C <= 4096 else 4


def ln_inputs(C, mode):
    """One way the model calls wf_lc_ln_modulate.  x = rn_bf16(12 + N(0, 1)) (bf16 spacing 1 / 16: a one-pass variance loses digits).
    adaln / gidx / row0: a [T, 3C] fp32 table [shift | scale | unused], row stride 3C; affine: weight / bias vectors, plus_one = 0.
    `groups` [L] is the table row each token takes (what the kernel must derive from rows_per_group, row0 or the index)."""
    L = LN_L
    seed = 100 + 10 * LN_C.index(C) + LN_MODES.index(mode)
    x = (LN_OFFSET + _randn((L, C), seed)).to(BF)
    d = dict(x=x, L=L, C=C, mode=mode, rpg=0, row0=0, gidx=None, plus_one=1, mod_ld=3 * C)
    if mode == "affine":
        d.update(mul=1.0 + 0.3 * _randn((C,), seed + 1), add=0.3 * _randn((C,), seed + 2), plus_one=0, mod_ld=0,
                 groups=torch.zeros(L, dtype=torch.long), table=None)
        return d
    row0 = LN_ROW0 if mode == "row0" else 0
    T = (row0 + L - 1) // LN_RPG + 1
    table = 0.3 * _randn((T, 3 * C), seed + 1)
    if mode == "gidx":
        groups = (torch.arange(L) // LN_RPG)[torch.randperm(L, generator=_gen(seed + 3))]
        d.update(gidx=groups.to(torch.int32), rpg=LN_RPG)          # rows_per_group is ignored when an index is given
    else:
        groups = (row0 + torch.arange(L)) // LN_RPG
        d.update(rpg=LN_RPG, row0=row0)
    d.update(table=table, add=table[:, :C], mul=table[:, C:2 * C], groups=groups)
    return d


def ln_rows(d, which="own"):
    """(mul, add) float64 [L, C] per token: own, `swap` (shift and scale exchanged), `neighbour` (the next group's parameters)."""
    m, a = d["mul"].to(F64), d["add"].to(F64)
    if d["mode"] == "affine":
        m, a = m.expand(d["L"], -1), a.expand(d["L"], -1)
    else:
        g = d["groups"] if which != "neighbour" else (d["groups"] + 1) % d["table"].shape[0]
        m, a = m[g], a[g]
    return (a, m) if which == "swap" else (m, a)


def ln_ref(x64, m64, a64, plus_one, unbiased=False):
    """LayerNorm (biased variance, as F.layer_norm; `unbiased`: the perturbed form) * (plus_one + mul) + add, and the bar."""
    C = x64.shape[-1]
    mu = x64.mean(-1, keepdim=True)
    xc = x64 - mu
    var = (xc * xc).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt((var * C / (C - 1) if unbiased else var) + EPS)
    sc = plus_one + m64
    ref = xc * r * sc + a64
    vpt = ln_vpt(C)
    n_mu, n_var = 1 + 4 * vpt + 8, 8 * vpt + 8                       # fp32 adds a term passes through: see the GPU test's docstring
    dmu = n_mu * U * x64.abs().mean(-1, keepdim=True) + U * mu.abs()
    dr = ((n_var + 5) * U + dmu * dmu / var) / 2 + 2.0 ** -22
    pre = (r * sc).abs() * (dmu + U * xc.abs()) + (xc * r * sc).abs() * (dr + 3 * U) + U * ref.abs()
    return ref, pre + U_BF * (ref.abs() + pre) + 1e-30


# ---- wf_lc_norm_heads ----------------------------------------------------------------------------------------------------------------
HEADS_H = (1, 15, 16, 17, 32)                     # blockIdx.y covers 16 heads: one partly filled, one full, a second with one head
HEADS_GRID = (2, 2, 5)
HEADS_L = 2 * 2 * 5
HEADS_K0, HEADS_LOUT = 7, HEADS_L + 11
Q_SCALE = LOG2E / math.sqrt(128.0)


def rope_angles64(f, h, w, swap_hw=False):
    """rope_3d.py precompute_freqs_cis_3d in float64: of the 64 rotation pairs of a 128-channel head the first 22 turn with the frame
    index, the next 21 with the row, the last 21 with the column, pair i of an axis of n pairs at 10000^(-i / n): [f h w, 64]."""
    n_hw = 128 // 6
    n_t = 64 - 2 * n_hw

    def freqs(n):
        return 1.0 / torch.pow(torch.tensor(10000.0, dtype=F64), torch.arange(n, dtype=F64) / n)

    t, y, x = torch.meshgrid(torch.arange(f, dtype=F64), torch.arange(h, dtype=F64), torch.arange(w, dtype=F64), indexing="ij")
    t, y, x = t.reshape(-1, 1), y.reshape(-1, 1), x.reshape(-1, 1)
    if swap_hw:
        y, x = x, y
    return torch.cat([t * freqs(n_t), y * freqs(n_hw), x * freqs(n_hw)], dim=1)


def heads_inputs(H):
    """src bf16 [L, 3C] (the kernel reads the column block [C, 2C)), heads at scales 0.5 ... 2 as projected heads are; weight fp32 [128]
    with bf16 values (the reference's weight is a bf16 parameter)."""
    C = H * 128
    seed = 300 + H
    hs = (2.0 ** torch.linspace(-1.0, 1.0, H)).repeat_interleave(128) if H > 1 else torch.ones(C)
    src = (1.5 * _randn((HEADS_L, 3 * C), seed) * torch.cat([torch.ones(C), hs, torch.ones(C)])).to(BF)
    weight = (1.0 + 0.1 * _randn((128,), seed + 1)).to(BF).to(F32)
    return src, weight


def heads_ref(a64, w64, ang, s, variant=None):
    """float64 RMSNorm over each head's 128 channels * weight, interleaved RoPE (ang [L, 64] or None), * s -> (ref, bar) [H, L, 128].
    variant: "row_rms" (RMS over the whole row), "half_split" (pairs (p, p + 64) instead of (2p, 2p + 1))."""
    L, C = a64.shape
    H = C // 128
    ah = a64.view(L, H, 128)
    ms = (a64 * a64).mean(-1).view(L, 1, 1) if variant == "row_rms" else (ah * ah).mean(-1, keepdim=True)
    n = ah / torch.sqrt(ms + EPS) * w64
    if ang is None:
        cs, sn, e_t = torch.ones(L, 1, 64, dtype=F64), torch.zeros(L, 1, 64, dtype=F64), 0.0
    else:
        cs, sn = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]
        e_t = ang.abs().max().item() * 2.0 ** -20 + 2 * U           # the fp32 table: angle pos * fp32 pow, then cosf / sinf
    if variant == "half_split":
        n0, n1 = n[..., :64], n[..., 64:]
    else:
        n0, n1 = n.view(L, H, 64, 2)[..., 0], n.view(L, H, 64, 2)[..., 1]
    re, im = n0 * cs - n1 * sn, n0 * sn + n1 * cs
    P_re, P_im = (n0 * cs).abs() + (n1 * sn).abs(), (n0 * sn).abs() + (n1 * cs).abs()
    A = n0.abs() + n1.abs()

    def join(a, b):
        return (torch.cat([a, b], -1) if variant == "half_split" else torch.stack([a, b], -1).reshape(L, H, 128)).permute(1, 0, 2)

    ref, P, A = join(re, im) * s, join(P_re, P_im), join(A, A)
    e_r = 14 * U / 2 + 2.0 ** -22
    eta = 2.0 ** -7 + 2.0 ** -15 + e_r + 2 * U
    rot = s * ((eta + 5 * U) * (1 + eta) * P + e_t * (1 + eta) * A)
    return ref, rot + U_BF * (ref.abs() + rot) + 1e-30


# ---- wf_lc_swiglu --------------------------------------------------------------------------------------------------------------------
SWIGLU_CASES = {"small": (5, 8, 2 * 8 + 64), "loop": (3053, 11008, 22016)}          # L, Hd, ld


def swiglu_inputs(L, Hd, ld, device="cpu", seed=400):
    """buf bf16 [L, ld]: columns [0, Hd) = a, uniform over [-20, 20] (both tails of the sigmoid) with exact zeros sprinkled in,
    [Hd, 2 Hd) = b ~ 2 N(0, 1); whatever lies behind 2 Hd is NaN (never read)."""
    buf = torch.full((L, ld), float("nan"), dtype=BF, device=device)
    a = (torch.rand((L, Hd), generator=_gen(seed, device), device=device, dtype=F32) * 40.0 - 20.0)
    a[:, ::97] = 0.0
    buf[:, :Hd] = a.to(BF)
    buf[:, Hd:2 * Hd] = (2.0 * _randn((L, Hd), seed + 1, device)).to(BF)
    return buf


def swiglu_ref(a64, b64, variant=None):
    """silu(a) * b and the bar.  variant: "swap" (silu(b) * a), "gelu" (tanh-GELU(a) * b)."""
    if variant == "swap":
        a64, b64 = b64, a64
    if variant == "gelu":
        act = 0.5 * a64 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (a64 + 0.044715 * a64 ** 3)))
    else:
        act = a64 * torch.sigmoid(a64)
    ref = act * b64
    e_a = (a64.abs() * U + 2.0 ** -22) * torch.sigmoid(-a64) + 2.0 ** -22 + 2 * U
    rel = (1 + e_a) * (1 + U_BF) * (1 + U) * (1 + U_BF) - 1
    return ref, ref.abs() * rel + 1e-30


# ---- wf_lc_gate_residual -------------------------------------------------------------------------------------------------------------
GATE_CASES = {"small": (9, 8, 3), "loop": (8197, 4096, 7)}          # L, C, tokens per frame


def gate_inputs(L, C, tpf, device="cpu", seed=500):
    """x bf16 [L, C]; ybuf bf16 [L, 2C] (y = its columns [C, 2C), ldy = 2C); table fp32 [T, 2C] (gate = its columns [C, 2C)); a
    shuffled group index."""
    T = (L + tpf - 1) // tpf
    x = _randn((L, C), seed, device).to(BF)
    ybuf = _randn((L, 2 * C), seed + 1, device).to(BF)
    table = 0.25 + 0.5 * _randn((T, 2 * C), seed + 2, device)
    gidx = torch.randint(0, T, (L,), generator=_gen(seed + 3), dtype=torch.int32).to(device)
    return x, ybuf, table, gidx


def gate_ref(x64, y64, g64):
    """x + gate * y (gate None: x + y) and the bar: one fp32 product, one fp32 sum, one bf16 rounding."""
    gy = y64 if g64 is None else g64 * y64
    ref = x64 + gy
    pre = U * gy.abs() + U * ref.abs()
    return ref, pre + U_BF * (ref.abs() + pre) + 1e-30


# ---- wf_lc_mean_pool_blocks, bsa.block_scores ----------------------------------------------------------------------------------------
POOL_CASES = [(block, H, nb) for block in (64, 128) for H in (1, 3) for nb in (1, 13)]
POOL_DROP_ROW = 5
SCORE_CASES = [(13, 13), (5, 770)]
SCORE_HEADS, SCORE_KTAIL = 2, 32


def pool_inputs(block, H, nb):
    """bf16 [H, nb * block, 128]: head h sits at offset 1 + h / 2 (means away from zero) under a spread of 4."""
    seed = 600 + block + 10 * H + nb
    off = (1.0 + 0.5 * torch.arange(H, dtype=F32)).view(H, 1, 1)
    return (off + 4.0 * _randn((H, nb * block, 128), seed)).to(BF)


def pool_ref(x64, block, drop_row=None):
    """Mean of each block of rows (`drop_row`: that row of every block left out of the sum) and the bar: block / 16 + 16 fp32 adds."""
    H, L, D = x64.shape
    xb = x64.view(H, L // block, block, D)
    tot = xb.sum(2)
    if drop_row is not None:
        tot = tot - xb[:, :, drop_row]
    ref = tot / block
    e = (block // 16 + 16) * U * xb.abs().mean(2)
    return ref, e + U_BF * (ref.abs() + e) + 1e-30


def scores_inputs(nq, nk):
    seed = 700 + nq + nk
    return _randn((SCORE_HEADS, nq, 128), seed).to(BF), _randn((SCORE_HEADS, nk, 128), seed + 1).to(BF)


def scores_ref(q64, k64, tail=0):
    """Per head q k^T (`tail`: the last products of the 128 left out) and the bf16-output bar of the GEMM model."""
    z = torch.einsum("hqd,hkd->hqk", q64[..., :128 - tail], k64[..., :128 - tail])
    S = torch.einsum("hqd,hkd->hqk", q64.abs(), k64.abs())
    ev = C_ACC * S + U * (z.abs() + C_ACC * S)
    return z, ev + U_BF * (z.abs() + ev) + 1e-30


# ---- wf_gather_rows_bf16 -------------------------------------------------------------------------------------------------------------
GATHER_GRID, GATHER_CHUNK = (8, 8, 16), (4, 4, 8)


# ---- wf_bsa_topk_lists / wf_bsa_cdf_lists under ties ---------------------------------------------------------------------------------
SEL_NQ, SEL_HEADS = 7, 2
SIX_VALUES = (-2.0, -0.0, 0.0, 0.5, 0.50390625, 3.0)          # 0.5 and 0.50390625 are 0x3F00 / 0x3F01: one high key byte
SIX_PROBS = (0.20, 0.25, 0.25, 0.20, 0.05, 0.05)              # the 96th place falls among the 0.5s, the cdf counts among the zeros
# name: kind, n_k, n_sel, blocks per segment (None: one segment), seed
SEL_CASES = {
    "gauss_257_32": ("gauss", 257, 32, None, 11),
    "gauss_770_96": ("gauss", 770, 96, 385, 12),
    "gauss_1540_192": ("gauss", 1540, 192, None, 13),
    "gauss_2048_256": ("gauss", 2048, 256, 1024, 14),
    "six_770_96": ("six", 770, 96, None, 15),
}
SEL_EQUAL_ROW = (1, 3)                                          # (head, query block) of six_770_96 whose scores are all 0.5
SEL_MIN_TIE_SHARE = 0.10


def sel_scores(name):
    """bf16 [heads, n_q, n_k] block scores of a selection case."""
    kind, nk, nsel, bps, seed = SEL_CASES[name]
    if kind == "gauss":
        return (6.0 * _randn((SEL_HEADS, SEL_NQ, nk), seed)).to(BF)
    pick = torch.multinomial(torch.tensor(SIX_PROBS), SEL_HEADS * SEL_NQ * nk, replacement=True, generator=_gen(seed))
    sc = torch.tensor(SIX_VALUES, dtype=F32)[pick].view(SEL_HEADS, SEL_NQ, nk).to(BF)
    sc[SEL_EQUAL_ROW[0], SEL_EQUAL_ROW[1]] = 0.5
    return sc


def bf16_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def sort_key16(bits):
    """The kernel's documented 16-bit key of a bf16 score (bf16_sort_key): ascending in the sign-magnitude total order, -0 below +0."""
    b = bits.astype(np.int64)
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)


def topn_mask(bits, n):
    """bits uint16 [..., n_k], n an int or an array [...] -> bool mask of each row's first n blocks in (key descending, block ascending)."""
    key = sort_key16(bits)
    order = np.argsort(-key, axis=-1, kind="stable")                 # stable: equal keys stay in ascending block order
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(bits.shape[-1]), bits.shape), axis=-1)
    return rank < np.asarray(n)[..., None]


def tie_rows(bits, n):
    """bool [...]: rows whose n-th and (n + 1)-th best keys are equal (which block is taken is then decided by the tie rule)."""
    srt = -np.sort(-sort_key16(bits), axis=-1)
    n = np.broadcast_to(np.asarray(n), bits.shape[:-1])[..., None]
    inside = n < bits.shape[-1]
    a = np.take_along_axis(srt, np.minimum(n, bits.shape[-1] - 1), -1)
    b = np.take_along_axis(srt, np.maximum(n - 1, 0), -1)
    return ((a == b) & inside & (n > 0))[..., 0]


def group_lists_ref(mask, block, bps):
    """bool [heads, n_q, n_k] -> (lists: [head][group] int64 arrays, counts int [heads, groups]): per group of g = 256 / block query
    blocks the ascending union, entry = physical block * 2^g + flags, physical block = (b // bps) * heads * bps + head * bps + b % bps."""
    Hh, nq, nk = mask.shape
    gs = 256 // block
    ng = (nq + gs - 1) // gs
    lists, counts = [], np.zeros((Hh, ng), dtype=np.int64)
    for h in range(Hh):
        row = []
        for g in range(ng):
            flags = np.zeros(nk, dtype=np.int64)
            for r in range(gs):
                if g * gs + r < nq:
                    flags |= mask[h, g * gs + r].astype(np.int64) << r
            b = np.nonzero(flags)[0]
            phys = (b // bps) * (Hh * bps) + h * bps + b % bps
            row.append(phys * (1 << gs) + flags[b])
            counts[h, g] = len(b)
        lists.append(row)
    return lists, counts
