"""GPU-free inputs, float64 references and per-element error bars for testing every entry point of csrc/attention.hip (wf_attn_fwd,
wf_attn_fwd_split, wf_attn_fwd_part + wf_attn_merge, wf_attn_cross2_fwd, wf_attn_bsa_fwd) element by element, and the table of cases: the
smallest shapes that reach the 5-slot LDS ring's wrap, the ragged last tile, the <1> / <0> kernel switch at Lkp > 1024, both bodies of the
pre-scaled form, splits without tiles, the two-window part launch with a hole, the merging last part launch with 11 earlier slots, the
(H + 7) / 8 * 8 grid with dummy workgroups and the 256-row query block.  tests/test_attn_cases.py asserts on the references alone that
every case is sharp enough -- each planted key, dropped from the reference, moves some output by more than (DISCRIM + 1) bars -- before a
GPU sees it; tests/test_gpu_attn_fp64.py launches them.

Inputs of a planted-key case: q = rn_bf16(gain * N(0,1)) (times ALPHA = 128^-1/2 log2(e) in the pre-scaled form, softmax_scale = 0), k, v =
rn_bf16(N(0,1)); the scores then spread by about `gain` in natural-log units (gain 3; 2 where a form must stay under the un-tracked body's
norm bound |q| |k| <= 50).  A planted pair (row r, key j) overwrites k_j = rn_bf16(q_r * T / (ALPHA |q_r|^2)): row r scores exactly T (exp2
units) on key j, far above the log-sum of its random scores, so key j carries row r.  A spike row has an anchor key in tile 0 (score
T_ANCHOR: its running max from the prologue on) and one late key SPIKE_FIRE / SPIKE_HOLD exp2 units above it: the kernel's deferred
rescale (fires when a row max grew by more than 8) must fire for the first and must not need to for the second.

Error model of one output element (read off attn_w4_body; U = 2^-24, ref = sum_j P_j v_j in float64, W = sum_j P_j |v_j|):
  * scores: bf16 x bf16 products are exact in fp32; the MFMA chain (8 steps of 16 products, started from 0 or, pre-scaled, from -m) and
    the one fma c s - c m round partial sums of size <= S = ALPHA sum_d |q_d k_d| (+ |m| <= S): |dt| <= 24 U S_row in exp2 units, S_row the
    row's largest S.  p = v_exp_f32(t) adds <= 2^-22 relative.  The SAME fp32 p feeds numerator and row sum, so these errors only perturb
    the weights: P'_j = P_j (1 + d_j) / sum_i P_i (1 + d_i), |d| <= eps_s = ln2 * 24 U S_row + 2^-22, which moves the output by <= 2 eps_s W.
    The reference max (first tile's, running, or deferred by < 2^8) cancels exactly: P and l use the same m.
  * P is rounded to bf16 (v_cvt_pk_bf16_f32, nearest even: <= 2^-8 relative) for the P.V MFMA only; the row sum l is taken over the
    UN-rounded fp32 p.  So the rounding does not cancel: it moves the output by <= 2^-8 sum_j P_j |v_j| = 2^-8 W.
  * fp32 accumulation of P.V (n / 16 MFMA steps), of l (32 in-lane adds per tile, one add per tile, one lane exchange), the rare rescale
    products, 1 / l (fp32 division: <= 2^-22 however it is formed), the product o * (1 / l), and for the split / part forms the flash
    combine (one exp2, one product and one add per slot): gamma = (n / 8 + 64) U + 2^-22 on W + |ref|, far more than the chains need.
  * the output is rounded to bf16 once: 2^-8 of the value.
      e = 2^-8 W + 2 eps_s W + gamma (W + |ref|),      bar = e + 2^-8 (|ref| + e)
  * accumulate (O += result): the old bf16 value is exact, the un-rounded result is added in fp32 (one rounding U) and the sum is rounded
    to bf16:  bar = e + U |old + ref| + 2^-8 (|old + ref| + e + U |old + ref|).
  * wf_attn_cross2_fwd: context 1's result is rounded to bf16 (its own bar), context 2's un-rounded result is added to it in the same way.
Both 2^-8 terms are worst cases of round-to-nearest, no statistics; a float32 simulation of this arithmetic (not the kernel) sits at 0.35 -
0.65 of the bar (tests/test_attn_cases.py asserts <= 1 for every case).

Exact key counts: K = 0, so every valid p is exactly 1 and l = kv_len exactly; V is the indicator v_j[d] = [d == j mod 128] inside a
window of <= 1024 keys, so out[r, d] * kv_len = count_d <= 8 up to one division and one bf16 rounding (count_bar).  K's pad rows stay
zero, so a wrongly included pad key gets p = 1; layouts() puts 64.0 into V^T's pad columns and 1e4 into whole tiles behind the last one."""
import math

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
LOG2E = 1.4426950408889634
SCALE = 128.0 ** -0.5
ALPHA = SCALE * LOG2E
U = 2.0 ** -24
U_BF = 2.0 ** -8
DISCRIM = 8.0
KB = 64
T_PLANT, T_ANCHOR, SPIKE_FIRE, SPIKE_HOLD = 28.0, 22.0, 10.0, 7.0
V_PAD, TILE_PAD, K_GARBAGE = 64.0, 1.0e4, 1.0e4

# name: entry point, H, Lq, kv (cross2: (kv1, kv2); bsa: key blocks), options.
#   pre: the pre-scaled-Q form (softmax_scale = 0); Lkp: padded key rows (default: kv rounded up to 64); segs: all-gathered segments;
#   forms: the launches the GPU test makes on the case's ONE set of inputs (names only: what each launch is stands next to the case)
CASES = {
    # wf_attn_fwd, scale > 0: k_attn_w4<1> (Lkp <= 1024) and <0> (Lkp > 1024)
    "fwd_k1": dict(entry="fwd", H=1, Lq=1, kv=1, forms=["plain"]),
    "fwd_k63": dict(entry="fwd", H=1, Lq=64, kv=63, forms=["plain", "acc"]),
    "fwd_k64_pre": dict(entry="fwd", H=3, Lq=1, kv=64, pre=True, forms=["plain"]),
    "fwd_k65": dict(entry="fwd", H=1, Lq=255, kv=65, forms=["plain"]),
    "fwd_k100_lkp256": dict(entry="fwd", H=3, Lq=65, kv=100, Lkp=256, forms=["plain"]),
    "fwd_k449_h9": dict(entry="fwd", H=9, Lq=300, kv=449, forms=["plain", "acc"]),
    "fwd_k1024": dict(entry="fwd", H=3, Lq=65, kv=1024, forms=["plain"]),
    "fwd_k1025": dict(entry="fwd", H=1, Lq=257, kv=1025, forms=["plain", "acc"]),
    # scale = 0 (k_attn_w4<4>): no bounds / bounds that select the un-tracked body / bounds too large (tracked again)
    "fwd_pre_k703": dict(entry="fwd", H=3, Lq=256, kv=703, pre=True, gain=2.0, forms=["plain", "untracked", "toolarge", "acc"]),
    # dense segments [P][H][seg][128] with P = 2 (and the same data in packed slots, kmax_stride > H) and P = 4
    "fwd_pre_seg2_k321": dict(entry="fwd", H=9, Lq=64, kv=321, Lkp=384, segs=2, pre=True, gain=2.0, forms=["plain", "untracked", "packed"]),
    "fwd_seg4_k2113": dict(entry="fwd", H=1, Lq=300, kv=2113, Lkp=2304, segs=4, forms=["plain"]),
    # wf_attn_fwd_split
    "split_k703_h9": dict(entry="split", H=9, Lq=64, kv=703, forms=["split2", "split3", "split8", "split3_acc"]),
    "split_pre_k320": dict(entry="split", H=3, Lq=257, kv=320, pre=True, gain=2.0, forms=["split8", "split8_untracked"]),   # nsplit > 5 tiles
    "split_k63_one_tile": dict(entry="split", H=1, Lq=65, kv=63, forms=["split2"]),                                        # writes O directly
    # wf_attn_fwd_part + wf_attn_merge: P = 3 segments of 6 tiles, 17 tiles (one key in the last), the own segment is 1
    "part_k1025_h9": dict(entry="part", H=9, Lq=65, kv=1025, Lkp=1152, segs=3, pre=True, gain=2.0,
                          forms=["part_one_window", "part_hole_inner3", "part_omerge", "part_12slots"]),
    # wf_attn_cross2_fwd: tile counts (5, 8) and (6, 11)
    "cross2_257_449_h9": dict(entry="cross2", H=9, Lq=300, kv=(257, 449), forms=["cross2"]),
    "cross2_321_703": dict(entry="cross2", H=3, Lq=257, kv=(321, 703), forms=["cross2"]),
    # wf_attn_bsa_fwd through bsa.sparse_attention: sel[i] = key blocks of query block i
    "bsa128_h9": dict(entry="bsa", H=9, Lq=512, kv=8, block=128, sel=[[0, 3, 7], list(range(8)), [2], [1, 2, 4, 5, 6]], forms=["bsa"]),
    "bsa64": dict(entry="bsa", H=3, Lq=320, kv=11, block=64, sel=[[10], list(range(11)), [0, 4, 5, 9], [3], [0, 1, 2, 3, 4, 5, 6, 7, 8, 10]],
                  forms=["bsa"]),
    "bsa64_seg2": dict(entry="bsa", H=1, Lq=256, kv=12, block=64, segs=2, sel=[[0, 5, 6, 11], list(range(12)), [6], [4, 5, 6, 7]], forms=["bsa"]),
}
REQUIRED_KV = (1, 63, 64, 65, 100, 257, 320, 321, 449, 703, 1024, 1025, 2113)
REQUIRED_LQ = (1, 64, 65, 255, 256, 257, 300)
REQUIRED_ROWS = (0, 63, 64, 255, 256)


def pad64(n):
    return (n + KB - 1) // KB * KB


def lkp_of(c):
    if c["entry"] == "bsa":
        return (c["kv"] + (0 if c.get("segs", 1) > 1 else 1)) * c["block"]   # one trailing garbage block where the layout allows it
    return c.get("Lkp", pad64(c["kv"]))


def split_bounds(ntiles, nsplit):
    """attn_launch's split of a sweep: [(first tile, end tile)] of the splits that get tiles."""
    tps = -(-ntiles // nsplit)
    return [(s * tps, min((s + 1) * tps, ntiles)) for s in range(-(-ntiles // tps))]


def part_steps(form, ntiles, tiles_per_seg):
    """The wf_attn_fwd_part launches of a form: dicts (t0, t1, t0b, t1b, inner, slot, merge) and the slot count."""
    s = tiles_per_seg
    if form == "part_one_window":          # two launches of one window each, separate merge
        return [dict(t0=0, t1=s, inner=1, slot=0), dict(t0=s, t1=ntiles, inner=1, slot=1)], 2, False
    if form == "part_hole_inner3":         # the own segment first, then both sides of the hole as ONE sequence in 3 inner splits
        return [dict(t0=s, t1=2 * s, inner=1, slot=0), dict(t0=0, t1=s, t0b=2 * s, t1b=3 * s, inner=3, slot=1)], 4, False
    if form == "part_omerge":              # the last launch folds slot 0 in and writes O
        return [dict(t0=s, t1=2 * s, inner=1, slot=0), dict(t0=0, t1=s, t0b=2 * s, t1b=3 * s, inner=1, slot=1, merge=True)], 2, True
    if form == "part_12slots":             # 11 one-tile launches and a merging last one: MAX_MERGE earlier slots
        return [dict(t0=i, t1=i + 1, inner=1, slot=i) for i in range(11)] + [dict(t0=11, t1=ntiles, inner=1, slot=11, merge=True)], 12, True
    raise KeyError(form)


def step_windows(st, ntiles):
    """Tile ranges one part launch's inner splits walk (the joined sequence cut into ceil(n / inner) pieces)."""
    tiles = list(range(st["t0"], min(st["t1"], ntiles))) + list(range(st.get("t0b", 0), min(st.get("t1b", 0), ntiles)))
    tps = -(-len(tiles) // st["inner"])
    return [tiles[i:i + tps] for i in range(0, len(tiles), tps)]


def boundary_keys(c):
    """Keys a case must plant: 0, kv - 1, first / last key of the tiles round the ring wrap, of every split, part window and segment."""
    kv = c["kv"]
    nt = -(-kv // KB)
    keys = {0, kv - 1}
    for t in (4, 5, 9, 10):
        keys.update((t * KB, t * KB + KB - 1))
    seg = lkp_of(c) // c.get("segs", 1)
    for s in range(c.get("segs", 1)):
        keys.update((s * seg, (s + 1) * seg - 1))
    for f in c["forms"]:
        if f.startswith("split"):
            for a, b in split_bounds(nt, int(f[5])):
                keys.update((a * KB, b * KB - 1))
        if f.startswith("part"):
            for st in part_steps(f, nt, seg // KB)[0]:
                for w in step_windows(st, nt):
                    runs = [w[0]] + [t for p, t in zip(w, w[1:]) if t != p + 1]          # first tile of every contiguous run
                    ends = [p for p, t in zip(w, w[1:]) if t != p + 1] + [w[-1]]
                    for a, b in zip(runs, ends):
                        keys.update((a * KB, b * KB + KB - 1))
    return sorted(j for j in keys if 0 <= j < kv)


def _rows_order(Lq, skip):
    req = [r for r in dict.fromkeys(REQUIRED_ROWS + (Lq - 1,)) if r < Lq]
    rest = [r for r in ((11 * i + 5) % Lq for i in range(Lq)) if r not in req and r not in skip]
    return req + list(dict.fromkeys(rest))


def plan_pairs(c):
    """-> (planted [(row, key, T)], spikes {"fire": (row, anchor key, spike key), "hold": ...})."""
    Lq, kv = c["Lq"], c["kv"]
    keys = boundary_keys(c)
    spikes = {}
    if Lq >= 40 and kv >= 129:
        rows = (37, 101) if Lq >= 128 else (37, 21)
        late = [kv * 3 // 4 + 2, kv // 2 + 3]
        for name, r, anchor, j in zip(("fire", "hold"), rows, (5, 9), late):
            while j in keys:
                j += 1
            spikes[name] = (r, anchor, j)
    rows = _rows_order(Lq, {s[0] for s in spikes.values()})
    n_req = len([r for r in dict.fromkeys(REQUIRED_ROWS + (Lq - 1,)) if r < Lq])
    taken = set(keys) | {x for s in spikes.values() for x in s[1:]}
    extra = [j for j in ((17 * i + 21) % kv for i in range(kv)) if j not in taken]
    keys = keys + extra[:max(0, min(n_req, kv) - len(keys))]          # every required row gets a key where kv allows
    pairs = [(rows[i % len(rows)], j, T_PLANT) for i, j in enumerate(sorted(keys))]
    for name, (r, anchor, j) in spikes.items():
        pairs += [(r, anchor, T_ANCHOR), (r, j, T_ANCHOR + (SPIKE_FIRE if name == "fire" else SPIKE_HOLD))]
    return pairs, spikes


def plan_pairs_bsa(c):
    """Block-sparse: per query block the first and the last key of its first and last selected block; the spike rows sit in the query
    block that selects every key block."""
    blk, pairs, spikes = c["block"], [], {}
    used = set()
    for qb, sel in enumerate(c["sel"]):
        ks = sorted({min(sel) * blk, min(sel) * blk + blk - 1, max(sel) * blk, max(sel) * blk + blk - 1})
        rows = [qb * blk, qb * blk + blk - 1, qb * blk + 63 % blk, qb * blk + 64 % blk]
        for i, j in enumerate(ks):
            while j in used:          # a key carries one row: take its neighbour inside the same block
                j += 1 if j % blk < blk // 2 else -1
            used.add(j)
            pairs.append((rows[i % len(rows)], j, T_PLANT))
    qb = [len(s) for s in c["sel"]].index(c["kv"])
    for name, r, anchor, j in (("fire", qb * blk + 37, 5, c["kv"] * blk * 3 // 4 + 2), ("hold", qb * blk + 21, 9, c["kv"] * blk // 2 + 3)):
        while j in used:
            j += 1
        used.update((anchor, j))
        spikes[name] = (r, anchor, j)
        pairs += [(r, anchor, T_ANCHOR), (r, j, T_ANCHOR + (SPIKE_FIRE if name == "fire" else SPIKE_HOLD))]
    return pairs, spikes


def key_mask(c):
    """bsa: [Lq, n keys] bool, True where the row's query block selected the key's block; None elsewhere."""
    if c["entry"] != "bsa":
        return None
    blk = c["block"]
    m = torch.zeros(c["Lq"] // blk, c["kv"], dtype=torch.bool)
    for qb, sel in enumerate(c["sel"]):
        m[qb, sel] = True
    return m.repeat_interleave(blk, 0).repeat_interleave(blk, 1)


def make_bar(W, ref, S_row, n):
    """Per-element bar of one un-accumulated attention output: (e, bar) with bar = e + 2^-8 (|ref| + e)."""
    eps_s = math.log(2.0) * 24 * U * S_row + 2.0 ** -22
    gamma = (n / 8 + 64) * U + 2.0 ** -22
    e = U_BF * W + 2 * eps_s * W + gamma * (W + ref.abs())
    return e, e + U_BF * (ref.abs() + e) + 1e-30


def bar_sum(e, total):
    """Bar of rn_bf16(old + result) (accumulate; cross2's second context): e bounds the un-rounded addend's error, one fp32 add, one rounding."""
    e2 = e + U * total.abs()
    return e2 + U_BF * (total.abs() + e2) + 1e-30


class Context:
    """One softmax over one key set: inputs as the kernel gets them, the float64 reference and everything the bar needs."""

    def __init__(self, c, seed, kv, pairs, mask=None, q=None):
        H, Lq, pre = c["H"], c["Lq"], bool(c.get("pre"))
        g = torch.Generator().manual_seed(seed)
        if q is None:
            q = (torch.randn(H, Lq, 128, generator=g) * c.get("gain", 3.0) * (ALPHA if pre else 1.0)).to(BF)
        k = torch.randn(H, kv, 128, generator=g).to(BF)
        v = torch.randn(H, kv, 128, generator=g).to(BF)
        qe = q.to(F64) / (ALPHA if pre else 1.0)          # the reference's Q: the very bf16 values, un-scaled in float64
        for r, j, T in pairs:
            k[:, j] = (qe[:, r] * (T / (ALPHA * qe[:, r].pow(2).sum(-1, keepdim=True)))).to(BF)
        self.q, self.k, self.v, self.kv, self.pairs, self.mask = q, k, v, kv, pairs, mask
        k64, v64 = k.to(F64), v.to(F64)
        t = torch.einsum("hqd,hkd->hqk", qe, k64) * ALPHA          # exp2 units
        s_abs = torch.einsum("hqd,hkd->hqk", qe.abs(), k64.abs()) * ALPHA
        if mask is not None:
            t = t.masked_fill(~mask, -math.inf)
            s_abs = s_abs.masked_fill(~mask, 0.0)
        self.t = t
        self.P = torch.softmax(t * math.log(2.0), -1)
        self.ref = self.P @ v64
        self.W = self.P @ v64.abs()
        self.S_row = s_abs.max(-1, keepdim=True).values
        self.n_eff = kv
        self.e, self.bar = make_bar(self.W, self.ref, self.S_row, kv)

    def drop_ref(self, r, j):
        """Row r of the reference with key j left out: [H, 128]."""
        t = self.t[:, r].clone()
        t[:, j] = -math.inf
        return (torch.softmax(t * math.log(2.0), -1).unsqueeze(1) @ self.v.to(F64))[:, 0]

    def drop_ratio(self, r, j, bar=None):
        """min over heads of max_d |ref without key j - ref| / bar on row r."""
        bar = self.bar if bar is None else bar
        return ((self.drop_ref(r, j) - self.ref[:, r]).abs() / bar[:, r]).amax(-1).min().item()


class Planted:
    def __init__(self, name):
        c = CASES[name]
        self.name, self.c = name, c
        seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
        if c["entry"] == "cross2":
            self.ctx, q = [], None
            for i, kv in enumerate(c["kv"]):
                pairs, spikes = plan_pairs(dict(c, kv=kv, forms=[], Lkp=pad64(kv)))
                self.ctx.append(Context(c, seed + i, kv, pairs, q=q))
                q = self.ctx[0].q
            a, b = self.ctx
            self.ref = a.ref + b.ref
            # context 1 is rounded to bf16 (its own bar), context 2 is added un-rounded, then ONE more rounding
            self.bar = bar_sum(a.bar + b.e, self.ref)
            self.spikes = spikes
        else:
            if c["entry"] == "bsa":
                pairs, self.spikes = plan_pairs_bsa(c)
                kv = c["kv"] * c["block"]
            else:
                pairs, self.spikes = plan_pairs(c)
                kv = c["kv"]
            self.ctx = [Context(c, seed, kv, pairs, key_mask(c))]
            self.ref, self.bar = self.ctx[0].ref, self.ctx[0].bar
        self.q = self.ctx[0].q
        g = torch.Generator().manual_seed(seed + 99)
        self.old = torch.randn(c["H"], c["Lq"], 128, generator=g).to(BF)          # what an accumulate run finds in O
        self.ref_acc = self.old.to(F64) + self.ref
        self.bar_acc = bar_sum(self.ctx[0].e, self.ref_acc) if len(self.ctx) == 1 else None

    def discrimination(self, acc=False):
        """[(context, row, key, ratio)]: how far (in bars) the reference without that planted key lies from the reference."""
        out = []
        for i, cx in enumerate(self.ctx):
            bar = self.bar_acc if acc else self.bar
            out += [(i, r, j, cx.drop_ratio(r, j, bar)) for r, j, T in cx.pairs if T != T_ANCHOR]          # an anchor only sets a row's early max
        return out


_CACHE = {}


def planted(name):
    if name not in _CACHE:
        _CACHE[name] = Planted(name)
    return _CACHE[name]


# ---- layouts ------------------------------------------------------------------------------------------------------------------------
def layouts(k, v, Lkp, segs=1, k_garbage=False):
    """k, v bf16 [H, n, 128] -> (K [H, Lkp, 128] or [P, H, seg, 128], V^T [H, Lkp / 64, 128, 64] or [P, H, seg / 64, 128, 64]) as the
    header states them, with everything it leaves free filled adversely: the pad keys of the last tile hold V_PAD in V^T (the kernel must
    mask p, not lean on zeros), whole tiles behind it hold TILE_PAD in K and V^T.  K's pad rows inside the last tile are zero (the
    header's contract) or, k_garbage, +-K_GARBAGE row by row (a launch must give the same bits either way)."""
    H, n, _ = k.shape
    nt = pad64(n)
    kp = torch.full((H, Lkp, 128), TILE_PAD, dtype=BF)
    vp = torch.full((H, Lkp, 128), TILE_PAD, dtype=BF)
    kp[:, :n], vp[:, :n] = k, v
    kp[:, n:nt] = 0.0
    if k_garbage:
        kp[:, n:nt] = (K_GARBAGE * (1 - 2 * (torch.arange(n, nt) % 2))).to(BF).view(1, -1, 1)
    vp[:, n:nt] = V_PAD
    vt = vp.view(H, Lkp // KB, KB, 128).transpose(2, 3).contiguous()
    if segs > 1:
        seg = Lkp // segs
        kp = kp.view(H, segs, seg, 128).transpose(0, 1).contiguous()
        vt = vt.view(H, segs, seg // KB, 128, KB).transpose(0, 1).contiguous()
    return kp, vt


def unlayout(kp, vt):
    """Inverse of layouts (tests): -> k, v [H, Lkp, 128]."""
    if kp.dim() == 4:
        P, H, seg, _ = kp.shape
        kp = kp.transpose(0, 1).reshape(H, P * seg, 128)
        vt = vt.transpose(0, 1).reshape(H, P * seg // KB, 128, KB)
    H, Lkp, _ = kp.shape
    return kp, vt.transpose(2, 3).reshape(H, Lkp, 128)


# ---- exact key counts ---------------------------------------------------------------------------------------------------------------
COUNT_WINDOW = 1024


def count_windows(n):
    return [(lo, min(lo + COUNT_WINDOW, n)) for lo in range(0, n, COUNT_WINDOW)]


def indicator_v(H, n, lo, hi):
    """v_j[d] = 1 iff d == j mod 128 for lo <= j < hi, else 0."""
    v = torch.zeros(H, n, 128, dtype=BF)
    j = torch.arange(lo, hi)
    v[:, j, j % 128] = 1.0
    return v


def expected_counts(n, lo, hi, mask=None):
    """-> (count [rows or 1, 128] float64, l [rows or 1, 1]): keys of the window per column and keys in all, per row of `mask` ([Lq, n])."""
    onehot = torch.zeros(n, 128, dtype=F64)
    j = torch.arange(lo, hi)
    onehot[j, j % 128] = 1.0
    m = torch.ones(1, n, dtype=F64) if mask is None else mask.to(F64)
    return m @ onehot, m.sum(-1, keepdim=True)


def count_bar(count):
    """|out * l - count| <= count (2^-8 + 2^-20): o = count and l are exact small integers in fp32 (p = 1 exactly, v in {0, 1}), 1 / l errs
    by <= 2^-22 however it is formed, the product by 2^-24, and the bf16 rounding by 2^-8; a column with count 0 is exactly 0."""
    return count * (U_BF + 2.0 ** -20)


def count_discrimination(n, lo, hi, v_pad=V_PAD):
    """min over the window's keys j (in units of the bar at column j mod 128) of |perturbed - ref| * l for the reference with j omitted,
    with j doubled, and -- one number -- with the pad key n included (its V^T column holds v_pad everywhere)."""
    count, l = expected_counts(n, lo, hi)
    count, l = count[0], float(l)
    j = torch.arange(lo, hi)
    cj, bj = count[j % 128], count_bar(count[j % 128])
    omit = ((cj - 1) * l / (l - 1) - cj).abs() / bj if n > 1 else torch.full_like(cj, math.inf)
    twice = ((cj + 1) * l / (l + 1) - cj).abs() / bj
    pad = (((count + v_pad) * l / (l + 1) - count).abs() / count_bar(count).clamp_min(1e-300)).max().item()
    return omit.min().item(), twice.min().item(), pad
