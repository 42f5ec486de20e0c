"""GPU: the LongCat DiT's non-GEMM kernels (csrc/longcat_ops.hip) -- wf_lc_ln_modulate, wf_lc_norm_heads, wf_lc_swiglu,
wf_lc_gate_residual, wf_lc_mean_pool_blocks, the block scores (bsa.block_scores), wf_gather_rows_bf16 and the block selection
wf_bsa_topk_lists / wf_bsa_cdf_lists -- called one at a time through the C-ABI with the views, strides and offsets the model passes,
against float64 references of the same operation, element by element.  Cases, inputs, references and bars live in
tests/longcat_cases.py; tests/test_longcat_cases.py shows on the CPU that every bar holds for the project's own restatement of the
operation and that every perturbed reference below is >= DISCRIM + 1 bars from the true one.  Every output is a view inside a larger buffer of
NaN sentinels (integer outputs: the same bit pattern), which must come back bit-identical.  U = 2^-24 (fp32), 2^-8 = one bf16 rounding.

wf_lc_ln_modulate (k_lc_ln<VPT>, VPT = 1 / 2 / 4 chunks of 8 channels per thread for C <= 2048 / 4096 / 8192; two-pass statistics over
registers; x = rn_bf16(12 + N(0, 1))).  Mean: a value passes through one pair add, <= 4 VPT adds of the thread's sum, 6 wave levels and
2 adds of block_sum_4: n_mu = 1 + 4 VPT + 8 adds of positive terms, then one division: |d mu| <= n_mu U mean|x| + U |mu|.  The centred
value carries d mu + U |x - mu|.  Variance: the square (U), 8 VPT adds in the thread, 6 + 2 in block_sum_4, the division by C and the
add of eps: (n_var + 5) U with n_var = 8 VPT + 8, and the shifted mean adds d mu^2 (the first-order term cancels: sum (x - mu) = 0);
rsqrtf 2^-22:  |d r| / r <= ((n_var + 5) U + d mu^2 / var) / 2 + 2^-22.  y = (x - mu) r (p + mul) + add, p = plus_one, built without
contraction: three more roundings on the product, one on the sum; one bf16 rounding:
    pre = |r (p + mul)| (d mu + U |x - mu|) + |(x - mu) r (p + mul)| (d r + 3 U) + U |ref|,      bar = pre + 2^-8 (|ref| + pre).
Perturbed references: shift and scale exchanged, the next group's parameters, and at C = 8 the unbiased variance (sqrt(7 / 8): 6 %; at
C >= 2048 it is 1 / (2 C) of the value, below a bf16 ulp, so only C = 8 can assert it).

wf_lc_norm_heads (k_lc_heads: 16 lanes x 8 channels per (row, head)).  Sum of squares: 8 squares (U) and adds in the lane, 4 levels of
the 16-lane xor tree, the add of eps: 14 U on positive terms; rsqrtf 2^-22: e_r = 14 U / 2 + 2^-22.  y = rn_bf16(rn_bf16(x r) w): two bf16
roundings and two fp32 products: stored y = n (1 + h), |h| <= eta = 2^-7 + 2^-15 + e_r + 2 U, n = x r w in float64.  RoPE on the pairs
(2p, 2p + 1) in fp32 without contraction (two products, one sum) from the model's fp32 tables -- angle pos * freq with freq an fp32
pow and the product rounded (<= 2^-20 |angle| in all), cosf / sinf (2 U): e_t = 2^-20 max|angle| + 2 U per table entry (0 without
RoPE) --, the scale (U), one bf16 rounding.  With P = |n0 cos| + |n1 sin| (|n0 sin| + |n1 cos| for the odd channel), A = |n0| + |n1|:
    rot = s ((eta + 5 U)(1 + eta) P + e_t (1 + eta) A),      bar = rot + 2^-8 (|ref| + rot).
The angles of the reference are float64 from rope_3d.py's formula (longcat_cases.rope_angles64), not longcat_dit.rope_tables.  Perturbed
references: h and w positions exchanged, the RMS over the whole row (heads carry scales 0.5 ... 2), the pairing (p, p + 64).

wf_lc_swiglu (o = rn_bf16(rn_bf16(a / (1 + __expf(-a))) b)).  __expf is exp2(-a log2 e): the argument's rounding |a| U and v_exp_f32
2^-22 reach the quotient through e / (1 + e) = sigmoid(-a); the add U, the division 2^-22 + U:  e_a = (|a| U + 2^-22) sigmoid(-a) + 2^-22
+ 2 U.  Then a bf16 rounding, the fp32 product (U) and the output's bf16 rounding:  bar = |ref| ((1 + e_a)(1 + 2^-8)(1 + U)(1 + 2^-8) - 1).
Perturbed: silu(b) a; tanh-GELU(a) b.

wf_lc_gate_residual (o = rn_bf16(x + g y), product and sum separate fp32 operations):  pre = U |g y| + U |ref|, bar = pre + 2^-8 (|ref| +
pre).  Perturbed: the next frame's gate; no gate (and, for the NULL-gate run, the gate applied).  The loop cases of swiglu and
gate_residual need a third pass of the grid-stride loop (8192 workgroups x 256 threads cover 2 097 152 chunks); every element is
compared, so a chunk a later pass skipped, or wrote twice (the residual is read-modify-write), shows.  Their float64 references are
computed on the GPU by torch, in row chunks.

wf_lc_mean_pool_blocks: a column's sum is block / 16 adds in the thread and 16 adds over the row groups, the division by the power of
two is exact:  e = (block / 16 + 16) U mean|x|, bar = e + 2^-8 (|ref| + e).  Perturbed: one row of every block left out.
bsa.block_scores (wf_gemm_bf16_batched, K = 128, bf16 out): the GEMM model of tests/test_gpu_dit_kernels_fp64.py without a bias:
e_v = c S + U (|z| + c S), c = 2^-22, S = sum |q| |k|;  bar = e_v + 2^-8 (|z| + e_v).  Perturbed: the last 32 products left out.

Exact: wf_gather_rows_bf16 equals in[index] bit for bit; the selection kernels equal "sort by (16-bit key descending, block ascending),
take the first n" and its per-group union bit for bit, on inputs that tie at the n-th place as the real scores do (the cdf entry with
each row's n taken from the kernel's own row_counts, so the cdf rounding -- pinned by g14c -- stays out).  Every WF_CHECK_ARG line of
the six entry points refuses: non-zero status, wf_last_error names the entry, the guarded output is untouched.
The measured max(|err| / bar) of every float case goes through tests._tol.within."""
import numpy as np
import pytest
import torch

from tests import longcat_cases as lc
from tests._tol import within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
DISCRIM = lc.DISCRIM


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """The CPU-side references are small tensors: a thread pool only adds its hand-over time to each float64 operation."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


class Guarded:
    """A sentinel-filled buffer and the view of it a kernel may write (`pick`: buffer -> view)."""

    def __init__(self, shape, pick, dtype=BF):
        if dtype == BF:
            self.buf = torch.full(shape, lc.SENT16, dtype=torch.int16, device=DEV).view(BF)
        else:
            self.buf = torch.full(shape, lc.SENT32, dtype=torch.int32, device=DEV).view(dtype)
        self.pick = pick
        self.view = pick(self.buf)
        assert self.view.numel() < self.buf.numel() and self.view.data_ptr() != self.buf.data_ptr()
        self.snap = self.buf.clone()

    def fill(self, values):
        self.view.copy_(values)
        self.snap = self.buf.clone()

    def check(self, what):
        """Everything outside the view still holds the bits it held before the call."""
        torch.cuda.synchronize()
        c = self.buf.clone()
        self.pick(c).copy_(self.pick(self.snap))
        assert torch.equal(_bits(c), _bits(self.snap)), f"{what}: cells outside the output were written"

    def untouched(self, what):
        torch.cuda.synchronize()
        assert torch.equal(_bits(self.buf), _bits(self.snap)), f"{what}: a refused call wrote to its output"


def _call(name, *args):
    from worldforge_amd import _ffi, ops
    _ffi.call(name, *args, ops.stream())


def _discriminates(name, disc):
    print(f"[discrim] {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in disc.items()))
    for what, r in disc.items():
        assert r >= DISCRIM, f"{name}: reference with {what}: max err / bar = {r:.2f} < {DISCRIM}: the bar cannot see it"


# ---- float-valued kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", lc.LN_MODES)
@pytest.mark.parametrize("C", lc.LN_C)
def test_ln_modulate_vs_fp64(C, mode):
    d = lc.ln_inputs(C, mode)
    L = d["L"]
    x = d["x"].to(DEV)
    if mode == "affine":
        mul, add = d["mul"].to(DEV), d["add"].to(DEV)
    else:
        table = d["table"].to(DEV)
        add, mul = table[:, :C], table[:, C:2 * C]
        assert table.stride(0) == d["mod_ld"]
    gidx = d["gidx"].to(DEV) if d["gidx"] is not None else None
    g = Guarded((L + 6, C), lambda b: b[3:3 + L])
    _call("wf_lc_ln_modulate", x.data_ptr(), mul.data_ptr(), add.data_ptr(), d["mod_ld"], d["rpg"], d["row0"],
          gidx.data_ptr() if gidx is not None else None, d["plus_one"], g.view.data_ptr(), L, C, lc.EPS)
    g.check(f"ln_modulate C={C} {mode}")
    got = g.view.cpu().to(F64)
    assert torch.isfinite(got).all()
    x64 = d["x"].to(F64)
    ref, bar = lc.ln_ref(x64, *lc.ln_rows(d), d["plus_one"])
    within(f"lc_ln_modulate.C{C}.{mode}", lc.ratio(got, ref, bar), 1.0)
    disc = {"shift / scale swapped": lc.ratio(got, lc.ln_ref(x64, *lc.ln_rows(d, "swap"), d["plus_one"])[0], bar)}
    if mode != "affine":
        disc["the next group's parameters"] = lc.ratio(got, lc.ln_ref(x64, *lc.ln_rows(d, "neighbour"), d["plus_one"])[0], bar)
    if C == 8:
        disc["the unbiased variance"] = lc.ratio(got, lc.ln_ref(x64, *lc.ln_rows(d), d["plus_one"], unbiased=True)[0], bar)
    _discriminates(f"lc_ln_modulate.C{C}.{mode}", disc)


@pytest.mark.parametrize("scale", [1.0, lc.Q_SCALE], ids=["s1", "sq"])
@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("H", lc.HEADS_H)
def test_norm_heads_vs_fp64(H, rope, scale):
    from worldforge_amd.longcat_dit import rope_tables
    L, C, k0, lout = lc.HEADS_L, H * 128, lc.HEADS_K0, lc.HEADS_LOUT
    src, w = lc.heads_inputs(H)
    sd, wd = src.to(DEV), w.to(DEV)
    view = sd[:, C:2 * C]                                              # the K column block of a [L, 3C] qkv buffer
    cos, sin = (t.to(DEV) for t in rope_tables(128, *lc.HEADS_GRID))
    g = Guarded((H + 2, lout, 128), lambda b: b[1:H + 1, k0:k0 + L])   # rows [k0, k0 + L) of [H, lout, 128]
    _call("wf_lc_norm_heads", view.data_ptr(), sd.stride(0), wd.data_ptr(), cos.data_ptr() if rope else None,
          sin.data_ptr() if rope else None, g.view.data_ptr(), L, lout, H, lc.EPS, float(scale))
    name = f"lc_norm_heads.H{H}.{'rope' if rope else 'norope'}.{'s1' if scale == 1.0 else 'sq'}"
    g.check(name)
    got = g.view.cpu().to(F64)
    assert torch.isfinite(got).all()
    a64, w64 = src[:, C:2 * C].to(F64), w.to(F64)
    ang = lc.rope_angles64(*lc.HEADS_GRID) if rope else None
    ref, bar = lc.heads_ref(a64, w64, ang, scale)
    within(name, lc.ratio(got, ref, bar), 1.0)
    disc = {}
    if rope:
        disc["h and w swapped"] = lc.ratio(got, lc.heads_ref(a64, w64, lc.rope_angles64(*lc.HEADS_GRID, swap_hw=True), scale)[0], bar)
        disc["pairs (p, p + 64)"] = lc.ratio(got, lc.heads_ref(a64, w64, ang, scale, "half_split")[0], bar)
    if H > 1:
        disc["the RMS of the whole row"] = lc.ratio(got, lc.heads_ref(a64, w64, ang, scale, "row_rms")[0], bar)
    _discriminates(name, disc)


def _row_chunks(L, rows=512):
    return [(r0, min(r0 + rows, L)) for r0 in range(0, L, rows)]


@pytest.mark.parametrize("case", list(lc.SWIGLU_CASES))
def test_swiglu_vs_fp64(case):
    L, Hd, ld = lc.SWIGLU_CASES[case]
    dev = DEV if case == "loop" else "cpu"                             # where the inputs are made and the float64 reference runs
    buf = lc.swiglu_inputs(L, Hd, ld, dev)
    bd = buf.to(DEV)
    g = Guarded((L + 4, Hd), lambda b: b[2:2 + L])
    _call("wf_lc_swiglu", bd.data_ptr(), ld, g.view.data_ptr(), L, Hd)
    g.check(f"swiglu {case}")
    worst, disc = 0.0, {"the halves swapped": 0.0, "tanh-GELU": 0.0}
    for r0, r1 in _row_chunks(L):
        a64, b64 = buf[r0:r1, :Hd].to(F64), buf[r0:r1, Hd:2 * Hd].to(F64)
        got = g.view[r0:r1].to(dev).to(F64)
        assert torch.isfinite(got).all()
        ref, bar = lc.swiglu_ref(a64, b64)
        worst = max(worst, lc.ratio(got, ref, bar))
        disc["the halves swapped"] = max(disc["the halves swapped"], lc.ratio(got, lc.swiglu_ref(a64, b64, "swap")[0], bar))
        disc["tanh-GELU"] = max(disc["tanh-GELU"], lc.ratio(got, lc.swiglu_ref(a64, b64, "gelu")[0], bar))
    within(f"lc_swiglu.{case}", worst, 1.0)
    _discriminates(f"lc_swiglu.{case}", disc)


@pytest.mark.parametrize("case,form", [("small", "frames"), ("small", "index"), ("small", "nogate"), ("loop", "frames"), ("loop", "nogate")])
def test_gate_residual_vs_fp64(case, form):
    L, C, tpf = lc.GATE_CASES[case]
    dev = DEV if case == "loop" else "cpu"
    x, ybuf, table, gidx = lc.gate_inputs(L, C, tpf, dev)
    yd, td, gd = ybuf.to(DEV), table.to(DEV), gidx.to(DEV)
    g = Guarded((L + 16, C), lambda b: b[8:8 + L])                     # x: a row range of a guarded buffer
    g.fill(x.to(DEV))
    yv, gate = yd[:, C:], td[:, C:]                                    # column slices: ldy = gate_ld = 2C
    gated = form != "nogate"
    _call("wf_lc_gate_residual", g.view.data_ptr(), yv.data_ptr(), yd.stride(0), gate.data_ptr() if gated else None, td.stride(0),
          tpf if gated else 0, 0, gd.data_ptr() if form == "index" else None, L, C)
    g.check(f"gate_residual {case} {form}")
    T = table.shape[0]
    rows = torch.arange(L, device=dev)
    frame = rows // tpf
    own = gidx.long() if form == "index" else frame
    gate64 = table[:, C:].to(F64)
    worst, disc = 0.0, {}

    def note(what, r):
        disc[what] = max(disc.get(what, 0.0), r)

    for r0, r1 in _row_chunks(L):
        x64, y64 = x[r0:r1].to(F64), ybuf[r0:r1, C:].to(F64)
        got = g.view[r0:r1].to(dev).to(F64)
        assert torch.isfinite(got).all()
        ref, bar = lc.gate_ref(x64, y64, gate64[own[r0:r1]] if gated else None)
        worst = max(worst, lc.ratio(got, ref, bar))
        if gated:
            note("the gate dropped", lc.ratio(got, lc.gate_ref(x64, y64, None)[0], bar))
            note("the next group's gate", lc.ratio(got, lc.gate_ref(x64, y64, gate64[(own[r0:r1] + 1) % T])[0], bar))
        else:
            note("a gate applied", lc.ratio(got, lc.gate_ref(x64, y64, gate64[frame[r0:r1]])[0], bar))
    within(f"lc_gate_residual.{case}.{form}", worst, 1.0)
    _discriminates(f"lc_gate_residual.{case}.{form}", disc)


@pytest.mark.parametrize("block,H,nb", lc.POOL_CASES)
def test_mean_pool_vs_fp64(block, H, nb):
    from worldforge_amd import bsa
    x = lc.pool_inputs(block, H, nb)
    xd = x.to(DEV)
    g = Guarded((H * nb + 4, 128), lambda b: b[2:2 + H * nb])
    _call("wf_lc_mean_pool_blocks", xd.data_ptr(), g.view.data_ptr(), H, nb * block, block)
    g.check(f"mean_pool {block} {H} {nb}")
    assert torch.equal(_bits(bsa.mean_pool(xd, block)).view(-1), _bits(g.view).reshape(-1))          # the wrapper: the same call
    got = g.view.cpu().to(F64).view(H, nb, 128)
    ref, bar = lc.pool_ref(x.to(F64), block)
    name = f"lc_mean_pool.b{block}.H{H}.nb{nb}"
    within(name, lc.ratio(got, ref, bar), 1.0)
    _discriminates(name, {"one row left out": lc.ratio(got, lc.pool_ref(x.to(F64), block, lc.POOL_DROP_ROW)[0], bar)})


@pytest.mark.parametrize("nq,nk", lc.SCORE_CASES)
def test_block_scores_vs_fp64(nq, nk):
    from worldforge_amd import bsa
    q, k = lc.scores_inputs(nq, nk)
    sc = bsa.block_scores(q.to(DEV), k.to(DEV))
    torch.cuda.synchronize()
    assert sc.shape == (lc.SCORE_HEADS, nq, nk) and nk % 8 and sc._base is not None
    pad = sc._base[:, :, nk:]
    assert pad.shape[-1] == 8 - nk % 8 and (_bits(pad) == 0).all(), "the zero-padded key columns must score +0"
    got = sc.cpu().to(F64)
    ref, bar = lc.scores_ref(q.to(F64), k.to(F64))
    within(f"bsa_block_scores.{nq}x{nk}", lc.ratio(got, ref, bar), 1.0)
    _discriminates(f"bsa_block_scores.{nq}x{nk}",
                   {"the last 32 products left out": lc.ratio(got, lc.scores_ref(q.to(F64), k.to(F64), lc.SCORE_KTAIL)[0], bar)})


# ---- exact kernels -------------------------------------------------------------------------------------------------------------------
def _gather(src, ld_in, idx, out, ld_out, n, C):
    _call("wf_gather_rows_bf16", src.data_ptr(), ld_in, idx.data_ptr(), out.data_ptr(), ld_out, n, C)


def test_gather_rows_c8_with_repeats():
    gen = torch.Generator().manual_seed(21)
    src = torch.randn((37, 16), generator=gen).to(BF).to(DEV)          # rows of 8 channels, 16 apart
    idx = torch.randint(0, 37, (53,), generator=gen, dtype=torch.int32).to(DEV)
    g = Guarded((53 + 4, 24), lambda b: b[2:2 + 53, 8:16])             # ld_out = 24 > C
    _gather(src[:, :8], 16, idx, g.view, 24, 53, 8)
    g.check("gather C=8")
    assert torch.equal(_bits(g.view), _bits(src[:, :8][idx.long()]))


def test_gather_rows_block_permutation_round_trip():
    from worldforge_amd import bsa
    T, Hh, W = lc.GATHER_GRID
    L = T * Hh * W
    perm, pos = bsa.block_permutation(T, Hh, W, lc.GATHER_CHUNK, DEV)
    x = torch.randn((L, 64), generator=torch.Generator().manual_seed(22)).to(BF).to(DEV)
    g = Guarded((L + 4, 72), lambda b: b[2:2 + L, :64])
    _gather(x, 64, perm, g.view, 72, L, 64)
    g.check("gather perm")
    assert torch.equal(_bits(g.view), _bits(x[perm.long()]))
    back = Guarded((L + 4, 80), lambda b: b[2:2 + L, 8:72])
    _gather(g.view, 72, pos, back.view, 80, L, 64)                     # reads the strided view the first call wrote
    back.check("gather pos")
    assert torch.equal(_bits(back.view), _bits(x)), "permute and inverse permute must restore the rows"
    assert not torch.equal(_bits(g.view), _bits(x))


def test_gather_rows_fp32_rows_as_bf16_pairs():
    """The way out of the block order (longcat_dit.py forward_tokens, use_bsa): fp32 [L, 64] rows moved as 128 bf16 each, strides doubled."""
    from worldforge_amd import bsa
    T, Hh, W = lc.GATHER_GRID
    L = T * Hh * W
    perm, pos = bsa.block_permutation(T, Hh, W, lc.GATHER_CHUNK, DEV)
    yo = torch.randn((L, 64), generator=torch.Generator().manual_seed(23)).to(DEV)
    g = Guarded((L + 4, 68), lambda b: b[2:2 + L, :64], dtype=F32)
    _gather(yo, 2 * yo.stride(0), pos, g.view, 2 * g.view.stride(0), L, 2 * yo.shape[1])
    g.check("gather fp32")
    assert g.view.stride(0) == 68 and torch.equal(_bits(g.view), _bits(yo[pos.long()]))


SEL_THRESHOLDS = {"gauss": (0.6,), "six": (0.45, 0.7)}                 # six: the counts fall among the +0s / among the -0s


def _int_guard(n):
    return Guarded((n + 16,), lambda b: b[8:8 + n], dtype=torch.int32)


def _check_selection(name, bits, n, block, bps, mask, lists, counts, mx):
    """mask int32 [heads, n_q, words], lists int32 [heads, groups, mx], counts int32 [heads, groups] (all on the CPU) against the rule."""
    Hh, nq, nk = bits.shape
    want = lc.topn_mask(bits, n)
    got = ((mask.numpy().view(np.uint32)[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(Hh, nq, -1).astype(bool)
    assert not got[..., nk:].any(), f"{name}: mask bits behind the last key block are set"
    wrong = np.nonzero((got[..., :nk] != want).any(-1))
    assert wrong[0].size == 0, f"{name}: rows (head, query block) {list(zip(*wrong))[:8]} select other blocks than the rule"
    ref_lists, ref_counts = lc.group_lists_ref(want, block, bps)
    assert np.array_equal(counts.numpy(), ref_counts), f"{name}: counts"
    ln = lists.numpy()
    for h in range(Hh):
        for gi, ent in enumerate(ref_lists[h]):
            assert len(ent) <= mx and np.array_equal(ln[h, gi, :len(ent)], ent), f"{name}: list of head {h}, group {gi}"
            assert not ln[h, gi, len(ent):].any(), f"{name}: entries behind the count of head {h}, group {gi}"


@pytest.mark.parametrize("block", [64, 128])
@pytest.mark.parametrize("name", list(lc.SEL_CASES))
def test_topk_lists_ties_vs_rule(name, block):
    kind, nk, nsel, bps, seed = lc.SEL_CASES[name]
    bps = bps or nk
    sc = lc.sel_scores(name)
    bits = lc.bf16_bits(sc)
    share = lc.tie_rows(bits, nsel).mean()
    assert share >= lc.SEL_MIN_TIE_SHARE, share                        # (a property of the inputs; also asserted on the CPU)
    Hh, nq = lc.SEL_HEADS, lc.SEL_NQ
    ld = (nk + 7) // 8 * 8 + 8
    scb = torch.full((Hh, nq, ld), 3.0e38, dtype=BF, device=DEV)       # columns behind n_k would win every selection if they were read
    scb[:, :, :nk] = sc.to(DEV)
    gs = 256 // block
    ng, nw, mx = (nq + gs - 1) // gs, (nk + 31) // 32, min(gs * nsel, nk)
    gl, gc, gm = _int_guard(Hh * ng * mx), _int_guard(Hh * ng), _int_guard(Hh * nq * nw)
    _call("wf_bsa_topk_lists", scb.data_ptr(), ld, Hh, nq, nk, nsel, block, bps, gl.view.data_ptr(), gc.view.data_ptr(), mx, gm.view.data_ptr())
    for g, what in ((gl, "lists"), (gc, "counts"), (gm, "mask")):
        g.check(f"topk {name} {what}")
    print(f"[ties] {name}: {share:.2f} of the rows tie at place {nsel}")
    _check_selection(f"topk {name} block {block}", bits, nsel, block, bps, gm.view.cpu().view(Hh, nq, nw), gl.view.cpu().view(Hh, ng, mx),
                     gc.view.cpu().view(Hh, ng), mx)


@pytest.mark.parametrize("block", [64, 128])
@pytest.mark.parametrize("name", list(lc.SEL_CASES))
def test_cdf_lists_ties_vs_rule(name, block):
    kind, nk, nsel, bps, seed = lc.SEL_CASES[name]
    bps = bps or nk
    sc = lc.sel_scores(name)
    bits = lc.bf16_bits(sc)
    Hh, nq = lc.SEL_HEADS, lc.SEL_NQ
    ld = (nk + 7) // 8 * 8 + 8
    scb = torch.full((Hh, nq, ld), 3.0e38, dtype=BF, device=DEV)
    scb[:, :, :nk] = sc.to(DEV)
    gs = 256 // block
    ng, nw = (nq + gs - 1) // gs, (nk + 31) // 32
    for thr in SEL_THRESHOLDS[kind]:
        gl, gc, gm, gr = _int_guard(Hh * ng * nk), _int_guard(Hh * ng), _int_guard(Hh * nq * nw), _int_guard(Hh * nq)
        _call("wf_bsa_cdf_lists", scb.data_ptr(), ld, Hh, nq, nk, float(thr), nsel, block, bps, gl.view.data_ptr(), gc.view.data_ptr(), nk,
              gm.view.data_ptr(), gr.view.data_ptr())
        for g, what in ((gl, "lists"), (gc, "counts"), (gm, "mask"), (gr, "row counts")):
            g.check(f"cdf {name} {what}")
        n = gr.view.cpu().view(Hh, nq).numpy().astype(np.int64)        # the kernel's own counts: the cdf rounding is g14c's business
        assert (n >= nsel).all() and (n <= nk).all()
        ties = lc.tie_rows(bits, n)
        print(f"[ties] {name} cdf {thr}: counts {n.min()} .. {n.max()}, {ties.mean():.2f} of the rows tie at their count")
        if kind == "six":
            assert ties.any()
        _check_selection(f"cdf {name} thr {thr} block {block}", bits, n, block, bps, gm.view.cpu().view(Hh, nq, nw),
                         gl.view.cpu().view(Hh, ng, nk), gc.view.cpu().view(Hh, ng), nk)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _refusals():
    """(entry, [(message fragment, args)], guarded output): one call per WF_CHECK_ARG line, each breaking that line alone."""
    L, C, H, Hd = 12, 64, 2, 16
    x = torch.zeros((L, 2 * C), dtype=BF, device=DEV)
    f = torch.zeros((L, 4 * C), dtype=F32, device=DEV)
    idx = torch.zeros((L,), dtype=torch.int32, device=DEV)
    P = lambda t: t.data_ptr()          # noqa: E731

    g = Guarded((L + 4, C), lambda b: b[2:2 + L])
    o = P(g.view)
    yield "wf_lc_ln_modulate", g, [
        ("null pointer", (P(x), P(f), P(f), 4 * C, 4, 0, None, 1, None, L, C, lc.EPS)),
        ("<= 8192", (P(x), P(f), P(f), 4 * C, 4, 0, None, 1, o, L, 8200, lc.EPS)),
        ("row0 >= 0", (P(x), P(f), P(f), 4 * C, 4, -1, None, 1, o, L, C, lc.EPS)),
        ("alignment", (P(x), P(f), P(f), 4 * C, 4, 0, None, 1, o + 2, L, C, lc.EPS))]
    g = Guarded((L + 4, C), lambda b: b[2:2 + L])
    o = P(g.view)
    yield "wf_lc_gate_residual", g, [
        ("null pointer", (o, None, 2 * C, P(f), 4 * C, 4, 0, None, L, C)),
        ("ldy", (o, P(x), 2 * C + 4, P(f), 4 * C, 4, 0, None, L, C)),
        ("a gate needs", (o, P(x), 2 * C, P(f), 4 * C, 0, 0, None, L, C)),
        ("alignment", (o + 2, P(x), 2 * C, P(f), 4 * C, 4, 0, None, L, C))]
    src = torch.zeros((L, 3 * H * 128), dtype=BF, device=DEV)
    g = Guarded((H + 2, L + 4, 128), lambda b: b[1:H + 1, 2:2 + L])
    o = P(g.view)
    yield "wf_lc_norm_heads", g, [
        ("null pointer", (P(src), 3 * H * 128, None, P(f), P(f), o, L, L + 4, H, lc.EPS, 1.0)),
        ("Lout >= L", (P(src), 3 * H * 128, P(f), P(f), P(f), o, L, L - 1, H, lc.EPS, 1.0)),
        ("cos/sin", (P(src), 3 * H * 128, P(f), P(f), None, o, L, L + 4, H, lc.EPS, 1.0)),
        ("alignment", (P(src), 3 * H * 128, P(f), P(f), P(f), o + 2, L, L + 4, H, lc.EPS, 1.0))]
    g = Guarded((L + 4, Hd), lambda b: b[2:2 + L])
    o = P(g.view)
    yield "wf_lc_swiglu", g, [
        ("null pointer", (P(x), 2 * C, None, L, Hd)),
        ("ld >= 2 Hd", (P(x), 2 * Hd - 8, o, L, Hd)),
        ("alignment", (P(x) + 2, 2 * C, o, L, Hd))]
    xin = torch.zeros((H, 128, 128), dtype=BF, device=DEV)
    g = Guarded((H * 2 + 4, 128), lambda b: b[2:2 + 2 * H])
    o = P(g.view)
    yield "wf_lc_mean_pool_blocks", g, [
        ("null pointer", (None, o, H, 128, 64)),
        ("block must be", (P(xin), o, H, 128, 32)),
        ("whole", (P(xin), o, H, 72, 64))]
    g = Guarded((L + 4, C), lambda b: b[2:2 + L])
    o = P(g.view)
    yield "wf_gather_rows_bf16", g, [
        ("null pointer", (P(x), 2 * C, None, o, C, L, C)),
        ("multiples of 8", (P(x), 2 * C, P(idx), o, C, L, 12)),
        ("alignment", (P(x), 2 * C, P(idx), o + 2, C, L, C))]


def test_every_argument_check_refuses_and_leaves_the_output_alone():
    from worldforge_amd import _ffi, ops
    lib = _ffi.lib()
    n_lines = 0
    for entry, g, calls in _refusals():
        fn = getattr(lib, entry)
        for fragment, args in calls:
            rc = fn(*args, ops.stream())
            msg = lib.wf_last_error().decode(errors="replace")
            assert rc != 0, f"{entry}: a call breaking '{fragment}' was accepted"
            assert msg.startswith(entry) and fragment in msg, f"{entry}: wf_last_error says '{msg}', expected the '{fragment}' line"
            n_lines += 1
        g.untouched(entry)
    assert n_lines == 21
