"""CPU: tests/longcat_cases.py -- before a GPU sees a case, the references alone show that it can be trusted: every float64 reference
lies within its bar of the project's own CPU restatement of the operation (oracle/longcat_dit.py layer_norm / modulate / rms_norm_head /
rope_apply, F.silu(a) * b in bf16, oracle/bsa.mean_pool; the ratio is printed), every perturbed reference lies >= DISCRIM bars away, the
selection inputs tie at the n_sel-th place as often as the real scores do, the selection rule agrees with torch.topk where nothing ties
and with a brute-force sort where everything does, and the two loop cases do need a third pass of their grid-stride loops."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import bsa as obsa
from oracle import longcat_dit as olc
from tests import longcat_cases as lc

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """The tensors here are small: a thread pool only adds its hand-over time to every one of the thousands of float64 operations."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _within(name, got, ref, bar):
    r = lc.ratio(got.to(F64), ref, bar)
    print(f"[cpu restatement] {name}: max |err| / bar = {r:.3f}")
    assert r <= 1.0, (name, r)


def _far(name, ref, other, bar):
    """A result within one bar of `ref` is then >= DISCRIM bars from `other`."""
    r = lc.ratio(other, ref, bar)
    assert r >= lc.DISCRIM + 1, f"{name}: the perturbed reference is only {r:.2f} bars away"


def test_tables_hold_what_the_kernels_switch_on():
    assert [lc.ln_vpt(C) for C in lc.LN_C] == [1, 1, 2, 2, 4, 4] and all(C % 8 == 0 for C in lc.LN_C)
    assert {(H + 15) // 16 for H in lc.HEADS_H} == {1, 2} and 16 in lc.HEADS_H and 15 in lc.HEADS_H and 17 in lc.HEADS_H
    assert lc.HEADS_L == 20 and lc.HEADS_K0 + lc.HEADS_L < lc.HEADS_LOUT
    assert len(lc.POOL_CASES) == 8 and lc.SCORE_CASES == [(13, 13), (5, 770)]
    assert {(c[1], c[2]) for c in lc.SEL_CASES.values() if c[0] == "gauss"} == {(257, 32), (770, 96), (1540, 192), (2048, 256)}
    assert {-(-c[1] // 256) for c in lc.SEL_CASES.values()} == {2, 4, 7, 8}          # key blocks a thread of k_bsa_topk_lists owns


def test_loop_cases_run_a_third_pass_that_wraps_inside_a_row():
    L, Hd, ld = lc.SWIGLU_CASES["loop"]
    n8 = L * (Hd // 8)
    assert n8 == 4_200_928 and n8 - 2 * lc.PASS_CHUNKS == 6_624 and lc.PASS_CHUNKS % (Hd // 8) != 0 and ld == 2 * Hd
    L, C, tpf = lc.GATE_CASES["loop"]
    n8 = L * (C // 8)
    assert n8 == 4_196_864 and n8 - 2 * lc.PASS_CHUNKS == 2_560
    assert (lc.PASS_CHUNKS // (C // 8)) % tpf != 0                                    # a pass ends inside a frame's group of rows
    assert lc.SWIGLU_CASES["small"] == (5, 8, 80) and lc.GATE_CASES["small"][:2] == (9, 8)


@pytest.mark.parametrize("mode", lc.LN_MODES)
@pytest.mark.parametrize("C", lc.LN_C)
def test_ln_reference(C, mode):
    d = lc.ln_inputs(C, mode)
    x64 = d["x"].to(F64)
    m64, a64 = lc.ln_rows(d)
    ref, bar = lc.ln_ref(x64, m64, a64, d["plus_one"])
    if mode == "affine":
        want = olc.layer_norm(d["x"], d["mul"], d["add"])
    elif mode == "adaln":
        want = olc.modulate(d["x"], d["add"], d["mul"], lc.LN_RPG)
    else:   # modulate()'s own lines with the rows' parameters gathered
        want = (olc.layer_norm(d["x"].float()) * (d["mul"][d["groups"]] + 1) + d["add"][d["groups"]]).to(BF)
    assert want.dtype == BF
    _within(f"ln C={C} {mode}", want, ref, bar)
    assert len(set(d["groups"].tolist())) >= (3 if mode != "affine" else 1)
    assert (x64.mean(-1) - lc.LN_OFFSET).abs().max().item() < 1.0 and 0.1 < x64.var(-1).min().item() < 4.0    # unit spread around the offset
    # discrimination
    _far("swap", ref, lc.ln_ref(x64, *lc.ln_rows(d, "swap"), d["plus_one"])[0], bar)
    if mode != "affine":
        _far("neighbour", ref, lc.ln_ref(x64, *lc.ln_rows(d, "neighbour"), d["plus_one"])[0], bar)
    unb = lc.ratio(lc.ln_ref(x64, m64, a64, d["plus_one"], unbiased=True)[0], ref, bar)
    if C == 8:
        assert abs(math.sqrt(7 / 8) - 1) > 0.06 and unb >= lc.DISCRIM + 1, unb
    # (at C >= 2048 the two variances differ by 1 / (2C) of the value, below a bf16 ulp: only C = 8 can tell them apart)


@pytest.mark.parametrize("scale", [1.0, lc.Q_SCALE], ids=["s1", "sq"])
@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("H", lc.HEADS_H)
def test_heads_reference(H, rope, scale):
    src, w = lc.heads_inputs(H)
    C = H * 128
    a = src[:, C:2 * C]
    ang = lc.rope_angles64(*lc.HEADS_GRID) if rope else None
    ref, bar = lc.heads_ref(a.to(F64), w.to(F64), ang, scale)
    want = olc.rms_norm_head(a.view(lc.HEADS_L, H, 128).permute(1, 0, 2), w.to(BF))
    assert want.dtype == BF
    want = want.float()          # rope_apply on fp32 leaves its result un-rounded: the kernel scales in front of its one rounding
    if rope:
        tab = olc.rope_angles(128, *lc.HEADS_GRID)
        assert (tab[:, 0::2].to(F64) - ang).abs().max().item() <= ang.max().item() * 2.0 ** -20          # the e_t term of the bar
        want = olc.rope_apply(want, tab)
    _within(f"heads H={H} rope={rope} s={scale:.3f}", (want * scale).to(BF), ref, bar)
    a64, w64 = a.to(F64), w.to(F64)
    if rope:
        _far("hw_swap", ref, lc.heads_ref(a64, w64, lc.rope_angles64(*lc.HEADS_GRID, swap_hw=True), scale)[0], bar)
        _far("half_split", ref, lc.heads_ref(a64, w64, ang, scale, "half_split")[0], bar)
    if H > 1:                    # one head: the row IS the head
        _far("row_rms", ref, lc.heads_ref(a64, w64, ang, scale, "row_rms")[0], bar)


@pytest.mark.parametrize("case", list(lc.SWIGLU_CASES))
def test_swiglu_reference(case):
    L, Hd, ld = lc.SWIGLU_CASES[case]
    L = min(L, 6)                # the loop case: a few rows of the same width (the reference is element-wise)
    buf = lc.swiglu_inputs(L, Hd, ld)
    a, b = buf[:, :Hd], buf[:, Hd:2 * Hd]
    assert Hd == 8 or (a.float().min() < -19 and a.float().max() > 19)          # both tails of the sigmoid
    ref, bar = lc.swiglu_ref(a.to(F64), b.to(F64))
    _within(f"swiglu {case}", Fn.silu(a) * b, ref, bar)
    _far("swap", ref, lc.swiglu_ref(a.to(F64), b.to(F64), "swap")[0], bar)
    _far("gelu", ref, lc.swiglu_ref(a.to(F64), b.to(F64), "gelu")[0], bar)


@pytest.mark.parametrize("case", list(lc.GATE_CASES))
def test_gate_residual_reference(case):
    L, C, tpf = lc.GATE_CASES[case]
    L = min(L, 5 * tpf + 1)
    x, ybuf, table, gidx = lc.gate_inputs(L, C, tpf)
    y, gate = ybuf[:, C:], table[:, C:]
    grp = torch.arange(L) // tpf
    for name, g in (("frames", gate[grp]), ("index", gate[gidx.long()]), ("nogate", None)):
        ref, bar = lc.gate_ref(x.to(F64), y.to(F64), None if g is None else g.to(F64))
        want = (x.float() + (y.float() if g is None else g * y.float())).to(BF)
        _within(f"gate_residual {case} {name}", want, ref, bar)
        if g is not None:
            _far("no gate", ref, lc.gate_ref(x.to(F64), y.to(F64), None)[0], bar)
    ref, bar = lc.gate_ref(x.to(F64), y.to(F64), gate[grp].to(F64))
    _far("neighbour frame", ref, lc.gate_ref(x.to(F64), y.to(F64), gate[(grp + 1) % table.shape[0]].to(F64))[0], bar)


@pytest.mark.parametrize("block,H,nb", lc.POOL_CASES)
def test_pool_reference(block, H, nb):
    x = lc.pool_inputs(block, H, nb)
    ref, bar = lc.pool_ref(x.to(F64), block)
    want = obsa.mean_pool(x, block)
    assert want.dtype == BF and ref.abs().min().item() > 0
    _within(f"mean_pool block={block} H={H} nb={nb}", want, ref, bar)
    _far("row dropped", ref, lc.pool_ref(x.to(F64), block, lc.POOL_DROP_ROW)[0], bar)


@pytest.mark.parametrize("nq,nk", lc.SCORE_CASES)
def test_scores_reference(nq, nk):
    q, k = lc.scores_inputs(nq, nk)
    ref, bar = lc.scores_ref(q.to(F64), k.to(F64))
    _within(f"block_scores {nq}x{nk}", torch.matmul(q, k.transpose(-1, -2)), ref, bar)
    _far("k tail", ref, lc.scores_ref(q.to(F64), k.to(F64), lc.SCORE_KTAIL)[0], bar)


# ---- the selection rule ---------------------------------------------------------------------------------------------------------------
def test_sort_key_is_the_sign_magnitude_total_order():
    vals = torch.tensor([-3.0, -0.5, -0.0, 0.0, 0.5, 0.50390625, 3.0], dtype=BF)
    key = lc.sort_key16(lc.bf16_bits(vals))
    assert (np.diff(key) > 0).all() and key.min() >= 0 and key.max() <= 0xFFFF
    assert key[4] >> 8 == key[5] >> 8 and key[4] != key[5]
    allbits = np.arange(0x10000, dtype=np.uint16)
    fin = allbits[(allbits & 0x7FFF) <= 0x7F80]                      # everything but NaN
    f = torch.from_numpy(fin.view(np.int16).copy()).view(BF).to(F64).numpy()
    o = np.argsort(lc.sort_key16(fin), kind="stable")
    assert (np.diff(f[o]) >= 0).all() and len(set(lc.sort_key16(fin).tolist())) == len(fin)


@pytest.mark.parametrize("name", list(lc.SEL_CASES))
def test_selection_inputs_tie_and_the_rule_is_a_top_n(name):
    kind, nk, nsel, bps, seed = lc.SEL_CASES[name]
    sc = lc.sel_scores(name)
    bits = lc.bf16_bits(sc)
    ties = lc.tie_rows(bits, nsel)
    share = ties.mean()
    print(f"[ties] {name}: {share:.2f} of the rows tie at place {nsel} of {nk}")
    assert share >= lc.SEL_MIN_TIE_SHARE
    if kind == "six":
        assert ties.all() and set(np.unique(bits).tolist()) == set(lc.bf16_bits(torch.tensor(lc.SIX_VALUES, dtype=BF)).tolist())
        h, q = lc.SEL_EQUAL_ROW
        assert len(set(bits[h, q].tolist())) == 1
    mask = lc.topn_mask(bits, nsel)
    assert (mask.sum(-1) == nsel).all()
    f = sc.to(F64).numpy()
    for h in range(lc.SEL_HEADS):
        for q in range(lc.SEL_NQ):
            # brute force: python's sort by (value descending with -0 < +0, block ascending)
            order = sorted(range(nk), key=lambda b: (-f[h, q, b], math.copysign(1.0, f[h, q, b]) < 0, b))
            assert set(order[:nsel]) == set(np.nonzero(mask[h, q])[0].tolist())
            if not ties[h, q]:   # nothing to decide: any top-k gives this set
                assert set(torch.topk(sc[h, q].float(), nsel)[1].tolist()) == set(order[:nsel])
    if kind == "six":
        assert mask[lc.SEL_EQUAL_ROW][:nsel].all()                   # the all-equal row takes blocks 0 .. n_sel - 1
    # per-row counts (the cdf entry): the same rule with n per row
    n_rows = np.arange(lc.SEL_HEADS * lc.SEL_NQ).reshape(lc.SEL_HEADS, lc.SEL_NQ) * 37 % (nk + 1)
    mv = lc.topn_mask(bits, n_rows)
    assert (mv.sum(-1) == n_rows).all() and lc.topn_mask(bits[0, 0], int(n_rows[0, 1])).sum() == n_rows[0, 1]


def test_group_lists_reference_equals_the_product_form():
    """group_lists_ref against worldforge_amd.bsa.group_lists (torch, CPU) on a tie-free selection, both block sizes, two segments."""
    from worldforge_amd import bsa
    nk, nsel = 48, 9
    g = torch.Generator().manual_seed(5)
    idx = torch.stack([torch.stack([torch.randperm(nk, generator=g)[:nsel] for _ in range(lc.SEL_NQ)]) for _ in range(lc.SEL_HEADS)])
    mask = np.zeros((lc.SEL_HEADS, lc.SEL_NQ, nk), dtype=bool)
    np.put_along_axis(mask, idx.numpy(), True, axis=-1)
    for block in (64, 128):
        for bps in (nk, nk // 2):
            want, wc, mx = bsa.group_lists(idx, nk, None, block, bps)
            lists, counts = lc.group_lists_ref(mask, block, bps)
            assert np.array_equal(counts, wc.numpy())
            for h in range(lc.SEL_HEADS):
                for gi, ent in enumerate(lists[h]):
                    assert np.array_equal(ent, want[h, gi, :len(ent)].numpy())
