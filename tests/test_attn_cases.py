"""CPU: tests/attn_cases.py -- the table reaches what it must, and the references alone prove every case sharp enough for an
element-by-element GPU test of csrc/attention.hip: dropping any planted key (or a spike) from the float64 reference moves some output of its row by more than
DISCRIM + 1 bars (so an output within one bar of the reference is >= DISCRIM bars from the perturbed one), the spike rows do force / do
not force the deferred rescale, the un-tracked forms stay under the kernel's norm bound, and a float32 simulation of the kernel's
arithmetic (NOT the kernel) stays inside the bar."""
import math

import pytest
import torch

from tests import attn_cases as ac

F64, BF = torch.float64, torch.bfloat16
NAMES = list(ac.CASES)


def _sweeps(c):
    """Tile counts of the sweeps single workgroups walk."""
    if c["entry"] == "cross2":
        return [sum(-(-n // 64) for n in c["kv"])]
    if c["entry"] == "bsa":
        g, tpe = 256 // c["block"], c["block"] // 64
        return [len(set().union(*c["sel"][i:i + g])) * tpe for i in range(0, len(c["sel"]), g)]
    nt = -(-c["kv"] // 64)
    out = []
    for f in c["forms"]:
        if f.startswith("split"):
            out += [b - a for a, b in ac.split_bounds(nt, int(f[5]))]
        elif f.startswith("part"):
            for st in ac.part_steps(f, nt, ac.lkp_of(c) // c["segs"] // 64)[0]:
                out += [len(w) for w in ac.step_windows(st, nt)]
        else:
            out.append(nt)
    return out


def test_table_reaches_every_required_shape():
    kvs = {n for c in ac.CASES.values() if c["entry"] != "bsa" for n in (c["kv"] if isinstance(c["kv"], tuple) else (c["kv"],))}
    assert set(ac.REQUIRED_KV) <= kvs
    assert set(ac.REQUIRED_LQ) <= {c["Lq"] for c in ac.CASES.values()}
    assert {c["H"] for c in ac.CASES.values()} == {1, 3, 9}
    assert ac.lkp_of(ac.CASES["fwd_k100_lkp256"]) == 256
    assert ac.lkp_of(ac.CASES["fwd_k1024"]) == 1024 and ac.lkp_of(ac.CASES["fwd_k1025"]) > 1024          # the <1> / <0> switch
    for entry in ("fwd", "split", "part", "cross2", "bsa"):
        cs = [c for c in ac.CASES.values() if c["entry"] == entry]
        assert any(c["H"] == 9 for c in cs), entry
        assert any(((n - 1) // 5) % 2 == 1 for c in cs for n in _sweeps(c)), entry          # a sweep that wraps the 5-slot ring an odd number of times
        # block-sparse keys are whole blocks, there is no ragged tile: wf_attn_bsa_fwd's argument check rejects Lkp % block != 0 ("Lq and Lkp
        # must be whole %d-token blocks", WF_EINVAL) and sets kv_len = Lkp, and bsa.sparse_attention derives Lkp from k's shape
        if entry != "bsa":
            assert any(n % 64 for c in cs for n in (c["kv"] if isinstance(c["kv"], tuple) else (c["kv"],))), entry
    forms = {f for c in ac.CASES.values() for f in c["forms"]}
    assert {"plain", "acc", "untracked", "toolarge", "packed", "split2", "split3", "split8", "part_one_window", "part_hole_inner3",
            "part_omerge", "part_12slots", "cross2", "bsa"} <= forms
    assert {c.get("segs", 1) for c in ac.CASES.values() if c["entry"] == "fwd"} >= {1, 2, 4}
    sp = ac.CASES["split_pre_k320"]
    assert len(ac.split_bounds(-(-sp["kv"] // 64), 8)) < 8          # nsplit above the tile count: splits without tiles
    assert len(ac.split_bounds(1, 2)) == 1                           # one tile: the launch writes O itself
    b64 = ac.CASES["bsa64"]
    assert {len(s) for s in b64["sel"]} >= {1, b64["kv"]} and {c["block"] for c in ac.CASES.values() if c["entry"] == "bsa"} == {64, 128}


@pytest.mark.parametrize("name", NAMES)
def test_planted_pairs_cover_the_boundaries(name):
    c = ac.CASES[name]
    p = ac.planted(name)
    for i, cx in enumerate(p.ctx):
        keys, rows = {j for r, j, T in cx.pairs}, {r for r, j, T in cx.pairs}
        assert len(keys) == len(cx.pairs), "a key carries one row"
        if c["entry"] == "bsa":
            blk = c["block"]
            firsts = {(min(s) * blk, max(s) * blk + blk - 1) for s in c["sel"]}
            assert all(a in keys and b in keys for a, b in firsts)
            want_rows = {r for r in ac.REQUIRED_ROWS + (c["Lq"] - 1,) if r < c["Lq"]}
        else:
            cc = dict(c, kv=cx.kv, forms=c["forms"] if len(p.ctx) == 1 else [], Lkp=ac.lkp_of(c) if len(p.ctx) == 1 else ac.pad64(cx.kv))
            assert set(ac.boundary_keys(cc)) <= keys
            want_rows = {r for r in ac.REQUIRED_ROWS + (c["Lq"] - 1,) if r < c["Lq"]} if cx.kv >= 6 else {0}
        assert want_rows <= rows, (want_rows - rows)


@pytest.mark.parametrize("name", NAMES)
def test_references_discriminate_every_planted_key(name):
    c = ac.CASES[name]
    p = ac.planted(name)
    modes = [False] + ([True] if any(f.endswith("acc") for f in c["forms"]) else [])
    for acc in modes:
        for ctx, r, j, ratio in p.discrimination(acc):
            if p.ctx[ctx].kv == 1:
                continue          # the only key cannot be left out
            assert ratio >= ac.DISCRIM + 1, (name, acc, ctx, r, j, ratio)


@pytest.mark.parametrize("name", NAMES)
def test_spike_rows_force_and_spare_the_deferred_rescale(name):
    c = ac.CASES[name]
    p = ac.planted(name)
    cx = p.ctx[-1]
    if c["Lq"] >= 40 and cx.kv >= 129:
        assert set(p.spikes) == {"fire", "hold"}
    for kind, (r, anchor, j) in p.spikes.items():
        t = cx.t[:, r]
        t0 = j // 64 * 64
        earlier = t[:, :t0].amax(-1)
        # the anchor is the row's maximum over tile 0 (what the prologue commits) and over every key before the spike's tile
        assert torch.equal(earlier, t[:, anchor]) and anchor < 64 <= t0
        rise = t[:, j] - earlier
        if kind == "fire":
            assert rise.min().item() >= 9.0, rise          # >= 2^9: past the kernel's threshold of 8
        else:
            assert 6.0 <= rise.min().item() and rise.max().item() <= 7.75, rise          # about 2^7: under it
        assert (t[:, j] >= t.amax(-1) - 1e-9).all()          # and it then carries the row


@pytest.mark.parametrize("name", [n for n in NAMES if any("untracked" in f for f in ac.CASES[n]["forms"])])
def test_untracked_forms_stay_under_the_norm_bound(name):
    cx = ac.planted(name).ctx[0]
    qn2 = cx.q.float().pow(2).sum(-1).amax(-1)
    kn2 = cx.k.float().pow(2).sum(-1).amax(-1)
    assert (qn2 * kn2 <= 2500.0 * 0.98).all(), (qn2 * kn2).sqrt()          # attn_untracked_ok, with room for its fp32 sums
    assert (qn2 * 1.0e6 > 2500.0).all()                                    # a "too large" key bound of 1e6 does leave the fast body


@pytest.mark.parametrize("name", NAMES)
def test_reference_identities_and_simulated_kernel(name):
    c = ac.CASES[name]
    p = ac.planted(name)
    pre = bool(c.get("pre"))
    total = 0
    for cx in p.ctx:
        assert torch.allclose(cx.P.sum(-1), torch.ones(1, dtype=F64), atol=1e-13)
        qe = cx.q.to(F64) / (ac.ALPHA if pre else 1.0)
        s = torch.einsum("hqd,hkd->hqk", qe, cx.k.to(F64)) * ac.SCALE          # the textbook statement, natural-log units
        if cx.mask is not None:
            s = s.masked_fill(~cx.mask, -math.inf)
        assert torch.allclose(torch.softmax(s, -1) @ cx.v.to(F64), cx.ref, rtol=1e-10, atol=1e-13)
        for r, j, T in (cx.pairs[0], cx.pairs[-1]):
            if cx.kv == 1:
                continue
            keep = torch.ones(cx.kv, dtype=torch.bool)
            keep[j] = False
            brute = torch.softmax(s[:, r][:, keep], -1).unsqueeze(1) @ cx.v.to(F64)[:, keep]
            assert torch.allclose(brute[:, 0], cx.drop_ref(r, j), rtol=1e-8, atol=1e-12)
        # float32 simulation of the kernel's arithmetic: fp32 scores, exp2 against the row max, P rounded to bf16 for P.V only, fp32 sums
        t = torch.einsum("hqd,hkd->hqk", cx.q.float(), cx.k.float()) * (1.0 if pre else ac.ALPHA)
        if cx.mask is not None:
            t = t.masked_fill(~cx.mask, -math.inf)
        pp = torch.exp2(t - t.amax(-1, keepdim=True))
        sim = (pp.to(BF).float() @ cx.v.float()) / pp.sum(-1, keepdim=True)
        if len(p.ctx) == 1:
            assert ((sim.to(BF).to(F64) - cx.ref).abs() / cx.bar).max().item() <= 1.0
            assert (((sim + p.old.float()).to(BF).to(F64) - p.ref_acc).abs() / p.bar_acc).max().item() <= 1.0
        else:
            total = (total + sim).to(BF).float()
    if len(p.ctx) == 2:
        assert ((total.to(F64) - p.ref).abs() / p.bar).max().item() <= 1.0


def test_layouts_round_trip_and_fill_the_free_cells():
    g = torch.Generator().manual_seed(3)
    k, v = torch.randn(2, 321, 128, generator=g).to(BF), torch.randn(2, 321, 128, generator=g).to(BF)
    for segs, garbage in ((1, False), (2, True)):
        kp, vt = ac.layouts(k, v, 512, segs, garbage)
        kk, vv = ac.unlayout(kp, vt)
        assert torch.equal(kk[:, :321], k) and torch.equal(vv[:, :321], v)
        assert (vv[:, 321:384] == ac.V_PAD).all() and (kk[:, 384:] == ac.TILE_PAD).all() and (vv[:, 384:] == ac.TILE_PAD).all()
        pad = kk[:, 321:384].float()
        if garbage:
            assert (pad.abs() == torch.tensor(ac.K_GARBAGE).to(BF).float()).all() and (pad > 0).any() and (pad < 0).any()
        else:
            assert (pad == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_key_counts_discriminate_every_key(name):
    """The exact-count construction: for every key of every window, a reference that omits it, one that counts it twice and one that
    includes the first pad key each lie >= DISCRIM count-bars away."""
    c = ac.CASES[name]
    kvs = c["kv"] if isinstance(c["kv"], tuple) else (c["kv"] * c["block"] if c["entry"] == "bsa" else c["kv"],)
    for n in kvs:
        seen = 0
        for lo, hi in ac.count_windows(n):
            count, l = ac.expected_counts(n, lo, hi)
            assert count.max().item() <= 8 and float(l) == n
            seen += count.sum().item()
            omit, twice, pad = ac.count_discrimination(n, lo, hi)
            assert min(omit, pad) >= ac.DISCRIM and (twice >= ac.DISCRIM or n == 1), (n, lo, hi, omit, twice, pad)          # one key twice is the same softmax
        assert seen == n
    if c["entry"] == "bsa":          # per query block: only its selected keys count
        m = ac.key_mask(c)
        count, l = ac.expected_counts(kvs[0], 0, min(kvs[0], ac.COUNT_WINDOW), m)
        blk = c["block"]
        for qb, sel in enumerate(c["sel"]):
            assert float(l[qb * blk]) == len(sel) * blk
            assert count[qb * blk].sum().item() == sum(blk for b in sel if b * blk < ac.COUNT_WINDOW)
