"""GPU: the kernels of csrc/vit.hip called one at a time through the C-ABI, element by element against float64 references on the kernel's
own inputs.  Inputs, references and bars (with their error models) are in tests/vggt_cases.py; tests/test_vggt_host.py proves on the CPU
that the cases see a dropped last tile, a skipped rescale, the wrong RoPE pairing and a rotated position 0.  Every measured
max(|err| / bar) goes through tests._tol.within with the bar 1 (the new cases have no entries in tolerances_mi355x.json yet).

Q, K, V are three column slices of one [nseq L, 3 H 64] buffer; the output is a view into a wider buffer with one more row: guard
columns and the guard row must come back untouched."""
import pytest
import torch

from tests import vggt_cases as vc
from tests._tol import within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
SENT16 = 0x7FA5


def _call(name, *args):
    from worldforge_amd import ops
    from worldforge_amd._ffi import call
    call(name, *args, ops.stream())


def _attn(qkv, nseq, H, L, guard=8, rows_extra=1):
    inner = H * 64
    out = torch.full((nseq * L + rows_extra, inner + guard), SENT16, dtype=torch.int16, device=DEV).view(BF)
    _call("wf_vit_attn_fwd", qkv.data_ptr(), qkv.data_ptr() + 2 * inner, qkv.data_ptr() + 4 * inner, 3 * inner, out.data_ptr(), inner + guard,
          nseq, H, L, vc.SCALE)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("nseq,H,L", vc.ATTN_SHAPES + (vc.SAMPLED,), ids=str)
def test_vit_attn_vs_fp64(nseq, H, L):
    sampled = (nseq, H, L) == vc.SAMPLED
    rows = sorted(set(range(0, L, 41)) | set(range(L - 70, L))) if sampled else None
    c = vc.AttnCase(nseq, H, L, rows=rows, device=DEV)
    inner = H * 64
    qkv = torch.cat([c.qkv, torch.full((1, 3 * inner), float("nan"), dtype=BF)], 0).to(DEV)   # a NaN row behind the last sequence: never read
    out = _attn(qkv, nseq, H, L)
    got = out.cpu()
    raw = got.view(torch.int16)
    assert bool((raw[:nseq * L, inner:] == SENT16).all()), "guard columns written"
    assert bool((raw[nseq * L] == SENT16).all()), "guard row written"
    y = got[:nseq * L, :inner].to(F64).view(nseq, L, H, 64)[:, c.rows]
    assert bool(torch.isfinite(y).all())
    ratio = (y - c.ref).abs() / c.bar
    r = ratio.max().item()
    planted = {name: ratio[:, int((c.rows == row).nonzero()[0])].max().item() for name, (row, _) in c.plan.items()}
    print(f"vit_attn nseq {nseq} H {H} L {L}: max err / bar = {r:.3f}; planted rows {planted}")
    within("vit_attn", r, 1.0)
    if nseq == 2:      # sequence 1 of the call equals, bit for bit, a single call on its slice
        one = _attn(qkv[L:], 1, H, L)
        assert torch.equal(one[:L, :inner].view(torch.int16), out[L:2 * L, :inner].view(torch.int16))
    again = _attn(qkv, nseq, H, L)
    assert torch.equal(again.view(torch.int16), out.view(torch.int16)), "two calls differ"


@pytest.mark.parametrize("norm,rope", [(True, True), (True, False), (False, True)], ids=str)
@pytest.mark.parametrize("nseq,H,gh,gw", [(1, 1, 1, 1), (3, 2, 4, 6), (2, 16, 21, 37)], ids=str)
def test_vit_qk_norm_rope_vs_fp64(nseq, H, gh, gw, norm, rope):
    c = vc.NormRopeCase(nseq, H, gh, gw, norm=norm, rope=rope)
    M, inner = nseq * c.L, H * 64
    buf = torch.cat([c.qkv, torch.full((1, 3 * inner), SENT16, dtype=torch.int16).view(BF)], 0).to(DEV)      # one guard row
    before = buf.clone()
    d = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
    qw, qb, kw, kb, cs, sn, pos = (d(t) for t in (c.qw, c.qb, c.kw, c.kb, c.cs, c.sn, c.pos))
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    scale = 0.25
    _call("wf_vit_qk_norm_rope", buf.data_ptr(), buf.data_ptr() + 2 * inner, 3 * inner, p(qw), p(qb), p(kw), p(kb), c.eps, p(cs), p(sn), c.max_pos,
          p(pos), nseq, c.L, H, scale)
    torch.cuda.synchronize()
    raw, raw0 = buf.cpu().view(torch.int16), before.cpu().view(torch.int16)
    assert torch.equal(raw[:, 2 * inner:], raw0[:, 2 * inner:]), "the v slice changed"
    assert torch.equal(raw[M], raw0[M]), "the guard row changed"
    got = buf.cpu()[:M].to(F64).view(M, 3, H, 64)
    rq, bq, rk, bk = c.reference()
    r = max(((got[:, 0] - rq * scale).abs() / (bq * scale)).max().item(), ((got[:, 1] - rk).abs() / bk).max().item())   # out_scale is a power of two
    print(f"vit_qk_norm_rope nseq {nseq} H {H} grid {gh}x{gw} norm {norm} rope {rope}: max err / bar = {r:.3f}")
    within("vit_qk_norm_rope", r, 1.0)
    if norm and rope:  # special-token rows equal the norm alone, bit for bit
        alone = before.clone()
        _call("wf_vit_qk_norm_rope", alone.data_ptr(), alone.data_ptr() + 2 * inner, 3 * inner, p(qw), p(qb), p(kw), p(kb), c.eps, None, None, 0,
              None, nseq, c.L, H, scale)
        torch.cuda.synchronize()
        a = alone.cpu().view(torch.int16).view(-1, 3 * inner)
        for s in range(nseq):
            assert torch.equal(raw[s * c.L:s * c.L + 5], a[s * c.L:s * c.L + 5])
        assert not torch.equal(raw[5:c.L], a[5:c.L])


@pytest.mark.parametrize("n,H,W", [(2, 56, 84), (1, 14, 14)], ids=str)
def test_vit_patch_rows_vs_fp64(n, H, W):
    g = torch.Generator().manual_seed(H + W)
    img = torch.rand(n, 3, H, W, generator=g)
    img[0, :, 0, :3] = torch.tensor([[0.0, 1.0, 0.485]]).expand(3, 3)            # the ends of the range and a value next to a mean
    ref, bar = vc.patch_rows_reference(img)
    R = ref.shape[0]
    out = torch.full((R + 1, 592), SENT16, dtype=torch.int16, device=DEV).view(BF)
    x = img.to(DEV)
    _call("wf_vit_patch_rows", x.data_ptr(), out.data_ptr(), n, H, W)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got.view(torch.int16)[R] == SENT16).all()), "guard row written"
    assert bool((got[:R, 588:].view(torch.int16) == 0).all()), "columns 588..591 must be exactly zero"
    r = ((got[:R, :588].to(F64) - ref[:, :588]).abs() / (bar[:, :588] + 1e-30)).max().item()
    print(f"vit_patch_rows n {n} {H}x{W}: max err / bar = {r:.3f}")
    within("vit_patch_rows", r, 1.0)


def test_vit_kernels_refuse_bad_arguments():
    from worldforge_amd._ffi import lib
    L = lib()
    x = torch.zeros(16, 3 * 64, dtype=BF, device=DEV)
    o = torch.full((16, 64), SENT16, dtype=torch.int16, device=DEV)
    p, po = x.data_ptr(), o.data_ptr()

    def refused(rc, entry):
        assert rc != 0 and entry.encode() in L.wf_last_error(), (entry, rc, L.wf_last_error())

    f = L.wf_vit_attn_fwd
    for args in ((None, p + 128, p + 256, 192, po, 64, 1, 1, 16, 0.125), (p, p + 128, p + 256, 192, None, 64, 1, 1, 16, 0.125),
                 (p, p + 128, p + 256, 192, po, 64, 0, 1, 16, 0.125), (p, p + 128, p + 256, 192, po, 64, 1, 0, 16, 0.125),
                 (p, p + 128, p + 256, 192, po, 64, 1, 1, 0, 0.125), (p, p + 128, p + 256, 192, po, 64, 1, 1, 16, 0.0),
                 (p, p + 128, p + 256, 190, po, 64, 1, 1, 16, 0.125), (p, p + 128, p + 256, 192, po, 32, 1, 1, 16, 0.125),
                 (p + 2, p + 128, p + 256, 192, po, 64, 1, 1, 16, 0.125), (p, p + 128, p + 256, 192, po, 64, 70000, 1, 16, 0.125)):
        refused(f(*args, None), "wf_vit_attn_fwd")
    w = torch.ones(64, dtype=F32, device=DEV)
    t = torch.ones(4, 16, dtype=F32, device=DEV)
    pos = torch.zeros(16, 2, dtype=torch.int32, device=DEV)
    wp, tp, pp = w.data_ptr(), t.data_ptr(), pos.data_ptr()
    x0 = x.clone()
    f = L.wf_vit_qk_norm_rope
    for args in ((None, p + 128, 192, wp, wp, wp, wp, 1e-5, tp, tp, 3, pp, 1, 16, 1, 1.0), (p, p + 128, 192, wp, None, wp, wp, 1e-5, tp, tp, 3, pp, 1, 16, 1, 1.0),
                 (p, p + 128, 192, wp, wp, wp, wp, 1e-5, tp, None, 3, pp, 1, 16, 1, 1.0), (p, p + 128, 192, wp, wp, wp, wp, 1e-5, tp, tp, 3, None, 1, 16, 1, 1.0),
                 (p, p + 128, 192, wp, wp, wp, wp, 0.0, tp, tp, 3, pp, 1, 16, 1, 1.0), (p, p + 128, 192, wp, wp, wp, wp, 1e-5, tp, tp, 3, pp, 1, 0, 1, 1.0),
                 (p, p + 128, 192, wp, wp, wp, wp, 1e-5, tp, tp, 3, pp, 1, 16, 0, 1.0), (p, p + 128, 192, wp, wp, wp, wp, 1e-5, tp, tp, 3, pp, 1, 16, 1, 0.0),
                 (p, p + 128, 32, wp, wp, wp, wp, 1e-5, tp, tp, 3, pp, 1, 16, 1, 1.0), (p, p + 128, 192, wp, wp, wp, wp, 1e-5, tp, tp, -1, pp, 1, 16, 1, 1.0)):
        refused(f(*args, None), "wf_vit_qk_norm_rope")
    img = torch.zeros(3 * 28 * 28, dtype=F32, device=DEV)
    f = L.wf_vit_patch_rows
    for args in ((None, po, 1, 28, 28), (img.data_ptr(), None, 1, 28, 28), (img.data_ptr(), po, 0, 28, 28), (img.data_ptr(), po, 1, 27, 28),
                 (img.data_ptr(), po, 1, 28, 15), (img.data_ptr(), po, 1, 0, 28)):
        refused(f(*args, None), "wf_vit_patch_rows")
    torch.cuda.synchronize()
    assert bool((o == SENT16).all()) and torch.equal(x.view(torch.int16), x0.view(torch.int16)), "a refused call wrote"
