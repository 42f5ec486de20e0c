"""GPU: the CLIP vision encoder's kernels (csrc/clip.hip) called one at a time through the C-ABI, element by element against float64
references on the kernel's own fp32 inputs.  Inputs, references and bars are in tests/clip_cases.py, where every bar is derived from the
kernel's arithmetic (tests/test_clip_host.py proves on the CPU that each case sees an operand or a P narrowed to bf16).  Every measured
max(|err| / bar) goes through tests._tol.within with the bar 1; the exact-integer GEMM cases assert equality.  Operands sit in buffers
with padded leading dimensions, outputs in wider buffers whose guard columns and guard row must come back untouched."""
import pytest
import torch

from tests import clip_cases as cc
from tests._tol import within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
SENT = -7.25e33


def _padded(t, pad):
    """t [R, C] in a [R, C + pad] device buffer -> (view, ld)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=F32, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf, t.shape[1] + pad


def _gemm(X, W, bias, M, N, K, epi, old=None):
    """-> out [M, N] on the CPU after the guard checks, from padded operands (ldx = K + 4, ldw = K + 8, ldo = N + 4, one guard row)."""
    from worldforge_amd import ops
    from worldforge_amd._ffi import call
    xb, ldx = _padded(X, 4)
    wb, ldw = _padded(W, 8)
    out = torch.full((M + 1, N + 4), SENT, dtype=F32, device=DEV)
    if old is not None:
        out[:M, :N] = old.to(DEV)
    bd = bias.to(DEV) if bias is not None else None
    call("wf_gemm_f32", xb.data_ptr(), wb.data_ptr(), None if bd is None else bd.data_ptr(), out.data_ptr(), M, N, K, ldx, ldw, N + 4, epi,
         ops.stream())
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got[:M, N:] == SENT).all()), "guard columns written"
    assert bool((got[M] == SENT).all()), "row M written"
    return got[:M, :N]


@pytest.mark.parametrize("kind,M,N,K", cc.exact_case_list(), ids=lambda v: str(v))
def test_gemm_f32_is_exact_on_integers(kind, M, N, K):
    X, W = cc.exact_inputs(kind, M, N, K)
    cols = cc.columns(N, K)
    got = _gemm(X, W, None, M, N, K, cc.EPI_F32)[:, cols].to(F64)
    ref = X.to(F64) @ W[cols].to(F64).T
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} elements differ, max |err| {float((got - ref).abs().max())}"


@pytest.mark.parametrize("i", range(len(cc.RANDOM_CASES)), ids=lambda i: "-".join(str(v) for v in cc.RANDOM_CASES[i]))
def test_gemm_f32_vs_fp64_every_epilogue(i):
    c = cc.GemmCase(*cc.RANDOM_CASES[i])
    got = _gemm(c.X, c.W, c.bias, c.M, c.N, c.K, c.epi, c.old)
    assert bool(torch.isfinite(got).all())
    r = ((got.to(F64) - c.ref).abs() / c.bar).max().item()
    print(f"gemm_f32 M {c.M} N {c.N} K {c.K} epilogue {c.epi}: max err / bar = {r:.3f}")
    again = _gemm(c.X, c.W, c.bias, c.M, c.N, c.K, c.epi, c.old)
    assert torch.equal(got, again), "two calls differ"
    within("clip_gemm_f32", r, 1.0)


def test_gemm_f32_refuses_bad_arguments():
    from worldforge_amd._ffi import lib
    x = torch.zeros(8, 16, dtype=F32, device=DEV)
    w = torch.zeros(8, 16, dtype=F32, device=DEV)
    o = torch.full((8, 8), SENT, dtype=F32, device=DEV)
    f = lib().wf_gemm_f32
    xp, wp, op = x.data_ptr(), w.data_ptr(), o.data_ptr()
    assert f(xp, wp, None, op, 8, 8, 16, 16, 16, 8, 2, None) == 0
    for M, N, K, ldx, ldw, ldo, epi in ((0, 8, 16, 16, 16, 8, 2), (8, 6, 16, 16, 16, 8, 2), (8, 8, 14, 16, 16, 8, 2), (8, 8, 16, 12, 16, 8, 2),
                                        (8, 8, 16, 16, 18, 8, 2), (8, 8, 16, 16, 16, 4, 2), (8, 8, 16, 16, 16, 8, 0), (8, 8, 16, 16, 16, 8, 3),
                                        (8, 8, 16, 16, 16, 8, 7), (8, 8, 16, 16, 16, 8, 1)):
        o.fill_(SENT)
        assert f(xp, wp, None, op, M, N, K, ldx, ldw, ldo, epi, None) == -1, (M, N, K, ldx, ldw, ldo, epi)
        assert bool((o == SENT).all())
    assert f(None, wp, None, op, 8, 8, 16, 16, 16, 8, 2, None) == -1
    assert f(xp + 4, wp, None, op, 8, 8, 12, 16, 16, 8, 2, None) == -1          # a pointer that is not 16-byte aligned
    assert f(xp, wp, xp + 8, op, 8, 8, 16, 16, 16, 8, 2, None) == -1


@pytest.mark.parametrize("H,L,D", cc.ATTN_SHAPES, ids=lambda v: str(v))
def test_clip_attn_vs_fp64(H, L, D):
    from worldforge_amd import ops
    from worldforge_amd._ffi import call
    c = cc.AttnCase(H, L, D)
    inner, guard = H * D, 4
    qkv = c.qkv.to(DEV)
    out = torch.full((L + 1, inner + guard), SENT, dtype=F32, device=DEV)
    outs = []
    for _ in range(2):
        call("wf_clip_attn_fwd", qkv.data_ptr(), qkv.data_ptr() + 4 * inner, qkv.data_ptr() + 8 * inner, 3 * inner, out.data_ptr(),
             inner + guard, H, L, D, c.scale, ops.stream())
        torch.cuda.synchronize()
        outs.append(out.cpu())
    got = outs[0]
    assert torch.equal(outs[0], outs[1]), "two calls differ"
    assert bool((got[:L, inner:] == SENT).all()), "guard columns written"
    assert bool((got[L] == SENT).all()), "row L written"
    y = got[:L, :inner].to(F64).view(L, H, D)
    assert bool(torch.isfinite(y).all())
    r = ((y - c.ref).abs() / c.bar).max().item()
    print(f"clip_attn H {H} L {L} D {D}: max err / bar = {r:.3f}")
    within("clip_attn", r, 1.0)


def test_clip_attn_refuses_bad_arguments():
    from worldforge_amd._ffi import lib
    x = torch.zeros(16, 3 * 80, dtype=F32, device=DEV)
    o = torch.full((16, 80), SENT, dtype=F32, device=DEV)
    f = lib().wf_clip_attn_fwd
    p, op = x.data_ptr(), o.data_ptr()
    assert f(p, p + 320, p + 640, 240, op, 80, 1, 16, 80, 0.1, None) == 0
    o.fill_(SENT)
    for ldqkv, ldo, H, L, D, scale in ((240, 80, 1, 0, 80, 0.1), (240, 80, 1, 1025, 80, 0.1), (240, 80, 0, 16, 80, 0.1), (240, 80, 1, 16, 76, 0.1),
                                       (240, 80, 1, 16, 136, 0.1), (240, 80, 1, 16, 4, 0.1), (242, 80, 1, 16, 80, 0.1), (240, 78, 1, 16, 80, 0.1),
                                       (240, 80, 4, 16, 80, 0.1), (240, 80, 1, 16, 80, 0.0), (240, 80, 1, 16, 80, float("inf")),
                                       (240, 80, 1, 16, 80, float("nan"))):
        assert f(p, p + 320, p + 640, ldqkv, op, ldo, H, L, D, scale, None) == -1, (ldqkv, ldo, H, L, D, scale)
    assert f(p, p + 320, None, 240, op, 80, 1, 16, 80, 0.1, None) == -1
    assert f(p, p + 324, p + 640, 240, op, 80, 1, 16, 80, 0.1, None) == -1        # K not 16-byte aligned
    torch.cuda.synchronize()
    assert bool((o == SENT).all())


def test_patch_rows_is_the_conv_weights_flattening_order():
    from worldforge_amd import ops
    from worldforge_amd._ffi import call, lib
    for S, p in ((64, 4), (28, 14), (6, 3)):
        G = S // p
        px = torch.randn(3, S, S, generator=torch.Generator().manual_seed(S))
        rows = torch.full((G * G + 1, 3 * p * p), SENT, dtype=F32, device=DEV)
        pd = px.to(DEV)
        call("wf_clip_patch_rows", pd.data_ptr(), rows.data_ptr(), S, p, ops.stream())
        want = px.view(3, G, p, G, p).permute(1, 3, 0, 2, 4).reshape(G * G, 3 * p * p)          # unfold: [py, px][c, ph, pw]
        got = rows.cpu()
        assert torch.equal(got[:-1], want) and bool((got[-1] == SENT).all())
    f = lib().wf_clip_patch_rows
    assert f(pd.data_ptr(), rows.data_ptr(), 7, 3, None) == -1 and f(None, rows.data_ptr(), 6, 3, None) == -1
    assert f(pd.data_ptr(), rows.data_ptr(), 0, 0, None) == -1
