"""GPU: the UMT5 encoder's kernels (csrc/t5.hip) called one at a time through the C-ABI, element by element against float64 references
on the kernel's own inputs.  Every measured max(|err| / bar) goes through tests._tol.within with the bar 1.

wf_t5_attn_fwd: inputs, reference and bar in tests/umt5_cases.py (tests/test_umt5_host.py proves on the CPU that the cases see a bucket
boundary moved by one).  Q, K, V are three column slices of one [L, 3 H 64] buffer, the output is a view into a wider buffer whose guard
columns must come back untouched.
wf_t5_gated_gelu: y = 0.5 g (1 + t) u, t = tanh(a), a = c (g + 0.044715 g^3) in fp32.  a carries <= 6 U |a| (three products, one sum,
the constant), which tanh damps by 1 - t^2; tanhf is good to 2 ulp and the sum 1 + t rounds once: |d(1 + t)| <= 2^-22 + 6 U |a| (1 -
t^2).  Three more products: 4 U |ref|.  So e32 = 0.5 |g u| (2^-22 + 6 U |a| (1 - t^2)) + 4 U |ref| and bar = 2^-8 |ref| + e32 (1 + 2^-8).
wf_t5_rmsnorm: the sum of C squares (positive terms) is C / 256 in-lane operations, 6 wave levels and 3 adds deep: relative (C / 256 +
10) U; mean, + eps: 2 U; rsqrtf 2^-22; halved by the root.  Two products 2 U: gamma = (C / 512 + 6) U + 2^-22 + 2 U, bar = |ref| (2^-8 +
gamma (1 + 2^-8)).  An all-zero row gives exactly 0.
wf_t5_embed: equality.
The stacked feed-forward-in GEMM [wi_0; wi_1] at the released shape (M 512, N 20480, K 4096, WF_EPI_F32) on 64 sampled columns with the
GEMM bar of tests/test_gpu_dit_kernels_fp64.py: e_v = 2^-22 S, bar = e_v + 2 U |z|."""
import math

import numpy as np
import pytest
import torch

from tests import umt5_cases as uc
from tests._tol import within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
U, U_BF = 2.0 ** -24, 2.0 ** -8
SENT16 = 0x7FA5


def _call(name, *args):
    from worldforge_amd import ops
    from worldforge_amd._ffi import call
    call(name, *args, ops.stream())


@pytest.mark.parametrize("H,L,kv", uc.case_list(), ids=lambda v: str(v))
def test_t5_attn_vs_fp64(H, L, kv):
    from worldforge_amd import umt5
    c = uc.AttnCase(H, L, kv, umt5.relative_position_bucket)
    qkv = c.qkv.to(DEV)
    inner, guard = H * 64, 8
    out = torch.full((L + 1, inner + guard), SENT16, dtype=torch.int16, device=DEV).view(BF)
    bias, lut = c.bias.to(DEV).contiguous(), torch.from_numpy(c.lut).to(DEV)
    _call("wf_t5_attn_fwd", qkv.data_ptr(), qkv.data_ptr() + 2 * inner, qkv.data_ptr() + 4 * inner, 3 * inner, out.data_ptr(),
          inner + guard, bias.data_ptr(), lut.data_ptr(), 512, 32, H, L, kv)
    torch.cuda.synchronize()
    got = out.cpu()
    raw = got.view(torch.int16)
    assert bool((raw[:L, inner:] == SENT16).all()), "guard columns written"
    assert bool((raw[L] == SENT16).all()), "row L written"
    y = got[:L, :inner].to(F64).view(L, H, 64)
    assert bool(torch.isfinite(y).all())
    r = ((y - c.ref).abs() / c.bar).max().item()
    print(f"t5_attn H {H} L {L} kv {kv}: max err / bar = {r:.3f} ({len(c.plan)} planted boundaries)")
    within("t5_attn", r, 1.0)


def test_t5_attn_refuses_bad_arguments():
    from worldforge_amd._ffi import lib
    x = torch.zeros(16, 3 * 64, dtype=BF, device=DEV)
    o = torch.zeros(16, 64, dtype=BF, device=DEV)
    b = torch.zeros(32, dtype=F32, device=DEV)
    lut = torch.zeros(1023, dtype=torch.uint8, device=DEV)
    f = lib().wf_t5_attn_fwd
    p = x.data_ptr()
    for L, kv in ((16, 0), (16, 17), (513, 4), (0, 0)):
        assert f(p, p + 128, p + 256, 192, o.data_ptr(), 64, b.data_ptr(), lut.data_ptr(), 512, 32, 1, L, kv, None) == -1, (L, kv)
    assert f(p, p + 128, p + 256, 192, o.data_ptr(), 64, b.data_ptr(), lut.data_ptr(), 512, 32, 0, 16, 16, None) == -1
    assert f(p, p + 128, p + 256, 192, o.data_ptr(), 64, b.data_ptr(), lut.data_ptr(), 8, 32, 1, 16, 16, None) == -1      # L > lmax
    assert f(p, p + 128, p + 256, 192, o.data_ptr(), 64, None, lut.data_ptr(), 512, 32, 1, 16, 16, None) == -1


G_SPECIAL = (0.0, 1e-3, -1e-3, 30.0, -30.0, 1e4, -1e4)


@pytest.mark.parametrize("M", [1, 70])
@pytest.mark.parametrize("F", [4, 192, 10240])
def test_t5_gated_gelu_vs_fp64(M, F):
    g = torch.Generator().manual_seed(7 * M + F)
    x = torch.randn(M, 2 * F, generator=g) * 2.0
    x[:, F:] = torch.randn(M, F, generator=g)
    for m in range(M):           # the special gate values walk through the columns and the rows, each beside an ordinary u
        for i in range(min(F, len(G_SPECIAL))):
            x[m, (m + i * max(F // len(G_SPECIAL), 1)) % F] = G_SPECIAL[(m + i) % len(G_SPECIAL)]
    xd = x.to(DEV)
    out = torch.empty(M, F, dtype=BF, device=DEV)
    _call("wf_t5_gated_gelu", xd.data_ptr(), 2 * F, out.data_ptr(), M, F)
    y = out.cpu().to(F64)
    assert bool(torch.isfinite(y).all())
    gg, uu = x[:, :F].to(F64), x[:, F:].to(F64)
    a = math.sqrt(2.0 / math.pi) * (gg + 0.044715 * gg ** 3)
    t = torch.tanh(a)
    ref = 0.5 * gg * (1.0 + t) * uu
    e32 = 0.5 * (gg * uu).abs() * (2.0 ** -22 + 6 * U * a.abs() * (1.0 - t * t)) + 4 * U * ref.abs()
    bar = U_BF * ref.abs() + e32 * (1 + U_BF) + 1e-30
    r = ((y - ref).abs() / bar).max().item()
    print(f"t5_gated_gelu M {M} F {F}: max err / bar = {r:.3f}")
    within("t5_gated_gelu", r, 1.0)
    if M > 1 or F > 4:
        assert all(bool((gg == float(np.float32(v))).any()) for v in G_SPECIAL)     # (the gates are fp32 values)
    assert bool((y[gg == -1e4] == 0).all()) and bool((y[gg == -30.0] == 0).all())


@pytest.mark.parametrize("C", [128, 4096])
def test_t5_rmsnorm_vs_fp64(C):
    g = torch.Generator().manual_seed(C)
    L = 9
    x = torch.randn(L, C, generator=g)
    x[3] = 0.0                                  # an all-zero row
    x[5] *= 1e4                                 # rows of magnitude 1e4
    x[6] = 1e4 * torch.sign(x[6])
    x[7] *= 1e-4
    w = (1.0 + 0.5 * torch.randn(C, generator=g)).to(BF).to(F32)
    eps = 1e-6
    out = torch.empty(L, C, dtype=BF, device=DEV)
    xd, wd = x.to(DEV), w.to(DEV)
    _call("wf_t5_rmsnorm", xd.data_ptr(), wd.data_ptr(), out.data_ptr(), L, C, eps)
    y = out.cpu().to(F64)
    x64 = x.to(F64)
    ref = x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + float(np.float32(eps))) * w.to(F64)
    gamma = (C / 512 + 6) * U + 2.0 ** -22 + 2 * U
    bar = ref.abs() * (U_BF + gamma * (1 + U_BF)) + 1e-30
    assert bool((y[3] == 0).all())
    r = ((y - ref).abs() / bar).max().item()
    print(f"t5_rmsnorm C {C}: max err / bar = {r:.3f}")
    within("t5_rmsnorm", r, 1.0)
    # a mean-subtracting norm would fail: the bar can see it
    ln = (x64 - x64.mean(-1, keepdim=True))
    ln = ln * torch.rsqrt(ln.pow(2).mean(-1, keepdim=True) + eps) * w.to(F64)
    assert ((ln - ref).abs() / bar)[[0, 1, 2]].max().item() > 8


def test_t5_embed_is_exact():
    g = torch.Generator().manual_seed(3)
    V, C, L = 97, 128, 70
    table = torch.randn(V, C, generator=g).to(BF)
    ids = torch.randint(0, V, (L,), generator=g).to(torch.int32)
    ids[0], ids[1] = 0, V - 1
    out = torch.full((L, C), float("nan"), dtype=F32, device=DEV)
    td, idd = table.to(DEV), ids.to(DEV)
    _call("wf_t5_embed", idd.data_ptr(), td.data_ptr(), out.data_ptr(), L, V, C)
    assert torch.equal(out.cpu(), table.to(F32)[ids.long()])


def test_stacked_ffn_in_gemm_at_the_released_shape():
    from worldforge_amd import dit
    M, N, K = 512, 20480, 4096
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(M, K, generator=g, device=DEV, dtype=F32).to(BF)
    w = (torch.randn(N, K, generator=g, device=DEV, dtype=F32) * K ** -0.5).to(BF)
    out = torch.empty(M, N, dtype=F32, device=DEV)
    dit.gemm(x, w, None, out, 2)
    cols = torch.randperm(N, generator=torch.Generator().manual_seed(6))[:64].sort().values
    cols[0], cols[1], cols[-2], cols[-1] = 0, 10239, 10240, N - 1           # the seam between wi_0 and wi_1 and both ends
    got = out[:, cols.to(DEV)].cpu().to(F64)
    x64, w64 = x.cpu().to(F64), w[cols.to(DEV)].cpu().to(F64)
    z, S = x64 @ w64.T, x64.abs() @ w64.abs().T
    bar = 2.0 ** -22 * S + 2 * U * z.abs() + 1e-30
    r = ((got - z).abs() / bar).max().item()
    print(f"stacked ffn-in gemm: max err / bar = {r:.3f}")
    within("t5_ffn_in_gemm", r, 1.0)
