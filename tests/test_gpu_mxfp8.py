"""GPU: the opt-in MX-fp8 linear layers (csrc/mxfp8.hip, linear_precision="mxfp8").

  * wf_mx_quant_e4m3 bit for bit against a CPU reference built here from torch's float8_e4m3fn / float8_e8m0fnu, on random rows and on
    the edge cases (zero blocks, amax a power of two and exactly 448 * 2^e, RNE ties, e4m3 subnormals, bf16 denormals, NaN / Inf, a
    strided row as the padded FFN's ffh[:, :ffn_dim]).
  * wf_gemm_mxfp8 exactly on small-integer e4m3 operands with distinct per-block scales on both sides (pins the row / column, k order
    and scale-lane mapping of the scaled MFMA), then at the production shapes and every epilogue against a float64 product of the
    DEQUANTIZED operands read back from the device: the same quantized inputs on both sides, so the bar is the fp32-accumulation class.
  * Wan / LongCat forwards in mxfp8 against the oracle with the same six linears quantize-dequantized (and against the plain oracle),
    the stale-weight guard, and the end-to-end smoke job's PSNR.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from worldforge_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


# ---- CPU reference of the OCP MX-fp8 quantizer ---------------------------------------------------------------------------------------
def ref_quant(x: torch.Tensor):
    """x [M, K] (bf16 values, any float dtype) -> (q uint8 [M, K], s uint8 [M, K/32]).  e = the smallest integer with amax / 2^e <= 448,
    clamped to [-127, 127]; q = RNE_e4m3(x / 2^e); a block with a NaN / Inf: s = 0xff, q = 0x7f."""
    M, K = x.shape
    xb = x.float().reshape(M, K // 32, 32)
    amax = xb.abs().amax(-1)
    bad = ~torch.isfinite(xb).all(-1)
    m, E = torch.frexp(torch.where(bad, torch.zeros_like(amax), amax))  # amax = (2m) 2^(E-1), 2m in [1, 2)
    e = (E - 1) - 8 + (2 * m > 1.75).int()
    e = torch.where(amax == 0, torch.full_like(e, -127), e).clamp(-127, 127)
    s = torch.pow(2.0, e.double()).to(torch.float8_e8m0fnu).view(torch.uint8)
    inv = torch.pow(2.0, -e.double()).float()
    q = (xb * inv[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    s = torch.where(bad, torch.full_like(s, 0xFF), s)
    q = torch.where(bad[..., None], torch.full_like(q, 0x7F), q)
    return q.reshape(M, K), s


def dequant(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """float64 values of an MX-fp8 matrix (q [R, K] uint8, s [R, K/32] uint8)."""
    R, K = q.shape
    v = q.cpu().contiguous().view(torch.float8_e4m3fn).double().reshape(R, K // 32, 32)
    sc = torch.pow(2.0, s.cpu().double() - 127.0)
    return (v * sc[..., None]).reshape(R, K)


def qdq(x: torch.Tensor) -> torch.Tensor:
    """quantize-dequantize (CPU reference) in x's dtype, for the simulated-MX oracle"""
    return dequant(*ref_quant(x.to(BF))).to(x.dtype)


def _edge_rows(K=256):
    """rows of 8 blocks each: one edge case per block"""
    rows = []
    g = torch.Generator().manual_seed(3)
    base = lambda: torch.randn(K, generator=g).to(BF).float()  # noqa: E731
    r = base()
    r[0:32] = 0.0                                   # zero block
    r[32:64] = r[32:64].clamp(-0.9, 0.9); r[40] = 1.0; r[41] = -1.0   # amax exactly 2^0
    r[64:96] = r[64:96] * 10; r[70] = 448.0 / 8; r[64:96] = r[64:96].clamp(-56, 56)   # amax exactly 448 * 2^-3
    r[96:128] = torch.tensor([448.0, 17.0, 19.0, -17.0, 21.0, 23.0, 25.0, 27.0] * 4)  # e = 0: RNE ties at spacing 2 (16..32)
    r[128:160] = torch.tensor([448.0, 3 * 2.0 ** -10, 2.0 ** -10, 5 * 2.0 ** -10, 3 * 2.0 ** -8, -2.0 ** -9, 2.0 ** -7, 7 * 2.0 ** -11] * 4)  # subnormals
    r[160:192] = torch.tensor([(i + 1) * 2.0 ** -133 for i in range(32)])  # bf16 denormals (clamped e = -127)
    r[192:224] = -0.0                               # negative zeros
    r[224:256] = r[224:256] * 1e30                  # large block
    rows.append(r)
    for bad in (float("nan"), float("inf"), float("-inf")):
        r = base()
        r[37] = bad                                 # one non-finite element poisons block 1 only
        rows.append(r)
    r = base()
    r[0:32] = 1.75 * 2.0 ** 120; r[32:64] = 2.0 ** 127  # the largest bf16 exponents: e = 112, 119
    rows.append(r)
    return torch.stack(rows).to(BF)


def _quant_dev(x):
    q, s = ops.mx_quant(x)
    torch.cuda.synchronize()
    return q.cpu(), s.cpu()


def test_quantizer_bit_exact_random_and_edge_cases():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(97, 1024, generator=g) * torch.logspace(-30, 30, 97)[:, None]).to(BF)
    x = torch.cat([x, _edge_rows().repeat(1, 4)], 0)
    q, s = _quant_dev(x.to(DEV))
    rq, rs = ref_quant(x)
    assert torch.equal(s, rs), (s != rs).nonzero()[:8]
    assert torch.equal(q, rq), (q != rq).nonzero()[:8]
    # the edge rows really exercise what they claim
    er = ref_quant(_edge_rows())[1]
    assert er[0, 0] == 0 and er[0, 1] == 127 - 8 and er[0, 2] == 127 - 3 and er[0, 3] == 127 and er[0, 5] == 0
    assert (er[1:4, 1] == 0xFF).all() and (er[1:4, 0] != 0xFF).all() and er[4, 0] == 127 + 112 and er[4, 1] == 127 + 119
    # the dequantized values of a non-finite block are non-finite
    d = dequant(q[-4:-1], s[-4:-1])
    assert not torch.isfinite(d[:, 32:64]).any() and torch.isfinite(d[:, :32]).all()


def test_quantizer_strided_rows():
    """the FFN-down operand ffh[:, :ffn_dim]: rows read through a stride wider than K"""
    g = torch.Generator().manual_seed(2)
    big = torch.randn(333, 14080, generator=g).to(BF)
    x = big.to(DEV)[:, :13824]
    q, s = _quant_dev(x)
    rq, rs = ref_quant(big[:, :13824])
    assert torch.equal(s, rs) and torch.equal(q, rq)


# ---- GEMM ------------------------------------------------------------------------------------------------------------------------------
def _gemm(xq, xs, wq, ws, bias, out, epi, gate=None):
    ops.gemm_mxfp8(xq, xs, wq, ws, bias, out, epi, gate)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("M,N,K", [(300, 264, 384), (64, 520, 128), (516, 256, 640)])
def test_gemm_layout_exact(M, N, K):
    """small-integer e4m3 elements (|v| <= 8) with distinct per-block scales 2^-2 .. 2^2 on BOTH operands: every product is a multiple of
    2^-10 below 2^10 and every sum stays below 2^24 ulps -- exact in fp32, so the result must equal the float64 product exactly."""
    g = torch.Generator().manual_seed(M + N + K)
    ints = torch.randint(-8, 9, (M + N, K), generator=g).float()
    codes = ints.to(torch.float8_e4m3fn).view(torch.uint8)
    sc = torch.randint(125, 130, (M + N, K // 32), generator=g).to(torch.uint8)
    xq_full = torch.zeros(M, K + 64, dtype=torch.uint8)
    xq_full[:, :K] = codes[:M]
    xq = xq_full.to(DEV)[:, :K]  # row stride K + 64
    xs, wq, ws = sc[:M].to(DEV), codes[M:].contiguous().to(DEV), sc[M:].contiguous().to(DEV)
    want = dequant(codes[:M], sc[:M]) @ dequant(codes[M:], sc[M:]).T
    out = torch.full((M, N), float("nan"), device=DEV)
    got = _gemm(xq, xs, wq, ws, None, out, 2).cpu().double()
    assert torch.equal(got, want), (got - want).abs().max()
    # a k-order or scale-lane error that preserves the sums of a symmetric case does not hide: the transposed problem too
    out2 = torch.full((N, M), float("nan"), device=DEV)
    got2 = _gemm(wq, ws, xq.contiguous(), xs, None, out2, 2).cpu().double()
    assert torch.equal(got2, want.T)


@pytest.mark.parametrize("M,N,K", [(1100, 3820, 128), (1100, 3820, 384), (300, 264, 128)])
def test_mx_and_bf16_epilogues_agree_bit_for_bit(M, N, K):
    """wf_gemm_mxfp8 and wf_gemm_bf16 share one epilogue (csrc/gemm_pp.h); here they must give the same bits.  X in [-4, 4] and W in
    [-2, 2] are small integers: at most two mantissa bits, so the MX quantizer represents them exactly under any power-of-two block scale
    (asserted), and every dot product is an integer below 2^24, exact in fp32 in any summation order -- both kernels hand their epilogues
    the same accumulator bits.  Shapes: ragged M and N with N % 8 == 4 (the half-chunk store) where the bf16 call takes the ping-pong
    kernel, at one K tile of the MX kernel and at three; and a small problem where the bf16 call takes the 128 x 128 k_gemm, whose
    untransposed epilogue must give the same bits too.  Outputs are strided views with guard rows and columns."""
    from worldforge_amd import dit
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randint(-4, 5, (M, K), generator=g).to(BF)
    w = torch.randint(-2, 3, (N, K), generator=g).to(BF)
    bias, gate = torch.randn(N, generator=g), torch.randn(N, generator=g)
    ldo = (N + 15) // 8 * 8  # guard columns; a multiple of 8 keeps the view below the guard row 16-byte aligned in bf16
    old = torch.randn(M + 2, ldo, generator=g)
    xd, wd, bias_d, gate_d = x.to(DEV), w.to(DEV), bias.to(DEV), gate.to(DEV)
    xq, xs = ops.mx_quant(xd)
    wq, ws = ops.mx_quant(wd)
    torch.cuda.synchronize()
    assert torch.equal(dequant(xq, xs), x.double()) and torch.equal(dequant(wq, ws), w.double())
    guard = torch.ones(M + 2, ldo, dtype=torch.bool)
    guard[1:M + 1, :N] = False
    for epi in (0, 1, 2, 3):
        init = old.to(BF if epi < 2 else torch.float32)
        buf_bf, buf_mx = init.to(DEV), init.to(DEV)
        dit.gemm(xd, wd, bias_d, buf_bf[1:M + 1, :N], epi, gate_d if epi == 3 else None)
        _gemm(xq, xs, wq, ws, bias_d, buf_mx[1:M + 1, :N], epi, gate_d if epi == 3 else None)
        got_bf, got_mx = buf_bf.cpu(), buf_mx.cpu()
        assert torch.equal(got_mx, got_bf), (epi, (got_mx != got_bf).nonzero()[:8])
        assert torch.equal(got_bf[guard], init[guard]), epi
        if epi == 2:  # and the common bits are the right ones: an exact integer sum plus one fp32 addition
            assert torch.equal(got_bf[1:M + 1, :N], x.float() @ w.float().T + bias)


C2 = [(15360, 5120), (5120, 5120), (14080, 5120), (5120, 13824)]
LONGCAT = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)]
FP32_BAR = 2e-5
SHAPES = [(32760, n, k) for n, k in C2] + [(4095, n, k) for n, k in C2] + [(8190, n, k) for n, k in LONGCAT]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_numerics_production_shapes(M, N, K):
    """every epilogue against float64 on the dequantized device operands (sampled rows: every 256-row tile's first and last row and one
    random row, plus the ragged last tile whole).  fp32 outputs: relative Frobenius <= FP32_BAR; bf16 outputs additionally carry their own
    rounding (<= 2^-9 of each value).  FP32_BAR is 2e-5, not the 1e-5 of an fp32 K loop: the scaled MFMA measured 1.46e-5 at EVERY shape
    here, independent of K (4096 .. 13 824) -- a per-instruction property of v_mfma_scale_f32_32x32x64_f8f6f4, not an accumulation that
    grows with the K loop -- while a K tile lost from the loop shows up above 30x the bar (checked below)."""
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N + K)
    x = torch.randn(M, K, generator=g, device=DEV).to(BF)
    w = (torch.randn(N, K, generator=g, device=DEV) / math.sqrt(K)).to(BF)
    bias = torch.randn(N, generator=g, device=DEV) * 0.1
    gate = torch.randn(N, generator=g, device=DEV)
    xq, xs = ops.mx_quant(x)
    wq, ws = ops.mx_quant(w)
    nt = -(-M // 256)
    rows = sorted(set([t * 256 for t in range(nt)] + [min(t * 256 + 255, M - 1) for t in range(nt)]
                      + torch.randint(0, M, (nt,), generator=torch.Generator().manual_seed(K)).tolist() + list(range((nt - 1) * 256, M))))
    rows_t = torch.tensor(rows)
    xd = dequant(xq[rows_t.to(DEV)], xs[rows_t.to(DEV)])
    wd = dequant(wq, ws)
    z = xd @ wd.T + bias.cpu().double()
    old = torch.randn(M, N, generator=g, device=DEV)
    for epi in (0, 1, 2, 3):
        if epi in (2, 3):
            out = old.clone() if epi == 3 else torch.full((M, N), float("nan"), device=DEV)
            want = z if epi == 2 else old.cpu().double()[rows_t] + z * gate.cpu().double()
        else:
            out = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
            want = z if epi == 0 else F.gelu(z, approximate="tanh")
        _gemm(xq, xs, wq, ws, bias, out, epi, gate if epi == 3 else None)
        got = out[rows_t.to(DEV)].cpu().double()
        err = (got - want).norm().item() / want.norm().item()
        if epi in (2, 3):
            assert err <= FP32_BAR, (epi, err)
        else:
            assert err <= 2.0 ** -8, (epi, err)
            e_r = (got - want.to(BF).double()).norm().item() / want.norm().item()
            assert e_r <= 1e-3, (epi, e_r)
        assert torch.isfinite(got).all()
        del out
    # the K loop's last tile counts: dropping its 128 products is visible far above the bar
    z_short = xd[:, :-128] @ wd[:, :-128].T + bias.cpu().double()
    assert (z_short - z).norm().item() / z.norm().item() > 30 * FP32_BAR


# ---- forwards against the simulated-MX oracle ---------------------------------------------------------------------------------------
# The mxfp8 forward must follow the simulated-MX oracle clearly more closely than the plain one: e_sim <= SIM_RATIO e_plain (measured
# 0.48 Wan, 0.55 LongCat).  It cannot follow it to within 2x the bf16 path's own error (measured 3.9x Wan, 1.9x LongCat): the engine's
# bf16 activations differ from the oracle's by ~1 bf16 ulp, and about one element in 16 then lands on the other side of an e4m3 rounding
# boundary (e4m3 keeps 4 of bf16's 8 significant bits), an error of one e4m3 step each -- fp8 rounding amplifies the bf16 difference.
SIM_RATIO = 0.75
WAN_Q = (".self_attn.q", ".self_attn.k", ".self_attn.v", ".self_attn.o", ".cross_attn.q", ".cross_attn.o", ".ffn.0", ".ffn.2")


def _rel(a, b):
    return (a.double() - b.double()).norm().item() / b.double().norm().item()


def test_wan_forward_vs_simulated_mx_oracle(monkeypatch):
    from oracle import dit as odit
    from worldforge_amd import dit
    dim, heads, ffn, layers = 256, 2, 640, 2
    ocfg = odit.DiTConfig(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=layers, text_dim=64)
    W = odit.random_weights(ocfg, seed=11)
    Wb = {k: (v.to(BF).float() if v.dim() >= 2 else v) for k, v in W.items()}
    cfg = dit.DiTConfig(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=layers, text_dim=64)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(36, 3, 8, 10, generator=g).to(BF)
    ctx, clip = torch.randn(30, 64, generator=g).to(BF), torch.randn(257, 1280, generator=g).to(BF)
    outs = {}
    for prec in ("bf16", "mxfp8"):
        m = dit.WanTransformer3DModel(cfg, DEV, linear_precision=prec).load_state_dict(W)
        outs[prec] = m.forward_tokens(x.to(DEV), 749.0, ctx.to(DEV), clip.to(DEV)).cpu()
    args = (ocfg, x.float(), torch.tensor(749), ctx.float(), clip.float())
    plain = odit.forward(Wb, *args)
    lin0 = odit._lin

    def lin_mx(xx, WW, prefix):
        if prefix.startswith("blocks.") and prefix.endswith(WAN_Q):
            return F.linear(qdq(xx), qdq(WW[prefix + ".weight"]), WW.get(prefix + ".bias"))
        return lin0(xx, WW, prefix)

    monkeypatch.setattr(odit, "_lin", lin_mx)
    sim = odit.forward(Wb, *args)
    monkeypatch.setattr(odit, "_lin", lin0)
    e_bf, e_sim, e_plain = _rel(outs["bf16"], plain), _rel(outs["mxfp8"], sim), _rel(outs["mxfp8"], plain)
    print(f"[wan] bf16 vs oracle {e_bf:.3e}; mxfp8 vs simulated-MX oracle {e_sim:.3e}, vs plain oracle {e_plain:.3e}")
    assert e_sim <= SIM_RATIO * e_plain


def test_longcat_forward_vs_simulated_mx_oracle(monkeypatch):
    from oracle import longcat_dit as olc
    from worldforge_amd.longcat_dit import LongCatConfig, LongCatVideoTransformer3DModel
    C, heads, depth = 256, 2, 2
    kw = dict(hidden_size=C, depth=depth, num_heads=heads, caption_channels=96, adaln_tembed_dim=64)
    ocfg, cfg = olc.LongCatConfig(**kw), LongCatConfig(**kw)
    W = olc.random_weights(ocfg, seed=4)
    g = torch.Generator().manual_seed(6)
    T, h, w, ncond = 4, 8, 12, 1
    x = torch.randn(16, T, h, w, generator=g).to(BF)
    cap = torch.randn(40, 96, generator=g).to(BF)
    mask = torch.zeros(40, dtype=torch.int64)
    mask[:29] = 1
    ts = [0.0] * ncond + [812.0] * (T - ncond)
    outs = {}
    for prec in ("bf16", "mxfp8"):
        m = LongCatVideoTransformer3DModel(cfg, DEV, linear_precision=prec).load_state_dict(W)
        outs[prec] = m.forward_tokens(x.to(DEV), ts, cap.to(DEV), mask, ncond).cpu()
    args = (W, ocfg, x.float(), torch.tensor(ts), cap.float(), mask)
    plain = olc.forward(*args, num_cond_latents=ncond)
    names = [f"blocks.{i}.{n}.weight" for i in range(depth)
             for n in ("attn.qkv", "attn.proj", "cross_attn.q_linear", "cross_attn.proj", "ffn.w1", "ffn.w3", "ffn.w2")]
    pick = {id(W[k]) for k in names}

    class _F:  # the oracle module's `F` with F.linear quantize-dequantizing the six block linears, picked by tensor identity
        def __getattr__(self, name):
            return getattr(F, name)

        @staticmethod
        def linear(xx, ww, bb=None):
            if id(ww) in pick:
                return F.linear(qdq(xx), qdq(ww), bb)
            return F.linear(xx, ww, bb)

    monkeypatch.setattr(olc, "F", _F())
    sim = olc.forward(*args, num_cond_latents=ncond)
    monkeypatch.setattr(olc, "F", F)
    e_bf, e_sim, e_plain = _rel(outs["bf16"], plain), _rel(outs["mxfp8"], sim), _rel(outs["mxfp8"], plain)
    print(f"[longcat] bf16 vs oracle {e_bf:.3e}; mxfp8 vs simulated-MX oracle {e_sim:.3e}, vs plain oracle {e_plain:.3e}")
    assert e_sim <= SIM_RATIO * e_plain


def test_weights_changed_requantizes():
    from worldforge_amd import dit
    cfg = dit.DiTConfig(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(36, 3, 8, 10, generator=g).to(BF).to(DEV)
    ctx, clip = torch.randn(30, 64, generator=g).to(BF).to(DEV), torch.randn(257, 1280, generator=g).to(BF).to(DEV)
    m = dit.WanTransformer3DModel(cfg, DEV, linear_precision="mxfp8").init_random(3)
    before = m.forward_tokens(x, 500.0, ctx, clip).clone()
    w = m.w["blocks.1.ffn.2.w"]
    w.mul_(-2.0)  # an in-place edit (what a LoRA fold into the same tensors does)
    assert torch.equal(m.forward_tokens(x, 500.0, ctx, clip), before)  # the fp8 copy is derived data: stale until declared
    m.weights_changed()
    after = m.forward_tokens(x, 500.0, ctx, clip).clone()
    fresh = dit.WanTransformer3DModel(cfg, DEV, linear_precision="mxfp8")
    fresh.w = {k: v.clone() for k, v in m.w.items()}
    assert not torch.equal(after, before)
    assert torch.equal(after, fresh.forward_tokens(x, 500.0, ctx, clip))


def test_cfg_pair_split_qkv_composes():
    """the CFG pair's split qkv[d:] / qkv[:d] calls on row slices of the MX weight equal the single forwards bit for bit"""
    from worldforge_amd import dit
    cfg = dit.DiTConfig(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(36, 3, 8, 10, generator=g).to(BF).to(DEV)
    ca, cb = torch.randn(30, 64, generator=g).to(BF).to(DEV), torch.randn(12, 64, generator=g).to(BF).to(DEV)
    clip = torch.randn(257, 1280, generator=g).to(BF).to(DEV)
    m = dit.WanTransformer3DModel(cfg, DEV, linear_precision="mxfp8").init_random(5)
    ra, rb = m.forward_tokens(x, 431.0, ca, clip).clone(), m.forward_tokens(x, 431.0, cb, clip).clone()
    a, b = m.forward_tokens_pair(x, 431.0, ca, cb, clip)
    assert torch.equal(a, ra) and torch.equal(b, rb)
    qkv = m._wl["blocks.0.qkv.w"]
    top = qkv[256:]
    assert top.q.data_ptr() == qkv.q.data_ptr() + 256 * 256 and top.s.shape == (512, 8)


def test_smoke_job_psnr_mxfp8():
    import __graft_entry__ as ge
    job = dict(dim=256, ffn_dim=512, heads=2, layers=2, Fr=9, H=32, Wd=32, steps=3, guide=2)
    p_bf, _ = ge.parity_run(**job)
    p_mx, err = ge.parity_run(**job, linear_precision="mxfp8")
    print(f"[smoke job] PSNR vs CPU oracle: bf16 {p_bf:.2f} dB, mxfp8 {p_mx:.2f} dB (max abs err {err:.4f})")
    assert p_mx >= 30.0, p_mx


def test_longcat_smoke_job_psnr_mxfp8():
    import __graft_entry__ as ge
    job = dict(hidden=256, heads=2, depth=2, Fr=9, H=32, Wd=32, steps=3, guide=2)
    p_bf, _ = ge.longcat_parity_run(**job)
    p_mx, err = ge.longcat_parity_run(**job, linear_precision="mxfp8")
    print(f"[longcat smoke job] PSNR vs CPU oracle: bf16 {p_bf:.2f} dB, mxfp8 {p_mx:.2f} dB (max abs err {err:.4f})")
    assert p_mx >= 30.0, p_mx
