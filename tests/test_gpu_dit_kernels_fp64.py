"""GPU: the DiT's non-attention kernels -- wf_gemm_bf16 at every GEMM call of the Wan and LongCat forwards, wf_rmsnorm_heads(_bound) with
RoPE, wf_ln_modulate, wf_act, wf_patchify / wf_unpatchify -- called one at a time through the C-ABI (or dit.gemm, with the views, strides
and epilogues the model passes) at the production shapes, against float64 CPU references of the same operation, element by element.

GEMM error model (per output element; z = x.w + b in float64, S = sum |x| |w| over the K products, U = 2^-24 the fp32 unit roundoff):
  * a bf16 x bf16 product has 16 significant bits: it is exact in fp32.  Only the fp32 accumulation errs: about K / 16 MFMA steps, each
    rounding a partial sum by <= U of its size.  The partial sums of zero-mean products are a random walk far below S and their rounding
    errors are independent, so the accumulated error stays below U S (the argument of tests/test_gpu_vae_wide_kernels.py); the bar
    allows 4x that:  c = 2^-22,  e_acc = c S.
  * the epilogue adds the bias in fp32 (one rounding):  e_v = c S + U (|z| + c S)  bounds |v - z| for the kernel's pre-epilogue v.
  * epilogue 0 (bf16 out): round to nearest bf16, <= 2^-8 of the value (8 significant bits):  bar = e_v + 2^-8 (|z| + e_v).
  * epilogue 2 (f32 out): the value is stored as it is; the bar allows two fp32 roundings:  bar = e_v + 2 U |z|.
  * epilogue 1 (GELU(tanh) to bf16): the input error propagates through |gelu'(z)| + e_v (|gelu''| <= 1 on the reals).  The kernel
    evaluates gelu = v / (1 + 2^t), t = c0 v (1 + 0.044715 v^2), c0 = -2 sqrt(2/pi) log2(e), with v_exp_f32 / v_rcp_f32 (<= 2^-22 each,
    generous for their 1-ulp accuracy).  t is formed by three fp32 roundings (<= 4 U |t|), which exp2 turns into a relative error of
    ln2 * 4 U |t| of e = 2^t; through 1 / (1 + e) that is |v| d e / (1 + e)^2, d = ln2 4 U |t| + 2^-22 -- the term that grows with
    |c0 v p|.  The reciprocal and the final product add (2^-22 + 2 U) |gelu|.  Then the bf16 rounding, 2^-8 of the value.
  * epilogue 3 (fp32 residual: out = old + gate (acc + b), gate = 1 when NULL): |gate| e_v + U |gate z| (the product) + U |old + gate z|
    (the sum).  epilogue 4 (fp32 accumulate: out = old + v): e_v + U |old + z|.
  * LongCat's _gemm_f32 (an fp32 activation a split into hi = rn_bf16(a), lo = rn_bf16(a - hi), run as epilogue 2 then 4): hi + lo
    differs from a by <= 2^-8 |a - hi| <= 2^-16 |a| per element, so <= 2^-16 S in all (a rigorous bound, no statistics), plus two
    accumulations (2 c S) and the roundings of epilogue 2 and 4 (U |z| each, and U |z| for the a - hi subtraction's reuse).
Every case checks the full rows of a row set (first and last row of every 128-row band, one random row per band, the whole ragged last
256-row tile) and the full columns of a column set (first and last column of every 64-column band, one random column per band): every
(row tile, column tile) workgroup of the 128 x 128, 256 x 256 and 256 x 320 kernels has whole rows and whole columns checked.  The
outputs are views into larger buffers (>= 64 more columns, 128 more rows) whose guard cells hold a NaN sentinel (finite values for the
read-modify-write epilogues 3 / 4) and must come back bit-identical.
Discrimination: each comparison is repeated against references that omit the last 32 products of K, the bias (where there is one) and
the gate (epilogue 3 with a gate); each must exceed the bar by >= DISCRIM: the bars can see a lost K tile, bias or gate.

wf_rmsnorm_heads (+RoPE, out_scale s): y = rn(rn(a r) w) (r = 1 / sqrt(mean(a^2) + eps) over the row's C channels), rotated by the
angles of model.py:32-39 / 478-485 (computed here in float64, NOT from dit.rope_tables), times s, then rn to bf16.  With n = a r w in
float64 (r in float64), each intermediate bf16 rounding is <= 2^-8 and r is off by e_r = (104 adds: 40 per lane, 6 wave levels, 2 waves,
sum of squares of positive terms) U / 2 + 2^-22 (rsqrt): stored y0 = n0 (1 + h), |h| <= eta = 2^-7 + 2^-15 + e_r + U.  The rotation re =
y0 cos - y1 sin in fp32 from fp32 tables (<= U each) carries (eta + 4 U)(1 + eta) P, P = |n0 cos| + |n1 sin|; the scale U, the final
rounding 2^-8 (|ref| + that):  bar = s (eta + 5 U)(1 + eta) P + 2^-8 (|ref| + s (eta + 5 U)(1 + eta) P).
The bound of wf_rmsnorm_heads_bound is the max over rows of |stored row of a head|^2, an fp32 sum of 128 positive squares (16 adds deep):
|got - ref| <= 16 U ref.  Discrimination: references with the h and w positions swapped and with the RMS over the head's 128 channels
instead of the row must each exceed the bar by >= DISCRIM.
wf_ln_modulate (two-pass fp32 statistics over C = 5120, rows with a common offset mu0 = 10^3 over unit spread): the mean's fp32 sum of
positive terms is at most 17 adds deep (5 per thread, 6 wave levels, 4 waves, plus the in-vector adds): |d mu| <= 17 U mean|x|; the
centred values carry d mu + U |x - mu|; the variance (17 adds, positive terms) 17 U var + d mu^2, so |d r| / r <= (17 U + d mu^2 / var) / 2
+ 2^-22 (rsqrt); the modulation 4 U |y|; the bf16 output 2^-8 (|y| + ...).
wf_act: SiLU v / (1 + e^-v) (__expf: exp2(v log2e), relative |v| U + 2^-22; the division 2^-22), GELU(erf) 0.5 v (1 + erf(v / sqrt2))
(erff <= 2^-22 |erf| + the argument's rounding through erf'), the sum a + b (U); then the output rounding (bf16 2^-8, fp32 U).
The measured max(|err| / bar) of every case goes through tests._tol.within."""
import math

import numpy as np
import pytest
import torch

from tests._tol import within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24
C_ACC = 2.0 ** -22
U_BF = 2.0 ** -8
DISCRIM = 8.0            # a perturbed reference (dropped K tail, bias, gate, swapped RoPE axes, per-head RMS) must exceed the bar by this
KTAIL = 32               # products of K the "lost K tile" reference omits
SENT16 = 0x7FA5          # NaN bit pattern (bf16) of the guard cells of 16-bit outputs
SENT32 = 0x7FC0A5A5      # NaN bit pattern (fp32) of the guard cells of fp32 outputs
OLD_GUARD = -3.25        # finite guard value of the read-modify-write epilogues
EPI_BF16, EPI_GELU, EPI_F32, EPI_RESID, EPI_ACC = 0, 1, 2, 3, 4
D, F_WAN, F_PAD = 5120, 13824, 14080          # Wan dim, FFN features, FFN-up rows as stored (dit.ffn_padded_features)
C2, C3 = (21, 30, 52), (21, 45, 80)           # latent token grids (frames, H / 2, W / 2) of configs 2 and 3
L_C2, L_C3 = 21 * 30 * 52, 21 * 45 * 80       # 32 760, 75 600


def _n_cu():
    """The device's CU count (pp_wide's input).  Case ids are made at collection for a 256-CU MI355X (no GPU is opened then); each case
    asserts the device agrees."""
    return torch.cuda.get_device_properties(0).multi_processor_count


def gemm_kernel(M, N, K, ldx, ldw, n_cu):
    """gemm_impl's `big` gate and pp_wide (csrc/gemm.hip), in Python: which kernel a wf_gemm_bf16 call runs."""
    big = (K % 64 == 0 and M >= 1024 and N >= 256 and N % 4 == 0 and M * N >= (1 << 22) and M * ldx * 2 < (1 << 32)
           and N * ldw * 2 < (1 << 32))
    if not big:
        return "k_gemm"
    if N % 320:
        return "pp256"
    mt = -(-M // 256)
    t256, t320 = mt * -(-N // 256), mt * (N // 320)
    r256, r320 = -(-t256 // n_cu), -(-t320 // n_cu)
    return "pp320" if r320 * 320 <= r256 * 256 else "pp256"


def _shard(L, P=8, rank=7):
    from worldforge_amd.parallel import shard_plan
    return shard_plan(L, P).bounds(rank)


_S2 = _shard(L_C2)              # the last (ragged) rank of an 8-rank C2 job: 4 088 tokens
_S3 = _shard(L_C3)              # ... of C3: 9 296 tokens
M_S2, M_S3 = _S2[1] - _S2[0], _S3[1] - _S3[0]

# name: (M, N, K, epilogue, options).  x: "ffn_up" = FFN-down reads FFN-up's GELU output through the padded row stride (as in the layer);
# split: the Q / KV calls of the sequence-parallel layer (W row slice, output column slice, ldo = 3 d); pad: FFN-up's zero weight rows
GEMM_CASES = {
    "wan_qkv": (L_C2, 3 * D, D, EPI_BF16, {}),
    "wan_q_split": (L_C2, D, D, EPI_BF16, dict(split=(0, D))),
    "wan_kv_split": (L_C2, 2 * D, D, EPI_BF16, dict(split=(D, 3 * D))),
    "wan_self_o_gated": (L_C2, D, D, EPI_RESID, dict(gate=True)),
    "wan_cross_o_nogate": (L_C2, D, D, EPI_RESID, {}),
    "wan_ffn0": (L_C2, F_PAD, D, EPI_GELU, dict(pad=F_WAN)),
    "wan_ffn2": (L_C2, D, F_WAN, EPI_RESID, dict(gate=True, x="ffn_up")),
    "wan_patch": (L_C2, D, 144, EPI_F32, {}),
    "wan_head": (L_C2, 64, D, EPI_F32, {}),
    "wan_cross_kv_text": (512, 2 * D, D, EPI_BF16, {}),
    "wan_cross_kv_img": (257, 2 * D, D, EPI_BF16, {}),
    "wan_text_emb0": (512, D, 4096, EPI_GELU, {}),
    "wan_text_emb2": (512, D, D, EPI_BF16, {}),
    "wan_time_proj": (1, 6 * D, D, EPI_F32, {}),
    "s8_qkv": (M_S2, 3 * D, D, EPI_BF16, {}),
    "s8_ffn0": (M_S2, F_PAD, D, EPI_GELU, dict(pad=F_WAN)),
    "s8_ffn2": (M_S2, D, F_WAN, EPI_RESID, dict(gate=True, x="ffn_up")),
    "c3_ffn0": (L_C3, F_PAD, D, EPI_GELU, dict(pad=F_WAN)),
    "c3_ffn2": (L_C3, D, F_WAN, EPI_RESID, dict(gate=True, x="ffn_up")),
    "c3s8_ffn0": (M_S3, F_PAD, D, EPI_GELU, dict(pad=F_WAN)),
    "lc_qkv": (37440, 3 * 4096, 4096, EPI_BF16, {}),
    "lc_w13": (37440, 22016, 4096, EPI_BF16, dict(bias=False)),
    "lc_w2": (37440, 4096, 11008, EPI_BF16, dict(bias=False)),
    "lc_proj": (37440, 4096, 4096, EPI_BF16, {}),
    # epilogue 4 (fp32 accumulate) on the 320-wide tile and on the 128 x 128 kernel
    "acc_pp320": (L_C2, D, D, EPI_ACC, {}),
    "acc_kgemm": (512, D, 4096, EPI_ACC, {}),
}
N_CU_ID = 256


def _ldx(name):
    M, N, K, epi, o = GEMM_CASES[name]
    return F_PAD if o.get("x") == "ffn_up" else K


def _kind(name, n_cu=N_CU_ID):
    M, N, K, epi, o = GEMM_CASES[name]
    ldw = D if o.get("split") else K
    return gemm_kernel(M, N, K, _ldx(name), ldw, n_cu)


# the epilogues production runs on each kernel (dit.py, longcat_dit.py at the table's shapes), which the table must reach
PRODUCTION_EPIS = {"k_gemm": {EPI_BF16, EPI_GELU, EPI_F32, EPI_ACC}, "pp256": {EPI_BF16, EPI_GELU}, "pp320": {EPI_BF16, EPI_GELU, EPI_RESID}}
_GUARDS = {"calls": 0, "checked": 0}


def test_gemm_table_reaches_every_kernel_and_epilogue():
    """The table covers k_gemm, the 256-wide and the 320-wide ping-pong tile, each with every epilogue production runs on it (on this
    device's CU count: pp_wide depends on it), plus epilogue 4 on pp320."""
    seen = {}
    for name, (M, N, K, epi, o) in GEMM_CASES.items():
        seen.setdefault(_kind(name, _n_cu()), set()).add(epi)
    for kind, epis in PRODUCTION_EPIS.items():
        assert epis <= seen.get(kind, set()), f"{kind}: table reaches epilogues {seen.get(kind)}, production uses {epis}"
    assert EPI_ACC in seen["pp320"]


def _rows_set(M, rng):
    s = set()
    for b0 in range(0, M, 128):
        b1 = min(b0 + 128, M)
        s.update((b0, b1 - 1, int(rng.integers(b0, b1))))
    s.update(range((M - 1) // 256 * 256, M))
    return sorted(s)


def _cols_set(N, rng):
    s = set()
    for b0 in range(0, N, 64):
        b1 = min(b0 + 64, N)
        s.update((b0, b1 - 1, int(rng.integers(b0, b1))))
    return sorted(s)


def _randn(shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV, dtype=F32) * scale).to(dtype)


def _gelu64(z):
    return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def _gelu64_d(z):
    k = math.sqrt(2.0 / math.pi)
    t = torch.tanh(k * (z + 0.044715 * z ** 3))
    return 0.5 * (1.0 + t) + 0.5 * z * (1.0 - t * t) * k * (1.0 + 3 * 0.044715 * z * z)


def _epi(epi, z, old, gate):
    """The epilogue applied in float64 to the pre-epilogue value z (= x.w + b)."""
    if epi == EPI_GELU:
        return _gelu64(z)
    if epi == EPI_RESID:
        return old + (z if gate is None else gate * z)
    if epi == EPI_ACC:
        return old + z
    return z


def gemm_bar(epi, z, S, old, gate):
    """The module docstring's per-element bar."""
    ev = C_ACC * S + U * (z.abs() + C_ACC * S)
    if epi == EPI_BF16:
        return ev + U_BF * (z.abs() + ev) + 1e-30
    if epi == EPI_F32:
        return ev + 2 * U * z.abs() + 1e-30
    if epi == EPI_GELU:
        g = _gelu64(z).abs()
        t = -2.0 * math.sqrt(2.0 / math.pi) * math.log2(math.e) * z * (1.0 + 0.044715 * z * z)
        d = math.log(2.0) * 4 * U * t.abs() + 2.0 ** -22
        s = torch.sigmoid(-t * math.log(2.0))                       # 1 / (1 + e), e = 2^t
        eg = z.abs() * d * s * (1.0 - s) + g * (2.0 ** -22 + 2 * U)
        pre = (_gelu64_d(z).abs() + ev) * ev + eg
        return pre + U_BF * (g + pre) + 1e-30
    if epi == EPI_RESID:
        ga = 1.0 if gate is None else gate.abs()
        gz = z if gate is None else gate * z
        return ga * ev + U * gz.abs() + U * (old + gz).abs() + 1e-30
    return ev + U * (old + z).abs() + 1e-30


def _ratio(got, ref, bar):
    return ((got - ref).abs() / bar).max().item()


class _Ref:
    """float64 reference pieces of one checked set: z = x.w + b, S = |x|.|w|, tail = the last KTAIL products."""

    def __init__(self):
        self.z, self.S, self.tail = [], [], []

    def add(self, x64, w64, b64):
        self.z.append(x64 @ w64.T + (b64 if b64 is not None else 0.0))
        self.S.append(x64.abs() @ w64.abs().T)
        self.tail.append(x64[:, -KTAIL:] @ w64[:, -KTAIL:].T)

    def cat(self):
        return torch.cat(self.z), torch.cat(self.S), torch.cat(self.tail)


def _guard_fill(shape, epi):
    if epi in (EPI_RESID, EPI_ACC):
        return torch.full(shape, OLD_GUARD, dtype=F32, device=DEV)
    if epi in (EPI_BF16, EPI_GELU):
        return torch.full(shape, SENT16, dtype=torch.int16, device=DEV).view(BF)
    return torch.full(shape, SENT32, dtype=torch.int32, device=DEV).view(F32)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _ffn_up_output(M, seed):
    """FFN-up into the padded [M, 14 080] buffer, as the layer computes it: FFN-down's X is its first 13 824 columns."""
    from worldforge_amd import dit
    h = _randn((M, D), seed)
    w = _randn((F_PAD, D), seed + 1, 1.0 / math.sqrt(D))
    b = _randn((F_PAD,), seed + 2, 0.1, F32)
    w[F_WAN:] = 0
    b[F_WAN:] = 0
    ffh = torch.empty((M, F_PAD), dtype=BF, device=DEV)
    dit.gemm(h, w, b, ffh, EPI_GELU)
    return ffh


@pytest.mark.parametrize("name", list(GEMM_CASES), ids=[f"{n}-{_kind(n)}-epi{GEMM_CASES[n][3]}" for n in GEMM_CASES])
def test_gemm_bf16_vs_fp64(name):
    from worldforge_amd import dit
    M, N, K, epi, o = GEMM_CASES[name]
    seed = 1000 + 10 * sorted(GEMM_CASES).index(name)
    rng = np.random.default_rng(seed)
    assert K >= 100                                                    # the accumulation model's K
    kind = _kind(name)
    assert _kind(name, _n_cu()) == kind, f"{name}: this device ({_n_cu()} CUs) runs {_kind(name, _n_cu())}, the case id says {kind}"
    # operands
    if o.get("x") == "ffn_up":
        x = _ffn_up_output(M, seed + 5)[:, :K]                         # ldx = 14 080
        assert x.stride(0) == F_PAD
    else:
        x = _randn((M, K), seed)
    if o.get("split"):
        wfull = _randn((3 * D, K), seed + 1, 1.0 / math.sqrt(K))
        bfull = _randn((3 * D,), seed + 2, 0.1, F32)
        s0, s1 = o["split"]
        w, b = wfull[s0:s1], bfull[s0:s1]
    else:
        w = _randn((N, K), seed + 1, 1.0 / math.sqrt(K))
        b = _randn((N,), seed + 2, 0.1, F32) if o.get("bias", True) else None
    if o.get("pad"):
        w[o["pad"]:] = 0
        b[o["pad"]:] = 0
    gate = _randn((N,), seed + 3, 0.5, F32) + 0.25 if o.get("gate") else None
    # the output: a view into a guard-filled buffer (the split calls: a column slice of [M, 3 d] with ldo = 3 d, as the layer passes it)
    if o.get("split"):
        c0, width = o["split"][0], 3 * D
    else:
        c0, width = 0, N + 64
    buf = _guard_fill((M + 128, width), epi)
    out = buf[:M, c0:c0 + N]
    if epi in (EPI_RESID, EPI_ACC):   # an fp32 residual with a row-dependent offset of tens: the add is not negligible
        rows_off = 10.0 + 40.0 * torch.arange(M, device=DEV, dtype=F32)[:, None] / max(M, 1)
        out.copy_(rows_off + _randn((M, N), seed + 4, 1.0, F32))
    snap = buf.clone()
    _GUARDS["calls"] += 1
    dit.gemm(x, w, b, out, epi, gate=gate)
    torch.cuda.synchronize()
    assert out.stride(0) == width and (o.get("split") is None or width > N)
    gb, gs = _bits(buf), _bits(snap)
    assert torch.equal(gb[M:], gs[M:]), f"{name}: the guard rows below the output were written"
    assert torch.equal(gb[:M, c0 + N:], gs[:M, c0 + N:]), f"{name}: the guard columns right of the output were written"
    if c0:
        assert torch.equal(gb[:M, :c0], gs[:M, :c0]), f"{name}: the columns left of the output were written"
    _GUARDS["checked"] += 1
    del gb, gs
    # float64 references of the row set (all N columns) and the column set (all M rows, in row chunks)
    rows, cols = _rows_set(M, rng), _cols_set(N, rng)
    w64 = w.cpu().to(F64)
    b64 = b.cpu().to(F64) if b is not None else None
    g64 = gate.cpu().to(F64) if gate is not None else None
    rr, rc = _Ref(), _Ref()
    ridx = torch.tensor(rows, device=DEV)
    rr.add(x[ridx].cpu().to(F64), w64, b64)
    cidx = torch.tensor(cols)
    wc64, bc64 = w64[cidx], (b64[cidx] if b64 is not None else None)
    CH = max(1, (1 << 26) // K)
    for r0 in range(0, M, CH):
        rc.add(x[r0:r0 + CH].cpu().to(F64), wc64, bc64)
    del w64
    got_r = out[ridx].cpu().to(F64)
    got_c = out[:, cidx.to(DEV)].cpu().to(F64)
    old_r = snap[:M, c0:c0 + N][ridx].cpu().to(F64) if epi in (EPI_RESID, EPI_ACC) else None
    old_c = snap[:M, c0:c0 + N][:, cidx.to(DEV)].cpu().to(F64) if epi in (EPI_RESID, EPI_ACC) else None
    del snap, buf
    checks = [(got_r, *rr.cat(), old_r, g64, b64), (got_c, *rc.cat(), old_c, g64[cidx] if g64 is not None else None, bc64)]
    worst, disc = 0.0, {"k_tail": math.inf, "bias": math.inf, "gate": math.inf}
    for got, z, S, tail, old, g, bb in checks:
        assert torch.isfinite(got).all()
        bar = gemm_bar(epi, z, S, old, g)
        worst = max(worst, _ratio(got, _epi(epi, z, old, g), bar))
        disc["k_tail"] = min(disc["k_tail"], _ratio(got, _epi(epi, z - tail, old, g), bar))
        if bb is not None:
            disc["bias"] = min(disc["bias"], _ratio(got, _epi(epi, z - bb, old, g), bar))
        if g is not None:
            disc["gate"] = min(disc["gate"], _ratio(got, _epi(epi, z, old, None), bar))
    within(f"dit_gemm.{name}.{kind}.epi{epi}", worst, 1.0)
    print(f"[discrim] dit_gemm.{name}: " + ", ".join(f"{k} {v:.3g}" for k, v in disc.items() if v != math.inf))
    for what, r in disc.items():
        if r != math.inf:
            assert r >= DISCRIM, f"{name}: reference without the {what}: max err / bar = {r:.2f} < {DISCRIM}: the bar cannot see it"
    assert _GUARDS["checked"] == _GUARDS["calls"]


def test_longcat_gemm_f32_hi_lo_pair_vs_fp64():
    """LongCat's _gemm_f32 (the adaLN projections: T = 24 latent frames, K = 512 -> 2 C = 8192): an fp32 activation split into a bf16
    hi / lo pair, run as epilogue 2 then epilogue 4 on the 128 x 128 kernel, against the fp32 activation in float64.  Dropping the lo
    GEMM must fail the bar."""
    from worldforge_amd.longcat_dit import LongCatVideoTransformer3DModel
    M, N, K = 24, 8192, 512
    assert gemm_kernel(M, N, K, K, K, _n_cu()) == "k_gemm"
    a = _randn((M, K), 77, 1.0, F32) * 3.0
    w = _randn((N, K), 78, 1.0 / math.sqrt(K))
    b = _randn((N,), 79, 0.1, F32)
    buf = _guard_fill((M + 128, N + 64), EPI_F32)
    out = buf[:M, :N]
    snap = buf.clone()
    LongCatVideoTransformer3DModel._gemm_f32(None, a, w, b, out)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf[M:]), _bits(snap[M:])) and torch.equal(_bits(buf[:M, N:]), _bits(snap[:M, N:]))
    a64, w64, b64 = a.cpu().to(F64), w.cpu().to(F64), b.cpu().to(F64)
    z = a64 @ w64.T + b64
    S = a64.abs() @ w64.abs().T
    bar = (2.0 ** -16 + 2 * C_ACC) * S + 3 * U * z.abs() + 1e-30
    got = out.cpu().to(F64)
    within("dit_gemm.lc_gemm_f32.hi_lo", _ratio(got, z, bar), 1.0)
    z_hi = a.to(BF).cpu().to(F64) @ w64.T + b64                    # the hi GEMM alone: one bf16 term of a
    r = _ratio(got, z_hi, bar)
    assert r >= DISCRIM, f"without the lo GEMM: max err / bar = {r:.2f} < {DISCRIM}"
    r = _ratio(got, z - b64, bar)
    assert r >= DISCRIM, f"without the bias: max err / bar = {r:.2f} < {DISCRIM}"


# ---- 2. the per-token producers --------------------------------------------------------------------------------------------------------
def rope_angles64(f, h, w, swap_hw=False):
    """model.py:32-39 (rope_params: 1 / 10000^(2i / dim) per axis, dim = 128 - 4 (128 // 6) = 44 for frames, 2 (128 // 6) = 42 for h and w)
    and 478-485 (the 64 pairs are [22 frame | 21 h | 21 w] and token (t, y, x) takes angle pos * freq), in float64: [f h w, 64]."""
    c = 64
    dhw = c // 3
    df = c - 2 * dhw

    def freqs(npairs):
        dim = 2 * npairs
        return 1.0 / torch.pow(torch.tensor(10000.0, dtype=F64), torch.arange(0, dim, 2, dtype=F64) / dim)

    t, y, x = torch.meshgrid(torch.arange(f, dtype=F64), torch.arange(h, dtype=F64), torch.arange(w, dtype=F64), indexing="ij")
    t, y, x = t.reshape(-1, 1), y.reshape(-1, 1), x.reshape(-1, 1)
    if swap_hw:
        y, x = x, y
    return torch.cat([t * freqs(df), y * freqs(dhw), x * freqs(dhw)], dim=1)


def _heads_ref(a64, w64, ang, s, eps, per_head=False):
    """float64 RMSNorm over the row (or, discriminating, over each head's 128 channels) + RoPE + scale: [rows, H, 128] and the P terms."""
    R, C = a64.shape
    H = C // 128
    if per_head:
        ah = a64.view(R, H, 128)
        n = (ah / torch.sqrt((ah * ah).mean(-1, keepdim=True) + eps)).reshape(R, C) * w64
    else:
        n = a64 / torch.sqrt((a64 * a64).mean(-1, keepdim=True) + eps) * w64
    n = n.view(R, H, 64, 2)
    cs, sn = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]
    n0, n1 = n[..., 0], n[..., 1]
    re, im = n0 * cs - n1 * sn, n0 * sn + n1 * cs
    P_re, P_im = (n0 * cs).abs() + (n1 * sn).abs(), (n0 * sn).abs() + (n1 * cs).abs()
    ref = torch.stack([re, im], -1).view(R, H, 128) * s
    P = torch.stack([P_re, P_im], -1).view(R, H, 128)
    return ref, P


HEAD_CASES = {
    "c2_q": (C2, None, "q"), "c2_k": (C2, None, "k"),
    "c3_q": (C3, None, "q"), "c3_k": (C3, None, "k"),
    "c2_rank7of8_q": (C2, _S2, "q"), "c2_rank7of8_k": (C2, _S2, "k"),
}


@pytest.mark.parametrize("bound", [False, True], ids=["plain", "bound"])
@pytest.mark.parametrize("case", list(HEAD_CASES))
def test_rmsnorm_heads_rope_vs_fp64(case, bound):
    """wf_rmsnorm_heads(_bound) on the self-attention Q (out_scale = log2(e) / sqrt(128)) or K (1.0) column block of a [L, 3 d] qkv
    buffer, with the RoPE tables the model passes (dit.rope_tables; a shard passes its rows), into a destination with 64 pre-filled rows
    past L.  Heads carry different scales (0.5 ... 2), as projected heads do."""
    from worldforge_amd import _ffi, dit, ops
    (f, h, w), shard, which = HEAD_CASES[case]
    Lfull = f * h * w
    lo, hi = shard if shard is not None else (0, Lfull)
    L, H, eps = hi - lo, D // 128, 1e-6
    s = 1.4426950408889634 / math.sqrt(128.0) if which == "q" else 1.0
    col0 = 0 if which == "q" else D
    seed = 500 + sorted(HEAD_CASES).index(case)
    hscale = 2.0 ** torch.linspace(-1.0, 1.0, H, device=DEV, dtype=F32).repeat_interleave(128)
    qkv = (_randn((L, 3 * D), seed, 1.0, F32) * torch.cat([hscale, hscale, torch.ones(D, device=DEV)])).to(BF)
    weight = 1.0 + _randn((D,), seed + 1, 0.1, F32)
    cos, sin = dit.rope_tables(128, f, h, w)
    cos, sin = cos[lo:hi].to(DEV), sin[lo:hi].to(DEV)
    Lout = L + 64
    out = torch.full((H, Lout, 128), SENT16, dtype=torch.int16, device=DEV).view(BF)
    view = qkv[:, col0:col0 + D]
    if bound:
        ws = torch.empty((int(_ffi.lib().wf_rmsnorm_heads_bound_ws_floats(L, D)),), dtype=F32, device=DEV)
        mx = torch.full((H,), float("nan"), dtype=F32, device=DEV)
        _ffi.call("wf_rmsnorm_heads_bound", view.data_ptr(), qkv.stride(0), weight.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                  out.data_ptr(), L, Lout, D, float(eps), float(s), ws.data_ptr(), mx.data_ptr(), ops.stream())
    else:
        _ffi.call("wf_rmsnorm_heads", view.data_ptr(), qkv.stride(0), weight.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                  out.data_ptr(), L, Lout, D, float(eps), float(s), ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(out[:, L:].view(torch.int16), torch.full_like(out[:, L:].view(torch.int16), SENT16)), "rows >= L were written"
    # every 4th row plus the whole first and last frame of the grid or shard: every position of every axis is reached
    rows = torch.unique(torch.cat([torch.arange(0, L, 4), torch.arange(0, min(L, h * w)), torch.arange(max(0, L - h * w), L)]))
    ang_all, ang_sw = rope_angles64(f, h, w), rope_angles64(f, h, w, swap_hw=True)
    e_r = 104 * U / 2 + 2.0 ** -22
    eta = 2.0 ** -7 + 2.0 ** -15 + e_r + U
    w64 = weight.cpu().to(F64)
    worst = 0.0
    norm2 = torch.zeros(H, dtype=F64)
    CH = 8192
    for i0 in range(0, len(rows), CH):
        ri = rows[i0:i0 + CH]
        a64 = view[ri.to(DEV)].cpu().to(F64)
        got = out[:, ri.to(DEV)].cpu().to(F64).permute(1, 0, 2)          # [rows, H, 128]
        assert torch.isfinite(got).all()
        ref, P = _heads_ref(a64, w64, ang_all[lo + ri], s, eps)
        rop = s * (eta + 5 * U) * (1 + eta) * P
        bar = rop + U_BF * (ref.abs() + rop) + 1e-30
        worst = max(worst, _ratio(got, ref, bar))
        if i0 == 0:   # the discriminating references on the first chunk (the first frame and more: every h and w position)
            d_swap = _ratio(got, _heads_ref(a64, w64, ang_sw[lo + ri], s, eps)[0], bar)
            d_head = _ratio(got, _heads_ref(a64, w64, ang_all[lo + ri], s, eps, per_head=True)[0], bar)
    within(f"dit_heads.{case}.{'bound' if bound else 'plain'}", worst, 1.0)
    print(f"[discrim] dit_heads.{case}: hw_swap {d_swap:.3g}, head_rms {d_head:.3g}")
    assert d_swap >= DISCRIM, f"h / w positions swapped: max err / bar = {d_swap:.2f} < {DISCRIM}"
    assert d_head >= DISCRIM, f"RMS over the head's 128 channels: max err / bar = {d_head:.2f} < {DISCRIM}"
    if bound:   # the bound is a max over every row: all rows of the output are read for its reference
        for r0 in range(0, L, CH):
            got = out[:, r0:min(r0 + CH, L)].cpu().to(F64)
            norm2 = torch.maximum(norm2, (got * got).sum(-1).max(1).values)
        got_b = mx.cpu().to(F64)
        rel = ((got_b - norm2).abs() / norm2).max().item()
        assert rel <= 16 * U, f"bound: max relative deviation from the float64 max of the stored rows' |row|^2 = {rel:.3e} > 16 U"


@pytest.mark.parametrize("mode", ["adaln_bf16", "affine_f32"])
def test_ln_modulate_vs_fp64(mode):
    """wf_ln_modulate at L = 32 760, C = 5120, as the layer calls it: AdaLN (plus_one = 1, mul / add = the modulation rows) to bf16, and
    the affine form (plus_one = 0, weight / bias) to fp32.  Every row carries an offset of 10^3 over unit spread: the centred second
    pass is what keeps the variance."""
    from worldforge_amd import _ffi, ops
    from worldforge_amd._ffi import WF_BF16, WF_F32
    L, C, eps = L_C2, D, 1e-6
    mu0 = 1000.0
    x = mu0 + _randn((L, C), 61, 1.0, F32) + _randn((L, 1), 62, 1.0, F32)
    if mode == "adaln_bf16":
        mul, add, p1, odt, od = _randn((C,), 63, 0.1, F32), _randn((C,), 64, 0.1, F32), 1.0, BF, WF_BF16
    else:
        mul, add, p1, odt, od = 1.0 + _randn((C,), 63, 0.1, F32), _randn((C,), 64, 0.1, F32), 0.0, F32, WF_F32
    out = torch.empty((L, C), dtype=odt, device=DEV)
    _ffi.call("wf_ln_modulate", x.data_ptr(), mul.data_ptr(), add.data_ptr(), out.data_ptr(), od, L, C, float(eps), int(p1), ops.stream())
    torch.cuda.synchronize()
    m64, a64 = mul.cpu().to(F64), add.cpu().to(F64)
    worst = 0.0
    for r0 in range(0, L, 4096):
        x64 = x[r0:r0 + 4096].cpu().to(F64)
        mu = x64.mean(-1, keepdim=True)
        xc = x64 - mu
        var = (xc * xc).mean(-1, keepdim=True)
        r = 1.0 / torch.sqrt(var + eps)
        sc = p1 + m64
        ref = xc * r * sc + a64
        dmu = 17 * U * x64.abs().mean(-1, keepdim=True)
        dr = (17 * U + dmu * dmu / var) / 2 + 2.0 ** -22
        pre = (r * sc).abs() * (dmu + U * xc.abs()) + (xc * r * sc).abs() * (dr + 3 * U) + U * ref.abs()
        bar = pre + (U_BF * (ref.abs() + pre) if odt == BF else U * ref.abs()) + 1e-30
        got = out[r0:r0 + 4096].cpu().to(F64)
        assert torch.isfinite(got).all()
        worst = max(worst, _ratio(got, ref, bar))
    within(f"dit_ln_modulate.{mode}", worst, 1.0)


ACT_CASES = {
    "silu_f32_bf16": (0, F32, None, BF),        # SiLU of the time embedding (dit.py _embed_condition) into the next GEMM's bf16 operand
    "silu_f32_f32": (0, F32, None, F32),        # LongCat's t_embedder / adaLN SiLU (longcat_dit.py _act)
    "gelu_f32_bf16": (1, F32, None, BF),        # GELU(erf) of the image embedding MLP
    "sum_f32_f32": (2, F32, F32, F32),          # e = modulation + e0 (every layer), head modulation
}


@pytest.mark.parametrize("n", [6 * D, 6 * D - 36], ids=["n30720", "n30684"])
@pytest.mark.parametrize("case", list(ACT_CASES))
def test_act_vs_fp64(case, n):
    from worldforge_amd import _ffi, ops
    from worldforge_amd._ffi import WF_BF16, WF_F32
    mode, ta, tb, to = ACT_CASES[case]
    dt = {F32: WF_F32, BF: WF_BF16}
    a = _randn((n + 64,), 71, 4.0, ta)
    b = _randn((n + 64,), 72, 1.0, tb) if tb is not None else None
    out = _guard_fill((n + 64,), EPI_BF16 if to == BF else EPI_F32)
    _ffi.call("wf_act", a.data_ptr(), dt[ta], b.data_ptr() if b is not None else None, dt[tb] if b is not None else 0, out.data_ptr(),
              dt[to], mode, n, ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[n:]), _bits(_guard_fill((64,), EPI_BF16 if to == BF else EPI_F32))), "elements >= n were written"
    v = a[:n].cpu().to(F64)
    got = out[:n].cpu().to(F64)
    if mode == 0:
        ref = v * torch.sigmoid(v)
        ea = (v.abs() * U + 2.0 ** -22) * torch.sigmoid(-v) + 2.0 ** -22 + 2 * U   # exp argument and __expf through e / (1 + e); division, add
        pre = ref.abs() * ea
    elif mode == 1:
        ref = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
        derf = 2.0 / math.sqrt(math.pi) * torch.exp(-v * v / 2)
        pre = 0.5 * v.abs() * (2.0 ** -22 * torch.erf(v / math.sqrt(2.0)).abs() + 2 * U * (v.abs() / math.sqrt(2.0)) * derf) + 3 * U * ref.abs()
    else:
        b64 = b[:n].cpu().to(F64)
        ref = v + b64
        pre = torch.zeros_like(ref)
    bar = pre + (U_BF * (ref.abs() + pre) if to == BF else U * (ref.abs() + pre)) + 1e-30
    within(f"dit_act.{case}", _ratio(got, ref, bar), 1.0)


def test_patchify_unpatchify_c2_bit_exact():
    """wf_patchify at the C2 latent (36 channels x 21 x 60 x 104 -> [32 760, 144]) and wf_unpatchify of the 16-channel head output, bit
    for bit against the view / permute forms of model.py:534-537 and 584-607."""
    from worldforge_amd import _ffi, ops
    Cin, Cout, T, Hh, Ww = 36, 16, 21, 60, 104
    h2, w2 = Hh // 2, Ww // 2
    L = T * h2 * w2
    x = _randn((Cin, T, Hh, Ww), 81)
    tok = torch.full((L + 64, Cin * 4), SENT16, dtype=torch.int16, device=DEV).view(BF)
    _ffi.call("wf_patchify", x.data_ptr(), tok.data_ptr(), Cin, T, Hh, Ww, ops.stream())
    want = x.view(Cin, T, h2, 2, w2, 2).permute(1, 2, 4, 0, 3, 5).reshape(L, Cin * 4)
    torch.cuda.synchronize()
    assert torch.equal(tok[:L].view(torch.int16), want.view(torch.int16))
    assert torch.equal(tok[L:].view(torch.int16), torch.full_like(tok[L:].view(torch.int16), SENT16))
    y = _randn((L, 4 * Cout), 82, 1.0, F32)
    out = torch.full((Cout * T * Hh * Ww + 64,), SENT32, dtype=torch.int32, device=DEV).view(F32)
    _ffi.call("wf_unpatchify", y.data_ptr(), out.data_ptr(), Cout, T, Hh, Ww, ops.stream())
    want = y.view(T, h2, w2, 2, 2, Cout).permute(5, 0, 1, 3, 2, 4).reshape(-1)
    torch.cuda.synchronize()
    n = want.numel()
    assert torch.equal(out[:n].view(torch.int32), want.view(torch.int32))
    assert torch.equal(out[n:].view(torch.int32), torch.full_like(out[n:].view(torch.int32), SENT32))
