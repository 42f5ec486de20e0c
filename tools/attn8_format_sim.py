"""CPU simulation of the proposed 8-bit self-attention format (INT8 Q K^T, e4m3 P, MX-e4m3 V^T) against fp64 attention -- the go / no-go
measurement of DESIGN.md section 4e.  No GPU, no kernel: the format only.

Format: Q8 / K8 = per-row INT8 with s = amax / 127 in fp32 (K about the per-head mean of its valid rows: softmax is invariant to it), scores
sq sk int32(q8 . k8), P = exp2(s - m) with the final row max, rounded to e4m3 as rne(P * 256), the row sum on the unrounded P, V as OCP
MX-e4m3 with one E8M0 scale per 32 consecutive keys of a channel (what wf_mx_quant_e4m3 writes for the V^T tiles).  Everything else fp64.

Usage:  python tools/attn8_format_sim.py        prints rel-L2 errors of the attention output for each rounding alone and all together
"""
import torch

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
QSCALE = 128.0 ** -0.5 * 1.4426950408889634  # softmax_scale * log2(e): what the Q producers fold in
MX_QKV_GAIN3 = 9.1e-2                        # Q, K, V as MX-e4m3 with exact P at q gain 3 (the alternative format)


# ---- the format, restated (CPU, fp64 apart from the roundings) --------------------------------------------------------------------------
def ref_quant_rows(x: torch.Tensor, L: int, mean=None):
    """x bf16 [H, Lp, 128] -> (int8 [H, Lp, 128], f32 [H, Lp]): the row formula above in fp32 with IEEE division."""
    f = x.float()
    if mean is not None:
        f = f - mean.float()[:, None, :]
    finite = torch.isfinite(f).all(-1)
    amax = torch.where(finite, f.abs().amax(-1), torch.zeros(()))
    s = amax / 127.0
    q = torch.clamp(torch.round(f / s[..., None]), -127.0, 127.0)
    ok = finite & (amax > 0)
    q = torch.where(ok[..., None], q, torch.zeros(()))
    s = torch.where(finite, s, torch.full((), float("nan")))
    q[:, L:], s[:, L:] = 0.0, 0.0
    return q.to(torch.int8), s


def mx_qdq_keys(v: torch.Tensor, on: bool = True) -> torch.Tensor:
    """v f64 [Lkp, 128] (rows = keys, Lkp % 32 == 0) -> its MX-e4m3 value: one scale 2^e per 32 consecutive keys of a channel, e the
    smallest integer with amax / 2^e <= 448 (wf_mx_quant_e4m3), elements rounded to nearest even."""
    if not on:
        return v.clone()
    b = v.reshape(-1, 32, v.shape[1])
    amax = b.abs().amax(1, keepdim=True)
    e = torch.ceil(torch.log2(torch.clamp(amax, min=1e-300) / 448.0)).clamp(-127, 127)
    e = torch.where(amax > 0, e, torch.full_like(e, -127.0))
    sc = torch.exp2(e)
    return ((b / sc).float().to(F8).double() * sc).reshape(v.shape)


def exact_attention(q, k, v, kv_len):
    """fp64 softmax2(q k^T) v over the first kv_len keys (q pre-scaled: exp2 domain)."""
    s = q.double() @ k.double()[:kv_len].T
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return (p @ v.double()[:kv_len]) / p.sum(-1, keepdim=True)


def sim_attention(q, k, v, kv_len, round_qk=True, round_p=True, round_v=True):
    """q [Lq, 128], k / v [Lkp, 128] (bf16 values; rows >= kv_len of k and v zero) -> (sim, exact-P attention on the same dequantized
    operands), both fp64 [Lq, 128]."""
    Lkp = k.shape[0]
    if round_qk:
        kbar = k.float()[:kv_len].double().mean(0).float()
        q8, sq = ref_quant_rows(q.to(BF)[None], q.shape[0])
        k8, sk = ref_quant_rows(k.to(BF)[None], kv_len, kbar[None])
        qd, kd = q8[0].double() * sq[0].double()[:, None], k8[0].double() * sk[0].double()[:, None]
    else:
        qd, kd = q.double(), k.double()
    vd = mx_qdq_keys(v.double(), round_v)
    s = (qd @ kd.T)[:, :kv_len]
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    pr = (p * 256.0).float().to(F8).double() / 256.0 if round_p else p
    den = p.sum(-1, keepdim=True)
    return (pr @ vd[:kv_len]) / den, (p @ vd[:kv_len]) / den


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def make_qkv(Lq, Lk, gain, seed, H=1, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    Lkp = (Lk + 63) // 64 * 64
    q = (torch.randn(H, Lq, 128, generator=g, device=device) * (gain * QSCALE)).to(BF)
    k = torch.zeros(H, Lkp, 128, dtype=BF, device=device)
    v = torch.zeros(H, Lkp, 128, dtype=BF, device=device)
    k[:, :Lk] = (torch.randn(H, Lk, 128, generator=g, device=device) + 0.5 * torch.randn(H, 1, 128, generator=g, device=device)).to(BF)
    v[:, :Lk] = torch.randn(H, Lk, 128, generator=g, device=device).to(BF)
    return q, k, v


def table(shapes=((256, 4096), (128, 32768)), gains=(1, 3, 6)):
    rows = []
    for Lq, Lk in shapes:
        for gain in gains:
            q, k, v = (t[0] for t in make_qkv(Lq, Lk, gain, 10 + gain))
            ref = exact_attention(q, k, v, Lk)
            e = lambda **kw: rel(sim_attention(q, k, v, Lk, **kw)[0], ref)  # noqa: E731
            rows.append((Lq, Lk, gain, e(), e(round_p=False, round_v=False), e(round_qk=False, round_v=False), e(round_qk=False, round_p=False)))
    return rows


if __name__ == "__main__":
    print("Lq x Lk      gain  e_fmt (all)  INT8 QK only  e4m3 P only  MX-e4m3 V only")
    for Lq, Lk, gain, e_all, e_qk, e_p, e_v in table():
        print(f"{Lq:4d} x {Lk:<6d} {gain:4d}  {e_all:.3e}    {e_qk:.3e}     {e_p:.3e}    {e_v:.3e}")
    print(f"gate: e_fmt at gain 3 must not exceed {MX_QKV_GAIN3 / 4:.3e} (a quarter of the MX-e4m3 Q / K / V figure)")
