"""GPU-free inputs, float64 references and per-element bars for wf_t5_attn_fwd (csrc/t5.hip), and the fixture reader of the UMT5 tests.
tests/test_umt5_host.py asserts on the references alone that every boundary case is sharp; tests/test_gpu_umt5_kernels_fp64.py launches.

Inputs of a case (H, L, kv_len): one [L, 3 * H * 64] bf16 buffer as the stacked QKV GEMM leaves it; q = rn_bf16(0.5 N(0,1)), k, v =
rn_bf16(N(0,1)).  The bias table of head h is a permutation of {-62, -58, ..., 62}: entries 4 apart, so a key in the wrong bucket is off
by e^4 at least.  For every bucket boundary d | d + 1 of the released rule (7|8, 11|12, 15|16, 22|23, 31|32, 45|46, 63|64, 90|91) and both
sides of the query, a free query row r gets two planted keys j1 = r +- d, j2 = r +- (d + 1) with k_j = rn_bf16(q_r (T - bias[h][bucket(j -
r)]) / |q_r|^2): both score about T = 300 on row r WITH their bias, far above every other key (random scores of a few units plus a
bias <= 62), so the row's output is about (v_j1 + v_j2) / 2 and a bucket boundary moved by one turns it into about v_j1 or v_j2.

Error model of one output element (read off k_t5_attn; U = 2^-24; ref = sum_j P_j v_j in float64 with the fp32 bias added exactly, W =
sum_j P_j |v_j|): that of tests/attn_cases.py (make_bar) with the score error taken over S + B, S = sum_d |q_d k_d| and B the row's
largest |bias|: bf16 x bf16 products are exact in fp32, the MFMA chain of 4 steps rounds partial sums <= S, the bias add and the
subtraction of the row maximum round values <= 2 (S + B): |ds| <= 24 U (S + B) in natural units, expf <= 2^-22.  The same fp32 p feeds
numerator and row sum (weights perturbed by eps_s: 2 eps_s W), P is rounded to bf16 for the P.V product only (2^-8 W), fp32 accumulation
of P.V, of the row sum, the reciprocal and the product (gamma (W + |ref|)), one bf16 rounding of the output:
    e = 2^-8 W + 2 eps_s W + gamma (W + |ref|),   bar = e + 2^-8 (|ref| + e)        (make_bar; S_row handed over in its exp2 units)."""
import json
import math
import os

import numpy as np
import torch

from tests.attn_cases import LOG2E, make_bar

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
D = 64
T_PLANT = 300.0
BOUNDARIES = (7, 11, 15, 22, 31, 45, 63, 90)      # d | d + 1: the last distance of a bucket of the released rule
HS = (3, 64)
LS = (1, 16, 63, 64, 65, 200, 512)
KV_CUT = {16: 9, 63: 37, 64: 37, 65: 41, 200: 173, 512: 301}    # cuts a 16-key and a 64-key tile (kv % 16 != 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_umt5.npz")
GOLDEN64 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_umt5_y64.npz")


def case_list():
    out = []
    for H in HS:
        for L in LS:
            for kv in sorted({1, KV_CUT.get(L, 1), L}):
                out.append((H, L, kv))
    return out


def lut_of(bucket_fn, lmax=512):
    return np.array([bucket_fn(r) for r in range(-(lmax - 1), lmax)], dtype=np.uint8)


def plant_plan(L, kv):
    """[(d, side, r, j1, j2)]: for each boundary and side the first free row whose two keys exist and are free."""
    rows, keys, plan = set(), set(), []
    for d in BOUNDARIES:
        for side in (1, -1):
            for r in range(L):
                rr = (r * 37 + 11 * d) % L                      # spread the rows over the query tiles
                j1, j2 = rr + side * d, rr + side * (d + 1)
                if rr in rows or not (0 <= j1 < kv and 0 <= j2 < kv) or j1 in keys or j2 in keys:
                    continue
                rows.add(rr)
                keys.update((j1, j2))
                plan.append((d, side, rr, j1, j2))
                break
    return plan


class AttnCase:
    def __init__(self, H, L, kv, bucket_fn):
        self.H, self.L, self.kv = H, L, kv
        g = torch.Generator().manual_seed(1000 * H + 10 * L + kv)
        qkv = torch.randn(L, 3, H, D, generator=g)
        qkv[:, 0] *= 0.5
        self.bias = torch.stack([torch.randperm(32, generator=g).to(F32) * 4.0 - 62.0 for _ in range(H)], 0)     # [H][32]
        self.lut = lut_of(bucket_fn)
        self.plan = plant_plan(L, kv)
        qkv = qkv.to(BF)
        for d, side, r, j1, j2 in self.plan:
            q = qkv[r, 0].to(F64)                                                            # [H, 64]
            for j in (j1, j2):
                b = self.bias[:, int(self.lut[j - r + 511])].to(F64)
                qkv[j, 1] = (q * ((T_PLANT - b) / q.pow(2).sum(-1)).unsqueeze(-1)).to(BF)
        self.qkv = qkv.reshape(L, 3 * H * D).contiguous()
        self.ref, self.W, self.S_row = self.reference(self.lut)
        self.e, self.bar = make_bar(self.W, self.ref, self.S_row, kv)

    def reference(self, lut, rows=None):
        """float64 on the kernel's own bf16 inputs -> (ref, W, S_row) [rows, H, 64] / [rows, H, 1]; S_row in make_bar's exp2 units."""
        H, L, kv = self.H, self.L, self.kv
        x = self.qkv.view(L, 3, H, D).to(F64)
        rows = torch.arange(L) if rows is None else torch.as_tensor(rows)
        q, k, v = x[rows, 0], x[:kv, 1], x[:kv, 2]
        rel = torch.arange(kv)[None, :] - rows[:, None] + 511                                 # [rows, kv]
        b = self.bias.to(F64)[:, torch.from_numpy(lut.astype(np.int64))[rel]]                 # [H, rows, kv]
        s = torch.einsum("rhd,jhd->hrj", q, k) + b
        s_abs = torch.einsum("rhd,jhd->hrj", q.abs(), k.abs()) + b.abs()
        P = torch.softmax(s, -1)
        ref = torch.einsum("hrj,jhd->rhd", P, v)
        W = torch.einsum("hrj,jhd->rhd", P, v.abs())
        S_row = (s_abs.amax(-1).transpose(0, 1).unsqueeze(-1)) * LOG2E
        return ref, W, S_row


def shifted(bucket_fn, d, up):
    """The rule with the boundary d | d + 1 moved by one: up -> d + 1 joins d's bucket; else d joins d + 1's (both signs)."""
    def f(rel):
        a = abs(rel)
        if up and a == d + 1:
            return bucket_fn(int(math.copysign(d, rel)))
        if not up and a == d:
            return bucket_fn(int(math.copysign(d + 1, rel)))
        return bucket_fn(rel)
    return f


# ---- fixture -------------------------------------------------------------------------------------------------------------------------------
def bf16_of_bits(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(BF)


_FIX = None


def fixture():
    """{config, keys, sd (bf16 tensors), cases [(ids, mask, y64, ybf)], bucket_rel, bucket}: read once."""
    global _FIX
    if _FIX is None:
        z, z64 = np.load(GOLDEN), np.load(GOLDEN64)
        keys = [str(k) for k in z["keys"]]
        _FIX = dict(config=json.loads(bytes(z["config"]).decode()), keys=keys, sd={k: bf16_of_bits(z["sd." + k]) for k in keys},
                    cases=[(torch.from_numpy(z[f"ids{i}"].astype(np.int64)), torch.from_numpy(z[f"mask{i}"].astype(np.int64)),
                            torch.from_numpy(z64[f"y64_{i}"]), bf16_of_bits(z[f"ybf_{i}"])) for i in range(3)],
                    bucket_rel=z["bucket_rel"], bucket=z["bucket"])
    return _FIX


def write_folder(path, sd=None, config=None, rename=None, extra=None):
    """A synthetic `text_encoder/` folder (config.json + model.safetensors) from the fixture's state dict."""
    from safetensors.torch import save_file
    fx = fixture()
    sd = dict(fx["sd"] if sd is None else sd)
    for old, new in (rename or {}).items():
        sd[new] = sd.pop(old)
    sd.update(extra or {})
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(fx["config"] if config is None else config, f)
    save_file({k: v.contiguous().clone() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))
    return path
