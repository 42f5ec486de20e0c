"""GPU-free inputs, float64 references and per-element bars for wf_gemm_f32 and wf_clip_attn_fwd (csrc/clip.hip), and the fixture reader of
the CLIP tests.  tests/test_clip_host.py asserts on the references alone that every case can see a narrowed operand;
tests/test_gpu_clip_kernels_fp64.py launches.  U = 2^-24 (half an ulp of fp32) throughout.

wf_gemm_f32, exact cases: one operand holds integers in [-2047, 2047], the other {-1, 0, 1}, K <= 5120: every partial sum of every
summation order is an integer below 2047 * 5120 < 2^24, so fp32 is exact and the result must EQUAL the float64 product.  An operand
rounded to bf16 (8 significant bits) moves the 11-bit integers and the result.  (Integers up to 2047 are exact in fp16, so these cases
cannot see an fp16 split with a dropped low term: see test_clip_host.py.)

wf_gemm_f32, random cases, error model read off k_gemm_f32: v = sum_k x w + bias is, per wave, one chain of at most 8 ceil(ceil(K / 8) / 4)
fp32 fma (zero padding is exact), then three additions of the waves' partial sums and the bias: every term passes through at most
chain(K) = 8 ceil(ceil(K / 8) / 4) + 4 roundings, so |dv| <= e_v = 1.01 chain U (S + |bias|), S = sum_k |x w|.  Epilogues (g = the activation,
|g'| <= 1.13 for both; HIP's erff is taken at 4 ulp, expf at 1 ulp, the division is correctly rounded):
    F32         bar = e_v
    F32_ACC     out = old + v, one more rounding:                                   e_v + U |ref|
    F32_GELU    t = v / sqrt 2 (rounded constant and product, damped by erf' t <= 0.49: 1 U), erff (8 U absolute), 1 + erf (2 U): 11 U on the
                factor, two more products:                                          1.13 e_v + 5.5 U |v| + 3 U |ref|
    QUICK_GELU  u = -1.702 v (U relative: |u| U on the exponent), expf (2 U), 1 + E, 1 / d, v r (3 U); the relative error of
                s = 1 / (1 + E) is (1 - s) times that of E:                         1.13 e_v + |ref| ((1 - s) (1.702 |v| + 3) + 4) U

wf_clip_attn_fwd, error model read off k_clip_attn (ref = sum_j P_j v_j in float64, W = sum_j P_j |v_j|, S = scale max_j sum_d |q_d k_jd|
of the row): a score is a chain of D fma and the scale product, the subtraction of the row maximum rounds a value <= 2 S: |ds| <= (D + 5)
U S; the maximum is one of the computed scores and the same m shifts numerator and denominator, so it cancels.  expf: 2 U.  eps = (D + 5)
U S + 2 U perturbs every weight relatively, numerator and denominator: 2 eps W.  P . V and the row sum are, per wave, chains over at most
32 ceil(ceil(L / 32) / 4) keys, then three additions: n = 32 ceil(ceil(L / 32) / 4) + 4 roundings on W and on the sum; the reciprocal and
the last product: 3 U.     bar = 1.01 (2 eps W + n U (W + |ref|) + 3 U |ref|)."""
import json
import math
import os

import numpy as np
import torch

F64, F32, BF, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
U = 2.0 ** -24
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPI_F32, EPI_ACC, EPI_GELU, EPI_QUICK = 2, 4, 5, 6


# ---- wf_gemm_f32 -----------------------------------------------------------------------------------------------------------------------------
EXACT_MS = (1, 31, 257)
EXACT_NK = ((1280, 588), (64, 48), (1280, 5120), (3840, 1280))     # the last two are compared on 64 sampled columns
SAMPLED = {(1280, 5120), (3840, 1280)}


def exact_case_list():
    return [(kind, M, N, K) for kind in "ab" for M in EXACT_MS for (N, K) in EXACT_NK]


def columns(N, K, seed=0):
    """The compared columns: all, or 64 sampled ones with both ends and a tile seam (63 | 64) among them."""
    if (N, K) not in SAMPLED:
        return torch.arange(N)
    c = torch.randperm(N, generator=torch.Generator().manual_seed(N + K + seed))[:64].sort().values
    c[0], c[1], c[2], c[-1] = 0, 63, 64, N - 1
    return c.unique()


def exact_inputs(kind, M, N, K):
    """(X [M, K], W [N, K]) fp32: kind a = X integers in [-2047, 2047], W in {-1, 0, 1}; kind b = the roles swapped."""
    g = torch.Generator().manual_seed(7 * M + 3 * N + K + (kind == "b"))
    big = lambda r: torch.randint(-2047, 2048, (r, K), generator=g).to(F32)  # noqa: E731
    tern = lambda r: torch.randint(-1, 2, (r, K), generator=g).to(F32)  # noqa: E731
    return (big(M), tern(N)) if kind == "a" else (tern(M), big(N))


def split_f16x3_drop(t, drop):
    """t -> the sum of an fp16 three-term split (hi, mid, lo) with term `drop` left out, in float64."""
    x = t.to(F64)
    hi = x.to(F16).to(F64)
    mid = (x - hi).to(F16).to(F64)
    lo = (x - hi - mid).to(F16).to(F64)
    return sum(p for i, p in enumerate((hi, mid, lo)) if i != drop)


RANDOM_CASES = (            # (M, N, K, epilogue, bias)
    (31, 64, 48, EPI_F32, False), (31, 64, 48, EPI_ACC, True), (31, 64, 48, EPI_GELU, True), (31, 64, 48, EPI_QUICK, True),
    (1, 68, 588, EPI_GELU, True), (257, 1280, 588, EPI_ACC, False), (65, 132, 1280, EPI_F32, True), (257, 320, 160, EPI_QUICK, True),
    (257, 160, 320, EPI_GELU, False),
)


def chain(K):
    return 8 * math.ceil(math.ceil(K / 8) / 4) + 4


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def quick64(v):
    return v * torch.sigmoid(1.702 * v)


class GemmCase:
    """fp32 inputs with full 24-bit significands, the float64 result of the epilogue and its bar."""

    def __init__(self, M, N, K, epi, has_bias):
        self.M, self.N, self.K, self.epi = M, N, K, epi
        g = torch.Generator().manual_seed(M + 10 * N + 100 * K + epi)
        self.X = torch.randn(M, K, generator=g)
        self.W = torch.randn(N, K, generator=g) * K ** -0.5 * 1.5
        self.bias = torch.randn(N, generator=g) * 0.3 if has_bias else None
        self.old = torch.randn(M, N, generator=g) if epi == EPI_ACC else None
        self.ref, self.bar = self.reference(self.X, self.W)

    def reference(self, X, W):
        x, w = X.to(F64), W.to(F64)
        b = self.bias.to(F64) if self.bias is not None else torch.zeros(self.N, dtype=F64)
        v = x @ w.T + b
        e_v = 1.01 * chain(self.K) * U * (x.abs() @ w.abs().T + b.abs())
        if self.epi == EPI_F32:
            return v, e_v + 1e-300
        if self.epi == EPI_ACC:
            ref = self.old.to(F64) + v
            return ref, e_v + U * ref.abs() + 1e-300
        if self.epi == EPI_GELU:
            ref = gelu64(v)
            return ref, 1.13 * e_v + 5.5 * U * v.abs() + 3 * U * ref.abs() + 1e-300
        ref, s = quick64(v), torch.sigmoid(1.702 * v)
        return ref, 1.13 * e_v + ref.abs() * ((1 - s) * (1.702 * v.abs() + 3) + 4) * U + 1e-300


# ---- wf_clip_attn_fwd --------------------------------------------------------------------------------------------------------------------------
ATTN_SHAPES = ((1, 1, 80), (2, 31, 80), (2, 64, 64), (3, 65, 80), (2, 257, 80), (1, 257, 64), (1, 577, 128))     # (H, L, D)
AHEAD = 60.0


class AttnCase:
    """One stacked [L, 3 H D] fp32 buffer as the QKV GEMM leaves it.  Row L // 3 has q = 0 (all scores equal: a uniform softmax over all L
    keys); row L // 2 has ONE key (2 L // 3) ahead of the row's other scores by 60 in every head."""

    def __init__(self, H, L, D):
        self.H, self.L, self.D, self.scale = H, L, D, float(D) ** -0.5
        g = torch.Generator().manual_seed(1000 * H + 10 * L + D)
        qkv = torch.randn(L, 3, H, D, generator=g)
        qkv[:, 0] *= 1.5
        self.flat_row, self.peak_row, self.peak_key = (L // 3, L // 2, (2 * L) // 3) if L >= 4 else (None, None, None)
        if self.flat_row is not None:
            qkv[self.flat_row, 0] = 0.0
            r, j = self.peak_row, self.peak_key
            q = qkv[r, 0].to(F64)                                                     # [H, D]
            s = torch.einsum("hd,jhd->hj", q, qkv[:, 1].to(F64)) * self.scale
            s[:, j] = -1e30
            T = s.amax(-1) + AHEAD
            qkv[j, 1] = (q * (T / self.scale / q.pow(2).sum(-1)).unsqueeze(-1)).to(F32)
        self.qkv = qkv.reshape(L, 3 * H * D).contiguous()
        self.ref, self.bar = self.reference()

    def reference(self, round_p=None):
        """float64 on the kernel's own fp32 inputs -> (ref, bar) [L, H, D]; round_p: a dtype P is rounded to before P . V (host checks)."""
        H, L, D = self.H, self.L, self.D
        x = self.qkv.view(L, 3, H, D).to(F64)
        q, k, v = x[:, 0], x[:, 1], x[:, 2]
        s = torch.einsum("ihd,jhd->hij", q, k) * self.scale
        S = (torch.einsum("ihd,jhd->hij", q.abs(), k.abs()) * self.scale).amax(-1)      # [H, L]
        P = torch.softmax(s, -1)
        if round_p is not None:
            P = P.to(round_p).to(F64)
        ref = torch.einsum("hij,jhd->ihd", P, v)
        W = torch.einsum("hij,jhd->ihd", P, v.abs())
        eps = ((D + 5) * U * S + 2 * U).transpose(0, 1).unsqueeze(-1)                   # [L, H, 1]
        n = 32 * math.ceil(math.ceil(L / 32) / 4) + 4
        bar = 1.01 * (2 * eps * W + n * U * (W + ref.abs()) + 3 * U * ref.abs()) + 1e-300
        return ref, bar

    def peak_margin(self):
        """The smallest lead of the planted key over the other keys of its row, over the heads (float64)."""
        x = self.qkv.view(self.L, 3, self.H, self.D).to(F64)
        s = torch.einsum("hd,jhd->hj", x[self.peak_row, 0], x[:, 1]) * self.scale
        top = s[:, self.peak_key].clone()
        s[:, self.peak_key] = -1e30
        return (top - s.amax(-1)).min().item()


# ---- fixture -----------------------------------------------------------------------------------------------------------------------------------
def bf16_of_bits(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(BF)


def last_layer_fill(config, seed):
    """Seeded values for the tensors the fixture does not store: the last encoder layer and post_layernorm."""
    from worldforge_amd import clip
    cfg = clip.CLIPVisionConfig.from_dict(config)
    g = torch.Generator().manual_seed(seed)
    last = f"encoder.layers.{cfg.num_hidden_layers - 1}."
    return {k: torch.randn(*s, generator=g) for k, s in clip.expected_state_dict(cfg).items() if k.startswith((last, "post_layernorm."))}


_FIX = None


def fixture():
    """{config, sd (fp32 tensors holding bf16 values; the unstored last layer and post_layernorm filled with seed 1), cases {name: (act,
    pixel_values, y64, rel_f32, rel_bf16)}}: read once."""
    global _FIX
    if _FIX is None:
        z0, z1 = np.load(os.path.join(GOLD, "g25_clip_w0.npz")), np.load(os.path.join(GOLD, "g25_clip_w1.npz"))
        config = json.loads(bytes(z0["config"]).decode())
        sd = {}
        for k in (str(k) for k in z0["keys"]):
            z = z1 if "sd." + k in z1.files else z0
            sd[k] = bf16_of_bits(z["sd." + k]).to(F32)
        stored = sorted(sd)
        sd.update(last_layer_fill(config, 1))
        cases = {}
        for name in ("gelu", "quick"):
            z = np.load(os.path.join(GOLD, f"g25_clip_{name}.npz"))
            cases[name] = (str(z["hidden_act"]), torch.from_numpy(z["pixel_values"]), torch.from_numpy(z["y64"]), float(z["rel_f32"]),
                           float(z["rel_bf16"]))
        _FIX = dict(config=config, sd=sd, stored=stored, cases=cases)
    return _FIX


def preprocess_fixture():
    """(processor settings, [(uint8 image [h, w, 3], pixel_values fp32 [3, 224, 224])])."""
    z = np.load(os.path.join(GOLD, "g25_clip_pre_img.npz"))
    return json.loads(bytes(z["processor"]).decode()), [(z[f"img{i}"], np.load(os.path.join(GOLD, f"g25_clip_pre_pv{i}.npz"))["pixel_values"])
                                                        for i in range(2)]


def write_folder(path, sd=None, config=None, prefix="", rename=None, extra=None, drop=()):
    """A synthetic `image_encoder/` folder (config.json + model.safetensors) from the fixture's state dict, keys under `prefix`."""
    from safetensors.torch import save_file
    fx = fixture()
    sd = {prefix + k: v for k, v in (fx["sd"] if sd is None else sd).items() if k not in drop}
    for old, new in (rename or {}).items():
        sd[new] = sd.pop(old)
    sd.update(extra or {})
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(fx["config"] if config is None else config, f)
    save_file({k: v.contiguous().clone() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))
    return path
