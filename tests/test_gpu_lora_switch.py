"""GPU: switchable LoRA adapters on a resident LongCat DiT -- the fold kernel (csrc/lora.hip, wf_lora_fold) against fp64 element by element,
and load_lora / enable_loras / disable_all_loras of LongCatVideoTransformer3DModel against the reference's run-time LoRA (golden g13), as a
state machine (bit for bit), under linear_precision="mxfp8", and in the two-stage run (distilled i2v, then the block-sparse refine pass)
on ONE resident model.

The kernel bound is derived, not measured: with e the fp64 value of
    base[n,k] + sum_j scale_j * sum_r U_j[n,r] * D_j[blk_j(n) * rank_j + r, k]
on the bf16-valued inputs and A = |base| + sum_j |scale_j| sum_r |U_j| |D_j|, every element must satisfy
    |out - e| <= 2^-8 |e| + 2 (R + 4) 2^-24 A,     R = the total rank:
half a bf16 ulp for the ONE rounding, plus the standard fp32 accumulation bound (R products, the scaling, the adapter sum and the base
add), doubled because the MFMA's internal summation order is not specified.  A kernel that truncates, rounds the product to bf16 before
the add, or rounds twice misses it on a large share of the elements."""
import os

import numpy as np
import pytest
import torch

from oracle import longcat_dit as olc
from tests import _tol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SCALES = (0.4, -0.25)


def _rel_l2(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return ((got - want).norm() / (want.norm() + 1e-12)).item()


def _factors(N, K, rank, nsep, seed):
    g = torch.Generator().manual_seed(seed)
    U = (torch.randn(N, rank, generator=g) * 0.3).to(BF)
    D = (torch.randn(nsep * rank, K, generator=g) / K ** 0.5).to(BF)
    return U, D


def _base(N, K, seed):
    return (torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) / K ** 0.5).to(BF)


def _ref(base, adapters):
    """fp64: (e, A) of the module docstring; adapters = [(U, D, nsep, scale)] bf16-valued CPU tensors."""
    e, A = base.to(F64), base.to(F64).abs()
    N = base.shape[0]
    for U, D, nsep, scale in adapters:
        rank, rows = U.shape[1], N // nsep
        scale = float(np.float32(scale))  # the entry point takes the scale as fp32
        U64, D64 = U.to(F64), D.to(F64)
        prod = torch.cat([U64[b * rows:(b + 1) * rows] @ D64[b * rank:(b + 1) * rank] for b in range(nsep)], 0)
        mag = torch.cat([U64[b * rows:(b + 1) * rows].abs() @ D64[b * rank:(b + 1) * rank].abs() for b in range(nsep)], 0)
        e = e + scale * prod
        A = A + abs(scale) * mag
    return e, A


def _check(out, base, adapters, what):
    e, A = _ref(base, adapters)
    R = sum(a[0].shape[1] for a in adapters)
    err = (out.cpu().to(F64) - e).abs()
    bound = 2.0 ** -8 * e.abs() + 2 * (R + 4) * 2.0 ** -24 * A
    worst = (err / bound).max().item()
    print(f"[lora fold] {what}: max |out - e| / bound = {worst:.3f}, elements over the bound: {int((err > bound).sum())} of {err.numel()}")
    assert torch.isfinite(out.float()).all(), what
    assert not (err > bound).any(), (what, worst, int((err > bound).sum()))


def _fold(base_d, adapters_d, out=None):
    from worldforge_amd import ops
    out = torch.full_like(base_d, float("nan")) if out is None else out
    ops.lora_fold(base_d, out, adapters_d)
    return out


def _dev(adapters):
    return [(U.to(DEV), D.to(DEV), nsep, s) for U, D, nsep, s in adapters]


@pytest.mark.parametrize("N,K,rank,nsep", [(96, 64, 8, 1), (160, 200, 24, 1), (768, 256, 8, 3), (512, 256, 16, 2), (1536, 4096, 128, 3),
                                           (256, 11008, 128, 1)])
def test_fold_kernel_against_fp64(N, K, rank, nsep):
    base = _base(N, K, 1)
    adapters = [(*_factors(N, K, rank, nsep, 2), nsep, SCALES[0])]
    base_d, ad_d = base.to(DEV), _dev(adapters)
    keep = base_d.clone()
    out = _fold(base_d, ad_d)          # out pre-filled with NaN: every element must be written
    _check(out, base, adapters, f"{N}x{K} rank {rank} nsep {nsep}")
    assert torch.equal(base_d, keep)   # base is only read
    inplace = base_d.clone()
    _fold(inplace, ad_d, out=inplace)  # out == base
    assert torch.equal(inplace, out)
    if nsep > 1:  # every row block uses its own rank slice: exchanging two slices of D is another matrix
        U, D, _, s = adapters[0]
        Ds = D.clone()
        Ds[:rank], Ds[rank:2 * rank] = D[rank:2 * rank], D[:rank]
        swapped = [(U, Ds, nsep, s)]
        out_s = _fold(base_d, _dev(swapped))
        _check(out_s, base, swapped, f"{N}x{K} rank {rank} nsep {nsep}, slices 0 and 1 of D exchanged")
        rows = N // nsep
        assert not torch.equal(out_s[:2 * rows], out[:2 * rows]) and torch.equal(out_s[2 * rows:], out[2 * rows:])


def test_fold_kernel_two_adapters_one_rounding():
    N, K = 768, 256
    base = _base(N, K, 3)
    adapters = [(*_factors(N, K, 8, 3, 4), 3, SCALES[0]), (*_factors(N, K, 16, 3, 5), 3, SCALES[1])]
    base_d = base.to(DEV)
    out = _fold(base_d, _dev(adapters))
    _check(out, base, adapters, "768x256 ranks 8 + 16, nsep 3")
    mixed = [adapters[0], (*_factors(N, K, 16, 1, 6), 1, SCALES[1])]  # fused-block and plain up-projections in one launch
    _check(_fold(base_d, _dev(mixed)), base, mixed, "768x256 ranks 8 (nsep 3) + 16 (nsep 1)")


def test_fold_kernel_row_slice():
    """A contiguous row slice of a matrix (the w1 / w3 halves of ffn.w13, a block's rows of ada.w): the other rows keep their bits."""
    N, K, r0, rows = 416, 128, 96, 192
    base = _base(N, K, 7)
    adapters = [(*_factors(rows, K, 8, 1, 8), 1, SCALES[0])]
    base_d = base.to(DEV)
    buf = base_d.clone()
    _fold(base_d[r0:r0 + rows], _dev(adapters), out=buf[r0:r0 + rows])
    _check(buf[r0:r0 + rows], base[r0:r0 + rows], adapters, "rows 96..288 of 416x128")
    assert torch.equal(buf[:r0], base_d[:r0]) and torch.equal(buf[r0 + rows:], base_d[r0 + rows:])


# ---- the DiT's methods ---------------------------------------------------------------------------------------------------------------
KW = dict(hidden_size=256, depth=2, num_heads=2, caption_channels=64, adaln_tembed_dim=64)
H = "___lorahyphen___"


def _model(W, **kw):
    from worldforge_amd.longcat_dit import LongCatConfig, LongCatVideoTransformer3DModel
    return LongCatVideoTransformer3DModel(LongCatConfig(**KW), DEV, **kw).load_state_dict(W)


def _same(Wa, Wb):
    return set(Wa) == set(Wb) and all(torch.equal(Wa[k], Wb[k]) for k in Wa)


def _snapshot(W):
    return {k: v.clone() for k, v in W.items()}


def test_enable_loras_matches_reference_runtime_lora():
    """Golden g13: the reference's run-time LoRA (out) and its base model (out_base) on the model of
    tests/test_gpu_longcat.py::test_lora_fold_matches_reference_runtime_lora, here built with the BASE weights."""
    from tests.fakes import lora_state
    L = np.load(os.path.join(os.path.dirname(__file__), "golden", "g13_longcat_lora.npz"))
    ocfg = olc.LongCatConfig(**KW)
    W = olc.random_weights(ocfg, seed=21)
    m = _model(W)
    args = (torch.from_numpy(L["x"]).to(BF).to(DEV), L["ts"].tolist(), torch.from_numpy(L["cap"]).to(BF).to(DEV), torch.from_numpy(L["mask"]), 1)
    m.load_lora(lora_state(ocfg), "k", multiplier=0.8, lora_network_dim=8, lora_network_alpha=4)
    assert m.active_loras == [] and list(m.lora_dict) == ["k"] and m.w is m.base_w
    m.enable_loras(["k", "not loaded"])   # unknown keys are ignored (LCD:219)
    assert m.active_loras == ["k"]
    got = m.forward_tokens(*args)
    err = _rel_l2(got, torch.from_numpy(L["out"]))
    off = _rel_l2(got, torch.from_numpy(L["out_base"]))
    print(f"[lora switch] rel. L2 to the reference's run-time LoRA {err:.4e}, to its base model {off:.4e}")
    _tol.within("lora_switch_vs_runtime_lora", err, 2e-2)
    assert off > 5e-2   # and not the base model
    m.disable_all_loras()
    assert m.active_loras == [] and m.w is m.base_w
    assert torch.equal(m.forward_tokens(*args), _model(W).forward_tokens(*args))


def test_state_machine_bit_for_bit():
    from tests.fakes import lora_state
    ocfg = olc.LongCatConfig(**KW)
    W = olc.random_weights(ocfg, seed=21)
    A, B = lora_state(ocfg, seed=33), lora_state(ocfg, seed=34)
    m = _model(W)
    base0 = _snapshot(m.w)
    m.load_lora(A, "A", multiplier=0.8)
    m.load_lora(B, "B", multiplier=1.1)
    m.enable_loras(["A"])
    assert m.w is not m.base_w and not _same(m.w, base0)
    wa = _snapshot(m.w)
    touched = [k for k in wa if m.w[k] is not m.base_w[k]]
    assert sorted(touched) == sorted(f"blocks.{i}.{n}" for i in range(2) for n in ("attn.qkv.w", "attn.proj.w", "cross_attn.kv_linear.w",
                                                                                   "ffn.w13", "ffn.w2"))
    ptrs = {k: m.w[k].data_ptr() for k in touched}
    m.enable_loras(["B"])
    wb = _snapshot(m.w)
    assert not _same(wa, wb)
    m.enable_loras(["A"])
    assert _same(m.w, wa)                                        # A -> B -> A reproduces the first A weights exactly
    m.enable_loras(["B"])
    fresh = _model(W)
    fresh.load_lora(B, "B", multiplier=1.1)
    fresh.enable_loras(["B"])
    assert _same(m.w, fresh.w) and _same(m.w, wb)                # base -> A -> B == a fresh model with only B
    assert {k: m.w[k].data_ptr() for k in touched} == ptrs       # ONE effective buffer per matrix, reused by every switch
    # untouched tensors are shared with the base, and the base is never written
    assert all(m.w[k] is m.base_w[k] for k in m.w if k not in touched) and _same(m.base_w, base0)

    # both adapters at once: test 1's two-adapter definition (one rounding) on the fused qkv weight of block 1
    m.enable_loras(["A", "B"])
    assert m.active_loras == ["A", "B"] and {k: m.w[k].data_ptr() for k in touched} == ptrs
    name = "lora" + H + "blocks.1.attn.qkv".replace(".", H)
    ads = []
    for sd, mult in ((A, 0.8), (B, 1.1)):
        U = torch.cat([sd[name + f".lora_up.blocks.{b}.weight"] for b in range(3)], 0).to(BF)
        ads.append((U, sd[name + ".lora_down.weight"].to(BF), 3, mult * float(sd[name + ".alpha_scale"])))
    _check(m.w["blocks.1.attn.qkv.w"], base0["blocks.1.attn.qkv.w"].cpu(), ads, "enable_loras([A, B]) on blocks.1.attn.qkv")

    # ffn.w1 / ffn.w3 land in their halves of w13; lora_state wraps w1 only: the w3 half keeps the base's bits
    Hd = ocfg.ffn_hidden
    m.enable_loras(["A"])
    assert torch.equal(m.w["blocks.0.ffn.w13"][Hd:], base0["blocks.0.ffn.w13"][Hd:])
    assert not torch.equal(m.w["blocks.0.ffn.w13"][:Hd], base0["blocks.0.ffn.w13"][:Hd])
    g = torch.Generator().manual_seed(9)
    n1, n3 = ("lora" + H + f"blocks.0.ffn.{w}".replace(".", H) for w in ("w1", "w3"))
    C13 = {}
    for n in (n1, n3):
        C13[n + ".lora_down.weight"] = torch.randn(8, 256, generator=g) / 16
        C13[n + ".lora_up.weight"] = torch.randn(Hd, 8, generator=g) * 0.3
    m.load_lora(C13, "C", multiplier=1.0, lora_network_dim=8, lora_network_alpha=4)   # no alpha_scale: alpha / dim = 0.5
    m.enable_loras(["C"])
    for n, lo in ((n1, 0), (n3, Hd)):
        _check(m.w["blocks.0.ffn.w13"][lo:lo + Hd], base0["blocks.0.ffn.w13"][lo:lo + Hd].cpu(),
               [(C13[n + ".lora_up.weight"].to(BF), C13[n + ".lora_down.weight"].to(BF), 1, 0.5)], f"ffn.w13 rows {lo}..{lo + Hd}")
    assert torch.equal(m.w["blocks.1.ffn.w13"], base0["blocks.1.ffn.w13"]) and m.w["blocks.0.ffn.w13"].data_ptr() == ptrs["blocks.0.ffn.w13"]

    # an in-place edit of a base tensor is picked up by weights_changed(); a new base deactivates and keeps the loaded adapters
    m.enable_loras(["A"])
    m.base_w["blocks.0.attn.proj.w"].mul_(2.0)
    m.weights_changed()
    assert not torch.equal(m.w["blocks.0.attn.proj.w"], wa["blocks.0.attn.proj.w"])
    m.base_w["blocks.0.attn.proj.w"].copy_(base0["blocks.0.attn.proj.w"])
    m.weights_changed()
    assert _same(m.w, wa)
    m.load_state_dict(W)
    assert m.active_loras == [] and sorted(m.lora_dict) == ["A", "B", "C"] and m.w is m.base_w and _same(m.w, base0)


def test_adaln_slice_of_the_stacked_matrix():
    """blocks.i.adaLN_modulation.1 is a row slice of the stacked ada.w: block 1's adapter leaves block 0's rows alone."""
    ocfg = olc.LongCatConfig(**KW)
    W = olc.random_weights(ocfg, seed=21)
    m = _model(W)
    g = torch.Generator().manual_seed(10)
    n = "lora" + H + "blocks.1.adaLN_modulation.1".replace(".", H)
    sd = {n + ".lora_down.weight": torch.randn(8, 64, generator=g) / 8, n + ".lora_up.weight": torch.randn(6 * 256, 8, generator=g) * 0.3,
          n + ".alpha_scale": torch.tensor(0.25)}
    base = m.w["ada.w"].clone()
    m.load_lora(sd, "ada", multiplier=2.0)
    m.enable_loras(["ada"])
    rows = 6 * 256
    assert torch.equal(m.w["ada.w"][:rows], base[:rows])
    _check(m.w["ada.w"][rows:], base[rows:].cpu(), [(sd[n + ".lora_up.weight"].to(BF), sd[n + ".lora_down.weight"].to(BF), 1, 0.5)],
           "ada.w rows of block 1")


def test_mxfp8_requantizes_from_the_effective_weights():
    from tests.fakes import lora_state
    ocfg = olc.LongCatConfig(**KW)
    W = olc.random_weights(ocfg, seed=21)
    L = np.load(os.path.join(os.path.dirname(__file__), "golden", "g13_longcat_lora.npz"))
    args = (torch.from_numpy(L["x"]).to(BF).to(DEV), L["ts"].tolist(), torch.from_numpy(L["cap"]).to(BF).to(DEV), torch.from_numpy(L["mask"]), 1)
    m = _model(W, linear_precision="mxfp8")
    base_out = m.forward_tokens(*args)
    m.load_lora(lora_state(ocfg), "k", multiplier=0.8)
    m.enable_loras(["k"])
    got = m.forward_tokens(*args)
    assert not torch.equal(got, base_out)
    from worldforge_amd.longcat_dit import LongCatConfig, LongCatVideoTransformer3DModel
    fresh = LongCatVideoTransformer3DModel(LongCatConfig(**KW), DEV, linear_precision="mxfp8")
    fresh.w = _snapshot(m.w)   # the effective bf16 weights
    assert torch.equal(got, fresh.forward_tokens(*args))
    m.disable_all_loras()
    assert torch.equal(m.forward_tokens(*args), base_out)


def test_two_stage_run_on_one_resident_model():
    """Distilled i2v with adapter A, then the block-sparse refine pass with adapter B, on ONE model == the same two calls on two models
    that each enabled one adapter; the base weights are unchanged at the end."""
    from tests.fakes import lora_state
    from worldforge_amd.longcat_pipeline import LongCatVideoPipeline
    from worldforge_amd.longcat_scheduler import FlowMatchEulerDiscreteScheduler
    from worldforge_amd.vae import AutoencoderKLWan
    ocfg = olc.LongCatConfig(**KW)
    W = olc.random_weights(ocfg, seed=3)
    A, B = lora_state(ocfg, seed=33), lora_state(ocfg, seed=34)
    bsa_params = dict(sparsity=0.5, chunk_3d_shape_q=[4, 4, 8], chunk_3d_shape_k=[4, 4, 8])
    vae = AutoencoderKLWan(DEV).init_random(seed=1)
    g = torch.Generator().manual_seed(7)
    image = torch.rand(3, 32, 32, generator=g)
    image_hi = torch.rand(3, 128, 128, generator=g)
    pe = (torch.randn(1, 1, 24, 64, generator=g) * 0.5).to(BF)
    pm = torch.zeros(1, 24, dtype=torch.int64)
    pm[:, :19] = 1

    def stage1(dit):
        pipe = LongCatVideoPipeline(vae, FlowMatchEulerDiscreteScheduler(shift=3.0), dit, device=DEV)
        out = pipe.generate_i2v(image=image, height=32, width=32, prompt_embeds=pe, prompt_attention_mask=pm, num_frames=5,
                                num_inference_steps=2, use_distill=True, guidance_scale=1.0, generator=torch.Generator().manual_seed(42))
        return torch.from_numpy(out)[0]

    def stage2(dit, video):
        pipe = LongCatVideoPipeline(vae, FlowMatchEulerDiscreteScheduler(shift=3.0), dit, device=DEV)
        frames = (video * 255).round().clamp(0, 255).to(torch.uint8)
        out = pipe.generate_refine(stage1_video=frames, height=128, width=128, prompt_embeds=pe, prompt_attention_mask=pm, image=image_hi,
                                   num_cond_frames=1, num_inference_steps=4, generator=torch.Generator().manual_seed(43), t_thresh=0.5,
                                   spatial_refine_only=True)
        return torch.from_numpy(out).clone()

    def one(adapter, key, **kw):
        m = _model(W, **kw)
        m.load_lora(adapter, key)
        m.enable_loras([key])
        return m

    want1 = stage1(one(A, "distill"))
    want2 = stage2(one(B, "refine", enable_bsa=True, bsa_params=bsa_params), want1)

    m = _model(W, bsa_params=bsa_params)
    base0 = _snapshot(m.w)
    m.load_lora(A, "distill")
    m.load_lora(B, "refine")
    m.enable_loras(["distill"])
    got1 = stage1(m)
    m.enable_loras(["refine"])
    m.enable_bsa()
    got2 = stage2(m, got1)
    assert torch.isfinite(got2).all()
    assert torch.equal(got1, want1) and torch.equal(got2, want2)
    assert not torch.equal(got2, stage2(_model(W, enable_bsa=True, bsa_params=bsa_params), want1))   # the adapter does act on the refine pass
    m.disable_all_loras()
    assert m.w is m.base_w and _same(m.w, base0)
