"""GPU: LongCat video continuation on a resident condition KV cache -- the append kernel wf_v_transpose_at (csrc/longcat_ops.hip) bit
for bit, the cached forward (longcat_dit.py cache_condition / forward_tokens_cached / forward_cached) against the fp32 CPU oracle, cache
invalidation, and generate_vc (longcat_pipeline.py) cached against uncached.

Reference: the condition tokens carry timestep 0, see only condition keys (attention.py:127-131) and skip cross-attention
(longcat_video_dit.py:108-111), so their stream does not depend on the noise tokens, the prompt or the step: the noise frames of the
UNMODIFIED oracle.longcat_dit.forward(concatenated latents, condition timesteps 0, num_cond_latents = ncl) are the mathematical value of the
cached forward.  Bar: the project's whole-model rel-L2 <= 2e-2 (tests/test_gpu_longcat.py test_forward_matches_oracle), through
tests/_tol.within."""
import functools

import pytest
import torch

from oracle import longcat_dit as olc
from tests import _tol
from tests.fakes import FakeVAE, lora_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
EINVAL = -1


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rel_l2(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return ((got - want).norm() / (want.norm() + 1e-12)).item()


def _pad64(n):
    return (n + 63) // 64 * 64


# ---- the kernel, exact bits ---------------------------------------------------------------------------------------------------------
def _sentinel(shape):
    """A bf16 pattern no transpose of the payload produces: finite, non-zero, different in neighbouring elements."""
    n = 1
    for s in shape:
        n *= s
    bits = (torch.arange(n, dtype=torch.int64) * 37 + 11) % 30000 + 0x0100
    return bits.to(torch.int16).view(BF).reshape(shape).to(DEV)


def _by_key(vt):
    """Vt [H, tiles, 128, 64] -> int16 bits [H, tiles * 64 (key), 128 (channel)]."""
    H, nt = vt.shape[:2]
    return vt.view(torch.int16).permute(0, 1, 3, 2).reshape(H, nt * 64, 128).cpu()


def _v_source(L, H, seed):
    """V as the forward hands it over: a column slice (the last third) of a wider [L, 3C] tensor."""
    C = H * 128
    wide = _rand((L, 3 * C), seed).to(BF).to(DEV)
    return wide, wide[:, 2 * C:]


KERNEL_CASES = [(0, 50), (24, 30), (24, 40), (24, 104), (63, 1), (1, 63), (1, 64), (64, 64), (72, 120), (130, 200)]


@pytest.mark.parametrize("k0,L", KERNEL_CASES)
@pytest.mark.parametrize("H", [1, 3])
def test_v_transpose_at_regions(H, k0, L):
    from worldforge_amd import ops
    from worldforge_amd._ffi import call
    end = _pad64(k0 + L)
    Lp = end + 64  # one later tile, which must stay untouched
    wide, V = _v_source(L, H, 3)
    vt = _sentinel((H, Lp // 64, 128, 64))
    before = _by_key(vt)
    call("wf_v_transpose_at", V.data_ptr(), wide.stride(0), vt.data_ptr(), k0, L, Lp, H, ops.stream())
    torch.cuda.synchronize()
    after = _by_key(vt)
    want = V.view(torch.int16).reshape(L, H, 128).permute(1, 0, 2).cpu()
    assert torch.equal(after[:, :k0], before[:, :k0]), "preserved prefix (keys < k0, the first touched tile's included)"
    assert torch.equal(after[:, k0:k0 + L], want), "transposed payload"
    assert (after[:, k0 + L:end] == 0).all(), "zero pad to the end of the last touched tile"
    assert torch.equal(after[:, end:], before[:, end:]), "later tiles untouched"


@pytest.mark.parametrize("k0,L", KERNEL_CASES)
@pytest.mark.parametrize("H", [1, 3])
def test_v_transpose_then_append_equals_one_transpose(H, k0, L):
    """wf_v_transpose of the first k0 rows followed by wf_v_transpose_at of the rest == wf_v_transpose of all rows, in every tile
    below ceil((k0 + L) / 64); with k0 = 0 that is the append kernel alone against wf_v_transpose."""
    from worldforge_amd import ops
    from worldforge_amd._ffi import call
    n = k0 + L
    Lp = _pad64(n) + 64
    wide, V = _v_source(n, H, 4)
    ld = wide.stride(0)
    whole, parts = _sentinel((H, Lp // 64, 128, 64)), _sentinel((H, Lp // 64, 128, 64))
    call("wf_v_transpose", V.data_ptr(), ld, whole.data_ptr(), n, Lp, H, ops.stream())
    if k0 > 0:
        call("wf_v_transpose", V.data_ptr(), ld, parts.data_ptr(), k0, Lp, H, ops.stream())
    call("wf_v_transpose_at", V[k0:].data_ptr(), ld, parts.data_ptr(), k0, L, Lp, H, ops.stream())
    torch.cuda.synchronize()
    nt = _pad64(n) // 64
    assert torch.equal(parts[:, :nt].view(torch.int16).cpu(), whole[:, :nt].view(torch.int16).cpu())


def test_v_transpose_at_rejects_bad_arguments_and_writes_nothing():
    from worldforge_amd import _ffi, ops
    H, L, Lp = 2, 40, 128
    wide, V = _v_source(L, H, 5)
    ld = wide.stride(0)
    vt = _sentinel((H, Lp // 64, 128, 64))
    before = vt.clone()
    fn = _ffi.lib().wf_v_transpose_at
    v, o, s = V.data_ptr(), vt.data_ptr(), ops.stream()
    bad = [(None, ld, o, 24, L, Lp, H), (v, ld, None, 24, L, Lp, H), (v, ld, o, -1, L, Lp, H), (v, ld, o, 24, 0, Lp, H),
           (v, ld, o, 24, -5, Lp, H), (v, ld, o, 100, L, Lp, H), (v, ld, o, 24, L, 100, H), (v, 128, o, 24, L, Lp, H)]
    for args in bad:
        assert fn(*args, s) == EINVAL, args
    torch.cuda.synchronize()
    assert torch.equal(vt.view(torch.int16), before.view(torch.int16))


# ---- the forward against the oracle ------------------------------------------------------------------------------------------------
def _cfg(C, heads, depth, cap, ct):
    from worldforge_amd.longcat_dit import LongCatConfig
    kw = dict(hidden_size=C, depth=depth, num_heads=heads, caption_channels=cap, adaln_tembed_dim=ct)
    return LongCatConfig(**kw), olc.LongCatConfig(**kw)


#            C  heads depth ncl T_noise h   w      tokens per frame, nc
FORWARD = [(256, 2, 3, 1, 3, 8, 12),    # 24, 24: the offset inside the first tile
           (384, 3, 2, 3, 2, 8, 12),    # 24, 72: crosses a tile boundary
           (256, 2, 2, 1, 2, 16, 16)]   # 64, 64: aligned


@functools.lru_cache(maxsize=None)
def _forward_case(case):
    """Weights, inputs and the oracle's noise frames of one case: computed once, shared by the tests, never written."""
    C, heads, depth, ncl, tn, h, w = case
    cfg, ocfg = _cfg(C, heads, depth, 96, 64)
    W = olc.random_weights(ocfg, seed=4)
    x = _rand((16, ncl + tn, h, w), 11).to(BF)
    cap = _rand((40, 96), 12).to(BF)
    mask = torch.zeros(40, dtype=torch.int64)
    mask[:29] = 1
    ts = [0.0] * ncl + [812.0] * tn
    want = olc.forward(W, ocfg, x.float(), torch.tensor(ts), cap.float(), mask, num_cond_latents=ncl)[:, ncl:].contiguous()
    return cfg, ocfg, W, x, cap, mask, ts, want


def _model(cfg, W):
    from worldforge_amd.longcat_dit import LongCatVideoTransformer3DModel
    return LongCatVideoTransformer3DModel(cfg, DEV).load_state_dict(W)


@pytest.mark.parametrize("track_max", [False, True])
@pytest.mark.parametrize("case", FORWARD)
def test_cached_forward_matches_oracle(case, track_max):
    from worldforge_amd.dit import head_max_norm2
    ncl = case[3]
    cfg, ocfg, W, x, cap, mask, ts, want = _forward_case(case)
    m = _model(cfg, W)
    m.attn_track_max = track_max
    xd, capd = x.to(DEV), cap.to(DEV)
    cache = m.cache_condition(xd[:, :ncl].contiguous())
    got = m.forward_tokens_cached(xd[:, ncl:].contiguous(), ts[ncl:], capd, mask, cache)
    assert got.shape == want.shape and got.dtype == F32 and torch.isfinite(got).all()
    unc = m.forward_tokens(xd, ts, capd, mask, ncl)[:, ncl:]
    e_c, e_u = _rel_l2(got, want), _rel_l2(unc, want)
    print(f"rel-L2 against the oracle: cached {e_c:.4e}, uncached {e_u:.4e}, cached vs uncached {_rel_l2(got, unc):.4e}")
    _tol.within("longcat vc uncached forward rel-L2", e_u, 2e-2)
    _tol.within("longcat vc cached forward rel-L2", e_c, 2e-2)
    if not track_max:
        # the un-tracked softmax body overflows silently under a bound that misses keys: the bound handed to the kernel (the last
        # block's) must cover ALL nc + L rows of the working K, the cached ones included
        kh, n = m.last_vc_keys
        assert n == cache.nc + (x.shape[1] - ncl) * (x.shape[2] // 2) * (x.shape[3] // 2)
        bound = m.last_kmax2.cpu()
        scan = head_max_norm2(kh, n, torch.empty(cfg.num_heads, dtype=F32, device=DEV)).cpu()   # the same arithmetic over every row
        assert (bound >= scan).all(), (bound, scan)
        assert (bound >= cache.kmax2[-1].cpu()).all()
        # and the exact value: 128 exact products of bf16 values summed in fp32 are within 128 * 2^-24 of it
        exact = kh[:, :n].double().pow(2).sum(-1).max(-1).values.cpu()
        assert (bound.double() >= exact * (1 - 2.0 ** -16)).all(), (bound, exact)
    else:
        assert m.last_kmax2 is None


# ---- behaviour ----------------------------------------------------------------------------------------------------------------------
def test_batch_of_two_equals_two_single_calls_and_a_cache_is_reusable():
    case = FORWARD[1]
    ncl = case[3]
    cfg, ocfg, W, x, cap, mask, ts, _ = _forward_case(case)
    m = _model(cfg, W)
    xd = x.to(DEV)
    noise = xd[:, ncl:].contiguous()
    cap2 = _rand((40, 96), 13).to(BF)
    mask2 = torch.ones(40, dtype=torch.int64)
    cache = m.cache_condition(xd[:, :ncl].contiguous())
    tn = noise.shape[1]
    both = m.forward_cached(torch.stack([noise, noise]), torch.tensor([[812.0] * tn, [812.0] * tn]),
                            torch.stack([cap, cap2])[:, None].to(DEV), torch.stack([mask, mask2]), cache)
    a = m.forward_tokens_cached(noise, [812.0] * tn, cap.to(DEV), mask, cache)
    b = m.forward_tokens_cached(noise, [812.0] * tn, cap2.to(DEV), mask2, cache)
    assert both.shape == (2, 16, tn, x.shape[2], x.shape[3])
    assert torch.equal(both[0], a) and torch.equal(both[1], b) and not torch.equal(a, b)
    # one cache over two different timesteps == a freshly built cache at the second
    later = m.forward_tokens_cached(noise, [304.0] * tn, cap.to(DEV), mask, cache)
    fresh = m.forward_tokens_cached(noise, [304.0] * tn, cap.to(DEV), mask, m.cache_condition(xd[:, :ncl].contiguous()))
    assert torch.equal(later, fresh) and not torch.equal(later, a)
    # the 1-D timestep form and the bf16 rounding of __call__ (longcat_video_dit.py:299-306): bf16(637) = 636
    c = m.forward_cached(noise[None], torch.tensor([637.0]), cap[None, None].to(DEV), mask[None], cache)
    d = m.forward_cached(noise[None], torch.tensor([[636.0] * tn]), cap[None, None].to(DEV), mask[None], cache)
    assert torch.equal(c, d)
    with pytest.raises(NotImplementedError):
        m(xd[None], torch.tensor([1.0]), cap[None, None].to(DEV), return_kv=True)


def test_stale_or_foreign_caches_are_refused():
    case = FORWARD[0]
    ncl = case[3]
    cfg, ocfg, W, x, cap, mask, ts, _ = _forward_case(case)
    m = _model(cfg, W)
    xd, capd = x.to(DEV), cap.to(DEV)
    cond, noise = xd[:, :ncl].contiguous(), xd[:, ncl:].contiguous()
    tsn = ts[ncl:]

    def run(cache, inp=noise):
        return m.forward_tokens_cached(inp, tsn, capd, mask, cache)

    cache = m.cache_condition(cond)
    run(cache)
    m.weights_changed()
    with pytest.raises(ValueError):
        run(cache)
    cache = m.cache_condition(cond)
    base = run(cache)
    m.load_lora(lora_state(ocfg), "k", multiplier=0.8, lora_network_dim=8, lora_network_alpha=4)
    m.enable_loras(["k"])
    with pytest.raises(ValueError):
        run(cache)
    cache_l = m.cache_condition(cond)
    assert not torch.equal(run(cache_l), base)   # the adapter is in the cached stream and in the noise stream
    m.disable_all_loras()
    with pytest.raises(ValueError):
        run(cache_l)
    cache = m.cache_condition(cond)
    assert torch.equal(run(cache), base)
    with pytest.raises(ValueError):   # another latent size
        run(cache, noise[:, :, :, :8].contiguous())
    with pytest.raises(ValueError):   # another model's cache
        _model(cfg, W).forward_tokens_cached(noise, tsn, capd, mask, cache)
    m.enable_bsa()
    with pytest.raises(NotImplementedError):
        run(cache)
    with pytest.raises(NotImplementedError):
        m.cache_condition(cond)
    m.disable_bsa()
    assert torch.equal(run(cache), base)
    m.comm = object()
    with pytest.raises(NotImplementedError):
        run(cache)


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_cond_frames,ncl,guidance", [(5, 2, 1.0), (1, 1, 4.0)])
def test_generate_vc_cached_against_uncached(num_cond_frames, ncl, guidance):
    """The tiny DiT behind the FakeVAE, 4 steps, 8 latent frames of 8 x 12.  The condition latents are the same bits on both routes.  The
    noise latents differ by what one forward differs (cached against uncached: both within the per-forward bar of the oracle) and by
    the reference's own dtype flow (the uncached loop rounds the latents to bf16 after every step, pipeline_longcat_video.py:1248, the
    cached one carries fp32, :1246; the DiT sees bf16 either way).  Stated bar: the per-forward 2e-2 rel-L2 -- ASSUMING that four Euler
    steps of the flow-match sampler (each adds dt * v with |dt| <= 1/4 of the sigma range to O(1) latents) do not amplify a per-forward
    velocity difference at these sizes; the measured difference is logged through _tol.within."""
    from worldforge_amd.longcat_pipeline import LongCatVideoPipeline
    from worldforge_amd.longcat_scheduler import FlowMatchEulerDiscreteScheduler
    cfg, ocfg = _cfg(256, 2, 2, 64, 64)
    m = _model(cfg, olc.random_weights(ocfg, seed=3))
    g = torch.Generator().manual_seed(7)
    video = torch.rand(3, 9, 64, 96, generator=g)
    pe, ne = (torch.randn(1, 1, 24, 64, generator=g) * 0.5).to(BF), (torch.randn(1, 1, 24, 64, generator=g) * 0.5).to(BF)
    pm, nm = torch.zeros(1, 24, dtype=torch.int64), torch.zeros(1, 24, dtype=torch.int64)
    pm[:, :19] = 1
    nm[:, :7] = 1
    out = {}
    for use in (True, False):
        pipe = LongCatVideoPipeline(FakeVAE(), FlowMatchEulerDiscreteScheduler(shift=3.0), m, device=DEV)
        out[use] = pipe.generate_vc(video, 64, 96, pe, pm, negative_prompt_embeds=ne, negative_prompt_attention_mask=nm, num_frames=29,
                                    num_cond_frames=num_cond_frames, num_inference_steps=4, guidance_scale=guidance,
                                    generator=torch.manual_seed(42), output_type="latent", use_kv_cache=use).float().cpu()
    a, b = out[True], out[False]
    assert a.shape == b.shape == (1, 16, 8, 8, 12) and torch.isfinite(a).all() and torch.isfinite(b).all()
    assert torch.equal(a[:, :, :ncl], b[:, :, :ncl])
    _tol.within("longcat generate_vc cached vs uncached noise latents rel-L2", _rel_l2(a[:, :, ncl:], b[:, :, ncl:]), 2e-2)
    with pytest.raises(NotImplementedError):
        pipe.generate_vc(video, 64, 96, pe, pm, offload_kv_cache=True)
    with pytest.raises(NotImplementedError):
        pipe.generate_vc(video, 64, 96, pe, pm, enhance_hf=True)
