"""GPU: the block-ordered condition cache of the LongCat refine pass -- the append pooling kernel wf_lc_mean_pool_blocks_at
(csrc/longcat_ops.hip) bit for bit, the cached block-sparse forward (longcat_dit.py cache_condition_blocks / forward_tokens_cached_blocks
/ forward_cached_blocks) against the fp32 CPU oracle run with the product's own block selections, the selections against the uncached
forward's, cache invalidation, and generate_refine(video=..., use_kv_cache=True) (longcat_pipeline.py) against use_kv_cache=False.

Reference: under block-sparse attention the condition tokens still carry timestep 0, see condition keys only (attention.py:124-131),
select among condition key blocks only and skip cross-attention, so the noise frames of the UNMODIFIED
oracle.longcat_dit.forward(concatenated latents, condition timesteps 0, num_cond_latents = ncl, bsa = params) are the mathematical value
of the cached forward.  Bar: 2e-2 rel-L2, what tests/test_gpu_bsa.py test_longcat_dit_with_block_sparse_attention carries for the same
arithmetic, through tests/_tol.within."""
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
KW = dict(hidden_size=256, depth=2, num_heads=2, caption_channels=64, adaln_tembed_dim=64)


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rel_l2(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return ((got - want).norm() / (want.norm() + 1e-12)).item()


def _bits(t):
    return t.view(torch.int16).cpu()


# ---- the kernel, exact bits ---------------------------------------------------------------------------------------------------------
def _sentinel(shape):
    """A bf16 pattern no mean of the payload produces by accident: finite, non-zero, different in neighbouring elements."""
    n = 1
    for s in shape:
        n *= s
    bits = (torch.arange(n, dtype=torch.int64) * 37 + 11) % 30000 + 0x0100
    return bits.to(torch.int16).view(BF).reshape(shape).to(DEV)


def _pool(x, block):
    from worldforge_amd import bsa
    return bsa.mean_pool(x.contiguous(), block)


def _pool_at(src, in_stride, out, b0, H, L, block):
    from worldforge_amd import ops
    from worldforge_amd._ffi import call
    call("wf_lc_mean_pool_blocks_at", src.data_ptr(), in_stride, out.data_ptr(), out.shape[1], b0, H, L, block, ops.stream())


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("b0", [0, 1, 3])
@pytest.mark.parametrize("block", [64, 128])
@pytest.mark.parametrize("H", [1, 3])
def test_mean_pool_at_regions(H, block, b0, nb):
    """Rows [r0, r0 + L) of a source whose heads lie further apart than L rows -> blocks [b0, b0 + nb) of a destination whose heads
    hold more blocks than are written: the written blocks are wf_lc_mean_pool_blocks' bits, every other block keeps its bits."""
    L, r0 = nb * block, 64
    src = _rand((H, r0 + L + 64, 128), 3).to(BF).to(DEV)   # head stride r0 + L + 64 rows: larger than needed
    out = _sentinel((H, b0 + nb + 2, 128))                 # two more blocks per head than needed
    before = _bits(out)
    _pool_at(src[:, r0:], src.shape[1], out, b0, H, L, block)
    torch.cuda.synchronize()
    after = _bits(out)
    want = _bits(_pool(src[:, r0:r0 + L], block))
    assert torch.equal(after[:, b0:b0 + nb], want), "pooled payload"
    assert torch.equal(after[:, :b0], before[:, :b0]), "blocks below b0"
    assert torch.equal(after[:, b0 + nb:], before[:, b0 + nb:]), "blocks behind the last one written"


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("block", [64, 128])
@pytest.mark.parametrize("H", [1, 3])
def test_mean_pool_at_dense_equals_mean_pool(H, block, nb):
    """b0 = 0 and dense strides: the bits of wf_lc_mean_pool_blocks."""
    x = _rand((H, nb * block, 128), 4).to(BF).to(DEV)
    out = _sentinel((H, nb, 128))
    _pool_at(x, x.shape[1], out, 0, H, nb * block, block)
    assert torch.equal(_bits(out), _bits(_pool(x, block)))


@pytest.mark.parametrize("nbc,nbl", [(1, 1), (4, 8), (8, 4), (3, 5)])
@pytest.mark.parametrize("block", [64, 128])
@pytest.mark.parametrize("H", [1, 3])
def test_pool_then_append_equals_one_pooling(H, block, nbc, nbl):
    """Pooling rows [0, nc) and appending rows [nc, nc + L) == one pooling over nc + L rows: how a step extends the cached means."""
    nc, L = nbc * block, nbl * block
    k = _rand((H, nc + L, 128), 5).to(BF).to(DEV)
    whole = _pool(k, block)
    parts = _sentinel((H, nbc + nbl, 128))
    parts[:, :nbc].copy_(_pool(k[:, :nc], block))
    _pool_at(k[:, nc:], nc + L, parts, nbc, H, L, block)
    assert torch.equal(_bits(parts), _bits(whole))


def test_mean_pool_at_rejects_bad_arguments_and_writes_nothing():
    from worldforge_amd import _ffi, ops
    H, L, block, stride = 2, 256, 128, 4
    src = _rand((H, L, 128), 6).to(BF).to(DEV)
    out = _sentinel((H, stride, 128))
    before = _bits(out)
    fn = _ffi.lib().wf_lc_mean_pool_blocks_at
    i, o, s = src.data_ptr(), out.data_ptr(), ops.stream()
    bad = [(None, L, o, stride, 1, H, L, block), (i, L, None, stride, 1, H, L, block),            # null pointers
           (i + 2, L, o, stride, 1, H, L, block), (i, L, o + 8, stride, 1, H, L, block),           # misaligned pointers
           (i, L, o, stride, 1, 0, L, block), (i, L, o, stride, 1, H, 0, block), (i, L, o, stride, 1, H, -128, block),  # sizes
           (i, L, o, 0, 0, H, L, block), (i, L, o, stride, -1, H, L, block),
           (i, L, o, stride, 1, H, L, 32), (i, L, o, stride, 1, H, L, 256),                        # block
           (i, L, o, stride, 1, H, 192, block),                                                    # L % block
           (i, L - 64, o, stride, 1, H, L, block),                                                 # heads closer than L rows
           (i, L, o, stride, 3, H, L, block), (i, L, o, 1, 0, H, L, block)]                        # b0 + L / block > head stride
    for args in bad:
        assert fn(*args, s) == EINVAL, args
        assert b"wf_lc_mean_pool_blocks_at" in _ffi.lib().wf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), before)


# ---- the forward against the oracle ------------------------------------------------------------------------------------------------
#          chunk      Hh  Ww  ncl T_noise     tokens per frame; condition blocks; noise blocks
GRIDS = [((4, 4, 8), 16, 32, 4, 4),     # 128; 4 of 128 tokens; 4
         ((4, 4, 8), 16, 32, 4, 8),     # 128; 4 of 128 tokens; 8: two frame chunks of noise
         ((4, 4, 4), 16, 16, 8, 4)]     # 64; 8 of 64 tokens (two frame chunks of condition); 4


def _params(chunk, sparsity=0.5):
    return dict(sparsity=sparsity, chunk_3d_shape_q=list(chunk), chunk_3d_shape_k=list(chunk))


def _model(chunk, W, **kw):
    from worldforge_amd.longcat_dit import LongCatConfig, LongCatVideoTransformer3DModel
    return LongCatVideoTransformer3DModel(LongCatConfig(**KW), DEV, enable_bsa=True, bsa_params=_params(chunk), **kw).load_state_dict(W)


@functools.lru_cache(maxsize=None)
def _inputs(grid):
    chunk, Hh, Ww, ncl, tn = grid
    W = olc.random_weights(olc.LongCatConfig(**KW), seed=6)
    x = _rand((16, ncl + tn, Hh, Ww), 11).to(BF)
    cap = _rand((20, 64), 12).to(BF)
    ts = [0.0] * ncl + [400.0] * tn
    return W, x, cap, ts


@functools.lru_cache(maxsize=None)
def _runs(grid):
    """One cached and one uncached forward of a grid with everything the tests read back: computed once, shared, never written."""
    chunk, Hh, Ww, ncl, tn = grid
    W, x, cap, ts = _inputs(grid)
    m = _model(chunk, W)
    xd, capd = x.to(DEV), cap.to(DEV)
    cache = m.cache_condition_blocks(xd[:, :ncl].contiguous())
    got = m.forward_tokens_cached_blocks(xd[:, ncl:].contiguous(), ts[ncl:], capd, None, cache)
    step_sel = [[s.cpu() for s in layer] for layer in m.last_bsa_indices]
    cond_sel = [s.cpu() for s in cache.bsa_indices]
    unc = m.forward_tokens(xd, ts, capd, None, ncl)
    unc_sel = [[s.cpu() for s in layer] for layer in m.last_bsa_indices]
    return m, cache, got.cpu(), step_sel, cond_sel, unc.cpu(), unc_sel


@pytest.mark.parametrize("grid", GRIDS)
def test_cached_forward_matches_oracle(grid):
    chunk, Hh, Ww, ncl, tn = grid
    W, x, cap, ts = _inputs(grid)
    m, cache, got, step_sel, cond_sel, unc, unc_sel = _runs(grid)
    blk = chunk[0] * chunk[1] * chunk[2]
    tpf = (Hh // 2) * (Ww // 2)
    nc, L = ncl * tpf, tn * tpf
    H = KW["num_heads"]
    assert cache.nc == nc and cache.ncl == ncl
    assert tuple(cache.k.shape) == (2, H, nc, 128) and tuple(cache.vt.shape) == (2, H, nc // 64, 128, 64)
    assert tuple(cache.kcmp.shape) == (2, H, nc // blk, 128) and len(cache.bsa_indices) == 2
    assert got.shape == (16, tn, Hh, Ww) and got.dtype == F32 and torch.isfinite(got).all()
    assert all(len(layer) == 1 for layer in step_sel) and len(step_sel) == 2     # one entry: the noise-query selection
    assert tuple(step_sel[0][0].shape[:2]) == (H, L // blk) and int(step_sel[0][0].max()) < (nc + L) // blk
    assert tuple(cond_sel[0].shape[:2]) == (H, nc // blk) and int(cond_sel[0].max()) < nc // blk
    ocfg = olc.LongCatConfig(**KW)
    tst = torch.tensor(ts)
    want = olc.forward(W, ocfg, x.float(), tst, cap.float(), None, num_cond_latents=ncl, bsa=_params(chunk),
                       bsa_indices=[[cond_sel[i], step_sel[i][0]] for i in range(2)])[:, ncl:]
    want_u = olc.forward(W, ocfg, x.float(), tst, cap.float(), None, num_cond_latents=ncl, bsa=_params(chunk), bsa_indices=unc_sel)[:, ncl:]
    e_c, e_u = _rel_l2(got, want), _rel_l2(unc[:, ncl:], want_u)
    print(f"rel-L2 against the oracle: cached {e_c:.4e}, uncached {e_u:.4e}; cached vs uncached {_rel_l2(got, unc[:, ncl:]):.4e}")
    _tol.within("longcat refine uncached block-sparse forward rel-L2", e_u, 2e-2)
    _tol.within("longcat refine cached block-sparse forward rel-L2", e_c, 2e-2)


def _share(a, b):
    """Share of (head, query block) rows whose selected key blocks are the same SET."""
    assert a.shape[:2] == b.shape[:2]
    same = sum(set(a[h, q].tolist()) == set(b[h, q].tolist()) for h in range(a.shape[0]) for q in range(a.shape[1]))
    return same / (a.shape[0] * a.shape[1])


@pytest.mark.parametrize("grid", GRIDS)
def test_selections_agree_with_the_uncached_run(grid):
    """The cached step's noise-query selection and the build's condition-query selection against the uncached forward's, per layer
    and head, as sets per query block.  The K / Q bits may differ where a GEMM takes another tile path at another row count, so rows
    may differ near ties: at least the 0.8 share tests/test_gpu_bsa.py requires of two independent gatings."""
    m, cache, got, step_sel, cond_sel, unc, unc_sel = _runs(grid)
    for i in range(2):
        s_noise, s_cond = _share(step_sel[i][0], unc_sel[i][1]), _share(cond_sel[i], unc_sel[i][0])
        print(f"layer {i}: noise-query selections equal in {s_noise:.3f} of the rows, condition-query selections in {s_cond:.3f}")
        assert s_noise >= 0.8 and s_cond >= 0.8, (i, s_noise, s_cond)


# ---- behaviour ----------------------------------------------------------------------------------------------------------------------
def test_batch_of_two_equals_two_single_calls_and_a_cache_is_reusable():
    grid = GRIDS[0]
    chunk, Hh, Ww, ncl, tn = grid
    W, x, cap, ts = _inputs(grid)
    m = _model(chunk, W)
    xd = x.to(DEV)
    cond, noise = xd[:, :ncl].contiguous(), xd[:, ncl:].contiguous()
    cap2 = _rand((20, 64), 13).to(BF)
    mask, mask2 = torch.ones(20, dtype=torch.int64), torch.ones(20, dtype=torch.int64)
    mask2[11:] = 0
    cache = m.cache_condition_blocks(cond)
    both = m.forward_cached_blocks(torch.stack([noise, noise]), torch.tensor([[400.0] * tn, [400.0] * tn]),
                                   torch.stack([cap, cap2])[:, None].to(DEV), torch.stack([mask, mask2]), cache)
    a = m.forward_tokens_cached_blocks(noise, [400.0] * tn, cap.to(DEV), mask, cache)
    b = m.forward_tokens_cached_blocks(noise, [400.0] * tn, cap2.to(DEV), mask2, cache)
    assert both.shape == (2, 16, tn, Hh, Ww)
    assert torch.equal(both[0], a) and torch.equal(both[1], b) and not torch.equal(a, b)
    later = m.forward_tokens_cached_blocks(noise, [152.0] * tn, cap.to(DEV), mask, cache)
    fresh = m.forward_tokens_cached_blocks(noise, [152.0] * tn, cap.to(DEV), mask, m.cache_condition_blocks(cond))
    assert torch.equal(later, fresh) and not torch.equal(later, a)


def test_stale_or_foreign_caches_are_refused():
    from worldforge_amd.longcat_dit import LongCatBlockCondCache, LongCatCondCache
    grid = GRIDS[0]
    chunk, Hh, Ww, ncl, tn = grid
    W, x, cap, ts = _inputs(grid)
    m = _model(chunk, W)
    xd, capd = x.to(DEV), cap.to(DEV)
    cond, noise = xd[:, :ncl].contiguous(), xd[:, ncl:].contiguous()
    tsn = ts[ncl:]

    def run(cache, inp=noise, model=m):
        return model.forward_tokens_cached_blocks(inp, [400.0] * inp.shape[1], capd, None, cache)

    cache = m.cache_condition_blocks(cond)
    assert isinstance(cache, LongCatBlockCondCache)
    base = run(cache)
    m.weights_changed()
    with pytest.raises(ValueError):   # stale weights
        run(cache)
    cache = m.cache_condition_blocks(cond)
    assert torch.equal(run(cache), base)
    m.load_lora(lora_state(olc.LongCatConfig(**KW)), "k", multiplier=0.8, lora_network_dim=8, lora_network_alpha=4)
    m.enable_loras(["k"])
    with pytest.raises(ValueError):   # a LoRA switch
        run(cache)
    cache_l = m.cache_condition_blocks(cond)
    assert not torch.equal(run(cache_l), base)
    m.disable_all_loras()
    with pytest.raises(ValueError):
        run(cache_l)
    cache = m.cache_condition_blocks(cond)
    assert torch.equal(run(cache), base)
    with pytest.raises(ValueError):   # another latent size
        run(cache, noise[:, :, :, :16].contiguous())
    m.bsa_params["sparsity"] = 0.25
    with pytest.raises(ValueError):   # a changed sparsity
        run(cache)
    m.bsa_params["sparsity"] = 0.5
    with pytest.raises(ValueError):   # another model's cache
        run(cache, model=_model(chunk, W))
    with pytest.raises(ValueError):   # noise frames that are no whole chunk
        run(cache, noise[:, :3].contiguous())
    with pytest.raises(ValueError):   # condition frames that are no whole chunk
        m.cache_condition_blocks(xd[:, :3].contiguous())
    # a dense model has the dense cache and its entry points, and neither cache stands in for the other
    m.disable_bsa()
    with pytest.raises(NotImplementedError):
        run(cache)
    with pytest.raises(NotImplementedError):
        m.cache_condition_blocks(cond)
    dense = m.cache_condition(cond)
    assert isinstance(dense, LongCatCondCache)
    with pytest.raises(ValueError):
        m.forward_tokens_cached(noise, tsn, capd, None, cache)
    m.enable_bsa()
    with pytest.raises(ValueError):
        run(dense)
    assert torch.equal(run(cache), base)
    m.comm = object()
    with pytest.raises(NotImplementedError):
        run(cache)
    with pytest.raises(NotImplementedError):
        m.cache_condition_blocks(cond)


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
def test_generate_refine_video_cached_against_uncached():
    """The tiny block-sparse DiT behind the FakeVAE: 5 stage-1 frames refined to new_frame_size = 10 at 128 x 128 with
    num_cond_frames = 5 taken from a conditioning video -> PIPE:1414-1424 pads to 4 condition + 4 noise latent frames of 8 x 8 tokens
    (two 128-token blocks per 4 frames), t_thresh 0.5, 4 inference steps of which the 2 below t_thresh run after the step at t_thresh.

    The condition latents are the same bits on both routes.  Bar for the noise latents, from what test_cached_forward_matches_oracle
    prints on an MI355X: `cached vs uncached 0.0000e+00` on all three grids -- one cached forward IS the uncached forward's noise frames,
    bit for bit.  Both routes issue the same kernels on the noise rows: every row-wise kernel and GEMM output row depends on its own
    row only (at these row counts both GEMMs take the same tile path), the K / V^T / pooled means a step reads are the same bits whether
    they were written by this forward or copied from the cache, so the gating picks the same blocks and the sparse kernel walks the same
    keys in the same order.  A per-forward difference of 0 compounded over any number of Euler steps (each adds dt * v in fp32 to the
    same latents on both routes) is 0: the bar is EQUALITY, recorded through _tol.within with the bar 0.  Should a larger size ever
    put the L-row and the (nc + L)-row GEMM on different tile paths, the forwards may differ by bf16 rounding of K / Q and this bar has
    to be derived again from the figure test_cached_forward_matches_oracle then prints; at the sizes of this test it must not move."""
    from worldforge_amd.longcat_pipeline import LongCatVideoPipeline
    from worldforge_amd.longcat_scheduler import FlowMatchEulerDiscreteScheduler
    m = _model((4, 4, 8), olc.random_weights(olc.LongCatConfig(**KW), seed=3))
    g = torch.Generator().manual_seed(7)
    stage1 = (torch.rand(5, 64, 64, 3, generator=g) * 255).to(torch.uint8)
    prev = (torch.rand(7, 128, 128, 3, generator=g) * 255).to(torch.uint8)   # the previous window's refined frames
    pe = (torch.randn(1, 1, 24, 64, generator=g) * 0.5).to(BF)
    pm = torch.zeros(1, 24, dtype=torch.int64)
    pm[:, :19] = 1
    out = {}
    for use in (True, False):
        pipe = LongCatVideoPipeline(FakeVAE(), FlowMatchEulerDiscreteScheduler(shift=3.0), m, device=DEV)
        out[use] = pipe.generate_refine(stage1, 128, 128, pe, pm, video=prev, num_cond_frames=5, num_inference_steps=4,
                                        generator=torch.manual_seed(42), output_type="latent", use_kv_cache=use).float().cpu()
    a, b = out[True], out[False]
    ncl = 4
    assert a.shape == b.shape == (1, 16, 8, 16, 16) and torch.isfinite(a).all() and torch.isfinite(b).all()
    assert torch.equal(a[:, :, :ncl], b[:, :, :ncl])
    rel = _rel_l2(a[:, :, ncl:], b[:, :, ncl:])
    print(f"generate_refine cached vs uncached noise latents rel-L2 {rel:.4e}")
    _tol.within("longcat generate_refine cached vs uncached noise latents rel-L2", rel, 0.0)
    assert torch.equal(a, b)
    frames = pipe.generate_refine(stage1, 128, 128, pe, pm, video=prev, num_cond_frames=5, num_inference_steps=4,
                                  generator=torch.manual_seed(42), output_type="pt", use_kv_cache=True)
    assert tuple(frames.shape) == (1, 10, 128, 128, 3)   # new_frame_size = 2 * 5: the padding is cropped (PIPE:1507)
    with pytest.raises(ValueError):
        pipe.generate_refine(stage1, 128, 128, pe, pm, image=torch.rand(3, 128, 128), video=prev, num_cond_frames=5)
    with pytest.raises(ValueError):
        pipe.generate_refine(stage1, 128, 128, pe, pm, num_cond_frames=5, num_inference_steps=4)
    with pytest.raises(ValueError):   # a video that is too short for the frames asked of it
        pipe.generate_refine(stage1, 128, 128, pe, pm, video=prev[:3], num_cond_frames=5, num_inference_steps=4)
