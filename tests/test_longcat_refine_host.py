"""CPU: the host-side facts the block-ordered condition cache of the LongCat refine pass rests on (worldforge_amd/longcat_dit.py
cache_condition_blocks / forward_tokens_cached_blocks, longcat_pipeline.py generate_refine with a conditioning video); the kernel and the
forward are checked on the GPU in tests/test_gpu_longcat_refine_cache.py."""
import inspect
import math

import pytest
import torch

from worldforge_amd import _ffi, bsa
from worldforge_amd.longcat_dit import LongCatBlockCondCache, LongCatVideoTransformer3DModel, rope_tables
from worldforge_amd.longcat_pipeline import LongCatVideoPipeline


@pytest.mark.parametrize("num_cond_frames,new_frame_size", [(1, 186), (5, 186), (13, 186), (26, 186), (5, 10), (13, 93), (0, 186)])
def test_refine_padding_arithmetic(num_cond_frames, new_frame_size):
    """LongCatVideoPipeline.refine_padding (what generate_refine pads by) against pipeline_longcat_video.py:1414-1424 evaluated here
    from the reference's own statements, and the properties the rest of the pass relies on: both latent counts are whole 4-frame
    blocks, the padded condition frames encode to exactly ncl latent frames, the padded video to ncl + nnl, and the crop of :1507
    recovers new_frame_size frames."""
    tsc, gran = 4, 4
    num_noise_frames = new_frame_size - num_cond_frames
    ncl = added_c = 0
    if num_cond_frames > 0:
        ncl = 1 + math.ceil((num_cond_frames - 1) / tsc)
        ncl = math.ceil(ncl / gran) * gran
        added_c = 1 + (ncl - 1) * tsc - num_cond_frames
    nnl = math.ceil(num_noise_frames / tsc)
    nnl = math.ceil(nnl / gran) * gran
    added_n = nnl * tsc - num_noise_frames
    assert LongCatVideoPipeline.refine_padding(num_cond_frames, new_frame_size, tsc) == (ncl, added_c, nnl, added_n)
    assert ncl % gran == 0 and nnl % gran == 0 and added_c >= 0 and added_n >= 0
    total = added_c + new_frame_size + added_n
    assert (total - 1) // tsc + 1 == ncl + nnl                        # the causal VAE's latent frame count of the padded video
    assert len(range(1 + tsc * (ncl + nnl - 1))[added_c:new_frame_size + added_c]) == new_frame_size  # PIPE:1507 on the decoded frames
    if num_cond_frames > 0:
        assert ncl >= 4 and 1 + (num_cond_frames + added_c - 1) // tsc == ncl   # PIPE:283 on the padded condition frames
    want = {(1, 186): (4, 12, 48, 7), (5, 186): (4, 8, 48, 11), (13, 186): (4, 0, 44, 3), (26, 186): (8, 3, 40, 0)}
    if (num_cond_frames, new_frame_size) in want:                     # worked by hand from the same statements
        assert (ncl, added_c, nnl, added_n) == want[(num_cond_frames, new_frame_size)]


@pytest.mark.parametrize("num_cond_frames,frames", [(1, 3), (5, 7), (13, 13), (26, 40)])
def test_refine_condition_frames_are_the_last_frames_front_padded(num_cond_frames, frames):
    """LongCatVideoPipeline.refine_condition_frames (PIPE:272-276): the LAST num_cond_frames frames of the video, their first one
    repeated in front up to the padded count; a video with fewer frames than asked for is refused."""
    ncl, added_c, _, _ = LongCatVideoPipeline.refine_padding(num_cond_frames, 186)
    video = torch.arange(frames, dtype=torch.float32).view(1, 1, frames, 1, 1).expand(1, 3, frames, 2, 2)
    got = LongCatVideoPipeline.refine_condition_frames(video, num_cond_frames + added_c, added_c)
    assert tuple(got.shape) == (1, 3, num_cond_frames + added_c, 2, 2) and 1 + (got.shape[2] - 1) // 4 == ncl
    first = frames - num_cond_frames
    assert got[0, 0, :, 0, 0].tolist() == [float(first)] * added_c + [float(f) for f in range(first, frames)]
    with pytest.raises(ValueError):
        LongCatVideoPipeline.refine_condition_frames(video[:, :, :num_cond_frames - 1], num_cond_frames + added_c, added_c)


@pytest.mark.parametrize("chunk,ncl,t1,t2,h,w", [((4, 4, 8), 4, 4, 8, 8, 16), ((4, 4, 4), 8, 4, 12, 8, 8), ((4, 4, 8), 8, 40, 4, 4, 8),
                                                  ((2, 4, 8), 2, 2, 6, 4, 16)])
def test_block_order_slice_does_not_depend_on_the_noise_frame_count(chunk, ncl, t1, t2, h, w):
    """The cache stores K rotated with the first nc rows of the BLOCK-ORDERED RoPE table of the condition-only grid; a step rotates
    its rows with rows nc.. of the (ncl + T) grid's table.  Valid because block order sorts by frame chunk first and ncl is whole
    chunks: the first nc rows of the permutation are the condition tokens whatever T is, and the rows behind them are the noise grid's
    own block order shifted by nc."""
    tpf = h * w
    nc = ncl * tpf
    p0, _ = bsa.block_permutation(ncl, h, w, chunk, "cpu")
    c0, s0 = rope_tables(128, ncl, h, w)
    for T in (t1, t2):
        perm, pos = bsa.block_permutation(ncl + T, h, w, chunk, "cpu")
        cos, sin = rope_tables(128, ncl + T, h, w)
        assert torch.equal(perm[:nc], p0) and int(perm[:nc].max()) == nc - 1
        assert torch.equal(cos[perm.long()][:nc], c0[p0.long()]) and torch.equal(sin[perm.long()][:nc], s0[p0.long()])
        pn, qn = bsa.block_permutation(T, h, w, chunk, "cpu")
        assert torch.equal(perm[nc:] - nc, pn) and torch.equal(pos[nc:] - nc, qn)
        assert torch.equal(perm[nc:] // tpf - ncl, pn // tpf)         # the per-row frame index the AdaLN kernels take


def test_mean_pool_at_validates_before_any_device_work():
    """Every invalid argument is WF_EINVAL (-1) on a machine without a GPU: nothing is launched, the fake pointers are never read."""
    fn = _ffi.lib().wf_lc_mean_pool_blocks_at
    i, o = 1 << 20, 1 << 21  # non-null, 16-byte aligned, never dereferenced
    bad = [(None, 256, o, 4, 1, 2, 256, 128), (i, 256, None, 4, 1, 2, 256, 128), (i + 2, 256, o, 4, 1, 2, 256, 128),
           (i, 256, o + 8, 4, 1, 2, 256, 128), (i, 256, o, 4, 1, 0, 256, 128), (i, 256, o, 4, 1, 2, 0, 128),
           (i, 256, o, 4, 1, 2, -128, 128), (i, 256, o, 0, 0, 2, 256, 128), (i, 256, o, 4, -1, 2, 256, 128),
           (i, 256, o, 4, 1, 2, 256, 32), (i, 256, o, 4, 1, 2, 192, 128), (i, 192, o, 4, 1, 2, 256, 128),
           (i, 256, o, 4, 3, 2, 256, 128), (i, 256, o, 2 ** 31 - 1, 2 ** 31 - 2, 2, 256, 128)]
    for args in bad:
        assert fn(*args, None) == -1, args
        assert b"wf_lc_mean_pool_blocks_at" in _ffi.lib().wf_last_error()


def test_entry_points_and_refusals_without_a_device():
    for name in ("cache_condition_blocks", "forward_tokens_cached_blocks", "forward_cached_blocks"):
        assert callable(getattr(LongCatVideoTransformer3DModel, name))
    assert {"k", "vt", "kcmp", "bsa_indices", "chunk", "sparsity", "cdf_threshold", "wver", "loras", "linear_precision",
            "latent_hw"} <= set(LongCatBlockCondCache.__dataclass_fields__)
    sig = inspect.signature(LongCatVideoPipeline.generate_refine)
    assert sig.parameters["video"].default is None and sig.parameters["use_kv_cache"].default is False
    pipe = LongCatVideoPipeline(vae=None, scheduler=None, dit=None, device="cpu")
    with pytest.raises(ValueError, match="both"):   # PIPE:1332, before anything else is touched
        pipe.generate_refine(None, 128, 128, None, None, image=object(), video=object(), num_cond_frames=5)
    with pytest.raises(ValueError, match="num_cond_frames"):   # a video nobody conditions on, a cache with nothing to hold
        pipe.generate_refine(None, 128, 128, None, None, video=object())
    with pytest.raises(ValueError, match="num_cond_frames"):
        pipe.generate_refine(None, 128, 128, None, None, use_kv_cache=True)
