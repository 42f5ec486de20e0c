"""CPU: the host-side facts LongCat video continuation rests on (worldforge_amd/longcat_dit.py cache_condition / forward_tokens_cached,
longcat_pipeline.py generate_vc); the kernels and the forward are checked on the GPU in tests/test_gpu_longcat_vc.py."""
import inspect

import pytest
import torch

from worldforge_amd import _ffi
from worldforge_amd.longcat_dit import LongCatVideoTransformer3DModel, rope_tables
from worldforge_amd.longcat_pipeline import LongCatVideoPipeline


@pytest.mark.parametrize("n,f1,f2,h,w", [(1, 1, 4, 4, 6), (2, 2, 5, 8, 8), (4, 4, 24, 30, 52), (3, 5, 9, 3, 7)])
def test_rope_rows_of_a_frame_do_not_depend_on_the_frame_count(n, f1, f2, h, w):
    """The cache stores K ALREADY ROTATED (the reference re-rotates per step, attention.py:168-172): valid because the table rows of
    frames 0..n-1 are the same bits in the condition-only grid and in the (condition + noise) grid of every step."""
    tpf = h * w
    c1, s1 = rope_tables(128, f1, h, w)
    c2, s2 = rope_tables(128, f2, h, w)
    assert torch.equal(c1[:n * tpf], c2[:n * tpf]) and torch.equal(s1[:n * tpf], s2[:n * tpf])


@pytest.mark.parametrize("num_cond_frames,ncl", [(1, 1), (5, 2), (13, 4)])
def test_num_cond_latents(num_cond_frames, ncl):
    """pipeline_longcat_video.py:1189; generate_vc refuses a job with no frame left to generate before it touches the device."""
    assert 1 + (num_cond_frames - 1) // 4 == ncl
    pipe = LongCatVideoPipeline(vae=None, scheduler=None, dit=None, device="cpu")
    with pytest.raises(ValueError, match="num_cond_frames"):
        pipe.generate_vc(None, 64, 96, None, None, num_frames=1 + 4 * (ncl - 1), num_cond_frames=num_cond_frames)
    for kw in (dict(offload_kv_cache=True), dict(enhance_hf=True)):
        with pytest.raises(NotImplementedError):
            pipe.generate_vc(None, 64, 96, None, None, **kw)


def test_v_transpose_at_validates_before_any_device_work():
    """Every invalid argument is WF_EINVAL (-1) on a machine without a GPU: nothing is launched, the fake pointers are never read."""
    fn = _ffi.lib().wf_v_transpose_at
    V, Vt = 1 << 20, 1 << 21  # non-null, 16-byte aligned, never dereferenced
    H, ld = 2, 3 * 256
    bad = [(None, ld, Vt, 0, 8, 64, H), (V, ld, None, 0, 8, 64, H),          # null pointer
           (V, ld, Vt, -1, 8, 64, H), (V, ld, Vt, 0, 0, 64, H), (V, ld, Vt, 0, -3, 64, H),   # k0 < 0, L <= 0
           (V, ld, Vt, 60, 8, 64, H), (V, ld, Vt, 2 ** 31 - 8, 64, 2 ** 31 - 64, H),         # k0 + L > Lp (also past int)
           (V, ld, Vt, 0, 8, 100, H), (V, 128, Vt, 0, 8, 64, H), (V, 260, Vt, 0, 8, 64, H)]  # Lp % 64, ld < H * 128, ld % 8
    for args in bad:
        assert fn(*args, None) == -1, args
        assert b"wf_v_transpose_at" in _ffi.lib().wf_last_error()


def test_call_keeps_rejecting_the_reference_cache_protocol():
    sig = inspect.signature(LongCatVideoTransformer3DModel.__call__)
    assert {"return_kv", "kv_cache_dict", "skip_crs_attn"} <= set(sig.parameters)
    for name in ("cache_condition", "forward_tokens_cached", "forward_cached"):
        assert callable(getattr(LongCatVideoTransformer3DModel, name))
