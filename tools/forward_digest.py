"""Digest of every way the LongCat and the Wan DiT forwards, the VAE and the two samplers can run: for comparing two checkouts bit for bit and
launch for launch.

    python tools/forward_digest.py [--only PREFIX] [--dump DIR] > digest.txt

One seeded random model of the multirank tests' size runs each path on a small grid (the Wan cases are named `wan.`..., the VAE's `vae.`...,
the samplers' `pipe.lc.`... and `pipe.wan.`...; `--only wan.` selects the Wan cases); per case (and per simulated rank) one line (the VAE's with flops=<flops_last> behind it):

    <case> out=<sha256> calls=<n> launches=<sha256> trace=<sha256>

out: every output tensor's bytes (the velocity; a cache's K / V^T / bound / pooled means) and the block selections where there are any.
The launch trace is taken by a recording proxy in place of the loaded library object of `_ffi`: every call to libwf_hip.so is noted with its
name, its scalar arguments as given and every pointer argument replaced by the ordinal of its first appearance in the trace.  `trace` is
the hash of that, `launches` the hash of the same lines without the pointers: the ordinals say which calls share a buffer, and with it
where PyTorch's allocator handed a freed temporary's block out again, which need not repeat from run to run.  Two checkouts whose `out`,
`calls` and `launches` agree and whose `trace` differs issue the same kernels on the same values, with a temporary of another lifetime;
--dump writes the full traces (one file per case) to find it with diff.

Run it twice on one checkout first: what is not stable from run to run there cannot be compared between checkouts.  The digests pin a
build's kernel rounding, not the model's contract: they are compared, never committed.  Uses only the model's public methods."""
import argparse
import ctypes
import hashlib
import os
import sys
import threading

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tests.fakes import SimComm  # noqa: E402
from worldforge_amd import _ffi  # noqa: E402
from worldforge_amd.dit import DiTConfig, WanTransformer3DModel  # noqa: E402
from worldforge_amd.longcat_dit import LongCatConfig, LongCatVideoTransformer3DModel  # noqa: E402

DEV = torch.device("cuda:0")
BF = torch.bfloat16
KW = dict(hidden_size=256, num_heads=2, caption_channels=64, adaln_tembed_dim=64)
_TLS = threading.local()


class _Recorder:
    """Stands where `_ffi` keeps the loaded library: attribute access hands out the real entry point wrapped in a note-taker."""

    def __init__(self, dll, protos):
        self._dll, self._protos, self._fns = dll, protos, {}

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            real = getattr(self._dll, name)
            argtypes = self._protos[name][1] if name in self._protos else None

            def fn(*args, _real=real, _name=name, _types=argtypes):
                trace = getattr(_TLS, "trace", None)
                if trace is not None:
                    trace.append((_name, _types, args))
                return _real(*args)

            self._fns[name] = fn
        return fn


def _install():
    dll = _ffi.lib()
    if not isinstance(dll, _Recorder):
        _ffi._LIB._dll = _Recorder(dll, _ffi._LIB.protos)


def _render(trace):
    """-> (lines with pointer ordinals, lines without pointers)."""
    seen, full, bare = {}, [], []
    for name, types, args in trace:
        a_full, a_bare = [], []
        for j, a in enumerate(args):
            is_ptr = types is not None and j < len(types) and types[j] in (ctypes.c_void_p, ctypes.c_char_p)
            if is_ptr and not isinstance(a, (bytes, ctypes.Array)):
                a_full.append("null" if not a else "p%d" % seen.setdefault(int(a), len(seen)))
            elif isinstance(a, ctypes.Array):
                a_full.append(repr(list(a)))
                a_bare.append(a_full[-1])
            else:
                a_full.append(repr(a))
                a_bare.append(a_full[-1])
        full.append(f"{name}({', '.join(a_full)})")
        bare.append(f"{name}({', '.join(a_bare)})")
    return full, bare


def _hash_into(h, obj):
    if obj is None:
        h.update(b"<none>")
    elif torch.is_tensor(obj):
        t = obj.detach().contiguous().cpu()
        h.update(f"{t.dtype}{tuple(t.shape)}".encode())
        h.update(t.view(torch.uint8).numpy().tobytes())
    elif isinstance(obj, (list, tuple)):
        h.update(f"[{len(obj)}".encode())
        for o in obj:
            _hash_into(h, o)
    elif hasattr(obj, "cpu"):  # a selection as the fused kernels leave it (bsa.SelectionMask / SelectionMaskVar): its index form
        _hash_into(h, obj.cpu())
    else:
        h.update(repr(obj).encode())


def _sha(obj):
    h = hashlib.sha256()
    _hash_into(h, obj)
    return h.hexdigest()[:32]


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _traced(fn):
    """fn() with this thread's library calls recorded -> (what fn returned, trace)."""
    _TLS.trace = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, _TLS.trace
    finally:
        _TLS.trace = None


def _run_ranks(P, fn):
    """tests/test_gpu_multirank.py `_run_ranks`: P simulated ranks as threads of this process; each rank's calls are traced apart."""
    shared = {"slots": [None] * P, "bar": threading.Barrier(P)}
    res, errs = [None] * P, []

    def worker(r):
        try:
            res[r] = _traced(lambda: fn(SimComm(P, r, shared)))
        except Exception as e:
            errs.append(e)
            shared["bar"].abort()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(P)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise errs[0]
    return res


def _model(depth=2, seed=5, **kw):
    return LongCatVideoTransformer3DModel(LongCatConfig(depth=depth, **KW), DEV, **kw).init_random(seed)


def _inputs(T, Hh, Ww, ncl, n_cap=30, t=500.0):
    x = _rand((16, T, Hh, Ww), 60).to(BF).to(DEV)
    cap = _rand((n_cap, 64), 61).to(BF).to(DEV)
    mask = torch.zeros(n_cap, dtype=torch.int64)
    mask[:21] = 1
    return x, cap, mask, [0.0] * ncl + [t] * (T - ncl)


def _bsa_params(chunk=(4, 4, 8), **kw):
    return dict(dict(sparsity=0.5, chunk_3d_shape_q=list(chunk), chunk_3d_shape_k=list(chunk)), **kw)


# ---- the cases: name -> callable returning [(suffix, outputs, trace)] -------------------------------------------------------------------
CASES = {}


def case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


def _single(fn):
    out, trace = _traced(fn)
    return [("", out, trace)]


def _dense(ncl, masked=True, zero_pad=False, **attrs):
    def run():
        cfg = LongCatConfig(depth=2, text_tokens_zero_pad=zero_pad, **KW)
        m = LongCatVideoTransformer3DModel(cfg, DEV).init_random(5)
        for k, v in attrs.items():
            setattr(m, k, v)
        x, cap, mask, ts = _inputs(3, 16, 20, ncl)
        return _single(lambda: m.forward_tokens(x, ts, cap, mask if masked else None, ncl))
    return run


CASES["dense.ncl0.nomask"] = _dense(0, masked=False)
CASES["dense.ncl0.mask"] = _dense(0)
CASES["dense.ncl1.mask"] = _dense(1)
CASES["dense.ncl1.track_max"] = _dense(1, attn_track_max=True)
CASES["dense.ncl1.no_prescale"] = _dense(1, attn_prescale=False)
CASES["dense.ncl1.zero_pad"] = _dense(1, zero_pad=True)


def _ranks(P, thw, exchange, seed=5, **model_kw):
    def run():
        m0 = _model(seed=seed, **model_kw)
        ncl = 4 if model_kw.get("enable_bsa") else 1
        x, cap, mask, ts = _inputs(*thw, ncl)

        def rank_fn(comm):
            m = LongCatVideoTransformer3DModel(m0.cfg, DEV, comm=comm, **model_kw)
            m.w = m0.w
            if exchange is not None:
                m.exchange_mode, m.exchange_chunks = exchange
            out = m.forward_tokens(x, ts, cap, None if model_kw.get("enable_bsa") else mask, ncl).clone()
            return out, m.last_bsa_indices

        return [(f".rank{r}", out, trace) for r, (out, trace) in enumerate(_run_ranks(P, rank_fn))]
    return run


for _P, _thw in ((2, (3, 16, 20)), (3, (5, 16, 24))):
    for _ex in (("gather", 1), ("chunked", 2), ("bcast", 1)):
        CASES[f"ranks{_P}.{_ex[0]}{_ex[1]}"] = _ranks(_P, _thw, _ex)


@case("ranks2.cfg_lockstep")
def _cfg_lockstep():
    m0 = _model(depth=3)
    T, Hh, Ww, ncl = 5, 16, 24, 1
    xs = _rand((2, 16, T, Hh, Ww), 60).to(BF).to(DEV)
    caps = _rand((2, 1, 30, 64), 61).to(BF).to(DEV)
    masks = torch.zeros(2, 30, dtype=torch.int64)
    masks[0, :21] = 1
    masks[1, :9] = 1
    tstep = torch.tensor([[0.0] * ncl + [500.0] * (T - ncl)] * 2)

    def rank_fn(comm):
        m = LongCatVideoTransformer3DModel(m0.cfg, DEV, comm=comm)
        m.w = m0.w
        return m(xs, tstep, caps, masks, num_cond_latents=ncl).clone()

    return [(f".rank{r}", out, trace) for r, (out, trace) in enumerate(_run_ranks(2, rank_fn))]


def _bsa(params, env=None, ncl=4):
    def run():
        m = _model(seed=6, enable_bsa=True, bsa_params=params)
        x, cap, _, ts = _inputs(8, 16, 32, ncl, n_cap=20, t=400.0)
        old = os.environ.get("WF_BSA_TORCH_SELECT")
        if env:
            os.environ["WF_BSA_TORCH_SELECT"] = "1"
        try:
            return _single(lambda: (m.forward_tokens(x, ts, cap, None, ncl), m.last_bsa_indices))
        finally:
            if env:
                os.environ.pop("WF_BSA_TORCH_SELECT")
                if old is not None:
                    os.environ["WF_BSA_TORCH_SELECT"] = old
    return run


CASES["bsa.topk.ncl4"] = _bsa(_bsa_params())
CASES["bsa.topk.ncl0"] = _bsa(_bsa_params(), ncl=0)
CASES["bsa.cdf"] = _bsa(_bsa_params(cdf_threshold=0.9))
CASES["bsa.cdf_only"] = _bsa(_bsa_params(cdf_threshold=0.9, sparsity=None))
CASES["bsa.topk.torch_select"] = _bsa(_bsa_params(), env=True)
CASES["bsa.cdf.torch_select"] = _bsa(_bsa_params(cdf_threshold=0.9), env=True)
CASES["bsa.blocks64"] = _bsa(_bsa_params((4, 4, 4)))
CASES["bsa.ranks2"] = _ranks(2, (8, 16, 32), None, seed=6, enable_bsa=True, bsa_params=_bsa_params())


def _dense_cache(track_max):
    def run():
        m = _model(depth=3, seed=4)
        m.attn_track_max = track_max
        ncl, tn = 1, 3
        x, cap, mask, ts = _inputs(ncl + tn, 8, 12, ncl, t=812.0)

        def go():
            cache = m.cache_condition(x[:, :ncl].contiguous())
            out = m.forward_cached(x[None, :, ncl:].contiguous(), torch.tensor([ts[ncl:]]), cap[None, None], mask[None], cache)
            return out, cache.k, cache.vt, cache.kmax2

        return _single(go)
    return run


CASES["cache.dense"] = _dense_cache(False)
CASES["cache.dense.track_max"] = _dense_cache(True)


def _block_cache(chunk, Hh, Ww, ncl, tn, **params):
    def run():
        m = _model(seed=6, enable_bsa=True, bsa_params=_bsa_params(chunk, **params))
        x, cap, _, ts = _inputs(ncl + tn, Hh, Ww, ncl, n_cap=20, t=400.0)

        def go():
            cache = m.cache_condition_blocks(x[:, :ncl].contiguous())
            out = m.forward_cached_blocks(x[None, :, ncl:].contiguous(), torch.tensor([ts[ncl:]]), cap[None, None], None, cache)
            return out, cache.k, cache.vt, cache.kcmp, cache.bsa_indices, m.last_bsa_indices

        return _single(go)
    return run


CASES["cache.blocks.128"] = _block_cache((4, 4, 8), 16, 32, 4, 8)
CASES["cache.blocks.64"] = _block_cache((4, 4, 4), 16, 16, 8, 4)
CASES["cache.blocks.cdf"] = _block_cache((4, 4, 8), 16, 32, 4, 4, cdf_threshold=0.9)


@case("mxfp8.ncl1")
def _mxfp8():
    m = _model(linear_precision="mxfp8")
    x, cap, mask, ts = _inputs(4, 8, 12, 1)
    return _single(lambda: m.forward_tokens(x, ts, cap, mask, 1))


# ---- the Wan DiT: the model and inputs of tests/test_gpu_multirank.py; every case traces TWO consecutive forwards (or CFG pairs), so that
# the second one finds the prompt-context cache filled ----------------------------------------------------------------------------------
def _wan_model(layers=2, **kw):
    cfg = DiTConfig(dim=256, ffn_dim=512, num_heads=2, num_layers=layers, text_dim=64)
    return WanTransformer3DModel(cfg, DEV, **kw).init_random(5)


def _wan_inputs(T, Hh, Ww):
    """-> latents, text, a second (shorter) text, image."""
    return (_rand((36, T, Hh, Ww), 60).to(BF).to(DEV), _rand((30, 64), 61).to(BF).to(DEV), _rand((12, 64), 72).to(BF).to(DEV),
            _rand((257, 1280), 62).to(BF).to(DEV))


def _twice(fn):
    return lambda: [fn(), fn()]


def _env_ctx_cache_off(run):
    """run() with WF_CTX_CACHE=0 (read by every forward; set around the whole case, simulated ranks included)."""
    def wrapped():
        old = os.environ.get("WF_CTX_CACHE")
        os.environ["WF_CTX_CACHE"] = "0"
        try:
            return run()
        finally:
            os.environ.pop("WF_CTX_CACHE")
            if old is not None:
                os.environ["WF_CTX_CACHE"] = old
    return wrapped


def _wan_single(layers=2, pair=None, model_kw=None, **attrs):
    """pair: None = forward_tokens, "tokens" = forward_tokens_pair, "cfg" = forward_cfg_pair, "call" = __call__ with a batch dimension."""
    def run():
        m = _wan_model(layers, **(model_kw or {}))
        for k, v in attrs.items():
            setattr(m, k, v)
        x, text, text_b, img = _wan_inputs(3, 16, 20)
        fn = {None: lambda: m.forward_tokens(x, 500.0, text, img),
              "call": lambda: m(x[None], torch.tensor([500.0]), text[None], img[None])[0],
              "tokens": lambda: m.forward_tokens_pair(x, 500.0, text, text_b, img),
              "cfg": lambda: m.forward_cfg_pair(x[None], torch.tensor([500.0]), text[None], text_b[None], img[None])}[pair]
        return _single(_twice(fn))
    return run


CASES["wan.default"] = _wan_single()
CASES["wan.track_max"] = _wan_single(attn_track_max=True)
CASES["wan.no_prescale"] = _wan_single(attn_prescale=False)
CASES["wan.no_ctx_cache"] = _env_ctx_cache_off(_wan_single())
CASES["wan.mxfp8"] = _wan_single(model_kw=dict(linear_precision="mxfp8"))
CASES["wan.call"] = _wan_single(pair="call")
CASES["wan.pair.share"] = _wan_single(3, "tokens", pair_share_layer0=True)
CASES["wan.pair.no_share"] = _wan_single(3, "tokens", pair_share_layer0=False)
CASES["wan.pair.share.no_ctx_cache"] = _env_ctx_cache_off(_wan_single(3, "tokens", pair_share_layer0=True))
CASES["wan.pair.cfg_pair"] = _wan_single(3, "cfg")


def _wan_ranks(P, thw, exchange, layers=2, pair=False, **attrs):
    def run():
        m0 = _wan_model(layers)
        x, text, text_b, img = _wan_inputs(*thw)

        def rank_fn(comm):
            m = WanTransformer3DModel(m0.cfg, DEV, comm=comm)
            m.w = m0.w
            if exchange is not None:
                m.exchange_mode, m.exchange_chunks = exchange
            for k, v in attrs.items():
                setattr(m, k, v)
            if pair:
                return _twice(lambda: [t.clone() for t in m.forward_tokens_pair(x, 500.0, text, text_b, img)])()
            return _twice(lambda: m.forward_tokens(x, 500.0, text, img).clone())()

        return [(f".rank{r}", out, trace) for r, (out, trace) in enumerate(_run_ranks(P, rank_fn))]
    return run


for _ex in (("gather", 1), ("chunked", 2), ("bcast", 1)):
    for _P, _thw in ((2, (3, 16, 20)), (3, (5, 16, 24))):   # (2 layers at P = 3: rank 2 owns no context layer)
        CASES[f"wan.ranks{_P}.{_ex[0]}{_ex[1]}"] = _wan_ranks(_P, _thw, _ex)
    CASES[f"wan.ranks2.layers3.{_ex[0]}{_ex[1]}"] = _wan_ranks(2, (3, 16, 20), _ex, layers=3)   # (an uneven layer count per rank)
CASES["wan.ranks2.no_ctx_cache"] = _env_ctx_cache_off(_wan_ranks(2, (3, 16, 20), None))
CASES["wan.ranks2.pair.lockstep"] = _wan_ranks(2, (3, 16, 20), None, layers=3, pair=True)
CASES["wan.ranks2.pair.sequential"] = _wan_ranks(2, (3, 16, 20), None, layers=3, pair=True, pair_lockstep=False)
CASES["wan.ranks2.pair.lockstep.no_prescale"] = _wan_ranks(2, (3, 16, 20), None, layers=3, pair=True, attn_prescale=False)  # (-> "gather")


# ---- the VAE (`vae.`...): one seeded model per precision, whole frames and as P simulated ranks on row slabs; the shapes of
# tests/test_gpu_vae.py's sharded tests (stage-0 row groups of 1 and of 2 ranks, an odd first-up slab row, a crop that is taken -- the
# "right" mask -- and one that is refused -- "rand"), and one-frame inputs for the T == 1 branches.  Lines carry flops=<flops_last> --------
_VAE_W = {}


def _vae(prec, comm=None):
    from oracle import vae as ovae
    from worldforge_amd.vae import AutoencoderKLWan
    if prec not in _VAE_W:
        _VAE_W[prec] = AutoencoderKLWan(DEV, precision=prec).load_state_dict(ovae.random_weights(seed=5)).w
    m = AutoencoderKLWan(DEV, comm=comm, precision=prec)
    m.w = _VAE_W[prec]
    return m


def _vae_op(what, H, T):
    """-> fn(model) -> outputs, on inputs made once (shared by the simulated ranks)."""
    if what in ("encode", "decode"):
        g = torch.Generator().manual_seed(21)
        x = (torch.rand(1, 3, 4 * T - 3, H, 48, generator=g) * 2 - 1).to(DEV)
        z = torch.randn(1, 16, T, H // 8, 6, generator=g).to(DEV)
        if what == "decode":
            return lambda m: m.decode(z, return_dict=False)[0].clone()

        def encode(m):
            post = m.encode(x).latent_dist
            return post.mode().clone(), post.sample(torch.Generator().manual_seed(1))
        return encode
    from tests.test_gpu_vae import _hole_mask
    g = torch.Generator().manual_seed(33)
    z = torch.randn(1, 16, T, H // 8, 32, generator=g).to(DEV)
    ref = torch.rand(1, 3, 4 * T - 3, H, 256, generator=g).to(DEV)
    mask = _hole_mask(4 * T - 3, H, 256, what.split(".")[1]).to(DEV)
    return lambda m: m.decode_blend_encode(z, ref, mask).mode().clone()


def _vae_case(prec, what, H, T=3, P=1):
    def run():
        op = _vae_op(what, H, T)
        _vae(prec)   # (the weights, before any thread asks for them)

        def go(comm=None):
            m = _vae(prec, comm)
            assert P == 1 or m.can_shard(H // 8)
            out = op(m)
            m.check_range()
            return out, m.flops_last

        res = [_traced(go)] if P == 1 else _run_ranks(P, go)
        return [("" if P == 1 else f".rank{r}", out, trace, flops) for r, ((out, flops), trace) in enumerate(res)]
    return run


for _prec in ("bf16", "fp16x3", "bf16x3", "fp16"):
    for _P, _H in ((1, 64), (2, 64), (4, 64), (8, 64), (2, 24), (8, 96)):
        for _what in ("encode", "decode", "dbe.right", "dbe.rand"):
            CASES[f"vae.{_prec}.P{_P}.H{_H}.{_what}"] = _vae_case(_prec, _what, _H, P=_P)
    for _P in (1, 2):
        for _what in ("encode", "decode"):
            CASES[f"vae.{_prec}.P{_P}.H64.T1.{_what}"] = _vae_case(_prec, _what, 64, T=1, P=_P)


# ---- the two samplers (`pipe.`...): a seeded small real DiT and the real scheduler behind tests.fakes.FakeVAE, a CPU generator, 3 steps.
# Every case traces the job twice, once for the frames ("np") and once for output_type="latent" --------------------------------------------
def _both_outputs(job):
    """job(output_type) -> what it returns -> [the frames as a tensor, the latents]."""
    return lambda: [torch.from_numpy(job("np")), job("latent")]


def _prompts(n=24):
    """-> (positive, negative) embeddings [1, 1, n, 64] and their masks [1, n]."""
    pe, ne = (_rand((1, 1, n, 64), 7) * 0.5).to(BF), (_rand((1, 1, n, 64), 8) * 0.5).to(BF)
    pm, nm = torch.zeros(1, n, dtype=torch.int64), torch.zeros(1, n, dtype=torch.int64)
    pm[:, :19] = 1
    nm[:, :7] = 1
    return pe, ne, pm, nm


def _guide(Fr, H, W):
    from tests.fakes import synthetic_ref_and_mask
    ref, mask = synthetic_ref_and_mask(Fr, H, W)
    return dict(video_ref=ref, mask=mask, guided=True, resample_steps=2, guide_steps=2, resample_round=2, use_pca_channel_selection=True,
                static=True)


def _lc_pipe(m, vae_dtype=torch.float32):
    from tests.fakes import FakeVAE
    from worldforge_amd.longcat_pipeline import LongCatVideoPipeline
    from worldforge_amd.longcat_scheduler import FlowMatchEulerDiscreteScheduler
    return LongCatVideoPipeline(FakeVAE(vae_dtype), FlowMatchEulerDiscreteScheduler(shift=3.0, flow_backend="tdiff"), m, device=DEV)


def _lc_i2v(guidance=1.0, guided=False, P=1, **kw):
    """generate_i2v on the latent grid (3, 16, 20).  P = 2: `cfg_split`, one CFG sample per simulated rank."""
    def run():
        Fr, H, W = 9, 128, 160
        m0 = _model()
        pe, ne, pm, nm = _prompts()
        image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3))
        extra = dict(_guide(Fr, H, W) if guided else {}, **kw)

        def go(world=None):
            m = m0
            if world is not None:
                m = LongCatVideoTransformer3DModel(m0.cfg, DEV)
                m.w = m0.w
            pipe = _lc_pipe(m)
            if world is not None:
                pipe.cfg_split = (world, world.split(2).group_index)
            return _both_outputs(lambda ot: pipe.generate_i2v(
                image=image, height=H, width=W, prompt_embeds=pe, prompt_attention_mask=pm, negative_prompt_embeds=ne,
                negative_prompt_attention_mask=nm, num_frames=Fr, num_inference_steps=3, guidance_scale=guidance,
                generator=torch.Generator().manual_seed(42), output_type=ot, **extra))()

        if P == 1:
            return _single(go)
        return [(f".rank{r}", out, trace) for r, (out, trace) in enumerate(_run_ranks(P, go))]
    return run


CASES["pipe.lc.i2v.nocfg"] = _lc_i2v()
CASES["pipe.lc.i2v.cfg"] = _lc_i2v(4.0)
CASES["pipe.lc.i2v.guided_dsg"] = _lc_i2v(4.0, guided=True)
CASES["pipe.lc.i2v.distill"] = _lc_i2v(use_distill=True)
CASES["pipe.lc.i2v.cfg_split.ranks2"] = _lc_i2v(4.0, P=2)


def _lc_vc(use_kv_cache, guidance):
    """generate_vc on the latent grid (4, 8, 12): 2 condition and 2 noise frames."""
    def run():
        m = _model(depth=3, seed=4)
        pe, ne, pm, nm = _prompts()
        video = torch.rand(3, 9, 64, 96, generator=torch.Generator().manual_seed(3))
        pipe = _lc_pipe(m)
        return _single(_both_outputs(lambda ot: pipe.generate_vc(
            video, 64, 96, pe, pm, negative_prompt_embeds=ne, negative_prompt_attention_mask=nm, num_frames=13, num_cond_frames=5,
            num_inference_steps=3, guidance_scale=guidance, generator=torch.Generator().manual_seed(42), output_type=ot,
            use_kv_cache=use_kv_cache)))
    return run


for _use in (True, False):
    for _g in (1.0, 4.0):
        CASES[f"pipe.lc.vc.{'cached' if _use else 'uncached'}.{'cfg' if _g > 1 else 'nocfg'}"] = _lc_vc(_use, _g)


def _lc_refine(cond=None, vae_dtype=torch.float32, **kw):
    """generate_refine of 5 stage-1 frames of 64 x 64 to 128 x 128 (4 latent frames of 8 x 8 tokens per block of the (4, 4, 8) chunks), 4
    inference steps cut at t_thresh = 0.5.  cond: None, "image" or "video"."""
    def run():
        m = _model(seed=6, enable_bsa=True, bsa_params=_bsa_params())
        pe, _, pm, _ = _prompts()
        g = torch.Generator().manual_seed(3)
        stage1 = (torch.rand(5, 64, 64, 3, generator=g) * 255).to(torch.uint8)
        given = {None: {}, "image": dict(image=torch.rand(3, 128, 128, generator=g), num_cond_frames=1),
                 "video": dict(video=(torch.rand(7, 128, 128, 3, generator=g) * 255).to(torch.uint8), num_cond_frames=5)}[cond]
        pipe = _lc_pipe(m, vae_dtype)
        return _single(_both_outputs(lambda ot: pipe.generate_refine(
            stage1, 128, 128, pe, pm, num_inference_steps=4, generator=torch.Generator().manual_seed(42), output_type=ot, **given, **kw)))
    return run


CASES["pipe.lc.refine.plain"] = _lc_refine()
CASES["pipe.lc.refine.image"] = _lc_refine("image")
CASES["pipe.lc.refine.video.cached"] = _lc_refine("video", use_kv_cache=True)
CASES["pipe.lc.refine.video.uncached"] = _lc_refine("video")
CASES["pipe.lc.refine.spatial_only"] = _lc_refine("image", spatial_refine_only=True)
CASES["pipe.lc.refine.vae_bf16"] = _lc_refine("image", vae_dtype=BF)


class _NoPairMethod:
    """A Wan DiT without forward_cfg_pair: the sampler then makes two plain calls."""

    def __init__(self, m):
        self._m, self.dtype = m, m.dtype

    def __call__(self, *a, **k):
        return self._m(*a, **k)


def _wan_pipe_case(guidance=1.0, guided=False, P=1, no_pair=False, latent_only=False, **kw):
    """WanImageToVideoPipeline.__call__ on the latent grid (3, 16, 20).  P = 2: `cfg_split`, one CFG branch per simulated rank."""
    def run():
        from tests.fakes import FakeVAE
        from worldforge_amd.pipeline import WanImageToVideoPipeline
        from worldforge_amd.scheduler import UniPCMultistepScheduler
        Fr, H, W = 9, 128, 160
        m0 = _wan_model()
        text, neg, img = (_rand((1, 30, 64), 7) * 0.5).to(BF), (_rand((1, 30, 64), 8) * 0.5).to(BF), _rand((1, 257, 1280), 9).to(BF)
        image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3))
        extra = dict(_guide(Fr, H, W) if guided else {}, **kw)

        def go(world=None):
            m = m0
            if world is not None:
                m = WanTransformer3DModel(m0.cfg, DEV)
                m.w = m0.w
            pipe = WanImageToVideoPipeline(_NoPairMethod(m) if no_pair else m, FakeVAE(),
                                           UniPCMultistepScheduler(flow_shift=3.0, flow_backend="tdiff"), device=DEV)
            if world is not None:
                pipe.cfg_split = (world, world.split(2).group_index)

            def job(ot):
                return pipe(image=image, height=H, width=W, num_frames=Fr, num_inference_steps=3, guidance_scale=guidance,
                            generator=torch.Generator().manual_seed(42), prompt_embeds=text, negative_prompt_embeds=neg,
                            image_embeds=img, output_type=ot, return_dict=False, **extra)[0]
            return job("latent") if latent_only else _both_outputs(job)()

        if P == 1:
            return _single(go)
        return [(f".rank{r}", out, trace) for r, (out, trace) in enumerate(_run_ranks(P, go))]
    return run


CASES["pipe.wan.nocfg"] = _wan_pipe_case()
CASES["pipe.wan.cfg_pair"] = _wan_pipe_case(4.0)
CASES["pipe.wan.cfg_two_calls"] = _wan_pipe_case(4.0, no_pair=True)
CASES["pipe.wan.guided_dsg"] = _wan_pipe_case(4.0, guided=True)
CASES["pipe.wan.cfg_split.ranks2"] = _wan_pipe_case(4.0, P=2)
CASES["pipe.wan.window"] = _wan_pipe_case(4.0, start_step=1, max_steps=2)
CASES["pipe.wan.latent"] = _wan_pipe_case(latent_only=True)


def main():
    ap =argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default="", help="run the cases whose name starts with this")
    ap.add_argument("--dump", default=None, help="folder for the full traces, one file per case")
    args = ap.parse_args()
    _install()
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    for name, fn in CASES.items():
        if not name.startswith(args.only):
            continue
        try:
            rows = fn()
        except (ValueError, NotImplementedError, AssertionError) as e:  # a host-side refusal; anything else ends the run
            print(f"{name} ERROR {type(e).__name__}: {e}", flush=True)
            continue
        for suffix, out, trace, *flops in rows:
            full, bare = _render(trace)
            print(f"{name}{suffix} out={_sha(out)} calls={len(full)} launches={_sha(bare)} trace={_sha(full)}"
                  + "".join(f" flops={v}" for v in flops), flush=True)
            if args.dump:
                with open(os.path.join(args.dump, f"{name}{suffix}.txt"), "w") as f:
                    f.write("\n".join(full) + "\n")


if __name__ == "__main__":
    main()
