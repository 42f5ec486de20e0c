"""One denoising step of LongCat video continuation on one MI355X: the cached step (forward_tokens_cached on a resident condition cache:
noise frames only) against the uncached step of the existing path (forward_tokens over all frames, num_cond_latents = ncl), in ONE
process, HIP events around every step, after warm-up, the two alternating.

Shape: the released width (hidden 4096, 32 heads, SwiGLU 11008, caption 4096), 93 frames of 480 x 832 = 24 latent frames of 60 x 104 =
1560 tokens per frame, 13 condition frames = 4 condition latent frames; `--depth` blocks (a step's time is linear in the depth: every
block does the same work; the released model has 48).  The uncached step is the code the parent commit runs, so it is the baseline; the
one condition on the cached step is that it is not slower (it does strictly less work).  The FLOP counts computed from the shapes are
written beside the measured ratio, as is the one-off cost of building the cache.
Writes profiles/longcat_vc_cache.md (or --out) and prints one JSON line.

--refine: the same comparison for the block-sparse refine pass of a continued window (forward_tokens_cached_blocks on a block-ordered
condition cache against forward_tokens with block-sparse attention on): 8 condition + 40 noise latent frames (a 93-frame window refined
to 186 frames with 26 condition frames, padded as pipeline_longcat_video.py:1417-1424 does) of 704 x 1280 -- the 720p bucket whose sides
the refine pass accepts (multiples of 64) -- = 44 x 80 tokens, chunk 4 x 4 x 8, sparsity 0.875.  APPENDS its section to the same file.
Usage:  python tools/longcat_vc_bench.py [--refine] [--depth 4] [--reps 6] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from worldforge_amd.longcat_dit import LongCatConfig, LongCatVideoTransformer3DModel  # noqa: E402

DEV = torch.device("cuda:0")


def step_flops(cfg, rows, q_noise, keys, n_cond, n_txt):
    """FLOPs of one step's blocks from the shapes: the token linears on `rows` rows, cross-attention on the q_noise noise rows, the
    noise-query attention over `keys` keys and (uncached only) the condition-query attention over its own n_cond keys."""
    C, Hd, H = cfg.hidden_size, cfg.ffn_hidden, cfg.num_heads
    lin = 2.0 * rows * (3 * C * C + C * C + 2 * Hd * C + Hd * C) + 2.0 * q_noise * 2 * C * C
    attn = 4.0 * 128 * H * (q_noise * keys + n_cond * n_cond + q_noise * n_txt)
    return cfg.depth * (lin + attn)


def refine_step_flops(cfg, rows, q_noise, keys, n_cond, n_txt, keep, blk):
    """The same for the block-sparse pass: every query attends to the `keep` share of its key blocks (int(keep * blocks) of them), and
    the gating scores every query block against every key block it may select (128 channels)."""
    C, Hd, H = cfg.hidden_size, cfg.ffn_hidden, cfg.num_heads
    lin = 2.0 * rows * (3 * C * C + C * C + 2 * Hd * C + Hd * C) + 2.0 * q_noise * 2 * C * C
    sel = lambda n: int(keep * (n // blk)) * blk  # noqa: E731
    attn = 4.0 * 128 * H * (q_noise * sel(keys) + n_cond * sel(n_cond) + q_noise * n_txt)
    gate = 2.0 * 128 * H * ((q_noise // blk) * (keys // blk) + (n_cond // blk) * (n_cond // blk))
    return cfg.depth * (lin + attn + gate)


def refine(a):
    chunk, sparsity = [4, 4, 8], 0.875
    ncl, tn, Hh, Ww = 8, 40, 704 // 8, 1280 // 8
    T, tpf, blk = ncl + tn, (Hh // 2) * (Ww // 2), chunk[0] * chunk[1] * chunk[2]
    cfg = LongCatConfig(depth=a.depth)
    m = LongCatVideoTransformer3DModel(cfg, DEV, enable_bsa=True, bsa_params=dict(sparsity=sparsity, chunk_3d_shape_q=chunk,
                                                                                   chunk_3d_shape_k=chunk)).init_random(seed=1)
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn((16, T, Hh, Ww), generator=g, device=DEV).to(torch.bfloat16)
    n_txt = 256
    cap = (torch.randn((n_txt, cfg.caption_channels), generator=g, device=DEV) * 0.5).to(torch.bfloat16)
    ts = [0.0] * ncl + [400.0] * tn
    cond, noise = x[:, :ncl].contiguous(), x[:, ncl:].contiguous()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        return s, e

    cache = m.cache_condition_blocks(cond)
    run_c = lambda: m.forward_tokens_cached_blocks(noise, ts[ncl:], cap, None, cache)  # noqa: E731
    run_u = lambda: m.forward_tokens(x, ts, cap, None, ncl)  # noqa: E731
    for _ in range(a.warmup):
        oc, ou = run_c(), run_u()
    torch.cuda.synchronize()
    diff = ((oc - ou[:, ncl:]).norm() / ou[:, ncl:].norm()).item()
    del oc, ou
    ev_c, ev_u, ev_b = [], [], []
    for _ in range(a.reps):
        ev_c.append(timed(run_c))
        ev_u.append(timed(run_u))
    for _ in range(2):
        ev_b.append(timed(lambda: m.cache_condition_blocks(cond)))
    torch.cuda.synchronize()
    tc, tu, tb = ([s.elapsed_time(e) for s, e in ev] for ev in (ev_c, ev_u, ev_b))
    L, nc = T * tpf, ncl * tpf
    f_u = refine_step_flops(cfg, L, L - nc, L, nc, n_txt, 1 - sparsity, blk)
    f_c = refine_step_flops(cfg, L - nc, L - nc, L, 0, n_txt, 1 - sparsity, blk)
    props = torch.cuda.get_device_properties(0)
    med = statistics.median
    r = dict(mode="refine", device=props.name, arch=getattr(props, "gcnArchName", ""), depth=a.depth, latent_frames=T,
             cond_latent_frames=ncl, tokens=L, cond_tokens=nc, cached_ms=round(med(tc), 3), cached_min_ms=round(min(tc), 3),
             cached_max_ms=round(max(tc), 3), uncached_ms=round(med(tu), 3), uncached_min_ms=round(min(tu), 3),
             uncached_max_ms=round(max(tu), 3), ratio=round(med(tc) / med(tu), 4), flop_ratio=round(f_c / f_u, 4),
             cache_build_ms=round(med(tb), 3),
             cache_mib=round((cache.k.numel() + cache.vt.numel() + cache.kcmp.numel()) * 2 / 2 ** 20, 1),
             cached_vs_uncached_rel_l2=round(diff, 5), reps=a.reps)
    lines = ["", "## The block-sparse refine pass of a continued window (`--refine`)", "",
             f"Box: {r['device']} ({r['arch']}), torch {torch.__version__}, HIP {torch.version.hip}.  Hidden {cfg.hidden_size}, {cfg.num_heads} "
             f"heads, {a.depth} of the released 48 blocks; {ncl} condition + {tn} noise latent frames of {Hh // 2} x {Ww // 2} = {tpf} tokens "
             f"({L} tokens, {nc} condition), chunk {chunk}, sparsity {sparsity}; caption {n_txt} tokens.  One process, the two steps alternating, "
             f"each between its own HIP events, {a.warmup} warm-up steps each, median (min .. max) of {a.reps}.", "",
             "| step | ms | FLOPs from the shapes |", "|---|---|---|",
             f"| uncached: `forward_tokens`, all {T} frames (the parent commit's code) | {r['uncached_ms']:.3f} ({r['uncached_min_ms']:.3f} .. {r['uncached_max_ms']:.3f}) | {f_u:.4e} |",
             f"| cached: `forward_tokens_cached_blocks`, {tn} noise frames | {r['cached_ms']:.3f} ({r['cached_min_ms']:.3f} .. {r['cached_max_ms']:.3f}) | {f_c:.4e} |", "",
             f"Measured cached / uncached: **{r['ratio']:.4f}**; expected from the FLOP counts: {r['flop_ratio']:.4f}.  The condition: cached "
             f"must not be slower -- {'holds' if r['ratio'] <= 1.0 else 'DOES NOT HOLD'}.", "",
             f"Building the cache (`cache_condition_blocks`, once per window): {r['cache_build_ms']:.3f} ms; it holds {r['cache_mib']:.1f} MiB for "
             f"these {a.depth} blocks.  Noise-frame velocities, cached against uncached, same inputs: rel-L2 {r['cached_vs_uncached_rel_l2']:.5f}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines))
    print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=93)
    ap.add_argument("--cond-frames", type=int, default=13)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--out", default=os.path.join("profiles", "longcat_vc_cache.md"))
    ap.add_argument("--refine", action="store_true", help="the block-sparse refine pass at 8 + 40 latent frames (appends to --out)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a step time is not measured on the CPU")
    if a.refine:
        return refine(a)
    T, ncl = (a.frames - 1) // 4 + 1, 1 + (a.cond_frames - 1) // 4
    Hh, Ww = a.height // 8, a.width // 8
    tpf = (Hh // 2) * (Ww // 2)
    cfg = LongCatConfig(depth=a.depth)
    m = LongCatVideoTransformer3DModel(cfg, DEV).init_random(seed=1)
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn((16, T, Hh, Ww), generator=g, device=DEV).to(torch.bfloat16)
    n_txt = 256
    cap = (torch.randn((n_txt, cfg.caption_channels), generator=g, device=DEV) * 0.5).to(torch.bfloat16)
    ts = [0.0] * ncl + [812.0] * (T - ncl)
    cond, noise = x[:, :ncl].contiguous(), x[:, ncl:].contiguous()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        return s, e, out

    cache = m.cache_condition(cond)
    run_c = lambda: m.forward_tokens_cached(noise, ts[ncl:], cap, None, cache)  # noqa: E731
    run_u = lambda: m.forward_tokens(x, ts, cap, None, ncl)  # noqa: E731
    for _ in range(a.warmup):
        oc, ou = run_c(), run_u()
    torch.cuda.synchronize()
    diff = ((oc - ou[:, ncl:]).norm() / ou[:, ncl:].norm()).item()  # same seeded inputs, the sizes that are timed
    ev_c, ev_u, ev_b = [], [], []
    for _ in range(a.reps):  # alternating: what else runs on the host hits both alike
        ev_c.append(timed(run_c)[:2])
        ev_u.append(timed(run_u)[:2])
    for _ in range(3):
        ev_b.append(timed(lambda: m.cache_condition(cond))[:2])
    torch.cuda.synchronize()
    tc, tu, tb = ([s.elapsed_time(e) for s, e in ev] for ev in (ev_c, ev_u, ev_b))
    L, nc = T * tpf, ncl * tpf
    f_u = step_flops(cfg, L, L - nc, L, nc, n_txt)
    f_c = step_flops(cfg, L - nc, L - nc, L, 0, n_txt)
    props = torch.cuda.get_device_properties(0)
    r = dict(device=props.name, arch=getattr(props, "gcnArchName", ""), depth=a.depth, latent_frames=T, cond_latent_frames=ncl,
             tokens=L, cond_tokens=nc, cached_ms=round(statistics.median(tc), 3), cached_min_ms=round(min(tc), 3),
             cached_max_ms=round(max(tc), 3), uncached_ms=round(statistics.median(tu), 3), uncached_min_ms=round(min(tu), 3),
             uncached_max_ms=round(max(tu), 3), ratio=round(statistics.median(tc) / statistics.median(tu), 4),
             flop_ratio=round(f_c / f_u, 4), cached_tflops=round(f_c / statistics.median(tc) / 1e9, 1),
             uncached_tflops=round(f_u / statistics.median(tu) / 1e9, 1), cache_build_ms=round(statistics.median(tb), 3),
             cache_mib=round((cache.k.numel() + cache.vt.numel()) * 2 / 2 ** 20, 1), cached_vs_uncached_rel_l2=round(diff, 5), reps=a.reps)
    lines = ["# LongCat video continuation: a cached step against an uncached step (tools/longcat_vc_bench.py)", "",
             f"Box: {r['device']} ({r['arch']}), torch {torch.__version__}, HIP {torch.version.hip}.  Hidden {cfg.hidden_size}, {cfg.num_heads} heads, "
             f"{a.depth} of the released 48 blocks; {a.frames} frames of {a.height} x {a.width} = {T} latent frames of {tpf} tokens ({L} tokens), "
             f"{a.cond_frames} condition frames = {ncl} latent frames ({nc} tokens, {nc % 64} past a 64-key tile); caption {n_txt} tokens.  One process, "
             f"the two steps alternating, each between its own HIP events, {a.warmup} warm-up steps each, median (min .. max) of {a.reps}.", "",
             "| step | ms | FLOPs from the shapes | TFLOP/s (whole step) |", "|---|---|---|---|",
             f"| uncached: `forward_tokens`, all {T} frames (the parent commit's code) | {r['uncached_ms']:.3f} ({r['uncached_min_ms']:.3f} .. {r['uncached_max_ms']:.3f}) | {f_u:.4e} | {r['uncached_tflops']:.1f} |",
             f"| cached: `forward_tokens_cached`, {T - ncl} noise frames | {r['cached_ms']:.3f} ({r['cached_min_ms']:.3f} .. {r['cached_max_ms']:.3f}) | {f_c:.4e} | {r['cached_tflops']:.1f} |", "",
             f"Measured cached / uncached: **{r['ratio']:.4f}**; expected from the FLOP counts: {r['flop_ratio']:.4f} (the linears, FFN and norms "
             f"lose {nc} of {L} rows, the condition-query attention launch disappears, the noise-query launch is unchanged).  The condition: "
             f"cached must not be slower -- {'holds' if r['ratio'] <= 1.0 else 'DOES NOT HOLD'}.", "",
             f"Building the cache (`cache_condition`, once per video): {r['cache_build_ms']:.3f} ms; it holds {r['cache_mib']:.1f} MiB for these "
             f"{a.depth} blocks.  Noise-frame velocities, cached against uncached, same inputs: rel-L2 {r['cached_vs_uncached_rel_l2']:.5f}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(r))


if __name__ == "__main__":
    main()
