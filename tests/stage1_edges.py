"""Stage 1 at its edges, on the CPU: what the GPU tests of the forward splat and of the crack filling need beyond a restatement's outputs.

  splat_candidates   per target pixel of one camera, the nearest z and the SET of sources that reach it with exactly that z (numpy float64,
                     the statements of oracle/warp.splat): a written colour must be that of one member, untorn; the engine's rule among
                     bit-equal z is the lowest source raster index
  tie / behind / mixed-sign / band / wrap scenes      the inputs of the splat cases, with the conditions they must meet measured here
  outlier_decisions, fill_decisions                   the outlier test and the closing of tests/stage1_cases.py restated per pixel, with a
                     switch that makes them blind beyond the pixel's own 64 x 16 tile (what a kernel with a wrong halo would compute)
  corner_views, wide_view, sparse_view                the inputs of the crack-fill cases

The reference package is never imported here."""
import numpy as np

from oracle import crackfill as ocf

TW, TH = 64, 16                                   # the tile of wf_crack_fill_ex's workgroups
SPLAT_GRID = 16384 * 256                          # threads of the splat's capped grid
LINEAR_GRID = 1024 * 256                          # threads per view of the crack fill's capped linear grids
HALF_EPS = 1e-9


# ---- the splat ------------------------------------------------------------------------------------------------------------------------------
def splat_world(depth, intrinsic, extrinsic):
    """oracle.warp.splat up to the world points: (world [3, H W] float64, valid [H W])."""
    H, W = depth.shape
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pixels = np.stack([x.flatten(), y.flatten(), np.ones_like(x.flatten())], axis=-1)
    cam = np.linalg.inv(intrinsic) @ pixels.T
    d = depth.flatten()
    with np.errstate(invalid="ignore"):
        valid = ~np.isnan(d) & (d > 0)
        p3 = np.zeros_like(cam)
        p3[:, valid] = cam[:, valid] * d[valid]
        R, t = extrinsic[:3, :3], extrinsic[:3, 3]
        world = R.T @ p3 + (-R.T @ t)[:, None]
    return world, valid


def splat_candidates(depth, intrinsic, extrinsic, new_cam, world=None):
    """One camera of oracle.warp.splat, per target pixel (flat index v W + u) instead of per winner.  Returns a dict:
      hit [H W] bool, zmin [H W] float64 (NaN where nothing lands), nland [H W] sources that land, ncand [H W] sources that land with
      z == zmin, lowest [H W] the smallest candidate source index (-1 where nothing lands), cand_t / cand_src the candidate pairs
      (target, source), src_t / src / src_z every landing source, has_pos / has_neg [H W] a source with z > 0 / z < 0 lands,
      band_u / band_v number of sources whose round(u) == W / round(v) == H is clipped, margin the smallest distance of a landing
      source's u or v from a half-integer, unstable [H W] targets whose candidate set changes when every source within HALF_EPS of a
      half-integer is rounded to the other side."""
    H, W = depth.shape
    if world is None:
        world = splat_world(depth, intrinsic, extrinsic)
    world, valid = world
    n = H * W
    out = dict(hit=np.zeros(n, bool), zmin=np.full(n, np.nan), nland=np.zeros(n, np.int64), ncand=np.zeros(n, np.int64),
               lowest=np.full(n, -1, np.int64), cand_t=np.zeros(0, np.int64), cand_src=np.zeros(0, np.int64), src_t=np.zeros(0, np.int64),
               src=np.zeros(0, np.int64), src_z=np.zeros(0), has_pos=np.zeros(n, bool), has_neg=np.zeros(n, bool), band_u=0, band_v=0,
               margin=np.inf, unstable=np.zeros(n, bool))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pc = new_cam[:3, :3] @ world + new_cam[:3, 3][:, None]
        vz = (np.abs(pc[2]) > 1e-6) & valid
        if vz.sum() == 0:
            return out
        wp = np.zeros((3, pc.shape[1]))
        wp[:, vz] = intrinsic @ (pc[:, vz] / pc[2, vz])
        u, v = wp[0], wp[1]
        ok = (u >= 0) & (u < W) & (v >= 0) & (v < H) & vz
    src = np.nonzero(ok)[0]
    if src.size == 0:
        return out
    u, v, z = u[src], v[src], pc[2, src]
    ur, vr = np.round(u).astype(np.int32), np.round(v).astype(np.int32)
    un, vn = np.clip(ur, 0, W - 1), np.clip(vr, 0, H - 1)
    t = vn.astype(np.int64) * W + un
    zmin = np.full(n, np.inf)
    np.minimum.at(zmin, t, z)
    is_c = z == zmin[t]
    out["hit"] = np.bincount(t, minlength=n) > 0
    out["nland"] = np.bincount(t, minlength=n)
    out["ncand"] = np.bincount(t[is_c], minlength=n)
    out["zmin"] = np.where(out["hit"], zmin, np.nan)
    low = np.full(n, n, np.int64)
    np.minimum.at(low, t[is_c], src[is_c])
    out["lowest"] = np.where(out["hit"], low, -1)
    out["cand_t"], out["cand_src"] = t[is_c], src[is_c]
    out["src_t"], out["src"], out["src_z"] = t, src, z
    out["has_pos"] = np.bincount(t[z > 0], minlength=n) > 0
    out["has_neg"] = np.bincount(t[z < 0], minlength=n) > 0
    out["band_u"], out["band_v"] = int((ur == W).sum()), int((vr == H).sum())
    du, dv = np.abs(u - np.floor(u) - 0.5), np.abs(v - np.floor(v) - 0.5)
    out["margin"] = float(min(du.min(), dv.min()))
    unstable = out["unstable"]
    for k in np.nonzero((du < HALF_EPS) | (dv < HALF_EPS))[0]:
        ua = [un[k]] + ([int(np.clip(2 * np.floor(u[k]) + 1 - ur[k], 0, W - 1))] if du[k] < HALF_EPS else [])
        va = [vn[k]] + ([int(np.clip(2 * np.floor(v[k]) + 1 - vr[k], 0, H - 1))] if dv[k] < HALF_EPS else [])
        for a in ua:
            for b in va:
                t2 = b * W + a
                if t2 == t[k]:
                    unstable[t2] |= bool(is_c[k])                       # leaves a set it is a member of
                else:
                    unstable[t2] |= not (z[k] > zmin[t2])               # joins, or takes over, the set of the other pixel
    return out


def check_colours(got_u8, image, cand, label=""):
    """got_u8 [H, W, 3] of one camera: every hit target outside cand["unstable"] carries the u8 triple of ONE source of its candidate set.
    Returns (hit targets, excluded targets, tied targets)."""
    flat = got_u8.reshape(-1, 3)
    src_u8 = (image.reshape(-1, 3)[cand["cand_src"]] * 255).astype(np.uint8)
    match = (src_u8 == flat[cand["cand_t"]]).all(-1)
    member = np.bincount(cand["cand_t"][match], minlength=flat.shape[0]) > 0
    look = cand["hit"] & ~cand["unstable"]
    bad = look & ~member
    assert not bad.any(), (label, int(bad.sum()), np.nonzero(bad)[0][:8])
    return int(cand["hit"].sum()), int((cand["hit"] & cand["unstable"]).sum()), int((cand["ncand"] > 1).sum())


def lowest_colours(image, cand):
    """u8 [H W, 3]: the colour of the lowest candidate source per target (zeros where nothing lands): the engine's tie rule."""
    out = np.zeros((cand["hit"].size, 3), np.uint8)
    out[cand["hit"]] = (image.reshape(-1, 3)[cand["lowest"][cand["hit"]]] * 255).astype(np.uint8)
    return out


def _cam(R=None, t=(0.0, 0.0, 0.0)):
    c = np.eye(4)
    if R is not None:
        c[:3, :3] = R
    c[:3, 3] = t
    return c


def _roty(th):
    return np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])


K_SMALL = np.array([[50.0, 0, 27.3], [0, 50.0, 19.4], [0, 0, 1]])
TIE_TZ = (2.0, 3.0)


def tie_case():
    """Constant depth under a pure translation along z: every target that is hit at all is hit by several sources of bit-equal z.
    -> (image, depth, K, E, cameras)."""
    H, W = 40, 56
    image = np.random.default_rng(21).random((H, W, 3)).astype(np.float32)
    return image, np.full((H, W), 2.0, np.float32), K_SMALL, np.eye(4), [_cam(t=(0, 0, tz)) for tz in TIE_TZ]


def behind_case():
    """A camera turned by 180 degrees about y: every source is behind it (z < 0), and some round to u == W."""
    H, W = 40, 56
    image = np.random.default_rng(22).random((H, W, 3)).astype(np.float32)
    return image, np.full((H, W), 2.0, np.float32), K_SMALL, np.eye(4), [_cam(np.diag([-1.0, 1.0, -1.0]), (0.3, 0.0, 1.0))]


def mixed_sign_case(invalid=False):
    """Two depth layers in 3 x 3 cells, the camera moved forward between them and turned slightly: the near layer is behind it (z < 0),
    the far one in front, and both reach the same targets.  invalid: a few 0, negative, NaN and +inf depths on top."""
    H, W = 40, 56
    rng = np.random.default_rng(23)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    near = ((yy // 3 + xx // 3) % 2) == 0
    depth = (np.where(near, 1.0, 3.0) + 0.05 * np.sin(xx / 5.0) + 0.03 * np.cos(yy / 4.0)).astype(np.float32)
    if invalid:
        for k, bad in enumerate((0.0, -1.5, np.nan, np.inf, -0.0, -np.inf)):
            depth[3 + 5 * k, 4 + 7 * k:4 + 7 * k + 3] = bad
            depth[30 - 4 * k, 50 - 6 * k] = bad
    image = rng.random((H, W, 3)).astype(np.float32)
    return image, depth, K_SMALL, np.eye(4), [_cam(_roty(0.04), (0.05, -0.02, -2.0))]


def band_case():
    """Sinusoidal depth under a pure sideways shift (x and y): sources whose u lies in [W - 0.5, W) or whose v lies in [H - 0.5, H) round to
    W / H and are clipped back to the last column / row."""
    H, W = 40, 56
    rng = np.random.default_rng(24)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = (3.0 + np.sin(xx / 4.0) + 0.5 * np.cos(yy / 3.1)).astype(np.float32)
    depth[rng.random((H, W)) < 0.02] = np.nan
    image = rng.random((H, W, 3)).astype(np.float32)
    return image, depth, K_SMALL, np.eye(4), [_cam(t=(0.97, 0.0, 0.0)), _cam(t=(0.4, 0.9, 0.0)), _cam(t=(-0.5, -0.7, 0.0))]


WRAP_FRAMES = 220


def wrap_case():
    """120 x 160 and 219 cameras: n H W just above the splat's 16384 x 256 threads, so the grid-stride loop takes a second step.  A
    slanted plane with a nearer box and 1 % NaN."""
    from worldforge_amd import warp
    H, W = 120, 160
    rng = np.random.default_rng(25)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = (3.0 + 0.01 * xx + 0.004 * yy + 0.2 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.float32)
    depth[H // 3:2 * H // 3, W // 3:W // 2] = (1.6 + 0.002 * xx + 0.001 * yy).astype(np.float32)[H // 3:2 * H // 3, W // 3:W // 2]
    depth[rng.random((H, W)) < 0.01] = np.nan
    image = rng.random((H, W, 3)).astype(np.float32)
    K = np.array([[130.0, 0, W / 2 - 0.5], [0, 130.0, H / 2 - 0.5], [0, 0, 1]])
    E = np.eye(4)
    cams = warp.camera_path("right", E, 25.0, WRAP_FRAMES, float(np.nanmean(depth)))[1:]
    return image, depth, K, E, cams


# ---- the crack filling ----------------------------------------------------------------------------------------------------------------------
def segment_ids(depth, mask, num_segments):
    """The segments of oracle.crackfill.segment_depth_map as one id map (-1 = in no segment)."""
    ids = np.full(depth.shape, -1, np.int32)
    with np.errstate(invalid="ignore"):
        for i, s in enumerate(ocf.segment_depth_map(depth, mask, num_segments)):
            assert not (ids[s] >= 0).any()
            ids[s] = i
    return ids


def outlier_decisions(ids, r, min_neighbors, drop=""):
    """The outlier test of tests/stage1_cases.fill_segment for every pixel at once: a pixel of a segment is an outlier when fewer than
    min_neighbors pixels of ITS segment lie in the (2 r + 1)^2 window around it (centre included, BORDER_REFLECT_101).  drop: which pixels
    outside the pixel's own 64 x 16 tile count as "other segment": "h" those of the tiles to its left and right, "v" of the tiles above and
    below, "d" of the diagonal tiles.  Segment ids stay the global ones."""
    H, W = ids.shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pid, pty, ptx = (np.pad(a, r, mode="reflect") for a in (ids, yy // TH, xx // TW))
    ty, tx = yy // TH, xx // TW
    cnt = np.zeros((H, W), np.int32)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            q, qy, qx = (a[dy:dy + H, dx:dx + W] for a in (pid, pty, ptx))
            same = q == ids
            oy, ox = qy != ty, qx != tx
            if "h" in drop:
                same &= ~(ox & ~oy)
            if "v" in drop:
                same &= ~(oy & ~ox)
            if "d" in drop:
                same &= ~(oy & ox)
            cnt += same
    return (ids >= 0) & (cnt < min_neighbors)


def halo_flips(ids, r, min_neighbors):
    """(decisions, flips across vertical tile edges, flips across horizontal ones, flips that ONLY the diagonal tile's halo decides)."""
    full = outlier_decisions(ids, r, min_neighbors)
    fh = outlier_decisions(ids, r, min_neighbors, "h") != full
    fv = outlier_decisions(ids, r, min_neighbors, "v") != full
    fd = outlier_decisions(ids, r, min_neighbors, "d") != full
    return full, int(fh.sum()), int(fv.sum()), int((fd & ~fh & ~fv).sum())


def fill_decisions(cleaned, min_valid_neighbors, tile_local=False):
    """The pixels oracle.crackfill.fill_small_cracks fills for the mask `cleaned` (3 x 3 closing, then >= min_valid_neighbors of the 8
    neighbours).  tile_local: every 64 x 16 tile decides with `cleaned` zero outside itself."""
    c = cleaned.astype(np.uint8)

    def decide(m):
        closed = ocf.close3(m)
        return (closed > m) & (m == 0) & (ocf.filter2d(m.astype(np.float32), ocf.K8) >= min_valid_neighbors)

    if not tile_local:
        return decide(c)
    H, W = c.shape
    out = np.zeros((H, W), bool)
    for y0 in range(0, H, TH):
        for x0 in range(0, W, TW):
            m = np.zeros_like(c)
            m[y0:y0 + TH, x0:x0 + TW] = c[y0:y0 + TH, x0:x0 + TW]
            out[y0:y0 + TH, x0:x0 + TW] = decide(m)[y0:y0 + TH, x0:x0 + TW]
    return out


def closing_flips(ids, outliers):
    """How many fill decisions (min_valid_neighbors = 2, over the segments that have outliers -- the others are not closed) change when the
    closing sees nothing beyond the tile."""
    n = 0
    for s in range(int(ids.max()) + 1):
        seg = ids == s
        if not (seg & outliers).any():
            continue
        cleaned = seg & ~outliers
        n += int((fill_decisions(cleaned, 2) != fill_decisions(cleaned, 2, True)).sum())
    return n


CORNER_SHAPES = [(35, 131), (17, 65), (16, 64), (32, 128)]
MIN_NEIGHBORS = {1: 4, 2: 7, 3: 10, 4: 14}       # as tests/test_gpu_stage1.py


def _tile_corners(H, W):
    return [(y, x) for y in range(TH, H, TH) for x in range(TW, W, TW)]


def corner_views(H, W, seed):
    """Views as test_gpu_stage1._views, made for tile borders: depth layers in 5 x 7 cells (their borders do not line up with 16 or 64);
    holes along the tile edges; a 2 x 2 block of far pixels, isolated from every other far pixel, across each tile corner; and one view per
    radius r = 1..4 in which, at each corner, a far pixel keeps exactly MIN_NEIGHBORS[r] far pixels in its window only because ONE of
    them lies in the diagonal tile.  -> (image u8 [n, H, W, 3], mask u8 [n, H, W], depth f32 [n, H, W] NaN = empty)."""
    rng = np.random.default_rng(seed)
    corners = _tile_corners(H, W)

    def layered(p_hole):
        cells = rng.integers(0, 3, ((H + 4) // 5, (W + 6) // 7)).repeat(5, 0).repeat(7, 1)[:H, :W]
        d = (np.choose(cells, [1.0, 2.5, 6.0]) + 0.2 * rng.random((H, W))).astype(np.float32)
        m = (rng.random((H, W)) > p_hole).astype(np.uint8)
        for y in range(TH, H, TH):                # holes on the tile edges
            m[y - 1, 2::5] = 0
            m[y, 4::5] = 0
        for x in range(TW, W, TW):
            m[1::4, x - 1] = 0
            m[3::4, x] = 0
        return d, m

    def finish(d, m):
        i = (rng.random((H, W, 3)) * 255).astype(np.uint8)
        d = np.where(m > 0, d, np.float32(np.nan)).astype(np.float32)
        i[m == 0] = 0
        return i, m, d

    out = [finish(*layered(0.12))]
    d, m = layered(0.12)
    for y, x in corners:                          # (15,63) (15,64) (16,63) (16,64): one far pixel in each of the four tiles
        d[max(0, y - 6):y + 6, max(0, x - 6):x + 6] = 1.1
        d[y - 1:y + 1, x - 1:x + 1], m[y - 1:y + 1, x - 1:x + 1] = 20.0, 1
    if not corners:
        d[H // 2, W // 2], m[H // 2, W // 2] = 20.0, 1
    out.append(finish(d, m))
    for r in (1, 2, 3, 4):
        d, m = layered(0.12)
        d[0, 0], m[0, 0] = 20.0, 1                # the far segment exists in every view, corners or not
        for k, (y, x) in enumerate(corners):
            lower = k % 2 == 0 and y + 4 < H and x + 4 < W   # the pixel sits in the lower-right tile of the corner, else in the upper-left
            sy, sx = (-1, -1) if lower else (1, 1)
            py, px = (y, x) if lower else (y - 1, x - 1)
            own = [(py - sy * j, px - sx * i) for j in range(r + 1) for i in range(r + 1)][:MIN_NEIGHBORS[r] - 1]
            for qy, qx in own + [(py + sy, px + sx)]:
                d[qy, qx], m[qy, qx] = 20.0, 1
        out.append(finish(d, m))
    out.append(finish(*layered(0.3)))
    return [np.stack([v[j] for v in out]) for j in range(3)]


WIDE_SHAPE = (17, 15430)
FAR_RUN = slice(2000, 2060)


def wide_view(seed=31):
    """One 17 x 15430 view: 262 310 pixels (more than the 1024 x 256 threads of the linear grids) in 2 x 242 tiles (more than the 256
    tiles k_cfx_order walks per step), layered as corner_views.  The far run in the last row is, at radius 1 with min_neighbors 3, the only
    part of the farthest segment that is kept: a segment that k_cfx_order meets only beyond its first 256 tiles."""
    H, W = WIDE_SHAPE
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 3, ((H + 4) // 5, (W + 6) // 7)).repeat(5, 0).repeat(7, 1)[:H, :W]
    d = (np.choose(cells, [1.0, 2.5, 6.0]) + 0.2 * rng.random((H, W))).astype(np.float32)
    m = (rng.random((H, W)) > 0.12).astype(np.uint8)
    d[8, 5::97], m[8, 5::97] = 20.0, 1            # isolated far pixels along the whole width
    d[H - 1, FAR_RUN], m[H - 1, FAR_RUN] = 20.0, 1   # and a run of them in the last row: tiles 273..274 of 484
    i = (rng.random((H, W, 3)) * 255).astype(np.uint8)
    d = np.where(m > 0, d, np.float32(np.nan)).astype(np.float32)
    i[m == 0] = 0
    return i[None], m[None], d[None]


def sparse_view(seed=32):
    """17 x 15430 for fill_small_cracks: the right 60 % of the columns empty but for a sprinkle of pixels (step 1 closes fewer than half of
    the holes, so the depth-guided step runs, the end of the last row -- beyond pixel 262 144 -- included), the rest full with one- to
    three-pixel holes.
    -> (image u8, mask u8, original depth f32)."""
    H, W = WIDE_SHAPE
    rng = np.random.default_rng(seed)
    m = np.ones((H, W), np.uint8)
    cut = int(0.4 * W)
    m[:, cut:] = (rng.random((H, W - cut)) < 0.2).astype(np.uint8)
    for y, x in zip(rng.integers(0, H, 900), rng.integers(2, cut - 3, 900)):
        m[y, x:x + int(rng.integers(1, 4))] = 0
    i = (rng.random((H, W, 3)) * 255).astype(np.uint8)
    i[m == 0] = 0
    od = (2.0 + 0.08 * rng.standard_normal((H, W))).astype(np.float32)
    return i, m, od
