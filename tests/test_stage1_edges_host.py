"""CPU: the inputs of the stage-1 edge cases (tests/stage1_edges.py) meet, on the reference's restatements alone, the conditions the GPU
tests of tests/test_gpu_warp.py and tests/test_gpu_stage1.py rely on -- tie counts, margins from a half-integer, clipped-band counts, sign
mixes, the number of outlier / fill decisions a missing tile halo would flip, and the sizes that make the capped grids wrap."""
import os

import numpy as np
import pytest

from oracle import crackfill as ocf
from oracle import warp as owarp
from tests import stage1_cases as sc
from tests import stage1_edges as se

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "g16_warp.npz"))


def _cands(case):
    image, depth, K, E, cams = case
    w = se.splat_world(depth, K, E)
    return [se.splat_candidates(depth, K, E, c, w) for c in cams]


# ---- the candidate sets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["right", "forward"])
def test_candidate_sets_hold_the_recorded_reference_and_the_oracle(name):
    """The helper restates the oracle (same hits, same nearest z), the recorded reference's colours are members of its sets everywhere, and
    no g16 target is left out: the closest approach of a source to a half-integer is 3.5e-7, far from the 1e-9 band."""
    cams = list(G[f"{name}_cams"])[1:]
    wi, wm, wd = owarp.splat(G["image"], G["depth"], G["K"], G["E"], cams)
    ties = 0
    for i, cd in enumerate(_cands((G["image"], G["depth"], G["K"], G["E"], cams))):
        assert np.array_equal(cd["hit"], wm[i].ravel() > 0)
        assert np.array_equal(cd["zmin"].astype(np.float32)[cd["hit"]], wd[i].ravel()[cd["hit"]])
        for got in (wi[i], G[f"{name}_imgs"][1 + i]):
            hit, excluded, tied = se.check_colours(got, G["image"], cd, (name, i))
            assert excluded == 0 and cd["margin"] > 1e-7
        ties += tied
    assert ties == (76 if name == "right" else 0)


def test_candidate_check_refuses_a_torn_or_foreign_colour():
    image, depth, K, E, cams = se.tie_case()
    cd = _cands((image, depth, K, E, cams))[0]
    good = se.lowest_colours(image, cd).reshape(40, 56, 3)
    se.check_colours(good, image, cd)
    t = int(np.nonzero(cd["ncand"] == 4)[0][0])
    a, b = cd["cand_src"][cd["cand_t"] == t][:2]
    torn = good.copy().reshape(-1, 3)
    ca, cb = (image.reshape(-1, 3)[[a, b]] * 255).astype(np.uint8)
    assert (ca != cb).all()
    torn[t] = (ca[0], cb[1], ca[2])                      # two bytes of one tied source, one of the other
    with pytest.raises(AssertionError):
        se.check_colours(torn.reshape(40, 56, 3), image, cd)
    foreign = good.copy().reshape(-1, 3)
    last = image.shape[0] * image.shape[1] - 1
    foreign[t] = (image.reshape(-1, 3)[last] * 255).astype(np.uint8)   # the last source does not land on t
    assert last not in cd["cand_src"][cd["cand_t"] == t]
    with pytest.raises(AssertionError):
        se.check_colours(foreign.reshape(40, 56, 3), image, cd)


def test_sources_on_a_half_integer_make_their_targets_unstable():
    """u = x + 0.5 exactly: every source may round either way, so every target it can reach is left out -- and only by this rule."""
    H, W = 6, 8
    K = np.eye(3)
    depth = np.ones((H, W), np.float32)
    cam = np.eye(4)
    cam[0, 3] = 0.5
    cd = se.splat_candidates(depth, K, np.eye(4), cam)
    assert cd["margin"] == 0.0 and cd["hit"].any() and cd["unstable"][cd["hit"]].all()
    cam[0, 3] = 0.25
    cd = se.splat_candidates(depth, K, np.eye(4), cam)
    assert cd["margin"] == 0.25 and not cd["unstable"].any()


# ---- the splat scenes -----------------------------------------------------------------------------------------------------------------------
def test_tie_case_is_all_exact_ties():
    want = {2.0: (560, 4, 0.15), 3.0: (368, 9, 0.06)}
    for tz, cd in zip(se.TIE_TZ, _cands(se.tie_case())):
        multi = cd["nland"] > 1
        hits, most, margin = want[tz]
        assert int(cd["hit"].sum()) == hits == int(multi.sum()) == int((cd["ncand"] > 1).sum()) >= 300
        assert np.array_equal(cd["ncand"][multi], cd["nland"][multi])          # every multi-hit target is an exact tie
        assert int(cd["ncand"].max()) == most and abs(cd["margin"] - margin) < 1e-6 and cd["margin"] >= 1e-3
        assert not cd["unstable"].any()


def test_behind_and_mixed_sign_cases():
    cd = _cands(se.behind_case())[0]
    assert int(cd["hit"].sum()) == 560 and (cd["src_z"] < 0).all() and cd["band_u"] >= 20 and cd["margin"] >= 1e-3
    for invalid in (False, True):
        cd = _cands(se.mixed_sign_case(invalid))[0]
        both = cd["has_pos"] & cd["has_neg"]
        assert int(both.sum()) >= 20 and (cd["zmin"][both] < 0).all()          # the source BEHIND the camera wins
        assert cd["margin"] > 1e-7 and not cd["unstable"].any()
    image, depth, K, E, cams = se.mixed_sign_case(True)
    with np.errstate(invalid="ignore"):
        kinds = [depth == 0, depth < 0, np.isnan(depth), depth == np.inf, depth == -np.inf]
    assert all(int(k.sum()) >= 2 for k in kinds)
    bad = np.nonzero(np.any(kinds, axis=0).ravel())[0]
    assert not np.isin(bad, cd["src"]).any()                                   # none of them lands, the +inf ones included


def test_band_case_reaches_both_clipped_bands():
    cds = _cands(se.band_case())
    assert max(cd["band_u"] for cd in cds) >= 10 and max(cd["band_v"] for cd in cds) >= 10
    assert _cands(se.mixed_sign_case(True))[0]["band_u"] >= 1 and _cands(se.mixed_sign_case(True))[0]["band_v"] >= 1
    assert all(cd["margin"] > 1e-7 and not cd["unstable"].any() for cd in cds)


def test_wrap_case_exceeds_the_capped_grid_and_stays_inside_the_exclusion_cap():
    image, depth, K, E, cams = se.wrap_case()
    assert len(cams) == se.WRAP_FRAMES - 1 and len(cams) * depth.size > se.SPLAT_GRID
    assert (len(cams) - 1) * depth.size < se.SPLAT_GRID < len(cams) * depth.size      # the LAST camera lies beyond the wrap
    wi, wm, wd = owarp.splat(image, depth, K, E, cams)
    worst = 0.0
    for i, cd in enumerate(_cands((image, depth, K, E, cams))):
        hit, excluded, tied = se.check_colours(wi[i], image, cd, i)
        assert hit > 0.5 * depth.size
        worst = max(worst, excluded / hit)
    assert worst <= 1e-3


# ---- the crack filling ----------------------------------------------------------------------------------------------------------------------
def test_untouched_variants_are_the_restatement():
    img, mask, depth = se.corner_views(35, 131, 7 * 35 + 131)
    for r in (1, 3):
        for f in (0, 1, 4):
            ids = se.segment_ids(depth[f], mask[f], 8)
            full = se.outlier_decisions(ids, r, se.MIN_NEIGHBORS[r])
            for s in range(int(ids.max()) + 1):
                seg = ids == s
                cnt = ocf.filter2d(seg.astype(np.float32), np.ones((2 * r + 1, 2 * r + 1), dtype=np.float32))
                assert np.array_equal(full & seg, seg & (cnt < se.MIN_NEIGHBORS[r]))
                cleaned = (seg & ~full).astype(np.uint8)
                fm = ocf.fill_small_cracks(np.zeros((35, 131, 3), np.float32), cleaned, 2)[1]
                assert np.array_equal(se.fill_decisions(cleaned, 2), (fm > 0) & (cleaned == 0))


@pytest.mark.parametrize("H,W", se.CORNER_SHAPES)
def test_corner_views_can_see_a_missing_halo(H, W):
    """For every radius and segment count the GPU test uses: how many outlier decisions flip when the halo beyond a vertical tile edge, a
    horizontal one, or ONLY the diagonal tile's is dropped, and how many fill decisions when the closing is blind beyond the tile.
    Measured at 35 x 131: vertical 105..233, horizontal 436..964, diagonal-only 4 / 16 / 34 / 46..50 for r = 1 / 2 / 3 / 4, closing
    171..558.  16 x 64 is ONE tile: nothing can flip, it is the case of a halo that lies wholly outside the image."""
    img, mask, depth = se.corner_views(H, W, 7 * H + W)
    assert img.shape[0] == 7 and int((~np.isnan(depth[0])).sum()) > 100
    tiles = ((H + se.TH - 1) // se.TH) * ((W + se.TW - 1) // se.TW)
    for nseg in (5, 8, 16):
        for r in (1, 2, 3, 4):
            fh = fv = fd = fc = 0
            for f in range(img.shape[0]):
                ids = se.segment_ids(depth[f], mask[f], nseg)
                full, a, b, c = se.halo_flips(ids, r, se.MIN_NEIGHBORS[r])
                fh, fv, fd = fh + a, fv + b, fd + c
                fc += se.closing_flips(ids, full)
            print(f"{H}x{W} nseg {nseg} r {r}: flips vertical {fh} horizontal {fv} diagonal-only {fd} closing {fc}")
            if tiles == 1:
                assert fh == fv == fd == fc == 0
            else:
                assert fh >= 8 and fv >= 8 and fc >= 4
                assert fd >= (4 if (H, W) == (35, 131) else 1)     # 3 x 3 tiles have four inner corners, the other shapes one


def test_wide_and_sparse_views_wrap_every_capped_grid():
    H, W = se.WIDE_SHAPE
    tiles = ((H + se.TH - 1) // se.TH) * ((W + se.TW - 1) // se.TW)
    assert H * W > se.LINEAR_GRID and tiles == 484 > 256 and H * W > 120 * 256
    img, mask, depth = se.wide_view()
    p = dict(min_neighbors=10, neighbor_radius=3, min_valid_neighbors=2, max_crack_size=6, depth_threshold=0.1)
    wi, wm, wd = sc.warp_frame_fill(img[0], mask[0], depth[0], p, 8)
    filled, dropped = (wm > 0) & (mask[0] == 0), (wm == 0) & (mask[0] > 0)
    assert filled.ravel()[se.LINEAR_GRID:].sum() >= 4 and dropped.sum() >= 100 and filled.sum() > 10000
    far = depth[0] == 20.0
    assert far.sum() > 100 and not (wd[far] == 20.0).any()                     # isolated far pixels: all outliers, along the whole width
    wd1 = sc.warp_frame_fill(img[0], mask[0], depth[0], dict(p, min_neighbors=3, neighbor_radius=1), 8)[2]
    kept = np.nonzero(wd1 == 20.0)                                             # at radius 1 / min_neighbors 3 the far run of the last row stays:
    assert len(kept[0]) >= 10 and (kept[0] == H - 1).all() and kept[1].min() >= 64 * (256 - 242)       # a segment only beyond tile 256
    simg, smask, sod = se.sparse_view()
    f = simg.astype(np.float32) / 255.0
    s1 = ocf.fill_small_cracks(f, smask, 2)[1]
    wm2 = ocf.fill_small_cracks_depth_guided(f, smask, sod, True, 0.1, 6, 2)[1]
    holes, step1, both = int((smask == 0).sum()), int(((s1 > 0) & (smask == 0)).sum()), int(((wm2 > 0) & (smask == 0)).sum())
    assert step1 < 0.45 * holes and both - step1 > 500                         # the depth-guided step runs and fills
    assert ((wm2 > 0) & (smask == 0)).ravel()[se.LINEAR_GRID:].sum() >= 8
