"""CPU: what makes the arbitrary-points cases of tests/pointrender_cases.py worth running, asserted on oracle/pointrender.py -- coverage that
the opening changes, covered pixels on all four borders, and pixels whose two nearest points are exact copies of each other (so that the
z-buffer's tie rule, the smaller index, decides the colour)."""
import numpy as np
import pytest

from oracle import pointrender as opr
from tests import pointrender_cases as pc


def owners(c, live, radius=0.05):
    """-> int64 [H, W]: the index in c["pts"] of the point the oracle lets own each pixel among the `live` points, -1 = none."""
    ids = np.nonzero(live)[0]
    with np.errstate(all="ignore"):
        x, y, z = opr.to_ndc(c["pts"][ids], *opr.cameras_from_opencv(c["cam"], c["K"], c["size"]))
        idx = opr.rasterize_nearest(x, y, z, c["size"], radius)
    return np.where(idx >= 0, ids[np.maximum(idx, 0)], -1)


def tie_pixels(c, own, live):
    """-> (bool [H, W]: owned by a point of [0, n // 8) whose exact copy at + n // 2 is live too, the number of pixels the copy owns)."""
    n = c["pts"].shape[0]
    low = (own >= 0) & (own < n // 8)
    low[low] = live[own[low] + n // 2]
    high = (own >= n // 2) & (own < n // 2 + n // 8)
    high[high] = live[own[high] - n // 2]
    return low, int(high.sum())


@pytest.mark.parametrize("H,W", pc.POINT_SHAPES)
def test_point_cases_cover_borders_and_ties(H, W):
    c = pc.points(H, W)
    n = c["pts"].shape[0]
    assert n == pc.N_POINTS and np.array_equal(c["pts"][n // 2:n // 2 + n // 8], c["pts"][:n // 8])
    live = c["drop"] == 0
    own = owners(c, live)
    raw = (own >= 0).astype(np.uint8)
    opened = opr.morph_open5(raw)
    borders = [int(raw[0].sum()), int(raw[-1].sum()), int(raw[:, 0].sum()), int(raw[:, -1].sum())]
    low, high = tie_pixels(c, own, live)
    print(f"{(H, W)}: raw {raw.mean():.2f} opened {opened.mean():.2f} borders {borders} ties low {int(low.sum())} high {high}")
    assert raw.mean() >= 0.8
    assert 0.4 <= opened.mean() <= 0.8
    assert min(borders) >= 20
    assert low.sum() >= 100 and high == 0


def test_big_case_is_covered_by_its_last_points():
    c = pc.big_points()
    assert c["pts"].shape == (pc.BIG_N, 3) and c["feats"].shape == (pc.BIG_N, 1) and pc.BIG_N > 2048 * 256
    assert (c["pts"][:pc.BIG_DEAD, 2] == -1).all()
    live = c["drop"] == 0
    own = owners(c, live)
    assert (own[own >= 0] >= pc.BIG_DEAD).all()
    assert (own >= 0).mean() > 0.5
