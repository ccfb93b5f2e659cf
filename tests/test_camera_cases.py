"""f4b at its edges (CPU): the tables of camera_cases.py reach the undistortion loop's `icdist < 0` exit at iteration 0 and later, and the
projection's divisions by zero, overflows and NaN; the case module's restatement of the loop is the oracle bit for bit; the oracle is the
compiled reference (where built) and the reference's recorded outputs (tests/golden/camera_cases.npz) bit for bit."""
import numpy as np
import pytest
from pathlib import Path

import camera_cases as cc
from oracles import orc_undistort_points, ref_undistort_points, orc_project_dist, ref_project_dist

G = Path(__file__).resolve().parent / "golden"


@pytest.mark.parametrize("dist", cc.DISTS, ids=cc.dist_id)
def test_exit_shares_and_restatement(dist):
    px, orc = cc.pixels(), cc.oracle_undistort(dist)
    out, exit_at = cc.restate_undistort(px, cc.K, dist)
    assert np.array_equal(cc.bits(out), cc.bits(orc))
    share, finite = (exit_at >= 0).mean(), np.isfinite(orc).all(1).mean()
    print(cc.dist_id(dist), "exit share", round(float(share), 3), "at iteration 0 / later:", int((exit_at == 0).sum()), int((exit_at >= 1).sum()),
          "finite share", float(finite))
    assert finite == 1.0
    if dist in cc.OLD_DISTS:
        assert share == 0
        return
    assert share >= 0.25
    ring = exit_at[:cc.N_RING]
    assert (ring == 0).sum() >= cc.RING_DIRS and (ring >= 1).sum() >= cc.RING_DIRS and (ring == -1).sum() >= cc.RING_DIRS   # all three kinds, on the rings
    first, later = np.flatnonzero(exit_at == 0), np.flatnonzero(exit_at >= 1)
    # the exit hands back the pixel itself (to the rounding of the trip through the normalised plane) whenever it is taken
    for rows in (first, later):
        assert np.abs(orc[rows] - px[rows]).max() < 1e-3
    # ... so a neighbour that stays in the loop lands elsewhere: the exit decides the result
    stay = np.flatnonzero(exit_at == -1)
    assert np.abs(orc[stay] - px[stay]).max() > 1.0


def test_zero_distortion_is_the_identity_on_the_table():
    """(u - c) / f * f + c in double comes back within a few ulps of c (1e-13 here), which the rounding to float hides for every
    coordinate whose float spacing is wider than that: cc.identity_rows().  A coordinate of exactly 0 is not among them: row 0 of the
    image comes back as 2.8e-14 from the oracle and from the reference alike (the same bits, test_oracle_matches_reference)."""
    px, out = cc.pixels(), cc.oracle_undistort(cc.OLD_DISTS[0])
    same = cc.identity_rows()
    assert np.array_equal(cc.bits(out[same]), cc.bits(px[same])) and (~same).sum() == 3 and (px[~same] == 0).any(1).all()
    assert np.abs(out[~same] - px[~same]).max() < 1e-12 and not np.array_equal(cc.bits(out[~same]), cc.bits(px[~same]))


@pytest.mark.parametrize("dist", cc.PROJ_DISTS, ids=cc.dist_id)
def test_projection_rows(dist):
    P, out = cc.points(), cc.oracle_project(dist)
    rows = dict(zip([k for k, _ in cc.SPECIAL_POINTS], cc.special_rows()))
    assert all(np.array_equal(P[r], np.array(p), equal_nan=True) for r, (_, p) in zip(cc.special_rows(), cc.SPECIAL_POINTS))
    ordinary = np.ones(len(P), bool)
    ordinary[cc.special_rows()] = False
    assert np.isfinite(out[ordinary]).all() and len(P) == 2000
    nan_rows = ("Z=0", "Z=0,X=0", "Z=-0", "Z=1e-300", "X=1e300", "Y=-1e300", "X=1e39", "X=NaN", "Y=NaN", "Z=NaN", "X=inf", "X=inf,Z=inf", "origin")
    for k in nan_rows:                                           # inf * 0 in the distortion polynomial, or NaN carried through
        assert np.isnan(out[rows[k]]).any(), k
    for k in ("Z=-2", "Z=-2,X<0", "Z=1e-300,X=0", "X=1e-40", "Z=+inf", "Z=-inf", "axis"):
        assert np.isfinite(out[rows[k]]).all(), k
    assert np.array_equal(out[rows["Z=+inf"]], np.float32(cc.K[2:])) and np.array_equal(out[rows["axis"]], np.float32(cc.K[2:]))
    assert np.isinf(out[rows["X=1e10"]]).any()                   # finite doubles beyond the float range: the final cast overflows
    # Z < 0 projects as if in front, mirrored through the principal point when the distortion is odd in (x, y)
    assert np.isnan(out).any(1).sum() >= len(nan_rows) and np.isnan(out[ordinary]).sum() == 0


@pytest.mark.ref
@pytest.mark.parametrize("dist", cc.DISTS, ids=cc.dist_id)
def test_oracle_matches_reference(dist):
    assert np.array_equal(cc.bits(cc.oracle_undistort(dist)), cc.bits(ref_undistort_points(cc.pixels(), cc.K, dist)))
    if dist in cc.PROJ_DISTS:
        assert cc.same_bits(cc.oracle_project(dist), ref_project_dist(cc.points(), cc.K, dist))


def test_oracle_matches_golden():
    z = np.load(G / "camera_cases.npz")
    assert np.array_equal(cc.bits(z["px"]), cc.bits(cc.pixels()[cc.GOLDEN_PIXELS])) and np.array_equal(z["P"], cc.points()[cc.GOLDEN_POINTS], equal_nan=True)
    assert set(cc.special_rows()) <= set(range(len(cc.points()))[cc.GOLDEN_POINTS])
    assert np.array_equal(z["K"], cc.K) and np.array_equal(z["dists"], cc.DISTS) and np.array_equal(z["proj_dists"], cc.PROJ_DISTS)
    for i, dist in enumerate(cc.DISTS):
        assert np.array_equal(cc.bits(orc_undistort_points(z["px"], cc.K, dist)), cc.bits(z[f"und{i}"])), dist
    for i, dist in enumerate(cc.PROJ_DISTS):
        assert cc.same_bits(orc_project_dist(z["P"], cc.K, dist), z[f"proj{i}"]), dist
