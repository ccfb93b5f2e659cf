"""f4b at its edges (GPU): alva_undistort_points and alva_project_dist against the oracle on the tables of camera_cases.py -- the seven
coefficient sets, the `icdist < 0` exit at iteration 0 and later, the hostile projection rows, n on both sides of the 256-thread block --
bit for bit (NaN where the oracle has NaN), and against the reference's recorded outputs."""
import numpy as np
import pytest
from pathlib import Path

import camera_cases as cc

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"


@pytest.mark.parametrize("dist", cc.DISTS, ids=cc.dist_id)
def test_undistort_matches_oracle(ctx, dist):
    import torch
    px, orc = cc.pixels(), cc.oracle_undistort(dist)
    for n in cc.SIZES + (len(px),):
        und = ctx.undistort_points(torch.from_numpy(px[:n].copy()).cuda(), cc.K, dist).cpu().numpy()
        assert und.shape == (n, 2) and np.array_equal(cc.bits(und), cc.bits(orc[:n])), n
    if dist == cc.OLD_DISTS[0]:
        same = cc.identity_rows()                                # zero coefficients: the exact identity, on the GPU too
        assert same.sum() == len(px) - 3 and np.array_equal(cc.bits(und[same]), cc.bits(px[same]))


@pytest.mark.parametrize("dist", cc.PROJ_DISTS, ids=cc.dist_id)
def test_project_matches_oracle(ctx, dist):
    import torch
    P, orc = cc.points(), cc.oracle_project(dist)
    for n in cc.SIZES + (len(P),):
        prj = ctx.project_dist(torch.from_numpy(P[:n].copy()).cuda(), cc.K, dist).cpu().numpy()
        assert prj.shape == (n, 2) and cc.same_bits(prj, orc[:n]), n
    rows = cc.special_rows()                                     # the special rows alone, one after the other: no ordinary lane beside them
    prj = ctx.project_dist(torch.from_numpy(P[rows].copy()).cuda(), cc.K, dist).cpu().numpy()
    assert cc.same_bits(prj, orc[rows])


def test_hip_matches_golden(ctx):
    import torch
    z = np.load(G / "camera_cases.npz")
    for i, dist in enumerate(z["dists"]):
        und = ctx.undistort_points(torch.from_numpy(z["px"]).cuda(), z["K"], dist).cpu().numpy()
        assert np.array_equal(cc.bits(und), cc.bits(z[f"und{i}"])), dist
    for i, dist in enumerate(z["proj_dists"]):
        prj = ctx.project_dist(torch.from_numpy(z["P"]).cuda(), z["K"], dist).cpu().numpy()
        assert cc.same_bits(prj, z[f"proj{i}"]), dist
