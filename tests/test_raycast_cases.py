"""CPU: the numpy restatement of the volume raycast (tests/raycast_cases.py, R0-R8 of include/alvaar_hip.h) against analytic truth.  The
kernel is compared with the restatement bit for bit in tests/test_gpu_mesh_raycast.py.

The bounds of the analytic tests are twice the restatement's own worst errors, measured when the test was written (the factor covers
other seeds of the same construction; it is not slack for the GPU, which has none):
    sphere at N = 32 (voxel 0.0625), 8 views, 24 x 18 rays each: a hit's distance from the sphere 0.00171 (0.027 voxel), its normal's angle
    to the analytic normal 6.48 degrees;
    wall and box at N = 32, 8 integrated views, seen from a ninth: depth against the exact render 0.0163 (0.26 voxel), median 0.0018, over
    the code-0 pixels that do not lie within one grid cell of a depth edge (10.3 % of the code-0 pixels do)."""
from __future__ import annotations

import numpy as np

import mesh_cases as Mc
import raycast_cases as Rc

MEASURED = dict(sphere_dist=0.00171, sphere_angle_deg=6.48, e2e_depth=0.0163)


def test_analytic_sphere_hits_normals_and_coverage():
    voxel = 2.0 / 32
    C = np.asarray(Mc.SPHERE_C)
    worst = dict(sphere_dist=0.0, sphere_angle_deg=0.0)
    for k in range(len(Rc.SPHERE_VIEWS)):
        res, miss = Rc.sphere_view(k)
        hit = res["code"] == 0
        assert set(np.unique(res["code"]).tolist()) <= {0, 1, 2}, k   # from outside the volume nothing is met from behind, nothing rejected
        # coverage: a condition, not a measurement
        must = miss <= Mc.SPHERE_R - 1.5 * voxel
        assert must.sum() >= 50 and hit[must].all(), (k, int((must & ~hit).sum()))
        assert not (hit & (miss > Mc.SPHERE_R + 0.5 * voxel)).any(), k   # and no hit on a ray that passes the sphere by
        p = res["point"][hit].astype(np.float64)
        r = np.linalg.norm(p - C, axis=1)
        worst["sphere_dist"] = max(worst["sphere_dist"], float(np.abs(r - Mc.SPHERE_R).max()))
        cos = (((p - C) / r[:, None]) * res["normal"][hit]).sum(1)
        worst["sphere_angle_deg"] = max(worst["sphere_angle_deg"], float(np.degrees(np.arccos(np.clip(cos, -1, 1))).max()))
        # t is the camera-space z, the point lies on the ray at t
        rays = res["rays6"][hit]
        assert np.abs(rays[:, :3] + res["t"][hit, None].astype(np.float64) * rays[:, 3:] - p).max() < 1e-6
        assert res["pose_ok"][must].all() and not res["pose_ok"][~hit].any()   # (a hit near the silhouette may be too grazing for a pose)
    print("worst", worst)
    for k, v in worst.items():
        assert v <= 2 * MEASURED[k], (k, v)


def test_wall_and_box_depth_from_a_ninth_pose():
    res, truth, T_cw = Rc.e2e_depth()
    assert not any(np.allclose(T_cw, T) for T in Mc.e2e_poses())
    gh, gw = truth.shape
    voxel = 2.0 / Mc.E2E_N
    code, depth = res["code"].reshape(gh, gw), res["t"].reshape(gh, gw)
    pad = np.pad(truth, 1, mode="edge")
    near = np.stack([pad[1 + dy:1 + dy + gh, 1 + dx:1 + dx + gw] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    edge = np.abs(near - truth[None]).max(0) > voxel             # within one grid cell of a depth edge
    seen = code == 0
    share = (edge & seen).sum() / seen.sum()
    err = np.abs(depth - truth)[seen & ~edge]
    print("code 0: %d of %d, at an edge %.1f %%, |depth - truth| max %.4f median %.4f" % (seen.sum(), seen.size, 100 * share, err.max(), np.median(err)))
    assert seen.sum() >= 1000 and share <= 0.15 and (truth[seen] > 0).all()
    assert err.max() <= 2 * MEASURED["e2e_depth"]
    assert (depth[~seen] == 0).all()


def test_table_sanity():
    """every code and every branch of R4 is reached, and every named ray gets the code it was written for"""
    names = [c["name"] for c in Rc.cases()]
    assert len(set(names)) == len(names)
    census = dict.fromkeys(("invalid", "first", "step", "hit", "behind", "exhausted", "hit_F0", "prev_F0", "normal0"), 0)
    codes = np.zeros(5, np.int64)
    pose_ok = pose_refused = fallback = first_axis = 0
    for c in Rc.cases():
        r = Rc.expected()[c["name"]]
        for k in census:
            census[k] += r["census"][k]
        codes += r["info"][1:6]
        assert r["info"][0] == len(r["code"]) and r["info"][1:6].sum() == len(r["code"]) and r["info"][6] <= 2 * r["info"][7] + 2
        if c.get("want") is not None:
            assert np.array_equal(r["code"], np.asarray(c["want"])), (c["name"], r["code"].tolist())
        miss = r["code"] != 0
        assert not r["t"][miss].any() and not r["point"][miss].any() and not r["normal"][miss].any()
        if c["kind"] == "pixels":
            pose_ok += int(r["pose_ok"].sum())
            pose_refused += int(((r["code"] == 0) & (r["pose_ok"] == 0)).sum())
            fallback += int(r["fallback"].sum())
            first_axis += int((r["pose_ok"] == 1).sum() - r["fallback"].sum())
            assert not r["pose"][r["pose_ok"] == 0].any()
            P = r["pose"][r["pose_ok"] == 1].astype(np.float64)
            if len(P):                                             # a rotation, y the normal, the translation the hit
                Rm = np.stack([P[:, 0:3], P[:, 4:7], P[:, 8:11]], 2)
                assert np.abs(Rm.transpose(0, 2, 1) @ Rm - np.eye(3)).max() < 1e-5 and np.abs(np.linalg.det(Rm) - 1).max() < 1e-5
                assert np.array_equal(P[:, 12:15], r["point"][r["pose_ok"] == 1].astype(np.float64))
    print(census, codes.tolist(), pose_ok, pose_refused, fallback)
    assert all(v > 0 for v in census.values()), census
    assert (codes > 0).all(), codes
    assert pose_ok > 0 and fallback > 0 and first_axis > 0
    by = Rc.expected()
    assert by["zero_gradient_pose"]["census"]["normal0"] == 1 and by["zero_gradient_pose"]["pose_ok"].sum() == 0
    g = by["grazing"]
    assert ((g["code"] == 0) & (g["pose_ok"] == 0)).sum() > 0 and g["pose_ok"].sum() > 0          # both sides of R7's gate
    assert by["fresh_volume_long_diagonal"]["info"][6] == 63 and by["F_zero_current"]["census"]["hit_F0"] == 1
    assert by["F_zero_prev"]["census"]["prev_F0"] == 1 and by["taps"]["info"][5] == 2
    # the sample count never reaches the loop's bound for finite input
    assert max(int(r["info"][6]) - (2 * int(r["info"][7]) - 1) for r in by.values()) <= 0


def test_grid_list_and_world_rays_agree():
    """in the restatement too: the grid is the list of its pixels, and the pixels' rays are world rays"""
    c = next(c for c in Rc.cases() if c["name"] == "grid_10x7")
    vol = (c["q"], c["w"], c["origin3"], c["voxel"], c["min_weight"])
    grid = Rc.expected()["grid_10x7"]
    lst = Rc.raycast_pixels(*vol, c["T_wc12"], c["calib8"], c["width"], c["height"], c["step"], Rc.grid_pixels(c["width"], c["height"], c["step"]))
    world = Rc.raycast(*vol, grid["rays6"])
    for k in ("t", "point", "normal", "code", "info"):
        assert np.array_equal(grid[k], lst[k]) and np.array_equal(grid[k], world[k]), k
    assert np.array_equal(grid["pose"], lst["pose"])
