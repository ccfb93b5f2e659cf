"""The scene mesh restatement (tests/mesh_cases.py) checked on the CPU: against itself, against the topology a closed surface must have,
against analytic surfaces, and on one end-to-end scene.  What the GPU is then compared with bit for bit (tests/test_gpu_mesh.py)."""
from __future__ import annotations

import numpy as np
import pytest

import mesh_cases as Mc

ICASES = {c["name"]: c for c in Mc.integrate_cases()}
XCASES = {c["name"]: c for c in Mc.extract_cases()}


def run_integrate(c):
    return Mc.integrate(c["q"], c["w"], c["origin3"], c["voxel"], c["trunc"], c["T_cw12"], c["calib8"], c["width"], c["height"], c["step"],
                        c["meas"], c["w_max"])


def run_extract(c):
    return Mc.extract(c["q"], c["w"], c["origin3"], c["voxel"], c["min_weight"], c["max_vertices"], c["max_triangles"])


# ---------------------------------------------------------------------------------------------------- integrate
@pytest.mark.parametrize("name", list(ICASES))
def test_integrate_accounts_for_every_voxel(name):
    c = ICASES[name]
    r = run_integrate(c)
    N = c["q"].shape[0]
    info = r["info"]
    assert info[0] + info[1] + info[3] + info[4] == N ** 3 and info[5] == N and info[2] <= info[0]
    upd = r["cat"] == 0
    assert np.array_equal(r["q"][~upd], c["q"][~upd]) and np.array_equal(r["w"][~upd], c["w"][~upd])
    assert np.all(r["w"][upd] >= 1) and np.all(r["w"][upd] <= max(c["w_max"], 1))
    # the update is a weighted mean: between the old value and the measurement
    lo, hi = np.minimum(c["q"].astype(int), r["q_m"]), np.maximum(c["q"].astype(int), r["q_m"])
    assert np.all((r["q"].astype(int) >= lo)[upd]) and np.all((r["q"].astype(int) <= hi)[upd])


def test_integrate_cases_reach_what_they_are_for():
    r = run_integrate(ICASES["wall_fronto"])
    assert r["info"][0] > 0 and r["info"][1] > 0 and r["info"][2] > 0 and r["info"][3] > 0
    # the fronto-parallel wall z = 0.3: q changes sign between the voxel layers on either side of it
    c = ICASES["wall_fronto"]
    zc = c["origin3"][2] + (np.arange(16) + 0.5) * c["voxel"]
    col = r["q"][:, 8, 8].astype(int)
    seen = r["w"][:, 8, 8] > 0
    assert np.all(col[seen & (zc < 0.3 - 0.01)] > 0) and np.all(col[seen & (zc > 0.3 + 0.01)] < 0)
    r = run_integrate(ICASES["behind_and_outside"])
    c = ICASES["behind_and_outside"]
    assert r["info"][3] > 0 and r["info"][0] > 0
    r = run_integrate(ICASES["holes_and_codes"])
    assert r["info"][4] > 0 and r["info"][0] > 0
    assert set(np.unique(ICASES["holes_and_codes"]["meas"][2])) >= {0, 1, 2, 3, 4, 5, 6, 7, 255}
    assert {0, 255} <= set(np.unique(ICASES["conf_edges"]["meas"][1]))
    c = ICASES["saturate"]
    r = run_integrate(c)
    upd = r["cat"] == 0
    assert np.any(r["w"][upd] == c["w_max"]) and np.any(c["w"][upd] > c["w_max"]) and np.all(r["w"][upd] <= c["w_max"])
    c = ICASES["negative_floor"]
    r = run_integrate(c)
    S = c["w"].astype(int) + 25   # conf 200 >> 3
    num, den = 2 * r["A"] + S, 2 * S
    differs = (r["cat"] == 0) & (num < 0) & (num % den != 0)   # where a floor is not a truncation
    assert differs.sum() > 10
    assert np.array_equal(r["q"][differs].astype(int), (-((-num[differs]) // den[differs])) - 1)
    c = ICASES["second_view"]
    r = run_integrate(c)
    assert np.any((r["cat"] == 0) & (c["w"] > 0)) and np.any((r["cat"] == 0) & (c["w"] == 0))


def test_integrate_exact_edges():
    c = ICASES["exact_edges"]
    r = run_integrate(c)
    # along k: s = 1, 0.75, 0.5, 0.25, 0, -0.25, -0.5, -0.75 at trunc 0.5
    k_cat = r["cat"][:, 4, 4]
    assert list(k_cat) == [0, 0, 0, 0, 0, 0, 0, 1]
    assert list(r["free"][:, 4, 4]) == [True, True, True, False, False, False, False, False]   # t = 2, 1.5 and exactly 1
    assert list(r["q"][:, 4, 4]) == [32767, 32767, 32767, 16384, 0, -16384, -32767, 0]   # t = 1 exactly is free; s = -trunc exactly is kept


# ---------------------------------------------------------------------------------------------------- extract
@pytest.mark.parametrize("name", list(XCASES))
def test_extract_is_consistent(name):
    c = XCASES[name]
    m = run_extract(c)
    info = m["info"]
    N = c["q"].shape[0]
    assert info[5] == N and info[3] == (c["w"] >= c["min_weight"]).sum()
    if info[0] != 0:
        assert len(m["vertices"]) == 0 and len(m["triangles"]) == 0
        return
    nv, nt = int(info[1]), int(info[2])
    assert m["vertices"].shape == (nv, 3) and m["normals"].shape == (nv, 3) and m["triangles"].shape == (nt, 3)
    assert nt == 0 or (m["triangles"].min() >= 0 and m["triangles"].max() < nv)
    # every vertex lies within its own cell
    lo = c["origin3"] + (m["cells"] + 0.5) * c["voxel"]
    assert np.all(m["vertices"] >= lo - 1e-5) and np.all(m["vertices"] <= lo + c["voxel"] + 1e-5)
    # unit normals (or zero)
    ln = np.linalg.norm(m["normals"].astype(np.float64), axis=1)
    assert np.all((np.abs(ln - 1) < 1e-6) | (ln == 0))
    # no directed edge twice: the surface is orientable as emitted (a smooth surface; hashed noise has cells with several sheets)
    a, b = Mc.edge_census(m["triangles"])
    assert name.startswith("hashed") or len(np.unique((a << 32) | b)) == len(a)


def test_extract_codes_and_caps():
    assert run_extract(XCASES["empty"])["info"][0] == 1
    one = run_extract(XCASES["one_cell"])
    assert list(one["info"][:3]) == [0, 1, 0] and list(one["cells"][0]) == [1, 1, 1]
    assert run_extract(XCASES["caps_exact"])["info"][0] == 0
    for name in ("cap_vertices_over", "cap_triangles_over"):
        m = run_extract(XCASES[name])
        assert m["info"][0] == 3 and np.array_equal(m["info"][1:3], run_extract(XCASES["caps_exact"])["info"][1:3])
    # q == 0 is outside: the plane lies between k = 3 (inside) and k = 4, at f = 1024 * 1000 / 1000
    m = run_extract(XCASES["plane_through_centres"])
    c = XCASES["plane_through_centres"]
    assert m["info"][0] == 0 and np.all(m["cells"][:, 2] == 3)
    assert np.allclose(m["vertices"][:, 2], c["origin3"][2] + 4.5 * c["voxel"], atol=1e-6)
    assert np.all(m["normals"][:, 2] == 1.0)
    assert m["info"][1] == 64 and m["info"][2] == 2 * 49
    # gating: fewer valid voxels, and a mesh only where the gate passes
    g = run_extract(XCASES["min_weight"])
    assert 0 < g["info"][3] < 16 ** 3 and 0 < g["info"][1] < run_extract(XCASES["caps_exact"])["info"][1]
    h = run_extract(XCASES["half_valid"])
    assert h["info"][0] == 0 and np.all(h["cells"][:, 0] >= 8)
    assert run_extract(XCASES["touches_border"])["info"][2] > 0


@pytest.mark.parametrize("name", ["sphere_n16", "sphere_n17", "sphere_n32", "sphere_n33"])
def test_sphere_is_a_closed_oriented_manifold(name):
    c = XCASES[name]
    m = run_extract(c)
    assert m["info"][0] == 0
    V, T = m["vertices"].astype(np.float64), m["triangles"]
    assert Mc.SPHERE_R / c["voxel"] >= 4
    # a closed 2-manifold: every undirected edge in exactly two triangles, once in each direction
    a, b = Mc.edge_census(T)
    fwd = (a << 32) | b
    assert len(np.unique(fwd)) == len(fwd)
    assert np.array_equal(np.sort(fwd), np.sort((b << 32) | a))
    E = len(fwd) // 2
    used = Mc.used_vertices(T, len(V))
    assert used.all()
    assert len(V) - E + len(T) == 2
    # the geometric normals agree with X4's at every vertex of the triangle
    gn = np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]])
    for k in range(3):
        assert np.all((gn * m["normals"][T[:, k]].astype(np.float64)).sum(1) > 0)
    # and point away from the centre (the free side)
    assert np.all((gn * (V[T].mean(1) - np.asarray(Mc.SPHERE_C))).sum(1) > 0)
    # every vertex within one voxel of the sphere
    d = np.abs(np.linalg.norm(V - np.asarray(Mc.SPHERE_C), axis=1) - Mc.SPHERE_R)
    assert d.max() < c["voxel"]


def test_box_is_closed():
    m = run_extract(XCASES["box_n16"])
    a, b = Mc.edge_census(m["triangles"])
    fwd = (a << 32) | b
    assert np.array_equal(np.sort(fwd), np.sort((b << 32) | a))
    assert len(m["vertices"]) - len(fwd) // 2 + len(m["triangles"]) == 2


# ---------------------------------------------------------------------------------------------------- end to end
# Measured on this scene (wall + box, 8 exact views on an arc, N = 32, grid 64 x 48, min_weight 2; 1391 used vertices, 2592 triangles):
# the largest and the median distance of a used vertex from the true surfaces, in voxels, and the share of the visible surface that has a
# used vertex within one voxel.  The restatement is deterministic, so these are what it gives; the assertions allow twice the errors, and
# a coverage lower by half of its shortfall from 1 (0.9673)
E2E_MAX_VOXELS, E2E_MEDIAN_VOXELS, E2E_COVERAGE = 0.9293, 0.0377, 0.9782


def e2e_measure():
    run = Mc.e2e_run()
    m, voxel = run["mesh"], run["voxel"]
    V = m["vertices"].astype(np.float64)
    used = Mc.used_vertices(m["triangles"], len(V))
    d = Mc.e2e_surface_distance(V[used]) / voxel
    # coverage: samples of the true surfaces inside the volume (a margin of 2 voxels) that some view sees -- the wall in front of which
    # the box does not stand, the box's five free faces -- count as covered with a used vertex within one voxel
    g = np.linspace(-0.85, 0.85, 35)
    X, Y = np.meshgrid(g, g)
    pts = [np.stack([X.ravel(), Y.ravel(), np.full(X.size, Mc.E2E_WALL_Z)], 1)]
    lo, hi = np.asarray(Mc.E2E_BOX[0]), np.asarray(Mc.E2E_BOX[1])
    inside_xy = (pts[0][:, 0] > lo[0] - voxel) & (pts[0][:, 0] < hi[0] + voxel) & (pts[0][:, 1] > lo[1] - voxel) & (pts[0][:, 1] < hi[1] + voxel)
    pts[0] = pts[0][~inside_xy]
    s = np.linspace(0.05, 0.95, 10)
    A, B = (a.ravel() for a in np.meshgrid(s, s))
    ext = hi - lo
    pts.append(np.stack([lo[0] + A * ext[0], lo[1] + B * ext[1], np.full(A.size, lo[2])], 1))   # the face towards the cameras
    for ax, side in ((0, 0), (0, 1), (1, 0), (1, 1)):
        o = 1 - ax
        p = np.zeros((A.size, 3))
        p[:, ax] = lo[ax] if side == 0 else hi[ax]
        p[:, o] = lo[o] + A * ext[o]
        p[:, 2] = lo[2] + B * (ext[2] - 2 * voxel)
        pts.append(p)
    pts = np.concatenate(pts)
    nearest = np.sqrt(((pts[:, None, :] - V[used][None, :, :]) ** 2).sum(2)).min(1)
    return d.max(), float(np.median(d)), float((nearest <= voxel).mean()), int(used.sum()), len(m["triangles"])


def test_end_to_end_scene():
    d_max, d_med, cover, n_used, n_tri = e2e_measure()
    print(f"e2e: max {d_max:.4f} voxels, median {d_med:.4f} voxels, coverage {cover:.4f}, used vertices {n_used}, triangles {n_tri}")
    assert n_tri > 1000
    assert d_max <= 2 * E2E_MAX_VOXELS
    assert d_med <= 2 * E2E_MEDIAN_VOXELS
    assert cover >= E2E_COVERAGE - (1 - E2E_COVERAGE) / 2
