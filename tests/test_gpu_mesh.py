"""The scene mesh stages (alva_mesh_integrate, alva_mesh_extract) on the GPU against their numpy restatement tests/mesh_cases.py: the
volume, the info, the vertices and normals (as uint32) and the triangles are EQUAL, bit for bit, for every case of the two tables, and
equal again on a second run.  Both sides do the same IEEE operations in the same order and every other sum is an integer sum, so there is
no tolerance."""
from __future__ import annotations

import numpy as np
import pytest

import mesh_cases as Mc

pytestmark = pytest.mark.gpu

ICASES = {c["name"]: c for c in Mc.integrate_cases()}
XCASES = {c["name"]: c for c in Mc.extract_cases()}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_integrate(ctx, c, q=None, w=None):
    q, w = _dev(c["q"] if q is None else q), _dev(c["w"] if w is None else w)
    info = ctx.mesh_integrate(q, w, c["origin3"], c["voxel"], c["trunc"], c["T_cw12"], c["calib8"], c["width"], c["height"], c["step"],
                              tuple(_dev(m) for m in c["meas"]), c["w_max"])
    return q.cpu().numpy(), w.cpu().numpy(), info


def _gpu_extract(ctx, c):
    return ctx.mesh_extract(_dev(c["q"]), _dev(c["w"]), c["origin3"], c["voxel"], c["min_weight"], c["max_vertices"], c["max_triangles"])


def _assert_mesh(got, want):
    vertices, normals, triangles, info = got
    print("gpu info", info.tolist(), "restatement", want["info"].tolist())
    assert np.array_equal(info, want["info"])
    assert vertices.dtype == np.float32 and vertices.shape == want["vertices"].shape
    assert np.array_equal(vertices.view(np.uint32), want["vertices"].view(np.uint32))
    assert normals.dtype == np.float32 and np.array_equal(normals.view(np.uint32), want["normals"].view(np.uint32))
    assert triangles.dtype == np.int32 and np.array_equal(triangles, want["triangles"])


@pytest.mark.parametrize("name", list(ICASES))
def test_integrate_equals_the_restatement_bit_for_bit(ctx, name):
    c = ICASES[name]
    want = Mc.integrate(c["q"], c["w"], c["origin3"], c["voxel"], c["trunc"], c["T_cw12"], c["calib8"], c["width"], c["height"], c["step"],
                        c["meas"], c["w_max"])
    got = _gpu_integrate(ctx, c)
    print("gpu info", got[2].tolist(), "restatement", want["info"].tolist())
    assert np.array_equal(got[2], want["info"])
    assert got[0].dtype == np.int16 and np.array_equal(got[0], want["q"])
    assert got[1].dtype == np.uint8 and np.array_equal(got[1], want["w"])
    again = _gpu_integrate(ctx, c)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", list(XCASES))
def test_extract_equals_the_restatement_bit_for_bit(ctx, name):
    c = XCASES[name]
    want = Mc.extract(c["q"], c["w"], c["origin3"], c["voxel"], c["min_weight"], c["max_vertices"], c["max_triangles"])
    got = _gpu_extract(ctx, c)
    _assert_mesh(got, want)
    again = _gpu_extract(ctx, c)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_extract_scans_more_workgroups_than_the_scan_has_threads(ctx):
    c = Mc.scan_case()
    assert c["q"].shape[0] ** 3 > 1024 * 256
    _assert_mesh(_gpu_extract(ctx, c), Mc.extract(c["q"], c["w"], c["origin3"], c["voxel"], c["min_weight"], c["max_vertices"], c["max_triangles"]))


def test_extract_over_its_cap_writes_nothing(ctx):
    import torch
    c = XCASES["cap_vertices_over"]
    mv, mt = c["max_vertices"], c["max_triangles"]
    v = torch.full((mv, 3), 7.0, dtype=torch.float32, device="cuda")
    n = torch.full((mv, 3), 7.0, dtype=torch.float32, device="cuda")
    t = torch.full((mt, 3), -7, dtype=torch.int32, device="cuda")
    import alvaar_amd.capi as capi
    info = np.zeros(8, np.int32)
    q, w = _dev(c["q"]), _dev(c["w"])
    o = np.ascontiguousarray(c["origin3"], np.float64)
    capi.check(capi.lib.alva_mesh_extract(ctx.h, q.data_ptr(), w.data_ptr(), 16, o.ctypes.data, float(c["voxel"]), 1, mv, mt, v.data_ptr(),
                                          n.data_ptr(), t.data_ptr(), info.ctypes.data))
    assert info[0] == 3 and info[1] == mv + 1
    assert bool((v == 7.0).all()) and bool((n == 7.0).all()) and bool((t == -7).all())


def test_bad_arguments_are_refused_and_the_context_stays_usable(ctx):
    import alvaar_amd.capi as capi
    c = XCASES["one_cell"]
    with pytest.raises(capi.AlvaError):
        ctx.mesh_extract(_dev(c["q"]), _dev(c["w"]), c["origin3"], c["voxel"], 0, 16, 16)
    with pytest.raises(capi.AlvaError):
        ctx.mesh_extract(_dev(np.zeros((3, 3, 3), np.int16)), _dev(np.zeros((3, 3, 3), np.uint8)), c["origin3"], c["voxel"], 1, 16, 16)
    i = ICASES["n4"]
    with pytest.raises(capi.AlvaError):
        ctx.mesh_integrate(_dev(i["q"]), _dev(i["w"]), i["origin3"], i["voxel"], 0.0, i["T_cw12"], i["calib8"], i["width"], i["height"], i["step"],
                           tuple(_dev(m) for m in i["meas"]), 128)
    with pytest.raises(capi.AlvaError):
        ctx.mesh_integrate(_dev(i["q"]), _dev(i["w"]), i["origin3"], i["voxel"], i["trunc"], i["T_cw12"], i["calib8"], i["width"], i["height"],
                           i["step"], tuple(_dev(m) for m in i["meas"]), 256)
    _assert_mesh(_gpu_extract(ctx, c), Mc.extract(c["q"], c["w"], c["origin3"], c["voxel"], c["min_weight"], c["max_vertices"], c["max_triangles"]))


def test_three_views_integrated_and_extracted(ctx):
    """the chain: three of the end-to-end scene's views integrated on the GPU and extracted, the same with the restatement, compared at the
    end (N = 17, grid 32 x 24)"""
    N, gw, gh, step = 17, 32, 24, 4
    width, height = gw * step, gh * step
    calib = Mc.calib_for(width, height, (-0.11, 0.02, 0.0004, -0.0003))
    origin, voxel = np.array([-1.0, -1.0, -1.0]), 2.0 / N
    poses = Mc.e2e_poses()[1:7:2]
    q, w = Mc.empty_volume(N)
    dq, dw = _dev(q), _dev(w)
    for T in poses:
        meas = Mc.full_meas(Mc.render(Mc.e2e_scene(), T, calib, width, height, step))
        r = Mc.integrate(q, w, origin, voxel, 3 * voxel, T, calib, width, height, step, meas)
        q, w = r["q"], r["w"]
        info = ctx.mesh_integrate(dq, dw, origin, voxel, 3 * voxel, T, calib, width, height, step, tuple(_dev(m) for m in meas))
        assert np.array_equal(info, r["info"])
    assert np.array_equal(dq.cpu().numpy(), q) and np.array_equal(dw.cpu().numpy(), w)
    want = Mc.extract(q, w, origin, voxel, 2, 1 << 16, 1 << 17)
    assert want["info"][0] == 0 and want["info"][2] > 200
    _assert_mesh(ctx.mesh_extract(dq, dw, origin, voxel, 2, 1 << 16, 1 << 17), want)
