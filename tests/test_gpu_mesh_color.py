"""The mesh colour stages (alva_color_thumb, alva_mesh_integrate_color, alva_mesh_color_at) on the GPU against their numpy restatement
tests/mesh_color_cases.py: the thumbnail, the three volumes, the info, the colours and the codes are EQUAL, bit for bit, and equal again
on a second run.  Both sides do the same IEEE operations in the same order and every other sum is an integer sum, so there is no
tolerance.  The coloured integration leaves in q, w and info[0..5] exactly what alva_mesh_integrate leaves on a copy of the volume."""
from __future__ import annotations

import numpy as np
import pytest

import mesh_cases as Mc
import mesh_color_cases as Cc

pytestmark = pytest.mark.gpu

TCASES = {c["name"]: c for c in Cc.thumb_cases()}
CCASES = {c["name"]: c for c in Cc.integrate_color_cases()}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------- thumbnail
@pytest.mark.parametrize("name", list(TCASES))
def test_thumb_equals_the_restatement_bit_for_bit(ctx, name):
    t = TCASES[name]
    img, cstep = t["img"], t["cstep"]
    # the buffer goes to the device as it is: the image is a view into it, with the buffer's pitch and its own offset
    d_img = _dev(t["buf"])[t["r0"]:t["r0"] + t["h"], t["c0"]:t["c0"] + t["w"]]
    assert d_img.stride(0) == t["buf"].shape[1] * 4 and np.array_equal(d_img.cpu().numpy(), img)
    want = Cc.thumb(img, cstep)
    got = ctx.color_thumb(d_img, cstep).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(ctx.color_thumb(d_img, cstep).cpu().numpy(), got)


def test_thumb_reads_nothing_past_its_blocks_and_not_the_alpha(ctx):
    img, cstep = TCASES["cstep4_odd"]["img"], 4
    h, w = img.shape[:2]
    edit = img.copy()
    edit[h // cstep * cstep:] ^= 255
    edit[:, w // cstep * cstep:] ^= 255
    edit[..., 3] ^= 255
    assert np.array_equal(ctx.color_thumb(_dev(edit), cstep).cpu().numpy(), Cc.thumb(img, cstep))


# ---------------------------------------------------------------------------------------------------- integrate
def _gpu_integrate_color(ctx, c):
    q, w, col = _dev(c["q"]), _dev(c["w"]), _dev(c["c"])
    info = ctx.mesh_integrate_color(q, w, col, c["origin3"], c["voxel"], c["trunc"], c["T_cw12"], c["calib8"], c["width"], c["height"],
                                    c["step"], tuple(_dev(m) for m in c["meas"]), _dev(c["thumb"]), c["cstep"], c["w_max"])
    return q.cpu().numpy(), w.cpu().numpy(), col.cpu().numpy(), info


def _gpu_integrate(ctx, c):
    q, w = _dev(c["q"]), _dev(c["w"])
    info = ctx.mesh_integrate(q, w, c["origin3"], c["voxel"], c["trunc"], c["T_cw12"], c["calib8"], c["width"], c["height"], c["step"],
                              tuple(_dev(m) for m in c["meas"]), c["w_max"])
    return q.cpu().numpy(), w.cpu().numpy(), info


def _check_integrate_color(ctx, c):
    want = Cc.run_integrate_color(c)
    got = _gpu_integrate_color(ctx, c)
    print("gpu info", got[3].tolist(), "restatement", want["info"].tolist())
    assert np.array_equal(got[3], want["info"])
    assert got[0].dtype == np.int16 and np.array_equal(got[0], want["q"])
    assert got[1].dtype == np.uint8 and np.array_equal(got[1], want["w"])
    assert got[2].dtype == np.uint8 and got[2].shape == want["c"].shape and np.array_equal(got[2], want["c"])
    # the distance stage on a copy of the same volume
    plain = _gpu_integrate(ctx, c)
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1])
    assert np.array_equal(plain[2][:6], got[3][:6]) and plain[2][6] == 0 and plain[2][7] == 0 and got[3][7] == 0
    return got


@pytest.mark.parametrize("name", list(CCASES))
def test_integrate_color_equals_the_restatement_bit_for_bit(ctx, name):
    c = CCASES[name]
    got = _check_integrate_color(ctx, c)
    again = _gpu_integrate_color(ctx, c)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)


def test_integrate_color_strides_over_a_volume_larger_than_its_grid(ctx):
    c = Cc.stride_case()
    assert c["q"].shape[0] ** 3 > 2048 * 256 and (c["q"].shape[0] - 1) ** 3 <= 2048 * 256
    got = _check_integrate_color(ctx, c)
    assert got[3][6] > 10000


def test_two_views_fused_one_after_the_other(ctx):
    """the chain on the device: two of the painted scene's views, thumbnail and integration, against the restatement's chain"""
    N, step = 17, 4
    width, height = 32 * step, 24 * step
    calib = Mc.calib_for(width, height, (-0.11, 0.02, 0.0004, -0.0003))
    origin, voxel = np.array([-1.0, -1.0, -1.0]), 2.0 / N
    q, w = Mc.empty_volume(N)
    c = np.zeros((N, N, N, 4), np.uint8)
    dq, dw, dc = _dev(q), _dev(w), _dev(c)
    for T in Mc.e2e_poses()[2:6:3]:
        rgba, _ = Cc.render_color(T, calib, width, height)
        meas = Mc.full_meas(Mc.render(Cc.paint_scene(), T, calib, width, height, step))
        r = Cc.integrate_color(q, w, c, origin, voxel, 3 * voxel, T, calib, width, height, step, meas, Cc.thumb(rgba, 4), 4)
        q, w, c = r["q"], r["w"], r["c"]
        th = ctx.color_thumb(_dev(rgba), 4)
        info = ctx.mesh_integrate_color(dq, dw, dc, origin, voxel, 3 * voxel, T, calib, width, height, step, tuple(_dev(m) for m in meas), th, 4)
        assert np.array_equal(info, r["info"])
    assert np.array_equal(dq.cpu().numpy(), q) and np.array_equal(dw.cpu().numpy(), w) and np.array_equal(dc.cpu().numpy(), c)
    assert (c[..., 3] > 0).sum() > 300


# ---------------------------------------------------------------------------------------------------- colour at
def _check_color_at(ctx, c, origin, voxel, pts):
    want = Cc.color_at(c, origin, voxel, pts)
    rgba, codes, info = ctx.mesh_color_at(_dev(c), origin, voxel, _dev(pts))
    print("gpu info", info.tolist(), "restatement", want["info"].tolist())
    assert np.array_equal(info, want["info"])
    assert codes.dtype == np.uint8 and np.array_equal(codes, want["code"])
    assert rgba.dtype == np.uint8 and rgba.shape == want["rgba"].shape and np.array_equal(rgba, want["rgba"])
    return want


def test_color_at_equals_the_restatement_bit_for_bit(ctx):
    want = _check_color_at(ctx, Cc.color_at_volume(), Cc.CA_ORIGIN, Cc.CA_VOXEL, Cc.color_at_points())
    assert set(np.unique(want["code"]).tolist()) == {0, 1, 2, 4}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_color_at_any_number_of_points(ctx, n):
    pts = Cc.color_at_points()
    pick = Mc.hashed(n, 17 + n) % len(pts)
    _check_color_at(ctx, Cc.color_at_volume(), Cc.CA_ORIGIN, Cc.CA_VOXEL, pts[pick])


def test_color_at_ends_to_one_double(ctx):
    c = np.full((8, 8, 8, 4), 9, np.uint8)
    e = Cc.end_points()
    assert np.all(_check_color_at(ctx, c, Cc.CA_ORIGIN, Cc.CA_VOXEL, e)["code"] == 0)
    for o in Cc.nudged_origins():
        k = _check_color_at(ctx, c, o, Cc.CA_VOXEL, e)["code"]
        assert 0 < (k == 1).sum() < len(e)


def test_color_at_a_hashed_volume_with_hashed_points(ctx):
    """N = 33, a non-dyadic voxel, 4096 points of which some lie outside"""
    N, origin, voxel = 33, np.array([0.3, -1.7, 2.1]), 0.061
    c = Cc.hashed_color_volume(N, 23, empty_share=3)
    h = Mc.hashed(3 * 4096, 29).reshape(-1, 3)
    pts = (origin + (h % 100003) / 100003.0 * (N + 1.0) * voxel - 0.5 * voxel).astype(np.float32)
    want = _check_color_at(ctx, c, origin, voxel, pts)
    assert want["info"][1] > 2000 and want["info"][2] > 100 and want["info"][3] > 0


def test_bad_arguments_are_refused_and_the_context_stays_usable(ctx):
    import alvaar_amd.capi as capi
    img = TCASES["cstep4_odd"]["img"]
    with pytest.raises(capi.AlvaError):
        ctx.color_thumb(_dev(img), 17)
    with pytest.raises(capi.AlvaError):
        ctx.color_thumb(_dev(img), 0)
    with pytest.raises(capi.AlvaError):
        ctx.color_thumb(_dev(img[:3]), 4)   # no whole block
    c = CCASES["n4_distortion"]
    with pytest.raises(capi.AlvaError):
        ctx.mesh_integrate_color(_dev(c["q"]), _dev(c["w"]), _dev(c["c"]), c["origin3"], c["voxel"], c["trunc"], c["T_cw12"], c["calib8"],
                                 c["width"], c["height"], c["step"], tuple(_dev(m) for m in c["meas"]), _dev(c["thumb"]), 0, c["w_max"])
    with pytest.raises(capi.AlvaError):
        ctx.mesh_color_at(_dev(np.zeros((3, 3, 3, 4), np.uint8)), Cc.CA_ORIGIN, Cc.CA_VOXEL, _dev(Cc.end_points()))
    with pytest.raises(capi.AlvaError):
        ctx.mesh_color_at(_dev(Cc.color_at_volume()), Cc.CA_ORIGIN, 0.0, _dev(Cc.end_points()))
    _check_integrate_color(ctx, c)
