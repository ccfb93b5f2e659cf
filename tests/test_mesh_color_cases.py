"""The mesh colour restatement tests/mesh_color_cases.py checked on the CPU: the thumbnail's rounding, the coloured integration against
tests/mesh_cases.py and its own invariants, the sampler's codes, and the painted wall-and-box scene end to end against its analytic
colours."""
from __future__ import annotations

import numpy as np
import pytest

import mesh_cases as Mc
import mesh_color_cases as Cc


# ---------------------------------------------------------------------------------------------------- thumbnail
@pytest.mark.parametrize("cstep", [1, 3, 4, 16])
def test_thumb_of_a_constant_image_is_that_constant(cstep):
    for v in (0, 1, 127, 254, 255):
        img = np.full((2 * cstep + 1, 3 * cstep + 2, 4), v, np.uint8)
        img[..., 3] = 7   # the alpha is not read
        t = Cc.thumb(img, cstep)
        assert t.shape == ((2 * cstep + 1) // cstep, (3 * cstep + 2) // cstep, 4)
        assert np.all(t[..., :3] == v) and np.all(t[..., 3] == 255)


def test_thumb_rounds_halves_up_exactly():
    """k pixels of 255 in a block of 16: 255 k / 16 = 15.9375 k; at cstep 2, k of 4: 63.75, 127.5 -- a true half -- and 191.25"""
    img = np.zeros((2, 8, 4), np.uint8)
    for k in range(4):
        blk = np.zeros(4, np.uint8)
        blk[:k + 1] = 255
        img[:, 2 * k:2 * k + 2, 0] = blk.reshape(2, 2)
    assert Cc.thumb(img, 2)[0, :, 0].tolist() == [64, 128, 191, 255]   # 63.75 -> 64, 127.5 -> 128 (half up), 191.25 -> 191
    # a half from 1s: two of four pixels 1 -> 0.5 -> 1; one of four -> 0.25 -> 0
    img = np.zeros((2, 4, 4), np.uint8)
    img[0, 0:2, 1] = 1
    img[0, 2, 1] = 1
    assert Cc.thumb(img, 2)[0, :, 1].tolist() == [1, 0]
    # cstep 4: 8 of 16 pixels 255 -> 127.5 -> 128; 8 of 16 pixels 1 -> 0.5 -> 1
    img = np.zeros((4, 8, 4), np.uint8)
    img[:2, :4, 2] = 255
    img[:2, 4:, 2] = 1
    assert Cc.thumb(img, 4)[0, :, 2].tolist() == [128, 1]


def test_thumb_reads_nothing_past_its_last_whole_block():
    case = next(c for c in Cc.thumb_cases() if c["name"] == "cstep4_odd")
    img, cstep = case["img"], case["cstep"]
    a = Cc.thumb(img, cstep)
    edit = img.copy()
    h, w = img.shape[:2]
    edit[h // cstep * cstep:] ^= 255
    edit[:, w // cstep * cstep:] ^= 255
    edit[..., 3] ^= 255
    assert np.array_equal(a, Cc.thumb(edit, cstep))


# ---------------------------------------------------------------------------------------------------- integrate
@pytest.mark.parametrize("name", [c["name"] for c in Mc.integrate_cases()])
def test_distance_and_weight_are_mesh_cases_integrate(name):
    ic = next(c for c in Mc.integrate_cases() if c["name"] == name)
    N = ic["q"].shape[0]
    c = Cc._ccase(ic, 7, prior=Cc.hashed_color_volume(N, 8, w_max=ic["w_max"]))
    want = Mc.integrate(ic["q"], ic["w"], ic["origin3"], ic["voxel"], ic["trunc"], ic["T_cw12"], ic["calib8"], ic["width"], ic["height"],
                        ic["step"], ic["meas"], ic["w_max"])
    got = Cc.run_integrate_color(c)
    assert np.array_equal(got["q"], want["q"]) and np.array_equal(got["w"], want["w"])
    assert np.array_equal(got["info"][:6], want["info"][:6]) and got["info"][7] == 0
    assert np.array_equal(got["cat"], want["cat"]) and np.array_equal(got["free"], want["free"])
    # K1
    assert np.array_equal(got["colored"], (want["cat"] == 0) & ~want["free"] & got["in_thumb"])
    assert got["info"][6] == got["colored"].sum()
    # what is not coloured keeps its bytes
    assert np.array_equal(got["c"][~got["colored"]], c["c"][~got["colored"]])


def test_every_color_case_takes_its_branches():
    cases = {c["name"]: c for c in Cc.integrate_color_cases()}
    total = 0
    for c in cases.values():
        r = Cc.run_integrate_color(c)
        total += int(r["info"][6])
    assert total > 1000
    r = Cc.run_integrate_color(cases["thumb_gate"])
    gated = (r["cat"] == 0) & ~r["free"] & ~r["in_thumb"]
    print("thumb_gate: coloured", int(r["info"][6]), "gated by the thumbnail", int(gated.sum()))
    assert gated.sum() > 0 and r["info"][6] > 0
    r = Cc.run_integrate_color(cases["n16_conf_edges"])
    wc0 = cases["n16_conf_edges"]["c"][..., 3][r["colored"]]
    assert set(np.unique(wc0).tolist()) == {0, 1, Mc.W_MAX - 1, Mc.W_MAX}   # every kind of prior weight meets a measurement


def test_fusing_the_same_colour_again_leaves_it_fixed_and_the_weight_saturates():
    ic = next(c for c in Mc.integrate_cases() if c["name"] == "wall_fronto")
    tw, th = ic["width"] // 4, ic["height"] // 4
    t = np.zeros((th, tw, 4), np.uint8)
    t[..., :3] = (201, 17, 96)
    c = Cc._ccase(ic, 0, thumb_img=t)
    q, w, col = c["q"], c["w"], c["c"]
    seen = np.zeros(q.shape, bool)
    for n in range(8):   # w_m = 200 >> 3 = 25: 25, 50, ... saturates at 128 in the sixth round
        r = Cc.integrate_color(q, w, col, c["origin3"], c["voxel"], c["trunc"], c["T_cw12"], c["calib8"], c["width"], c["height"], c["step"],
                               c["meas"], t, 4, c["w_max"])
        q, w, col = r["q"], r["w"], r["c"]
        seen |= r["colored"]
        assert np.all(col[seen][:, :3] == (201, 17, 96))
        assert np.all(col[seen][:, 3] == min(Mc.W_MAX, 25 * (n + 1)))
        assert np.all(col[~seen] == 0)
    assert seen.sum() > 100 and col[..., 3].max() == Mc.W_MAX


def test_a_new_colour_pulls_by_its_weight():
    """one voxel's arithmetic by hand: c = 10 with wc = 3 meets c_m = 200 with w_m = 25: (2 (30 + 5000) + 28) / 56 = 180 (179.64...)"""
    ic = next(c for c in Mc.integrate_cases() if c["name"] == "wall_fronto")
    tw, th = ic["width"] // 4, ic["height"] // 4
    t = np.full((th, tw, 4), 200, np.uint8)
    N = ic["q"].shape[0]
    prior = np.zeros((N, N, N, 4), np.uint8)
    prior[..., :3] = 10
    prior[..., 3] = 3
    r = Cc.run_integrate_color(Cc._ccase(ic, 0, prior=prior, thumb_img=t))
    assert np.all(r["c"][r["colored"]] == (180, 180, 180, 28))


# ---------------------------------------------------------------------------------------------------- colour at
def test_color_at_codes_and_fractions():
    c, pts = Cc.color_at_volume(), Cc.color_at_points()
    r = Cc.color_at(c, Cc.CA_ORIGIN, Cc.CA_VOXEL, pts)
    code, f = r["code"], r["f"]
    assert set(np.unique(code).tolist()) == {0, 1, 2, 4}
    ok = code == 0
    assert (f[ok] == 0).any() and (f[ok] == 256).any() and (f[ok] == 128).any()
    n_col = r["n_col"][code != 4]
    assert (n_col == 0).any() and (n_col == 1).any() and (n_col == 8).any() and ((n_col > 1) & (n_col < 8)).any()
    assert np.all(r["rgba"][~ok] == 0) and np.all(r["rgba"][ok, 3] == 255)
    assert r["info"][1:5].sum() == len(pts)
    # A1's ends are inside, a float32 either side decides
    e = Cc.end_points()
    r = Cc.color_at(np.full((8, 8, 8, 4), 9, np.uint8), Cc.CA_ORIGIN, Cc.CA_VOXEL, e)
    assert np.all(r["code"] == 0)
    codes = [Cc.color_at(np.full((8, 8, 8, 4), 9, np.uint8), o, Cc.CA_VOXEL, e)["code"] for o in Cc.nudged_origins()]
    assert all(0 < (k == 1).sum() < len(e) for k in codes)   # one double of the origin moves one end out and keeps the other in


def test_color_at_a_corner_is_that_voxel_and_a_constant_volume_is_constant():
    c = Cc.hashed_color_volume(8, 5)
    c[..., 3] = np.maximum(c[..., 3], 1)
    k, j, i = 3, 5, 2
    p = (Cc.CA_ORIGIN + (np.array([i, j, k]) + 0.5) * Cc.CA_VOXEL)[None]
    r = Cc.color_at(c, Cc.CA_ORIGIN, Cc.CA_VOXEL, p)
    assert r["rgba"][0, :3].tolist() == c[k, j, i, :3].tolist()
    c[..., :3] = (7, 200, 255)
    r = Cc.color_at(c, Cc.CA_ORIGIN, Cc.CA_VOXEL, Cc.color_at_points())
    assert np.all(r["rgba"][r["code"] == 0] == (7, 200, 255, 255))


# ---------------------------------------------------------------------------------------------------- end to end
# Measured on the painted scene (mesh_color_cases.PAINT_BOX on mesh_cases' wall, every surface its own base colour plus a colour linear in
# the world coordinates, mesh_cases' 8 exact views rendered at 256 x 192, thumbnail step 4, depth grid 64 x 48, N = 32, min_weight 2;
# 1073 used vertices): the largest and the mean channel error, in counts of 255, of a used vertex that is more than 1.5 voxels from a box
# edge and, in every view, from a silhouette or an edge between two surfaces (875 of them; 18.45 % are excluded); every such vertex has
# a colour.  The restatement is deterministic, so this is what it gives; the assertion allows twice the largest error.  The excluded
# share is a condition (at most 25 %), not a measurement
E2E_COLOR_MAX, E2E_COLOR_MEAN = 1.6291, 0.350
E2E_EXCLUDED_CAP = 0.25


def e2e_color_measure():
    run = Cc.e2e_color_run()
    m, voxel = run["mesh"], run["voxel"]
    V = m["vertices"].astype(np.float64)
    used = Mc.used_vertices(m["triangles"], len(V))
    excl = Cc.e2e_excluded(V, voxel, run["sids"], run["calib"], run["width"], run["height"])
    keep = used & ~excl
    sid = Cc.surface_id(V, 1.5 * voxel)
    want = Cc.paint(V, sid)
    got = run["colors"]
    err = np.abs(got["rgba"][:, :3].astype(np.float64) - want)
    has = got["code"] == 0
    return dict(keep=keep, used=used, has=has, sid=sid, err=err, excluded=float((used & excl).sum() / used.sum()))


def test_end_to_end_painted_scene():
    r = e2e_color_measure()
    keep, err = r["keep"], r["err"]
    print(f"e2e colour: used {int(r['used'].sum())}, excluded share {r['excluded']:.4f}, kept {int(keep.sum())}, without a colour "
          f"{int((keep & ~r['has']).sum())}, off every surface {int((keep & (r['sid'] == 0)).sum())}, max error {err[keep & r['has']].max():.3f}, "
          f"mean {err[keep & r['has']].mean():.3f}")
    assert r["excluded"] <= E2E_EXCLUDED_CAP
    assert keep.sum() > 500
    assert np.all(r["sid"][keep] > 0)
    assert np.all(r["has"][keep])
    assert err[keep].max() <= 2 * E2E_COLOR_MAX
