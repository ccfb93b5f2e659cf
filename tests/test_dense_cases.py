"""CPU: the numpy restatement of alva_depth_fuse and alva_depth_fill (tests/dense_cases.py) against things that are not the restatement:
the warp against closed-form geometry, the fusion against the analytic depth, the fill against a brute-force nearest-seed fill, against
the plain (not edge-aware) push-pull and against a cell-by-cell transcription of P1-P4 in plain Python."""
from __future__ import annotations

import numpy as np
import pytest

import dense_cases as Dn
import depth_cases as Dc

F32 = np.float32
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)


def _plane_state(z, gw, gh, w=10):
    return np.full((gh, gw), F32(1.0 / z), F32), np.full((gh, gw), w, np.uint8)


# ---------------------------------------------------------------------------------------------------- warp against geometry
def test_lateral_translation_carries_a_fronto_parallel_plane_at_its_depth():
    z, step, cells = 4.0, 4, 2
    cal = Dc.calib_of()
    gw, gh = Dc.W // step, Dc.H // step
    t = cells * step * z / Dc.F                       # the image moves by two cells
    T = np.concatenate([IDENT[:9], [t, -t, 0.0]])
    rho, w = _plane_state(z, gw, gh)
    keys, target, rho_new = Dn.warp(rho, w, T, cal, Dc.W, Dc.H, step)
    gy, gx = np.mgrid[0:gh, 0:gw]
    want = np.where((gx + cells < gw) & (gy - cells >= 0), (gy - cells) * gw + gx + cells, -1).reshape(-1)
    assert np.array_equal(target, want)
    got = Dn.fuse((rho, w), T, cal, Dc.W, Dc.H, step, None, decay=256)
    carried = got["src"] == 2
    assert carried.sum() == (gw - cells) * (gh - cells) and (got["src"][~carried] == 0).all()
    err = np.abs(1.0 / got["rho"][carried].astype(np.float64) / z - 1)
    print("lateral: largest relative error", err.max())
    assert err.max() <= 1e-6                          # one float rounding of rho, one of rho'
    assert (got["w"][carried] == 10).all()


def test_forward_translation_carries_a_plane_at_depth_minus_t_z():
    z, tz, step = 4.0, 0.5, 4
    cal = Dc.calib_of()
    gw, gh = Dc.W // step, Dc.H // step
    T = np.concatenate([IDENT[:9], [0.0, 0.0, -tz]])   # the camera moves forward: X_cur = X_prev - (0, 0, tz)
    rho, w = _plane_state(z, gw, gh)
    got = Dn.fuse((rho, w), T, cal, Dc.W, Dc.H, step, None, decay=256)
    carried = got["src"] == 2
    assert carried.sum() > 0.7 * gw * gh              # the image grows about the centre: the inner cells spread over the grid
    err = np.abs(1.0 / got["rho"][carried].astype(np.float64) / (z - tz) - 1)
    print("forward: largest relative error", err.max(), "cells", int(carried.sum()))
    assert err.max() <= 1e-6


@pytest.mark.parametrize("dist", [(0.0, 0.0, 0.0, 0.0), Dc.K_DIST4], ids=["pinhole", "distorted"])
@pytest.mark.parametrize("step", [1, 2, 4, 16])
def test_identity_maps_every_cell_to_itself(step, dist):
    cal = Dc.calib_of(dist=dist)
    gw, gh = Dc.W // step, Dc.H // step
    rho, w = Dn.state_of(2.0 + Dn.hashed_unit(gw * gh, 7).reshape(gh, gw), 8, share=1.0)
    keys, target, rho_new = Dn.warp(rho, w, IDENT, cal, Dc.W, Dc.H, step)
    assert np.array_equal(target, np.arange(gw * gh))
    assert np.array_equal(rho_new.view(np.uint32), rho.reshape(-1).view(np.uint32))   # P.z is exactly 1
    got = Dn.fuse((rho, w), IDENT, cal, Dc.W, Dc.H, step, None, decay=256)
    assert np.array_equal(got["rho"].view(np.uint32), rho.view(np.uint32)) and np.array_equal(got["w"], w) and (got["src"] == 2).all()


def test_where_a_near_and_a_far_plane_land_in_one_cell_the_near_one_is_kept():
    step = 4
    cal = Dc.calib_of()
    gw, gh = Dc.W // step, Dc.H // step
    gy, gx = np.mgrid[0:gh, 0:gw]
    near = (gx + gy) % 2 == 1                         # a checkerboard of the two planes
    rho = np.where(near, F32(1.0 / Dc.NEAR_Z), F32(1.0 / Dc.FAR_Z)).astype(F32)
    w = np.full((gh, gw), 10, np.uint8)
    T = np.concatenate([IDENT[:9], [0.35, 0.0, 0.0]])   # 20.3 px for the far plane, 31.2 px for the near one
    keys, target, rho_new = Dn.warp(rho, w, T, cal, Dc.W, Dc.H, step)
    flat_near = near.reshape(-1)
    hit_near = np.unique(target[(target >= 0) & flat_near])
    hit_far = np.unique(target[(target >= 0) & ~flat_near])
    both = np.intersect1d(hit_near, hit_far)
    assert len(both) > 200
    got = Dn.fuse((rho, w), T, cal, Dc.W, Dc.H, step, None, decay=256)
    depth_both = 1.0 / got["rho"].reshape(-1)[both].astype(np.float64)
    assert (np.abs(depth_both / Dc.NEAR_Z - 1) <= 1e-6).all()
    assert flat_near[got["source"].reshape(-1)[both]].all()
    only_far = np.setdiff1d(hit_far, hit_near)
    assert len(only_far) and (np.abs(1.0 / got["rho"].reshape(-1)[only_far].astype(np.float64) / Dc.FAR_Z - 1) <= 1e-6).all()


def test_ties_go_to_the_lowest_source_index_and_the_nearest_wins():
    c = Dn.fuse_cases()["collapse_all_into_one_ties"]
    got = Dn.oracle_fuse("collapse_all_into_one_ties")
    rho = c["prev"][0].reshape(-1)
    cells = np.nonzero(got["source"].reshape(-1) >= 0)[0]
    assert len(cells) == 1                            # every source lands in the principal point's cell
    winner = int(got["source"].reshape(-1)[cells[0]])
    assert rho[winner] == rho.max() and winner == int(np.nonzero(rho == rho.max())[0][0]) and (rho == rho.max()).sum() > 50


def test_the_fuse_cases_reach_every_src_and_every_drop():
    seen = set()
    for name in Dn.fuse_cases():
        seen |= set(np.unique(Dn.oracle_fuse(name)["src"]).tolist())
    assert seen == {0, 1, 2, 3, 4, 5}
    assert Dn.oracle_fuse("decay_0")["info"][2] == 0 and Dn.oracle_fuse("decay_0")["info"][3] == 0
    assert (Dn.oracle_fuse("w_max_40_saturates")["w"][Dn.oracle_fuse("w_max_40_saturates")["src"] == 3] <= 40).all()
    assert (Dn.oracle_fuse("w_max_40_saturates")["w"][Dn.oracle_fuse("w_max_40_saturates")["src"] == 3] == 40).any()
    assert not (Dn.oracle_fuse("all_behind")["source"] >= 0).any()
    c = Dn.fuse_cases()["behind_the_camera"]
    _, target, _ = Dn.warp(c["prev"][0], c["prev"][1], c["T"], c["calib8"], c["width"], c["height"], c["step"])
    live = (c["prev"][1] > 0).reshape(-1)
    assert (target[live] >= 0).any() and (target[live] < 0).any()
    assert Dn.oracle_fuse("width60_step8")["info"][6:].tolist() == [7, 8]


# ---------------------------------------------------------------------------------------------------- fusion against the analytic depth
def test_fusing_four_noisy_measurements_halves_the_error():
    step, K = 4, 4
    cal = Dc.calib_of()
    truth = Dc.grid_truth(Dc.two_depth_frame(40)[1], step)
    n = truth.size
    state, singles = None, []
    for k in range(K):
        e = (Dn.hashed_unit(n, 900 + k).reshape(truth.shape) * 2 - 1) * 0.02
        depth = (truth * (1 + e)).astype(F32)
        singles.append(float(np.median(np.abs(depth.astype(np.float64) / truth - 1))))
        got = Dn.fuse(state, IDENT, cal, Dc.W, Dc.H, step, (depth, np.full(truth.shape, 255, np.uint8), np.zeros(truth.shape, np.uint8)),
                      decay=256)
        state = (got["rho"], got["w"])
    assert (got["src"] == 3).all() and (got["w"] == 124).all()   # 4 x (255 >> 3), under w_max
    fused = float(np.median(np.abs(1.0 / got["rho"].astype(np.float64) / truth - 1)))
    print("median relative error: single measurements", singles, "fused", fused)
    assert fused < min(singles)


def test_a_jump_of_30_percent_replaces_a_light_cell_and_only_weakens_a_heavy_one():
    cal = Dc.calib_of(64, 64, 58.0)
    rho = np.full((16, 16), F32(0.25), F32)
    w = np.full((16, 16), 40, np.uint8)
    w[:, 8:] = 12
    depth = np.full((16, 16), F32(4.0 * 1.3), F32)
    conf = np.full((16, 16), 160, np.uint8)            # w_m = 20
    got = Dn.fuse((rho, w), IDENT, cal, 64, 64, 4, (depth, conf, np.zeros((16, 16), np.uint8)), decay=256)
    assert (got["src"][:, :8] == 5).all() and (got["w"][:, :8] == 20).all() and (got["rho"][:, :8] == F32(0.25)).all()
    assert (got["src"][:, 8:] == 4).all() and (got["w"][:, 8:] == 20).all()
    assert np.array_equal(got["rho"][:, 8:], (1.0 / depth[:, 8:].astype(np.float64)).astype(F32))
    tie = Dn.fuse((rho, np.full((16, 16), 20, np.uint8)), IDENT, cal, 64, 64, 4, (depth, conf, np.zeros((16, 16), np.uint8)), decay=256)
    assert (tie["src"] == 4).all()                     # w_m >= w'


# ---------------------------------------------------------------------------------------------------- fill: a transcription in plain Python
def fill_scalar(rho, w, guide, rho_ref, L):
    """P1-P4 cell by cell, on a grid with step 1"""
    gh, gw = w.shape
    lv = [{}]
    for y in range(gh):
        for x in range(gw):
            q = 0
            if w[y, x] > 0:
                q = min(max(int(np.rint(float(rho[y, x]) / rho_ref * 65536.0)), 0), (1 << 20) - 1)
            lv[0][(x, y)] = (q, int(w[y, x]), int(guide[y, x]))
    dims = [(gw, gh)]
    for l in range(L):
        cw, ch = (dims[l][0] + 1) // 2, (dims[l][1] + 1) // 2
        cur = {}
        for y in range(ch):
            for x in range(cw):
                kids = [lv[l][(2 * x + dx, 2 * y + dy)] for dy in (0, 1) for dx in (0, 1) if (2 * x + dx, 2 * y + dy) in lv[l]]
                ws = sum(k[1] for k in kids)
                q = (sum(k[1] * k[0] for k in kids) + ws // 2) // ws if ws else 0
                cur[(x, y)] = (q, min(255, ws), (sum(k[2] for k in kids) + len(kids) // 2) // len(kids))
        lv.append(cur)
        dims.append((cw, ch))
    val = {c: (v[0], L) for c, v in lv[L].items() if v[1] > 0}
    for l in range(L - 1, -1, -1):
        nxt = {}
        for (x, y), (q, W, g) in lv[l].items():
            if W > 0:
                nxt[(x, y)] = (q, l)
                continue
            S = acc = 0
            ev = 255
            for py, wy in ((y >> 1, 3), ((y >> 1) + (1 if y & 1 else -1), 1)):
                for px, wx in ((x >> 1, 3), ((x >> 1) + (1 if x & 1 else -1), 1)):
                    if (px, py) in val:
                        d = abs(g - lv[l + 1][(px, py)][2])
                        wt = wx * wy * max(1, 64 >> min(d >> 3, 6))
                        S += wt
                        acc += wt * val[(px, py)][0]
                        ev = min(ev, val[(px, py)][1])
            if S > 0:
                nxt[(x, y)] = ((acc + S // 2) // S, ev)
        val = nxt
    depth, level = np.zeros((gh, gw), F32), np.full((gh, gw), 255, np.uint8)
    for y in range(gh):
        for x in range(gw):
            if w[y, x] > 0:
                depth[y, x], level[y, x] = F32(1.0 / float(rho[y, x])), 0
            elif (x, y) in val and val[(x, y)][0] > 0:
                depth[y, x], level[y, x] = F32(65536.0 / (float(val[(x, y)][0]) * rho_ref)), val[(x, y)][1]
    return depth, level


@pytest.mark.parametrize("name", [n for n, c in Dn.fill_cases().items() if c["step"] == 1 and c["rho"].size <= 3100])
def test_fill_equals_the_cell_by_cell_transcription_evidence_levels_included(name):
    c = Dn.fill_cases()[name]
    want_depth, want_level = fill_scalar(c["rho"], c["w"], c["gray"], c["rho_ref"], c["max_level"])
    got = Dn.oracle_fill(name)
    assert np.array_equal(got["level"], want_level)
    assert np.array_equal(got["depth"].view(np.uint32), want_depth.view(np.uint32))
    assert got["info"].tolist() == [int((want_level == 0).sum()), int(((want_level > 0) & (want_level < 255)).sum()), int((want_level == 255).sum()),
                                    int(want_level[(want_level > 0) & (want_level < 255)].max(initial=0))]


def test_odd_grids_work():
    for name in ("odd_7x5_L3", "odd_1x1_L1", "odd_1x1_L8", "odd_17x1_L4", "odd_1x19_L5"):
        got = Dn.oracle_fill(name)
        assert got["depth"].shape == Dn.fill_cases()[name]["w"].shape and got["info"][:3].sum() == got["depth"].size
    one = Dn.oracle_fill("odd_1x1_L8")
    assert one["level"][0, 0] == 0 and one["depth"][0, 0] == F32(1.0 / float(Dn.fill_cases()["odd_1x1_L8"]["rho"][0, 0]))


# ---------------------------------------------------------------------------------------------------- fill against the analytic two-surface grid
def _nearest_seed_fill(s):
    ys, xs = np.nonzero(s["seed"])
    Y, X = np.mgrid[0:s["truth"].shape[0], 0:s["truth"].shape[1]]
    d2 = (Y[..., None] - ys) ** 2 + (X[..., None] - xs) ** 2
    k = d2.argmin(-1)                                  # the first of equally near seeds
    return 1.0 / s["rho"][ys[k], xs[k]].astype(np.float64)


@pytest.mark.parametrize("share", [0.30, 0.05])
def test_fill_beats_the_nearest_seed_and_the_plain_fill_on_the_two_surface_grid(share):
    s = Dn.two_surface_grid(share=share)
    got = Dn.fill(s["rho"], s["w"], s["guide"], 1, 1.0, 5)
    plain = Dn.fill(s["rho"], s["w"], s["guide"], 1, 1.0, 5, edge_aware=False)
    assert (got["depth"] > 0).all() and got["info"][2] == 0          # coverage is 100 % at max_level 5
    assert np.array_equal(got["depth"][s["seed"]].view(np.uint32), (1.0 / s["rho"][s["seed"]].astype(np.float64)).astype(F32).view(np.uint32))
    assert (got["level"][s["seed"]] == 0).all() and (got["level"][~s["seed"]] >= 1).all() and got["level"].max() <= 5
    err = np.abs(got["depth"].astype(np.float64) / s["truth"] - 1)
    err_nn = np.abs(_nearest_seed_fill(s) / s["truth"] - 1)
    hole = s["hole"]
    X = np.mgrid[0:s["truth"].shape[0], 0:s["truth"].shape[1]][1]
    band = (np.abs(X - s["edge_x"][:, None]) <= 3) & ~s["seed"]
    in3 = float((err[band] <= 0.03).mean())
    in3_plain = float((np.abs(plain["depth"].astype(np.float64) / s["truth"] - 1)[band] <= 0.03).mean())
    print("share %.2f: hole median %.5f (nearest seed %.5f), hole max %.4f (nearest seed %.4f), band within 3 %%: %.3f (plain %.3f), %d band cells"
          % (share, np.median(err[hole]), np.median(err_nn[hole]), err[hole].max(), err_nn[hole].max(), in3, in3_plain, band.sum()))
    assert np.median(err[hole]) < np.median(err_nn[hole])
    assert err[hole].max() < err_nn[hole].max()
    assert in3 >= 2 * in3_plain


def test_max_level_1_leaves_the_holes_interior_empty():
    s = Dn.two_surface_grid()
    got = Dn.fill(s["rho"], s["w"], s["guide"], 1, 1.0, 1)
    gh, gw = s["w"].shape
    inner = np.zeros((gh, gw), bool)
    inner[gh // 2 - 4:gh // 2 + 4, gw // 2 - 6:gw // 2 + 6] = True   # two cells inside the hole's rim
    assert (got["depth"][inner] == 0).all() and (got["level"][inner] == 255).all()
    assert set(np.unique(got["level"]).tolist()) == {0, 1, 255}


def test_a_grid_without_a_seed_stays_empty():
    got = Dn.oracle_fill("no_seed")
    assert not got["depth"].any() and (got["level"] == 255).all() and got["info"].tolist() == [0, 0, 256, 0]


def test_a_corner_seed_reaches_as_far_as_max_level_allows():
    for L in (4, 8):
        got = Dn.oracle_fill("corner_seed_00_flat_guide_L4" if L == 4 else "corner_seed_00_L8")
        assert got["level"][0, 0] == 0 and (got["depth"] > 0).all()   # 16 x 16 is one cell at level 4
        assert got["level"].max() == 4                                # and no evidence lies farther away than that
    q = Dn.oracle_fill("q_clips_both_ends")["q"]
    c = Dn.fill_cases()["q_clips_both_ends"]
    q0, _ = Dn.quantise(c["rho"], c["w"], c["rho_ref"])
    assert (q0 == Dn.Q_MAX).any() and ((q0 == 0) & (c["w"] > 0)).any() and q.max() <= Dn.Q_MAX


# ---------------------------------------------------------------------------------------------------- on the sweep's dense scenes (reported)
@pytest.mark.parametrize("name", ["dense_40_10_r2", "dense_90_60_r2"])
def test_report_the_filled_cells_on_the_sweeps_dense_scenes(name):
    c = Dc.cases()[name]
    sw = Dc.oracle_case(name)
    step = c["kw"]["step"]
    fused = Dn.fuse(None, IDENT, c["calib8"], Dc.W, Dc.H, step, (sw["depth"], sw["conf"], sw["code"]))
    got = Dn.fill(fused["rho"], fused["w"], c["cur"], step, 2.0 * c["rho"][1], 5)
    k_cur = int(name.split("_")[1])
    truth = Dc.grid_truth(Dc.two_depth_frame(k_cur)[1], step)
    filled = (got["level"] > 0) & (got["level"] < 255)
    err = np.abs(got["depth"].astype(np.float64) / truth - 1)
    within3 = float((err[filled] <= 0.03).mean())
    print("%s: raw coverage %.3f, dense coverage %.3f, filled cells within 3 %% of the analytic depth: %.3f (median error %.4f)"
          % (name, (sw["code"] == 0).mean(), (got["depth"] > 0).mean(), within3, np.median(err[filled])))
    assert fused["info"][1] == sw["info"][0] and (got["level"][sw["code"] == 0] == 0).all() and filled.any()   # reported, not bounded
