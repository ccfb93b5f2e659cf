"""Dense depth through the system surface (alva_system_depth_dense, AlvaAR(depth=True).depthDense) on the tracking stream of
tests/test_gpu_depth_system.py: every call equals the two stages replayed from what alva_system_debug_depth_dense hands back, the state's
life (it grows, survives a LOST episode, is emptied by every reset the header lists), and that a session that asks for dense depth on
every frame tracks -- and answers alva_system_depth -- bit for bit like one that never does.

A tracked frame with a state but without a reference frame (code 7, warp only) does not occur on that stream -- the ring keeps four
frames at growing baselines, so one of them always qualifies --; the last test builds a stream on which it does: the camera turns in place."""
from __future__ import annotations

import numpy as np
import pytest

import dense_cases as Dn
import sysdiff
from alvaar_amd import synth

pytestmark = pytest.mark.gpu

W, H, CELL = 640, 480, 12
SPEED, N_TRACK, N_BLACK, N_AFTER = 3, 110, 8, 8     # the stream of tests/test_gpu_depth_system.py
RESUME_K = SPEED * 85
STEP, LEVEL = 8, 5                                  # 80 x 60 grid pixels
KW = dict(step=STEP, max_level=LEVEL)


def _views():
    return [SPEED * k for k in range(N_TRACK)] + [None] * N_BLACK + [RESUME_K + SPEED * j for j in range(N_AFTER)]


def _calib8(k):
    return (k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"])


def _replay(ctx, ar, out):
    """the two stages called directly on what the debug call handed back -> the list of what differs from the system call's answer"""
    import torch
    depth, weight, src, level, info = out
    bad = []
    if info["ran"] < 0:
        return bad
    cal = _calib8(ar.intrinsics)
    if info["ran"] >= 1:
        prev = (torch.from_numpy(info["rho_before"]).cuda(), torch.from_numpy(info["w_before"]).cuda()) if info["ran"] == 2 else None
        meas = tuple(torch.from_numpy(a).cuda() for a in info["raw"]) if info["did_sweep"] else None
        rho, w, s, finfo = ctx.depth_fuse(prev, info["T_cp"], cal, W, H, STEP, meas, decay=Dn.DECAY, w_max=Dn.W_MAX, rel_tol=Dn.REL_TOL)
        for name, a, b in (("rho", rho, info["rho_after"]), ("w", w, weight), ("src", s, src)):
            if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
                bad.append(name)
        if finfo[:6].tolist() != info["fuse"].tolist():
            bad.append("fuse info")
    d, lv, linfo = ctx.depth_fill(torch.from_numpy(info["rho_after"]).cuda(), torch.from_numpy(weight).cuda(), torch.from_numpy(info["gray"]).cuda(),
                                  STEP, info["rho_ref"], LEVEL)
    if not np.array_equal(d.view(np.uint32), depth.view(np.uint32)):
        bad.append("depth")
    if not np.array_equal(lv, level):
        bad.append("level")
    if (int(linfo[1]), int(linfo[2])) != (info["filled"], info["empty"]) or info["count"] != int(linfo[0] + linfo[1]):
        bad.append("fill info")
    return bad


@pytest.fixture(scope="module")
def frames():
    import torch
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    black = np.zeros((H, W, 4), np.uint8) + np.array([0, 0, 0, 255], np.uint8)
    return torch.from_numpy(np.stack([black if v is None else synth.plane_stream_frame(canvas, v, W, H, f) for v in _views()])).cuda()


@pytest.fixture(scope="module")
def runs(ctx, frames):
    """the same frames through three sessions: dense (depthDense and depthImage after every frame), raw (depthImage only), never"""
    from alvaar_amd.system import AlvaAR
    out = {}
    for name in ("dense", "raw", "never"):
        ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, relocalization=True, depth=name != "never")
        rec, raws, calls, twice = [], [], [], None
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [int(v) for v in ar.state()]))
            if name == "never":
                continue
            if name == "dense":
                a = ar.depthDense(debug=True, **KW)
                info = a[4]
                calls.append(dict(status=info["status"], ran=info["ran"], did_sweep=info["did_sweep"], warped=info["warped"], fuse=info["fuse"],
                                  swept=info["swept"], count=info["count"], filled=info["filled"], empty=info["empty"], bad=_replay(ctx, ar, a),
                                  weight=a[1].copy(), level=a[3].copy(), depth=a[0].copy(), rho_before=info.get("rho_before"),
                                  w_before=info.get("w_before"), rho_after=info.get("rho_after"), T_cp=info.get("T_cp"), poses=info.get("poses"),
                                  raw_code=info["raw"][2].copy()))
                if twice is None and info["ran"] == 2 and info["status"] == 0 and sum(c["ran"] == 2 for c in calls) == 5:
                    b = ar.depthDense(debug=True, **KW)
                    c = ar.depthDense(**KW)
                    twice = dict(first=a, second=b, plain=c, bad=_replay(ctx, ar, b), restated=_restate(ar, a))
            raws.append(ar.depthImage(step=STEP))
        out[name] = dict(rec=rec, raws=raws, calls=calls, twice=twice, counters=ar.counters())
        ar.close()
    return out


def _restate(ar, a):
    """the numpy restatement on the same hand-over"""
    depth, weight, src, level, info = a
    f = Dn.fuse((info["rho_before"], info["w_before"]), info["T_cp"], _calib8(ar.intrinsics), W, H, STEP, info["raw"])
    g = Dn.fill(f["rho"], f["w"], info["gray"], STEP, info["rho_ref"], LEVEL)
    return dict(f, depth=g["depth"], level=g["level"], fill_info=g["info"])


def test_every_call_equals_the_two_stages_replayed(runs):
    calls = runs["dense"]["calls"]
    assert sum(c["ran"] == 2 for c in calls) > 40 and sum(c["ran"] == 1 for c in calls) >= 1
    for k, c in enumerate(calls):
        assert c["bad"] == [], (k, c["ran"], c["bad"])
        if c["ran"] < 0:
            assert c["status"] in (6, 7) and c["count"] == 0 and not c["depth"].any() and (c["level"] == 255).all() and not c["weight"].any(), k
        else:
            assert c["count"] == (c["depth"] > 0).sum() and c["fuse"].sum() == c["depth"].size and c["warped"] == (c["ran"] == 2), k
            assert c["did_sweep"] == (c["status"] == 0) and c["swept"] == (c["raw_code"] == 0).sum(), k
    tw = runs["dense"]["twice"]
    assert tw is not None
    depth, weight, src, level, info = tw["first"]
    r = tw["restated"]
    assert np.array_equal(r["rho"].view(np.uint32), info["rho_after"].view(np.uint32)) and np.array_equal(r["w"], weight)
    assert np.array_equal(r["src"], src) and np.array_equal(r["depth"].view(np.uint32), depth.view(np.uint32)) and np.array_equal(r["level"], level)
    # T_cp is the motion between the two poses it came with
    Rp, Rc = sysdiff._quat_to_rot(info["poses"][0][3:]), sysdiff._quat_to_rot(info["poses"][1][3:])
    assert np.abs(info["T_cp"][:9].reshape(3, 3) - Rc.T @ Rp).max() < 1e-12
    assert np.abs(info["T_cp"][9:] - Rc.T @ (info["poses"][0][:3] - info["poses"][1][:3])).max() < 1e-12


def test_first_7_without_a_state_then_weights_grow_and_coverage_is_complete(runs):
    calls = runs["dense"]["calls"]
    status = [r[0] for r in runs["dense"]["rec"]]
    first_ok = status.index(1)
    assert all(c["status"] == 6 and c["ran"] == -1 for c in calls[:first_ok])
    assert calls[first_ok]["status"] == 7 and calls[first_ok]["ran"] == -1      # no reference frame and no state: nothing is launched
    ran = [k for k, c in enumerate(calls) if c["ran"] >= 1]
    assert calls[ran[0]]["ran"] == 1 and calls[ran[0]]["status"] == 0 and all(calls[k]["ran"] == 2 for k in ran[1:6])
    means = [float(calls[k]["weight"].astype(np.float64).mean()) for k in ran[:6]]
    print("mean weight over the first six fused calls", means, "largest", [int(calls[k]["weight"].max()) for k in ran[:6]])
    assert all(b > a for a, b in zip(means, means[1:4]))                         # consecutive calls add up
    assert calls[ran[5]]["weight"].max() > calls[ran[0]]["weight"].max()
    k = ran[10]
    raw_cover = float((calls[k]["raw_code"] == 0).mean())
    dense_cover = float((calls[k]["depth"] > 0).mean())
    print("frame %d: raw coverage %.3f, dense coverage %.3f, levels %s" % (k, raw_cover, dense_cover, np.unique(calls[k]["level"]).tolist()))
    assert raw_cover < 0.5 and dense_cover == 1.0
    assert ((calls[k]["level"] == 0) == (calls[k]["weight"] > 0)).all()


def test_a_second_call_on_the_same_frame_does_not_fuse_again(runs):
    tw = runs["dense"]["twice"]
    (d1, w1, s1, l1, i1), (d2, w2, s2, l2, i2), (d3, w3, s3, l3, i3) = tw["first"], tw["second"], tw["plain"]
    assert i1["ran"] == 2 and i2["ran"] == 0 and tw["bad"] == []
    for a, b, c in ((d1, d2, d3), (w1, w2, w3), (s1, s2, s3), (l1, l2, l3)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8))
    assert np.array_equal(i1["rho_after"].view(np.uint32), i2["rho_after"].view(np.uint32))
    for key in ("filled", "empty", "status", "swept", "warped", "count"):
        assert i1[key] == i2[key] == i3[key], key
    assert i1["fuse"].tolist() == i2["fuse"].tolist() == i3["fuse"].tolist()


def test_code_6_keeps_the_state_across_a_lost_episode(runs):
    calls = runs["dense"]["calls"]
    status = [r[0] for r in runs["dense"]["rec"]]
    lost = [k for k, st in enumerate(status) if st == 4]
    assert lost
    for k in lost:
        assert calls[k]["status"] == 6 and calls[k]["ran"] == -1
    before = max(k for k in range(lost[0]) if calls[k]["ran"] >= 1)
    after = min(k for k in range(lost[-1] + 1, len(calls)) if calls[k]["ran"] >= 1)
    assert all(calls[k]["ran"] == -1 for k in range(before + 1, after))
    assert calls[after]["ran"] == 2                                              # warped from the state of before the loss, not begun afresh
    assert np.array_equal(calls[after]["rho_before"].view(np.uint32), calls[before]["rho_after"].view(np.uint32))
    assert np.array_equal(calls[after]["w_before"], calls[before]["weight"])
    assert np.array_equal(calls[after]["poses"][0], calls[before]["poses"][1])


def test_dense_calls_change_nothing_else(runs):
    never = runs["never"]["rec"]
    assert 1 in [r[0] for r in never] and 4 in [r[0] for r in never]
    for name in ("dense", "raw"):
        rec = runs[name]["rec"]
        assert len(rec) == len(never)
        for k, (ra, rb) in enumerate(zip(rec, never)):
            assert ra[0] == rb[0] and ra[3] == rb[3], (name, k)
            assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), (name, k)
    assert runs["dense"]["counters"] == runs["never"]["counters"] == runs["raw"]["counters"] and runs["never"]["counters"]["ba_solves"] > 0
    # alva_system_depth between dense calls answers the bytes it answers without them
    answered = 0
    for k, (a, b) in enumerate(zip(runs["dense"]["raws"], runs["raw"]["raws"])):
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
        assert a[3]["status"] == b[3]["status"] and a[3]["counts"].tolist() == b[3]["counts"].tolist(), k
        answered += a[3]["status"] == 0
    assert answered > 40


class _Feeder:
    """frames of the stream into a session, from any index on, with timestamps that keep growing"""

    def __init__(self, ar, frames):
        self.ar, self.frames, self.t, self.k = ar, frames, 0, 0

    def feed(self, k=None):
        if k is not None:
            self.k = k
        st = self.ar.find_camera_pose_device(int(self.frames[self.k].data_ptr()), 33.0 * self.t)
        self.k += 1
        self.t += 1
        return st

    def until_fused(self, start=None, limit=100):
        """feeds frames, asking for dense depth after each, until a call fuses -> that call's info and what was answered before it"""
        earlier = []
        for n in range(limit):
            self.feed(start if n == 0 else None)
            info = self.ar.depthDense(debug=True, **KW)[4]
            if info["ran"] >= 1:
                return info, earlier
            earlier.append((info["status"], info["ran"]))
        raise AssertionError("no dense call fused within %d frames: %s" % (limit, earlier))


def test_every_listed_reset_empties_the_state(frames):
    from alvaar_amd.system import AlvaAR, AlvaError, lib
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True)
    fd = _Feeder(ar, frames)
    black = N_TRACK                                   # the index of the first black frame

    def warps_next():
        fd.feed()
        info = ar.depthDense(debug=True, **KW)[4]
        assert info["ran"] == 2 and info["warped"] == 1, info["ran"]

    info, earlier = fd.until_fused(0)
    assert info["ran"] == 1 and info["warped"] == 0 and (7, -1) in earlier
    warps_next()
    # alva_system_reset_depth_dense
    ar.resetDepthDense()
    info = ar.depthDense(debug=True, **KW)[4]
    assert info["ran"] == 1 and info["warped"] == 0 and not info["rho_before"].any() and not info["w_before"].any()
    warps_next()
    # a changed step
    d16 = ar.depthDense(debug=True, step=16, max_level=LEVEL)
    assert d16[4]["ran"] == 1 and d16[0].shape == (H // 16, W // 16) and (d16[4]["gw"], d16[4]["gh"]) == (W // 16, H // 16)
    assert ar.depthDense(debug=True, **KW)[4]["ran"] == 1
    warps_next()
    # depth off: refused, and the state goes with the ring
    ar.set_depth(False)
    with pytest.raises(AlvaError, match="depth is off"):
        ar.depthDense(**KW)
    ar.set_depth(True)
    info = ar.depthDense(debug=True, **KW)[4]
    assert info["status"] in (6, 7) and info["ran"] == -1
    info, earlier = fd.until_fused()
    assert info["ran"] == 1
    warps_next()
    # alva_system_reset
    ar.reset()
    info = ar.depthDense(debug=True, **KW)[4]
    assert info["status"] == 6 and info["ran"] == -1
    info, earlier = fd.until_fused(0)
    assert info["ran"] == 1 and (7, -1) in earlier
    warps_next()
    # a new map: without relocalization the tracker starts over after the black frames
    gen = [fd.feed(black + j) for j in range(N_BLACK)]
    info, earlier = fd.until_fused(0)
    assert info["ran"] == 1 and (7, -1) in earlier, (gen, earlier)
    warps_next()
    # configure
    k = ar.intrinsics
    assert lib.alva_system_configure_ex(ar.h, W, H, k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"], CELL, 0, 0) == 0
    info = ar.depthDense(debug=True, **KW)[4]
    assert info["status"] == 6 and info["ran"] == -1
    info, earlier = fd.until_fused(0)
    assert info["ran"] == 1 and (7, -1) in earlier
    ar.close()


def test_the_state_grows_with_the_grid_inside_one_session(ctx, frames):
    """The first dense call of a session asks for the coarse grid of step 16, the second -- on the same frame -- for the file's grid of
    four times as many pixels: the device state is replaced by a larger one inside the live session.  The second call begins afresh on
    its grid and equals the stages replayed on what it handed back; the coarse grid again, on the next frame, begins afresh in the block
    that is now larger than it needs."""
    from alvaar_amd.system import AlvaAR
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True)
    fd = _Feeder(ar, frames)
    for n in range(100):                              # until a reference frame qualifies; no dense call before the coarse one
        fd.feed(0 if n == 0 else None)
        if ar.depthImage(step=STEP)[3]["status"] == 0:
            break
    else:
        raise AssertionError("no frame with a reference frame within 100")
    coarse = ar.depthDense(debug=True, step=16, max_level=LEVEL)
    assert coarse[4]["ran"] == 1 and coarse[4]["status"] == 0 and coarse[0].shape == (H // 16, W // 16)
    fine = ar.depthDense(debug=True, **KW)
    info = fine[4]
    assert info["ran"] == 1 and info["status"] == 0 and info["warped"] == 0 and info["did_sweep"] == 1
    assert (info["gw"], info["gh"]) == (W // STEP, H // STEP) and fine[0].shape == (H // STEP, W // STEP)
    assert not info["rho_before"].any() and not info["w_before"].any()
    assert info["count"] == (fine[0] > 0).sum() > 0 and info["fuse"].sum() == fine[0].size
    assert _replay(ctx, ar, fine) == []
    fd.feed()
    again = ar.depthDense(debug=True, step=16, max_level=LEVEL)
    assert again[4]["ran"] == 1 and again[4]["warped"] == 0 and again[0].shape == (H // 16, W // 16)
    assert not again[4]["rho_before"].any() and not again[4]["w_before"].any() and again[4]["fuse"].sum() == again[0].size
    ar.close()


def test_code_7_with_a_state_warps_it_without_a_measurement(ctx):
    """A stream built for this case: the tests' motion until a fused state exists, then the camera turns in place about its own y axis,
    one degree per frame.  In place no frame joins the ring (that takes a translation of 3 % of the median depth), and past acos(0.9) =
    25.8 degrees no kept frame looks the same way: a tracked frame with a state and without a reference frame.  Then it turns back."""
    import torch
    from alvaar_amd.system import AlvaAR
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5, margin=1400)   # room for the turned views
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True)
    count = [0]

    def step(R, t):
        frame = torch.from_numpy(synth.gray_to_rgba(synth.render_plane(canvas, W, H, f, R, t))).cuda()
        st = ar.find_camera_pose_device(int(frame.data_ptr()), 33.0 * count[0])
        count[0] += 1
        return st, ar.depthDense(debug=True, **KW)

    warped, k = 0, 0
    while warped < 8 and k < N_TRACK:
        st, a = step(*synth.plane_camera_pose(SPEED * k))
        warped += a[4]["ran"] == 2
        k += 1
    assert warped == 8 and a[4]["status"] == 0
    R0, t0 = synth.plane_camera_pose(SPEED * (k - 1))
    ring0 = ar.depth_ring()

    def turned(deg):
        return R0 @ synth.so3_exp(np.array([0.0, -np.radians(deg), 0.0])), t0

    seven, last, log, deg = None, a, [], 0
    while seven is None and deg < 45:
        deg += 1
        st, a = step(*turned(deg))
        log.append((deg, st, a[4]["status"], a[4]["ran"]))
        assert st == 1 and a[4]["status"] in (0, 7) and a[4]["ran"] == 2, log
        if a[4]["status"] == 7:
            seven = a
        else:
            last = a
    print("turning in place:", log)
    assert seven is not None and deg >= 20, log
    depth, weight, src, level, info = seven
    assert np.array_equal(ar.depth_ring(), ring0)                        # nothing joined the ring
    assert info["did_sweep"] == 0 and info["swept"] == 0 and info["warped"] == 1 and (info["raw"][2] == 255).all() and not info["raw"][0].any()
    assert set(np.unique(src).tolist()) <= {0, 2} and info["fuse"][2] > 0 and info["fuse"][[1, 3, 4, 5]].sum() == 0
    assert info["fuse"][0] + info["fuse"][2] == src.size
    assert _replay(ctx, ar, seven) == []
    # the state it warped is the one the call before left, and the weights it carries are those, decayed
    assert np.array_equal(info["rho_before"].view(np.uint32), last[4]["rho_after"].view(np.uint32)) and np.array_equal(info["w_before"], last[1])
    assert np.array_equal(info["poses"][0], last[4]["poses"][1])
    want = Dn.fuse((info["rho_before"], info["w_before"]), info["T_cp"], _calib8(ar.intrinsics), W, H, STEP, None)
    assert np.array_equal(want["rho"].view(np.uint32), info["rho_after"].view(np.uint32)) and np.array_equal(want["w"], weight)
    assert np.array_equal(want["src"], src)
    carried = src == 2
    assert np.array_equal(weight[carried], ((info["w_before"].reshape(-1)[want["source"][carried]].astype(np.int64) * Dn.DECAY) >> 8).astype(np.uint8))
    assert info["count"] == (depth > 0).sum() > 0 and ((level == 0) == (weight > 0)).all()
    assert 0 < info["rho_ref"] and np.isfinite(info["rho_ref"])          # the range needs no reference frame
    # the next frames warp from it, and with a reference frame again they measure again
    prev, back = seven, None
    while back is None and deg > 0:
        deg -= 1
        st, a = step(*turned(deg))
        assert st == 1 and a[4]["ran"] == 2, (deg, st, a[4]["ran"])
        assert np.array_equal(a[4]["rho_before"].view(np.uint32), prev[4]["rho_after"].view(np.uint32)) and np.array_equal(a[4]["w_before"], prev[1])
        assert _replay(ctx, ar, a) == []
        if a[4]["status"] == 0:
            back = a
        prev = a
    assert back is not None and back[4]["did_sweep"] == 1 and back[4]["swept"] > 0 and back[4]["fuse"][[1, 3, 4, 5]].sum() > 0
    ar.close()
