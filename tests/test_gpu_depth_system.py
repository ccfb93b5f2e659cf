"""Depth from motion through the system surface (alva_system_set_depth / alva_system_depth, AlvaAR(depth=True).depthImage) on the plane
stream of tests/test_gpu_hit_test.py and tests/test_gpu_relocalization.py: what the call answers and when, bit parity with the stage
called directly and with the numpy restatement tests/depth_cases.py, the ring of reference frames, and that a session with depth off --
or on -- tracks bit for bit like one that never heard of it."""
from __future__ import annotations

import numpy as np
import pytest

import depth_cases as Dc
import sysdiff
from alvaar_amd import synth

pytestmark = pytest.mark.gpu

W, H, CELL = 640, 480, 12
SPEED, N_TRACK, N_BLACK, N_AFTER = 3, 110, 8, 8     # the stream of tests/test_gpu_relocalization.py, with a shorter tail
RESUME_K = SPEED * 85
DETAIL_AFTER = 40                                   # frames after the first tracked one at which the answer is examined
STEP = 8                                            # 80 x 60 grid pixels: the restatement of the same sweep takes about 2 s
# Measured on the first GPU run (also in profiles/depth_timing.json): of the code-0 pixels of the examined frame, the share whose
# depth / analytic depth lies within 3 % of the median ratio (the map's one scale).  The test's floor is that value less a quarter of
# its distance to the trivial bound 0: the canvas is random and the tracker's poses carry their own error.
MEASURED_WITHIN3 = 0.9847   # 1500 of 4800 grid pixels answered, scale 3.68068, median |error| 0.00243


def _views():
    return [SPEED * k for k in range(N_TRACK)] + [None] * N_BLACK + [RESUME_K + SPEED * j for j in range(N_AFTER)]


def _analytic_depth(view, step):
    """the camera-space z of the plane z = 4 along the rays of the grid's centre pixels (synth.render_plane's lam)"""
    f = sysdiff.intrinsics(W, H)[0]
    R, t = synth.plane_camera_pose(view)
    xs, ys = np.meshgrid(np.arange(W // step) * step + step // 2, np.arange(H // step) * step + step // 2)
    d = np.stack([(xs - W * 0.5) / f, (ys - H * 0.5) / f, np.ones(xs.shape)], -1) @ R.T
    return (4.0 - t[2]) / d[..., 2]


@pytest.fixture(scope="module")
def runs():
    """the same frames through three sessions: depth on (depthImage after every frame), depth turned off, and never mentioned"""
    import torch
    from alvaar_amd.system import AlvaAR, AlvaError
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    views = _views()
    black = np.zeros((H, W, 4), np.uint8) + np.array([0, 0, 0, 255], np.uint8)
    dev = torch.from_numpy(np.stack([black if v is None else synth.plane_stream_frame(canvas, v, W, H, f) for v in views])).cuda()
    out = {}
    for name in ("on", "off", "never"):
        ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, relocalization=True, depth=name == "on")
        if name == "off":
            ar.set_depth(False)
        rec, answers, rings, seen, detail, first_ok, refused = [], [], [], [], None, None, None
        before = ar.depthImage(step=STEP) if name == "on" else None
        for k in range(len(views)):
            st = ar.find_camera_pose_device(int(dev[k].data_ptr()), 33.0 * k)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [int(v) for v in ar.state()]))
            if name != "on":
                continue
            answers.append(ar.depthImage(step=STEP))
            rings.append(ar.depth_ring())
            seen.append(len(ar.frame_map_point_ids()))
            if st == 1 and first_ok is None:
                first_ok = k
            if first_ok is not None and k == first_ok + DETAIL_AFTER and st == 1:
                detail = dict(frame=k, first=ar.depthImage(step=STEP, debug=True), second=ar.depthImage(step=STEP, debug=True),
                              plain=ar.depthImage(step=STEP), k=dict(ar.intrinsics), ring=ar.depth_ring(), pose7=ar.pose7()[0].copy())
        if name == "off":
            try:
                ar.depthImage()
            except AlvaError as e:
                refused = str(e)
        after_reset, counters = None, ar.counters()
        if name == "on":
            n_before = len(ar.depth_ring())
            ar.reset()
            after_reset = (n_before, len(ar.depth_ring()), ar.depthImage(step=STEP))
        out[name] = dict(rec=rec, answers=answers, rings=rings, seen=seen, detail=detail, before=before, first_ok=first_ok, refused=refused,
                         counters=counters, after_reset=after_reset)
        ar.close()
    return out


def test_answers_6_then_7_then_a_depth_image(runs):
    on = runs["on"]
    depth, conf, code, info = on["before"]   # before the first frame
    assert info["status"] == 6 and (code == 6).all() and not depth.any() and not conf.any() and not info["counts"].any()
    assert (info["gw"], info["gh"]) == (W // STEP, H // STEP) and code.shape == (H // STEP, W // STEP)
    status = [r[0] for r in on["rec"]]
    assert 3 in status and 4 in status and on["first_ok"] is not None
    blind = [k for k, (st, n) in enumerate(zip(status, on["seen"])) if st == 1 and n < 8]
    assert blind and min(blind) >= N_TRACK   # the first black frames still return 1, from the motion model, and see no map point
    for k, (st, (depth, conf, code, info)) in enumerate(zip(status, on["answers"])):
        if st != 1 or on["seen"][k] < 8:   # initialising (3), LOST (4), or fewer than 8 3-D points in the frame
            assert info["status"] == 6 and (code == 6).all() and not depth.any(), k
        else:
            assert info["status"] in (0, 7), k
            if info["status"] == 7:
                assert (code == 7).all() and not depth.any() and not info["counts"].any(), k
            else:
                assert info["counts"].sum() == code.size and (code <= 5).all() and info["counts"][0] == (code == 0).sum(), k
                assert ((depth > 0) == (code == 0)).all(), k
    # the first tracked frame is its own and only reference: no baseline yet
    assert on["answers"][on["first_ok"]][3]["status"] == 7 and len(on["rings"][on["first_ok"]]) == 1
    answered = [k for k, a in enumerate(on["answers"]) if a[3]["status"] == 0]
    assert answered and answered[0] - on["first_ok"] < 30 and len(answered) > 40


def test_depth_over_analytic_depth_is_the_maps_one_scale(runs):
    d = runs["on"]["detail"]
    assert d is not None
    depth, conf, code, info = d["first"]
    assert info["status"] == 0
    ok = code == 0
    ratio = depth[ok].astype(np.float64) / _analytic_depth(_views()[d["frame"]], STEP)[ok]
    scale = float(np.median(ratio))
    within3 = float((np.abs(ratio / scale - 1) <= 0.03).mean())
    print("frame %d: code 0 on %d of %d grid pixels, scale %.5f, within 3 %% of it: %.4f, within 5 %%: %.4f, median |error| %.5f" % (
        d["frame"], ok.sum(), ok.size, scale, within3, float((np.abs(ratio / scale - 1) <= 0.05).mean()),
        float(np.median(np.abs(ratio / scale - 1)))))
    assert within3 >= MEASURED_WITHIN3 - 0.25 * (MEASURED_WITHIN3 - 0.0)
    # the canvas is sparse: the floor on the number of answers is what the restatement gives on the same two images, poses and range
    want = Dc.sweep(info["cur"], info["ref"], _calib8(d["k"]), info["T_rc"], info["rho"][0], info["rho"][1], step=STEP, num_hyp=64,
                    patch_radius=2, min_texture=4, min_conf=96)
    print("restatement", want["info"].tolist(), "system", info["counts"].tolist())
    assert ok.sum() >= want["info"][0] > 100
    assert np.array_equal(code, want["code"]) and np.array_equal(conf, want["conf"])
    assert np.array_equal(depth.view(np.uint32), want["depth"].view(np.uint32))
    assert info["counts"].tolist() == want["info"][:6].tolist()


def _calib8(k):
    return (k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"])


def test_system_call_equals_the_stage_called_directly(ctx, runs):
    import torch
    d = runs["on"]["detail"]
    depth, conf, code, info = d["first"]
    got = ctx.depth_sweep(torch.from_numpy(info["cur"]).cuda(), torch.from_numpy(info["ref"]).cuda(), _calib8(d["k"]), info["T_rc"],
                          info["rho"][0], info["rho"][1], step=STEP, num_hyp=64, patch_radius=2, min_texture=4, min_conf=96)
    assert np.array_equal(got[0].view(np.uint32), depth.view(np.uint32)) and np.array_equal(got[1], conf) and np.array_equal(got[2], code)
    assert got[3][:6].tolist() == info["counts"].tolist() and (got[3][6], got[3][7]) == (info["gw"], info["gh"])
    # what the system handed over: the range from the frame's own points, a reference of the ring, a rotation matrix
    assert 0 < info["rho"][0] < info["rho"][1]
    R = info["T_rc"][:9].reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and R[2, 2] >= 0.9
    t_ref = [p[:3] for p in d["ring"]]
    c_ref = d["pose7"][:3] - sysdiff._quat_to_rot(d["pose7"][3:]) @ R.T @ info["T_rc"][9:]   # the reference's centre, from T_rc
    assert min(np.linalg.norm(c_ref - t) for t in t_ref) < 1e-9
    assert not np.array_equal(info["cur"], info["ref"]) and info["cur"].any() and info["ref"].any()


def test_two_calls_on_one_frame_return_the_same_bytes(runs):
    d = runs["on"]["detail"]
    for a, b, c in zip(d["first"][:3], d["second"][:3], d["plain"][:3]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8))
    for key in ("cur", "ref", "T_rc"):
        assert np.array_equal(d["first"][3][key], d["second"][3][key])
    assert d["first"][3]["rho"] == d["second"][3]["rho"] and d["first"][3]["counts"].tolist() == d["plain"][3]["counts"].tolist()


def test_depth_on_or_off_tracks_like_a_session_that_never_heard_of_it(runs):
    never = runs["never"]["rec"]
    assert 1 in [r[0] for r in never] and 4 in [r[0] for r in never]
    for name in ("off", "on"):
        rec = runs[name]["rec"]
        assert len(rec) == len(never)
        for k, (ra, rb) in enumerate(zip(rec, never)):
            assert ra[0] == rb[0] and ra[3] == rb[3], (name, k)
            assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), (name, k)
    assert runs["off"]["counters"] == runs["never"]["counters"] == runs["on"]["counters"] and runs["never"]["counters"]["ba_solves"] > 0
    assert runs["off"]["refused"] is not None and "depth is off" in runs["off"]["refused"]


SWEEP_RANGES = dict(step=(1, 16), num_hyp=(8, 256), patch_radius=(1, 4), min_texture=(0, 255), min_conf=(0, 255))


@pytest.fixture(scope="module")
def stream():
    import torch
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    return torch.from_numpy(np.stack([synth.plane_stream_frame(canvas, SPEED * k, W, H, f) for k in range(70)])).cuda()


@pytest.mark.parametrize("call", ["depthImage", "depthDense", "meshUpdate"])
def test_the_sweeps_ranges_at_the_session(stream, call):
    """the three session calls that sweep take the same five parameters with the same ranges: every value just outside a range is a bad
    argument and leaves the session as it was, every value just inside is swept with, and with depth off each call is refused by name"""
    from alvaar_amd.system import AlvaAR, AlvaError
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True)
    fed = [0]

    def feed():
        st = ar.find_camera_pose_device(int(stream[fed[0]].data_ptr()), 33.0 * fed[0])
        fed[0] += 1
        return st

    def ask(**kw):
        """-> whether the call swept"""
        if call == "depthImage":
            return ar.depthImage(**kw)[3]["status"] == 0
        if call == "depthDense":
            info = ar.depthDense(debug=True, **kw)[4]
            return info["status"] == 0 and info["did_sweep"] == 1
        return ar.meshUpdate(resolution=32, rel_extent=2.0, **kw)["status"] == 0

    while fed[0] < 40 and not (feed() == 1 and ar.depthImage(step=STEP)[3]["status"] == 0):
        pass
    assert ar.depthImage(step=STEP)[3]["status"] == 0
    for name, (lo, hi) in SWEEP_RANGES.items():
        for value in (lo - 1, hi + 1):
            with pytest.raises(AlvaError, match="not configured or bad argument"):
                ask(**{name: value})
        for value in (lo, hi):
            assert feed() == 1                        # (a frame of its own: a volume integrates a frame once)
            assert ask(**{name: value}), (name, value)
    ar.set_depth(False)
    with pytest.raises(AlvaError, match="depth is off"):
        ask()
    ar.set_depth(True)                                # the ring is empty again: answered, with nothing to sweep against
    assert not ask(step=STEP)
    ar.close()


def test_ring_fills_survives_lost_and_is_emptied_by_reset(runs):
    on = runs["on"]
    status = [r[0] for r in on["rec"]]
    sizes = [len(r) for r in on["rings"]]
    assert max(sizes) == 4 and all(s == 0 for s, st in zip(sizes, status[:on["first_ok"]]))
    for a, b, st in zip(on["rings"], on["rings"][1:], status[1:]):   # an entry joins as the newest or nothing changes
        assert np.array_equal(a, b) or (st == 1 and len(b) == min(len(a) + 1, 4) and np.array_equal(a[:3], b[1:]))
    lost = [k for k, st in enumerate(status) if st == 4]
    assert lost and status[lost[0] - 1] == 1
    for k in lost:   # LOST: the ring is what it was, and nothing is answered
        assert np.array_equal(on["rings"][k], on["rings"][lost[0] - 1]) and len(on["rings"][k]) == 4
    back = [k for k in range(lost[-1] + 1, len(status)) if status[k] == 1]
    assert back, status[lost[0]:]
    kept = {tuple(p) for p in on["rings"][lost[0] - 1]}
    assert kept & {tuple(p) for p in on["rings"][back[0]]}   # entries from before the loss are still there when tracking is back
    assert on["answers"][back[-1]][3]["status"] in (0, 7)
    n_before, n_after, (depth, conf, code, info) = on["after_reset"]
    assert n_before >= 1 and n_after == 0 and info["status"] == 6 and (code == 6).all()
