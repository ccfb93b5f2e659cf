"""The hit test (alva_hit_test / alva_system_hit_test) on the GPU against its numpy restatement tests/hit_cases.py.

Discrete outputs (code, m, best_it, n_in, the count before the cap) are compared exactly: both sides decide in float64 in the same
operation order, and every compared case is asserted to be >= 1e-7 (relative) away from each decision that a last bit could flip.
Moments: |delta| <= 1e-11 x sum|terms| -- at most 2048 double additions in another order give 2048 x 1.1e-16 x sum|terms| = 2.3e-13 x
sum|terms|; the tolerance is that with a 40x margin.  Poses: 1e-6 absolute -- float32 entries below 8 have a half-ulp of at most 2.4e-7
and the double error upstream is <= 1e-9 given the moments bound and an eigenvalue ratio >= 100, which the oracle asserts."""
from __future__ import annotations

import numpy as np
import pytest

import hit_cases as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import alvaar_amd
    return alvaar_amd.Context(0)


def _gpu(ctx, case, taps=None):
    import torch
    taps = case["taps"] if taps is None else taps
    radii = {r for _, r in taps}
    assert len(radii) == 1
    P = torch.from_numpy(case["P"]).cuda() if len(case["P"]) else torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    return ctx.hit_test(P, case["pose7"], case["calib8"], [uv for uv, _ in taps], radius_px=radii.pop(), want_moments=True, **case["kw"])


def _compare(got, want_list):
    poses, info, mom = got
    for k, r in enumerate(want_list):
        print(H.info_of(r), info[k].tolist(), r["sel_margin"], r["gap_margin"], r["thr_margin"], r["eig_ratio"])
        assert H.margins_ok(r), k
        assert info[k].tolist() == H.info_of(r), k
        if r["code"] in (0, 3, 4):
            delta = np.abs(mom[k] - r["moments"])
            print("  moments: max |delta| / sum|terms| =", float((delta / np.maximum(r["moment_scale"], 1e-300)).max()))
            assert mom[k][0] == r["moments"][0] and (delta <= 1e-11 * r["moment_scale"]).all(), (k, delta)
        else:
            assert not mom[k].any()
        if r["code"] == 0:
            print("  pose: max |delta| =", float(np.abs(poses[k].astype(np.float64) - r["pose"]).max()))
            assert np.abs(poses[k].astype(np.float64) - r["pose"].astype(np.float64)).max() <= 1e-6, k
        else:
            assert not poses[k].any(), k   # a pose is written only for code 0


def _base_case():
    return dict(P=H.base_scene(), pose7=H.POSE_BASE, calib8=H.K_BASE, taps=H.BASE_TAPS, kw={})


def test_base_taps_one_call_equals_five_calls_equals_the_oracle(ctx):
    case = _base_case()
    want = H.oracle_case(case)
    assert [r["code"] for r in want] == [0, 0, 0, 1, 0] and [r["m"] for r in want] == [44, 46, 50, 7, 31]
    r40 = [t for t in case["taps"] if t[1] == 40.0]
    together = _gpu(ctx, case, r40)
    single = [_gpu(ctx, case, [t]) for t in case["taps"]]
    for k in range(len(r40)):   # the four radius-40 taps as one call and one by one: the same bits
        for a, b in zip(together, single[k]):
            assert np.array_equal(a[k].view(np.uint8), b[0].view(np.uint8)), k
    _compare(tuple(np.concatenate([s[j] for s in single]) for j in range(3)), want)
    # five rays in one launch (the radius is per call: the fifth tap is compared at 40 too) against five launches
    five = [(uv, 40.0) for uv, _ in case["taps"]]
    a = _gpu(ctx, case, five)
    b = [_gpu(ctx, case, [t]) for t in five]
    for j in range(3):
        assert np.array_equal(a[j].view(np.uint8), np.concatenate([x[j] for x in b]).view(np.uint8))
    assert a[0][1, 4] < -0.999   # the wall: normal ~ (-1, 0, 0)


@pytest.mark.parametrize("name", sorted(H.edge_cases()))
def test_edge_case_equals_the_oracle(ctx, name):
    case = H.edge_cases()[name]
    want = H.oracle_case(case)
    if case["want"] is not None:
        assert [r["code"] for r in want] == case["want"]
    got = _gpu(ctx, case)
    _compare(got, want)
    if name == "rays16":
        one = [_gpu(ctx, case, [t]) for t in case["taps"]]
        for j in range(3):
            assert np.array_equal(got[j].view(np.uint8), np.concatenate([x[j] for x in one]).view(np.uint8))
    if name == "cap5000":
        assert got[1][0, 4] == 5000 and got[1][0, 1] == 2048
        first = dict(case, P=case["P"][:2048])   # the first 2048 in index order, and nothing else
        again = _gpu(ctx, first)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[2], got[2]) and again[1][0, :4].tolist() == got[1][0, :4].tolist()
    if name == "exact_plane":
        assert got[1][0, 3] == got[1][0, 1] == 192 and got[2][0, 3] == 0 and got[2][0, 9] == 0
        assert got[0][0, 4:7].tolist() == [0, 0, -1]


def test_the_ray_is_the_undistorted_tap(ctx):
    import torch
    case = H.edge_cases()["distorted"]
    taps = np.array([uv for uv, _ in case["taps"]], np.float32)
    und = ctx.undistort_points(torch.from_numpy(taps).cuda(), case["calib8"][:4], case["calib8"][4:]).cpu().numpy()
    poses, info, _ = _gpu(ctx, case)
    t, R = case["pose7"][:3], H.quat_to_rot(case["pose7"][3:])
    for k in range(len(taps)):
        assert tuple(und[k]) == H.undistort(case["calib8"], *taps[k])       # the restatement is alva_undistort_points, bitwise
        assert np.abs(und[k] - taps[k]).max() > 0.05                         # and the distortion moves the tap
        dc = np.array([(und[k][0] - case["calib8"][2]) / case["calib8"][0], (und[k][1] - case["calib8"][3]) / case["calib8"][1], 1.0])
        dw = R @ (dc / np.linalg.norm(dc))
        along = poses[k][12:15].astype(np.float64) - t
        assert info[k][0] == 0 and np.linalg.norm(np.cross(along, dw)) <= 2e-6 * max(1.0, np.linalg.norm(along))


def test_bad_arguments_are_rejected(ctx):
    import torch
    import alvaar_amd
    case = _base_case()
    P = torch.from_numpy(case["P"]).cuda()
    tap = [(250.0, 240.0)]
    for kw in (dict(uv=np.zeros((0, 2))), dict(uv=[(1.0, 1.0)] * 17), dict(uv=tap, num_iterations=0), dict(uv=tap, num_iterations=4097),
               dict(uv=tap, radius_px=0.0), dict(uv=tap, radius_px=-3.0)):
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.hit_test(P, case["pose7"], case["calib8"], **kw)
    poses, info = ctx.hit_test(P, case["pose7"], case["calib8"], tap)   # and the context is as good as before
    assert info[0, 0] == 0 and info[0, 1] == 44


def test_permuting_the_unselected_points_changes_no_bit(ctx):
    case = _base_case()
    taps = [t for t in case["taps"] if t[1] == 40.0][:3]
    a = _gpu(ctx, case, taps)
    sel = np.unique(np.concatenate([H.oracle(case["P"], case["pose7"], case["calib8"], uv, r)["sel"] for uv, r in taps]))
    rest = np.setdiff1d(np.arange(len(case["P"])), sel)
    P = case["P"].copy()
    P[rest] = P[np.random.RandomState(5).permutation(rest)]
    assert not np.array_equal(P, case["P"])
    b = _gpu(ctx, dict(case, P=P), taps)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ---------------------------------------------------------------------------------------------------- the system surface
W, Hh, CELL = 640, 480, 12            # the stream of tests/test_gpu_relocalization.py
SPEED, N_TRACK, N_BLACK = 3, 110, 8
TAPS = np.array([(320, 240), (200, 150), (440, 330), (160, 360), (480, 120)], np.float32)


@pytest.fixture(scope="module")
def sessions():
    """the same frames through two sessions: one calls hitTest after every frame, the other never does"""
    import torch
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    f = sysdiff.intrinsics(W, Hh)[0]
    canvas = synth.texture_canvas(W, Hh, 5)
    frames = [synth.plane_stream_frame(canvas, SPEED * k, W, Hh, f) for k in range(N_TRACK)]
    frames += [np.zeros((Hh, W, 4), np.uint8) + np.array([0, 0, 0, 255], np.uint8)] * N_BLACK
    dev = torch.from_numpy(np.stack(frames)).cuda()
    out = {}
    for name in ("with", "without"):
        ar = AlvaAR(W, Hh, cell_size=CELL, random_sampling=False, relocalization=True)
        rec, hits, detail = [], [], None
        if name == "with":
            before = ar.hitTest(TAPS)
        first_ok = None
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(dev[k].data_ptr()), 33.0 * k)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [int(v) for v in ar.state()]))
            if name == "with":
                hits.append(ar.hitTest(TAPS))
                if st == 1 and first_ok is None:
                    first_ok = k
                if first_ok is not None and k == first_ok + 40 and st == 1:
                    ids, xyz, fl, _, _ = ar.map_points()
                    detail = dict(frame=k, first=hits[-1], second=ar.hitTest(TAPS), order=ar.frame_map_point_ids().copy(), ids=ids.copy(),
                                  xyz=xyz.copy(), flags=fl.copy(), pose7=ar.pose7()[0].copy(), k=dict(ar.intrinsics))
        out[name] = dict(rec=rec, hits=hits, detail=detail, before=before if name == "with" else None)
        ar.close()
    return out


def test_system_hit_test_equals_the_stage_and_the_oracle(ctx, sessions):
    import torch
    d = sessions["with"]["detail"]
    assert d is not None
    # the frame's observed 3-D points in the map container's order
    want_ids = d["ids"][(d["flags"][:, 0] == 1) & (d["flags"][:, 1] == 1)]
    assert sorted(d["order"].tolist()) == sorted(want_ids.tolist()) and len(d["order"]) >= 200
    row = {int(i): r for r, i in enumerate(d["ids"])}
    P = np.ascontiguousarray(d["xyz"][[row[int(i)] for i in d["order"]]])
    k = d["k"]
    calib8 = (k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"])
    poses, info = d["first"]
    for a, b in zip(d["first"], d["second"]):   # two identical calls
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    got = ctx.hit_test(torch.from_numpy(P).cuda(), d["pose7"], calib8, TAPS, radius_px=40, num_iterations=64, seed=12345, want_moments=True)
    assert np.array_equal(got[0].view(np.uint8), poses.view(np.uint8)) and np.array_equal(got[1], info)
    want = [H.oracle(P, d["pose7"], calib8, uv, 40.0, 64, 12345) for uv in TAPS]
    _compare(got, want)
    assert (info[:, 0] == 0).sum() >= 3, info[:, 0]
    # the stream is a fronto-parallel textured plane: the anchors' normals agree with one another
    normals = poses[info[:, 0] == 0][:, 4:7]
    assert (np.abs(normals @ normals[0]) > 0.99).all()


def test_hit_test_leaves_tracking_bitwise_unchanged(sessions):
    a, b = sessions["with"]["rec"], sessions["without"]["rec"]
    assert len(a) == len(b) and 1 in [r[0] for r in a] and 4 in [r[0] for r in a]
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0] == rb[0] and ra[3] == rb[3], k
        assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), k


def test_not_tracking_gives_code_5(sessions):
    s = sessions["with"]
    poses, info = s["before"]   # before the first frame
    assert (info[:, 0] == 5).all() and not poses.any()
    status = [r[0] for r in s["rec"]]
    assert 3 in status and 4 in status
    for st, (poses, info) in zip(status, s["hits"]):
        if st == 1:
            assert (info[:, 0] != 5).all()
        else:   # initialising (3), LOST (4)
            assert (info[:, 0] == 5).all() and not poses.any()
