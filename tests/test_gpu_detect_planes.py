"""Plane detection (alva_detect_planes / alva_system_detect_planes) on the GPU against its numpy restatement tests/plane_cases.py.

Info and labels are compared exactly: both sides decide in float64 in the same operation order, and every compared case is asserted to
be >= 1e-7 (relative) away from each threshold decision and to pass the eigenvalue, sign, axis and facing guards of plane_cases.
Moments: the count is exact and |delta| <= 40 x count x 2^-53 x sum|terms| -- `count` double additions in another order, with the hit
test's 40x margin.  Planes: 1e-6 absolute -- float32 entries below 8 have a half-ulp of at most 2.4e-7, and the double error upstream
(moments, then an eigenvector with eigenvalue ratios >= 100 and >= 1.1) is <= 1e-9.

The system test's rel_thickness: REL_THICKNESS_MEASURED is the rank-90 % residual of the map's 3-D points about their least-squares
plane divided by D (the median depth of the frame's points), printed by the test on the GPU run: 0.00128905 on an MI355X;
REL_THICKNESS is the chosen value, 3 x that = 0.00386715."""
from __future__ import annotations

import numpy as np
import pytest

import hit_cases as H
import plane_cases as C

pytestmark = pytest.mark.gpu

REL_THICKNESS_MEASURED = 0.00128905   # map points 2559, frame points 1726, D = 13.8323 at the compared frame
REL_THICKNESS = 3 * REL_THICKNESS_MEASURED


@pytest.fixture(scope="module")
def ctx():
    import alvaar_amd
    return alvaar_amd.Context(0)


def _gpu(ctx, case, P=None, **over):
    import torch
    P = case["P"] if P is None else P
    dev = torch.from_numpy(P).cuda() if len(P) else torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    return ctx.detect_planes(dev, case["pose7"], want_labels=True, want_moments=True, **dict(case["kw"], **over))


def _same_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def _compare(got, r):
    planes, info, labels, mom = got
    print(info[:, :5].tolist(), r["info"][:, :5].tolist(), C.margins_text(r))
    assert r["thr_margin"] >= C.MARGIN_MIN
    assert np.array_equal(info, r["info"])
    assert np.array_equal(labels, r["labels"])
    for k in range(len(info)):
        if info[k, 0] in (0, 4):
            delta, count = np.abs(mom[k] - r["moments"][k]), r["moments"][k][0]
            print("  moments: max |delta| / sum|terms| =", float((delta / np.maximum(r["moment_scale"][k], 1e-300)).max()))
            assert mom[k][0] == count and (delta <= 40 * count * 2.0 ** -53 * r["moment_scale"][k]).all(), (k, delta)
        else:
            assert not mom[k].any()
        if info[k, 0] == 0:
            print("  plane: max |delta| =", float(np.abs(planes[k].astype(np.float64) - r["planes"][k]).max()))
            assert np.abs(planes[k].astype(np.float64) - r["planes"][k].astype(np.float64)).max() <= 1e-6, k
            assert planes[k, 15] == 1 and not planes[k, [3, 7, 11]].any() and not planes[k, 19:].any()
        else:
            assert not planes[k].any(), k   # a plane is written only for code 0
    assert C.margins_ok(r), C.margins_text(r)   # the guards (last, so that a failure here says that all of the above held)


@pytest.mark.parametrize("name", sorted(C.edge_cases()))
def test_edge_case_equals_the_oracle(ctx, name):
    case, want = C.edge_cases()[name], C.oracle_of(name)
    assert want["info"][:, 0].tolist() == case["want"]
    got = _gpu(ctx, case)
    if name == "base_max1":
        wall = C.oracle_of("base")["labels"] == 1
        assert (got[2][wall] == -1).all() and wall.sum() == 897
    if name == "base_max8":
        assert got[1][3:].tolist() == [C.NOT_RUN] * 5
    if name == "exact_plane":
        assert got[1][0].tolist() == [0, 192, 0, 192, 192, 0, 0, 0] and got[3][0][3] == 0 and got[3][0][9] == 0
        assert got[0][0, 16] == np.float32(15 / 64) and got[0][0, 17] == np.float32(11 / 64) and got[0][0, 4:7].tolist() == [0, 0, -1]
    if name == "tie":
        assert got[1][0, 2] == 0 and got[1][1, 2] == 0
    if name == "code4":
        assert got[1][0].tolist() == [4, 11, 0, 11, 10, 0, 0, 0] and (got[2] == -1).all()
    _compare(got, want)


def test_one_point_more_than_the_bound_is_rejected(ctx):
    import torch
    import alvaar_amd
    P = torch.zeros((C.N_CAP + 1, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.detect_planes(P, H.POSE_BASE, 0.01)
    planes, info = ctx.detect_planes(P[:C.N_CAP], H.POSE_BASE, 0.01, num_iterations=2, max_planes=1)   # all at one point: no hypothesis
    assert info[0].tolist() == [2, C.N_CAP, -1, 0, 0, 0, 0, 0] and not planes.any()


def test_two_identical_calls_give_identical_bytes(ctx):
    case = C.edge_cases()["base"]
    a, b = _gpu(ctx, case), _gpu(ctx, case)
    assert len(a) == 4 and _same_bytes(a, b)
    assert a[1][:, 0].tolist() == [0, 0, 3, 5]


def test_max_planes_2_is_the_prefix_of_max_planes_4(ctx):
    case = C.edge_cases()["base"]
    a, b = _gpu(ctx, case), _gpu(ctx, case, max_planes=2)
    assert b[1][:, 0].tolist() == [0, 0]
    assert _same_bytes([a[0][:2], a[1][:2], a[2], a[3][:2]], b)


def test_permuting_the_unlabelled_points_changes_no_record_bit(ctx):
    case = C.edge_cases()["base"]
    a = _gpu(ctx, case)
    rest = np.nonzero(a[2] == -1)[0]
    assert len(rest) == 2800 - 1606 - 897
    P = case["P"].copy()
    P[rest] = P[np.random.RandomState(5).permutation(rest)]   # the same positions in the array, as a set
    assert not np.array_equal(P, case["P"])
    b = _gpu(ctx, case, P=P)
    # the records: every bit.  (Round 2's info is a best count over hypotheses that index the permuted points.  The test-only moments
    # are sums over the consensus set in live order, and a consensus point outside the final set stays unlabelled and has moved -- round
    # 1 counts 898 and keeps 897 --, so they are held to the reordering bound, not to the bit)
    assert _same_bytes([a[0], a[1][:2]], [b[0], b[1][:2]])
    assert np.array_equal(a[2], b[2])                                      # the labelled points did not move
    want = C.oracle_of("base")
    for k in range(2):
        print(k, np.abs(a[3][k] - b[3][k]).max())
        assert a[3][k][0] == b[3][k][0] and (np.abs(a[3][k] - b[3][k]) <= 40 * a[3][k][0] * 2.0 ** -53 * want["moment_scale"][k]).all()
    assert not a[3][2:].any() and not b[3][2:].any()


def test_bad_arguments_are_rejected(ctx):
    import torch
    import alvaar_amd
    case = C.edge_cases()["base"]
    P = torch.from_numpy(case["P"]).cuda()
    for kw in (dict(thickness=0.0), dict(thickness=-1.0), dict(thickness=float("inf")), dict(thickness=float("nan")), dict(min_inliers=7),
               dict(min_inliers=C.N_CAP + 1), dict(max_planes=0), dict(max_planes=9), dict(num_iterations=0), dict(num_iterations=4097)):
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.detect_planes(P, case["pose7"], **dict(dict(thickness=0.01), **kw))
    planes, info = ctx.detect_planes(P, case["pose7"], **case["kw"])   # and the context is as good as before
    assert info[:, 0].tolist() == [0, 0, 3, 5] and info[0, 4] == 1606 and info[1, 4] == 897


# ---------------------------------------------------------------------------------------------------- the system surface
W, Hh, CELL = 640, 480, 12            # the stream of tests/test_gpu_hit_test.py
SPEED, N_TRACK, N_BLACK = 3, 110, 8
TAPS = np.array([(320, 240), (200, 150), (440, 330), (160, 360), (480, 120)], np.float32)


@pytest.fixture(scope="module")
def sessions():
    """the same frames through two sessions: one calls detectPlanes after every frame, the other never does"""
    import torch
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    f = sysdiff.intrinsics(W, Hh)[0]
    canvas = synth.texture_canvas(W, Hh, 5)
    frames = [synth.plane_stream_frame(canvas, SPEED * k, W, Hh, f) for k in range(N_TRACK)]
    frames += [np.zeros((Hh, W, 4), np.uint8) + np.array([0, 0, 0, 255], np.uint8)] * N_BLACK
    dev = torch.from_numpy(np.stack(frames)).cuda()
    rel = REL_THICKNESS
    out = {}
    for name in ("with", "without"):
        ar = AlvaAR(W, Hh, cell_size=CELL, random_sampling=False, relocalization=True)
        rec, found, detail, before, first_ok = [], [], None, None, None
        if name == "with":
            before = ar.detectPlanes(rel)
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(dev[k].data_ptr()), 33.0 * k)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [int(v) for v in ar.state()]))
            if name == "with":
                res = ar.detectPlanes(rel)
                found.append((res[0].copy(), res[1].copy()))
                if st == 1 and first_ok is None:
                    first_ok = k
                if first_ok is not None and k == first_ok + 40 and st == 1:
                    ids, xyz, fl, _, _ = ar.map_points()
                    detail = dict(frame=k, first=res, second=ar.detectPlanes(rel), hits=ar.hitTest(TAPS), order=ar.frame_map_point_ids().copy(),
                                  ids=ids.copy(), xyz=xyz.copy(), flags=fl.copy(), pose7=ar.pose7()[0].copy(), rel=rel)
        out[name] = dict(rec=rec, found=found, detail=detail, before=before)
        ar.close()
    return out


def test_system_detect_planes_equals_the_stage_and_the_oracle(ctx, sessions):
    import torch
    d = sessions["with"]["detail"]
    assert d is not None
    planes, info, ids, labels = d["first"]
    assert _same_bytes(d["first"], d["second"])   # two identical calls
    # the points: every 3-D point of the map, in ascending id
    want_ids = d["ids"][d["flags"][:, 0] == 1][-C.N_CAP:]
    assert np.array_equal(ids, want_ids) and len(ids) >= 200 and len(labels) == len(ids)
    row = {int(i): r for r, i in enumerate(d["ids"])}
    P = np.ascontiguousarray(d["xyz"][[row[int(i)] for i in ids]])
    # D: the rank n / 2 camera-frame depth of the frame's observed 3-D points
    seen = d["xyz"][[row[int(i)] for i in d["order"]]]
    t, R = d["pose7"][:3], H.quat_to_rot(d["pose7"][3:])
    dd = seen - t
    depth = (R[0, 2] * dd[:, 0] + R[1, 2] * dd[:, 1]) + R[2, 2] * dd[:, 2]
    D = np.partition(depth, len(depth) // 2)[len(depth) // 2]
    # the figure REL_THICKNESS comes from: rank-90 % residual about the least-squares plane of the map's points, over D
    c = P.mean(axis=0)
    nrm = np.linalg.eigh(np.cov((P - c).T))[1][:, 0]
    res = np.sort(np.abs((P - c) @ nrm))
    measured = res[int(0.9 * len(res))] / D
    print("map points %d, frame points %d, D = %.6g, rank-90%% residual / D = %.6g, rel_thickness used = %.6g" % (len(P), len(seen), D, measured, d["rel"]))
    assert abs(measured / REL_THICKNESS_MEASURED - 1) < 0.05   # the figure REL_THICKNESS was derived from still describes this stream
    thickness = np.float64(d["rel"]) * D
    got = ctx.detect_planes(torch.from_numpy(P).cuda(), d["pose7"], thickness, 48, 4, 128, seed=12345, want_labels=True, want_moments=True)
    assert _same_bytes([planes, info, labels], got[:3])
    _compare(got, C.oracle(P, d["pose7"], thickness, 48, 4, 128, 12345))
    # the stream is one fronto-parallel textured plane: the first plane is it
    assert info[0, 0] == 0 and (labels == 0).sum() >= len(P) / 2
    poses, hinfo = d["hits"]
    normals = poses[hinfo[:, 0] == 0][:, 4:7]
    assert len(normals) >= 3 and (np.abs(normals @ planes[0, 4:7]) > 0.99).all()


def test_detect_planes_leaves_tracking_bitwise_unchanged(sessions):
    a, b = sessions["with"]["rec"], sessions["without"]["rec"]
    assert len(a) == len(b) and 1 in [r[0] for r in a] and 4 in [r[0] for r in a]
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0] == rb[0] and ra[3] == rb[3], k
        assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), k


def test_not_tracking_gives_code_6(sessions):
    s = sessions["with"]
    planes, info, ids, labels = s["before"]   # before the first frame
    assert (info[:, 0] == 6).all() and not planes.any() and len(ids) == 0 and len(labels) == 0
    status = [r[0] for r in s["rec"]]
    assert 3 in status and 4 in status
    for st, (planes, info) in zip(status, s["found"]):
        if st == 1:
            assert (info[:, 0] != 6).all()
        else:   # initialising (3), LOST (4)
            assert (info[:, 0] == 6).all() and (info[:, 2] == -1).all() and not planes.any()
