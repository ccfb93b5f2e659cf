"""Plane outlines (alva_plane_outlines / alva_system_detect_plane_outlines) on the GPU against the restatement tests/outline_cases.py.

Every comparison is exact -- the grid coordinates, the info rows, the outline's bytes and the area's bits: the outline is a set function
of the plane's points with exact predicates (double products in the written order, then integers), so there is nothing to leave a
margin for.  tests/test_outline_cases.py asserts on the CPU what each scene is meant to exercise."""
from __future__ import annotations

import numpy as np
import pytest

import outline_cases as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import alvaar_amd
    return alvaar_amd.Context(0)


def _gpu(ctx, P, labels, planes, max_vertices=64):
    import torch
    n = len(P)
    dp = torch.from_numpy(np.ascontiguousarray(P)).cuda() if n else torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    dl = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).cuda() if n else torch.zeros(0, dtype=torch.int32, device="cuda")
    return ctx.plane_outlines(dp, dl, planes, max_vertices=max_vertices, want_q=True)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want):
    """got = (outline, info, area, q) of the GPU, want = the restatement's dict: every byte"""
    outline, info, area, q = got
    print(info[:, :3].tolist(), want["info"][:, :3].tolist())
    assert np.array_equal(q, want["q"])
    assert np.array_equal(info, want["info"])
    assert outline.dtype == np.float32 and np.array_equal(_bytes(outline), _bytes(want["outline"]))
    assert area.dtype == np.float64 and np.array_equal(_bytes(area), _bytes(want["area"]))


@pytest.mark.parametrize("name", sorted(O.scenes()))
def test_scene_equals_the_restatement(ctx, name):
    s, want = O.scenes()[name], O.oracle_of(name)
    got = _gpu(ctx, s["P"], s["labels"], s["planes"], **s["kw"])
    _same(got, want)
    if name == "circle":
        assert got[1][0].tolist() == [0, 600, 600, 0, 0, 0, 0, 0]
    if name == "circle_64":
        assert got[1][0].tolist() == [3, 0, 600, 0, 0, 0, 0, 0] and not got[0].any() and not got[3].any() and got[2][0] == 0
    if name == "base_max8":
        assert got[1][:, 0].tolist() == [0, 0, 5, 5, 5, 5, 5, 5]
    if name in ("collinear", "identical"):
        assert got[1][0].tolist() == [2, 0, 40, 0, 0, 0, 0, 0]
    if name == "m2":
        assert got[1][0].tolist() == [1, 0, 2, 0, 0, 0, 0, 0]


def test_no_points_at_all(ctx):
    planes = O.scenes()["base_max8"]["planes"].copy()
    planes[1, 16:18] = 0
    outline, info, area, q = _gpu(ctx, np.zeros((0, 3)), np.zeros(0, np.int32), planes)
    assert info[:, 0].tolist() == [1, 4, 5, 5, 5, 5, 5, 5] and not info[:, 1:].any() and not outline.any() and not area.any() and not q.any()


def test_duplicating_every_point_changes_no_outline(ctx):
    s, d = O.scenes()["n513"], O.scenes()["duplicated"]
    a, b = _gpu(ctx, s["P"], s["labels"], s["planes"]), _gpu(ctx, d["P"], d["labels"], d["planes"])
    assert np.array_equal(_bytes(a[0]), _bytes(b[0])) and np.array_equal(_bytes(a[2]), _bytes(b[2])) and np.array_equal(a[3], b[3])
    assert b[1][0].tolist() == [0, a[1][0, 1], 2 * a[1][0, 2], 0, 0, 0, 0, 0]


@pytest.mark.parametrize("name", ["base", "circle", "n2049"])
def test_permuting_points_with_their_labels_changes_no_byte(ctx, name):
    s = O.scenes()[name]
    a = _gpu(ctx, s["P"], s["labels"], s["planes"], **s["kw"])
    perm = np.random.RandomState(11).permutation(len(s["P"]))
    b = _gpu(ctx, s["P"][perm], s["labels"][perm], s["planes"], **s["kw"])
    assert len(a) == 4 and all(np.array_equal(_bytes(x), _bytes(y)) for x, y in zip(a, b))
    _same(b, O.oracle_of(name))


def test_two_identical_calls_give_identical_bytes(ctx):
    s = O.scenes()["base"]
    a, b = _gpu(ctx, s["P"], s["labels"], s["planes"]), _gpu(ctx, s["P"], s["labels"], s["planes"])
    assert len(a) == 4 and all(np.array_equal(_bytes(x), _bytes(y)) for x, y in zip(a, b))
    assert a[1][:, :3].tolist() == [[0, 15, 1606], [0, 16, 897]]


def test_bad_arguments_are_rejected_and_the_context_stays_usable(ctx):
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    s = O.scenes()["base"]
    P, L = torch.from_numpy(s["P"]).cuda(), torch.from_numpy(s["labels"]).cuda()
    big_p = torch.zeros((O.N_CAP + 1, 3), dtype=torch.float64, device="cuda")
    big_l = torch.zeros(O.N_CAP + 1, dtype=torch.int32, device="cuda")
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.plane_outlines(big_p, big_l, s["planes"])
    for planes in (np.zeros((0, 24), np.float32), np.zeros((9, 24), np.float32)):
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.plane_outlines(P, L, planes)
    for mv in (7, 1025):
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.plane_outlines(P, L, s["planes"], max_vertices=mv)
    # null pointers, through the C entry point itself
    rec = np.ascontiguousarray(s["planes"])
    outline, info, area = np.zeros((2, 64, 2), np.float32), np.zeros((2, 8), np.int32), np.zeros(2)
    good = [ctx.h, P.data_ptr(), len(s["P"]), L.data_ptr(), 2, rec.ctypes.data, 64, outline.ctypes.data, None, info.ctypes.data, area.ctypes.data]
    for null in (0, 1, 3, 5, 7, 9, 10):
        args = list(good)
        args[null] = None
        assert capi.lib.alva_plane_outlines(*args) == -1, null
    assert not outline.any() and not info.any() and not area.any()
    assert capi.lib.alva_plane_outlines(*good) == 2   # the next good call is right
    want = O.oracle_of("base")
    assert np.array_equal(_bytes(outline), _bytes(want["outline"])) and np.array_equal(info, want["info"]) and np.array_equal(_bytes(area), _bytes(want["area"]))
    _same(_gpu(ctx, s["P"], s["labels"], s["planes"]), want)


# ---------------------------------------------------------------------------------------------------- the system surface
W, Hh, CELL = 640, 480, 12            # the stream and session set-up of tests/test_gpu_detect_planes.py
SPEED, N_TRACK, N_BLACK = 3, 110, 8
REL_THICKNESS = 3 * 0.00128905        # tests/test_gpu_detect_planes.py: REL_THICKNESS


@pytest.fixture(scope="module")
def sessions():
    """the same frames through two sessions: one calls detectPlanes and detectPlaneOutlines after every frame, the other never does"""
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
        rec, calls, detail, before, first_ok = [], [], None, None, None
        if name == "with":
            before = ar.detectPlaneOutlines(REL_THICKNESS)
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(dev[k].data_ptr()), 33.0 * k)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [int(v) for v in ar.state()]))
            if name == "with":
                plain = ar.detectPlanes(REL_THICKNESS)
                full = ar.detectPlaneOutlines(REL_THICKNESS)
                calls.append((st, plain, full))
                if st == 1 and first_ok is None:
                    first_ok = k
                if first_ok is not None and k == first_ok + 40 and st == 1:
                    ids, xyz, fl, _, _ = ar.map_points()
                    detail = dict(plain=plain, full=full, ids=ids.copy(), xyz=xyz.copy())
        out[name] = dict(rec=rec, calls=calls, detail=detail, before=before)
        ar.close()
    return out


def test_first_four_results_are_detect_planes_own(sessions):
    calls = sessions["with"]["calls"]
    assert sum(st == 1 for st, _, _ in calls) >= 40
    for k, (st, plain, full) in enumerate(calls):
        assert len(plain) == 4 and len(full) == 7
        assert all(np.array_equal(_bytes(a), _bytes(b)) for a, b in zip(plain, full[:4])), k


def test_system_outlines_equal_the_stage_and_the_restatement(ctx, sessions):
    d = sessions["with"]["detail"]
    assert d is not None
    planes, info, ids, labels, outlines, oinfo, areas = d["full"]
    row = {int(i): r for r, i in enumerate(d["ids"])}
    P = np.ascontiguousarray(d["xyz"][[row[int(i)] for i in ids]])
    assert len(P) >= 200 and len(labels) == len(P) and outlines.shape == (4, 64, 2)
    got = _gpu(ctx, P, labels, planes)
    assert np.array_equal(_bytes(outlines), _bytes(got[0])) and np.array_equal(oinfo, got[1]) and np.array_equal(_bytes(areas), _bytes(got[2]))
    _same(got, O.oracle(P, labels, planes))
    # which planes have an outline: those the detection found
    assert info[0, 0] == 0 and [c == 0 for c in oinfo[:, 0]] == [c == 0 for c in info[:, 0]] and (oinfo[info[:, 0] != 0, 0] == 5).all()
    # the stream's plane: at least a quadrilateral, inside the plane's rectangle grown by one cell, and not larger than it
    h, cell = oinfo[0, 1], float(max(planes[0, 16], planes[0, 17])) / 2.0 ** 20
    print("plane 0: %d vertices of %d points, area %.6g of the rectangle's %.6g" % (h, oinfo[0, 2], areas[0], float(planes[0, 16]) * float(planes[0, 17])))
    assert h >= 4 and oinfo[0, 2] == (labels == 0).sum()
    v = outlines[0, :h].astype(np.float64)
    assert (np.abs(v[:, 0]) <= float(planes[0, 16]) / 2 + cell).all() and (np.abs(v[:, 1]) <= float(planes[0, 17]) / 2 + cell).all()
    assert 0 < areas[0] <= (float(planes[0, 16]) + 2 * cell) * (float(planes[0, 17]) + 2 * cell)
    assert not outlines[0, h:].any()


def test_not_tracking_gives_code_6(sessions):
    s = sessions["with"]
    planes, info, ids, labels, outlines, oinfo, areas = s["before"]   # before the first frame
    assert (info[:, 0] == 6).all() and (oinfo[:, 0] == 6).all() and not oinfo[:, 1:].any() and not outlines.any() and not areas.any()
    assert not planes.any() and len(ids) == 0 and len(labels) == 0
    status = [st for st, _, _ in s["calls"]]
    assert 1 in status and 3 in status and 4 in status   # tracking, initialising, LOST
    for st, _, full in s["calls"]:
        if st == 1:
            assert (full[5][:, 0] != 6).all()
        else:
            assert (full[1][:, 0] == 6).all() and (full[5][:, 0] == 6).all() and not full[4].any() and not full[6].any()


def test_the_calls_leave_tracking_bitwise_unchanged(sessions):
    a, b = sessions["with"]["rec"], sessions["without"]["rec"]
    assert len(a) == len(b) and 1 in [r[0] for r in a] and 4 in [r[0] for r in a]
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0] == rb[0] and ra[3] == rb[3], k
        assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), k


def test_system_bad_arguments():
    import alvaar_amd
    from alvaar_amd.system import AlvaAR
    ar = AlvaAR(W, Hh, cell_size=CELL, random_sampling=False)
    try:
        for mv in (0, 7, 1025):
            with pytest.raises(alvaar_amd.AlvaError):
                ar.detectPlaneOutlines(REL_THICKNESS, max_vertices=mv)
        with pytest.raises(alvaar_amd.AlvaError):
            ar.detectPlaneOutlines(REL_THICKNESS, max_planes=9)
        assert (ar.detectPlaneOutlines(REL_THICKNESS)[5][:, 0] == 6).all()
    finally:
        ar.close()
