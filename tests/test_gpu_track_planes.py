"""Plane tracking (alva_track_planes / alva_system_track_planes) on the GPU against its numpy restatement tests/track_cases.py.

The comparison rules are those of tests/test_gpu_detect_planes.py: info and labels exactly (both sides decide in float64 in the same
operation order, and every compared case is asserted to be >= 1e-7 away from each threshold and each tie decision and to pass
plane_cases' five guards); moments: the count exactly and |delta| <= 40 x count x 2^-53 x sum|terms|; records: 1e-6 absolute, and zero
where no plane was written.

The system test runs the stream and the two sessions of tests/test_gpu_detect_planes.py; one session calls trackPlanes after every
frame.  Every call is replayed through Context.track_planes (same bytes) with the priors that a Python restatement of
csrc/slam/plane_tracks.hpp keeps; every tenth call, and the first three, also through oracle_track.

Measured on an MI355X: the floor is found at frame 6, the first tracked frame, and keeps id 0 in every later status-1 call; frames 110 to
112 (the first black ones) still return status 1 but see no 3-D point, so they are answered with code 6 like the LOST frames after them;
every replayed call passed the restatement's margins."""
from __future__ import annotations

import numpy as np
import pytest

import hit_cases as H
import plane_cases as C
import track_cases as T

pytestmark = pytest.mark.gpu

REL_THICKNESS = 3 * 0.00128905   # tests/test_gpu_detect_planes.py: REL_THICKNESS
COS_MERGE = 0.98480775301220802  # plane_tracks.hpp: cos 10 deg


@pytest.fixture(scope="module")
def ctx():
    import alvaar_amd
    return alvaar_amd.Context(0)


def _dev(P):
    import torch
    return torch.from_numpy(np.ascontiguousarray(P)).cuda() if len(P) else torch.zeros((0, 3), dtype=torch.float64, device="cuda")


def _gpu(ctx, case, prior="case", **over):
    prior = case["prior"] if isinstance(prior, str) else prior
    return ctx.track_planes(_dev(case["P"]), case["pose7"], prior24=prior, want_labels=True, want_moments=True, **dict(case["kw"], **over))


def _same_bytes(a, b):
    return len(a) == len(b) and all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
                                    for x, y in zip(a, b))


def _compare(got, r, n_prior, t1_exact_tie=False):
    planes, info, labels, mom = got
    print(info[:, :6].tolist(), r["info"][:, :6].tolist(), T.margins_text(r))
    assert r["thr_margin"] >= T.MARGIN_MIN and r["tie_margin_t4"] >= T.MARGIN_MIN
    assert r["tie_margin_t1"] == 0 if t1_exact_tie else r["tie_margin_t1"] >= T.MARGIN_MIN
    assert np.array_equal(info, r["info"])
    assert np.array_equal(labels, r["labels"])
    for k in range(len(info)):
        if info[k, 0] in ((0, 8) if k < n_prior else (0, 4)):   # the refit ran
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
    assert T.margins_ok(r, t1_exact_tie), T.margins_text(r)   # the guards (last, so that a failure here says that all of the above held)


@pytest.mark.parametrize("name", sorted(T.cases()))
def test_scene_equals_the_restatement(ctx, name):
    case, want = T.cases()[name], T.oracle_of(name)
    assert want["info"][:, 0].tolist() == case["want"]
    got = _gpu(ctx, case)
    if name == "exact_tie":
        assert got[1][:, 3:5].tolist() == [[96, 96], [48, 48]] and (got[2][:96] == 0).all() and (got[2][96:] == 1).all()
        assert got[0][0, 14] == np.float32(4.0625) and got[0][1, 14] == np.float32(4.25)
    if name == "code8":
        assert got[1].tolist() == [[8, 11, -1, 11, 10, 1, 0, 0], [4, 11, 0, 11, 10, 0, 0, 0]] and (got[2] == -1).all()
    if name == "swapped":
        assert got[1][:2, 3:5].tolist() == [[899, 899], [1604, 1604]]
    _compare(got, want, len(case["prior"]), case["t1_exact_tie"])


@pytest.mark.parametrize("name", ["base", "tie", "n2049"])
def test_without_priors_the_bytes_are_detect_planes(ctx, name):
    case = C.edge_cases()[name]
    dev = _dev(case["P"])
    a = ctx.detect_planes(dev, case["pose7"], want_labels=True, want_moments=True, **case["kw"])
    b = ctx.track_planes(dev, case["pose7"], prior24=None, want_labels=True, want_moments=True, **case["kw"])
    c = ctx.track_planes(dev, case["pose7"], prior24=np.zeros((0, 24), np.float32), want_labels=True, want_moments=True, **case["kw"])
    assert len(a) == 4 and _same_bytes(a, b) and _same_bytes(a, c)
    assert a[1][:, 0].tolist() == case["want"]


def test_two_identical_calls_give_identical_bytes(ctx):
    for name in ("self_base", "grow", "stack8"):
        case = T.cases()[name]
        a, b = _gpu(ctx, case), _gpu(ctx, case)
        assert len(a) == 4 and _same_bytes(a, b), name
        assert a[1][:, 0].tolist() == case["want"]


def test_bad_arguments_are_rejected(ctx):
    import torch
    import alvaar_amd
    case = T.cases()["self_base"]
    big = torch.zeros((C.N_CAP + 1, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(alvaar_amd.AlvaError):   # one point more than the bound
        ctx.track_planes(big, case["pose7"], 0.01, prior24=case["prior"])
    assert _gpu(ctx, case)[1][:, 0].tolist() == [0, 0, 3, 5]       # the context is as good as before
    with pytest.raises(alvaar_amd.AlvaError):   # more priors than slots
        _gpu(ctx, case, max_planes=1)
    with pytest.raises(alvaar_amd.AlvaError):
        _gpu(ctx, case, prior=np.tile(case["prior"], (5, 1))[:9], max_planes=8)
    got = _gpu(ctx, case)
    assert got[1][:, 0].tolist() == [0, 0, 3, 5] and got[1][:2, 4].tolist() == [1604, 899]
    P = _dev(case["P"])
    for kw in (dict(thickness=0.0), dict(thickness=float("nan")), dict(min_inliers=7), dict(max_planes=9), dict(num_iterations=0),
               dict(num_iterations=4097)):
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.track_planes(P, case["pose7"], prior24=case["prior"], **dict(dict(thickness=0.01), **kw))
    assert _same_bytes(_gpu(ctx, case), got)


def test_chaining_self_base_is_a_fixed_point_of_what_is_counted(ctx):
    """self_base, then again with its own kept records as priors: the same codes, counts and labels, records within 1e-6"""
    case = T.cases()["self_base"]
    a = _gpu(ctx, case)
    prior = a[0][a[1][:, 0] == 0]
    assert len(prior) == 2
    b = _gpu(ctx, case, prior=prior)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.abs(a[0].astype(np.float64) - b[0]).max() <= 1e-6
    _compare(b, T.oracle_track(case["P"], case["pose7"], prior, **case["kw"]), 2)


# ---------------------------------------------------------------------------------------------------- the system surface
W, Hh, CELL = 640, 480, 12            # the stream and session set-up of tests/test_gpu_detect_planes.py
SPEED, N_TRACK, N_BLACK = 3, 110, 8
KW = dict(min_inliers=48, max_planes=4, num_iterations=128)


class Tracks:
    """csrc/slam/plane_tracks.hpp, restated: [(record, id, age)] in ascending id"""

    def __init__(self):
        self.list, self.next_id = [], 0

    def priors(self):
        return np.array([t[0] for t in self.list], np.float32).reshape(-1, 24)

    def apply(self, planes, info, thickness):
        n_prior, alive = len(self.list), []
        ids, merged = np.full(len(info), -1, np.int32), np.full(len(info), -1, np.int32)
        for s in range(len(info)):
            if info[s, 0] != 0:
                continue
            if s < n_prior:
                alive.append([s, planes[s].copy(), self.list[s][1], self.list[s][2] + 1, False])
            else:
                alive.append([s, planes[s].copy(), self.next_id, 0, False])
                self.next_id += 1
            ids[s] = alive[-1][2]
        dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
        for b in range(1, len(alive)):
            rb = alive[b][1].astype(np.float64)
            for a in range(b):
                ra = alive[a][1].astype(np.float64)
                if not alive[a][4] and abs(dot(ra[4:7], rb[4:7])) >= COS_MERGE and abs(dot(ra[4:7], rb[12:15] - ra[12:15])) <= thickness and \
                        abs(dot(rb[4:7], ra[12:15] - rb[12:15])) <= thickness:
                    alive[b][4], merged[alive[b][0]] = True, alive[a][2]
                    break
        self.list = [(t[1], t[2], t[3]) for t in alive if not t[4]]
        return ids, merged


@pytest.fixture(scope="module")
def sessions():
    """the same frames through two sessions: one calls trackPlanes after every frame (twice at one frame, the second time with outlines;
    at the last tracked frame once more after resetPlanes, then after another resetPlanes with outlines, next to detectPlaneOutlines),
    the other never does"""
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
        rec, calls, first_ok, fresh_detect = [], [], None, None

        def call(k, st, what, **kw):
            res = ar.trackPlanes(REL_THICKNESS, **kw)
            d = dict(frame=k, status=st, what=what, res=tuple(np.copy(x) for x in res))
            if st == 1:
                ids, xyz, fl, _, _ = ar.map_points()
                d.update(order=ar.frame_map_point_ids().copy(), ids=ids.copy(), xyz=xyz.copy(), flags=fl.copy(), pose7=ar.pose7()[0].copy())
            calls.append(d)

        if name == "with":
            call(-1, 0, "before")
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(dev[k].data_ptr()), 33.0 * k)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [int(v) for v in ar.state()]))
            if name == "with":
                call(k, st, "frame")
                if st == 1 and first_ok is None:
                    first_ok = k
                if first_ok is not None and k == first_ok + 40 and st == 1:
                    call(k, st, "outlines", max_vertices=64)
                if k == N_TRACK - 1 and st == 1:
                    ar.resetPlanes()
                    call(k, st, "reset")
                    ar.resetPlanes()
                    call(k, st, "fresh", max_vertices=64)
                    fresh_detect = tuple(np.copy(x) for x in ar.detectPlaneOutlines(REL_THICKNESS, max_vertices=64, **KW))
        out[name] = dict(rec=rec, calls=calls, fresh_detect=fresh_detect)
        ar.close()
    return out


def _inputs(d):
    """the stage's inputs at a recorded call, as alva_system_track_planes derives them: points in ascending id, thickness = rel x D"""
    ids = d["ids"][d["flags"][:, 0] == 1][-C.N_CAP:]
    row = {int(i): r for r, i in enumerate(d["ids"])}
    P = np.ascontiguousarray(d["xyz"][[row[int(i)] for i in ids]])
    seen = d["xyz"][[row[int(i)] for i in d["order"]]]
    t, R = d["pose7"][:3], H.quat_to_rot(d["pose7"][3:])
    dd = seen - t
    depth = (R[0, 2] * dd[:, 0] + R[1, 2] * dd[:, 1]) + R[2, 2] * dd[:, 2]
    D = np.partition(depth, len(depth) // 2)[len(depth) // 2]
    return ids, P, np.float64(REL_THICKNESS) * D


@pytest.fixture(scope="module")
def replay(ctx, sessions):
    """every status-1 call replayed through Context.track_planes with the priors that the restated PlaneTracks keeps: a list of
    dict(call, ids, P, thickness, prior, stage = (planes, info, labels), plane_ids, merged) -- and the asserts that need no oracle"""
    import torch
    tracks, out = Tracks(), []
    for d in sessions["with"]["calls"]:
        planes, info, pids, merged, ids, labels = d["res"][:6]
        if d["status"] != 1 or len(d["order"]) == 0:   # not tracking, or a frame that sees no 3-D point (no depth to scale the slab by):
            print("code 6 at frame", d["frame"], "status", d["status"])   # nothing runs, and the list stays as it is
            assert (info[:, 0] == 6).all() and (info[:, 2] == -1).all() and not planes.any() and (pids == -1).all() and (merged == -1).all()
            assert len(ids) == 0 and len(labels) == 0
            continue
        if d["what"] in ("reset", "fresh"):
            tracks.list = []
        want_ids, P, thickness = _inputs(d)
        assert np.array_equal(ids, want_ids) and len(labels) == len(ids)
        prior = tracks.priors()
        Pd = torch.from_numpy(P).cuda()
        lab = torch.empty(len(P), dtype=torch.int32, device="cuda")
        stage = ctx.track_planes(Pd, d["pose7"], thickness, prior24=prior, seed=12345, want_labels=True, labels_out=lab, **KW)
        assert _same_bytes([planes, info, labels], stage), (d["frame"], d["what"])
        want_pids, want_merged = tracks.apply(planes, info, thickness)
        assert np.array_equal(pids, want_pids) and np.array_equal(merged, want_merged), (d["frame"], pids, want_pids, merged, want_merged)
        assert (info[:len(prior), 5] == 1).all() and not info[len(prior):, 5].any()
        if d["what"] == "outlines":   # the outlines of the result: alva_plane_outlines on the same points, labels and records
            o = ctx.plane_outlines(Pd, lab, planes, max_vertices=64)
            assert _same_bytes(d["res"][6:], o) and (o[1][info[:, 0] == 0, 0] == 0).all() and (o[1][info[:, 0] != 0, 0] == 5).all()
            assert (o[2][info[:, 0] == 0] > 0).all()
        out.append(dict(call=d, P=P, thickness=thickness, prior=prior, stage=stage, plane_ids=pids, merged=merged))
    return out


def test_system_track_planes_equals_the_stage_and_follows_the_id_rules(replay, sessions):
    kinds = [r["call"]["what"] for r in replay]
    assert kinds.count("frame") >= 40 and kinds.count("outlines") == 1 and kinds.count("reset") == 1
    calls = sessions["with"]["calls"]
    assert calls[0]["what"] == "before" and (calls[0]["res"][1][:, 0] == 6).all()
    status = [d["status"] for d in calls]
    assert 3 in status and 4 in status and status.index(1) > 1   # initialising and LOST calls were among those answered with code 6


def test_system_calls_equal_the_restatement(ctx, replay):
    """EVERY replayed status-1 call through oracle_track, on the points, pose, thickness and priors of that call.  A call whose inputs pass
    all margins is compared in full (info, labels, moments, records).  One that passes the threshold and tie margins and whose normals
    are defined (eig_ratio) but misses an axis guard (axis_ratio, sign, ref, face: they decide a record's in-plane axes or the side its
    normal faces, never a count) is held to info and labels, which come through thresholds only.  One that misses a threshold or tie margin
    has a decision that a last bit may take either way, and nothing exact can be asked of it; at least nine calls in ten must be
    compared in full, and the call with outlines (40 frames in, the frame tests/test_gpu_detect_planes.py compares) is one of them.
    Measured on an MI355X: all 106 calls in full."""
    import torch
    full = counted = 0
    for r in replay:
        d = r["call"]
        want = T.oracle_track(r["P"], d["pose7"], r["prior"], r["thickness"], seed=12345, **KW)
        ok = T.margins_ok(want)
        decided = want["thr_margin"] >= T.MARGIN_MIN and min(want["tie_margin_t1"], want["tie_margin_t4"]) >= T.MARGIN_MIN and \
            all(g["eig_ratio"] >= C.MIN_EIG_RATIO for g in want["guards"])
        print(d["frame"], d["what"], "margins ok" if ok else "MARGINS: " + T.margins_text(want))
        # moments are not part of the system's answer: from the stage, on the same inputs
        got = ctx.track_planes(torch.from_numpy(r["P"]).cuda(), d["pose7"], r["thickness"], prior24=r["prior"], seed=12345, want_labels=True,
                               want_moments=True, **KW)
        assert _same_bytes(got[:3], r["stage"])
        if ok:
            _compare(got, want, len(r["prior"]))
            full += 1
        elif decided:
            assert np.array_equal(got[1], want["info"]) and np.array_equal(got[2], want["labels"]), d["frame"]
            counted += 1
        assert ok or d["what"] != "outlines"
    print("calls %d: compared in full %d, info and labels only %d, not comparable %d" % (len(replay), full, counted, len(replay) - full - counted))
    assert full >= 0.9 * len(replay)


def test_a_tracked_frame_that_sees_no_3d_point_is_answered_like_a_lost_one(sessions):
    """the first black frames still return status 1 but observe no 3-D point, so there is no depth to scale the slab by: code 6 in every
    slot, ids -1, nothing looked at (the replay fixture asserts the same of every such call); alva_system_detect_planes answers the same
    frames as an empty map (codes 1, 5) -- for tracking that answer would be code 7 for every plane, and the list would be emptied"""
    blind = [d for d in sessions["with"]["calls"] if d["status"] == 1 and len(d["order"]) == 0]
    assert len(blind) >= 1 and all(d["frame"] >= N_TRACK for d in blind)
    for d in blind:
        planes, info, pids, merged, ids, labels = d["res"][:6]
        assert info.tolist() == [[6, 0, -1, 0, 0, 0, 0, 0]] * 4 and (pids == -1).all() and (merged == -1).all() and not planes.any() and len(ids) == 0


def test_the_floor_keeps_its_id(replay):
    """From the first call that returns the floor -- the plane with the most inliers -- its id appears with code 0 in every later
    status-1 call, up to resetPlanes.  Measured on an MI355X: id 0 since frame 6, never lost (the restatement, fed the same inputs, agrees:
    test_system_calls_equal_the_restatement)."""
    floor_id, since = None, None
    for r in replay:
        d = r["call"]
        planes, info, pids = d["res"][0], d["res"][1], d["res"][2]
        if d["what"] == "reset":
            break
        found = info[:, 0] == 0
        if floor_id is None and found.any():
            k = int(np.argmax(np.where(found, info[:, 4], -1)))
            floor_id, since = int(pids[k]), d["frame"]
            continue
        if floor_id is not None:
            assert floor_id in pids[found].tolist(), (d["frame"], floor_id, pids.tolist(), info[:, :6].tolist())
            k = pids.tolist().index(floor_id)
            assert info[k, 5] == 1   # tracked, not found anew
    print("floor id", floor_id, "since frame", since)
    assert floor_id is not None


def test_reset_planes_makes_every_plane_new(replay):
    k = [r["call"]["what"] for r in replay].index("reset")
    before, after = replay[k - 1], replay[k]
    info, pids = after["call"]["res"][1], after["call"]["res"][2]
    assert len(after["prior"]) == 0 and not info[:, 5].any() and (info[:, 0] == 0).any()
    seen = max(int(r["plane_ids"].max()) for r in replay[:k])
    assert (pids[info[:, 0] == 0] > seen).all()   # fresh ids
    assert len(before["prior"]) >= 1              # (there was something to forget)


def test_without_tracked_planes_the_session_answers_as_detection(sessions, replay):
    """After resetPlanes, trackPlanes(max_vertices=64) and detectPlaneOutlines(max_vertices=64) at the same frame with the same max_planes,
    min_inliers and num_iterations: the same bytes in planes, info, ids, labels, outlines, outline_info and areas (merged_into is not
    compared) -- without priors the session's tracking path is detection --, and the planes' ids are fresh and ascending."""
    k = [r["call"]["what"] for r in replay].index("fresh")
    planes, info, pids, merged, ids, labels, outlines, oinfo, areas = replay[k]["call"]["res"]
    assert replay[k]["call"]["status"] == 1 and len(replay[k]["prior"]) == 0
    assert _same_bytes([planes, info, ids, labels, outlines, oinfo, areas], sessions["with"]["fresh_detect"])
    found = info[:, 0] == 0
    print("codes", info[:, 0].tolist(), "plane ids", pids.tolist())
    assert found.any()   # (the comparison is not vacuous)
    seen = max(int(r["plane_ids"].max()) for r in replay[:k])
    assert (pids[found] > seen).all() and (np.diff(pids[found]) > 0).all() and (pids[~found] == -1).all()


def test_track_planes_leaves_tracking_bitwise_unchanged(sessions):
    a, b = sessions["with"]["rec"], sessions["without"]["rec"]
    assert len(a) == len(b) and 1 in [r[0] for r in a] and 4 in [r[0] for r in a]
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0] == rb[0] and ra[3] == rb[3], k
        assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), k


# ---------------------------------------------------------------------------------------------------- the list and the map
@pytest.fixture(scope="module")
def short_session():
    """the first frames of the same stream through a session of its own, up to the twelfth tracked frame; then the rules that
    need a list of two planes or a map thrown away.  A slab an eighth as thick as REL_THICKNESS with min_inliers 8 cuts the stream's one
    surface into parallel slices further apart than the slab: several planes, none merged"""
    import torch
    import sysdiff
    import alvaar_amd
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    f = sysdiff.intrinsics(W, Hh)[0]
    canvas = synth.texture_canvas(W, Hh, 5)
    dev = torch.from_numpy(np.stack([synth.plane_stream_frame(canvas, SPEED * k, W, Hh, f) for k in range(24)])).cuda()
    ar = AlvaAR(W, Hh, cell_size=CELL, random_sampling=False, relocalization=True)
    out = {}

    def run(tracked):
        status = []
        for k in range(len(dev)):
            status.append(ar.find_camera_pose_device(int(dev[k].data_ptr()), 33.0 * k))
            if status.count(1) == tracked:
                break
        return status

    out["status"] = run(12)
    thin = dict(min_inliers=8, max_planes=8)
    out["thin"] = [tuple(np.copy(x) for x in ar.trackPlanes(REL_THICKNESS / 8, **thin)) for _ in range(2)]
    try:
        ar.trackPlanes(REL_THICKNESS / 8, min_inliers=8, max_planes=1)
        out["error"] = None
    except alvaar_amd.AlvaError as e:
        out["error"] = str(e)
    out["after_error"] = tuple(np.copy(x) for x in ar.trackPlanes(REL_THICKNESS / 8, **thin))
    ar.reset()                                     # the map is thrown away, and the list with it
    out["reset_call"] = tuple(np.copy(x) for x in ar.trackPlanes(REL_THICKNESS / 8, **thin))
    out["status2"] = run(3)   # the same frames again, up to the third tracked one
    out["new_map"] = tuple(np.copy(x) for x in ar.trackPlanes(REL_THICKNESS / 8, max_planes=1, min_inliers=8))
    ar.close()
    return out


def test_max_planes_below_the_tracked_count_is_an_argument_error(short_session):
    s = short_session
    assert s["status"].count(1) == 12
    first, second = s["thin"]
    kept = first[2][(first[1][:, 0] == 0) & (first[3] < 0)]
    assert len(kept) >= 2, (first[1][:, :6].tolist(), first[3].tolist())
    n = len(kept)
    assert second[1][:n, 5].tolist() == [1] * n and second[2][:n][second[1][:n, 0] == 0].tolist() == kept[second[1][:n, 0] == 0].tolist()
    tracked = int(((second[1][:, 0] == 0) & (second[3] < 0)).sum())
    assert tracked >= 2 and s["error"] is not None and "max_planes" in s["error"]
    third = s["after_error"]                       # the refused call left the list as it was
    assert third[1][:tracked, 5].tolist() == [1] * tracked
    assert third[2][:tracked][third[1][:tracked, 0] == 0].tolist() == second[2][(second[1][:, 0] == 0) & (second[3] < 0)][third[1][:tracked, 0] == 0].tolist()


def test_a_reset_map_takes_its_planes_with_it(short_session):
    s = short_session
    assert (s["reset_call"][1][:, 0] == 6).all()   # right after reset(): not tracking
    assert s["status2"][-1] == 1                   # the same frames again: initialised anew, and tracking at the last of them
    planes, info, pids, merged, ids, labels = s["new_map"]
    # max_planes = 1 is accepted (the list is empty: before the reset at least two planes were tracked), and the plane is new, under an id
    # that the old map never used
    seen = max(int(r[2].max()) for r in s["thin"] + [s["after_error"]])
    assert info[0, 0] == 0 and info[0, 5] == 0 and pids[0] > seen
