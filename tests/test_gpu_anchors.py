"""Anchors (alva_anchor_attach / alva_anchor_update / alva_system_create_anchors / alva_system_update_anchors) on the GPU against their
numpy restatement tests/anchor_cases.py.

Attach is a set function of bit patterns: index, count and the bits of dist2 are compared with ==.  Update: info exactly (every case is
asserted to be >= 1e-7 away from each decision, or exactly on it by construction); rt12 within 1e-9 x max(1, largest |coordinate| of the
case), the project's FP64 stage bar; pose16 within 1e-6, the bar of the plane records.

The system test runs the stream and the two sessions of tests/test_gpu_track_planes.py (110 plane frames + 8 black, cell 12,
relocalization on).  One session creates four anchors at the tenth tracked frame (three hitTest poses and detectPlanes' first plane),
calls updateAnchors after every frame and removes one anchor midway; every call is replayed through Context.anchor_update and
Context.anchor_attach with the inputs that the restated list (anchor_cases.Anchors) derives from map_points() snapshots, and must give
the same bytes.

A stream of its own provokes what the long one never needs, a re-attach: five of an anchor's eight supports are merged away.

Measured on an MI355X.  Stage 2 follows the header's butterfly order exactly, and the doubles agree BIT FOR BIT: all 17 cases, max |d rt12|
= 0 and max |d pose16| = 0 (so do the floats).  The system stream, per anchor (updates, updates that saw a support away from its
attach-time position, largest |t|, largest rotation angle, supports vanished, re-attaches): anchor 0: 98, 90, 0.225, 0.859 deg, 4, 0;
anchor 1 (removed midway): 46, 38, 0.0986, 0.38 deg, 2, 0; anchor 2: 98, 90, 0.105, 0.373 deg, 0, 0; anchor 3: 98, 90, 0.195, 0.756 deg,
3, 0.  So local BA does move the supports on this stream; every update was code 0, and no anchor ever fell
below half its supports.  98 updates and 1 attach were replayed with the system's bytes; 115 of 115 anchor updates compared with the
restatement passed its margins."""
from __future__ import annotations

import math

import numpy as np
import pytest

import anchor_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import alvaar_amd
    return alvaar_amd.Context(0)


def _dev(P):
    import torch
    return torch.from_numpy(np.ascontiguousarray(P, np.float64)).cuda() if len(P) else torch.zeros((0, 3), dtype=torch.float64, device="cuda")


def _same_bytes(a, b):
    return len(a) == len(b) and all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
                                    for x, y in zip(a, b))


def _attach_equal(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and \
        np.array_equal(np.ascontiguousarray(got[1]).view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64))


# ---------------------------------------------------------------------------------------------------- stage 1
@pytest.mark.parametrize("K", [8, 64])
def test_attach_equals_the_restatement_at_every_size(ctx, K):
    for n in A.attach_sizes(K):
        P, pos = A.attach_points(n)
        got, want = ctx.anchor_attach(_dev(P), pos, K), A.attach(P, pos, K)
        assert (got[2] == min(K, n)).all(), n
        assert _attach_equal(got, want), (K, n, got[0][:, :8].tolist(), want[0][:, :8].tolist())


def test_attach_refuses_one_point_too_many(ctx):
    import torch
    import alvaar_amd
    P, pos = A.attach_points(513)
    before = ctx.anchor_attach(_dev(P), pos, 8)
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.anchor_attach(torch.zeros((A.N_CAP + 1, 3), dtype=torch.float64, device="cuda"), pos, 8)
    assert _same_bytes(ctx.anchor_attach(_dev(P), pos, 8), before)   # the context is as good as before


def test_attach_ties_duplicates_and_zero_distance(ctx):
    P, pos = A.lattice()
    for K in (8, 27, 64):   # 1 + 6 + 12 + 8 = 27 points within d = 3; the cut at 8 and at 64 falls inside a group of equal distances
        got, want = ctx.anchor_attach(_dev(P), pos, K), A.attach(P, pos, K)
        assert _attach_equal(got, want), K
    got = ctx.anchor_attach(_dev(P), pos, 8)
    assert got[1][0].tolist() == [0, 1, 1, 1, 1, 1, 1, 2] and got[0][0, 0] == 5 * 121 + 5 * 11 + 5      # d = 0: the anchor sits on a point
    assert got[0][0, 1:7].tolist() == sorted(got[0][0, 1:7].tolist()) and got[0][0, 7] == np.flatnonzero((P ** 2).sum(1) == 2).min()
    P, pos = A.duplicates()
    got = ctx.anchor_attach(_dev(P), pos, 9)
    assert _attach_equal(got, A.attach(P, pos, 9))
    assert (got[0][0, 1::3] == got[0][0, 0::3] + 40).all() and (got[0][0, 2::3] == got[0][0, 0::3] + 80).all()
    P, _ = A.attach_points(2049)
    got = ctx.anchor_attach(_dev(P), P[[700, 2048]], 8)
    assert got[0][:, 0].tolist() == [700, 2048] and got[1][:, 0].tolist() == [0, 0] and _attach_equal(got, A.attach(P, P[[700, 2048]], 8))


def test_sixteen_anchors_equal_sixteen_calls_and_calls_repeat(ctx):
    P, _ = A.attach_points(2049)
    rng = np.random.default_rng(3)
    pos = rng.standard_normal((16, 3)) * 2
    dev = _dev(P)
    all16 = ctx.anchor_attach(dev, pos, 32)
    assert _same_bytes(all16, ctx.anchor_attach(dev, pos, 32))       # two identical calls
    for a in range(16):
        one = ctx.anchor_attach(dev, pos[a:a + 1], 32)
        assert _same_bytes([x[a:a + 1] for x in all16], one), a
    assert _attach_equal(all16, A.attach(P, pos, 32))


# ---------------------------------------------------------------------------------------------------- stage 2
def _gpu_update(ctx, cases):
    return ctx.anchor_update([c["count"] for c in cases], np.stack([c["ref"] for c in cases]), np.stack([c["cur"] for c in cases]),
                             np.stack([c["pose_ref"] for c in cases]))


def _compare_update(pose, rt12, info, want, case, name):
    scale = max(1.0, float(np.abs(case["ref"][:case["count"]]).max(initial=0)), float(np.abs(case["cur"][:case["count"]]).max(initial=0)))
    d_rt, d_pose = float(np.abs(rt12 - want["rt12"]).max()), float(np.abs(pose.astype(np.float64) - want["pose"]).max())
    bits = np.array_equal(rt12.view(np.uint64), want["rt12"].view(np.uint64)) and np.array_equal(pose.view(np.uint32), want["pose"].view(np.uint32))
    print("%-16s info %s  max |d rt12| %.3g  max |d pose| %.3g  %s  %s" % (name, info[:3].tolist(), d_rt, d_pose,
                                                                         "bit for bit" if bits else "NOT bitwise", A.margins_text(want)))
    assert A.margins_ok(want, case["exact"]), A.margins_text(want)
    assert np.array_equal(info, want["info"])
    assert d_rt <= 1e-9 * scale and d_pose <= 1e-6
    assert pose[15] == 1 and not pose[[3, 7, 11]].any()
    return d_rt, d_pose, bits


def test_update_equals_the_restatement(ctx):
    """every case of anchor_cases.update_cases: m = 0 1 3 4 63 64, the identity, a pure translation, rotations of 1, 90 and 180 degrees, the
    trimmed case, a trim that leaves three, collinear supports and near-collinear ones on both sides of the gap test"""
    worst_rt = worst_pose = 0.0
    exact = 0
    names = sorted(A.update_cases())
    for name in names:
        case, want = A.update_cases()[name], A.oracle_of(name)
        assert want["code"] == case["code"] and want["kept"] == case["kept"]
        pose, rt12, info = _gpu_update(ctx, [case])
        d_rt, d_pose, bits = _compare_update(pose[0], rt12[0], info[0], want, case, name)
        worst_rt, worst_pose, exact = max(worst_rt, d_rt), max(worst_pose, d_pose), exact + bits
    print("cases %d: bit for bit %d; max |d rt12| %.3g, max |d pose| %.3g" % (len(names), exact, worst_rt, worst_pose))


def test_identity_is_bitwise(ctx):
    case = A.update_cases()["identity"]
    pose, rt12, info = _gpu_update(ctx, [case])
    want = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
    assert np.array_equal(rt12[0].view(np.uint64), want.view(np.uint64))
    assert np.array_equal(pose[0].view(np.uint32), case["pose_ref"].view(np.uint32)) and info[0].tolist() == [0, 32, 32, 0, 0, 0, 0, 0]
    none = A.update_cases()["m0"]                                    # no support: the reference pose, byte for byte
    pose, rt12, info = _gpu_update(ctx, [none])
    assert np.array_equal(rt12[0].view(np.uint64), want.view(np.uint64)) and np.array_equal(pose[0].view(np.uint32), none["pose_ref"].view(np.uint32))
    assert info[0].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]


def test_sixty_four_anchors_equal_sixty_four_calls(ctx):
    names = sorted(A.update_cases())
    cases = [A.update_cases()[names[k % len(names)]] for k in range(64)]
    all64 = _gpu_update(ctx, cases)
    assert _same_bytes(all64, _gpu_update(ctx, cases))
    for k in (0, 1, 2, 3, 4, 5, 31, 62, 63) + tuple(range(6, 6 + len(names))):
        assert _same_bytes([x[k:k + 1] for x in all64], _gpu_update(ctx, [cases[k]])), (k, names[k % len(names)])
    for k in range(64):   # every row is the row of its case alone
        first = names.index(names[k % len(names)])
        assert _same_bytes([x[k] for x in all64], [x[first] for x in all64]), k
    # a partly filled workgroup: 5 anchors are two workgroups of four waves, three of them idle
    five = _gpu_update(ctx, cases[:5])
    assert _same_bytes(five, [x[:5] for x in all64])


def test_bad_arguments_are_rejected(ctx):
    import alvaar_amd
    P, pos = A.attach_points(513)
    dev = _dev(P)
    good = ctx.anchor_attach(dev, pos, 8)
    for bad in (dict(pos3=np.zeros((0, 3))), dict(pos3=np.zeros((17, 3))), dict(max_support=7), dict(max_support=65)):
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.anchor_attach(dev, **dict(dict(pos3=pos, max_support=8), **bad))
        assert _same_bytes(ctx.anchor_attach(dev, pos, 8), good)
    case = A.update_cases()["planted32"]
    good = _gpu_update(ctx, [case])
    for count in ([65], [-1], [], [1] * 65):
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.anchor_update(count, np.zeros((len(count), 64, 3)), np.zeros((len(count), 64, 3)), np.tile(A.POSE_REF, (len(count), 1)))
        assert _same_bytes(_gpu_update(ctx, [case]), good)


# ---------------------------------------------------------------------------------------------------- the system surface
W, Hh, CELL = 640, 480, 12            # the stream and session set-up of tests/test_gpu_track_planes.py
SPEED, N_TRACK, N_BLACK = 3, 110, 8
REL_THICKNESS = 3 * 0.00128905
TAPS = np.array([(320, 240), (200, 150), (440, 330), (160, 360), (480, 120)], np.float32)
K_SUPPORT = 32


def _snapshot(ar):
    ids, xyz, fl, _, _ = ar.map_points()
    keep = fl[:, 0] == 1
    order = np.argsort(ids[keep], kind="stable")
    return ids[keep][order].copy(), np.ascontiguousarray(xyz[keep][order])


@pytest.fixture(scope="module")
def sessions():
    """the same frames through two sessions: one creates anchors at its tenth tracked frame, updates them after every frame, removes one
    midway and, when the stream is over, resets; the other never touches the API"""
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
        rec, events, tracked = [], [], 0
        if name == "with":
            events.append(dict(what="create", frame=-1, status=0, res=ar.createAnchors(A.pose_of()[None], K_SUPPORT)))
            events.append(dict(what="update", frame=-1, status=0, res=ar.updateAnchors()))
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(dev[k].data_ptr()), 33.0 * k)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [int(v) for v in ar.state()]))
            tracked += st == 1
            if name != "with":
                continue
            snap = _snapshot(ar) if st == 1 else None
            if st == 1 and tracked == 10:
                hits = ar.hitTest(TAPS)
                planes = ar.detectPlanes(REL_THICKNESS)
                ok = np.flatnonzero(hits[1][:, 0] == 0)[:3]
                poses = np.concatenate([hits[0][ok], planes[0][:1, :16]])
                events.append(dict(what="create", frame=k, status=st, snap=snap, poses=poses.copy(), hits=hits, planes=planes,
                                   res=ar.createAnchors(poses, K_SUPPORT)))
            if st != 1 and k >= N_TRACK and not any(e["what"] == "create" and e["frame"] >= N_TRACK for e in events):
                events.append(dict(what="create", frame=k, status=st, res=ar.createAnchors(A.pose_of()[None], K_SUPPORT)))   # while LOST
            events.append(dict(what="update", frame=k, status=st, snap=snap, res=ar.updateAnchors()))
            if st == 1 and tracked == 55:
                victim = int(events[-1]["res"][0][1])
                events.append(dict(what="remove", frame=k, status=st, id=victim, res=(ar.removeAnchor(victim), ar.removeAnchor(victim))))
        if name == "with":
            # the stream is over: a reset throws the map away and the anchors with it; ids go on from where they were
            ar.reset()
            events.append(dict(what="update_after_reset", frame=len(frames), status=0, res=ar.updateAnchors()))
            again = 0
            for k in range(40):
                st = ar.find_camera_pose_device(int(dev[k].data_ptr()), 33.0 * k)
                again += st == 1
                if again == 3:
                    break
            events.append(dict(what="create_after_reset", frame=k, status=st, res=ar.createAnchors(A.pose_of(t=_snapshot(ar)[1][0])[None], 8)))
            events.append(dict(what="update_new_map", frame=k, status=st, res=ar.updateAnchors()))
            ar.resetAnchors()
            events.append(dict(what="update_after_reset_anchors", frame=k, status=st, res=ar.updateAnchors()))
        out[name] = dict(rec=rec, events=events)
        ar.close()
    return out


def _stage_fns(ctx, attaches):
    def attach_fn(P, pos3, K):
        got = ctx.anchor_attach(_dev(P), pos3, K)
        attaches.append(len(pos3))
        return got

    def update_fn(count, ref, cur, pose_ref):
        return ctx.anchor_update(count, ref, cur, pose_ref)
    return attach_fn, update_fn


@pytest.fixture(scope="module")
def replay(ctx, sessions):
    """the anchored session's events through the restated list with the stages on the GPU: every answer must have the system's bytes"""
    attaches, stage_calls = [], []
    attach_fn, update_fn = _stage_fns(ctx, attaches)
    L = A.Anchors()
    stats = {}
    for e in sessions["with"]["events"]:
        if e["what"] == "create":
            if e["status"] != 1:
                ids, info = e["res"]
                assert (ids == -1).all() and info.tolist() == [[6, 0, 0, 0, 0, 0, 0, 0]] * len(ids), (e["frame"], info.tolist())
                continue
            cand_ids, cand_P = e["snap"]
            want = L.create(e["poses"], K_SUPPORT, cand_ids[-A.N_CAP:], cand_P[-A.N_CAP:], attach_fn)
            assert _same_bytes(e["res"], want), (e["res"], want)
        elif e["what"] == "remove":
            assert e["res"] == (True, False) and L.remove(e["id"]) == 1
        elif e["what"] == "update":
            if e["status"] != 1:
                assert _same_bytes(e["res"], L.not_tracking()), e["frame"]
                continue
            before = {a["id"]: len(a["sup"]) for a in L.list}
            n_att = len(attaches)
            want = L.update(e["snap"][0], e["snap"][1], update_fn, attach_fn, on_stage=stage_calls.append)
            assert _same_bytes(e["res"], want), (e["frame"], e["res"][2].tolist(), want[2].tolist())
            if L.list:
                s = stage_calls[-1]
                for k, a in enumerate(L.list):
                    st = stats.setdefault(a["id"], dict(updates=0, moved=0, max_t=0.0, max_deg=0.0, vanished=0, reattached=0, codes=set()))
                    m = int(s["count"][k])
                    R = s["rt12"][k, :9].reshape(3, 3)
                    st["updates"] += 1
                    st["moved"] += bool((s["ref"][k, :m] != s["cur"][k, :m]).any())
                    st["max_t"] = max(st["max_t"], float(np.linalg.norm(s["rt12"][k, 9:])))
                    st["max_deg"] = max(st["max_deg"], math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(R) - 1) / 2)))))
                    st["vanished"] += before[a["id"]] - m
                    st["reattached"] += int(want[2][k, 3])
                    st["codes"].add(int(want[2][k, 0]))
                assert (len(attaches) > n_att) == bool(want[2][:, 3].any())
    return dict(stats=stats, stage_calls=stage_calls, attaches=attaches, final=L)


def test_system_anchors_follow_the_map(sessions, replay):
    ev = sessions["with"]["events"]
    created = [e for e in ev if e["what"] == "create" and e["status"] == 1]
    assert len(created) == 1
    e = created[0]
    assert (e["hits"][1][:, 0] == 0).sum() >= 3 and e["planes"][1][0, 0] == 0, (e["hits"][1][:, 0].tolist(), e["planes"][1][:, 0].tolist())
    ids, info = e["res"]
    assert ids.tolist() == [0, 1, 2, 3] and (info[:, 0] == 0).all() and (info[:, 1] == K_SUPPORT).all() and (info[:, 2] == len(e["snap"][0])).all()
    updates = [x for x in ev if x["what"] == "update" and x["status"] == 1 and len(x["res"][0])]
    assert len(updates) >= 60
    assert updates[0]["res"][0].tolist() == [0, 1, 2, 3] and updates[-1]["res"][0].tolist() == [0, 2, 3]      # one was removed midway
    for x in updates:
        assert set(x["res"][2][:, 0].tolist()) <= {0, 1, 2}
        assert x["res"][2][:, 4].tolist() == [x["res"][2][0, 4]] * len(x["res"][0])     # the same age: every update ran for all of them
    # the first update, on the map the anchors were created on: nothing has moved, and the poses are the created ones
    assert np.array_equal(updates[0]["res"][1], e["poses"]) and (updates[0]["res"][2][:, 0] == 0).all()
    print("anchor: updates, updates that saw a moved support, max |t|, max angle (deg), supports vanished, re-attaches, codes")
    for aid, s in sorted(replay["stats"].items()):
        print("  %d: %d, %d, %.3g, %.3g, %d, %d, %s" % (aid, s["updates"], s["moved"], s["max_t"], s["max_deg"], s["vanished"], s["reattached"],
                                                      sorted(s["codes"])))
    print("stage calls replayed: %d updates, %d attaches" % (len(replay["stage_calls"]), len(replay["attaches"])))


def test_system_updates_equal_the_restatement(replay):
    """every replayed stage call through the numpy restatement too: info exactly and the pose within 1e-6 wherever the call's margins
    hold (a call on real map data may sit near a trim threshold; those are counted, and at least nine in ten must be comparable)"""
    total = compared = 0
    for s in replay["stage_calls"][::3]:
        want = A.update(s["count"], s["ref"], s["cur"], s["pose_ref"])
        for k, r in enumerate(want["per"]):
            total += 1
            if not A.margins_ok(r):
                print("margins:", A.margins_text(r))
                continue
            compared += 1
            assert np.array_equal(s["info"][k], r["info"]), (s["info"][k].tolist(), r["info"].tolist())
            scale = max(1.0, float(np.abs(s["cur"][k]).max()), float(np.abs(s["ref"][k]).max()))
            assert np.abs(s["rt12"][k] - r["rt12"]).max() <= 1e-9 * scale and np.abs(s["pose"][k].astype(np.float64) - r["pose"]).max() <= 1e-6
    print("anchor updates %d, compared %d" % (total, compared))
    assert total >= 60 and compared >= 0.9 * total


def test_not_tracking_answers_code_6_and_keeps_the_list(sessions):
    ev = sessions["with"]["events"]
    assert ev[0]["what"] == "create" and ev[0]["res"][0].tolist() == [-1] and ev[0]["res"][1][0].tolist() == [6, 0, 0, 0, 0, 0, 0, 0]
    assert ev[1]["what"] == "update" and len(ev[1]["res"][0]) == 0
    status = [x["status"] for x in ev if x["what"] == "update"]
    assert 3 in status and 4 in status and 1 in status
    lost = [x for x in ev if x["what"] == "update" and x["status"] == 4]
    last_ok = [x for x in ev if x["what"] == "update" and x["status"] == 1 and x["frame"] < lost[0]["frame"]][-1]
    for x in lost:   # the pose delivered last, again and again; nothing ages
        assert x["res"][0].tolist() == [0, 2, 3] and (x["res"][2][:, 0] == 6).all()
        assert np.array_equal(x["res"][1].view(np.uint32), last_ok["res"][1].view(np.uint32))
        assert np.array_equal(x["res"][2][:, 4:6], last_ok["res"][2][:, 4:6])
    lost_create = [x for x in ev if x["what"] == "create" and x["frame"] >= N_TRACK]
    assert len(lost_create) == 1 and lost_create[0]["status"] != 1 and lost_create[0]["res"][1][0, 0] == 6 and lost_create[0]["res"][0][0] == -1


def test_a_reset_map_takes_its_anchors_with_it_and_ids_go_on(sessions):
    ev = {x["what"]: x for x in sessions["with"]["events"]}
    assert len(ev["update_after_reset"]["res"][0]) == 0
    assert ev["create_after_reset"]["status"] == 1
    ids, info = ev["create_after_reset"]["res"]
    assert ids.tolist() == [4] and info[0, 0] == 0 and info[0, 1] == 8          # 0 .. 3 were used by the old map
    aid, pose, info = ev["update_new_map"]["res"]
    assert aid.tolist() == [4] and info[0, :6].tolist() == [0, 8, 8, 0, 1, 8]
    assert len(ev["update_after_reset_anchors"]["res"][0]) == 0


# ---------------------------------------------------------------------------------------------------- a re-attach, provoked
@pytest.fixture(scope="module")
def merged_session():
    """the stream's first frames up to the 60th tracked one in a session of its own; an anchor with 8 supports is put among map points
    that the camera has left behind, and five of its supports are then merged into points in view (alva_system_merge_map_points: the
    absorbed id is gone) -- three alive of eight is below half, so the next update re-attaches"""
    import torch
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    f = sysdiff.intrinsics(W, Hh)[0]
    canvas = synth.texture_canvas(W, Hh, 5)
    ar = AlvaAR(W, Hh, cell_size=CELL, random_sampling=False, relocalization=True)
    tracked = 0
    for k in range(90):
        frame = torch.from_numpy(synth.plane_stream_frame(canvas, SPEED * k, W, Hh, f)).cuda()
        tracked += ar.find_camera_pose_device(int(frame.data_ptr()), 33.0 * k) == 1
        if tracked == 60:
            break
    ids, xyz, fl, _, _ = ar.map_points()
    out = dict(tracked=tracked, snap0=_snapshot(ar))
    cand_ids, cand_P = out["snap0"]
    is_lost = dict(zip(ids.tolist(), ((fl[:, 0] == 1) & (fl[:, 1] == 0)).tolist()))
    seen = [int(i) for i in ids[(fl[:, 0] == 1) & (fl[:, 1] == 1)]][::-1]
    # the left-behind point with the most left-behind points among its 8 nearest
    lost_rows = [r for r, i in enumerate(cand_ids.tolist()) if is_lost[i]]
    best, best_n = None, -1
    for r in lost_rows[:400]:
        near = np.argsort(((cand_P - cand_P[r]) ** 2).sum(1), kind="stable")[:8]
        n_lost = sum(is_lost[int(cand_ids[j])] for j in near)
        if n_lost > best_n:
            best, best_n = r, n_lost
    out["pose"] = A.pose_of(t=cand_P[best]) if best is not None else A.pose_of()
    out["create"] = ar.createAnchors(out["pose"][None], 8)
    out["up0"] = ar.updateAnchors()
    index, _, _ = A.attach(cand_P, out["pose"][None, 12:15].astype(np.float64), 8)
    supports = [int(cand_ids[j]) for j in index[0] if j >= 0]
    merged = []
    for sid in supports:
        if len(merged) == 5 or not is_lost.get(sid, False):
            continue
        for t in seen[:200]:
            if ar.merge_map_points(sid, t):
                merged.append((sid, t))
                seen.remove(t)
                break
    out.update(supports=supports, merged=merged, snap1=_snapshot(ar), up1=ar.updateAnchors(), up2=ar.updateAnchors())
    ar.close()
    return out


def test_an_anchor_left_with_under_half_its_supports_is_reattached(ctx, merged_session):
    m = merged_session
    assert m["tracked"] == 60 and len(m["merged"]) == 5, (m["tracked"], m["merged"], m["supports"])
    attaches = []
    attach_fn, update_fn = _stage_fns(ctx, attaches)
    L = A.Anchors()
    assert _same_bytes(m["create"], L.create(m["pose"], 8, *m["snap0"], attach_fn)) and m["create"][1][0, :2].tolist() == [0, 8]
    assert L.list[0]["sup"] == m["supports"]
    assert _same_bytes(m["up0"], L.update(*m["snap0"], update_fn, attach_fn)) and m["up0"][2][0, :6].tolist() == [0, 8, 8, 0, 1, 8]
    gone = {a for a, _ in m["merged"]}
    assert not gone & set(m["snap1"][0].tolist())                                   # the absorbed ids left the map
    want = L.update(*m["snap1"], update_fn, attach_fn)
    assert _same_bytes(m["up1"], want), (m["up1"][2].tolist(), want[2].tolist())
    assert m["up1"][2][0, 1] == 3 and m["up1"][2][0, 3:6].tolist() == [1, 2, 8] and len(attaches) == 2      # re-attached: through stage 1 again
    assert len(L.list[0]["sup"]) == 8 and not gone & set(L.list[0]["sup"])
    assert np.array_equal(L.list[0]["ref_pose"].view(np.uint32), m["up1"][1][0].view(np.uint32))    # the delivered pose is the new reference
    want = L.update(*m["snap1"], update_fn, attach_fn)
    assert _same_bytes(m["up2"], want) and m["up2"][2][0, :6].tolist() == [0, 8, 8, 0, 3, 8]
    assert np.array_equal(m["up2"][1], m["up1"][1])                                  # nothing moved since: the same pose


def test_anchors_leave_tracking_bitwise_unchanged(sessions):
    a, b = sessions["with"]["rec"], sessions["without"]["rec"]
    assert len(a) == len(b) and 1 in [r[0] for r in a] and 4 in [r[0] for r in a]
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0] == rb[0] and ra[3] == rb[3], k
        assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), k
