"""Relocalization after tracking loss (alva_system_set_relocalization, alva_reloc_match): the kernel against a numpy brute force, and the
LOST state machine on synthetic plane streams -- a blackout followed by an earlier view of the same world (recovered in the same map), a
blackout followed by a different world (never recovered, reset after max_lost_frames), reproducibility, grouped sessions, explicit reset.
No reference counterpart: the reference resets its map on tracking loss, and with the feature off so does the product."""
from __future__ import annotations

import numpy as np
import pytest

from alvaar_amd import synth
import sysdiff
from record_cases import _brute_force, _flip

pytestmark = pytest.mark.gpu

W, H, CELL = 640, 480, 12
# the plane stream at three views per frame (~6 px of motion): ten keyframes by frame 90, so the keyframes the blackout creates are past
# the early-map reset rule (kfid < 10 && n_3d < 3, mapper.cpp:35-43) and the loss goes through the pose-failure counter
SPEED, N_TRACK, N_BLACK, N_AFTER = 3, 110, 8, 30
RESUME_K = SPEED * 85   # 24 frames (72 views) behind the last tracked frame


# ---------------------------------------------------------------------------------------------------- the kernel
def _make_problem(seed=3, n_rows=12000, n_q=2600):
    rng = np.random.RandomState(seed)
    rows = np.zeros((n_rows, 64), np.uint8)
    desc = rng.randint(0, 256, (n_rows, 32)).astype(np.uint8)
    ids = rng.permutation(10 * n_rows).astype(np.int32)[:n_rows] + 1_000_000_000 // 2   # large ids: nothing may pack them into 20 bits
    ids[rng.rand(n_rows) < 0.05] = -1                                                        # unused rows
    q = rng.randint(0, 256, (n_q, 32)).astype(np.uint8)
    valid = (rng.rand(n_q) > 0.03).astype(np.uint8)
    live = np.nonzero(ids >= 0)[0]
    planted = rng.choice(n_q, int(0.4 * n_q), replace=False)
    targets = set()
    for qi in planted:                                   # copies of a live row with <= 20 flipped bits
        r = rng.choice(live)
        targets.add(int(r))
        q[qi], _ = _flip(rng, desc[r], rng.randint(0, 21))
    planted_set = set(planted.tolist())
    special = [i for i in range(n_q) if i not in planted_set][:40]
    free = iter([r for r in rng.permutation(live) if int(r) not in targets])
    # identical descriptors under two ids: the smaller id wins, the second distance equals the best -> rejected by the ratio test
    r1, r2 = next(free), next(free)
    desc[r2] = desc[r1]
    q[special[0]] = desc[r1]
    # a query at exactly max_dist (51) from its row: accepted (random rows lie ~128 bits away)
    r = next(free)
    q[special[1]], _ = _flip(rng, desc[r], 51)
    r = next(free)
    q[special[2]], _ = _flip(rng, desc[r], 52)           # one bit beyond: rejected
    # the ratio boundary: best 40, second 50 -> 40 < 0.8 * 50 is false; best 39, second 50 accepted
    for k, nb in ((3, 40), (4, 39)):
        ra, rb = next(free), next(free)
        q[special[k]], used = _flip(rng, desc[ra], nb)
        desc[rb], _ = _flip(rng, q[special[k]], 50, avoid=used)
    # several queries with the same best row: one-to-one, smallest (distance, query index) keeps it
    r = next(free)
    for k, nb in ((5, 7), (6, 3), (7, 3), (8, 12)):
        q[special[k]], _ = _flip(rng, desc[r], nb)
    for k in range(9):
        valid[special[k]] = 1
    rows[:, 0:4] = np.frombuffer(np.int32(7).tobytes(), np.uint8)
    rows[:, 4:8] = ids.view(np.uint8).reshape(-1, 4)
    rows[:, 8:32] = rng.randn(n_rows, 3).view(np.uint8).reshape(-1, 24)
    rows[:, 32:64] = desc
    return q, valid, rows, special


def test_reloc_match_equals_numpy_brute_force_and_ignores_row_order():
    import torch
    import alvaar_amd
    q, valid, rows, special = _make_problem()
    want = _brute_force(q, valid, rows)
    wd = {qi: (i, d) for qi, i, d in want}
    ids = rows[:, 4:8].copy().view(np.int32)[:, 0]
    assert special[0] not in wd                                            # identical descriptors under two ids
    assert special[1] in wd and wd[special[1]][1] == 51 and special[2] not in wd
    assert special[3] not in wd and special[4] in wd and wd[special[4]][1] == 39
    assert special[6] in wd and all(special[k] not in wd for k in (5, 7, 8))
    assert len(want) > 900
    ctx = alvaar_amd.Context(0)
    rng = np.random.RandomState(1)
    bv = rng.randn(len(q), 3)
    unpx = rng.rand(len(q), 2).astype(np.float32) * 600
    dq, dv = torch.from_numpy(q).cuda(), torch.from_numpy(valid).cuda()
    dbv, duv = torch.from_numpy(bv).cuda(), torch.from_numpy(unpx).cuda()
    results = []
    for perm in (np.arange(len(rows)), rng.permutation(len(rows))):
        r = np.ascontiguousarray(rows[perm])
        match, obv, ouv, owpt = ctx.reloc_match(dq, torch.from_numpy(r).cuda(), dv, bv=dbv, unpx=duv)
        m = match.cpu().numpy()
        got = [(int(a), int(c), int(d)) for a, b, c, d in m]
        assert got == want
        assert np.array_equal(m[:, 2], r[m[:, 1], 4:8].copy().view(np.int32)[:, 0])   # the row named holds the id reported
        xyz = r[m[:, 1], 8:32].copy().view(np.float64)
        assert np.array_equal(owpt.cpu().numpy(), xyz)
        assert np.array_equal(obv.cpu().numpy(), bv[m[:, 0]])
        assert np.array_equal(ouv.cpu().numpy(), unpx[m[:, 0]].astype(np.float64))
        results.append(got)
    assert results[0] == results[1]
    # degenerate sizes: no rows, no queries
    m0, _, _, _ = ctx.reloc_match(dq, torch.zeros((0, 64), dtype=torch.uint8).cuda(), dv)
    assert m0.shape[0] == 0
    assert ids.min() == -1


# ---------------------------------------------------------------------------------------------------- the state machine
def _frames(resume_canvas_seed=None):
    """N_TRACK frames of the plane stream, N_BLACK black frames, then N_AFTER frames resuming at view RESUME_K (an earlier view of the
    same plane, far behind the last tracked one) -- or of another canvas"""
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    fr = [synth.plane_stream_frame(canvas, SPEED * k, W, H, f) for k in range(N_TRACK)]
    fr += [np.zeros((H, W, 4), np.uint8) + np.array([0, 0, 0, 255], np.uint8)] * N_BLACK
    after = canvas if resume_canvas_seed is None else synth.texture_canvas(W, H, resume_canvas_seed)
    fr += [synth.plane_stream_frame(after, RESUME_K + SPEED * j, W, H, f) for j in range(N_AFTER)]
    views = [SPEED * k for k in range(N_TRACK)] + [None] * N_BLACK + [RESUME_K + SPEED * j for j in range(N_AFTER)]
    return np.stack(fr), views


def _run(frames, reloc, max_lost=0, stop_after=None):
    import torch
    from alvaar_amd.system import AlvaAR
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, relocalization=reloc, max_lost_frames=max_lost)
    dev = torch.from_numpy(frames).cuda()
    rec = []
    for k in range(len(frames) if stop_after is None else stop_after):
        st = ar.find_camera_pose_device(int(dev[k].data_ptr()), 33.0 * k)
        rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [int(v) for v in ar.state()]))
    stats = ar.relocalization_stats()
    return ar, rec, stats


def _gt7(k):
    R, t = synth.plane_camera_pose(k)
    # rotation matrix -> quaternion (x, y, z, w)
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.copysign(np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
    return np.concatenate([t, [x, y, z, w]])


def _sim3_from(ref7, got7):
    """the gauge alignment of sysdiff.sim3_aligned_diff (rotation: chordal mean of the orientations; scale and translation by least
    squares on the centres), returned as (c, R, t, extent of the reference centres)"""
    A = np.array([p[:3] for p in got7]); B = np.array([p[:3] for p in ref7])
    ma, mb = A.mean(0), B.mean(0)
    M = sum(sysdiff._quat_to_rot(pr[3:]) @ sysdiff._quat_to_rot(pg[3:]).T for pr, pg in zip(ref7, got7))
    U, S, Vt = np.linalg.svd(M)
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    RA = (R @ (A - ma).T).T
    c = float(((B - mb) * RA).sum() / (RA ** 2).sum())
    return c, R, mb - c * R @ ma, float(np.linalg.norm(B - mb, axis=1).max())


def _aligned_errors(sim, ref7, got7):
    c, R, t, extent = sim
    dpos = drot = 0.0
    for pr, pg in zip(ref7, got7):
        dpos = max(dpos, float(np.linalg.norm(c * R @ pg[:3] + t - pr[:3])) / extent)
        Rr, Rg = sysdiff._quat_to_rot(pr[3:]), R @ sysdiff._quat_to_rot(pg[3:])
        drot = max(drot, float(np.arccos(np.clip((np.trace(Rr.T @ Rg) - 1) / 2, -1, 1))))
    return dpos, drot


@pytest.fixture(scope="module")
def blackout_runs():
    frames, views = _frames()
    out = {}
    for name, reloc in (("off", False), ("on", True), ("on2", True)):
        ar, rec, stats = _run(frames, reloc)
        out[name] = (rec, stats, ar.counters())
        ar.close()
    return frames, views, out


def test_blackout_then_earlier_view_relocalizes_into_the_same_map(blackout_runs):
    frames, views, runs = blackout_runs
    off, on = runs["off"][0], runs["on"][0]
    st_off, st_on = [r[0] for r in off], [r[0] for r in on]
    cut = st_off.index(2)
    assert N_TRACK <= cut < N_TRACK + N_BLACK and 1 in st_off[:cut]
    for k in range(cut):   # feature on == feature off up to the frame that resets: status, the 16 counters, poses, bitwise
        assert on[k][0] == off[k][0] and on[k][3] == off[k][3], k
        assert np.array_equal(on[k][1].view(np.uint64), off[k][1].view(np.uint64)), k
    assert 2 not in st_on
    back = N_TRACK + N_BLACK
    first_ok = next(k for k in range(cut, len(st_on)) if st_on[k] == 1)
    assert set(st_on[cut:first_ok]) == {4} and first_ok < back + 3, st_on[cut:]
    assert set(st_on[first_ok:]) == {1}, st_on[first_ok:]
    last_good = max(k for k in range(cut) if st_on[k] == 1)
    for k in range(cut, first_ok):   # status 4: the pose of the last status-1 frame
        assert np.array_equal(on[k][2], on[last_good][2]), k
    # keyframe / map-point ids continue: the map of the frames before the loss is the one the camera is back in
    kf_before, mp_before = on[cut - 1][3][11], on[cut - 1][3][12]
    assert on[first_ok][3][11] > kf_before and on[first_ok][3][12] >= mp_before and on[first_ok][3][8] == 1
    stats = runs["on"][1]
    assert stats["successes"] == 1 and stats["lost_frames"] == 0 and stats["attempts"] == first_ok - cut
    # the trajectory after relocalization in the gauge of the one before the loss (Sim(3) fitted on the pre-loss frames only)
    pre = [k for k in range(cut) if st_on[k] == 1 and views[k] is not None]
    sim = _sim3_from([_gt7(views[k]) for k in pre], [on[k][1] for k in pre])
    post = [k for k in range(first_ok, len(on)) if st_on[k] == 1 and views[k] is not None][:30]
    assert len(post) >= 25
    dpos, drot = _aligned_errors(sim, [_gt7(views[k]) for k in post], [on[k][1] for k in post])
    print(f"post-relocalization error in the pre-loss gauge: centre {dpos:.3e} x extent, rotation {drot:.3e} rad "
          f"(relocalized on frame {first_ok - back} after the scene returned, {runs['on'][1]['last_inliers']} inliers)")
    assert dpos < 0.02 and drot < 1e-2, (dpos, drot)
    # teeth: the feature-off run re-initialises into a new gauge, which the same check rejects (or it has no pose at all)
    post_off = [k for k in range(back, len(off)) if st_off[k] == 1]
    if post_off:
        dpos_off, drot_off = _aligned_errors(sim, [_gt7(views[k]) for k in post_off], [off[k][1] for k in post_off])
        assert dpos_off > 0.02 or drot_off > 1e-2, (dpos_off, drot_off)


def test_relocalization_is_reproducible(blackout_runs):
    _, _, runs = blackout_runs
    a, b = runs["on"], runs["on2"]
    assert [r[0] for r in a[0]] == [r[0] for r in b[0]]
    for ra, rb in zip(a[0], b[0]):
        assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and ra[3] == rb[3]
    assert a[1] == b[1] and a[2] == b[2]


def test_a_different_world_is_never_relocalized_and_resets_after_max_lost_frames():
    frames, _ = _frames(resume_canvas_seed=99)
    max_lost = 12
    ar, rec, stats = _run(frames, True, max_lost)
    ar.close()
    st = [r[0] for r in rec]
    e = st.index(4)
    assert 1 not in st[e:e + max_lost] and st[e:e + max_lost] == [4] * max_lost, st[e:]
    assert st[e + max_lost] == 2 and 2 not in st[:e + max_lost]
    assert stats["successes"] == 0 and stats["attempts"] >= max_lost


def test_explicit_reset_while_lost():
    import torch
    frames, _ = _frames()
    ar, rec, _ = _run(frames, True, stop_after=N_TRACK + 6)
    assert rec[-1][0] == 4
    assert ar.getFramePoints() == []
    ar.reset()
    assert ar.relocalization_stats()["lost_frames"] == 0
    dev = torch.from_numpy(frames[N_TRACK + N_BLACK]).cuda()
    assert ar.find_camera_pose_device(int(dev.data_ptr()), 33.0 * (N_TRACK + 6)) == 3
    ar.close()


def test_grouped_session_through_a_blackout_equals_its_solo_run():
    import torch
    from alvaar_amd.system import AlvaAR, SystemGroup
    f = sysdiff.intrinsics(W, H)[0]
    frames, _ = _frames()
    n = len(frames)
    canvas = synth.texture_canvas(W, H, 7)
    steady = np.stack([synth.plane_stream_frame(canvas, k, W, H, f) for k in range(n)])
    dev = [torch.from_numpy(frames).cuda(), torch.from_numpy(steady).cuda()]

    def record(ar):
        ids, px, _ = ar.keypoints()
        return ar.pose7()[0].copy(), ids.copy(), px.copy(), list(ar.state())

    solo = []
    for d in dev:
        ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, relocalization=True)
        solo.append([(ar.find_camera_pose_device(int(d[k].data_ptr()), 33.0 * k),) + record(ar) for k in range(n)])
        ar.close()
    assert 4 in [r[0] for r in solo[0]] and 1 in [r[0] for r in solo[0][N_TRACK + N_BLACK:]]
    group = SystemGroup([], 2)
    sessions = [AlvaAR(W, H, cell_size=CELL, random_sampling=False, relocalization=True) for _ in dev]
    group.set_sessions(sessions)
    together = [[] for _ in dev]
    for k in range(n):
        st = group.step_device([int(d[k].data_ptr()) for d in dev], 33.0 * k)
        for i, ar in enumerate(sessions):
            together[i].append((int(st[i]),) + record(ar))
    for ar in sessions:
        ar.close()
    group.close()
    for i in range(len(dev)):
        for k in range(n):
            a, b = solo[i][k], together[i][k]
            assert a[0] == b[0] and a[4] == b[4], (i, k)
            assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)), (i, k)
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)), (i, k)
