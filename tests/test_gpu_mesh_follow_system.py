"""The volume following the camera through the system surface (alva_system_set_mesh_follow, alva_system_mesh_move,
alva_system_mesh_follow_stats; AlvaAR(depth=True, mesh_follow=block).meshUpdate / meshMove / meshFollowStats) on the stream of
tests/test_gpu_mesh_system.py at rel_extent 1 with a block of 2 voxels, where the camera's swing shifts the volume many times
(tests/test_mesh_shift_cases.py counts them on the analytic poses): every update equals the restated shift by the call's own shift and
then alva_mesh_integrate replayed on the test's copy -- the colour volume too, with mesh colour on --, the shift is the restated rule's,
the origin is origin0 + offset voxel bit for bit, mesh(), meshDepth(), meshRaycast() and meshColorAt() equal the stages on the copy
with the new origin, meshMove, the offset's life, and that a session that follows tracks bit for bit like one that never asks."""
from __future__ import annotations

import numpy as np
import pytest

import mesh_shift_cases as Sc
import sysdiff
import test_gpu_mesh_raycast_system as Rs
import test_gpu_mesh_system as Ms
from alvaar_amd import synth

pytestmark = pytest.mark.gpu

W, H, CELL = Ms.W, Ms.H, Ms.CELL
N_TRACK, N_BLACK = Ms.N_TRACK, Ms.N_BLACK
STEP, RES, EVERY = Ms.STEP, Sc.STREAM_RES, Sc.STREAM_EVERY
EXTENT, BLOCK = Sc.STREAM_EXTENT, Sc.STREAM_BLOCK
KW = dict(resolution=RES, rel_extent=EXTENT, step=STEP)
CAPS = Ms.CAPS
CSTEP = 4
assert (Ms.SPEED, Ms.RES, Ms.EVERY, Ms.N_TRACK) == (Sc.STREAM_SPEED, RES, EVERY, Sc.STREAM_TRACKED)


@pytest.fixture(scope="module")
def frames():
    import torch
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    black = np.zeros((H, W, 4), np.uint8) + np.array([0, 0, 0, 255], np.uint8)
    return torch.from_numpy(np.stack([black if v is None else synth.plane_stream_frame(canvas, v, W, H, f) for v in Ms._views()])).cuda()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Copy:
    """the test's own copy of the volumes: the restated shift by the call's shift, then the integration stage replayed on what the debug
    calls handed back"""

    def __init__(self, ctx, ar, color):
        self.ctx, self.ar, self.color, self.q, self.w, self.c, self.geo = ctx, ar, color, None, None, None, None
        self.origin0, self.offset, self.lost = None, np.zeros(3, np.int64), 0

    def replay(self, info, frame, state, stats):
        """-> the list of what differs from the system's answers"""
        import torch
        if info["status"] != 0:
            return [] if info["shifted"] == 0 and not info["shift"].any() else ["shifted without integrating"]
        n = info["resolution"]
        bad = []
        if info["placed"]:
            self.q, self.w = torch.zeros((n, n, n), dtype=torch.int16, device="cuda"), torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
            self.c = torch.zeros((n, n, n, 4), dtype=torch.uint8, device="cuda")
            self.origin0, self.offset, self.lost = info["origin"].copy(), np.zeros(3, np.int64), 0
            self.voxel = info["voxel"]
            if info["shifted"]:
                bad.append("placed and shifted")
        if info["shifted"] != int(info["shift"].any()):
            bad.append("shifted flag")
        if info["shifted"]:   # the restatement, on the host, by the call's own shift
            q, w, c, sinfo = Sc.shift(self.q.cpu().numpy(), self.w.cpu().numpy(), self.c.cpu().numpy() if self.color else None, info["shift"])
            self.q, self.w = _dev(q), _dev(w)
            if self.color:
                self.c = _dev(c)
            self.offset = self.offset + info["shift"]
            self.lost += int(sinfo[2])
        # origin0 + offset voxel, bit for bit, and a voxel that never changes
        if not np.array_equal(info["origin"].view(np.uint64), Sc.follow_origin(self.origin0, self.offset, self.voxel).view(np.uint64)):
            bad.append("origin")
        if info["voxel"] != self.voxel or info["trunc"] != 3.0 * self.voxel:
            bad.append("voxel")
        if stats["offset"].tolist() != self.offset.tolist() or stats["lost"] != self.lost or stats["block"] != BLOCK:
            bad.append("stats")
        self.geo = (info["origin"], info["voxel"], info["trunc"])
        raw = tuple(_dev(a) for a in info["raw"])
        if self.color:
            thumb, c_sys, flags = state
            th = self.ctx.color_thumb(frame, CSTEP)
            if not np.array_equal(th.cpu().numpy(), thumb) or flags != 3:
                bad.append("thumb")
            got = self.ctx.mesh_integrate_color(self.q, self.w, self.c, info["origin"], info["voxel"], info["trunc"], info["T_cw"],
                                                Ms._calib8(self.ar.intrinsics), W, H, STEP, raw, th, CSTEP, w_max=128)
            if not np.array_equal(self.c.cpu().numpy(), c_sys):
                bad.append("c")
            if info["colored"] != got[6] or info["color_fused"] != 1:
                bad.append("colored")
        else:
            got = self.ctx.mesh_integrate(self.q, self.w, info["origin"], info["voxel"], info["trunc"], info["T_cw"], Ms._calib8(self.ar.intrinsics),
                                          W, H, STEP, raw, w_max=128)
        if not np.array_equal(self.q.cpu().numpy(), info["q"]):
            bad.append("q")
        if not np.array_equal(self.w.cpu().numpy(), info["w"]):
            bad.append("w")
        if got[:5].tolist() != [info[k] for k in ("updated", "hidden", "free", "outside", "no_depth")] or info["count"] != got[0]:
            bad.append("info")
        return bad

    def consumers(self, ar, pose):
        """mesh(), meshDepth(), meshRaycast() and meshColorAt() against the stages on the copy with the copy's origin"""
        bad = []
        origin, voxel = self.geo[0], self.geo[1]
        if not Ms._same_mesh(ar.mesh(**CAPS), self.ctx.mesh_extract(self.q, self.w, origin, voxel, 2, CAPS["max_vertices"], CAPS["max_triangles"])):
            bad.append("mesh")
        T = Rs._T_wc(pose)
        calib8 = Ms._calib8(ar.intrinsics)
        want = self.ctx.mesh_raycast_pixels(self.q, self.w, origin, voxel, 2, T, calib8, W, H, STEP, None)
        bad += ["depth " + k for k in Rs._depth_differs(ar.meshDepth(step=STEP), want, H // STEP, W // STEP)]
        rays = Rs._world_rays((origin, voxel), pose[:3])
        t, p, nrm, codes, rinfo = ar.meshRaycast(rays)
        ref = self.ctx.mesh_raycast(self.q, self.w, origin, voxel, 2, _dev(rays))
        if not (Rs._same(t, ref["t"]) and Rs._same(p, ref["point"]) and Rs._same(nrm, ref["normal"]) and Rs._same(codes, ref["code"])):
            bad.append("rays")
        hits = int((codes == 0).sum())
        if self.color:
            rgba, ccodes, cinfo = ar.meshColorAt(p)
            s_rgba, s_codes, s_info = self.ctx.mesh_color_at(self.c, origin, voxel, _dev(p))
            if not (np.array_equal(rgba, s_rgba) and np.array_equal(ccodes, s_codes) and np.array_equal(cinfo, s_info)):
                bad.append("color_at")
        return bad, hits


def _expected_shift(info_before, pose):
    """V1 - V3 restated on the session's own pose and the volume's geometry before the call.  At rel_extent 1 the placement's m0 is the
    side, and the side is voxel x 32 exactly"""
    side = info_before["voxel"] * RES
    T = Rs._T_wc(pose)
    target = Sc.follow_target(T[9:], T[:9], side / EXTENT)
    return Sc.follow_shift(target, info_before["origin"], side, info_before["voxel"], BLOCK)


@pytest.fixture(scope="module")
def runs(ctx, frames):
    """the same frames through three sessions that all ask for depthImage and depthDense after every frame: two that follow -- without and
    with mesh colour -- and ask for meshUpdate and the volume's consumers on every fifth frame, one that never calls the mesh"""
    from alvaar_amd.system import AlvaAR
    out = {}
    for name in ("follow", "color", "never"):
        ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, relocalization=True, depth=True, mesh_color=name == "color",
                    mesh_follow=0 if name == "never" else BLOCK)
        copy = _Copy(ctx, ar, name == "color")
        rec, calls, last = [], [], None
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
            raw = ar.depthImage(step=STEP)
            dense = ar.depthDense(step=STEP, max_level=5)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [a.copy() for a in raw[:3]], [a.copy() for a in dense[:4]]))
            if name != "never" and (k % EVERY == 0 or k >= N_TRACK + N_BLACK):   # (after the black frames on every frame)
                pose = ar.pose7()[0].copy()
                info = ar.meshUpdate(debug=True, **KW)
                stats = ar.meshFollowStats()
                state = ar.mesh_color_state(RES) if name == "color" else None
                c = dict(frame=k, tracker=st, info=info, stats=stats, bad=copy.replay(info, frames[k], state, stats))
                if info["status"] == 0:
                    if last is not None:
                        c["want_shift"] = _expected_shift(last, pose)
                    c["consumers"], c["hits"] = copy.consumers(ar, pose)
                    last = info
                calls.append(c)
        out[name] = dict(rec=rec, calls=calls)
        ar.close()
    return out


@pytest.mark.parametrize("name", ["follow", "color"])
def test_every_update_equals_the_restated_shift_then_the_stage_replayed(runs, name):
    calls = runs[name]["calls"]
    done = [c for c in calls if c["info"]["status"] == 0]
    assert len(done) >= 10 and done[0]["info"]["placed"] == 1 and all(c["info"]["placed"] == 0 for c in done[1:])
    shifted = [c for c in done if c["info"]["shifted"]]
    print(name, "placed at frame", done[0]["frame"], "shifts", [(c["frame"], c["info"]["shift"].tolist()) for c in shifted], "lost",
          done[-1]["stats"]["lost"])
    assert len(shifted) >= 3
    for c in calls:
        assert c["bad"] == [], (c["frame"], c["bad"])
    for c in done:
        assert c["consumers"] == [], (c["frame"], c["consumers"])
        if "want_shift" in c:                                   # the rule, restated on the session's own pose
            assert tuple(c["info"]["shift"].tolist()) == c["want_shift"], c["frame"]
        assert all(v % BLOCK == 0 for v in c["info"]["shift"])
    assert sum(c["hits"] for c in shifted) > 0                  # the rays met a surface in shifted volumes
    total = np.sum([c["info"]["shift"] for c in shifted], axis=0)
    assert np.abs(total).max() >= 3 * BLOCK and done[-1]["stats"]["offset"].tolist() == total.tolist()
    assert done[-1]["stats"]["shifts"] == len(shifted)
    # the volume moved: the last origin is not the placement's, by whole voxels
    assert not np.array_equal(done[-1]["info"]["origin"], done[0]["info"]["origin"])


def test_the_lost_episode_keeps_the_offset(runs):
    calls = runs["follow"]["calls"]
    lost = [c for c in calls if c["tracker"] == 4]
    assert lost
    k0 = calls.index(lost[0])
    kept = calls[max(k for k in range(k0) if calls[k]["info"]["status"] == 0)]
    assert kept["stats"]["shifts"] >= 3
    for c in lost:
        assert c["info"]["status"] == 6 and c["info"]["shifted"] == 0 and not c["info"]["shift"].any()
        assert c["stats"]["offset"].tolist() == kept["stats"]["offset"].tolist() and c["stats"]["shifts"] == kept["stats"]["shifts"]
        assert np.array_equal(c["info"]["origin"], kept["info"]["origin"])
    after = next(c for c in calls[k0:] if c["info"]["status"] == 0)
    assert after["info"]["placed"] == 0 and after["info"]["frames"] == kept["info"]["frames"] + 1


def test_following_changes_nothing_else(runs):
    b = runs["never"]["rec"]
    assert 1 in [r[0] for r in b] and 4 in [r[0] for r in b]
    for name in ("follow", "color"):
        a = runs[name]["rec"]
        assert len(a) == len(b)
        answered = 0
        for k, (ra, rb) in enumerate(zip(a, b)):
            assert ra[0] == rb[0], k
            assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), k
            for x, y in zip(ra[3] + ra[4], rb[3] + rb[4]):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
            answered += bool((ra[3][2] == 0).any())
        assert answered > 40


def _centre(info):
    return info["origin"] + info["voxel"] * RES / 2


def _zero_stats(ar, block=0):
    st = ar.meshFollowStats()
    return st["block"] == block and st["shifts"] == 0 and not st["offset"].any() and st["lost"] == 0


def test_follow_off_keeps_the_placement_and_move_moves_it(ctx, frames):
    """one session with mesh_follow = 0: the placement stays where it is, update after update (the assertions of
    tests/test_gpu_mesh_system.py, restated), and alva_system_mesh_move moves it when the app says so"""
    from alvaar_amd.system import AlvaAR, AlvaError
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True)
    fd = Ms._Feeder(ar, frames)
    assert _zero_stats(ar)
    none = ar.meshMove((0.0, 0.0, 0.0))
    assert none["status"] == 5 and none["shifted"] == 0 and not none["shift"].any() and none["resolution"] == 0 and _zero_stats(ar)
    first, _ = fd.until_integrated(0, rel_extent=EXTENT)
    assert first["placed"] == 1 and first["shifted"] == 0
    infos = [first]
    for _ in range(16):
        fd.feed()
        infos.append(ar.meshUpdate(debug=True, **KW))
    done = [i for i in infos if i["status"] == 0]
    assert len(done) >= 8 and [i["frames"] for i in done] == list(range(1, len(done) + 1))
    for i in done:
        assert i["shifted"] == 0 and not i["shift"].any() and (i["placed"] == 1) == (i is first)
        assert np.array_equal(i["origin"], first["origin"]) and i["voxel"] == first["voxel"] and i["trunc"] == 3.0 * i["voxel"]
    assert _zero_stats(ar)
    for bad_block in (0, 3, 64, -8):
        with pytest.raises(AlvaError, match="bad argument"):
            ar.meshMove(_centre(first), block=bad_block)
    with pytest.raises(AlvaError, match="bad argument"):
        ar.setMeshFollow(3)
    # the copy: the last debug call's volume
    last = done[-1]
    q, w, voxel = last["q"], last["w"], last["voxel"]
    weighted = int((w > 0).sum())
    assert weighted > 0
    # to the current centre, to less than a block from it, to a point that is not finite: 0, and nothing is launched
    for c in (_centre(last), _centre(last) + 7.9 * voxel, _centre(last) - np.array([0.0, 7.9, 0.0]) * voxel, (np.nan, 0.0, np.inf)):
        r = ar.meshMove(c, block=8)
        assert r["shifted"] == 0 and r["status"] == 0 and not r["shift"].any() and r["copied"] == r["kept"] == r["lost"] == 0
        assert r["resolution"] == RES and np.array_equal(r["origin"], last["origin"]) and _zero_stats(ar)
    # by one block of 8 along x (the eight-voxel path), 3 along -z on top of it (the one-voxel path): the restated shift of the copy
    offset, lost_sum = np.zeros(3, np.int64), 0
    for c, block, s in ((_centre(last) + np.array([8.5, 0.0, 0.0]) * voxel, 8, (8, 0, 0)),
                        (_centre(last) + np.array([8.0, 0.5, -3.2]) * voxel, 1, (0, 0, -3))):
        r = ar.meshMove(c, block=block)
        q, w, _, sinfo = Sc.shift(q, w, None, s)
        offset += np.array(s)
        lost_sum += int(sinfo[2])
        assert r["shifted"] == 1 and r["status"] == 0 and tuple(r["shift"].tolist()) == s
        assert [r["copied"], r["kept"], r["lost"], r["colored"]] == sinfo[:4].tolist() and r["resolution"] == RES
        origin = Sc.follow_origin(first["origin"], offset, voxel)
        assert np.array_equal(r["origin"].view(np.uint64), origin.view(np.uint64)) and r["voxel"] == voxel
        st = ar.meshFollowStats()
        assert st["offset"].tolist() == offset.tolist() and st["lost"] == lost_sum and st["block"] == 0
        assert Ms._same_mesh(ar.mesh(**CAPS), ctx.mesh_extract(_dev(q), _dev(w), origin, voxel, 2, CAPS["max_vertices"], CAPS["max_triangles"]))
    assert st["shifts"] == 2
    # the next update integrates into the moved volume, where it lies now (follow is off: it does not move it back)
    fd.feed()
    nxt = ar.meshUpdate(debug=True, **KW)
    assert nxt["status"] == 0 and nxt["placed"] == 0 and nxt["shifted"] == 0 and np.array_equal(nxt["origin"], origin)
    dq, dw = _dev(q), _dev(w)
    ctx.mesh_integrate(dq, dw, origin, voxel, nxt["trunc"], nxt["T_cw"], Ms._calib8(ar.intrinsics), W, H, STEP, tuple(_dev(a) for a in nxt["raw"]),
                       w_max=128)
    assert np.array_equal(dq.cpu().numpy(), nxt["q"]) and np.array_equal(dw.cpu().numpy(), nxt["w"])
    # far away: the volume is emptied, the loss is reported, the tallies add up
    weighted = int((nxt["w"] > 0).sum())
    far = ar.meshMove(_centre(nxt) + 1000.0 * voxel * RES, block=4)
    assert far["shifted"] == 1 and far["copied"] == 0 and far["kept"] == 0 and far["lost"] == weighted > 0
    assert all(v % 4 == 0 and v >= RES for v in far["shift"])
    st2 = ar.meshFollowStats()
    assert st2["shifts"] == 3 and st2["lost"] == lost_sum + weighted and st2["offset"].tolist() == (offset + far["shift"]).tolist()
    assert np.array_equal(far["origin"].view(np.uint64), Sc.follow_origin(first["origin"], st2["offset"], voxel).view(np.uint64))
    m = ar.mesh(**CAPS)[3]
    assert m["status"] == 1 and m["valid"] == 0                    # a volume, and nothing in it
    # absurdly far: the shift is limited, nothing overflows
    absurd = ar.meshMove((1e300, -1e300, _centre(far)[2]), block=32)
    assert absurd["shifted"] == 1 and absurd["shift"].tolist() == [1 << 24, -(1 << 24), 0] and absurd["lost"] == 0
    ar.close()


def _coloured_update(ar, fd, limit=100, start=None, **kw):
    """feeds frames, asking for a debug update after each, until one integrates with colour -> that call's info"""
    for n in range(limit):
        fd.feed(start if n == 0 else None)
        info = ar.meshUpdate(debug=True, **dict(KW, **kw))
        if info["status"] == 0 and info["color_fused"] == 1:
            return info
    raise AssertionError("no coloured update within %d frames" % limit)


def _move_differs(ctx, ar, fd, frames, info, by, block, **kw):
    """The session's volume moved by `by` voxels right after the debug update `info` integrated, against alva_mesh_shift on the copies
    taken just before the move: the call's info, the colour volume, the distance volume's surface -- and the distance volume itself, as
    the next update hands it back, against the integration replayed on the shifted copies -> the list of what differs"""
    res, voxel = info["resolution"], info["voxel"]
    q, w = _dev(info["q"]), _dev(info["w"])
    c_before, flags = ar.mesh_color_state(res)[1:]
    assert flags & 2 and c_before.any()
    r = ar.meshMove(info["origin"] + voxel * res / 2 + np.asarray(by, np.float64) * voxel, block=block)
    q2, w2, c2, sinfo = ctx.mesh_shift(q, w, r["shift"], _dev(c_before))
    bad = []
    if r["shifted"] != 1 or r["shift"].tolist() != [block * int(v / block) for v in by]:
        bad.append("shift")
    if [r["copied"], r["kept"], r["lost"], r["colored"], r["resolution"]] != sinfo[[0, 1, 2, 3, 7]].tolist() or r["status"] != 0:
        bad.append("info")
    if sinfo[1] == 0 or sinfo[3] == 0:
        bad.append("nothing weighted or coloured was copied")
    c_after, flags = ar.mesh_color_state(res)[1:]
    if not np.array_equal(c_after, c2.cpu().numpy()) or not flags & 2:
        bad.append("c")
    if not Ms._same_mesh(ar.mesh(**CAPS), ctx.mesh_extract(q2, w2, r["origin"], voxel, 2, CAPS["max_vertices"], CAPS["max_triangles"])):
        bad.append("mesh")
    nxt = _coloured_update(ar, fd, limit=10, **kw)
    if nxt["placed"] or nxt["shifted"] or not np.array_equal(nxt["origin"], r["origin"]):
        bad.append("next update")
    ctx.mesh_integrate_color(q2, w2, c2, nxt["origin"], voxel, nxt["trunc"], nxt["T_cw"], Ms._calib8(ar.intrinsics), W, H, STEP,
                             tuple(_dev(a) for a in nxt["raw"]), ctx.color_thumb(frames[fd.k - 1], CSTEP), CSTEP, w_max=128)
    if not np.array_equal(q2.cpu().numpy(), nxt["q"]) or not np.array_equal(w2.cpu().numpy(), nxt["w"]):
        bad.append("q, w after the next update")
    if not np.array_equal(c2.cpu().numpy(), ar.mesh_color_state(res)[1]):
        bad.append("c after the next update")
    return bad, nxt


def test_the_volume_and_its_colours_move_together_across_a_resolution_change(ctx, frames):
    """Mesh colour on: a move at resolution 32 makes the second volume block and the second colour block; the volume is then placed
    anew at resolution 64, where the next move finds both second blocks made for another resolution"""
    from alvaar_amd.system import AlvaAR
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True, mesh_color=True)
    fd = Ms._Feeder(ar, frames)
    info = _coloured_update(ar, fd, start=0)
    assert info["placed"] == 1 and info["resolution"] == RES
    bad, _ = _move_differs(ctx, ar, fd, frames, info, (8.5, 0.0, 0.0), 8)
    assert bad == []
    info = _coloured_update(ar, fd, limit=10, resolution=64)
    assert info["placed"] == 1 and info["resolution"] == 64 and info["frames"] == 1
    bad, nxt = _move_differs(ctx, ar, fd, frames, info, (0.0, -8.5, 8.5), 8, resolution=64)
    assert bad == [] and nxt["resolution"] == 64 and nxt["frames"] == 2
    ar.close()


def test_colour_dropped_and_brought_back_after_a_move(ctx, frames):
    """Mesh colour on, a move (both colour blocks exist), colour off (both go, and the thumbnail), colour on: the colours start over on
    the volume that is there, and the next move makes the second colour block again"""
    from alvaar_amd.system import AlvaAR, AlvaError
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True, mesh_color=True)
    fd = Ms._Feeder(ar, frames)
    info = _coloured_update(ar, fd, start=0)
    bad, nxt = _move_differs(ctx, ar, fd, frames, info, (8.5, 0.0, 0.0), 8)
    assert bad == []
    probe = (nxt["origin"] + nxt["voxel"] * RES / 2).astype(np.float32).reshape(1, 3)
    assert ar.meshColorAt(probe)[1][0] != 5
    ar.setMeshColor(False)
    with pytest.raises(AlvaError, match="alva_system_set_mesh_color"):
        ar.meshColorAt(probe)
    ar.setMeshColor(True)
    assert ar.meshColorAt(probe)[1][0] == 5            # a volume, but no colour volume yet
    info = _coloured_update(ar, fd, limit=10)
    assert info["placed"] == 0 and info["frames"] == nxt["frames"] + 1 and np.array_equal(info["origin"], nxt["origin"])
    c = ar.mesh_color_state(RES)[1]
    assert (c[..., 3] > 0).sum() == info["colored"] > 0  # the colours started over: only this update's
    bad, _ = _move_differs(ctx, ar, fd, frames, info, (0.0, 0.0, -8.5), 8)
    assert bad == []
    ar.close()


def test_every_listed_reset_clears_the_offset(frames):
    from alvaar_amd.system import AlvaAR, lib
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True, mesh_follow=4)
    fd = Ms._Feeder(ar, frames)
    black = N_TRACK

    def placed_then_moved(start=None, limit=100, **kw):
        """a fresh placement (offset zero from the start), then a move that gives it an offset"""
        info, _ = fd.until_integrated(start, limit=limit, **dict(dict(rel_extent=EXTENT), **kw))
        assert info["placed"] == 1 and info["shifted"] == 0 and _zero_stats(ar, 4)
        n = info["resolution"]
        r = ar.meshMove(info["origin"] + info["voxel"] * n / 2 + np.array([0.0, 4.5, -8.5]) * info["voxel"], block=4)
        assert r["shifted"] == 1 and r["shift"].tolist() == [0, 4, -8]
        st = ar.meshFollowStats()
        assert st["offset"].tolist() == [0, 4, -8] and st["shifts"] == 1 and st["block"] == 4

    assert _zero_stats(ar, 4)
    placed_then_moved(0)
    ar.resetMesh()                                                  # alva_system_reset_mesh
    assert _zero_stats(ar, 4) and ar.mesh(**CAPS)[3]["status"] == 5
    placed_then_moved(limit=5)
    placed_then_moved(limit=5, resolution=64)                       # a changed resolution: placed anew by the call itself
    placed_then_moved(limit=5, rel_extent=3.0)                      # a changed extent
    ar.setMeshFollow(8)                                             # the switch itself touches nothing
    st = ar.meshFollowStats()
    assert st["block"] == 8 and st["offset"].tolist() == [0, 4, -8] and st["shifts"] == 1
    ar.setMeshFollow(4)
    ar.set_depth(False)                                             # depth off
    assert _zero_stats(ar, 4)
    ar.set_depth(True)
    placed_then_moved()
    ar.reset()                                                      # alva_system_reset
    assert _zero_stats(ar, 4)
    placed_then_moved(0)
    for j in range(N_BLACK):                                        # a new map: without relocalization the tracker starts over
        fd.feed(black + j)
    placed_then_moved(0)
    k = ar.intrinsics                                               # configure: the offset goes, the switch stays
    assert lib.alva_system_configure_ex(ar.h, W, H, k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"], CELL, 0, 0) == 0
    assert _zero_stats(ar, 4) and ar.mesh(**CAPS)[3]["status"] == 5
    placed_then_moved(0)
    ar.close()
