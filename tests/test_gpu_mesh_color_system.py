"""Mesh colour through the system surface (alva_system_set_mesh_color, alva_system_mesh_colored, alva_system_mesh_color_at;
AlvaAR(depth=True, mesh_color=True)) on the tracking stream of tests/test_gpu_depth_system.py, its channels tinted by a known affine map of
the gray value so that R, G and B differ, with meshUpdate on every fifth frame (and on every frame once the tracker has relocalized):
every coloured update equals alva_color_thumb + alva_mesh_integrate_color replayed on what alva_system_debug_mesh_update and
alva_system_debug_mesh_color hand back, mesh(colors=True) equals mesh() in what they share and alva_mesh_color_at on its own vertices,
meshColorAt on meshRaycast's hit points equals the stage, a session with colour on tracks and answers bit for bit like one with it off,
the four ways a frame can reach the session give the same colour bytes, the colours' life, and the tint relation on the coloured
vertices."""
from __future__ import annotations

import numpy as np
import pytest

import mesh_color_cases as Cc
import sysdiff
from alvaar_amd import synth

pytestmark = pytest.mark.gpu

W, H, CELL = 640, 480, 12
SPEED, N_TRACK, N_BLACK, N_AFTER = 3, 110, 8, 8     # the stream of tests/test_gpu_depth_system.py
RESUME_K = SPEED * 85
STEP, RES, EXTENT, EVERY = 8, 32, 2.0, 5
KW = dict(resolution=RES, rel_extent=EXTENT, step=STEP)
CAPS = dict(max_vertices=1 << 15, max_triangles=1 << 16)
CSTEP = Cc.COLOR_STEP
N_ROUTE = 60                                        # frames of the stream that the route comparison feeds
# the tint: G = G_A + (3 R >> 2), B = B_A + (R >> 1) with R the stream's gray value
G_A, B_A = 16, 40
# The tint relation on the coloured vertices: the largest |g - (G_A + 0.75 r)| and |b - (B_A + 0.5 r)| over the last coloured mesh.  The
# maps are affine and every stage is a weighted mean, so only the roundings (the tint's shifts, T1, K3 per update, A4) separate the
# channels.  Measured on the first GPU run, where the restatement's replay of the same stream gives the same bytes and so the same value;
# the assertion allows it plus one count
TINT_ERR = 1.0


def _views():
    return [SPEED * k for k in range(N_TRACK)] + [None] * N_BLACK + [RESUME_K + SPEED * j for j in range(N_AFTER)]


def _calib8(k):
    return (k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"])


def _tint(frame):
    r = frame[..., 0].astype(np.int32)
    out = frame.copy()
    out[..., 1] = G_A + (3 * r >> 2)
    out[..., 2] = B_A + (r >> 1)
    return out


@pytest.fixture(scope="module")
def frames_np():
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    black = np.zeros((H, W, 4), np.uint8) + np.array([0, 0, 0, 255], np.uint8)
    return np.stack([black if v is None else _tint(synth.plane_stream_frame(canvas, v, W, H, f)) for v in _views()])


@pytest.fixture(scope="module")
def frames(frames_np):
    import torch
    return torch.from_numpy(frames_np).cuda()


class _Copy:
    """the test's own copy of the three volumes: stage 1 and stage 2 replayed on what the debug calls handed back"""

    def __init__(self, ctx, ar):
        self.ctx, self.ar, self.q, self.w, self.c, self.geo = ctx, ar, None, None, None, None

    def replay(self, info, frame, state):
        """-> the list of what differs from the system's answers"""
        import torch
        if info["status"] != 0:
            return []
        thumb, c_sys, flags = state
        n = info["resolution"]
        if info["placed"]:
            self.q = torch.zeros((n, n, n), dtype=torch.int16, device="cuda")
            self.w = torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
            self.c = torch.zeros((n, n, n, 4), dtype=torch.uint8, device="cuda")
        self.geo = (info["origin"], info["voxel"], info["trunc"])
        bad = []
        th = self.ctx.color_thumb(frame, CSTEP)
        if not np.array_equal(th.cpu().numpy(), thumb) or flags != 3:
            bad.append("thumb")
        got = self.ctx.mesh_integrate_color(self.q, self.w, self.c, info["origin"], info["voxel"], info["trunc"], info["T_cw"],
                                            _calib8(self.ar.intrinsics), W, H, STEP, tuple(torch.from_numpy(a).cuda() for a in info["raw"]), th,
                                            CSTEP, w_max=128)
        if not np.array_equal(self.q.cpu().numpy(), info["q"]):
            bad.append("q")
        if not np.array_equal(self.w.cpu().numpy(), info["w"]):
            bad.append("w")
        if not np.array_equal(self.c.cpu().numpy(), c_sys):
            bad.append("c")
        if got[:5].tolist() != [info[k] for k in ("updated", "hidden", "free", "outside", "no_depth")] or info["count"] != got[0]:
            bad.append("info")
        if info["colored"] != got[6] or info["color_fused"] != 1:
            bad.append("colored")
        return bad


@pytest.fixture(scope="module")
def runs(ctx, frames):
    """the same frames through two sessions that both ask for depthImage, depthDense after every frame and meshUpdate, mesh and meshDepth
    on every fifth: one with mesh colour on, which also asks for the colours, one with it off"""
    from alvaar_amd.system import AlvaAR
    out = {}
    for name in ("on", "off"):
        ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, relocalization=True, depth=True, mesh_color=name == "on")
        copy = _Copy(ctx, ar)
        rec, calls = [], []
        before = ar.meshColorAt(np.zeros((3, 3), np.float32)) if name == "on" else None
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
            raw = ar.depthImage(step=STEP)
            dense = ar.depthDense(step=STEP, max_level=5)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [a.copy() for a in raw[:3]], [a.copy() for a in dense[:4]]))
            if k % EVERY == 0 or k >= N_TRACK + N_BLACK:   # (after the black frames on every frame)
                info = ar.meshUpdate(debug=True, **KW)
                m = ar.mesh(**CAPS)
                md = ar.meshDepth(step=STEP)
                c = dict(frame=k, tracker=st, info=info, mesh=m, mesh_depth=md)
                if name == "on":
                    state = ar.mesh_color_state(RES)
                    c.update(state=state, bad=copy.replay(info, frames[k], state), colored=ar.mesh(colors=True, **CAPS))
                    if copy.c is not None:
                        c["copy_c"] = copy.c.cpu().numpy()
                        # rays down the optical axes of a grid of pixels of the current pose: meshRaycast's points, then their colours
                        t, p, nrm, codes, rinfo = ar.meshRaycast(_rays(ar), min_weight=2)
                        c.update(ray_points=p.copy(), ray_codes=codes.copy(), ray_colors=ar.meshColorAt(p))
                calls.append(c)
        out[name] = dict(rec=rec, calls=calls, before=before)
        ar.close()
    return out


def _rays(ar):
    """world rays through a 12 x 9 grid of pixels of the session's current pose (no distortion in this stream)"""
    k = ar.intrinsics
    pose = ar.pose7()[0]
    R, t = sysdiff._quat_to_rot(pose[3:]), pose[:3]
    u, v = np.meshgrid(np.linspace(20, W - 20, 12), np.linspace(20, H - 20, 9))
    d = np.stack([(u.ravel() - k["cx"]) / k["fx"], (v.ravel() - k["cy"]) / k["fy"], np.ones(u.size)], 1) @ R.T
    return np.concatenate([np.broadcast_to(t, d.shape), d], 1)


def test_every_coloured_update_equals_the_stages_replayed(runs):
    calls = runs["on"]["calls"]
    done = [c for c in calls if c["info"]["status"] == 0]
    assert len(done) >= 10 and done[0]["info"]["placed"] == 1
    for c in calls:
        assert c["bad"] == [], (c["frame"], c["bad"])
        if c["info"]["status"] != 0:
            assert c["info"]["colored"] == 0 and c["info"]["color_fused"] == 0
    assert all(c["info"]["colored"] > 0 for c in done)
    # the restatement on one update's hand-over: the volume before is the update before's
    a, b = done[3], done[4]
    r = Cc.integrate_color(a["info"]["q"], a["info"]["w"], a["state"][1], b["info"]["origin"], b["info"]["voxel"], b["info"]["trunc"], b["info"]["T_cw"],
                           _calib8(_intrinsics()), W, H, STEP, b["info"]["raw"], b["state"][0], CSTEP)
    assert np.array_equal(r["q"], b["info"]["q"]) and np.array_equal(r["w"], b["info"]["w"]) and np.array_equal(r["c"], b["state"][1])
    assert r["info"][6] == b["info"]["colored"]


def _intrinsics():
    from alvaar_amd.system import camera_intrinsics
    return camera_intrinsics(W, H)


def test_restated_thumbnail_of_a_tracked_frame(runs, frames_np):
    c = [c for c in runs["on"]["calls"] if c["info"]["status"] == 0][5]
    assert np.array_equal(Cc.thumb(frames_np[c["frame"]], CSTEP), c["state"][0])


def test_colored_mesh_is_the_mesh_and_the_stage_on_its_vertices(ctx, runs):
    import torch
    calls = [c for c in runs["on"]["calls"] if "copy_c" in c]
    assert len(calls) >= 10
    with_colour = 0
    for c in calls:
        v, n, t, info = c["mesh"]
        cv, cn, col, ct, cinfo = c["colored"]
        assert np.array_equal(v.view(np.uint32), cv.view(np.uint32)) and np.array_equal(n.view(np.uint32), cn.view(np.uint32)) and np.array_equal(t, ct)
        assert {k: cinfo[k] for k in info if k not in ("origin",)} == {k: info[k] for k in info if k not in ("origin",)}
        assert col.dtype == np.uint8 and col.shape == (len(v), 4)
        if len(v) == 0:
            continue
        geo = c["info"]
        rgba, codes, sinfo = ctx.mesh_color_at(torch.from_numpy(c["copy_c"]).cuda(), geo["origin"], geo["voxel"], torch.from_numpy(cv).cuda())
        assert np.array_equal(col, rgba), c["frame"]
        assert cinfo["colored"] == sinfo[1] == int((col[:, 3] == 255).sum())
        assert np.all((col[:, 3] == 255) | (col == 0).all(1))
        with_colour += cinfo["colored"] > 0
    assert with_colour >= 8
    # and the restatement on the last one
    c = calls[-1]
    want = Cc.color_at(c["copy_c"], c["info"]["origin"], c["info"]["voxel"], c["colored"][0])
    assert np.array_equal(want["rgba"], c["colored"][2])


def test_color_at_on_the_raycasts_hit_points_equals_the_stage(ctx, runs):
    import torch
    calls = [c for c in runs["on"]["calls"] if "ray_points" in c]
    hits = 0
    for c in calls:
        rgba, codes, info = c["ray_colors"]
        geo = c["info"]
        want = ctx.mesh_color_at(torch.from_numpy(c["copy_c"]).cuda(), geo["origin"], geo["voxel"], torch.from_numpy(c["ray_points"]).cuda())
        assert np.array_equal(rgba, want[0]) and np.array_equal(codes, want[1]) and np.array_equal(info, want[2]), c["frame"]
        hit = c["ray_codes"] == 0
        hits += int((hit & (codes == 0)).sum())
    assert hits > 200                                  # hit points with a colour
    before = runs["on"]["before"]                      # no volume yet: code 5 for every point, nothing launched
    assert np.all(before[1] == 5) and not before[0].any() and before[2].tolist() == [3, 0, 0, 0, 0, 0, 0, 0]


def test_colour_changes_nothing_else(runs):
    a, b = runs["on"], runs["off"]
    assert len(a["rec"]) == len(b["rec"]) and 1 in [r[0] for r in b["rec"]] and 4 in [r[0] for r in b["rec"]]
    for k, (ra, rb) in enumerate(zip(a["rec"], b["rec"])):
        assert ra[0] == rb[0], k
        assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), k
        for x, y in zip(ra[3] + ra[4], rb[3] + rb[4]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
    assert len(a["calls"]) == len(b["calls"])
    integrated = 0
    for ca, cb in zip(a["calls"], b["calls"]):
        ia, ib = ca["info"], cb["info"]
        assert ia["status"] == ib["status"], ca["frame"]
        assert cb["info"]["colored"] == 0 and cb["info"]["color_fused"] == 0
        for key in ("updated", "hidden", "free", "outside", "no_depth", "resolution", "swept", "frames", "placed", "count"):
            assert ia[key] == ib[key], (ca["frame"], key)
        if ia["status"] == 0:
            integrated += 1
            assert np.array_equal(ia["q"], ib["q"]) and np.array_equal(ia["w"], ib["w"]), ca["frame"]
        for x, y in zip(ca["mesh"][:3] + ca["mesh_depth"][:3], cb["mesh"][:3] + cb["mesh_depth"][:3]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), ca["frame"]
    assert integrated >= 10


def test_the_colours_across_a_lost_episode(runs):
    calls = runs["on"]["calls"]
    lost = [c for c in calls if c["tracker"] == 4]
    assert lost
    k0 = calls.index(lost[0])
    kb = max(k for k in range(k0) if calls[k]["info"]["status"] == 0)
    kept = calls[kb]
    for c in calls[kb + 1:k0] + lost:                  # kept: the same colour bytes, the same coloured mesh, while nothing is fused
        assert c["info"]["status"] == 6 and c["info"]["color_fused"] == 0
        assert np.array_equal(c["state"][1], kept["state"][1]) and c["state"][2] & 2
        assert np.array_equal(c["colored"][2], kept["colored"][2])
    assert not lost[-1]["state"][2] & 1                # the kept thumbnail is an earlier frame's: a LOST frame takes none
    after = next(c for c in calls[k0:] if c["info"]["status"] == 0)
    assert after["info"]["placed"] == 0 and after["info"]["color_fused"] == 1 and after["bad"] == []


def test_the_coloured_vertices_keep_the_tint(runs):
    c = [c for c in runs["on"]["calls"] if c["info"]["status"] == 0][-1]
    v, n, col, t, info = c["colored"]
    has = col[:, 3] == 255
    assert has.sum() >= 20                             # (the stream's mesh is sparse at this resolution: a few dozen vertices)
    r, g, b = (col[has, k].astype(np.float64) for k in range(3))
    err = max(float(np.abs(g - (G_A + 0.75 * r)).max()), float(np.abs(b - (B_A + 0.5 * r)).max()))
    # the restatement's own value: stage 3 restated on the replayed colour volume at the same vertices
    want = Cc.color_at(c["copy_c"], c["info"]["origin"], c["info"]["voxel"], v)
    wh = want["rgba"][:, 3] == 255
    wr, wg, wb = (want["rgba"][wh, k].astype(np.float64) for k in range(3))
    werr = max(float(np.abs(wg - (G_A + 0.75 * wr)).max()), float(np.abs(wb - (B_A + 0.5 * wr)).max()))
    print("tint relation: coloured vertices %d of %d, largest error %.3f counts (restatement %.3f), r from %d to %d" % (
        has.sum(), len(col), err, werr, r.min(), r.max()))
    assert r.max() - r.min() > 20                      # the relation is tested over a range of values
    assert TINT_ERR is not None, "measure first: the figure above goes into TINT_ERR"
    assert err <= TINT_ERR + 1 and werr <= TINT_ERR + 1


def _feed(ar, route, frames, frames_np, k, ts):
    from alvaar_amd.system import lib
    if route == "host":                                # pageable host memory the session knows nothing about: the pinned staging copy
        st = lib.alva_system_find_camera_pose_ts(ar.h, frames_np[k].ctypes.data, ts, ar._pose_ptr)
    elif route == "wrapper":                           # AlvaAR's own frame buffer: device memory written over the BAR, else its registered buffer
        st = ar.findCameraPose(frames_np[k], ts)[1]
    elif route == "device":
        st = ar.find_camera_pose_device(int(frames[k].data_ptr()), ts)
    else:                                              # device memory with the next-frame hint
        st = ar.find_camera_pose_device(int(frames[k].data_ptr()), ts, int(frames[k + 1].data_ptr()))
    assert st >= 0
    return st


@pytest.mark.parametrize("light", [False, True])
def test_the_same_colour_bytes_whichever_way_the_frame_arrives(frames, frames_np, light):
    """with light off the thumbnail waits for itself; with light on, light's wait covers it"""
    from alvaar_amd.system import AlvaAR
    got = {}
    for route in ("host", "wrapper", "device", "hint"):
        ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True, mesh_color=True, light=light)
        seq = []
        for k in range(N_ROUTE):
            st = _feed(ar, route, frames, frames_np, k, 33.0 * k)
            info = ar.meshUpdate(**KW) if k % EVERY == 0 else None
            thumb, c, flags = ar.mesh_color_state(RES)
            seq.append((st, None if info is None else (info["status"], info["colored"], info["color_fused"]), flags, thumb.tobytes(), c.tobytes()))
        got[route] = seq
        ar.close()
    assert sum(st == 1 for st, *_ in got["device"]) > 20
    assert sum(1 for s in got["device"] if s[1] is not None and s[1][2] == 1) >= 3
    for route in ("host", "wrapper", "hint"):
        diff = [k for k, (a, b) in enumerate(zip(got[route], got["device"])) if a != b]
        assert diff == [], (route, diff[:8])


def test_overwriting_a_device_frame_after_the_call_does_not_reach_the_thumbnail(frames, frames_np):
    import torch
    from alvaar_amd.system import AlvaAR
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True, mesh_color=True)
    buf = frames[0].clone()
    checked = 0
    for k in range(40):
        buf.copy_(frames[k])
        torch.cuda.synchronize()                       # (the copy runs on torch's stream, the session on its own)
        st = ar.find_camera_pose_device(int(buf.data_ptr()), 33.0 * k)
        buf.fill_(77)                                  # the caller reuses its memory at once
        if st == 1:
            thumb, _, flags = ar.mesh_color_state(RES)
            assert flags & 1 and np.array_equal(thumb, Cc.thumb(frames_np[k], CSTEP)), k
            checked += 1
    assert checked > 10
    ar.close()


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

    def until_integrated(self, start=None, limit=100, **kw):
        earlier = []
        for n in range(limit):
            self.feed(start if n == 0 else None)
            info = self.ar.meshUpdate(**dict(KW, **kw))
            if info["status"] == 0:
                return info, earlier
            earlier.append(info["status"])
        raise AssertionError("no update integrated within %d frames: %s" % (limit, earlier))


def test_every_listed_reset_empties_the_colours(frames):
    from alvaar_amd.system import AlvaAR, AlvaError, lib
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True, mesh_color=True)
    fd = _Feeder(ar, frames)
    black = N_TRACK
    probe = np.zeros((4, 3), np.float32)

    def weights(res=RES):
        return ar.mesh_color_state(res)[1][..., 3].astype(np.int64)

    def colours_grow(**kw):
        """the next update adds to the colours that are there"""
        w0 = weights(kw.get("resolution", RES))
        info, _ = fd.until_integrated(limit=5, **kw)
        assert info["placed"] == 0 and info["color_fused"] == 1 and info["colored"] > 0
        w1 = weights(kw.get("resolution", RES))
        assert w0.sum() > 0 and np.all(w1 >= w0) and w1.sum() > w0.sum()

    def fresh(info, res=RES):
        """a placing update: the colours are this update's alone -- every coloured voxel carries one measurement's weight (at most 31)"""
        assert info["placed"] == 1 and info["frames"] == 1 and info["color_fused"] == 1 and info["colored"] > 0
        w = weights(res)
        assert (w > 0).sum() == info["colored"] and w.max() <= 31

    def emptied():
        assert np.all(ar.meshColorAt(probe)[1] == 5) and ar.mesh(colors=True, **CAPS)[4]["status"] == 5

    emptied()
    fresh(fd.until_integrated(0)[0])
    colours_grow()
    # alva_system_reset_mesh
    ar.resetMesh()
    emptied()
    fresh(fd.until_integrated(limit=5)[0])
    colours_grow()
    # a changed resolution, a changed extent: placed anew by the call itself
    fresh(fd.until_integrated(limit=5, resolution=64)[0], 64)
    fresh(fd.until_integrated(limit=5, rel_extent=3.0)[0])
    colours_grow(rel_extent=3.0)
    # colour off: the calls are refused by name, the geometry goes on; on again: the colours start over on the volume that is there
    ar.setMeshColor(False)
    with pytest.raises(AlvaError, match="alva_system_set_mesh_color"):
        ar.meshColorAt(probe)
    with pytest.raises(AlvaError, match="alva_system_set_mesh_color"):
        ar.mesh(colors=True, **CAPS)
    info, _ = fd.until_integrated(limit=5, rel_extent=3.0)
    assert info["placed"] == 0 and info["color_fused"] == 0 and info["colored"] == 0
    ar.setMeshColor(True)
    assert np.all(ar.meshColorAt(probe)[1] == 5)       # a volume, but no colour volume yet
    v, n, col, t, minfo = ar.mesh(colors=True, **CAPS)
    assert minfo["status"] in (0, 1) and minfo["colored"] == 0 and not col.any()
    info = ar.meshUpdate(**dict(KW, rel_extent=3.0))   # the current frame was not reduced (colour was off): geometry only, if at all
    assert info["color_fused"] == 0
    info, _ = fd.until_integrated(limit=5, rel_extent=3.0)
    assert info["placed"] == 0 and info["color_fused"] == 1
    w = weights()
    assert (w > 0).sum() == info["colored"] and w.max() <= 31
    # depth off: the volume goes with the ring, and the colours with the volume
    ar.set_depth(False)
    emptied()
    ar.set_depth(True)
    fresh(fd.until_integrated()[0])
    colours_grow()
    # alva_system_reset
    ar.reset()
    emptied()
    fresh(fd.until_integrated(0)[0])
    colours_grow()
    # a new map: without relocalization the tracker starts over after the black frames
    for j in range(N_BLACK):
        fd.feed(black + j)
    fresh(fd.until_integrated(0)[0])
    # configure
    k = ar.intrinsics
    assert lib.alva_system_configure_ex(ar.h, W, H, k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"], CELL, 0, 0) == 0
    emptied()
    fresh(fd.until_integrated(0)[0])
    ar.close()


def test_with_colour_off_the_new_calls_name_the_switch(frames):
    from alvaar_amd.system import AlvaAR, AlvaError
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True)
    ar.find_camera_pose_device(int(frames[0].data_ptr()), 0.0)
    with pytest.raises(AlvaError, match="alva_system_set_mesh_color"):
        ar.meshColorAt(np.zeros((1, 3), np.float32))
    with pytest.raises(AlvaError, match="alva_system_set_mesh_color"):
        ar.mesh(colors=True, **CAPS)
    with pytest.raises(AlvaError, match="alva_system_set_mesh_color"):
        ar.mesh_color_state(RES)
    assert ar.mesh(**CAPS)[3]["status"] == 5
    ar.close()
    # colour without depth: the switch holds, nothing is kept, and the update is refused as before
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, mesh_color=True)
    for k in range(3):
        ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
    with pytest.raises(AlvaError, match="depth is off"):
        ar.meshUpdate(**KW)
    assert np.all(ar.meshColorAt(np.zeros((1, 3), np.float32))[1] == 5)
    ar.close()
