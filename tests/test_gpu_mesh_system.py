"""The scene mesh through the system surface (alva_system_mesh_update / alva_system_mesh, AlvaAR(depth=True).meshUpdate / mesh) on the
tracking stream of tests/test_gpu_depth_system.py, with meshUpdate on every fifth frame (and on every frame once the tracker has
relocalized, so that the few frames left meet one that integrates): every call's volume equals alva_mesh_integrate
replayed on what alva_system_debug_mesh_update hands back, mesh() equals alva_mesh_extract on that copy, the codes, the volume's life
(kept across a LOST episode, emptied by every reset the header lists), that a session that builds a mesh tracks -- and answers depthImage
and depthDense -- bit for bit like one that never does, and that the mesh lies on the stream's plane."""
from __future__ import annotations

import numpy as np
import pytest

import sysdiff
from alvaar_amd import synth

pytestmark = pytest.mark.gpu

W, H, CELL = 640, 480, 12
SPEED, N_TRACK, N_BLACK, N_AFTER = 3, 110, 8, 8     # the stream of tests/test_gpu_depth_system.py
RESUME_K = SPEED * 85
STEP, RES, EXTENT, EVERY = 8, 32, 2.0, 5
KW = dict(resolution=RES, rel_extent=EXTENT, step=STEP)
CAPS = dict(max_vertices=1 << 15, max_triangles=1 << 16)
PLANE_Z = 4.0                                       # synth.render_plane


def _views():
    return [SPEED * k for k in range(N_TRACK)] + [None] * N_BLACK + [RESUME_K + SPEED * j for j in range(N_AFTER)]


def _calib8(k):
    return (k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"])


@pytest.fixture(scope="module")
def frames():
    import torch
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    black = np.zeros((H, W, 4), np.uint8) + np.array([0, 0, 0, 255], np.uint8)
    return torch.from_numpy(np.stack([black if v is None else synth.plane_stream_frame(canvas, v, W, H, f) for v in _views()])).cuda()


class _Copy:
    """the test's own copy of the volume: alva_mesh_integrate replayed on what the debug call handed back"""

    def __init__(self, ctx, ar):
        self.ctx, self.ar, self.q, self.w, self.geo = ctx, ar, None, None, None

    def replay(self, info):
        """-> the list of what differs from the system call's answer"""
        import torch
        if info["status"] != 0:
            return []
        n = info["resolution"]
        if info["placed"]:
            self.q = torch.zeros((n, n, n), dtype=torch.int16, device="cuda")
            self.w = torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
        self.geo = (info["origin"], info["voxel"], info["trunc"])
        got = self.ctx.mesh_integrate(self.q, self.w, info["origin"], info["voxel"], info["trunc"], info["T_cw"], _calib8(self.ar.intrinsics), W, H,
                                      STEP, tuple(torch.from_numpy(a).cuda() for a in info["raw"]), w_max=128)
        bad = []
        if not np.array_equal(self.q.cpu().numpy(), info["q"]):
            bad.append("q")
        if not np.array_equal(self.w.cpu().numpy(), info["w"]):
            bad.append("w")
        if got[:5].tolist() != [info[k] for k in ("updated", "hidden", "free", "outside", "no_depth")] or info["count"] != got[0]:
            bad.append("info")
        if info["swept"] != int((info["raw"][2] == 0).sum()):
            bad.append("swept")
        return bad

    def extract(self, min_weight=2):
        return self.ctx.mesh_extract(self.q, self.w, self.geo[0], self.geo[1], min_weight, CAPS["max_vertices"], CAPS["max_triangles"])


def _same_mesh(a, b):
    """the system's (vertices, normals, triangles, info dict) against the stage's (vertices, normals, triangles, info8)"""
    return (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            and np.array_equal(a[2], b[2]) and [a[3][k] for k in ("status", "vertices", "triangles", "valid", "inside", "resolution")] == b[3][:6].tolist())


@pytest.fixture(scope="module")
def runs(ctx, frames):
    """the same frames through two sessions that both ask for depthImage and depthDense after every frame: one that calls meshUpdate and
    mesh on every fifth frame, one that never does"""
    from alvaar_amd.system import AlvaAR
    out = {}
    for name in ("mesh", "never"):
        ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, relocalization=True, depth=True)
        copy = _Copy(ctx, ar)
        rec, calls = [], []
        before = ar.mesh(**CAPS)[3]["status"] if name == "mesh" else None
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
            raw = ar.depthImage(step=STEP)
            dense = ar.depthDense(step=STEP, max_level=5)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [a.copy() for a in raw[:3]], [a.copy() for a in dense[:4]]))
            if name == "mesh" and (k % EVERY == 0 or k >= N_TRACK + N_BLACK):   # (after the black frames on every frame)
                info = ar.meshUpdate(debug=True, **KW)
                again = ar.meshUpdate(**KW)
                m = ar.mesh(**CAPS)
                c = dict(frame=k, tracker=st, info=info, again=again, bad=copy.replay(info), mesh=m, pose=ar.pose7()[0].copy())
                if copy.q is not None:
                    c["same_mesh"] = _same_mesh(m, copy.extract())
                calls.append(c)
        out[name] = dict(rec=rec, calls=calls, before=before)
        ar.close()
    return out


def test_every_update_equals_the_stage_replayed_and_the_mesh_the_extraction(runs):
    calls = runs["mesh"]["calls"]
    done = [c for c in calls if c["info"]["status"] == 0]
    assert len(done) >= 10 and done[0]["info"]["placed"] == 1 and all(c["info"]["placed"] == 0 for c in done[1:])
    assert [c["info"]["frames"] for c in done] == list(range(1, len(done) + 1))
    for c in calls:
        assert c["bad"] == [], (c["frame"], c["bad"])
        assert c.get("same_mesh", True), c["frame"]
    for c in done:
        i = c["info"]
        assert i["resolution"] == RES and i["updated"] + i["hidden"] + i["outside"] + i["no_depth"] == RES ** 3 and i["count"] == i["updated"] > 0
        assert i["trunc"] == 3.0 * i["voxel"] and i["voxel"] > 0
        assert np.array_equal(i["origin"], done[0]["info"]["origin"]) and i["voxel"] == done[0]["info"]["voxel"]   # the placement stays
    # T_cw is the inverse of the pose the session answers
    c = done[-1]
    R, t = sysdiff._quat_to_rot(c["pose"][3:]), c["pose"][:3]
    assert np.abs(c["info"]["T_cw"][:9].reshape(3, 3) - R.T).max() < 1e-12 and np.abs(c["info"]["T_cw"][9:] + R.T @ t).max() < 1e-12


def test_codes(runs):
    assert runs["mesh"]["before"] == 5                                            # no volume before the first update
    calls = runs["mesh"]["calls"]
    first = next(k for k, c in enumerate(calls) if c["info"]["status"] == 0)
    for c in calls[:first]:
        assert c["info"]["status"] in (6, 7) and c["info"]["count"] == 0 and c["mesh"][3]["status"] == 5 and c["info"]["resolution"] == 0
    for c in calls:
        if c["info"]["status"] == 0:                                              # a second call on the same frame integrates nothing
            assert c["again"]["status"] == 8 and c["again"]["count"] == 0 and c["again"]["frames"] == c["info"]["frames"]
            assert c["again"]["resolution"] == RES and np.array_equal(c["again"]["origin"], c["info"]["origin"])
        else:
            assert c["again"]["status"] == c["info"]["status"]
    # the black frames: not tracking, and the volume is kept -- mesh() answers the same bytes, and the next update adds to it
    lost = [c for c in calls if c["tracker"] == 4]
    assert lost
    k0 = calls.index(lost[0])
    kb = max(k for k in range(k0) if calls[k]["info"]["status"] == 0)
    kept = calls[kb]
    assert kept["info"]["frames"] >= 10
    for c in calls[kb + 1:k0] + lost:                                             # (the frame that loses the track is not status 4 yet)
        assert c["info"]["status"] == 6 and c["info"]["resolution"] == RES and c["info"]["frames"] == kept["info"]["frames"]
        assert c["mesh"][3]["status"] == 0
        for a, b in zip(c["mesh"][:3], kept["mesh"][:3]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    after = next(c for c in calls[k0:] if c["info"]["status"] == 0)
    assert after["info"]["placed"] == 0 and after["info"]["frames"] == kept["info"]["frames"] + 1


def test_mesh_calls_change_nothing_else(runs):
    a, b = runs["mesh"]["rec"], runs["never"]["rec"]
    assert len(a) == len(b) and 1 in [r[0] for r in b] and 4 in [r[0] for r in b]
    answered = 0
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0] == rb[0], k
        assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), k
        for x, y in zip(ra[3] + ra[4], rb[3] + rb[4]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
        answered += bool((ra[3][2] == 0).any())
    assert answered > 40


def test_the_mesh_lies_on_the_streams_plane(runs):
    calls = runs["mesh"]["calls"]
    c = [c for c in calls if c["info"]["status"] == 0][-1]
    v, n, t, info = c["mesh"]
    assert info["status"] == 0 and len(t) > 0
    used = np.zeros(len(v), bool)
    used[t.reshape(-1)] = True
    # the plane in the camera frame of that view, in the stream's units: n_c . X = d_c
    view = _views()[c["frame"]]
    R_true, t_true = synth.plane_camera_pose(view)
    n_c, d_c = R_true.T @ np.array([0.0, 0.0, 1.0]), PLANE_Z - t_true[2]
    R, tw = sysdiff._quat_to_rot(c["pose"][3:]), c["pose"][:3]
    Xc = (v[used].astype(np.float64) - tw) @ R            # R_wc^T (X - t), row-wise
    h = Xc @ n_c
    scale = float(np.median(h)) / d_c                     # the map's own scale: map units per unit of the stream
    err = np.abs(h - scale * d_c)
    print("frame %d: %d used vertices of %d, %d triangles, scale %.5f, |distance| max %.4f median %.4f map units, trunc %.4f" % (
        c["frame"], used.sum(), len(v), len(t), scale, err.max(), float(np.median(err)), info["trunc"]))
    assert scale > 0 and err.max() <= info["trunc"]


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
        """feeds frames, asking for an update after each, until one integrates -> that call's info and the statuses before it"""
        earlier = []
        for n in range(limit):
            self.feed(start if n == 0 else None)
            info = self.ar.meshUpdate(**dict(KW, **kw))
            if info["status"] == 0:
                return info, earlier
            earlier.append(info["status"])
        raise AssertionError("no update integrated within %d frames: %s" % (limit, earlier))


def test_the_extraction_block_grows_with_the_caps(ctx, frames):
    """One frame, one volume, four extractions: caps too small for the surface (the first call's device block is sized for them), CAPS
    (the block is replaced by a larger one inside the live session), the small caps again, CAPS again."""
    from alvaar_amd.system import AlvaAR, lib
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True)
    fd = _Feeder(ar, frames)
    copy = _Copy(ctx, ar)
    want, log = None, []
    for n in range(100):                              # until the volume has a surface; no extraction by the session before that
        fd.feed(0 if n == 0 else None)
        info = ar.meshUpdate(debug=True, **KW)
        assert copy.replay(info) == []
        log.append(info["status"])
        if info["status"] == 0:
            want = copy.extract()
            log.append(tuple(want[3][:3].tolist()))
            if want[3][0] == 0 and want[3][1] > 8 and want[3][2] > 0:   # more vertices than the small caps hold
                break
    else:
        raise AssertionError("no surface within 100 frames: %s" % log)
    small = dict(max_vertices=8, max_triangles=8)

    def too_small():
        v, nrm, t = np.full((8, 3), 7.5, np.float32), np.full((8, 3), 7.5, np.float32), np.full((8, 3), 77, np.int32)
        i8, geo = np.zeros(8, np.int32), np.zeros(5)
        rc = lib.alva_system_mesh(ar.h, 2, 8, 8, v.ctypes.data, nrm.ctypes.data, t.ctypes.data, i8.ctypes.data, geo.ctypes.data)
        assert rc == 0 and i8[0] == 3 and i8[1:3].tolist() == want[3][1:3].tolist()      # (the counts are the true ones)
        assert (v == 7.5).all() and (nrm == 7.5).all() and (t == 77).all()                # no row is written
        m = ar.mesh(**small)
        assert m[3]["status"] == 3 and len(m[0]) == len(m[1]) == len(m[2]) == 0

    too_small()
    first = ar.mesh(**CAPS)
    too_small()
    second = ar.mesh(**CAPS)
    assert first[3]["status"] == 0 and _same_mesh(first, want) and _same_mesh(second, want)
    for a, b in zip(first[:3], second[:3]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    ar.close()


def test_every_listed_reset_empties_the_volume(frames):
    from alvaar_amd.system import AlvaAR, AlvaError, lib
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True)
    fd = _Feeder(ar, frames)
    black = N_TRACK                                   # the index of the first black frame

    def adds_next():
        info, _ = fd.until_integrated(limit=5)
        assert info["placed"] == 0 and info["frames"] >= 2
        assert ar.mesh(**CAPS)[3]["status"] in (0, 1)

    def emptied():
        assert ar.mesh(**CAPS)[3]["status"] == 5

    emptied()
    info, earlier = fd.until_integrated(0)
    assert info["placed"] == 1 and info["frames"] == 1 and 7 in earlier
    adds_next()
    # alva_system_reset_mesh
    ar.resetMesh()
    emptied()
    info, _ = fd.until_integrated(limit=5)
    assert info["placed"] == 1 and info["frames"] == 1
    adds_next()
    # a changed resolution, a changed extent: placed anew by the call itself
    info, _ = fd.until_integrated(limit=5, resolution=64)
    assert info["placed"] == 1 and info["frames"] == 1 and info["resolution"] == 64
    assert ar.mesh(**CAPS)[3]["resolution"] == 64
    info, _ = fd.until_integrated(limit=5, rel_extent=3.0)
    assert info["placed"] == 1 and info["frames"] == 1 and info["resolution"] == RES
    adds_next_kw = fd.until_integrated(limit=5, rel_extent=3.0)[0]
    assert adds_next_kw["placed"] == 0 and adds_next_kw["frames"] == 2
    with pytest.raises(AlvaError, match="bad argument"):
        ar.meshUpdate(resolution=48)
    # depth off: refused, and the volume goes with the ring
    ar.set_depth(False)
    with pytest.raises(AlvaError, match="depth is off"):
        ar.meshUpdate(**KW)
    emptied()
    ar.set_depth(True)
    assert ar.meshUpdate(**KW)["status"] in (6, 7)
    info, _ = fd.until_integrated()
    assert info["placed"] == 1 and info["frames"] == 1
    adds_next()
    # alva_system_reset
    ar.reset()
    emptied()
    assert ar.meshUpdate(**KW)["status"] == 6
    info, earlier = fd.until_integrated(0)
    assert info["placed"] == 1 and info["frames"] == 1 and 7 in earlier
    adds_next()
    # a new map: without relocalization the tracker starts over after the black frames
    for j in range(N_BLACK):
        fd.feed(black + j)
    info, earlier = fd.until_integrated(0)
    assert info["placed"] == 1 and info["frames"] == 1 and 7 in earlier
    adds_next()
    # configure
    k = ar.intrinsics
    assert lib.alva_system_configure_ex(ar.h, W, H, k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"], CELL, 0, 0) == 0
    emptied()
    assert ar.meshUpdate(**KW)["status"] == 6
    info, earlier = fd.until_integrated(0)
    assert info["placed"] == 1 and info["frames"] == 1 and 7 in earlier
    ar.close()
