"""The volume raycast through the system surface (alva_system_mesh_raycast / alva_system_mesh_depth / alva_system_mesh_hit_test,
AlvaAR.meshRaycast / meshDepth / meshHitTest) on the stream and with the parameters of tests/test_gpu_mesh_system.py (resolution 32, step
8, an update every fifth frame): every answer equals the stages replayed on the test's own copy of the volume, byte for byte; the codes
(5 without a volume -- before the first update, after every reset the mesh header lists -- and 6 for the calls that need the current
pose while the tracker is LOST, when an explicit pose and world rays still answer from the kept volume); a session that calls all three
on every frame tracks -- and answers depthImage, depthDense and mesh -- bit for bit like one that never does; and the depth image of
the volume lies on the stream's plane."""
from __future__ import annotations

import numpy as np
import pytest

import sysdiff
import mesh_cases as Mc
import raycast_cases as Rc
import test_gpu_mesh_system as Ms
from alvaar_amd import synth

pytestmark = pytest.mark.gpu

W, H, CELL, STEP, EVERY = Ms.W, Ms.H, Ms.CELL, Ms.STEP, Ms.EVERY
KW, CAPS = Ms.KW, Ms.CAPS
# the call's bound of 16 taps: 14 hashed over the image, one just off it, one far off it
TAPS = np.concatenate([(Mc.hashed(28, 5).reshape(14, 2) % 4096) / 4095.0 * np.array([W - 1.0, H - 1.0]), [[-5.0, 20.0], [320.0, 1e6]]]).astype(np.float32)


@pytest.fixture(scope="module")
def frames():
    import torch
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    black = np.zeros((H, W, 4), np.uint8) + np.array([0, 0, 0, 255], np.uint8)
    return torch.from_numpy(np.stack([black if v is None else synth.plane_stream_frame(canvas, v, W, H, f) for v in Ms._views()])).cuda()


def _T_wc(pose7):
    """the session's own T_wc12 of a pose (t, q = x y z w): quat_to_rot's operations in their order, then t"""
    t, (x, y, z, w) = pose7[:3], (float(v) for v in pose7[3:])
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]
    return np.array(R + list(t), np.float64)


def _world_rays(geo, eye):
    """200 rays through the volume, two of them rejected: half from hashed origins in and around it towards hashed points inside it; half
    from about `eye` -- the pose the volume was placed from, so its centre lies on the surface, on that pose's optical axis -- towards the
    central fifth of the volume, which is within 11 degrees of that axis and so inside what the camera saw"""
    o, side = geo[0], geo[1] * Ms.RES
    rays = Rc.hashed_rays(200, 77)                       # (written for the cube [-1, 1]^3)
    target = o + (0.2 + 0.6 * (Mc.hashed(600, 78).reshape(200, 3) % 4096) / 4095.0) * side
    rays[:, :3] = o + (rays[:, :3] + 1.0) / 2.0 * side
    rays[100:, :3] = np.asarray(eye) + (rays[100:, :3] - (o + side / 2.0)) * 0.05
    target[100:] = o + (0.4 + 0.2 * (Mc.hashed(300, 79).reshape(100, 3) % 4096) / 4095.0) * side
    rays[:, 3:] = (target - rays[:, :3]) * 0.7
    rays[7, 0] = np.nan
    rays[9, 3:] = 0.0
    return rays


class _Volume:
    """the test's own copy of the session's volume, as alva_system_debug_mesh_update handed it back"""

    def __init__(self, ctx, calib8):
        self.ctx, self.calib8, self.q, self.geo = ctx, calib8, None, None

    def keep(self, info):
        import torch
        if info["status"] == 0:
            self.q, self.w = torch.from_numpy(info["q"].copy()).cuda(), torch.from_numpy(info["w"].copy()).cuda()
            self.geo = (info["origin"].copy(), info["voxel"])

    def pixels(self, T_wc, step=STEP, uv=None):
        import torch
        return self.ctx.mesh_raycast_pixels(self.q, self.w, self.geo[0], self.geo[1], 2, T_wc, self.calib8, W, H, step,
                                            None if uv is None else torch.from_numpy(uv).cuda())

    def rays(self, rays6, t_near=0.0, t_far=np.inf, min_weight=2):
        import torch
        return self.ctx.mesh_raycast(self.q, self.w, self.geo[0], self.geo[1], min_weight, torch.from_numpy(rays6).cuda(), t_near, t_far)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _depth_differs(got, want, gh, gw):
    """meshDepth's answer against the pixels stage's on the grid"""
    depth, normals, codes, info = got
    bad = [k for k, a, b in (("depth", depth, want["t"].reshape(gh, gw)), ("normals", normals, want["normal"].reshape(gh, gw, 3)),
                             ("codes", codes, want["code"].reshape(gh, gw))) if not _same(a, b)]
    if [info["rays"], *info["counts"], info["max_samples"], info["resolution"]] != want["info"].tolist() or info["status"] != 0:
        bad.append("info")
    return bad


@pytest.fixture(scope="module")
def runs(ctx, frames):
    """the same frames through two sessions that both ask for depthImage, depthDense and, on every fifth frame, meshUpdate and mesh: one
    that calls meshDepth, meshRaycast and meshHitTest on every frame, one that never does"""
    from alvaar_amd.system import AlvaAR
    out = {}
    gw, gh = W // STEP, H // STEP
    fixed_T = None
    for name in ("rays", "never"):
        ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, relocalization=True, depth=True)
        vol = _Volume(ctx, Ms._calib8(ar.intrinsics))
        rec, calls = [], []
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
            raw = ar.depthImage(step=STEP)
            dense = ar.depthDense(step=STEP, max_level=5)
            r = [st, ar.pose7()[0].copy(), ar._pose.copy(), ar.state().copy(), tuple(ar.counters().values()), [a.copy() for a in raw[:3]],
                 [a.copy() for a in dense[:4]]]
            if k % EVERY == 0 or k >= Ms.N_TRACK + Ms.N_BLACK:
                info = ar.meshUpdate(debug=True, **KW)
                m = ar.mesh(**CAPS)
                r.append([a.copy() for a in m[:3]])
                vol.keep(info)
                if info["status"] == 0:
                    out["geometry"], out["intrinsics"] = dict(trunc=info["trunc"], voxel=info["voxel"]), dict(ar.intrinsics)
            rec.append(r)
            if name != "rays":
                continue
            c = dict(frame=k, tracker=st, pose=ar.pose7()[0].copy(), have=vol.q is not None)
            c["depth"] = ar.meshDepth(step=STEP)
            c["taps"] = ar.meshHitTest(TAPS)
            if vol.q is None:
                c["world"] = ar.meshRaycast(np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 1.0]]))
                c["depth_T"] = ar.meshDepth(T_wc=_T_wc(c["pose"]), step=STEP)
            else:
                if fixed_T is None:
                    fixed_T = _T_wc(c["pose"])               # the pose of the first frame with a volume, asked for on every later frame
                rays = _world_rays(vol.geo, fixed_T[9:])
                c["world"] = ar.meshRaycast(rays)
                c["depth_T"] = ar.meshDepth(T_wc=fixed_T, step=STEP)
                bad = []
                # the stages replayed on the copy
                w = vol.rays(rays)
                t, p, n, codes, info = c["world"]
                bad += ["world." + key for key, a in (("t", t), ("point", p), ("normal", n), ("code", codes)) if not _same(a, w[key])]
                if [info["rays"], *info["counts"], info["max_samples"], info["resolution"]] != w["info"].tolist():
                    bad.append("world.info")
                bad += ["depth_T." + b for b in _depth_differs(c["depth_T"], vol.pixels(fixed_T), gh, gw)]
                if st == 1:
                    T = _T_wc(c["pose"])
                    bad += ["depth." + b for b in _depth_differs(c["depth"], vol.pixels(T), gh, gw)]
                    h = vol.pixels(T, uv=TAPS)
                    poses, tinfo = c["taps"]
                    if not _same(poses, h["pose"]):
                        bad.append("taps.pose")
                    want = np.zeros((len(TAPS), 8), np.int32)
                    want[:, 0], want[:, 1], want[:, 2], want[:, 3] = h["code"], h["pose_ok"], h["info"][6], h["info"][7]
                    if not np.array_equal(tinfo, want):
                        bad.append("taps.info")
                c["bad"] = bad
            calls.append(c)
        if name == "rays":   # other parameters once, at the end of the stream, on the kept volume
            rays = _world_rays(vol.geo, fixed_T[9:])
            a, b = ar.meshRaycast(rays, min_weight=1, t_near=0.25, t_far=1.5), vol.rays(rays, 0.25, 1.5, min_weight=1)
            out["other_parameters"] = all(_same(x, b[key]) for x, key in zip(a[:4], ("t", "point", "normal", "code")))
            out["other_step"] = _depth_differs(ar.meshDepth(T_wc=fixed_T, step=5), vol.pixels(fixed_T, step=5), H // 5, W // 5)
            ar.resetMesh()
            out["after_reset"] = (ar.meshDepth(step=STEP), ar.meshHitTest(TAPS), ar.meshRaycast(rays))
        out[name] = dict(rec=rec, calls=calls)
        ar.close()
    return out


def test_every_answer_equals_the_stages_replayed_on_the_copy(runs):
    calls = runs["rays"]["calls"]
    have = [c for c in calls if c["have"]]
    tracked = [c for c in have if c["tracker"] == 1]
    assert len(have) >= 60 and len(tracked) >= 50
    for c in have:
        assert c["bad"] == [], (c["frame"], c["bad"])
    last = tracked[-1]
    # the equalities above were about something: depth from motion leaves most of this volume unseen (about a sixth of the depth image's
    # pixels meet a surface), so of the 100 world rays aimed into the seen frustum a sixth is expected to hit; the two bad rays are rejected
    share = last["depth"][3]["counts"][0] / last["depth"][3]["rays"]
    print("hits: %d of the depth image's %d pixels, %d of 200 world rays" % (last["depth"][3]["counts"][0], last["depth"][3]["rays"], last["world"][4]["counts"][0]))
    assert share > 0.1 and last["world"][4]["counts"][0] >= 5 and last["world"][4]["counts"][4] == 2
    assert any((c["taps"][1][:, 1] == 1).any() for c in tracked)                    # a tap that found a pose
    assert (last["taps"][1][14:, 0] <= 3).all()                                     # the taps off the image have rays like any other
    assert runs["other_parameters"] and runs["other_step"] == []


def test_codes(runs):
    calls = runs["rays"]["calls"]
    gw, gh = W // STEP, H // STEP
    before = [c for c in calls if not c["have"]]
    assert before and any(c["tracker"] == 1 for c in before)                      # tracking, and still no volume: code 5, not 6
    after = runs["after_reset"]
    for depth, taps, world in [(c["depth"], c["taps"], c["world"]) for c in before] + [(c["depth_T"], c["taps"], c["world"]) for c in before] + [after]:
        assert depth[3]["status"] == 5 and (depth[2] == 5).all() and not depth[0].any() and not depth[1].any() and depth[0].shape == (gh, gw)
        assert depth[3]["rays"] == gw * gh and not depth[3]["counts"].any()
        assert (taps[1][:, 0] == 5).all() and not taps[1][:, 1:].any() and not taps[0].any()
        assert world[4]["status"] == 5 and (world[3] == 5).all() and not world[0].any()
    # the black frames: the calls that need the current pose answer 6; an explicit pose and world rays answer from the kept volume
    lost = [c for c in calls if c["tracker"] == 4]
    assert len(lost) >= 5 and all(c["have"] for c in lost)
    kept = [c for c in calls if c["frame"] < lost[0]["frame"] and c["tracker"] == 1][-1]
    for c in lost:
        assert c["depth"][3]["status"] == 6 and (c["depth"][2] == 6).all() and not c["depth"][0].any()
        assert (c["taps"][1][:, 0] == 6).all() and not c["taps"][0].any()
        assert c["depth_T"][3]["status"] == 0 and c["world"][4]["status"] == 0 and c["bad"] == []
        for a, b in zip(c["depth_T"][:3] + c["world"][:4], kept["depth_T"][:3] + kept["world"][:4]):
            assert _same(a, b)                                                    # (nothing was integrated in between: the same bytes)
    assert any(c["tracker"] == 1 for c in calls if c["frame"] > lost[-1]["frame"])


def test_raycast_calls_change_nothing_else(runs):
    a, b = runs["rays"]["rec"], runs["never"]["rec"]
    assert len(a) == len(b) and 1 in [r[0] for r in b] and 4 in [r[0] for r in b]
    meshes = 0
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0] == rb[0] and ra[4] == rb[4], k
        assert _same(ra[1], rb[1]) and _same(ra[2], rb[2]) and np.array_equal(ra[3], rb[3]), k
        assert len(ra) == len(rb)
        for x, y in zip(ra[5] + ra[6] + (ra[7] if len(ra) > 7 else []), rb[5] + rb[6] + (rb[7] if len(rb) > 7 else [])):
            assert _same(x, y), k
        meshes += len(ra) > 7 and len(ra[7][2]) > 0
    assert meshes >= 10


def test_the_volumes_depth_lies_on_the_streams_plane(runs):
    calls = runs["rays"]["calls"]
    c = [c for c in calls if c["have"] and c["tracker"] == 1 and c["frame"] < Ms.N_TRACK][-1]
    depth, normals, codes, info = c["depth"]
    hit = codes == 0
    assert hit.sum() > 500
    gh, gw = depth.shape
    # the pixels' rays in the camera frame (no distortion on this stream): X_c = depth (x, y, 1)
    k = runs["intrinsics"]
    assert not any(k[d] for d in ("k1", "k2", "p1", "p2"))
    f, cx, cy = k["fx"], k["cx"], k["cy"]
    u =(np.arange(gw) * STEP + STEP // 2)[None, :].repeat(gh, 0)
    v = (np.arange(gh) * STEP + STEP // 2)[:, None].repeat(gw, 1)
    Xc = np.stack([(u - cx) / f, (v - cy) / f, np.ones_like(u, float)], -1)[hit] * depth[hit][:, None].astype(np.float64)
    view = Ms._views()[c["frame"]]
    R_true, t_true = synth.plane_camera_pose(view)
    n_c, d_c = R_true.T @ np.array([0.0, 0.0, 1.0]), Ms.PLANE_Z - t_true[2]
    h = Xc @ n_c
    scale = float(np.median(h)) / d_c
    err = np.abs(h - scale * d_c)
    trunc, vox = runs["geometry"]["trunc"], runs["geometry"]["voxel"]
    print("frame %d: %d depths, scale %.5f, |distance| max %.4f median %.4f map units, trunc %.4f voxel %.4f" % (
        c["frame"], hit.sum(), scale, err.max(), float(np.median(err)), trunc, vox))
    # the mesh file's own bound for the mesh's used vertices, plus one voxel
    assert scale > 0 and err.max() <= trunc + vox


def test_the_ray_block_grows_with_the_call(ctx, frames):
    """The session's first cast is one tap (the device block of rays and outputs is sized for it), then three world rays, then the depth
    image on the grid -- thousands of rays: the block is replaced by a larger one inside the live session --, then the three rays again."""
    from alvaar_amd.system import AlvaAR
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True)
    fd = Ms._Feeder(ar, frames)
    vol = _Volume(ctx, Ms._calib8(ar.intrinsics))
    for n in range(100):                              # until there is a volume; no cast by the session before that
        fd.feed(0 if n == 0 else None)
        vol.keep(ar.meshUpdate(debug=True, **KW))
        if vol.q is not None:
            break
    else:
        raise AssertionError("no update integrated within 100 frames")
    pose = ar.pose7()[0].copy()
    T = _T_wc(pose)
    gw, gh = W // STEP, H // STEP
    rays = _world_rays(vol.geo, pose[:3])[100:103]
    poses, tinfo = ar.meshHitTest(TAPS[:1])
    first = ar.meshRaycast(rays)
    depth = ar.meshDepth(step=STEP)
    second = ar.meshRaycast(rays)
    assert depth[3]["rays"] == gw * gh > 256 and first[4]["rays"] == 3
    for a, b in zip(first[:4], second[:4]):
        assert _same(a, b)
    assert first[4]["status"] == second[4]["status"] == 0 and first[4]["counts"].tolist() == second[4]["counts"].tolist()
    want = vol.rays(rays)
    assert all(_same(a, want[key]) for a, key in zip(second[:4], ("t", "point", "normal", "code")))
    assert _depth_differs(depth, vol.pixels(T), gh, gw) == []
    h = vol.pixels(T, uv=TAPS[:1])
    assert _same(poses, h["pose"]) and tinfo[0, :4].tolist() == [int(h["code"][0]), int(h["pose_ok"][0]), int(h["info"][6]), int(h["info"][7])]
    ar.close()


def test_every_listed_reset_leaves_no_volume_to_cast_into(frames):
    """code 5 after each way the mesh header lists to empty the volume, and an answer again once an update has integrated"""
    from alvaar_amd.system import AlvaAR, lib
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True)
    fd = Ms._Feeder(ar, frames)
    ray = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
    identity = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])

    def statuses():
        return (ar.meshDepth(T_wc=identity, step=STEP)[3]["status"], ar.meshDepth(step=STEP)[3]["status"], ar.meshRaycast(ray)[4]["status"],
                set(ar.meshHitTest(TAPS[:3])[1][:, 0].tolist()))

    def emptied():
        assert statuses() == (5, 5, 5, {5})

    def filled():
        a, b, c, d = statuses()
        assert a == 0 and b == 0 and c == 0 and max(d) <= 3

    emptied()
    fd.until_integrated(0)
    filled()
    ar.resetMesh()                                    # alva_system_reset_mesh
    emptied()
    fd.until_integrated(limit=5)
    filled()
    ar.set_depth(False)                               # depth off: the volume goes with the ring
    emptied()
    ar.set_depth(True)
    emptied()
    fd.until_integrated()
    filled()
    ar.reset()                                        # alva_system_reset
    emptied()
    fd.until_integrated(0)
    filled()
    for j in range(Ms.N_BLACK):                       # a new map: without relocalization the tracker starts over after the black frames
        fd.feed(Ms.N_TRACK + j)
    assert any(fd.feed(0 if n == 0 else None) == 1 for n in range(100))
    emptied()
    fd.until_integrated()
    filled()
    k = ar.intrinsics                                 # configure
    assert lib.alva_system_configure_ex(ar.h, W, H, k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"], CELL, 0, 0) == 0
    emptied()
    ar.close()
