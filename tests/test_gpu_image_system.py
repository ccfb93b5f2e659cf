"""Image detection through the system surface (alva_system_add_image / alva_system_detect_images, AlvaAR.addImage / detectImages) on the
640 x 480 plane stream, with the crop of the stream's own canvas and a distractor of the same size both added: every answer equals the
device stages replayed on what the debug entry hands back and the host placement restated here; the crop is found and placed on the
frames that track, within twice the error of the restatement's CPU chain on the same frames; the distractor never is; before the map
exists the crop is seen (code 6); a session that asks on every fifth frame tracks -- and answers depthImage and lightEstimate -- bit for
bit like one that never asks; and the pictures' life: ids, refusals, configure and reset."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import image_cases as IC
import sysdiff
from alvaar_amd import synth

pytestmark = pytest.mark.gpu

W, H, CELL = 640, 480, 12
SPEED, N_FRAMES, EVERY = 2, 151, 5      # stream frames 0, 2, .. 300: the chain's frames 0, 60, 120, 200, 300 are indices 0, 30, 60, 100, 150
WIDTH_M = 0.5


@pytest.fixture(scope="module")
def pictures():
    return IC.chain_pictures(W, H)


@pytest.fixture(scope="module")
def frames(pictures):
    import torch
    f = sysdiff.intrinsics(W, H)[0]
    return torch.from_numpy(np.stack([synth.plane_stream_frame(pictures[0], SPEED * k, W, H, f) for k in range(N_FRAMES)])).cuda()


@pytest.fixture(scope="module")
def chain():
    rows = IC.chain_rows()
    for row in rows:
        print(row)
    return {row["k"]: row for row in rows}


def _frame_points_cam(ar, pose7):
    """the map points the frame observes, in the camera frame of Twc = pose7 (what the placement intersects with the picture)"""
    ids, xyz = ar.map_points()[:2]
    pts = xyz[np.isin(ids, ar.frame_map_point_ids())]
    R = _rot_of(pose7[3:])
    return (pts - pose7[:3]) @ R


def _rot_of(q):
    import hit_cases
    return hit_cases.quat_to_rot(q)


@pytest.fixture(scope="module")
def runs(frames, pictures):
    from alvaar_amd.system import AlvaAR
    _, crop, distractor, _ = pictures
    out = {}
    for name in ("asks", "never"):
        ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, depth=True, light=True)
        rec, side, calls = [], [], []
        if name == "asks":
            assert ar.detectImages()[0].shape == (0,)          # no picture: nothing to answer
            ids = (ar.addImage(crop, WIDTH_M), ar.addImage(distractor))
            assert ids == (0, 1)
            first = ar.detectImages()
            assert first[5][:, 0].tolist() == [7, 7]           # no frame yet
        for k in range(N_FRAMES):
            st = ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [int(v) for v in ar.state()]))
            if name == "asks" and k % EVERY == 0:
                ans = ar.detectImages(debug=True)
                dbg = ans[6]
                calls.append(dict(k=k, status=st, ans=ans, pts_cam=_frame_points_cam(ar, dbg["pose7"]) if dbg["tracked"][0] else None,
                                  again=ar.detectImages()))
            d, e = ar.depthImage(step=8), ar.lightEstimate()
            side.append(b"".join(np.ascontiguousarray(a).tobytes() for a in (*d[:3], *e[:5])))
        out[name] = dict(rec=rec, side=side, calls=calls, counters=ar.counters(), K=ar.intrinsics)
        ar.close()
    return out


def test_asking_changes_nothing_in_the_session(runs):
    a, b = runs["asks"], runs["never"]
    assert [r[0] for r in b["rec"]].count(1) > 100
    for k, (ra, rb) in enumerate(zip(a["rec"], b["rec"])):
        assert ra[0] == rb[0] and ra[3] == rb[3], k
        assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), k
    assert a["counters"] == b["counters"] and b["counters"]["ba_solves"] > 0
    assert a["side"] == b["side"]   # depthImage and lightEstimate keep their bytes


def test_every_answer_equals_the_stages_replayed(ctx, runs):
    import torch
    K = runs["asks"]["K"]
    calib4 = (K["fx"], K["fy"], K["cx"], K["cy"])
    for call in runs["asks"]["calls"]:
        ids, poses, extents, scale, quads, info, dbg = call["ans"]
        k, n, nf = call["k"], len(ids), int(dbg["n_frame"][0])
        assert ids.tolist() == [0, 1] and (info[:, 6] == nf).all() and 0 < nf <= IC.TRAIN_CAP
        for x, y in zip(call["again"], call["ans"][:6]):       # nothing is remembered: the same frame gives the same bytes
            assert x.tobytes() == y.tobytes(), k
        # stage 1 and stage 2 on what the call saw
        cap = torch.zeros((IC.TRAIN_CAP, 32), dtype=torch.uint8, device="cuda")
        cap[:nf] = torch.from_numpy(dbg["desc"][:nf]).cuda()
        unpx = torch.zeros((IC.TRAIN_CAP, 2), dtype=torch.float32, device="cuda")
        unpx[:nf] = torch.from_numpy(dbg["unpx"][:nf]).cuda()
        want_unpx = ctx.undistort_points(torch.from_numpy(dbg["kp"][:nf].copy()).cuda(), calib4, (K["k1"], K["k2"], K["p1"], K["p2"]))
        assert np.array_equal(want_unpx.cpu().numpy(), dbg["unpx"][:nf]), k
        match, xy, count = ctx.image_match(torch.from_numpy(dbg["qdesc"][:n].copy()).cuda(), torch.from_numpy(dbg["qxy"][:n].copy()).cuda(), dbg["nq"][:n],
                                           cap, unpx, torch.tensor([nf], dtype=torch.int32).cuda())
        Hm, sinfo, mask, sR, st = ctx.image_homography(xy, count, dbg["wh"][:n], (W, H), calib4)
        cnt = count.cpu().numpy()
        assert cnt.tolist() == dbg["count"][:n].tolist(), k
        for j in range(n):
            assert np.array_equal(match.cpu().numpy()[j, :cnt[j]], dbg["match"][j, :cnt[j]]), (k, j)
            assert xy.cpu().numpy()[j, :cnt[j]].tobytes() == dbg["xy"][j, :cnt[j]].tobytes(), (k, j)
        assert sinfo.tolist() == dbg["stage_info"][:n].tolist(), k
        for got, want in ((Hm, dbg["H"]), (mask, dbg["mask"]), (sR, dbg["stage_R"]), (st, dbg["stage_t"])):
            assert got.tobytes() == want[:n].tobytes(), k
        # the refinement and the host side
        for j in range(n):
            code = int(info[j, 0])
            assert info[j, 1:4].tolist() == sinfo[j, 1:4].tolist()
            if sinfo[j, 0] != 0:
                assert code == sinfo[j, 0] and not poses[j].any() and not quads[j].any() and not extents[j].any() and scale[j] == 0
                continue
            m, (w, h) = cnt[j], dbg["wh"][j]
            pairs, keep = dbg["xy"][j, :m], mask[j, :m].astype(bool)
            wpts = np.c_[(pairs[keep, 0] - w / 2) / w, (pairs[keep, 1] - h / 2) / w, np.zeros(keep.sum())]
            R0, t0 = sR[j].reshape(3, 3), st[j]
            pose0 = np.r_[-R0.T @ t0, _quat_of(R0.T)]
            ok, pose, _, _ = ctx.pnp_refine(torch.from_numpy(pairs[keep, 2:].copy()).cuda(), torch.from_numpy(wpts).cuda(), pose0, calib4)
            Rr = _rot_of(pose[3:] / np.linalg.norm(pose[3:])).T
            tr = -Rr @ pose[:3]
            pc = (Rr @ np.c_[(pairs[:, 0] - w / 2) / w, (pairs[:, 1] - h / 2) / w, np.zeros(m)].T).T + tr
            err = np.hypot(calib4[0] * pc[:, 0] / pc[:, 2] + calib4[2] - pairs[:, 2], calib4[1] * pc[:, 1] / pc[:, 2] + calib4[3] - pairs[:, 3])
            kept = int(((pc[:, 2] > 0) & (err <= 3.0)).sum())
            assert ok and info[j, 4] == kept, (k, j)
            if code == 4:
                assert kept < 20
                continue
            assert np.abs(dbg["R"][j].reshape(3, 3) - Rr).max() < 1e-9 and np.abs(dbg["t"][j] - tr).max() < 1e-9, (k, j)
            a = h / w
            corners = np.array([[-.5, -.5 * a, 0], [.5, -.5 * a, 0], [.5, .5 * a, 0], [-.5, .5 * a, 0]])
            cc = (Rr @ corners.T).T + tr
            want_quad = np.c_[calib4[0] * cc[:, 0] / cc[:, 2] + calib4[2], calib4[1] * cc[:, 1] / cc[:, 2] + calib4[3]]
            assert np.abs(quads[j] - want_quad).max() < 1e-3, (k, j)
            if not dbg["tracked"][0]:
                assert code == 6 and call["status"] != 1 and not poses[j].any() and not extents[j].any()
                continue
            P = call["pts_cam"]
            P = P[P[:, 2] > 0]
            d = P / P[:, 2:]
            lam = (Rr[:, 2] @ tr) / (d @ Rr[:, 2])
            q = lam[:, None] * d - tr
            inside = (lam > 0) & (np.abs(q @ Rr[:, 0]) <= 0.5) & (np.abs(q @ Rr[:, 1]) <= 0.5 * a)
            ratios = np.sort((P[:, 2] / lam)[inside])
            assert info[j, 5] == len(ratios), (k, j)
            if len(ratios) < 8:
                assert code == 5 and not poses[j].any()
                continue
            width = ratios[len(ratios) // 2]
            assert code == 0 and abs(extents[j, 0] - width) <= 1e-6 * width and abs(extents[j, 1] - width * a) <= 1e-6 * width
            assert scale[j] == (np.float32(WIDTH_M / width) if j == 0 else 0)
            Rwc, twc = _rot_of(dbg["pose7"][3:]), dbg["pose7"][:3]
            want = np.zeros(16)
            want[0:3], want[4:7], want[8:11], want[12:15], want[15] = Rwc @ Rr[:, 0], Rwc @ -Rr[:, 2], Rwc @ Rr[:, 1], Rwc @ (width * tr) + twc, 1
            assert np.abs(poses[j] - want).max() < 1e-5 * max(1.0, np.abs(want).max()), (k, j)
            Rw = poses[j].reshape(4, 4)[:3, :3].T
            assert np.abs(np.cross(Rw[:, 0], Rw[:, 1]) - Rw[:, 2]).max() < 1e-5   # right-handed: x cross y = z


def _quat_of(R):
    """unit quaternion (x y z w) of a rotation matrix, largest-pivot form"""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return q / np.linalg.norm(q)


def test_the_distractor_is_never_found(runs):
    for call in runs["asks"]["calls"]:
        assert call["ans"][5][1, 0] in (1, 2, 3), call["k"]


def test_the_crop_is_found_and_placed_where_it_is(runs, chain, pictures):
    """The bounds are twice the restatement chain's CPU errors on the same stream frames (the GPU detector's canonical keypoint order
    breaks match ties differently from the oracle's, so the pairs are not identical).  Measured on an MI355X (chain in brackets):
      frame  60   rotation 2.193 deg (3.191)   centre 0.00276 (0.00325)   extent 0.00182
      frame 120   rotation 1.378 deg (1.987)   centre 0.00176 (0.00108)   extent 0.00203
      frame 200   rotation 2.174 deg (6.405)   centre 0.00440 (0.01332)   extent 0.00395
      frame 300   rotation 1.359 deg (6.825)   centre 0.00464 (0.02382)   extent 0.00534
      frame   0   status 3, code 6, corner error 0.985 px against 3 + 1.044"""
    canvas, _, _, origin = pictures
    f = sysdiff.intrinsics(W, H)[0]
    calls = {SPEED * c["k"]: c for c in runs["asks"]["calls"]}
    tracked = 0
    for k in IC.CHAIN_FRAMES:
        call = calls[k]
        ids, poses, extents, scale, quads, info, dbg = call["ans"]
        R_true, t_true, width_m = IC.crop_pose_in_camera(k, canvas.shape, origin, f)
        ref = chain[k]["crop"]
        if call["status"] != 1:
            # before the map: seen, not placed; the corners within threshold_px + the chain's refit rms of the analytic ones
            a = IC.CROP_WH[1] / IC.CROP_WH[0]
            cc = (R_true @ np.array([[-.5, -.5 * a, 0], [.5, -.5 * a, 0], [.5, .5 * a, 0], [-.5, .5 * a, 0]]).T).T + t_true
            want = np.c_[f * cc[:, 0] / cc[:, 2] + W / 2, f * cc[:, 1] / cc[:, 2] + H / 2]
            err = np.abs(quads[0] - want).max()
            print(k, "status", call["status"], "code", info[0].tolist(), "corner error", err, "bound", 3.0 + ref["rms_px"])
            assert info[0, 0] == 6 and err <= 3.0 + ref["rms_px"], k
            continue
        tracked += 1
        assert info[0, 0] == 0, (k, info[0].tolist())
        Rwc, twc = _rot_of(dbg["pose7"][3:]), dbg["pose7"][:3]
        Rw = poses[0].reshape(4, 4)[:3, :3].T.astype(np.float64)
        Rc = Rwc.T @ np.stack([Rw[:, 0], Rw[:, 2], -Rw[:, 1]], axis=1)        # back to the columns r1 r2 r3
        tc = Rwc.T @ (poses[0][12:15].astype(np.float64) - twc) / extents[0, 0]
        rot, pos = IC.pose_errors(Rc, tc, R_true, t_true)
        # the map's scale: the map points' own depth against the plane z = 4 under the true camera pose of this frame
        P = call["pts_cam"]
        P = P[P[:, 2] > 0]
        R_wc_true, t_wc_true = synth.plane_camera_pose(k)
        true_depth = (4.0 - t_wc_true[2]) / ((P / P[:, 2:]) @ R_wc_true.T)[:, 2]
        map_scale = float(np.median(P[:, 2] / true_depth))
        ext = abs(extents[0, 0] / (width_m * map_scale) - 1)
        print(k, "info", info[0].tolist(), "rotation %.3f deg (chain %.3f)  centre %.5f (chain %.5f)  extent %.5f  scale %.5f m/unit" %
              (rot, ref["refit"][0], pos, ref["refit"][1], ext, scale[0]))
        assert rot <= 2 * ref["refit"][0] and pos <= 2 * ref["refit"][1] and ext <= 2 * ref["refit"][1], k
        assert abs(scale[0] * extents[0, 0] - WIDTH_M) < 1e-5
    assert tracked >= 3


def test_the_life_of_the_pictures(pictures, frames):
    from alvaar_amd.system import AlvaAR, AlvaError, lib
    _, crop, distractor, _ = pictures
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False)
    with pytest.raises(AlvaError, match="96 .. 1024"):
        ar.addImage(crop[:95])
    with pytest.raises(AlvaError, match="keypoints"):
        ar.addImage(np.full((128, 128), 90, np.uint8))
    ids = [ar.addImage(crop if i % 2 == 0 else distractor, 0.1 * i) for i in range(8)]
    assert ids == list(range(8))
    with pytest.raises(AlvaError, match="8 pictures"):
        ar.addImage(crop)
    ar.removeImage(3)
    with pytest.raises(AlvaError):
        ar.removeImage(3)
    assert ar.addImage(crop[:, ::-1].copy()) == 8                     # ids are not reused
    ar.find_camera_pose_device(int(frames[0].data_ptr()), 0.0)
    out = ar.detectImages()
    assert out[0].tolist() == [0, 1, 2, 4, 5, 6, 7, 8]
    assert [a.shape for a in out] == [(8,), (8, 16), (8, 2), (8,), (8, 4, 2), (8, 8)]
    assert [a.dtype for a in out] == [np.int32, np.float32, np.float32, np.float32, np.float32, np.int32]
    assert out[5][[0, 2, 3, 5], 0].tolist() == [6] * 4 and set(out[5][[1, 4, 6], 0].tolist()) <= {1, 2, 3}   # crops (ids 0 2 4 6), distractors (1 5 7)
    # the pictures are the app's: they outlive reset and a new configuration
    ar.reset()
    ar.find_camera_pose_device(int(frames[0].data_ptr()), 0.0)
    again = ar.detectImages()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(out, again))
    K = ar.intrinsics
    lib.alva_system_configure.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_double] * 8
    assert lib.alva_system_configure(ar.h, W, H, K["fx"], K["fy"], K["cx"], K["cy"], 0.0, 0.0, 0.0, 0.0) == 0
    assert ar.detectImages()[5][:, 0].tolist() == [7] * 8          # the pictures are there, the new configuration has no frame yet
    ar.find_camera_pose_device(int(frames[0].data_ptr()), 0.0)
    assert ar.detectImages()[0].tolist() == [0, 1, 2, 4, 5, 6, 7, 8] and ar.detectImages()[5][0, 0] == 6
    ar.resetImages()
    assert len(ar.detectImages()[0]) == 0 and ar.addImage(crop) == 9
    ar.close()
