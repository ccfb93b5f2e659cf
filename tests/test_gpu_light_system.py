"""Light estimation through the system surface (alva_system_light, AlvaAR(light=True).lightEstimate) on the tracking stream of
tests/test_gpu_depth_system.py: every answer equals the three stages replayed on the frames with the rotations the debug entry hands
back, a session that asks on every frame tracks -- and answers alva_system_depth -- bit for bit like one with light off, the four ways a
frame can reach the session give the same bytes, and the environment's life: codes 5 and 1, kept across a LOST episode, emptied by every
reset the header lists."""
from __future__ import annotations

import numpy as np
import pytest

import light_cases as Lc
import sysdiff
from alvaar_amd import synth

pytestmark = pytest.mark.gpu

W, H, CELL = 640, 480, 12
SPEED, N_TRACK, N_BLACK, N_AFTER = 3, 110, 8, 8     # the stream of tests/test_gpu_depth_system.py
RESUME_K = SPEED * 85
N_ROUTE = 60                                        # frames of the stream that the route comparison feeds


def _views():
    return [SPEED * k for k in range(N_TRACK)] + [None] * N_BLACK + [RESUME_K + SPEED * j for j in range(N_AFTER)]


def _calib8(k):
    return (k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"])


def _bytes(answer):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in answer[:5])


@pytest.fixture(scope="module")
def frames_np():
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    black = np.zeros((H, W, 4), np.uint8) + np.array([0, 0, 0, 255], np.uint8)
    return np.stack([black if v is None else synth.plane_stream_frame(canvas, v, W, H, f) for v in _views()])


@pytest.fixture(scope="module")
def frames(frames_np):
    import torch
    return torch.from_numpy(frames_np).cuda()


class _Replay:
    """the three stages called directly, frame by frame, on what the debug entry hands back"""

    def __init__(self, ctx, calib8):
        self.ctx, self.calib8, self.state, self.bad = ctx, calib8, None, []

    def frame(self, k, frame, answer):
        dbg = answer[5]
        if not dbg["fed"]:
            return
        if dbg["frames"] == 1:
            self.state = None                       # the session's environment was emptied before this frame
        acc = self.ctx.light_bin(frame, self.calib8, None if dbg["R_wc"] is None else dbg["R_wc"].reshape(-1), Lc.STEP)
        self.state, was = self.ctx.light_fuse(acc, self.state, Lc.MIN_PIXELS, Lc.W_NEW, Lc.W_MAX, want_acc=True)
        if not np.array_equal(was.cpu().numpy(), dbg["acc"]):
            self.bad.append((k, "acc"))
        if not np.array_equal(self.state.cpu().numpy(), dbg["state"]):
            self.bad.append((k, "state"))
        if _bytes(self.ctx.light_estimate(self.state)) != _bytes(answer):
            self.bad.append((k, "estimate"))


@pytest.fixture(scope="module")
def runs(ctx, frames):
    """the same frames through two sessions: light on (lightEstimate and depthImage after every frame) and light off"""
    from alvaar_amd.system import AlvaAR
    out = {}
    for name in ("on", "off"):
        ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, relocalization=True, depth=True, light=name == "on")
        rep = _Replay(ctx, _calib8(ar.intrinsics))
        rec, answers, raws = [], [], []
        first = ar.lightEstimate(debug=True) if name == "on" else None
        for k in range(len(frames)):
            st = ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
            rec.append((st, ar.pose7()[0].copy(), ar._pose.copy(), [int(v) for v in ar.state()]))
            if name == "on":
                a = ar.lightEstimate(debug=True)
                rep.frame(k, frames[k], a)
                answers.append(a)
            raws.append(ar.depthImage(step=8))
        out[name] = dict(rec=rec, answers=answers, raws=raws, counters=ar.counters(), bad=rep.bad, first=first)
        ar.close()
    return out


def test_light_changes_nothing_else(runs):
    on, off = runs["on"], runs["off"]
    assert 1 in [r[0] for r in off["rec"]] and 4 in [r[0] for r in off["rec"]] and len(on["rec"]) == len(off["rec"])
    for k, (ra, rb) in enumerate(zip(on["rec"], off["rec"])):
        assert ra[0] == rb[0] and ra[3] == rb[3], k
        assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32)), k
    assert on["counters"] == off["counters"] and off["counters"]["ba_solves"] > 0
    answered = 0
    for k, (a, b) in enumerate(zip(on["raws"], off["raws"])):
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
        assert a[3]["status"] == b[3]["status"] and a[3]["counts"].tolist() == b[3]["counts"].tolist(), k
        answered += a[3]["status"] == 0
    assert answered > 40


def test_every_answer_equals_the_stages_replayed(runs):
    on = runs["on"]
    assert on["bad"] == []
    status = [r[0] for r in on["rec"]]
    tracked = [k for k, st in enumerate(status) if st == 1]
    assert len(tracked) > 60
    for k, a in enumerate(on["answers"]):
        sh, pd, pc, amb, info, dbg = a
        assert dbg["fed"] and (dbg["R_wc"] is not None) == (status[k] == 1), k
        if dbg["R_wc"] is not None:
            R = sysdiff._quat_to_rot(on["rec"][k][1][3:])
            assert np.abs(dbg["R_wc"] - R).max() < 1e-12 and np.abs(dbg["R_wc"] @ dbg["R_wc"].T - np.eye(3)).max() < 1e-9, k
        assert info[3] == (W // Lc.STEP) * (H // Lc.STEP), k
    # and the restatement on one tracked frame's hand-over: the accumulators of the frame, then the state and the answer from the state before
    k = tracked[20]
    prev, cur = on["answers"][k - 1][5], on["answers"][k][5]
    st = Lc.fuse(cur["acc"].view(np.uint64).copy(), Lc.unpack_state(prev["state"]))
    assert np.array_equal(Lc.pack_state(st), cur["state"])
    assert _bytes(Lc.estimate(st)) == _bytes(on["answers"][k])


def test_restated_bin_of_a_tracked_frame(runs, frames_np):
    on = runs["on"]
    k = [i for i, r in enumerate(on["rec"]) if r[0] == 1][20]
    dbg = on["answers"][k][5]
    from alvaar_amd.system import camera_intrinsics
    want = Lc.bin_frame(frames_np[k], _calib8(camera_intrinsics(W, H)), dbg["R_wc"].reshape(-1), Lc.STEP)
    assert np.array_equal(want, dbg["acc"].view(np.uint64))


def test_codes_and_the_environment_across_a_lost_episode(runs):
    on = runs["on"]
    sh, pd, pc, amb, info, dbg = on["first"]
    assert info.tolist() == [5, 0, 0, 0, 0, 0, 0, 0] and not sh.any() and amb.tolist() == [0.0, 1.0, 1.0, 1.0] and not dbg["fed"]
    status = [r[0] for r in on["rec"]]
    first_ok = status.index(1)
    assert first_ok > 0
    for k in range(first_ok):                        # initialising: no environment yet, the frame's own values already
        sh, pd, pc, amb, info, dbg = on["answers"][k]
        assert info[0] == 1 and info[1] == 0 and info[5] == 0 and amb[0] > 0 and sh[0].all() and not sh[1:].any() and not pd.any(), k
    sh, pd, pc, amb, info, dbg = on["answers"][first_ok]
    assert info[0] == 0 and info[1] > 0 and info[5] == 1
    cells = [int(a[4][1]) for a in on["answers"]]
    fused = [int(a[4][5]) for a in on["answers"]]
    assert all(b >= a for a, b in zip(cells[first_ok:], cells[first_ok + 1:]))      # what was seen is still there
    lost = [k for k, st in enumerate(status) if st == 4]
    assert lost
    for k in lost:                                   # kept across the LOST episode: the black frames touch no cell
        sh, pd, pc, amb, info, dbg = on["answers"][k]
        assert info[0] == 0 and info[1] == cells[lost[0] - 1] and info[5] == fused[lost[0] - 1] and info[2] == 0 and amb[0] == 0, k
        assert np.array_equal(dbg["state"][:13 * Lc.CELLS], on["answers"][lost[0] - 1][5]["state"][:13 * Lc.CELLS]), k
    after = [k for k in range(lost[-1] + 1, len(status)) if status[k] == 1]
    assert after and fused[after[-1]] == fused[lost[0] - 1] + len(after) and cells[after[-1]] >= cells[lost[0] - 1]
    print("cells with a value", cells[first_ok], "->", cells[-1], "frames fused", fused[-1], "ambient", float(on["answers"][-1][3][0]))


def _feed(ar, route, frames, frames_np, k, ts):
    from alvaar_amd.system import lib
    if route == "host":                              # pageable host memory the session knows nothing about: the pinned staging copy
        st = lib.alva_system_find_camera_pose_ts(ar.h, frames_np[k].ctypes.data, ts, ar._pose_ptr)
    elif route == "wrapper":                         # AlvaAR's own frame buffer: device memory written over the BAR, else its registered buffer
        st = ar.findCameraPose(frames_np[k], ts)[1]
    elif route == "device":
        st = ar.find_camera_pose_device(int(frames[k].data_ptr()), ts)
    else:                                            # device memory with the next-frame hint
        st = ar.find_camera_pose_device(int(frames[k].data_ptr()), ts, int(frames[k + 1].data_ptr()))
    assert st >= 0
    return st


def test_the_same_answer_bytes_whichever_way_the_frame_arrives(frames, frames_np):
    from alvaar_amd.system import AlvaAR
    got = {}
    for route in ("host", "wrapper", "device", "hint"):
        ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, light=True)
        seq = []
        for k in range(N_ROUTE):
            st = _feed(ar, route, frames, frames_np, k, 33.0 * k)
            seq.append((st, _bytes(ar.lightEstimate())))
        got[route] = seq
        if route == "wrapper":
            print("the wrapper's frame buffer is", "device memory written over the BAR" if ar._bar_frame else "a registered host buffer")
        ar.close()
    assert sum(st == 1 for st, _ in got["device"]) > 20
    for route in ("host", "wrapper", "hint"):
        diff = [k for k, (a, b) in enumerate(zip(got[route], got["device"])) if a != b]
        assert diff == [], (route, diff[:8])


def test_every_listed_reset_empties_the_environment(frames):
    from alvaar_amd.system import AlvaAR, AlvaError, lib
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, light=True)
    t = [0]

    def feed(k):
        st = ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * t[0])
        t[0] += 1
        return st

    def until_environment(start=0, limit=100):
        for k in range(start, start + limit):
            feed(k)
            info = ar.lightEstimate()[4]
            if info[0] == 0:
                return k
        raise AssertionError("no environment within %d frames" % limit)

    def empty(code):
        sh, pd, pc, amb, info, dbg = ar.lightEstimate(debug=True)
        assert info[0] == code and info[1] == 0 and info[5] == 0 and not dbg["state"][:13 * Lc.CELLS].any(), info
        return info

    k = until_environment()
    feed(k + 1)
    assert ar.lightEstimate()[4][5] == 2
    # alva_system_reset_light: the environment goes, the switch stays
    ar.resetLight()
    empty(5)
    feed(k + 2)
    info = ar.lightEstimate()[4]
    assert info[0] == 0 and info[5] == 1
    # light off: refused by name; on again: empty
    ar.set_light(False)
    with pytest.raises(AlvaError, match="alva_system_set_light"):
        ar.lightEstimate()
    feed(k + 3)
    ar.set_light(True)
    empty(5)
    feed(k + 4)
    assert ar.lightEstimate()[4][5] == 1
    # alva_system_reset
    ar.reset()
    empty(5)
    k = until_environment()
    # a new map: without relocalization the tracker starts over on the black frames
    sts = [feed(N_TRACK + j) for j in range(N_BLACK)]
    info = empty(1)
    assert info[2] == 0, sts
    until_environment()
    # configure
    c = ar.intrinsics
    assert lib.alva_system_configure_ex(ar.h, W, H, c["fx"], c["fy"], c["cx"], c["cy"], c["k1"], c["k2"], c["p1"], c["p2"], CELL, 0, 0) == 0
    empty(5)
    until_environment()
    ar.close()


def test_wrapper_shapes_and_dtypes(frames):
    from alvaar_amd.system import AlvaAR
    ar = AlvaAR(W, H, cell_size=CELL, random_sampling=False, light=True)
    ar.find_camera_pose_device(int(frames[0].data_ptr()), 0.0)
    out = ar.lightEstimate()
    assert len(out) == 5 and [a.shape for a in out] == [(9, 3), (3,), (3,), (4,), (8,)]
    assert [a.dtype for a in out] == [np.float32] * 4 + [np.int32]
    dbg = ar.lightEstimate(debug=True)[5]
    assert dbg["acc"].shape == (Lc.ACC_WORDS,) and dbg["state"].shape == (Lc.STATE_BYTES,) and dbg["fed"] and dbg["frames"] == 1
    ar.close()
    off = AlvaAR(W, H, cell_size=CELL, random_sampling=False)
    from alvaar_amd.system import AlvaError
    with pytest.raises(AlvaError, match="alva_system_set_light"):
        off.lightEstimate()
    off.close()
