"""Per-call time of the two anchor stages and of an updateAnchors call in a session.

  Context.anchor_attach   the base scene of tests/hit_cases.py (2800 points) and 16384 random points, 1 and 16 anchors, K = 32
  Context.anchor_update   1, 5 and 64 anchors of 32 supports each (a planted rigid motion)
  Context.hit_test        the five base taps on the base scene: k_hit_test, for comparison in the same run
  AlvaAR.updateAnchors    five anchors (K = 32) in a session on the plane stream of the tests, 40 tracked frames in

  python tools/anchors_timing.py                    wall time per call (JSON line)
  python tools/anchors_timing.py --kernels OUTDIR   runs itself in a child process under rocprofv3 --kernel-trace --stats (no counters)
                                                    and adds the kernels' own times per configuration, read from the dispatch trace:
                                                    the configurations run in a fixed order, CALLS + WARMUP dispatches each

Prints one JSON line."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CALLS, WARMUP = 200, 20
ATTACH = [(2800, 1), (2800, 16), (16384, 1), (16384, 16)]
UPDATE = [1, 5, 64]
SESSION_ANCHORS = 5


def _timed(call):
    import numpy as np
    import torch
    t = []
    for _ in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return dict(median=round(1e6 * float(np.median(t[WARMUP:])), 1), max=round(1e6 * max(t[WARMUP:]), 1))


def timed():
    import numpy as np
    import torch
    import alvaar_amd
    import anchor_cases as A
    import hit_cases as H
    ctx = alvaar_amd.Context(0)
    rng = np.random.default_rng(1)
    scenes = {2800: H.base_scene(), 16384: rng.standard_normal((16384, 3)) * 2}
    res = dict(calls=CALLS, warmup=WARMUP)
    for n, a in ATTACH:
        P = torch.from_numpy(np.ascontiguousarray(scenes[n])).cuda()
        pos = scenes[n][:: max(1, n // 16)][:a] + 0.01
        res["attach_%d_points_%d_anchors_wall_us" % (n, a)] = _timed(lambda: ctx.anchor_attach(P, pos, 32))
    case = A.update_cases()["planted32"]
    for a in UPDATE:
        count, ref, cur = [32] * a, np.tile(case["ref"], (a, 1, 1)), np.tile(case["cur"], (a, 1, 1))
        pose = np.tile(case["pose_ref"], (a, 1))
        res["update_%d_anchors_wall_us" % a] = _timed(lambda: ctx.anchor_update(count, ref, cur, pose))
    P = torch.from_numpy(H.base_scene()).cuda()
    taps = [uv for uv, _ in H.BASE_TAPS]
    res["hit_test_5_taps_wall_us"] = _timed(lambda: ctx.hit_test(P, H.POSE_BASE, H.K_BASE, taps, radius_px=40, num_iterations=64))
    res.update(session())
    return res


def session():
    import numpy as np
    import torch
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    W, Hh = 640, 480
    f = sysdiff.intrinsics(W, Hh)[0]
    canvas = synth.texture_canvas(W, Hh, 5)
    ar = AlvaAR(W, Hh, cell_size=12, random_sampling=False, relocalization=True)
    tracked = 0
    for k in range(80):
        frame = torch.from_numpy(synth.plane_stream_frame(canvas, 3 * k, W, Hh, f)).cuda()
        tracked += ar.find_camera_pose_device(int(frame.data_ptr()), 33.0 * k) == 1
        if tracked == 40:
            break
    taps = np.array([(320, 240), (200, 150), (440, 330), (160, 360), (480, 120)], np.float32)
    poses, info = ar.hitTest(taps)
    ids, cinfo = ar.createAnchors(poses[info[:, 0] == 0][:SESSION_ANCHORS], 32)
    out = dict(session_tracked_frames=tracked, session_map_points=int((ar.map_points()[2][:, 0] == 1).sum()), session_anchors=int((ids >= 0).sum()))
    out["session_update_anchors_wall_us"] = _timed(ar.updateAnchors)
    out["session_update_codes"] = ar.updateAnchors()[2][:, 0].tolist()
    ar.close()
    return out


def kernel_times(outdir):
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", outdir, "-o", "anchors", "--output-format", "csv", "--",
           sys.executable, str(Path(__file__).resolve())]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    rows = []
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()

    def chunks(kernel, labels):
        import numpy as np
        d = [us for _, name, us in rows if kernel in name]
        out = {}
        for k, label in enumerate(labels):
            part = d[k * (WARMUP + CALLS) + WARMUP:(k + 1) * (WARMUP + CALLS)]
            if part:
                out[label] = dict(calls=len(part), avg_us=round(float(np.mean(part)), 2), min_us=round(min(part), 2), max_us=round(max(part), 2))
        return out

    # (the session's create adds one k_anchor_attach dispatch and its updates CALLS + WARMUP + 1 k_anchor_update dispatches at the end)
    return dict(k_anchor_attach=chunks("k_anchor_attach", ["%d_points_%d_anchors" % c for c in ATTACH]),
                k_anchor_update=chunks("k_anchor_update", ["%d_anchors" % a for a in UPDATE] + ["session_%d_anchors" % SESSION_ANCHORS]),
                k_hit_test=chunks("k_hit_test", ["5_taps_2800_points"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", default=None, help="also run under rocprofv3 into this directory and report the kernels per configuration")
    a = ap.parse_args()
    res = timed()
    if a.kernels:
        res["kernels"] = kernel_times(a.kernels)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
