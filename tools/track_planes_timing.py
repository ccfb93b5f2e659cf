"""Per-call time of plane tracking (alva_track_planes) next to plane detection.  Two steps, each a process of its own:

  base     the base scene of tests/hit_cases.py (2800 points: a floor, a wall, clutter): Context.detect_planes, then Context.track_planes
           in the steady state -- the scene's two planes as priors, fed its own output --, CALLS times each after a warm-up
  system   a tracking session on the synthetic plane stream: AlvaAR.detectPlanes next to AlvaAR.trackPlanes, wall time per call

  python tools/track_planes_timing.py --step base       one step, wall time per call (JSON line)
  python tools/track_planes_timing.py --kernels OUTDIR [--csv FILE] [--json FILE]
        every step under `timeout -k 10 <s> rocprofv3 --kernel-trace --stats` (no counters), one after the other, stopping at the first
        that fails; adds the kernels' own times from the trace -- k_track_claim, the rounds queued behind it, and as the yardstick from
        the same run k_plane_round's floor round (the first of every four launches of a detection) -- and writes them to FILE

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

CALLS, WARMUP = 300, 20
STEPS = (("base", 120), ("system", 180))   # name, time limit in seconds
MAX_PLANES = 4


def _wall(call):
    import numpy as np
    import torch
    t = []
    for k in range(WARMUP + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        t.append(time.perf_counter() - t0)
    return dict(median=round(1e6 * float(np.median(t[WARMUP:])), 1), max=round(1e6 * max(t[WARMUP:]), 1)), out


def step_base():
    import torch
    import alvaar_amd
    import hit_cases as H
    import plane_cases as C
    ctx = alvaar_amd.Context(0)
    P = torch.from_numpy(H.base_scene()).cuda()
    res = dict(points=int(P.shape[0]), calls=CALLS)
    res["detect_planes_wall_us"], det = _wall(lambda: ctx.detect_planes(P, H.POSE_BASE, **C.BASE_KW))
    res["detect_planes_codes"] = det[1][:, 0].tolist()
    state = dict(prior=det[0][det[1][:, 0] == 0])

    def track():
        out = ctx.track_planes(P, H.POSE_BASE, prior24=state["prior"], **C.BASE_KW)
        state["prior"] = out[0][out[1][:, 0] == 0]   # its own output: the steady state
        return out

    res["track_planes_wall_us"], out = _wall(track)
    res["track_planes_info"] = out[1][:, :6].tolist()
    return res


def step_system():
    import numpy as np
    import torch
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    w, h, rel = 640, 480, 3 * 0.00128905   # the stream and session of tests/test_gpu_detect_planes.py
    f = sysdiff.intrinsics(w, h)[0]
    canvas = synth.texture_canvas(w, h, 5)
    dev = torch.from_numpy(np.stack([synth.plane_stream_frame(canvas, 3 * k, w, h, f) for k in range(80)])).cuda()
    ar = AlvaAR(w, h, cell_size=12, random_sampling=False)
    status = [ar.find_camera_pose_device(int(dev[k].data_ptr()), 33.0 * k) for k in range(len(dev))]
    res = dict(last_status=status[-1], calls=CALLS)
    res["detectPlanes_wall_us"], out = _wall(lambda: ar.detectPlanes(rel))
    res["trackPlanes_wall_us"], tr = _wall(lambda: ar.trackPlanes(rel))
    res.update(points=int(len(out[2])), detect_codes=out[1][:, 0].tolist(), track_info=tr[1][:, :6].tolist(), plane_ids=tr[2].tolist())
    ar.close()
    return res


def kernel_rows(outdir, step):
    """from the trace, in launch order: a k_track_claim, then the rounds queued behind it (as many as the call before left slots free --
    read off the trace: the k_plane_round launches up to the next claim); the k_plane_round launches before the first claim are the
    detections', four per call, the first of each the floor round"""
    rows = []
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        trace = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        per, seen_claim, after_claim = {}, False, 0
        for r in trace:
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            if "k_track_claim" in r["Kernel_Name"]:
                per.setdefault("k_track_claim", []).append(us)
                seen_claim, after_claim = True, 0
            elif "k_plane_round" in r["Kernel_Name"]:
                if seen_claim:
                    per.setdefault("k_plane_round[tracking, round %d]" % after_claim, []).append(us)
                    after_claim += 1
                else:
                    per.setdefault("k_plane_round[detection]", []).append(us)
        if "k_plane_round[detection]" in per:
            per["k_plane_round[detection, floor round]"] = per["k_plane_round[detection]"][0::MAX_PLANES]
        for k, v in sorted(per.items()):
            v = v[len(v) // 10:]   # past the warm-up
            rows.append(dict(step=step, kernel=k, calls=len(v), avg_us=round(sum(v) / len(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--kernels", default=None, help="run every step under rocprofv3 into this directory and report the kernels' times")
    ap.add_argument("--csv", default=None, help="with --kernels: write the kernel rows here")
    ap.add_argument("--json", default=None, help="with --kernels: write the result line here too")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step_system() if a.step == "system" else step_base()))
        return
    if not a.kernels:
        ap.error("--step or --kernels")
    res, rows = {}, []
    for step, limit in STEPS:
        out = os.path.join(a.kernels, step)
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "track_planes", "--output-format", "csv",
               "--", sys.executable, str(Path(__file__).resolve()), "--step", step]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:   # nothing more is started on the GPU after a step that failed
            print(json.dumps(dict(res, failed=step, returncode=r.returncode)))
            sys.exit(1)
        res[step] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        rows += kernel_rows(out, step)
    res["kernels"] = rows
    if a.csv:
        with open(a.csv, "w", newline="") as fh:
            wr = csv.DictWriter(fh, fieldnames=["step", "kernel", "calls", "avg_us", "min_us", "max_us"], quoting=csv.QUOTE_NONNUMERIC)
            wr.writeheader()
            wr.writerows(rows)
    if a.json:
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
