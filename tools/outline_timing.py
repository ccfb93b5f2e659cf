"""Per-call time of the plane outlines (alva_plane_outlines) next to plane detection.  Three steps, each a process of its own:

  base     the base scene of tests/hit_cases.py (2800 points: a floor, a wall, clutter) as the detector labels it: Context.detect_planes,
           then Context.plane_outlines with 2 planes and max_vertices = 64, CALLS times each after a warm-up
  circle   the documented worst-case shape: 600 points on a circle, all of them vertices (tests/outline_cases.py), max_vertices = 1024
  system   a tracking session on the synthetic plane stream: AlvaAR.detectPlanes next to AlvaAR.detectPlaneOutlines, wall time per call

  python tools/outline_timing.py --step base        one step, wall time per call (JSON line)
  python tools/outline_timing.py --kernels OUTDIR [--csv FILE]
        every step under `timeout -k 10 <s> rocprofv3 --kernel-trace --stats` (no counters), one after the other, stopping at the first
        that fails; adds the kernels' own times -- k_plane_outline, and k_plane_round's floor round (the first of every four launches)
        from the same run as the yardstick -- and writes them to FILE

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
STEPS = (("base", 120), ("circle", 120), ("system", 180))   # name, time limit in seconds


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


def step_stage(name):
    import torch
    import alvaar_amd
    import outline_cases as O
    import plane_cases as C
    ctx = alvaar_amd.Context(0)
    s = O.scenes()[name]
    P, L = torch.from_numpy(s["P"]).cuda(), torch.from_numpy(s["labels"]).cuda()
    res = dict(points=int(P.shape[0]), planes=len(s["planes"]), calls=CALLS, max_vertices=s["kw"].get("max_vertices", 64))
    if name == "base":
        res["detect_planes_wall_us"], out = _wall(lambda: ctx.detect_planes(P, C.POSE_BASE, **C.BASE_KW))
        res["detect_planes_codes"] = out[1][:, 0].tolist()
    res["plane_outlines_wall_us"], out = _wall(lambda: ctx.plane_outlines(P, L, s["planes"], **s["kw"]))
    res["outline_info"] = out[1][:, :3].tolist()
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
    res["detectPlaneOutlines_wall_us"], full = _wall(lambda: ar.detectPlaneOutlines(rel))
    res.update(points=int(len(out[2])), detect_codes=out[1][:, 0].tolist(), outline_info=full[5][:, :3].tolist())
    ar.close()
    return res


def kernel_rows(outdir, step):
    """k_plane_outline over all its launches, k_plane_round's floor round from the trace (launch 0 of every call's four)"""
    rows = []
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        per = {}
        trace = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        for r in trace:
            for k in ("k_plane_outline", "k_plane_round"):
                if k in r["Kernel_Name"]:
                    per.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        if step != "circle" and "k_plane_round" in per:
            per["k_plane_round[floor round]"] = per["k_plane_round"][0::4]
        for k, v in sorted(per.items()):
            v = v[len(v) // 10:]   # past the warm-up
            rows.append(dict(step=step, kernel=k, calls=len(v), avg_us=round(sum(v) / len(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--kernels", default=None, help="run every step under rocprofv3 into this directory and report the kernels' times")
    ap.add_argument("--csv", default=None, help="with --kernels: write the kernel rows here")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step_system() if a.step == "system" else step_stage(a.step)))
        return
    if not a.kernels:
        ap.error("--step or --kernels")
    res, rows = {}, []
    for step, limit in STEPS:
        out = os.path.join(a.kernels, step)
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "outline", "--output-format", "csv", "--",
               sys.executable, str(Path(__file__).resolve()), "--step", step]
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
    print(json.dumps(res))


if __name__ == "__main__":
    main()
