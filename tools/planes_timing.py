"""Per-call time of the hit test and of plane detection on the base scene of tests/hit_cases.py (2800 points: a floor, a wall, clutter):
Context.hit_test with the five base taps and Context.detect_planes (thickness 0.01, 48 inliers, 4 planes, 128 iterations), CALLS times
each after a warm-up.

  python tools/planes_timing.py                     wall time per call (JSON line)
  rocprofv3 --kernel-trace --stats -- python tools/planes_timing.py
                                                    the same run with the kernels' own times in the profiler's kernel_stats.csv
  python tools/planes_timing.py --kernels OUTDIR    does that in a child process and adds k_hit_test's and k_plane_round's rows

Prints one JSON line: median wall time per call of each, and with --kernels the kernels' calls, average and maximum."""
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


def timed():
    import numpy as np
    import torch
    import alvaar_amd
    import hit_cases as H
    import plane_cases as C
    ctx = alvaar_amd.Context(0)
    P = torch.from_numpy(H.base_scene()).cuda()
    taps = [uv for uv, _ in H.BASE_TAPS]
    res = dict(points=int(P.shape[0]), calls=CALLS)
    for name, call in (("hit_test_5_taps", lambda: ctx.hit_test(P, H.POSE_BASE, H.K_BASE, taps, radius_px=40, num_iterations=64)),
                       ("detect_planes", lambda: ctx.detect_planes(P, H.POSE_BASE, **C.BASE_KW))):
        t = []
        for k in range(WARMUP + CALLS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call()
            t.append(time.perf_counter() - t0)
        res[name + "_wall_us"] = dict(median=round(1e6 * float(np.median(t[WARMUP:])), 1), max=round(1e6 * max(t[WARMUP:]), 1))
        res[name + "_codes"] = out[1][:, 0].tolist()
    return res


def kernel_stats(outdir):
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", outdir, "-o", "planes", "--output-format", "csv", "--",
           sys.executable, str(Path(__file__).resolve())]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    stats = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "k_hit_test" in r["Name"] or "k_plane_round" in r["Name"]:
                name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0]
                stats[name] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2), min_us=round(float(r["MinNs"]) / 1e3, 2),
                                   max_us=round(float(r["MaxNs"]) / 1e3, 2))
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", default=None, help="also run under rocprofv3 into this directory and report the two kernels")
    a = ap.parse_args()
    res = timed()
    if a.kernels:
        res["kernels"] = kernel_stats(a.kernels)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
