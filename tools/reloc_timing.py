"""Wall time of relocalization at 640x480, cell 12 (the 2000-keypoint workload) with the full map window: a plane stream tracked for
N frames, a blackout (the system goes LOST), LOST frames on a blank image, LOST frames on a different world (a full attempt: detection,
description, the global match, the pose solve that fails), then the same world again (the relocalizing frame: attempt + keyframe).

  python tools/reloc_timing.py                      per-frame wall times (JSON line)
  python tools/reloc_timing.py --kernels OUTDIR     the same run once more under rocprofv3 --kernel-trace --stats (a child process);
                                                    prints the match kernels' times from its kernel_stats.csv

Prints one JSON line: map size, median / max wall time of the LOST frames of each kind, the relocalizing frame, the matcher's kernels."""
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


def frames_timed(n_track=110, n_black=8, n_other=12, resume_k=255, n_after=10, speed=3):
    import numpy as np
    import torch
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    import sysdiff
    w, h = 640, 480
    f = sysdiff.intrinsics(w, h)[0]
    canvas, other = synth.texture_canvas(w, h, 5), synth.texture_canvas(w, h, 99)
    fr = [synth.plane_stream_frame(canvas, speed * k, w, h, f) for k in range(n_track)]
    fr += [np.zeros((h, w, 4), np.uint8) + np.array([0, 0, 0, 255], np.uint8)] * n_black
    fr += [synth.plane_stream_frame(other, resume_k + speed * j, w, h, f) for j in range(n_other)]
    fr += [synth.plane_stream_frame(canvas, resume_k + speed * (n_other + j), w, h, f) for j in range(n_after)]
    kind = ["track"] * n_track + ["black"] * n_black + ["other"] * n_other + ["back"] * n_after
    dev = torch.from_numpy(np.stack(fr)).cuda()
    ar = AlvaAR(w, h, cell_size=12, random_sampling=False, relocalization=True)
    out, map_points = [], 0
    for k in range(len(fr)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = ar.find_camera_pose_device(int(dev[k].data_ptr()), 33.0 * k)
        dt = time.perf_counter() - t0
        s = ar.relocalization_stats()
        if st == 4 and not map_points:
            map_points = int(ar.state()[7])
        out.append((kind[k], st, dt, s["last_inliers"]))
    ar.close()
    return out, map_points


def summarise(rows, map_points, n_track=110):
    import numpy as np
    res = dict(width=640, height=480, cell=12, map_points=map_points)
    for name, sel in (("lost_blank", lambda r: r[0] == "black" and r[1] == 4), ("lost_other_world", lambda r: r[0] == "other" and r[1] == 4)):
        t = [r[2] for r in rows if sel(r)]
        if t:
            res[name + "_ms"] = dict(median=round(1e3 * float(np.median(t)), 3), max=round(1e3 * max(t), 3), frames=len(t))
    reloc = [r for r in rows if r[0] == "back" and r[1] == 1]
    if reloc:
        res["relocalizing_frame_ms"] = round(1e3 * reloc[0][2], 3)
        res["relocalizing_inliers"] = reloc[0][3]
    track = [r[2] for r in rows[60:n_track] if r[1] == 1]
    if track:
        res["tracking_frame_median_ms"] = round(1e3 * float(np.median(track)), 3)
    res["statuses"] = "".join(str(r[1]) for r in rows[n_track - 4:])
    return res


def kernel_stats(outdir):
    env = dict(os.environ)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", outdir, "-o", "reloc", "--output-format", "csv", "--",
           sys.executable, str(Path(__file__).resolve()), "--no-kernels-child"]
    subprocess.run(cmd, check=True, env=env, stdout=subprocess.DEVNULL)
    stats = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "reloc" in r["Name"] or "pack_map" in r["Name"]:
                name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0]
                stats[name] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2),
                                   max_us=round(float(r["MaxNs"]) / 1e3, 2))
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", default=None, help="also run under rocprofv3 into this directory and report the match kernels")
    ap.add_argument("--no-kernels-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    rows, mp = frames_timed()
    res = summarise(rows, mp)
    if a.kernels and not a.no_kernels_child:
        res["kernels"] = kernel_stats(a.kernels)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
