#!/usr/bin/env python3
"""bench.py -- hot-path throughput on MI355X (see the driver contract).  stdout carries exactly ONE line: a COMPACT JSON object
(< 4 KB, bench_common.compact_line; round 3's 26 KB line could not be parsed by the driver); progress goes to stderr.

A plain run (`--gpus N --steps K --warmup W`) measures the headline and nothing else: set-up, warm-up, the K timed steps, the
outputs of the last one when --dump-outputs DIR is given, the line.  --full adds everything else -- the sustained, look-ahead and
host-fed loops, frame sections, the map merge, local BA, per-kernel tables, rooflines and bounds, the CPU baseline, the secondary
lines of bench_detail.py -- into the line where they fit and into bench_detail.json; the reference's and RCCL's own prints go to
stderr.

HEADLINE (`value`): frames/s of the reference's OWN dataflow through the drop-in surface -- System::findCameraPose
(src/slam/src/system.cpp:106-175) = alva_system_find_camera_pose_device -- on a synthetic 640x480 stream with ~2000 keypoints per frame
(cell size 12 => 2120 cells; BASELINE.json configs[1]), every frame ALREADY resident in HBM, in the STEADY STATE of a long session.  A
"step" is ONE frame through the whole per-frame state machine, every stage consuming what the previous one produced:
    RGBA -> gray -> LK pyramid (+Scharr)                                                        (a2, a3)
    motion-model priors -> forward-backward KLT, with undistortion / bearings                  (a4; visual_frontend.cpp:103-243)
    compaction of the 3-D survivors on the device                                              (:275-298)
    P3P-LMedS (100 hypotheses) -> drop its outliers -> robust PnP (5 LM iterations) on the tracker's OWN survivors (a8, a9; :245-417)
    host bookkeeping of the frame (keypoint updates / removals, motion model, keyframe decision)
and on the frames the reference's keyframe policy selects (every ~18th here): grid Shi-Tomasi detection + ORB description (a5, a6),
triangulation, covisibility, guided Hamming matching to the local map + map-point merges (a7 / f1), local bundle adjustment with outlier
sweep, write-back and culling (a10-a13).  UNTIMED top-up: the session runs until the 30-keyframe window of the reference's mapper is
full, then --warmup W steps.  Then EXACTLY --steps K timed steps (barrier + device sync on both sides, MAX over ranks): `value` =
N K / that time, `ms_per_step` = the time / K.  The top-up aims the window at the middle of a keyframe period, so that it holds the
nearest whole number to its natural share of keyframes; a short window (K = 20 holds 1 or 2 where the natural density is 1.1) still
over- or under-states the long-run rate by ~10 %: --full continues the SAME loop for >= 0.5 s and reports that as `sustained`.

N > 1: `python bench.py --gpus N` runs itself as a child under `python -m torch.distributed.run --nproc-per-node N` (one rank per GPU,
RCCL); launched BY torchrun (WORLD_SIZE set) it checks WORLD_SIZE == --gpus.  It refuses to run when fewer than N devices are visible.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

import bench_common as bc
from bench_common import ROOT, W, H, NKP, HBM_PEAK_GBS, STREAM_FRAMES, SYSTEM_CELL, SystemJob, log, compact_line

import numpy as np
import torch

PMC_FILES = ["r6_pmc_track_klt.json", "r5_pmc_track_klt.json", "r4_pmc_track_klt.json", "r3_pmc_track_klt.json"]   # newest first


def bench_ba(ctx, reps: int = 3):
    from alvaar_amd import synth
    pb = synth.make_ba_problem(20, 3000, 42)
    ctx.local_ba(pb, 5, 0.0)  # warm (scratch allocation)
    t0 = time.perf_counter()
    for _ in range(reps):
        r = ctx.local_ba(pb, 5, 0.0)
    dt = (time.perf_counter() - t0) / reps
    nobs = len(pb["obs_kf"])
    iters = int(r["info"][0]) - 1
    return dict(residual_blocks=nobs, lm_iterations=iters, ms_per_solve=dt * 1e3,
                residual_block_iters_per_s=nobs * iters / dt, final_cost=float(r["info"][2]),
                note="whole alva_local_ba call incl. host structure build, H2D of the problem and D2H of results; the synthetic problem of "
                     "SURVEY.md 8(d) converges by function tolerance 0 after 4 accepted steps (5 iterations allowed)"), pb


def measured_peaks(ctx):
    """FP64 MFMA TFLOP/s and integer VALU Tops/s of this GPU (alva_microbench_peaks): the guide lists neither"""
    import ctypes as C
    from alvaar_amd.capi import lib, check
    lib.alva_microbench_peaks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    a, b = C.c_double(0), C.c_double(0)
    best = [0.0, 0.0]
    for _ in range(3):
        check(lib.alva_microbench_peaks(ctx.h, C.byref(a), C.byref(b)))
        best = [max(best[0], a.value), max(best[1], b.value)]
    return best


def roofline_ba(ctx, pb, peaks):
    """Roofline of the local-BA kernels on the 20 KF x 3000 pts problem: the per-point Jacobian kernel and the pair reduction against
    HBM, the Schur-complement GEMM against the MEASURED FP64-MFMA ceiling (event-timed kernels over whole alva_local_ba calls)."""
    from alvaar_amd import capi
    reps = 3
    kt = capi.kernel_times(lambda: ctx.local_ba(pb, 5, 0.0), reps)
    nobs, npt = len(pb["obs_kf"]), len(pb["anchor_kf"])
    nfree = int((np.asarray(pb["kf_const"]) == 0).sum())
    m = ((6 * nfree + 1 + 15) // 16) * 16                      # reduced camera system + rhs column, padded to 16 x 16 MFMA tiles
    out = {"problem": {"residual_blocks": nobs, "points": npt, "free_keyframes": nfree}, "kernels": {}}
    alg = {
        # per residual block and Jacobian evaluation: 60 B in (2 observations + indices), 112 B stored (J_obs 2x6 + residual)
        "k_point<true, true>": ("hbm", (60 + 112) * nobs),
        "k_pairs": ("hbm", 112 * nobs + 27 * 8 * 400),
        "k_gemm": ("mfma", 2.0 * m * m * npt),                    # G = Z'Z: [m x points] x [points x m], FP64
    }
    for k, (bound, work) in alg.items():
        hit = [n for n in kt if n.startswith(k.split("<")[0])]
        if not hit:
            continue
        calls, us = kt[hit[0]]
        if bound == "hbm":
            a = work / (us * 1e-6) / 1e9
            out["kernels"][hit[0]] = {"bound": "hbm", "avg_us": round(us, 2), "launches_per_solve": calls / reps, "alg_bytes": int(work),
                                      "achieved_GBps": round(a, 1), "peak_GBps": HBM_PEAK_GBS, "frac": a / HBM_PEAK_GBS}
        else:
            a = work / (us * 1e-6) / 1e12
            out["kernels"][hit[0]] = {"bound": "mfma_f64", "avg_us": round(us, 2), "launches_per_solve": calls / reps, "flops": int(work),
                                      "achieved_TFLOPs": round(a, 2), "peak_TFLOPs_measured": round(peaks[0], 1),
                                      "peak_TFLOPs_spec": 78.6, "frac_of_measured": a / peaks[0]}
    tot = sum(c / reps * u for c, u in kt.values())
    out["kernel_us_per_solve"] = round(tot, 1)
    out["largest"] = {n: round(c / reps * u, 1) for n, (c, u) in sorted(kt.items(), key=lambda kv: -kv[1][0] * kv[1][1])[:6]}
    out["note"] = ("one 20 KF x 3000 pts problem cannot fill the chip: the reduced camera system is 109 x 109 and k_solve is a single-workgroup "
                   "dependent chain; MFMA utilisation is reported against the measured v_mfma_f64_16x16x4_f64 ceiling (alva_microbench_peaks)")
    return out


def cpu_baseline(seed: int, warm: int = 600, timed: int = 150, frames_8: int = 150):
    """The reference itself on the host cores of this box (SURVEY.md 8(d) "CPU baseline timing" (1)-(3)), same stream, explicit
    timestamps, fixed-seed sampling, Ceres' wall-clock caps frozen (they would silently skip work):
      (1) System::findCameraPose frames/s on ONE core (the reference is single-threaded: wasm, NO_THREADS Ceres) at cell 12 (the metric's
          ~2000 keypoints) IN THE REGIME `value` IS TIMED IN: the same endless stream (stream_index), `warm` untimed frames -- the
          30-keyframe window full, ~9 500 map points, as SystemJob.warm_to_steady_state leaves the HIP path -- then `timed` frames on the
          clock: this is cpu_baseline.value.  Beside it: the cold start (the first 150 frames: initialisation, young map), 8 independent
          reference Systems on 8 host threads on those same 150 frames (streams are independent: that is how the reference would use 8
          cores), the SHIPPED cell 40 (system.cpp:15), 1280x720 / cell 15 (configs[4]);
      (2) per-stage milliseconds, cpu_stage_table();  (3) one local-BA solve through Ceres with the reference's cost functions.
    Bounded sample: ~25 s of CPU work in total (the untimed warm-up is ~10 s of it)."""
    sys.path.insert(0, str(ROOT / "tests"))
    import oracles
    from alvaar_amd import synth
    if not oracles.ref_available():
        return cpu_baseline_port(seed)
    import sysdiff
    import threading
    from bench_common import stream_index, STREAM_FRAMES
    canvas = synth.texture_canvas(W, H, seed)
    frames = [synth.gray_to_rgba(synth.frame_gray(canvas, k, W, H, noise_seed=11)) for k in range(STREAM_FRAMES)]

    def run(n, out, slot, w=W, h=H, cell=SYSTEM_CELL, fr=frames, skip=0):
        ref = sysdiff.RefSystem(w, h, cell)
        for k in range(skip):
            ref.step(fr[stream_index(k) if fr is frames else k], 33.0 * k)
        kf0 = int(ref.state()[11])
        t0 = time.perf_counter()
        st = [ref.step(fr[stream_index(k) if fr is frames else k], 33.0 * k)[0] for k in range(skip, skip + n)]
        out[slot] = (time.perf_counter() - t0, st, int(ref.state()[2]), len(ref.keyframe_ids()), int(ref.state()[11]) - kf0, int(ref.state()[7]))
        ref.close()
    steady = [None]
    run(timed, steady, 0, skip=warm)
    dts, sts, nkp_s, nkf_s, kf_timed, nmp_s = steady[0]
    one = [None]
    run(150, one, 0)
    dt1, st1, nkp, nkf = one[0][:4]
    res = [None] * 8
    th = [threading.Thread(target=run, args=(frames_8, res, i)) for i in range(8)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt8 = time.perf_counter() - t0
    c40 = [None]
    run(200, c40, 0, cell=40)
    canvas720 = synth.texture_canvas(1280, 720, seed)
    frames720 = [synth.gray_to_rgba(synth.frame_gray(canvas720, k, 1280, 720, noise_seed=11)) for k in range(40)]
    c720 = [None]
    run(40, c720, 0, w=1280, h=720, cell=15, fr=frames720)
    pbba = synth.make_ba_problem(20, 3000, 42)
    t1 = time.perf_counter()
    r = oracles.Ref.local_ba(pbba, 5, 0.0)
    dtb = time.perf_counter() - t1
    desc = lambda tup, n: f"{tup[1].count(3)} initialising, {tup[1].count(1)} tracked, {tup[3]} keyframes, {tup[2]} keypoints at the end, {n} frames"
    return {"value": timed / dts, "unit": "frames/s", "cores": 1, "kind": "reference",
            "sample": f"steady state, frames {warm}-{warm + timed} of the same endless stream, cell {SYSTEM_CELL}: the reference's System::findCameraPose "
                      f"(oracle/_ref) after {warm} untimed frames ({nkf_s} keyframes in the window, {nmp_s} map points), {sts.count(1)} tracked frames "
                      f"timed with {kf_timed} keyframes incl. local BA, {nkp_s} keypoints at the end; + 1 local-BA solve (20 KF x 3000 pts)",
            "cold_start": {"value": 150 / dt1, "unit": "frames/s", "cores": 1,
                           "sample": f"the first 150 frames of the stream: {st1.count(3)} initialising, {st1.count(1)} tracked, {nkf} keyframes with local BA, {nkp} keypoints at the end"},
            "eight_threads": {"value": 8 * frames_8 / dt8, "unit": "frames/s", "cores": 8,
                              "sample": f"8 independent reference Systems on 8 host threads, the first {frames_8} frames each (cold start; the reference is single-threaded; independent streams are its only parallelism)"},
            "system_cell40_shipped": {"value": 200 / c40[0][0], "unit": "frames/s", "cores": 1, "sample": "640x480, cell 40 (system.cpp:15): " + desc(c40[0], 200)},
            "system_1280x720_cell15": {"value": 40 / c720[0][0], "unit": "frames/s", "cores": 1, "sample": "configs[4] geometry: " + desc(c720[0], 40)},
            "local_ba_residual_block_iters_per_s": len(pbba["obs_kf"]) * (int(r["info"][0]) - 1) / dtb,
            "local_ba_ms": dtb * 1e3}


def cpu_baseline_port(seed: int, budget_s: float = 12.0):
    """Fallback when the compiled reference is absent: the stage-wise C restatement on a bounded sample of the stage list."""
    sys.path.insert(0, str(ROOT / "tests"))
    import oracles
    from scipy.spatial.transform import Rotation
    from alvaar_amd import synth
    O = oracles.Orc
    frames = synth.stream_rgba(W, H, 4, seed=seed, noise=True)
    pts = np.random.RandomState(seed).uniform(30, [W - 30, H - 30], (NKP, 2)).astype(np.float32)
    pb = synth.make_pnp_problem(NKP, seed, outlier_frac=0.1, pose_noise=0.01)
    prev = O.rgba2gray(frames[0])
    n, t0 = 0, time.perf_counter()
    while True:
        k = 1 + n % 3
        g = O.rgba2gray(frames[k])
        O.fbklt(prev, g, pts, pts, 3)
        ok, R, t, outl = O.p3p_lmeds(pb["bv"], pb["wpt"], fx=pb["K"][0], fy=pb["K"][1])
        keep = np.setdiff1d(np.arange(NKP), outl)
        q = Rotation.from_matrix(R).as_quat()
        O.pnp_refine(pb["uv"][keep], pb["wpt"][keep], np.concatenate([t, q]), pb["K"])
        n += 1
        if time.perf_counter() - t0 > budget_s or n >= 40:
            break
    dt = time.perf_counter() - t0
    return {"value": n / dt, "unit": "frames/s", "cores": 1, "kind": "port",
            "sample": f"{n} tracking frames (gray, 2 LK pyramids, fb-KLT 3 levels, P3P-LMedS, PnP) through the C restatement; no keyframes"}


def launch_latency(ctx):
    import ctypes as C
    from alvaar_amd.capi import lib, check
    lib.alva_microbench_launch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    a, b = C.c_double(0), C.c_double(0)
    best = [1e9, 1e9]
    for _ in range(3):
        check(lib.alva_microbench_launch(ctx.h, 200, C.byref(a), C.byref(b)))
        best = [min(best[0], a.value), min(best[1], b.value)]
    return best


def pmc_reference(kernel: str, sources: list[str]):
    """HBM traffic and L2 hit rate of `kernel` from the PMC passes committed under profiles/ (rocprofv3 --pmc cannot run inside this
    process).  The file is stamped with the commit and the sha256 of the kernel's source files at capture time: if the sources have
    changed since, the numbers are reported as stale (null) instead of silently carried over."""
    import hashlib
    f = next((p for p in (ROOT / "profiles" / n for n in PMC_FILES) if p.exists()), ROOT / "profiles" / PMC_FILES[-1])
    if not f.exists():
        return None, None, {"file": None, "note": "no PMC capture committed for this kernel"}
    j = json.loads(f.read_text())
    now = {src: hashlib.sha256((ROOT / src).read_bytes()).hexdigest()[:16] for src in sources}
    stale = any(j.get("source_sha16", {}).get(src) != h for src, h in now.items())
    k = j.get("kernels", {}).get(kernel, {})
    stamp = {"file": str(f.relative_to(ROOT)), "captured_at_commit": j.get("commit"), "source_sha16_at_capture": j.get("source_sha16"), "stale": stale}
    if stale:
        return None, None, stamp
    return k.get("hbm_bytes_per_launch"), k.get("l2_hit_rate"), stamp



def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(n: int) -> None:
    """`python bench.py --gpus N` with no WORLD_SIZE in the environment: run N ranks (one per GPU) under torch.distributed.run.
    Fails loudly when the box shows fewer than N devices -- it must never print an `n_gpus: 1` line for an N-GPU request."""
    have = torch.cuda.device_count()
    if have < n:
        sys.exit(f"bench.py: --gpus {n} requested but only {have} GPU(s) visible; refusing to measure fewer ranks than asked for")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), str(ROOT / "bench.py"), *sys.argv[1:]]
    log("launching " + " ".join(cmd))
    sys.stdout.flush()
    # a fresh child process, not exec: this process may already have touched the GPU (device_count above)
    rc = subprocess.call(cmd)
    sys.exit(128 - rc if rc < 0 else rc)     # killed by signal S: exit 128 + S, as a shell reports it


def dump_outputs(out_dir: str, sysjob) -> None:
    """What the caller of the timed path holds after its last step: the 16 floats of the pose the call wrote, its status, and the
    frame's keypoints (ids, pixel positions, 3-D flags).  A few tens of KB in all."""
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    ids, px, is3d = sysjob.ar.keypoints()
    arrays = {"pose": sysjob.ar._pose, "status": np.array([sysjob.last_status]), "keypoint_ids": ids,
              "keypoint_px": px, "keypoint_is3d": is3d}
    for name, a in arrays.items():
        np.save(d / f"{name}.npy", np.asarray(a, np.float32 if name in ("pose", "keypoint_px") else np.float64))
    log(f"outputs of the last timed step -> {d}")


def write_detail(detail: dict) -> str:
    txt = json.dumps(detail, indent=1)
    (ROOT / "bench_detail.json").write_text(txt)
    out_dir = ROOT / "gpurun_out"
    if out_dir.is_dir():
        (out_dir / "bench_detail.json").write_text(txt)
    return "bench_detail.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: sustained / look-ahead / host-fed loops, frame sections, map merge, local BA, "
                         "rooflines and bounds, CPU baseline, secondary lines -> bench_detail.json.  Off: the headline line only")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last timed step returned to the caller "
                                                           "(pose, status, the frame's keypoints) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: no CPU baseline")
    ap.add_argument("--config", choices=["640x480", "720p-streams"], default="640x480",
                    help="640x480 = BASELINE configs[1] (the metric's configuration, default); 720p-streams = configs[4]: one independent "
                         "1280x720 stream (cell 15 => 4080 cells) per GPU, what an 8-GPU run of that config executes on every rank")
    ap.add_argument("--quick", action="store_true", help="--full: headline, roofline, local BA and CPU baseline only (no secondary lines in bench_detail.json)")
    ap.add_argument("--launcher", action="store_true", help="run under torch.distributed.run even for --gpus 1 (the N > 1 path's launcher, testable on a 1-GPU box)")
    ap.add_argument("--merge-every", type=int, default=4, help="shared-map merge (RCCL all_gather + fuse) every this many keyframes in the merge line")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and (args.gpus > 1 or args.launcher):
        launch_ranks(args.gpus)            # exits with the ranks' status
    if env_world is not None and int(env_world) != args.gpus:
        sys.exit(f"bench.py: launched with WORLD_SIZE={env_world} but --gpus {args.gpus}; they must agree")
    # stdout carries exactly one line, the JSON: the compiled reference (cpu_baseline) and RCCL print to the C-level stdout, so fd 1 is
    # pointed at stderr for the duration of the run and the line is written to the saved descriptor at the end
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    from alvaar_amd import multi
    import torch.distributed as td
    shard = multi.shard_from_env()
    rank, world, local = shard.rank, shard.world, shard.local_rank
    if local >= torch.cuda.device_count():
        sys.exit(f"bench.py: rank {rank} has LOCAL_RANK {local} but only {torch.cuda.device_count()} GPU(s) are visible")
    torch.cuda.set_device(local)
    # "nccl" IS RCCL on ROCm.  The data path has no collective (independent streams); the group carries the barrier + timing reduction
    # and the optional shared-map merge -- with --full initialised for ONE rank too, so that the merge line runs on RCCL in every full run.
    try:
        dist = multi.init_process_group(shard, "nccl", force=args.full)
        dist_err = None
    except Exception as e:   # a single-GPU box without a usable RCCL still measures the data path
        if world > 1:
            raise
        dist, dist_err = False, repr(e)

    is720 = args.config == "720p-streams"
    Wc, Hc, cellc = (1280, 720, 15) if is720 else (W, H, SYSTEM_CELL)
    sysjob = SystemJob(local, seed=shard.stream_seed, width=Wc, height=Hc, cell=cellc)

    def timed(fn, warmup, steps):
        """W untimed + exactly K timed steps, barrier + device sync on both sides, MAX over ranks"""
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        if dist:
            td.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if dist:
            el = multi.max_over_ranks(el, torch.device("cuda", local))
            td.barrier()
        torch.cuda.synchronize()
        return el

    # ---- headline: the System surface, frames resident in HBM, STEADY STATE (30-keyframe window full; ~600 untimed frames)
    log("warming the session into steady state")
    extra, period = sysjob.warm_to_steady_state(then_untimed=args.warmup)
    log(f"steady state after {extra} frames, keyframe period {period}")
    ar = sysjob.ar
    kf_before = int(ar.state()[11])
    dt = timed(sysjob.step, args.warmup, args.steps)
    kf_in_window = int(ar.state()[11]) - kf_before
    hist_timed = list(sysjob.status_hist)
    value = world * args.steps / dt
    log(f"{args.steps} timed steps: {args.steps / dt:.0f} frames/s per rank")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, sysjob)
    head = {"metric": "frames/sec @640x480 2000kp; local-BA residuals/sec (20KFx3k pts)",
            "value": value, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8/i16 image stages, f32 KLT, f64 pose+BA", "data": "synthetic",
            "config": {"workload": ("configs[4]: 1280x720 RGBA stream per GPU, ~4000 keypoints/frame (cell 15), " if is720 else
                                    "configs[1]: 640x480 RGBA stream, ~2000 keypoints/frame (cell 12), ") +
                                   "System::findCameraPose dataflow (fb-KLT -> P3P-LMedS -> PnP; keyframes: detect + describe, triangulate, "
                                   "map matching, local BA) via alva_system_find_camera_pose_device, steady state, frames resident in HBM",
                       "value_is": "frames/s over exactly --steps timed steps (steps_timed); --full adds `sustained`: the same loop continued "
                                   "for >= 0.5 s",
                       "keyframe_period_frames": period,
                       "parallelism": f"{world} independent camera streams, one per GPU, no collective on the data path"},
            "steps_timed": args.steps, "seconds_timed": dt, "keyframes_timed": kf_in_window}
    if not args.full:
        if rank == 0:
            os.write(real_stdout, (compact_line(head) + "\n").encode())
        if dist:
            td.barrier()
            td.destroy_process_group()
        return
    # the same loop continued for at least 0.5 s (the same count on every rank): `sustained`
    long_steps = max(args.steps, int(0.6 * args.steps / max(dt, 1e-9)) + 1)
    if dist and world > 1:
        t = torch.tensor([long_steps], device=f"cuda:{local}")
        td.all_reduce(t, op=td.ReduceOp.MAX)
        long_steps = int(t.item())
    kf_before = int(ar.state()[11])
    dt_long = timed(sysjob.step, 0, long_steps)
    kf_long = int(ar.state()[11]) - kf_before
    log(f"sustained: {long_steps / dt_long:.0f} frames/s per rank ({long_steps} steps)")
    ar.timing()
    ar.timing_keyframe()
    kf0 = int(ar.state()[11])
    n_sec = 400
    for _ in range(n_sec):
        sysjob.step()
    sections, kf_detail, n_kf_sec = ar.timing(), ar.timing_keyframe(), int(ar.state()[11]) - kf0
    sys_state = ar.state()
    sys_counters = ar.counters()
    # the same loop with look-ahead hints (the caller names the next frame: its images are built behind this frame's pose solve)
    kf_before = int(ar.state()[11])
    dt_ahead = timed(sysjob.step_ahead, 5, long_steps)
    kf_ahead = int(ar.state()[11]) - kf_before
    log(f"with next-frame hints: {long_steps / dt_ahead:.0f} frames/s per rank")
    # PCIe-fed variant: host RGBA in through AlvaAR.findCameraPose (memImg.write + the registered buffer read in place), same length
    dt_host = timed(sysjob.step_host, 5, long_steps)
    ar.timing()
    for _ in range(100):
        sysjob.step_host()
    sections_host = ar.timing()
    t0 = time.perf_counter()
    for i in range(50):
        np.copyto(ar.mem_img, sysjob.host_frames[i])
    copy_us = (time.perf_counter() - t0) / 50 * 1e6
    log(f"host-fed: {long_steps / dt_host:.0f} frames/s per rank")
    # ---- the optional shared-map merge on the process group's backend (RCCL): pack -> ONE all_gather_into_tensor -> fuse on the GPU
    merge = None
    try:
        import alvaar_amd
        mctx = alvaar_amd.Context(local)
        rounds = []
        for _ in range(3):
            for _ in range(int(max(period, 8) * args.merge_every)):
                sysjob.step()
            if dist:
                td.barrier()
            rounds.append(multi.map_merge_round(ar, mctx, shard))
        last = rounds[-1]
        merge = {k_: last.get(k_) for k_ in last if not k_.endswith("_us")}
        merge.update({"every_keyframes": args.merge_every, "world": world,
                      "pack_us": round(min(r["pack_us"] for r in rounds), 1), "all_gather_us": round(min(r["all_gather_us"] for r in rounds), 1),
                      "fuse_us": round(min(r["fuse_us"] for r in rounds), 1),
                      "note": "north_star's optional shared-map merge: this rank's 3-D map points (id, xyz, descriptor medoid; 64 B records) -> one "
                              "all_gather_into_tensor on the process group (RCCL over xGMI when N > 1; one rank fuses nothing: the rule only fuses "
                              "across streams) -> alva_fuse_map_points -> absorbed ids re-pointed in this rank's map; NOT part of `value`"})
    except Exception as e:
        merge = {"error": repr(e), "process_group_error": dist_err}
    log(f"map merge: {merge}")
    if dist and world == 1:
        # one rank: nothing below needs the group, and RCCL's helper threads would compete with the 16 worker threads of the secondary
        # group lines for the container's CPU quota (measured: 32 sessions 13.4 k frames/s inside this process, 18 - 19 k stand-alone)
        td.destroy_process_group()
        dist = False
    if rank == 0:
        import alvaar_amd
        from alvaar_amd import capi
        bctx = alvaar_amd.Context(local)
        log("local BA")
        ba, ba_pb = bench_ba(bctx)
        peaks = measured_peaks(bctx)
        lat_dep, lat_rt = launch_latency(bctx)
        P = Wc * Hc
        # ---- roofline: per-KERNEL durations from HIP events recorded on each launch stream, over a further pass of the headline loop
        # (the events cost a few us per launch, so they stay out of the pass that gives `value`)
        # one whole period of the synthetic stream (forward and back through its frames): the tracker's launch time follows the frame's
        # content (its slowest slots), and a 200-step window of it was 10 % off the rocprofv3 average over the whole command in one run
        PROF_STEPS = 2 * (STREAM_FRAMES - 1)
        log("kernel times of the headline loop")
        ar.klt_work()
        kt = capi.kernel_times(sysjob.step, PROF_STEPS)
        klt_levels, klt_slots = ar.klt_work()
        nkp = int(sys_state[2])
        n3d = int(sys_state[4])
        PYR = 1 + 1 / 4 + 1 / 16 + 1 / 64
        # ALGORITHMIC bytes per launch (SURVEY.md 8(d) per-unit figures x the units one launch processes)
        alg = {
            "k_level0<true>": 4 * P + 2 * P,                        # RGBA in; gray copy + padded level 0 out
            "k_pyr_rest": P + (P / 4 + P / 16 + P / 64) + 4 * P * PYR,   # level 0 in; levels 1-3 + every level's Scharr pair out
            # the two above as ONE launch (round 6): RGBA in; gray copy + padded levels 0-3 + every level's Scharr pair out
            "k_pyr_all": 4 * P + 2 * P + (P / 4 + P / 16 + P / 64) + 4 * P * PYR,
            # fb-KLT, one launch per frame over every slot: the four levels of BOTH pyramids once (gray u8 + Ix,Iy i16 = 5 B/px per level)
            # + the slot table in (33 B per slot) + per-slot results out (1 + 8 + 8 + 24 B, device memory)
            "k_track_klt": 2 * 5 * P * PYR + 33 * nkp + 41 * nkp,
            "k_track_stage_in": 2 * 33 * nkp,                       # slot table: pinned host -> device
            "k_track_compact": 42 * nkp + 41 * nkp + 64 * n3d,      # per-slot results in; the same to pinned host + correspondences of the pose solve out
        }
        per_frame = {k: v[0] / PROF_STEPS * v[1] for k, v in kt.items()}
        kernels = {k: {"launches_per_frame": round(v[0] / PROF_STEPS, 3), "avg_us": round(v[1], 2),
                       **({"alg_bytes": int(alg[k]), "GBps": round(alg[k] / (v[1] * 1e-6) / 1e9, 1)} if k in alg else {})}
                   for k, v in sorted(kt.items(), key=lambda kv: -per_frame[kv[0]])[:28]}
        dom = max(per_frame, key=per_frame.get)
        hbm_dom = max((k for k in per_frame if k in alg), key=per_frame.get)
        achieved = alg[hbm_dom] / (kt[hbm_dom][1] * 1e-6) / 1e9
        traffic, l2_hit, pmc_stamp = pmc_reference(hbm_dom, ["alvaar_amd/csrc/klt.hip", "alvaar_amd/csrc/stages_hip.hip", "alvaar_amd/csrc/track_slots.hpp"])
        klt_us_total = kt["k_track_klt"][0] * kt["k_track_klt"][1] if "k_track_klt" in kt else None
        # ---- SURVEY.md 8(d), last table row: the three end-to-end bounds of one frame next to the achieved number
        chain = ["k_level0<true>", "k_pyr_rest", "k_pyr_all", "k_track_stage_in", "k_track_klt", "k_track_compact", "k_p3p_pnp_s", "k_pose_all", "k_p3p_s", "k_p3p", "k_pnp"]
        chain_launches = sum(round(kt[k][0] / PROF_STEPS) for k in chain if k in kt)
        chain_kernel_us = sum(per_frame.get(k, 0.0) for k in chain)
        launches_per_frame = sum(v[0] for v in kt.values()) / PROF_STEPS
        bounds = {
            "hbm_frames_per_s": HBM_PEAK_GBS * 1e9 / (18.3 * P),
            "pcie_gen5_host_fed_frames_per_s": 63e9 / (4 * P),
            "launch_latency_frames_per_s": 1e6 / (chain_launches * lat_dep + 2 * lat_rt),
            "dependent_kernel_chain_frames_per_s": 1e6 / max(chain_kernel_us, 1e-9),
            "achieved_sustained_frames_per_s": long_steps / dt_long,
            "inputs": {"irreducible_hbm_bytes_per_frame": int(18.3 * P), "rgba_bytes_per_frame": 4 * P, "pcie_GBps": 63.0,
                       "us_per_dependent_empty_launch": round(lat_dep, 2), "us_launch_plus_sync_round_trip": round(lat_rt, 2),
                       "launches_on_the_tracking_chain": chain_launches, "host_waits_per_tracking_frame": 2,
                       "launches_per_frame_all": round(launches_per_frame, 2), "tracking_chain_kernel_us": round(chain_kernel_us, 1)},
            "note": "SURVEY.md 8(d): HBM roof = 8 TB/s over the irreducible 18.3 P bytes of a frame; PCIe Gen5 x16 upload of the RGBA frame for a "
                    "host-fed stream; launch latency = the tracking frame's dependent launches at the measured empty-launch rate + its two host "
                    "waits at the measured launch+sync round trip (alva_microbench_launch); dependent_kernel_chain = the same chain's measured "
                    "kernel durations with zero gaps -- the bound this single stream actually runs against"}
        us = lambda d, n: {a: round(1e6 * b / max(n, 1), 1) for a, b in d.items()}
        log("assembling the record")
        out = {
            **head,
            "config": {**head["config"],
                       "frames_resident_in_hbm": True, "stream": f"{STREAM_FRAMES} frames, (2, 1) px per frame, forwards / backwards",
                       "keypoints_per_frame": nkp, "keypoints_3d": n3d, "keyframes_in_map": int(sys_state[6]), "map_points": int(sys_state[7]),
                       "keyframes_created_so_far": int(sys_state[11]),
                       "status_histogram_reset_init_tracked": {"1_tracked": hist_timed[1], "2_reset": hist_timed[2], "3_initialising": hist_timed[3]},
                       "untimed_frames_to_steady_state": extra,
                       "env": {"GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES")}},
            "natural_keyframes_timed": (args.steps / period) if period else None,
            "sustained": {"frames_per_s": world * long_steps / dt_long, "steps": long_steps, "seconds": dt_long, "keyframes": kf_long,
                          "ms_per_step": dt_long / long_steps * 1e3, "over_value": world * long_steps / dt_long / value},
            "system_lookahead": {"frames_per_s": world * long_steps / dt_ahead, "ms_per_step": dt_ahead / long_steps * 1e3, "steps": long_steps,
                                 "keyframes": kf_ahead,
                                 "note": "the sustained loop with alva_system_hint_next_frame_device before every call; NOT `value`: the "
                                         "reference's findCameraPose is handed one frame per call"},
            "system_surface": {"frames_per_s": world * long_steps / dt_host, "ms_per_step": dt_host / long_steps * 1e3, "steps": long_steps,
                               "caller_copy_us": round(copy_us, 1),
                               "per_frame_us_host_fed": us(sections_host, 100),
                               "note": "the same loop fed from HOST memory exactly as src/system.js does: memImg.write(frame) = one 1.2 MB copy into the "
                                       "wrapper's ONE registered frame buffer, read in place over PCIe by the gray / pyramid kernel"},
            "bounds": bounds,
            "frame_sections_us": {"per_frame": us(sections, n_sec), "frames": n_sec, "keyframes": n_kf_sec,
                                  "per_keyframe_detail": us(kf_detail, n_kf_sec),
                                  "ms_per_keyframe": round(1e3 * (sections["keyframe_create"] + sections["mapping"]) / max(n_kf_sec, 1), 3),
                                  "local_ba_solves_total": sys_counters["ba_solves"],
                                  "note": "host wall-clock per section of the frame loop (alva_system_debug_timing); keyframe sections averaged over ALL frames in per_frame"},
            "klt": {"keypoint_levels_per_s": (klt_levels / (klt_us_total * 1e-6)) if klt_us_total else None,
                    "keypoint_levels_per_frame": klt_levels / PROF_STEPS, "slots_per_frame": klt_slots / PROF_STEPS,
                    "kernel_us": kt.get("k_track_klt", (0, None))[1], "l2_hit_rate": l2_hit, "pmc": pmc_stamp},
            "map_merge": merge,
            "local_ba": ba,
            "roofline_ba": roofline_ba(bctx, ba_pb, peaks),
            "measured_peaks": {"mfma_f64_TFLOPs": peaks[0], "valu_int32_Tops": peaks[1],
                               "note": "alva_microbench_peaks: independent v_mfma_f64_16x16x4_f64 chains / xor-popcount-add chains on every SIMD"},
            "roofline": {"bound": "hbm", "limiter": "latency", "kernel": hbm_dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_stamp": pmc_stamp,
                         "avg_us": kt[hbm_dom][1], "alg_bytes_per_launch": int(alg[hbm_dom]),
                         "largest_kernel_by_time": dom,
                         "note": "algorithmic bytes / HIP-event kernel time of the dominant kernel against the 8 TB/s HBM peak.  HBM is the contract's "
                                 "axis, not what limits this kernel: traffic ~ algorithmic bytes (nothing re-read) and the frame is 1.2 MB; the "
                                 "kernel runs as long as its slowest keypoint's dependent LK iterations (limiter: latency)"},
            "kernels": kernels,
        }
        if not args.no_cpu_baseline and world == 1:   # the contract: reference CPU path timed on rank 0 at N = 1 only
            log("cpu baseline")
            out["cpu_baseline"] = cpu_baseline(shard.stream_seed)
        out["detail_file"] = "bench_detail.json"
        write_detail(out)
        secondary = not args.quick and world == 1
        if secondary:
            # the three secondary figures the driver's record should carry (~10 s): 32 sessions on this GPU through
            # alva_system_group, the 1280x720 System stream (configs[4] geometry), configs[2]'s ORB + Hamming frame -- measured BEFORE
            # the line is printed, flat keys in the compact line
            import bench_detail
            sysjob.ar.close()
            del sysjob
            torch.cuda.empty_cache()
            out.update(bench_detail.run_secondary(local, shard.stream_seed, args.steps, bctx, ba_pb, peaks, is720, part="line"))
            write_detail(out)
        # the driver's line: printed NOW, before the remaining secondary lines -- nothing else is ever written to stdout
        os.write(real_stdout, (compact_line(out) + "\n").encode())
        log("compact line written")
        if secondary:
            out.update(bench_detail.run_secondary(local, shard.stream_seed, args.steps, bctx, ba_pb, peaks, is720,
                                                  with_cpu=not args.no_cpu_baseline, part="rest"))
            write_detail(out)
            log("bench_detail.json written")
    if dist:
        td.barrier()
        td.destroy_process_group()


if __name__ == "__main__":
    main()
