"""Per-launch time of light estimation (alva_light_bin, alva_light_fuse, alva_light_estimate) beside the pyramid build it follows, and
what a session pays for it.

  stages    at 640 x 480 and 1280 x 720, in one run: the kernels' own times (the library's HIP-event timing, alva_prof_enable) of
            k_light_bin, k_light_fuse and k_light_estimate, and of k_pyr_all on the same frame (the launch the bin is queued behind in
            a session: it has just pulled the frame through L2); the wall time per call of alva_light_estimate, which waits and
            downloads
  session   sustained frames/s of a session on the tests' plane stream (device frames, no look-ahead hint) with light on and with light
            off, in the same process, alternating, the better of three passes each; and the wall time of lightEstimate()

  python tools/light_timing.py        prints one JSON line and writes it to profiles/light_timing.json"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CALLS, WARMUP = 200, 20
SIZES = [(640, 480), (1280, 720)]
STEP, MIN_PIXELS, W_NEW, W_MAX = 4, 64, 32, 224


def stages():
    import numpy as np
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    ctx = alvaar_amd.Context(0)
    res = {}
    R = np.array([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]]).reshape(-1)
    for w, h in SIZES:
        rgba = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (h, w, 4), dtype=np.uint8)).cuda()
        calib = (0.9 * w, 0.9 * w, w / 2, h / 2, 0.0, 0.0, 0.0, 0.0)
        pyr = capi.Pyramid(ctx, w, h)
        gray = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        acc = torch.zeros(capi.LIGHT_ACC_WORDS, dtype=torch.int64, device="cuda")
        state = torch.zeros(capi.LIGHT_STATE_BYTES, dtype=torch.uint8, device="cuda")

        def frame():   # what a session enqueues per frame, in its order
            pyr.build_from_rgba(rgba, gray)
            ctx.light_bin(rgba, calib, R, STEP, acc=acc)
            ctx.light_fuse(acc, state, MIN_PIXELS, W_NEW, W_MAX)

        def estimate():
            return ctx.light_estimate(state)

        for _ in range(WARMUP):
            frame()
            estimate()
        ctx.sync()
        out = dict(kernels={n: dict(launches_per_call=c / CALLS, avg_us=round(us, 2)) for n, (c, us) in capi.kernel_times(frame, CALLS).items()})
        out["kernels"].update({n: dict(launches_per_call=c / CALLS, avg_us=round(us, 2)) for n, (c, us) in capi.kernel_times(estimate, CALLS).items()})
        t = []
        for _ in range(CALLS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            estimate()
            t.append(time.perf_counter() - t0)
        out["estimate_wall_us"] = dict(median=round(1e6 * float(np.median(t)), 1), max=round(1e6 * max(t), 1))
        out["info"] = estimate()[4].tolist()
        res["%dx%d" % (w, h)] = out
        pyr.close()
    ctx.close()
    return dict(calls=CALLS, warmup=WARMUP, step=STEP, stages=res)


def session():
    import numpy as np
    import torch
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    W, H, N = 640, 480, 110
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    frames = torch.from_numpy(np.stack([synth.plane_stream_frame(canvas, 3 * k, W, H, f) for k in range(N)])).cuda()
    ptrs = [int(frames[k].data_ptr()) for k in range(N)]
    best = {True: 0.0, False: 0.0}
    tracked, est = {}, None
    for _ in range(3):
        for light in (False, True):
            ar = AlvaAR(W, H, cell_size=12, random_sampling=False, light=light)
            for k in range(10):                      # the first frames initialise: not part of the sustained rate
                ar.find_camera_pose_device(ptrs[k], 33.0 * k)
            torch.cuda.synchronize()
            n_ok = 0
            t0 = time.perf_counter()
            for k in range(10, N):
                n_ok += ar.find_camera_pose_device(ptrs[k], 33.0 * k) == 1
            dt = time.perf_counter() - t0
            best[light] = max(best[light], (N - 10) / dt)
            tracked[light] = n_ok
            if light:
                t = []
                for _ in range(60):
                    t1 = time.perf_counter()
                    info = ar.lightEstimate()[4]
                    t.append(time.perf_counter() - t1)
                est = dict(median=round(1e6 * float(np.median(t[10:])), 1), max=round(1e6 * max(t[10:]), 1), info=info.tolist())
            ar.close()
    return dict(session=dict(image=[W, H], frames=N - 10, tracked=dict(light_on=tracked[True], light_off=tracked[False]),
                             frames_per_s=dict(light_on=round(best[True], 1), light_off=round(best[False], 1)),
                             per_frame_cost_us=round(1e6 / best[True] - 1e6 / best[False], 1), lightEstimate_wall_us=est))


def main():
    res = stages()
    res.update(session())
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "light_timing.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
