"""Per-call time of the depth sweep, at stage and at session level, with k_hit_test timed in the same run as the yardstick.

  Context.depth_sweep   the dense two-depth scene of tests/depth_cases.py at 640 x 480 (frames 40 against 10):
                        step 4 / 64 hypotheses / patch radius 2 and step 2 / 128 / 3; wall time per call (with the results' download) and
                        the kernels' own times (the library's HIP-event timing, alva_prof_enable)
  Context.hit_test      the five base taps of tests/hit_cases.py: k_hit_test, for comparison
  AlvaAR.depthImage     in a session on the plane stream of the tests, 40 tracked frames in: wall time per call at step 4 and step 8,
                        and the figures tests/test_gpu_depth_system.py bounds (step 8: answers, share within 3 % of the map's scale)

  python tools/depth_timing.py        prints one JSON line and writes it to profiles/depth_timing.json"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CALLS, WARMUP = 50, 5
W, H, F = 640, 480, 580.0
CONFIGS = [dict(step=4, num_hyp=64, patch_radius=2), dict(step=2, num_hyp=128, patch_radius=3)]


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


def stage():
    import numpy as np
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    import depth_cases as Dc
    import hit_cases as Hc
    ctx = alvaar_amd.Context(0)
    cur = torch.from_numpy(np.array(Dc.two_depth_frame(40, W, H, F)[0])).cuda()
    ref = torch.from_numpy(np.array(Dc.two_depth_frame(10, W, H, F)[0])).cuda()
    calib, T = Dc.calib_of(W, H, F), Dc.T_rc(40, 10)
    res = dict(calls=CALLS, warmup=WARMUP, image=[W, H])
    for cfg in CONFIGS:
        name = "step%d_d%d_r%d" % (cfg["step"], cfg["num_hyp"], cfg["patch_radius"])

        def call():
            return ctx.depth_sweep(cur, ref, calib, T, *Dc.RHO_RANGE, min_texture=4, min_conf=96, **cfg)
        info = call()[3]
        res[name] = dict(info=info.tolist(), wall_us=_timed(call))
        k = capi.kernel_times(call, CALLS)
        res[name]["kernels_avg_us"] = {n: round(us, 2) for n, (_, us) in k.items()}
    P = torch.from_numpy(Hc.base_scene()).cuda()
    taps = [uv for uv, _ in Hc.BASE_TAPS]

    def hit():
        return ctx.hit_test(P, Hc.POSE_BASE, Hc.K_BASE, taps, radius_px=40, num_iterations=64)
    res["hit_test_5_taps"] = dict(wall_us=_timed(hit), kernels_avg_us={n: round(us, 2) for n, (_, us) in capi.kernel_times(hit, CALLS).items()})
    return res


def session():
    import numpy as np
    import torch
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    ar = AlvaAR(W, H, cell_size=12, random_sampling=False, relocalization=True, depth=True)
    first_ok, view = None, 0
    for k in range(110):
        view = 3 * k
        frame = torch.from_numpy(synth.plane_stream_frame(canvas, view, W, H, f)).cuda()
        st = ar.find_camera_pose_device(int(frame.data_ptr()), 33.0 * k)
        if st == 1 and first_ok is None:
            first_ok = k
        if first_ok is not None and k == first_ok + 40:
            break
    out = dict(session_frame=k, session_first_tracked_frame=first_ok, session_ring=len(ar.depth_ring()))
    for step in (4, 8):
        depth, conf, code, info = ar.depthImage(step=step)
        out["session_step%d" % step] = dict(status=info["status"], counts=info["counts"].tolist(), wall_us=_timed(lambda: ar.depthImage(step=step)))
        if info["status"] == 0:
            R, t = synth.plane_camera_pose(view)
            xs, ys = np.meshgrid(np.arange(W // step) * step + step // 2, np.arange(H // step) * step + step // 2)
            d = np.stack([(xs - W * 0.5) / f, (ys - H * 0.5) / f, np.ones(xs.shape)], -1) @ R.T
            ok = code == 0
            ratio = depth[ok].astype(np.float64) / ((4.0 - t[2]) / d[..., 2])[ok]
            err = np.abs(ratio / np.median(ratio) - 1)
            out["session_step%d" % step].update(scale=round(float(np.median(ratio)), 5), within_3pct=round(float((err <= 0.03).mean()), 4),
                                                within_5pct=round(float((err <= 0.05).mean()), 4), median_error=round(float(np.median(err)), 5))
    ar.close()
    return out


def main():
    res = stage()
    res.update(session())
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "depth_timing.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
