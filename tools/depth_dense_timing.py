"""Per-call time of dense depth (alva_depth_fuse, alva_depth_fill), at stage and at session level, with the sweep timed in the same run.

  Context.depth_sweep / depth_fuse / depth_fill
                        the dense two-depth scene of tests/depth_cases.py at 640 x 480 (frames 40 against 10), step 4 / 64 hypotheses /
                        patch radius 2 and step 2 / 128 / 3, max_level 5: the sweep's outputs fused with a state carried from frame 10,
                        then filled; wall time per call (with the results' download) and the kernels' own times (the library's
                        HIP-event timing, alva_prof_enable)
  AlvaAR.depthDense / depthImage
                        in a session on the plane stream of the tests: wall time per call of both, for both configurations.  A
                        depthDense call fuses once per frame, so the fusing call is timed over 55 consecutive frames, one call each
                        (from 30 tracked frames in; the first 5 are warm-up); then, on the last of them, the second call on a frame,
                        which fills without fusing, and depthImage

  python tools/depth_dense_timing.py        prints one JSON line and writes it to profiles/depth_dense_timing.json"""
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
LEVEL = 5
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


def _name(cfg):
    return "step%d_d%d_r%d" % (cfg["step"], cfg["num_hyp"], cfg["patch_radius"])


def stage():
    import numpy as np
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    import dense_cases as Dn
    import depth_cases as Dc
    ctx = alvaar_amd.Context(0)
    cur = torch.from_numpy(np.array(Dc.two_depth_frame(40, W, H, F)[0])).cuda()
    ref = torch.from_numpy(np.array(Dc.two_depth_frame(10, W, H, F)[0])).cuda()
    calib, T = Dc.calib_of(W, H, F), Dc.T_rc(40, 10)
    res = dict(calls=CALLS, warmup=WARMUP, image=[W, H], max_level=LEVEL)
    for cfg in CONFIGS:
        step = cfg["step"]
        gw, gh = W // step, H // step
        raw = ctx.depth_sweep(cur, ref, calib, T, *Dc.RHO_RANGE, min_texture=4, min_conf=96, **cfg)
        meas = tuple(torch.from_numpy(a).cuda() for a in raw[:3])
        prev = tuple(torch.from_numpy(a).cuda() for a in Dn.state_of(Dc.grid_truth(Dc.two_depth_frame(10, W, H, F)[1], step), 11))
        T_cp = Dn.T_cp(10, 40)

        def sweep():
            return ctx.depth_sweep(cur, ref, calib, T, *Dc.RHO_RANGE, min_texture=4, min_conf=96, **cfg)

        def fuse():
            return ctx.depth_fuse(prev, T_cp, calib, W, H, step, meas)
        rho, w, src, finfo = fuse()
        state = (torch.from_numpy(rho).cuda(), torch.from_numpy(w).cuda())

        def fill():
            return ctx.depth_fill(state[0], state[1], cur, step, 2.0 * Dc.RHO_RANGE[1], LEVEL)
        linfo = fill()[2]
        out = dict(grid=[gw, gh], sweep_info=raw[3].tolist(), fuse_info=finfo.tolist(), fill_info=linfo.tolist())
        for name, call in (("sweep", sweep), ("fuse", fuse), ("fill", fill)):
            out[name + "_wall_us"] = _timed(call)
            out[name + "_kernels"] = {n: dict(launches_per_call=c / CALLS, avg_us=round(us, 2)) for n, (c, us) in capi.kernel_times(call, CALLS).items()}
        res[_name(cfg)] = out
    return res


def session():
    import numpy as np
    import torch
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    out = {}
    for cfg in CONFIGS:
        ar = AlvaAR(W, H, cell_size=12, random_sampling=False, relocalization=True, depth=True)
        first_ok, k, fusing = None, 0, []
        kw = dict(cfg, max_level=LEVEL)
        for k in range(110):
            frame = torch.from_numpy(synth.plane_stream_frame(canvas, 3 * k, W, H, f)).cuda()
            st = ar.find_camera_pose_device(int(frame.data_ptr()), 33.0 * k)
            if st == 1 and first_ok is None:
                first_ok = k
            if first_ok is not None and k >= first_ok + 20:   # (ten calls first, so that there is a state to warp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                info = ar.depthDense(**kw)[4]
                if k >= first_ok + 30:
                    fusing.append(time.perf_counter() - t0)
            if len(fusing) == WARMUP + CALLS:
                break
        fusing = fusing[WARMUP:]
        raw = ar.depthImage(**cfg)
        out["session_" + _name(cfg)] = dict(
            frame=k, first_tracked_frame=first_ok, status=info["status"], fuse=info["fuse"].tolist(), filled=info["filled"], empty=info["empty"],
            raw_counts=raw[3]["counts"].tolist(),
            depthDense_fusing_wall_us=dict(median=round(1e6 * float(np.median(fusing)), 1), max=round(1e6 * max(fusing), 1), calls=len(fusing)),
            depthDense_fill_only_wall_us=_timed(lambda: ar.depthDense(**kw)), depthImage_wall_us=_timed(lambda: ar.depthImage(**cfg)))
        ar.close()
    return out


def main():
    res = stage()
    res.update(session())
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "depth_dense_timing.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
