"""Per-call time of the volume raycast (alva_mesh_raycast, alva_mesh_raycast_pixels), at stage and at session level, with the sweep and
the mesh extraction timed in the same run for scale.

  Context.mesh_raycast_pixels / mesh_raycast
                        the end-to-end scene of tests/mesh_cases.py (a wall and a box, 8 exact views on an arc integrated on the device)
                        at N = 64 and N = 128, seen from a ninth pose at 640 x 480: the grid of step 4 (160 x 120 rays), 16 taps, and 4096
                        world rays (those of 4096 hashed pixels); wall time per call -- which includes the outputs' download -- and the
                        kernel's own time (the library's HIP-event timing, alva_prof_enable) on the context's stream; the largest number of
                        samples a ray took (R8), which decides the kernel's time
  Context.mesh_extract  the same volumes extracted: the five launches' times
  Context.depth_sweep   k_depth_sweep on the dense two-depth scene of tests/depth_cases.py at 640 x 480, step 4 / 64 hypotheses / radius 2
  AlvaAR.meshDepth / meshRaycast / meshHitTest
                        in a session on the plane stream of the tests, resolution 64 and 128, after 30 integrated frames: wall time per
                        call of the depth image at step 4, of 4096 world rays and of 16 taps

  python tools/raycast_timing.py        prints one JSON line and writes it to profiles/raycast_timing.json"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CALLS, WARMUP = 50, 5
W, H, F, STEP = 640, 480, 580.0, 4
SIZES = (64, 128)
N_WORLD, N_TAPS = 4096, 16


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


def _kernels(capi, call):
    return {n: dict(launches_per_call=c / CALLS, avg_us=round(us, 2)) for n, (c, us) in capi.kernel_times(call, CALLS).items()}


def _hashed_pixels(n, seed):
    import numpy as np
    import mesh_cases as Mc
    return ((Mc.hashed(2 * n, seed).reshape(n, 2) % 4096) / 4095.0 * np.array([W - 1.0, H - 1.0])).astype(np.float32)


def stage():
    import numpy as np
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    import depth_cases as Dc
    import mesh_cases as Mc
    import raycast_cases as Rc
    ctx = alvaar_amd.Context(0)
    res = dict(calls=CALLS, warmup=WARMUP, image=[W, H], step=STEP, grid=[W // STEP, H // STEP], taps=N_TAPS, world_rays=N_WORLD)
    width, height = Mc.E2E_GW * Mc.E2E_STEP, Mc.E2E_GH * Mc.E2E_STEP
    calib_small, calib = Mc.calib_for(width, height), Mc.calib_for(W, H)
    poses = Mc.e2e_poses()
    images = [tuple(torch.from_numpy(a).cuda() for a in Mc.full_meas(Mc.render(Mc.e2e_scene(), T, calib_small, width, height, Mc.E2E_STEP))) for T in poses]
    T_wc = Rc.T_wc_of(Mc.look_at(Rc.E2E_NINTH, (0.0, 0.0, 0.3)))
    taps = torch.from_numpy(_hashed_pixels(N_TAPS, 3)).cuda()
    O, D = Rc.pixel_rays(T_wc, calib, _hashed_pixels(N_WORLD, 4))
    rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([O, D], 1))).cuda()
    for N in SIZES:
        origin, voxel = np.array([-1.0, -1.0, -1.0]), 2.0 / N
        q = torch.zeros((N, N, N), dtype=torch.int16, device="cuda")
        w = torch.zeros((N, N, N), dtype=torch.uint8, device="cuda")
        for T, meas in zip(poses, images):
            ctx.mesh_integrate(q, w, origin, voxel, 3 * voxel, T, calib_small, width, height, Mc.E2E_STEP, meas)

        def grid():
            return ctx.mesh_raycast_pixels(q, w, origin, voxel, 2, T_wc, calib, W, H, STEP)

        def tap():
            return ctx.mesh_raycast_pixels(q, w, origin, voxel, 2, T_wc, calib, W, H, STEP, taps)

        def world():
            return ctx.mesh_raycast(q, w, origin, voxel, 2, rays)

        def extract():
            return ctx.mesh_extract(q, w, origin, voxel, 2, 1 << 19, 1 << 20)
        out = dict(extract_info=extract()[3].tolist())
        for name, call in (("grid", grid), ("taps", tap), ("world", world)):
            out[name + "_info"] = call()["info"].tolist()
            out[name + "_wall_us"] = _timed(call)
            out[name + "_kernels"] = _kernels(capi, call)
        out["extract_wall_us"] = _timed(extract)
        out["extract_kernels"] = _kernels(capi, extract)
        res["n%d" % N] = out
    cur = torch.from_numpy(np.array(Dc.two_depth_frame(40, W, H, F)[0])).cuda()
    ref = torch.from_numpy(np.array(Dc.two_depth_frame(10, W, H, F)[0])).cuda()

    def sweep():
        return ctx.depth_sweep(cur, ref, Dc.calib_of(W, H, F), Dc.T_rc(40, 10), *Dc.RHO_RANGE, step=4, num_hyp=64, patch_radius=2, min_texture=4,
                               min_conf=96)
    res["sweep_step4_d64_r2"] = dict(image=[W, H], wall_us=_timed(sweep), kernels=_kernels(capi, sweep))
    return res


def session():
    import numpy as np
    import torch
    import mesh_cases as Mc
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    out = {}
    for N in SIZES:
        ar = AlvaAR(W, H, cell_size=12, random_sampling=False, relocalization=True, depth=True)
        k, info, st = 0, None, 0
        for k in range(110):
            frame = torch.from_numpy(synth.plane_stream_frame(canvas, 3 * k, W, H, f)).cuda()
            st = ar.find_camera_pose_device(int(frame.data_ptr()), 33.0 * k)
            info = ar.meshUpdate(resolution=N, rel_extent=2.0, step=4)
            if info["status"] == 0 and info["frames"] >= 30:
                break
        depth = ar.meshDepth(step=STEP)
        # world rays: from the camera's position towards hashed points of the volume
        origin, side = info["origin"], info["voxel"] * N
        target = origin + (Mc.hashed(3 * N_WORLD, 6).reshape(N_WORLD, 3) % 4096) / 4095.0 * side
        eye = ar.pose7()[0][:3]
        rays = np.concatenate([np.tile(eye, (N_WORLD, 1)), target - eye], 1)
        world = ar.meshRaycast(rays)
        taps = _hashed_pixels(N_TAPS, 3)
        hit = ar.meshHitTest(taps)
        out["session_n%d" % N] = dict(
            frame=k, tracker=st, frames_integrated=info["frames"],
            depth_info=[depth[3]["rays"], *depth[3]["counts"].tolist(), depth[3]["max_samples"], depth[3]["resolution"]],
            world_info=[world[4]["rays"], *world[4]["counts"].tolist(), world[4]["max_samples"], world[4]["resolution"]],
            taps_codes=hit[1][:, 0].tolist(), taps_poses=int(hit[1][:, 1].sum()),
            meshDepth_wall_us=_timed(lambda: ar.meshDepth(step=STEP)), meshRaycast_wall_us=_timed(lambda: ar.meshRaycast(rays)),
            meshHitTest_wall_us=_timed(lambda: ar.meshHitTest(taps)))
        ar.close()
    return out


def main():
    res = stage()
    res.update(session())
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "raycast_timing.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
