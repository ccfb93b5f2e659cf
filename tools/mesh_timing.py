"""Per-call time of the scene mesh (alva_mesh_integrate, alva_mesh_extract), at stage and at session level, with the sweep timed in the
same run for scale.

  Context.mesh_integrate / mesh_extract
                        the end-to-end scene of tests/mesh_cases.py (a wall and a box, 8 exact views on an arc, grid 64 x 48) at N = 64
                        and N = 128: one view integrated into the volume the other seven built, and that volume extracted; wall time
                        per call and the kernels' own times (the library's HIP-event timing, alva_prof_enable) on the context's stream
  Context.depth_sweep   k_depth_sweep on the dense two-depth scene of tests/depth_cases.py at 640 x 480, step 4 / 64 hypotheses / radius 2
  AlvaAR.meshUpdate / mesh
                        in a session on the plane stream of the tests, resolution 64 and 128, step 4: wall time per call.  An update
                        integrates once per frame, so it is timed over consecutive frames, one call each; mesh() on the last of them

  python tools/mesh_timing.py        prints one JSON line and writes it to profiles/mesh_timing.json"""
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
SIZES = (64, 128)


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


def stage():
    import numpy as np
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    import depth_cases as Dc
    import mesh_cases as Mc
    ctx = alvaar_amd.Context(0)
    res = dict(calls=CALLS, warmup=WARMUP, grid=[Mc.E2E_GW, Mc.E2E_GH])
    width, height = Mc.E2E_GW * Mc.E2E_STEP, Mc.E2E_GH * Mc.E2E_STEP
    calib = Mc.calib_for(width, height)
    poses = Mc.e2e_poses()
    images = [tuple(torch.from_numpy(a).cuda() for a in Mc.full_meas(Mc.render(Mc.e2e_scene(), T, calib, width, height, Mc.E2E_STEP))) for T in poses]
    for N in SIZES:
        origin, voxel = np.array([-1.0, -1.0, -1.0]), 2.0 / N
        q = torch.zeros((N, N, N), dtype=torch.int16, device="cuda")
        w = torch.zeros((N, N, N), dtype=torch.uint8, device="cuda")
        for T, meas in zip(poses[:-1], images[:-1]):
            ctx.mesh_integrate(q, w, origin, voxel, 3 * voxel, T, calib, width, height, Mc.E2E_STEP, meas)

        def integrate():
            return ctx.mesh_integrate(q, w, origin, voxel, 3 * voxel, poses[-1], calib, width, height, Mc.E2E_STEP, images[-1])

        def extract():
            return ctx.mesh_extract(q, w, origin, voxel, 2, 1 << 19, 1 << 20)
        out = dict(integrate_info=integrate().tolist(), extract_info=extract()[3].tolist())
        for name, call in (("integrate", integrate), ("extract", extract)):
            out[name + "_wall_us"] = _timed(call)
            out[name + "_kernels"] = _kernels(capi, call)
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
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    out = {}
    for N in SIZES:
        ar = AlvaAR(W, H, cell_size=12, random_sampling=False, relocalization=True, depth=True)
        first_ok, k, updates, info = None, 0, [], None
        for k in range(110):
            frame = torch.from_numpy(synth.plane_stream_frame(canvas, 3 * k, W, H, f)).cuda()
            st = ar.find_camera_pose_device(int(frame.data_ptr()), 33.0 * k)
            if st == 1 and first_ok is None:
                first_ok = k
            if first_ok is not None and k >= first_ok + 20:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                info = ar.meshUpdate(resolution=N, rel_extent=2.0, step=4)
                if info["status"] == 0 and info["frames"] > WARMUP:
                    updates.append(time.perf_counter() - t0)
            if len(updates) == CALLS:
                break
        m = ar.mesh(min_weight=2, max_vertices=1 << 19, max_triangles=1 << 20)
        out["session_n%d" % N] = dict(
            frame=k, first_tracked_frame=first_ok, update={key: info[key] for key in ("status", "updated", "hidden", "free", "outside", "no_depth", "swept", "frames")},
            mesh={key: m[3][key] for key in ("status", "vertices", "triangles", "valid", "inside")},
            meshUpdate_wall_us=dict(median=round(1e6 * float(np.median(updates)), 1), max=round(1e6 * max(updates), 1), calls=len(updates)),
            mesh_wall_us=_timed(lambda: ar.mesh(min_weight=2, max_vertices=1 << 19, max_triangles=1 << 20)))
        ar.close()
    return out


def main():
    res = stage()
    res.update(session())
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "mesh_timing.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
