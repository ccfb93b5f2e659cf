"""Per-launch time of mesh colour (alva_color_thumb, alva_mesh_integrate_color, alva_mesh_color_at), each beside its neighbour from the same
run, and what a session pays for it.

  thumbnail   at 640 x 480 and 1280 x 720: the kernels' own times (the library's HIP-event timing, alva_prof_enable) of k_color_thumb
              (step 4) beside k_light_bin and k_pyr_all on the same frame, in the order a session enqueues them
  integrate   the painted scene of tests/mesh_color_cases.py (8 exact views, depth grid 64 x 48, colour 256 x 192) at N = 64 and 128:
              one view integrated into the volume the other seven built, with colour (k_mesh_integrate's colour instantiation) and
              without, on copies of the same volume
  colour at   k_mesh_color_at on that scene's mesh vertices and on 4096 hashed points; wall time per call (it waits)
  session     sustained frames/s of a session on the tests' plane stream (device frames, no look-ahead hint) with mesh colour on and
              off (depth on in both), in the same process, alternating, the better of three passes each; and per call, over consecutive
              frames, meshUpdate with colour beside meshUpdate without, mesh(colors=True) beside mesh()

  python tools/mesh_color_timing.py        prints one JSON line and writes it to profiles/mesh_color_timing.json"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CALLS, WARMUP = 100, 10
SIZES = [(640, 480), (1280, 720)]
VOLUMES = (64, 128)
CSTEP = 4


def _kernels(capi, call, calls=CALLS):
    return {n: dict(launches_per_call=c / calls, avg_us=round(us, 2)) for n, (c, us) in capi.kernel_times(call, calls).items()}


def _timed(call, calls=CALLS):
    import numpy as np
    import torch
    t = []
    for _ in range(WARMUP + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return dict(median=round(1e6 * float(np.median(t[WARMUP:])), 1), max=round(1e6 * max(t[WARMUP:]), 1))


def thumbnail(ctx, capi):
    import numpy as np
    import torch
    res = {}
    R = np.array([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]]).reshape(-1)
    for w, h in SIZES:
        rgba = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (h, w, 4), dtype=np.uint8)).cuda()
        calib = (0.9 * w, 0.9 * w, w / 2, h / 2, 0.0, 0.0, 0.0, 0.0)
        pyr = capi.Pyramid(ctx, w, h)
        gray = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        acc = torch.zeros(capi.LIGHT_ACC_WORDS, dtype=torch.int64, device="cuda")

        def frame():   # what a session with colour and light enqueues per frame, in its order
            pyr.build_from_rgba(rgba, gray)
            ctx.color_thumb(rgba, CSTEP)
            ctx.light_bin(rgba, calib, R, 4, acc=acc)

        for _ in range(WARMUP):
            frame()
        ctx.sync()
        res["%dx%d" % (w, h)] = dict(kernels=_kernels(capi, frame))
        pyr.close()
    return res


def integrate_and_sample(ctx, capi):
    import numpy as np
    import torch
    import mesh_cases as Mc
    import mesh_color_cases as Cc
    width, height = Mc.E2E_GW * Mc.E2E_STEP, Mc.E2E_GH * Mc.E2E_STEP
    calib = Mc.calib_for(width, height)
    poses = Mc.e2e_poses()
    images = [tuple(torch.from_numpy(a).cuda() for a in Mc.full_meas(Mc.render(Cc.paint_scene(), T, calib, width, height, Mc.E2E_STEP))) for T in poses]
    thumbs = [ctx.color_thumb(torch.from_numpy(Cc.render_color(T, calib, width, height)[0]).cuda(), CSTEP) for T in poses]
    res = dict(depth_grid=[Mc.E2E_GW, Mc.E2E_GH], colour_image=[width, height])
    for N in VOLUMES:
        origin, voxel = np.array([-1.0, -1.0, -1.0]), 2.0 / N
        q = torch.zeros((N, N, N), dtype=torch.int16, device="cuda")
        w = torch.zeros((N, N, N), dtype=torch.uint8, device="cuda")
        c = torch.zeros((N, N, N, 4), dtype=torch.uint8, device="cuda")
        for T, meas, th in zip(poses[:-1], images[:-1], thumbs[:-1]):
            ctx.mesh_integrate_color(q, w, c, origin, voxel, 3 * voxel, T, calib, width, height, Mc.E2E_STEP, meas, th, CSTEP)
        q2, w2 = q.clone(), w.clone()

        def colour():
            return ctx.mesh_integrate_color(q, w, c, origin, voxel, 3 * voxel, poses[-1], calib, width, height, Mc.E2E_STEP, images[-1], thumbs[-1], CSTEP)

        def plain():
            return ctx.mesh_integrate(q2, w2, origin, voxel, 3 * voxel, poses[-1], calib, width, height, Mc.E2E_STEP, images[-1])
        out = dict(colour_info=colour().tolist(), plain_info=plain().tolist())
        out["kernels_colour"] = _kernels(capi, colour)
        out["kernels_plain"] = _kernels(capi, plain)
        out["colour_wall_us"], out["plain_wall_us"] = _timed(colour), _timed(plain)
        v = ctx.mesh_extract(q, w, origin, voxel, 2, 1 << 19, 1 << 20)[0]
        pts = {"vertices": torch.from_numpy(v).cuda(),
               "4096": torch.from_numpy((origin + (Mc.hashed(3 * 4096, 3).reshape(-1, 3) % 100003) / 100003.0 * 2.0).astype(np.float32)).cuda()}
        for name, p in pts.items():
            def at():
                return ctx.mesh_color_at(c, origin, voxel, p)
            out["color_at_" + name] = dict(points=int(p.shape[0]), info=at()[2].tolist(), kernels=_kernels(capi, at), wall_us=_timed(at))
        res["n%d" % N] = out
    return res


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
    tracked = {}
    for _ in range(3):
        for colour in (False, True):
            ar = AlvaAR(W, H, cell_size=12, random_sampling=False, depth=True, mesh_color=colour)
            for k in range(10):                      # the first frames initialise: not part of the sustained rate
                ar.find_camera_pose_device(ptrs[k], 33.0 * k)
            torch.cuda.synchronize()
            n_ok = 0
            t0 = time.perf_counter()
            for k in range(10, N):
                n_ok += ar.find_camera_pose_device(ptrs[k], 33.0 * k) == 1
            dt = time.perf_counter() - t0
            best[colour] = max(best[colour], (N - 10) / dt)
            tracked[colour] = n_ok
            ar.close()
    out = dict(image=[W, H], frames=N - 10, tracked=dict(colour_on=tracked[True], colour_off=tracked[False]),
               frames_per_s=dict(colour_on=round(best[True], 1), colour_off=round(best[False], 1)),
               per_frame_cost_us=round(1e6 / best[True] - 1e6 / best[False], 1))
    # per call: an update integrates once per frame, so it is timed over consecutive frames, one call each
    for colour in (False, True):
        ar = AlvaAR(W, H, cell_size=12, random_sampling=False, depth=True, mesh_color=colour)
        first_ok, updates, info = None, [], None
        for k in range(N):
            st = ar.find_camera_pose_device(ptrs[k], 33.0 * k)
            if st == 1 and first_ok is None:
                first_ok = k
            if first_ok is not None and k >= first_ok + 20:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                info = ar.meshUpdate(resolution=64, rel_extent=2.0, step=4)
                if info["status"] == 0 and info["frames"] > 5:
                    updates.append(time.perf_counter() - t0)
        caps = dict(min_weight=2, max_vertices=1 << 19, max_triangles=1 << 20)
        m = ar.mesh(colors=colour, **caps)
        out["colour_on" if colour else "colour_off"] = dict(
            update={key: info[key] for key in ("status", "updated", "colored", "color_fused", "swept", "frames")},
            mesh={key: m[-1][key] for key in m[-1] if key in ("status", "vertices", "triangles", "colored")},
            meshUpdate_wall_us=dict(median=round(1e6 * float(np.median(updates)), 1), max=round(1e6 * max(updates), 1), calls=len(updates)),
            mesh_wall_us=_timed(lambda: ar.mesh(colors=colour, **caps), 50))
        ar.close()
    return out


def main():
    import alvaar_amd
    from alvaar_amd import capi
    ctx = alvaar_amd.Context(0)
    res = dict(calls=CALLS, warmup=WARMUP, cstep=CSTEP, thumbnail=thumbnail(ctx, capi))
    res["integrate"] = integrate_and_sample(ctx, capi)
    ctx.close()
    res["session"] = session()
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "mesh_color_timing.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
