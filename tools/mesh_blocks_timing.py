"""Per-launch time of the mesh in blocks (alva_mesh_block_digest, alva_mesh_extract_blocks) beside its yardsticks from the same run, and
what a session pays per meshBlocks() call.

  digest    the digest pass's one launch (the library's HIP-event timing, alva_prof_enable) on the wall-and-box scene of
            tests/mesh_cases.py integrated at 64^3, 128^3 and 256^3, for the block edges 8, 16 and 32; beside it, in the same run, a
            plain device-to-device copy of q and w (torch's copy_: hipMemcpyAsync, one per array; HIP events around every batch on an
            idle stream, as the library's timing brackets every launch) -- the pass reads those bytes once, and the shift's yardstick
            is this copy -- and the ratio of the two
  extract   the block extraction's three launches for 1, 8 and all present blocks (edge 16) beside alva_mesh_extract's five on the
            same volume
  session   the tests' plane stream (device frames), resolution 64, an update on every fifth frame: the wall time of meshBlocks() with
            nothing changed, with the blocks one update touched, and with ALL, beside mesh() in the same process, and the bytes each
            hands back

  python tools/mesh_blocks_timing.py        prints one JSON line and writes it to profiles/mesh_blocks_timing.json"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CALLS, WARMUP = 30, 5
VOLUMES = (64, 128, 256)
EDGES = (8, 16, 32)


def _kernels(capi, call, calls=CALLS):
    for _ in range(WARMUP):
        call()
    return {n: round(us, 2) for n, (c, us) in capi.kernel_times(call, calls).items()}


def _copy_us(pairs, calls=CALLS):
    import torch
    for _ in range(WARMUP):
        for dst, src in pairs:
            dst.copy_(src)
    total = 0.0
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for dst, src in pairs:
            dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
    return round(1e3 * total / calls, 2)


def stages(ctx, capi):
    import numpy as np
    import torch
    import mesh_cases as Mc
    width, height = Mc.E2E_GW * Mc.E2E_STEP, Mc.E2E_GH * Mc.E2E_STEP
    calib = Mc.calib_for(width, height)
    poses = Mc.e2e_poses()
    images = [tuple(torch.from_numpy(a).cuda() for a in Mc.full_meas(Mc.render(Mc.e2e_scene(), T, calib, width, height, Mc.E2E_STEP))) for T in poses]
    res = {}
    for N in VOLUMES:
        origin, voxel = np.array([-1.0, -1.0, -1.0]), 2.0 / N
        q = torch.zeros((N, N, N), dtype=torch.int16, device="cuda")
        w = torch.zeros((N, N, N), dtype=torch.uint8, device="cuda")
        for T, meas in zip(poses, images):
            ctx.mesh_integrate(q, w, origin, voxel, 3 * voxel, T, calib, width, height, Mc.E2E_STEP, meas)
        q2, w2 = torch.empty_like(q), torch.empty_like(w)
        out = dict(bytes_q_w=3 * N * N * N, copy_q_w_us=_copy_us([(q2, q), (w2, w)]))
        for B in EDGES:
            k = _kernels(capi, lambda: ctx.mesh_block_digest(q, w, (0, 0, 0), 2, B))
            us = [v for n, v in k.items() if "k_mesh_block_count" in n]
            assert len(us) == 1, k
            counts = ctx.mesh_block_digest(q, w, (0, 0, 0), 2, B)[1]
            out["digest_B%d" % B] = dict(us=us[0], ratio_to_copy=round(us[0] / out["copy_q_w_us"], 2), blocks=len(counts),
                                         present=int((counts[:, 1] > 0).sum()))
        B = 16
        digest, counts, nb3 = ctx.mesh_block_digest(q, w, (0, 0, 0), 2, B)
        keys = np.stack(np.meshgrid(np.arange(nb3[2]), np.arange(nb3[1]), np.arange(nb3[0]), indexing="ij")[::-1], -1).reshape(-1, 3)
        present = keys[counts[:, 1] > 0]
        mid = len(present) // 2
        for name, sel in (("1", present[mid:mid + 1]), ("8", present[max(0, mid - 4):mid + 4]), ("all_present", present)):
            r = ctx.mesh_extract_blocks(q, w, origin, voxel, (0, 0, 0), 2, B, sel, 1 << 21, 1 << 22)
            k = _kernels(capi, lambda: ctx.mesh_extract_blocks(q, w, origin, voxel, (0, 0, 0), 2, B, sel, 1 << 21, 1 << 22))
            k = {n: v for n, v in k.items() if "k_mesh_block" in n}
            out["extract_B16_%s" % name] = dict(blocks=len(sel), vertices=int(r["info"][1]), triangles=int(r["info"][2]), kernels_us=k,
                                                sum_us=round(sum(k.values()), 2))
        k = _kernels(capi, lambda: ctx.mesh_extract(q, w, origin, voxel, 2, 1 << 21, 1 << 22))
        k = {n: v for n, v in k.items() if n.startswith("k_mesh_")}
        info = ctx.mesh_extract(q, w, origin, voxel, 2, 1 << 21, 1 << 22)[3]
        out["extract_whole"] = dict(vertices=int(info[1]), triangles=int(info[2]), kernels_us=k, sum_us=round(sum(k.values()), 2))
        res["n%d" % N] = out
    return res


def _wall(call, calls=CALLS):
    import numpy as np
    import torch
    t = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return round(1e6 * float(np.median(t)), 1)


def _bytes(m):
    return int(sum(m[k].nbytes for k in ("keys", "state", "ranges", "digest", "vertices", "normals", "triangles")))


def session():
    import numpy as np
    import torch
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    W, H, N, RES, B = 640, 480, 110, 64, 16
    f = sysdiff.intrinsics(W, H)[0]
    canvas = synth.texture_canvas(W, H, 5)
    frames = torch.from_numpy(np.stack([synth.plane_stream_frame(canvas, 3 * k, W, H, f) for k in range(N)])).cuda()
    ar = AlvaAR(W, H, cell_size=12, random_sampling=False, depth=True)
    caps = dict(max_vertices=1 << 19, max_triangles=1 << 20)
    touched, touched_blocks, touched_bytes = [], [], []
    for k in range(N):
        ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
        if k % 5:
            continue
        info = ar.meshUpdate(resolution=RES, rel_extent=2.0, step=4)
        if info["status"] != 0:
            continue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = ar.meshBlocks(block=B, **caps)
        dt = time.perf_counter() - t0
        if info["frames"] > 2:   # (the first calls allocate, and report everything)
            touched.append(dt)
            touched_blocks.append(m["info"]["blocks"])
            touched_bytes.append(_bytes(m))
    whole = ar.mesh(**caps)
    every = ar.meshBlocks(block=B, all=True, **caps)
    quiet = ar.meshBlocks(block=B, **caps)
    out = dict(image=[W, H], resolution=RES, block=B, present=every["info"]["present"],
               mesh_us=_wall(lambda: ar.mesh(**caps)), mesh_bytes=int(whole[0].nbytes + whole[1].nbytes + whole[2].nbytes),
               mesh_vertices=len(whole[0]), mesh_triangles=len(whole[2]),
               blocks_nothing_changed_us=_wall(lambda: ar.meshBlocks(block=B, **caps)), blocks_nothing_changed_bytes=_bytes(quiet),
               blocks_all_us=_wall(lambda: ar.meshBlocks(block=B, all=True, **caps)), blocks_all_bytes=_bytes(every),
               blocks_all_vertices=len(every["vertices"]), blocks_all_triangles=len(every["triangles"]),
               blocks_one_update_us=round(1e6 * float(np.median(touched)), 1) if touched else None, blocks_one_update_calls=len(touched),
               blocks_one_update_blocks=float(np.median(touched_blocks)) if touched else None,
               blocks_one_update_bytes=float(np.median(touched_bytes)) if touched else None)
    ar.close()
    return out


def main():
    import alvaar_amd
    from alvaar_amd import capi
    ctx = alvaar_amd.Context(0)
    res = dict(calls=CALLS, warmup=WARMUP, stages=stages(ctx, capi))
    ctx.close()
    res["session"] = session()
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "mesh_blocks_timing.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
