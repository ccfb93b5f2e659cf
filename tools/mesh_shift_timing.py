"""Per-launch time of the volume shift (alva_mesh_shift) beside its yardsticks from the same run, and what a session pays for following.

  shift     k_mesh_shift's own time (the library's HIP-event timing, alva_prof_enable) at 64^3, 128^3 and 256^3, with and without the
            colour volume, for s = (8,0,0) (eight voxels per lane), (1,0,0) (one voxel per lane) and (0,0,8) (eight per lane, whole
            planes); beside each, in the same run: k_mesh_integrate on the same volume, and a plain device-to-device copy of the same
            bytes (torch's copy_ of q, w and c: hipMemcpyAsync, one per array), HIP events around every batch on an idle stream as
            the library's timing brackets every launch -- the shift loads at most those bytes and stores exactly those bytes; and
            the aligned shift once more with every weight zero, which leaves two of the three count sums out
  session   the tests' plane stream (device frames) with mesh_follow = 2 at rel_extent 1, an update on every frame once the volume is
            placed: the wall time of a meshUpdate call that shifted beside one that did not, same session, same stream

  python tools/mesh_shift_timing.py        prints one JSON line and writes it to profiles/mesh_shift_timing.json"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CALLS, WARMUP = 50, 5
VOLUMES = (64, 128, 256)
SHIFTS = ((8, 0, 0), (1, 0, 0), (0, 0, 8))


def _kernel_us(capi, call, match, calls=CALLS):
    for _ in range(WARMUP):
        call()
    hit = {n: us for n, (c, us) in capi.kernel_times(call, calls).items() if match in n}
    assert len(hit) == 1, hit
    return round(next(iter(hit.values())), 2)


def _copy_us(pairs, calls=CALLS):
    """the plain device-to-device copy of the same bytes: HIP events around every batch of copies on an idle stream, as the library's
    timing brackets every launch (so both figures include their launches), and the mean over `calls`"""
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


def shift(ctx, capi):
    import numpy as np
    import torch
    import mesh_cases as Mc
    res = {}
    for N in VOLUMES:
        n = N * N * N
        torch.manual_seed(N)   # (the bytes do not matter to a mover; the counts want some zeros among the weights)
        q = torch.randint(-32767, 32768, (N, N, N), dtype=torch.int16, device="cuda")
        w = torch.randint(0, 4, (N, N, N), dtype=torch.uint8, device="cuda")
        c = torch.randint(0, 256, (N, N, N, 4), dtype=torch.uint8, device="cuda")
        outs = (torch.empty_like(q), torch.empty_like(w), torch.empty_like(c))
        out = dict(bytes_plain=3 * n, bytes_colour=7 * n)
        for colour in (False, True):
            key = "colour" if colour else "plain"
            for s in SHIFTS:
                def call():
                    return ctx.mesh_shift(q, w, s, c if colour else None, out=outs[:3 if colour else 2])
                out["shift_%s_%d_%d_%d_us" % ((key,) + s)] = _kernel_us(capi, call, "k_mesh_shift")
            if not colour:   # the same bytes moved with every weight zero: two of the three counts stay zero, and a zero sum is not added
                w0 = torch.zeros_like(w)
                out["shift_plain_8_0_0_zero_weights_us"] = _kernel_us(capi, lambda: ctx.mesh_shift(q, w0, SHIFTS[0], out=outs[:2]), "k_mesh_shift")
            pairs = [(outs[0], q), (outs[1], w)] + ([(outs[2], c)] if colour else [])
            out["copy_%s_us" % key] = _copy_us(pairs)
        # k_mesh_integrate on the same volume size: a wall 0.3 in front of the cube's far side, seen from outside
        width, height, step = 256, 192, 4
        calib = Mc.calib_for(width, height)
        T = Mc.look_at((0.0, 0.0, -2.5), (0.0, 0.0, 0.0))
        meas = tuple(torch.from_numpy(a).cuda() for a in Mc.full_meas(np.full((height // step, width // step), 2.8, np.float32)))
        origin, voxel = np.array([-1.0, -1.0, -1.0]), 2.0 / N
        q2, w2 = torch.zeros_like(q), torch.zeros_like(w)
        out["integrate_us"] = _kernel_us(capi, lambda: ctx.mesh_integrate(q2, w2, origin, voxel, 3 * voxel, T, calib, width, height, step, meas),
                                         "k_mesh_integrate")
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
    out = dict(image=[W, H], resolution=32, rel_extent=1.0, block=2)
    for colour in (False, True):
        ar = AlvaAR(W, H, cell_size=12, random_sampling=False, depth=True, mesh_color=colour, mesh_follow=2)
        shifted, still = [], []
        for k in range(N):
            ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = ar.meshUpdate(resolution=32, rel_extent=1.0, step=8)
            dt = time.perf_counter() - t0
            if info["status"] == 0 and info["frames"] > 3:   # (the first shift allocates the second block)
                (shifted if info["shifted"] else still).append(dt)
        st = ar.meshFollowStats()
        out["colour_on" if colour else "colour_off"] = dict(
            shifts=st["shifts"], offset=st["offset"].tolist(), lost=st["lost"],
            meshUpdate_shifted_us=dict(median=round(1e6 * float(np.median(shifted)), 1), calls=len(shifted)) if shifted else None,
            meshUpdate_still_us=dict(median=round(1e6 * float(np.median(still)), 1), calls=len(still)) if still else None)
        ar.close()
    return out


def main():
    import alvaar_amd
    from alvaar_amd import capi
    ctx = alvaar_amd.Context(0)
    res = dict(calls=CALLS, warmup=WARMUP, shift=shift(ctx, capi))
    ctx.close()
    res["session"] = session()
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "mesh_shift_timing.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
