"""Per-launch time of image detection's stages beside the hit test, and what a whole detectImages call costs a session.

  stages    at 640 x 480 and 1280 x 720, with 1 and with 8 pictures (256 x 192 crops of the frame's own canvas), in one run: the
            kernels' own times (the library's HIP-event timing, alva_prof_enable) of the frame's ORB launch set (1500 features, 8
            levels), of alva_image_match's three launches and of k_image_homography (256 iterations), and of k_hit_test (one ray, 64
            iterations, the hit test's base scene) as the yardstick of a RANSAC launch of the same kind
  session   the wall time of detectImages() in a tracking session on the tests' plane stream with the crop and the distractor added

  python tools/image_timing.py        prints one JSON line and writes it to profiles/image_timing.json"""
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


def stages():
    import numpy as np
    import torch
    import alvaar_amd
    import hit_cases
    from alvaar_amd import capi, synth
    ctx = alvaar_amd.Context(0)
    res = {}
    pts = torch.from_numpy(hit_cases.base_scene()).cuda()
    tap = [hit_cases.BASE_TAPS[0][0]]
    for w, h in SIZES:
        f = 0.866 * w
        canvas = synth.texture_canvas(w, h, 5)
        ch, cw = canvas.shape
        R_wc, t_wc = synth.plane_camera_pose(60)
        frame = torch.from_numpy(synth.render_plane(canvas, w, h, f, R_wc, t_wc)).cuda()
        orb = capi.Orb(ctx, w, h, 1500, 1.2, 8, 20)
        small = capi.Orb(ctx, 256, 192, 500, 1.2, 7, 20)
        kp = torch.zeros((capi.IMAGE_TRAIN_CAP, 6), dtype=torch.float32, device="cuda")
        desc = torch.zeros((capi.IMAGE_TRAIN_CAP, 32), dtype=torch.uint8, device="cuda")
        qdesc = torch.zeros((8, capi.IMAGE_QUERY_CAP, 32), dtype=torch.uint8, device="cuda")
        qxy = torch.zeros((8, capi.IMAGE_QUERY_CAP, 2), dtype=torch.float32, device="cuda")
        nq = []
        for j in range(8):   # crops spread over the part of the canvas the frame sees
            x0, y0 = cw // 2 - 100 + 40 * (j % 4) - 60, ch // 2 - 80 + 50 * (j // 4) - 25
            k, d = small.detect_and_compute(torch.from_numpy(np.ascontiguousarray(canvas[y0:y0 + 192, x0:x0 + 256])).cuda(), cap=capi.IMAGE_QUERY_CAP)
            nq.append(len(k))
            qdesc[j, :len(k)], qxy[j, :len(k)] = d, k[:, :2]
        out = {}
        for n_img in (1, 8):
            state = {}

            def detect():
                state["n"] = orb.detect_and_compute(frame, cap=capi.IMAGE_TRAIN_CAP)[0].shape[0]

            def match():
                k, d = orb.detect_and_compute(frame, cap=capi.IMAGE_TRAIN_CAP)
                n = len(k)
                kp[:n], desc[:n] = k, d
                n_train = torch.tensor([n], dtype=torch.int32, device="cuda")
                txy = kp[:, :2].contiguous()
                state["m"] = ctx.image_match(qdesc[:n_img].contiguous(), qxy[:n_img].contiguous(), nq[:n_img], desc, txy, n_train)

            match()
            _, xy, count = state["m"]

            def both():
                m = ctx.image_match(qdesc[:n_img].contiguous(), qxy[:n_img].contiguous(), nq[:n_img], desc, kp[:, :2].contiguous(),
                                    torch.tensor([state["n"]], dtype=torch.int32, device="cuda"))
                state["h"] = ctx.image_homography(m[1], m[2], [(256, 192)] * n_img, (w, h), (f, f, w / 2, h / 2))

            def hit():
                ctx.hit_test(pts, hit_cases.POSE_BASE, hit_cases.K_BASE, tap)

            detect()
            for _ in range(WARMUP):
                detect(); both(); hit()
            ctx.sync()
            kern = {}
            for fn in (detect, both, hit):
                kern.update({n: dict(launches_per_call=c / CALLS, avg_us=round(us, 2)) for n, (c, us) in capi.kernel_times(fn, CALLS).items()})
            orb_us = sum(v["avg_us"] * v["launches_per_call"] for n, v in kern.items() if not n.startswith(("k_image", "k_hit")))
            out[f"{n_img}_pictures"] = dict(frame_keypoints=state["n"], pairs=state["m"][2].cpu().tolist(), codes=state["h"][1][:, 0].tolist(),
                                            frame_orb_launch_set_us=round(orb_us, 2),
                                            kernels={n: v for n, v in kern.items() if n.startswith(("k_image", "k_hit"))})
        res["%dx%d" % (w, h)] = out
        orb.close()
        small.close()
    ctx.close()
    return dict(calls=CALLS, warmup=WARMUP, stages=res)


def session():
    import numpy as np
    import torch
    import image_cases as IC
    import sysdiff
    from alvaar_amd import synth
    from alvaar_amd.system import AlvaAR
    W, H, N = 640, 480, 60
    f = sysdiff.intrinsics(W, H)[0]
    canvas, crop, distractor, _ = IC.chain_pictures(W, H)
    frames = torch.from_numpy(np.stack([synth.plane_stream_frame(canvas, 2 * k, W, H, f) for k in range(N)])).cuda()
    ar = AlvaAR(W, H, cell_size=12, random_sampling=False)
    ar.addImage(crop, 0.5)
    ar.addImage(distractor)
    for k in range(N):
        st = ar.find_camera_pose_device(int(frames[k].data_ptr()), 33.0 * k)
    t = []
    for _ in range(60):
        t0 = time.perf_counter()
        info = ar.detectImages()[5]
        t.append(time.perf_counter() - t0)
    ar.close()
    return dict(session=dict(image=[W, H], pictures=2, status=int(st), info=info.tolist(),
                             detectImages_wall_us=dict(median=round(1e6 * float(np.median(t[10:])), 1), max=round(1e6 * max(t[10:]), 1))))


def main():
    res = stages()
    res.update(session())
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "image_timing.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
