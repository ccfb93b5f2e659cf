"""Image detection's device stages (include/alvaar_hip.h, alva_image_match and alva_image_homography) restated in numpy, step for step.
The reference has no image detection, so this file is what the two stages are pinned to (tests/test_image_cases.py checks the restatement
itself, tests/test_gpu_image_match.py and tests/test_gpu_image_homography.py the kernels against it, bit for bit).

All decisions of the homography stage are taken in float64 with the operation order written here, which is the kernel's: elementwise
numpy does not contract a * b + c into an FMA, nothing below goes through a BLAS product, and division and square root are correctly
rounded on both sides.  The hypotheses are evaluated side by side (arrays over `it`), which changes no single operation."""
from __future__ import annotations

import numpy as np

IMAGE_MAX, QUERY_CAP, TRAIN_CAP = 8, 512, 2048
NO_DIST = 257
PIVOT_MIN = 1e-12


def hash32(x: int) -> int:
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def sample_words(seed: int, num_iterations: int) -> np.ndarray:
    return np.array([[hash32(seed ^ (((4 * it + j) * 0x9E3779B9) & 0xFFFFFFFF)) for j in range(4)] for it in range(num_iterations)], np.uint32)


def words_for(indices, m: int) -> np.ndarray:
    """explicit words (h_rand4) that select the given indices among m pairs: the smallest w with (w * m) >> 32 == index"""
    return np.array([[-((-int(i) << 32) // m) for i in row] for row in indices], np.uint32).reshape(-1, 4)


# ---- stage 1

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(q: np.ndarray, t: np.ndarray) -> np.ndarray:
    """[nq, 32] x [nt, 32] uint8 -> [nq, nt] int32"""
    return _POP[q[:, None, :] ^ t[None, :, :]].sum(axis=2, dtype=np.int32)


def match_oracle(qdesc, qxy, tdesc, txy, n_train, max_dist=64, ratio=0.8):
    """One image.  qdesc [nq, 32] uint8, qxy [nq, 2] float32, tdesc [cap, 32], txy [cap, 2] float32, n_train the frame's count as the device
    holds it (clamped to [0, cap] here as there).  Returns (match [k, 3] int32 = query, train, distance in ascending query index, xy
    [k, 4] float64 = x, y, u, v)."""
    nq, cap = len(qdesc), len(tdesc)
    nt = min(max(int(n_train), 0), cap)
    cand = []   # (query, best row, distance) of the accepted queries
    if nq and nt:
        D = hamming(np.asarray(qdesc, np.uint8), np.asarray(tdesc, np.uint8)[:nt])
        for q in range(nq):
            row = int(np.argmin(D[q]))   # (the first minimum: the lowest train index on ties)
            best = int(D[q, row])
            others = np.delete(D[q], row)
            second = int(others.min()) if len(others) else NO_DIST
            if best <= max_dist and np.float32(best) < np.float32(ratio) * np.float32(second):
                cand.append((q, row, best))
    owner = {}
    for q, row, best in cand:   # one-to-one: the smallest (distance, query index) keeps the row
        if row not in owner or (best, q) < owner[row]:
            owner[row] = (best, q)
    kept = [(q, row, best) for q, row, best in cand if owner[row] == (best, q)]
    match = np.array(kept, np.int32).reshape(-1, 3)
    xy = np.zeros((len(kept), 4))
    for i, (q, row, _) in enumerate(kept):
        xy[i] = [np.float64(qxy[q][0]), np.float64(qxy[q][1]), np.float64(txy[row][0]), np.float64(txy[row][1])]
    return match, xy


# ---- stage 2

def normalise(xy, wh, frame_wh):
    """pairs (x, y, u, v) -> p [m, 2] in the picture's unit-width frame, q [m, 2] in normalised frame coordinates, s"""
    xy = np.asarray(xy, np.float64).reshape(-1, 4)
    w, h = np.float64(wh[0]), np.float64(wh[1])
    W, H = np.float64(frame_wh[0]), np.float64(frame_wh[1])
    s = max(W, H) / 2
    p = np.stack([(xy[:, 0] - w / 2) / w, (xy[:, 1] - h / 2) / w], axis=1)
    q = np.stack([(xy[:, 2] - W / 2) / s, (xy[:, 3] - H / 2) / s], axis=1)
    return p, q, s


def solve_models(p, q, idx):
    """idx [n, 4]: the 8 x 9 systems of n hypotheses solved side by side -> (h [n, 8], ok [n])"""
    n = len(idx)
    a = np.zeros((n, 8, 9))
    for i in range(4):
        x, y, u, v = p[idx[:, i], 0], p[idx[:, i], 1], q[idx[:, i], 0], q[idx[:, i], 1]
        a[:, 2 * i, 0], a[:, 2 * i, 1], a[:, 2 * i, 2] = x, y, 1.0
        a[:, 2 * i, 6], a[:, 2 * i, 7], a[:, 2 * i, 8] = -(x * u), -(y * u), u
        a[:, 2 * i + 1, 3], a[:, 2 * i + 1, 4], a[:, 2 * i + 1, 5] = x, y, 1.0
        a[:, 2 * i + 1, 6], a[:, 2 * i + 1, 7], a[:, 2 * i + 1, 8] = -(x * v), -(y * v), v
    ok = np.ones(n, bool)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        for k in range(8):
            piv = np.full(n, k)
            best = np.abs(a[:, k, k])
            for r in range(k + 1, 8):
                v = np.abs(a[:, r, k])
                better = v > best
                best = np.where(better, v, best)
                piv = np.where(better, r, piv)
            ok &= best > PIVOT_MIN
            top, low = a[rows, k, :].copy(), a[rows, piv, :].copy()
            a[rows, piv, :] = top
            a[rows, k, :] = low
            for r in range(k + 1, 8):
                f = a[:, r, k] / a[:, k, k]
                for c in range(k + 1, 9):
                    a[:, r, c] = a[:, r, c] - f * a[:, k, c]
        h = np.zeros((n, 8))
        for k in range(7, -1, -1):
            acc = a[:, k, 8].copy()
            for c in range(k + 1, 8):
                acc = acc - a[:, k, c] * h[:, c]
            h[:, k] = acc / a[:, k, k]
    return h, ok


def weights(h, x, y):
    return (h[..., 6, None] * x + h[..., 7, None] * y) + 1.0


def inliers(h, p, q, s, thr2):
    """h [n, 8] -> bool [n, m]: w > 0 and the squared forward transfer error in pixels <= thr2"""
    x, y, u, v = p[:, 0], p[:, 1], q[:, 0], q[:, 1]
    with np.errstate(all="ignore"):
        w = weights(h, x, y)
        X = (h[:, 0, None] * x + h[:, 1, None] * y) + h[:, 2, None]
        Y = (h[:, 3, None] * x + h[:, 4, None] * y) + h[:, 5, None]
        dx = (X / w - u) * s
        dy = (Y / w - v) * s
        return (w > 0) & (dx * dx + dy * dy <= thr2)


def pose_from_h(h, s, frame_wh, calib4):
    """the pose step: (code 0 or 4, R [3, 3], t [3])"""
    fx, fy, cx, cy = (np.float64(c) for c in calib4)
    W, H = np.float64(frame_wh[0]), np.float64(frame_wh[1])
    sx, sy, ox, oy = s / fx, s / fy, (W / 2 - cx) / fx, (H / 2 - cy) / fy
    Hm = np.array([[h[0], h[1], h[2]], [h[3], h[4], h[5]], [h[6], h[7], 1.0]])
    a = [np.array([sx * Hm[0, c] + ox * Hm[2, c], sy * Hm[1, c] + oy * Hm[2, c], Hm[2, c]]) for c in range(3)]

    def dot(u, v):
        return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]

    with np.errstate(all="ignore"):
        n1, n2 = np.sqrt(dot(a[0], a[0])), np.sqrt(dot(a[1], a[1]))
        d12 = dot(a[0], a[1])
        rat = n1 / n2
        if not (rat >= 0.5 and rat <= 2.0) or not (np.abs(d12) / (n1 * n2) <= 0.5):
            return 4, np.zeros((3, 3)), np.zeros(3)
    lam = 1.0 / np.sqrt(n1 * n2)
    r1 = a[0] / n1
    d = dot(r1, a[1])
    v = a[1] - d * r1
    r2 = v / np.sqrt(dot(v, v))
    r3 = np.array([r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]])
    return 0, np.stack([r1, r2, r3], axis=1), lam * a[2]


def homography_oracle(xy, wh, frame_wh, calib4, num_iterations=256, threshold_px=3.0, min_inliers=20, seed=12345, rand4=None):
    """One image.  Returns a dict: info [8] int32, H [9], mask [QUERY_CAP] uint8, R [9], t [3] (what alva_image_homography returns for
    it), and counts [num_iterations] (-1 where the hypothesis was skipped; for the tests of the restatement)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 4)[:QUERY_CAP]
    m = len(xy)
    out = dict(info=np.zeros(8, np.int32), H=np.zeros(9), mask=np.zeros(QUERY_CAP, np.uint8), R=np.zeros(9), t=np.zeros(3),
               counts=np.full(num_iterations, -1))
    out["info"][1], out["info"][2] = m, -1
    if m < 4 or m < min_inliers:
        out["info"][0] = 1
        return out
    p, q, s = normalise(xy, wh, frame_wh)
    thr2 = np.float64(np.float32(threshold_px)) * np.float64(np.float32(threshold_px))
    words = sample_words(seed, num_iterations) if rand4 is None else np.asarray(rand4, np.uint32).reshape(-1, 4)[:num_iterations]
    idx = ((words.astype(np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
    distinct = np.array([len(set(row)) == 4 for row in idx.tolist()], bool)
    h, ok = solve_models(p, q, idx)
    with np.errstate(all="ignore"):
        front = np.all(weights(h, p[idx, 0], p[idx, 1]) > 0, axis=1)
    alive = distinct & ok & front
    counts = np.where(alive, inliers(h, p, q, s, thr2).sum(axis=1), -1)
    out["counts"] = counts
    if not alive.any():
        out["info"][0] = 2
        return out
    win = int(np.argmax(counts))   # (the first maximum: the lowest iteration on ties)
    out["info"][2], out["info"][3] = win, counts[win]
    out["H"][:8], out["H"][8] = h[win], 1.0
    out["mask"][:m] = inliers(h[win:win + 1], p, q, s, thr2)[0]
    if counts[win] < min_inliers:
        out["info"][0] = 3
        return out
    code, R, t = pose_from_h(h[win], s, frame_wh, calib4)
    out["info"][0] = code
    out["R"], out["t"] = R.reshape(-1), t
    return out


# ---- scenes

def homography_of_pose(R, t, frame_wh, calib4):
    """the H (h33 = 1) that maps the picture's unit-width frame to normalised frame coordinates for X_cam = R (x, y, 0) + t"""
    fx, fy, cx, cy = calib4
    W, H = frame_wh
    s = max(W, H) / 2
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    N = np.array([[1 / s, 0, -W / 2 / s], [0, 1 / s, -H / 2 / s], [0, 0, 1.0]])
    G = N @ K @ np.stack([R[:, 0], R[:, 1], t], axis=1)
    return G / G[2, 2]


def project_pairs(Hm, wh, frame_wh, xy_image):
    """picture pixels [m, 2] -> pairs [m, 4] under the homography Hm (normalised coordinates on both sides)"""
    w, h = wh
    W, H = frame_wh
    s = max(W, H) / 2
    px, py = (xy_image[:, 0] - w / 2) / w, (xy_image[:, 1] - h / 2) / w
    den = Hm[2, 0] * px + Hm[2, 1] * py + Hm[2, 2]
    u = (Hm[0, 0] * px + Hm[0, 1] * py + Hm[0, 2]) / den * s + W / 2
    v = (Hm[1, 0] * px + Hm[1, 1] * py + Hm[1, 2]) / den * s + H / 2
    return np.stack([xy_image[:, 0], xy_image[:, 1], u, v], axis=1)


def rot_xyz(ax, ay, az):
    cx_, sx_, cy_, sy_, cz_, sz_ = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx_], [0, sx_, cx_]])
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
    Rz = np.array([[cz_, -sz_, 0], [sz_, cz_, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


CALIB = (554.256, 554.256, 320.0, 240.0)
FRAME = (640, 480)
WH = (256, 192)


def planted_scene(m, outlier_fraction, seed, wh=WH, frame_wh=FRAME, calib4=CALIB, noise_px=0.0):
    """m pairs of a picture seen under a known pose, a fraction of them replaced by uniform clutter -> (xy [m, 4], R, t, is_inlier)"""
    rng = np.random.default_rng(seed)
    R = rot_xyz(*rng.uniform(-0.35, 0.35, 3))
    t = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.15, 0.15), rng.uniform(1.2, 2.0)])
    pts = np.stack([rng.uniform(0, wh[0], m), rng.uniform(0, wh[1], m)], axis=1)
    xy = project_pairs(homography_of_pose(R, t, frame_wh, calib4), wh, frame_wh, pts)
    xy[:, 2:] += rng.normal(0, noise_px, (m, 2)) if noise_px else 0.0
    bad = np.zeros(m, bool)
    bad[rng.permutation(m)[:int(round(outlier_fraction * m))]] = True
    xy[bad, 2] = rng.uniform(0, frame_wh[0], bad.sum())
    xy[bad, 3] = rng.uniform(0, frame_wh[1], bad.sum())
    return xy, R, t, ~bad


# ---- the launches the tests run: every entry is one alva_image_homography call (up to 8 images share its parameters)

def integer_translation_pairs():
    """A 256 x 256 picture in a 512 x 512 frame (w = s = 256: every normalised coordinate is a dyadic rational), moved by (40, 24) pixels:
    H = [1 0 a; 0 1 b; 0 0 1] is recovered exactly from the four corner pairs, so the squared error of a pair displaced by a whole number
    of pixels is that integer exactly and `<=` decides at the threshold.  Pairs 0..3 the sample; 4..7 off by (3, 0), (0, -3): 9 = 3^2,
    in; (3, 1): 10, out; (2, 2): 8, in; the rest exact."""
    corners = np.array([[0, 0], [256, 0], [256, 256], [0, 256]], np.float64)
    more = np.array([[64, 64], [192, 64], [128, 128], [64, 192], [32, 96], [200, 40], [17, 233], [99, 101]], np.float64)
    pts = np.concatenate([corners, more])
    xy = np.concatenate([pts, pts + [40.0, 24.0]], axis=1)
    xy[4, 2:] += [3, 0]
    xy[5, 2:] += [0, -3]
    xy[6, 2:] += [3, 1]
    xy[7, 2:] += [2, 2]
    expect = np.ones(len(xy), np.uint8)
    expect[6] = 0
    return xy, expect


def bowtie_pairs(m=24, seed=5):
    """pairs 0..3: a rectangle whose targets form a concave quadrilateral -- the homography through them exists (no pivot fails) but its
    w is negative at one corner, so the sign rule must skip it; the other pairs are a clean planted scene"""
    xy, _, _, _ = planted_scene(m, 0.0, seed)
    xy[0] = [64, 32, 250, 170]
    xy[1] = [192, 32, 390, 180]
    xy[2] = [192, 160, 300, 215]
    xy[3] = [64, 160, 260, 310]
    return xy


def launches():
    L = []

    def add(name, images, iterations=256, thr=3.0, min_inliers=20, seed=12345, rand4=None, frame=FRAME, calib=CALIB, expect=None):
        L.append(dict(name=name, images=images, iterations=iterations, thr=thr, min_inliers=min_inliers, seed=seed, rand4=rand4, frame=frame,
                      calib=calib, expect=expect))

    # sizes: m = 0, 3 (code 1), 4, 5, 64, 65, 512, 30 % clutter and half a pixel of noise; min_inliers 4 so that the small ones run
    sizes = [0, 3, 4, 5, 64, 65, 512, 200]
    add("sizes", [(planted_scene(m, 0.3 if m >= 64 else 0.0, 100 + m, noise_px=0.5 if m >= 64 else 0.0)[0], WH) for m in sizes], iterations=256,
        min_inliers=4, expect=[1, 1, None, None, 0, 0, 0, 0])
    # iteration counts around the lane stripe (256 threads own iterations it, it + 256, ...) and the wave (64)
    for iters in (1, 63, 64, 65, 255, 256, 257, 4096):
        add(f"iterations-{iters}", [(planted_scene(64, 0.3, 7, noise_px=0.5)[0], WH), (planted_scene(65, 0.5, 8, noise_px=0.5)[0], (300, 180))],
            iterations=iters, seed=777 + iters)
    # 70 % clutter: the planted model must win
    add("outliers-70", [(planted_scene(300, 0.7, 21, noise_px=0.3)[0], WH)], iterations=1024, seed=4242, expect=[0])
    # the threshold edge, explicit words: iteration 0 draws the corners
    xy, _ = integer_translation_pairs()
    add("threshold-edge", [(xy, (256, 256))], min_inliers=4, rand4=words_for([[0, 1, 2, 3]], len(xy)), frame=(512, 512),
        calib=(400.0, 400.0, 256.0, 256.0), expect=[0])
    # skip rules through explicit words: a repeated index (each position), three collinear points (a pivot fails), the sign rule; the
    # last two iterations draw the same clean model through different pairs: equal counts, the lower iteration wins
    xy = bowtie_pairs()
    xy[4], xy[5], xy[6] = [10, 10, 100, 100], [20, 20, 110, 110], [30, 30, 120, 120]   # collinear in the picture (and in the frame)
    idx = [[8, 8, 9, 10], [8, 9, 8, 10], [8, 9, 10, 8], [9, 8, 8, 10], [9, 8, 10, 8], [9, 10, 8, 8], [4, 5, 6, 12], [0, 1, 2, 3],
           [8, 13, 17, 21], [9, 14, 18, 22]]
    add("skips-and-tie", [(xy, WH)], min_inliers=10, rand4=words_for(idx, len(xy)), expect=[0])
    add("all-skipped", [(xy, WH)], min_inliers=10, rand4=words_for(idx[:8], len(xy)), expect=[2])
    # the codes: 1 (fewer pairs than min_inliers), 3 (clutter only), 4 (an anisotropic affine map: |a1| / |a2| = 3), 0
    rng = np.random.default_rng(9)
    clutter = np.stack([rng.uniform(0, 256, 40), rng.uniform(0, 192, 40), rng.uniform(0, 640, 40), rng.uniform(0, 480, 40)], axis=1)
    pts = np.stack([rng.uniform(0, 256, 40), rng.uniform(0, 192, 40)], axis=1)
    squeezed = np.concatenate([pts, np.stack([320 + 0.9 * (pts[:, 0] - 128), 240 + 0.3 * (pts[:, 1] - 96)], axis=1)], axis=1)
    sheared = np.concatenate([pts, np.stack([320 + (pts[:, 0] - 128) + 0.8 * (pts[:, 1] - 96), 240 + (pts[:, 1] - 96)], axis=1)], axis=1)
    add("codes", [(planted_scene(19, 0.0, 1)[0], WH), (clutter, WH), (squeezed, WH), (sheared, WH), (planted_scene(40, 0.2, 2)[0], WH)],
        expect=[1, 3, 4, 4, 0])
    # eight pictures of different sizes in one launch, one of them without pairs; an off-centre principal point
    ms = [17, 0, 512, 33, 129, 64, 300, 5]
    whs = [(256, 192), (96, 96), (1024, 768), (640, 480), (333, 217), (192, 256), (500, 400), (128, 100)]
    add("eight", [(planted_scene(m, 0.4 if m >= 33 else 0.0, 50 + m, wh=wh, frame_wh=(1280, 720), calib4=(900.0, 905.0, 650.5, 351.25),
                                 noise_px=0.4 if m >= 33 else 0.0)[0], wh) for m, wh in zip(ms, whs)],
        iterations=300, min_inliers=12, frame=(1280, 720), calib=(900.0, 905.0, 650.5, 351.25), seed=99)
    return L


def run_launch(launch):
    return [homography_oracle(xy, wh, launch["frame"], launch["calib"], launch["iterations"] if launch["rand4"] is None else len(launch["rand4"]),
                              launch["thr"], launch["min_inliers"], launch["seed"], launch["rand4"]) for xy, wh in launch["images"]]


# ---- the launches of the match tests: every entry is one alva_image_match call

def flip(desc, bits):
    """a copy of the 32-byte descriptor with the given bit positions inverted: its distance to the original is len(bits)"""
    out = np.array(desc, np.uint8)
    for b in bits:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def _random_frame(rng, cap):
    return rng.integers(0, 256, (cap, 32), dtype=np.uint8), rng.uniform(0, 640, (cap, 2)).astype(np.float32)


def _image(rng, nq, tdesc, n_live, near=0.5):
    """nq queries: a share `near` of them copies of live train rows with 0 .. 40 bits inverted (several may copy one row), the rest random"""
    qdesc = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    for q in range(nq):
        if n_live and rng.random() < near:
            qdesc[q] = flip(tdesc[rng.integers(0, n_live)], rng.permutation(256)[:rng.integers(0, 41)])
    return qdesc, rng.uniform(0, 256, (nq, 2)).astype(np.float32)


def match_launches():
    L = []
    rng = np.random.default_rng(2024)

    def add(name, images, tdesc, txy, n_train, max_dist=64, ratio=0.8, expect=None):
        L.append(dict(name=name, images=images, tdesc=tdesc, txy=txy, n_train=n_train, max_dist=max_dist, ratio=ratio, expect=expect))

    # query counts around the wave (64) and the workgroup (256), one call
    tdesc, txy = _random_frame(rng, 2048)
    add("query-sizes", [_image(rng, nq, tdesc, 2048) for nq in (0, 1, 63, 64, 65, 255, 257, 512)], tdesc, txy, 2048)
    # frame counts: none, one (second = 257), two, one past four chunks, and a device count above the block's capacity
    for cap, n_train in ((0, 0), (64, 0), (1, 1), (2, 2), (257, 257), (300, 257), (100, 150), (64, -3)):
        tdesc, txy = _random_frame(rng, cap)
        add(f"train-{cap}-{n_train}", [_image(rng, 65, tdesc, min(max(n_train, 0), cap), near=0.8)], tdesc, txy, n_train)
    # eight pictures of different sizes, one of them empty
    tdesc, txy = _random_frame(rng, 1500)
    add("eight", [_image(rng, nq, tdesc, 1500) for nq in (300, 17, 0, 512, 64, 129, 1, 450)], tdesc, txy, 1500)

    # the edges, built bit by bit.  Train rows 0 .. 299 random (a random pair is ~128 +- 8 bits apart); the rows named below are planted
    def edges(ratio, plan):
        """plan: per query (train rows to plant as {row: bits inverted from the query}, expected train row or None)"""
        tdesc, txy = _random_frame(rng, 300)
        qdesc = rng.integers(0, 256, (len(plan), 32), dtype=np.uint8)
        expect = {}
        for q, (rows, want) in enumerate(plan):
            for row, (src, nbits) in rows.items():
                base = qdesc[q] if src is None else qdesc[src]
                if src is not None:
                    qdesc[q] = base
                tdesc[row] = flip(base, range(nbits))
            expect[q] = want
        return [(qdesc, rng.uniform(0, 256, (len(plan), 2)).astype(np.float32))], tdesc, txy, expect

    # ratio 0.8: best == max_dist is accepted, one more is not
    img, tdesc, txy, expect = edges(0.8, [({10: (None, 64)}, 10), ({11: (None, 65)}, None), ({12: (None, 0)}, 12)])
    add("edge-max-dist", img, tdesc, txy, 300, 64, 0.8, expect)
    # ratio 0.5: best 10 against second 20 is exactly ratio * second and is refused by `<`; 9 against 20 is accepted
    img, tdesc, txy, expect = edges(0.5, [({20: (None, 10), 21: (None, 20)}, None), ({30: (None, 9), 31: (None, 20)}, 30),
                                          ({40: (None, 20), 41: (None, 10)}, None)])
    add("edge-ratio", img, tdesc, txy, 300, 64, 0.5, expect)
    # a distance tie on two train rows: the lower index is the best, the other one the second -- refused at ratio 0.8 ...
    plan = [({50: (None, 5), 45: (None, 5)}, None)]
    img, tdesc, txy, expect = edges(0.8, plan)
    add("edge-train-tie", img, tdesc, txy, 300, 64, 0.8, expect)
    # ... and at ratio 1.5, where it passes, the lower row is named.  Two queries (1, 2: identical) and three (3, 4, 5: identical) claim
    # one row at equal distance: the lowest query keeps it; of 6, 7, 8 the closest (8) does
    plan = [({50: (None, 5), 45: (None, 5)}, 45), ({60: (None, 7)}, 60), ({60: (1, 7)}, None), ({70: (None, 3)}, 70), ({70: (3, 3)}, None),
            ({70: (3, 3)}, None)]
    img, tdesc, txy, expect = edges(1.5, plan)
    qdesc, qxy = img[0]
    qdesc = np.concatenate([qdesc, np.stack([flip(tdesc[80], range(6)), flip(tdesc[80], range(100, 106)), flip(tdesc[80], range(200, 204))])])
    qxy = np.concatenate([qxy, qxy[:3] + 1])
    expect.update({6: None, 7: None, 8: 80})
    add("edge-claims", [(qdesc, qxy)], tdesc, txy, 300, 64, 1.5, expect)
    return L


def pack_images(images):
    """[(qdesc [nq, 32], qxy [nq, 2])] -> the stage's blocks: qdesc [n, QUERY_CAP, 32] uint8, qxy [n, QUERY_CAP, 2] float32, nq [n] int32"""
    n = len(images)
    qdesc, qxy, nq = np.zeros((n, QUERY_CAP, 32), np.uint8), np.zeros((n, QUERY_CAP, 2), np.float32), np.zeros(n, np.int32)
    for j, (d, xy) in enumerate(images):
        nq[j] = len(d)
        qdesc[j, :len(d)], qxy[j, :len(d)] = d, xy
    return qdesc, qxy, nq


def run_match_launch(launch):
    return [match_oracle(d, xy, launch["tdesc"], launch["txy"], launch["n_train"], launch["max_dist"], launch["ratio"]) for d, xy in launch["images"]]


# ---- the chain on rendered frames: ORB (the oracle's) -> match -> homography -> a least-squares refit standing in for the refinement

CHAIN_FRAMES = (0, 60, 120, 200, 300)
CHAIN_F = 554.256
CROP_WH = (256, 192)


def lstsq_homography(p, q):
    rows, rhs = [], []
    for (x, y), (u, v) in zip(p, q):
        rows += [[x, y, 1, 0, 0, 0, -x * u, -y * u], [0, 0, 0, x, y, 1, -x * v, -y * v]]
        rhs += [u, v]
    return np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0]


def chain_pictures(width=FRAME[0], height=FRAME[1]):
    """(canvas of the stream, the crop the tests look for, a crop of the same place from another canvas, the crop's origin in the canvas)"""
    from alvaar_amd import synth
    canvas = synth.texture_canvas(width, height, 5)
    ch, cw = canvas.shape
    x0, y0 = cw // 2 - 100, ch // 2 - 80
    crop = np.ascontiguousarray(canvas[y0:y0 + CROP_WH[1], x0:x0 + CROP_WH[0]])
    distractor = np.ascontiguousarray(synth.texture_canvas(width, height, 11)[y0:y0 + CROP_WH[1], x0:x0 + CROP_WH[0]])
    return canvas, crop, distractor, (x0, y0)


def crop_pose_in_camera(k, canvas_shape, origin, f=CHAIN_F):
    """the analytic pose of the crop in the camera of stream frame k, in units of the crop's width: (R, t, width in metres)"""
    from alvaar_amd import synth
    ch, cw = canvas_shape
    centre = np.array([(origin[0] + CROP_WH[0] / 2 - cw / 2) * 4 / f, (origin[1] + CROP_WH[1] / 2 - ch / 2) * 4 / f, 4.0])
    width = CROP_WH[0] * 4 / f   # (the picture's axes are the world's: x right, y down, z into the plane)
    R_wc, t_wc = synth.plane_camera_pose(k)
    return R_wc.T, R_wc.T @ (centre - t_wc) / width, width


def pose_errors(R, t, R_true, t_true):
    """(rotation error in degrees, centre error relative to the distance)"""
    ang = np.degrees(np.arccos(np.clip((np.trace(R.T @ R_true) - 1) / 2, -1, 1)))
    return float(ang), float(np.linalg.norm(t - t_true) / np.linalg.norm(t_true))


def chain_rows(frames=CHAIN_FRAMES):
    """per frame: pairs, consensus, pose errors of the minimal sample and of the refit for the crop, and the distractor's numbers"""
    from alvaar_amd import synth
    from oracles import Orc
    W, H = FRAME
    canvas, crop, distractor, origin = chain_pictures()
    targets = [Orc.orb(img, 500, 1.2, 7, 20) for img in (crop, distractor)]
    rows = []
    for k in frames:
        R_wc, t_wc = synth.plane_camera_pose(k)
        frame = synth.render_plane(canvas, W, H, CHAIN_F, R_wc, t_wc)
        kp, desc = Orc.orb(frame, 1500, 1.2, 8, 20)
        R_true, t_true, _ = crop_pose_in_camera(k, canvas.shape, origin)
        row = dict(k=k, n_frame=len(kp))
        for name, (tkp, tdesc) in zip(("crop", "distractor"), targets):
            match, xy = match_oracle(tdesc, tkp[:, :2], desc, kp[:, :2], len(kp), 64, 0.8)
            out = homography_oracle(xy, CROP_WH, FRAME, CALIB, 256, 3.0, 20)
            r = dict(pairs=len(match), code=int(out["info"][0]), count=int(out["info"][3]))
            if name == "crop" and out["info"][0] == 0:
                r["minimal"] = pose_errors(out["R"].reshape(3, 3), out["t"], R_true, t_true)
                p, q, s = normalise(xy, CROP_WH, FRAME)
                keep = out["mask"][:len(xy)].astype(bool)
                h = lstsq_homography(p[keep], q[keep])
                code, R, t = pose_from_h(h, s, FRAME, CALIB)
                r["refit"] = pose_errors(R, t, R_true, t_true) if code == 0 else None
                # the refit's rms transfer error over its inliers, in pixels
                hm = np.append(h, 1.0).reshape(3, 3)
                pr = (hm @ np.c_[p[keep], np.ones(keep.sum())].T).T
                r["rms_px"] = float(np.sqrt(np.mean(np.sum((pr[:, :2] / pr[:, 2:] - q[keep]) ** 2, axis=1))) * s)
            row[name] = r
        rows.append(row)
    return rows
