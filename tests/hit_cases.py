"""The hit test's definition (include/alvaar_hip.h, alva_hit_test) restated in numpy, line for line, and the scenes the tests run it on.
The reference has no hit test, so this file is what alva_hit_test is pinned to (tests/test_hit_cases.py checks the restatement itself,
tests/test_gpu_hit_test.py the kernel against it).

All decisions are taken in float64 with the operation order written here, which is the kernel's (elementwise numpy does not contract
a * b + c into an FMA; nothing below goes through a BLAS product).  Beside its result the oracle returns three margins -- how far the
scene is from a decision that could fall the other way under a last-bit difference:
  sel_margin   min over the points in front of the camera of |d^2 / radius^2 - 1|
  gap_margin   (second best score - best score) / best score, over hypotheses that draw another index triple than the winner
               (inf when there is no other, or when both are exactly 0: exact zeros tie on both sides and the lowest iteration wins)
  thr_margin   min over the selected points of |distance / threshold - 1| (threshold 0: points at distance exactly 0 are inliers by
               `<=`, the others are infinitely far from it)
Every case a GPU test compares must have all three >= MARGIN_MIN."""
from __future__ import annotations

import numpy as np

HIT_CAP = 2048
MIN_SELECTED, MIN_INLIERS = 24, 16
INLIER_FACTOR = 3.7065     # 2.5 x 1.4826
MIN_COS = 0.0872
MARGIN_MIN = 1e-7
MIN_EIG_RATIO = 100.0
K_BASE = (579.4, 579.4, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0)
POSE_BASE = np.array([0.1, -0.05, 0.2, 0.0, 0.0, 0.0, 1.0])
BASE_TAPS = [((250.0, 240.0), 40.0), ((560.0, 240.0), 40.0), ((320.0, 100.0), 40.0), ((5.0, 5.0), 40.0), ((5.0, 5.0), 80.0)]


def hash32(x: int) -> int:
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def sample_words(seed: int, num_iterations: int) -> np.ndarray:
    return np.array([[hash32(seed ^ (((3 * it + j) * 0x9E3779B9) & 0xFFFFFFFF)) for j in range(3)] for it in range(num_iterations)], np.uint32)


def words_for(indices, m: int) -> np.ndarray:
    """explicit words that select the given indices among m points: the smallest w with (w * m) >> 32 == index"""
    return np.array([[-((-int(i) << 32) // m) for i in row] for row in indices], np.uint32)


def quat_to_rot(q):
    """R_wc of pose7's quaternion (x y z w), the operation order of the library's quat_to_rot"""
    x, y, z, w = (np.float64(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def undistort(calib8, u, v):
    """alva_undistort_dev (cv::undistortPoints with R = K, 5 fixed iterations): float32 in, float32 out"""
    fx, fy, cx, cy, k1, k2, p1, p2 = (np.float64(c) for c in calib8)
    ifx, ify = 1.0 / fx, 1.0 / fy
    u, v = np.float64(np.float32(u)), np.float64(np.float32(v))
    x = (u - cx) * ifx
    y = (v - cy) * ify
    x0, y0 = x, y
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((0 * r2 + 0) * r2 + 0) * r2) / (1 + ((0 * r2 + k2) * r2 + k1) * r2)
        if icdist < 0:
            x = (u - cx) * ifx
            y = (v - cy) * ify
            break
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + 0 * r2 + 0 * r2 * r2
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + 0 * r2 + 0 * r2 * r2
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    xx, yy, ww = fx * x + 0 * y + cx, 0 * x + fy * y + cy, 1.0 / (0 * x + 0 * y + 1)
    return np.float32(xx * ww), np.float32(yy * ww)


def _distances(Q, q0, n):
    d = Q - q0
    return np.abs((d[:, 0] * n[0] + d[:, 1] * n[1]) + d[:, 2] * n[2])


def oracle(P, pose7, calib8, uv, radius_px, num_iterations=64, seed=12345, rand3=None):
    """One ray.  Returns a dict: code, m, best_it, n_in, n_sel (info[0..4]), moments [10], pose [16] float32 (code 0), the three
    margins, eig_ratio (code 0 / 4), sel (indices of the kept points)."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    pose7 = np.asarray(pose7, np.float64)
    t, R = pose7[:3], quat_to_rot(pose7[3:])
    fx, fy, cx, cy = (np.float64(c) for c in calib8[:4])
    out = dict(code=1, m=0, best_it=-1, n_in=0, n_sel=0, moments=np.zeros(10), pose=np.zeros(16, np.float32), sel_margin=np.inf,
               gap_margin=np.inf, thr_margin=np.inf, eig_ratio=np.inf, sel=np.zeros(0, np.int64))
    # 1. ray
    uu, vv = (np.float64(c) for c in undistort(calib8, uv[0], uv[1]))
    dc = np.array([(uu - cx) / fx, (vv - cy) / fy, 1.0])
    dc = dc / np.sqrt(dc[0] * dc[0] + dc[1] * dc[1] + dc[2] * dc[2])
    dw = np.array([R[i, 0] * dc[0] + R[i, 1] * dc[1] + R[i, 2] * dc[2] for i in range(3)])
    # 2. selection
    r2 = np.float64(np.float32(radius_px)) * np.float64(np.float32(radius_px))
    if len(P):
        d = P - t
        pcx = (R[0, 0] * d[:, 0] + R[1, 0] * d[:, 1]) + R[2, 0] * d[:, 2]
        pcy = (R[0, 1] * d[:, 0] + R[1, 1] * d[:, 1]) + R[2, 1] * d[:, 2]
        pcz = (R[0, 2] * d[:, 0] + R[1, 2] * d[:, 1]) + R[2, 2] * d[:, 2]
        front = pcz > 0
        with np.errstate(all="ignore"):
            eu = (fx * pcx / pcz + cx) - uu
            ev = (fy * pcy / pcz + cy) - vv
            d2 = eu * eu + ev * ev
        sel = np.nonzero(front & (d2 <= r2))[0]
        if front.any():
            out["sel_margin"] = float(np.abs(d2[front] / r2 - 1).min())
    else:
        sel = np.zeros(0, np.int64)
    out["n_sel"] = len(sel)
    sel = sel[:HIT_CAP]
    m = len(sel)
    out["m"], out["sel"] = m, sel
    if m < MIN_SELECTED:
        return out
    Q = P[sel]
    # 3. hypotheses
    words = sample_words(seed, num_iterations) if rand3 is None else np.asarray(rand3, np.uint32).reshape(-1, 3)
    k = m // 2
    best, best_score, best_n, best_q0, scored = -1, np.inf, None, None, []
    for it in range(len(words)):
        i0, i1, i2 = ((int(w) * m) >> 32 for w in words[it])
        if i0 == i1 or i0 == i2 or i1 == i2:
            continue
        u, w = Q[i1] - Q[i0], Q[i2] - Q[i0]
        c = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]])
        nn = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        if not nn > 0:
            continue
        n = c / nn
        score = np.partition(_distances(Q, Q[i0], n), k)[k]
        scored.append((score, (i0, i1, i2)))
        if score < best_score:
            best, best_score, best_n, best_q0, best_triple = it, score, n, Q[i0], (i0, i1, i2)
    out["code"] = 2
    if best < 0:
        return out
    out["best_it"] = best
    others = [s for s, triple in scored if triple != best_triple]
    if others:
        second = min(others)
        if not (second == 0 and best_score == 0):
            out["gap_margin"] = float((second - best_score) / best_score) if best_score > 0 else np.inf
    # 4. inliers
    dist = _distances(Q, best_q0, best_n)
    thr = INLIER_FACTOR * best_score
    inl = dist <= thr
    if thr > 0:
        out["thr_margin"] = float(np.abs(dist / thr - 1).min())
    n_in = int(inl.sum())
    out["n_in"] = n_in
    X = Q[inl] - best_q0
    out["moments"] = np.array([float(n_in), X[:, 0].sum(), X[:, 1].sum(), X[:, 2].sum(), (X[:, 0] * X[:, 0]).sum(), (X[:, 0] * X[:, 1]).sum(),
                               (X[:, 0] * X[:, 2]).sum(), (X[:, 1] * X[:, 1]).sum(), (X[:, 1] * X[:, 2]).sum(), (X[:, 2] * X[:, 2]).sum()])
    out["moment_scale"] = np.array([float(n_in), np.abs(X[:, 0]).sum(), np.abs(X[:, 1]).sum(), np.abs(X[:, 2]).sum(), (X[:, 0] * X[:, 0]).sum(),
                                    np.abs(X[:, 0] * X[:, 1]).sum(), np.abs(X[:, 0] * X[:, 2]).sum(), (X[:, 1] * X[:, 1]).sum(),
                                    np.abs(X[:, 1] * X[:, 2]).sum(), (X[:, 2] * X[:, 2]).sum()])   # the sums of |terms| the tolerance scales with
    out["code"] = 3
    if n_in < MIN_INLIERS:
        return out
    # 5. refit: centroid and covariance from the moments about Q0, normal = eigenvector of the smallest eigenvalue, facing the camera
    mom = out["moments"]
    mu = mom[1:4] / n_in
    S = np.array([[mom[4], mom[5], mom[6]], [mom[5], mom[7], mom[8]], [mom[6], mom[8], mom[9]]]) / n_in - np.outer(mu, mu)
    lam, V = np.linalg.eigh(S)
    out["eig_ratio"] = float(lam[1] / lam[0]) if lam[0] > 0 else np.inf
    n = V[:, 0] / np.linalg.norm(V[:, 0])
    c = best_q0 + mu
    if not n @ (t - c) > 0:
        n = -n
    # 6. intersection
    out["code"] = 4
    den = n @ dw
    if not abs(den) >= MIN_COS:
        return out
    lmb = n @ (c - t) / den
    if not lmb > 0:
        return out
    p = t + lmb * dw
    # 7. pose
    x = None
    for col in (0, 1):
        a = R[:, col]
        x = a - (a @ n) * n
        if np.linalg.norm(x) >= 1e-6:
            break
    x = x / np.linalg.norm(x)
    z = np.cross(x, n)
    pose = np.zeros(16, np.float32)
    pose[0:3], pose[4:7], pose[8:11], pose[12:15], pose[15] = x, n, z, p, 1.0
    out["pose"], out["code"] = pose, 0
    out["normal"], out["point"], out["ray"] = n, p, dw
    return out


def info_of(r) -> list:
    return [r["code"], r["m"], r["best_it"], r["n_in"], r["n_sel"], 0, 0, 0]


def margins_ok(r) -> bool:
    return min(r["sel_margin"], r["gap_margin"], r["thr_margin"]) >= MARGIN_MIN and (r["code"] not in (0, 4) or r["eig_ratio"] >= MIN_EIG_RATIO)


# ---------------------------------------------------------------------------------------------------- scenes
def base_scene():
    """floor z = 4 (1600 points), wall x = 1.2 (900), clutter (300), shuffled.  RandomState(1); each surface's 0.003 randn noise is drawn
    right after the surface's own coordinates -- the order that gives the selection counts 44 / 46 / 50 / 7 / 31 for BASE_TAPS"""
    rng = np.random.RandomState(1)
    nf, nw, ncl = 1600, 900, 300
    floor = np.column_stack([rng.uniform(-2, 1.2, nf), rng.uniform(-1.5, 1.5, nf), np.full(nf, 4.0)]) + 0.003 * rng.randn(nf, 3)
    wall = np.column_stack([np.full(nw, 1.2), rng.uniform(-1.5, 1.5, nw), rng.uniform(2.0, 4.0, nw)]) + 0.003 * rng.randn(nw, 3)
    clutter = np.column_stack([rng.uniform(-2, 2, ncl), rng.uniform(-1.5, 1.5, ncl), rng.uniform(1.5, 6, ncl)])
    P = np.vstack([floor, wall, clutter])
    rng.shuffle(P)
    return np.ascontiguousarray(P)


def backproject(uv, depth, pose7=POSE_BASE, calib8=K_BASE):
    """world points at the given depths along the (undistorted = raw, for zero distortion) pixels uv [n,2]"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    depth = np.broadcast_to(np.asarray(depth, np.float64), (len(uv),))
    t, R = np.asarray(pose7[:3], np.float64), quat_to_rot(pose7[3:])
    pc = np.column_stack([(uv[:, 0] - calib8[2]) / calib8[0] * depth, (uv[:, 1] - calib8[3]) / calib8[1] * depth, depth])
    return pc @ R.T + t


def disc_pixels(rng, n, centre, radius):
    """n pixels uniformly inside a disc"""
    r, a = radius * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    return np.column_stack([centre[0] + r * np.cos(a), centre[1] + r * np.sin(a)])


def plane_under_tap(rng, n, tap=(320.0, 240.0), radius=30.0, depth=4.0, noise=0.002, tilt=(0.2, -0.1), pose7=POSE_BASE, calib8=K_BASE):
    """n points of a tilted plane (camera-frame depth = depth + tilt . normalised pixel offset, plus noise) that all project inside
    `radius` of the tap"""
    uv = disc_pixels(rng, n, tap, radius)
    xn, yn = (uv[:, 0] - calib8[2]) / calib8[0], (uv[:, 1] - calib8[3]) / calib8[1]
    return backproject(uv, depth + tilt[0] * xn + tilt[1] * yn + noise * rng.randn(n), pose7, calib8)


def far_points(rng, n, pose7=POSE_BASE, calib8=K_BASE):
    """n points in front of the camera that project far outside any tap's circle used here (pixels 2000 .. 3000 to the right)"""
    uv = np.column_stack([rng.uniform(2000, 3000, n), rng.uniform(-500, 900, n)])
    return backproject(uv, rng.uniform(2, 6, n), pose7, calib8)


def pick_seed(P, pose7, calib8, uv, radius, want_code, num_iterations=64, first=1):
    """the first seed >= first under which the oracle gives want_code with every margin above the guard (chosen on the CPU, as the
    definition's test plan asks; the guard itself is never relaxed)"""
    for seed in range(first, first + 200):
        r = oracle(P, pose7, calib8, uv, radius, num_iterations, seed)
        if r["code"] == want_code and margins_ok(r):
            return seed
    raise AssertionError("no seed gives code %d with safe margins" % want_code)


CENTRE = (320.0, 240.0)
K_DIST = (579.4, 579.4, 320.0, 240.0, -0.12, 0.03, 0.001, -0.0015)


def edge_cases():
    """name -> dict(P, pose7, calib8, taps [(uv, radius)], kw for oracle / Context.hit_test, want = expected codes or None): the edge
    scenes of tests/test_gpu_hit_test.py, at the smallest sizes that exercise them; tests/test_hit_cases.py asserts on the CPU that each
    is far from every last-bit decision"""
    rng = np.random.RandomState(11)
    cases = {}

    def add(name, P, taps=((CENTRE, 40.0),), pose7=POSE_BASE, calib8=K_BASE, want=None, **kw):
        cases[name] = dict(P=np.ascontiguousarray(P, np.float64).reshape(-1, 3), pose7=np.asarray(pose7, np.float64), calib8=tuple(calib8),
                           taps=list(taps), kw=kw, want=want)

    add("n0", np.zeros((0, 3)), want=[1])
    for n in (63, 64, 65):
        add("n%d" % n, plane_under_tap(rng, n), want=[0])
    plane = plane_under_tap(rng, 24)
    far = far_points(rng, 700)
    add("m23", np.vstack([far[:300], plane[:23], far[300:]]), want=[1])
    add("m24", np.vstack([far[:300], plane[:12], far[300:], plane[12:]]), want=[0])
    add("cap5000", plane_under_tap(rng, 5000), want=[0])
    front = plane_under_tap(rng, 40)
    add("behind", np.vstack([2 * POSE_BASE[:3] - front, front]), want=[0])
    mid = plane_under_tap(rng, 60)
    add("iters1", mid, want=[0], num_iterations=1)
    add("iters250", mid, want=[0], num_iterations=250, seed=pick_seed(mid, POSE_BASE, K_BASE, CENTRE, 40.0, 0, 250))
    add("rays16", base_scene(), taps=[((100.0 + 140.0 * (i % 4), 90.0 + 100.0 * (i // 4)), 40.0) for i in range(16)])
    add("skip_first", mid, want=[0], rand3=np.vstack([[[0, 0, 1 << 31]], words_for([[3, 17, 40]], 60)]))
    add("skip_all", mid, want=[2], rand3=np.array([[0, 0, 1 << 31], [5, 5, 9], [1 << 30, 7, 1 << 30]], np.uint32))
    line = POSE_BASE[:3] + np.array([[0.0, 0.0, 4.0], [0.125, 0.0, 4.0], [0.25, 0.0, 4.0]])   # same y and z: the cross product is exactly 0
    col = np.vstack([line, mid])
    add("collinear_then_plane", col, want=[0], rand3=words_for([[0, 1, 2], [5, 20, 45]], 63))
    add("collinear_only", col, want=[2], rand3=words_for([[0, 1, 2], [2, 0, 1]], 63))
    gx, gy = np.meshgrid(np.arange(-8, 8) / 64.0, np.arange(-6, 6) / 64.0)
    add("exact_plane", np.column_stack([gx.ravel(), gy.ravel(), np.full(gx.size, 4.0)]), want=[0])
    # half a plane, half clutter: the rank m / 2 distance is the plane's, and fewer than 16 of the 24 points lie within 3.7065 x it
    half = np.vstack([plane_under_tap(rng, 13, noise=0.001), backproject(disc_pixels(rng, 11, CENTRE, 30.0), rng.uniform(1.5, 8.0, 11))])
    add("code3", half, want=[3], seed=pick_seed(half, POSE_BASE, K_BASE, CENTRE, 40.0, 3))
    # a plane seen at 87 degrees: depth 4 / (1 - tan(87 deg) x_n) along the pixel column x_n
    uv = np.column_stack([CENTRE[0] + rng.uniform(-12, 12, 80), CENTRE[1] + rng.uniform(-30, 30, 80)])
    xn = (uv[:, 0] - K_BASE[2]) / K_BASE[0]
    add("grazing", backproject(uv, 4.0 / (1.0 - np.tan(np.deg2rad(87.0)) * xn) + 0.0005 * rng.randn(80)), want=[4])
    add("outside_image", base_scene(), taps=[((-200.0, -200.0), 40.0)], want=[1])
    add("distorted", base_scene(), taps=[((250.0, 240.0), 40.0), ((520.0, 260.0), 40.0), ((330.0, 120.0), 40.0)], calib8=K_DIST, want=[0, 0, 0])
    q = np.array([0.05, -0.08, 0.03, 1.0])
    add("rotated", base_scene(), taps=[((250.0, 240.0), 40.0), ((500.0, 240.0), 40.0)], pose7=np.concatenate([POSE_BASE[:3], q / np.linalg.norm(q)]))
    return cases


def oracle_case(case):
    return [oracle(case["P"], case["pose7"], case["calib8"], uv, radius, **case["kw"]) for uv, radius in case["taps"]]
