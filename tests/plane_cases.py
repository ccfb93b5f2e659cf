"""The plane detector's definition (include/alvaar_hip.h, alva_detect_planes) restated in numpy, line for line, and the scenes the
tests run it on.  The reference has no plane detection, so this file is what alva_detect_planes is pinned to
(tests/test_plane_cases.py checks the restatement itself, tests/test_gpu_detect_planes.py the kernel against it).

All decisions are taken in float64 with the operation order written here, which is the kernel's (elementwise numpy does not contract
a * b + c into an FMA; nothing that decides goes through a BLAS product).  The eigenvectors come from numpy.linalg.eigh where the
kernel runs a cyclic Jacobi; the margins below keep every decision downstream of them away from the last bits:
  thr_margin   min over every scored hypothesis of every run round and every live point, over the consensus set's distances and over
               the refit's distances, of | |d| / thickness - 1 |
  eig_ratio    lambda1 / lambda0 of the refit's covariance (>= 100: the normal is defined)
  axis_ratio   lambda2 / lambda1 (>= 1.1: the long axis is defined)
  sign_margin  |x . a| (>= 1e-3: the sign of the long axis is defined), a being the axis the definition orients x by
  ref_margin   | |R_wc[:,0] . nrm| - 0.9 | (>= 1e-3: which axis that is, R_wc[:,0] or R_wc[:,1], is defined)
  face_margin  |nrm . (t - c)| / |t - c| (>= 1e-3: the side the normal faces is defined)
Every case a GPU test compares must have thr_margin >= MARGIN_MIN and, per found plane, the five guards."""
from __future__ import annotations

import functools

import numpy as np

import hit_cases as H

N_CAP = 16384
MARGIN_MIN = H.MARGIN_MIN
MIN_EIG_RATIO, MIN_AXIS_RATIO, MIN_SIGN, MIN_FACE, MIN_REF = 100.0, 1.1, 1e-3, 1e-3, 1e-3
AXIS_SWITCH = 0.9
POSE_BASE = H.POSE_BASE
NOT_RUN = [5, 0, -1, 0, 0, 0, 0, 0]


def sample_words(seed: int, r: int, num_iterations: int) -> np.ndarray:
    """round r's words: w_j = h(seed ^ ((3 (r * num_iterations + it) + j) * 0x9E3779B9))"""
    return np.array([[H.hash32(seed ^ (((3 * (r * num_iterations + it) + j) * 0x9E3779B9) & 0xFFFFFFFF)) for j in range(3)]
                     for it in range(num_iterations)], np.uint32)


def _dist(X, n):
    """(dx nx + dy ny) + dz nz, signed"""
    return (X[:, 0] * n[0] + X[:, 1] * n[1]) + X[:, 2] * n[2]


def _margin(d, thickness):
    return float(np.abs(np.abs(d) / thickness - 1).min()) if len(d) else np.inf


def oracle(P, pose7, thickness, min_inliers=48, max_planes=4, num_iterations=128, seed=12345, rand3=None):
    """Returns a dict: info [max_planes, 8] int32, planes [max_planes, 24] float32, moments and moment_scale [max_planes, 10], labels [n],
    found (the return value), thr_margin, and per found plane a dict in `guards` (eig_ratio, axis_ratio, sign_margin, ref_margin,
    face_margin, normal, centre, x)."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    pose7 = np.asarray(pose7, np.float64)
    t, R = pose7[:3], H.quat_to_rot(pose7[3:])
    thickness = np.float64(thickness)
    n = len(P)
    info = np.tile(np.array(NOT_RUN, np.int32), (max_planes, 1))
    planes = np.zeros((max_planes, 24), np.float32)
    moments, scale = np.zeros((max_planes, 10)), np.zeros((max_planes, 10))
    labels = np.full(n, -1, np.int32)
    out = dict(info=info, planes=planes, moments=moments, moment_scale=scale, labels=labels, found=0, thr_margin=np.inf, guards=[])
    words_all = None if rand3 is None else np.asarray(rand3, np.uint32).reshape(-1, 3)
    for r in range(max_planes):
        live = np.nonzero(labels == -1)[0]   # ascending index
        m = len(live)
        # 1. too few points
        if m < min_inliers:
            info[r] = [1, m, -1, 0, 0, 0, 0, 0]
            return out
        L = P[live]
        # 2. hypotheses
        words = sample_words(seed, r, num_iterations) if words_all is None else words_all[r * num_iterations:(r + 1) * num_iterations]
        best, best_count, best_n, best_q0 = -1, -1, None, None
        for it in range(num_iterations):
            i0, i1, i2 = ((int(w) * m) >> 32 for w in words[it])
            if i0 == i1 or i0 == i2 or i1 == i2:
                continue
            u, w = L[i1] - L[i0], L[i2] - L[i0]
            c = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]])
            nn = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
            if not nn > 0:
                continue
            nh = c / nn
            d = _dist(L - L[i0], nh)
            out["thr_margin"] = min(out["thr_margin"], _margin(d, thickness))
            count = int((np.abs(d) <= thickness).sum())
            # 3. the largest count wins, the lowest `it` on ties
            if count > best_count:
                best, best_count, best_n, best_q0 = it, count, nh, L[i0]
        if best < 0:
            info[r] = [2, m, -1, 0, 0, 0, 0, 0]
            return out
        if best_count < min_inliers:
            info[r] = [3, m, best, best_count, 0, 0, 0, 0]
            return out
        # 4. refit over the winner's consensus set: ten moments of x = P_i - Q0
        X = L - best_q0
        X = X[np.abs(_dist(X, best_n)) <= thickness]
        assert len(X) == best_count
        terms = [np.ones(len(X)), X[:, 0], X[:, 1], X[:, 2], X[:, 0] * X[:, 0], X[:, 0] * X[:, 1], X[:, 0] * X[:, 2], X[:, 1] * X[:, 1],
                 X[:, 1] * X[:, 2], X[:, 2] * X[:, 2]]
        mom = np.array([v.sum() for v in terms])
        moments[r], scale[r] = mom, np.array([np.abs(v).sum() for v in terms])
        inv = 1.0 / np.float64(best_count)
        mu = mom[1:4] * inv
        S = np.array([[mom[4] * inv - mu[0] * mu[0], mom[5] * inv - mu[0] * mu[1], mom[6] * inv - mu[0] * mu[2]],
                      [0, mom[7] * inv - mu[1] * mu[1], mom[8] * inv - mu[1] * mu[2]], [0, 0, mom[9] * inv - mu[2] * mu[2]]])
        S = S + np.triu(S, 1).T
        lam, V = np.linalg.eigh(S)
        c = best_q0 + mu
        nrm = V[:, 0] / np.linalg.norm(V[:, 0])
        facing = nrm @ (t - c)
        if not facing > 0:
            nrm = -nrm
        # 5. final set
        d = _dist(L - c, nrm)
        out["thr_margin"] = min(out["thr_margin"], _margin(d, thickness))
        F = np.abs(d) <= thickness
        n_in = int(F.sum())
        if n_in < min_inliers:
            info[r] = [4, m, best, best_count, n_in, 0, 0, 0]
            return out
        labels[live[F]] = r
        # 6. extent: the long axis is the eigenvector of the LARGEST eigenvalue of the step-4 covariance
        # (oriented by the camera's x axis, or by its y axis when the plane faces along the camera's x axis)
        an = R[0, 0] * nrm[0] + R[1, 0] * nrm[1] + R[2, 0] * nrm[2]
        a = R[:, 1] if abs(an) > AXIS_SWITCH else R[:, 0]
        x = V[:, 2] - (V[:, 2] @ nrm) * nrm
        x = x / np.linalg.norm(x)
        if x @ a < 0:
            x = -x
        z = np.cross(x, nrm)
        ex, ez = _dist(L[F] - c, x), _dist(L[F] - c, z)
        lo_x, hi_x, lo_z, hi_z = ex.min(), ex.max(), ez.min(), ez.max()
        p = c + ((lo_x + hi_x) / 2) * x + ((lo_z + hi_z) / 2) * z
        # 7. record
        planes[r, 0:3], planes[r, 4:7], planes[r, 8:11], planes[r, 12:15], planes[r, 15] = x, nrm, z, p, 1.0
        planes[r, 16], planes[r, 17], planes[r, 18] = hi_x - lo_x, hi_z - lo_z, nrm @ p
        info[r] = [0, m, best, best_count, n_in, 0, 0, 0]
        out["found"] = r + 1
        out["guards"].append(dict(eig_ratio=float(lam[1] / lam[0]) if lam[0] > 0 else np.inf,
                                  axis_ratio=float(lam[2] / lam[1]) if lam[1] > 0 else np.inf, sign_margin=float(abs(x @ a)), ref_margin=float(abs(abs(an) - AXIS_SWITCH)),
                                  face_margin=float(abs(facing) / np.linalg.norm(t - c)), normal=nrm, centre=p, x=x))
    return out


def margins_ok(res) -> bool:
    return res["thr_margin"] >= MARGIN_MIN and all(g["eig_ratio"] >= MIN_EIG_RATIO and g["axis_ratio"] >= MIN_AXIS_RATIO and
                                                   g["sign_margin"] >= MIN_SIGN and g["face_margin"] >= MIN_FACE and g["ref_margin"] >= MIN_REF for g in res["guards"])


def margins_text(res) -> str:
    return "thr %.1e | " % res["thr_margin"] + " | ".join("eig %.1e axis %.2f sign %.1e face %.1e ref %.1e" % (
        g["eig_ratio"], g["axis_ratio"], g["sign_margin"], g["face_margin"], g["ref_margin"]) for g in res["guards"])


# ---------------------------------------------------------------------------------------------------- scenes
BASE_KW = dict(thickness=0.01, min_inliers=48, max_planes=4, num_iterations=128)


def noisy_plane(rng, n, noise=0.002):
    """n points of a 3 x 2 rectangle in the plane z = 4 + 0.2 x - 0.1 y in front of POSE_BASE, plus noise along z"""
    x, y = rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n)
    return np.column_stack([x, y, 4.0 + 0.2 * x - 0.1 * y + noise * rng.randn(n)]) + POSE_BASE[:3]


def pick_seed(P, pose7, want_codes, first=1, **kw):
    """the first seed >= first under which the oracle gives the wanted codes with every margin above its guard (chosen on the CPU; the
    guards themselves are never relaxed)"""
    for seed in range(first, first + 200):
        r = oracle(P, pose7, seed=seed, **kw)
        if r["info"][:, 0].tolist() == want_codes and margins_ok(r):
            return seed
    raise AssertionError("no seed gives the codes %s with safe margins" % (want_codes,))


@functools.lru_cache(maxsize=None)
def edge_cases():
    """name -> dict(P, pose7, kw for oracle / Context.detect_planes, want = expected codes per round): the edge scenes of
    tests/test_gpu_detect_planes.py at the smallest sizes that exercise them; tests/test_plane_cases.py asserts on the CPU that each is
    far from every last-bit decision"""
    rng = np.random.RandomState(21)
    cases = {}

    def add(name, P, want, pose7=POSE_BASE, seeded=False, **kw):
        P = np.ascontiguousarray(P, np.float64).reshape(-1, 3)
        kw = dict(dict(thickness=0.01, min_inliers=48, max_planes=2, num_iterations=32), **kw)
        if seeded:
            kw["seed"] = pick_seed(P, pose7, want, **kw)
        cases[name] = dict(P=P, pose7=np.asarray(pose7, np.float64), kw=kw, want=want)

    add("n0", np.zeros((0, 3)), [1, 5])
    add("n47", noisy_plane(rng, 47), [1, 5])
    # one noisy plane at the wave, workgroup and tile edges: the second round finds fewer than min_inliers live points (code 1) or no
    # second plane among the few points off the first (code 3)
    for n in (63, 64, 65, 511, 512, 513, 2047, 2048, 2049):
        P = noisy_plane(rng, n)
        want = oracle(P, POSE_BASE, thickness=0.01, min_inliers=48, max_planes=2, num_iterations=32, seed=1)["info"][:, 0].tolist()
        assert want[0] == 0 and want[1] in (1, 3), (n, want)
        add("n%d" % n, P, want, seeded=True)
    big = noisy_plane(rng, N_CAP)
    add("n16384", big, [0, 1], seeded=True, num_iterations=8)
    add("base", H.base_scene(), [0, 0, 3, 5], **BASE_KW)
    add("base_max1", H.base_scene(), [0], **dict(BASE_KW, max_planes=1))
    add("base_max8", H.base_scene(), [0, 0, 3, 5, 5, 5, 5, 5], **dict(BASE_KW, max_planes=8))
    q = np.array([0.05, -0.08, 0.03, 1.0])
    add("rotated", H.base_scene(), [0, 0, 3, 5], pose7=np.concatenate([POSE_BASE[:3], q / np.linalg.norm(q)]), **BASE_KW)
    # the hit test's exact grid: every distance is exactly 0, the extents are the grid's
    gx, gy = np.meshgrid(np.arange(-8, 8) / 64.0, np.arange(-6, 6) / 64.0)
    add("exact_plane", np.column_stack([gx.ravel(), gy.ravel(), np.full(gx.size, 4.0)]), [0, 1])
    mid = noisy_plane(rng, 60)
    kw3 = dict(num_iterations=3, max_planes=1)
    add("skip_first", mid, [0], rand3=np.vstack([[[0, 0, 1 << 31]], H.words_for([[3, 17, 40], [5, 20, 45]], 60)]), **kw3)
    add("skip_all", mid, [2], rand3=np.array([[0, 0, 1 << 31], [5, 5, 9], [1 << 30, 7, 1 << 30]], np.uint32), **kw3)
    line = POSE_BASE[:3] + np.array([[0.0, 0.0, 4.0], [0.125, 0.0, 4.0], [0.25, 0.0, 4.0]])   # same y and z: the cross product is exactly 0
    col = np.vstack([line, mid])
    add("collinear_then_plane", col, [0], rand3=H.words_for([[0, 1, 2], [5, 20, 45]], 63), num_iterations=2, max_planes=1)
    add("collinear_only", col, [2], rand3=H.words_for([[0, 1, 2], [2, 0, 1]], 63), num_iterations=2, max_planes=1)
    # tie: two exact planes of 30 grid points each (z = 4 and x = z; 6 x 5 grids, so that the long axis is defined) and 20 points off
    # both; hypothesis 0 draws the second plane, hypothesis 1 the first, both count 30: the lower `it` wins, the other follows
    g6, g5 = np.meshgrid(np.arange(6) / 8.0, np.arange(5) / 8.0)
    pa = np.column_stack([g6.ravel() - 1.0, g5.ravel(), np.full(30, 4.0)])
    pb = np.column_stack([2.0 + g6.ravel(), g5.ravel(), 2.0 + g6.ravel()])
    off = np.column_stack([rng.uniform(-0.9, 0.9, 20), rng.uniform(1.0, 2.0, 20), rng.uniform(2.2, 3.8, 20)])
    tie = np.vstack([pa, pb, off])
    add("tie", tie, [0, 0], min_inliers=24, num_iterations=2, max_planes=2,
        rand3=np.vstack([H.words_for([[30, 35, 58], [0, 5, 28]], 80), H.words_for([[0, 5, 28], [1, 4, 29]], 50)]))
    # code 4: the hypothesis plane z = 0 counts all 11 points, the refitted plane (horizontal, at 0.54 x thickness) only 10
    th = 0.01
    ang3, ang7 = 2 * np.pi * np.arange(3) / 3, 2 * np.pi * (np.arange(7) + 0.25) / 7
    c4 = np.vstack([np.column_stack([np.cos(ang3), np.sin(ang3), np.zeros(3)]),
                    np.column_stack([0.5 * np.cos(ang7), 0.5 * np.sin(ang7), np.full(7, 0.99 * th)]), [[0.0, 0.0, -0.99 * th]]])
    add("code4", c4 + np.array([0.0, 0.0, 4.0]), [4], thickness=th, min_inliers=11, num_iterations=1, max_planes=1,
        rand3=H.words_for([[0, 1, 2]], 11))
    return cases


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """the oracle's result for edge_cases()[name], computed once per process and shared: callers must not change it"""
    return oracle_case(edge_cases()[name])


def oracle_case(case):
    return oracle(case["P"], case["pose7"], **case["kw"])
