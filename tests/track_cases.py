"""The plane tracker's definition (include/alvaar_hip.h, alva_track_planes: T0 to T6) restated in numpy, line for line, and the scenes the
tests run it on.  The reference tracks no planes, so this file is what alva_track_planes is pinned to (tests/test_track_cases.py checks
the restatement itself, tests/test_gpu_track_planes.py the kernel against it).  T6 -- the new planes among the unclaimed points -- is
plane_cases.oracle, unchanged, on those points.

All decisions are taken in float64 in the written operation order, as in plane_cases; the eigenvectors come from numpy.linalg.eigh where
the kernel runs a cyclic Jacobi.  The margins that keep every decision away from the last bits:
  thr_margin   plane_cases' | |d| / thickness - 1 |, over both claim passes (every point against every plane of the pass) and over T6's
               rounds
  tie_margin   over the points that lie inside the slabs of two or more planes of a pass, (second smallest |d| - smallest |d|) /
               thickness: which of the planes takes the point.  Kept separately for T1 (tie_margin_t1) and T4 (tie_margin_t4); inf when
               no point lies in two slabs
  guards       plane_cases' five (eig_ratio, axis_ratio, sign_margin, ref_margin, face_margin), per kept plane: tracked ones first, in
               slot order, then T6's
Every case a GPU test compares must have thr_margin >= MARGIN_MIN, both tie margins >= MARGIN_MIN (exact_tie's T1 margin is 0 by
construction: every number in it is dyadic, both sides compute the same bits and the lower slot wins) and the guards."""
from __future__ import annotations

import functools

import numpy as np

import hit_cases as H
import plane_cases as C

MARGIN_MIN = C.MARGIN_MIN
POSE_ORIGIN = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


def _claim(P, planes, thickness):
    """T1 / T4: planes = [(j, c, n)] -> (assignment [n] = j or -1, counts {j: size}, thr margin, tie margin)"""
    n = len(P)
    assign = np.full(n, -1, np.int64)
    best = np.full(n, np.inf)
    second = np.full(n, np.inf)   # the second smallest |d| among the planes whose slab holds the point
    thr = np.inf
    for j, c, nrm in planes:      # ascending j: a strict < keeps the lowest j on ties
        X = P - c
        d = np.abs((X[:, 0] * nrm[0] + X[:, 1] * nrm[1]) + X[:, 2] * nrm[2])
        thr = min(thr, C._margin(d, thickness))
        inside = d <= thickness
        better = inside & (d < best)
        second = np.where(better, best, np.where(inside, np.minimum(second, d), second))
        assign[better] = j
        best = np.where(better, d, best)
    two = np.isfinite(second)
    tie = float(((second[two] - best[two]) / thickness).min()) if two.any() else np.inf
    return assign, {j: int((assign == j).sum()) for j, _, _ in planes}, thr, tie


def oracle_track(P, pose7, prior24, thickness, min_inliers=48, max_planes=4, num_iterations=128, seed=12345, rand3=None):
    """Returns plane_cases.oracle's dict (info, planes, moments, moment_scale, labels, found, thr_margin, guards) with tie_margin_t1,
    tie_margin_t4 and `unclaimed` (the indices T6 ran on)."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    pose7 = np.asarray(pose7, np.float64)
    t, R = pose7[:3], H.quat_to_rot(pose7[3:])
    thickness = np.float64(thickness)
    prior = np.zeros((0, 24), np.float32) if prior24 is None else np.asarray(prior24, np.float32).reshape(-1, 24)
    n, n_prior = len(P), len(prior)
    assert n_prior <= max_planes
    info = np.tile(np.array(C.NOT_RUN, np.int32), (max_planes, 1))
    planes = np.zeros((max_planes, 24), np.float32)
    moments, scale = np.zeros((max_planes, 10)), np.zeros((max_planes, 10))
    labels = np.full(n, -1, np.int32)
    out = dict(info=info, planes=planes, moments=moments, moment_scale=scale, labels=labels, found=0, thr_margin=np.inf,
               tie_margin_t1=np.inf, tie_margin_t4=np.inf, guards=[], unclaimed=np.arange(n))
    # T0
    usable = [bool(np.isfinite(rec).all() and rec[15] == 1) for rec in prior]
    for j in range(n_prior):
        info[j] = [7 if usable[j] else 9, n, -1, 0, 0, 1, 0, 0]
    if n == 0:   # nothing is launched
        if n_prior < max_planes:
            info[n_prior] = [1, 0, -1, 0, 0, 0, 0, 0]
        return out
    # T1
    pl = [(j, prior[j, 12:15].astype(np.float64), prior[j, 4:7].astype(np.float64)) for j in range(n_prior) if usable[j]]
    assign, claimed, thr, out["tie_margin_t1"] = _claim(P, pl, thickness)
    out["thr_margin"] = min(out["thr_margin"], thr)
    refit = []
    fits = {}
    for j, c, _ in pl:
        info[j, 3] = claimed[j]
        # T2
        if claimed[j] < min_inliers:
            continue
        # T3: plane_cases.oracle's step 4 with Q0 = c_j
        X = P[assign == j] - c
        terms = [np.ones(len(X)), X[:, 0], X[:, 1], X[:, 2], X[:, 0] * X[:, 0], X[:, 0] * X[:, 1], X[:, 0] * X[:, 2], X[:, 1] * X[:, 1],
                 X[:, 1] * X[:, 2], X[:, 2] * X[:, 2]]
        mom = np.array([v.sum() for v in terms])
        moments[j], scale[j] = mom, np.array([np.abs(v).sum() for v in terms])
        inv = 1.0 / np.float64(claimed[j])
        mu = mom[1:4] * inv
        S = np.array([[mom[4] * inv - mu[0] * mu[0], mom[5] * inv - mu[0] * mu[1], mom[6] * inv - mu[0] * mu[2]],
                      [0, mom[7] * inv - mu[1] * mu[1], mom[8] * inv - mu[1] * mu[2]], [0, 0, mom[9] * inv - mu[2] * mu[2]]])
        S = S + np.triu(S, 1).T
        lam, V = np.linalg.eigh(S)
        c2 = c + mu
        nrm = V[:, 0] / np.linalg.norm(V[:, 0])
        facing = nrm @ (t - c2)
        if not facing > 0:
            nrm = -nrm
        refit.append((j, c2, nrm))
        fits[j] = (lam, V, facing)
    # T4
    assign, inliers, thr, out["tie_margin_t4"] = _claim(P, refit, thickness)
    out["thr_margin"] = min(out["thr_margin"], thr)
    for j, c2, nrm in refit:
        info[j, 4] = inliers[j]
        if inliers[j] < min_inliers:
            info[j, 0] = 8
            continue
        # T5: plane_cases.oracle's steps 6 and 7 over the T4 set
        lam, V, facing = fits[j]
        F = assign == j
        labels[F] = j
        an = R[0, 0] * nrm[0] + R[1, 0] * nrm[1] + R[2, 0] * nrm[2]
        a = R[:, 1] if abs(an) > C.AXIS_SWITCH else R[:, 0]
        x = V[:, 2] - (V[:, 2] @ nrm) * nrm
        x = x / np.linalg.norm(x)
        if x @ a < 0:
            x = -x
        z = np.cross(x, nrm)
        ex, ez = C._dist(P[F] - c2, x), C._dist(P[F] - c2, z)
        lo_x, hi_x, lo_z, hi_z = ex.min(), ex.max(), ez.min(), ez.max()
        p = c2 + ((lo_x + hi_x) / 2) * x + ((lo_z + hi_z) / 2) * z
        planes[j, 0:3], planes[j, 4:7], planes[j, 8:11], planes[j, 12:15], planes[j, 15] = x, nrm, z, p, 1.0
        planes[j, 16], planes[j, 17], planes[j, 18] = hi_x - lo_x, hi_z - lo_z, nrm @ p
        info[j, 0] = 0
        out["found"] += 1
        out["guards"].append(dict(eig_ratio=float(lam[1] / lam[0]) if lam[0] > 0 else np.inf,
                                  axis_ratio=float(lam[2] / lam[1]) if lam[1] > 0 else np.inf, sign_margin=float(abs(x @ a)),
                                  ref_margin=float(abs(abs(an) - C.AXIS_SWITCH)), face_margin=float(abs(facing) / np.linalg.norm(t - c2)),
                                  normal=nrm, centre=p, x=x, slot=j))
    # T6: detection, unchanged, on the unclaimed points; its round r is slot n_prior + r
    live = np.nonzero(labels == -1)[0]
    out["unclaimed"] = live
    rounds = max_planes - n_prior
    if rounds > 0:
        d = C.oracle(P[live], pose7, thickness, min_inliers, rounds, num_iterations, seed, rand3)
        info[n_prior:], planes[n_prior:], moments[n_prior:], scale[n_prior:] = d["info"], d["planes"], d["moments"], d["moment_scale"]
        got = d["labels"] >= 0
        labels[live[got]] = d["labels"][got] + n_prior
        out["thr_margin"] = min(out["thr_margin"], d["thr_margin"])
        out["found"] += int((d["info"][:, 0] == 0).sum())
        out["guards"] += [dict(g, slot=n_prior + k) for k, g in enumerate(d["guards"])]
    return out


def margins_ok(res, t1_exact_tie=False) -> bool:
    t1 = res["tie_margin_t1"] == 0 if t1_exact_tie else res["tie_margin_t1"] >= MARGIN_MIN
    return bool(t1 and res["tie_margin_t4"] >= MARGIN_MIN and C.margins_ok(res))


def margins_text(res) -> str:
    return "tie T1 %.1e T4 %.1e | " % (res["tie_margin_t1"], res["tie_margin_t4"]) + C.margins_text(res)


# ---------------------------------------------------------------------------------------------------- scenes
def grid(z):
    """48 points: np.arange(-4, 4) / 2 x np.arange(-3, 3) / 2 at height z"""
    gx, gy = np.meshgrid(np.arange(-4, 4) / 2.0, np.arange(-3, 3) / 2.0)
    return np.column_stack([gx.ravel(), gy.ravel(), np.full(gx.size, float(z))])


def flat_prior(z):
    """the record of the plane at height z that faces a camera below it: long axis x, normal (0, 0, -1), short axis z = x cross n = (0, 1, 0)"""
    rec = np.zeros(24, np.float32)
    rec[0], rec[6], rec[9], rec[14], rec[15] = 1, -1, 1, z, 1
    rec[16], rec[17], rec[18] = 3.5, 2.5, -z
    return rec


def kept(res):
    """the records of a result's code-0 slots, in slot order: the next call's priors"""
    return res["planes"][res["info"][:, 0] == 0].copy()


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(P, pose7, prior, kw, want = the codes per slot, t1_exact_tie)"""
    out = {}

    def add(name, P, prior, want, pose7=H.POSE_BASE, t1_exact_tie=False, **kw):
        out[name] = dict(P=np.ascontiguousarray(P, np.float64).reshape(-1, 3), pose7=np.asarray(pose7, np.float64),
                         prior=np.ascontiguousarray(prior, np.float32).reshape(-1, 24), kw=kw, want=want, t1_exact_tie=t1_exact_tie)

    base = C.edge_cases()["base"]
    P, det = base["P"], C.oracle_of("base")
    two = det["planes"][:2].copy()
    add("self_base", P, two, [0, 0, 3, 5], **C.BASE_KW)
    add("full_slots", P, two, [0, 0], **dict(C.BASE_KW, max_planes=2))
    rot = C.edge_cases()["rotated"]
    add("rotated", P, C.oracle_of("rotated")["planes"][:2].copy(), [0, 0, 3, 5], pose7=rot["pose7"], **C.BASE_KW)
    add("swapped", P, two[::-1].copy(), [0, 0, 3, 5], **C.BASE_KW)
    # grow: the floor as detected on the half of the scene with x below the median, then the whole scene
    half = P[P[:, 0] < np.median(P[:, 0])]
    assert len(half) == 1400
    first = C.oracle(half, H.POSE_BASE, seed=1, **C.BASE_KW)
    assert first["info"][:, 0].tolist()[:2] == [0, 3] and C.margins_ok(first), first["info"][:, 0]
    add("grow", P, first["planes"][:1].copy(), [0, 0, 3, 5], **C.BASE_KW)
    add("lost", P[det["labels"] != 1], two, [0, 7, 3, 5], **C.BASE_KW)
    zeroed = two.copy()
    zeroed[0] = 0
    add("unusable", P, zeroed, [9, 0, 0, 3], **C.BASE_KW)
    c4 = C.edge_cases()["code4"]
    add("code8", c4["P"], flat_prior(4.0), [8, 4], pose7=c4["pose7"], thickness=c4["kw"]["thickness"], min_inliers=11, max_planes=2,
        num_iterations=1, rand3=c4["kw"]["rand3"])
    add("exact_tie", np.vstack([grid(4), grid(4.125), grid(4.25)]), np.stack([flat_prior(4.0), flat_prior(4.25)]), [0, 0], pose7=POSE_ORIGIN,
        t1_exact_tie=True, thickness=5 / 32, min_inliers=48, max_planes=2, num_iterations=8)
    add("stack8", np.vstack([grid(4 + k / 4) for k in range(8)]), np.stack([flat_prior(4 + k / 4) for k in range(8)]), [0] * 8,
        pose7=POSE_ORIGIN, thickness=1 / 16, min_inliers=48, max_planes=8, num_iterations=8)
    add("all_claimed", grid(4), flat_prior(4.0), [0, 1], pose7=POSE_ORIGIN, thickness=1 / 16, min_inliers=48, max_planes=2, num_iterations=8)
    add("n0", np.zeros((0, 3)), two, [7, 7, 1, 5], **C.BASE_KW)
    for name in ["n%d" % n for n in (63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 16384)]:
        e = C.edge_cases()[name]
        add(name, e["P"], C.oracle_of(name)["planes"][:1].copy(), [0, 1], pose7=e["pose7"], **e["kw"])
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """the restatement's result for cases()[name], computed once per process and shared: callers must not change it"""
    case = cases()[name]
    return oracle_track(case["P"], case["pose7"], case["prior"], **case["kw"])
