"""Local-BA problems shaped like the ones the map layer builds (Slam::local_ba, slam/mapper.cpp), shared by test_oracle_vs_ref.py (the
restatement against Ceres), test_gpu_ba.py (ba.hip against both) and test_ba_cases.py (the table's own checks).

synth.make_ba_problem makes ONE shape: the anchor of every point is its lowest observing slot (observer > anchor in every residual block,
so only one triangle of the pair sums M[observer][anchor] is ever filled), the constant keyframes are slots 0 and 1 (cidx[k] = k - 2), and
no point has more than a few tens of residual blocks.  The mapper fills pose slots from the newest keyframe down (anchor = the HIGHER slot),
scatters its constants and accepts 64 keyframes.  The transforms below turn the synth problems into that shape; make_ring_problem gives what
the fixed camera path of synth cannot: many keyframes that all see the scene.

Every case names the properties it exists for; case() asserts them -- with numpy and the CPU oracle, never with the kernel -- whenever the
case is built, so a case cannot silently stop covering its branch.

What the CPU oracle sees in each case (test_ba_cases.py -s prints these lines): keyframes, free keyframes, residual blocks, blocks with
observer < anchor / observer > anchor, distinct (observer, anchor) pairs with both free below / above the diagonal, most blocks of one point,
blocks with chi2 > 5.9915 and blocks behind their camera at the oracle's result, summaries / accepted steps:

  case                           kf  free  blocks  obs<anc  obs>anc  free pairs  max/pt   Huber-active  behind summaries / accepted
  reversed_c3_11_19              20    17    7552     7552        0   136 /   0      19    187   2.5 %       0     6 / 6
  reversed_c0_7_8_19_outliers    20    16    7552     7552        0   120 /   0      19   1250  16.6 %       0     6 / 6
  permuted_outliers              20    17    7552      953     6599    61 /  75      19    813  10.8 %       0     6 / 6
  permuted_ftol                  14    12    4630     2514     2116    23 /  43      13     86   1.9 %       0     3 / 3
  rejected_reversed               6     4     522      522        0     6 /   0       5     13   2.5 %       1     6 / 3
  rejected_permuted               6     4     522      308      214     4 /   2       5     13   2.5 %       1     6 / 3
  behind_outliers                12    10    1824     1822        2    45 /   1      11     86   4.7 %       6     6 / 6
  free8                          10     8    1770     1770        0    28 /   0       9     60   3.4 %       0     6 / 6
  free16                         18    16    5639     1808     3831    49 /  71      17    336   6.0 %       0     6 / 6
  free21                         23    21    8550     8550        0   210 /   0      22    270   3.2 %       0     6 / 6
  free22                         24    22    9038     9038        0   226 /   0      23    322   3.6 %       0     6 / 6
  free1                           6     1     719      719        0     0 /   0       5    310  43.1 %       0     6 / 6
  free0                           6     0     673      673        0     0 /   0       5    342  50.8 %       0     6 / 6
  ring64                         64    62    5910     5910        0   568 /   0      63    181   3.1 %       0     6 / 6
  ring70                         70    68    4608     4608        0   620 /   0      69    147   3.2 %       0     6 / 6
  ring128                       128   126    3632     3632        0   646 /   0     127      0   0.0 %       0     6 / 6
  xyz_reversed                   12    10    3363     3039        0    45 /   0      12     88   2.6 %       0     6 / 6
  xyz_permuted_outliers           9     6    1599     1341       57     8 /   7       9    424  26.5 %       0     6 / 6

Tolerances: ba_compare's bars (poses 1e-8, inverse depth 1e-7, XYZ 1e-6, costs 1e-8 relative, counts / flags / chi2 classes exact) for
every case.  No case has needed a bar of its own and no seed has been discarded (DISCARDED_SEEDS)."""
import functools

import numpy as np

from alvaar_amd import synth
from alvaar_amd.synth import pose7, quat_xyzw_to_rot, se3_exp

CHI2 = 5.9915
# seeds replaced because the restatement and Ceres disagreed on a count or a chi2 class (a decision on a rounding edge): case family -> seeds
DISCARDED_SEEDS = {}


# ---- transforms (all return a new dict; the arrays of the input are never written) -----------------------------------------------------
def relabel(pb, perm):
    """Renumber the keyframe slots: old slot k becomes perm[k].  Which observation of a point is its anchor does not change."""
    perm = np.asarray(perm, np.int32)
    n = len(pb["poses"])
    assert sorted(perm.tolist()) == list(range(n))
    old_of_new = np.argsort(perm)
    out = dict(pb)
    for key in ("poses", "poses_gt", "kf_const"):
        if key in pb:
            out[key] = np.ascontiguousarray(pb[key][old_of_new])
    out["anchor_kf"] = perm[pb["anchor_kf"]].astype(np.int32)
    out["obs_kf"] = perm[pb["obs_kf"]].astype(np.int32)
    return out


def reverse(pb):
    """The mapper's order: slots run from the newest keyframe down, so a point's anchor (its oldest observer) has the HIGHEST slot."""
    n = len(pb["poses"])
    return relabel(pb, np.arange(n - 1, -1, -1))


def permute(pb, seed):
    return relabel(pb, np.random.RandomState(seed).permutation(len(pb["poses"])))


def set_constants(pb, slots):
    out = dict(pb)
    kfc = np.zeros(len(pb["poses"]), np.uint8)
    kfc[list(slots)] = 1
    out["kf_const"] = kfc
    return out


def add_outliers(pb, frac, lo=4.0, hi=9.0, seed=0):
    """Shift a share `frac` of the observations by lo .. hi pixels per axis, random signs."""
    rng = np.random.RandomState(seed)
    n = len(pb["obs_kf"])
    idx = rng.choice(n, max(1, int(round(frac * n))), replace=False)
    uv = np.array(pb["obs_uv"], float)
    uv[idx] += rng.uniform(lo, hi, (len(idx), 2)) * rng.choice([-1.0, 1.0], (len(idx), 2))
    return dict(pb, obs_uv=uv)


def as_xyz(pb):
    """XYZ mode has a residual for EVERY observation (no anchor): the anchor observations come back as residual blocks."""
    n = len(pb["anchor_kf"])
    out = dict(pb)
    out["obs_kf"] = np.concatenate([pb["anchor_kf"], pb["obs_kf"]]).astype(np.int32)
    out["obs_pt"] = np.concatenate([np.arange(n, dtype=np.int32), pb["obs_pt"]]).astype(np.int32)
    out["obs_uv"] = np.concatenate([pb["anchor_uv"], pb["obs_uv"]])
    return out


def make_ring_problem(n_kf, n_pt, seed, every=7, arc=(3, 12), n_outside=0, radius=6.0, px_noise=0.5, pose_noise=0.005, invdepth_noise=0.02,
                      fx=579.4, fy=579.4, cx=320.0, cy=240.0):
    """Cameras on a closed loop around a small scene, all looking at its centre: every camera can see every point.  Every `every`-th
    point is observed by ALL cameras (n_kf - 1 residual blocks), the others by an arc of arc[0] .. arc[1] neighbouring cameras that may
    wrap around the loop's end.  The anchor is the HIGHEST observing slot.  `n_outside` more points lie outside the loop, each BEHIND one
    camera that observes it all the same (depth flag 0, small chi2).  Same keys as synth.make_ba_problem."""
    rng = np.random.RandomState(seed)
    K = np.array([fx, fy, cx, cy])
    Rs, ts = [], []
    for k in range(n_kf):
        th = 2.0 * np.pi * k / n_kf
        c = np.array([radius * np.sin(th), 0.4 * np.sin(3.0 * th), -radius * np.cos(th)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        Rs.append(np.stack([x, np.cross(z, x), z], 1))   # X_w = R X_c + t
        ts.append(c)
    pts = rng.uniform(-1.2, 1.2, (n_pt, 3))
    views = []
    for p in range(n_pt):
        if p % every == 0:
            views.append((np.arange(n_kf), None))
        else:
            views.append((np.unique((rng.randint(n_kf) + np.arange(rng.randint(arc[0], arc[1] + 1))) % n_kf), None))
    for _ in range(n_outside):
        # a point OUTSIDE the loop, about two metres behind camera j: seen from the far side of the loop, and matched -- wrongly -- in camera
        # j at the pixel it would have there if it lay in front (the projection does not change when the camera-frame point changes sign)
        j = rng.randint(n_kf)
        th = 2.0 * np.pi * j / n_kf
        X = np.array([(radius + 2.0) * np.sin(th), 0.0, -(radius + 2.0) * np.cos(th)]) + rng.uniform(-0.2, 0.2, 3)
        front = []
        for k in range(n_kf):
            pc = Rs[k].T @ (X - ts[k])
            if pc[2] > 0.5 and abs(fx * pc[0] / pc[2]) < cx - 1 and abs(fy * pc[1] / pc[2]) < cy - 1:
                front.append(k)
        assert len(front) >= 3 and (Rs[j].T @ (X - ts[j]))[2] < -0.5
        views.append((np.sort(rng.choice(front, min(len(front), 8), replace=False)), j))
        pts = np.vstack([pts, X])
    n_pt = len(pts)
    poses_gt = np.stack([pose7(R, t) for R, t in zip(Rs, ts)])
    poses = poses_gt.copy()
    for k in range(n_kf):
        Rn, tn = se3_exp(rng.normal(0, pose_noise, 6))
        poses[k] = pose7(Rn @ Rs[k], Rn @ ts[k] + tn)
    anchor_kf = np.zeros(n_pt, np.int32)
    anchor_uv = np.zeros((n_pt, 2))
    rho = np.zeros(n_pt)
    pts_xyz = np.zeros((n_pt, 3))
    obs_kf, obs_pt, obs_uv = [], [], []
    for p, (seen, wrong) in enumerate(views):
        a = int(seen.max())
        for k in list(seen) + ([wrong] if wrong is not None else []):
            pc = Rs[k].T @ (pts[p] - ts[k])
            uv = np.array([fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy])
            if k != wrong:
                assert pc[2] > 0.5 and 0 <= uv[0] < 2 * cx and 0 <= uv[1] < 2 * cy
            uv += rng.normal(0, px_noise, 2)
            if k == a:
                anchor_kf[p], anchor_uv[p] = a, uv
                rho[p] = (1.0 / pc[2]) * (1.0 + rng.normal(0, invdepth_noise))
            else:
                obs_kf.append(k)
                obs_pt.append(p)
                obs_uv.append(uv)
        pa = np.array([(anchor_uv[p, 0] - cx) / fx, (anchor_uv[p, 1] - cy) / fy, 1.0]) / rho[p]
        pts_xyz[p] = quat_xyzw_to_rot(poses[a, 3:]) @ pa + poses[a, :3]
    kfc = np.zeros(n_kf, np.uint8)
    return dict(poses=poses, poses_gt=poses_gt, kf_const=kfc, calib=K, anchor_kf=anchor_kf, anchor_uv=anchor_uv, inv_depth=rho, pts_xyz=pts_xyz,
                pts_gt=pts, obs_kf=np.asarray(obs_kf, np.int32), obs_pt=np.asarray(obs_pt, np.int32), obs_uv=np.asarray(obs_uv, float).reshape(-1, 2))


# ---- the properties, from the problem alone ... ----------------------------------------------------------------------------------------
def shape(pb):
    okf, akf = np.asarray(pb["obs_kf"]), np.asarray(pb["anchor_kf"])[np.asarray(pb["obs_pt"])]
    free = np.asarray(pb["kf_const"]) == 0
    both = free[okf] & free[akf]
    pairs = set(zip(okf[both].tolist(), akf[both].tolist()))
    n = max(len(okf), 1)
    per_pt = np.bincount(np.asarray(pb["obs_pt"]), minlength=len(pb["anchor_kf"])) if len(okf) else np.zeros(1, int)
    return dict(blocks=len(okf), below=int((okf < akf).sum()), above=int((okf > akf).sum()), share_below=float((okf < akf).sum()) / n,
                share_above=float((okf > akf).sum()) / n, free_pairs_below=sum(o < a for o, a in pairs), free_pairs_above=sum(o > a for o, a in pairs),
                n_free=int(free.sum()), n_kf=len(free), max_blocks=int(per_pt.max()) if len(per_pt) else 0)


def _check(name, prop, pb, orc):
    """One property of the table in the issue's wording; `orc` = the CPU oracle's result for the case."""
    s = shape(pb)
    kfc = np.asarray(pb["kf_const"]).astype(bool)
    akf = np.asarray(pb["anchor_kf"])
    nobs = max(s["blocks"], 1)
    if prop == "reversed":               # the mapper's order: observer < anchor in 100 % of the blocks
        assert s["below"] == s["blocks"] > 0, (name, s)
    elif prop == "both_triangles":       # >= 10 % of the blocks on either side of the diagonal
        assert s["share_below"] >= 0.10 and s["share_above"] >= 0.10, (name, s)
    elif prop == "free_pairs_below":     # >= 20 distinct (observer, anchor) pairs with both keyframes free, observer < anchor
        assert s["free_pairs_below"] >= 20, (name, s)
    elif prop == "free_pairs_both":      # ... on either side of the diagonal
        assert s["free_pairs_below"] >= 20 and s["free_pairs_above"] >= 20, (name, s)
    elif prop == "scattered_constants":  # not a prefix; some constant slot is an anchor; some free slot is an anchor
        nconst = int(kfc.sum())
        assert nconst > 0 and not kfc[:nconst].all(), name
        assert kfc[akf].any() and (~kfc[akf]).any(), name
    elif prop == "huber":                # 2 % .. 30 % of the blocks beyond the Huber threshold at the oracle's result
        share = float((orc["chi2"] > CHI2).sum()) / nobs
        assert 0.02 <= share <= 0.30, (name, share)
    elif prop == "depth_flag":           # >= 3 blocks behind their camera at the oracle's result
        assert int((orc["depth"] == 0).sum()) >= 3, name
    elif prop == "rejected_step":
        assert orc["info"][3] < orc["info"][0], (name, orc["info"])
    elif prop == "long_point":           # the observation loop of k_point runs twice; the free-camera map leaves the LDS
        assert s["max_blocks"] >= 65 and s["n_free"] > 64, (name, s)
    elif prop.startswith("free="):
        assert s["n_free"] == int(prop[5:]), (name, s)
    elif prop.startswith("n_kf="):
        assert s["n_kf"] == int(prop[5:]), (name, s)
    else:
        raise KeyError(prop)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
# (6, 150, 4) at these noise levels is the rejected-step recipe of test_gpu_ba.py
_REJ = dict(pose_noise=0.1, invdepth_noise=0.3)


def _synth(nkf, npt, seed, **kw):
    return synth.make_ba_problem(nkf, npt, seed, **kw)


# name -> (builder, inv_depth, iters, ftol, properties)
_TABLE = {
    # the mapper's order on the suite's 20-keyframe row; constants scattered, one of them the last slot (= the anchors' favourite)
    "reversed_c3_11_19": (lambda: set_constants(reverse(_synth(20, 600, 42)), (3, 11, 19)), True, 5, 0.0,
                          ("reversed", "free_pairs_below", "scattered_constants", "free=17")),
    "reversed_c0_7_8_19_outliers": (lambda: add_outliers(set_constants(reverse(_synth(20, 600, 42)), (0, 7, 8, 19)), 0.05, seed=1), True, 5, 0.0,
                                    ("reversed", "free_pairs_below", "scattered_constants", "huber", "free=16")),
    # both triangles of M in one problem
    "permuted_outliers": (lambda: add_outliers(set_constants(permute(_synth(20, 600, 42), 7), (2, 9, 17)), 0.05, seed=2), True, 5, 0.0,
                          ("both_triangles", "free_pairs_both", "scattered_constants", "huber", "free=17")),
    "permuted_ftol": (lambda: set_constants(permute(_synth(14, 500, 11), 3), (5, 13)), True, 5, 1e-3,
                      ("both_triangles", "free_pairs_both", "scattered_constants", "free=12")),
    # a rejected step with the anchors on the other side
    "rejected_reversed": (lambda: reverse(_synth(6, 150, 4, **_REJ)), True, 5, 0.0, ("reversed", "rejected_step", "free=4")),
    "rejected_permuted": (lambda: relabel(_synth(6, 150, 4, **_REJ), (3, 0, 5, 1, 4, 2)), True, 5, 0.0,
                          ("scattered_constants", "rejected_step", "free=4")),
    # blocks that end behind their camera, among outliers
    "behind_outliers": (lambda: add_outliers(set_constants(make_ring_problem(12, 250, 8, n_outside=6), (1, 11)), 0.04, seed=3), True, 5, 0.0,
                        ("scattered_constants", "free_pairs_below", "huber", "depth_flag", "free=10")),
    # the edges of the reduced system's padding and of k_solve's LDS / device-memory switch (21 free in LDS, 22 the first outside)
    "free8": (lambda: set_constants(reverse(_synth(10, 300, 21)), (2, 9)), True, 5, 0.0, ("reversed", "free_pairs_below", "scattered_constants", "free=8")),
    "free16": (lambda: set_constants(permute(_synth(18, 500, 22), 5), (4, 16)), True, 5, 0.0, ("both_triangles", "free_pairs_both", "scattered_constants", "free=16")),
    "free21": (lambda: add_outliers(set_constants(reverse(_synth(23, 600, 23)), (6, 22)), 0.03, seed=4), True, 5, 0.0,
               ("reversed", "free_pairs_below", "scattered_constants", "huber", "free=21")),
    "free22": (lambda: add_outliers(set_constants(reverse(_synth(24, 600, 24)), (6, 23)), 0.03, seed=5), True, 5, 0.0,
               ("reversed", "free_pairs_below", "scattered_constants", "huber", "free=22")),
    "free1": (lambda: set_constants(reverse(_synth(6, 200, 25)), (0, 1, 3, 4, 5)), True, 5, 0.0, ("reversed", "free=1")),
    "free0": (lambda: set_constants(reverse(_synth(6, 200, 26)), range(6)), True, 5, 0.0, ("free=0",)),
    # many keyframes that all see the scene: the mapper's largest window, and more free cameras / blocks per point than one wave has lanes
    "ring64": (lambda: add_outliers(set_constants(make_ring_problem(64, 400, 31), (5, 40)), 0.03, seed=6), True, 5, 0.0,
               ("reversed", "free_pairs_below", "scattered_constants", "huber", "free=62", "n_kf=64")),
    "ring70": (lambda: add_outliers(set_constants(make_ring_problem(70, 300, 32), (0, 33)), 0.03, seed=7), True, 5, 0.0,
               ("reversed", "free_pairs_below", "scattered_constants", "huber", "long_point", "free=68")),
    # the largest problem the C ABI takes (ALVA_LOCAL_BA_MAX_KF keyframes)
    "ring128": (lambda: set_constants(make_ring_problem(128, 150, 33), (17, 90)), True, 5, 0.0,
                ("reversed", "free_pairs_below", "scattered_constants", "long_point", "free=126", "n_kf=128")),
    # the XYZ kernels (DP = 3) on relabelled slots and scattered constants
    "xyz_reversed": (lambda: as_xyz(set_constants(reverse(_synth(12, 400, 6)), (4, 11))), False, 5, 0.0, ("scattered_constants", "free=10")),
    "xyz_permuted_outliers": (lambda: add_outliers(as_xyz(set_constants(permute(_synth(9, 250, 5), 9), (0, 3, 8))), 0.05, seed=8), False, 5, 0.0,
                              ("scattered_constants", "huber", "free=6")),
}
CASE_NAMES = list(_TABLE)
INV_NAMES = [n for n in CASE_NAMES if _TABLE[n][1]]
XYZ_NAMES = [n for n in CASE_NAMES if not _TABLE[n][1]]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(name, pb, inv_depth, iters, ftol, props, pt_tol, orc): the problem, how it is solved, what it covers, and the CPU oracle's
    result for it (read-only: shared between tests).  Asserts the case's properties."""
    from oracles import Orc
    build, inv, iters, ftol, props = _TABLE[name]
    pb = build()
    orc = Orc.local_ba(pb, iters, ftol, inv_depth=inv)
    assert orc["ok"], name
    for prop in props:
        _check(name, prop, pb, orc)
    return dict(name=name, pb=pb, inv_depth=inv, iters=iters, ftol=ftol, props=props, pt_tol=1e-7 if inv else 1e-6, orc=orc)


def describe(name):
    """One line of oracle-side numbers for a case (printed by test_ba_cases.py -s)."""
    c = case(name)
    s, o = shape(c["pb"]), c["orc"]
    return ("%-28s kf %3d free %3d blocks %6d  observer<anchor %6d  >anchor %6d  free pairs %4d / %4d  max blocks/pt %3d  huber %5d (%.1f %%)  behind %3d  "
            "summaries %d accepted %d") % (name, s["n_kf"], s["n_free"], s["blocks"], s["below"], s["above"], s["free_pairs_below"], s["free_pairs_above"],
                                           s["max_blocks"], int((o["chi2"] > CHI2).sum()), 100.0 * (o["chi2"] > CHI2).sum() / max(s["blocks"], 1),
                                           int((o["depth"] == 0).sum()), int(o["info"][0]), int(o["info"][3]))


# ---- degenerate sizes the C ABI accepts ----------------------------------------------------------------------------------------------
def degenerate(kind):
    pb = set_constants(reverse(_synth(5, 60, 40)), (0, 4))
    if kind == "n_obs=0":
        return dict(pb, obs_kf=np.zeros(0, np.int32), obs_pt=np.zeros(0, np.int32), obs_uv=np.zeros((0, 2)))
    if kind == "n_pt=0":
        return dict(pb, obs_kf=np.zeros(0, np.int32), obs_pt=np.zeros(0, np.int32), obs_uv=np.zeros((0, 2)), anchor_kf=np.zeros(0, np.int32),
                    anchor_uv=np.zeros((0, 2)), inv_depth=np.zeros(0), pts_xyz=np.zeros((0, 3)))
    if kind == "free_kf_without_blocks":   # slot 2 observes nothing and anchors nothing, and is free
        keep = (pb["obs_kf"] != 2) & (pb["anchor_kf"][pb["obs_pt"]] != 2)
        used = np.zeros(len(pb["anchor_kf"]), bool)
        used[pb["obs_pt"][keep]] = True
        used &= pb["anchor_kf"] != 2
        keep &= used[pb["obs_pt"]]
        remap = np.cumsum(used) - 1
        return dict(pb, obs_kf=pb["obs_kf"][keep], obs_pt=remap[pb["obs_pt"][keep]].astype(np.int32), obs_uv=pb["obs_uv"][keep],
                    anchor_kf=pb["anchor_kf"][used], anchor_uv=pb["anchor_uv"][used], inv_depth=pb["inv_depth"][used], pts_xyz=pb["pts_xyz"][used])
    raise KeyError(kind)


DEGENERATE = ["n_obs=0", "n_pt=0", "free_kf_without_blocks"]
