"""The PnP refinement's branch table: named problems, each chosen because the minimiser of alva_pnp_refine / k_pnp (Ceres' trust-region
loop restated, csrc/pnp.hip) leaves the one path the other PnP tests take -- every step accepted, 3 + 2 summaries, function tolerance.

A case is generator arguments, not data: synth.make_pnp_problem(**gen), then `mods`, then the start pose.  `start = (w, seed)` replaces
the generator's start pose by the ground truth moved by a rotation vector ~ N(0, w) and a translation ~ N(0, 3 w) (RandomState(seed));
`None` keeps the generator's.  `sig` is the path the plain-C checker takes
(oracle/alva_oracle.c, orc_pnp_refine_trace), written "<solve 1> | <solve 2>" with one letter per minimiser decision -- A accepted,
R rejected, I invalid, T the candidate on which a tolerance ended the solve -- and the exit reason; `branch` names the predicate of
BRANCHES the case exists for.  tests/test_pnp_cases.py checks both on the CPU and, where the compiled reference is built, that Ceres
itself takes the same path; tests/test_gpu_pose.py runs the kernel over the table.

Branches the search did not reach.  A bounded search on the CPU checker -- 13 824 perturbed starts of the ordinary generator (n = 37 / 130 /
300 / 513, 0-45 % outliers, w = 0.3 ... 2.0, max_iters 5 / 10 / 20) and 55 296 solves of deliberately ill-conditioned but finite problems
(all world points equal, collinear points, coordinates scaled by 1e-6 / 1e6 / 1e12, a point 1e-7 in front of the start camera, half the
points 1e8 away; robust and plain, up to 60 iterations) -- found NO invalid step (Cholesky failure or model cost change <= 0), hence
neither "an invalid step" nor "five invalid steps -> failure", and no exit through the radius floor.  Mathematically the model cost
change of a damped normal-equation step is positive; an invalid step needs rounding to defeat that, and none of these inputs did.  Those
two branches of lm_next_step stay untested.  A rejected step in the SECOND solve turned up twice in those 69 120 solves; one is in the table.

Decision margins.  HIP, checker and Ceres round differently, so a case is only usable when none of its decisions is close:
  rel      every judged step: |rel - 1e-3| / max(|rel|, 1e-3)                  (accept / reject, trust_region_minimizer.cc:744-829)
  ftol     every candidate:   | |x_cost - cand_cost| / x_cost / 1e-3 - 1 |     (function tolerance)
  chi2     every point:       |chi2 / threshold - 1| at the evaluation the outlier sweep reads
"Close" is NEAR below: 100 x the largest relative difference measured between the checker and the compiled reference over this table in
the quantities those decisions are taken on (tests/test_pnp_cases.py::test_checker_equals_reference computes, prints and bounds them):
  cost   |cost_checker - cost_Ceres| of every iteration, relative to the cost the step started from (the scale rel and the function
         tolerance see it at); initial and final cost of each solve, relative to the initial cost          measured 1.9e-9
  rel    |rel_checker - relative_decrease_Ceres| / max(|rel|, 1e-3)                                           measured 3.6e-10
  chi2   |chi2_checker - chi2err_Ceres| / threshold, every point, at the evaluation the sweep reads          measured 4.1e-9
The largest is 4.1e-9 (far-from-converged cases, where a chi2 is 1e4 x the threshold); MEASURED_DEV rounds it up to 1e-8, NEAR = 1e-6.
Every case's three margins are >= NEAR (test_margins; the smallest in the table is 6.1e-3, a chi2 of `plain_only`); the cases were
chosen once, on the CPU, so that this holds."""
from __future__ import annotations

import numpy as np

from alvaar_amd import synth

MEASURED_DEV = 1e-8
NEAR = 100.0 * MEASURED_DEV
REL_MIN, FTOL = 1e-3, 1e-3
CHI2_TH = 5.9915


def _case(name, branch, sig, gen, start=None, mods=(), max_iters=5, robust=True, l2=True):
    return dict(name=name, branch=branch, sig=sig, gen=gen, start=start, mods=tuple(mods), max_iters=max_iters, robust=robust, l2=l2)


def _g(n, seed, outlier_frac, **kw):
    return dict(n=n, seed=seed, outlier_frac=outlier_frac, **kw)


CASES = [
    # a rejected step in solve 1, then convergence; outliers, so the second solve runs
    _case("reject_converge", "rejected_then_converges", "ARRRRAAAAT:function_tolerance | AT:function_tolerance", _g(61, 3, 0.1), start=(0.5, 2), max_iters=10),
    # ... the same path without outliers: one solve
    _case("reject_converge_clean", "rejected_then_converges", "ARRRRAAAAT:function_tolerance | :not_run", _g(37, 1, 0.0), start=(0.5, 2), max_iters=10),
    # rejected steps, accepted ones, then the iteration cap
    _case("reject_cap", "rejected_then_cap", "ARRRRAAAAA:max_iterations | AT:function_tolerance", _g(61, 1, 0.1), start=(0.7, 2), max_iters=10),
    _case("reject_first_cap", "rejected_then_cap", "RAAAAAAAAA:max_iterations | AT:function_tolerance", _g(61, 1, 0.1), start=(0.7, 1), max_iters=10),
    # the LAST step of solve 1 is rejected: at the kept pose every point is an outlier (the call would return false), at the rejected
    # candidate one is not -- the verdicts must come from the candidate, and the second solve must run
    _case("reject_final", "rejected_final_step", "ARRRR:max_iterations | AAAT:parameter_tolerance", _g(130, 8, 0.0), start=(1.0, 2), max_iters=5),
    _case("reject_final_after_two", "rejected_final_step", "AARRRRR:max_iterations | AAAT:parameter_tolerance", _g(130, 1, 0.3), start=(1.3, 2), max_iters=7),
    _case("reject_final_both", "rejected_final_step", "AARRRR:max_iterations | AARRRR:max_iterations", _g(300, 7, 0.0), start=(1.3, 2), max_iters=6),
    # the cap with every step accepted
    _case("cap_accepted", "cap_all_accepted", "AAAAA:max_iterations | AT:function_tolerance", _g(600, 1, 0.2, pose_noise=0.3)),
    # every point an outlier -> false, no second solve
    _case("all_outliers_shifted", "all_outliers", "RRRRA:max_iterations | :not_run", _g(50, 2, 0.0), mods=[("shift_uv", 500.0)]),
    _case("all_outliers_rejecting", "all_outliers", "ARRRR:max_iterations | :not_run", _g(37, 1, 0.0), start=(0.5, 2)),
    # no outlier -> no second solve
    _case("no_outliers", "no_outliers", "AAT:function_tolerance | :not_run", _g(37, 5, 0.0, pose_noise=0.005)),
    _case("max_iters_0", "max_iters_0", ":max_iterations | :max_iterations", _g(130, 4, 0.1), max_iters=0),
    _case("max_iters_1", "max_iters_1", "A:max_iterations | A:max_iterations", _g(130, 4, 0.1), max_iters=1),
    # exact data, exact start: the gradient is exactly zero
    _case("gradient_exit", "gradient_exit", ":gradient | :not_run", dict(n=37, exact=True)),
    # four points mirrored through the camera centre (first, last and two in between): outliers by depth only
    _case("behind_camera", "behind_camera", "AAT:function_tolerance | T:function_tolerance", _g(130, 6, 0.0), mods=[("behind", (0, 5, 64, 129))]),
    # a rejected step in the second (L2) solve
    _case("reject_solve_2", "rejected_in_solve_2", "ARRRRRAAAA:max_iterations | AAAAARARRA:max_iterations", _g(130, 4, 0.0), start=(1.3, 4), max_iters=10),
    _case("reject_solve_2_first", "rejected_in_solve_2", "AARRRRR:max_iterations | RRRRRAA:max_iterations", _g(300, 12, 0.0), start=(1.3, 2), max_iters=7),
    # exit through the parameter tolerance
    _case("parameter_tolerance", "parameter_tolerance", "AAAAAAA:max_iterations | AAT:parameter_tolerance", _g(37, 1, 0.0), start=(0.7, 1), max_iters=7),
    # the switches: plain least squares only; robust without the L2 pass
    _case("plain_only", "plain_l2_only", "AT:function_tolerance | :not_run", _g(61, 3, 0.1), robust=False, l2=False),
    _case("robust_only", "plain_l2_only", "AAT:function_tolerance | :not_run", _g(61, 3, 0.1), robust=True, l2=False),
    _case("robust_only_reject_final", "rejected_final_step", "ARRRR:max_iterations | :not_run", _g(130, 8, 0.0), start=(1.0, 2), max_iters=5, l2=False),
]


def quat_mul(a, b):
    """Hamilton product, (x y z w)"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def perturbed_start(pose_gt, w, seed):
    rng = np.random.RandomState(seed)
    rv, tv = rng.normal(0, w, 3), rng.normal(0, 3 * w, 3)
    th = np.linalg.norm(rv)
    dq = np.concatenate([np.sin(th / 2) * rv / th, [np.cos(th / 2)]])
    q = quat_mul(dq, pose_gt[3:])
    return np.concatenate([pose_gt[:3] + tv, q if q[3] >= 0 else -q])


def exact_problem(n):
    """Identity pose and data on which every residual is EXACTLY zero in float64, with or without fused multiply-adds: depth a power of
    two, x / z and y / z multiples of 1 / 64, uv = fl(fl(K0 * x / z) + K2) in the operation order of the projection.  The gradient is then
    exactly 0 in the checker, in Ceres and on the device, and the solve ends on the gradient tolerance before any step."""
    K = tuple(float(np.float32(v)) for v in (579.4, 579.4, 320.0, 240.0))
    k = np.arange(n)
    z = 2.0 ** (1 + k % 3)
    xn, yn = ((k * 7) % 33 - 16) / 64.0, ((k * 5) % 25 - 12) / 64.0
    wpt = np.column_stack([xn * z, yn * z, z])
    uv = np.column_stack([K[0] * xn + K[2], K[1] * yn + K[3]])
    pose = np.array([0.0, 0, 0, 0, 0, 0, 1])
    return dict(uv=uv, wpt=wpt, K=(579.4, 579.4, 320.0, 240.0), pose_gt=pose, pose_init=pose.copy())


def build(case) -> dict:
    """-> dict(uv, wpt, pose_init, K, pose_gt, kw = the keyword arguments of Context.pnp_refine / Orc.pnp_refine)"""
    pb = exact_problem(case["gen"]["n"]) if case["gen"].get("exact") else synth.make_pnp_problem(**case["gen"])
    uv, wpt, gt = pb["uv"].copy(), pb["wpt"].copy(), pb["pose_gt"]
    for mod in case["mods"]:
        if mod[0] == "behind":     # mirror the listed points through the camera centre: same pixel, negative depth -- outliers by the depth test alone
            idx = list(mod[1])
            wpt[idx] = 2 * gt[:3] - wpt[idx]
        elif mod[0] == "shift_uv":  # every observation moved: nothing fits
            uv = uv + mod[1]
        else:
            raise ValueError(mod)
    start = case["start"]
    pose0 = pb["pose_init"] if start is None else perturbed_start(gt, *start)
    return dict(uv=np.ascontiguousarray(uv), wpt=np.ascontiguousarray(wpt), pose_init=pose0, K=pb["K"], pose_gt=gt,
                kw=dict(max_iters=case["max_iters"], robust=case["robust"], l2=case["l2"]))


_LETTER = dict(accepted="A", rejected="R", invalid="I", tolerance="T")


def signature(trace) -> str:
    return " | ".join("".join(_LETTER[k] for k in s["kinds"]) + ":" + s["exit"] for s in trace["solves"])


def margins(trace) -> dict:
    """the three distances of the module docstring, each the minimum over the call (inf where there is nothing to decide)"""
    rel_m, ftol_m = np.inf, np.inf
    for s in trace["solves"]:
        for kind, rel, fdec in zip(s["kinds"], s["rel"], s["fdec"]):
            if kind == "invalid":
                continue
            ftol_m = min(ftol_m, abs(fdec / FTOL - 1))
            if kind != "tolerance":
                rel_m = min(rel_m, abs(rel - REL_MIN) / max(abs(rel), REL_MIN))
    chi2 = trace["chi2"]
    return dict(rel=rel_m, ftol=ftol_m, chi2=float(np.abs(chi2 / np.float64(np.float32(CHI2_TH)) - 1).min()) if len(chi2) else np.inf)


def _s(trace, k):
    return trace["solves"][k]


# name -> predicate(ok, outliers, n, trace): the branch a case is in the table for
BRANCHES = {
    "rejected_then_converges": lambda ok, out, n, t: ok and "rejected" in _s(t, 0)["kinds"] and _s(t, 0)["exit"] == "function_tolerance",
    "rejected_then_cap": lambda ok, out, n, t: "rejected" in _s(t, 0)["kinds"][:-1] and _s(t, 0)["kinds"][-1] == "accepted" and _s(t, 0)["exit"] == "max_iterations",
    "rejected_final_step": lambda ok, out, n, t: _s(t, 0)["kinds"][-1] == "rejected" and _s(t, 0)["exit"] == "max_iterations" and 0 < len(out) < n,
    "cap_all_accepted": lambda ok, out, n, t: set(_s(t, 0)["kinds"]) == {"accepted"} and _s(t, 0)["exit"] == "max_iterations",
    "all_outliers": lambda ok, out, n, t: not ok and len(out) == n and _s(t, 1)["exit"] == "not_run",
    "no_outliers": lambda ok, out, n, t: ok and len(out) == 0 and _s(t, 1)["exit"] == "not_run",
    "max_iters_0": lambda ok, out, n, t: _s(t, 0)["kinds"] == [] and _s(t, 0)["exit"] == "max_iterations",
    "max_iters_1": lambda ok, out, n, t: len(_s(t, 0)["kinds"]) == 1 and _s(t, 0)["exit"] == "max_iterations",
    "gradient_exit": lambda ok, out, n, t: ok and _s(t, 0)["kinds"] == [] and _s(t, 0)["exit"] == "gradient",
    "behind_camera": lambda ok, out, n, t: ok and 0 < len(out) < n,
    "rejected_in_solve_2": lambda ok, out, n, t: "rejected" in _s(t, 1)["kinds"],
    "parameter_tolerance": lambda ok, out, n, t: "parameter_tolerance" in (_s(t, 0)["exit"], _s(t, 1)["exit"]),
    "plain_l2_only": lambda ok, out, n, t: _s(t, 1)["exit"] == "not_run",
}


# ---------------------------------------------------------------------------------------------------- verdict-bit and stride edges
# k_pnp keeps one verdict bit per point in a 64-bit register mask, point i in bit i / 512 of thread i % 512; alva_pnp_refine admits
# n <= 64 * 512.  The sizes straddle a wave (64), the workgroup (512), two strides, and the last bit of the mask.
EDGE_SIZES = (4, 5, 63, 64, 65, 511, 512, 513, 1025, 32767, 32768)


def edge_planted(n) -> np.ndarray:
    """index 0, n - 1, and every multiple of 512 and every 512 k + 511 that exists"""
    return np.unique([0, n - 1] + list(range(0, n, 512)) + list(range(511, n, 512)))


def edge_problem(n) -> dict:
    """an ordinary converging problem (0.3 px noise, so that no inlier comes near the threshold by chance among 32 768) whose planted
    outliers -- observations moved by (40, -35) px -- sit on the first and last bit of the first and last thread"""
    pb = synth.make_pnp_problem(n, 100 + n % 97, outlier_frac=0.0, noise_px=0.3, pose_noise=0.01)
    planted = edge_planted(n)
    uv = pb["uv"].copy()
    uv[planted] += np.array([40.0, -35.0])
    return dict(uv=uv, wpt=pb["wpt"], pose_init=pb["pose_init"], K=pb["K"], pose_gt=pb["pose_gt"], planted=planted)
