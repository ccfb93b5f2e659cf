"""GPU parity: a8 (P3P + LMedS) and a9 (robust PnP refinement).  FP64; the reference's libm/Eigen
rounding is not reproducible on the device, so poses are compared within a stated tolerance
(1e-8 absolute on R,t for P3P; 1e-9 on the 7 pose parameters for PnP -- far inside the 1e-5 RMSE bar of
BASELINE.json) while the discrete outputs (winning hypothesis' outlier set, LM iteration counts,
outlier lists) must match exactly.

The second half runs the refinement over the branch table of tests/pnp_cases.py (rejected steps, the iteration cap, a rejected final
step, every exit the search reached), over the sizes at which the per-thread verdict masks and the point stride change, and the pose
chain over both launch routes of pose_launch (fused k_p3p_pnp_s | k_p3p_s / k_p3p + k_pnp), alone and alternating on one context."""
import numpy as np
import pytest

import pnp_cases as PC
from alvaar_amd import synth
from oracles import Orc, Ref, ref_available

pytestmark = pytest.mark.gpu

P3P_TOL = 1e-8
PNP_TOL = 1e-9


def _checkers():
    return [("orc", Orc)] + ([("ref", Ref)] if ref_available() else [])


def test_sampler_matches_reference_stream():
    """Host sampler (std::mt19937 + uniform_int_distribution) == the oracle's restated stream."""
    import ctypes as C
    import alvaar_amd
    from oracles import orc_lib, _p
    for n in (4, 5, 192, 2000):
        a = np.zeros((150, 4), np.int32)
        b = np.zeros((150, 4), np.int32)
        alvaar_amd.check(alvaar_amd.lib.alva_p3p_draw_samples(n, 150, 0, 12345, a.ctypes.data))
        orc_lib().orc_p3p_draw_samples(n, 150, C.c_uint32(12345), _p(b))
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n,seed,outl", [(2000, 3, 0.1), (192, 4, 0.3), (12, 5, 0.0), (501, 6, 0.45), (4080, 7, 0.2), (10432, 8, 0.2), (19000, 9, 0.1)])
def test_p3p_lmeds(ctx, n, seed, outl):
    import torch
    pb = synth.make_pnp_problem(n, seed, outlier_frac=outl)
    ok, R, t, out = ctx.p3p_lmeds(torch.from_numpy(pb["bv"]).cuda(), torch.from_numpy(pb["wpt"]).cuda())
    for name, O in _checkers():
        ok2, R2, t2, out2 = O.p3p_lmeds(pb["bv"], pb["wpt"])
        assert ok == ok2 and ok, name
        assert np.abs(t - t2).max() < P3P_TOL and np.abs(R - R2).max() < P3P_TOL, name
        assert np.array_equal(out, out2), name


def test_p3p_too_few_points(ctx):
    import torch
    pb = synth.make_pnp_problem(3, 1, outlier_frac=0.0)
    ok, R, t, out = ctx.p3p_lmeds(torch.from_numpy(pb["bv"]).cuda(), torch.from_numpy(pb["wpt"]).cuda())
    assert not ok and len(out) == 0


@pytest.mark.parametrize("n,seed,outl,noise", [(2000, 3, 0.1, 0.01), (192, 4, 0.3, 0.02), (30, 5, 0.0, 0.005), (500, 6, 0.2, 0.05),
                                               (4080, 8, 0.15, 0.02)])
def test_pnp_refine(ctx, n, seed, outl, noise):
    import torch
    pb = synth.make_pnp_problem(n, seed, outlier_frac=outl, pose_noise=noise)
    ok, pose, out, info = ctx.pnp_refine(torch.from_numpy(pb["uv"]).cuda(), torch.from_numpy(pb["wpt"]).cuda(), pb["pose_init"], pb["K"])
    for name, O in _checkers():
        ok2, p2, o2, i2 = O.pnp_refine(pb["uv"], pb["wpt"], pb["pose_init"], pb["K"])
        assert ok == ok2, name
        assert np.array_equal(out, o2), name
        assert info[0] == i2[0] and info[4] == i2[4], (name, info, i2)
        assert np.allclose(info[[1, 2, 5, 6]], i2[[1, 2, 5, 6]], rtol=1e-9), name
        assert np.abs(pose - p2).max() < PNP_TOL, name
    rmse = np.sqrt(np.mean((pose[:3] - pb["pose_gt"][:3]) ** 2))
    assert rmse < 0.05


def test_pnp_all_outliers_returns_false(ctx):
    import torch
    pb = synth.make_pnp_problem(50, 2, outlier_frac=0.0)
    uv = pb["uv"] + 500.0
    ok, pose, out, info = ctx.pnp_refine(torch.from_numpy(uv).cuda(), torch.from_numpy(pb["wpt"]).cuda(), pb["pose_init"], pb["K"])
    ok2, p2, o2, i2 = Orc.pnp_refine(uv, pb["wpt"], pb["pose_init"], pb["K"])
    assert ok == ok2 and np.array_equal(out, o2)


def _rot_to_pose7(R, t):
    """Sophus::SE3d(R, t) -> [t, qx qy qz qw] (same branch rule as Eigen::Quaternion(R))."""
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(R).as_quat()
    if q[3] < 0:
        q = -q
    return np.concatenate([t, q])


@pytest.mark.parametrize("n,seed,outl", [(2000, 3, 0.1), (192, 4, 0.3), (40, 5, 0.0), (501, 6, 0.4)])
def test_compute_pose_chain(ctx, n, seed, outl):
    """alva_compute_pose == p3pRansac -> drop outliers -> ceresPnP of VisualFrontend::computePose (visual_frontend.cpp:300-399),
    checked against the chained oracle / reference calls on the compacted arrays."""
    import torch
    pb = synth.make_pnp_problem(n, seed, outlier_frac=outl)
    K = pb["K"]
    st, pose, m1, m2 = ctx.compute_pose(torch.from_numpy(pb["bv"]).cuda(), torch.from_numpy(pb["uv"]).cuda(), torch.from_numpy(pb["wpt"]).cuda(), K)
    for name, O in _checkers():
        ok1, R, t, out1 = O.p3p_lmeds(pb["bv"], pb["wpt"], fx=K[0], fy=K[1])
        assert ok1 and st >= 1, name
        mask = np.zeros(n, bool)
        mask[out1] = True
        assert np.array_equal(m1, mask), name
        keep = np.flatnonzero(~mask)
        ok2, p2, out2, _ = O.pnp_refine(pb["uv"][keep], pb["wpt"][keep], _rot_to_pose7(R, t), K)
        bad = np.zeros(n, bool)
        bad[keep[out2]] = True
        assert np.array_equal(m2, bad), name
        accept = ok2 and (len(keep) - len(out2)) >= 5 and len(out2) <= 0.5 * len(keep)
        assert st == (2 if accept else 1), name
        # sign of the quaternion is a representation choice; compare up to it
        if np.dot(pose[3:], p2[3:]) < 0:
            p2 = np.concatenate([p2[:3], -p2[3:]])
        assert np.abs(pose - p2).max() < 1e-8, (name, pose, p2)


def test_compute_pose_rejects_garbage(ctx):
    """P3P on unrelated 2-D/3-D sets: fewer than 5 inliers is impossible to rule out by construction, so only
    check the status agrees with the chained oracle."""
    import torch
    pb = synth.make_pnp_problem(60, 9, outlier_frac=0.0)
    rng = np.random.default_rng(0)
    wpt = rng.normal(size=pb["wpt"].shape) * 5
    K = pb["K"]
    st, pose, m1, m2 = ctx.compute_pose(torch.from_numpy(pb["bv"]).cuda(), torch.from_numpy(pb["uv"]).cuda(), torch.from_numpy(wpt).cuda(), K)
    ok1, R, t, out1 = Orc.p3p_lmeds(pb["bv"], wpt, fx=K[0], fy=K[1])
    assert (st >= 1) == bool(ok1)


def test_compute_pose_too_few(ctx):
    import torch
    pb = synth.make_pnp_problem(3, 1, outlier_frac=0.0)
    st, pose, m1, m2 = ctx.compute_pose(torch.from_numpy(pb["bv"]).cuda(), torch.from_numpy(pb["uv"]).cuda(),
                                        torch.from_numpy(pb["wpt"]).cuda(), pb["K"])
    assert st == 0


def test_compute_pose_enqueue_collect_equals_blocking_call(ctx):
    import torch
    pb = synth.make_pnp_problem(700, 11, outlier_frac=0.2)
    bv, uv, wp = (torch.from_numpy(pb[k]).cuda() for k in ("bv", "uv", "wpt"))
    a = ctx.compute_pose(bv, uv, wp, pb["K"])
    ctx.compute_pose_enqueue(bv, uv, wp, pb["K"])
    b = ctx.compute_pose_collect()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    with pytest.raises(Exception):
        ctx.compute_pose_collect()   # nothing pending


def test_p3p_many_degenerate_samples_force_a_redraw(ctx):
    """Most world points coincide, so most drawn triples are degenerate and do not count as LMedS iterations
    (Lmeds.hpp:88-92): the first batch of samples cannot supply 100 valid hypotheses and the call re-draws a longer prefix
    of the same stream.  Same result as the oracle's one-by-one loop."""
    import torch
    pb = synth.make_pnp_problem(400, 31, outlier_frac=0.1)
    wpt = pb["wpt"].copy()
    bv = pb["bv"].copy()
    rng = np.random.RandomState(5)
    dup = rng.rand(400) < 0.7
    wpt[dup] = wpt[0]                       # 70 % of the points are the same 3-D point
    bv[dup] = bv[0]
    ok, R, t, out = ctx.p3p_lmeds(torch.from_numpy(bv).cuda(), torch.from_numpy(wpt).cuda(), fx=pb["K"][0], fy=pb["K"][1])
    ok2, R2, t2, out2 = Orc.p3p_lmeds(bv, wpt, fx=pb["K"][0], fy=pb["K"][1])
    assert ok == ok2
    if ok:
        assert np.abs(R - R2).max() < P3P_TOL and np.abs(t - t2).max() < P3P_TOL and np.array_equal(out, out2)
    st, pose, m1, m2 = ctx.compute_pose(torch.from_numpy(bv).cuda(), torch.from_numpy(pb["uv"]).cuda(), torch.from_numpy(wpt).cuda(), pb["K"])
    assert (st >= 1) == bool(ok2)
    if ok2:
        mask = np.zeros(400, bool)
        mask[out2] = True
        assert np.array_equal(m1, mask)


# ---- the refinement over the branch table (tests/pnp_cases.py) ---------------------------------------------------------------------
_cpu_cache = {}


def _cpu_pnp(key, pb, kw):
    """the checkers' results for one problem, computed once per process"""
    if key not in _cpu_cache:
        _cpu_cache[key] = [(name, O.pnp_refine(pb["uv"], pb["wpt"], pb["pose_init"], pb["K"], **kw)) for name, O in _checkers()]
    return _cpu_cache[key]


def _assert_pnp_equal(got, want, n, tag):
    ok, pose, out, info = got
    ok2, p2, o2, i2 = want
    assert ok == ok2, tag
    assert np.array_equal(out, o2), (tag, len(out), len(o2))
    assert all(info[k] == i2[k] for k in (0, 3, 4, 7)), (tag, info, i2)
    assert np.allclose(info[[1, 2, 5, 6]], i2[[1, 2, 5, 6]], rtol=1e-9), (tag, info, i2)
    if len(o2) < n:   # (every point an outlier: ceresPnP returns before it writes the pose)
        assert np.abs(pose - p2).max() < PNP_TOL, (tag, pose, p2)


@pytest.mark.parametrize("case", PC.CASES, ids=[c["name"] for c in PC.CASES])
def test_pnp_refine_branch_table(ctx, case):
    """Every path of lm_next_step / lm_after_candidate the table reaches: same verdict, same outlier list, same summary and success
    counts in both solves as the checker (and Ceres, where built).  A kernel that skipped the radius update after a rejection, kept the
    rejected candidate's Hessian, or read the verdicts at the kept pose instead of the last evaluation fails the reject_* cases."""
    import torch
    b = PC.build(case)
    got = ctx.pnp_refine(torch.from_numpy(b["uv"]).cuda(), torch.from_numpy(b["wpt"]).cuda(), b["pose_init"], b["K"], **b["kw"])
    print(case["name"], "ok", got[0], "outliers", len(got[2]), "info", got[3])
    for name, want in _cpu_pnp(("case", case["name"]), b, b["kw"]):
        _assert_pnp_equal(got, want, len(b["uv"]), (case["name"], name))


@pytest.mark.parametrize("n", PC.EDGE_SIZES)
def test_pnp_refine_verdict_bits_and_strides(ctx, n):
    """Planted outliers on the first and last point, on every multiple of 512 and on every 512 k + 511: the first and last thread's
    first and last verdict bits, up to bit 63 at n = 32768.  From n = 63 on the problem converges as usual and the outlier list is
    exactly the planted set; at n = 4 and 5 two planted outliers leave too few points for that, and the list is the checker's."""
    import torch
    e = PC.edge_problem(n)
    got = ctx.pnp_refine(torch.from_numpy(e["uv"]).cuda(), torch.from_numpy(e["wpt"]).cuda(), e["pose_init"], e["K"])
    for name, want in _cpu_pnp(("edge", n), e, {}):
        _assert_pnp_equal(got, want, n, (n, name))
    if n >= 63:
        assert got[0] and np.array_equal(got[2], e["planted"])
        assert np.sqrt(np.mean((got[1][:3] - e["pose_gt"][:3]) ** 2)) < 0.05


# ---- the pose chain over both launch routes ----------------------------------------------------------------------------------------
POSE_ROUTE_CASES = [(4, 100), (5, 100), (6, 100), (7168, 100), (7169, 100), (10432, 100), (500, 164), (500, 165), (500, 200)]   # (n, p3p_iters)


def _pose_problem(n):
    pb = synth.make_pnp_problem(n, 40 + n % 13, outlier_frac=0.2, noise_px=0.5) if n >= 10 else synth.make_pnp_problem(n, 40 + n, outlier_frac=0.0, noise_px=0.1)
    return pb, tuple(__import__("torch").from_numpy(pb[k]).cuda() for k in ("bv", "uv", "wpt"))


def _chained_checker(pb, p3p_iters):
    """p3pRansac -> drop its outliers -> ceresPnP on the compacted arrays -> the acceptance tests of VisualFrontend::computePose:
    (status, pose or None, P3P outlier mask, PnP outlier mask), as test_compute_pose_chain spells it out"""
    key = ("pose", len(pb["uv"]), p3p_iters)
    if key not in _cpu_cache:
        n, K = len(pb["uv"]), pb["K"]
        ok1, R, t, out1 = Orc.p3p_lmeds(pb["bv"], pb["wpt"], max_iters=p3p_iters, fx=K[0], fy=K[1])
        m1, m2, pose, st = np.zeros(n, bool), np.zeros(n, bool), None, 0
        if ok1:
            st = 1
            m1[out1] = True
            keep = np.flatnonzero(~m1)
            ok2, pose, out2, _ = Orc.pnp_refine(pb["uv"][keep], pb["wpt"][keep], _rot_to_pose7(R, t), K)
            m2[keep[out2]] = True
            if len(out2) == len(keep):
                pose = None
            elif ok2 and (len(keep) - len(out2)) >= 5 and len(out2) <= 0.5 * len(keep):
                st = 2
        _cpu_cache[key] = (st, pose, m1, m2)
    return _cpu_cache[key]


def _assert_pose_equals_chain(got, want, tag):
    st, pose, m1, m2 = got
    st2, p2, w1, w2 = want
    assert st == st2, (tag, st, st2)
    assert np.array_equal(m1, w1) and np.array_equal(m2, w2), tag
    if p2 is not None:
        if np.dot(pose[3:], p2[3:]) < 0:   # the sign of the quaternion is a representation choice
            p2 = np.concatenate([p2[:3], -p2[3:]])
        assert np.abs(pose - p2).max() < 1e-8, (tag, pose, p2)


def _bit_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("n,p3p_iters", POSE_ROUTE_CASES)
def test_compute_pose_launch_routes(ctx, monkeypatch, n, p3p_iters):
    """pose_launch takes one launch (k_p3p_pnp_s) up to n = 7168 and H = p3p_iters + 28 = 192, two launches beyond either: both sides of
    both thresholds and the smallest problems, against the chained checker; where the fused launch applies, the two launches
    (ALVA_POSE_UNFUSED=1, read per call) must give the same bits."""
    pb, (bv, uv, wp) = _pose_problem(n)
    monkeypatch.delenv("ALVA_POSE_UNFUSED", raising=False)
    got = ctx.compute_pose(bv, uv, wp, pb["K"], p3p_iters=p3p_iters)
    print(n, p3p_iters, "status", got[0], "p3p outliers", int(got[2].sum()), "pnp outliers", int(got[3].sum()))
    _assert_pose_equals_chain(got, _chained_checker(pb, p3p_iters), (n, p3p_iters))
    if n >= 100:
        assert got[0] == 2
    if n <= 7168 and p3p_iters + 28 <= 192:
        monkeypatch.setenv("ALVA_POSE_UNFUSED", "1")
        assert _bit_equal(ctx.compute_pose(bv, uv, wp, pb["K"], p3p_iters=p3p_iters), got), (n, p3p_iters)


ROUTE_SEQUENCE = [(500, 100), (7169, 100), (500, 100), (500, 200), (500, 100)]   # fused, two launches (n), fused, two launches (H = 228), fused


@pytest.fixture(scope="module")
def fresh_pose_results():
    """each distinct call of ROUTE_SEQUENCE on a context of its own that has done nothing else"""
    import alvaar_amd
    res = {}
    for n, iters in sorted(set(ROUTE_SEQUENCE)):
        pb, (bv, uv, wp) = _pose_problem(n)
        c = alvaar_amd.Context(0)
        res[(n, iters)] = c.compute_pose(bv, uv, wp, pb["K"], p3p_iters=iters)
        c.close()
    return res


@pytest.mark.parametrize("split", [False, True], ids=["blocking", "enqueue_collect"])
def test_compute_pose_routes_alternate_on_one_context(monkeypatch, fresh_pose_results, split):
    """Both routes share one pinned block (the samples at its start, the result behind them: the offsets move with H and n) and one
    sequence counter per context.  Alternating them on ONE context must give, call by call, the bits a fresh context gives."""
    import alvaar_amd
    monkeypatch.delenv("ALVA_POSE_UNFUSED", raising=False)
    c = alvaar_amd.Context(0)
    try:
        for step, (n, iters) in enumerate(ROUTE_SEQUENCE):
            pb, (bv, uv, wp) = _pose_problem(n)
            if split:
                c.compute_pose_enqueue(bv, uv, wp, pb["K"], p3p_iters=iters)
                got = c.compute_pose_collect()
            else:
                got = c.compute_pose(bv, uv, wp, pb["K"], p3p_iters=iters)
            assert got[0] == 2, (step, n, iters)
            assert _bit_equal(got, fresh_pose_results[(n, iters)]), (step, n, iters)
            _assert_pose_equals_chain(got, _chained_checker(pb, iters), (step, n, iters))
    finally:
        c.close()
