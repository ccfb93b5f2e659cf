"""GPU parity: a10-a13 -- local bundle adjustment (LM + Huber + Schur, FP64 with the reduced camera system
formed on the FP64 matrix core).  Tolerances: poses 1e-8, point parameters 1e-7 (inverse depth) / 1e-6 (XYZ),
costs 1e-8 relative; iteration / accepted-step counts, depth flags and the chi2 > 5.9915 outlier
classification must match exactly."""
import numpy as np
import pytest

import ba_cases
from alvaar_amd import synth
from alvaar_amd.capi import AlvaError
from oracles import Orc, Ref, ref_available
from test_oracle_vs_ref import ba_compare, xyz_problem

pytestmark = pytest.mark.gpu


def _checkers(full=False):
    return [("orc", Orc)] + ([("ref", Ref)] if ref_available() else [])


# Noise levels of the rows that are not synth.make_ba_problem's defaults.  (6, 150, 4) at pose noise 0.1 / inverse-depth noise 0.3 is the
# REJECTED-STEP problem: within 5 iterations three of its five steps are rejected (info[0] = 6 summaries, info[3] = 3 = the start + two
# accepted steps, by the CPU oracle and by Ceres) -- no other row of this file rejects a step.
_NOISE = {(6, 150, 4): dict(pose_noise=0.1, invdepth_noise=0.3)}


def _problem(nkf, npt, seed, **default):
    return synth.make_ba_problem(nkf, npt, seed, **_NOISE.get((nkf, npt, seed), default))


@pytest.mark.parametrize("nkf,npt,seed,iters,ftol", [(6, 200, 1, 5, 0.0), (20, 600, 42, 5, 0.0), (8, 300, 2, 5, 1e-3), (5, 80, 3, 2, 0.0),
                                                     (3, 10, 4, 5, 0.0), (6, 150, 4, 5, 0.0)])
def test_local_ba_invdepth(ctx, nkf, npt, seed, iters, ftol):
    pb = _problem(nkf, npt, seed)
    g = ctx.local_ba(pb, iters, ftol)
    if (nkf, npt, seed) in _NOISE:
        assert g["info"][3] < g["info"][0]   # a step was rejected
    for name, O in _checkers():
        ba_compare(g, O.local_ba(pb, iters, ftol))


@pytest.mark.parametrize("nkf,npt,seed", [(6, 150, 5), (12, 400, 6)])
def test_local_ba_xyz(ctx, nkf, npt, seed):
    pb = xyz_problem(nkf, npt, seed)
    g = ctx.local_ba(pb, 5, 0.0, inv_depth=False)
    for name, O in _checkers():
        ba_compare(g, O.local_ba(pb, 5, 0.0, inv_depth=False), pt_tol=1e-6)


def test_local_ba_full_size(ctx):
    """BASELINE config 4: 20 KF x 3000 pts, 5 LM iterations.  Compared against the compiled reference
    (Ceres) when present, else the restatement; plus size-independent properties: the cost decreases
    monotonically over accepted steps and the result is invariant to the order observations are listed in."""
    pb = synth.make_ba_problem(20, 3000, 42)
    g = ctx.local_ba(pb, 5, 0.0)
    O = Ref if ref_available() else Orc
    ba_compare(g, O.local_ba(pb, 5, 0.0))
    assert g["info"][2] < 0.1 * g["info"][1]
    perm = np.random.RandomState(0).permutation(len(pb["obs_kf"]))
    pb2 = dict(pb, obs_kf=pb["obs_kf"][perm], obs_pt=pb["obs_pt"][perm], obs_uv=pb["obs_uv"][perm])
    g2 = ctx.local_ba(pb2, 5, 0.0)
    assert np.abs(g2["poses"] - g["poses"]).max() < 1e-10
    assert np.allclose(g2["chi2"], g["chi2"][perm], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("nkf,npt,seed", [(28, 900, 9), (40, 600, 10)])
def test_local_ba_more_cameras_than_fit_in_lds(ctx, nkf, npt, seed):
    """More than 21 free cameras (6 x free, rounded up to a multiple of 16, > 128: BaHost::sizes): the reduced camera system no longer fits
    the LDS and the blocked Cholesky runs on the copy in device memory (k_solve<false>); same tolerances."""
    pb = synth.make_ba_problem(nkf, npt, seed)
    assert int((pb["kf_const"] == 0).sum()) > 21
    g = ctx.local_ba(pb, 5, 0.0)
    ba_compare(g, Orc.local_ba(pb, 5, 0.0))


@pytest.mark.parametrize("sizes", [[(20, 3000, 42)], [(20, 3000, 42), (8, 400, 1), (12, 1500, 2), (5, 120, 3), (6, 150, 4)], [(6 + (b % 9), 200 + 37 * b, 10 + b) for b in range(64)]])
def test_local_ba_batch_bitwise_equal_to_single_solves(ctx, sizes):
    """alva_local_ba_batch: B ragged problems with one set of launches per LM iteration; every problem's poses, points, chi2 / depth flags
    and LM bookkeeping (summaries, accepted steps, costs) are BIT-IDENTICAL to its own alva_local_ba call.  Problems stop at different
    iterations (function tolerance 1e-3, as Optimizer::localBA sets it)."""
    from alvaar_amd import synth
    # alternating noise levels: problems converge after different numbers of iterations
    # ((6, 150, 4): the rejected-step problem, at its own noise levels)
    pbs = [_problem(k, n, s, pose_noise=(0.0002 if i % 3 == 0 else 0.02), invdepth_noise=(0.001 if i % 3 == 0 else 0.05)) for i, (k, n, s) in enumerate(sizes)]
    for ftol, iters in ((1e-3, 5), (0.0, 5)):
        single = [ctx.local_ba(pb, iters, ftol) for pb in pbs]
        batch = ctx.local_ba_batch(pbs, iters, ftol)
        stops = set()
        for a, b in zip(single, batch):
            assert a["ok"] == b["ok"]
            assert np.array_equal(a["info"][:4], b["info"])
            assert np.array_equal(a["poses"].view(np.uint64), b["poses"].view(np.uint64))
            assert np.array_equal(a["pts"].view(np.uint64), b["pts"].view(np.uint64))
            assert np.array_equal(a["chi2"].view(np.uint64), b["chi2"].view(np.uint64)) and np.array_equal(a["depth"], b["depth"])
            stops.add(int(a["info"][0]))
        if any(key in _NOISE for key in sizes) and ftol == 0.0:
            assert any(b["info"][3] < b["info"][0] for b in batch)   # a step was rejected inside the batch
        if len(sizes) > 8 and ftol > 0:
            assert len(stops) > 1     # the batch really is ragged in iterations too


@pytest.mark.parametrize("nkf,npt,seed,iters,ftol", [(6, 200, 1, 5, 0.0), (20, 3000, 42, 5, 0.0), (14, 1500, 9, 5, 1e-3), (3, 10, 4, 5, 0.0), (31, 900, 12, 3, 0.0)])
def test_local_ba_csr_bitwise_equal_to_the_host_structured_solve(ctx, nkf, npt, seed, iters, ftol):
    """alva_local_ba_csr -- observations grouped by point, the (observing, anchor) pair grouping built by the device's stable counting
    sort, the outlier sweep's test returned as one bit per residual block -- against alva_local_ba on the same problem: poses and point
    parameters BIT-IDENTICAL, iteration counts equal, the bits == (chi2 > threshold or point behind the camera) of the host-structured
    solve."""
    pb = dict(synth.make_ba_problem(nkf, npt, seed))
    rng = np.random.RandomState(seed)
    # outliers, so that the sweep has something to flag
    bad_obs = rng.choice(len(pb["obs_kf"]), max(2, len(pb["obs_kf"]) // 200), replace=False)
    uv = pb["obs_uv"].copy()
    uv[bad_obs] += rng.uniform(4, 9, (len(bad_obs), 2))
    pb["obs_uv"] = uv
    a = ctx.local_ba(pb, iters, ftol)
    b = ctx.local_ba_csr(pb, iters, ftol, chi2_threshold=5.9915)
    assert a["ok"] == b["ok"] and list(a["info"][:4]) == list(b["info"][:4])
    assert np.array_equal(a["poses"].view(np.uint64), b["poses"].view(np.uint64))
    assert np.array_equal(a["pts"].view(np.uint64), b["pts"].view(np.uint64))
    want = (a["chi2"] > 5.9915) | (a["depth"] == 0)
    assert np.array_equal(b["bad"], want[b["order"]]) and b["n_bad"] == int(want.sum()) and b["n_bad"] >= 1


_NO_POLL_CHILD = """
import sys
import numpy as np
import alvaar_amd
from alvaar_amd import synth
ctx = alvaar_amd.Context(0)
out = {}
for i, (args, noise) in enumerate(eval(sys.argv[2])):
    pb = synth.make_ba_problem(*args, **noise)
    for name, r in (("ba", ctx.local_ba(pb, 5, 0.0)), ("csr", ctx.local_ba_csr(pb, 5, 0.0, chi2_threshold=5.9915))):
        for key, v in r.items():
            out["%s%d_%s" % (name, i, key)] = np.asarray(v)
np.savez(sys.argv[1], **out)
"""


def test_local_ba_no_poll_driver_bitwise_equal_to_polling(ctx, tmp_path):
    """ALVA_NO_POLL=1 is read once per process, so the stream-wait form of the driver needs a process of its own: a fresh child solves two
    of this file's problems (one of them the rejected-step problem) through alva_local_ba and alva_local_ba_csr; poses, points, chi2,
    depth flags / bad bits, info and ok are BIT-IDENTICAL to this process's polling results."""
    import os
    import subprocess
    import sys
    from pathlib import Path
    cases = [((6, 200, 1), {}), ((6, 150, 4), _NOISE[(6, 150, 4)])]
    npz = tmp_path / "no_poll.npz"
    root = Path(__file__).resolve().parents[1]
    env = dict(os.environ, ALVA_NO_POLL="1", PYTHONPATH=os.pathsep.join([str(root)] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    child = subprocess.run([sys.executable, "-c", _NO_POLL_CHILD, str(npz), repr(cases)], env=env, cwd=str(root), timeout=300)
    assert child.returncode == 0
    got = np.load(npz)
    for i, (args, noise) in enumerate(cases):
        pb = synth.make_ba_problem(*args, **noise)
        for name, want in (("ba", ctx.local_ba(pb, 5, 0.0)), ("csr", ctx.local_ba_csr(pb, 5, 0.0, chi2_threshold=5.9915))):
            assert set(want) == {k[len(name) + 2:] for k in got.files if k.startswith("%s%d_" % (name, i))}
            for key, v in want.items():
                w, g = np.asarray(v), got["%s%d_%s" % (name, i, key)]
                assert w.dtype == g.dtype and w.shape == g.shape, (name, i, key)
                assert w.tobytes() == g.tobytes(), (name, i, key)


# ---- problems shaped like the map layer's (tests/ba_cases.py): anchors with the higher slot, both triangles of the pair sums, scattered
# constants, Huber-active and behind-the-camera blocks, the edges of the reduced system's sizes, 64 .. 128 keyframes
@pytest.mark.parametrize("name", ba_cases.CASE_NAMES)
def test_local_ba_map_shaped(ctx, name):
    """alva_local_ba on every case of the table against the CPU oracle and, where built, Ceres: ba_compare's bars, unchanged."""
    c = ba_cases.case(name)
    pb, inv = c["pb"], c["inv_depth"]
    g = ctx.local_ba(pb, c["iters"], c["ftol"], inv_depth=inv)
    checks = [("orc", c["orc"])] + ([("ref", Ref.local_ba(pb, c["iters"], c["ftol"], inv_depth=inv))] if ref_available() else [])
    for who, want in checks:   # the figures first, then the bars
        print("%s vs %s: info %s / %s  poses %.3g  points %.3g  chi2 class differs in %d  depth differs in %d" % (
            name, who, g["info"][:4], want["info"][:4], np.abs(g["poses"] - want["poses"]).max(), np.abs(g["pts"] - want["pts"]).max() if len(g["pts"]) else 0.0,
            int(((g["chi2"] > 5.9915) != (want["chi2"] > 5.9915)).sum()), int((g["depth"] != want["depth"]).sum())))
    for who, want in checks:
        ba_compare(g, want, pt_tol=c["pt_tol"])
    if "rejected_step" in c["props"]:
        assert g["info"][3] < g["info"][0]


@pytest.mark.parametrize("name", ba_cases.INV_NAMES)
def test_local_ba_csr_map_shaped(ctx, name):
    """alva_local_ba_csr on the same cases: bit-identical to alva_local_ba, and the sweep's bits == (chi2 > threshold or behind the camera)
    of alva_local_ba AND of the CPU oracle.  Cases with more than 32 keyframes are refused on the host."""
    c = ba_cases.case(name)
    pb = c["pb"]
    if len(pb["poses"]) > 32:
        with pytest.raises(AlvaError, match="error -1.*bad argument"):
            ctx.local_ba_csr(pb, c["iters"], c["ftol"], chi2_threshold=5.9915)
        return
    a = ctx.local_ba(pb, c["iters"], c["ftol"])
    b = ctx.local_ba_csr(pb, c["iters"], c["ftol"], chi2_threshold=5.9915)
    assert a["ok"] == b["ok"] and list(a["info"][:4]) == list(b["info"][:4])
    assert np.array_equal(a["poses"].view(np.uint64), b["poses"].view(np.uint64))
    assert np.array_equal(a["pts"].view(np.uint64), b["pts"].view(np.uint64))
    want = (a["chi2"] > 5.9915) | (a["depth"] == 0)
    assert np.array_equal(b["bad"], want[b["order"]]) and b["n_bad"] == int(want.sum())
    orc = c["orc"]
    want = (orc["chi2"] > 5.9915) | (orc["depth"] == 0)
    assert np.array_equal(b["bad"], want[b["order"]]) and b["n_bad"] == int(want.sum())
    if "huber" in c["props"] or "depth_flag" in c["props"]:
        assert b["n_bad"] >= 3


_BATCH = ["reversed_c3_11_19", "permuted_outliers", "free1", "reversed_c0_7_8_19_outliers", "free21", "rejected_permuted", "behind_outliers", "free8", "free16",
          "permuted_ftol", "free0"]


def test_local_ba_batch_map_shaped(ctx):
    """One batch that mixes relabelled, scattered-constant, outlier, 0-, 1- and 21-free problems (21: the largest system the batch takes):
    every problem BIT-IDENTICAL to its own alva_local_ba call, with and without the function tolerance."""
    pbs = [ba_cases.case(n)["pb"] for n in _BATCH]
    assert max(int((pb["kf_const"] == 0).sum()) for pb in pbs) == 21
    for ftol, iters in ((1e-3, 5), (0.0, 5)):
        single = [ctx.local_ba(pb, iters, ftol) for pb in pbs]
        batch = ctx.local_ba_batch(pbs, iters, ftol)
        for name, a, b in zip(_BATCH, single, batch):
            assert a["ok"] == b["ok"], name
            assert np.array_equal(a["info"][:4], b["info"]), name
            assert np.array_equal(a["poses"].view(np.uint64), b["poses"].view(np.uint64)), name
            assert np.array_equal(a["pts"].view(np.uint64), b["pts"].view(np.uint64)), name
            assert np.array_equal(a["chi2"].view(np.uint64), b["chi2"].view(np.uint64)) and np.array_equal(a["depth"], b["depth"]), name
        if ftol == 0.0:
            assert any(b["info"][3] < b["info"][0] for b in batch)   # a step was rejected inside the batch
            for name, b in zip(_BATCH, batch):   # and the batch's own results against the oracle, where the case is solved this way
                c = ba_cases.case(name)
                if (c["iters"], c["ftol"]) == (iters, ftol):
                    ba_compare(b, c["orc"])


def test_local_ba_batch_refuses_a_system_that_does_not_fit_the_lds(ctx):
    """22 free keyframes: the batch keeps every reduced system in LDS and refuses the list on the host (bad argument), whatever else is in
    it; the caller's arrays are not touched."""
    pbs = [ba_cases.case("free8")["pb"], ba_cases.case("free22")["pb"]]
    before = [(pb["poses"].copy(), pb["inv_depth"].copy()) for pb in pbs]
    with pytest.raises(AlvaError, match="error -1.*bad argument"):
        ctx.local_ba_batch(pbs, 5, 0.0)
    assert all(np.array_equal(pb["poses"], p) and np.array_equal(pb["inv_depth"], t) for pb, (p, t) in zip(pbs, before))
    ctx.local_ba_batch(pbs[:1], 5, 0.0)   # the context is as usable as before


@pytest.mark.parametrize("kind", ba_cases.DEGENERATE)
def test_local_ba_degenerate_sizes(ctx, kind):
    """Sizes the C ABI accepts and the map layer never sends: no observations, no points (nothing moves, one summary, ok), a free keyframe
    that no residual block touches (it stays where it was) -- what the CPU oracle returns.  (No free keyframe at all: case free0.)"""
    pb = ba_cases.degenerate(kind)
    want = Orc.local_ba(pb, 5, 0.0)
    g = ctx.local_ba(pb, 5, 0.0)
    ba_compare(g, want)
    if kind == "free_kf_without_blocks":
        # (the device stores every free pose with its quaternion normalised again: one rounding, not a step)
        assert np.abs(g["poses"][2] - pb["poses"][2]).max() < 1e-15
        b = ctx.local_ba_csr(pb, 5, 0.0, chi2_threshold=5.9915)
        assert np.array_equal(g["poses"].view(np.uint64), b["poses"].view(np.uint64)) and np.array_equal(g["pts"].view(np.uint64), b["pts"].view(np.uint64))
        return
    assert g["ok"] and g["info"][0] == 1 and g["info"][3] == 1
    assert np.abs(g["poses"] - pb["poses"]).max() < 1e-15 and np.array_equal(g["pts"], pb["inv_depth"])
    b = ctx.local_ba_csr(pb, 5, 0.0, chi2_threshold=5.9915)
    assert b["ok"] and b["info"][0] == 1 and b["n_bad"] == 0 and np.array_equal(g["poses"].view(np.uint64), b["poses"].view(np.uint64))
    with pytest.raises(AlvaError, match="error -1.*bad argument"):   # the batch takes no empty problem
        ctx.local_ba_batch([pb], 5, 0.0)


def test_local_ba_refuses_more_keyframes_than_documented(ctx):
    """ALVA_LOCAL_BA_MAX_KF (include/alvaar_hip.h) keyframes are solved (case ring128); one more is refused by all three entry points on
    the host, as a bad argument, before anything is launched."""
    import re
    from pathlib import Path
    header = (Path(__file__).resolve().parents[1] / "include" / "alvaar_hip.h").read_text()
    max_kf = int(re.search(r"#define\s+ALVA_LOCAL_BA_MAX_KF\s+(\d+)", header).group(1))
    assert max_kf >= 64   # the mapper sends up to 64
    assert len(ba_cases.case("ring128")["pb"]["poses"]) == max_kf
    small = ba_cases.case("free1")["pb"]
    n = max_kf + 1
    poses = np.tile(small["poses"][:1], (n, 1))
    poses[:len(small["poses"])] = small["poses"]
    kfc = np.ones(n, np.uint8)
    kfc[:len(small["poses"])] = small["kf_const"]
    pb = dict(small, poses=poses, kf_const=kfc)
    for call in (lambda: ctx.local_ba(pb, 5, 0.0), lambda: ctx.local_ba_csr(pb, 5, 0.0), lambda: ctx.local_ba_batch([pb], 5, 0.0),
                 lambda: ctx.local_ba_batch([small, pb], 5, 0.0)):
        with pytest.raises(AlvaError, match="error -1.*bad argument"):
            call()
    assert np.array_equal(pb["poses"], poses)
    ba_compare(ctx.local_ba(small, 5, 0.0), ba_cases.case("free1")["orc"])   # the context is as usable as before
