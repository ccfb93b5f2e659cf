"""alva_find_plane on the GPU, through alva_find_plane_trace, against its numpy restatement on the case table of
tests/findplane_cases.py.

EXACT, no tolerance: every score as a bit pattern (+inf where the iteration is skipped), the planes of the scored iterations, the
winner, its score, kth, every inlier flag, the inlier count and found / not found -- the library rounds once per operation in a written
order (-ffp-contract=off, correctly rounded divide and sqrt), and the restatement does the same.
MOMENTS: |got - exact sum| <= n_in * 2^-53 * sum|terms| per entry -- the bound of ANY summation order of n_in exact products
((n_in - 1) u / (1 - (n_in - 1) u) <= n_in u); the difference is taken by math.fsum over the terms and -got, so nothing is measured.
POSE: the origin within 1 float ulp of the restatement's (a last-bit difference of the double sum can cross a float rounding boundary).
Rotation entries within ROT_TOL = 4 x the largest difference seen against the float64 restatement (numpy.linalg.eigh for the
eigenvector) over the table's found cases.  Measured maximum on an MI355X: 1.1920929e-07 (one float ulp of an entry in [0.5, 1)), the same figure
as between the two CPU restatements; 4 x that is 4.8e-7, under the project's 1e-5 float bar for f3."""
from __future__ import annotations

import math

import numpy as np
import pytest

import findplane_cases as F

pytestmark = pytest.mark.gpu

ROT_TOL = 4.8e-7
assert ROT_TOL <= 1e-5
NAMES = sorted(F.cases())


@pytest.fixture(scope="module")
def ctx():
    import alvaar_amd
    c = alvaar_amd.Context(0)
    yield c
    c.close()


_dev = {}


def _points(name):
    import torch
    if name not in _dev:
        _dev[name] = torch.from_numpy(F.cases()[name]["P"]).cuda()
    return _dev[name]


def _gpu(ctx, name, trace=True):
    c = F.cases()[name]
    return ctx.find_plane(_points(name), c["pose7"], samples3=c["S"], want_trace=trace)


def _blob(got):
    """every output byte of a traced call"""
    pose, t = got
    parts = [np.zeros(16, np.float32) if pose is None else pose, t["scores"], t["planes"], t["inlier"], t["moments"],
             np.array([t["best"], t["n_inliers"], t["kth"], pose is not None], np.int32), np.array([t["best_score"]], np.float32)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


@pytest.fixture(scope="module")
def table(ctx):
    """the whole table, once; shared by the tests below and left unchanged"""
    return {name: _gpu(ctx, name) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_discrete_outputs_are_exact(table, name):
    r = F.cases()[name]["r"]
    pose, t = table[name]
    assert t["kth"] == r["kth"]
    assert np.array_equal(F.bits(t["scores"]), F.bits(r["scores"])), (name, np.flatnonzero(F.bits(t["scores"]) != F.bits(r["scores"])))
    scored = np.isfinite(r["scores"])
    assert np.array_equal(F.bits(t["planes"][scored]), F.bits(r["planes"][scored])), name
    assert not t["planes"][~scored].any()
    assert t["best"] == r["best"] and F.bits(t["best_score"])[0] == F.bits(r["best_score"])[0], (name, t["best"], t["best_score"])
    assert np.array_equal(t["inlier"], r["inlier"]), (name, np.flatnonzero(t["inlier"] != r["inlier"]))
    assert t["n_inliers"] == r["n_in"] == int(t["inlier"].sum())
    assert (pose is not None) == r["found"], name


@pytest.mark.parametrize("name", NAMES)
def test_moments_within_the_bound_of_any_summation_order(table, name):
    r = F.cases()[name]["r"]
    got = table[name][1]["moments"]
    if r["n_in"] == 0:
        assert not got.any()
        return
    assert got[9] == r["n_in"]
    for k in range(13):
        delta = abs(math.fsum(list(r["moment_terms"][k]) + [-float(got[k])]))
        bound = r["n_in"] * 2.0 ** -53 * r["moment_abs"][k]
        assert delta <= bound, (name, k, delta, bound)


def test_poses(table):
    worst_rot, worst_org = 0.0, 0
    for name in NAMES:
        r = F.cases()[name]["r"]
        pose = table[name][0]
        if not r["found"]:
            continue
        assert pose[3] == pose[7] == pose[11] == 0.0 and pose[15] == 1.0
        ulps = np.abs(pose[12:15].astype(np.float64) - r["origin"].astype(np.float64)) / np.spacing(np.abs(r["origin"])).astype(np.float64)
        rot = float(np.abs(pose[:12].astype(np.float64) - r["pose"][:12].astype(np.float64)).max())
        print("%-20s origin: %g ulp   rotation: max |delta| = %.9g" % (name, ulps.max(), rot))
        worst_rot, worst_org = max(worst_rot, rot), max(worst_org, ulps.max())
        assert ulps.max() <= 1.0, (name, ulps)
        assert rot <= ROT_TOL, (name, rot)
    print("largest rotation difference:", worst_rot, " largest origin difference (ulp):", worst_org)
    # both flip branches, and a rotated camera: the normal (the rotation's first column, R1 (1,0,0)) ends on the side the restatement says
    for name in ("camera_above", "camera_below", "pose_rotated"):
        assert np.sign(table[name][0][2]) == np.sign(F.cases()[name]["r"]["normal"][2]) != 0


@pytest.mark.parametrize("name", NAMES)
def test_without_the_trace_the_same_bits(ctx, table, name):
    plain = _gpu(ctx, name, trace=False)
    pose = table[name][0]
    assert (plain is None) == (pose is None)
    assert plain is None or np.array_equal(plain.view(np.uint32), pose.view(np.uint32))


def test_the_table_twice_on_one_context_is_identical(ctx, table):
    for name in NAMES:
        assert _blob(_gpu(ctx, name)) == _blob(table[name]), name


def test_shared_buffers_keep_nothing_between_calls(table):
    """find-plane shares scratch slot 9 and the pinned block with plane detection and the hit test, and both grow on demand: the cases in
    growing then shrinking order of n and iteration count, with one alva_detect_planes and one alva_hit_test call in between, against every
    case alone on a context of its own"""
    import torch
    import alvaar_amd
    import hit_cases as H
    fresh = {}
    for name in NAMES:
        c = alvaar_amd.Context(0)
        fresh[name] = _blob(_gpu(c, name))
        c.close()
        assert fresh[name] == _blob(table[name]), name
    size = lambda name: (len(F.cases()[name]["P"]), len(F.cases()[name]["S"]))
    up = sorted(NAMES, key=size)
    by_iters = sorted(NAMES, key=lambda name: size(name)[::-1])
    other = torch.from_numpy(H.base_scene()).cuda()
    c = alvaar_amd.Context(0)
    for k, name in enumerate(up + up[::-1] + by_iters + by_iters[::-1]):
        if k % 9 == 4:
            c.detect_planes(other, H.POSE_BASE, 0.03)
        if k % 9 == 7:
            _, info = c.hit_test(other, H.POSE_BASE, H.K_BASE, [(250.0, 240.0)])
            assert info[0, 0] == 0 and info[0, 1] == 44
        assert _blob(_gpu(c, name)) == fresh[name], (k, name)
    c.close()


def test_bad_arguments_are_rejected_and_the_context_survives(ctx, table):
    import torch
    import alvaar_amd
    name = "n257"
    c = F.cases()[name]
    P, n = _points(name), len(c["P"])
    for i, j, bad in ((0, 0, n), (len(c["S"]) - 1, 2, n), (3, 1, -1), (5, 0, 2 ** 31 - 1), (2, 2, -2 ** 31)):
        S = c["S"].copy()
        S[i, j] = bad                # one index outside [0, n): rejected on the host, nothing is launched
        for trace in (False, True):
            with pytest.raises(alvaar_amd.AlvaError):
                ctx.find_plane(P, c["pose7"], samples3=S, want_trace=trace)
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.find_plane(torch.zeros((12289, 3), dtype=torch.float64, device="cuda"), c["pose7"], samples3=c["S"], want_trace=True)
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.find_plane(P, c["pose7"], samples3=np.zeros((0, 3), np.int32), want_trace=True)
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.find_plane(P, c["pose7"], num_iterations=0)
    assert _blob(_gpu(ctx, name)) == _blob(table[name])          # the same context still answers a table case, to the bit
    S = c["S"].copy()
    S[0] = [n - 1, n - 1, 0]                                      # a repeated index stays legal: the iteration is skipped
    _, t = ctx.find_plane(P, c["pose7"], samples3=S, want_trace=True)
    assert np.isinf(t["scores"][0]) and np.array_equal(F.bits(t["scores"][1:]), F.bits(table[name][1]["scores"][1:]))
