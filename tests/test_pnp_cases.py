"""CPU: the PnP branch table (tests/pnp_cases.py).  Every case takes the minimiser path it is named for, by the plain-C checker's trace
(orc_pnp_refine_trace); the traced call returns exactly what orc_pnp_refine returns; no decision of any case is close; and, marked `ref`,
the checker equals the compiled reference -- Ceres itself -- on every case: same path iteration by iteration, same outliers, same counts."""
import numpy as np
import pytest

import pnp_cases as PC
from oracles import Orc, Ref

IDS = [c["name"] for c in PC.CASES]


@pytest.fixture(scope="module")
def orc_runs():
    """name -> (built problem, (ok, pose, outliers, info, trace)) of the checker, computed once"""
    runs = {}
    for c in PC.CASES:
        b = PC.build(c)
        runs[c["name"]] = (b, Orc.pnp_refine_trace(b["uv"], b["wpt"], b["pose_init"], b["K"], **b["kw"]))
    return runs


def test_table_names_are_unique_and_cover_the_branches():
    assert len(set(IDS)) == len(IDS)
    assert {c["branch"] for c in PC.CASES} == set(PC.BRANCHES)
    for c in PC.CASES:
        n = c["gen"]["n"]
        assert 37 <= n <= 600, c["name"]


@pytest.mark.parametrize("case", PC.CASES, ids=IDS)
def test_case_reaches_its_branch(case, orc_runs):
    b, (ok, pose, out, info, tr) = orc_runs[case["name"]]
    n = len(b["uv"])
    sig = PC.signature(tr)
    print(case["name"], sig, "ok", ok, "outliers", len(out), "/", n)
    assert np.isfinite(b["uv"]).all() and np.isfinite(b["wpt"]).all() and np.isfinite(b["pose_init"]).all()
    assert PC.BRANCHES[case["branch"]](ok, out, n, tr), (case["name"], sig)
    assert sig == case["sig"]
    for mod in case["mods"]:
        if mod[0] == "behind":   # the mirrored points, and only they, are outliers: by depth alone (their chi2 is an inlier's)
            assert list(out) == list(mod[1]) and (tr["chi2"][list(mod[1])] < PC.CHI2_TH).all()
    # the trace and info[] tell the same story: summaries = 1 + decisions that were judged (a tolerance exit pushes none), successes = 1 + accepted
    for k, s in enumerate(tr["solves"]):
        if s["exit"] == "not_run":
            assert not info[4 * k:4 * k + 4].any()
            continue
        assert info[4 * k] == 1 + sum(kd != "tolerance" for kd in s["kinds"])
        assert info[4 * k + 3] == 1 + s["kinds"].count("accepted")
        assert (s["mcc"] > 0).all() or "invalid" in s["kinds"]
        rejected = np.array([kd == "rejected" for kd in s["kinds"]], bool)
        assert (s["rel"][rejected] <= PC.REL_MIN).all()
        # a retry after a rejection runs with the radius divided by 2, 4, 8, ... (levenberg_marquardt_strategy.cc:148-153)
        factor = 2.0
        for i in range(1, len(s["kinds"])):
            if s["kinds"][i - 1] in ("rejected", "invalid"):
                assert s["radius"][i] == s["radius"][i - 1] / factor
                factor *= 2
            else:
                factor = 2.0


def test_reject_final_verdicts_come_from_the_rejected_candidate(orc_runs):
    """`reject_final`: the same call stopped one iteration earlier ends on the accepted pose, where every point is an outlier -> false.
    With the rejected fifth step the verdicts are the candidate's: one point is not an outlier, the call goes on into the second solve."""
    case = next(c for c in PC.CASES if c["name"] == "reject_final")
    b, (ok, pose, out, info, tr) = orc_runs["reject_final"]
    first_rejected = tr["solves"][0]["kinds"].index("rejected")
    ok1, pose1, out1, _ = Orc.pnp_refine(b["uv"], b["wpt"], b["pose_init"], b["K"], **dict(b["kw"], max_iters=first_rejected))
    assert not ok1 and len(out1) == len(b["uv"])
    assert ok and len(out) == len(b["uv"]) - 1


@pytest.mark.parametrize("case", PC.CASES, ids=IDS)
def test_traced_call_returns_what_the_plain_call_returns(case, orc_runs):
    b, (ok, pose, out, info, tr) = orc_runs[case["name"]]
    ok2, pose2, out2, info2 = Orc.pnp_refine(b["uv"], b["wpt"], b["pose_init"], b["K"], **b["kw"])
    assert ok == ok2 and np.array_equal(out, out2)
    assert np.array_equal(pose.view(np.uint64), pose2.view(np.uint64)) and np.array_equal(info.view(np.uint64), info2.view(np.uint64))


@pytest.mark.parametrize("case", PC.CASES, ids=IDS)
def test_margins(case, orc_runs):
    """(c) no rel near 1e-3, no cost change near the function tolerance, no chi2 near the threshold"""
    _, (ok, pose, out, info, tr) = orc_runs[case["name"]]
    m = PC.margins(tr)
    print(case["name"], "rel %.3e ftol %.3e chi2 %.3e" % (m["rel"], m["ftol"], m["chi2"]), "NEAR", PC.NEAR)
    assert m["rel"] >= PC.NEAR and m["ftol"] >= PC.NEAR and m["chi2"] >= PC.NEAR


def deviations(to, tr, info_o, info_r):
    """largest relative differences checker vs reference in what the decisions are taken on (pnp_cases' docstring)"""
    d = dict(cost=0.0, rel=0.0, chi2=0.0)
    for k, (so, sr) in enumerate(zip(to["solves"], tr["solves"])):
        m = len(sr["kinds"])
        if so["exit"] != "not_run":
            d["cost"] = max(d["cost"], abs(info_o[4 * k + 1] - info_r[4 * k + 1]) / info_r[4 * k + 1] if info_r[4 * k + 1] else 0.0,
                            abs(info_o[4 * k + 2] - info_r[4 * k + 2]) / info_r[4 * k + 1] if info_r[4 * k + 1] else 0.0)
        if m:
            # Ceres records the candidate's cost for a judged iteration, the unchanged cost for an invalid one: cand_cost in both cases
            d["cost"] = max(d["cost"], float(np.max(np.abs(so["cand_cost"][:m] - sr["cost"]) / so["x_cost"][:m])))
            j = [i for i, kd in enumerate(sr["kinds"]) if kd != "invalid"]
            d["rel"] = max(d["rel"], float(np.max(np.abs(so["rel"][j] - sr["rel"][j]) / np.maximum(np.abs(sr["rel"][j]), PC.REL_MIN), initial=0.0)))
    if len(to["chi2"]):
        d["chi2"] = float(np.max(np.abs(to["chi2"] - tr["chi2"]) / PC.CHI2_TH))
    return d


@pytest.mark.ref
def test_checker_equals_reference(orc_runs):
    """(b) on every case: ok, the outlier list, both solves' summary and success counts, and the path itself -- accepted / rejected /
    invalid per iteration, the termination class -- are Ceres'; costs and pose within test_oracle_vs_ref.py::test_pnp_refine's tolerances.
    Also measures how far the two are apart in the decision quantities: 100 x that is pnp_cases.NEAR."""
    worst = dict(cost=0.0, rel=0.0, chi2=0.0)
    term_of = dict(max_iterations=1, gradient=0, radius=0, parameter_tolerance=0, function_tolerance=0, invalid_steps=2, not_run=None)
    for case in PC.CASES:
        name = case["name"]
        b, (ok, pose, out, info, tr) = orc_runs[name]
        ok2, pose2, out2, info2, tr2 = Ref.pnp_refine_trace(b["uv"], b["wpt"], b["pose_init"], b["K"], **b["kw"])
        assert ok == ok2, name
        assert np.array_equal(out, out2), name
        assert all(info[i] == info2[i] for i in (0, 3, 4, 7)), (name, info, info2)
        for so, sr in zip(tr["solves"], tr2["solves"]):
            assert [kd for kd in so["kinds"] if kd != "tolerance"] == sr["kinds"], (name, so["kinds"], sr["kinds"])
            assert term_of[so["exit"]] == sr["termination"], (name, so["exit"], sr["termination"])
        assert np.allclose(info[[1, 2, 5, 6]], info2[[1, 2, 5, 6]], rtol=1e-9), (name, info, info2)
        if len(out) < len(b["uv"]):   # (all outliers: ceresPnP returns before it writes the pose)
            assert np.abs(pose - pose2).max() < 1e-9, name
        d = deviations(tr, tr2, info, info2)
        print("%-26s cost %.2e rel %.2e chi2 %.2e" % (name, d["cost"], d["rel"], d["chi2"]))
        for key in worst:
            worst[key] = max(worst[key], d[key])
    print("largest deviations", worst, "MEASURED_DEV", PC.MEASURED_DEV)
    assert max(worst.values()) <= PC.MEASURED_DEV


@pytest.mark.ref
def test_reference_trace_entry_returns_what_the_plain_entry_returns():
    case = next(c for c in PC.CASES if c["name"] == "reject_solve_2")
    b = PC.build(case)
    a = Ref.pnp_refine(b["uv"], b["wpt"], b["pose_init"], b["K"], **b["kw"])
    t = Ref.pnp_refine_trace(b["uv"], b["wpt"], b["pose_init"], b["K"], **b["kw"])
    assert a[0] == t[0] and np.array_equal(a[1], t[1]) and np.array_equal(a[2], t[2]) and np.array_equal(a[3], t[3])
