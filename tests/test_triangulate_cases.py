"""f2a on its gates (CPU): every scene of triangulate_cases.py reaches what it is named for, the case module's restatement is the oracle
bit for bit, and the oracle agrees with the compiled reference (where built) and with the reference's recorded outputs
(tests/golden/triangulate_cases.npz) under test_triangulate._compare's rule."""
import numpy as np
import pytest
from pathlib import Path

import triangulate_cases as tc
from oracles import orc_triangulate, ref_triangulate

G = Path(__file__).resolve().parent / "golden"


@pytest.mark.parametrize("case_id", tc.CASE_IDS)
def test_restatement_is_the_oracle(case_id):
    c = tc.case(case_id)
    r, o = tc.restate(*tc.inputs(tc.scene(c.scene)), tc.K, c.max_err), tc.oracle(case_id)
    for k in tc.OUT_KEYS:
        assert tc.same_bits(r[k], o[k]), k


@pytest.mark.parametrize("name,gate,other", [("depth_l", "lpt", "rpt"), ("depth_r", "rpt", "lpt")])
def test_depth_sweep_crosses_the_gate(name, gate, other):
    s, st = tc.scene(name), tc.oracle(name)["status"]
    r = tc.restate(*tc.inputs(s))
    z = r[gate][:, 2]
    assert len(st) == 2 * tc.SWEEP and np.array_equal(np.diff(s["step"]), np.ones(len(st) - 1))
    assert set(np.unique(st)) == {0, 1}                          # both sides of the gate, and the reprojection gate plays no part
    assert (st[1:] != st[:-1]).any()                             # a pair of neighbouring steps with different statuses
    assert np.array_equal(st == 1, z < 0.1)                      # ... decided by this depth alone
    assert np.abs(z - 0.1).max() < 300 * np.spacing(0.1) and (z < 0.1).any() and (z >= 0.1).any()
    assert (r[other][:, 2] > 0.19).all() and max(r["ldist"].max(), r["rdist"].max()) < 0.01
    print(name, "rows below / at or above 0.1:", int((z < 0.1).sum()), int((z >= 0.1).sum()), "on 0.1 exactly:", int((z == 0.1).sum()))


@pytest.mark.parametrize("name,dist", [("reproj_l", "ldist"), ("reproj_r", "rdist")])
def test_reproj_sweep_sits_on_the_gate(name, dist):
    s, st = tc.scene(name), tc.oracle(name)["status"]
    r = tc.restate(*tc.inputs(s))
    d, dd, other = r[dist], r[dist + "_d"], r["rdist" if dist == "ldist" else "ldist"]
    me = np.float32(tc.MAX_ERR)
    assert (other == 0).all() and (r["lpt"][:, 2] > 1).all() and (r["rpt"][:, 2] > 1).all()    # only the swept distance decides
    assert np.array_equal(st, np.where(d > me, 2, 0))
    on = np.flatnonzero(d == me)
    assert len(on) >= 8 and (st[on] == 0).all()                  # distance == maxErr exactly: kept
    up = on + 1                                                  # the next row of the same run: one ulp further out
    assert (s["axis"][up] == s["axis"][on]).all() and (s["j"][up] == s["j"][on] + 1).all() and (st[up] == 2).all() and (d[up] > me).all()
    for a in range(4):                                           # along each axis the double norm is 3.0 itself
        row = np.flatnonzero((s["axis"] == a) & (s["j"] == 0))
        assert len(row) == 1 and dd[row[0]] == tc.MAX_ERR and st[row[0]] == 0
        run = np.flatnonzero(s["axis"] == a)
        assert np.array_equal(st[run], np.where(s["j"][run] > 0, 2, 0))
    diag = on[s["axis"][on] == tc.AXES.index("diag")]            # the diagonal's is not: only the cast to float puts it on the gate
    assert (dd[diag] > tc.MAX_ERR).sum() >= 1 and (dd[diag] < tc.MAX_ERR).sum() >= 1 and (dd[diag] != tc.MAX_ERR).all()
    zero = np.flatnonzero(s["axis"] == tc.AXES.index("zero"))
    assert len(zero) == 1 and d[zero[0]] == 0
    if name == "reproj_l":                                       # maxErr = 0 keeps distance 0 and nothing else
        assert np.array_equal(np.flatnonzero(tc.oracle("limit-0-reproj_l")["status"] == 0), zero)


def test_parallel_rows_give_the_nan_and_infinities_they_are_named_for():
    o, r = tc.oracle("parallel"), tc.restate(*tc.inputs(tc.scene("parallel")))
    names = list(tc.PARALLEL)
    for i, k in enumerate(names):
        _, _, _, nan, finite_parallax = tc.PARALLEL[k]
        assert np.isnan(o["lpt"][i]).all() == nan and np.isnan(o["lpt"][i]).any() == nan, k
        assert np.isnan(o["wpt"][i]).all() == nan and np.isnan(o["inv_depth"][i]) == nan, k
        assert np.isfinite(o["parallax"][i]) == finite_parallax, k
        assert (r["det"][i] == 0) == nan, k                      # NaN exactly where the 2 x 2 system is singular
        if nan:
            assert o["status"][i] == 0, k                        # every gate comparison is false
    st = dict(zip(names, o["status"]))
    assert st["diverging_1e-3"] == 1 and o["lpt"][names.index("diverging_1e-3"), 2] < -99
    assert st["diverging_1e-7"] == 1 and st["converging_1e-3"] == 0 and st["ordinary"] == 0
    assert st["zero_baseline"] == 1 and np.isposinf(o["inv_depth"][names.index("zero_baseline")])
    assert st["f2u_z_zero"] == 1 and st["f2u_z_negative"] == 2


def test_sizes_groups_and_limits():
    assert [len(tc.scene(f"scene-{n}")["group"]) for n in tc.SIZES] == [1, 255, 256, 257, 513]
    for n in tc.SIZES[1:]:
        assert set(np.unique(tc.oracle(f"scene-{n}")["status"])) == {0, 1, 2}
    g = tc.scene("groups")
    grp = g["group"]
    assert len(g["T"]) == 8 and np.array_equal(np.flatnonzero(grp == 7), [len(grp) - 1])       # the last block: the last point only
    assert set(np.unique(grp)) == {0, 1, 2, 4, 5, 6, 7} and (np.diff(grp) < 0).any()           # block 3 unused; indices not sorted
    assert set(np.unique(tc.oracle("groups")["status"])) == {0, 1, 2}
    assert tc.LIMITS == (0.0, 3.0, 1e9, float("inf"))
    base = tc.oracle("scene-257")["status"]
    zero, big, inf = (tc.oracle(f"limit-{e}-scene-257")["status"] for e in ("0", "1e+09", "inf"))
    assert np.array_equal(zero == 1, base == 1) and (zero[base != 1] == 2).all()               # 0: every distance is above it
    assert np.array_equal(big, np.where(base == 1, 1, 0)) and np.array_equal(inf, big)         # 1e9, inf: none is
    for c in tc.CASES:
        assert c.id in tc.CASE_IDS and len(tc.scene(c.scene)["group"]) <= 600


@pytest.mark.ref
@pytest.mark.parametrize("case_id", tc.CASE_IDS)
def test_oracle_matches_reference(case_id):
    c = tc.case(case_id)
    s = tc.scene(c.scene)
    ref, T = ref_triangulate(s["pose_kf"], s["pose_new"], s["group"], s["bvl"], s["bvr"], s["unpxl"], s["unpxr"], tc.K, c.max_err)
    assert np.abs(T - s["T"]).max() < 1e-14
    orc = orc_triangulate(T, *tc.inputs(s)[1:], tc.K, c.max_err)
    assert tc.close_to_reference(orc, ref, tc.restate(T, *tc.inputs(s)[1:], tc.K, c.max_err), c.max_err) is None


@pytest.mark.parametrize("case_id", tc.GOLDEN_IDS)
def test_oracle_matches_golden(case_id):
    z = np.load(G / "triangulate_cases.npz")
    c = tc.case(case_id)
    s, want = tc.golden_case(z, case_id)
    for k, v in s.items():                                       # the fixture holds this table's inputs
        assert np.array_equal(v, tc.scene(c.scene)[k], equal_nan=True) if k != "T" else np.abs(v - tc.scene(c.scene)[k]).max() < 1e-14, k
    orc = orc_triangulate(s["T"], s["group"], s["bvl"], s["bvr"], s["unpxl"], s["unpxr"], tc.K, c.max_err)
    assert tc.close_to_reference(orc, want, tc.restate(s["T"], s["group"], s["bvl"], s["bvr"], s["unpxl"], s["unpxr"], tc.K, c.max_err), c.max_err) is None
