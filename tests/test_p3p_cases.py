"""CPU: the P3P-LMedS hypothesis table (tests/p3p_cases.py) against the plain-C checker alone -- every case reaches the property it
exists for, the two halves of one LMedS iteration (orc_p3p_model, orc_p3p_penalty) replayed hypothesis by hypothesis give the result of
orc_p3p_lmeds, and the table's models are stable enough for the 1e-8 comparison tests/test_gpu_p3p_hypotheses.py makes."""
import numpy as np
import pytest

import p3p_cases as PC
from oracles import Orc


@pytest.mark.parametrize("case", PC.CASES, ids=[c["name"] for c in PC.CASES])
def test_case_reaches_its_property(case):
    b, o = PC.build(case), PC.checker(case)
    r = o["replay"]
    print(case["name"], "valid", int(o["valid"].sum()), "of", b["H"], "distinct penalties", len(np.unique(o["penalty"][o["valid"]])), r)
    assert b["samples"].shape == (case["H"], 4) and b["samples"].min() >= 0 and b["samples"].max() < case["n"]
    assert b["bv"].shape == b["wpt"].shape == (case["n"], 3)
    assert PC.PROPS[case["prop"]](b, o, r), (case["name"], case["prop"])


def test_table_covers_the_sizes():
    """the sizes at which the kernels change path; odd and even n both occur"""
    ns = {c["n"] for c in PC.CASES}
    Hs = {c["H"] for c in PC.CASES}
    assert {4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 7168, 7169, 19000} <= ns
    assert {1, 4, 63, 64, 65, 192, 193, 256, 257, 300} <= Hs
    assert {(c["n"] > 7168, c["H"] > 192) for c in PC.CASES if c["n"] == 7169} == {(True, False), (True, True)}
    assert sum(c["prod"] for c in PC.CASES) >= 3 and any(c["prod"] and c["n"] > 7168 for c in PC.CASES)
    assert all(PC.BY_NAME[k]["n"] <= 7168 for k in PC.BATCH_TRIO) and len({PC.BY_NAME[k]["H"] for k in PC.BATCH_TRIO}) == 3


def test_repeated_index_invalidates_only_among_the_first_three():
    b = PC.build("n257_H192")
    i, j, k, l = (int(v) for v in b["samples"][0])
    assert Orc.p3p_model(b["bv"], b["wpt"], [i, j, k, l])[0]
    for s in ([i, i, k, l], [i, j, j, l], [i, j, i, l]):
        assert not Orc.p3p_model(b["bv"], b["wpt"], s)[0], s
    for s in ([i, j, k, i], [i, j, k, k]):
        assert Orc.p3p_model(b["bv"], b["wpt"], s)[0], s


@pytest.mark.parametrize("name", [c["name"] for c in PC.CASES if c["prod"]] + ["coincident"])
def test_halves_replayed_equal_the_whole(name):
    """orc_p3p_lmeds is made of orc_p3p_model + orc_p3p_penalty: their replay over the stream gives its model bit for bit and its
    outlier list.  (`coincident`: the loop skips samples without a model, the replay does the same over a longer prefix.)"""
    b = PC.build(name)
    it = b["max_iters"]
    samples = b["samples"] if PC.BY_NAME[name]["prod"] else Orc.p3p_draw_samples(b["n"], 11 * it)
    o = PC.oracle_eval(b["bv"], b["wpt"], samples)
    r = PC.replay(o["valid"], o["penalty"], it)
    assert r["used"] == it
    ok, R, t, out = Orc.p3p_lmeds(b["bv"], b["wpt"], max_iters=it)
    m = o["models"][r["best"]]
    _, inl, k = Orc.p3p_penalty(m, b["bv"], b["wpt"], Orc.p3p_threshold())
    assert k == int(inl.sum())
    assert ok and np.array_equal(R.ravel().view(np.uint64), m[:9].view(np.uint64)) and np.array_equal(t.view(np.uint64), m[9:].view(np.uint64))
    assert np.array_equal(out, np.flatnonzero(inl == 0))


def test_nan_key_counts_as_inf():
    b = PC.build("n5_H128")
    m = np.full(12, np.nan)
    pen, inl, k = Orc.p3p_penalty(m, b["bv"], b["wpt"], Orc.p3p_threshold())
    assert pen == np.inf and k == 0 and not inl.any()


def test_models_move_less_than_the_tolerance_under_one_ulp():
    """Assertion (b) of the GPU test allows SKIP_CAP of the valid hypotheses to differ from the checker by more than MODEL_TOL.  That
    the table is inside this cap is shown here by the checker alone: every input moved by one ulp (coincident points stay coincident)
    changes no hypothesis' validity and moves no more than that share of the checker's own models by more than MODEL_TOL."""
    total = moved = 0
    worst = 0.0
    for case in PC.CASES:
        o, p = PC.checker(case), PC.checker(case, ulp=True)
        both = o["valid"] & p["valid"]
        assert np.array_equal(o["valid"], p["valid"]), case["name"]
        d = np.abs(o["models"][both] - p["models"][both]).max(axis=1) if both.any() else np.zeros(0)
        total += int(both.sum())
        moved += int((d > PC.MODEL_TOL).sum())
        worst = max(worst, float(d.max()) if len(d) else 0.0)
    print("valid hypotheses", total, "moved by more than", PC.MODEL_TOL, ":", moved, "largest move", worst)
    assert total > 2000
    assert moved <= PC.SKIP_CAP * total
