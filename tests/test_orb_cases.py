"""CPU: every case of orb_cases.py still reaches the branch of orb.hip's culls it exists for -- asserted from the predictor's counts and
the oracle's keypoints, so that a case that stops reaching its branch fails here instead of passing quietly on the GPU -- and, where the
compiled reference is built, cv::ORB's own result on every case equals the oracle's (its behaviour at ties is what the GPU is held to)."""
import numpy as np
import pytest

import orb_cases as oc
from oracles import Orc, Ref


def test_case_ids():
    assert tuple(c.id for c in oc.cases()) == oc.CASE_IDS and len(set(oc.CASE_IDS)) == len(oc.CASE_IDS)


@pytest.mark.parametrize("nf,scale,nlevels", [(300, 1.2, 8), (500, 1.2, 8), (400, 1.5, 4), (200, 2.0, 2), (250, 1.1, 6), (300, 1.2, 1)])
def test_features_per_level_restates_the_oracle(nf, scale, nlevels):
    """a tie-free image with more candidates than 2 n_l on every level: each level keeps exactly n_l"""
    spec = ("smooth", 640, 480, 1)
    lv = oc.predict(spec, nf, scale, nlevels)
    assert all(v.n1 > 2 * v.n_l > 0 for v in lv), lv
    assert [v.m for v in lv] == oc.features_per_level(nf, scale, nlevels) and sum(v.m for v in lv) == nf


def test_zero_budget_table():
    for nf, want in oc.ZERO_BUDGETS.items():
        assert oc.features_per_level(nf, 1.2, 8) == want, nf


@pytest.mark.parametrize("case_id", oc.CASE_IDS)
def test_case_reaches_its_branch(case_id):
    c = oc.case(case_id)
    kp, desc, lv = oc.oracle(case_id)
    assert len(kp) == sum(v.m for v in lv) < oc.ORACLE_CAP and len(lv) == c.nlevels
    for v in lv:
        assert v.m <= v.n2 <= v.n1 and v.w * v.h // 4 + 64 >= v.n1   # the level's candidate lists have room for all of them
        assert v.m >= min(v.n_l, v.n2)
    l0 = lv[0]
    over = [v.m > oc.launch_bound(v.n_l) for v in lv]
    assert any(over) == (c.group == "bound_over"), lv
    if c.group == "tie_small":
        assert l0.m > l0.n_l and l0.n2 <= oc.RANK_CAP and l0.h <= oc.ROW_CAP, l0        # ties kept by cull_harris_body
    elif c.group == "tie_big":
        assert l0.n2 > oc.RANK_CAP and l0.n_l < l0.m <= oc.SORT_CAP, l0                 # ties kept by cull_harris_big, LDS rank sort
    elif c.group == "tie_levels":
        assert any(v.m > v.n_l > 0 for v in lv), lv
        assert sum(v.m > 0 for v in lv) >= 2, lv
    elif c.group == "bound_at":
        assert l0.n_l == 1 and l0.m == oc.launch_bound(l0.n_l) == 1024, l0
    elif c.group == "bound_over":
        assert l0.n_l == 1 and l0.m == 1089 > oc.launch_bound(l0.n_l), l0
    elif c.group == "split_4096":
        sp, label = oc.split_points(), case_id.split("-", 1)[1]
        assert l0.n_l == c.nf == sp[label] and l0.n1 == sp["n1"]
        if label == "nf_lo":
            assert l0.n2 <= oc.RANK_CAP < l0.n1 and l0.m == l0.n_l, l0                  # the last budget cull_harris_body takes
        elif label == "nf_lo+1":
            assert l0.n2 > oc.RANK_CAP and l0.m == l0.n_l <= oc.SORT_CAP, l0            # the first one cull_harris_big takes
        elif label == "sort_cap":
            assert l0.n2 > oc.RANK_CAP and l0.m == oc.SORT_CAP, l0                      # the most the LDS rank sort orders
        elif label == "sort_cap+1":
            assert l0.n2 > oc.RANK_CAP and l0.m == oc.SORT_CAP + 1, l0                  # the fewest the row buckets order
        elif label in ("n1-1", "n1", "n1+1"):                                          # Harris cull: n = n1 against keepN = n_l
            assert l0.n2 == l0.n1 > oc.SORT_CAP and l0.n1 - l0.n_l == {"n1-1": 1, "n1": 0, "n1+1": -1}[label], l0
            assert l0.m == min(l0.n1, l0.n_l), l0
        else:                                                                          # FAST cull: n = n1 against keepN = 2 n_l
            assert 2 * sp["half"] - l0.n1 in (0, 1)
            assert (l0.n1 > 2 * l0.n_l) == (label == "half-1"), l0
            assert l0.n2 > oc.RANK_CAP and l0.m == l0.n_l, l0
            if label != "half-1":
                assert l0.n2 == l0.n1, l0
    elif c.group == "edge_small":                                                      # the same edges inside cull_harris_body
        ep, label = oc.edge_points(), case_id.split("-", 1)[1]
        assert l0.n_l == c.nf == ep[label] and l0.n1 == ep["n1"] and l0.n2 <= oc.RANK_CAP and l0.h <= oc.ROW_CAP, l0
        assert l0.m == min(l0.n2, l0.n_l) > 0, l0
        if label in ("n1-1", "n1", "n1+1"):
            assert l0.n2 == l0.n1 and l0.n1 - l0.n_l == {"n1-1": 1, "n1": 0, "n1+1": -1}[label], l0
        else:
            assert 2 * ep["half"] - l0.n1 in (0, 1)
            assert (l0.n1 > 2 * l0.n_l) == (label == "half-1") and (l0.n2 == l0.n1) == (label != "half-1"), l0
    elif c.group == "zero_budgets":
        assert [v.n_l for v in lv] == oc.ZERO_BUDGETS[c.nf]
        assert all(v.m == 0 for v in lv if v.n_l == 0) and all(v.m <= v.n_l for v in lv)
        assert any(v.n_l == 0 and v.n1 > 0 for v in lv), lv                             # a zero budget that has candidates to refuse
        if c.nf:
            assert len(kp) > 0 and any(a.n_l == 0 and b.n_l > 0 or a.n_l > 0 and b.n_l == 0 for a, b in zip(lv, lv[1:])), lv
            assert all(v.n1 > 2 * v.n_l for v in lv[:-1]), lv                           # both culls cut (n > keepN) on the levels with a budget
    elif c.group == "tall":
        assert l0.h > oc.ROW_CAP and 0 < l0.m <= l0.n2 <= oc.RANK_CAP, l0               # few candidates, sent to cull_harris_big by its rows
        assert all(v.h <= oc.ROW_CAP for v in lv[1:]) and lv[1].h > 1024
        assert [v.m > 0 for v in lv] == [v.w > 2 * oc.BORDER for v in lv] and sum(v.m > 0 for v in lv) == 3, lv
    else:
        raise AssertionError(c.group)


def test_batch_cases_exceed_the_sort_cap():
    for i, (spec, nf, scale, nlevels) in enumerate(oc.batch_cases()):
        (v,), = [oc.batch_oracle(i)[2]]
        assert nlevels == 1 and v.n_l == nf > oc.SORT_CAP and v.n2 > oc.RANK_CAP and v.m > oc.SORT_CAP, v
    assert oc.batch_oracle(0)[2][0].m == nf < oc.batch_oracle(1)[2][0].m   # the random bytes fill the budget, the tiled image ties above it
    assert len({oc.image(spec).shape for spec, *_ in oc.batch_cases()}) == 1 and len({b[1:] for b in oc.batch_cases()}) == 1


def test_tall_fast_images_carry_over_scan_chunks():
    for i, chunks in ((0, 3), (1, 2)):
        g = oc.tall_fast_image(i)
        xy, sc = Orc.fast(g, 20)
        assert (g.shape[0] + oc.SCAN_ROWS - 1) // oc.SCAN_ROWS == chunks
        assert (xy[:, 1] >= (chunks - 1) * oc.SCAN_ROWS).sum() > 0 and (xy[:, 1] < oc.SCAN_ROWS).sum() > 0   # corners in the first and the last chunk
        assert np.array_equal(np.lexsort((xy[:, 0], xy[:, 1])), np.arange(len(xy)))       # the oracle's order is row-major


@pytest.mark.ref
@pytest.mark.parametrize("case_id", oc.CASE_IDS)
def test_reference_equals_oracle(case_id):
    """cv::ORB itself on every case: the same set, bitwise, in (octave, y, x) order -- its ties included"""
    c = oc.case(case_id)
    kp, desc, _ = oc.oracle(case_id)
    rkp, rd = Ref.orb(oc.image(c.spec), c.nf, scale=c.scale, nlevels=c.nlevels, fast_thr=c.thr, cap=oc.ORACLE_CAP)
    ri = oc.orb_key(rkp)
    assert len(rkp) == len(kp)
    assert np.array_equal(rkp[ri].view(np.uint32), kp.view(np.uint32)) and np.array_equal(rd[ri], desc)


@pytest.mark.ref
def test_reference_equals_oracle_on_the_other_inputs():
    for i in range(len(oc.batch_cases())):
        spec, nf, scale, nlevels = oc.batch_cases()[i]
        kp, desc, _ = oc.batch_oracle(i)
        rkp, rd = Ref.orb(oc.image(spec), nf, scale=scale, nlevels=nlevels, fast_thr=20, cap=oc.ORACLE_CAP)
        ri = oc.orb_key(rkp)
        assert np.array_equal(rkp[ri].view(np.uint32), kp.view(np.uint32)) and np.array_equal(rd[ri], desc), i
    for i in range(2):
        g = oc.tall_fast_image(i)
        (xy, sc), (rxy, rsc) = Orc.fast(g, 20), Ref.fast(g, 20)
        assert np.array_equal(xy, rxy) and np.array_equal(sc, rsc), i
