"""CPU: the rows of tests/klt_cases.py do what they aim at (by the plain-C oracle alone), and -- where the compiled reference is built --
the oracle agrees with it bitwise on every row and on LK pyramids of other windows and depths than 9 / 3."""
import numpy as np
import pytest

import klt_cases as K
from alvaar_amd import synth
from oracles import Orc, Ref, pyr_dims


def _default_case(case):
    return dict(case, args=dict(K.DEFAULT), built=3)


def _tracked_share(status):
    return float(status.astype(bool).mean())


@pytest.mark.parametrize("name", [n for n in K.ROW_NAMES if K.KIND[n] == "crit"])
def test_criteria_rows_change_the_answer_and_keep_tracking(name):
    for case in K.row(name)["cases"]:
        lk, fb = K.lk_result(case), K.fb_result(case)
        assert not K.same_lk(lk, K.lk_result(_default_case(case))), case["name"]
        assert not K.same_fb(fb, K.fb_result(_default_case(case))), case["name"]
        assert 0.05 < _tracked_share(lk[1]) < 0.98 and 0.05 < _tracked_share(fb[1]) < 0.98, case["name"]


def test_default_row_keeps_tracking():
    for case in K.row("default")["cases"]:
        assert 0.05 < _tracked_share(K.lk_result(case)[1]) < 0.98 and 0.05 < _tracked_share(K.fb_result(case)[1]) < 0.98, case["name"]


@pytest.mark.parametrize("name,target", sorted(K.CLAMPED.items()))
def test_clamped_values_equal_their_clamp_targets(name, target):
    for a, b in zip(K.row(name)["cases"], K.row(target)["cases"]):
        assert a["args"] != b["args"] and a["image"] == b["image"]
        assert K.same_lk(K.lk_result(a), K.lk_result(b)) and K.same_fb(K.fb_result(a), K.fb_result(b)), a["name"]


def test_zero_iterations_leave_the_prior():
    """max_iters <= 0 skips the iteration: every point keeps the position it was given (scaled down and up again through the levels: exact)"""
    for case in K.row("iters=0")["cases"]:
        nx, st, _ = K.lk_result(case)
        assert np.array_equal(nx.view(np.uint32), case["init"].view(np.uint32)) and 0 < st.sum() < len(st)


def test_the_oscillation_rule_alone_stops_some_points():
    """max_iters=100 with eps=0: a point stops on a zero step, on the oscillation rule or at the count.  Some run longer than the default
    30 iterations and some stop short of 100, so the rule is what ended them."""
    c = K.row("iters=100,eps=0")["cases"][0]
    _, st, _, deltas, counts = Orc.lk_deltas(c["prev"], c["curr"], c["pts"], c["init"], 3, max_iters=100, eps=0.0)
    last = deltas[np.arange(len(counts)), np.maximum(counts - 1, 0)]
    by_rule = st.astype(bool) & (counts > 1) & (counts < 100) & (last != 0).any(axis=1)
    assert by_rule.sum() > 20 and (counts[by_rule] > 30).any() and (counts == 100).any()


def _verdict_pieces(case):
    """the forward-backward verdict rebuilt from Orc.lk: forward status, err, inBorder of the forward result, backward status, nrm"""
    w, h = K.IMAGES[case["image"]][:2]
    fwd, st, err = K.lk_result(_default_case(case))
    back, bst, _ = Orc.lk(case["curr"], case["prev"], fwd, case["pts"], 0)
    d = (case["pts"] - back).astype(np.float32).astype(np.float64)
    nrm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    inb = (fwd[:, 0] >= 1) & (fwd[:, 0] < np.float32(w) - 1) & (fwd[:, 1] >= 1) & (fwd[:, 1] < np.float32(h) - 1)
    return st.astype(bool), err, inb, bst.astype(bool), nrm


def _verdict(case, err_thresh, fb_dist):
    st, err, inb, bst, nrm = _verdict_pieces(case)
    return st & ~(err > np.float32(err_thresh)) & inb & bst & ~(nrm > float(np.float32(fb_dist)))


@pytest.mark.parametrize("name", [n for n in K.ROW_NAMES if K.KIND[n] == "gate"])
def test_gate_rows_accept_exactly_the_points_the_thresholds_admit(name):
    r = K.row(name)
    e, f = r["args"]["err_thresh"], r["args"]["fb_dist"]
    for case in r["cases"]:
        pr, st = K.fb_result(case)
        want = _verdict(case, e, f)
        assert np.array_equal(st.astype(bool), want), case["name"]
        assert not K.same_fb((pr, st), K.fb_result(_default_case(case))), case["name"]
        if e == 0.0 or f == 0.0:
            assert st.sum() == 0        # err is a positive eigenvalue, and no backward pass returns to the keypoint's very bits here
        elif np.isinf(e):
            s, _, inb, bst, _ = _verdict_pieces(case)
            assert st.sum() == (s & inb & bst).sum() > K.fb_result(_default_case(case))[1].sum()
        else:
            assert 0 < st.sum() < len(st)


@pytest.mark.parametrize("gate", ["err", "fb"])
@pytest.mark.parametrize("k", range(K.N_TIES))
def test_tie_rows_flip_exactly_the_intended_point(gate, k):
    point, at, below = K.ties()[gate][k]
    assert below < at and np.nextafter(below, np.float32(np.inf)) == at
    ra, rb = K.row("tie-%s-%d-at" % (gate, k)), K.row("tie-%s-%d-below" % (gate, k))
    ca, cb = ra["cases"][0], rb["cases"][0]
    assert ca["image"] == cb["image"] == K.TIE_IMAGE
    key = "err_thresh" if gate == "err" else "fb_dist"
    assert ra["args"][key] == float(at) and rb["args"][key] == float(below)
    (pa, sa), (pb, sb) = K.fb_result(ca), K.fb_result(cb)
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    assert np.flatnonzero(sa != sb).tolist() == [point] and sa[point] == 1 and sb[point] == 0
    st, err, inb, bst, nrm = _verdict_pieces(ca)
    if gate == "err":
        assert err[point] == at                         # the gate at equality
    else:
        assert float(below) < nrm[point] <= float(at)
    for r in (ra, rb):                                   # and every case of the row is the verdict at that threshold
        for case in r["cases"]:
            assert np.array_equal(K.fb_result(case)[1].astype(bool), _verdict(case, r["args"]["err_thresh"], r["args"]["fb_dist"])), case["name"]


def test_one_fb_tie_sits_at_equality():
    """the first forward-backward tie is a point whose nrm is itself a float: fb_dist == nrm passes, the float below fails"""
    point, at, _ = K.ties()["fb"][0]
    nrm = _verdict_pieces(K.row("default")["cases"][0])[4]
    assert nrm[point] == float(at)


@pytest.mark.parametrize("k", range(K.N_BANDS))
def test_band_rows_decide_inside_the_float_band(k):
    key, levels, point, trio = K.bands()[k]
    assert trio[0] < trio[1] < trio[2] and np.nextafter(trio[0], trio[2]) == trio[1] and np.nextafter(trio[1], trio[2]) == trio[2]
    rows = [K.row("band-%d-%s" % (k, s)) for s in ("lo", "mid", "hi")]
    cases = [r["cases"][0] for r in rows]
    assert all(c["image"] == key and r["args"]["num_levels"] == levels and r["args"]["eps"] == float(e) for c, r, e in zip(cases, rows, trio))
    # with eps itself the point takes a step on level 0 whose length rounds to eps: |delta|^2 is within 2^-23 of (double) eps^2, the
    # 64-lane layout's float test cannot tell them apart (its band is +-1e-5) and the comparison in double decides
    c = cases[1]
    _, _, _, deltas, counts = Orc.lk_deltas(c["prev"], c["curr"], c["pts"], c["init"], levels, eps=float(trio[1]))
    d = deltas[point, :counts[point]].astype(np.float64)
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    hit = np.float32(np.sqrt(d2)) == trio[1]
    assert hit.any()
    assert (np.abs(d2[hit] / float(trio[1]) ** 2 - 1) < 2.0 ** -22).all()
    res = [K.lk_result(c) for c in cases]
    bits = [(r[0][point].view(np.uint32).tolist(), int(r[1][point])) for r in res]
    assert bits[0] != bits[1] or bits[1] != bits[2]
    assert not K.same_lk(res[0], res[2])
    for r in res:
        assert 0.05 < _tracked_share(r[1]) < 0.98


def test_band_rows_come_from_several_points_and_both_depths():
    b = K.bands()
    assert len(b) >= 5 and len({(key, point) for key, _, point, _ in b}) == len(b) and {lv for _, lv, _, _ in b} == {0, 3}


DEPTH_DIMS = {"d200": [(200, 152), (100, 76), (50, 38), (25, 19), (13, 10)], "c64": [(64, 48), (32, 24), (16, 12)],
              "e1156": [(1156, 1156), (578, 578), (289, 289), (145, 145), (73, 73), (37, 37), (19, 19), (10, 10)]}


@pytest.mark.parametrize("name", K.DEPTHS)
def test_depth_rows_have_the_stated_levels(name):
    r = K.row(name)
    L = r["args"]["num_levels"]
    assert sorted({(c["image"], c["built"]) for c in r["cases"]}) == sorted([(k, b) for k in K.DEPTH_IMAGES for b in K.BUILT] + [("e1156", 7)])
    by_depth = {}
    for case in r["cases"]:
        dims = K.levels_built(case)
        full = DEPTH_DIMS[case["image"]]
        assert dims == full[:case["built"] + 1]                     # the `<= win` rule cuts 200 x 152 after 13 x 10, 64 x 48 after 16 x 12
        assert min(full[-1]) < 16 <= min(full[-2])                   # only the top level is smaller than the 16 x 16 search tile
        top = min(L, len(dims) - 1)
        lk, fb = K.lk_result(case), K.fb_result(case)
        assert 0.05 < _tracked_share(lk[1]) < 0.98 and 0.05 < _tracked_share(fb[1]) < 0.98, case["name"]
        # the level the search starts on is min(num_levels, built levels - 1): the same start gives the same bits whatever was asked for
        # and built, another start gives others
        by_depth.setdefault((case["image"], top), []).append((lk, fb))
    for (key, top), rs in by_depth.items():
        for lk, fb in rs[1:]:
            assert K.same_lk(lk, rs[0][0]) and K.same_fb(fb, rs[0][1]), (key, top)
    for key in K.DEPTH_IMAGES:
        tops = sorted(t for k, t in by_depth if k == key)
        for a, b in zip(tops, tops[1:]):
            assert not K.same_lk(by_depth[key, a][0][0], by_depth[key, b][0][0]), (key, a, b)
    if L == 7:
        assert sorted(t for k, t in by_depth if k == "d200") == [0, 1, 2, 4] and sorted(t for k, t in by_depth if k == "c64") == [0, 1, 2]
        assert [t for k, t in by_depth if k == "e1156"] == [7]       # all eight levels a pyramid can hold


def test_eight_level_case_differs_by_start_level():
    res = [K.lk_result(next(c for c in K.row(name)["cases"] if c["image"] == "e1156")) for name in K.DEPTHS]
    assert not K.same_lk(res[0], res[1]) and not K.same_lk(res[1], res[2]) and not K.same_lk(res[0], res[2])


def test_row_table_is_complete():
    assert len(K.ROW_NAMES) == len(set(K.ROW_NAMES)) == 1 + 16 + 7 + 4 * K.N_TIES + 3 * K.N_BANDS + 3
    for name in K.ROW_NAMES:
        r = K.row(name)
        assert set(r["args"]) == set(K.DEFAULT) and np.isfinite(r["args"]["eps"])
        for c in r["cases"]:
            assert 300 <= len(c["pts"]) <= 2000 and np.isfinite(c["pts"]).all() and np.isfinite(c["init"]).all()
            w, h = K.IMAGES[c["image"]][:2]
            x, y = c["pts"][:, 0], c["pts"][:, 1]
            inside = (x > 5) & (x < w - 5) & (y > 5) & (y < h - 5)
            outside = (x < 0) | (x > w - 1) | (y < 0) | (y > h - 1)
            assert inside.sum() > 100 and outside.sum() > 5 and (~inside & ~outside).sum() > 5       # inside, outside and on the border


# ---- against the compiled reference ------------------------------------------------------------------------------------------------------
@pytest.mark.ref
@pytest.mark.parametrize("name", K.ROW_NAMES)
def test_oracle_equals_reference_on_every_row(name):
    for case in K.row(name)["cases"]:
        if name in K.LK_ROW_NAMES:
            assert K.same_lk(K.lk_result(case), K.lk_result(case, Ref)), case["name"]
        assert K.same_fb(K.fb_result(case), K.fb_result(case, Ref)), case["name"]


PYR_SIZES = [(200, 152), (64, 48), (36, 28)]
PYR_DEEP = (1156, 1156, 9, 7)           # the smallest size with all eight levels at the tracker's window
PYR_WINS = [3, 5, 7, 12, 15]
PYR_DEPTHS = [0, 5, 7]


def pyr_frame(w, h, k):
    """frame k of the pyramid tests' stream at that size"""
    return synth.frame_gray(synth.texture_canvas(w, h, seed=w + h, margin=64), 3 + k, w, h, noise_seed=11)


@pytest.mark.ref
@pytest.mark.parametrize("w,h", PYR_SIZES)
@pytest.mark.parametrize("win", PYR_WINS)
def test_pyramid_other_windows_and_depths_bit_exact(w, h, win):
    g = pyr_frame(w, h, 0)
    for depth in PYR_DEPTHS:
        og, od = Orc.build_pyramid(g, win, depth)
        rg, rd = Ref.build_pyramid(g, win, depth)     # (asserts that the reference built as many levels as pyr_dims says)
        assert len(og) == len(rg) == len(pyr_dims(w, h, win, depth))
        for l in range(len(og)):
            assert np.array_equal(og[l], rg[l]), (depth, "gray", l)
            assert np.array_equal(od[l], rd[l]), (depth, "deriv", l)


@pytest.mark.ref
def test_pyramid_of_eight_levels_bit_exact():
    w, h, win, depth = PYR_DEEP
    g = pyr_frame(w, h, 0)
    og, od = Orc.build_pyramid(g, win, depth)
    rg, rd = Ref.build_pyramid(g, win, depth)
    assert len(og) == len(rg) == 8
    assert len(pyr_dims(w - 4, h, win, depth)) == 7        # four columns fewer and the eighth level is 9 wide: not built
    for l in range(8):
        assert np.array_equal(og[l], rg[l]) and np.array_equal(od[l], rd[l]), l


def test_pyramid_sizes_stop_by_the_window_rule():
    assert [len(pyr_dims(36, 28, win, 7)) for win in PYR_WINS] == [4, 3, 2, 2, 1]
    assert [len(pyr_dims(200, 152, win, 7)) for win in PYR_WINS] == [6, 5, 5, 4, 4]
    assert [len(pyr_dims(64, 48, win, 5)) for win in PYR_WINS] == [4, 4, 3, 2, 2]
