"""GPU: P3P-LMedS hypothesis by hypothesis (alva_p3p_hypotheses) over the table of tests/p3p_cases.py, on both launch routes -- route 0
the single-problem launch of alva_p3p_lmeds (k_p3p_s up to H = 192, k_p3p above), route 1 the batched tracker's three launches
(k_p3p_hyp_batch / k_p3p_batch / k_p3p_select_batch).  test_gpu_pose.py and the track-batch tests see the winner only; here every
hypothesis' validity, model, LMedS penalty and inlier mask and the selection's replay are checked:

  a  valid[h] is the checker's, exactly
  b  |model - checker's model| < 1e-8 (test_gpu_pose.py's P3P_TOL); a hypothesis beyond it is counted and skipped in (b) only, and over
     the whole table at most 1 % of the valid hypotheses may be (test_p3p_cases.py shows with the checker alone that one ulp on the
     inputs moves 6 of the table's 4552 models that far)
  c  penalty[h] == the checker's penalty OF THE DEVICE'S OWN MODEL, bit for bit, and mask h == its inlier vector, bits from n on zero:
     the same IEEE operations in the same order on both sides (-ffp-contract=off) -- the radix select, its early exit, the even-n
     pass and the ballots, without a tolerance
  d  best / n_valid_used / have_model == the sequential replay of the device's own valid[] and penalty[]; the selected model is row
     `best` bitwise, the inlier bytes are its mask (route 0) / the checker's vector (route 1), n_inliers their count
  e  route 1 == route 0 bit for bit
  f  alva_p3p_lmeds on the same problem returns that model and the complement of that inlier set
  g  a repeated call gives identical bytes whatever ran in between; the arrival counter is back at zero after every call
  h  bad arguments are rejected and the context works afterwards

Measured on an MI355X: (b) skipped 2 of 4552 valid hypotheses on route 0 and the same 2 of 4248 on route 1 -- one of `invalid_edges`
(2.6e-8 from the checker) and one of `even_keys_equal`, whose fourth point repeats a point of its triple, so that the four candidate
poses explain it equally well and rounding picks (9.8 from the checker's pick).  (c) needed no tolerance anywhere.

The assertions bite: on a scratch build, flipping the selection's tie-break (`oi < bi` -> `oi > bi`) fails 16 of these tests (the n = 4 / 5,
coincident, noise-free, dup_same_round, dup_lane_order and even_keys_equal cases on both routes); letting the cap in one hypothesis late
(`before < max_iters` -> `<=`) fails 7 (n64_H4, cap_mid_round, cap_after_invalid on both routes and the batch of three); counting keys
`<=` instead of `<` the median key in the even-n pass fails 32.  `ctot == mid` -> `>=` in that pass fails none and cannot: ctot counts
the keys below the key of rank mid, so it never exceeds mid and the two comparisons are the same predicate."""
import numpy as np
import pytest

import p3p_cases as PC
from oracles import Orc

pytestmark = pytest.mark.gpu

IDS = [c["name"] for c in PC.CASES]
BATCHABLE = [c["name"] for c in PC.CASES if c["n"] <= 7168]
FIELDS = ("models", "valid", "penalty", "inlier", "model")
SELECTION = ("best", "n_valid_used", "have_model", "n_inliers")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.fixture(scope="module")
def dev():
    """the cases' arrays on the device, uploaded once"""
    import torch
    return {name: (torch.from_numpy(PC.build(name)["bv"].copy()).cuda(), torch.from_numpy(PC.build(name)["wpt"].copy()).cuda()) for name in IDS}


def _run(ctx, dev, names, route):
    pbs = []
    for name in names:
        b = PC.build(name)
        pbs.append(dict(bv=dev[name][0], wpt=dev[name][1], samples=b["samples"], max_iters=b["max_iters"]))
    return dict(zip(names, ctx.p3p_hypotheses(pbs, err=PC.ERR, fx=PC.FX, fy=PC.FY, route=route)))


@pytest.fixture(scope="module")
def route0(ctx, dev):
    """every case through the single-problem launch, one call"""
    return _run(ctx, dev, IDS, 0)


@pytest.fixture(scope="module")
def route1(ctx, dev):
    """every case the batch accepts (n <= 7168) as ONE batch: 31 problems of different n and H"""
    return _run(ctx, dev, BATCHABLE, 1)


_pen_cache = {}


def _checker_penalty(name, h, model):
    """Orc.p3p_penalty of a device model, once per distinct model (route 1's models are route 0's when (e) holds)"""
    key = (name, h, model.tobytes())
    if key not in _pen_cache:
        b = PC.build(name)
        _pen_cache[key] = Orc.p3p_penalty(model, b["bv"], b["wpt"], Orc.p3p_threshold(PC.ERR, PC.FX, PC.FY))
    return _pen_cache[key]


def _model_skips(name, got):
    """(b): (valid hypotheses, those whose model is further than MODEL_TOL from the checker's)"""
    o = PC.checker(name)
    v = o["valid"]
    d = np.abs(got["models"][v] - o["models"][v]).max(axis=1) if v.any() else np.zeros(0)
    return int(v.sum()), int((~(d < PC.MODEL_TOL)).sum()), float(d.max()) if len(d) else 0.0


def _unpack(mask_row, n):
    bits = np.unpackbits(mask_row.view(np.uint8), bitorder="little")
    return bits[:n], bits[n:]


def _assert_case(name, got, route):
    b, o = PC.build(name), PC.checker(name)
    n, H = b["n"], b["H"]
    tag = (name, route)
    assert got["counter_after"] == 0, tag
    # a
    assert np.array_equal(got["valid"] != 0, o["valid"]), (tag, np.flatnonzero((got["valid"] != 0) != o["valid"]))
    # b (the cap over the table: test_model_skips_within_cap)
    nv, skipped, worst = _model_skips(name, got)
    print(name, "route", route, "valid", nv, "of", H, "models beyond", PC.MODEL_TOL, ":", skipped, "largest difference", worst)
    # c
    for h in range(H):
        if not got["valid"][h]:
            assert got["penalty"][h] == np.inf and not got["models"][h].any(), (tag, h)
            assert route == 1 or not got["masks"][h].any(), (tag, h)
            continue
        pen, inl, _ = _checker_penalty(name, h, got["models"][h])
        assert _bits(got["penalty"][h:h + 1])[0] == _bits(np.array([pen]))[0], (tag, h, got["penalty"][h], pen)
        if route == 0:
            head, tail = _unpack(got["masks"][h], n)
            assert np.array_equal(head, inl), (tag, h, np.flatnonzero(head != inl))
            assert not tail.any(), (tag, h)
    # d
    r = PC.replay(got["valid"] != 0, got["penalty"], b["max_iters"])
    print(name, "route", route, "selection", {k: got[k] for k in SELECTION}, "replay", r)
    assert (got["best"], got["n_valid_used"], got["have_model"]) == (r["best"], r["used"], r["have_model"]), tag
    if r["have_model"]:
        best = r["best"]
        assert np.array_equal(_bits(got["model"]), _bits(got["models"][best])), tag
        want = _unpack(got["masks"][best], n)[0] if route == 0 else _checker_penalty(name, best, got["models"][best])[1]
        assert np.array_equal(got["inlier"], want), (tag, np.flatnonzero(got["inlier"] != want))
        assert got["n_inliers"] == int(want.sum()), tag
    else:
        assert got["n_inliers"] == 0 and got["best"] == -1, tag


def _assert_same_bytes(a, b, tag, masks=False):
    for k in FIELDS + (("masks",) if masks else ()):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (tag, k)
    assert all(a[k] == b[k] for k in SELECTION), (tag, {k: (a[k], b[k]) for k in SELECTION})


@pytest.mark.parametrize("name", IDS)
def test_single_launch(route0, name):
    """(a) - (d) on route 0"""
    _assert_case(name, route0[name], 0)


@pytest.mark.parametrize("name", BATCHABLE)
def test_batch_launch(route0, route1, name):
    """(a) - (d) on route 1, and (e): the batch's bits are the single launch's.  (Where there is no model the selection writes neither
    the model nor the inlier bytes; they are compared where there is one.)"""
    _assert_case(name, route1[name], 1)
    a, c = route0[name], route1[name]
    if a["have_model"] and c["have_model"]:
        _assert_same_bytes(a, c, name)
    else:
        for k in ("models", "valid", "penalty"):
            assert np.array_equal(_bits(a[k]), _bits(c[k])), (name, k)
        assert all(a[k] == c[k] for k in SELECTION), name


def test_batch_of_three_sizes(ctx, dev, route0):
    """Three problems of different n and H in one batch: workgroups beyond a problem's H leave at once, LDS is sized for the largest n
    -- the same bits as each problem alone."""
    got = _run(ctx, dev, list(PC.BATCH_TRIO), 1)
    for name in PC.BATCH_TRIO:
        _assert_case(name, got[name], 1)
        _assert_same_bytes(route0[name], got[name], name)


def test_model_skips_within_cap(route0, route1):
    """(b) over the table, per route: at most SKIP_CAP of the valid hypotheses differ from the checker's model by more than MODEL_TOL"""
    for route, res in ((0, route0), (1, route1)):
        counts = [_model_skips(name, got) for name, got in res.items()]
        total, skipped = sum(c[0] for c in counts), sum(c[1] for c in counts)
        print("route", route, "valid hypotheses", total, "models beyond", PC.MODEL_TOL, ":", skipped,
              {name: c[1] for (name, _), c in zip(res.items(), counts) if c[1]})
        assert total > 2000 and skipped <= PC.SKIP_CAP * total, (route, skipped, total)


@pytest.mark.parametrize("name", [c["name"] for c in PC.CASES if c["prod"]])
def test_production_call_returns_the_instrument_s_winner(ctx, dev, route0, name):
    """(f) alva_p3p_lmeds draws max_iters + 28 samples of the seed-12345 stream -- the rows the table gave the instrument -- and must
    return the selected model's R, t bitwise and the complement of the inlier bytes"""
    import alvaar_amd
    b, got = PC.build(name), route0[name]
    drawn = np.zeros((b["max_iters"] + 28, 4), np.int32)
    alvaar_amd.check(alvaar_amd.lib.alva_p3p_draw_samples(b["n"], len(drawn), 0, 12345, drawn.ctypes.data))
    assert np.array_equal(drawn, b["samples"])
    ok, R, t, out = ctx.p3p_lmeds(dev[name][0], dev[name][1], max_iters=b["max_iters"], err=PC.ERR, fx=PC.FX, fy=PC.FY, seed=12345)
    assert ok and got["have_model"] and got["n_valid_used"] == b["max_iters"]
    assert np.array_equal(_bits(R.ravel()), _bits(got["model"][:9])) and np.array_equal(_bits(t), _bits(got["model"][9:]))
    assert np.array_equal(out, np.flatnonzero(got["inlier"] == 0))


@pytest.mark.parametrize("route", [0, 1])
def test_repeatable_and_leaves_no_trace(ctx, dev, route0, route1, route):
    """(g) the same call again, after problems of other sizes -- one without any model, one whose scratch layout is larger -- gives the
    bytes of the first call; the arrival counter is back at zero each time"""
    first = (route0, route1)[route]
    for name, between in (("cap_round_end", "none_valid"), ("n65_H63", "n513_H257"), ("coincident", "n7168_H130")):
        mid = _run(ctx, dev, [between], route)[between]
        again = _run(ctx, dev, [name], route)[name]
        assert mid["counter_after"] == 0 and again["counter_after"] == 0
        if mid["have_model"]:
            _assert_same_bytes(first[between], mid, (between, route))
        _assert_same_bytes(first[name], again, (name, route), masks=route == 0)


def test_bad_arguments_are_rejected(ctx, dev, route0):
    """(h)"""
    import torch
    import alvaar_amd
    name = "n65_H63"
    b = PC.build(name)
    bv, wpt = dev[name]
    good = dict(bv=bv, wpt=wpt, samples=b["samples"], max_iters=b["max_iters"])
    big = torch.zeros((19001, 3), dtype=torch.float64, device="cuda")
    mid = torch.zeros((7169, 3), dtype=torch.float64, device="cuda")
    bad = [
        (dict(good, n=3), 0), (dict(good, n=3), 1),                                       # n < 4
        (dict(good, bv=big, wpt=big), 0),                                                 # n > 19000
        (dict(good, bv=mid, wpt=mid), 1),                                                 # n > 7168 in a batch
        (dict(good, samples=np.zeros((0, 4), np.int32)), 0), (dict(good, samples=np.zeros((0, 4), np.int32)), 1),   # H <= 0
        (dict(good, bv=None, n=65), 0), (dict(good, wpt=None), 1),                        # null pointers
        (dict(good, samples=np.full((4, 4), 65, np.int32)), 0), (dict(good, samples=np.full((4, 4), -1, np.int32)), 1),   # index outside the problem
        (dict(good, max_iters=0), 0),
    ]
    for pb, route in bad:
        with pytest.raises(alvaar_amd.AlvaError):
            ctx.p3p_hypotheses([pb], route=route)
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.p3p_hypotheses([good], route=2)
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.p3p_hypotheses([], route=0)
    with pytest.raises(alvaar_amd.AlvaError):
        ctx.p3p_hypotheses([good, dict(good, n=3)], route=1)                              # one bad problem rejects the batch before any launch
    for route in (0, 1):
        again = ctx.p3p_hypotheses([good], err=PC.ERR, fx=PC.FX, fy=PC.FY, route=route)[0]
        _assert_same_bytes(route0[name], again, (name, route))
