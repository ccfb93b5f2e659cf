"""The P3P-LMedS hypothesis table: named problems, each chosen because one of the steps that decide the winner of alva_p3p_lmeds -- a
hypothesis' validity, its LMedS penalty (the radix select, its one-key early exit and the even-n pass of csrc/p3p_device.hpp), its inlier
mask, and the selection replay "first max_iters valid, strict <, earliest on ties" in 64-lane rounds of 256-hypothesis blocks -- takes a
path the final answer of a random problem does not show.

A case is generator arguments, not data: a problem (`gen`), the first H samples of the sampler's stream on n points (Orc.p3p_draw_samples:
alva_p3p_draw_samples' stream, restated), then `edits` of sample rows, in order:
  ("invalid", rows)   the row repeats an index among its first three -- (i, i, j, k) on even rows, (i, j, j, k) on odd ones: the world
                      triple's cross product is exactly zero, the hypothesis has no model on any implementation
  ("all_invalid",)    every row
  ("best_to", row)    the row holding the smallest penalty (the plain-C checker's, strictly smallest) is swapped to `row`
  ("copy", a, b)      row b becomes a copy of row a
  ("fourth_apart",)   where a row's fourth point coincides with one of its first three, the fourth index moves on to the next point
                      that does not: all four candidate poses explain a repeated point equally well, and which one is kept would be
                      decided by rounding
Generators: ("pnp", seed, outlier share, pixel noise) = synth.make_pnp_problem; ("coincident",) = the problem of
test_gpu_pose.py::test_p3p_many_degenerate_samples_force_a_redraw (70 % of the points are one point: coincident triples are exactly
degenerate too, and every model's keys tie at the median).
`prop` names the predicate of PROPS the case exists for; tests/test_p3p_cases.py asserts it with the checker alone, so a case that stops
reaching its branch fails there and not silently on the GPU.  `prod` marks cases whose samples are the unedited stream with
H = max_iters + 28, the shape alva_p3p_lmeds itself launches: the GPU test compares those with the production call.

Only exactly degenerate or clearly valid samples: the table has no nearly collinear triple, whose validity would depend on rounding."""
from __future__ import annotations

import functools

import numpy as np

from alvaar_amd import synth
from oracles import Orc

ERR, FX, FY = 3.0, 579.4, 579.4
MODEL_TOL = 1e-8          # test_gpu_pose.py's P3P_TOL: the project's figure for this stage
SKIP_CAP = 0.01           # share of valid hypotheses whose model may differ by more than MODEL_TOL, over the whole table


def _case(name, prop, n, H, gen, max_iters=None, edits=(), prod=False):
    if max_iters is None:
        max_iters = max(1, H - 28)
    if prod:
        assert not edits and H == max_iters + 28
    return dict(name=name, prop=prop, n=n, H=H, gen=gen, max_iters=max_iters, edits=tuple(edits), prod=prod)


def _pnp(seed, outl=0.2, noise=0.5):
    return ("pnp", seed, outl, noise)


CASES = [
    # ---- sizes: n at the mask word, the batch stride (256), the single launch's stride (512), the default-LDS boundary and the maximum;
    #      H at one group of four lanes, the 64-lane round, inline vs pinned samples (192 | 193) and the 256-hypothesis block
    _case("n4_H128", "few_distinct", 4, 128, _pnp(44, 0.0, 0.1)),
    _case("n5_H128", "few_distinct", 5, 128, _pnp(45, 0.0, 0.1)),
    _case("n63_H1", "all_valid", 63, 1, _pnp(1, 0.1)),
    _case("n64_H4", "all_valid", 64, 4, _pnp(2, 0.3)),
    _case("n65_H63", "all_valid", 65, 63, _pnp(3, 0.2), prod=True),
    _case("n255_H64", "all_valid", 255, 64, _pnp(4, 0.0)),
    _case("n256_H65", "all_valid", 256, 65, _pnp(5, 0.3)),
    _case("n257_H192", "all_valid", 257, 192, _pnp(6, 0.1), prod=True),
    _case("n511_H193", "all_valid", 511, 193, _pnp(7, 0.2), prod=True),
    _case("n512_H256", "all_valid", 512, 256, _pnp(8, 0.3)),
    _case("n513_H257", "all_valid", 513, 257, _pnp(9, 0.1)),
    _case("n300_H300", "all_valid", 300, 300, _pnp(10, 0.2)),
    _case("n7168_H130", "all_valid", 7168, 130, _pnp(11, 0.2)),
    _case("n7169_H64", "all_valid", 7169, 64, _pnp(12, 0.2), prod=True),      # raised dynamic LDS, samples in the arguments (k_p3p_s)
    _case("n7169_H200", "all_valid", 7169, 200, _pnp(12, 0.2)),               # ... samples in pinned memory (k_p3p)
    _case("n19000_H40", "all_valid", 19000, 40, _pnp(13, 0.1)),
    # ---- no model at chosen positions: first and last hypothesis, both sides of every round and block edge
    _case("invalid_edges", "invalid_at", 130, 257, _pnp(34), max_iters=300, edits=[("invalid", (0, 63, 64, 127, 128, 191, 192, 255, 256))]),
    # ---- max_iters against the valid count.  In the three cap_* cases the strictly best row of the stream sits right AFTER the
    #      hypothesis on which the cap is reached: it must not win
    _case("cap_mid_round", "cap_mid_round", 130, 200, _pnp(15), max_iters=100,
          edits=[("invalid", (3, 17, 64, 65, 100)), ("best_to", 105)]),       # 100th valid = row 104
    _case("cap_round_end", "cap_round_end", 77, 200, _pnp(16), max_iters=123,
          edits=[("invalid", (0, 31, 62, 63, 90)), ("best_to", 128)]),        # 123rd valid = row 127
    _case("cap_block_end", "cap_block_end", 200, 300, _pnp(17), max_iters=250,
          edits=[("invalid", (5, 64, 128, 129, 200, 254)), ("best_to", 256)]),  # 250th valid = row 255
    _case("cap_after_invalid", "cap_mid_round", 96, 140, _pnp(18), max_iters=58,
          edits=[("invalid", (10, 20, 60, 61)), ("best_to", 62)]),            # 58th valid = row 59; rows 60, 61 have no model; best = row 62, same round
    _case("fewer_valid", "fewer_valid", 130, 65, _pnp(19), max_iters=100, edits=[("invalid", tuple(range(2, 65, 7)))]),
    _case("none_valid", "none_valid", 130, 70, _pnp(20), max_iters=100, edits=[("all_invalid",)]),
    _case("none_valid_H4", "none_valid", 64, 4, _pnp(21), max_iters=4, edits=[("all_invalid",)]),
    _case("one_valid_last", "one_valid_last", 65, 257, _pnp(22), max_iters=5, edits=[("invalid", tuple(range(256)))]),
    # ---- ties
    _case("coincident", "key_ties", 400, 300, ("coincident",), max_iters=100, edits=[("fourth_apart",)]),
    _case("noise_free", "penalty_ties", 100, 128, _pnp(23, 0.0, 0.0)),
    _case("noise_free_odd", "penalty_ties", 101, 128, _pnp(24, 0.0, 0.0)),
    _case("dup_same_round", "dup_wins_first", 130, 300, _pnp(25), max_iters=272, edits=[("best_to", 70), ("copy", 70, 100)]),
    _case("dup_next_round", "dup_wins_first", 131, 300, _pnp(26), max_iters=272, edits=[("best_to", 10), ("copy", 10, 100)]),
    _case("dup_next_block", "dup_wins_first", 130, 300, _pnp(27), max_iters=272, edits=[("best_to", 200), ("copy", 200, 270)]),
    _case("dup_lane_order", "dup_wins_first", 64, 64, _pnp(28), max_iters=64, edits=[("best_to", 62), ("copy", 62, 63)]),
    # ---- even n, both arms of "is rank mid-1 below the median key"
    _case("even_keys_distinct", "even_distinct", 512, 40, _pnp(29, 0.3)),
    # (unedited: where the fourth point repeats one of the triple, the kept pose may differ from the checker's -- assertion (b) counts it)
    _case("even_keys_equal", "even_equal", 40, 64, ("coincident",), max_iters=64),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert all(c["H"] <= 300 for c in CASES)

# the problems of one batch launch (route 1): different n and H, so that workgroups leave at blockIdx.x >= H and LDS is sized for n_max
BATCH_TRIO = ("n513_H257", "n64_H4", "n7168_H130")


def _problem(case, ulp):
    g = case["gen"]
    n = case["n"]
    if g[0] == "pnp":
        pb = synth.make_pnp_problem(n, g[1], outlier_frac=g[2], noise_px=g[3])
        bv, wpt = pb["bv"].copy(), pb["wpt"].copy()
    else:
        pb = synth.make_pnp_problem(n, 31, outlier_frac=0.1)
        bv, wpt = pb["bv"].copy(), pb["wpt"].copy()
    if ulp:   # every input moved by one ulp, up or down (test_p3p_cases.py: how far the checker's models move)
        rng = np.random.RandomState(1000 + n)
        for a in (bv, wpt):
            a[...] = np.nextafter(a, np.where(rng.rand(*a.shape) < 0.5, -np.inf, np.inf))
    if g[0] == "coincident":
        dup = np.random.RandomState(5).rand(n) < 0.7
        wpt[dup] = wpt[0]
        bv[dup] = bv[0]
    return np.ascontiguousarray(bv), np.ascontiguousarray(wpt)


def oracle_eval(bv, wpt, samples):
    """the checker, hypothesis by hypothesis: valid [H] bool, models [H,12] (zero where none), penalty [H] (+inf where none)"""
    H = len(samples)
    thr = Orc.p3p_threshold(ERR, FX, FY)
    valid, models, pen = np.zeros(H, bool), np.zeros((H, 12)), np.full(H, np.inf)
    for h in range(H):
        ok, m = Orc.p3p_model(bv, wpt, samples[h])
        if ok:
            valid[h], models[h] = True, m
            pen[h] = Orc.p3p_penalty(m, bv, wpt, thr)[0]
    return dict(valid=valid, models=models, penalty=pen)


def replay(valid, penalty, max_iters):
    """The selection, one hypothesis after the other (Lmeds.hpp:60-150): the first max_iters VALID hypotheses in draw order, strict <,
    so the earliest on ties.  Returns dict(best (-1: none), used, have_model, cap_row = the row on which the cap was reached or -1)."""
    best, best_p, used, cap_row = -1, 1.7976931348623157e308, 0, -1
    for h in range(len(valid)):
        if used >= max_iters:
            break
        if not valid[h]:
            continue
        if penalty[h] < best_p:
            best, best_p = h, penalty[h]
        used += 1
        if used == max_iters:
            cap_row = h
    return dict(best=best, used=used, have_model=int(best >= 0), cap_row=cap_row)


def _invalid_row(row, h):
    s = row.copy()
    if h % 2 == 0:
        s[1] = s[0]
    else:
        s[2] = s[1]
    return s


@functools.lru_cache(maxsize=None)
def _build(name, ulp):
    case = BY_NAME[name]
    n, H = case["n"], case["H"]
    bv, wpt = _problem(case, ulp)
    samples = Orc.p3p_draw_samples(n, H)
    if ulp:
        samples = _build(name, False)["samples"]    # the same rows: "best_to" is decided on the unperturbed problem
    else:
        for e in case["edits"]:
            if e[0] == "invalid":
                for h in e[1]:
                    samples[h] = _invalid_row(samples[h], h)
            elif e[0] == "all_invalid":
                for h in range(H):
                    samples[h] = _invalid_row(samples[h], h)
            elif e[0] == "best_to":
                o = oracle_eval(bv, wpt, samples)
                order = np.argsort(o["penalty"], kind="stable")
                assert o["penalty"][order[0]] < o["penalty"][order[1]], (name, "the stream's best penalty is not unique")
                a, b = int(order[0]), e[1]
                assert o["valid"][b], (name, "best_to: target row has no model")
                samples[[a, b]] = samples[[b, a]]
            elif e[0] == "fourth_apart":
                for h in range(H):
                    tri = wpt[samples[h, :3]]
                    j = int(samples[h, 3])
                    while (wpt[j] == tri).all(axis=1).any():
                        j = (j + 1) % n
                    samples[h, 3] = j
            elif e[0] == "copy":
                samples[e[2]] = samples[e[1]]
            else:
                raise ValueError(e)
    samples.setflags(write=False)
    bv.setflags(write=False)
    wpt.setflags(write=False)
    return dict(name=name, case=case, n=n, H=H, max_iters=case["max_iters"], bv=bv, wpt=wpt, samples=samples, err=ERR, fx=FX, fy=FY)


def build(case, ulp=False):
    """the case's arrays (read-only, shared between callers): bv, wpt [n,3], samples [H,4], max_iters, err, fx, fy"""
    return _build(case["name"] if isinstance(case, dict) else case, bool(ulp))


@functools.lru_cache(maxsize=None)
def _checker(name, ulp):
    b = _build(name, ulp)
    o = oracle_eval(b["bv"], b["wpt"], b["samples"])
    o["replay"] = replay(o["valid"], o["penalty"], b["max_iters"])
    return o


def checker(case, ulp=False):
    """oracle_eval + replay of a case, computed once per process"""
    return _checker(case["name"] if isinstance(case, dict) else case, bool(ulp))


def median_keys(b, o, h):
    """(key of rank mid-1, key of rank mid) of hypothesis h under the checker's model"""
    k = Orc.p3p_sorted_keys(o["models"][h], b["bv"], b["wpt"])
    return k[b["n"] // 2 - 1], k[b["n"] // 2]


def _rows_with(case, kind):
    return [h for e in case["edits"] if e[0] == kind for h in e[1]]


def _used_rows(o, r):
    """rows the selection looked at: valid ones up to the cap"""
    last = r["cap_row"] if r["cap_row"] >= 0 else len(o["valid"]) - 1
    return [h for h in range(last + 1) if o["valid"][h]]


def _best_sits_after_cap(b, o, r):
    """the cap is reached, and the strictly best hypothesis of the whole stream is the next valid row behind it"""
    cap = r["cap_row"]
    if cap < 0 or r["used"] != b["max_iters"]:
        return False
    nxt = next((h for h in range(cap + 1, b["H"]) if o["valid"][h]), -1)
    return nxt >= 0 and nxt == int(np.argmin(o["penalty"])) and o["penalty"][nxt] < o["penalty"][r["best"]] and r["best"] <= cap


def _dup_wins_first(b, o, r):
    (_, a, c), = [e for e in b["case"]["edits"] if e[0] == "copy"]
    p = o["penalty"]
    others = np.delete(p, [a, c])
    return a < c <= r["cap_row"] and p[a] == p[c] and p[a] < others.min() and r["best"] == a


PROPS = {
    "all_valid": lambda b, o, r: bool(o["valid"].all()) and r["used"] == min(b["H"], b["max_iters"]),
    # n = 4 / 5: the median is one of very few keys, so 128 hypotheses share a handful of penalties and the winner is a tie's first row
    "few_distinct": lambda b, o, r: bool(o["valid"].all()) and len(np.unique(o["penalty"])) <= 8
                    and int((o["penalty"][:r["cap_row"] + 1] == o["penalty"][r["best"]]).sum()) >= 2,
    "invalid_at": lambda b, o, r: sorted(np.flatnonzero(~o["valid"]).tolist()) == sorted(_rows_with(b["case"], "invalid")),
    "cap_mid_round": lambda b, o, r: _best_sits_after_cap(b, o, r) and r["cap_row"] % 64 not in (0, 63),
    "cap_round_end": lambda b, o, r: _best_sits_after_cap(b, o, r) and r["cap_row"] % 64 == 63 and r["cap_row"] % 256 != 255,
    "cap_block_end": lambda b, o, r: _best_sits_after_cap(b, o, r) and r["cap_row"] == 255 and b["H"] > 256,
    "fewer_valid": lambda b, o, r: 0 < r["used"] == int(o["valid"].sum()) < b["max_iters"] and r["cap_row"] == -1,
    "none_valid": lambda b, o, r: not o["valid"].any() and r == dict(best=-1, used=0, have_model=0, cap_row=-1),
    "one_valid_last": lambda b, o, r: np.flatnonzero(o["valid"]).tolist() == [b["H"] - 1] and r["best"] == b["H"] - 1 and r["used"] == 1,
    # median ties inside the keys of every valid hypothesis, and equal penalties across hypotheses
    "key_ties": lambda b, o, r: b["n"] % 2 == 0 and o["valid"].any()
                and all(np.equal(*median_keys(b, o, h)) for h in np.flatnonzero(o["valid"]))
                and len(np.unique(o["penalty"][o["valid"]])) < int(o["valid"].sum()),
    # exact data: the winner is decided by the tie rule alone
    "penalty_ties": lambda b, o, r: int((o["penalty"][_used_rows(o, r)] == o["penalty"][r["best"]]).sum()) >= 2,
    "dup_wins_first": _dup_wins_first,
    "even_distinct": lambda b, o, r: b["n"] % 2 == 0 and bool(o["valid"].all())
                     and all(np.less(*median_keys(b, o, h)) for h in range(b["H"])),
    "even_equal": lambda b, o, r: b["n"] % 2 == 0 and o["valid"].any()
                  and all(np.equal(*median_keys(b, o, h)) for h in np.flatnonzero(o["valid"])),
}
assert all(c["prop"] in PROPS for c in CASES)
