"""The match-to-map case table (tests/mtm_cases.py) proved on the CPU: by the plain-C checker's trace (orc_match_to_map_trace) every case
reaches the branch it is named for and gives the result it states; twins differ in the named outcome only; the traced call equals the
untraced ones; the table covers every ending, candidate gate, neighbourhood size and merge branch.  Marked `ref`: the checker equals
the compiled reference's own Mapper::matchToMap on every case that needs no flags."""
import numpy as np
import pytest

import mtm_cases as T
from oracles import (MTM_ENDS, orc_match_to_map, orc_match_to_map_flags, orc_match_to_map_trace, ref_available, ref_match_to_map)

GATES = ("px", "kp_nodesc", "shared_kf", "coproj", "desc")
KEPT = {k for k, _, _, _ in T.TWINS}
_runs = {}


def _run(c):
    if c["name"] not in _runs:
        _runs[c["name"]] = orc_match_to_map_trace(c["pb"], c["aux"], c["mhd"], c["ohd"], **c["kw"])
    return _runs[c["name"]]


def test_names_unique():
    names = [c["name"] for c in T.CASES]
    assert len(set(names)) == len(names)
    assert all(k in T.BY_NAME and d in T.BY_NAME for k, d, _, _ in T.TWINS)
    assert max(len(c["pb"]["mp_id"]) for c in T.CASES) <= 300


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c["name"])
def test_case_reaches_its_branch(case):
    out, trace = _run(case)
    assert np.array_equal(out, T.expected_rows(case)), "the checker's result is not the one the case states"
    assert len(trace) == len(case["pb"]["local"])
    for li, claim in case["claims"].items():
        got = {k: trace[li][k] for k in claim}
        assert got == claim, f"list position {li}: {trace[li]}"
    for t in trace:      # the columns are consistent with one another
        assert t["total"] == sum(t[g] for g in GATES) + t["nvalid"]
        assert (t["best_pos"] >= 0) == (t["nvalid"] > 0) and (t["sec_pos"] >= 0) == (t["nvalid"] > 1)
        assert t["end"] in MTM_ENDS[1:]
    # an empty result must never pass for agreement: the case reaches the scan, and a case whose name says so matches
    if case["scan"]:
        assert any(t["total"] > 0 for t in trace), "no local point of this case reaches the scan"
    if case["name"] in KEPT or case["name"].endswith("_kept"):
        assert case["matches"] and int((out >= 0).sum()) == len(case["matches"])
    if case["group"] not in ("point", "size"):
        assert case["scan"]


@pytest.mark.parametrize("case", [c for c in T.CASES if c["exact"]], ids=lambda c: c["name"])
def test_threshold_quantities_are_exact(case):
    """the quantity a twin puts at (or one float past) a threshold, recomputed in the kernel's operation order, IS that float"""
    for what, (value, want) in case["exact"].items():
        assert np.asarray(value).tobytes() == np.asarray(want, np.asarray(value).dtype).tobytes(), what


@pytest.mark.parametrize("kept,dropped,end,gate", T.TWINS, ids=lambda v: v if isinstance(v, str) and "_" in v else None)
def test_twins_differ_in_the_named_outcome(kept, dropped, end, gate):
    ck, cd = T.BY_NAME[kept], T.BY_NAME[dropped]
    (ok, tk), (od, td) = _run(ck), _run(cd)
    a, b = tk[0], td[0]
    assert a["end"] == "matched" and b["end"] == end
    assert int((ok >= 0).sum()) == 1 and int((od >= 0).sum()) == 0
    if gate is not None:        # the same neighbourhood; one candidate more falls to the named gate and to no other
        assert a["total"] == b["total"]
        assert b[gate] == a[gate] + 1 and b["nvalid"] == a["nvalid"] - 1
        assert all(a[g] == b[g] for g in GATES if g != gate)
    elif end == "ratio_reject":  # the same candidates pass the gates; only the ratio test differs
        assert all(a[g] == b[g] for g in GATES + ("total", "nvalid"))


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c["name"])
def test_traced_equals_untraced(case):
    out, _ = _run(case)
    assert np.array_equal(out, orc_match_to_map_flags(case["pb"], case["aux"], case["mhd"], case["ohd"], **case["kw"]))
    if case["mhd"] is None:
        ids = case["pb"]["mp_id"]
        assert orc_match_to_map(case["pb"], case["aux"], **case["kw"]) == {int(ids[k]): int(ids[out[k]]) for k in range(len(out)) if out[k] >= 0}
        # all-ones flags say the same as no flags
        n_obs = len(case["pb"]["obs_kf"])
        has = np.array([1 if case["pb"]["obs_ptr"][m + 1] > case["pb"]["obs_ptr"][m] else 0 for m in range(len(ids))], np.uint8)
        assert np.array_equal(out, orc_match_to_map_flags(case["pb"], case["aux"], has, np.ones(n_obs, np.uint8), **case["kw"]))


def test_table_covers():
    traces = [t for c in T.CASES for t in _run(c)[1]]
    assert {t["end"] for t in traces} == set(MTM_ENDS[1:])
    for g in GATES:
        assert any(t[g] > 0 for t in traces), g
    assert {1, 63, 64, 65, 128, 129} <= {t["total"] for t in traces} and any(t["total"] >= 150 for t in traces)
    for col in ("merge_better", "merge_equal", "merge_worse"):
        assert any(t[col] > 0 for t in traces), col
    # the best and the second in each of the three chunks, and at each position where a chunk begins or ends
    assert {0, 1, 2} <= {t["best_pos"] // 64 for t in traces if t["best_pos"] >= 0}
    assert {0, 1, 2} <= {t["sec_pos"] // 64 for t in traces if t["sec_pos"] >= 0}
    assert {0, 63, 64, 127, 128, 149} <= {t["best_pos"] for t in traces}
    groups = {c["group"] for c in T.CASES}
    assert groups == {"point", "scan", "walk", "gate", "desc", "ratio", "arbitration", "size", "records"}
    cells = {c["pb"]["cell_size"] for c in T.CASES}
    assert {16, 35, 64} <= cells and any(c["pb"]["calib"][8] % c["pb"]["cell_size"] for c in T.CASES)
    assert {len(c["pb"]["local"]) for c in T.CASES} >= {0, 1, 3, 4, 5} and {len(c["pb"]["mp_id"]) for c in T.CASES} >= {1, 255, 256, 257}


def test_permuted_rows_give_the_permuted_result():
    """the helper the GPU test uses, on the checker: rows in another order, indices relabelled"""
    c = T.BY_NAME["arb_5_5_7_different_workgroups"]
    q, perm = T.permuted(c, 5)
    inv = np.argsort(perm)
    out = _run(c)[0]
    want = np.array([inv[out[r]] if out[r] >= 0 else -1 for r in perm], np.int32)
    assert np.array_equal(orc_match_to_map_flags(q["pb"], q["aux"], q["mhd"], q["ohd"], **q["kw"]), want) and (want >= 0).any()


@pytest.mark.ref
@pytest.mark.parametrize("case", T.FLAT_CASES, ids=lambda c: c["name"])
def test_checker_equals_reference(case):
    """the reference's own Mapper::matchToMap on the case's map, and the checker under the container orders the reference reports"""
    if not ref_available():
        pytest.skip("compiled reference not present")
    ref, aux = ref_match_to_map(case["pb"], **case["kw"])
    assert orc_match_to_map(case["pb"], aux, **case["kw"]) == ref
    assert np.array_equal(aux["kf_t"], case["aux"]["kf_t"]) and np.array_equal(aux["cell_ptr"], case["aux"]["cell_ptr"])
