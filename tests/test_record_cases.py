"""The case tables of tests/record_cases.py against their own numpy statements, without a GPU: every case must produce, by the statement
alone, what it aims at -- the tie is won by the later row with the smaller id, the boundary pair falls on its side, the candidate at 128
bits or more is a candidate and loses, every pack filter removes something, the overflow log overflows on its 49th insert -- so that no
device test of test_gpu_map_records.py can pass vacuously."""
import numpy as np
import pytest

import record_cases as rc
from map_merge_ref import fuse_duplicates_sequential

LAUNCHES = rc.reloc_launches()
FUSE = rc.fuse_cases()
_by_name = lambda cases: pytest.mark.parametrize("case", cases, ids=[c["name"] for c in cases])


# ---------------------------------------------------------------------------------------------------- relocalization
def test_reloc_launches_cover_the_sizes_the_issue_names():
    assert {len(c["q"]) for c in LAUNCHES} >= set(rc.QUERY_COUNTS) and {len(c["rows"]) for c in LAUNCHES} >= set(rc.ROW_COUNTS)
    assert {c["max_dist"] for c in LAUNCHES} >= {0, 256} and {c["ratio"] for c in LAUNCHES} >= {0.0, 0.5, 0.8, 1.5}
    assert any(c["qvalid"] is None for c in LAUNCHES) and any(c["qvalid"] is not None and not c["qvalid"].all() for c in LAUNCHES)
    unused = np.concatenate([rc.row_ids(c["rows"]) for c in LAUNCHES])
    assert {-1, -2 ** 31} <= set(unused[unused < 0].tolist())
    big = next(c for c in LAUNCHES if c["name"] == "queries_2049")
    assert {1023, 1024, 2047, 2048, 255, 256, 63, 64} <= set(big["aim"]["kept"])


@_by_name(LAUNCHES)
def test_reloc_statement_gives_what_the_launch_aims_at(case):
    aim = case["aim"]
    got = rc._brute_force(case["q"], case["qvalid"], case["rows"], case["max_dist"], case["ratio"])
    by_q = {qi: (i, d) for qi, i, d in got}
    assert len(by_q) == len(got) and [g[0] for g in got] == sorted(by_q)
    for qi, pair in aim["kept"].items():
        assert by_q.get(qi) == pair, (qi, by_q.get(qi), pair)
    for qi in aim["rejected"]:
        assert qi not in by_q, qi
    assert (len(got) == 0) if aim["none"] else (len(got) >= 1 and len(aim["kept"]) >= 1)
    ids = rc.row_ids(case["rows"])
    for qi, win, lose in aim["ties"]:           # equal distances; the winner has the smallest id and is not the first of the tied rows
        d = [rc.hamming(case["q"][qi], case["rows"][r, 32:64]) for r in [win] + lose]
        assert len(set(d)) == 1 and d[0] > 0 and case["ratio"] > 1
        assert win > min(lose) and all(ids[win] < ids[r] for r in lose) and by_q[qi] == (int(ids[win]), d[0])
        assert len({r // 64 for r in [win] + lose}) == (1 if "one_chunk" in case["name"] else len(lose) + 1)
    for qi, best, second in aim.get("boundary", ()):   # exactly at the boundary: rejected; one bit inside: accepted
        d = np.sort([rc.hamming(case["q"][qi], r[32:64]) for r in case["rows"]])
        assert (d[0], d[1]) == (best, second) and ((qi in by_q) == (best < case["ratio"] * second)) and best in (19, 20)
    if aim["same_as"]:
        other = next(c for c in LAUNCHES if c["name"] == aim["same_as"])
        assert other["qvalid"] is None and case["qvalid"].all() and np.array_equal(other["q"], case["q"])
        assert got == rc._brute_force(other["q"], None, other["rows"], other["max_dist"], other["ratio"])
    # the statement does not depend on the row order
    assert got == rc._brute_force(case["q"], case["qvalid"], rc.permuted_rows(case), case["max_dist"], case["ratio"])


def test_reloc_launches_with_one_live_row_sit_at_the_257_boundary():
    for name, kept in (("single_row_205_of_1", True), ("single_row_206_of_65", False), ("single_row_205_of_129", True), ("single_row_206_of_2", False)):
        c = next(c for c in LAUNCHES if c["name"] == name)
        ids = rc.row_ids(c["rows"])
        live = np.flatnonzero(ids >= 0)
        assert len(live) == 1
        d = rc.hamming(c["q"][0], c["rows"][live[0], 32:64])
        assert d == (205 if kept else 206) and (np.float32(d) < np.float32(c["ratio"]) * np.float32(257)) == kept
        assert all(rc.hamming(c["q"][0], c["rows"][r, 32:64]) == 0 for r in range(len(ids)) if r != live[0])   # the unused rows would win


# ---------------------------------------------------------------------------------------------------- fuse
@_by_name(FUSE)
def test_fuse_statement_gives_what_the_case_aims_at(case):
    aim, ix = case["aim"], case["index"]
    keep, absorbed = fuse_duplicates_sequential(case["stream"], case["ids"], case["xyz"], case["desc"], case["max_dist"], case["max_hamming"])
    k2, a2, rounds = rc.fuse_fixed_point(case)
    assert np.array_equal(k2, keep) and np.array_equal(a2, absorbed)      # the fixed point is the sequential rule
    mh = case["max_hamming"]
    for rec, near, far in aim.get("pairs", ()):
        cand = dict(rc.fuse_candidates(case, ix[rec]))
        assert cand.get(ix[near]) == aim["h_near"] and keep[ix[near]] and keep[ix[far]]
        if mh >= 127:
            assert cand == {ix[near]: aim["h_near"], ix[far]: mh} and (mh < 128 or 128 <= cand[ix[far]] <= mh)
        else:
            assert ix[far] not in cand and rc.hamming(case["desc"][ix[far]], case["desc"][ix[rec]]) == mh + 1
        assert absorbed[ix[rec]] == ix[near]
    if "pairs" in aim:
        assert {ix[f] < ix[n] for _, n, f in aim["pairs"]} == {True, False}          # the far one earlier, and later
        assert absorbed[ix[aim["absorbed_at"]]] == ix["lone_at"]
        assert rc.hamming(case["desc"][ix["lone_at"]], case["desc"][ix["rec_at"]]) == mh
        assert aim["survives"] is None or (keep[ix[aim["survives"]]] and
                                           rc.hamming(case["desc"][ix["lone_over"]], case["desc"][ix["rec_over"]]) == mh + 1)
    if "n_candidates" in aim:
        cand = rc.fuse_candidates(case, ix["rec"])
        assert len(cand) == aim["n_candidates"] and aim["error"] == (len(cand) > 32)
        assert cand[0][0] < 64 <= cand[-1][0] and absorbed[ix["rec"]] == ix[aim["winner"]] == cand[-1][0]
        assert sorted(h for _, h in cand)[1:3] == [6, 6]
    for rec, by in aim.get("absorbed", {}).items():
        assert absorbed[ix[rec]] == ix[by]
    for rec in aim.get("survive", ()):
        assert keep[ix[rec]]
    if aim.get("some_absorbed"):
        assert 0 < (~keep).sum() < len(keep)
    for rec, win in aim.get("winners", {}).items():
        cand = rc.fuse_candidates(case, ix[rec])
        best = min(h for _, h in cand)
        assert sum(j < 64 for j, _ in cand) == 4 and sum(j >= 64 for j, _ in cand) == 4
        assert absorbed[ix[rec]] == ix[win] == min(j for j, h in cand if h == best)
    if "winners" in aim:
        assert ix[aim["winners"]["rec_a"]] >= 64 and len([1 for j, h in rc.fuse_candidates(case, ix["rec_b"]) if h == 9]) == 2
    for rec, first in aim.get("links", ()):      # the link's first choice among ALL its candidates is one that has been absorbed
        cand = rc.fuse_candidates(case, ix[rec])
        assert len(cand) == 2 and min((h, j) for j, h in cand)[1] == ix[first] and not keep[ix[first]]
    for rec, kept in aim.get("verdicts", {}).items():
        assert keep[ix[rec]] == kept
    if "min_rounds" in aim:
        assert len(set(case["stream"].tolist())) >= 5 and rounds >= aim["min_rounds"], rounds


def test_fuse_cases_cover_the_sizes_the_issue_names():
    assert {len(c["ids"]) for c in FUSE} >= {1, 3, 4, 5, 64, 65, 129}
    assert {c["max_hamming"] for c in FUSE} >= {0, 127, 128, 200, 256} and 0.0 in {c["max_dist"] for c in FUSE}
    c = next(c for c in FUSE if c["name"] == "max_hamming_256")
    assert any(np.array_equal(c["desc"][c["index"][f]], ~c["desc"][c["index"][r]]) for r, _, f in c["aim"]["pairs"])
    for c in FUSE:                                 # the block form holds the same records
        b = rc.fuse_block(c)
        live = b[rc.row_ids(b) >= 0]
        assert np.array_equal(rc.row_ids(live), c["ids"]) and np.array_equal(live[:, 32:64], c["desc"])


# ---------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("n_slots", rc.PACK_SLOT_COUNTS)
def test_pack_case_filters(n_slots):
    c = rc.pack_case(n_slots)
    rec, kinds = c["records"], np.array(c["kinds"], dtype=object)
    assert len(kinds) == n_slots and len(rec) % 4096 == 0 and len(rec) >= max(n_slots, 1)
    # the tables as the log leaves them: a medoid where the last operation of the slot is an add
    last = {}
    for slot, op, kf, d, rh in c["ops"]:
        last[slot] = op
    has = np.array([last.get(s, 3) == 0 for s in range(n_slots)], bool)
    kept = rc.pack_host_filter(rec, n_slots, has, has.astype(np.int32))
    assert kept.tolist() == [s for s in range(n_slots) if kinds[s] == "live"]
    assert {int(rec[s]["id"]) for s in kept} == set(c["want"])
    if n_slots >= 255:      # every filter removes at least one record, and it is the only filter that removes it
        r = rec[:n_slots]
        passes = {"free": r["id"] >= 0, "not3d": r["is3d"] != 0, "nodesc": r["has_desc"] != 0, "table": has}
        for kind, col in (("free", "free"), ("not3d", "not3d"), ("nodesc", "nodesc"), ("unwritten", "table"), ("cleared", "table")):
            hit = np.flatnonzero(kinds == kind)
            assert len(hit) >= 1 and not passes[col][hit].any(), kind
            assert all(passes[o][hit].all() for o in passes if o != col), kind
    n = len(c["want"])
    assert {0, n} <= set(c["capacities"]) and max(c["capacities"]) > n and (n == 0 or any(0 < k < n for k in c["capacities"]) or n == 1)
    if n_slots > 4096:
        assert kinds[4095] == "live" and kinds[4096] == "live"


# ---------------------------------------------------------------------------------------------------- medoid store (host build)
ref = pytest.mark.ref
SEQS = ("growth+ties", "random", "release+reuse")


def _replay_per_operation(launches, slot):
    t = np.zeros(rc.TABLE_BYTES, np.uint8)
    rc.host_apply(t, True, [])
    for ops in launches:
        for o in ops:
            if o[0] == slot:
                rc.host_apply(t, False, [o[1:]])
    return t


@ref
@pytest.mark.parametrize("cut", rc.MEDOID_CUTS)
@pytest.mark.parametrize("name", SEQS)
def test_host_tables_fed_the_cut_logs_equal_the_per_operation_replay(name, cut):
    log = rc.medoid_cut_log(name, cut)
    assert sum(len(l) for l in log["launches"]) > 40 and (cut is None) == (len(log["launches"]) == 1)
    assert cut is None or all(len(l) == cut for l in log["launches"][:-1])
    assert sum(b is not None for b in log["border"]) >= (1 if cut is None else 5)
    assert any(o[1] == 2 for l in log["launches"] for o in l) or name == "random"       # a clear in mid-chain
    for slot in (rc.POINT, rc.BYSTANDER):
        t = np.zeros(rc.TABLE_BYTES, np.uint8)
        rc.host_apply(t, True, [])
        for ops, want in zip(log["launches"], log["border"]):
            rc.host_apply(t, False, [o[1:] for o in ops if o[0] == slot])
            if slot == rc.POINT and want is not None:
                assert rc.same_table(rc.table_view(t), want)
        assert np.array_equal(t, _replay_per_operation(log["launches"], slot))
    assert rc.same_table(rc.table_view(_replay_per_operation(log["launches"], rc.POINT)), log["final"])
    assert len(rc.table_view(_replay_per_operation(log["launches"], rc.BYSTANDER))[2]) == log["bystander_count"]


@ref
def test_host_tables_of_the_many_point_log():
    log, slots, final = rc.medoid_many_points(40)
    assert len(final) == 40 and max(final) < slots
    assert [o[0] for o in log[:40]] == sorted(final)                        # interleaved: entry k of every chain before entry k + 1 of any
    for slot, want in final.items():
        chain = [o for o in log if o[0] == slot]
        assert 3 in [o[1] for o in chain[1:]]                               # a reset in mid-chain
        assert rc.same_table(rc.table_view(_replay_per_operation([chain], slot)), want)


@ref
def test_overflow_logs_set_the_flag_on_the_insert_they_aim_at():
    for log in rc.medoid_overflow_logs():
        t = np.zeros(rc.TABLE_BYTES, np.uint8)
        rc.host_apply(t, True, [o[1:] for o in log["fill"]])
        before = t.copy()
        assert rc.same_table(rc.table_view(t), log["want"]) and len(rc.table_view(t)[2]) == log["count"]
        rc.host_apply(t, False, [log["over"][1:]])
        assert rc.table_view(t)[4]                                           # the flag
        t[rc.OVERFLOW_BYTES] = 0
        assert np.array_equal(t, before)                                     # otherwise as it was
        rc.host_apply(t, False, [(0, 5000, np.zeros(32, np.uint8), 0)] if log["name"] == "rehash_to_127" else [])
        assert (len(rc.table_view(t)[2]) == log["count"] + 1) == (log["name"] == "rehash_to_127")   # only the 49th was refused for room
