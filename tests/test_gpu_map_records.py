"""GPU: the map-record block's writers and readers on the case tables of tests/record_cases.py (what each case aims at, and the proof that
the numpy statements alone produce it: test_record_cases.py).  alva_reloc_match and alva_fuse_map_points against their statements at the
size, tie and threshold edges; alva_pack_map_records against the host filter over the records and the tables' export; the descriptor tables
(medoid.hip) with whole chains of operations per launch, hundreds of points per launch, growth of the store and the sticky overflow flag.
Every comparison is equality of integers or bytes."""
import numpy as np
import pytest

import record_cases as rc

pytestmark = pytest.mark.gpu

LAUNCHES = rc.reloc_launches()
FUSE = rc.fuse_cases()
_by_name = lambda cases: pytest.mark.parametrize("case", cases, ids=[c["name"] for c in cases])


# ---------------------------------------------------------------------------------------------------- relocalization
def _reloc(ctx, case, rows, gather=True):
    """one launch -> [(query, id, distance)], after checking the row column and the gathered correspondences"""
    import torch
    q, nq = case["q"], len(case["q"])
    rng = np.random.RandomState(5)
    bv, unpx = rng.randn(nq, 3), (rng.rand(nq, 2) * 600).astype(np.float32)
    dv = None if case["qvalid"] is None else torch.from_numpy(case["qvalid"]).cuda()
    match, obv, ouv, owpt = ctx.reloc_match(torch.from_numpy(q).cuda(), torch.from_numpy(rows).cuda(), dv, case["max_dist"], case["ratio"],
                                            bv=torch.from_numpy(bv).cuda() if gather else None,
                                            unpx=torch.from_numpy(unpx).cuda() if gather else None, wpt=gather)
    m = match.cpu().numpy()
    assert np.array_equal(m[:, 2], rc.row_ids(rows)[m[:, 1]])                  # the row named holds the id reported
    if gather:
        assert np.array_equal(owpt.cpu().numpy().view(np.uint64), rows[m[:, 1], 8:32].copy().view(np.uint64))
        assert np.array_equal(obv.cpu().numpy().view(np.uint64), bv[m[:, 0]].view(np.uint64))
        assert np.array_equal(ouv.cpu().numpy().view(np.uint64), unpx[m[:, 0]].astype(np.float64).view(np.uint64))
    else:
        assert obv is None and ouv is None and owpt is None
    return [(int(a), int(c), int(d)) for a, b, c, d in m]


@_by_name(LAUNCHES)
def test_reloc_match_equals_the_statement_in_both_row_orders_with_and_without_gather(ctx, case):
    want = rc._brute_force(case["q"], case["qvalid"], case["rows"], case["max_dist"], case["ratio"])
    given = _reloc(ctx, case, case["rows"])
    permuted = _reloc(ctx, case, rc.permuted_rows(case))
    bare = _reloc(ctx, case, case["rows"], gather=False)                     # all three gather outputs null, bv / unpx null
    assert given == want, (given[:8], want[:8])
    assert permuted == given and bare == given
    if case["aim"]["same_as"]:                                               # qvalid = NULL equals qvalid all ones
        other = next(c for c in LAUNCHES if c["name"] == case["aim"]["same_as"])
        assert _reloc(ctx, other, other["rows"]) == given


def test_reloc_match_keeps_no_claim_of_an_earlier_larger_launch():
    """the larger launch claims row 0 for (distance 0, query 2); the next one's only claimant of row 0 is (distance 3, query 0), which a
    claim word left over from the first launch would beat"""
    import alvaar_amd
    ctx = alvaar_amd.Context(0)
    by = {c["name"]: c for c in LAUNCHES}
    for name in ("unused_chunk_between_live_chunks", "rows_2", "tie_three_chunks", "single_row_205_of_1"):
        c = by[name]
        want = rc._brute_force(c["q"], c["qvalid"], c["rows"], c["max_dist"], c["ratio"])
        assert _reloc(ctx, c, c["rows"]) == want and len(want) >= 1, name
        if name == "rows_2":
            assert want[0] == (0, int(rc.row_ids(c["rows"])[0]), 3) and by["unused_chunk_between_live_chunks"]["aim"]["kept"][2][1] == 0
    ctx.close()


# ---------------------------------------------------------------------------------------------------- fuse
def _fuse(ctx, case):
    import torch
    from alvaar_amd import multi
    block = torch.from_numpy(rc.fuse_block(case)).cuda()
    s, i, keep, absorbed, rounds = multi.fuse_duplicates_rounds(block, ctx, case["max_dist"], case["max_hamming"])
    assert np.array_equal(s.cpu().numpy(), case["stream"]) and np.array_equal(i.cpu().numpy(), case["ids"])
    return keep.cpu().numpy(), absorbed.cpu().numpy().astype(np.int64), rounds


def _assert_fuse_equals_the_sequential_rule(ctx, case):
    from map_merge_ref import fuse_duplicates_sequential
    keep, absorbed, rounds = _fuse(ctx, case)
    rk, ra = fuse_duplicates_sequential(case["stream"], case["ids"], case["xyz"], case["desc"], case["max_dist"], case["max_hamming"])
    assert np.array_equal(keep, rk), (case["name"], np.flatnonzero(keep != rk))
    assert np.array_equal(absorbed, ra), (case["name"], np.flatnonzero(absorbed != ra), absorbed[absorbed != ra], ra[absorbed != ra])
    return rounds


@_by_name([c for c in FUSE if not c["aim"].get("error")])
def test_fuse_equals_the_sequential_rule(ctx, case):
    rounds = _assert_fuse_equals_the_sequential_rule(ctx, case)
    print(f"{case['name']}: {rounds} rounds")
    assert rounds == rc.fuse_fixed_point(case)[2]
    if "min_rounds" in case["aim"]:
        assert rounds >= 3


def test_fuse_refuses_a_33rd_candidate_and_the_context_stays_usable():
    import alvaar_amd
    from alvaar_amd.capi import AlvaError
    ctx = alvaar_amd.Context(0)
    by = {c["name"]: c for c in FUSE}
    with pytest.raises(AlvaError, match="more than 32 candidates"):
        _fuse(ctx, by["candidates_33"])
    _assert_fuse_equals_the_sequential_rule(ctx, by["candidates_32"])
    ctx.close()


# ---------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("n_slots", rc.PACK_SLOT_COUNTS)
def test_pack_map_records_equals_the_host_filter(ctx, n_slots):
    import torch
    from alvaar_amd import capi
    c = rc.pack_case(n_slots)
    rec, want, stream_id = c["records"], c["want"], 3
    store = capi.MedoidStore(ctx)
    store.replay(c["ops"], n_slots)
    chunks = [torch.from_numpy(rec[a:a + 4096].view(np.uint8).copy()).cuda() for a in range(0, len(rec), 4096)]
    table = torch.tensor([ch.data_ptr() for ch in chunks], dtype=torch.int64).cuda()
    # the expected set: the host filter over the records and the tables' export
    desc, valid, info = store.export(np.arange(n_slots)) if n_slots else (np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8), np.zeros((0, 3), np.int32))
    slots = rc.pack_host_filter(rec, n_slots, valid, info[:, 0])
    expected = {int(rec[s]["id"]): (rec[s]["X"].copy().view(np.uint64).tolist(), bytes(desc[s])) for s in slots}
    assert expected == want and not info[:, 2].any()                      # ... which is the set the case was built to give
    unused = np.zeros(64, np.uint8)
    unused[4:8] = 255
    for cap in c["capacities"]:
        out = torch.full((cap + 2, 64), 0xAB, dtype=torch.uint8).cuda()      # two guard rows behind the capacity
        count = store.pack_records(table, n_slots, stream_id, cap, out)
        rows = out.cpu().numpy()
        assert count == len(want), (cap, count)                              # below capacity too: the true total
        assert (rows[cap:] == 0xAB).all()                                    # at most `capacity` rows written
        written = rows[:min(count, cap)]
        ids = rc.row_ids(written).tolist()
        assert len(set(ids)) == len(ids) and set(ids) <= set(want)           # distinct members of the expected set
        for r in written:
            xyz, med = want[int(r[4:8].copy().view(np.int32)[0])]
            assert int(r[0:4].copy().view(np.int32)[0]) == stream_id
            assert r[8:32].copy().view(np.uint64).tolist() == xyz and bytes(r[32:64]) == med
        if cap >= count:
            assert sorted(ids) == sorted(want)
            assert (rows[count:cap] == unused).all()                         # zero, id -1
    store.close()


# ---------------------------------------------------------------------------------------------------- medoid store
SEQS = ("growth+ties", "random", "release+reuse")


@pytest.mark.ref
@pytest.mark.parametrize("cut", rc.MEDOID_CUTS)
@pytest.mark.parametrize("name", SEQS)
def test_medoid_chains_cut_into_launches_equal_the_per_operation_expectation(ctx, name, cut):
    from alvaar_amd import capi
    log = rc.medoid_cut_log(name, cut)
    store = capi.MedoidStore(ctx)
    for k, (ops, want) in enumerate(zip(log["launches"], log["border"])):
        store.replay(ops, 16)
        if want is not None:
            assert rc.same_table(store.dump(rc.POINT), want), (log["name"], k)
    assert rc.same_table(store.dump(rc.POINT), log["final"])
    desc, valid, info = store.export([rc.POINT, rc.BYSTANDER])
    med, has, bk, entries = log["final"]
    assert bool(valid[0]) == has and info[0, 0] == len(entries) and (not has or np.array_equal(desc[0], med))
    assert info[1, 0] == log["bystander_count"] and not info[:, 2].any()
    store.close()


@pytest.mark.ref
def test_medoid_300_points_interleaved_in_one_launch(ctx):
    from alvaar_amd import capi
    log, slots, final = rc.medoid_many_points()
    assert len(final) == 300
    store = capi.MedoidStore(ctx)
    store.replay(log, slots)
    for slot, want in final.items():
        assert rc.same_table(store.dump(slot), want), slot
    fresh = store.dump(0)                                                     # a slot between the touched ones
    assert not fresh[1] and fresh[2] == [] and fresh[3] == 1 and not fresh[4]
    store.close()


@pytest.mark.ref
def test_medoid_store_growth_keeps_the_old_tables_and_resets_the_new(ctx):
    from alvaar_amd import capi
    log = rc.medoid_cut_log("growth+ties", 7)
    store = capi.MedoidStore(ctx)
    for ops in log["launches"][:12]:
        store.replay(ops, 16)
    old = [store.dump_raw(s) for s in range(16)]
    assert len(store.dump(rc.POINT)[2]) > 5 and len(store.dump(rc.BYSTANDER)[2]) > 5
    d = np.arange(32, dtype=np.uint8)
    store.replay([(8999, 0, 4, d, 13)], 9000)                                 # past the first 8 192 slots
    for s in range(16):
        assert np.array_equal(store.dump_raw(s), old[s]), s
    for s in (16, 8191, 8192, 8998, 9000, 16383):
        raw = store.dump_raw(s)
        med, has, entries, bk, over = rc.table_view(raw)
        assert not has and entries == [] and bk == 1 and not over and raw[:32].view(np.int32)[2] == 0, s
    med, has, entries, bk, over = store.dump(8999)
    assert has and np.array_equal(med, d) and entries == [(4, 0.0)] and bk == 13 and not over
    for ops in log["launches"][12:]:                                          # the old tables live on in the new block
        store.replay(ops, 9000)
    assert rc.same_table(store.dump(rc.POINT), log["final"])
    store.close()


@pytest.mark.ref
def test_medoid_overflow_flag_is_sticky_until_reset(ctx):
    from alvaar_amd import capi
    for log in rc.medoid_overflow_logs():
        store = capi.MedoidStore(ctx)
        bystander = [rc._bystander_op(k) for k in range(20)]
        store.replay([(rc.POINT, 3, -1, None, 0), (rc.BYSTANDER, 3, -1, None, 0)] + bystander[:10] + log["fill"], 16)
        before, other = store.dump_raw(rc.POINT), store.dump_raw(rc.BYSTANDER)
        assert rc.same_table(rc.table_view(before), log["want"]) and len(rc.table_view(before)[2]) == log["count"]
        store.replay([log["over"]], 16)
        after = store.dump_raw(rc.POINT)
        assert rc.table_view(after)[4], log["name"]                           # the flag ...
        desc, valid, info = store.export([rc.POINT, rc.BYSTANDER])
        assert info[0, 2] == 1 and info[1, 2] == 0 and info[0, 0] == log["count"] and info[1, 0] == 10   # ... reported by the export
        after[rc.OVERFLOW_BYTES] = 0
        assert np.array_equal(after, before), log["name"]                     # the table otherwise as after the last good insert
        assert np.array_equal(store.dump_raw(rc.BYSTANDER), other)            # the bystander untouched
        store.replay([(rc.POINT, 2, -1, None, 0)] + bystander[10:], 16)       # OP_CLEAR: the flag stays
        med, has, entries, bk, over = store.dump(rc.POINT)
        assert over and not has and entries == [] and bk == log["want"][2]
        assert len(store.dump(rc.BYSTANDER)[2]) == 20 and not store.dump(rc.BYSTANDER)[4]
        store.replay([(rc.POINT, 3, -1, None, 0)], 16)                        # OP_RESET: a freshly constructed map point
        med, has, entries, bk, over = store.dump(rc.POINT)
        assert not over and not has and entries == [] and bk == 1
        assert store.export([rc.POINT])[2][0, 2] == 0
        store.close()
