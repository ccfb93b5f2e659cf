"""GPU: alva_bf_match_hamming_batch (k_bf_partial_b / k_bf_final_b) against the CPU oracle, match by match.

The matcher is integer-exact, so every comparison is an equality: rows [0, min(*d_n_query, cap_query)) of idx / dist equal
Orc.bf_match (and Ref.bf_match where the compiled reference is built), rows beyond them still hold the value the test put there.
The shapes are the ones the detector lane of the tracker never produces: query counts of 0, 1, below / at / above one wave and above
cap_query, train counts at and around the 64-row LDS chunk and the 256-row workgroup tile, matches without a train set beside matches
with one, grids far smaller and far larger than the query count, and camera counts on both sides of alva_xcd_item's switch at 8."""
import functools

import numpy as np
import pytest

from oracles import Orc, Ref, ref_available

pytestmark = pytest.mark.gpu

CAP = 320
FILL = -7
NQ = [0, 1, 63, 64, 65, 300, 320, 325, 17]
NT = [513, 0, 1, 64, 255, 256, 257, 1100, 0]


@functools.lru_cache(maxsize=None)
def _match(seed, nq, nt, identical=False):
    """one match's data and its answer, computed once: (query [max(nq, 1), 32], train [nt, 32], oracle idx, oracle dist, planted
    [(query row, train index, distance)]).  Random bytes with planted rows; the oracle's answer covers the rows the call may
    write, [0, min(nq, CAP)), and is None where there are none."""
    rng = np.random.RandomState(1000 + seed)
    q = rng.randint(0, 256, (max(nq, 1), 32)).astype(np.uint8)
    t = rng.randint(0, 256, (nt, 32)).astype(np.uint8)
    if identical:
        t[:] = t[0]
    # equal train rows on both sides of an LDS chunk boundary (63 | 64), of a workgroup tile boundary (255 | 256), and in a later tile
    if nt > 256:
        t[256] = t[255]
    if nt > 700:
        t[64] = t[63]
        t[700] = t[63]
    n = min(nq, CAP)
    planted = []
    if n and nt:
        one_bit = np.zeros(32, np.uint8)
        one_bit[seed % 32] = 1 << (seed % 8)
        rows = [(t[0], 0, 0)]                                        # an exact copy
        if nt == 1 or identical:
            rows += [(~t[0], 0, 256)]                                # the complement of the only row there is: the largest key, 256 << 20
        if identical:
            rows += [(t[nt - 1] ^ one_bit, 0, 1)]                    # a tie of every train row: the lowest index wins
        if nt > 256 and not identical:
            rows += [(t[255], 255, 0), (t[256] ^ one_bit, 255, 1)]   # the tie crosses workgroups
        if nt > 700 and not identical:
            rows += [(t[700], 63, 0), (t[64] ^ one_bit, 63, 1)]      # ... and crosses LDS chunks
        # from the last row downwards (the last query block's last lanes) and, where there is room for both, from row 0 upwards
        for k, (row, idx, dist) in enumerate(rows):
            for at in ([n - 1 - k, k] if n >= 2 * len(rows) else [n - 1 - k]):
                if at >= 0:
                    q[at] = row
                    planted.append((at, idx, dist))
    if n == 0 or nt == 0:
        return q, t, None, None, planted
    oi, od = Orc.bf_match(q[:n], t)
    if ref_available():
        ri, rd = Ref.bf_match(q[:n], t)
        assert np.array_equal(oi, ri) and np.array_equal(od, rd)
    for at, idx, dist in planted:   # the oracle itself gives the planted answers
        assert oi[at] == idx and od[at] == dist, (seed, nq, nt, at)
    return q, t, oi, od, planted


def _run(ctx, specs, expected_queries, with_null=True):
    """one batch call on [(seed, nq, nt, identical)]; returns per match (idx, dist) as numpy (None for a match passed as all-NULL)"""
    import torch
    from alvaar_amd import capi
    data = [_match(*s) for s in specs]
    qs, nqd, ts, idx, dist = [], [], [], [], []
    for (seed, nq, nt, *_), (q, t, *_) in zip(specs, data):
        if nt == 0 and with_null:
            for lst in (qs, nqd, ts, idx, dist):
                lst.append(None)
            continue
        qs.append(torch.from_numpy(q).cuda())
        nqd.append(torch.tensor([nq], dtype=torch.int32, device="cuda"))
        ts.append(torch.from_numpy(t).cuda() if nt else None)
        idx.append(torch.full((CAP,), FILL, dtype=torch.int32, device="cuda"))
        dist.append(torch.full((CAP,), FILL, dtype=torch.int32, device="cuda"))
    capi.bf_match_hamming_batch(ctx, qs, nqd, CAP, ts, [s[2] for s in specs], idx, dist, expected_queries)
    ctx.sync()
    return [(None, None) if i is None else (i.cpu().numpy(), d.cpu().numpy()) for i, d in zip(idx, dist)]


def _check(specs, got):
    for c, (spec, (idx, dist)) in enumerate(zip(specs, got)):
        seed, nq, nt = spec[:3]
        if idx is None:
            assert nt == 0
            continue
        n = min(nq, CAP) if nt else 0
        q, t, oi, od, planted = _match(*spec)
        if n:
            assert np.array_equal(idx[:n], oi), (c, spec, np.flatnonzero(idx[:n] != oi)[:8])
            assert np.array_equal(dist[:n], od), (c, spec, np.flatnonzero(dist[:n] != od)[:8])
        assert np.array_equal(idx[n:], np.full(CAP - n, FILL, np.int32)), (c, spec)   # rows beyond the query count: untouched
        assert np.array_equal(dist[n:], np.full(CAP - n, FILL, np.int32)), (c, spec)


RAGGED = [(100 + c, NQ[c], NT[c]) for c in range(9)]


def test_ragged_matrix_in_one_call(ctx):
    """nine matches of every size class in one call; 325 queries are clamped to cap_query = 320, the match with 0 queries and 513 train
    rows writes nothing, the two matches without a train set are NULL in every pointer table"""
    got = _run(ctx, RAGGED, 300)
    assert got[1] == (None, None) and got[8] == (None, None)
    _check(RAGGED, got)
    # the planted rows, stated: exact copy -> 0; complement -> 256; equal train rows -> the lowest index, across chunks and workgroups
    idx, dist = got[7]                                    # 320 of 325 queries x 1100 train rows
    want = set(_match(*RAGGED[7])[4])
    assert {(i, d) for _, i, d in want} == {(0, 0), (255, 0), (255, 1), (63, 0), (63, 1)}
    assert all(idx[at] == i and dist[at] == d for at, i, d in want)
    idx, dist = got[2]                                    # 63 queries x 1 train row
    want = set(_match(*RAGGED[2])[4])
    assert {(i, d) for _, i, d in want} == {(0, 0), (0, 256)} and all(idx[at] == i and dist[at] == d for at, i, d in want)


def test_independent_popcount(ctx):
    """the same call against a popcount written here (np.unpackbits), not against either oracle library"""
    specs = [RAGGED[5], RAGGED[6], RAGGED[7]]            # 300 x 256, 320 x 257, 325 -> 320 x 1100
    got = _run(ctx, specs, 300)
    for spec, (idx, dist) in zip(specs, got):
        q, t = _match(*spec)[:2]
        n = min(spec[1], CAP)
        d = np.unpackbits(q[:n, None, :] ^ t[None, :, :], axis=2).sum(axis=2, dtype=np.int32)   # [n, nt]
        want_idx = d.argmin(axis=1).astype(np.int32)     # argmin keeps the first minimum: the lowest train index
        assert np.array_equal(idx[:n], want_idx) and np.array_equal(dist[:n], d[np.arange(n), want_idx])
        assert np.array_equal(idx[n:], np.full(CAP - n, FILL, np.int32)) and np.array_equal(dist[n:], np.full(CAP - n, FILL, np.int32))


@pytest.mark.parametrize("expected", [1, 64, 200, 10000])
def test_grid_sizing(ctx, expected):
    """expected_queries only sizes the grid: 1 makes every workgroup loop five times over 300 queries (and one block of k_bf_final_b
    loop twice over 320), 10000 is clamped to divup(cap_query, 64) query blocks; the answers are the same"""
    _check(RAGGED, _run(ctx, RAGGED, expected))


def _mapping_specs(count):
    return [(c, NQ[(c + 5) % 9], NT[(2 * c) % 9]) for c in range(count)]


@pytest.mark.parametrize("count", [1, 3, 7, 8, 9, 16, 17])
def test_camera_to_workgroup_mapping(ctx, count):
    """alva_xcd_item: below 8 matches workgroup L serves match L / per_cam, from 8 on match 8 * (L / 8 / per_cam) + L % 8 of a grid
    padded to a multiple of 8 matches (the padding returns).  Every match has its own data, so a swapped or dropped index shows."""
    specs = _mapping_specs(count)
    got = _run(ctx, specs, 200)
    _check(specs, got)


def test_identical_train_rows(ctx):
    """every train row the same: every query's answer is train row 0, from every chunk and every workgroup tile"""
    specs = [(50, 300, 1100, True), (51, 65, 257, True), (52, 17, 64, True)]
    got = _run(ctx, specs, 300)
    _check(specs, got)
    for spec, (idx, dist) in zip(specs, got):
        assert np.array_equal(idx[:spec[1]], np.zeros(spec[1], np.int32))
        assert all(idx[at] == i and dist[at] == d for at, i, d in _match(*spec)[4]) and 256 in dist[:spec[1]]


def test_nothing_to_do(ctx):
    # no match has a train set: ALVA_OK before anything is launched, outputs as they were (here real tensors, not NULL)
    specs = [(60, 300, 0), (61, 17, 0), (62, 0, 0)]
    for idx, dist in _run(ctx, specs, 300, with_null=False):
        assert np.array_equal(idx, np.full(CAP, FILL, np.int32)) and np.array_equal(dist, np.full(CAP, FILL, np.int32))
    # ... and the same call with every pointer of every match NULL
    assert _run(ctx, specs, 300) == [(None, None)] * 3
    # train sets present, every device query count 0: launched, and nothing written
    specs = [(63, 0, 513), (64, 0, 64), (65, 0, 1)]
    for idx, dist in _run(ctx, specs, 300):
        assert np.array_equal(idx, np.full(CAP, FILL, np.int32)) and np.array_equal(dist, np.full(CAP, FILL, np.int32))


def test_equals_the_single_call(ctx):
    """a batch of three against three alva_bf_match_hamming calls.  The one contract difference is not exercised here: for
    n_train == 0 the single call writes -1 into idx and dist of every query, the batch skips that match and writes nothing."""
    import torch
    specs = [(70, 300, 1100), (71, 65, 257), (72, 17, 64)]
    got = _run(ctx, specs, 300)
    for spec, (idx, dist) in zip(specs, got):
        q, t = _match(*spec)[:2]
        i1, d1 = ctx.bf_match_hamming(torch.from_numpy(q[:spec[1]]).cuda(), torch.from_numpy(t).cuda())
        assert np.array_equal(idx[:spec[1]], i1.cpu().numpy()) and np.array_equal(dist[:spec[1]], d1.cpu().numpy())
    _check(specs, got)


def test_argument_errors(ctx):
    """each returns non-zero with a message before anything is launched: the outputs keep the test's fill"""
    import torch
    import alvaar_amd
    from alvaar_amd import capi
    q, t = (torch.from_numpy(a).cuda() for a in _match(80, 65, 257)[:2])
    nq = torch.tensor([65], dtype=torch.int32, device="cuda")
    idx = torch.full((CAP,), FILL, dtype=torch.int32, device="cuda")
    dist = torch.full((CAP,), FILL, dtype=torch.int32, device="cuda")
    raw = torch.zeros(8 + 65 * 32, dtype=torch.uint8, device="cuda")
    q_off8 = raw[8:].view(65, 32)                        # rows 8 bytes off the 16-byte alignment the kernels' b128 loads need
    assert q_off8.data_ptr() % 16 == 8
    bad = {
        "count = 0": ([], [], CAP, [], [], [], []),
        "cap_query = 0": ([q], [nq], 0, [t], [257], [idx], [dist]),
        "n_train = 1 << 20": ([q], [nq], CAP, [t], [1 << 20], [idx], [dist]),
        "query off by 8 bytes": ([q_off8], [nq], CAP, [t], [257], [idx], [dist]),
        "NULL train with n_train > 0": ([q], [nq], CAP, [None], [257], [idx], [dist]),
        "a bad match behind a good one": ([q, q], [nq, nq], CAP, [t, None], [257, 5], [idx, idx], [dist, dist]),
    }
    for what, args in bad.items():
        with pytest.raises(alvaar_amd.AlvaError, match="bad argument") as e:
            capi.bf_match_hamming_batch(ctx, *args, 300)
        assert "alvaar_hip error" in str(e.value), what
        ctx.sync()
        assert int((idx != FILL).sum()) == 0 and int((dist != FILL).sum()) == 0, what
