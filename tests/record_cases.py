"""TEST INFRASTRUCTURE: case tables for the 64-byte map-record block {i32 stream, i32 id, f64 xyz[3], u8 medoid[32]} and the chain around it
-- the descriptor tables that produce the medoid (medoid.hip), the kernel that writes the block (alva_pack_map_records), and its two
readers, relocalization (alva_reloc_match) and the shared-map fuse (alva_fuse_map_points) -- with the numpy statement of each operation.
Everything is integer or bitwise: every comparison made against these tables is equality.

No GPU is needed to build a case.  test_record_cases.py shows that the numpy statements alone produce what each case aims at (so that no
device test passes vacuously); test_gpu_map_records.py runs the kernels on the same cases."""
from __future__ import annotations

import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)


# ---------------------------------------------------------------------------------------------------- relocalization: the statement
def _brute_force(q, qvalid, rows, max_dist=51, ratio=0.8):
    """(query, id, distance) of the accepted one-to-one pairs in ascending query index -- the definition in alvaar_hip.h
    (qvalid None = every query valid)"""
    ids = rows[:, 4:8].copy().view(np.int32)[:, 0]
    live = np.nonzero(ids >= 0)[0]
    rd, rid = rows[live, 32:64], ids[live]
    best = {}
    for q0 in range(0, len(q), 128):
        d = _POP[q[q0:q0 + 128, None, :] ^ rd[None, :, :]].sum(-1, dtype=np.int32)   # [chunk][live rows]
        for i in range(d.shape[0]):
            qi = q0 + i
            if (qvalid is not None and not qvalid[qi]) or d.shape[1] == 0:
                continue
            order = np.lexsort((rid, d[i]))
            b = order[0]
            second = int(d[i][order[1]]) if len(order) > 1 else 257
            bd = int(d[i][b])
            if bd <= max_dist and np.float32(bd) < np.float32(ratio) * np.float32(second):
                best[qi] = (int(live[b]), bd)
    claim = {}
    for qi, (r, bd) in best.items():
        if r not in claim or (bd, qi) < claim[r]:
            claim[r] = (bd, qi)
    return [(qi, int(ids[r]), bd) for qi, (r, bd) in sorted(best.items()) if claim[r] == (bd, qi)]


def _flip(rng, desc, nbits, avoid=None):
    bits = np.unpackbits(desc)
    choice = np.setdiff1d(np.arange(256), avoid) if avoid is not None else np.arange(256)
    pos = rng.choice(choice, nbits, replace=False)
    bits[pos] ^= 1
    return np.packbits(bits), pos


def hamming(a, b):
    return int(_POP[np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)].sum())


def make_rows(ids, desc, xyz, stream=7):
    n = len(ids)
    rows = np.zeros((n, 64), np.uint8)
    rows[:, 0:4] = np.frombuffer(np.int32(stream).tobytes(), np.uint8)
    rows[:, 4:8] = np.ascontiguousarray(ids, np.int32).view(np.uint8).reshape(n, 4)
    rows[:, 8:32] = np.ascontiguousarray(xyz, np.float64).view(np.uint8).reshape(n, 24)
    rows[:, 32:64] = desc
    return rows


def row_ids(rows):
    return rows[:, 4:8].copy().view(np.int32)[:, 0]


# ---------------------------------------------------------------------------------------------------- relocalization: the launches
class _Launch:
    """random queries and rows (about 128 bits apart: nothing is accepted by chance at max_dist 51), into which a case plants the
    rows and queries that matter by flipping a chosen number of bits"""

    def __init__(self, name, nq, nr, seed, max_dist=51, ratio=0.8):
        self.name, self.max_dist, self.ratio = name, max_dist, ratio
        self.rng = rng = np.random.RandomState(seed)
        self.q = rng.randint(0, 256, (nq, 32)).astype(np.uint8)
        self.desc = rng.randint(0, 256, (nr, 32)).astype(np.uint8)
        self.ids = (rng.permutation(50 * max(nr, 1))[:nr] + 500_000_000).astype(np.int32)   # large: nothing may pack an id into few bits
        self.xyz = rng.randn(nr, 3)
        self.qvalid = None
        self.kept, self.rejected, self.ties = {}, [], []

    def query_near_row(self, qi, row, nbits, avoid=None):
        self.q[qi], used = _flip(self.rng, self.desc[row], nbits, avoid)
        return used

    def row_near_query(self, row, qi, nbits, avoid=None):
        self.desc[row], used = _flip(self.rng, self.q[qi], nbits, avoid)
        return used

    def keep(self, qi, row, dist):
        self.kept[qi] = (int(self.ids[row]), dist)

    def done(self, **aim):
        a = dict(kept=self.kept, rejected=self.rejected, ties=self.ties, none=False, same_as=None)
        a.update(aim)
        return dict(name=self.name, q=self.q, qvalid=self.qvalid, rows=make_rows(self.ids, self.desc, self.xyz), max_dist=self.max_dist,
                    ratio=self.ratio, aim=a)


QUERY_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
ROW_COUNTS = (1, 2, 63, 64, 65, 128, 129)


def _query_count_launch(nq, seed):
    """an accepted pair on both sides of every 64 border of the queries (the emit kernel's wave ballots, its 1024-query passes and their
    running base; the merge kernel's 256-query blocks), at the first and at the last query"""
    picked = sorted({0, nq - 1} | {b + o for b in range(64, nq + 1, 64) for o in (-1, 0) if b + o < nq})
    L = _Launch(f"queries_{nq}", nq, len(picked) + 2, seed)
    rows = L.rng.permutation(len(picked) + 1)   # one row stays unmatched, the last is unused
    for k, qi in enumerate(picked):
        L.query_near_row(qi, rows[k], k % 21)
        L.keep(qi, rows[k], k % 21)
    L.ids[-1] = -1
    L.rejected = [qi for qi in (1, 62, 66, 1022, 1026) if qi < nq - 1 and qi not in picked]
    return L.done()


def _row_count_launch(nr, seed):
    """pairs at the first and the last row and on both sides of the 64-row chunk borders"""
    targets = sorted({r for r in (0, nr - 1, 63, 64, 127, 128) if 0 <= r < nr})
    L = _Launch(f"rows_{nr}", len(targets) + 1, nr, seed)
    for k, r in enumerate(targets):
        L.query_near_row(k, r, 3 + k)
        L.keep(k, r, 3 + k)
    L.rejected = [len(targets)]
    return L.done()


def _single_live_row(name, nr, live_row, nbits, seed, accepted):
    """one live row: second = 257, accepted iff best < ratio * 257 (0.8 * 257 = 205.6).  Every unused row is a copy of the query, which
    would win at distance 0 if it were read; their ids are negative numbers of several kinds"""
    L = _Launch(name, 1, nr, seed, max_dist=256, ratio=0.8)
    L.query_near_row(0, live_row, nbits)
    unused = (-1, -2 ** 31, -7, -(2 ** 30))
    for r in range(nr):
        if r != live_row:
            L.desc[r] = L.q[0]
            L.ids[r] = unused[r % len(unused)]
    if accepted:
        L.keep(0, live_row, nbits)
    else:
        L.rejected = [0]
    return L.done(none=not accepted)


def _tie_launch(name, nr, tied, seed):
    """tied = [(row, id)]: every one of them `dist` bits from query 0 (different bits each); ratio 1.5 accepts best == second, so the
    winner -- the smallest id, which lies at a later row than a larger one -- is visible in the output"""
    dist = 12
    L = _Launch(name, 3, nr, seed, ratio=1.5)
    used = np.zeros(0, np.int64)
    for row, mp_id in tied:
        used = np.concatenate([used, L.row_near_query(row, 0, dist, avoid=used)])
        L.ids[row] = mp_id
    win = min(tied, key=lambda t: t[1])
    L.keep(0, win[0], dist)
    L.ties = [(0, win[0], [r for r, _ in tied if r != win[0]])]
    spare = next(r for r in range(nr) if r not in [t[0] for t in tied])
    L.query_near_row(2, spare, 9)
    L.keep(2, spare, 9)
    L.rejected = [1]
    return L.done()


def _ratio_boundary_launch(seed):
    """ratio 0.5 (exact in float): best 20 against second 40 is rejected (20 < 20 is false), best 19 is accepted; best and second lie in
    different 64-row chunks, in both orders, so the second distance is one that only the merge of the chunks' records can supply"""
    L = _Launch("ratio_boundary_across_chunks", 5, 129, seed, ratio=0.5)
    for qi, (best_row, nb, second_row) in enumerate(((10, 20, 100), (101, 19, 11), (128, 20, 12), (13, 19, 127))):
        used = L.row_near_query(best_row, qi, nb)
        L.row_near_query(second_row, qi, 40, avoid=used)
        if nb == 19:
            L.keep(qi, best_row, 19)
        else:
            L.rejected.append(qi)
    L.rejected.append(4)
    return L.done(boundary=[(0, 20, 40), (1, 19, 40), (2, 20, 40), (3, 19, 40)])


def _claims_launch(name, seed, qvalid):
    """claimants of one row in different 256-query blocks (the merge kernel's workgroups) and different 1024-query passes (the emit kernel)"""
    L = _Launch(name, 2049, 20, seed)
    for qi, row, nb in ((10, 4, 5), (300, 4, 5), (1500, 4, 5), (200, 9, 9), (1300, 9, 4), (2048, 11, 6), (5, 11, 6), (700, 15, 2)):
        L.query_near_row(qi, row, nb)
    if qvalid == "off":      # the would-be winners are switched off: the next claimant keeps the row
        L.qvalid = np.ones(2049, np.uint8)
        L.qvalid[[10, 1300]] = 0
        L.keep(300, 4, 5), L.keep(200, 9, 9)
        L.rejected = [10, 1500, 1300, 2048]
    else:
        L.qvalid = np.ones(2049, np.uint8) if qvalid == "ones" else None
        L.keep(10, 4, 5), L.keep(1300, 9, 4)   # equal distance: the smaller query index; else the smaller distance
        L.rejected = [300, 1500, 200, 2048]
    L.keep(5, 11, 6), L.keep(700, 15, 2)
    return L.done(same_as="claims_qvalid_none" if qvalid == "ones" else None)


def reloc_launches():
    out = [_query_count_launch(nq, 100 + i) for i, nq in enumerate(QUERY_COUNTS)]
    out += [_row_count_launch(nr, 200 + i) for i, nr in enumerate(ROW_COUNTS)]
    # ---- rows: one live row, unused chunks, unused ids other than -1
    out.append(_single_live_row("single_row_205_of_1", 1, 0, 205, 301, True))
    out.append(_single_live_row("single_row_206_of_65", 65, 64, 206, 302, False))         # chunk 0 all unused
    out.append(_single_live_row("single_row_205_of_129", 129, 70, 205, 303, True))        # chunks 0 and 2 all unused
    out.append(_single_live_row("single_row_206_of_2", 2, 1, 206, 304, False))
    L = _Launch("unused_chunk_between_live_chunks", 4, 129, 305)
    for r in range(64, 128):
        L.ids[r] = -1 if r % 2 else -2 ** 31
    for qi, (row, nb) in enumerate(((63, 4), (128, 6), (0, 0))):
        L.query_near_row(qi, row, nb)
        L.keep(qi, row, nb)
    L.desc[100] = L.q[3]                       # an unused row identical to query 3
    L.rejected = [3]
    out.append(L.done())
    L = _Launch("every_row_unused", 65, 65, 306, max_dist=256, ratio=1.5)
    L.ids[:] = -1
    L.ids[::3] = -2 ** 31
    L.desc[:] = L.q
    out.append(L.done(none=True))
    # ---- ties observed
    out.append(_tie_launch("tie_in_one_chunk", 40, [(10, 900), (20, 100)], 401))
    out.append(_tie_launch("tie_across_chunks", 100, [(5, 900), (70, 100)], 402))
    out.append(_tie_launch("tie_three_chunks", 129, [(3, 500), (80, 100), (128, 300)], 403))
    out.append(_ratio_boundary_launch(404))
    # ---- thresholds
    L = _Launch("max_dist_0", 3, 10, 501, max_dist=0)
    L.query_near_row(0, 4, 0), L.keep(0, 4, 0)
    L.query_near_row(1, 5, 1)
    L.rejected = [1, 2]
    out.append(L.done())
    L = _Launch("max_dist_256", 2, 3, 502, max_dist=256)   # query 0: 150 < 0.8 * 200; its complement: 26 < 0.8 * 56
    for row, nb in ((0, 150), (1, 200), (2, 230)):
        L.row_near_query(row, 0, nb)
    L.q[1] = ~L.q[0]
    L.keep(0, 0, 150), L.keep(1, 2, 26)
    out.append(L.done())
    for md, ok in ((256, True), (255, False)):               # the complement of the only row: distance 256 < 1.5 * 257
        L = _Launch(f"complement_at_max_dist_{md}", 1, 1, 503, max_dist=md, ratio=1.5)
        L.q[0] = ~L.desc[0]
        if ok:
            L.keep(0, 0, 256)
        else:
            L.rejected = [0]
        out.append(L.done(none=not ok))
    L = _Launch("ratio_0", 3, 10, 504, ratio=0.0)
    L.query_near_row(0, 3, 0), L.query_near_row(1, 6, 5)
    L.rejected = [0, 1, 2]
    out.append(L.done(none=True))
    L = _Launch("best_at_max_dist_and_one_over", 3, 12, 505, max_dist=37)
    L.query_near_row(0, 2, 37), L.keep(0, 2, 37)
    L.query_near_row(1, 6, 38)
    L.rejected = [1, 2]
    out.append(L.done())
    # ---- one-to-one claims
    out.append(_claims_launch("claims_qvalid_none", 601, None))
    out.append(_claims_launch("claims_qvalid_ones", 601, "ones"))
    out.append(_claims_launch("claims_winner_invalid", 601, "off"))
    assert len({c["name"] for c in out}) == len(out)
    assert all(len(c["q"]) <= 2049 and len(c["rows"]) <= 129 for c in out)
    return out


def permuted_rows(launch):
    """the launch's rows in one fixed other order"""
    perm = np.random.RandomState(77).permutation(len(launch["rows"]))
    return np.ascontiguousarray(launch["rows"][perm])


# ---------------------------------------------------------------------------------------------------- shared-map fuse
class _Fuse:
    """records added stream by stream; ids count up per stream in the order of the calls, so within a stream the records keep that order"""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.recs, self.next_id = [], {}

    def desc(self):
        return self.rng.randint(0, 256, 32).astype(np.uint8)

    def near(self, d, nbits):
        return _flip(self.rng, d, nbits)[0]

    def add(self, stream, xyz, desc, label=None):
        i = self.next_id.get(stream, 0)
        self.next_id[stream] = i + 1
        self.recs.append((stream, i, np.asarray(xyz, np.float64), np.asarray(desc, np.uint8), label))

    def fill(self, stream, n):   # isolated records far from everything a case places (those lie inside the unit cube around 0)
        for _ in range(n):
            self.add(stream, self.rng.uniform(10, 60, 3), self.desc())

    def done(self, name, max_dist=0.05, max_hamming=51, **aim):
        order = sorted(range(len(self.recs)), key=lambda k: self.recs[k][:2])
        r = [self.recs[k] for k in order]
        index = {rec[4]: i for i, rec in enumerate(r) if rec[4] is not None}
        return dict(name=name, stream=np.array([x[0] for x in r], np.int32), ids=np.array([x[1] for x in r], np.int32),
                    xyz=np.array([x[2] for x in r], np.float64).reshape(-1, 3), desc=np.array([x[3] for x in r], np.uint8).reshape(-1, 32),
                    max_dist=max_dist, max_hamming=max_hamming, index=index, aim=aim)


def fuse_candidates(case, i):
    """[(record, hamming)] of the earlier records of other streams within the radius and the Hamming bound, ascending record index,
    whether they survive or not: what k_fuse_candidates lists for record i"""
    st, xyz, desc = case["stream"], case["xyz"], case["desc"]
    out = []
    for j in range(i):
        if st[j] != st[i] and ((xyz[j] - xyz[i]) ** 2).sum() <= case["max_dist"] ** 2:
            h = hamming(desc[j], desc[i])
            if h <= case["max_hamming"]:
                out.append((j, h))
    return out


def fuse_fixed_point(case):
    """the rule evaluated the way map_merge.hip does: every record takes its best candidate among those that survived the previous
    round, until no verdict changes.  Returns (keep, absorbed_by, rounds)."""
    n = len(case["ids"])
    cands = [fuse_candidates(case, i) for i in range(n)]
    keep = np.ones(n, bool)
    rounds = 0
    while True:
        new, absorbed = np.ones(n, bool), -np.ones(n, np.int64)
        for i in range(n):
            alive = [(h, j) for j, h in cands[i] if keep[j]]
            if alive:
                new[i], absorbed[i] = False, min(alive)[1]
        rounds += 1
        changed = not np.array_equal(new, keep)
        keep = new
        if not changed:
            return keep, absorbed, rounds


def _hamming_case(mh, seed):
    """a record with two surviving candidates, one near and one at the far end of the bound (for max_hamming >= 128: at 128 or more bits,
    where a distance kept in the top byte of a signed word turns negative); the far one lies earlier in one group and later in the other.
    The candidates are 0.08 apart, so neither absorbs the other.  Plus a lone candidate exactly at the bound and one a bit over it."""
    f = _Fuse(seed)
    h_near, h_far = (0, 1) if mh == 0 else (5, mh)
    pairs = []
    for g, (s_far, s_near) in enumerate(((0, 1), (1, 0))):
        p, t = np.array([0.5 * g, 0.2, -0.1]), f.desc()
        f.add(s_far, p + [0.04, 0, 0], f.near(t, h_far), f"far{g}")
        f.add(s_near, p - [0.04, 0, 0], f.near(t, h_near), f"near{g}")
        f.add(2, p, t, f"rec{g}")
        pairs.append((f"rec{g}", f"near{g}", f"far{g}"))
    t = f.desc()
    f.add(0, [0.1, 0.7, 0.3], f.near(t, mh), "lone_at")
    f.add(3, [0.1, 0.7, 0.3], t, "rec_at")
    over = None
    if mh < 256:
        t = f.desc()
        f.add(1, [-0.6, 0.7, 0.3], f.near(t, mh + 1), "lone_over")
        f.add(3, [-0.6, 0.7, 0.3], t, "rec_over")
        over = "rec_over"
    for s in range(4):
        f.fill(s, 3)
    return f.done(f"max_hamming_{mh}", max_hamming=mh, pairs=pairs, h_near=h_near, h_far=h_far, absorbed_at="rec_at", survives=over)


def _cap_case(ncand, seed):
    """ncand candidates for one record, all of stream 0 (they cannot absorb one another), lying at records 50 .. 50 + ncand + 5 -- on both
    sides of the 64-record border of the candidate scan -- among decoys inside the radius whose descriptors are far; the smallest distance
    is the LAST candidate's, the second smallest is shared by two"""
    f = _Fuse(seed)
    t, p = f.desc(), np.array([0.3, -0.2, 0.6])
    f.fill(0, 50)
    for k in range(ncand):
        h = 1 if k == ncand - 1 else (6 if k in (3, 20) else 8 + (k * 7) % 40)
        f.add(0, p + f.rng.uniform(-0.01, 0.01, 3), f.near(t, h), f"cand{k}")
        if k % 6 == 0:
            f.add(0, p + f.rng.uniform(-0.01, 0.01, 3), f.desc())          # a decoy: inside the radius, ~128 bits away
    f.fill(0, 5)
    f.add(1, p, t, "rec")
    f.fill(1, 4)
    return f.done(f"candidates_{ncand}", n_candidates=ncand, error=ncand > 32, winner=f"cand{ncand - 1}")


def _cluster_case(n, seed):
    """n records over up to four streams around a few physical points: plain duplicates"""
    f = _Fuse(seed)
    nb = max(1, n // 3)
    base_p, base_d = f.rng.uniform(-0.9, 0.9, (nb, 3)) * 5, [f.desc() for _ in range(nb)]
    for i in range(n):
        b = i % nb
        f.add(i * min(n, 4) // n, base_p[b] + f.rng.normal(0, 0.008, 3), f.near(base_d[b], int(f.rng.randint(0, 21))))
    return f.done(f"records_{n}", some_absorbed=n >= 3)


def _border_case(seed):
    """129 records.  Two records of stream 1 have eight candidates each at records 56 .. 71 of stream 0 (alternating), four before and four
    after the 64-record border of the scan: one has its single best candidate behind the border, the other two equal best candidates, one
    on each side -- the earlier must win, which holds only if the compacted list keeps the ascending record order"""
    f = _Fuse(seed)
    ta, tb = f.desc(), f.desc()
    pa, pb = np.array([0.2, 0.2, 0.2]), np.array([-0.5, 0.1, 0.4])
    f.fill(0, 56)
    for k, (ha, hb) in enumerate(zip((30, 25, 9, 28, 4, 26, 9, 31), (30, 25, 9, 28, 27, 9, 26, 31))):
        f.add(0, pa + f.rng.uniform(-0.01, 0.01, 3), f.near(ta, ha), f"a{k}")
        f.add(0, pb + f.rng.uniform(-0.01, 0.01, 3), f.near(tb, hb), f"b{k}")
    f.fill(0, 28)
    f.add(1, pa, ta, "rec_a")
    f.add(1, pb, tb, "rec_b")
    f.fill(1, 27)
    return f.done("records_129_candidates_across_the_64_border", winners={"rec_a": "a4", "rec_b": "b2"})


def _chain_case(seed):
    """Seven streams.  R0 .. R6 on a line 0.04 apart (each sees only its predecessor, 20 bits away).  From R2 on every link's FIRST choice
    is a decoy 3 bits away that a record of stream 0 has absorbed, so the verdict falls to the predecessor: R1 absorbed, R2 survives (both
    its candidates are gone), R3 absorbed by R2, R4 survives, ...  -- the verdict of R6 depends on all links before it."""
    f = _Fuse(seed)
    d = [f.desc()]
    for k in range(1, 7):
        d.append(f.near(d[-1], 20))
    decoy = {k: f.near(d[k], 3) for k in range(2, 7)}
    for k in range(2, 7):                                                   # the anchors that absorb the decoys: stream 0
        side = 1.0 if k % 2 else -1.0
        f.add(0, [0.04 * k, 0.08 * side, 0], decoy[k], f"anchor{k}")
    f.add(0, [0, 0, 0], d[0], "R0")
    for k in range(1, 7):
        if k + 1 in decoy:                                                 # the decoy of link k + 1 lives in stream k
            side = 1.0 if (k + 1) % 2 else -1.0
            f.add(k, [0.04 * (k + 1), 0.04 * side, 0], decoy[k + 1], f"decoy{k + 1}")
        f.add(k, [0.04 * k, 0, 0], d[k], f"R{k}")
    for s in range(7):
        f.fill(s, 2)
    return f.done("absorption_chain", links=[(f"R{k}", f"decoy{k}") for k in range(2, 7)],
                  verdicts={f"R{k}": (k % 2 == 0) for k in range(7)}, min_rounds=3)


def _coincident_case(seed):
    f = _Fuse(seed)
    t, u = f.desc(), f.desc()
    p, q = np.array([0.25, -0.5, 0.125]), np.array([-0.3, 0.3, 0.7])
    f.add(0, p, t, "a")
    f.add(1, p, f.near(t, 4), "same_place")              # absorbed
    f.add(2, p.copy(), f.near(t, 4), "same_place_2")     # absorbed by "a" too: "same_place" did not survive
    f.add(0, q, u, "b")
    f.add(1, q + [1e-9, 0, 0], f.near(u, 4), "a_nanometre_off")   # survives
    f.add(2, [q[0], q[1], np.nextafter(q[2], 1)], f.near(u, 4), "one_ulp_off")   # survives
    f.fill(0, 2), f.fill(1, 2)
    return f.done("max_dist_0", max_dist=0.0, absorbed={"same_place": "a", "same_place_2": "a"}, survive=["a_nanometre_off", "one_ulp_off"])


def fuse_cases():
    out = [_hamming_case(mh, 700 + i) for i, mh in enumerate((0, 127, 128, 200, 256))]
    out += [_cap_case(32, 710), _cap_case(33, 711), _coincident_case(712)]
    out += [_cluster_case(n, 720 + i) for i, n in enumerate((1, 3, 4, 5, 64, 65))]
    out += [_border_case(730), _chain_case(731)]
    for c in out:
        assert np.array_equal(np.lexsort((c["ids"], c["stream"])), np.arange(len(c["ids"])))
    return out


def fuse_block(case):
    """the case as one block of 64-byte records (what alvaar_amd.multi.fuse_duplicates takes), with some unused rows in between"""
    n = len(case["ids"])
    rows = make_rows(case["ids"], case["desc"], case["xyz"])
    rows[:, 0:4] = case["stream"].view(np.uint8).reshape(n, 4)
    pad = make_rows(-np.ones(2, np.int32), np.zeros((2, 32), np.uint8), np.zeros((2, 3)), stream=0)
    return np.concatenate([rows[:n // 2], pad, rows[n // 2:], pad])


# ---------------------------------------------------------------------------------------------------- record packing
PACK_KINDS = ("live", "free", "not3d", "nodesc", "unwritten", "cleared")
PACK_SLOT_COUNTS = (0, 1, 255, 256, 257, 4101)


def pack_case(n_slots, seed=None):
    """n_slots map-point records (Context.mp_record_dtype(), 4096 per chunk) and the medoid log that gives their tables.  Every kind but
    "live" differs from a live record in exactly the one thing its filter reads: a free record (id -1), a record that is not 3-D, one with
    has_desc = 0, one whose table was never written, one whose table was cleared back to no medoid.  A live table gets one add, or two
    adds of different descriptors, after which the medoid is the second (MapPoint::addDesc: distance 0 to itself is the first strict
    minimum)."""
    from alvaar_amd.capi import Context
    rng = np.random.RandomState(800 + n_slots if seed is None else seed)
    rec = np.zeros(max(1, (n_slots + 4095) // 4096) * 4096, Context.mp_record_dtype())
    rec["id"] = -1
    kinds = [PACK_KINDS[k] for k in rng.choice(6, n_slots, p=[0.5, 0.1, 0.1, 0.1, 0.1, 0.1])]
    if n_slots >= 255:
        for k, s in enumerate(rng.permutation(n_slots - 2)[:6] + 1):
            kinds[s] = PACK_KINDS[k]
        kinds[0] = kinds[n_slots - 1] = "live"
    if n_slots == 1:
        kinds = ["live"]
    if n_slots > 4096:
        kinds[4095] = kinds[4096] = "live"
    ids = (rng.permutation(20 * max(n_slots, 1))[:n_slots] + 1_000).astype(np.int64)
    if n_slots >= 255:
        ids[0], ids[n_slots - 1] = 0, 2 ** 31 - 1
    ops, medoid = [], {}
    special = (-0.0, 5e-324, 1e-310, -1.7976931348623157e308)
    for s, kind in enumerate(kinds):
        r = rec[s]
        r["X"] = rng.randn(3) * 4
        if s % 9 == 0:
            r["X"][s % 3] = special[(s // 9) % 4]
        r["id"] = -1 if kind == "free" else ids[s]
        r["is3d"], r["has_desc"], r["observed"] = kind != "not3d", kind != "nodesc", 1
        r["inv_depth"], r["anchor_kf"], r["dev_slot"] = -1.0, 3, s
        if kind == "unwritten":
            continue
        ops.append((s, 3, -1, None, 0))
        d = [rng.randint(0, 256, 32).astype(np.uint8) for _ in range(1 + s % 2)]
        for k, dk in enumerate(d):
            ops.append((s, 0, 10 + 5 * k, dk, 13 if k == 0 else 0))
        medoid[s] = d[-1]
        if kind == "cleared":
            ops.append((s, 2, -1, None, 0))
    live = [s for s, k in enumerate(kinds) if k == "live"]
    want = {int(rec[s]["id"]): (rec[s]["X"].copy().view(np.uint64).tolist(), bytes(medoid[s])) for s in live}
    assert len(want) == len(live)
    n = len(live)
    return dict(name=f"slots_{n_slots}", n_slots=n_slots, records=rec, kinds=kinds, ops=ops, medoid=medoid, want=want,
                capacities=sorted({n + 3, n, max(n - 1, 0), n // 2, 0}))


def pack_cases():
    return [pack_case(n) for n in PACK_SLOT_COUNTS]


def pack_host_filter(records, n_slots, has_medoid, count):
    """slots the pack keeps: the record's own header, and the slot's table (has_medoid / count as MedoidStore.export reports them)"""
    r = records[:n_slots]
    return np.flatnonzero((r["id"] >= 0) & (r["is3d"] != 0) & (r["has_desc"] != 0) & (np.asarray(has_medoid[:n_slots]) != 0) &
                          (np.asarray(count[:n_slots]) > 0))


# ---------------------------------------------------------------------------------------------------- medoid store (needs oracle/_ref)
TABLE_SLOT = np.dtype([("key", "<i4"), ("next", "<i4"), ("dist", "<f4"), ("pad", "<i4"), ("desc", "u1", 32)])
TABLE_OP = np.dtype([("op", "<i4"), ("kf", "<i4"), ("rehash_to", "<i4"), ("next", "<i4"), ("desc", "u1", 32), ("pad", "<i4", 4)])
TABLE_CAP = 48
TABLE_BYTES = 64 + TABLE_CAP * TABLE_SLOT.itemsize + 60 * 4
OVERFLOW_BYTES = slice(24, 28)     # Table::overflow (csrc/slam/medoid_table.hpp)
MEDOID_CUTS = (2, 7, None)          # operations per launch; None: the whole log in one launch
POINT, BYSTANDER = 5, 9


def host_apply(table, fresh, log):
    """the host build of the tables (oracle/sys_cpu.cpp: syscpu_medoid_apply) on one table; log = [(op, kf, desc | None, rehash_to)]"""
    import ctypes as C
    import oracles
    L = oracles.ref_lib()
    L.syscpu_medoid_apply.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    rec = np.zeros(len(log), TABLE_OP)
    for i, (op, kf, d, rh) in enumerate(log):
        rec[i]["op"], rec[i]["kf"], rec[i]["rehash_to"], rec[i]["next"] = op, kf, rh, -1
        if d is not None:
            rec[i]["desc"] = d
    assert L.syscpu_medoid_apply(table.ctypes.data, int(fresh), len(log), rec.ctypes.data) == table.size == TABLE_BYTES


def table_view(table):
    """raw table -> (medoid, has medoid, [(key, dist)] in iteration order, bucket count, overflow): what MedoidStore.dump returns"""
    hdr = table[:32].view(np.int32)
    slots = table[64:64 + TABLE_CAP * TABLE_SLOT.itemsize].view(TABLE_SLOT)
    out, s = [], int(hdr[0])
    while s != -1 and len(out) <= TABLE_CAP:
        out.append((int(slots[s]["key"]), float(slots[s]["dist"])))
        s = int(slots[s]["next"])
    return table[32:64].copy(), bool(hdr[5]), out, int(hdr[3]), bool(hdr[6])


def same_table(got, want):
    """a dump (MedoidStore.dump / table_view) against the per-operation expectation (medoid_cases.ref_ops), overflow clear"""
    g_med, g_has, g_entries, g_bk, g_over = got
    med, has, bk, entries = want
    return (not g_over) and g_has == has and g_bk == bk and g_entries == entries and (not has or np.array_equal(g_med, med))


def _flat_log(first_kf, first_desc, ops):
    """the map layer's log of one point as one list [(index of the MapPoint call it belongs to, -1 = the constructor, op, kf, desc,
    rehash_to)] and the reference's table after every call.  A call that logs nothing leaves the table as it was, so after log entry k the
    table is the one expected after call number entry[k][0]."""
    import medoid_cases as mc
    want = mc.ref_ops(first_kf, first_desc, ops)
    head, per_op = mc.map_layer_log(first_kf, first_desc, ops, want)
    flat = [(-1,) + o for o in head] + [(i,) + o for i, log in enumerate(per_op) for o in log]
    return want, flat


def _bystander_op(k):
    return (BYSTANDER, 0, 1000 + k, np.full(32, k % 251, np.uint8), {0: 13, 13: 29, 29: 59}.get(k, 0))


def medoid_cut_log(name, cut):
    """one sequence of medoid_cases.sequences() for point POINT, a reset first, unrelated adds for BYSTANDER woven in, cut into launches
    of `cut` operations.  Returns dict(launches = [[(slot, op, kf, desc, rehash_to)]], border = [expected table of POINT after each launch
    or None where no MapPoint call has completed yet], final, want, bystander_count)."""
    import medoid_cases as mc
    _, first_kf, first_desc, ops = next(s for s in mc.sequences() if s[0] == name)
    want, flat = _flat_log(first_kf, first_desc, ops)
    entries, nb = [((POINT, 3, -1, None, 0), None), ((BYSTANDER, 3, -1, None, 0), None)], 0
    for k, (i, op, kf, d, rh) in enumerate(flat):
        if k % 3 == 0 and nb < 40:
            entries.append((_bystander_op(nb), None))
            nb += 1
        entries.append(((POINT, op, kf, d, rh), i))
    step = len(entries) if cut is None else cut
    launches, border, last = [], [], None
    for a in range(0, len(entries), step):
        part = entries[a:a + step]
        launches.append([e[0] for e in part])
        for _, i in part:
            last = i if i is not None else last
        border.append(want[last] if last is not None and last >= 0 else None)
    return dict(name=f"{name}/{cut}", launches=launches, border=border, final=want[-1], want=want, bystander_count=nb)


def medoid_many_points(n_points=300, per=40):
    """n_points points in ONE launch, their chains interleaved entry by entry: each point gets three junk adds, a reset in mid-chain, then
    a rotated slice of the `random` sequence.  Returns (log, slots, {slot: expected table at the end})."""
    import medoid_cases as mc
    _, first_kf, first_desc, ops = next(s for s in mc.sequences() if s[0] == "random")
    rng = np.random.RandomState(9)
    chains, final = [], {}
    for p in range(n_points):
        r = (p * 7) % len(ops)
        want, flat = _flat_log(first_kf, first_desc, (ops[r:] + ops[:r])[:per])
        slot = 1 + 3 * p
        chain = [(slot, 0, 900 + j, rng.randint(0, 256, 32).astype(np.uint8), 13 if j == 0 else 0) for j in range(3)]
        chain += [(slot, 3, -1, None, 0)] + [(slot,) + e[1:] for e in flat]
        chains.append(chain)
        final[slot] = want[-1]
    log = [c[k] for k in range(max(len(c) for c in chains)) for c in chains if k < len(c)]
    return log, 3 * n_points + 1, final


def medoid_overflow_logs():
    """[dict(name, fill = the log that leaves POINT with its last good table, over = the one insert that overflows, want = the table the
    reference has after `fill`)]: a 49th distinct keyframe (the table holds 48), and an insert that asks for 127 buckets (it holds 59).
    The rehash counts of `fill` are the reference container's own."""
    rng = np.random.RandomState(11)
    d = rng.randint(0, 256, (60, 32)).astype(np.uint8)
    out = []
    want, flat = _flat_log(1, d[1], [(0, k, d[k]) for k in range(2, 50)])
    assert len(flat) == 49 and [e[2] for e in flat] == list(range(1, 50))
    out.append(dict(name="49th_descriptor", fill=[(POINT,) + e[1:] for e in flat[:48]], over=(POINT,) + flat[48][1:], want=want[46], count=48))
    want, flat = _flat_log(1, d[1], [(0, k, d[k]) for k in range(2, 6)])
    out.append(dict(name="rehash_to_127", fill=[(POINT,) + e[1:] for e in flat], over=(POINT, 0, 77, d[50], 127), want=want[-1], count=5))
    return out
