"""The shift restatement tests/mesh_shift_cases.py checked on the CPU: against a naive triple loop, its own properties over the whole
case table, the extraction's world invariance under a shift, and the follow rule V1-V4 on hand-made cases."""
from __future__ import annotations

import numpy as np
import pytest

import mesh_cases as Mc
import mesh_shift_cases as Sc


# ---------------------------------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("N", [4, 5])
def test_slices_equal_the_naive_triple_loop(N):
    q, w, c = Sc.case_volume(N, 7 + N)
    shifts = [s for _, s in Sc.case_shifts(N)] + [(1, 1, 1), (-1, 2, -3), (N - 1, -(N - 1), N - 1), (2, 0, -N)]
    for s in shifts:
        for col in (None, c):
            got, want = Sc.shift(q, w, col, s), Sc.shift_naive(q, w, col, s)
            for a, b in zip(got, want):
                assert (a is None and b is None) or np.array_equal(a, b), s


def test_the_table_has_what_the_stage_can_get_wrong():
    ids = [c[0] for c in Sc.cases()]
    assert len(ids) == len(set(ids))
    for N in Sc.CASE_N:
        shifts = {s for _, n, s in Sc.cases() if n == N}
        for want in [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, -1), (8, 0, 0), (-8, 0, 0), (16, 0, 0), (-16, 0, 0), (0, 0, 16),
                     (3, -5, 8), (-8, 16, 0), (N - 1, 0, 0), (N, 0, 0), (N + 1, 0, 0), (0, -(N - 1), 0), (0, 0, N),
                     (Sc.INT_MAX, 0, 0), (0, Sc.INT_MIN, 0), (Sc.INT_MIN, Sc.INT_MAX, Sc.INT_MIN)]:
            assert want in shifts, (N, want)
    # the volumes use q's whole range and the five weights
    q, w, c = Sc.volumes()[32]
    assert q.min() == -32768 and q.max() == 32767 and set(np.unique(w)) == {0, 1, 127, 128, 255}
    assert (c[..., 3] == 0).any() and (c[..., 3] == 255).any()


@pytest.mark.parametrize("cid,N,s", Sc.cases(), ids=[c[0] for c in Sc.cases()])
def test_properties(cid, N, s):
    q, w, c = Sc.volumes()[N]
    q2, w2, c2, info = Sc.expected(N, s)
    overlap = int(np.prod([max(0, N - abs(v)) for v in s])) if all(abs(v) < N for v in s) else 0
    assert info[0] == overlap and info[7] == N and not info[4:7].any()
    assert info[1] + info[2] == (w > 0).sum()   # kept + lost = weighted before
    assert info[1] == (w2 > 0).sum() and info[3] == (c2[..., 3] > 0).sum()
    qn, wn, cn, info_n = Sc.shift(q, w, None, s)
    assert cn is None and np.array_equal(qn, q2) and np.array_equal(wn, w2) and np.array_equal(info_n[:3], info[:3]) and info_n[3] == 0
    if s == (0, 0, 0):
        assert np.array_equal(q2, q) and np.array_equal(w2, w) and np.array_equal(c2, c)
    if overlap == 0:
        assert not q2.any() and not w2.any() and not c2.any()
    # there and back: exactly the overlap is restored, the rest is zero
    back = tuple(-v if v != Sc.INT_MIN else Sc.INT_MAX for v in s)   # (-INT_MIN is no int; any |s| >= N does the same)
    q3, w3, c3, _ = Sc.shift(q2, w2, c2, back)
    keep = np.zeros((N, N, N), bool)
    if overlap:
        keep[tuple(slice(max(0, v), min(N, N + v)) for v in reversed(s))] = True
    assert np.array_equal(q3, np.where(keep, q, 0)) and np.array_equal(w3, np.where(keep, w, 0))
    assert np.array_equal(c3, np.where(keep[..., None], c, 0))


# ---------------------------------------------------------------------------------------------------- world invariance
def _kept_cells(cells, s, N):
    """cells of the original volume whose eight corners all lie in the overlap: (cell - s) is a cell of the shifted volume"""
    p = cells - np.asarray(s)
    return np.all((p >= 0) & (p <= N - 2), axis=1)


@pytest.mark.parametrize("solid", ["sphere", "box"])
@pytest.mark.parametrize("s", [(3, -5, 8), (-8, 16, 0), (9, 0, 0), (0, 0, -13)])
def test_extraction_is_invariant_in_the_world(solid, s):
    """origin -1 and voxel 2^-4 are dyadic, so o + s voxel and X3's arithmetic are exact in double: the shifted volume with the moved
    origin gives the SAME float vertices for every cell wholly inside the overlap, in scan order, and the same triangles up to the
    vertices' renumbering"""
    N = 32
    dist = Mc.sphere_dist(Mc.SPHERE_C, Mc.SPHERE_R) if solid == "sphere" else Mc.box_dist((-0.7, -0.6, -0.5), (0.6, 0.8, 0.7))
    q, w, origin, voxel = Mc.sampled(N, dist)
    assert voxel == 2.0 ** -4 and np.all(origin == -1.0)
    a = Mc.extract(q, w, origin, voxel, 1, 1 << 20, 1 << 21)
    q2, w2, _, info = Sc.shift(q, w, None, s)
    origin2 = origin + np.asarray(s, np.float64) * voxel
    assert np.all((origin2 - origin) / voxel == np.asarray(s))   # exact
    b = Mc.extract(q2, w2, origin2, voxel, 1, 1 << 20, 1 << 21)
    assert a["info"][0] == 0 and b["info"][0] == 0
    keep = _kept_cells(a["cells"], s, N)
    assert 0 < keep.sum() < len(keep), "the shift must cut the surface"
    assert np.array_equal(a["cells"][keep] - np.asarray(s), b["cells"])   # scan order survives the filter
    assert np.array_equal(a["vertices"][keep].view(np.uint32), b["vertices"].view(np.uint32))
    assert np.array_equal(a["normals"][keep].view(np.uint32), b["normals"].view(np.uint32))
    # the float rounding of a non-dyadic origin would allow this much; here it is not needed
    assert np.abs(a["vertices"][keep] - b["vertices"]).max() <= 4 * 2.0 ** -23 * np.abs(a["vertices"]).max()
    # triangles: the quads (two triangles each) all of whose cells were kept, renumbered
    renum = np.full(len(keep), -1, np.int64)
    renum[keep] = np.arange(keep.sum())
    quads = a["triangles"].reshape(-1, 6)
    quads = renum[quads[np.all(keep[quads], axis=1)]]
    assert len(quads) > 0 and np.array_equal(quads.reshape(-1, 3), b["triangles"])


# ---------------------------------------------------------------------------------------------------- the follow rule
ORIGIN, SIDE, VOXEL = (-4.0, -4.0, -4.0), 8.0, 0.25   # the centre is the world's origin: d = c / 0.25


@pytest.mark.parametrize("block,d,want", [
    (4, 3.999, 0), (4, 4.0, 4), (4, 7.999, 4), (4, 8.0, 8), (4, -3.999, 0), (4, -4.0, -4), (4, -7.9, -4), (4, -8.0, -8),
    (1, 0.999, 0), (1, 1.0, 1), (1, -0.999, 0), (1, -1.0, -1), (1, 13.7, 13), (1, -13.7, -13),
    (32, 31.999, 0), (32, 32.0, 32), (32, -31.999, 0), (32, -32.0, -32), (32, 65.0, 64), (32, -95.9, -64),
    (8, float("nan"), 0), (8, float("inf"), 0), (8, float("-inf"), 0), (8, 1e30, 1 << 24), (8, -1e30, -(1 << 24)), (32, 1e300, 1 << 24),
])
def test_follow_rule_per_axis(block, d, want):
    for axis in range(3):
        c = [0.0, 0.0, 0.0]
        c[axis] = d * VOXEL
        s = Sc.follow_shift(c, ORIGIN, SIDE, VOXEL, block)
        assert s[axis] == want and all(s[a] == 0 for a in range(3) if a != axis), (axis, s)
        assert s[axis] % block == 0


def test_follow_rule_leaves_less_than_a_block():
    rng = np.random.RandomState(5)
    for block in Sc.FOLLOW_BLOCKS:
        for _ in range(50):
            c = rng.uniform(-40, 40, 3)
            s = Sc.follow_shift(c, ORIGIN, SIDE, VOXEL, block)
            origin = Sc.follow_origin(ORIGIN, s, VOXEL)
            assert Sc.follow_shift(c, origin, SIDE, VOXEL, block) == (0, 0, 0)   # hysteresis: the remainder is under a block
            rest = (c - (origin + SIDE / 2)) / VOXEL
            assert np.all(np.abs(rest) < block)


def test_the_session_tests_stream_moves_the_target_by_three_blocks():
    """what tests/test_gpu_mesh_follow_system.py relies on, counted on the analytic poses: wherever in frames 10..50 the volume is placed
    (the session places it at frame 10), the stream shifts it at least three times and by at least three blocks along x"""
    for k_place in range(10, 51, 5):
        moves = Sc.stream_shifts(k_place)
        total = np.sum([s for _, s in moves], axis=0)
        assert len(moves) >= 3 and abs(total[0]) >= 3 * Sc.STREAM_BLOCK, (k_place, moves)
        assert all(v % Sc.STREAM_BLOCK == 0 for _, s in moves for v in s)


def test_follow_target_and_origin():
    R = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])   # the optical axis is world x
    assert Sc.follow_target((1.0, 2.0, 3.0), R, 4.0) == (5.0, 2.0, 3.0)
    o0 = (0.1, -0.7, 3.3)
    assert np.array_equal(Sc.follow_origin(o0, (0, 0, 0), 0.37), np.array(o0))   # offset 0: origin0's bits
    assert np.array_equal(Sc.follow_origin(o0, (4, -8, 12), 0.25), np.array([1.1, -2.7, 6.3]))
