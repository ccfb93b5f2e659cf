"""a6 at its edges (CPU): the table of describe_cases.py reaches what it claims -- one describable pixel at 63 x 63, hostile coordinates all
invalid with their neighbours untouched, all-zero descriptors on a flat image -- and the oracle is the compiled reference (where built) and
the reference's recorded outputs (tests/golden/describe_cases.npz) bit for bit."""
import numpy as np
import pytest
from pathlib import Path

import describe_cases as dc
from oracles import Orc, Ref

G = Path(__file__).resolve().parent / "golden"


def test_stated_validity_and_sizes():
    for c in dc.CASES:
        d, v = dc.oracle(c.id)
        if c.valid is not None:
            assert np.array_equal(v, c.valid), c.id
        assert not d[v == 0].any(), c.id                          # an invalid point's descriptor is 32 zero bytes
    assert dc.oracle("63x63")[1].sum() == 2 and dc.image(dc.case("63x63").spec).shape == (63, 63)
    assert [len(dc.case(f"n{n}").pts) for n in dc.SIZES] == [7, 8, 9, 64, 65]
    for n in dc.SIZES:
        d, v = dc.oracle(f"n{n}")
        assert 0 < v.sum() < n and d[v == 1].any(1).all()         # valid and invalid points in every launch shape


def test_blur_images_pin_what_they_claim():
    for k, spec in dc.BLUR.items():
        h, w = dc.image(spec).shape
        assert w > 6 and h > 6, k
    assert {dc.image(dc.BLUR[k]).shape[::-1] for k in ("7x7", "8x7", "7x64", "64x16", "65x17", "67x7")} == {(7, 7), (8, 7), (7, 64), (64, 16), (65, 17), (67, 7)}
    assert not dc.blur_oracle("zeros").any() and (dc.blur_oracle("full") == 255).all()
    assert set(np.unique(dc.blur_oracle("checker"))) == {127, 128}
    s = dc.blur_centres(dc.image(dc.BLUR["ties"]))               # exact halves: round half to even, not half up
    assert s.dtype == np.float32 and np.array_equal(s, np.float32(dc.TIE_FLOORS) + np.float32(0.5))
    want = [k if k % 2 == 0 else k + 1 for k in dc.TIE_FLOORS]
    assert list(dc.blur_oracle("ties")[3, 3::7]) == want and sum(k % 2 == 0 for k in dc.TIE_FLOORS) == 4


def test_hostile_points_are_invalid_and_leave_their_neighbours_alone():
    c = dc.case("hostile")
    d, v = dc.oracle("hostile")
    bad = dc.hostile_rows()
    assert len(bad) == 3 * len(dc.HOSTILE)
    assert [repr(x) for x in dc.HOSTILE[:7]] == ["nan", "inf", "-inf", "3000000000.0", "-3000000000.0", "2147483520.0", "-0.0"]
    assert all(float(np.float32(x)) == x for x in dc.HOSTILE[3:-2])   # each is a float as written (+-1e30 round)
    assert not v[bad].any() and not d[bad].any()
    good = np.setdiff1d(np.arange(len(v)), bad)
    assert v[good].all() and len(good) == len(bad) + 1
    d2, v2 = Orc.describe(dc.image(c.spec), c.pts[good])          # the valid points on their own: the same descriptors
    assert v2.all() and np.array_equal(d2, d[good]) and d2.any(1).all()
    # 2^32 + 512 with a valid row would be column 512 after a wrapping conversion: that pixel is describable here, and is the last valid row
    assert (c.pts[bad] == np.float32(4294967808.0)).any() and np.array_equal(c.pts[-1], (512.0, dc.HOSTILE_Y)) and v[-1] == 1


def test_flat_and_two_level_images():
    d, v = dc.oracle("flat")
    assert v.sum() >= 4 and not d.any()                           # t0 < t1 is false on every tie
    d, v = dc.oracle("halves")
    c = dc.case("halves")
    assert v.all()
    # the blur smears the seam over columns 47 .. 52; the pattern reaches 13 pixels (rotated by one degree: 14 at most)
    far, near = (c.pts[:, 0] <= 32) | (c.pts[:, 0] >= 67), np.abs(c.pts[:, 0] - 50) <= 5
    assert far.sum() >= 6 and not d[far].any() and d[near].any(1).all()
    assert len({bytes(r) for r in d[near]}) > 5                   # the seam's position shows in the bits


@pytest.mark.ref
def test_oracle_matches_reference():
    for k in dc.BLUR_IDS:
        assert np.array_equal(dc.blur_oracle(k), Ref.orb_blur(dc.image(dc.BLUR[k]))), k
    for c in dc.CASES:
        d, v = dc.oracle(c.id)
        rd, rv = Ref.describe(dc.image(c.spec), c.pts)
        assert np.array_equal(v, rv) and np.array_equal(d, rd), c.id


def test_oracle_matches_golden():
    z = np.load(G / "describe_cases.npz")
    assert list(z["blur_ids"]) == list(dc.BLUR_IDS) and list(z["ids"]) == list(dc.CASE_IDS)
    for k in dc.BLUR_IDS:
        assert np.array_equal(z[f"blur_g_{k}"], dc.image(dc.BLUR[k])) and np.array_equal(z[f"blur_out_{k}"], dc.blur_oracle(k)), k
    for c in dc.CASES:
        d, v = dc.oracle(c.id)
        assert np.array_equal(z[f"g_{c.id}"], dc.image(c.spec)) and np.array_equal(z[f"pts_{c.id}"].view(np.uint32), c.pts.view(np.uint32)), c.id
        assert np.array_equal(z[f"valid_{c.id}"], v) and np.array_equal(z[f"desc_{c.id}"], d), c.id
