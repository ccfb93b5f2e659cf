"""f4a at its edges (CPU): the designed tiles of clahe_cases.py have the residuals they are built for, the grid and size cases reach the
extension, clamp and no-clip paths they are named for; the oracle is OpenCV's CLAHE in the compiled reference (where built) and the
reference's recorded outputs (tests/golden/clahe_cases.npz) bit for bit."""
import numpy as np
import pytest
from pathlib import Path

import clahe_cases as kc
from oracles import orc_clahe, ref_clahe

G = Path(__file__).resolve().parent / "golden"


def _stats(case_id):
    c = kc.case(case_id)
    return kc.tile_stats(kc.image(case_id), c.clip, c.tiles)


@pytest.mark.parametrize("case_id", ["designed-mid", "designed-ends"])
def test_designed_tiles_have_their_residuals(case_id):
    s = _stats(case_id)
    assert s["limit"] == kc.DESIGN_LIMIT and (s["tw"], s["th"]) == (kc.TILE, kc.TILE) and s["reflections"] == 0
    assert [(int(b), int(r)) for b, r in zip(s["batch"], s["residual"])] == list(kc.DESIGN)
    assert tuple(sorted(set(int(r) for r in s["residual"]))) == kc.RESIDUALS          # 0, 1, 100, 128, 129, 255 each occur
    assert s["batch"][list(s["residual"]).index(0)] > 0                               # residual 0 with a batch to spread
    assert 256 // 100 == 2 and 256 % 100 != 0 and 256 // 129 == 1 and 256 // 255 == 1   # a truncating step, and steps of 1


def test_edges_reach_what_they_are_named_for():
    s = _stats("5x3-t4x2")
    assert (s["ew"], s["eh"], s["tw"], s["th"]) == (8, 4, 2, 2)
    s = _stats("7x7-t7x7")
    assert (s["tw"], s["th"]) == (1, 1) and 0 < s["raw_limit"] < 1 and s["limit"] == 1 and (s["excess"] == 0).all()
    s = _stats("33x17-t8x8")
    assert (s["ew"], s["eh"], s["tw"], s["th"]) == (40, 24, 5, 3) and (s["excess"] > 0).any()
    s = _stats("300x10-t1x10")
    assert (s["tw"], s["th"]) == (300, 1) and s["limit"] == 3 and len(set(s["residual"])) > 3 and (s["excess"] > 0).all()
    s = _stats("17x16-t1x1")
    assert (s["tw"], s["th"]) == (17, 16) and s["excess"][0] > 0
    s = _stats("256x1-t3x1")
    assert (s["ew"], s["eh"], s["tw"], s["th"]) == (258, 2, 86, 2) and (s["excess"] > 0).any()
    s = _stats("64x48-clip1000")
    assert s["limit"] == 750 > s["tw"] * s["th"] and (s["excess"] == 0).all()
    assert np.array_equal(kc.oracle("64x48-clip1000"), orc_clahe(kc.image("64x48-clip1000"), 0.0, (4, 4)))   # ... the same as no clip
    s = _stats("64x48-clip0")
    assert s["limit"] == 0
    s = _stats("3x2-t8x5")
    assert (s["ew"], s["eh"]) == (8, 5) and s["reflections"] > 1
    s = _stats("320x240-t7x9")
    assert (s["ew"], s["eh"]) == (322, 243) and (s["residual"] > 128).any() and (s["batch"] > 0).any()
    for c in kc.CASES:
        assert c.w <= 320 and c.h <= 240 and kc.image(c.id).shape == (c.h, c.w)
        assert not np.array_equal(kc.oracle(c.id), kc.image(c.id)) or c.id == "7x7-t7x7"


@pytest.mark.ref
@pytest.mark.parametrize("case_id", kc.CASE_IDS)
def test_oracle_matches_opencv(case_id):
    c = kc.case(case_id)
    assert np.array_equal(kc.oracle(case_id), ref_clahe(kc.image(case_id), c.clip, c.tiles))


def test_oracle_matches_golden():
    z = np.load(G / "clahe_cases.npz")
    assert list(z["ids"]) == list(kc.GOLDEN_IDS)
    for c in map(kc.case, kc.GOLDEN_IDS):
        assert (float(z[f"clip_{c.id}"]), tuple(z[f"tiles_{c.id}"])) == (c.clip, c.tiles)
        assert np.array_equal(z[f"g_{c.id}"], kc.image(c.id)) and np.array_equal(z[f"out_{c.id}"], kc.oracle(c.id)), c.id
