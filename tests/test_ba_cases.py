"""CPU: the case table of tests/ba_cases.py checks itself -- every case still has the properties it exists for (asserted by ba_cases.case with
numpy and the CPU oracle), the table as a whole covers every property, and the slot transforms leave the problem what it was."""
import numpy as np
import pytest

import ba_cases
from alvaar_amd import synth
from oracles import Orc


@pytest.mark.parametrize("name", ba_cases.CASE_NAMES)
def test_case_has_its_properties(name):
    c = ba_cases.case(name)   # asserts the properties
    print(ba_cases.describe(name))
    pb = c["pb"]
    n_kf, n_pt = len(pb["poses"]), len(pb["anchor_kf"])
    assert pb["obs_kf"].dtype == np.int32 and pb["obs_pt"].dtype == np.int32 and pb["anchor_kf"].dtype == np.int32
    assert 0 <= pb["obs_kf"].min() and pb["obs_kf"].max() < n_kf and 0 <= pb["obs_pt"].min() and pb["obs_pt"].max() < n_pt
    assert 0 <= pb["anchor_kf"].min() and pb["anchor_kf"].max() < n_kf
    if c["inv_depth"]:   # the anchor observation carries no residual block
        assert (pb["obs_kf"] != pb["anchor_kf"][pb["obs_pt"]]).all()


def test_table_covers_every_property():
    have = set()
    for name in ba_cases.CASE_NAMES:
        have |= set(ba_cases._TABLE[name][4])
    want = {"reversed", "both_triangles", "free_pairs_below", "free_pairs_both", "scattered_constants", "huber", "depth_flag", "rejected_step",
            "long_point", "free=21", "free=22", "free=8", "free=16", "free=1", "free=0", "n_kf=64"}
    assert want <= have, want - have
    # a rejected step in a RELABELLED row, the XYZ kernels on relabelled rows
    assert any("rejected_step" in ba_cases._TABLE[n][4] and ("reversed" in ba_cases._TABLE[n][4] or "scattered_constants" in ba_cases._TABLE[n][4])
               for n in ba_cases.INV_NAMES)
    assert len(ba_cases.XYZ_NAMES) >= 2
    assert all(len(v) <= 1 for v in ba_cases.DISCARDED_SEEDS.values())   # at most one seed in five per case family


@pytest.mark.parametrize("how", ["reverse", "permute"])
def test_relabel_is_the_same_problem(how):
    """Renumbering the slots changes the order of the unknowns, not the minimisation: the oracle takes the same steps and ends at the same
    poses (in their new slots), points and chi2, up to the rounding of a reordered elimination."""
    pb = synth.make_ba_problem(8, 200, 3)
    perm = np.arange(7, -1, -1) if how == "reverse" else np.random.RandomState(1).permutation(8)
    pb2 = ba_cases.relabel(pb, perm)
    assert np.array_equal(pb2["poses"][perm], pb["poses"]) and np.array_equal(pb2["kf_const"][perm], pb["kf_const"])
    assert np.array_equal(pb2["obs_kf"], perm[pb["obs_kf"]]) and np.array_equal(pb2["anchor_kf"], perm[pb["anchor_kf"]])
    a, b = Orc.local_ba(pb, 5, 0.0), Orc.local_ba(pb2, 5, 0.0)
    assert list(a["info"][[0, 3]]) == list(b["info"][[0, 3]])
    assert np.abs(b["poses"][perm] - a["poses"]).max() < 1e-9 and np.abs(b["pts"] - a["pts"]).max() < 1e-9
    assert np.allclose(a["chi2"], b["chi2"], rtol=1e-7, atol=1e-10)


def test_transforms_leave_their_input_alone():
    pb = synth.make_ba_problem(6, 100, 2)
    before = {k: np.array(v, copy=True) for k, v in pb.items()}
    ba_cases.add_outliers(ba_cases.set_constants(ba_cases.reverse(pb), (1, 4)), 0.1, seed=1)
    ba_cases.as_xyz(pb)
    assert all(np.array_equal(pb[k], before[k]) for k in before)
    out = ba_cases.add_outliers(pb, 0.1, seed=1)
    moved = np.abs(out["obs_uv"] - pb["obs_uv"])
    hit = moved.max(axis=1) > 0
    assert hit.sum() == round(0.1 * len(hit)) and (moved[hit] >= 4.0).all() and (moved[hit] <= 9.0).all()
