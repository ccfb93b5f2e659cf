"""match_to_map.hip over the case table (tests/mtm_cases.py; tests/test_mtm_cases.py proves on the CPU that every case reaches the branch it
is named for): alva_match_to_map, alva_match_to_map_flags and alva_match_to_map_records each return exactly the plain-C checker's
match_of_mp -- every row, the -1s included.  Discrete output: no tolerances."""
import ctypes as C

import numpy as np
import pytest

import mtm_cases as T
from oracles import orc_match_to_map_flags

pytestmark = pytest.mark.gpu

_want = {}


def want(c):
    """the checker's match_of_mp for the case, computed once; the table states the same result (test_mtm_cases.py)"""
    if c["name"] not in _want:
        w = orc_match_to_map_flags(c["pb"], c["aux"], c["mhd"], c["ohd"], **c["kw"])
        assert np.array_equal(w, T.expected_rows(c))
        w.setflags(write=False)
        _want[c["name"]] = w
    return _want[c["name"]]


def _d(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _kw(c):
    kw = dict(c["kw"])
    return int(kw.pop("num_kp3d", c["pb"]["num_kp3d"])), kw


def run_flat(ctx, c, flags, aux=None):
    from oracles import flatten_match_to_map
    pb, aux = c["pb"], c["aux"] if aux is None else aux
    cell_mp, local = flatten_match_to_map(pb, aux)
    kp3, kw = _kw(c)
    args = (pb["calib"], pb["cell_size"], aux["num_cells_w"], aux["grid_cells"], _d(aux["cell_ptr"], np.int32), _d(cell_mp), _d(aux["kf_q"]),
            _d(aux["kf_t"]), _d(pb["mp_wpt"]), _d(pb["mp_is3d"]), _d(pb["obs_ptr"]), _d(pb["obs_kf"]), _d(pb["obs_px"]), _d(pb["obs_desc"]),
            len(pb["kf_id"]) - 1, kp3, _d(local))
    if not flags:
        return ctx.match_to_map(*args, **kw).cpu().numpy()
    return ctx.match_to_map_flags(*args, mp_has_desc=None if c["mhd"] is None else _d(c["mhd"]),
                                  obs_has_desc=None if c["ohd"] is None else _d(c["ohd"]), **kw).cpu().numpy()


def run_records(ctx, c, kf_ids=None):
    from alvaar_amd.capi import MedoidStore
    from oracles import flatten_match_to_map
    pb, aux = c["pb"], c["rec"].get("aux", c["aux"])
    cell_mp, local = flatten_match_to_map(pb, aux)
    chunks, table, slot_of, ops, n_slots = T.records_of(pb, shuffle_seed=len(pb["mp_id"]), mp_has_desc=c["mhd"], obs_has_desc=c["ohd"], **c["rec"])
    store = MedoidStore(ctx)
    try:
        store.replay(ops, n_slots)
        kp3, kw = _kw(c)
        out = ctx.match_to_map_records(pb["calib"], pb["cell_size"], aux["num_cells_w"], aux["grid_cells"], _d(aux["cell_ptr"], np.int32), _d(cell_mp),
                                       _d(pb["kf_id"] if kf_ids is None else kf_ids, np.int32), _d(aux["kf_q"]), _d(aux["kf_t"]), len(pb["kf_id"]) - 1,
                                       _d(slot_of), table, store, kp3, _d(local), **kw).cpu().numpy()
    finally:
        store.close()
    del chunks
    return out


@pytest.mark.parametrize("case", T.FLAT_CASES, ids=lambda c: c["name"])
def test_flat_form(ctx, case):
    assert np.array_equal(run_flat(ctx, case, flags=False), want(case))


@pytest.mark.parametrize("case", T.FLAG_CASES, ids=lambda c: c["name"])
def test_flags_form(ctx, case):
    assert np.array_equal(run_flat(ctx, case, flags=True), want(case))


@pytest.mark.parametrize("case", T.RECORD_CASES, ids=lambda c: c["name"])
def test_record_form(ctx, case):
    assert np.array_equal(run_records(ctx, case), want(case))


@pytest.mark.parametrize("flags", [False, True], ids=["flat", "flags"])
def test_flat_forms_skip_a_grid_entry_without_frame_obs(ctx, flags):
    """the record form's guard holds in the flat forms too: a grid entry whose map point does not observe the frame is no candidate"""
    c = T.BY_NAME["rec_grid_entry_without_frame_obs"]
    assert len(c["rec"]["aux"]["cell_kp"]) == len(c["aux"]["cell_kp"]) + 1
    assert np.array_equal(run_flat(ctx, c, flags, aux=c["rec"]["aux"]), want(c))


def test_table_forwards_then_backwards_on_one_context(ctx):
    """the calls share one scratch buffer whose size and layout change from case to case and from form to form"""
    order = T.FLAG_CASES + T.FLAG_CASES[::-1]
    for c in order:
        assert np.array_equal(run_flat(ctx, c, flags=True), want(c)), c["name"]
    small = [c for c in T.RECORD_CASES if "n_slots" not in c["rec"]][::7]
    for c in small + small[::-1]:
        assert np.array_equal(run_records(ctx, c), want(c)), c["name"]
        if c["only"] is None:
            assert np.array_equal(run_flat(ctx, c, flags=True), want(c)), c["name"]


@pytest.mark.parametrize("name", ["arb_5_5_7_different_workgroups", "scan_later_chunk_between_best_and_second_kept"])
def test_permuted_rows(ctx, name):
    """the same map with its rows in another order, indices relabelled: the permuted result"""
    c = T.BY_NAME[name]
    q, perm = T.permuted(c, 5)
    inv = np.argsort(perm)
    w = want(c)
    expect = np.array([inv[w[r]] if w[r] >= 0 else -1 for r in perm], np.int32)
    assert (expect >= 0).any()
    assert np.array_equal(run_flat(ctx, q, flags=False), expect)
    assert np.array_equal(run_flat(ctx, q, flags=True), expect)
    assert np.array_equal(run_records(ctx, q), expect)


def test_empty_map_returns_ok_and_leaves_the_output(ctx):
    """n_mp == 0: ALVA_OK from all three entry points before any pointer is looked at, nothing launched, the output untouched"""
    import torch
    from alvaar_amd.capi import lib
    out = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    cal = np.ascontiguousarray(T.CASES[0]["pb"]["calib"], np.float64)
    p = out.data_ptr()
    f = C.c_float
    assert lib.alva_match_to_map(ctx.h, cal.ctypes.data, 35, 19, 266, None, None, 2, None, None, 0, None, None, None, None, None, None, 1, 100, 0, None,
                                 f(2.0), f(0.2), p) == 0
    assert lib.alva_match_to_map_flags(ctx.h, cal.ctypes.data, 35, 19, 266, None, None, 2, None, None, 0, None, None, None, None, None, None, None, None,
                                       1, 100, 0, None, f(2.0), f(0.2), p) == 0
    assert lib.alva_match_to_map_records(ctx.h, cal.ctypes.data, 35, 19, 266, None, None, 2, None, None, None, 1, 11, 0, None, None, None, 100, 0, None,
                                         f(2.0), f(0.2), p) == 0
    ctx.sync()
    assert (out == 77).all()


def test_keyframe_table_of_65_is_refused(ctx):
    """the record form keeps the keyframe ids in 64 shared-memory words: a table of 64 works (rec_40_entries_38_kept_kf_table_64), one of 65 is
    an argument error, and nothing is launched"""
    import torch
    from alvaar_amd.capi import AlvaError, lib
    c = T.BY_NAME["rec_40_entries_38_kept_kf_table_64"]
    assert len(c["pb"]["kf_id"]) == 64
    pb, aux = c["pb"], c["aux"]
    ids65 = _d(np.concatenate([pb["kf_id"], [99]]), np.int32)
    q65, t65 = _d(np.concatenate([aux["kf_q"], [[0, 0, 0, 1.0]]])), _d(np.concatenate([aux["kf_t"], [[0, 0, 0.0]]]))
    out = torch.full((len(pb["mp_id"]),), 77, dtype=torch.int32, device="cuda")
    dummy = torch.zeros(64, dtype=torch.int32, device="cuda")
    cal = np.ascontiguousarray(pb["calib"], np.float64)
    rc = lib.alva_match_to_map_records(ctx.h, cal.ctypes.data, 35, aux["num_cells_w"], aux["grid_cells"], dummy.data_ptr(), dummy.data_ptr(), 65,
                                       ids65.data_ptr(), q65.data_ptr(), t65.data_ptr(), 63, int(pb["kf_id"][63]), len(pb["mp_id"]), dummy.data_ptr(),
                                       dummy.data_ptr(), dummy.data_ptr(), 100, 1, dummy.data_ptr(), C.c_float(2.0), C.c_float(0.2), out.data_ptr())
    assert rc != 0
    ctx.sync()
    assert (out == 77).all()
    with pytest.raises(AlvaError):
        run_records(ctx, c, kf_ids=np.concatenate([pb["kf_id"], [99]]))
    assert np.array_equal(run_records(ctx, c), want(c))      # and the context still works
