"""GPU: the slot-wise tracking step (HipStages::track_begin: k_track_stage_in, k_track_klt, k_track_klt_retry, then k_track_compact or the
compaction phase of k_pose_all) given a slot table and compared, slot by slot and BIT FOR BIT, with the numpy restatement of
Stages::track_begin (tests/trackstep_cases.py; its tables and their properties are asserted in tests/test_trackstep_cases.py).  The step
runs through the test-only probe (include/alvaar_system_testing.h, alvaar_amd.capi.TrackProbe): one set of stages, no map layer.  There
is no tolerance anywhere in this file: everything the step decides is integer logic or IEEE double in a written operation order.

What is compared per step: code, px, unpx, bv of all n slots (lost slots are zeros), p3p_req, n_pose, the gathered correspondences
(n_pose rows of Pbv, Puv, Pwpt read back from the device), and the probe's account of what ran (table route, copy kernel, k_pose_all
queued / go / abort, retry launch, compaction launches, sequence number).  With a pose solve behind the step: status, both outlier masks
and both poses against the stand-alone solve on the RESTATEMENT's correspondences.

Not covered here: the lane-group form of the tracker (k_track_klt_q_multi, 12 slots per wave, the sessions of an alva_system_group).  It
needs the group's fiber scheduler around it and stays covered by the group-equals-solo tests of tests/test_gpu_system.py."""
import numpy as np
import pytest

import trackstep_cases as T

pytestmark = pytest.mark.gpu

POSE_ALL_MAX_N = 7168      # alva_pose_all_possible (csrc/pnp.hip)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def probe():
    from alvaar_amd import capi
    p = capi.TrackProbe(0, T.W, T.H, T.CALIB8)
    yield p
    p.close()


def _step(probe, c, route, want_pose=0, carry=None):
    """feeds the case's two frames and runs one step; a machine without host-writable device memory answers routes 1 and 2 with
    ALVA_ERR_STATE, which skips"""
    from alvaar_amd import capi
    rgba, _ = T.frames()
    if carry is None:
        probe.frame(rgba[c["frames"][0]])
    probe.frame(rgba[c["frames"][1]])
    kw = dict(use_prior=c["use_prior"], klt_levels=c["klt_levels"], want_pose=want_pose, do_p3p=1, do_random=0, table_route=route)
    try:
        if carry is not None:
            return probe.step(c["n"], T.TCW_Q, T.TCW_T, carry=carry, **kw)
        return probe.step(c["n"], T.TCW_Q, T.TCW_T, px=c["px"], is3d=c["is3d"], wpt=c["wpt"], **kw)
    except capi.TrackProbeError as e:
        if route in (1, 2) and e.rc == capi.TrackProbeError.ERR_STATE and "device table" in str(e):
            pytest.skip("no host-writable device memory (hipDeviceAttributeIsLargeBar is 0): " + str(e))
        raise


def _check(ctx, probe, c, got, route, want_pose, pose_all=True, poll=True):
    w = c["want"]
    n = c["n"]
    label = (c["name"], route, want_pose)
    info = got["info"]
    print(label, "codes", np.bincount(got["code"], minlength=4), "p3p_req", got["p3p_req"], "n_pose", got["n_pose"], "status", got["status"], info)
    assert np.array_equal(got["code"], w["code"]), label
    for k in ("px", "unpx", "bv"):
        assert np.array_equal(_bits(got[k]), _bits(w[k])), (label, k)
    assert got["p3p_req"] == w["p3p_req"] and got["n_pose"] == w["n_pose"], label
    for k in ("Pbv", "Puv", "Pwpt"):
        assert got[k].shape == w[k].shape and np.array_equal(_bits(got[k]), _bits(w[k])), (label, k)
    # what ran
    assert info["route"] == route, label
    assert info["stage_in"] == int(route == 0), label
    assert info["retry"] == w["p3p_req"], label
    queued = bool(want_pose and pose_all and poll and 4 <= n <= POSE_ALL_MAX_N)
    assert info["pose_all_queued"] == int(queued), label
    assert info["pose_all_answer"] == (0 if not queued else 1 if (not w["p3p_req"] and w["n_pose"] >= 4) else 2), label
    assert info["compact_launches"] == (0 if queued else 1) + w["p3p_req"], label
    # the pose behind the step
    if not want_pose or w["n_pose"] < 4:
        assert got["status"] == -1 and not got["p3p_outlier"].any() and not got["pnp_outlier"].any(), label
        return
    import torch
    st, pose, m1, m2 = ctx.compute_pose(torch.from_numpy(w["Pbv"]).cuda(), torch.from_numpy(w["Puv"]).cuda(), torch.from_numpy(w["Pwpt"]).cuda(),
                                        [float(v) for v in T.CALIB8[:4]], 100, 3.0, 5, 5.9915, False, 12345)
    print(label, "stand-alone status", st, "outliers", int(m1.sum()), int(m2.sum()))
    assert got["status"] == st, label
    assert np.array_equal(got["p3p_outlier"].astype(bool), m1) and np.array_equal(got["pnp_outlier"].astype(bool), m2), label
    if st == 2:
        assert np.array_equal(_bits(got["pose7"]), _bits(pose)), label
    # the same solve on the probe's own context, which also returns the accepted P3P pose
    st2, p3p2, pose2, m12, m22 = probe.solve_pose(w["Pbv"], w["Puv"], w["Pwpt"])
    assert st2 == st and np.array_equal(m12.astype(bool), m1) and np.array_equal(m22.astype(bool), m2), label
    assert np.array_equal(_bits(got["pose7_p3p"]), _bits(p3p2)) and np.array_equal(_bits(got["pose7"]), _bits(pose2)), label


@pytest.mark.parametrize("want_pose", [0, 1])
@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("name", T.case_names())
def test_step_equals_restatement(ctx, probe, name, route, want_pose):
    """every case through the pinned table + copy kernel and through the host-written device table; with the compaction kernel
    (want_pose = 0) and with the fused compaction + pose launch queued behind the tracker (want_pose = 1, n <= 7168)"""
    c = T.case(name)
    _check(ctx, probe, c, _step(probe, c, route, want_pose), route, want_pose)


def test_pose_solve_has_outliers_to_order(ctx, probe):
    """mixed_200's wrong world points survive the tracker, so both masks of the pose solve are non-empty and a permuted correspondence
    list would show in them"""
    c = T.case("mixed_200")
    got = _step(probe, c, 0, 1)
    _check(ctx, probe, c, got, 0, 1)
    assert got["status"] == 2 and got["p3p_outlier"].any() and got["pnp_outlier"].any()
    assert got["info"]["pose_all_answer"] == 1


@pytest.mark.parametrize("name", ["mixed_200", "req_32_of_100", "pose_4", "size_6145", "size_7168"])
def test_pose_all_off(ctx, probe, monkeypatch, name):
    """ALVA_NO_POSE_ALL=1: the compaction kernel and the separate pose launches behind it, with a pose wanted"""
    monkeypatch.setenv("ALVA_NO_POSE_ALL", "1")
    c = T.case(name)
    for route in (0, 1):
        got = _step(probe, c, route, 1)
        assert got["info"]["pose_all_queued"] == 0 and got["info"]["compact_launches"] >= 1
        _check(ctx, probe, c, got, route, 1, pose_all=False)


@pytest.mark.parametrize("name", ["req_32_of_100", "req_0_of_3", "pose_3", "all_lost"])
def test_pose_all_abort(ctx, probe, name):
    """p3pReq_, or fewer than four correspondences: the queued fused launch is told to end after its compaction, and the step still
    returns the restatement's results"""
    c = T.case(name)
    got = _step(probe, c, 0, 1)
    assert got["info"]["pose_all_queued"] == 1 and got["info"]["pose_all_answer"] == 2
    _check(ctx, probe, c, got, 0, 1)
    if name == "all_lost":
        assert got["status"] == -1 and got["n_pose"] == 0 and got["p3p_req"] == 1


def test_stream_waits(ctx, monkeypatch):
    """ALVA_NO_POLL=1 on a probe created under it: the step waits on the stream instead of the completion words"""
    from alvaar_amd import capi
    monkeypatch.setenv("ALVA_NO_POLL", "1")
    p = capi.TrackProbe(0, T.W, T.H, T.CALIB8)
    try:
        for name in ("mixed_200", "req_32_of_100"):
            c = T.case(name)
            for want_pose in (0, 1):
                _check(ctx, p, c, _step(p, c, 0, want_pose), 0, want_pose, poll=False)
    finally:
        p.close()


def test_repeated_steps_on_one_probe(ctx, probe):
    """the counter block is reset by the compaction's last workgroup -- also after the two-compaction path -- and the sequence numbers
    go on: mixed_200 three times, req_32_of_100, mixed_200"""
    seq = None
    for k, name in enumerate(["mixed_200", "mixed_200", "mixed_200", "req_32_of_100", "mixed_200"]):
        c = T.case(name)
        want_pose = k & 1
        got = _step(probe, c, 0, want_pose)
        _check(ctx, probe, c, got, 0, want_pose)
        if seq is not None:
            assert got["info"]["seq"] == seq + 1 + c["want"]["p3p_req"]      # a retry's second compaction publishes under the next number
        seq = got["info"]["seq"]


@pytest.mark.parametrize("want_pose", [0, 1])
def test_carry_chain(ctx, probe, want_pose):
    """assembled -> carried -> carried -> assembled: the two alternating buffer sets, the carry index, and the return to a host-written
    table; the images move between the steps"""
    a, b, c, d = T.carry_chain()
    _check(ctx, probe, a, _step(probe, a, 1, want_pose), 1, want_pose)
    _check(ctx, probe, b, _step(probe, b, 2, want_pose, carry=b["carry"]), 2, want_pose)
    _check(ctx, probe, c, _step(probe, c, 2, want_pose, carry=c["carry"]), 2, want_pose)
    _check(ctx, probe, d, _step(probe, d, 1, want_pose), 1, want_pose)
    _check(ctx, probe, a, _step(probe, a, 0, want_pose), 0, want_pose)      # and a pinned table behind a device one


def test_steps_across_a_growth_of_the_blocks(ctx):
    """a FRESH probe (the module's has long since grown): 200 slots, then 2049 -- the step's blocks are carved for twice the capacity, every
    field behind the counters moves, the host-written tables are reallocated and scrubbed, the completion words zeroed again -- then a
    step carried from that one's tracked slots, then the pinned table again; each with the fused pose launch or the pose solve behind it"""
    from alvaar_amd import capi
    small, (big, carried) = T.case("mixed_200"), T.grown_carry()
    p = capi.TrackProbe(0, T.W, T.H, T.CALIB8)
    try:
        _check(ctx, p, small, _step(p, small, 1, 1), 1, 1)
        _check(ctx, p, big, _step(p, big, 1, 1), 1, 1)
        _check(ctx, p, carried, _step(p, carried, 2, 1, carry=carried["carry"]), 2, 1)
        _check(ctx, p, small, _step(p, small, 0, 1), 0, 1)
    finally:
        p.close()


def test_arguments(ctx, probe):
    from alvaar_amd import capi
    mixed = T.case("mixed_200")
    rgba, _ = T.frames()

    def still_works():
        _check(ctx, probe, mixed, _step(probe, mixed, 0, 1), 0, 1)

    probe.frame(rgba[0])
    probe.frame(rgba[1])
    got = probe.step(0, T.TCW_Q, T.TCW_T, px=np.zeros((0, 2), np.float32), is3d=np.zeros(0, np.uint8), wpt=np.zeros((0, 3)))
    assert got["n_pose"] == 0 and got["p3p_req"] == 0 and got["status"] == -1 and len(got["code"]) == 0 and len(got["Pbv"]) == 0
    still_works()
    # 65536 slots: the packed counter's 16-bit fields
    n = 65536
    with pytest.raises(capi.TrackProbeError) as e:
        probe.step(n, T.TCW_Q, T.TCW_T, px=np.zeros((n, 2), np.float32), is3d=np.zeros(n, np.uint8), wpt=np.zeros((n, 3)))
    assert e.value.rc == capi.TrackProbeError.ERR_ARG
    still_works()
    # a carried table with nothing to carry it from: right after a refused step, and after a step through the pinned table
    for _ in range(2):
        with pytest.raises(capi.TrackProbeError) as e:
            probe.step(10, T.TCW_Q, T.TCW_T, carry=np.arange(10, dtype=np.uint16), table_route=2)
        assert e.value.rc == capi.TrackProbeError.ERR_STATE
        still_works()
    # ... and with more slots than the previous table had
    got = _step(probe, mixed, 1, 0)      # (skips where there is no device table)
    _check(ctx, probe, mixed, got, 1, 0)
    with pytest.raises(capi.TrackProbeError) as e:
        probe.step(201, T.TCW_Q, T.TCW_T, carry=np.arange(201, dtype=np.uint16) % 200, table_route=2)
    assert e.value.rc == capi.TrackProbeError.ERR_STATE
    still_works()


def test_every_form_ran(ctx, probe):
    """the probe's account names each launch form at least once: the copy kernel, the device table, the carried table, the compaction
    kernel, k_pose_all answered go, k_pose_all aborted, the retry launch"""
    mixed, req = T.case("mixed_200"), T.case("req_32_of_100")
    seen = [_step(probe, mixed, 0, 0)["info"], _step(probe, mixed, 0, 1)["info"], _step(probe, req, 0, 1)["info"]]
    assert seen[0]["stage_in"] == 1 and seen[0]["route"] == 0 and seen[0]["compact_launches"] == 1 and seen[0]["pose_all_queued"] == 0
    assert seen[1]["pose_all_queued"] == 1 and seen[1]["pose_all_answer"] == 1 and seen[1]["compact_launches"] == 0
    assert seen[2]["pose_all_answer"] == 2 and seen[2]["retry"] == 1 and seen[2]["compact_launches"] == 1
    a, b = T.carry_chain()[:2]
    dev = _step(probe, a, 1, 0)["info"]      # (skips where there is no device table)
    car = _step(probe, b, 2, 0, carry=b["carry"])["info"]
    assert dev["route"] == 1 and dev["stage_in"] == 0 and car["route"] == 2 and car["stage_in"] == 0
