"""CPU: the numpy restatement of plane tracking (tests/track_cases.py) -- every scene of the GPU tests gives its expected codes and is
far from every last-bit decision, without priors it is plane_cases.oracle field by field -- the host bookkeeping
(csrc/slam/plane_tracks.hpp, through the stand-alone tests/cpp/plane_tracks_host.cpp) and the public surface: the headers declare
alva_track_planes / alva_system_track_planes / alva_system_reset_planes, alva::System::trackPlanes and resetPlanes compile, the library
exports them."""
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import plane_cases as C
import track_cases as T

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("name", sorted(T.cases()))
def test_every_scene_gives_its_codes_with_safe_margins(name):
    case, r = T.cases()[name], T.oracle_of(name)
    print(name, r["info"][:, :6].tolist(), T.margins_text(r))
    n_prior = len(case["prior"])
    assert r["info"][:, 0].tolist() == case["want"]
    assert r["info"][:n_prior, 5].tolist() == [1] * n_prior and not r["info"][n_prior:, 5].any()
    assert (r["info"][:n_prior, 1] == len(case["P"])).all() and (r["info"][:n_prior, 2] == -1).all()
    for k, code in enumerate(case["want"]):
        if code != 0:
            assert not r["planes"][k].any()
        assert (r["labels"] == k).sum() == (r["info"][k, 4] if code == 0 else 0)
    assert r["found"] == case["want"].count(0)
    assert r["thr_margin"] >= T.MARGIN_MIN and r["tie_margin_t4"] >= T.MARGIN_MIN
    if case["t1_exact_tie"]:
        assert r["tie_margin_t1"] == 0   # by construction: see test_scene_details
    else:
        assert r["tie_margin_t1"] >= T.MARGIN_MIN
    for g in r["guards"]:
        assert g["eig_ratio"] >= C.MIN_EIG_RATIO and g["axis_ratio"] >= C.MIN_AXIS_RATIO and g["face_margin"] >= C.MIN_FACE, g["slot"]
        assert g["sign_margin"] >= C.MIN_SIGN and g["ref_margin"] >= C.MIN_REF, g["slot"]
    assert T.margins_ok(r, case["t1_exact_tie"])


def test_scene_details():
    i = T.oracle_of("self_base")["info"]
    assert i[0].tolist() == [0, 2800, -1, 1604, 1604, 1, 0, 0] and i[1].tolist() == [0, 2800, -1, 899, 899, 1, 0, 0]
    assert i[2, :2].tolist() == [3, 297] and i[3].tolist() == C.NOT_RUN
    assert len(T.oracle_of("self_base")["unclaimed"]) == 297
    assert np.array_equal(T.oracle_of("full_slots")["info"], i[:2])                     # no round: the tracked slots are the same
    s = T.oracle_of("swapped")
    assert s["info"][:2, 3:5].tolist() == [[899, 899], [1604, 1604]]                     # the slot follows the prior, not the size
    assert np.array_equal(s["planes"][0], T.oracle_of("self_base")["planes"][1])
    g, first = T.oracle_of("grow"), T.cases()["grow"]["prior"][0]
    assert abs(first[16] - 3.16) < 0.01 and abs(first[17] - 2.69) < 0.01                 # the floor as the half scene shows it
    assert g["info"][0].tolist() == [0, 2800, -1, 1606, 1606, 1, 0, 0]
    assert abs(g["planes"][0, 16] - 3.56) < 0.01 and abs(g["planes"][0, 17] - 3.40) < 0.01   # grown
    assert g["info"][1, :2].tolist() == [0, 1194] and g["info"][1, 4] == 897 and g["info"][1, 5] == 0 and g["planes"][1, 4] < -0.9999   # the wall, NEW
    lo = T.oracle_of("lost")["info"]
    assert lo[0, 3:5].tolist() == [1604, 1606] and lo[1].tolist() == [7, 1903, -1, 2, 0, 1, 0, 0]
    u = T.oracle_of("unusable")
    assert u["info"][0].tolist() == [9, 2800, -1, 0, 0, 1, 0, 0] and u["info"][2, 5] == 0 and u["planes"][2, 6] < -0.9999   # the floor, new, slot 2
    c8 = T.oracle_of("code8")
    assert c8["info"].tolist() == [[8, 11, -1, 11, 10, 1, 0, 0], [4, 11, 0, 11, 10, 0, 0, 0]] and (c8["labels"] == -1).all()
    assert c8["moments"][0][0] == 11 and c8["moments"][1][0] == 11 and len(c8["unclaimed"]) == 11
    e = T.oracle_of("exact_tie")
    assert e["info"][:, 3:5].tolist() == [[96, 96], [48, 48]] and e["tie_margin_t1"] == 0 and e["tie_margin_t4"] == 0.4 and abs(e["thr_margin"] - 0.2) < 1e-15
    assert (e["labels"][:96] == 0).all() and (e["labels"][96:] == 1).all()             # the middle layer went to slot 0
    assert e["planes"][0, 14] == np.float32(4.0625) and e["planes"][1, 14] == np.float32(4.25)
    s8 = T.oracle_of("stack8")
    assert s8["info"][:, 3:5].tolist() == [[48, 48]] * 8 and [float(v) for v in s8["planes"][:, 14]] == [4 + k / 4 for k in range(8)]
    assert T.oracle_of("all_claimed")["info"].tolist() == [[0, 48, -1, 48, 48, 1, 0, 0], [1, 0, -1, 0, 0, 0, 0, 0]]
    assert T.oracle_of("n0")["info"][:, :6].tolist() == [[7, 0, -1, 0, 0, 1], [7, 0, -1, 0, 0, 1], [1, 0, -1, 0, 0, 0], [5, 0, -1, 0, 0, 0]]
    assert T.oracle_of("n16384")["thr_margin"] >= 0.2


def test_chaining_self_base_changes_nothing_that_is_counted():
    """self_base fed its own output: the same codes, counts and labels, records within 1e-6"""
    case, a = T.cases()["self_base"], T.oracle_of("self_base")
    b = T.oracle_track(case["P"], case["pose7"], T.kept(a), **case["kw"])
    assert T.margins_ok(b), T.margins_text(b)
    assert np.array_equal(a["info"], b["info"]) and np.array_equal(a["labels"], b["labels"])
    assert np.abs(a["planes"].astype(np.float64) - b["planes"]).max() <= 1e-6


@pytest.mark.parametrize("name", sorted(C.edge_cases()))
def test_without_priors_the_restatement_is_detections(name):
    case, want = C.edge_cases()[name], C.oracle_of(name)
    got = T.oracle_track(case["P"], case["pose7"], None, **case["kw"])
    for key in ("info", "planes", "moments", "moment_scale", "labels"):
        assert np.array_equal(got[key], want[key]), key
    assert got["found"] == int((want["info"][:, 0] == 0).sum()) and got["thr_margin"] == want["thr_margin"]
    assert got["tie_margin_t1"] == np.inf and got["tie_margin_t4"] == np.inf and len(got["guards"]) == len(want["guards"])
    for g, w in zip(got["guards"], want["guards"]):
        assert all(np.array_equal(g[k], w[k]) for k in w)


def test_plane_tracks_bookkeeping(tmp_path):
    """csrc/slam/plane_tracks.hpp through its stand-alone program: ids kept and dropped, ages, a fresh id after a loss, the merge at 9
    degrees and none at 11, a merge refused by each offset test alone, a subsumed plane that subsumes nothing, clearing on a generation
    change, ids not reused"""
    exe = tmp_path / "plane_tracks_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(ROOT / "tests" / "cpp" / "plane_tracks_host.cpp")])
    out = subprocess.run([str(exe)], text=True, capture_output=True)
    assert out.returncode == 0 and re.fullmatch(r"\d+ 0 failures", out.stdout.strip()), out.stdout


def test_headers_declare_plane_tracking():
    hip = (ROOT / "include" / "alvaar_hip.h").read_text()
    sysh = (ROOT / "include" / "alvaar_system.h").read_text()
    assert re.search(r"\bint\s+alva_track_planes\s*\(\s*alva_ctx\s*\*", hip)
    assert re.search(r"\bint\s+alva_system_track_planes\s*\(\s*alva_system\s*\*", sysh)
    assert re.search(r"\bvoid\s+alva_system_reset_planes\s*\(\s*alva_system\s*\*", sysh)


def test_system_class_track_planes_compiles():
    src = r'''
#include "alvaar_system.h"
int use(alva::System &s, float *planes, int *info, int *pids, int *merged, int *ids, int *labels, float *outl, int *oinfo, double *areas) {
    int (alva::System::*native)(double, int, int, int, float *, int *, int *, int *, int *, int *, int, int, float *, int *, double *) =
        &alva::System::trackPlanes;
    void (alva::System::*forget)() = &alva::System::resetPlanes;
    (void) native;
    (void) forget;
    s.resetPlanes();
    const int a = s.trackPlanes(0.01, 48, 4, 128, planes, info, pids, merged, ids, labels, 16384);
    return a + s.trackPlanes(0.01, 48, 4, 128, planes, info, pids, merged, ids, labels, 16384, 64, outl, oinfo, areas);
}
'''
    with tempfile.TemporaryDirectory() as d:
        f = Path(d) / "t.cpp"
        f.write_text(src)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-fsyntax-only", str(f)])


def test_library_exports_plane_tracking():
    import ctypes
    lib = ctypes.CDLL(str(ROOT / "alvaar_amd" / "libalvaar_hip.so"))
    assert hasattr(lib, "alva_track_planes") and hasattr(lib, "alva_system_track_planes") and hasattr(lib, "alva_system_reset_planes")
