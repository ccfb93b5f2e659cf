"""CPU: the numpy restatement of plane detection (tests/plane_cases.py) -- on the base scene it finds the floor and the wall and then
stops, every scene of the GPU tests gives its expected codes and is far from every last-bit decision -- and the public surface: the
headers declare alva_detect_planes / alva_system_detect_planes and alva::System::detectPlanes compiles.

The base scene's wall is the plane x = 1.2 and POSE_BASE has the identity rotation, so the wall's normal is the camera's x axis and
every in-plane direction is perpendicular to it (|x . R_wc[:,0]| = 3.6e-5): the definition orients such a plane's long axis by the
camera's y axis instead (|R_wc[:,0] . nrm| > 0.9), and test_the_wall_is_oriented_by_the_cameras_y_axis pins that."""
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import hit_cases as H
import plane_cases as C

ROOT = Path(__file__).resolve().parent.parent


def test_round_words_continue_the_hit_tests_stream():
    w = C.sample_words(12345, 0, 4)
    assert np.array_equal(w, H.sample_words(12345, 4))      # round 0 is the hit test's stream
    w2 = C.sample_words(12345, 2, 4)
    assert np.array_equal(w2, H.sample_words(12345, 12)[8:])   # round r starts at hypothesis r * num_iterations
    assert w.dtype == np.uint32 and w.shape == (4, 3)


@pytest.mark.parametrize("seed", [1, 2, 12345])
def test_oracle_finds_the_floor_then_the_wall_then_stops(seed):
    P = H.base_scene()
    r = C.oracle(P, H.POSE_BASE, seed=seed, **C.BASE_KW)
    print(r["info"][:, :5].tolist(), C.margins_text(r))
    assert r["info"][:, 0].tolist() == [0, 0, 3, 5] and r["found"] == 2
    assert r["info"][0, 1] == 2800 and r["info"][0, 4] == 1606 and r["info"][1, 1] == 2800 - 1606 and r["info"][1, 4] == 897
    assert 8 <= r["info"][2, 3] <= 9 and r["info"][3].tolist() == C.NOT_RUN
    floor, wall = r["planes"][0].astype(np.float64), r["planes"][1].astype(np.float64)
    assert floor[6] < -0.9999 and wall[4] < -0.9999                     # normals (0, 0, -1) and (-1, 0, 0): both face the camera
    assert abs(floor[18] + 4.0) < 0.01 and abs(wall[18] + 1.2) < 0.01   # offsets nrm . p
    assert r["thr_margin"] >= C.MARGIN_MIN
    assert r["guards"][0]["eig_ratio"] > 5e4 and 1.15 < r["guards"][0]["axis_ratio"] < 1.25 and 2.0 < r["guards"][1]["axis_ratio"] < 2.4
    for k, plane in enumerate((floor, wall)):
        M = plane[:16].reshape(4, 4).T                                   # out[4 c + r] = M[r][c]
        Rm = M[:3, :3]
        assert np.allclose(Rm.T @ Rm, np.eye(3), atol=1e-6) and np.linalg.det(Rm) > 0.999 and M[3].tolist() == [0, 0, 0, 1]
        assert not plane[19:].any()
        pts = P[r["labels"] == k]
        assert len(pts) == r["info"][k, 4]
        local = (pts - M[:3, 3]) @ Rm                                    # every inlier lies inside the rectangle, and touches its sides
        assert np.abs(local[:, 1]).max() <= 0.01 + 1e-6
        for axis, ext in ((0, plane[16]), (2, plane[17])):
            assert abs(local[:, axis].max() - ext / 2) < 1e-5 and abs(local[:, axis].min() + ext / 2) < 1e-5
    assert plane_area(floor) > 0.8 * 3.2 * 3.0 and plane_area(wall) > 0.8 * 3.0 * 2.0
    assert (r["labels"] == -1).sum() == 2800 - 1606 - 897


def plane_area(plane):
    return plane[16] * plane[17]


def test_the_three_seeds_give_the_same_two_planes():
    P = H.base_scene()
    res = [C.oracle(P, H.POSE_BASE, seed=s, **C.BASE_KW) for s in (1, 2, 12345)]
    for r in res[1:]:
        for k in range(2):
            assert abs(r["planes"][k, 4:7].astype(np.float64) @ res[0]["planes"][k, 4:7]) > 0.9999
            assert abs(r["planes"][k, 18] - res[0]["planes"][k, 18]) < 2e-3
            assert (r["labels"] == k).sum() == (res[0]["labels"] == k).sum()


@pytest.mark.parametrize("name", sorted(C.edge_cases()))
def test_every_scene_gives_its_codes_with_safe_margins(name):
    case, r = C.edge_cases()[name], C.oracle_of(name)
    print(name, r["info"][:, :5].tolist(), C.margins_text(r))
    assert r["info"][:, 0].tolist() == case["want"]
    stop = [k for k, c in enumerate(case["want"]) if c != 0]
    for k in range(len(case["want"])):
        if stop and k > stop[0]:
            assert r["info"][k].tolist() == C.NOT_RUN
        if case["want"][k] != 0:
            assert not r["planes"][k].any()
    assert r["thr_margin"] >= C.MARGIN_MIN
    for g in r["guards"]:
        assert g["eig_ratio"] >= C.MIN_EIG_RATIO and g["axis_ratio"] >= C.MIN_AXIS_RATIO and g["face_margin"] >= C.MIN_FACE
    for k, g in enumerate(r["guards"]):
        assert g["sign_margin"] >= C.MIN_SIGN, (k, g["sign_margin"])
    assert C.margins_ok(r)


def test_the_wall_is_oriented_by_the_cameras_y_axis():
    r = C.oracle_of("base")
    floor, wall = r["guards"]
    assert floor["ref_margin"] > 0.89 and abs(floor["normal"][0]) < 0.01      # the floor: by the camera's x axis
    assert floor["x"] @ np.array([1.0, 0, 0]) > 0.9 and floor["sign_margin"] > 0.9
    assert wall["normal"][0] < -0.9999 and wall["ref_margin"] > 0.09           # the wall faces along it: by the camera's y axis
    assert wall["x"] @ np.array([0, 1.0, 0]) > 0.999 and wall["sign_margin"] > 0.999
    assert abs(wall["x"] @ np.array([1.0, 0, 0])) < 1e-3                      # (what the x axis would have had to decide by)
    rot = C.oracle_of("rotated")["guards"][1]
    assert rot["ref_margin"] > 0.05 and rot["sign_margin"] > 0.9


def test_scene_details():
    e = C.oracle_of("exact_plane")
    assert e["info"][0].tolist() == [0, 192, 0, 192, 192, 0, 0, 0] and e["moments"][0][3] == 0 and e["moments"][0][9] == 0
    assert e["planes"][0, 16] == np.float32(15 / 64) and e["planes"][0, 17] == np.float32(11 / 64) and e["planes"][0, 4:7].tolist() == [0, 0, -1]
    t = C.oracle_of("tie")
    assert t["info"][0, 2] == 0 and t["info"][0, 3] == 30 and t["info"][1, 2] == 0 and t["info"][1, 3] == 30   # equal counts: the lower `it`
    assert set(np.nonzero(t["labels"] == 0)[0]) == set(range(30, 60)) and set(np.nonzero(t["labels"] == 1)[0]) == set(range(30))
    c4 = C.oracle_of("code4")
    assert c4["info"][0].tolist() == [4, 11, 0, 11, 10, 0, 0, 0] and (c4["labels"] == -1).all() and c4["moments"][0][0] == 11
    m1 = C.oracle_of("base_max1")
    wall = C.oracle_of("base")["labels"] == 1
    assert wall.sum() == 897 and (m1["labels"][wall] == -1).all()
    assert C.oracle_of("n16384")["info"][0, 1] == C.N_CAP


def test_headers_declare_plane_detection():
    hip = (ROOT / "include" / "alvaar_hip.h").read_text()
    sysh = (ROOT / "include" / "alvaar_system.h").read_text()
    assert re.search(r"\bint\s+alva_detect_planes\s*\(\s*alva_ctx\s*\*", hip)
    assert re.search(r"\bint\s+alva_system_detect_planes\s*\(\s*alva_system\s*\*", sysh)


def test_system_class_detect_planes_compiles():
    src = r'''
#include "alvaar_system.h"
int use(alva::System &s, float *planes, int *info, int *ids, int *labels) {
    int (alva::System::*native)(double, int, int, int, float *, int *, int *, int *, int) = &alva::System::detectPlanes;
    (void) native;
    return s.detectPlanes(0.01, 48, 4, 128, planes, info, ids, labels, 16384);
}
'''
    with tempfile.TemporaryDirectory() as d:
        f = Path(d) / "t.cpp"
        f.write_text(src)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-fsyntax-only", str(f)])


def test_library_exports_plane_detection():
    import ctypes
    lib = ctypes.CDLL(str(ROOT / "alvaar_amd" / "libalvaar_hip.so"))
    assert hasattr(lib, "alva_detect_planes") and hasattr(lib, "alva_system_detect_planes")
