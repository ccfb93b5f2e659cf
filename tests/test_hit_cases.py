"""CPU: the numpy restatement of the hit test (tests/hit_cases.py) on the base scene -- it finds the floor and the wall, gives the codes
of the base taps, and every compared case is far from a last-bit decision -- and the public surface: the headers declare
alva_hit_test / alva_system_hit_test and alva::System::hitTest compiles."""
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import hit_cases as H

ROOT = Path(__file__).resolve().parent.parent


def _base():
    P = H.base_scene()
    return P, [H.oracle(P, H.POSE_BASE, H.K_BASE, uv, rad) for uv, rad in H.BASE_TAPS]


def test_hash32_against_hand_computed_values():
    # x = 0 stays 0 through every xor-shift and product
    assert H.hash32(0) == 0
    # x = 1: 1 -> *0x7feb352d = 0x7feb352d -> ^ (>> 15 = 0xffd6) = 0x7febcafb -> *0x846ca68b = 0x6889f849 (mod 2^32) -> ^ (>> 16 = 0x6889)
    assert H.hash32(1) == 0x688990C0
    # x = 12345 = 0x3039: * 0x7feb352d = 0x95574705 -> ^ (>> 15 = 0x12aae) = 0x95566dab -> * 0x846ca68b = 0x912e6dd9 -> ^ (>> 16 = 0x912e)
    assert H.hash32(12345) == 0x912EFCF7
    w = H.sample_words(12345, 2)
    assert w.dtype == np.uint32 and w.shape == (2, 3)
    assert int(w[1, 2]) == H.hash32(12345 ^ ((5 * 0x9E3779B9) & 0xFFFFFFFF))


def test_shared_header_hashes_maps_and_fits_like_the_restatement(tmp_path):
    """the host-compilable part of csrc/plane_fit.hpp, which hit_test.hip, detect_planes.hip and find_plane.hip share: the hash values
    above, the word-to-index map at m = 1, m = 2048 and w = 0xffffffff, the plane through a collinear and a 3-4-5 triple, and the host
    eigen-solve for N = 3 and 4 on diagonal matrices (tests/cpp/plane_fit_host.cpp)"""
    exe = tmp_path / "plane_fit_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), str(ROOT / "tests" / "cpp" / "plane_fit_host.cpp")])
    out = subprocess.check_output([str(exe)], text=True)
    assert out.strip() == "32 0 failures", out


def test_words_for_selects_the_requested_indices():
    for m in (24, 44, 63, 2048):
        idx = [[0, 1, m - 1], [m // 2, m // 3, 7]]
        w = H.words_for(idx, m)
        assert [[(int(x) * m) >> 32 for x in row] for row in w] == idx


def test_oracle_finds_the_floor_and_the_wall():
    P, res = _base()
    t = H.POSE_BASE[:3]
    for k, truth, offset in ((0, np.array([0, 0, 1.0]), 4.0), (1, np.array([1.0, 0, 0]), 1.2), (2, np.array([0, 0, 1.0]), 4.0)):
        r = res[k]
        assert r["code"] == 0
        assert abs(r["normal"] @ truth) > 0.999
        assert r["normal"] @ (t - r["point"]) > 0                       # faces the camera
        assert abs(r["point"] @ truth - offset) < 0.01                  # on the plane
        along = r["point"] - t
        assert np.linalg.norm(np.cross(along, r["ray"])) < 1e-9 and along @ r["ray"] > 0   # on the tap's ray
        pose = r["pose"].reshape(4, 4).T                                 # out[4 c + r] = M[r][c]
        Rm = pose[:3, :3].astype(np.float64)
        assert np.allclose(Rm.T @ Rm, np.eye(3), atol=1e-6) and np.linalg.det(Rm) > 0.999
        assert np.allclose(Rm[:, 1], r["normal"], atol=1e-6) and np.allclose(pose[:3, 3], r["point"], atol=1e-6)
        assert pose[3].tolist() == [0, 0, 0, 1]
    assert res[1]["normal"][0] < -0.999                                  # the wall's normal: a plane findPlane cannot return


def test_base_tap_codes_counts_and_margins():
    _, res = _base()
    assert [r["code"] for r in res] == [0, 0, 0, 1, 0]
    assert [r["m"] for r in res] == [44, 46, 50, 7, 31]
    assert [r["n_sel"] for r in res] == [44, 46, 50, 7, 31]
    assert res[4]["n_in"] >= H.MIN_INLIERS and res[3]["n_in"] == 0 and res[3]["best_it"] == -1
    for r in res:
        print(H.info_of(r), r["sel_margin"], r["gap_margin"], r["thr_margin"], r["eig_ratio"])
        assert r["sel_margin"] >= H.MARGIN_MIN and r["gap_margin"] >= H.MARGIN_MIN and r["thr_margin"] >= H.MARGIN_MIN
        assert H.margins_ok(r)


def test_oracle_codes_on_small_scenes():
    rng = np.random.RandomState(7)
    plane = H.plane_under_tap(rng, 60)
    tap = (320.0, 240.0)
    assert H.oracle(plane[:23], H.POSE_BASE, H.K_BASE, tap, 40.0)["code"] == 1
    assert H.oracle(plane[:24], H.POSE_BASE, H.K_BASE, tap, 40.0)["code"] == 0
    assert H.oracle(np.zeros((0, 3)), H.POSE_BASE, H.K_BASE, tap, 40.0)["code"] == 1
    # words (0, 0, x): two equal indices, every hypothesis skipped
    r = H.oracle(plane, H.POSE_BASE, H.K_BASE, tap, 40.0, rand3=[[0, 0, 1 << 31]] * 4)
    assert r["code"] == 2 and r["m"] == 60 and r["best_it"] == -1
    # points behind the camera that project into the circle are not selected
    behind = 2 * H.POSE_BASE[:3] - plane
    r = H.oracle(np.vstack([behind, plane]), H.POSE_BASE, H.K_BASE, tap, 40.0)
    assert r["m"] == 60 and r["sel"].min() == 60


def test_headers_declare_the_hit_test():
    hip = (ROOT / "include" / "alvaar_hip.h").read_text()
    sysh = (ROOT / "include" / "alvaar_system.h").read_text()
    assert re.search(r"\bint\s+alva_hit_test\s*\(\s*alva_ctx\s*\*", hip)
    assert re.search(r"\bint\s+alva_system_hit_test\s*\(\s*alva_system\s*\*", sysh)


def test_system_class_hit_test_compiles():
    src = r'''
#include "alvaar_system.h"
int use(alva::System &s, const float *uv, float *poses, int *info) {
    int (alva::System::*native)(const float *, int, float, int, float *, int *) = &alva::System::hitTest;
    (void) native;
    return s.hitTest(uv, 5, 40.0f, 64, poses, info);
}
'''
    with tempfile.TemporaryDirectory() as d:
        f = Path(d) / "t.cpp"
        f.write_text(src)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-fsyntax-only", str(f)])


def test_every_edge_case_is_far_from_a_last_bit_decision():
    for name, case in H.edge_cases().items():
        res = H.oracle_case(case)
        codes = [r["code"] for r in res]
        print(name, [H.info_of(r)[:5] for r in res], ["%.1e %.1e %.1e %.1e" % (r["sel_margin"], r["gap_margin"], r["thr_margin"], r["eig_ratio"]) for r in res])
        if case["want"] is not None:
            assert codes == case["want"], (name, codes)
        for r in res:
            assert H.margins_ok(r), (name, H.info_of(r), r["sel_margin"], r["gap_margin"], r["thr_margin"], r["eig_ratio"])
    c = H.oracle_case(H.edge_cases()["cap5000"])[0]
    assert c["n_sel"] == 5000 and c["m"] == H.HIT_CAP and list(c["sel"]) == list(range(H.HIT_CAP))
    e = H.oracle_case(H.edge_cases()["exact_plane"])[0]
    assert e["n_in"] == e["m"] == 192 and e["moments"][3] == 0 and e["moments"][9] == 0   # score 0: every point is an inlier by `<=`
    assert H.oracle_case(H.edge_cases()["m23"])[0]["m"] == 23 and H.oracle_case(H.edge_cases()["m24"])[0]["m"] == 24
