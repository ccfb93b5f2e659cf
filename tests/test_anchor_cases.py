"""CPU: the numpy restatement of the anchors (tests/anchor_cases.py) -- every case of the GPU tests gives the code it was built for and
is far from every decision a last bit could turn (or sits on it exactly, by construction); a planted rigid motion comes back to 1e-12,
with four gross outliers too; an unmoved map gives I and 0 bit for bit; a half turn and a collinear support behave -- the host list
(csrc/slam/anchors.hpp, through the stand-alone tests/cpp/anchors_host.cpp) and its restatement, and the public surface: the headers
declare alva_anchor_attach / alva_anchor_update / alva_system_create_anchors / _update_anchors / _remove_anchor / _reset_anchors,
alva::System's four methods compile, the library exports them."""
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import anchor_cases as A

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("name", sorted(A.update_cases()))
def test_every_case_gives_its_code_with_safe_margins(name):
    case, r = A.update_cases()[name], A.oracle_of(name)
    print(name, r["info"].tolist(), A.margins_text(r))
    assert r["code"] == case["code"] and r["m"] == case["count"] and r["kept"] == case["kept"]
    assert r["info"].tolist() == [case["code"], case["count"], case["kept"], 0, 0, 0, 0, 0]
    for key in ("trim_margin", "gap_margin"):
        assert r[key] == 0 if key in case["exact"] else r[key] >= A.MARGIN_MIN, key
    for key in ("m_from_4", "kept_from_4"):   # integers: exactly at the bound where the case says so, at least 1 away otherwise
        assert (r[key] == 0) == (key in case["exact"]), key
    assert A.margins_ok(r, case["exact"])
    assert r["pose"][15] == 1 and not r["pose"][[3, 7, 11]].any()


@pytest.mark.parametrize("name", ["planted32", "outliers4", "rot1", "rot90", "rot180", "translation", "m4", "m63", "m64"])
def test_a_planted_motion_is_recovered(name):
    case, r = A.update_cases()[name], A.oracle_of(name)
    dR, dt = np.abs(np.array(r["R"]) - case["R"]).max(), np.abs(np.array(r["t"]) - case["t"]).max()
    print(name, "max |dR| %.3g  max |dt| %.3g" % (dR, dt))
    assert dR <= 1e-12 and dt <= 1e-12
    # and the pose is [R | t] o the reference pose
    ref = case["pose_ref"].astype(np.float64)
    want = np.concatenate([np.concatenate([case["R"] @ ref[4 * c:4 * c + 3] + (case["t"] if c == 3 else 0), [float(c == 3)]]) for c in range(4)])
    assert np.abs(r["pose"] - want).max() <= 1e-6


def test_four_gross_outliers_are_dropped():
    r = A.oracle_of("outliers4")
    assert r["kept"] == 28 and r["refit_det"] and r["code"] == 0
    first = A.rigid_fit(np.arange(64) < 32, A.update_cases()["outliers4"]["ref"], A.update_cases()["outliers4"]["cur"])
    assert np.abs(np.array(first["R"]) - A.PLANTED_R).max() > 1e-3   # (the first fit was off: the refit did the work)


def test_an_unmoved_map_gives_identity_bit_for_bit():
    r = A.oracle_of("identity")
    want = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
    assert np.array_equal(r["rt12"].view(np.uint64), want.view(np.uint64))
    assert np.array_equal(r["pose"].view(np.uint32), A.POSE_REF.view(np.uint32))
    assert r["med"] == 0 and r["kept"] == 32   # the med = 0 clause: r_j <= 1e-9 rho keeps every support


def test_a_half_turn_has_w_zero():
    case, r = A.update_cases()["rot180"], A.oracle_of("rot180")
    assert abs(np.trace(np.array(r["R"])) + 1) <= 1e-12     # trace = 1 + 2 cos(180 deg)
    assert np.abs(np.array(r["R"]) - case["R"]).max() <= 1e-12


def test_collinear_supports_are_translation_only():
    for name in ("collinear", "near_line_under"):
        case, r = A.update_cases()[name], A.oracle_of(name)
        assert r["code"] == 1 and np.array_equal(np.array(r["R"]), np.eye(3))
        m = case["count"]
        assert np.abs(np.array(r["t"]) - (case["cur"][:m].mean(0) - case["ref"][:m].mean(0))).max() <= 1e-12
    assert A.oracle_of("near_line_over")["code"] == 0


def test_the_first_fit_stands_when_the_trim_leaves_too_few():
    case, r = A.update_cases()["trim_to_3"], A.oracle_of("trim_to_3")
    first = A.rigid_fit(np.arange(64) < 5, case["ref"], case["cur"])
    assert r["kept"] == 3 and "refit_det" not in r and first["det"]
    assert np.array_equal(np.array(r["R"]), np.array(first["R"])) and r["t"] == first["t"]


def test_wave_sum_is_the_butterfly():
    """the tree over adjacent pairs equals the xor butterfly, masks 1 2 4 .. 32, in every lane"""
    rng = np.random.default_rng(5)
    v = rng.standard_normal(64) * 10.0 ** rng.integers(-8, 8, 64)
    s = v.copy()
    for k in range(6):
        s = s + s[np.arange(64) ^ (1 << k)]
    assert (s == s[0]).all() and s[0] == A.wave_sum(v)


# ------------------------------------------------------------------------------------------------ stage 1
@pytest.mark.parametrize("K", [8, 64])
def test_attach_restatement(K):
    for n in A.attach_sizes(K):
        P, pos = A.attach_points(n)
        index, dist2, count = A.attach(P, pos, K)
        assert (count == min(K, n)).all()
        for a in range(len(pos)):
            c = count[a]
            assert (index[a, c:] == -1).all() and not dist2[a, c:].any()
            d = ((P - pos[a]) ** 2).sum(1)
            assert sorted(index[a, :c].tolist()) == sorted(np.argsort(d, kind="stable")[:c].tolist())
            assert (np.diff(dist2[a, :c]) >= 0).all()


def test_attach_ties_go_to_the_lower_index():
    P, pos = A.lattice()
    index, dist2, count = A.attach(P, pos, 8)
    centre = 5 * 121 + 5 * 11 + 5
    assert dist2[0].tolist() == [0, 1, 1, 1, 1, 1, 1, 2] and index[0, 0] == centre
    assert index[0, 1:7].tolist() == sorted(index[0, 1:7].tolist())
    d = (P ** 2).sum(1)
    assert index[0, 7] == np.flatnonzero(d == 2).min()     # twelve points at d = 2: the lowest index
    P, pos = A.duplicates()
    index, dist2, count = A.attach(P, pos, 9)
    for j in range(0, 9, 3):   # the three copies of a point side by side, ascending index
        assert dist2[0, j] == dist2[0, j + 1] == dist2[0, j + 2] and index[0, j + 1] == index[0, j] + 40 and index[0, j + 2] == index[0, j] + 80


# ------------------------------------------------------------------------------------------------ the list
def test_anchor_list_bookkeeping(tmp_path):
    """csrc/slam/anchors.hpp through its stand-alone program: ids not reused, supports dropped for good, the re-attach trigger at
    exactly half, clearing on a generation change, the 65th anchor refused"""
    exe = tmp_path / "anchors_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(ROOT / "tests" / "cpp" / "anchors_host.cpp")])
    out = subprocess.run([str(exe)], text=True, capture_output=True)
    assert out.returncode == 0 and re.fullmatch(r"\d+ 0 failures", out.stdout.strip()), out.stdout


def test_the_restated_list_follows_the_same_rules():
    attach_fn, update_fn = A.oracle_fns()
    rng = np.random.default_rng(9)
    ids, P = np.arange(100, 140, dtype=np.int32), rng.standard_normal((40, 3))
    L = A.Anchors()
    got, info = L.create(np.stack([A.pose_of(t=P[3]), A.pose_of(t=(np.nan, 0, 0)), A.pose_of(t=P[20])]), 10, ids, P, attach_fn)
    assert got.tolist() == [0, -1, 1] and info[:, :3].tolist() == [[0, 10, 40], [4, 0, 40], [0, 10, 40]]
    assert L.list[0]["sup"][0] == 103 and L.list[1]["sup"][0] == 120            # an anchor on a point: that point first
    assert L.create(A.pose_of()[None], 10, ids[:3], P[:3], attach_fn)[1][0, :3].tolist() == [1, 0, 3]
    # an unmoved map: identity, nobody re-attached
    aid, pose, info = L.update(ids, P, update_fn, attach_fn)
    assert aid.tolist() == [0, 1] and info[:, :6].tolist() == [[0, 10, 10, 0, 1, 10]] * 2
    assert np.array_equal(pose[0].view(np.uint32), A.pose_of(t=P[3]).view(np.uint32))
    # five of anchor 0's ten supports vanish: exactly half, no re-attach; a sixth: re-attached to the ten nearest that remain
    sup = list(L.list[0]["sup"])
    keep = ~np.isin(ids, sup[:5])
    aid, pose, info = L.update(ids[keep], P[keep], update_fn, attach_fn)
    assert info[0, :6].tolist() == [0, 5, 5, 0, 2, 10] and L.list[0]["sup"] == sup[5:]
    keep &= ~np.isin(ids, sup[5:6])
    aid, pose, info = L.update(ids[keep], P[keep], update_fn, attach_fn)
    assert info[0, :6].tolist() == [0, 4, 4, 1, 3, 10] and len(L.list[0]["sup"]) == 10 and not set(L.list[0]["sup"]) & set(sup[:6])
    aid, pose, info = L.update(ids, P, update_fn, attach_fn)                      # the vanished points are back in the map: not in the anchor
    assert info[0, :6].tolist() == [0, 10, 10, 0, 4, 10] and not set(L.list[0]["sup"]) & set(sup[:6])
    # not tracking: code 6, the last pose, the list as it was
    aid, pose6, info = L.not_tracking()
    assert info[:, 0].tolist() == [6, 6] and np.array_equal(pose6, pose) and info[0, 4] == 4
    assert L.remove(0) == 1 and L.remove(0) == 0 and [a["id"] for a in L.list] == [1]
    L.clear()
    assert L.create(A.pose_of()[None], 8, ids, P, attach_fn)[0].tolist() == [2]   # ids go on
    for _ in range(63):
        L.create(A.pose_of()[None], 8, ids, P, attach_fn)
    got, info = L.create(A.pose_of()[None], 8, ids, P, attach_fn)
    assert got.tolist() == [-1] and info[0, 0] == 3 and len(L.list) == 64


# ------------------------------------------------------------------------------------------------ headers and exports
NAMES = ("alva_anchor_attach", "alva_anchor_update", "alva_system_create_anchors", "alva_system_update_anchors", "alva_system_remove_anchor",
         "alva_system_reset_anchors")


def test_headers_declare_the_anchors():
    hip = (ROOT / "include" / "alvaar_hip.h").read_text()
    sysh = (ROOT / "include" / "alvaar_system.h").read_text()
    assert re.search(r"\bint\s+alva_anchor_attach\s*\(\s*alva_ctx\s*\*", hip) and re.search(r"\bint\s+alva_anchor_update\s*\(\s*alva_ctx\s*\*", hip)
    for name in ("create_anchors", "update_anchors", "remove_anchor"):
        assert re.search(r"\bint\s+alva_system_%s\s*\(\s*alva_system\s*\*" % name, sysh), name
    assert re.search(r"\bvoid\s+alva_system_reset_anchors\s*\(\s*alva_system\s*\*", sysh)
    assert "masks 1, 2, 4, 8, 16, 32" in hip   # the order of the sums is part of the definition


def test_system_class_anchor_methods_compile():
    src = r'''
#include "alvaar_system.h"
int use(alva::System &s, const float *poses, int *ids, float *out, int *info) {
    int (alva::System::*create)(const float *, int, int, int *, int *) = &alva::System::createAnchors;
    int (alva::System::*update)(int, int *, float *, int *) = &alva::System::updateAnchors;
    int (alva::System::*remove)(int) = &alva::System::removeAnchor;
    void (alva::System::*forget)() = &alva::System::resetAnchors;
    (void) create; (void) update; (void) remove; (void) forget;
    const int made = s.createAnchors(poses, 3, 32, ids, info);
    const int n = s.updateAnchors(64, ids, out, info);
    const int gone = s.removeAnchor(ids[0]);
    s.resetAnchors();
    return made + n + gone;
}
'''
    with tempfile.TemporaryDirectory() as d:
        f = Path(d) / "t.cpp"
        f.write_text(src)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-fsyntax-only", str(f)])


def test_library_exports_the_anchors():
    import ctypes
    lib = ctypes.CDLL(str(ROOT / "alvaar_amd" / "libalvaar_hip.so"))
    assert all(hasattr(lib, name) for name in NAMES)
