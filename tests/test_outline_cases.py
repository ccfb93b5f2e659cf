"""CPU: the restatement of the plane outline (tests/outline_cases.py) -- its hull equals a brute-force hull on random small sets and
does not depend on the order of the points, every scene of the GPU tests is what it is meant to be -- and the public surface: the
headers declare alva_plane_outlines / alva_system_detect_plane_outlines, alva::System::detectPlaneOutlines compiles and the library
exports both."""
import itertools
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import outline_cases as O
import plane_cases as C

ROOT = Path(__file__).resolve().parent.parent


def in_closed_hull(p, others) -> bool:
    """is p in the closed convex hull of the distinct points `others` (p not among them)?  By Caratheodory, iff it lies on a segment
    between two of them or in a closed triangle of three of them.  Integer predicates only"""
    for a, b in itertools.combinations(others, 2):
        if O.cross(a, b, p) == 0 and (a[0] - p[0]) * (b[0] - p[0]) + (a[1] - p[1]) * (b[1] - p[1]) <= 0:
            return True
    for a, b, c in itertools.combinations(others, 3):
        s = [O.cross(a, b, p), O.cross(b, c, p), O.cross(c, a, p)]
        if O.cross(a, b, c) != 0 and (all(v >= 0 for v in s) or all(v <= 0 for v in s)):
            return True
    return False


def check_polygon(verts):
    """strictly convex, counter-clockwise, from the lexicographically smallest vertex"""
    h = len(verts)
    assert h >= 3 and verts[0] == min(verts) and len(set(verts)) == h
    for i in range(h):
        a, b, c = verts[i], verts[(i + 1) % h], verts[(i + 2) % h]
        assert (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]) > 0


def test_the_hull_equals_a_brute_force_hull_on_200_random_small_sets():
    rng = np.random.RandomState(7)
    seen_sizes = set()
    for t in range(200):
        n, span = rng.randint(1, 13), (2, 3, 5, 50, O.Q_MAX)[t % 5]   # small spans: many collinear triples and duplicates
        q = rng.randint(-span, span + 1, (n, 2))
        if t % 10 == 9:
            q[:, 1] = 2 * q[:, 0] % (span + 1)
        pts = sorted(set(map(tuple, q.tolist())))
        brute = [p for p in pts if not in_closed_hull(p, [o for o in pts if o != p])]
        got = O.hull(q)
        assert sorted(got) == brute, (q.tolist(), got, brute)
        if len(got) >= 3:
            check_polygon(got)
            assert O.area2(got) > 0
        else:   # no area: one point, or the two ends of a segment
            assert len(pts) == 1 or all(O.cross(pts[0], pts[-1], p) == 0 for p in pts)
        seen_sizes.add(min(len(got), 5))
    assert seen_sizes == {1, 2, 3, 4, 5}


def test_the_restatement_does_not_depend_on_the_order_of_the_points():
    s, want = O.scenes()["base"], O.oracle_of("base")
    perm = np.random.RandomState(3).permutation(len(s["P"]))
    got = O.oracle(s["P"][perm], s["labels"][perm], s["planes"])
    for key in ("outline", "q", "info", "area"):
        assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), key


def test_exact_plane_gives_the_four_grid_corners():
    r = O.oracle_of("exact_plane")
    rec = O.scenes()["exact_plane"]["planes"][0]
    assert rec[16] == np.float32(15 / 64) and rec[17] == np.float32(11 / 64)
    assert r["info"][0].tolist() == [0, 4, 192, 0, 0, 0, 0, 0]   # 16 x 12 grid points, those on the edges are no vertices
    hu, hv = 1 << 19, (11 << 19) // 15 + 1                      # half extents in cells of (15 / 64) / 2^20: 2^19 and rint(384477.87)
    assert r["q"][0, :4].tolist() == [[-hu, -hv], [hu, -hv], [hu, hv], [-hu, hv]] and not r["q"][0, 4:].any()
    assert abs(r["area"][0] / ((15 / 64) * (11 / 64)) - 1) < 1e-5
    assert r["outline"][0, 2].tolist() == [np.float32(15 / 128), np.float32(hv * (15 / 64) / 2 ** 20)]


def test_the_base_scenes_hulls_cover_four_fifths_of_their_rectangles():
    r, s = O.oracle_of("base"), O.scenes()["base"]
    assert r["info"][:, :3].tolist() == [[0, 15, 1606], [0, 16, 897]] and r["found"] == 2
    ratio = [r["area"][k] / (float(s["planes"][k, 16]) * float(s["planes"][k, 17])) for k in range(2)]
    print(ratio)
    assert [round(v, 3) for v in ratio] == [0.791, 0.776]
    for k in range(2):   # every point of the plane lies in the polygon's closed interior
        code, x, z, p, ext = O.frame(s["planes"][k])
        q = O.quantise(s["P"][s["labels"] == k], x, z, p, ext)
        v = [tuple(map(int, a)) for a in r["q"][k, :r["info"][k, 1]]]
        for i in range(len(v)):
            a, b = v[i], v[(i + 1) % len(v)]
            assert ((b[0] - a[0]) * (q[:, 1] - a[1]) - (b[1] - a[1]) * (q[:, 0] - a[0]) >= 0).all()


def test_every_scene_is_what_it_is_meant_to_be():
    S, R = O.scenes(), {name: O.oracle_of(name) for name in O.scenes()}
    for name, r in R.items():   # the found planes of the detector's scenes have 4 to 24 vertices
        for k in range(len(r["info"])):
            if r["info"][k, 0] == 0 and not name.startswith(("circle", "m3")):
                assert 4 <= r["info"][k, 1] <= 24, (name, k)
            if r["info"][k, 0] == 0:
                check_polygon([tuple(map(int, a)) for a in r["q"][k, :r["info"][k, 1]]])
            else:
                assert not r["outline"][k].any() and not r["q"][k].any() and r["area"][k] == 0 and r["info"][k, 1] == 0
    for n in (63, 64, 65, 511, 512, 513, 2049):
        assert R["n%d" % n]["info"][0, [0, 2]].tolist() == [0, n], n   # the detector labels every point of these planes
    assert R["m2"]["info"][0].tolist() == [1, 0, 2, 0, 0, 0, 0, 0] and R["m3"]["info"][0, :3].tolist() == [0, 3, 3]
    assert R["n16384"]["info"][0, [0, 2]].tolist() == [0, O.N_CAP]
    assert R["rotated"]["info"][:, :3].tolist() == [[0, 15, 1606], [0, 16, 897]]
    assert R["base_max8"]["info"][:, 0].tolist() == [0, 0, 5, 5, 5, 5, 5, 5] and not S["base_max8"]["planes"][2:].any()
    base = R["base"]
    for name in ("interleaved", "foreign_labels"):
        assert all(np.array_equal(R[name][key], base[key]) for key in ("outline", "q", "info", "area")), name
    lab = S["interleaved"]["labels"]
    assert lab[:1794:2].tolist() == [0] * 897 and lab[1:1794:2].tolist() == [1] * 897
    lab = S["foreign_labels"]["labels"]
    assert (lab == 2).sum() > 100 and (lab == -7).sum() > 50 and (lab == 1 << 30).sum() > 30 and (lab == -1).sum() > 0
    w = R["wall_only"]
    assert w["info"][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and np.array_equal(w["q"][1], base["q"][1]) and w["area"][1] == base["area"][1]
    assert R["collinear"]["info"][0].tolist() == [2, 0, 40, 0, 0, 0, 0, 0] and R["identical"]["info"][0].tolist() == [2, 0, 40, 0, 0, 0, 0, 0]
    d, s = R["duplicated"], R["n513"]
    assert d["info"][0].tolist() == [0, s["info"][0, 1], 2 * 513, 0, 0, 0, 0, 0]
    assert np.array_equal(d["q"], s["q"]) and np.array_equal(d["outline"], s["outline"]) and d["area"][0] == s["area"][0]
    c = R["circle"]
    assert c["info"][0].tolist() == [0, O.CIRCLE_N, O.CIRCLE_N, 0, 0, 0, 0, 0]   # the hull is all 600 points
    radius2 = (c["q"][0, :O.CIRCLE_N].astype(np.int64) ** 2).sum(axis=1)
    assert np.abs(np.sqrt(radius2) - O.CIRCLE_R).max() < 1 and abs(c["area"][0] / np.pi - 1) < 1e-4
    assert R["circle_64"]["info"][0].tolist() == [3, 0, O.CIRCLE_N, 0, 0, 0, 0, 0]
    for name in ("zero_extents", "nan_centre", "inf_extent"):
        for k in (0, 1):
            r = R["%s_%d" % (name, k)]
            assert r["info"][k].tolist() == [4, 0, 0, 0, 0, 0, 0, 0]
            assert np.array_equal(r["q"][1 - k], base["q"][1 - k]) and r["area"][1 - k] == base["area"][1 - k]
    assert C.oracle_of("base")["info"][:, 0].tolist() == [0, 0, 3, 5]


def test_frame_codes():
    rec = O.hand_frame([0.0, 0.0, 4.0], 2.0, 1.0)
    assert O.frame(rec)[0] == 0 and O.frame(rec)[4] == 2.0
    assert O.frame(np.zeros(24, np.float32))[0] == 5
    for idx, val in ((16, np.nan), (17, np.nan), (16, np.inf), (0, np.nan), (10, np.inf), (14, -np.inf)):
        bad = rec.copy()
        bad[idx] = val
        assert O.frame(bad)[0] == 4, (idx, val)
    bad = rec.copy()
    bad[16:18] = [-1.0, 0.0]
    assert O.frame(bad)[0] == 4
    bad[15] = 2
    assert O.frame(bad)[0] == 5   # the record check comes first


def test_rounding_is_half_to_even_and_clamped():
    x, z, p = np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.zeros(3)
    cell = 2.0 ** -20
    P = np.array([[0.5 * cell, 1.5 * cell, 0], [2.5 * cell, -0.5 * cell, 0], [9.0, -9.0, 0]])
    assert O.quantise(P, x, z, p, 1.0).tolist() == [[0, 2], [2, 0], [O.Q_MAX, -O.Q_MAX]]


def test_headers_declare_plane_outlines():
    hip = (ROOT / "include" / "alvaar_hip.h").read_text()
    sysh = (ROOT / "include" / "alvaar_system.h").read_text()
    assert re.search(r"\bint\s+alva_plane_outlines\s*\(\s*alva_ctx\s*\*", hip)
    assert re.search(r"\bint\s+alva_system_detect_plane_outlines\s*\(\s*alva_system\s*\*", sysh)


def test_system_class_detect_plane_outlines_compiles():
    src = r'''
#include "alvaar_system.h"
int use(alva::System &s, float *planes, int *info, int *ids, int *labels, float *outlines, int *oinfo, double *areas) {
    int (alva::System::*native)(double, int, int, int, float *, int *, int *, int *, int, int, float *, int *, double *) =
        &alva::System::detectPlaneOutlines;
    (void) native;
    return s.detectPlaneOutlines(0.01, 48, 4, 128, planes, info, ids, labels, 16384, 64, outlines, oinfo, areas);
}
'''
    with tempfile.TemporaryDirectory() as d:
        f = Path(d) / "t.cpp"
        f.write_text(src)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-fsyntax-only", str(f)])


def test_library_exports_plane_outlines():
    import ctypes
    lib = ctypes.CDLL(str(ROOT / "alvaar_amd" / "libalvaar_hip.so"))
    assert hasattr(lib, "alva_plane_outlines") and hasattr(lib, "alva_system_detect_plane_outlines")
