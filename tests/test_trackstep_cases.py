"""CPU: the tracking step's restatement and case tables (tests/trackstep_cases.py) are what tests/test_gpu_trackstep.py compares the HIP step
with -- so every property a case is named for is asserted here, on the restatement's own outcome: a change of synth or of the pool
cannot silently empty a case."""
import numpy as np
import pytest

import trackstep_cases as T


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _alt_differs(w):
    """retried slots whose outcome under the other value of p3p_req differs in code or in position bits"""
    return w["retried"] & ((w["code"] != w["alt_code"]) | (_bits(w["px"]) != _bits(w["alt_px"])).any(1))


def test_scene():
    rgba, gray = T.frames()
    assert len(rgba) == 6 and all(f.shape == (T.H, T.W, 4) for f in rgba)
    assert all(np.array_equal(g, f[..., 0]) for g, f in zip(gray, rgba))     # (r = g = b: the gray conversion is the identity on them)
    dx, dy = T.SHIFT[1]
    assert np.array_equal(gray[0][20:200, 20:280], gray[1][20 + dy:200 + dy, 20 + dx:280 + dx])     # the content moved by MOTION
    assert gray[T.FLAT].min() == gray[T.FLAT].max()
    assert np.all(T.CALIB8[4:] != 0)
    assert not np.array_equal(T.TCW_Q, [0, 0, 0, 1]) and np.any(T.TCW_T != 0) and abs((T.TCW_Q ** 2).sum() - 1) < 1e-15


def test_world_point_projects_to_its_prior():
    rng = np.random.RandomState(0)
    u = np.stack([rng.uniform(-5, T.W + 5, 200), rng.uniform(-5, T.H + 5, 200)], 1)
    for depth in (0.7, 4.0, -3.0):     # behind the camera: the same pixel
        assert np.abs(T.project(T.world_point(u, np.full(200, depth))) - u).max() < 2e-3


def test_pool():
    P = T.pool()
    n = len(P["kind"])
    assert 300 <= n <= 1200
    kinds = set(P["kind"])
    assert {"close", "off", "far", "slight", "behind", "2d", "out0", "out1", "out2", "out3"} <= kinds
    q = P["proj"]
    for side, m in enumerate((q[:, 0] < 0, q[:, 1] < 0, q[:, 0] >= np.float32(T.W), q[:, 1] >= np.float32(T.H))):
        out = P["kind"] == "out%d" % side
        assert out.sum() >= 4 and m[out].all() and not P["from_prior"][out].any()
        d = np.where(side % 2 == 0, q[out, 0], q[out, 1]) - (0 if side < 2 else (T.W, T.H)[side - 2])
        assert np.all(np.abs(d) < 1.0)      # outside by a fraction of a pixel
    # on the bounds themselves: width and height exactly (outside), the last float32 below them (inside), 0 from both sides
    k = {name: int(np.flatnonzero(P["kind"] == name)[0]) for name in kinds if name.startswith("edge_")}
    assert q[k["edge_hi_0_320"], 0] == np.float32(T.W) and not P["from_prior"][k["edge_hi_0_320"]]
    assert q[k["edge_hi_1_240"], 1] == np.float32(T.H) and not P["from_prior"][k["edge_hi_1_240"]]
    assert q[k["edge_lo_0_320"], 0] == np.nextafter(np.float32(T.W), np.float32(0)) and P["from_prior"][k["edge_lo_0_320"]]
    assert q[k["edge_lo_1_240"], 1] == np.nextafter(np.float32(T.H), np.float32(0)) and P["from_prior"][k["edge_lo_1_240"]]
    assert 0 <= q[k["edge_hi_0_0"], 0] < 1e-4 and P["from_prior"][k["edge_hi_0_0"]]
    assert 0 <= q[k["edge_hi_1_0"], 1] < 1e-4 and P["from_prior"][k["edge_hi_1_0"]]
    assert -1e-4 < q[k["edge_lo_0_0"], 0] < 0 and not P["from_prior"][k["edge_lo_0_0"]]
    assert -1e-4 < q[k["edge_lo_1_0"], 1] < 0 and not P["from_prior"][k["edge_lo_1_0"]]
    behind = P["kind"] == "behind"
    zc = T.se3_apply(T.TCW_Q, T.TCW_T, P["wpt"][behind])[:, 2]
    assert np.all(zc < 0) and P["from_prior"][behind].all()      # the step does not look at the depth's sign
    # priors relative to the true motion
    d = np.linalg.norm(q - (P["px"] + T.MOTION), axis=1)
    assert d[P["kind"] == "close"].max() < 0.7
    assert 3.5 < d[P["kind"] == "off"].min() and d[P["kind"] == "off"].max() < 14.5
    assert d[P["kind"] == "far"].min() > 17
    assert not P["is3d"][(P["kind"] == "2d") | (P["kind"] == "2d_border")].any()


@pytest.mark.parametrize("name", T.case_names())
def test_case_is_consistent(name):
    c = T.case(name)
    w = c["want"]
    n = c["n"]
    assert len(c["px"]) == len(c["is3d"]) == len(c["wpt"]) == len(w["code"]) == n
    lost = w["code"] == 0
    assert not w["px"][lost].any() and not w["unpx"][lost].any() and not w["bv"][lost].any()
    assert np.all(np.abs(np.linalg.norm(w["bv"][~lost], axis=1) - 1) < 1e-15)
    sel = np.flatnonzero((c["is3d"] != 0) & ~lost)
    assert w["n_pose"] == len(sel) == len(w["Pbv"]) == len(w["Puv"]) == len(w["Pwpt"])
    assert np.array_equal(_bits(w["Pwpt"]), _bits(c["wpt"][sel])) and np.array_equal(_bits(w["Pbv"]), _bits(w["bv"][sel]))
    assert np.array_equal(w["Puv"], w["unpx"][sel].astype(np.float64))
    assert w["good"] == (w["code"] == 1).sum() and w["n_prior"] == w["from_prior"].sum()
    assert w["p3p_req"] == int(w["n_prior"] > 0 and float(w["good"]) < 0.33 * float(w["n_prior"]))
    assert np.array_equal(w["retried"], w["from_prior"] & (w["code"] != 1))
    assert set(np.unique(w["code"][w["retried"]])) <= {0, 3} and not np.any((w["code"] == 3) & ~w["retried"])
    if w["alt_code"] is not None:
        same = ~w["retried"]
        assert np.array_equal(w["alt_code"][same], w["code"][same]) and np.array_equal(_bits(w["alt_px"][same]), _bits(w["px"][same]))


def test_mixed_200():
    c = T.case("mixed_200")
    w = c["want"]
    assert c["n"] == 200 and c["use_prior"] == 1 and w["p3p_req"] == 0
    assert np.bincount(w["code"], minlength=4).min() >= 10      # every code at least 10 times
    d3, lost = c["is3d"] != 0, w["code"] == 0
    assert (lost & w["retried"]).sum() >= 1        # prior pass and retry both failed
    assert (lost & d3 & ~w["from_prior"]).sum() >= 1   # full pyramid failed
    assert (lost & ~d3).sum() >= 1                 # 2-D failed
    q = np.zeros((200, 2), np.float32)
    q[d3] = T.project(c["wpt"][d3])
    for m in (q[:, 0] < 0, q[:, 1] < 0, q[:, 0] >= np.float32(T.W), q[:, 1] >= np.float32(T.H)):
        assert (m & d3).sum() >= 1 and not w["from_prior"][m & d3].any()
    # a tenth of the 3-D slots have a world point that is wrong: it projects far from where the image content went; some of them survive
    # the tracker and are the pose solve's outliers
    wrong = d3 & (np.linalg.norm(q - (c["px"] + T.MOTION), axis=1) > 15)
    assert wrong.sum() >= 0.1 * d3.sum() and (wrong & ~lost).sum() >= 10
    # ... and a few are wrong by less than P3P's 3 px and more than the refinement's 2.45 px: tracked to where the image went
    slight = d3 & (w["code"] == 1) & (np.abs(np.linalg.norm(q - (c["px"] + T.MOTION), axis=1) - 2.75) < 0.2)
    assert (slight & (np.linalg.norm(w["px"] - (c["px"] + T.MOTION), axis=1) < 0.3)).sum() >= 5
    # slot kinds interleave
    assert (np.diff((d3 & ~lost).astype(int)) != 0).sum() >= 50


def test_no_prior_200():
    c, m = T.case("no_prior_200"), T.case("mixed_200")
    w = c["want"]
    assert c["use_prior"] == 0 and all(np.array_equal(c[k], m[k]) for k in ("px", "is3d", "wpt"))
    assert set(np.unique(w["code"])) == {0, 2} and w["p3p_req"] == 0 and w["n_prior"] == 0
    assert (w["code"] == 0).sum() >= 10 and (w["code"] == 2).sum() >= 10


@pytest.mark.parametrize("name,good,n_prior,req", [("req_33_of_100", 33, 100, 0), ("req_32_of_100", 32, 100, 1), ("req_1_of_3", 1, 3, 0),
                                                   ("req_0_of_3", 0, 3, 1), ("req_no_3d", 0, 0, 0)])
def test_req_cases(name, good, n_prior, req):
    w = T.case(name)["want"]
    assert (w["good"], w["n_prior"], w["p3p_req"]) == (good, n_prior, req)
    if name == "req_no_3d":
        assert not T.case(name)["is3d"].any() and w["n_pose"] == 0
    if req:
        # the retry launch can be told from the first launch: at least 10 retried slots (all of them where there are fewer) come out
        # differently under p3p_req = 0, and at least one retried slot ends tracked
        differs = _alt_differs(w)
        assert differs.sum() >= min(10, w["retried"].sum()) and w["retried"].sum() == n_prior - good
        assert (w["code"][w["retried"]] == 3).sum() >= 1
    elif n_prior:
        assert _alt_differs(w).sum() >= 1      # and the other way round: the first launch's result is not the retry launch's


def test_all_lost():
    c = T.case("all_lost")
    w = c["want"]
    assert c["frames"] == (0, T.FLAT) and not w["code"].any() and w["n_pose"] == 0 and w["p3p_req"] == 1 and w["n_prior"] >= 10


@pytest.mark.parametrize("name,n_pose", [("pose_3", 3), ("pose_4", 4)])
def test_pose_edge_cases(name, n_pose):
    c = T.case(name)
    w = c["want"]
    assert w["n_pose"] == n_pose and w["p3p_req"] == 0
    assert ((c["is3d"] != 0) & (w["code"] == 0)).sum() >= 1 and ((c["is3d"] == 0) & (w["code"] != 0)).sum() >= 1


def test_size_edges():
    base = T.case("size_513")
    for n in T.SIZE_EDGES:
        c = T.case("size_%d" % n)
        assert c["n"] == n and all(np.array_equal(c[k], base[k][:n]) for k in ("px", "is3d", "wpt"))      # one table, cut
    for n in T.SIZE_EDGES + T.SIZE_LARGE:
        c = T.case("size_%d" % n)
        w = c["want"]
        assert c["n"] == n
        if n >= 63:
            corr = ((c["is3d"] != 0) & (w["code"] != 0)).astype(int)
            runs = np.diff(np.flatnonzero(np.diff(corr) != 0))
            assert 0 < corr.sum() < n and (np.diff(corr) != 0).sum() >= n // 4 and len(set(runs)) >= 3      # irregular alternation
            assert np.bincount(w["code"], minlength=4).min() >= 1
    # sizes where the 16-byte copy units of the staged table end past n: 8n, n, 24n
    assert any(8 * n % 16 for n in T.SIZE_EDGES) and any(n % 16 for n in T.SIZE_EDGES) and any(24 * n % 16 for n in T.SIZE_EDGES)
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parent.parent / "alvaar_amd" / "csrc" / "track_slices.hpp").read_text()
    nt, max_wg = (int(re.search(r"%s = (\d+)" % k, src).group(1)) for k in ("CMP_NT", "CMP_MAX_WG"))
    assert max(T.SIZE_LARGE) > nt * max_wg and 7168 in T.SIZE_LARGE and 6145 in T.SIZE_LARGE and 2049 in T.SIZE_LARGE


def test_carry_chain():
    a, b, c, d = T.carry_chain()
    assert a["carry"] is None and d["carry"] is None and a["name"] == "mixed_200"
    for prev, s in ((a, b), (b, c)):
        carry = s["carry"]
        assert carry.dtype == np.uint16 and np.all(np.diff(carry.astype(int)) > 0) and len(carry) == s["n"] < prev["n"]
        assert np.array_equal(carry, np.flatnonzero(prev["want"]["code"]))
        assert np.array_equal(_bits(s["px"]), _bits(prev["want"]["px"][carry])) and np.array_equal(s["is3d"], prev["is3d"][carry])
        assert np.array_equal(_bits(s["wpt"]), _bits(prev["wpt"][carry]))
        w = s["want"]
        assert s["n"] >= 50 and 0 < (w["code"] == 0).sum() < s["n"] and w["n_pose"] >= 20
    assert [s["frames"] for s in (a, b, c, d)] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert all(np.array_equal(d[k], a[k]) for k in ("px", "is3d", "wpt")) and 0 < (d["want"]["code"] != 0).sum() < 200


def test_grown_carry():
    a, b = T.grown_carry()
    assert a is T.case("size_2049") and a["n"] > 2048 > T.case("mixed_200")["n"]      # past the blocks a 200-slot step reserved
    carry = b["carry"]
    assert carry.dtype == np.uint16 and np.array_equal(carry, np.flatnonzero(a["want"]["code"])) and 1024 < b["n"] == len(carry) < a["n"]
    assert np.array_equal(_bits(b["px"]), _bits(a["want"]["px"][carry])) and np.array_equal(b["is3d"], a["is3d"][carry])
    assert np.array_equal(_bits(b["wpt"]), _bits(a["wpt"][carry])) and b["frames"] == (1, 2)
    w = b["want"]
    assert 0 < (w["code"] == 0).sum() < b["n"] and w["n_pose"] >= 20


def test_block_layouts_equal_their_restatement(tmp_path):
    """the three blocks of the fused tracking step (csrc/track_step.hpp: device, pinned, host-written) against the literal arithmetic they
    replaced, for every capacity track_reserve can produce and two bases: offsets, sizes, disjoint fields inside the block, room for the
    carry index, the completion words inside the 256-byte header and 8-byte aligned, 16-byte alignment from d_is3d on, the two tables
    track_in_bytes apart (tests/cpp/track_layout.cpp)"""
    import re
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    src = (root / "alvaar_amd" / "csrc" / "track_slots.hpp").read_text()
    early, done = re.search(r"constexpr int TRK_HDR_EARLY = (\d+), TRK_HDR_DONE = (\d+);", src).groups()
    exe = tmp_path / "track_layout"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), str(root / "tests" / "cpp" / "track_layout.cpp")])
    out = subprocess.check_output([str(exe), early, done], text=True)
    checks, word, fails, _ = out.split()
    assert word == "checks" and int(fails) == 0 and int(checks) > 65535 * 2 * 100, out


def test_pose_layouts_equal_their_restatement(tmp_path):
    """the pose solve's blocks (csrc/pose_layout.hpp: P3P scratch with and without masks, PnP scratch bare / session / batch, the pinned
    pose block behind samples and behind PoseGo, P3P's own pinned block with and without the probe's tail) against the literal arithmetic
    they replaced, for every n up to ALVA_P3P_MAX_N and every H up to 2200: offsets, sizes, disjoint fields inside the block, the record
    slots' lines; the draw schedule against its literal expressions and the angular threshold bit for bit (tests/cpp/pose_layout.cpp)"""
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "pose_layout"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), str(root / "tests" / "cpp" / "pose_layout.cpp")])
    out = subprocess.check_output([str(exe)], text=True)
    checks, word, fails, _ = out.split()
    assert word == "checks" and int(fails) == 0 and int(checks) > (19001 + 2200) * 16 * 4 * 10, out


@pytest.mark.parametrize("name", ["mixed_200", "req_32_of_100", "size_257"])
def test_no_prior_equals_all_slots_2d(name):
    """the restatement against itself: use_prior = 0 is the restatement with every slot marked 2-D, except for n_pose and the
    correspondences"""
    c = T.case(name)
    _, gray = T.frames()
    g0, g1 = gray[c["frames"][0]], gray[c["frames"][1]]
    a = T.restate(g0, g1, c["px"], c["is3d"], c["wpt"], use_prior=0)
    b = T.restate(g0, g1, c["px"], np.zeros_like(c["is3d"]), c["wpt"], use_prior=1)
    for k in ("code", "px", "unpx", "bv"):
        assert np.array_equal(_bits(a[k]) if a[k].dtype != np.uint8 else a[k], _bits(b[k]) if b[k].dtype != np.uint8 else b[k]), k
    assert a["p3p_req"] == b["p3p_req"] == 0 and b["n_pose"] == 0 and a["n_pose"] == ((c["is3d"] != 0) & (a["code"] != 0)).sum()
