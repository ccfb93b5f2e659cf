"""The restatement of image detection's device stages (tests/image_cases.py) checked on its own, without a GPU: that it computes what the
definition in include/alvaar_hip.h says, at every rule, and that the chain it defines finds a picture in rendered frames."""
from __future__ import annotations

import numpy as np
import pytest

import image_cases as IC

LAUNCHES = {L["name"]: L for L in IC.launches()}
MATCHES = {L["name"]: L for L in IC.match_launches()}


# ---- stage 2

def _scalar_solve(p, q, idx):
    """the model step written out for ONE hypothesis with plain Python floats, independently of the side-by-side form"""
    a = []
    for i in idx:
        x, y, u, v = (float(c) for c in (p[i, 0], p[i, 1], q[i, 0], q[i, 1]))
        a.append([x, y, 1.0, 0.0, 0.0, 0.0, -(x * u), -(y * u), u])
        a.append([0.0, 0.0, 0.0, x, y, 1.0, -(x * v), -(y * v), v])
    for k in range(8):
        piv = k
        for r in range(k + 1, 8):
            if abs(a[r][k]) > abs(a[piv][k]):
                piv = r
        if not abs(a[piv][k]) > 1e-12:
            return None
        a[k], a[piv] = a[piv], a[k]
        for r in range(k + 1, 8):
            f = a[r][k] / a[k][k]
            for c in range(k + 1, 9):
                a[r][c] = a[r][c] - f * a[k][c]
    h = [0.0] * 8
    for k in range(7, -1, -1):
        acc = a[k][8]
        for c in range(k + 1, 8):
            acc = acc - a[k][c] * h[c]
        h[k] = acc / a[k][k]
    return h


def test_the_side_by_side_solver_equals_the_scalar_one_bit_for_bit_also_on_pivot_ties():
    rng = np.random.default_rng(0)
    xy = IC.planted_scene(40, 0.5, 3, noise_px=0.5)[0]
    # pivot ties: pairs on a square grid share |x| and |y|, so several rows of a column hold the same magnitude
    grid = np.array([[64.0 * i, 48.0 * j, 300 + 50.0 * i + 3 * j, 200 + 40.0 * j - 2 * i] for i in range(5) for j in range(5)])
    for pairs, wh in ((xy, IC.WH), (grid, (256, 192))):
        p, q, _ = IC.normalise(pairs, wh, IC.FRAME)
        idx = np.array([rng.permutation(len(pairs))[:4] for _ in range(200)])
        h, ok = IC.solve_models(p, q, idx)
        for k, row in enumerate(idx):
            want = _scalar_solve(p, q, row)
            assert (want is not None) == bool(ok[k])
            if want is not None:
                assert np.array(want).tobytes() == h[k].tobytes(), k
    assert not ok.all() and ok.any()   # (the grid has collinear triples: both branches ran)


@pytest.mark.parametrize("m", [4, 5, 64, 512])
def test_an_exact_homography_is_recovered_with_every_pair_counted(m):
    xy, R, t, _ = IC.planted_scene(m, 0.0, 10 + m)
    out = IC.homography_oracle(xy, IC.WH, IC.FRAME, IC.CALIB, 64, 3.0, 4)
    assert out["info"][:4].tolist() == [0, m, int(np.argmax(out["counts"])), m]
    assert out["mask"][:m].all() and not out["mask"][m:].any()
    assert (out["counts"][out["counts"] >= 0] == m).all()
    Hm = IC.homography_of_pose(R, t, IC.FRAME, IC.CALIB)
    assert np.abs(out["H"].reshape(3, 3) - Hm).max() < 1e-9


def test_the_pose_of_an_analytic_homography_is_exact():
    rng = np.random.default_rng(1)
    for frame, calib in ((IC.FRAME, IC.CALIB), ((1280, 720), (900.0, 905.0, 650.5, 351.25))):
        for _ in range(20):
            R = IC.rot_xyz(*rng.uniform(-0.6, 0.6, 3))
            t = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), rng.uniform(0.8, 5.0)])
            Hm = IC.homography_of_pose(R, t, frame, calib)
            code, R2, t2 = IC.pose_from_h(Hm.reshape(-1)[:8], max(frame) / 2, frame, calib)
            assert code == 0
            assert np.abs(R2 - R).max() < 1e-12 and np.abs(t2 - t).max() < 1e-12 * max(1.0, np.abs(t).max())
            assert np.linalg.det(R2) > 0.999999   # right-handed


def test_the_threshold_is_inclusive_where_the_error_is_exact():
    launch = LAUNCHES["threshold-edge"]
    xy, expect = IC.integer_translation_pairs()
    out = IC.run_launch(launch)[0]
    assert out["H"].tolist() == [1.0, 0.0, (40 + 128 - 256) / 256, 0.0, 1.0, (24 + 128 - 256) / 256, 0.0, 0.0, 1.0]
    assert out["mask"][:len(xy)].tolist() == expect.tolist()   # 9 <= 9 and 8 <= 9 in, 10 out
    assert out["info"].tolist() == [0, 12, 0, 11, 0, 0, 0, 0]
    # a hair under 3 px: the pairs at exactly 3 px fall out, the one at sqrt(8) stays
    tight = IC.homography_oracle(xy, (256, 256), launch["frame"], launch["calib"], 1, np.nextafter(np.float32(3), np.float32(0)), 4,
                                 rand4=launch["rand4"])
    assert tight["info"][3] == 9 and tight["mask"][4:8].tolist() == [0, 0, 0, 1]


def test_every_skip_rule_and_the_tie_rule():
    launch = LAUNCHES["skips-and-tie"]
    out = IC.run_launch(launch)[0]
    # iterations 0..5 repeat an index (every position pair), 6 draws three collinear pairs (a pivot fails), 7 the bow-tie (sign rule)
    assert out["counts"][:8].tolist() == [-1] * 8
    xy, wh = launch["images"][0]
    p, q, _ = IC.normalise(xy, wh, launch["frame"])
    h, ok = IC.solve_models(p, q, np.array([[4, 5, 6, 12], [0, 1, 2, 3]]))
    assert ok.tolist() == [False, True]   # the collinear sample dies in the solve, the bow-tie only at the sign rule
    assert (IC.weights(h[1:], p[:4, 0], p[:4, 1]) <= 0).any()
    # 8 and 9 draw the same clean model through other pairs: equal counts, the lower iteration wins
    assert out["counts"][8] == out["counts"][9] and out["info"][2] == 8 and out["info"][0] == 0
    assert IC.run_launch(LAUNCHES["all-skipped"])[0]["info"].tolist() == [2, 24, -1, 0, 0, 0, 0, 0]


def test_the_sample_stream_is_the_hit_tests_hash_with_four_words():
    import hit_cases
    assert IC.hash32(123456789) == hit_cases.hash32(123456789)
    w = IC.sample_words(12345, 3)
    assert w[2, 1] == IC.hash32(12345 ^ ((9 * 0x9E3779B9) & 0xFFFFFFFF))
    assert IC.words_for([[0, 5, 11, 3]], 12).dtype == np.uint32
    assert ((IC.words_for([[0, 5, 11, 3]], 12).astype(np.uint64) * 12) >> 32).tolist() == [[0, 5, 11, 3]]


def test_every_code_and_every_expectation_of_the_launches():
    seen = set()
    for launch in LAUNCHES.values():
        outs = IC.run_launch(launch)
        for j, o in enumerate(outs):
            seen.add(int(o["info"][0]))
            if launch["expect"] is not None and launch["expect"][j] is not None:
                assert o["info"][0] == launch["expect"][j], (launch["name"], j)
            if o["info"][0] != 0:
                assert not o["R"].any() and not o["t"].any()
            if o["info"][0] in (1, 2):
                assert not o["H"].any() and not o["mask"].any() and o["info"][2] == -1
            else:
                assert o["mask"].sum() == o["info"][3]
    assert seen == {0, 1, 2, 3, 4}


def test_the_planted_model_wins_against_70_percent_clutter():
    launch = LAUNCHES["outliers-70"]
    xy, R, t, good = IC.planted_scene(300, 0.7, 21, noise_px=0.3)
    out = IC.run_launch(launch)[0]
    mask = out["mask"][:300].astype(bool)
    assert out["info"][0] == 0 and (mask & good).sum() >= 0.9 * good.sum() and (mask & ~good).sum() <= 3
    # the minimal-sample pose is rough (four noisy pairs); it is the refinement's starting point, not the answer
    ang = np.degrees(np.arccos(np.clip((np.trace(out["R"].reshape(3, 3).T @ R) - 1) / 2, -1, 1)))
    assert ang < 20 and np.linalg.norm(out["t"] - t) < 0.2 * np.linalg.norm(t)


# ---- stage 1

def test_the_match_rules_at_their_edges():
    for name in ("edge-max-dist", "edge-ratio", "edge-train-tie", "edge-claims"):
        launch = MATCHES[name]
        match, xy = IC.run_match_launch(launch)[0]
        got = {int(q): int(t) for q, t, _ in match}
        assert got == {q: t for q, t in launch["expect"].items() if t is not None}, name
        assert (np.diff(match[:, 0]) > 0).all() and len(set(match[:, 1])) == len(match)   # ascending queries, one-to-one
        qdesc, qxy = launch["images"][0]
        for i, (qi, ti, d) in enumerate(match):
            assert d == IC.hamming(qdesc[qi:qi + 1], launch["tdesc"][ti:ti + 1])[0, 0]
            assert xy[i].tolist() == [float(qxy[qi, 0]), float(qxy[qi, 1]), float(launch["txy"][ti, 0]), float(launch["txy"][ti, 1])]
    # one train row: second = 257, every close query is accepted and the closest one keeps the row
    launch = MATCHES["train-1-1"]
    match, _ = IC.run_match_launch(launch)[0]
    d = IC.hamming(launch["images"][0][0], launch["tdesc"])[:, 0]
    assert len(match) == 1 and match[0, 2] == d.min() and match[0, 0] == int(np.argmin(d))
    # the device count is clamped to the block
    assert len(IC.run_match_launch(MATCHES["train-64--3"])[0][0]) == 0
    a = IC.run_match_launch(MATCHES["train-100-150"])[0][0]
    assert len(a) and a[:, 1].max() < 100


def test_the_match_does_not_depend_on_how_it_is_computed():
    """a second, brute-force formulation of the same rules (sorting instead of argmin / delete)"""
    launch = MATCHES["eight"]
    for (qdesc, qxy), (match, _) in zip(launch["images"], IC.run_match_launch(launch)):
        kept = {}
        if len(qdesc):
            D = IC.hamming(qdesc, launch["tdesc"][:launch["n_train"]])
            for q in range(len(qdesc)):
                order = np.lexsort((np.arange(D.shape[1]), D[q]))
                best, second = D[q, order[0]], D[q, order[1]]
                if best <= launch["max_dist"] and np.float32(best) < np.float32(launch["ratio"]) * np.float32(second):
                    row = int(order[0])
                    if row not in kept or (best, q) < kept[row]:
                        kept[row] = (int(best), q)
        want = sorted((q, row, d) for row, (d, q) in kept.items())
        assert [tuple(r) for r in match.tolist()] == want


# ---- the chain on rendered frames: ORB (the oracle's) -> match -> homography -> a least-squares refit standing in for the refinement

@pytest.fixture(scope="module")
def chain():
    rows = IC.chain_rows()
    for row in rows:
        print(row)
    return rows


def test_the_chain_finds_the_crop_in_every_frame(chain):
    """Recorded: see the printed rows.  The bounds are not fitted to them: min_inliers = 20 is the issue's; inliers lie within 3 px of a
    picture that spans about 250 px in the frame, so the in-plane angle and the scale (= the distance) are held to 3 / 125 = 2.4 %, and
    the tilt, which shows only through foreshortening, to acos(1 - 3 / 250) = 8.9 degrees."""
    for row in chain:
        r = row["crop"]
        assert r["pairs"] >= 20 and r["code"] == 0 and r["count"] >= 20, row
        assert r["refit"] is not None and r["refit"][0] < 8.9 and r["refit"][1] < 0.024, row


def test_the_distractor_stays_below_min_inliers_in_every_frame(chain):
    for row in chain:
        r = row["distractor"]
        assert r["code"] in (1, 2, 3) and r["count"] < 20, row
