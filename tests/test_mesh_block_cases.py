"""CPU: the numpy restatement of the block meshes (tests/mesh_block_cases.py).  Union: over every block size and lattice the blocks'
vertices and normals are the whole-volume extraction's (tests/mesh_cases.py) byte for byte, their triangles are its triangles, each
once and in its order within a block.  Digest: one voxel's q changes exactly the blocks whose box holds it, a weight among valid
weights changes none, crossing min_weight does, an unseen block has digest 0.  Shift: a block whose box lies in both cubes keeps its
digest, counts and -- with a dyadic origin and voxel -- its bytes.  List: csrc/slam/mesh_blocks.hpp, through the stand-alone
tests/cpp/mesh_blocks_host.cpp, answers a scripted session exactly as the restated G2 - G6."""
import copy
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_block_cases as Bc
import mesh_cases as Mc
import mesh_shift_cases as Sc

ROOT = Path(__file__).resolve().parent.parent
BIG = 1 << 22


@functools.lru_cache(maxsize=None)
def volume(name):
    """(q, w, origin3, voxel, min_weight), read-only"""
    if name == "sphere":
        q, w, o, vx = Mc.sampled(17, Mc.sphere_dist(Mc.SPHERE_C, Mc.SPHERE_R))
        out = (q, w, o, vx, 1)
    elif name == "wall_and_box":
        r = Mc.e2e_run()
        out = (r["q"], r["w"], r["origin3"], r["voxel"], 2)
    elif name == "hashed":
        q, w = Mc.hashed_volume(12, 41, -3000, 3000, 4)
        out = (q, w, np.array([0.3, -0.2, 0.1]), 0.07, 2)
    else:
        c = Mc.scan_case()
        out = (c["q"], c["w"], c["origin3"], c["voxel"], 1)
    for a in out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def whole(name):
    q, w, o, vx, mw = volume(name)
    return Mc.extract(q, w, o, vx, mw, BIG, BIG)


@pytest.mark.parametrize("lattice", Bc.LATTICES, ids=lambda l: "L%d_%d_%d" % l)
@pytest.mark.parametrize("B", Bc.BLOCKS)
@pytest.mark.parametrize("name", ["sphere", "wall_and_box", "hashed", "scan"])
def test_union(name, B, lattice):
    q, w, o, vx, mw = volume(name)
    N = q.shape[0]
    ref = whole(name)
    assert ref["info"][0] == 0
    keys = Bc.block_keys(N, lattice, B)
    assert np.array_equal(Bc.key_order(keys), np.arange(len(keys)))   # L1: the enumeration is ascending
    got = Bc.extract_blocks(q, w, o, vx, lattice, mw, B, keys, BIG, BIG)
    digest, counts, nb3 = Bc.digest_counts(q, w, lattice, mw, B)
    assert int(nb3.prod()) == len(keys) and len(set(digest[counts[:, 1] > 0].tolist())) == int((counts[:, 1] > 0).sum())
    cell_id = {tuple(c): n for n, c in enumerate(ref["cells"].tolist())}
    tri_at = {tuple(t): n for n, t in enumerate(ref["triangles"].tolist())}
    assert len(tri_at) == len(ref["triangles"])
    seen_cells, seen_tris = set(), []
    for n, (blk, key) in enumerate(zip(got["blocks"], keys)):
        assert (blk["nv"], blk["nq"]) == tuple(counts[n]) and blk["digest"] == digest[n]
        v0, nv, t0, nt = got["ranges"][n]
        assert nv == blk["nv"] and nt == 2 * blk["nq"]
        cells = got["cells"][v0:v0 + nv]
        # L2: the extended range, in ascending cell index
        d = cells + np.asarray(lattice) - B * key
        assert np.all(d >= -1) and np.all(d <= B - 1)
        lin = (cells[:, 2] * N + cells[:, 1]) * N + cells[:, 0]
        assert np.all(np.diff(lin) > 0)
        ids = np.array([cell_id[tuple(c)] for c in cells.tolist()], np.int64)   # (a KeyError: a vertex the whole mesh does not have)
        assert got["vertices"][v0:v0 + nv].tobytes() == ref["vertices"][ids].tobytes()
        assert got["normals"][v0:v0 + nv].tobytes() == ref["normals"][ids].tobytes()
        seen_cells.update(ids.tolist())
        tris = got["triangles"][t0:t0 + nt]
        assert nt == 0 or (tris.min() >= 0 and tris.max() < nv)
        at = [tri_at[tuple(t)] for t in ids[tris].tolist()] if nt else []
        assert at == sorted(at)   # X6's order within the block
        seen_tris += at
        # the quads are the block's own voxels'
        dq = blk["quad_voxels"][:, :3] + np.asarray(lattice) - B * key
        assert np.all(dq >= 0) and np.all(dq <= B - 1)
    assert seen_cells == set(range(len(ref["cells"])))
    assert sorted(seen_tris) == list(range(len(ref["triangles"])))   # each once
    assert 2 * int(counts[:, 1].sum()) == len(ref["triangles"]) and got["info"][2] == len(ref["triangles"])


# ---------------------------------------------------------------------------------------------------- the digest
DIG_N, DIG_B, DIG_LAT, DIG_MW = 20, 8, (5, -13, 40), 2


@functools.lru_cache(maxsize=None)
def digest_volume():
    q, w = Mc.hashed_volume(DIG_N, 61, -3000, 3000, 3)
    return q, w


def _local_at(axis, where):
    """a local index on `axis` whose d is 0 (first), B - 1 (last) or 3 (interior), away from the cube's faces"""
    want = {"first": 0, "last": DIG_B - 1, "interior": 3}[where]
    for i in range(2, DIG_N - 2):
        if (DIG_LAT[axis] + i) % DIG_B == want:   # Python's % is a floor's
            return i
    raise AssertionError


@pytest.mark.parametrize("wz", ["first", "last", "interior"])
@pytest.mark.parametrize("wy", ["first", "last", "interior"])
@pytest.mark.parametrize("wx", ["first", "last", "interior"])
def test_digest_one_voxel(wx, wy, wz):
    q, w = [a.copy() for a in digest_volume()]
    i, j, k = _local_at(0, wx), _local_at(1, wy), _local_at(2, wz)
    w[k, j, i] = 3
    base = Bc.digest_counts(q, w, DIG_LAT, DIG_MW, DIG_B)[0]
    keys = Bc.block_keys(DIG_N, DIG_LAT, DIG_B)
    g = np.array(DIG_LAT) + (i, j, k)
    d = g[None, :] - DIG_B * keys
    holds = np.all((d >= -1) & (d <= DIG_B), 1)
    assert holds.sum() == 2 ** sum(x != "interior" for x in (wx, wy, wz))   # 1 to 8 blocks
    q2 = q.copy()
    q2[k, j, i] += 1
    assert np.array_equal(Bc.digest_counts(q2, w, DIG_LAT, DIG_MW, DIG_B)[0] != base, holds)
    for other in (2, 255):   # a weight among the valid ones
        w2 = w.copy()
        w2[k, j, i] = other
        assert np.array_equal(Bc.digest_counts(q, w2, DIG_LAT, DIG_MW, DIG_B)[0], base)
    w2 = w.copy()
    w2[k, j, i] = DIG_MW - 1   # across min_weight
    assert np.array_equal(Bc.digest_counts(q, w2, DIG_LAT, DIG_MW, DIG_B)[0] != base, holds)


def test_digest_of_an_unseen_block_is_zero():
    q, w = [a.copy() for a in digest_volume()]
    keys = Bc.block_keys(DIG_N, DIG_LAT, DIG_B)
    n = len(keys) // 2
    l0 = DIG_B * keys[n] - np.array(DIG_LAT) - 1
    lo, hi = np.maximum(l0, 0), np.minimum(l0 + DIG_B + 2, DIG_N)
    w[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = DIG_MW - 1
    digest, counts, _ = Bc.digest_counts(q, w, DIG_LAT, DIG_MW, DIG_B)
    assert digest[n] == 0 and tuple(counts[n]) == (0, 0) and np.count_nonzero(digest) >= len(keys) - 1 - 26
    q0, w0 = Mc.empty_volume(9)
    digest, counts, _ = Bc.digest_counts(q0, w0, (-1, 0, 7), 1, 8)
    assert not digest.any() and not counts.any()


def test_splitmix_known_values():
    """the finaliser is splitmix64's: the first outputs of the generator seeded with 0 (Vigna's reference implementation)"""
    x = np.array([0, 0x9E3779B97F4A7C15], np.uint64)
    assert Bc.splitmix(x).tolist() == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]


# ---------------------------------------------------------------------------------------------------- shift invariance
@pytest.mark.parametrize("s", [(8, 0, 0), (-16, 8, 0), (3, 0, -5)], ids=lambda s: "s%d_%d_%d" % s)
@pytest.mark.parametrize("B", [8, 16])
def test_shift_invariance(B, s):
    q, w, origin, voxel = Mc.sampled(32, Mc.sphere_dist(Mc.SPHERE_C, Mc.SPHERE_R))
    assert voxel == 2.0 ** -4 and np.all(origin == -1.0)   # dyadic: o + s voxel and X3's arithmetic are exact
    N = 32
    q2, w2, _, _ = Sc.shift(q, w, None, s)
    origin2 = origin + np.asarray(s, np.float64) * voxel
    both, surfaces = 0, 0
    for lattice in ((0, 0, 0), (5, -13, 40), (-9, -9, -9)):
        lattice2 = tuple(int(a + b) for a, b in zip(lattice, s))   # the destination's voxel 0 is the source's voxel s
        keys2 = Bc.block_keys(N, lattice2, B)
        for key in Bc.block_keys(N, lattice, B):
            l1 = B * key - np.asarray(lattice) - 1
            l2 = B * key - np.asarray(lattice2) - 1
            if not (np.all(l1 >= 0) and np.all(l1 + B + 1 < N) and np.all(l2 >= 0) and np.all(l2 + B + 1 < N)):
                continue   # the box does not lie in both cubes
            assert np.any(np.all(keys2 == key, 1))
            a = Bc.block_mesh(q, w, origin, voxel, lattice, 1, B, key)
            b = Bc.block_mesh(q2, w2, origin2, voxel, lattice2, 1, B, key)
            assert a["digest"] == b["digest"] and (a["nv"], a["nq"]) == (b["nv"], b["nq"])
            for f in ("vertices", "normals", "triangles"):
                assert a[f].tobytes() == b[f].tobytes()
            both += 1
            surfaces += a["nq"] > 0
    if B == 8:   # (a box of 18 voxels need not fit the overlap of two cubes of 32)
        assert both >= 1 and surfaces >= 1


# ---------------------------------------------------------------------------------------------------- the selection
def test_selection_rules():
    q, w, o, vx, mw = volume("sphere")
    keys = Bc.block_keys(17, (3, 3, 3), 8)
    assert Bc.extract_blocks(q, w, o, vx, (3, 3, 3), mw, 8, keys[:0], 10, 10)["info"].tolist() == [1, 0, 0, 0, 0, 17, 8, 0]
    for bad in (keys[[1, 0]], keys[[2, 2]], keys[[0]] - 1, keys[[-1]] + (1, 0, 0)):
        with pytest.raises(Bc.Refused):
            Bc.extract_blocks(q, w, o, vx, (3, 3, 3), mw, 8, bad, BIG, BIG)
    full = Bc.extract_blocks(q, w, o, vx, (3, 3, 3), mw, 8, keys, BIG, BIG)
    nv, nt = int(full["info"][1]), int(full["info"][2])
    assert Bc.extract_blocks(q, w, o, vx, (3, 3, 3), mw, 8, keys, nv, nt)["info"][0] == 0
    for caps in ((nv - 1, nt), (nv, nt - 1)):
        over = Bc.extract_blocks(q, w, o, vx, (3, 3, 3), mw, 8, keys, *caps)
        assert over["info"][:3].tolist() == [3, nv, nt] and len(over["vertices"]) == 0 and not over["ranges"].any()


# ---------------------------------------------------------------------------------------------------- the list
def _script_call(lines, gen, mw, B, all_, caps, N, lattice, digest, counts):
    lines.append("call %d %d %d %d %d %d %d %d %d %d %d %d" % (gen, mw, B, int(all_), *caps, N, *lattice, len(digest)))
    lines += ["%d %d %d" % (int(d), c[0], c[1]) for d, c in zip(digest, counts)]


def _parse(out):
    """the program's output -> [(info, reports)]"""
    calls = []
    for line in out.strip().splitlines():
        f = line.split()
        if f[0] == "info":
            calls.append(([int(v) for v in f[1:]], []))
        else:
            v = [int(x) for x in f]
            calls[-1][1].append(((v[0], v[1], v[2]), *v[3:]))
    return calls


def test_block_list_follows_the_restated_rule(tmp_path):
    exe = tmp_path / "mesh_blocks_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(ROOT / "tests" / "cpp" / "mesh_blocks_host.cpp")])
    r = Mc.e2e_run()
    q, w = r["q"].copy(), r["w"].copy()
    N, B, mw, room = 32, 8, 2, (4096, BIG, BIG)
    lattice = (0, 0, 0)
    L, lines, want, notes = Bc.BlockList(), [], [], []

    def call(gen, mw_, all_, caps, note):
        digest, counts, _ = Bc.digest_counts(q, w, lattice, mw_, B)
        _script_call(lines, gen, mw_, B, all_, caps, N, lattice, digest, counts)
        want.append(L.call(gen, mw_, B, all_, *caps, N, lattice, digest, counts))
        notes.append(note)
        return want[-1]

    info, rep = call(7, mw, False, room, "first")
    n_present = info[6]
    assert info[0] == 0 and info[5] == 1 and n_present > 8 and [s[1] for s in rep] == [1] * n_present
    assert [s[0] for s in rep] == sorted((s[0] for s in rep), key=lambda k: k[::-1])
    info, rep = call(7, mw, False, room, "unchanged")
    assert info[:5] == [0, 0, 0, 0, 0] and info[5] == 1 and rep == []
    info, rep = call(7, mw, True, room, "unchanged, ALL")
    assert info[1] == n_present and {s[1] for s in rep} == {0}
    # one voxel of the surface band, in the interior of a block: one block changes
    k0, j0, i0 = [int(v[0]) for v in np.nonzero((w >= mw) & (np.abs(q.astype(int)) < 20000) & (np.indices(q.shape) % B == 3).all(0))]
    q[k0, j0, i0] += 1
    info, rep = call(7, mw, False, room, "one voxel")
    assert [(s[0], s[1]) for s in rep] == [((i0 // B, j0 // B, k0 // B), 2)]
    # a shift by two blocks: what leaves the cube is state 4, what stays inside the cube's interior is not reported
    before = dict(L.table)
    q, w, _, _ = Sc.shift(q, w, None, (16, 0, 0))
    lattice = (16, 0, 0)
    info, rep = call(7, mw, False, room, "shift")
    left = sorted((k for k in before if k[0] < 2), key=lambda k: k[::-1])
    assert [s[0] for s in rep if s[1] == 4] == left and len(left) > 0 and info[4] == len(left)
    assert all(s[0][0] == 2 and s[1] in (2, 3) for s in rep if s[1] != 4)   # the blocks now at the cube's face; x = 3 keeps its boxes
    # carve a block's surface away: everything in its box in front of the surface
    victim = next(s[0] for s in call(7, mw, True, room, "ALL after the shift")[1] if s[0][0] == 3)
    lo = B * np.array(victim) - np.array(lattice) - 1
    q = q.copy()
    q[max(lo[2], 0):lo[2] + B + 2, max(lo[1], 0):lo[1] + B + 2, max(lo[0], 0):lo[0] + B + 2] = 32767
    info, rep = call(7, mw, False, room, "carved")
    assert (victim, 3) in [(s[0], s[1]) for s in rep] and info[4] >= 1
    # over a cap, then with room: the answer a single call gives
    q[lo[2] + 2, lo[1] + 2, lo[0] + 2] = -5
    w[lo[2] + 2, lo[1] + 2, lo[0] + 2] = 200
    twin = copy.deepcopy(L)
    digest, counts, _ = Bc.digest_counts(q, w, lattice, mw, B)
    single = twin.call(7, mw, B, True, *room, N, lattice, digest, counts)
    n_rep, nv, nt = single[0][1:4]
    for caps in ((n_rep - 1, BIG, BIG), (4096, nv - 1, BIG), (4096, BIG, nt - 1)):
        info, rep = call(7, mw, True, caps, "over a cap")
        assert info == [3, n_rep, nv, nt] + single[0][4:] and rep == []
    assert call(7, mw, True, (n_rep, nv, nt), "exact caps") == single
    # another min_weight: the epoch moves and everything is new
    epoch = L.epoch
    info, rep = call(7, mw + 1, False, room, "min_weight")
    assert info[5] == epoch + 1 and info[1] == info[6] > 0 and {s[1] for s in rep} == {1}
    assert call(7, mw + 1, False, room, "unchanged")[0][1] == 0
    # the volume's generation moves on (emptied, placed or replaced)
    info, rep = call(8, mw + 1, False, room, "generation")
    assert info[5] == epoch + 2 and {s[1] for s in rep} == {1}
    # a reset
    L.reset()
    lines.append("reset")
    info, rep = call(8, mw + 1, False, room, "reset")
    assert info[5] == epoch + 3 and {s[1] for s in rep} == {1} and info[4] == 0
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = _parse(out.stdout)
    assert len(got) == len(want)
    for g, x, note in zip(got, want, notes):
        assert g[0] == x[0] and g[1] == x[1], note


# ---------------------------------------------------------------------------------------------------- the public surface
NAMES = ("alva_mesh_block_digest", "alva_mesh_extract_blocks", "alva_system_mesh_blocks", "alva_system_reset_mesh_blocks")


def test_headers_declare_the_calls():
    hip = (ROOT / "include" / "alvaar_hip.h").read_text()
    sysh = (ROOT / "include" / "alvaar_system.h").read_text()
    for name in NAMES[:2]:
        assert re.search(r"\bint\s+%s\s*\(\s*alva_ctx\s*\*" % name, hip), name
    for name in NAMES[2:]:
        assert re.search(r"\bint\s+%s\s*\(\s*alva_system\s*\*" % name, sysh), name
    for tag in ("L1 lattice", "L2 ownership", "L3 digest", "L4 counts"):
        assert tag in hip
    for tag in ("G1 volume", "G2 table", "G3 digests", "G4 states", "G5 caps", "G6 meshes", "#define ALVA_MESH_BLOCKS_ALL 1"):
        assert tag in sysh


def test_system_class_methods_compile(tmp_path):
    src = r'''
#include "alvaar_system.h"
int use(alva::System &s, int *keys, int *binfo, float *v, float *n, uint8_t *c, int *t, int *lattice, int *info, double *geo) {
    int (alva::System::*blocks)(int, int, bool, int, int, int, int *, int *, float *, float *, uint8_t *, int *, int *, int *, double *) =
        &alva::System::meshBlocks;
    int (alva::System::*forget)() = &alva::System::resetMeshBlocks;
    (void) blocks; (void) forget;
    return s.meshBlocks(2, 16, false, 64, 1000, 2000, keys, binfo, v, n, c, t, lattice, info, geo) + s.resetMeshBlocks();
}
'''
    f = tmp_path / "t.cpp"
    f.write_text(src)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-fsyntax-only", str(f)])


def test_library_exports_the_calls():
    import ctypes
    lib = ctypes.CDLL(str(ROOT / "alvaar_amd" / "libalvaar_hip.so"))
    assert all(hasattr(lib, name) for name in NAMES)
