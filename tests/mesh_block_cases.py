"""The scene mesh in blocks (include/alvaar_hip.h: alva_mesh_block_digest / alva_mesh_extract_blocks, L1-L4) and the session's list
(include/alvaar_system.h: alva_system_mesh_blocks, G1-G6) restated in numpy / plain Python.  The reference has no scene mesh, so this
file is what the two stages and the rule are pinned to: tests/test_mesh_block_cases.py checks the restatement against the whole-volume
extraction (tests/mesh_cases.py), its own properties and the host list (csrc/slam/mesh_blocks.hpp); tests/test_gpu_mesh_blocks.py the
kernels against it, byte for byte.

A block is restated on its own box of (B + 2)^3 voxels, cut out of the volume with everything outside the cube invalid: that a block's
mesh is a function of that box alone (L3) is thereby part of the restatement, and that the blocks together are the whole mesh is what
the union test shows."""
from __future__ import annotations

import numpy as np

import mesh_cases as Mc

F32 = np.float32
U64 = np.uint64
BLOCKS = (8, 16, 32)
LATTICES = ((0, 0, 0), (3, 3, 3), (-1, -1, -1), (-8, -8, -8), (-9, -9, -9), (5, -13, 40))


# ---------------------------------------------------------------------------------------------------- L1
def grid(N, lattice3, B):
    """(bmin [3], nb [3]): the lowest key and the number of blocks per axis (numpy's // is a floor)"""
    lat = np.asarray(lattice3, np.int64).reshape(3)
    bmin = lat // B
    return bmin, (lat + N - 1) // B - bmin + 1


def block_keys(N, lattice3, B):
    """the grid's keys [nb,3] = (b_x, b_y, b_z) in ascending (b_z, b_y, b_x)"""
    bmin, nb = grid(N, lattice3, B)
    z, y, x = np.meshgrid(np.arange(nb[2]), np.arange(nb[1]), np.arange(nb[0]), indexing="ij")
    return np.stack([bmin[0] + x.reshape(-1), bmin[1] + y.reshape(-1), bmin[2] + z.reshape(-1)], 1)


def key_order(keys):
    """the rank of keys [n,3] in ascending (z, y, x)"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    return np.lexsort((keys[:, 0], keys[:, 1], keys[:, 2]))


# ---------------------------------------------------------------------------------------------------- L3
def splitmix(x):
    """the splitmix64 finaliser on uint64 arrays (the products wrap mod 2^64)"""
    with np.errstate(over="ignore"):
        z = x + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def box_of(q, w, lattice3, min_weight, B, key):
    """the block's box: (valid, inside, q) each [E,E,E] in [z][y][x] with E = B + 2, d = index - 1; l0 = the local index of d = -1 per axis
    (x, y, z).  Voxels outside the cube are invalid"""
    q, w = np.asarray(q, np.int16), np.asarray(w, np.uint8)
    N, E = q.shape[0], B + 2
    lat = np.asarray(lattice3, np.int64).reshape(3)
    l0 = B * np.asarray(key, np.int64).reshape(3) - lat - 1
    ax = [l0[a] + np.arange(E) for a in range(3)]
    ok = [(v >= 0) & (v < N) for v in ax]
    cl = [np.clip(v, 0, N - 1) for v in ax]
    inb = ok[2][:, None, None] & ok[1][None, :, None] & ok[0][None, None, :]
    qb = q[cl[2][:, None, None], cl[1][None, :, None], cl[0][None, None, :]].astype(np.int64)
    wb = w[cl[2][:, None, None], cl[1][None, :, None], cl[0][None, None, :]]
    valid = inb & (wb >= min_weight)   # X1
    return valid, valid & (qb < 0), np.where(valid, qb, 0), l0


def box_digest(valid, qb):
    E = valid.shape[0]
    p = np.arange(E * E * E, dtype=U64).reshape(E, E, E)
    x = (p << U64(17)) | U64(0x10000) | (qb.astype(np.int64) & 0xFFFF).astype(U64)
    with np.errstate(over="ignore"):
        return U64(splitmix(x)[valid].sum(dtype=U64))


# ---------------------------------------------------------------------------------------------------- L2, L4
def block_mesh(q, w, origin3, voxel, lattice3, min_weight, B, key, floats=True):
    """one block: a dict with digest (uint64), nv, nq, and -- with floats -- vertices, normals float32 [nv,3], triangles int32 [2 nq,3]
    (local indices), cells [nv,3] (the LOCAL cell index i, j, k of each vertex) and quad_voxels [nq,4] (i, j, k, a: local)"""
    valid, inside, qb, l0 = box_of(q, w, lattice3, min_weight, B, key)
    N = np.asarray(q).shape[0]
    C = B + 1
    corner = lambda a, c: a[(c >> 2):(c >> 2) + C, ((c >> 1) & 1):((c >> 1) & 1) + C, (c & 1):(c & 1) + C]
    # X2 on the cells d in [-1, B - 1]^3 (a cell that does not exist in the cube has an invalid corner)
    n_in = sum(corner(inside, c).astype(np.int64) for c in range(8))
    active = np.logical_and.reduce([corner(valid, c) for c in range(8)]) & (n_in > 0) & (n_in < 8)
    ck, cj, ci = np.nonzero(active)   # ascending cell index
    nv = len(ci)
    # X6 on the own voxels d in [0, B - 1]^3: box index d + 1, cell index d + 1
    vid = np.full((C, C, C), -1, np.int64)
    vid[ck, cj, ci] = np.arange(nv)
    dz, dy, dx = np.meshgrid(np.arange(B), np.arange(B), np.arange(B), indexing="ij")
    d = [dx.reshape(-1), dy.reshape(-1), dz.reshape(-1)]
    keys, quads, qvox = [], [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3

        def vox(arr, da=0):
            u = [d[0] + 1, d[1] + 1, d[2] + 1]
            u[a] = u[a] + da
            return arr[u[2], u[1], u[0]]

        def cell(arr, db=0, dc=0):
            u = [d[0] + 1, d[1] + 1, d[2] + 1]
            u[b], u[c] = u[b] + db, u[c] + dc
            return arr[u[2], u[1], u[0]]

        # X6's grid conditions on the local index: implied by the invalid outside, restated all the same
        p = [l0[0] + 1 + d[0], l0[1] + 1 + d[1], l0[2] + 1 + d[2]]
        ok = (p[a] >= 0) & (p[a] < N - 1) & (p[b] >= 1) & (p[b] < N - 1) & (p[c] >= 1) & (p[c] < N - 1)
        emit = ok & vox(valid) & vox(valid, 1) & (vox(inside) != vox(inside, 1)) & cell(active, -1, -1) & cell(active, 0, -1) & cell(active) & cell(active, -1, 0)
        Q = np.stack([cell(vid, -1, -1), cell(vid, 0, -1), cell(vid), cell(vid, -1, 0)], 1)[emit]
        ins = vox(inside)[emit]
        keys.append((((d[2] * B + d[1]) * B + d[0]) * 3 + a)[emit])
        quads.append(np.where(ins[:, None], Q[:, [0, 1, 2, 0, 2, 3]], Q[:, [0, 2, 1, 0, 3, 2]]))
        qvox.append(np.stack([p[0][emit], p[1][emit], p[2][emit], np.full(int(emit.sum()), a)], 1))
    keys, quads, qvox = np.concatenate(keys), np.concatenate(quads), np.concatenate(qvox)
    order = np.argsort(keys, kind="stable")
    out = dict(digest=box_digest(valid, qb), nv=nv, nq=len(keys))
    if not floats:
        return out
    # X3, X4 on the LOCAL cell index and the volume's origin
    o = np.asarray(origin3, np.float64).reshape(-1)
    voxel = np.float64(voxel)
    p = [l0[0] + ci, l0[1] + cj, l0[2] + ck]
    qc = [corner(qb, c)[active] for c in range(8)]
    tot, m = [np.zeros(nv, np.int64) for _ in range(3)], np.zeros(nv, np.int64)
    for a in range(3):
        for lo in range(8):
            if lo & (1 << a):
                continue
            hi = lo | (1 << a)
            cross = (qc[lo] < 0) != (qc[hi] < 0)
            qa, qb_ = np.abs(qc[lo]), np.abs(qc[hi])
            D = np.where(cross, qa + qb_, 1)
            f = (2048 * qa + D) // (2 * D)
            for ax in range(3):
                tot[ax] += np.where(cross, 1024 * (p[ax] + ((lo >> ax) & 1)) + (f if ax == a else 0), 0)
            m += cross
    vertices, normals = np.zeros((nv, 3), F32), np.zeros((nv, 3), F32)
    g = [sum(qc[c] if (c >> ax) & 1 else -qc[c] for c in range(8)) for ax in range(3)]
    L2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
    length = np.sqrt(np.maximum(L2, 1).astype(np.float64))
    for ax in range(3):
        X = (tot[ax] + m // 2) // np.maximum(m, 1)
        vertices[:, ax] = (o[ax] + (X.astype(np.float64) / 1024.0 + 0.5) * voxel).astype(F32)
        normals[:, ax] = np.where(L2 == 0, F32(0), (g[ax].astype(np.float64) / length).astype(F32))
    out.update(vertices=vertices, normals=normals, triangles=quads[order].reshape(-1, 3).astype(np.int32), cells=np.stack(p, 1),
               quad_voxels=qvox[order])
    return out


def digest_counts(q, w, lattice3, min_weight, B):
    """alva_mesh_block_digest -> (digest [nb] uint64, counts [nb,2] int32 = (nv, nq), nb3 [3] int32)"""
    N = np.asarray(q).shape[0]
    keys = block_keys(N, lattice3, B)
    digest, counts = np.zeros(len(keys), U64), np.zeros((len(keys), 2), np.int32)
    for n, key in enumerate(keys):
        r = block_mesh(q, w, None, None, lattice3, min_weight, B, key, floats=False)
        digest[n], counts[n] = r["digest"], (r["nv"], r["nq"])
    return digest, counts, grid(N, lattice3, B)[1].astype(np.int32)


class Refused(ValueError):
    """ALVA_ERR_ARG"""


def check_selection(N, lattice3, B, sel_keys):
    sel = np.asarray(sel_keys, np.int64).reshape(-1, 3)
    bmin, nb = grid(N, lattice3, B)
    if np.any(sel < bmin) or np.any(sel >= bmin + nb):
        raise Refused("a key outside the block grid")
    zyx = [tuple(k[::-1]) for k in sel.tolist()]
    if any(not a < b for a, b in zip(zyx, zyx[1:])):
        raise Refused("not strictly ascending in (z, y, x)")
    return sel


def pack_blocks(blocks, N, B, max_vertices, max_triangles):
    """the selected blocks' dicts (block_mesh) packed in selection order: what alva_mesh_extract_blocks hands back"""
    nv, nt = sum(b["nv"] for b in blocks), sum(2 * b["nq"] for b in blocks)
    code = 3 if nv > max_vertices or nt > max_triangles else 1 if nv == 0 else 0
    info = np.array([code, nv, nt, len(blocks), sum(b["nq"] > 0 for b in blocks), N, B, 0], np.int32)
    ranges = np.zeros((len(blocks), 4), np.int32)
    out = dict(vertices=np.zeros((0, 3), F32), normals=np.zeros((0, 3), F32), triangles=np.zeros((0, 3), np.int32), cells=np.zeros((0, 3), np.int64))
    if code != 3:
        v0 = t0 = 0
        for n, b in enumerate(blocks):
            ranges[n] = (v0, b["nv"], t0, 2 * b["nq"])
            v0, t0 = v0 + b["nv"], t0 + 2 * b["nq"]
    if code == 0:
        out = {k: np.concatenate([b[k] for b in blocks]) for k in out}
    return dict(ranges=ranges, info=info, blocks=blocks, **out)


def extract_blocks(q, w, origin3, voxel, lattice3, min_weight, B, sel_keys, max_vertices, max_triangles):
    """alva_mesh_extract_blocks -> a dict: vertices, normals, triangles, ranges [n_sel,4] int32, info [8] int32, and for the tests cells
    [nv,3] and blocks (the per-block dicts of block_mesh)"""
    N = np.asarray(q).shape[0]
    sel = check_selection(N, lattice3, B, sel_keys)
    return pack_blocks([block_mesh(q, w, origin3, voxel, lattice3, min_weight, B, key) for key in sel], N, B, max_vertices, max_triangles)


# ---------------------------------------------------------------------------------------------------- G2 - G6
class BlockList:
    """the session's table (csrc/slam/mesh_blocks.hpp restated): key -> digest of the present blocks of the last successful call"""

    def __init__(self):
        self.table, self.epoch, self.min_weight, self.block, self.generation = {}, 0, 0, 0, -1

    def reset(self):
        self.table, self.epoch = {}, self.epoch + 1

    def call(self, generation, min_weight, B, all_, max_blocks, max_vertices, max_triangles, N, lattice3, digest, counts):
        """G2, G4, G5 and the table's part of G6 -> (info [8], reports): a report is (key (x, y, z), state, v0, nv, t0, nt, digest); no
        reports with code 3.  digest / counts are the digest stage's"""
        if generation != self.generation or min_weight != self.min_weight or B != self.block:   # G2
            self.reset()
        self.generation, self.min_weight, self.block = generation, min_weight, B
        keys = [tuple(int(v) for v in k) for k in block_keys(N, lattice3, B)]
        bmin, nb = grid(N, lattice3, B)
        present = {k: n for n, k in enumerate(keys) if counts[n][1] > 0}
        zyx = lambda k: k[::-1]
        reports = []
        for k in sorted(present, key=zyx):   # G4
            n = present[k]
            state = 1 if k not in self.table else 2 if self.table[k] != int(digest[n]) else 0
            if state or all_:
                reports.append([k, state, 0, int(counts[n][0]), 0, 2 * int(counts[n][1]), int(digest[n])])
        n_extract = len(reports)
        for k in sorted(set(self.table) - set(present), key=zyx):
            inside = all(bmin[a] <= k[a] < bmin[a] + nb[a] for a in range(3))
            reports.append([k, 3 if inside else 4, 0, 0, 0, 0, self.table[k]])
        sv, st = sum(r[3] for r in reports), sum(r[5] for r in reports)
        code = 3 if len(reports) > max_blocks or sv > max_vertices or st > max_triangles else 0   # G5
        info = [code, len(reports), sv, st, len(reports) - n_extract, self.epoch, len(present), B]
        if code == 3:
            return info, []
        v0 = t0 = 0
        for r in reports[:n_extract]:
            r[2], r[4] = v0, t0
            v0, t0 = v0 + r[3], t0 + r[5]
        self.table = {k: int(digest[n]) for k, n in present.items()}   # G6
        return info, [tuple(r) for r in reports]
