// Scene mesh in blocks: the volume's surface per block of a world-fixed lattice (L1 - L4 of include/alvaar_hip.h) -- a digest and two
// counts per block (alva_mesh_block_digest) and the meshes of selected blocks, each with indices of its own (alva_mesh_extract_blocks).
// What ARKit hands out as ARMeshAnchors and WebXR as XRMesh objects with lastChangedTime.  The reference has no counterpart; the
// definitions are pinned by the numpy restatement tests/mesh_block_cases.py.  The predicates and the vertex are alva_mesh_extract's own
// bodies (mesh_device.hpp): X1 - X6 exist once.
//
// A workgroup of 256 takes one block and works on its box of (B + 2)^3 voxels, d in [-1, B]^3, in LDS:
//   load      the box's voxels in the order of L3's p -- consecutive p are consecutive along i, so a wave's loads are runs of B + 2
//             contiguous voxels -- each reduced to two bits (valid, inside), which is all X2 and X6 ask; a voxel outside the cube is
//             invalid.  34^3 bytes at B = 32.  With DIGEST, L3's term per valid voxel, summed per thread, per wave, per workgroup: one
//             workgroup owns one block, so the sum is stored, not added atomically
//   cells     the (B + 1)^3 cells d in [-1, B - 1]^3 in ascending index, 256 at a time: X2 from the LDS bits, the activity of a wave's 64
//             cells one ballot word in LDS; nv = their count
//   quads     the B^3 own voxels in ascending index, 256 at a time: X6 from the LDS bits and words; nq = their count
// k_mesh_block_count    load, cells, quads -> digest (DIGEST) and (nv, nq); the block is the grid's (blockIdx.x) or the selection's
// k_mesh_block_ranges   one workgroup: the exclusive scan of the selection's counts -> ranges, totals, the code
// k_mesh_block_emit     load, cells, then the exclusive scan of the words' popcounts (a cell's rank is a prefix count), the vertices of the
//                       active cells and the triangles of the own voxels' quads, whose place is a running prefix over the 256-voxel steps
// alva_mesh_block_digest is one launch, alva_mesh_extract_blocks three, whatever N and n_sel.  No workgroup waits for another: what one
// launch needs of the one before comes from the stream's order.  Nothing but the outputs and the context's scratch is written.
#include "common.hpp"
#include "mesh_device.hpp"
#include "wave_utils.hpp"
#include <climits>
#include <cmath>

namespace {

constexpr int BLOCKS_SCRATCH_SLOT = 9;   // (shared with the other synchronous stages)
constexpr int BLOCKS_N_MIN = 4, BLOCKS_N_MAX = 256;
constexpr int BLOCKS_LATTICE_MAX = 1 << 30;   // |lattice| at most: lattice + N cannot overflow

struct BlockArgs {
    const int16_t *q;
    const uint8_t *w;
    int N, min_weight;
    int lattice[3];
    int bmin[3], nb[3];   // L1's grid: the lowest key and the number of blocks per axis
    const int *keys;      // [n][3], or null: the grid's blocks in ascending (b_z, b_y, b_x)
    int n;                // blocks
    unsigned long long *digest;   // [n] (DIGEST)
    int *counts;                  // [n][2] = nv, nq
    // the extraction
    double o[3], voxel;
    int max_vertices, max_triangles;
    int *ranges;   // [n][4] = v0, nv, t0, nt
    int *info;     // [8]
    float *vertices, *normals;
    int *triangles;
};

__host__ __device__ __forceinline__ int floor_div(int g, int B) { return g >= 0 ? g / B : -((-g + B - 1) / B); }

// L3's term of one valid voxel
__device__ __forceinline__ unsigned long long block_digest_term(int p, int q) {
    const unsigned long long x = ((unsigned long long) p << 17) | 0x10000ull | (unsigned long long) (uint16_t) q;
    unsigned long long z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <int B>
struct BlockTile {
    static constexpr int E = B + 2, C = B + 1;   // the box's and the cells' edge
    static constexpr int E3 = E * E * E, C3 = C * C * C, B3 = B * B * B;
    static constexpr int WORDS = (C3 + 255) / 256 * 4;   // every 256-cell step writes its four words
    uint8_t state[E3];   // bit 0 valid, bit 1 inside, by L3's p
    unsigned long long bits[WORDS];   // bit l of word W = the cell of index 64 W + l is active; the index is ((d_z + 1) C + d_y + 1) C + d_x + 1
    int wpre[WORDS];   // (emit) the active cells of the words before
    int s4[4];
    unsigned long long s4u[4];
};

// the key of the workgroup's block and l0 = the local voxel index of d = (-1, -1, -1)
__device__ __forceinline__ void block_of_workgroup(const BlockArgs &A, int B, int (&l0)[3]) {
    int key[3];
    if (A.keys) {
#pragma unroll
        for (int a = 0; a < 3; a++) key[a] = A.keys[3 * blockIdx.x + a];
    } else {
        const int id = blockIdx.x;
        key[0] = A.bmin[0] + id % A.nb[0];
        key[1] = A.bmin[1] + (id / A.nb[0]) % A.nb[1];
        key[2] = A.bmin[2] + id / (A.nb[0] * A.nb[1]);
    }
#pragma unroll
    for (int a = 0; a < 3; a++) l0[a] = B * key[a] - A.lattice[a] - 1;
}

// load: the box into T.state; returns the thread's part of L3's sum (DIGEST)
template <int B, bool DIGEST>
__device__ __forceinline__ unsigned long long block_load(const BlockArgs &A, const int (&l0)[3], BlockTile<B> &T) {
    using Tl = BlockTile<B>;
    const int N = A.N;
    unsigned long long sum = 0;
    for (int p = threadIdx.x; p < Tl::E3; p += 256) {
        const int li = l0[0] + p % Tl::E, lj = l0[1] + (p / Tl::E) % Tl::E, lk = l0[2] + p / (Tl::E * Tl::E);
        int st = 0;
        if ((unsigned) li < (unsigned) N && (unsigned) lj < (unsigned) N && (unsigned) lk < (unsigned) N) {
            const int idx = (lk * N + lj) * N + li;
            if (A.w[idx] >= A.min_weight) {   // X1
                const int qv = A.q[idx];
                st = qv < 0 ? 3 : 1;
                if constexpr (DIGEST) sum += block_digest_term(p, qv);
            }
        }
        T.state[p] = (uint8_t) st;
    }
    return sum;
}

// cells: T.bits from T.state; returns the thread's count of active cells
template <int B>
__device__ __forceinline__ int block_cells(BlockTile<B> &T) {
    using Tl = BlockTile<B>;
    const int vs[3] = {1, Tl::E, Tl::E * Tl::E};
    int nv = 0;
    for (int c0 = 0; c0 < Tl::C3; c0 += 256) {   // (every thread takes every step: the ballot is the whole wave's)
        const int c = c0 + threadIdx.x;
        bool active = false;
        if (c < Tl::C3) {
            const int p = ((c / (Tl::C * Tl::C)) * Tl::E + (c / Tl::C) % Tl::C) * Tl::E + c % Tl::C;   // the cell's minimum corner in the box
            // X2 (a cell that does not exist in the cube has a corner outside it, which is invalid)
            active = mesh_cell_active_at(
                vs, [&](int o) { return (T.state[p + o] & 1) != 0; }, [&](int o) { return (T.state[p + o] & 2) != 0; });
        }
        const unsigned long long word = __ballot(active);
        if ((threadIdx.x & 63) == 0) T.bits[c >> 6] = word;
        nv += active ? 1 : 0;
    }
    return nv;
}

template <int B>
__device__ __forceinline__ bool block_cell_active(const BlockTile<B> &T, int c) { return (T.bits[c >> 6] >> (c & 63)) & 1ull; }

// quads: X6's mask of the own voxel v = (d_z B + d_y) B + d_x, l0 as above
template <int B>
__device__ __forceinline__ int block_quad_mask(const BlockArgs &A, const int (&l0)[3], const BlockTile<B> &T, int v, int &cell) {
    using Tl = BlockTile<B>;
    const int d[3] = {v % B, (v / B) % B, v / (B * B)};
    const int p[3] = {l0[0] + 1 + d[0], l0[1] + 1 + d[1], l0[2] + 1 + d[2]};   // the local voxel index: X6's grid conditions are on it
    const int vs[3] = {1, Tl::E, Tl::E * Tl::E}, cs[3] = {1, Tl::C, Tl::C * Tl::C};
    const int pv = ((d[2] + 1) * Tl::E + d[1] + 1) * Tl::E + d[0] + 1;
    cell = ((d[2] + 1) * Tl::C + d[1] + 1) * Tl::C + d[0] + 1;
    const int cv = cell;
    if (!(T.state[pv] & 1)) return 0;   // (also every voxel outside the cube, whose p is no index)
    return mesh_quad_mask(
        p, A.N, vs, cs, [&](int o) { return (T.state[pv + o] & 1) != 0; }, [&](int o) { return (T.state[pv + o] & 2) != 0; },
        [&](int o) { return block_cell_active(T, cv + o); });
}

// the sum of v over the workgroup's four waves, delivered to every thread
__device__ __forceinline__ int blocks_sum_256(int v, int *s4) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    const int r = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    __syncthreads();
    return r;
}

template <int B, bool DIGEST>
__global__ void __launch_bounds__(256) k_mesh_block_count(const BlockArgs A) {
    __shared__ BlockTile<B> T;
    int l0[3];
    block_of_workgroup(A, B, l0);
    unsigned long long sum = block_load<B, DIGEST>(A, l0, T);
    __syncthreads();
    if constexpr (DIGEST) {
        // (integers mod 2^64: the order of the additions does not matter)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
        if ((threadIdx.x & 63) == 0) T.s4u[threadIdx.x >> 6] = sum;
    }
    const int nv = blocks_sum_256(block_cells(T), T.s4);   // (its barriers also publish the words and s4u)
    int nq = 0;
    for (int v = threadIdx.x; v < BlockTile<B>::B3; v += 256) {
        int cell;
        nq += __popc(block_quad_mask(A, l0, T, v, cell) & 7);
    }
    nq = blocks_sum_256(nq, T.s4);
    if (threadIdx.x == 0) {
        if constexpr (DIGEST) A.digest[blockIdx.x] = (T.s4u[0] + T.s4u[1]) + (T.s4u[2] + T.s4u[3]);
        A.counts[2 * blockIdx.x] = nv;
        A.counts[2 * blockIdx.x + 1] = nq;
    }
}

// the exclusive scan of one value per thread over a workgroup of T threads (a multiple of 64, at most 1024); total = the sum of all
template <int THREADS>
__device__ __forceinline__ int blocks_excl_scan(int v, int *s16, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s16[wave] = x;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int u = 0; u < THREADS / 64; u++) {
        base += u < wave ? s16[u] : 0;
        total += s16[u];
    }
    __syncthreads();
    return base + x - v;
}

__global__ void __launch_bounds__(1024) k_mesh_block_ranges(const BlockArgs A) {
    __shared__ int s16[16];
    const int n = A.n, per = (n + 1023) / 1024;
    const int b0 = threadIdx.x * per < n ? threadIdx.x * per : n, b1 = b0 + per < n ? b0 + per : n;
    // (the totals fit an int: a volume has fewer than 2^24 cells, each in at most 8 blocks, and fewer than 3 * 2^24 quads)
    int sv = 0, sq = 0, sp = 0;
    for (int b = b0; b < b1; b++) {
        sv += A.counts[2 * b];
        sq += A.counts[2 * b + 1];
        sp += A.counts[2 * b + 1] > 0;
    }
    int tv, tq, tp;
    int ov = blocks_excl_scan<1024>(sv, s16, tv), oq = blocks_excl_scan<1024>(sq, s16, tq);
    (void) blocks_excl_scan<1024>(sp, s16, tp);
    const bool over = tv > A.max_vertices || 2 * tq > A.max_triangles;
    for (int b = b0; b < b1 && !over; b++) {
        const int cv = A.counts[2 * b], cq = A.counts[2 * b + 1];
        A.ranges[4 * b] = ov;
        A.ranges[4 * b + 1] = cv;
        A.ranges[4 * b + 2] = 2 * oq;
        A.ranges[4 * b + 3] = 2 * cq;
        ov += cv;
        oq += cq;
    }
    if (threadIdx.x == 0) {
        A.info[0] = over ? 3 : tv == 0 ? 1 : 0;
        A.info[1] = tv;
        A.info[2] = 2 * tq;
        A.info[3] = n;
        A.info[4] = tp;
        A.info[5] = A.N;
        A.info[6] = 0;   // (B: the host's)
        A.info[7] = 0;
    }
}

template <int B>
__global__ void __launch_bounds__(256) k_mesh_block_emit(const BlockArgs A) {
    using Tl = BlockTile<B>;
    __shared__ Tl T;
    if (A.info[0] == 3) return;
    const int nv = A.ranges[4 * blockIdx.x + 1];
    if (nv == 0) return;   // (no active cell: no vertex and no quad)
    const int v0 = A.ranges[4 * blockIdx.x], t0 = A.ranges[4 * blockIdx.x + 2];
    int l0[3];
    block_of_workgroup(A, B, l0);
    (void) block_load<B, false>(A, l0, T);
    __syncthreads();
    (void) block_cells(T);
    __syncthreads();
    {   // the words' prefix counts: a thread takes PER consecutive words
        constexpr int PER = (Tl::WORDS + 255) / 256;
        const int w0 = threadIdx.x * PER;
        int mine = 0, total;
        for (int u = w0; u < w0 + PER && u < Tl::WORDS; u++) mine += __popcll(T.bits[u]);
        int at = blocks_excl_scan<256>(mine, T.s4, total);
        for (int u = w0; u < w0 + PER && u < Tl::WORDS; u++) {
            T.wpre[u] = at;
            at += __popcll(T.bits[u]);
        }
    }
    __syncthreads();
    const auto rank = [&](int c) { return T.wpre[c >> 6] + __popcll(T.bits[c >> 6] & ((1ull << (c & 63)) - 1ull)); };
    const int N = A.N;
    // L2's vertices: X3 / X4 on the cell's local index
    for (int c = threadIdx.x; c < Tl::C3; c += 256) {
        if (!block_cell_active(T, c)) continue;
        const int p[3] = {l0[0] + c % Tl::C, l0[1] + (c / Tl::C) % Tl::C, l0[2] + c / (Tl::C * Tl::C)};   // all eight corners lie in the cube
        const int idx = (p[2] * N + p[1]) * N + p[0];
        int q[8];
#pragma unroll
        for (int k = 0; k < 8; k++) q[k] = A.q[idx + (k & 1) + ((k >> 1) & 1) * N + (k >> 2) * N * N];
        float v[3], n[3];
        mesh_cell_vertex(q, p, A.o, A.voxel, v, n);
        const size_t at = 3 * ((size_t) v0 + rank(c));
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            A.vertices[at + ax] = v[ax];
            A.normals[at + ax] = n[ax];
        }
    }
    // L2's triangles: the quads before a voxel are those of the steps before it (done), of the lower waves of its step (LDS) and of the
    // lower lanes of its wave (ballots)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int cs[3] = {1, Tl::C, Tl::C * Tl::C};
    int done = 0;
    for (int v = threadIdx.x; v < Tl::B3; v += 256) {   // (B^3 is a multiple of 256: every thread takes every step)
        int cell;
        const int mask = block_quad_mask(A, l0, T, v, cell);
        const unsigned long long b0 = __ballot(mask & 1), b1 = __ballot(mask & 2), b2 = __ballot(mask & 4);
        if (lane == 0) T.s4[wave] = __popcll(b0) + __popcll(b1) + __popcll(b2);
        __syncthreads();
        int quad = done + __popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt);
        for (int u = 0; u < wave; u++) quad += T.s4[u];
        done += (T.s4[0] + T.s4[1]) + (T.s4[2] + T.s4[3]);
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!(mask & (1 << a))) continue;
            const int sb = cs[(a + 1) % 3], sc = cs[(a + 2) % 3];
            mesh_quad_triangles(A.triangles + 3 * (size_t) t0 + 6 * (size_t) quad, (mask & 8) != 0, rank(cell - sb - sc), rank(cell - sc), rank(cell),
                                rank(cell - sb));
            quad++;
        }
    }
}

// the arguments both calls share; fills A's volume, lattice and grid
int blocks_common(BlockArgs &A, alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const int *h_lattice3, int min_weight, int B) {
    ALVA_ARG(ctx && d_q && d_w && h_lattice3);
    ALVA_ARG(N >= BLOCKS_N_MIN && N <= BLOCKS_N_MAX);
    ALVA_ARG(B == 8 || B == 16 || B == 32);
    ALVA_ARG(min_weight >= 1 && min_weight <= 255);
    A.q = d_q; A.w = d_w; A.N = N; A.min_weight = min_weight;
    for (int a = 0; a < 3; a++) {
        ALVA_ARG(h_lattice3[a] >= -BLOCKS_LATTICE_MAX && h_lattice3[a] <= BLOCKS_LATTICE_MAX);
        A.lattice[a] = h_lattice3[a];
        A.bmin[a] = floor_div(h_lattice3[a], B);   // L1
        A.nb[a] = floor_div(h_lattice3[a] + N - 1, B) - A.bmin[a] + 1;
    }
    return ALVA_OK;
}

template <bool DIGEST>
void launch_count(const BlockArgs &A, int B, hipStream_t st) {
    if (B == 8) hipLaunchKernelGGL((k_mesh_block_count<8, DIGEST>), dim3(A.n), dim3(256), 0, st, A);
    else if (B == 16) hipLaunchKernelGGL((k_mesh_block_count<16, DIGEST>), dim3(A.n), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((k_mesh_block_count<32, DIGEST>), dim3(A.n), dim3(256), 0, st, A);
}

}  // namespace

extern "C" int alva_mesh_block_digest(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const int *h_lattice3, int min_weight, int B,
                                      int *h_nb3, unsigned long long *d_digest, int *d_counts) {
    BlockArgs A{};
    if (const int rc = blocks_common(A, ctx, d_q, d_w, N, h_lattice3, min_weight, B)) return rc;
    ALVA_ARG(h_nb3 && d_digest && d_counts && ((uintptr_t) d_digest % 8) == 0 && ((uintptr_t) d_counts % 4) == 0);
    A.n = A.nb[0] * A.nb[1] * A.nb[2];
    A.digest = d_digest; A.counts = d_counts;
    launch_count<true>(A, B, ctx->stream);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(alva_stream_sync(ctx->stream));
    memcpy(h_nb3, A.nb, sizeof(A.nb));
    return ALVA_OK;
}

extern "C" int alva_mesh_extract_blocks(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const double *h_origin3, double voxel,
                                        const int *h_lattice3, int min_weight, int B, int n_sel, const int *h_sel_keys, int max_vertices,
                                        int max_triangles, float *d_vertices, float *d_normals, int *d_triangles, int *h_ranges, int *h_info8) {
    BlockArgs A{};
    if (const int rc = blocks_common(A, ctx, d_q, d_w, N, h_lattice3, min_weight, B)) return rc;
    ALVA_ARG(h_origin3 && d_vertices && d_normals && d_triangles && h_info8);
    ALVA_ARG(std::isfinite(voxel) && voxel > 0 && max_vertices >= 1 && max_triangles >= 1);
    for (int i = 0; i < 3; i++) ALVA_ARG(std::isfinite(h_origin3[i]));
    ALVA_ARG(n_sel >= 0 && n_sel <= A.nb[0] * A.nb[1] * A.nb[2] && (n_sel == 0 || (h_sel_keys && h_ranges)));
    for (int s = 0; s < n_sel; s++) {
        const int *k = h_sel_keys + 3 * s;
        for (int a = 0; a < 3; a++) ALVA_ARG(k[a] >= A.bmin[a] && k[a] < A.bmin[a] + A.nb[a]);
        if (s > 0) {   // strictly ascending (z, y, x)
            const int *p = k - 3;
            ALVA_ARG(p[2] < k[2] || (p[2] == k[2] && (p[1] < k[1] || (p[1] == k[1] && p[0] < k[0]))));
        }
    }
    memset(h_info8, 0, 8 * sizeof(int));
    h_info8[0] = 1; h_info8[5] = N; h_info8[6] = B;
    if (n_sel == 0) return ALVA_OK;   // nothing selected: no surface, and nothing to launch
    memcpy(A.o, h_origin3, sizeof(A.o));
    A.voxel = voxel;
    A.max_vertices = max_vertices; A.max_triangles = max_triangles;
    A.vertices = d_vertices; A.normals = d_normals; A.triangles = d_triangles;
    A.n = n_sel;
    const size_t n = (size_t) n_sel, ints = 8 + 4 * n;   // what comes back: the info, the ranges
    int *pin = nullptr;
    int rc = alva_ctx_pinned(ctx, (64 + 3 * n + ints) * sizeof(int), (void **) &pin);
    if (rc) return rc;
    uint8_t *scr = nullptr;
    rc = alva_ctx_scratch(ctx, BLOCKS_SCRATCH_SLOT, (ints + 3 * n + 2 * n) * sizeof(int), (void **) &scr);
    if (rc) return rc;
    A.info = (int *) scr;
    A.ranges = A.info + 8;
    int *d_keys = A.ranges + 4 * n;
    A.counts = d_keys + 3 * n;
    A.keys = d_keys;
    int *pin_keys = pin + 64, *pin_back = pin_keys + 3 * n;
    memcpy(pin_keys, h_sel_keys, 3 * n * sizeof(int));
    ALVA_HIP(hipMemcpyAsync(d_keys, pin_keys, 3 * n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    launch_count<false>(A, B, ctx->stream);
    ALVA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_block_ranges, dim3(1), dim3(1024), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    if (B == 8) hipLaunchKernelGGL(k_mesh_block_emit<8>, dim3(n_sel), dim3(256), 0, ctx->stream, A);
    else if (B == 16) hipLaunchKernelGGL(k_mesh_block_emit<16>, dim3(n_sel), dim3(256), 0, ctx->stream, A);
    else hipLaunchKernelGGL(k_mesh_block_emit<32>, dim3(n_sel), dim3(256), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(hipMemcpyAsync(pin_back, A.info, ints * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ALVA_HIP(alva_stream_sync(ctx->stream));
    memcpy(h_info8, pin_back, 8 * sizeof(int));
    h_info8[6] = B;
    if (h_info8[0] != 3) memcpy(h_ranges, pin_back + 8, 4 * n * sizeof(int));
    return ALVA_OK;
}
