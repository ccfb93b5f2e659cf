// Plane outlines: the convex boundary polygon of each detected plane (ARCore Plane.getPolygon / ARKit ARPlaneGeometry / WebXR
// XRPlane.polygon; the reference has no counterpart, so the definition in include/alvaar_hip.h is pinned by the numpy restatement
// tests/outline_cases.py).
//
// The outline is a SET FUNCTION of the plane's points with exact predicates: the points are projected into the plane's frame in IEEE
// double in the written operation order (compile with -ffp-contract=off), snapped to an integer grid of 2^20 cells per extent, and from
// there on everything is integer arithmetic -- int64 cross products of differences below 2^23.  So any correct hull algorithm gives the
// same bits, the order of the points does not matter, and nothing below needs a fixed summation order.
//
// One launch serves all planes, one 512-thread workgroup per plane; no workgroup waits for another.  Within a workgroup:
//   gather   a strided pass over the labels: the plane's points are counted and the maxima of eight support functions (+-u, +-v, +-u+-v)
//            are taken as 64-bit keys that carry the extreme point itself (support value | tie-breaking coordinate), so the eight extreme
//            points come out of one integer max-reduction (__shfl_xor, then the waves through LDS)
//   prune    Akl-Toussaint: a second pass over the same points (now in L2) drops every point strictly inside the octagon through those
//            eight hull points and appends the rest to an LDS list (one LDS atomic per wave; the list's order is irrelevant).  On
//            scattered clouds a few hundred of several thousand survive; on a circle everything does, so the list holds the stage's
//            whole bound of 16384 points (128 KB of the CU's 160 KB: eight workgroups at most are ever launched, occupancy is no concern,
//            and no second, device-memory list with its own path is needed)
//   wrap     gift wrapping from the lexicographically smallest point: per step, a workgroup-wide reduction for "the point all others are
//            left of; among collinear ones the farthest" -- per lane over the list, __shfl_xor in the wave, the 8 waves through a
//            double-buffered LDS row, so one barrier per step.  The comparison is the sign of an int64 cross product, a total order
//            around the current vertex because that vertex is extreme.  At most max_vertices steps, whatever the input
//   finish   wave 0 sums the shoelace terms (int64: exact in any order) and the lanes write the vertices into pinned memory
#include "common.hpp"
#include <cmath>

namespace {

constexpr int PO_NT = 512, PO_WAVES = PO_NT / 64;
constexpr int PO_N_CAP = 16384, PO_MAX_PLANES = 8, PO_MIN_VERTICES = 8, PO_MAX_VERTICES = 1024;
constexpr int PO_Q = 1 << 21;   // grid coordinates are clamped to [-2^21, 2^21]

struct OutlineHead {   // one per plane, in pinned memory, followed by the plane's vertices
    int info[8];
    double area;
};

struct OutlineFrame {
    double x[3], z[3], p[3];
    double inv, cell;   // 2^20 / s and s / 2^20, computed once on the host
    int code, pad;      // the host's verdict on the frame: 0 run, 4 / 5 nothing to do
};

struct OutlineArgs {
    const double *pts;     // [n][3]
    const int *labels;     // [n]
    uint8_t *out;          // per plane: OutlineHead | int2 q[max_vertices] | float2 uv[max_vertices]
    size_t stride;         // bytes per plane in `out`
    int n, max_vertices;
    OutlineFrame f[PO_MAX_PLANES];
};

__device__ __forceinline__ long long po_cross(int ax, int ay, int bx, int by) { return (long long) ax * by - (long long) ay * bx; }

// does b replace a as the next vertex?  a, b are offsets from the current vertex; (0, 0) is "none" (the vertex itself or a copy of it).
// b wins when it lies to the right of the ray through a, or on it and farther
__device__ __forceinline__ bool po_better(int ax, int ay, int bx, int by) {
    if ((bx | by) == 0) return false;
    if ((ax | ay) == 0) return true;
    const long long cr = po_cross(ax, ay, bx, by);
    if (cr != 0) return cr < 0;
    return (long long) bx * bx + (long long) by * by > (long long) ax * ax + (long long) ay * ay;
}

// the grid point of input point i in plane frame F
__device__ __forceinline__ void po_quantise(const double *pts, int i, const OutlineFrame &F, int &qu, int &qv) {
    const double dx = pts[3 * (size_t) i] - F.p[0], dy = pts[3 * (size_t) i + 1] - F.p[1], dz = pts[3 * (size_t) i + 2] - F.p[2];
    const double u = (dx * F.x[0] + dy * F.x[1]) + dz * F.x[2], v = (dx * F.z[0] + dy * F.z[1]) + dz * F.z[2];
    qu = (int) fmin(fmax(rint(u * F.inv), (double) -PO_Q), (double) PO_Q);
    qv = (int) fmin(fmax(rint(v * F.inv), (double) -PO_Q), (double) PO_Q);
}

// The eight support keys of a grid point, U = qu + 2^21 and V = qv + 2^21 in [0, 2^22]: (support value << 24) | tie-breaking
// coordinate, in the order of the directions' angles 0, 45, .. 315 degrees.  The largest key of a direction is a point of the hull's
// face in that direction, and po_extreme recovers the point from the key
__device__ __forceinline__ void po_keys(int qu, int qv, unsigned long long (&k)[8]) {
    const unsigned long long U = (unsigned) (qu + PO_Q), V = (unsigned) (qv + PO_Q), M = 2 * PO_Q;
    k[0] = (U << 24) | V;                     // +u
    k[1] = ((U + V) << 24) | U;               // +u +v
    k[2] = (V << 24) | U;                     // +v
    k[3] = ((V + M - U) << 24) | U;           // -u +v
    k[4] = ((M - U) << 24) | (M - V);         // -u, then -v: the lexicographically smallest point, where the outline starts
    k[5] = ((2 * M - U - V) << 24) | U;       // -u -v
    k[6] = ((M - V) << 24) | U;               // -v
    k[7] = ((U + M - V) << 24) | U;           // +u -v
}

__device__ __forceinline__ void po_extreme(int dir, unsigned long long key, int &qu, int &qv) {
    const long long hi = (long long) (key >> 24), lo = (long long) (key & 0xffffff), M = 2 * PO_Q;
    long long U, V;
    switch (dir) {
    case 0: U = hi; V = lo; break;
    case 1: U = lo; V = hi - U; break;
    case 2: V = hi; U = lo; break;
    case 3: U = lo; V = hi - M + U; break;
    case 4: U = M - hi; V = M - lo; break;
    case 5: U = lo; V = 2 * M - hi - U; break;
    case 6: V = M - hi; U = lo; break;
    default: U = lo; V = U + M - hi; break;
    }
    qu = (int) (U - PO_Q);
    qv = (int) (V - PO_Q);
}

__global__ void __launch_bounds__(PO_NT) k_plane_outline(const OutlineArgs A) {
    __shared__ unsigned long long s_list[PO_N_CAP];       // survivors of the prune: (uint32) qu << 32 | (uint32) qv
    __shared__ int2 s_vert[PO_MAX_VERTICES];
    __shared__ unsigned long long s_key[PO_WAVES][8];
    __shared__ int2 s_best[2][PO_WAVES];
    __shared__ int s_cnt[PO_WAVES];
    __shared__ int s_m;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const OutlineFrame &F = A.f[k];
    OutlineHead *head = (OutlineHead *) (A.out + (size_t) k * A.stride);
    int2 *out_q = (int2 *) (head + 1);
    float2 *out_uv = (float2 *) (out_q + A.max_vertices);
    if (F.code != 0) return;   // the host has written the record

    // ---- gather: the plane's points, counted, and the eight extreme points among them
    unsigned long long key[8];
#pragma unroll
    for (int d = 0; d < 8; d++) key[d] = 0;
    int cnt = 0;
    for (int i = tid; i < A.n; i += PO_NT) {
        if (A.labels[i] != k) continue;
        int qu, qv;
        po_quantise(A.pts, i, F, qu, qv);
        unsigned long long kk[8];
        po_keys(qu, qv, kk);
#pragma unroll
        for (int d = 0; d < 8; d++) key[d] = kk[d] > key[d] ? kk[d] : key[d];
        cnt++;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
#pragma unroll
        for (int d = 0; d < 8; d++) {
            const unsigned long long other = __shfl_xor(key[d], o);
            key[d] = other > key[d] ? other : key[d];
        }
    }
    if (lane == 0) {
        s_cnt[wave] = cnt;
#pragma unroll
        for (int d = 0; d < 8; d++) s_key[wave][d] = key[d];
    }
    if (tid == 0) s_m = 0;
    __syncthreads();
    cnt = 0;
#pragma unroll
    for (int w = 0; w < PO_WAVES; w++) {
        cnt += s_cnt[w];
#pragma unroll
        for (int d = 0; d < 8; d++) key[d] = s_key[w][d] > key[d] ? s_key[w][d] : key[d];
    }
    if (cnt < 3) {
        if (tid == 0) {
            head->info[0] = 1; head->info[1] = 0; head->info[2] = cnt;
        }
        return;
    }
    int ex[8], ey[8];   // the octagon, counter-clockwise
#pragma unroll
    for (int d = 0; d < 8; d++) po_extreme(d, key[d], ex[d], ey[d]);
    bool any_edge = false;
#pragma unroll
    for (int d = 0; d < 8; d++) any_edge |= ex[d] != ex[(d + 1) & 7] || ey[d] != ey[(d + 1) & 7];

    // ---- prune: the points not strictly inside the octagon go into the list (every point when the octagon has no edge at all)
    for (int base = 0; base < A.n; base += PO_NT) {
        const int i = base + tid;
        bool keep = false;
        int qu = 0, qv = 0;
        if (i < A.n && A.labels[i] == k) {
            po_quantise(A.pts, i, F, qu, qv);
            bool inside = any_edge;
#pragma unroll
            for (int d = 0; d < 8; d++) {
                const int e0 = ex[(d + 1) & 7] - ex[d], e1 = ey[(d + 1) & 7] - ey[d];
                inside &= (e0 | e1) == 0 || po_cross(e0, e1, qu - ex[d], qv - ey[d]) > 0;
            }
            keep = !inside;
        }
        const unsigned long long mask = __ballot(keep);
        if (mask) {   // wave-uniform
            int pos = 0;
            if (lane == 0) pos = atomicAdd(&s_m, __popcll(mask));
            pos = __shfl(pos, 0) + __popcll(mask & ((1ull << lane) - 1));
            if (keep) s_list[pos] = ((unsigned long long) (unsigned) qu << 32) | (unsigned) qv;   // pos < the plane's points <= PO_N_CAP
        }
    }
    __syncthreads();
    const int m = s_m;

    // ---- wrap
    const int sx = ex[4], sy = ey[4];
    if (tid == 0) s_vert[0] = make_int2(sx, sy);
    int h = 1, cx = sx, cy = sy;
    bool overflow = false;
    for (int par = 0;; par ^= 1) {
        int ax = 0, ay = 0;
        for (int i = tid; i < m; i += PO_NT) {
            const unsigned long long e = s_list[i];
            const int bx = (int) (unsigned) (e >> 32) - cx, by = (int) (unsigned) e - cy;
            if (po_better(ax, ay, bx, by)) {
                ax = bx; ay = by;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const int bx = __shfl_xor(ax, o), by = __shfl_xor(ay, o);
            if (po_better(ax, ay, bx, by)) {
                ax = bx; ay = by;
            }
        }
        if (lane == 0) s_best[par][wave] = make_int2(ax, ay);
        __syncthreads();   // the only barrier of a step: the row written two steps ago has been read by every wave before this one
        ax = 0; ay = 0;
#pragma unroll
        for (int w = 0; w < PO_WAVES; w++) {
            const int2 b = s_best[par][w];
            if (po_better(ax, ay, b.x, b.y)) {
                ax = b.x; ay = b.y;
            }
        }
        const int nx = cx + ax, ny = cy + ay;
        if ((ax | ay) == 0 || (nx == sx && ny == sy)) break;   // every point is a copy of this one, or the outline has closed
        if (h == A.max_vertices) {
            overflow = true;
            break;
        }
        if (tid == 0) s_vert[h] = make_int2(nx, ny);
        h++;
        cx = nx; cy = ny;
    }
    if (h < 3 || overflow) {
        if (tid == 0) {
            head->info[0] = overflow ? 3 : 2; head->info[1] = 0; head->info[2] = cnt;
        }
        return;
    }
    __syncthreads();   // s_vert is complete

    // ---- finish: the vertices, and twice the area (int64 terms below 2^45, at most 1024 of them: exact in any order)
    for (int j = tid; j < h; j += PO_NT) {
        const int2 q = s_vert[j];
        out_q[j] = q;
        out_uv[j] = make_float2((float) ((double) q.x * F.cell), (float) ((double) q.y * F.cell));
    }
    if (wave == 0) {
        long long a2 = 0;
        for (int j = lane; j < h; j += 64) {
            const int2 a = s_vert[j], b = s_vert[j + 1 == h ? 0 : j + 1];
            a2 += (long long) a.x * b.y - (long long) b.x * a.y;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a2 += __shfl_xor(a2, o);
        if (lane == 0) {
            head->area = (((double) a2 * 0.5) * F.cell) * F.cell;
            head->info[0] = 0; head->info[1] = h; head->info[2] = cnt;
        }
    }
}

}  // namespace

extern "C" int alva_plane_outlines(alva_ctx *ctx, const double *d_points, int n, const int *d_labels, int n_planes, const float *h_planes24,
                                   int max_vertices, float *h_outline, int *h_outline_q, int *h_info8, double *h_area) {
    ALVA_ARG(ctx && h_planes24 && h_outline && h_info8 && h_area);
    ALVA_ARG(n >= 0 && n <= PO_N_CAP && ((d_points && d_labels) || n == 0));
    ALVA_ARG(n_planes >= 1 && n_planes <= PO_MAX_PLANES && max_vertices >= PO_MIN_VERTICES && max_vertices <= PO_MAX_VERTICES);
    const size_t nv = (size_t) n_planes * max_vertices;
    memset(h_outline, 0, nv * 2 * sizeof(float));
    if (h_outline_q) memset(h_outline_q, 0, nv * 2 * sizeof(int));
    memset(h_info8, 0, (size_t) n_planes * 8 * sizeof(int));
    memset(h_area, 0, (size_t) n_planes * sizeof(double));
    OutlineArgs A{};
    int to_run = 0;
    for (int k = 0; k < n_planes; k++) {
        const float *rec = h_planes24 + 24 * k;
        OutlineFrame &F = A.f[k];
        const double s = (double) (rec[16] > rec[17] ? rec[16] : rec[17]);   // a NaN extent gives the other one, or NaN
        bool finite = std::isfinite((double) rec[16]) && std::isfinite((double) rec[17]);
        for (int c = 0; c < 3; c++) {
            F.x[c] = (double) rec[c]; F.z[c] = (double) rec[8 + c]; F.p[c] = (double) rec[12 + c];
            finite = finite && std::isfinite(F.x[c]) && std::isfinite(F.z[c]) && std::isfinite(F.p[c]);
        }
        if (rec[15] != 1.f) F.code = 5;
        else if (!finite || !(s > 0)) F.code = 4;
        else if (n == 0) F.code = 1;
        else {
            F.inv = 1048576.0 / s;
            F.cell = s / 1048576.0;
            to_run++;
        }
        h_info8[8 * k] = F.code;
    }
    if (to_run == 0) return 0;
    A.stride = (sizeof(OutlineHead) + (size_t) max_vertices * (sizeof(int2) + sizeof(float2)) + 255) / 256 * 256;
    uint8_t *pin = nullptr;
    const int rc = alva_ctx_pinned(ctx, A.stride * n_planes, (void **) &pin);
    if (rc) return rc;
    A.pts = d_points;
    A.labels = d_labels;
    A.out = pin;
    A.n = n;
    A.max_vertices = max_vertices;
    for (int k = 0; k < n_planes; k++) {
        OutlineHead hd{};
        hd.info[0] = -1;   // a workgroup that runs writes its code
        memcpy(pin + k * A.stride, &hd, sizeof(hd));
    }
    hipLaunchKernelGGL(k_plane_outline, dim3(n_planes), dim3(PO_NT), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(alva_stream_sync(ctx->stream));
    int found = 0;
    for (int k = 0; k < n_planes; k++) {
        if (A.f[k].code != 0) continue;
        OutlineHead hd;
        memcpy(&hd, pin + k * A.stride, sizeof(hd));
        if (hd.info[0] < 0 || hd.info[0] > 3 || hd.info[1] < 0 || hd.info[1] > max_vertices) {
            alva_set_error("alva_plane_outlines: plane %d came back with code %d and %d vertices", k, hd.info[0], hd.info[1]);
            return ALVA_ERR_STATE;
        }
        memcpy(h_info8 + 8 * k, hd.info, sizeof(hd.info));
        if (hd.info[0] != 0) continue;
        const uint8_t *q = pin + k * A.stride + sizeof(OutlineHead);
        if (h_outline_q) memcpy(h_outline_q + (size_t) k * max_vertices * 2, q, (size_t) hd.info[1] * sizeof(int2));
        memcpy(h_outline + (size_t) k * max_vertices * 2, q + (size_t) max_vertices * sizeof(int2), (size_t) hd.info[1] * sizeof(float2));
        h_area[k] = hd.area;
        found++;
    }
    return found;
}
