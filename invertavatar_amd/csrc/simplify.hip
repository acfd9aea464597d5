// Mesh simplification on the device: quadric vertex clustering on a uniform grid (Rossignac-Borrel clusters, Lindstrom's quadric
// representative).  No counterpart in the reference; geometry.py (_simplify_numpy) restates every line in NumPy and is the definition.
//
// A vertex's cell is the fp32 function of TriangleGrid, clamp(floor((x - lo) * inv), 0, n - 1) per axis; its key the linear cell index
// (x slowest, z fastest) as int64, kNoCell for a vertex with a non-finite coordinate.  The caller sorts the keys (torch.sort); every
// other step is here:
//
//   box        : lo / hi of the finite vertices (min / max: no order dependence), per thread, wave, workgroup, then a final launch.
//   clusters   : heads of the sorted keys -> one-workgroup scan -> cluster ordinal per vertex (ascending cell index), start and key per
//                cluster.
//   classify   : per face: usable (three clusters), surviving (three different clusters), the rotated ordinal triple and its sort key,
//                the referenced flag of its clusters (plain stores of 1) and up to three (cluster, face) pair keys for the quadrics.
//                Counts by integer atomics, one per wave.  Without `ref` and `pairs` this is the count-only pass of the bisection.
//   face_heads : the caller sorts the face keys; heads of the sorted triples -> scan = position of every unique face, total F'.
//   refs       : scan of the referenced flags = output index of every cluster, total V'.  The host reads V' and F' once.
//   outputs    : vertex_map, the cluster of every output vertex and its size.      faces: the remapped unique triples, in sorted order.
//   accumulate : segmented sums of double rows over entries sorted by cluster (vertices: up to 4 columns of a double array; pairs: the
//                9 numbers of the face's plane quadric about the centre of the cluster's cell).  One thread walks kChunk = 32
//                consecutive entries in index order; a segment that lies strictly inside the chunk is complete and goes to the sums, the
//                first and the last segment of the chunk go to the next level as two rows (a chunk of one segment: the sum and a zero
//                row), which is reduced the same way until one chunk is left.  So a cluster of n entries costs log_16 n levels, not n
//                steps on one lane, single-vertex clusters are summed 32 per lane, and the order of every addition depends on the
//                entry order alone: no floating-point atomics, the same bits from run to run.
//   place      : per output vertex the mean m and, for 'quadric', the minimiser of the summed quadric about m through the truncated
//                pseudo-inverse (cyclic Jacobi, kSweeps fixed sweeps, double; eigenvalues <= 1e-3 of the largest are dropped), clamped
//                to the cell.  Plain IEEE double arithmetic (+ - * / sqrt), no fast-math intrinsics.
#include "geom_common.h"

#include <algorithm>
#include <cmath>

namespace {

using ia::cell_of; using ia::kScanBlock; using ia::on_device; using ia::wave_count; using ia::wave_min;

constexpr int kBlock = 256;
constexpr int kChunk = 32;
constexpr int kBoxBlocks = 1024;
constexpr int kSweeps = 8;
constexpr int kMaxAxis = 1 << 20;                    // cells per axis: the linear index stays below 2^60
constexpr int64_t kMaxCount = (int64_t)1 << 28;      // vertices and faces: 3 F pair slots stay below 2^31
constexpr int64_t kNoCell = INT64_MAX;
constexpr int kNoCluster = 0x7fffffff;

struct Cells {
    int n[3];
    float lo[3], inv[3];
    double cell[3];
};

// ------------------------------------------------------------------ box

__global__ __launch_bounds__(kBlock) void box_kernel(const float* __restrict__ verts, int64_t V, float* __restrict__ slots) {
    float m[6] = {INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY};       // min x y z, min of -x -y -z
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < V; i += (int64_t)gridDim.x * kBlock) {
        const float x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
        m[0] = fminf(m[0], x); m[1] = fminf(m[1], y); m[2] = fminf(m[2], z);
        m[3] = fminf(m[3], -x); m[4] = fminf(m[4], -y); m[5] = fminf(m[5], -z);
    }
    __shared__ float part[kBlock / 64][6];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float v = wave_min(m[k]);
        if (lane == 0) part[w][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = part[0][threadIdx.x];
        for (int j = 1; j < kBlock / 64; ++j) v = fminf(v, part[j][threadIdx.x]);
        slots[(int64_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(64) void box_final_kernel(const float* __restrict__ slots, int blocks, float* __restrict__ box) {
    const int k = threadIdx.x;
    if (k >= 6) return;
    float v = slots[k];
    for (int b = 1; b < blocks; ++b) v = fminf(v, slots[(int64_t)b * 6 + k]);
    box[k] = k < 3 ? v : -v;                         // lo x y z, hi x y z (+inf / -inf without a finite vertex)
}

// ------------------------------------------------------------------ keys, clusters

__global__ __launch_bounds__(kBlock) void keys_kernel(const float* __restrict__ verts, int64_t V, Cells g, int64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= V) return;
    const float x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
    int64_t key = kNoCell;
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
        const int ix = cell_of(x, g.lo[0], g.inv[0], g.n[0]), iy = cell_of(y, g.lo[1], g.inv[1], g.n[1]),
                  iz = cell_of(z, g.lo[2], g.inv[2], g.n[2]);
        key = ((int64_t)ix * g.n[1] + iy) * g.n[2] + iz;
    }
    keys[i] = key;
}

__global__ __launch_bounds__(kBlock) void key_heads_kernel(const int64_t* __restrict__ skeys, int64_t V, int* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= V) return;
    const int64_t k = skeys[i];
    flags[i] = (k != kNoCell && (i == 0 || k != skeys[i - 1])) ? 1 : 0;
}

// One workgroup: out[0 .. n) = exclusive sums of in[0 .. n), out[n] = total.  in == out is allowed.
__global__ __launch_bounds__(kScanBlock) void scan_kernel(const int* in, int* out, int64_t n) {
    const int total = ia::scan_workgroup<int>(in, out, n);
    if (threadIdx.x == 0) out[n] = total;
}

struct ClusterArgs {
    const int64_t* skeys;
    const int64_t* order;
    int64_t V;
    const int* excl;             // [V + 1] exclusive scan of the head flags
    int* vcluster;               // [V] by vertex
    int* vseg;                   // [V] by sorted position
    int* cstart;                 // [cap + 1]
    int64_t* ckey;               // [cap]
    int64_t cap;
    int* count;                  // K, number of vertices that have a cell
};

__global__ __launch_bounds__(kBlock) void clusters_kernel(ClusterArgs u) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= u.V) return;
    const int64_t key = u.skeys[i], o = u.order[i];
    const int K = u.excl[u.V];
    if (i == 0) {
        u.count[0] = K;
        if (key == kNoCell) { u.count[1] = 0; u.cstart[0] = 0; }
    }
    if (key == kNoCell) {
        u.vseg[i] = kNoCluster;
        if ((uint64_t)o < (uint64_t)u.V) u.vcluster[o] = -1;
        return;
    }
    const int head = (i == 0 || key != u.skeys[i - 1]) ? 1 : 0;
    const int cl = u.excl[i] + head - 1;
    u.vseg[i] = cl;
    if ((uint64_t)o < (uint64_t)u.V) u.vcluster[o] = cl;
    if (head && cl < u.cap) { u.cstart[cl] = (int)i; u.ckey[cl] = key; }
    if (i == u.V - 1 || u.skeys[i + 1] == kNoCell) {
        u.count[1] = (int)(i + 1);
        if (K <= u.cap) u.cstart[K] = (int)(i + 1);
    }
}

// ------------------------------------------------------------------ faces

struct ClassifyArgs {
    const int* faces;
    int64_t F;
    int64_t V;
    const int* vcluster;
    int K;
    int wide;                    // K^3 does not fit int64: key = b K + c, the caller sorts by it and then (stably) by a
    int* tri;                    // [F,3] rotated cluster ordinals, kNoCluster x 3 for a face that does not survive
    int64_t* key;                // [F]
    int* ref;                    // [K] or null
    int* pairs;                  // [3 F] or null
    int* count;                  // usable faces, surviving faces, pairs
};

__global__ __launch_bounds__(kBlock) void classify_kernel(ClassifyArgs u) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = f < u.F;
    int c0 = -1, c1 = -1, c2 = -1;
    if (live) {
        const int i0 = u.faces[3 * f], i1 = u.faces[3 * f + 1], i2 = u.faces[3 * f + 2];
        if ((int64_t)(unsigned)i0 < u.V && (int64_t)(unsigned)i1 < u.V && (int64_t)(unsigned)i2 < u.V && i0 >= 0 && i1 >= 0 && i2 >= 0) {
            c0 = u.vcluster[i0]; c1 = u.vcluster[i1]; c2 = u.vcluster[i2];
        }
    }
    const bool in_k = (unsigned)c0 < (unsigned)u.K && (unsigned)c1 < (unsigned)u.K && (unsigned)c2 < (unsigned)u.K;
    const bool usable = live && in_k;
    const bool surv = usable && c0 != c1 && c1 != c2 && c0 != c2;
    int npair = 0;
    if (live) {
        int a = kNoCluster, b = kNoCluster, c = kNoCluster;
        int64_t key = INT64_MAX;
        if (surv) {
            if (c0 < c1 && c0 < c2) { a = c0; b = c1; c = c2; }
            else if (c1 < c0 && c1 < c2) { a = c1; b = c2; c = c0; }
            else { a = c2; b = c0; c = c1; }
            key = (int64_t)b * u.K + c;
            if (!u.wide) key += (int64_t)a * u.K * u.K;
            if (u.ref) { u.ref[c0] = 1; u.ref[c1] = 1; u.ref[c2] = 1; }
        }
        u.tri[3 * f] = a; u.tri[3 * f + 1] = b; u.tri[3 * f + 2] = c;
        u.key[f] = key;
        const bool p1 = usable && c1 != c0, p2 = usable && c2 != c0 && c2 != c1;
        npair = (usable ? 1 : 0) + (p1 ? 1 : 0) + (p2 ? 1 : 0);
        if (u.pairs) {
            u.pairs[3 * f] = usable ? c0 : kNoCluster;
            u.pairs[3 * f + 1] = p1 ? c1 : kNoCluster;
            u.pairs[3 * f + 2] = p2 ? c2 : kNoCluster;
        }
    }
    wave_count(usable, u.count);
    wave_count(surv, u.count + 1);
    wave_count(npair >= 2, u.count + 2);             // pairs = usable + second + third, counted as three predicates
    wave_count(npair >= 3, u.count + 2);
    wave_count(npair >= 1, u.count + 2);
}

__device__ __forceinline__ bool face_head(const int* __restrict__ tri, const int64_t* __restrict__ perm, int64_t F, int64_t i) {
    const int64_t p = perm[i];
    if ((uint64_t)p >= (uint64_t)F) return false;
    const int a = tri[3 * p], b = tri[3 * p + 1], c = tri[3 * p + 2];
    if (a == kNoCluster) return false;
    if (i == 0) return true;
    const int64_t q = perm[i - 1];
    if ((uint64_t)q >= (uint64_t)F) return true;
    return a != tri[3 * q] || b != tri[3 * q + 1] || c != tri[3 * q + 2];
}

__global__ __launch_bounds__(kBlock) void face_heads_kernel(const int* __restrict__ tri, const int64_t* __restrict__ perm, int64_t F,
                                                           int* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < F) flags[i] = face_head(tri, perm, F, i) ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void faces_kernel(const int* __restrict__ tri, const int64_t* __restrict__ perm,
                                                      const int* __restrict__ fpos, int64_t F, const int* __restrict__ outidx, int K,
                                                      int64_t* __restrict__ faces_out, int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= F || !face_head(tri, perm, F, i)) return;
    const int64_t at = fpos[i], p = perm[i];
    if (at < 0 || at >= cap) return;
    for (int j = 0; j < 3; ++j) {
        const int c = tri[3 * p + j];
        faces_out[3 * at + j] = (unsigned)c < (unsigned)K ? (int64_t)outidx[c] : -1;
    }
}

struct OutArgs {
    const int* vcluster;
    int64_t V;
    const int* ref;
    const int* outidx;
    const int* cstart;
    int K;
    int64_t* vertex_map;
    int* ocl;
    int64_t* csize;
    int64_t cap;
};

__global__ __launch_bounds__(kBlock) void outputs_kernel(OutArgs u) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < u.V) {
        const int c = u.vcluster[i];
        u.vertex_map[i] = ((unsigned)c < (unsigned)u.K && u.ref[c]) ? (int64_t)u.outidx[c] : -1;
    }
    if (i < u.K && u.ref[i]) {
        const int64_t o = u.outidx[i];
        if (o >= 0 && o < u.cap) {
            u.ocl[o] = (int)i;
            u.csize[o] = (int64_t)u.cstart[i + 1] - u.cstart[i];
        }
    }
}

// ------------------------------------------------------------------ segmented sums

__device__ __forceinline__ void cell_centre(const Cells& g, int64_t key, double* cc) {
    const int64_t iz = key % g.n[2], iy = (key / g.n[2]) % g.n[1], ix = key / ((int64_t)g.n[2] * g.n[1]);
    cc[0] = (double)g.lo[0] + ((double)ix + 0.5) * g.cell[0];
    cc[1] = (double)g.lo[1] + ((double)iy + 0.5) * g.cell[1];
    cc[2] = (double)g.lo[2] + ((double)iz + 0.5) * g.cell[2];
}

struct AccArgs {
    const int* seg;              // [n] nondecreasing cluster per entry, kNoCluster entries last
    int64_t n;
    int K;
    double* sums;                // [K, D]
    int* seg_out;                // next level: [2 * chunks]
    double* rows_out;            // [2 * chunks, D]
    const double* rows;          // SRC 0: [n, D]
    const double* cols;          // SRC 1: [V, ld] columns col0 .. col0 + ncols of vertex order[e]
    int ld, col0, ncols;
    const int64_t* order;
    int64_t V;
    const float* verts;          // SRC 2: the quadric of face order[e] / 3 about the centre of cell ckey[seg[e]]
    const int* faces;
    int64_t F;
    const int64_t* ckey;
    Cells g;
};

template <int D, int SRC>
__device__ __forceinline__ void acc_row(const AccArgs& u, int64_t e, int s, double* r) {
#pragma unroll
    for (int k = 0; k < D; ++k) r[k] = 0.0;
    if (SRC == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) r[k] = u.rows[e * D + k];
    } else if (SRC == 1) {
        const int64_t v = u.order[e];
        if ((uint64_t)v >= (uint64_t)u.V) return;
        for (int k = 0; k < D; ++k)
            if (k < u.ncols) r[k] = u.cols[v * u.ld + u.col0 + k];
    } else {
        const int64_t slot = u.order[e];
        if ((uint64_t)slot >= (uint64_t)(3 * u.F) || (unsigned)s >= (unsigned)u.K) return;
        const int64_t f = slot / 3;
        const int i0 = u.faces[3 * f], i1 = u.faces[3 * f + 1], i2 = u.faces[3 * f + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= u.V || i1 >= u.V || i2 >= u.V) return;
        double A[3], B[3], C[3], cc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            A[a] = (double)u.verts[3 * (int64_t)i0 + a];
            B[a] = (double)u.verts[3 * (int64_t)i1 + a];
            C[a] = (double)u.verts[3 * (int64_t)i2 + a];
        }
        cell_centre(u.g, u.ckey[s], cc);
        double eab[3], ebc[3], eca[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { eab[a] = B[a] - A[a]; ebc[a] = C[a] - B[a]; eca[a] = A[a] - C[a]; }
        const double lab = (eab[0] * eab[0] + eab[1] * eab[1]) + eab[2] * eab[2], lbc = (ebc[0] * ebc[0] + ebc[1] * ebc[1]) + ebc[2] * ebc[2],
                     lca = (eca[0] * eca[0] + eca[1] * eca[1]) + eca[2] * eca[2];
        // the normal from the two shorter edges, as tri_dist
        const double* p = eab; const double* q = ebc;
        if (lab >= lbc && lab >= lca) { p = ebc; q = eca; } else if (lbc >= lca) { p = eca; q = eab; }
        const double nx = p[1] * q[2] - p[2] * q[1], ny = p[2] * q[0] - p[0] * q[2], nz = p[0] * q[1] - p[1] * q[0];
        const double d = (nx * (A[0] - cc[0]) + ny * (A[1] - cc[1])) + nz * (A[2] - cc[2]);
        r[0] = nx * nx; r[1] = nx * ny; r[2] = nx * nz; r[3] = ny * ny; r[4] = ny * nz; r[5] = nz * nz;
        r[6] = -(nx * d); r[7] = -(ny * d); r[8] = -(nz * d);
    }
}

template <int D, int SRC>
__global__ __launch_bounds__(kBlock) void accumulate_kernel(AccArgs u) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t e0 = t * kChunk, e1 = min(e0 + kChunk, u.n);
    if (e0 >= u.n) return;
    const bool last_level = u.n <= kChunk;
    double acc[D], r[D];
#pragma unroll
    for (int k = 0; k < D; ++k) acc[k] = 0.0;
    const int first = u.seg[e0];
    int cur = first;
    for (int64_t e = e0; e < e1; ++e) {
        const int s = u.seg[e];
        if (s != cur) {
            if (cur == first && !last_level) {
                u.seg_out[2 * t] = cur;
#pragma unroll
                for (int k = 0; k < D; ++k) u.rows_out[2 * t * D + k] = acc[k];
            } else if ((unsigned)cur < (unsigned)u.K) {
#pragma unroll
                for (int k = 0; k < D; ++k) u.sums[(int64_t)cur * D + k] = acc[k];
            }
#pragma unroll
            for (int k = 0; k < D; ++k) acc[k] = 0.0;
            cur = s;
        }
        if (s != kNoCluster) {
            acc_row<D, SRC>(u, e, s, r);
#pragma unroll
            for (int k = 0; k < D; ++k) acc[k] += r[k];
        }
    }
    if (last_level) {
        if ((unsigned)cur < (unsigned)u.K) {
#pragma unroll
            for (int k = 0; k < D; ++k) u.sums[(int64_t)cur * D + k] = acc[k];
        }
        return;
    }
    const bool one = cur == first;                   // one segment in the chunk: its sum and a zero row
    u.seg_out[2 * t + 1] = cur;
    if (one) u.seg_out[2 * t] = cur;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        if (one) u.rows_out[2 * t * D + k] = acc[k];
        u.rows_out[(2 * t + 1) * D + k] = one ? 0.0 : acc[k];
    }
}

// ------------------------------------------------------------------ representatives

struct PlaceArgs {
    const double* vsum;          // [K,4] position sums in columns 0..2
    const double* qsum;          // [K,9] or null ('mean')
    const int* ocl;
    const int* cstart;
    const int64_t* ckey;
    int K;
    int64_t Vout;
    Cells g;
    float* out;
};

__global__ __launch_bounds__(kBlock) void place_kernel(PlaceArgs u) {
    const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (o >= u.Vout) return;
    const int k = u.ocl[o];
    if ((unsigned)k >= (unsigned)u.K) { u.out[3 * o] = u.out[3 * o + 1] = u.out[3 * o + 2] = NAN; return; }
    const double cnt = (double)(u.cstart[k + 1] - u.cstart[k]);
    double mean[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) mean[a] = u.vsum[(int64_t)k * 4 + a] / cnt;
    if (!u.qsum) {
#pragma unroll
        for (int a = 0; a < 3; ++a) u.out[3 * o + a] = (float)mean[a];
        return;
    }
    double cc[3], m[3], x[3];
    cell_centre(u.g, u.ckey[k], cc);
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = m[a] = mean[a] - cc[a];
    const double* q = u.qsum + (int64_t)k * 9;
    double a[3][3] = {{q[0], q[1], q[2]}, {q[1], q[3], q[4]}, {q[2], q[4], q[5]}};
    const bool zero = q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0 && q[4] == 0.0 && q[5] == 0.0;
    if (!zero) {
        double r[3];                                 // the residual of A x = -b at the mean
#pragma unroll
        for (int i = 0; i < 3; ++i) r[i] = -q[6 + i] - ((a[i][0] * m[0] + a[i][1] * m[1]) + a[i][2] * m[2]);
        double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        for (int sweep = 0; sweep < kSweeps; ++sweep) {
#pragma unroll
            for (int pq = 0; pq < 3; ++pq) {
                const int p = pq == 2 ? 1 : 0, qq = pq == 0 ? 1 : 2, rr = 3 - p - qq;
                const double apq = a[p][qq];
                if (apq != 0.0) {
                    const double theta = (a[qq][qq] - a[p][p]) / (2.0 * apq);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    a[p][p] = a[p][p] - t * apq;
                    a[qq][qq] = a[qq][qq] + t * apq;
                    a[p][qq] = a[qq][p] = 0.0;
                    const double arp = a[rr][p], arq = a[rr][qq];
                    a[rr][p] = a[p][rr] = c * arp - s * arq;
                    a[rr][qq] = a[qq][rr] = s * arp + c * arq;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const double vp = v[i][p], vq = v[i][qq];
                        v[i][p] = c * vp - s * vq;
                        v[i][qq] = s * vp + c * vq;
                    }
                }
            }
        }
        const double lmax = fmax(a[0][0], fmax(a[1][1], a[2][2]));
        if (lmax > 0.0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double lam = a[j][j];
                if (lam > 1e-3 * lmax) {
                    const double w = ((v[0][j] * r[0] + v[1][j] * r[1]) + v[2][j] * r[2]) / lam;
#pragma unroll
                    for (int i = 0; i < 3; ++i) x[i] = x[i] + v[i][j] * w;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double half = 0.5 * u.g.cell[i];
        const double xi = x[i] == x[i] ? fmin(fmax(x[i], -half), half) : m[i];
        u.out[3 * o + i] = (float)(cc[i] + xi);
    }
}

__global__ __launch_bounds__(kBlock) void means_kernel(const double* __restrict__ vsum, const int* __restrict__ ocl,
                                                      const int* __restrict__ cstart, int K, int64_t Vout, int ncols,
                                                      double* __restrict__ out, int ld, int col0) {
    const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (o >= Vout) return;
    const int k = ocl[o];
    if ((unsigned)k >= (unsigned)K) return;
    const double cnt = (double)(cstart[k + 1] - cstart[k]);
    for (int j = 0; j < ncols; ++j) out[o * ld + col0 + j] = vsum[(int64_t)k * 4 + j] / cnt;
}

// ------------------------------------------------------------------ host side

unsigned blocks(int64_t n) { return ia::blocks(n, kBlock); }

int make_cells(const char* what, const float* lo, const float* inv, const double* cell, const int* dims, Cells& g) {
    IA_REQUIRE(lo && inv && dims, "%s: null pointer (lo, inv_cell, dims)", what);
    for (int a = 0; a < 3; ++a) {
        IA_REQUIRE(dims[a] >= 1 && dims[a] <= kMaxAxis, "%s: dims[%d] = %d is outside [1, 2^20]", what, a, dims[a]);
        IA_REQUIRE(std::isfinite(lo[a]) && std::isfinite(inv[a]) && inv[a] > 0.f, "%s: lo must be finite and inv_cell finite and > 0", what);
        g.n[a] = dims[a];
        g.lo[a] = lo[a];
        g.inv[a] = inv[a];
        g.cell[a] = 1.0;
        if (cell) {
            IA_REQUIRE(std::isfinite(cell[a]) && cell[a] > 0.0, "%s: cell sizes must be finite and > 0", what);
            g.cell[a] = cell[a];
        }
    }
    return IA_OK;
}

int64_t next_level(int64_t n) { return 2 * ia::ceil_div(n, kChunk); }

size_t acc_bytes(int64_t n, int width) {
    const int64_t n1 = n > kChunk ? next_level(n) : 0, n2 = n1 > kChunk ? next_level(n1) : 0;
    return (size_t)(n1 + n2) * (sizeof(double) * width) + (size_t)(n1 + n2 + 2) * sizeof(int);
}

template <int D, int SRC>
int run_accumulate(const char* what, AccArgs u, void* scratch, size_t scratch_bytes, hipStream_t s) {
    const size_t need = acc_bytes(u.n, D);
    if (scratch_bytes < need) return ia::fail(IA_ERR_INVALID_ARG, "%s: scratch holds %zu bytes, needs %zu", what, scratch_bytes, need);
    if (hipMemsetAsync(u.sums, 0, sizeof(double) * D * (size_t)u.K, s) != hipSuccess) return ia::check_launch(what);
    if (u.n == 0) return IA_OK;
    const int64_t n1 = u.n > kChunk ? next_level(u.n) : 0, n2 = n1 > kChunk ? next_level(n1) : 0;
    double* rows[2] = {static_cast<double*>(scratch), static_cast<double*>(scratch) + n1 * D};
    int* segs[2] = {reinterpret_cast<int*>(rows[1] + n2 * D), reinterpret_cast<int*>(rows[1] + n2 * D) + n1};
    u.rows_out = rows[0];
    u.seg_out = segs[0];
    accumulate_kernel<D, SRC><<<blocks(ia::ceil_div(u.n, kChunk)), kBlock, 0, s>>>(u);
    if (int st = ia::check_launch(what)) return st;
    int which = 0;
    while (u.n > kChunk) {
        u.n = next_level(u.n);
        u.seg = segs[which];
        u.rows = rows[which];
        which ^= 1;
        u.seg_out = segs[which];
        u.rows_out = rows[which];
        accumulate_kernel<D, 0><<<blocks(ia::ceil_div(u.n, kChunk)), kBlock, 0, s>>>(u);
        if (int st = ia::check_launch(what)) return st;
    }
    return IA_OK;
}

}  // namespace

extern "C" int ia_simplify_plan(const float* h_lo, const float* h_hi, const int* h_cells, int cells_long, double cell_size, int* h_dims,
                                float* h_inv_cell, double* h_cell) {
    IA_REQUIRE(h_lo && h_hi && h_dims && h_inv_cell && h_cell, "ia_simplify_plan: null pointer (lo, hi, dims, inv_cell, cell)");
    const int given = (h_cells ? 1 : 0) + (cells_long != 0 ? 1 : 0) + (cell_size != 0.0 ? 1 : 0);
    IA_REQUIRE(given == 1, "ia_simplify_plan: exactly one of cells[3], cells_long and cell_size must be given");
    double ext[3], longest = 0.0;
    for (int a = 0; a < 3; ++a) {
        IA_REQUIRE(std::isfinite(h_lo[a]) && std::isfinite(h_hi[a]) && h_hi[a] >= h_lo[a], "ia_simplify_plan: the box must be finite with hi >= lo");
        ext[a] = (double)h_hi[a] - (double)h_lo[a];
        longest = ext[a] > longest ? ext[a] : longest;
    }
    for (int a = 0; a < 3; ++a) {
        double h, n;
        if (h_cells) {
            IA_REQUIRE(h_cells[a] >= 1 && h_cells[a] <= kMaxAxis, "ia_simplify_plan: cells[%d] = %d is outside [1, 2^20]", a, h_cells[a]);
            n = (double)h_cells[a];
            h = ext[a] > 0.0 ? ext[a] / n : 1.0;
        } else {
            if (cells_long) {
                IA_REQUIRE(cells_long >= 1 && cells_long <= kMaxAxis, "ia_simplify_plan: cells = %d is outside [1, 2^20]", cells_long);
                h = longest > 0.0 ? longest / (double)cells_long : 1.0;
            } else {
                IA_REQUIRE(std::isfinite(cell_size) && cell_size > 0.0, "ia_simplify_plan: cell_size must be finite and > 0");
                h = cell_size;
            }
            n = std::ceil(ext[a] / h);
            n = n < 1.0 ? 1.0 : n;
            if (cells_long && longest > 0.0 && ext[a] == longest) n = (double)cells_long;
        }
        IA_REQUIRE(n <= (double)kMaxAxis, "ia_simplify_plan: more than 2^20 cells along axis %d", a);
        const float inv = (float)(1.0 / h);
        IA_REQUIRE(std::isfinite(inv) && inv > 0.f, "ia_simplify_plan: the cell size %g has no fp32 inverse", h);
        h_dims[a] = (int)n;
        h_inv_cell[a] = inv;
        h_cell[a] = h;
    }
    return IA_OK;
}

extern "C" int ia_simplify_box(const float* verts, int64_t V, void* scratch, size_t scratch_bytes, float* box, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount, "ia_simplify_box: V must be in [0, 2^28], got %lld", (long long)V);
    const size_t need = sizeof(float) * 6 * kBoxBlocks;
    if (scratch_bytes < need) return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_box: scratch holds %zu bytes, needs %zu", scratch_bytes, need);
    if ((V && !on_device(verts)) || !on_device(scratch) || !on_device(box))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_box: verts, scratch and box must be device pointers");
    const int nb = (int)std::min<int64_t>(kBoxBlocks, ia::ceil_div(V < 1 ? 1 : V, kBlock));
    hipStream_t s = (hipStream_t)stream;
    box_kernel<<<nb, kBlock, 0, s>>>(verts, V, static_cast<float*>(scratch));
    if (int st = ia::check_launch("ia_simplify_box")) return st;
    box_final_kernel<<<1, 64, 0, s>>>(static_cast<const float*>(scratch), nb, box);
    return ia::check_launch("ia_simplify_box (final)");
}

extern "C" int ia_simplify_keys(const float* verts, int64_t V, const float* h_lo, const float* h_inv_cell, const int* h_dims, int64_t* keys,
                                void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount, "ia_simplify_keys: V must be in [0, 2^28], got %lld", (long long)V);
    Cells g{};
    if (int st = make_cells("ia_simplify_keys", h_lo, h_inv_cell, nullptr, h_dims, g)) return st;
    if (V == 0) return IA_OK;
    if (!on_device(verts) || !on_device(keys)) return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_keys: verts and keys must be device pointers");
    keys_kernel<<<blocks(V), kBlock, 0, (hipStream_t)stream>>>(verts, V, g, keys);
    return ia::check_launch("ia_simplify_keys");
}

extern "C" int ia_simplify_clusters(const int64_t* sorted_keys, const int64_t* order, int64_t V, int* vert_cluster, int* sorted_cluster,
                                    int* cluster_start, int64_t* cluster_key, int64_t capacity, void* scratch, size_t scratch_bytes, int* count,
                                    void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount, "ia_simplify_clusters: V must be in [0, 2^28], got %lld", (long long)V);
    IA_REQUIRE(capacity >= 0, "ia_simplify_clusters: capacity must be >= 0");
    const size_t need = sizeof(int) * ((size_t)V + 1);
    if (scratch_bytes < need) return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_clusters: scratch holds %zu bytes, needs %zu", scratch_bytes, need);
    if (!on_device(count) || !on_device(cluster_start)) return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_clusters: count and cluster_start must be device pointers");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, 2 * sizeof(int), s) != hipSuccess || hipMemsetAsync(cluster_start, 0, sizeof(int), s) != hipSuccess)
        return ia::check_launch("ia_simplify_clusters (clear)");
    if (V == 0) return IA_OK;
    if (!on_device(sorted_keys) || !on_device(order) || !on_device(vert_cluster) || !on_device(sorted_cluster) || !on_device(scratch) ||
        (capacity && !on_device(cluster_key)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_clusters: keys, order, clusters and scratch must be device pointers");
    int* flags = static_cast<int*>(scratch);
    key_heads_kernel<<<blocks(V), kBlock, 0, s>>>(sorted_keys, V, flags);
    if (int st = ia::check_launch("ia_simplify_clusters (heads)")) return st;
    scan_kernel<<<1, kScanBlock, 0, s>>>(flags, flags, V);
    if (int st = ia::check_launch("ia_simplify_clusters (scan)")) return st;
    ClusterArgs u{sorted_keys, order, V, flags, vert_cluster, sorted_cluster, cluster_start, cluster_key, capacity, count};
    clusters_kernel<<<blocks(V), kBlock, 0, s>>>(u);
    return ia::check_launch("ia_simplify_clusters");
}

extern "C" int ia_simplify_classify(const int* faces, int64_t F, int64_t V, const int* vert_cluster, int K, int* tri, int64_t* key, int* ref,
                                    int* pairs, int* count, void* stream) {
    IA_REQUIRE(F >= 0 && F <= kMaxCount && V >= 0 && V <= kMaxCount && K >= 0 && K <= V,
               "ia_simplify_classify: F, V in [0, 2^28] and 0 <= K <= V, got F = %lld, V = %lld, K = %d", (long long)F, (long long)V, K);
    if (!on_device(count)) return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_classify: count must be a device pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, 3 * sizeof(int), s) != hipSuccess) return ia::check_launch("ia_simplify_classify (clear)");
    if (ref && K) {
        if (!on_device(ref)) return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_classify: ref must be a device pointer");
        if (hipMemsetAsync(ref, 0, sizeof(int) * (size_t)K, s) != hipSuccess) return ia::check_launch("ia_simplify_classify (clear)");
    }
    if (F == 0) return IA_OK;
    if (!on_device(faces) || (V && !on_device(vert_cluster)) || !on_device(tri) || !on_device(key) || (pairs && !on_device(pairs)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_classify: faces, vert_cluster, tri, key and pairs must be device pointers");
    const int wide = (double)K * (double)K * (double)K >= 9.0e18 ? 1 : 0;
    ClassifyArgs u{faces, F, V, vert_cluster, K, wide, tri, key, K ? ref : nullptr, pairs, count};
    classify_kernel<<<blocks(F), kBlock, 0, s>>>(u);
    return ia::check_launch("ia_simplify_classify");
}

extern "C" int ia_simplify_face_heads(const int* tri, const int64_t* perm, int64_t F, int* face_pos, void* stream) {
    IA_REQUIRE(F >= 0 && F <= kMaxCount, "ia_simplify_face_heads: F must be in [0, 2^28], got %lld", (long long)F);
    if (!on_device(face_pos)) return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_face_heads: face_pos must be a device pointer");
    hipStream_t s = (hipStream_t)stream;
    if (F == 0) {
        if (hipMemsetAsync(face_pos, 0, sizeof(int), s) != hipSuccess) return ia::check_launch("ia_simplify_face_heads (clear)");
        return IA_OK;
    }
    if (!on_device(tri) || !on_device(perm)) return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_face_heads: tri and perm must be device pointers");
    face_heads_kernel<<<blocks(F), kBlock, 0, s>>>(tri, perm, F, face_pos);
    if (int st = ia::check_launch("ia_simplify_face_heads")) return st;
    scan_kernel<<<1, kScanBlock, 0, s>>>(face_pos, face_pos, F);
    return ia::check_launch("ia_simplify_face_heads (scan)");
}

extern "C" int ia_simplify_refs(const int* ref, int K, int* out_index, void* stream) {
    IA_REQUIRE(K >= 0 && K <= kMaxCount, "ia_simplify_refs: K must be in [0, 2^28], got %d", K);
    if ((K && !on_device(ref)) || !on_device(out_index)) return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_refs: ref and out_index must be device pointers");
    scan_kernel<<<1, kScanBlock, 0, (hipStream_t)stream>>>(ref, out_index, K);
    return ia::check_launch("ia_simplify_refs");
}

extern "C" int ia_simplify_outputs(const int* vert_cluster, int64_t V, const int* ref, const int* out_index, const int* cluster_start, int K,
                                   int64_t* vertex_map, int* out_cluster, int64_t* cluster_size, int64_t capacity, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount && K >= 0 && K <= V && capacity >= 0, "ia_simplify_outputs: V in [0, 2^28], 0 <= K <= V and capacity >= 0");
    if (V == 0) return IA_OK;
    if (!on_device(vert_cluster) || !on_device(vertex_map) || (K && (!on_device(ref) || !on_device(out_index) || !on_device(cluster_start))) ||
        (capacity && (!on_device(out_cluster) || !on_device(cluster_size))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_outputs: every array must be a device pointer");
    OutArgs u{vert_cluster, V, ref, out_index, cluster_start, K, vertex_map, out_cluster, cluster_size, capacity};
    outputs_kernel<<<blocks(V), kBlock, 0, (hipStream_t)stream>>>(u);
    return ia::check_launch("ia_simplify_outputs");
}

extern "C" int ia_simplify_faces(const int* tri, const int64_t* perm, const int* face_pos, int64_t F, const int* out_index, int K,
                                 int64_t* faces_out, int64_t capacity, void* stream) {
    IA_REQUIRE(F >= 0 && F <= kMaxCount && K >= 0 && capacity >= 0, "ia_simplify_faces: F in [0, 2^28], K >= 0 and capacity >= 0");
    if (F == 0 || capacity == 0) return IA_OK;
    if (!on_device(tri) || !on_device(perm) || !on_device(face_pos) || !on_device(out_index) || !on_device(faces_out))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_faces: every array must be a device pointer");
    faces_kernel<<<blocks(F), kBlock, 0, (hipStream_t)stream>>>(tri, perm, face_pos, F, out_index, K, faces_out, capacity);
    return ia::check_launch("ia_simplify_faces");
}

extern "C" int ia_simplify_accumulate_scratch_bytes(int64_t n, int width, size_t* h_bytes) {
    IA_REQUIRE(n >= 0 && n <= 3 * kMaxCount && (width == 4 || width == 9), "ia_simplify_accumulate_scratch_bytes: n in [0, 3 * 2^28], width 4 or 9");
    IA_REQUIRE(h_bytes, "ia_simplify_accumulate_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = acc_bytes(n, width);
    return IA_OK;
}

extern "C" int ia_simplify_accumulate_verts(const double* cols, int ld, int col0, int ncols, const int64_t* order, const int* sorted_cluster,
                                            int64_t n, int64_t V, int K, double* sums, void* scratch, size_t scratch_bytes, void* stream) {
    IA_REQUIRE(n >= 0 && n <= V && V <= kMaxCount && K >= 0 && K <= V, "ia_simplify_accumulate_verts: 0 <= n <= V <= 2^28 and 0 <= K <= V");
    IA_REQUIRE(ld >= 1 && col0 >= 0 && ncols >= 1 && ncols <= 4 && col0 + ncols <= ld, "ia_simplify_accumulate_verts: 1 to 4 columns inside the row of %d", ld);
    if (K == 0) return IA_OK;
    if (!on_device(sums) || (n && (!on_device(cols) || !on_device(order) || !on_device(sorted_cluster))) || (acc_bytes(n, 4) && !on_device(scratch)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_accumulate_verts: every array must be a device pointer");
    AccArgs u{};
    u.seg = sorted_cluster; u.n = n; u.K = K; u.sums = sums;
    u.cols = cols; u.ld = ld; u.col0 = col0; u.ncols = ncols; u.order = order; u.V = V;
    return run_accumulate<4, 1>("ia_simplify_accumulate_verts", u, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int ia_simplify_accumulate_faces(const float* verts, int64_t V, const int* faces, int64_t F, const int64_t* pair_order,
                                            const int* sorted_pairs, int64_t n, const int64_t* cluster_key, int K, const float* h_lo,
                                            const float* h_inv_cell, const double* h_cell, const int* h_dims, double* sums, void* scratch,
                                            size_t scratch_bytes, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount && F >= 0 && F <= kMaxCount && n >= 0 && n <= 3 * F && K >= 0 && K <= V,
               "ia_simplify_accumulate_faces: V, F in [0, 2^28], 0 <= n <= 3 F and 0 <= K <= V");
    Cells g{};
    IA_REQUIRE(h_cell, "ia_simplify_accumulate_faces: cell must not be NULL");
    if (int st = make_cells("ia_simplify_accumulate_faces", h_lo, h_inv_cell, h_cell, h_dims, g)) return st;
    if (K == 0) return IA_OK;
    if (!on_device(sums) || !on_device(cluster_key) || (n && (!on_device(verts) || !on_device(faces) || !on_device(pair_order) || !on_device(sorted_pairs))) ||
        (acc_bytes(n, 9) && !on_device(scratch)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_accumulate_faces: every array must be a device pointer");
    AccArgs u{};
    u.seg = sorted_pairs; u.n = n; u.K = K; u.sums = sums;
    u.order = pair_order; u.V = V; u.verts = verts; u.faces = faces; u.F = F; u.ckey = cluster_key; u.g = g;
    return run_accumulate<9, 2>("ia_simplify_accumulate_faces", u, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int ia_simplify_place(const double* vert_sums, const double* quadric_sums, const int* out_cluster, const int* cluster_start,
                                 const int64_t* cluster_key, int K, int64_t n_out, const float* h_lo, const float* h_inv_cell,
                                 const double* h_cell, const int* h_dims, float* verts_out, int64_t capacity, void* stream) {
    IA_REQUIRE(K >= 0 && n_out >= 0 && n_out <= K, "ia_simplify_place: 0 <= n_out <= K, got n_out = %lld, K = %d", (long long)n_out, K);
    IA_REQUIRE(capacity >= n_out, "ia_simplify_place: verts_out holds %lld vertices, needs %lld", (long long)capacity, (long long)n_out);
    Cells g{};
    IA_REQUIRE(h_cell, "ia_simplify_place: cell must not be NULL");
    if (int st = make_cells("ia_simplify_place", h_lo, h_inv_cell, h_cell, h_dims, g)) return st;
    if (n_out == 0) return IA_OK;
    if (!on_device(vert_sums) || (quadric_sums && !on_device(quadric_sums)) || !on_device(out_cluster) || !on_device(cluster_start) ||
        !on_device(cluster_key) || !on_device(verts_out))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_place: every array must be a device pointer");
    PlaceArgs u{vert_sums, quadric_sums, out_cluster, cluster_start, cluster_key, K, n_out, g, verts_out};
    place_kernel<<<blocks(n_out), kBlock, 0, (hipStream_t)stream>>>(u);
    return ia::check_launch("ia_simplify_place");
}

extern "C" int ia_simplify_means(const double* vert_sums, const int* out_cluster, const int* cluster_start, int K, int64_t n_out, int ncols,
                                 double* out, int ld, int col0, int64_t capacity, void* stream) {
    IA_REQUIRE(K >= 0 && n_out >= 0 && n_out <= K, "ia_simplify_means: 0 <= n_out <= K, got n_out = %lld, K = %d", (long long)n_out, K);
    IA_REQUIRE(ld >= 1 && col0 >= 0 && ncols >= 1 && ncols <= 4 && col0 + ncols <= ld, "ia_simplify_means: 1 to 4 columns inside the row of %d", ld);
    IA_REQUIRE(capacity >= n_out, "ia_simplify_means: out holds %lld rows, needs %lld", (long long)capacity, (long long)n_out);
    if (n_out == 0) return IA_OK;
    if (!on_device(vert_sums) || !on_device(out_cluster) || !on_device(cluster_start) || !on_device(out))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_simplify_means: every array must be a device pointer");
    means_kernel<<<blocks(n_out), kBlock, 0, (hipStream_t)stream>>>(vert_sums, out_cluster, cluster_start, K, n_out, ncols, out, ld, col0);
    return ia::check_launch("ia_simplify_means");
}
