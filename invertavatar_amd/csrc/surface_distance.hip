// Distance between surfaces on the device: exact point-to-triangle-mesh distance through a uniform grid of triangle lists, and the
// reductions that turn distance arrays into Chamfer / Hausdorff / F-score numbers.  No counterpart in the reference.
//
// One per-triangle fp32 function, tri_dist, defines every result: the distance of a query point to a mesh is the minimum of tri_dist
// over ALL usable triangles, taken on the pair (distance, index).  The grid only decides which triangles need not be looked at, so
// the answer is bit-identical with the grid, without it (brute mode: the same kernel body walks every triangle), for every grid
// resolution and from run to run; the order in which a cell lists its triangles does not matter.
//
// tri_dist works in coordinates relative to the query point (a = A - p, ...): the minimum of the three clamped point-to-segment
// distances, replaced by the plane distance |n . a| / |n| (n: the cross product of the two shorter edges; with the longest edge in it
// the product cancels on needle-shaped triangles, 42 eps32 * extent measured on the CPU against 2.6 without) when the triangle has an
// area in fp32 (n . n > 0), the origin projects inside (n . (a x (b - a)), n . (b x (c - b)), n . (c x (a - c)) all >= 0) and the
// plane distance is the smaller of the two (a vertex the point coincides with keeps its exact 0).  Every operation is rounded on its own (the project
// builds with -ffp-contract=off), dot products are (x + y) + z: geometry.py restates the same lines in NumPy.  A triangle without
// area is a segment or a point and takes the segment branch; nothing divides by zero.
//
//   pack   : faces -> verts is chased once; a triangle becomes three float4 (A, B, C; A.w = 1 usable, 0 ignored: a non-finite
//            coordinate or an index outside [0, V)).
//   count  : a triangle's bounding box covers a box of cells; it is counted in each of them, or, when these are more than kMaxCells,
//            in the oversize list that every query tests first (so the entry count is at most kMaxCells * F however large a triangle
//            is).  One workgroup then turns the counts into offsets (CSR).  Integer atomics only.
//   fill   : the same traversal writes the triangle indices (cursor = integer atomic add; any order).
//   closest: one thread per query point.  Shells of cells of growing Chebyshev radius r around the point's (clamped) cell; after shell
//            r every triangle not yet seen lies, on some axis, wholly in cells beyond the cube, hence at least `lb` away, where lb is
//            the distance from p to the nearest face of the cube that still has cells behind it, evaluated in double with the cell
//            coordinate moved inward by 2^-21 relative (the fp32 cell function floor((x - lo) * inv) is monotone and two roundings
//            away from exact).  The search stops when best < lb - slack, slack = 64 eps32 * max(|p|, |mesh|) covering the fp32
//            evaluation error of tri_dist itself (7.4 eps32 * extent measured on the hard families): an unseen triangle can then
//            neither beat nor tie the best pair.  When no face has cells behind it the whole grid has been seen.
//   stats  : finite count, sum, sum of squares, max, sum |n_a . n_b|, non-finite count and counts <= t for up to 8 thresholds, in
//            double per thread, wave and workgroup in a fixed order; a second launch adds the workgroups' slots in index order.  No
//            floating-point atomics: bit-equal from run to run.
#include "geom_common.h"

#include <cmath>

namespace {

using ia::blocks; using ia::cell_of; using ia::kScanBlock; using ia::on_device; using ia::wave_max; using ia::wave_sum;

constexpr int kBlock = 256;
constexpr int kMaxCells = 64;                        // a triangle that covers more cells goes to the oversize list
constexpr int kMaxAxis = 1024;                       // cells per axis
constexpr int64_t kMaxGridCells = (int64_t)1 << 26;
constexpr int64_t kMaxFaces = (int64_t)1 << 25;      // kMaxCells * F entries stay below 2^31
constexpr int kMaxThr = 8;
constexpr int kStatVals = 6 + kMaxThr;               // count, sum, sum sq, max, normal sum, non-finite, <= t[0..7]
constexpr int kStatBlocks = 1024;
constexpr int kStatPer = 4;

using V3 = ia::Vec3<float>;                         // sub, dot ((x + y) + z), cross, finite3, tri_dist: geom_common.h

struct Grid {
    const int* cell_start;       // [ncell + 1] offsets into cell_tris; null: brute mode
    const int* cell_tris;        // [entries + n_over]: the cells' lists, then the oversize list
    int nx, ny, nz;
    float lo[3], inv[3];         // cell of x along an axis: clamp(floor((x - lo) * inv), 0, n - 1)
    int entries, n_over;
};

__device__ __forceinline__ V3 xyz(float4 v) { return {v.x, v.y, v.z}; }

__global__ __launch_bounds__(kBlock) void tri_pack_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                         float4* __restrict__ tris) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    float4 A = {0.f, 0.f, 0.f, 0.f}, B = A, C = A;
    if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
        A = {verts[3 * (int64_t)i0], verts[3 * (int64_t)i0 + 1], verts[3 * (int64_t)i0 + 2], 0.f};
        B = {verts[3 * (int64_t)i1], verts[3 * (int64_t)i1 + 1], verts[3 * (int64_t)i1 + 2], 0.f};
        C = {verts[3 * (int64_t)i2], verts[3 * (int64_t)i2 + 1], verts[3 * (int64_t)i2 + 2], 0.f};
        A.w = finite3(xyz(A)) && finite3(xyz(B)) && finite3(xyz(C)) ? 1.f : 0.f;
    }
    tris[3 * f] = A;
    tris[3 * f + 1] = B;
    tris[3 * f + 2] = C;
}

struct CellBox { int x0, x1, y0, y1, z0, z1; int64_t cells; };

__device__ __forceinline__ CellBox cell_box(const Grid& g, float4 A, float4 B, float4 C) {
    CellBox r;
    r.x0 = cell_of(fminf(A.x, fminf(B.x, C.x)), g.lo[0], g.inv[0], g.nx);
    r.x1 = cell_of(fmaxf(A.x, fmaxf(B.x, C.x)), g.lo[0], g.inv[0], g.nx);
    r.y0 = cell_of(fminf(A.y, fminf(B.y, C.y)), g.lo[1], g.inv[1], g.ny);
    r.y1 = cell_of(fmaxf(A.y, fmaxf(B.y, C.y)), g.lo[1], g.inv[1], g.ny);
    r.z0 = cell_of(fminf(A.z, fminf(B.z, C.z)), g.lo[2], g.inv[2], g.nz);
    r.z1 = cell_of(fmaxf(A.z, fmaxf(B.z, C.z)), g.lo[2], g.inv[2], g.nz);
    r.cells = (int64_t)(r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1) * (r.z1 - r.z0 + 1);
    return r;
}

// FILL = false: counts[cell] += 1 (counts[ncell + 1] for an oversize triangle).  FILL = true: the triangle's index goes to its cells'
// lists at start[cell] + cursor[cell]++, an oversize one to entries + cursor[ncell]++.
template <bool FILL>
__global__ __launch_bounds__(kBlock) void trigrid_pass_kernel(Grid g, const float4* __restrict__ tris, int F, int* counts, int* cursor,
                                                             int* __restrict__ cell_tris, int64_t capacity) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= F) return;
    const float4 A = tris[3 * f], B = tris[3 * f + 1], C = tris[3 * f + 2];
    if (A.w == 0.f) return;
    const CellBox r = cell_box(g, A, B, C);
    const int ncell = g.nx * g.ny * g.nz;
    if (r.cells > kMaxCells) {
        if (!FILL) { atomicAdd(counts + ncell + 1, 1); return; }
        const int64_t at = (int64_t)g.entries + atomicAdd(cursor + ncell, 1);
        if (at < capacity) cell_tris[at] = (int)f;
        return;
    }
    for (int ix = r.x0; ix <= r.x1; ++ix)
        for (int iy = r.y0; iy <= r.y1; ++iy)
            for (int iz = r.z0; iz <= r.z1; ++iz) {
                const int c = (ix * g.ny + iy) * g.nz + iz;
                if (!FILL) { atomicAdd(counts + c, 1); continue; }
                const int at = g.cell_start[c] + atomicAdd(cursor + c, 1);
                if (at < g.cell_start[c + 1] && at < capacity) cell_tris[at] = (int)f;
            }
}

// One workgroup: counts[0 .. n) -> exclusive offsets in place, counts[n] = total.
__global__ __launch_bounds__(kScanBlock) void trigrid_scan_kernel(int* counts, int n) {
    const int total = ia::scan_workgroup<int>(counts, counts, n);
    if (threadIdx.x == 0) counts[n] = total;
}

struct Query {
    const float* pts;
    int64_t N;
    const float4* tris;
    int F;
    float mesh_extent;           // largest |coordinate| of the usable triangles
    float* dist;
    int* face;
    float* point;
};

__global__ __launch_bounds__(kBlock) void closest_kernel(Query u, Grid g) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= u.N) return;
    const V3 p = {u.pts[3 * i], u.pts[3 * i + 1], u.pts[3 * i + 2]};
    float best = INFINITY;
    int bi = -1;
    if (!finite3(p)) {
        u.dist[i] = NAN;
        u.face[i] = -1;
        u.point[3 * i] = u.point[3 * i + 1] = u.point[3 * i + 2] = NAN;
        return;
    }
    auto visit = [&](int t) {
        if ((unsigned)t >= (unsigned)u.F) return;
        const float4 A = u.tris[3 * (int64_t)t], B = u.tris[3 * (int64_t)t + 1], C = u.tris[3 * (int64_t)t + 2];
        if (A.w == 0.f) return;
        V3 q;
        const float d = tri_dist(p, xyz(A), xyz(B), xyz(C), q);
        if (d < best || (d == best && t < bi)) { best = d; bi = t; }          // the minimum of the pair (distance, index)
    };
    if (!g.cell_start) {
        for (int t = 0; t < u.F; ++t) visit(t);
    } else {
        for (int k = 0; k < g.n_over; ++k) visit(g.cell_tris[g.entries + k]);
        auto visit_cell = [&](int ix, int iy, int iz) {
            const int c = (ix * g.ny + iy) * g.nz + iz;
            const int e1 = min(g.cell_start[c + 1], g.entries);
            for (int e = max(g.cell_start[c], 0); e < e1; ++e) visit(g.cell_tris[e]);
        };
        const int cx = cell_of(p.x, g.lo[0], g.inv[0], g.nx), cy = cell_of(p.y, g.lo[1], g.inv[1], g.ny),
                  cz = cell_of(p.z, g.lo[2], g.inv[2], g.nz);
        const int rmax = max(max(max(cx, g.nx - 1 - cx), max(cy, g.ny - 1 - cy)), max(cz, g.nz - 1 - cz));
        const double extent = fmax((double)u.mesh_extent, fmax(fabs((double)p.x), fmax(fabs((double)p.y), fabs((double)p.z))));
        const double slack = 64.0 * 1.1920928955078125e-7 * extent;
        const double in = 1.0 - 4.76837158203125e-7, out = 1.0 + 4.76837158203125e-7;       // 1 -+ 2^-21
        const int cc[3] = {cx, cy, cz}, nn[3] = {g.nx, g.ny, g.nz};
        const double pp[3] = {p.x, p.y, p.z};
        for (int r = 0; r <= rmax; ++r) {
            const int x0 = max(cx - r, 0), x1 = min(cx + r, g.nx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
            for (int ix = x0; ix <= x1; ++ix)
                for (int iy = y0; iy <= y1; ++iy) {
                    if (abs(ix - cx) == r || abs(iy - cy) == r) {
                        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1);
                        for (int iz = z0; iz <= z1; ++iz) visit_cell(ix, iy, iz);
                    } else {
                        if (cz - r >= 0) visit_cell(ix, iy, cz - r);
                        if (cz + r <= g.nz - 1) visit_cell(ix, iy, cz + r);
                    }
                }
            // every triangle not yet seen lies, on some axis, in cells >= c + r + 1 or <= c - r - 1 only
            double lb = INFINITY;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double cs = 1.0 / (double)g.inv[a], lo = (double)g.lo[a];
                const int up = cc[a] + r + 1, dn = cc[a] - r;
                if (up <= nn[a] - 1) lb = fmin(lb, (lo + (double)up * cs * in) - pp[a]);
                if (dn >= 1) lb = fmin(lb, pp[a] - (lo + (double)dn * cs * out));
            }
            if ((double)best < lb - slack) break;
        }
    }
    V3 q = {NAN, NAN, NAN};
    if (bi >= 0) {
        const float4 A = u.tris[3 * (int64_t)bi], B = u.tris[3 * (int64_t)bi + 1], C = u.tris[3 * (int64_t)bi + 2];
        tri_dist(p, xyz(A), xyz(B), xyz(C), q);
    }
    u.dist[i] = best;
    u.face[i] = bi;
    u.point[3 * i] = p.x + q.x;
    u.point[3 * i + 1] = p.y + q.y;
    u.point[3 * i + 2] = p.z + q.z;
}

// ------------------------------------------------------------------ statistics

struct StatArgs {
    const float* dist;
    int64_t N;
    float thr[kMaxThr];
    int n_thr;
    const int* face;             // with normals: closest face per entry
    const float* na;             // [N,3] normal of the entry's own sample
    const float* nb;             // [Fb,3] face normals of the other side
    int Fb;
    double* slots;               // [blocks][kStatVals]
    int blocks;
};

__global__ __launch_bounds__(kBlock) void stats_kernel(StatArgs s) {
    double acc[kStatVals];
#pragma unroll
    for (int k = 0; k < kStatVals; ++k) acc[k] = 0.0;
    acc[3] = -INFINITY;
    const int64_t stride = (int64_t)s.blocks * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < s.N; i += stride) {
        const float df = s.dist[i];
        if (!isfinite(df)) { acc[5] += 1.0; continue; }
        const double d = (double)df;
        acc[0] += 1.0;
        acc[1] += d;
        acc[2] += d * d;
        acc[3] = fmax(acc[3], d);
        if (s.face) {
            const int f = s.face[i];
            if ((unsigned)f < (unsigned)s.Fb) {
                const double x = (double)s.na[3 * i] * (double)s.nb[3 * (int64_t)f], y = (double)s.na[3 * i + 1] * (double)s.nb[3 * (int64_t)f + 1],
                             z = (double)s.na[3 * i + 2] * (double)s.nb[3 * (int64_t)f + 2];
                acc[4] += fabs((x + y) + z);
            }
        }
#pragma unroll
        for (int k = 0; k < kMaxThr; ++k) acc[6 + k] += (k < s.n_thr && df <= s.thr[k]) ? 1.0 : 0.0;
    }
    __shared__ double part[kBlock / 64][kStatVals];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kStatVals; ++k) {
        const double v = k == 3 ? wave_max(acc[k]) : wave_sum(acc[k]);
        if (lane == 0) part[w][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kStatVals) {
        const int k = threadIdx.x;
        double v = part[0][k];
        for (int j = 1; j < kBlock / 64; ++j) v = k == 3 ? fmax(v, part[j][k]) : v + part[j][k];
        s.slots[(int64_t)blockIdx.x * kStatVals + k] = v;
    }
}

__global__ __launch_bounds__(64) void stats_final_kernel(const double* __restrict__ slots, int blocks, double* __restrict__ out) {
    const int k = threadIdx.x;
    if (k >= kStatVals) return;
    double v = slots[k];
    for (int b = 1; b < blocks; ++b) v = k == 3 ? fmax(v, slots[(int64_t)b * kStatVals + k]) : v + slots[(int64_t)b * kStatVals + k];
    out[k] = v;
}

// ------------------------------------------------------------------ host side

int stat_blocks(int64_t n) {
    const int64_t b = ia::ceil_div(n < 1 ? 1 : n, (int64_t)kBlock * kStatPer);
    return (int)(b > kStatBlocks ? kStatBlocks : b);
}

int make_grid(const char* what, const float* lo, const float* inv, const int* dims, Grid& g) {
    IA_REQUIRE(lo && inv && dims, "%s: lo, inv_cell and dims must not be NULL", what);
    for (int a = 0; a < 3; ++a) {
        IA_REQUIRE(dims[a] >= 1 && dims[a] <= kMaxAxis, "%s: dims[%d] = %d is outside [1, %d]", what, a, dims[a], kMaxAxis);
        IA_REQUIRE(std::isfinite(lo[a]) && std::isfinite(inv[a]) && inv[a] > 0.f, "%s: lo must be finite and inv_cell finite and > 0", what);
        g.lo[a] = lo[a];
        g.inv[a] = inv[a];
    }
    IA_REQUIRE((int64_t)dims[0] * dims[1] * dims[2] <= kMaxGridCells, "%s: %d x %d x %d cells are more than 2^26", what, dims[0], dims[1],
               dims[2]);
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
    return IA_OK;
}

}  // namespace

extern "C" int ia_tri_pack(const float* verts, int V, const int* faces, int64_t F, void* tris, void* stream) {
    IA_REQUIRE(V >= 0 && F >= 0 && F <= kMaxFaces, "ia_tri_pack: V and F must be >= 0 and F <= 2^25, got V = %d, F = %lld", V, (long long)F);
    if (F == 0) return IA_OK;
    if ((V && !on_device(verts)) || !on_device(faces) || !on_device(tris))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_tri_pack: verts, faces and tris must be device pointers");
    tri_pack_kernel<<<blocks(F, kBlock), kBlock, 0, (hipStream_t)stream>>>(verts, V, faces, (int)F, static_cast<float4*>(tris));
    return ia::check_launch("ia_tri_pack");
}

extern "C" int ia_trigrid_plan(int64_t F, const float* h_lo, const float* h_hi, const int* h_request, int* h_dims, float* h_inv_cell) {
    IA_REQUIRE(F >= 0 && F <= kMaxFaces, "ia_trigrid_plan: F must be in [0, 2^25], got %lld", (long long)F);
    IA_REQUIRE(h_lo && h_hi && h_dims && h_inv_cell, "ia_trigrid_plan: null pointer (lo, hi, dims, inv_cell)");
    double ext[3], vol = 1.0;
    int nz_axes = 0;
    for (int a = 0; a < 3; ++a) {
        IA_REQUIRE(std::isfinite(h_lo[a]) && std::isfinite(h_hi[a]) && h_hi[a] >= h_lo[a], "ia_trigrid_plan: the box must be finite with hi >= lo");
        ext[a] = (double)h_hi[a] - (double)h_lo[a];
        if (ext[a] > 0.0) { vol *= ext[a]; ++nz_axes; }
    }
    // about one cell per triangle, cubic cells over the axes that have an extent
    const double target = F < 1 ? 1.0 : (double)F;
    const double cell = nz_axes ? std::pow(vol / target, 1.0 / nz_axes) : 1.0;
    int64_t total = 1;
    for (int a = 0; a < 3; ++a) {
        int n = 1;
        if (h_request && h_request[a] > 0) {
            IA_REQUIRE(h_request[a] <= kMaxAxis, "ia_trigrid_plan: at most %d cells per axis, got %d", kMaxAxis, h_request[a]);
            n = h_request[a];
        } else if (ext[a] > 0.0) {
            const double want = std::ceil(ext[a] / cell);
            n = want < 1.0 ? 1 : (want > 256.0 ? 256 : (int)want);
        }
        h_dims[a] = n;
        total *= n;
    }
    IA_REQUIRE(total <= kMaxGridCells, "ia_trigrid_plan: %lld cells are more than 2^26", (long long)total);
    for (int a = 0; a < 3; ++a) {
        // the last cell ends a little beyond hi, so that hi itself is not clamped
        const float inv = ext[a] > 0.0 ? (float)((double)h_dims[a] / (ext[a] * (1.0 + 1e-6))) : 1.f;
        h_inv_cell[a] = std::isfinite(inv) && inv > 0.f ? inv : 1.f;
    }
    return IA_OK;
}

extern "C" int ia_trigrid_count(const void* tris, int64_t F, const float* h_lo, const float* h_inv_cell, const int* h_dims, int* cell_start,
                                void* stream) {
    IA_REQUIRE(F >= 0 && F <= kMaxFaces, "ia_trigrid_count: F must be in [0, 2^25], got %lld", (long long)F);
    Grid g{};
    if (int st = make_grid("ia_trigrid_count", h_lo, h_inv_cell, h_dims, g)) return st;
    if ((F && !on_device(tris)) || !on_device(cell_start))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_trigrid_count: tris and cell_start must be device pointers");
    const int ncell = g.nx * g.ny * g.nz;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(cell_start, 0, sizeof(int) * ((size_t)ncell + 2), s) != hipSuccess) return ia::check_launch("ia_trigrid_count (clear)");
    if (F) {
        trigrid_pass_kernel<false><<<blocks(F, kBlock), kBlock, 0, s>>>(g, static_cast<const float4*>(tris), (int)F, cell_start, nullptr,
                                                                       nullptr, 0);
        if (int st = ia::check_launch("ia_trigrid_count (count)")) return st;
    }
    trigrid_scan_kernel<<<1, kScanBlock, 0, s>>>(cell_start, ncell);
    return ia::check_launch("ia_trigrid_count (scan)");
}

extern "C" int ia_trigrid_fill(const void* tris, int64_t F, const float* h_lo, const float* h_inv_cell, const int* h_dims, const int* cell_start,
                               int entries, int n_over, void* scratch, size_t scratch_bytes, int* cell_tris, void* stream) {
    IA_REQUIRE(F >= 0 && F <= kMaxFaces, "ia_trigrid_fill: F must be in [0, 2^25], got %lld", (long long)F);
    IA_REQUIRE(entries >= 0 && n_over >= 0 && (int64_t)entries <= kMaxCells * F && n_over <= F,
               "ia_trigrid_fill: entries = %d, n_over = %d are not counts of a grid of %lld triangles", entries, n_over, (long long)F);
    Grid g{};
    if (int st = make_grid("ia_trigrid_fill", h_lo, h_inv_cell, h_dims, g)) return st;
    const int ncell = g.nx * g.ny * g.nz;
    const size_t need = sizeof(int) * ((size_t)ncell + 1);
    if (scratch_bytes < need) return ia::fail(IA_ERR_INVALID_ARG, "ia_trigrid_fill: scratch holds %zu bytes, needs %zu", scratch_bytes, need);
    if ((F && !on_device(tris)) || !on_device(cell_start) || !on_device(scratch) || ((entries + n_over) && !on_device(cell_tris)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_trigrid_fill: tris, cell_start, scratch and cell_tris must be device pointers");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(scratch, 0, need, s) != hipSuccess) return ia::check_launch("ia_trigrid_fill (clear)");
    if (!F) return IA_OK;
    g.cell_start = cell_start;
    g.entries = entries;
    g.n_over = n_over;
    trigrid_pass_kernel<true><<<blocks(F, kBlock), kBlock, 0, s>>>(g, static_cast<const float4*>(tris), (int)F, nullptr,
                                                                  static_cast<int*>(scratch), cell_tris, (int64_t)entries + n_over);
    return ia::check_launch("ia_trigrid_fill");
}

extern "C" int ia_closest_point(const float* points, int64_t N, const void* tris, int64_t F, float mesh_extent, const float* h_lo,
                                const float* h_inv_cell, const int* h_dims, const int* cell_start, const int* cell_tris, int entries, int n_over,
                                float* dist, int* face, float* point, void* stream) {
    IA_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) / 3, "ia_closest_point: N must be >= 0 and 3 N < 2^31, got %lld", (long long)N);
    IA_REQUIRE(F >= 0 && F <= kMaxFaces, "ia_closest_point: F must be in [0, 2^25], got %lld", (long long)F);
    IA_REQUIRE(mesh_extent >= 0.f && std::isfinite(mesh_extent), "ia_closest_point: mesh_extent must be finite and >= 0");
    Grid g{};
    if (cell_start) {
        if (int st = make_grid("ia_closest_point", h_lo, h_inv_cell, h_dims, g)) return st;
        IA_REQUIRE(entries >= 0 && n_over >= 0 && (int64_t)entries <= kMaxCells * F && n_over <= F,
                   "ia_closest_point: entries = %d, n_over = %d are not counts of a grid of %lld triangles", entries, n_over, (long long)F);
        if (!on_device(cell_start) || ((entries + n_over) && !on_device(cell_tris)))
            return ia::fail(IA_ERR_INVALID_ARG, "ia_closest_point: cell_start and cell_tris must be device pointers");
        g.cell_start = cell_start;
        g.cell_tris = cell_tris;
        g.entries = entries;
        g.n_over = n_over;
    }
    if (N == 0) return IA_OK;
    if (!on_device(points) || (F && !on_device(tris)) || !on_device(dist) || !on_device(face) || !on_device(point))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_closest_point: points, tris, dist, face and point must be device pointers");
    Query u{points, N, static_cast<const float4*>(tris), (int)F, mesh_extent, dist, face, point};
    closest_kernel<<<blocks(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(u, g);
    return ia::check_launch("ia_closest_point");
}

extern "C" int ia_distance_stats_scratch_bytes(int64_t N, size_t* h_bytes) {
    IA_REQUIRE(N >= 0, "ia_distance_stats_scratch_bytes: N must be >= 0");
    IA_REQUIRE(h_bytes, "ia_distance_stats_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = sizeof(double) * kStatVals * (size_t)stat_blocks(N);
    return IA_OK;
}

extern "C" int ia_distance_stats(const float* dist, int64_t N, const float* h_thresholds, int n_thresholds, const int* face,
                                 const float* normals_a, const float* normals_b, int64_t Fb, void* scratch, size_t scratch_bytes, double* out,
                                 void* stream) {
    IA_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) / 3, "ia_distance_stats: N must be >= 0 and 3 N < 2^31, got %lld", (long long)N);
    IA_REQUIRE(n_thresholds >= 0 && n_thresholds <= kMaxThr && (n_thresholds == 0 || h_thresholds),
               "ia_distance_stats: 0 to %d thresholds (a host array), got %d", kMaxThr, n_thresholds);
    IA_REQUIRE(Fb >= 0 && Fb <= kMaxFaces, "ia_distance_stats: Fb must be in [0, 2^25]");
    const bool normals = face || normals_a || normals_b;
    const int nb = stat_blocks(N);
    const size_t need = sizeof(double) * kStatVals * (size_t)nb;
    if (scratch_bytes < need) return ia::fail(IA_ERR_INVALID_ARG, "ia_distance_stats: scratch holds %zu bytes, needs %zu", scratch_bytes, need);
    if ((N && !on_device(dist)) || !on_device(scratch) || !on_device(out))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_distance_stats: dist, scratch and out must be device pointers");
    if (normals && N && (!on_device(face) || !on_device(normals_a) || (Fb && !on_device(normals_b))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_distance_stats: face, normals_a and normals_b go together and must be device pointers");
    StatArgs s{};
    s.dist = dist;
    s.N = N;
    for (int k = 0; k < kMaxThr; ++k) s.thr[k] = k < n_thresholds ? h_thresholds[k] : 0.f;
    s.n_thr = n_thresholds;
    s.face = normals ? face : nullptr;
    s.na = normals_a;
    s.nb = normals_b;
    s.Fb = (int)Fb;
    s.slots = static_cast<double*>(scratch);
    s.blocks = nb;
    hipStream_t st = (hipStream_t)stream;
    stats_kernel<<<nb, kBlock, 0, st>>>(s);
    if (int e = ia::check_launch("ia_distance_stats")) return e;
    stats_final_kernel<<<1, 64, 0, st>>>(s.slots, nb, out);
    return ia::check_launch("ia_distance_stats (final)");
}
