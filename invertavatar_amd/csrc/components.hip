// Connected components on the device: labelling of {volume > level} on a lattice, per-component statistics, the filter that drops
// components from a volume, and the same labelling for the vertices of an indexed triangle mesh.  No counterpart in the reference.
//
// Union-find in which a parent is always a SMALLER linear index than its child, so the root of a finished component is its smallest
// index whatever order the unions arrive in.  Unions hook the larger root under the smaller with an integer atomic min; every loop
// strictly descends (parents only decrease, indices are >= 0), so every launch terminates under any scheduling of its workgroups:
// nobody waits for anybody.
//
//   tile     : one workgroup per 8 x 8 x 64 tile (z along the lanes).  Runs along z are found with a ballot, the remaining forward
//              neighbours inside the tile are united in LDS; parents leave as global linear indices (-1: outside).
//   seam     : forward neighbours that lie in another tile are united on the global parent array.  EVERY access to that array in this
//              launch is a relaxed agent-scope atomic: a parent written by a workgroup on another XCD is not seen by a plain load.
//   shortcut : tile roots that were hooked into another tile jump to their root (one walk per tile root instead of one per point).
//   flatten  : every point finds its root (the array is read-only in this launch) and the roots per 1024-point chunk are counted;
//   scan     : one workgroup turns the chunk counts into offsets and writes K;
//   rank     : root r receives its 0-based rank in index order; relabel: label = rank of the root + 1 (0 outside).
//
// Which pairs are united (pairs(), shared by tile and seam): a pair (p, q = p + (dx, dy, 0)) is skipped when p-1 and q-1 (one step
// back along z) are both inside, because that pair is united on behalf of p-1 and the z runs join the rest; the diagonal
// (dx, dy, -1) is skipped when (dx, dy, 0) or p-1 is inside, (dx, dy, +1) when (dx, dy, 0) or p+1 is.  A neighbour whose state a pass
// cannot see (outside the tile, in the tile pass) counts as outside, which only ever adds a redundant union.
//
// Only integer atomics (min on parents; add / min / max in the statistics): labels and statistics are bit-reproducible.
#include "geom_common.h"

#include <climits>

namespace {

using ia::blocks; using ia::check_volume; using ia::kScanBlock; using ia::on_device; using ia::unravel;

constexpr int kBlock = 256;
constexpr int kTX = 8, kTY = 8, kTZ = 64;            // tile: 64 rows of 64 points, 16 rows per wave
constexpr int kRows = kTX * kTY, kTilePts = kRows * kTZ;
constexpr int kPer = 4;                              // consecutive points per thread in the linear passes
constexpr int kChunk = kBlock * kPer;
constexpr int kRun = 8;                              // consecutive items per thread in the statistics

struct CcVol {
    const float* v;
    int nx, ny, nz;
    int64_t S, N;                                    // ny * nz, nx * ny * nz
    float level;
    int conn26;
    int ty, tz;                                      // tiles along y and z
};

#define IA_RLX __ATOMIC_RELAXED
#define IA_AGENT __HIP_MEMORY_SCOPE_AGENT
#define IA_WG __HIP_MEMORY_SCOPE_WORKGROUP

__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, IA_RLX, IA_AGENT); }
__device__ __forceinline__ void g_store(int* p, int v) { __hip_atomic_store(p, v, IA_RLX, IA_AGENT); }

__device__ __forceinline__ int g_find(const int* P, int x) {
    for (int p; (p = g_load(P + x)) != x;) x = p;    // p < x: strictly descending
    return x;
}

// Lock-free union on the global parent array.  After a lost race (old != a) the link a -> old may have been replaced by a -> b, so
// the union continues with (old, b): no connection is ever dropped.
__device__ void g_union(int* P, int a, int b) {
    for (;;) {
        a = g_find(P, a);
        b = g_find(P, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(P + a, b, IA_RLX, IA_AGENT);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ int l_find(const int* L, int x) {
    for (int p; (p = __hip_atomic_load(L + x, IA_RLX, IA_WG)) != x;) x = p;
    return x;
}

__device__ void l_union(int* L, int a, int b) {
    for (;;) {
        a = l_find(L, a);
        b = l_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + a, b, IA_RLX, IA_WG);
        if (old == a) return;
        a = old;
    }
}

// The forward pairs of one inside point (see the head of the file).  in(dx, dy, dz): is that neighbour inside, as far as this pass can
// tell; emit(dx, dy, dz): unite with it.
template <class In, class Emit>
__device__ __forceinline__ void pairs(bool conn26, In in, Emit emit) {
    const bool back = in(0, 0, -1), fwd = in(0, 0, 1);
    if (fwd) emit(0, 0, 1);
    const int cols = conn26 ? 4 : 2;
    for (int c = 0; c < cols; ++c) {
        const int dx = c == 0 ? 0 : 1, dy = c == 0 ? 1 : (c == 1 ? 0 : (c == 2 ? -1 : 1));
        if (in(dx, dy, 0)) {
            if (!(back && in(dx, dy, -1))) emit(dx, dy, 0);
        } else if (conn26) {
            if (!back && in(dx, dy, -1)) emit(dx, dy, -1);
            if (!fwd && in(dx, dy, 1)) emit(dx, dy, 1);
        }
    }
}

__device__ __forceinline__ void tile_origin(const CcVol& m, int& i0, int& j0, int& k0) {
    const unsigned b = blockIdx.x, tz = (unsigned)m.tz, ty = (unsigned)m.ty;
    const unsigned q = b / tz;
    k0 = (int)(b - q * tz) * kTZ;
    i0 = (int)(q / ty) * kTX;
    j0 = (int)(q - (q / ty) * ty) * kTY;
}

__global__ __launch_bounds__(kBlock) void cc_tile_kernel(CcVol m, int* __restrict__ parent) {
    __shared__ int L[kTilePts];
    int i0, j0, k0;
    tile_origin(m, i0, j0, k0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = k0 + lane;
    unsigned mine = 0;                                                  // bit q: my point of row w + 4 q is inside
    for (int q = 0; q < kRows / 4; ++q) {
        const int r = w + 4 * q, i = i0 + (r >> 3), j = j0 + (r & 7);
        const bool ok = i < m.nx && j < m.ny && k < m.nz;
        const bool in = ok && m.v[((int64_t)i * m.ny + j) * m.nz + k] > m.level;       // NaN: outside
        const unsigned long long mask = __ballot(in);
        const unsigned long long zeros = ~mask & ((1ull << lane) - 1ull);            // outside points below me in the row
        const int start = zeros ? 64 - __clzll((long long)zeros) : 0;               // my z run starts here
        L[r * kTZ + lane] = in ? r * kTZ + start : -1;
        mine |= in ? (1u << q) : 0u;
    }
    __syncthreads();
    for (int q = 0; q < kRows / 4; ++q) {
        if (!(mine >> q & 1)) continue;
        const int r = w + 4 * q, lx = r >> 3, ly = r & 7, p = r * kTZ + lane;
        auto at = [&](int dx, int dy, int dz) { return ((lx + dx) * kTY + ly + dy) * kTZ + lane + dz; };
        auto in = [&](int dx, int dy, int dz) {
            const int x = lx + dx, y = ly + dy, z = lane + dz;
            if (x >= kTX || (unsigned)y >= (unsigned)kTY || (unsigned)z >= (unsigned)kTZ) return false;
            return __hip_atomic_load(L + at(dx, dy, dz), IA_RLX, IA_WG) >= 0;       // the sign of an entry never changes
        };
        auto emit = [&](int dx, int dy, int dz) {
            if (dx | dy) l_union(L, p, at(dx, dy, dz));                          // (0,0,1) inside the tile is the run already
        };
        pairs(m.conn26 != 0, in, emit);
    }
    __syncthreads();
    for (int q = 0; q < kRows / 4; ++q) {
        const int r = w + 4 * q, i = i0 + (r >> 3), j = j0 + (r & 7);
        if (!(i < m.nx && j < m.ny && k < m.nz)) continue;
        int g = -1;
        if (mine >> q & 1) {
            const int root = l_find(L, r * kTZ + lane);
            const int rr = root >> 6;
            g = (int)(((int64_t)(i0 + (rr >> 3)) * m.ny + (j0 + (rr & 7))) * m.nz + k0 + (root & 63));
        }
        parent[((int64_t)i * m.ny + j) * m.nz + k] = g;
    }
}

__global__ __launch_bounds__(kBlock) void cc_seam_kernel(CcVol m, int* parent) {
    int i0, j0, k0;
    tile_origin(m, i0, j0, k0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = k0 + lane;
    if (k >= m.nz) return;
    for (int q = 0; q < kRows / 4; ++q) {
        const int r = w + 4 * q, lx = r >> 3, ly = r & 7, i = i0 + lx, j = j0 + ly;
        if (i >= m.nx || j >= m.ny) continue;
        if (lx != kTX - 1 && ly != 0 && ly != kTY - 1 && lane != 0 && lane != kTZ - 1) continue;     // no forward neighbour elsewhere
        const int64_t n = ((int64_t)i * m.ny + j) * m.nz + k;
        if (!(m.v[n] > m.level)) continue;
        auto in = [&](int dx, int dy, int dz) {
            const int x = i + dx, y = j + dy, z = k + dz;
            if (x >= m.nx || (unsigned)y >= (unsigned)m.ny || (unsigned)z >= (unsigned)m.nz) return false;
            return m.v[n + dx * m.S + dy * (int64_t)m.nz + dz] > m.level;
        };
        auto emit = [&](int dx, int dy, int dz) {
            const int x = lx + dx, y = ly + dy, z = lane + dz;
            if (x < kTX && (unsigned)y < (unsigned)kTY && (unsigned)z < (unsigned)kTZ) return;      // same tile: done in LDS
            g_union(parent, (int)n, (int)(n + dx * m.S + dy * (int64_t)m.nz + dz));
        };
        pairs(m.conn26 != 0, in, emit);
    }
}

// A point whose parent lies in another tile was a tile root; it jumps to its root now, so that the points below it find the root in
// a few steps.  Readers see the old or the new parent, both ancestors.
__global__ __launch_bounds__(kBlock) void cc_shortcut_kernel(int* parent, int64_t N, int ny, int nz) {
    const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const int x = g_load(parent + n);
    if (x < 0 || x == (int)n) return;
    const int y = g_load(parent + x);
    if (y == x) return;
    if (ny > 0) {                                    // volumes: leave points that hang below a root of their own tile
        int i, j, k, a, b, c;
        unravel((int)n, ny, nz, i, j, k);
        unravel(x, ny, nz, a, b, c);
        if ((i >> 3) == (a >> 3) && (j >> 3) == (b >> 3) && (k >> 6) == (c >> 6)) return;
    }
    g_store(parent + n, g_find(parent, y));
}

// root[n] = root of n (-1 outside); chunk_cnt[chunk] = roots in the chunk.  parent is read-only here.
__global__ __launch_bounds__(kBlock) void cc_flatten_kernel(const int* __restrict__ parent, int64_t N, int* __restrict__ root,
                                                           int* __restrict__ chunk_cnt) {
    const int64_t n0 = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x * kPer;
    int cnt = 0;
    for (int q = 0; q < kPer && n0 + q < N; ++q) {
        const int n = (int)(n0 + q);
        int x = parent[n];
        if (x >= 0) {
            for (int p; (p = parent[x]) != x;) x = p;
            cnt += x == n;
        }
        root[n] = x;
    }
    int excl, total;
    ia::block_scan<kBlock>(cnt, excl, total);
    if (threadIdx.x == 0) chunk_cnt[blockIdx.x] = total;
}

// One workgroup: chunk counts -> exclusive offsets in place, count[0] = K.
__global__ __launch_bounds__(kScanBlock) void cc_scan_kernel(int* chunk_cnt, int n_chunks, int* __restrict__ count) {
    const int total = ia::scan_workgroup<int>(chunk_cnt, chunk_cnt, n_chunks);
    if (threadIdx.x == 0) count[0] = total;          // K <= N < 2^31
}

// rank[r] = 0-based rank of root r in index order (only root entries are written).
__global__ __launch_bounds__(kBlock) void cc_rank_kernel(const int* __restrict__ root, int64_t N, const int* __restrict__ chunk_off,
                                                        int* __restrict__ rank) {
    const int64_t n0 = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x * kPer;
    int cnt = 0;
    for (int q = 0; q < kPer && n0 + q < N; ++q) cnt += root[n0 + q] == (int)(n0 + q);
    int excl, total;
    ia::block_scan<kBlock>(cnt, excl, total);
    int id = chunk_off[blockIdx.x] + excl;
    for (int q = 0; q < kPer && n0 + q < N; ++q)
        if (root[n0 + q] == (int)(n0 + q)) rank[n0 + q] = id++;
}

__global__ __launch_bounds__(kBlock) void cc_relabel_kernel(int* __restrict__ labels, int64_t N, const int* __restrict__ rank) {
    const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const int r = labels[n];
    labels[n] = r >= 0 ? rank[r] + 1 : 0;
}

// ------------------------------------------------------------------ statistics and the filter

__device__ __forceinline__ void lower(int* p, int v) { if (*p > v) atomicMin(p, v); }      // a stale read only adds an atomic
__device__ __forceinline__ void raise(int* p, int v) { if (*p < v) atomicMax(p, v); }

__global__ __launch_bounds__(kBlock) void cc_stats_init_kernel(int* __restrict__ stats, int64_t total, int width) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % width);
    // volumes [K,8]: count, min index, min i j k, max i j k;  meshes [K,3]: vertices, faces, min vertex
    stats[t] = width == 8 ? (c == 0 ? 0 : (c < 5 ? INT_MAX : -1)) : (c == 2 ? INT_MAX : 0);
}

// A thread walks kRun consecutive points and sends one set of atomics per run of equal labels within a row.
__global__ __launch_bounds__(kBlock) void cc_stats_kernel(const int* __restrict__ labels, int nx, int ny, int nz, int64_t N, int K,
                                                         int* stats) {
    const int64_t n0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kRun;
    if (n0 >= N) return;
    int i, j, k;
    unravel((int)n0, ny, nz, i, j, k);
    int cur = 0, cnt = 0, first = 0, ci = 0, cj = 0, k0 = 0, k1 = 0;
    auto flush = [&]() {
        if (cur < 1 || cur > K) return;              // labels outside 1..K are ignored, never written through
        int* row = stats + (int64_t)(cur - 1) * 8;
        atomicAdd(row, cnt);
        lower(row + 1, first); lower(row + 2, ci); lower(row + 3, cj); lower(row + 4, k0);
        raise(row + 5, ci); raise(row + 6, cj); raise(row + 7, k1);
    };
    for (int q = 0; q < kRun && n0 + q < N; ++q) {
        const int l = labels[n0 + q];
        if (l != cur || k == 0) {
            flush();
            cur = l; cnt = 0; first = (int)(n0 + q); ci = i; cj = j; k0 = k;
        }
        ++cnt; k1 = k;
        if (++k == nz) { k = 0; if (++j == ny) { j = 0; ++i; } }
    }
    flush();
}

__global__ __launch_bounds__(kBlock) void cc_keep_kernel(const float* volume, const int* __restrict__ labels, int64_t N,
                                                        const unsigned char* __restrict__ keep, int K, float fill, float* out) {
    const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const int l = labels[n];
    const float v = volume[n];
    out[n] = (l >= 1 && l <= K && !keep[l]) ? fill : v;
}

// ------------------------------------------------------------------ meshes

__global__ __launch_bounds__(kBlock) void mesh_init_kernel(int* __restrict__ parent, int V) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v < V) parent[v] = (int)v;
}

__global__ __launch_bounds__(kBlock) void mesh_hook_kernel(const int* __restrict__ faces, int64_t F, int V, int* parent) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) return;     // not a face of this mesh
    g_union(parent, a, b);
    g_union(parent, b, c);
}

__global__ __launch_bounds__(kBlock) void mesh_stats_verts_kernel(const int* __restrict__ labels, int V, int K, int* stats) {
    const int64_t v0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kRun;
    int cur = 0, cnt = 0, first = 0;
    auto flush = [&]() {
        if (cur < 1 || cur > K) return;
        atomicAdd(stats + (int64_t)(cur - 1) * 3, cnt);
        lower(stats + (int64_t)(cur - 1) * 3 + 2, first);
    };
    for (int q = 0; q < kRun && v0 + q < V; ++q) {
        const int l = labels[v0 + q];
        if (l != cur) { flush(); cur = l; cnt = 0; first = (int)(v0 + q); }
        ++cnt;
    }
    flush();
}

__global__ __launch_bounds__(kBlock) void mesh_stats_faces_kernel(const int* __restrict__ faces, int64_t F, const int* __restrict__ labels,
                                                                 int V, int K, int* stats) {
    const int64_t f0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kRun;
    int cur = 0, cnt = 0;
    auto flush = [&]() {
        if (cur >= 1 && cur <= K) atomicAdd(stats + (int64_t)(cur - 1) * 3 + 1, cnt);
    };
    for (int q = 0; q < kRun && f0 + q < F; ++q) {
        const int a = faces[3 * (f0 + q)];
        const int l = (unsigned)a < (unsigned)V ? labels[a] : 0;
        if (l != cur) { flush(); cur = l; cnt = 0; }
        ++cnt;
    }
    flush();
}

// ------------------------------------------------------------------ host side

size_t linear_scratch(int64_t n) { return sizeof(int) * ((size_t)n + (size_t)ia::ceil_div(n, kChunk)); }

// flatten .. relabel over a parent array of n entries: labels and count[0] = K.
int number_components(int* parent, int64_t n, int* labels, int* count, hipStream_t s, const char* what) {
    int* chunk = parent + n;
    const int64_t nc = ia::ceil_div(n, kChunk);
    cc_flatten_kernel<<<(unsigned)nc, kBlock, 0, s>>>(parent, n, labels, chunk);
    if (int st = ia::check_launch(what)) return st;
    cc_scan_kernel<<<1, kScanBlock, 0, s>>>(chunk, (int)nc, count);
    if (int st = ia::check_launch(what)) return st;
    cc_rank_kernel<<<(unsigned)nc, kBlock, 0, s>>>(labels, n, chunk, parent);
    if (int st = ia::check_launch(what)) return st;
    cc_relabel_kernel<<<blocks(n, kBlock), kBlock, 0, s>>>(labels, n, parent);
    return ia::check_launch(what);
}

}  // namespace

extern "C" int ia_components_scratch_bytes(int nx, int ny, int nz, size_t* h_bytes) {
    if (int st = check_volume(nx, ny, nz, "ia_components_scratch_bytes")) return st;
    IA_REQUIRE(h_bytes, "ia_components_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = linear_scratch((int64_t)nx * ny * nz);
    return IA_OK;
}

extern "C" int ia_volume_components(const float* volume, int nx, int ny, int nz, float level, int connectivity, int* labels, void* scratch,
                                    size_t scratch_bytes, int* count, void* stream) {
    if (int st = check_volume(nx, ny, nz, "ia_volume_components")) return st;
    IA_REQUIRE(connectivity == 6 || connectivity == 26, "ia_volume_components: connectivity must be 6 or 26, got %d", connectivity);
    if (!on_device(volume) || !on_device(labels) || !on_device(scratch) || !on_device(count))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_volume_components: volume, labels, scratch and count must be device pointers");
    const int64_t N = (int64_t)nx * ny * nz;
    if (scratch_bytes < linear_scratch(N))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_volume_components: scratch holds %zu bytes, needs %zu", scratch_bytes, linear_scratch(N));
    CcVol m{volume, nx, ny, nz, (int64_t)ny * nz, N, level, connectivity == 26 ? 1 : 0,
            (int)ia::ceil_div(ny, kTY), (int)ia::ceil_div(nz, kTZ)};
    const unsigned tiles = (unsigned)(ia::ceil_div(nx, kTX) * m.ty * m.tz);
    int* parent = static_cast<int*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    cc_tile_kernel<<<tiles, kBlock, 0, s>>>(m, parent);
    if (int st = ia::check_launch("ia_volume_components (tiles)")) return st;
    cc_seam_kernel<<<tiles, kBlock, 0, s>>>(m, parent);
    if (int st = ia::check_launch("ia_volume_components (seams)")) return st;
    cc_shortcut_kernel<<<blocks(N, kBlock), kBlock, 0, s>>>(parent, N, ny, nz);
    if (int st = ia::check_launch("ia_volume_components (shortcut)")) return st;
    return number_components(parent, N, labels, count, s, "ia_volume_components (numbering)");
}

extern "C" int ia_component_stats(const int* labels, int nx, int ny, int nz, int K, int* stats, void* stream) {
    if (int st = check_volume(nx, ny, nz, "ia_component_stats")) return st;
    const int64_t N = (int64_t)nx * ny * nz;
    IA_REQUIRE(K >= 0 && K <= N, "ia_component_stats: K = %d is not a component count of a volume of %lld points", K, (long long)N);
    if (K == 0) return IA_OK;
    if (!on_device(labels) || !on_device(stats))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_component_stats: labels and stats must be device pointers");
    hipStream_t s = (hipStream_t)stream;
    cc_stats_init_kernel<<<blocks((int64_t)K * 8, kBlock), kBlock, 0, s>>>(stats, (int64_t)K * 8, 8);
    if (int st = ia::check_launch("ia_component_stats (init)")) return st;
    cc_stats_kernel<<<blocks(N, kBlock * kRun), kBlock, 0, s>>>(labels, nx, ny, nz, N, K, stats);
    return ia::check_launch("ia_component_stats");
}

extern "C" int ia_volume_keep(const float* volume, const int* labels, int64_t n, const unsigned char* keep_flags, int K, float fill,
                              float* out, void* stream) {
    IA_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "ia_volume_keep: n must be in [0, 2^31)");
    IA_REQUIRE(K >= 0 && K <= n, "ia_volume_keep: K = %d is not a component count of %lld points", K, (long long)n);
    if (n == 0) return IA_OK;
    if (!on_device(volume) || !on_device(labels) || !on_device(keep_flags) || !on_device(out))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_volume_keep: volume, labels, keep_flags and out must be device pointers");
    cc_keep_kernel<<<blocks(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(volume, labels, n, keep_flags, K, fill, out);
    return ia::check_launch("ia_volume_keep");
}

extern "C" int ia_mesh_components_scratch_bytes(int V, size_t* h_bytes) {
    IA_REQUIRE(V >= 0, "ia_mesh_components_scratch_bytes: V must be >= 0");
    IA_REQUIRE(h_bytes, "ia_mesh_components_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = linear_scratch(V < 1 ? 1 : V);
    return IA_OK;
}

extern "C" int ia_mesh_components(const int* faces, int64_t F, int V, int* vert_labels, void* scratch, size_t scratch_bytes, int* count,
                                  void* stream) {
    IA_REQUIRE(V >= 0 && F >= 0 && F < ((int64_t)1 << 31) / 3, "ia_mesh_components: V and F must be >= 0 and 3 F < 2^31");
    if (!on_device(count)) return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_components: count must be a device pointer");
    hipStream_t s = (hipStream_t)stream;
    if (V == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) return ia::check_launch("ia_mesh_components (empty)");
        return IA_OK;
    }
    if ((F && !on_device(faces)) || !on_device(vert_labels) || !on_device(scratch))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_components: faces, vert_labels and scratch must be device pointers");
    if (scratch_bytes < linear_scratch(V))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_components: scratch holds %zu bytes, needs %zu", scratch_bytes, linear_scratch(V));
    int* parent = static_cast<int*>(scratch);
    mesh_init_kernel<<<blocks(V, kBlock), kBlock, 0, s>>>(parent, V);
    if (int st = ia::check_launch("ia_mesh_components (init)")) return st;
    if (F) {
        mesh_hook_kernel<<<blocks(F, kBlock), kBlock, 0, s>>>(faces, F, V, parent);
        if (int st = ia::check_launch("ia_mesh_components (hook)")) return st;
        cc_shortcut_kernel<<<blocks(V, kBlock), kBlock, 0, s>>>(parent, V, 0, 0);
        if (int st = ia::check_launch("ia_mesh_components (shortcut)")) return st;
    }
    return number_components(parent, V, vert_labels, count, s, "ia_mesh_components (numbering)");
}

extern "C" int ia_mesh_component_stats(const int* faces, int64_t F, int V, const int* vert_labels, int K, int* stats, void* stream) {
    IA_REQUIRE(V >= 0 && F >= 0 && F < ((int64_t)1 << 31) / 3, "ia_mesh_component_stats: V and F must be >= 0 and 3 F < 2^31");
    IA_REQUIRE(K >= 0 && K <= V, "ia_mesh_component_stats: K = %d is not a component count of a mesh of %d vertices", K, V);
    if (K == 0) return IA_OK;
    if ((F && !on_device(faces)) || !on_device(vert_labels) || !on_device(stats))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_component_stats: faces, vert_labels and stats must be device pointers");
    hipStream_t s = (hipStream_t)stream;
    cc_stats_init_kernel<<<blocks((int64_t)K * 3, kBlock), kBlock, 0, s>>>(stats, (int64_t)K * 3, 3);
    if (int st = ia::check_launch("ia_mesh_component_stats (init)")) return st;
    mesh_stats_verts_kernel<<<blocks(V, kBlock * kRun), kBlock, 0, s>>>(vert_labels, V, K, stats);
    if (int st = ia::check_launch("ia_mesh_component_stats (vertices)")) return st;
    if (F) {
        mesh_stats_faces_kernel<<<blocks(F, kBlock * kRun), kBlock, 0, s>>>(faces, F, vert_labels, V, K, stats);
        if (int st = ia::check_launch("ia_mesh_component_stats (faces)")) return st;
    }
    return IA_OK;
}
