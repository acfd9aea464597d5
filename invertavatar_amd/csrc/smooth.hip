// Mesh smoothing on the device (Taubin lambda | mu and plain Laplacian, uniform or cotangent weights) and vertex normals from the mesh.
// No counterpart in the reference; geometry.py (_adjacency_numpy, _cotangent_numpy, _smooth_numpy, _mesh_normals_numpy) restates every
// line in NumPy and is the definition.
//
// Layout.  A usable face (three distinct indices in [0, V), three finite vertices) emits six directed-edge keys i V + j and three
// incidence keys v F + f (int64; kNoKey, which sorts last, for an unusable face).  The caller sorts both key arrays (torch.sort, stable:
// equal edge keys stay in face order); every other step is here:
//
//   keys     : the nine keys per face, the number of usable faces (one integer atomic per wave) and the out-of-range flag.
//   heads    : first entry of every run of equal edge keys, counted per workgroup; a one-workgroup scan of the workgroup counts gives
//              every workgroup its first CSR slot and the host the total E (read once, with the two numbers above).
//   csr      : per run head its slot (workgroup offset + ballot rank): neighbors[slot] = j, edge_faces[slot] = run length, the key and
//              the run's first sorted position; boundary (length 1) and non-manifold (length > 2) entries counted by integer atomics.
//   offsets  : offsets[v] = lower bound of v V among the slot keys (V + 1 binary searches: vertices without neighbours cost nothing
//              special); the same kernel gives face_offsets from the sorted incidence keys.     face_ids: sorted position -> face.
//   vertices : boundary flag, largest degree, boundary vertices, and the list of vertices of degree > kHeavy.
//   cotangent: one thread per slot walks its run in sorted (= face) order: cot of the angle opposite the edge in double from the fp32
//              input positions, w = fp32(max(0, sum / 2)).
//   pinned   : non-finite, no neighbour, all weights zero, boundary (if fixed), caller's mask.
//   step     : one thread per vertex: p' = fp32(p + f (S / W - p)), S and W summed in double over the row in ascending j.  The degree
//              is about 6 on marching-cubes and clustered meshes (at most about 12), so a row per lane keeps every lane busy and reads
//              offsets, neighbours and its own position coalesced; the gathered positions are 12-byte reads that lie close by in
//              memory (vertices are numbered in lattice or cell order) and come from L2.  A vertex of degree > kHeavy is left to
//              step_heavy: one wave per such vertex, lane l sums entries l, l + 64, ... in order and the 64 partial sums are added in
//              a fixed butterfly, so a hub of any degree costs degree / 64 steps and its sum has one fixed order.
//   normals  : one thread per vertex over its faces in ascending face index.
//
// No floating-point atomics; every sum's order is fixed by the sorted layout, so results are bit-equal from run to run.  Plain IEEE
// double arithmetic (+ - * / sqrt, atan2 for the corner angles), no fast-math intrinsics; the build has -ffp-contract=off.
#include "geom_common.h"

#include <algorithm>
#include <cmath>

namespace {

using ia::kScanBlock; using ia::on_device; using ia::wave_count; using ia::wave_sum;

constexpr int kBlock = 256;
constexpr int kHeavy = 64;                           // neighbours beyond which a vertex gets a wave of its own
constexpr int64_t kMaxCount = (int64_t)1 << 28;      // vertices and faces: 6 F entries stay below 2^31, i V + j below 2^56
constexpr int64_t kNoKey = INT64_MAX;

__device__ __forceinline__ bool finite3(const float* __restrict__ v, int64_t i) {
    return isfinite(v[3 * i]) && isfinite(v[3 * i + 1]) && isfinite(v[3 * i + 2]);
}

using D3 = ia::Vec3<double>;                        // sub, dot ((x + y) + z), cross: geom_common.h
__device__ __forceinline__ D3 load3(const float* __restrict__ v, int64_t i) { return {(double)v[3 * i], (double)v[3 * i + 1], (double)v[3 * i + 2]}; }
__device__ __forceinline__ double len(D3 a) { return sqrt(dot(a, a)); }

// ------------------------------------------------------------------ keys

__global__ __launch_bounds__(kBlock) void keys_kernel(const float* __restrict__ verts, int64_t V, const int* __restrict__ faces, int64_t F,
                                                      int64_t* __restrict__ ekeys, int64_t* __restrict__ vkeys, int* __restrict__ count) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool usable = false;
    if (f < F) {
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        const bool in_range = (uint64_t)a < (uint64_t)V && (uint64_t)b < (uint64_t)V && (uint64_t)c < (uint64_t)V;
        if (!in_range) count[1] = 1;
        usable = in_range && a != b && b != c && a != c && finite3(verts, a) && finite3(verts, b) && finite3(verts, c);
        int64_t* e = ekeys + 6 * f;
        int64_t* k = vkeys + 3 * f;
        e[0] = usable ? a * V + b : kNoKey; e[1] = usable ? b * V + a : kNoKey;
        e[2] = usable ? b * V + c : kNoKey; e[3] = usable ? c * V + b : kNoKey;
        e[4] = usable ? c * V + a : kNoKey; e[5] = usable ? a * V + c : kNoKey;
        k[0] = usable ? a * F + f : kNoKey; k[1] = usable ? b * F + f : kNoKey; k[2] = usable ? c * F + f : kNoKey;
    }
    wave_count(usable, count);
}

// ------------------------------------------------------------------ run heads -> CSR

__device__ __forceinline__ bool is_head(const int64_t* __restrict__ skeys, int64_t n, int64_t e) {
    if (e >= n) return false;
    const int64_t k = skeys[e];
    return k != kNoKey && (e == 0 || k != skeys[e - 1]);
}

// Rank of the thread among the threads of its workgroup with `p` set (exclusive), and their number.
__device__ __forceinline__ int block_rank(bool p, int& total) {
    __shared__ int part[kBlock / 64];
    const unsigned long long m = __ballot(p);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();                                                      // (part may still be read from an earlier call)
    if (lane == 0) part[w] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int j = 0; j < kBlock / 64; ++j) {
        before += j < w ? part[j] : 0;
        all += part[j];
    }
    total = all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kBlock) void heads_kernel(const int64_t* __restrict__ skeys, int64_t n, int* __restrict__ blocksum) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int total;
    block_rank(is_head(skeys, n, e), total);
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
}

// One workgroup: out[0 .. n) = exclusive sums of in[0 .. n), out[n] = total.  in == out is allowed.
__global__ __launch_bounds__(kScanBlock) void scan_kernel(const int* in, int* out, int64_t n) {
    const int total = ia::scan_workgroup<int>(in, out, n);
    if (threadIdx.x == 0) out[n] = total;
}

struct CsrArgs {
    const int64_t* skeys;
    int64_t n;                   // sorted entries (6 F)
    int64_t V;
    const int* blockoff;         // exclusive scan of the workgroup counts
    int64_t E;                   // capacity of the slot arrays
    int* neighbors;
    int* edge_faces;
    int* run_start;
    int64_t* ukey;
    int* count;                  // [2] boundary entries, [3] non-manifold entries
};

__global__ __launch_bounds__(kBlock) void csr_kernel(CsrArgs u) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool head = is_head(u.skeys, u.n, e);
    int total;
    const int64_t slot = (int64_t)u.blockoff[blockIdx.x] + block_rank(head, total);
    int run = 0;
    if (head && slot < u.E) {
        const int64_t key = u.skeys[e];
        run = 1;
        while (e + run < u.n && u.skeys[e + run] == key) ++run;
        u.neighbors[slot] = (int)(key % u.V);
        u.edge_faces[slot] = run;
        u.run_start[slot] = (int)e;
        u.ukey[slot] = key;
    }
    wave_count(run == 1, u.count + 2);
    wave_count(run > 2, u.count + 3);
}

// out[v] = number of keys below v * mult, v in [0, V]: the first CSR slot (or incidence entry) of vertex v.
__global__ __launch_bounds__(kBlock) void offsets_kernel(const int64_t* __restrict__ keys, int64_t n, int64_t V, int64_t mult,
                                                         int* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v > V) return;
    const int64_t target = v * mult;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    out[v] = (int)lo;
}

__global__ __launch_bounds__(kBlock) void face_ids_kernel(const int64_t* __restrict__ vorder, int64_t n, int64_t F, int* __restrict__ face_ids) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const int64_t src = vorder[k];
    face_ids[k] = (uint64_t)src < (uint64_t)(3 * F) ? (int)(src / 3) : 0;
}

__global__ __launch_bounds__(kBlock) void vertices_kernel(const int* __restrict__ offsets, const int* __restrict__ edge_faces, int64_t V,
                                                          unsigned char* __restrict__ boundary, int* __restrict__ heavy, int* __restrict__ count) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool b = false;
    int deg = 0;
    if (v < V) {
        const int e0 = offsets[v], e1 = offsets[v + 1];
        deg = e1 - e0;
        for (int e = e0; e < e1; ++e) b = b || edge_faces[e] == 1;
        boundary[v] = b ? 1 : 0;
        if (deg > kHeavy) heavy[atomicAdd(count + 6, 1)] = (int)v;       // (rare; the order of the list changes no result)
    }
    wave_count(b, count + 4);
    const int m = ia::wave_max(deg);
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(count + 5, m);
}

// ------------------------------------------------------------------ cotangent weights

struct CotArgs {
    const float* verts;
    const int* faces;
    int64_t V, F, E;
    const int64_t* order;        // sorted position -> 6 f + slot of the face's six entries
    const int64_t* ukey;
    const int* run_start;
    const int* edge_faces;
    float* w;
};

__global__ __launch_bounds__(kBlock) void cotangent_kernel(CotArgs u) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= u.E) return;
    const int64_t key = u.ukey[s];
    const D3 pi = load3(u.verts, key / u.V), pj = load3(u.verts, key % u.V);
    const int64_t e0 = u.run_start[s];
    const int run = u.edge_faces[s];
    double sum = 0.0;
    for (int r = 0; r < run; ++r) {
        const int64_t src = u.order[e0 + r];
        if ((uint64_t)src >= (uint64_t)(6 * u.F)) continue;
        const int64_t f = src / 6;
        const int k = (int)(src % 6);
        const int64_t o = u.faces[3 * f + (k < 2 ? 2 : (k < 4 ? 0 : 1))];  // the corner opposite (a,b) (b,a) | (b,c) (c,b) | (c,a) (a,c)
        if ((uint64_t)o >= (uint64_t)u.V) continue;
        const D3 po = load3(u.verts, o);
        const D3 a = sub(pi, po), b = sub(pj, po);
        const double l = len(cross(a, b));
        if (l > 0.0 && isfinite(l)) sum += dot(a, b) / l;
    }
    u.w[s] = (float)fmax(0.0, 0.5 * sum);
}

// ------------------------------------------------------------------ pinned vertices, steps

struct PinArgs {
    const float* verts;
    int64_t V;
    const int* offsets;
    const float* w;              // or null (uniform)
    const unsigned char* boundary;
    int fix_boundary;
    const unsigned char* fixed;  // or null
    unsigned char* pinned;
};

__global__ __launch_bounds__(kBlock) void pinned_kernel(PinArgs u) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= u.V) return;
    const int e0 = u.offsets[v], e1 = u.offsets[v + 1];
    bool pin = !finite3(u.verts, v) || e1 == e0 || (u.fix_boundary && u.boundary[v]) || (u.fixed && u.fixed[v]);
    if (u.w && !pin) {
        bool any = false;
        for (int e = e0; e < e1; ++e) any = any || u.w[e] > 0.f;
        pin = !any;
    }
    u.pinned[v] = pin ? 1 : 0;
}

struct StepArgs {
    const float* in;
    float* out;
    int64_t V;
    const int* offsets;
    const int* neighbors;
    const float* w;              // or null (uniform)
    const unsigned char* pinned;
    double f;
    const int* heavy;
    int n_heavy;
};

__device__ __forceinline__ void move_vertex(const StepArgs& u, int64_t v, D3 s, double wsum) {
    const D3 p = load3(u.in, v);
    u.out[3 * v] = (float)(p.x + u.f * (s.x / wsum - p.x));
    u.out[3 * v + 1] = (float)(p.y + u.f * (s.y / wsum - p.y));
    u.out[3 * v + 2] = (float)(p.z + u.f * (s.z / wsum - p.z));
}

__global__ __launch_bounds__(kBlock) void step_kernel(StepArgs u) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= u.V) return;
    const int e0 = u.offsets[v], e1 = u.offsets[v + 1];
    if (u.pinned[v]) {
        u.out[3 * v] = u.in[3 * v]; u.out[3 * v + 1] = u.in[3 * v + 1]; u.out[3 * v + 2] = u.in[3 * v + 2];
        return;
    }
    if (e1 - e0 > kHeavy) return;                                         // step_heavy_kernel's
    D3 s{0.0, 0.0, 0.0};
    double wsum = 0.0;
    for (int e = e0; e < e1; ++e) {
        const double w = u.w ? (double)u.w[e] : 1.0;
        const D3 q = load3(u.in, u.neighbors[e]);
        s.x += w * q.x; s.y += w * q.y; s.z += w * q.z;
        wsum += w;
    }
    move_vertex(u, v, s, wsum);
}

__global__ __launch_bounds__(64) void step_heavy_kernel(StepArgs u) {
    const int lane = threadIdx.x;
    for (int h = blockIdx.x; h < u.n_heavy; h += gridDim.x) {
        const int64_t v = u.heavy[h];
        if ((uint64_t)v >= (uint64_t)u.V || u.pinned[v]) continue;
        const int e0 = u.offsets[v], e1 = u.offsets[v + 1];
        D3 s{0.0, 0.0, 0.0};
        double wsum = 0.0;
        for (int e = e0 + lane; e < e1; e += 64) {
            const double w = u.w ? (double)u.w[e] : 1.0;
            const D3 q = load3(u.in, u.neighbors[e]);
            s.x += w * q.x; s.y += w * q.y; s.z += w * q.z;
            wsum += w;
        }
        s.x = wave_sum(s.x); s.y = wave_sum(s.y); s.z = wave_sum(s.z);
        wsum = wave_sum(wsum);
        if (lane == 0) move_vertex(u, v, s, wsum);
    }
}

// ------------------------------------------------------------------ normals

struct NormalArgs {
    const float* verts;
    const int* faces;
    int64_t V, F;
    const int* face_offsets;
    const int* face_ids;
    int angle;
    float* out;
};

__global__ __launch_bounds__(kBlock) void normals_kernel(NormalArgs u) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= u.V) return;
    D3 s{0.0, 0.0, 0.0};
    const int k0 = u.face_offsets[v], k1 = u.face_offsets[v + 1];
    for (int k = k0; k < k1; ++k) {
        const int64_t f = u.face_ids[k];
        if ((uint64_t)f >= (uint64_t)u.F) continue;
        const int64_t ia = u.faces[3 * f], ib = u.faces[3 * f + 1], ic = u.faces[3 * f + 2];
        if ((uint64_t)ia >= (uint64_t)u.V || (uint64_t)ib >= (uint64_t)u.V || (uint64_t)ic >= (uint64_t)u.V) continue;
        const D3 a = load3(u.verts, ia), b = load3(u.verts, ib), c = load3(u.verts, ic);
        const D3 n = cross(sub(b, a), sub(c, a));
        if (!u.angle) {
            s.x += n.x; s.y += n.y; s.z += n.z;
            continue;
        }
        const double l = len(n);
        if (!(l > 0.0 && isfinite(l))) continue;
        const D3 cur = ia == v ? a : (ib == v ? b : c), nxt = ia == v ? b : (ib == v ? c : a), prv = ia == v ? c : (ib == v ? a : b);
        const double ang = atan2(l, dot(sub(nxt, cur), sub(prv, cur)));
        s.x += n.x / l * ang; s.y += n.y / l * ang; s.z += n.z / l * ang;
    }
    const double l = len(s);
    const bool ok = l > 0.0 && isfinite(l);
    u.out[3 * v] = ok ? (float)(s.x / l) : 0.f;
    u.out[3 * v + 1] = ok ? (float)(s.y / l) : 0.f;
    u.out[3 * v + 2] = ok ? (float)(s.z / l) : 0.f;
}

// ------------------------------------------------------------------ host side

unsigned blocks(int64_t n) { return ia::blocks(n, kBlock); }

}  // namespace

extern "C" int ia_mesh_edge_keys(const float* verts, int64_t V, const int* faces, int64_t F, int64_t* edge_keys, int64_t* vertex_keys,
                                 int* count, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount && F >= 0 && F <= kMaxCount, "ia_mesh_edge_keys: V and F must be in [0, 2^28], got V = %lld, F = %lld",
               (long long)V, (long long)F);
    if (!on_device(count)) return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_edge_keys: count must be a device pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, 8 * sizeof(int), s) != hipSuccess) return ia::check_launch("ia_mesh_edge_keys (clear)");
    if (F == 0) return IA_OK;
    if ((V && !on_device(verts)) || !on_device(faces) || !on_device(edge_keys) || !on_device(vertex_keys))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_edge_keys: verts, faces and both key arrays must be device pointers");
    keys_kernel<<<blocks(F), kBlock, 0, s>>>(verts, V, faces, F, edge_keys, vertex_keys, count);
    return ia::check_launch("ia_mesh_edge_keys");
}

extern "C" int ia_mesh_edge_heads_scratch_bytes(int64_t F, size_t* h_bytes) {
    IA_REQUIRE(F >= 0 && F <= kMaxCount, "ia_mesh_edge_heads_scratch_bytes: F must be in [0, 2^28], got %lld", (long long)F);
    IA_REQUIRE(h_bytes, "ia_mesh_edge_heads_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = sizeof(int) * ((size_t)blocks(6 * F) + 1);
    return IA_OK;
}

extern "C" int ia_mesh_edge_heads(const int64_t* sorted_keys, int64_t F, void* scratch, size_t scratch_bytes, int* count, void* stream) {
    IA_REQUIRE(F >= 0 && F <= kMaxCount, "ia_mesh_edge_heads: F must be in [0, 2^28], got %lld", (long long)F);
    const unsigned nb = blocks(6 * F);
    const size_t need = sizeof(int) * ((size_t)nb + 1);
    if (scratch_bytes < need) return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_edge_heads: scratch holds %zu bytes, needs %zu", scratch_bytes, need);
    if (!on_device(count) || !on_device(scratch) || (F && !on_device(sorted_keys)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_edge_heads: keys, scratch and count must be device pointers");
    hipStream_t s = (hipStream_t)stream;
    int* blocksum = static_cast<int*>(scratch);
    heads_kernel<<<nb, kBlock, 0, s>>>(sorted_keys, 6 * F, blocksum);
    if (int st = ia::check_launch("ia_mesh_edge_heads")) return st;
    scan_kernel<<<1, kScanBlock, 0, s>>>(blocksum, blocksum, nb);
    if (int st = ia::check_launch("ia_mesh_edge_heads (scan)")) return st;
    if (hipMemcpyAsync(count + 7, blocksum + nb, sizeof(int), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return ia::check_launch("ia_mesh_edge_heads (total)");
    return IA_OK;
}

extern "C" int ia_mesh_csr(const int64_t* sorted_keys, const int64_t* sorted_vertex_keys, const int64_t* vertex_order, int64_t V, int64_t F,
                           int64_t usable, int64_t E, const void* scratch, int* offsets, int* neighbors, int* edge_faces, int* run_start,
                           int64_t* slot_keys, unsigned char* boundary, int* face_offsets, int* face_ids, int* heavy, int* count,
                           void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount && F >= 0 && F <= kMaxCount && usable >= 0 && usable <= F && E >= 0 && E <= 6 * usable,
               "ia_mesh_csr: V, F in [0, 2^28], 0 <= usable <= F and 0 <= E <= 6 usable");
    if (!on_device(offsets) || !on_device(face_offsets) || !on_device(count) || (V && (!on_device(boundary) || !on_device(heavy))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_csr: offsets, face_offsets, boundary, heavy and count must be device pointers");
    if (F && (!on_device(sorted_keys) || !on_device(sorted_vertex_keys) || !on_device(vertex_order) || !on_device(scratch)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_csr: the sorted keys, the order and scratch must be device pointers");
    if (E && (!on_device(neighbors) || !on_device(edge_faces) || !on_device(run_start) || !on_device(slot_keys)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_csr: the slot arrays must be device pointers");
    if (usable && !on_device(face_ids)) return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_csr: face_ids must be a device pointer");
    hipStream_t s = (hipStream_t)stream;
    if (E) {
        CsrArgs u{sorted_keys, 6 * F, V, static_cast<const int*>(scratch), E, neighbors, edge_faces, run_start, slot_keys, count};
        csr_kernel<<<blocks(6 * F), kBlock, 0, s>>>(u);
        if (int st = ia::check_launch("ia_mesh_csr")) return st;
    }
    offsets_kernel<<<blocks(V + 1), kBlock, 0, s>>>(slot_keys, E, V, V, offsets);
    if (int st = ia::check_launch("ia_mesh_csr (offsets)")) return st;
    offsets_kernel<<<blocks(V + 1), kBlock, 0, s>>>(sorted_vertex_keys, 3 * usable, V, F, face_offsets);
    if (int st = ia::check_launch("ia_mesh_csr (face offsets)")) return st;
    if (usable) {
        face_ids_kernel<<<blocks(3 * usable), kBlock, 0, s>>>(vertex_order, 3 * usable, F, face_ids);
        if (int st = ia::check_launch("ia_mesh_csr (face ids)")) return st;
    }
    if (V) {
        vertices_kernel<<<blocks(V), kBlock, 0, s>>>(offsets, edge_faces, V, boundary, heavy, count);
        if (int st = ia::check_launch("ia_mesh_csr (vertices)")) return st;
    }
    return IA_OK;
}

extern "C" int ia_mesh_cotangent(const float* verts, int64_t V, const int* faces, int64_t F, const int64_t* edge_order, const int64_t* slot_keys,
                                 const int* run_start, const int* edge_faces, int64_t E, float* weights, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount && F >= 0 && F <= kMaxCount && E >= 0 && E <= 6 * F, "ia_mesh_cotangent: V, F in [0, 2^28] and 0 <= E <= 6 F");
    if (E == 0) return IA_OK;
    if (!on_device(verts) || !on_device(faces) || !on_device(edge_order) || !on_device(slot_keys) || !on_device(run_start) || !on_device(edge_faces) ||
        !on_device(weights))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_cotangent: every array must be a device pointer");
    CotArgs u{verts, faces, V, F, E, edge_order, slot_keys, run_start, edge_faces, weights};
    cotangent_kernel<<<blocks(E), kBlock, 0, (hipStream_t)stream>>>(u);
    return ia::check_launch("ia_mesh_cotangent");
}

extern "C" int ia_smooth_pinned(const float* verts, int64_t V, const int* offsets, const float* weights, const unsigned char* boundary,
                                int fix_boundary, const unsigned char* fixed, unsigned char* pinned, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount, "ia_smooth_pinned: V must be in [0, 2^28], got %lld", (long long)V);
    if (V == 0) return IA_OK;
    if (!on_device(verts) || !on_device(offsets) || !on_device(boundary) || !on_device(pinned) || (weights && !on_device(weights)) ||
        (fixed && !on_device(fixed)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_smooth_pinned: every array must be a device pointer");
    PinArgs u{verts, V, offsets, weights, boundary, fix_boundary, fixed, pinned};
    pinned_kernel<<<blocks(V), kBlock, 0, (hipStream_t)stream>>>(u);
    return ia::check_launch("ia_smooth_pinned");
}

extern "C" int ia_smooth_steps(float* verts_a, float* verts_b, int64_t V, const int* offsets, const int* neighbors, const float* weights,
                               const unsigned char* pinned, const int* heavy, int n_heavy, const double* h_factors, int n_steps, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount && n_steps >= 0 && n_heavy >= 0 && n_heavy <= V, "ia_smooth_steps: V in [0, 2^28], n_steps >= 0, 0 <= n_heavy <= V");
    IA_REQUIRE(n_steps == 0 || h_factors, "ia_smooth_steps: factors must not be NULL");
    if (V == 0 || n_steps == 0) return IA_OK;
    if (!on_device(verts_a) || !on_device(verts_b) || !on_device(offsets) || !on_device(pinned) || (weights && !on_device(weights)) ||
        (n_heavy && !on_device(heavy)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_smooth_steps: every array must be a device pointer");
    IA_REQUIRE(verts_a != verts_b, "ia_smooth_steps: the two position buffers must differ");
    hipStream_t s = (hipStream_t)stream;
    for (int k = 0; k < n_steps; ++k) {
        IA_REQUIRE(std::isfinite(h_factors[k]), "ia_smooth_steps: factor %d is not finite", k);
        StepArgs u{k % 2 ? verts_b : verts_a, k % 2 ? verts_a : verts_b, V, offsets, neighbors, weights, pinned, h_factors[k], heavy, n_heavy};
        step_kernel<<<blocks(V), kBlock, 0, s>>>(u);
        if (int st = ia::check_launch("ia_smooth_steps")) return st;
        if (n_heavy) {
            step_heavy_kernel<<<std::min(n_heavy, 4096), 64, 0, s>>>(u);
            if (int st = ia::check_launch("ia_smooth_steps (heavy)")) return st;
        }
    }
    return IA_OK;
}

extern "C" int ia_mesh_normals(const float* verts, int64_t V, const int* faces, int64_t F, const int* face_offsets, const int* face_ids,
                               int angle, float* normals, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount && F >= 0 && F <= kMaxCount, "ia_mesh_normals: V and F must be in [0, 2^28]");
    if (V == 0) return IA_OK;
    if (!on_device(verts) || !on_device(face_offsets) || !on_device(normals) || (F && !on_device(faces)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_normals: every array must be a device pointer");
    NormalArgs u{verts, faces, V, F, face_offsets, face_ids, angle ? 1 : 0, normals};
    normals_kernel<<<blocks(V), kBlock, 0, (hipStream_t)stream>>>(u);
    return ia::check_launch("ia_mesh_normals");
}
