// Fast winding numbers: an implicit cluster tree over the triangles with a far-field expansion per node.  No
// counterpart in the reference; the definition is geometry.WindingTree and its NumPy restatement.  The exact all-pairs sum of
// winding.hip stays the yardstick: with beta = inf the tree adds the same solid angles, in another order.
//
// Order    : usable triangles (A.w of ia_tri_pack) sorted by the 30-bit Morton key of their centroid (10 bits per axis over the cube
//            on the longest side of the box of the finite vertices; fp32: ((A + B) + C) * fp32(1/3), floor((c - lo) * scale), clamped
//            to [0, 1023]; x is the lowest bit of a triple).  The sort of the keys is the caller's (stable: ties by face index);
//            unusable triangles have the key 2^30, go last and belong to no leaf.
// Tree     : leaves of L = kLeaf sorted faces under nodes of B = kBranch children, level by level (cluster_tree.h).
// Node row : 5 float4 = (c.x, c.y, c.z, r) (D.x, D.y, D.z, A) (Q00, Q01, Q02, Q10) (Q11, Q12, Q20, Q21) (Q22, 0, 0, 0) with
//            A = sum a_t, D = sum a_t n_t, c = sum a_t c_t / A (the mean of the c_t when A = 0), Q = sum (c_t - c) (x) a_t n_t and
//            r = the largest distance of a vertex from c.  Leaves are summed in double in face order; an upper node is formed in
//            double from the double rows of its children in child order (A, D sums; c = sum A_k c_k / A; Q = sum Q_k + (c_k - c)
//            (x) D_k, which is exact; r = max |c_k - c| + r_k).  Every entry is rounded to fp32 once.  One thread per node, no
//            atomics: the same bits on every run.
// Query    : per point q, depth first from the root, children in index order.  At a node, in fp32 with every operation rounded on
//            its own: x = c - q, d2 = (x.x^2 + x.y^2) + x.z^2, far = d2 > (beta r)(beta r).  Far: add
//            ((D . x + tr Q) - 3 (x^T Q x) / d2) / (d2 sqrt(d2)); else a leaf adds solid_angle of its faces in sorted order; else
//            descend.  Terms are fp32, the running sum is double in visiting order, the result is the sum over 4 pi.  The value is
//            a pure function of point, mesh and beta.
// Kernel   : the wave-union walk of cluster_tree.h: a lane holds a node it accepted as far and needs what is below a near one.
#include "cluster_tree.h"

#include <cmath>

namespace {

using ia::blocks; using ia::on_device;
using namespace ia::tree;

constexpr int kBlock = 256;
constexpr int kRow = 20;                             // floats per node row, and doubles per scratch row
constexpr int kNoKey = 1 << 30;                      // key of an unusable triangle / a non-finite point

using V3 = ia::Vec3<float>;
using D3 = ia::Vec3<double>;

// ------------------------------------------------------------------ Morton keys

__device__ __forceinline__ unsigned spread10(unsigned x) {              // bit k of a 10-bit number -> bit 3 k
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__device__ __forceinline__ unsigned axis_cell(float x, float lo, float scale) {
    return (unsigned)fminf(fmaxf(floorf((x - lo) * scale), 0.f), 1023.f);   // (fmaxf drops a NaN: cell 0)
}

__device__ __forceinline__ int morton(V3 p, V3 lo, float scale) {
    return (int)(spread10(axis_cell(p.x, lo.x, scale)) | (spread10(axis_cell(p.y, lo.y, scale)) << 1) |
                 (spread10(axis_cell(p.z, lo.z, scale)) << 2));
}

__global__ __launch_bounds__(kBlock) void face_keys_kernel(const float4* __restrict__ tris, int F, V3 lo, float scale, int* __restrict__ keys) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= F) return;
    const Tri t = load_tri(tris, f);
    const float third = 1.f / 3.f;
    const V3 c = {((t.A.x + t.B.x) + t.C.x) * third, ((t.A.y + t.B.y) + t.C.y) * third, ((t.A.z + t.B.z) + t.C.z) * third};
    keys[f] = t.A.w == 0.f ? kNoKey : morton(c, lo, scale);
}

__global__ __launch_bounds__(kBlock) void point_keys_kernel(const float* __restrict__ pts, int64_t N, V3 lo, float scale, int* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const V3 p = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    keys[i] = finite3(p) ? morton(p, lo, scale) : kNoKey;
}

__global__ __launch_bounds__(kBlock) void gather_kernel(const float4* __restrict__ tris, int F, const int* __restrict__ order,
                                                        float4* __restrict__ sorted) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= F) return;
    const int f = order[s];
    if ((unsigned)f >= (unsigned)F) {                                       // (not a permutation: an unusable triangle)
        sorted[3 * (int64_t)s] = sorted[3 * (int64_t)s + 1] = sorted[3 * (int64_t)s + 2] = {0.f, 0.f, 0.f, 0.f};
        return;
    }
    sorted[3 * (int64_t)s] = tris[3 * (int64_t)f];
    sorted[3 * (int64_t)s + 1] = tris[3 * (int64_t)f + 1];
    sorted[3 * (int64_t)s + 2] = tris[3 * (int64_t)f + 2];
}

// ------------------------------------------------------------------ nodes

__device__ __forceinline__ D3 d3(float4 v) { return {(double)v.x, (double)v.y, (double)v.z}; }
__device__ __forceinline__ D3 add(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 mul(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }

struct Node64 {
    D3 c;
    double r, A;
    D3 D;
    double Q[9];
};

__device__ __forceinline__ void add_outer(double* Q, D3 u, D3 v) {        // Q += u (x) v
    Q[0] += u.x * v.x; Q[1] += u.x * v.y; Q[2] += u.x * v.z;
    Q[3] += u.y * v.x; Q[4] += u.y * v.y; Q[5] += u.y * v.z;
    Q[6] += u.z * v.x; Q[7] += u.z * v.y; Q[8] += u.z * v.z;
}

__device__ __forceinline__ void store_node(const Node64& n, double* __restrict__ row, float4* __restrict__ out) {
    row[0] = n.c.x; row[1] = n.c.y; row[2] = n.c.z; row[3] = n.r;
    row[4] = n.D.x; row[5] = n.D.y; row[6] = n.D.z; row[7] = n.A;
#pragma unroll
    for (int k = 0; k < 9; ++k) row[8 + k] = n.Q[k];
    row[17] = row[18] = row[19] = 0.0;
    out[0] = {(float)n.c.x, (float)n.c.y, (float)n.c.z, (float)n.r};
    out[1] = {(float)n.D.x, (float)n.D.y, (float)n.D.z, (float)n.A};
    out[2] = {(float)n.Q[0], (float)n.Q[1], (float)n.Q[2], (float)n.Q[3]};
    out[3] = {(float)n.Q[4], (float)n.Q[5], (float)n.Q[6], (float)n.Q[7]};
    out[4] = {(float)n.Q[8], 0.f, 0.f, 0.f};
}

// One thread per leaf: two passes over its faces (sums and centre, then Q and r about the centre).
__global__ __launch_bounds__(kBlock) void leaf_kernel(const float4* __restrict__ tris, int Fu, int leaves, double* __restrict__ rows,
                                                      float4* __restrict__ nodes) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= leaves) return;
    const Range fr = leaf_range(i, Fu);
    Node64 n = {};
    D3 S = {0.0, 0.0, 0.0}, M = {0.0, 0.0, 0.0};
    for (int f = fr.lo; f < fr.hi; ++f) {
        const Tri t = load_tri(tris, f);
        const D3 A = d3(t.A), B = d3(t.B), C = d3(t.C);
        const D3 an = mul(cross(sub(B, A), sub(C, A)), 0.5);                // area times unit normal
        const double a = sqrt(dot(an, an));
        const D3 ct = mul(add(add(A, B), C), 1.0 / 3.0);
        n.A += a;
        n.D = add(n.D, an);
        S = add(S, mul(ct, a));
        M = add(M, ct);
    }
    n.c = n.A > 0.0 ? mul(S, 1.0 / n.A) : mul(M, 1.0 / (double)(fr.hi - fr.lo));
    for (int f = fr.lo; f < fr.hi; ++f) {
        const Tri t = load_tri(tris, f);
        const D3 A = d3(t.A), B = d3(t.B), C = d3(t.C);
        const D3 an = mul(cross(sub(B, A), sub(C, A)), 0.5);
        const D3 ct = mul(add(add(A, B), C), 1.0 / 3.0);
        add_outer(n.Q, sub(ct, n.c), an);
        const D3 a = sub(A, n.c), b = sub(B, n.c), c = sub(C, n.c);
        n.r = fmax(n.r, sqrt(fmax(dot(a, a), fmax(dot(b, b), dot(c, c)))));
    }
    store_node(n, rows + (int64_t)i * kRow, nodes + (int64_t)i * 5);
}

// One thread per node of a level above the leaves.  span: faces under a full child.
__global__ __launch_bounds__(kBlock) void upper_kernel(int Fu, int span, int children, int child_start, int count, int start,
                                                       double* __restrict__ rows, float4* __restrict__ nodes) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= count) return;
    const Range kr = child_range(j, children);
    Node64 n = {};
    D3 S = {0.0, 0.0, 0.0}, M = {0.0, 0.0, 0.0};
    double faces = 0.0;
    for (int k = kr.lo; k < kr.hi; ++k) {
        const double* row = rows + (int64_t)(child_start + k) * kRow;
        const D3 ck = {row[0], row[1], row[2]};
        const double nk = (double)(min((int64_t)(k + 1) * span, (int64_t)Fu) - (int64_t)k * span);
        n.A += row[7];
        n.D = add(n.D, D3{row[4], row[5], row[6]});
        S = add(S, mul(ck, row[7]));
        M = add(M, mul(ck, nk));
        faces += nk;
    }
    n.c = n.A > 0.0 ? mul(S, 1.0 / n.A) : mul(M, 1.0 / faces);
    for (int k = kr.lo; k < kr.hi; ++k) {
        const double* row = rows + (int64_t)(child_start + k) * kRow;
        const D3 u = sub(D3{row[0], row[1], row[2]}, n.c);
#pragma unroll
        for (int e = 0; e < 9; ++e) n.Q[e] += row[8 + e];
        add_outer(n.Q, u, D3{row[4], row[5], row[6]});
        n.r = fmax(n.r, sqrt(dot(u, u)) + row[3]);
    }
    store_node(n, rows + (int64_t)(start + j) * kRow, nodes + (int64_t)(start + j) * 5);
}

// ------------------------------------------------------------------ query

constexpr double kFourPi = 4.0 * 3.14159265358979323846;

// counts: int32 [N, 2] = far terms and exact pairs of the point; bound: sum over the far terms of 3 A r^2 / (4 pi (d - r)^4).
__global__ __launch_bounds__(kBlock) void query_kernel(const float* __restrict__ pts, int64_t N, const float4* __restrict__ tris, int Fu,
                                                       const float4* __restrict__ nodes, Tree tree, float beta, double* __restrict__ out,
                                                       double* __restrict__ bound, int* __restrict__ counts) {
    IA_TREE_STAGE(tree);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    V3 q = {0.f, 0.f, 0.f};
    bool ok = false;
    if (i < N) {
        q = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        ok = finite3(q);
    }
    double acc = 0.0, bnd = 0.0;
    int n_far = 0, n_exact = 0;
    IA_TREE_WALK(tree, ok)
        const float4* row = nodes + 5 * (int64_t)node;
        const float4 n0 = row[0], n1 = row[1];
        const V3 x = {n0.x - q.x, n0.y - q.y, n0.z - q.z};
        const float d2 = dot(x, x);
        const float br = beta * n0.w;
        const bool walking = IA_TREE_WALKING;
        const bool hold = walking && d2 > br * br, need = walking && !hold;      // far, near
        if (hold) {
            const float4 n2 = row[2], n3 = row[3], n4 = row[4];
            const V3 D = {n1.x, n1.y, n1.z};
            const V3 Qx = {dot(V3{n2.x, n2.y, n2.z}, x), dot(V3{n2.w, n3.x, n3.y}, x), dot(V3{n3.z, n3.w, n4.x}, x)};
            const float tr = (n2.x + n3.x) + n4.x;
            const float term = ((dot(D, x) + tr) - 3.f * dot(x, Qx) / d2) / (d2 * sqrtf(d2));
            acc += (double)term;
            const double e = sqrt((double)d2) - (double)n0.w;
            bnd += 3.0 * (double)n1.w * ((double)n0.w * (double)n0.w) / (kFourPi * ((e * e) * (e * e)));
            ++n_far;
        }
    IA_TREE_LEAF
        const Range fr = leaf_range(j, Fu);
        for (int f = fr.lo; f < fr.hi; ++f) {
            const float4 A = tris[3 * (int64_t)f], B = tris[3 * (int64_t)f + 1], C = tris[3 * (int64_t)f + 2];     // (load_tri here: 6 more VGPRs)
            if (need) acc += (double)solid_angle(q, xyz(A), xyz(B), xyz(C));
        }
        if (need) n_exact += fr.hi - fr.lo;
    IA_TREE_END(tree, const int count = IA_TREE_COUNT(Fu, l), count)
    if (i >= N) return;
    out[i] = ok ? acc / kFourPi : (double)NAN;
    if (bound) bound[i] = ok ? bnd : (double)NAN;
    if (counts) { counts[2 * i] = n_far; counts[2 * i + 1] = n_exact; }
}

int check_cube(const float* h_lo, float h_scale, const char* what) {
    IA_REQUIRE(h_lo && std::isfinite(h_lo[0]) && std::isfinite(h_lo[1]) && std::isfinite(h_lo[2]), "%s: lo must be three finite floats", what);
    IA_REQUIRE(std::isfinite(h_scale) && h_scale >= 0.f, "%s: scale must be finite and >= 0, got %g", what, (double)h_scale);
    return IA_OK;
}

}  // namespace

extern "C" int ia_winding_tree_layout(int* h_leaf, int* h_branch, int* h_row_floats, int* h_max_levels) {
    IA_REQUIRE(h_leaf && h_branch && h_row_floats && h_max_levels, "ia_winding_tree_layout: the four outputs must not be NULL");
    *h_leaf = kLeaf;
    *h_branch = kBranch;
    *h_row_floats = kRow;
    *h_max_levels = kMaxLevels;
    return IA_OK;
}

extern "C" int ia_winding_tree_plan(int64_t F_usable, int* h_levels, int* h_counts, int64_t* h_nodes, size_t* h_scratch_bytes) {
    if (int e = check_faces(F_usable, "ia_winding_tree_plan")) return e;
    IA_REQUIRE(h_levels && h_counts && h_nodes && h_scratch_bytes, "ia_winding_tree_plan: the four outputs must not be NULL");
    const Levels t = levels_of(F_usable);
    *h_levels = t.n;
    for (int l = 0; l < kMaxLevels; ++l) h_counts[l] = l < t.n ? t.count[l] : 0;
    *h_nodes = t.total;
    *h_scratch_bytes = sizeof(double) * (size_t)kRow * (size_t)t.total;
    return IA_OK;
}

extern "C" int ia_winding_tree_face_keys(const void* tris, int64_t F, const float* h_lo, float h_scale, int* keys, void* stream) {
    IA_REQUIRE(F >= 0 && F <= kMaxFaces, "ia_winding_tree_face_keys: F must be >= 0 and <= 2^25, got %lld", (long long)F);
    if (int e = check_cube(h_lo, h_scale, "ia_winding_tree_face_keys")) return e;
    if (F == 0) return IA_OK;
    if (!on_device(tris) || !on_device(keys)) return ia::fail(IA_ERR_INVALID_ARG, "ia_winding_tree_face_keys: tris and keys must be device pointers");
    face_keys_kernel<<<blocks(F, kBlock), kBlock, 0, (hipStream_t)stream>>>(static_cast<const float4*>(tris), (int)F, V3{h_lo[0], h_lo[1], h_lo[2]},
                                                                            h_scale, keys);
    return ia::check_launch("ia_winding_tree_face_keys");
}

extern "C" int ia_winding_tree_point_keys(const float* points, int64_t N, const float* h_lo, float h_scale, int* keys, void* stream) {
    if (int e = check_points(N, "ia_winding_tree_point_keys")) return e;
    if (int e = check_cube(h_lo, h_scale, "ia_winding_tree_point_keys")) return e;
    if (N == 0) return IA_OK;
    if (!on_device(points) || !on_device(keys)) return ia::fail(IA_ERR_INVALID_ARG, "ia_winding_tree_point_keys: points and keys must be device pointers");
    point_keys_kernel<<<blocks(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(points, N, V3{h_lo[0], h_lo[1], h_lo[2]}, h_scale, keys);
    return ia::check_launch("ia_winding_tree_point_keys");
}

extern "C" int ia_winding_tree_gather(const void* tris, int64_t F, const int* order, void* sorted, void* stream) {
    IA_REQUIRE(F >= 0 && F <= kMaxFaces, "ia_winding_tree_gather: F must be >= 0 and <= 2^25, got %lld", (long long)F);
    if (F == 0) return IA_OK;
    if (!on_device(tris) || !on_device(order) || !on_device(sorted))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_winding_tree_gather: tris, order and sorted must be device pointers");
    IA_REQUIRE(tris != sorted, "ia_winding_tree_gather: sorted must not be tris");
    gather_kernel<<<blocks(F, kBlock), kBlock, 0, (hipStream_t)stream>>>(static_cast<const float4*>(tris), (int)F, order,
                                                                         static_cast<float4*>(sorted));
    return ia::check_launch("ia_winding_tree_gather");
}

extern "C" int ia_winding_tree_nodes(const void* sorted, int64_t F_usable, void* scratch, size_t scratch_bytes, void* nodes, int64_t n_nodes,
                                     void* stream) {
    if (int e = check_faces(F_usable, "ia_winding_tree_nodes")) return e;
    const Levels t = levels_of(F_usable);
    if (int e = check_nodes(t, F_usable, n_nodes, "ia_winding_tree_nodes")) return e;
    const size_t need = sizeof(double) * (size_t)kRow * (size_t)t.total;
    if (scratch_bytes < need) return ia::fail(IA_ERR_INVALID_ARG, "ia_winding_tree_nodes: scratch holds %zu bytes, needs %zu", scratch_bytes, need);
    if (t.n == 0) return IA_OK;
    if (!on_device(sorted) || !on_device(scratch) || !on_device(nodes))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_winding_tree_nodes: sorted, scratch and nodes must be device pointers");
    hipStream_t st = (hipStream_t)stream;
    double* rows = static_cast<double*>(scratch);
    float4* out = static_cast<float4*>(nodes);
    leaf_kernel<<<blocks(t.count[0], kBlock), kBlock, 0, st>>>(static_cast<const float4*>(sorted), (int)F_usable, t.count[0], rows, out);
    if (int e = ia::check_launch("ia_winding_tree_nodes (leaves)")) return e;
    int64_t span = kLeaf;
    for (int l = 1; l < t.n; ++l, span *= kBranch) {
        upper_kernel<<<blocks(t.count[l], kBlock), kBlock, 0, st>>>((int)F_usable, (int)span, t.count[l - 1], t.start[l - 1], t.count[l], t.start[l],
                                                                    rows, out);
        if (int e = ia::check_launch("ia_winding_tree_nodes (level)")) return e;
    }
    return IA_OK;
}

extern "C" int ia_winding_tree_query(const float* points, int64_t N, const void* sorted, int64_t F_usable, const void* nodes, int64_t n_nodes,
                                     float beta, double* out, double* bound, int* counts, void* stream) {
    if (int e = check_points(N, "ia_winding_tree_query")) return e;
    if (int e = check_faces(F_usable, "ia_winding_tree_query")) return e;
    IA_REQUIRE(beta > 1.f, "ia_winding_tree_query: beta must be greater than 1 (inf: never far), got %g", (double)beta);
    const Levels t = levels_of(F_usable);
    if (int e = check_nodes(t, F_usable, n_nodes, "ia_winding_tree_query")) return e;
    if (N == 0) return IA_OK;
    if (!on_device(points) || !on_device(out) || (bound && !on_device(bound)) || (counts && !on_device(counts)) ||
        (t.n && (!on_device(sorted) || !on_device(nodes))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_winding_tree_query: points, sorted, nodes, out, bound and counts must be device pointers");
    query_kernel<<<blocks(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(points, N, static_cast<const float4*>(sorted), (int)F_usable,
                                                                        static_cast<const float4*>(nodes), tree_of(t), beta, out, bound, counts);
    return ia::check_launch("ia_winding_tree_query");
}
