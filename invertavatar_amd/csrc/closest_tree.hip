// Closest point on the cluster tree: the exact point-to-mesh distance of surface_distance.hip by branch and bound over the implicit
// tree of winding_tree.hip.  No counterpart in the reference; the definition is geometry._closest_tree_numpy.
//
// The result is what ia_closest_point gives: the minimum over ALL usable triangles of the one fp32 function tri_dist (geom_common.h),
// taken on the pair (distance, input face index).  The tree only decides which triangles need not be looked at, so the answer is
// bit-identical to the brute mode and to the grid, for every order of the walk and from run to run.
//
// Boxes    : two float4 per node of the level layout of ia_winding_tree_plan, (lo.xyz, 0) (hi.xyz, 0).  A leaf takes the min / max per
//            axis over the vertices of its (at most L) sorted faces, an upper node over its (at most B) children, level by level.  Min
//            and max are exact and independent of order: the same bits on every run.  One thread per node.
// Skip     : lb = the distance from p to the box, in fp32 with every operation rounded on its own: g = max(max(lo - p, p - hi), 0)
//            per axis, lb = sqrt((gx^2 + gy^2) + gz^2).  A node is skipped iff lb is finite and lb - slack > best.dist with
//            slack = 2^-17 max(|p|_inf, mesh_extent) (= 64 eps32 times that, the margin of the grid).  tri_dist undershoots the true
//            distance by at most 16 eps32 extent (asserted; 3.3 measured) and lb overshoots the true box distance by a few eps32 of
//            its own size, so a skipped node holds no triangle whose computed distance is <= best.dist: neither the minimum nor the
//            tie can change.  A comparison with best = +inf or with an lb that overflowed is false: the node is entered, which is
//            always safe (and needed: far beyond 1.8e19 the squares overflow while the plane branch of tri_dist stays finite).
// Seed     : each lane descends from the root to the child with the smallest lb (the lowest index among equals) and evaluates that
//            one leaf, so that best is finite before anything is pruned.
// Walk     : the wave-union walk of winding_tree.hip without a stack: (level, index) are wave-uniform, depth first with children in
//            index order; a node's children are entered while the ballot of lanes that cannot skip it is non-zero, and a lane that
//            skipped a node stays masked until the walk leaves that subtree.  Box rows, leaf triangles and their input indices are
//            wave-uniform loads; each lane compares against its own best and passes over its seed leaf.  counts = (boxes tested,
//            point-triangle pairs evaluated) of the lane's own traversal, seed included: they do not depend on the other lanes.
#include "geom_common.h"

#include <cmath>

namespace {

using ia::blocks; using ia::on_device;

constexpr int kBlock = 256;
constexpr int kLeaf = 32, kBranch = 8;               // the layout of winding_tree.hip (checked against ia_winding_tree_layout)
constexpr int kLeafShift = 5, kBranchShift = 3;
constexpr int kMaxLevels = 8;
constexpr int64_t kMaxFaces = (int64_t)1 << 25;
static_assert((1 << kLeafShift) == kLeaf && (1 << kBranchShift) == kBranch, "shifts");

using V3 = ia::Vec3<float>;

struct Tree {
    int top;                                         // level of the root; -1: no node
    int start[kMaxLevels];
};

// Host: the levels of F_usable faces from ia_winding_tree_plan, after checking that the layout is the one compiled in here.
int plan(const char* what, int64_t Fu, int64_t n_nodes, Tree& tree, int* counts) {
    int leaf = 0, branch = 0, row = 0, max_levels = 0;
    if (int e = ia_winding_tree_layout(&leaf, &branch, &row, &max_levels)) return e;
    if (leaf != kLeaf || branch != kBranch || max_levels != kMaxLevels)
        return ia::fail(IA_ERR_UNSUPPORTED, "%s: the tree layout (%d, %d, %d) is not the one this file was built for", what, leaf, branch, max_levels);
    int levels = 0;
    int64_t total = 0;
    size_t bytes = 0;
    if (int e = ia_winding_tree_plan(Fu, &levels, counts, &total, &bytes)) return e;
    IA_REQUIRE(n_nodes == total, "%s: %lld usable faces make %lld nodes, got n_nodes = %lld", what, (long long)Fu, (long long)total,
               (long long)n_nodes);
    tree.top = levels - 1;
    int at = 0;
    for (int l = 0; l < kMaxLevels; ++l) {
        tree.start[l] = at;
        at += l < levels ? counts[l] : 0;
    }
    return IA_OK;
}

__device__ __forceinline__ V3 xyz(float4 v) { return {v.x, v.y, v.z}; }

// Nodes of level l over Fu faces.
__device__ __forceinline__ int level_count(int Fu, int l) { return (Fu + (kLeaf << (kBranchShift * l)) - 1) >> (kLeafShift + kBranchShift * l); }

// ------------------------------------------------------------------ boxes

__global__ __launch_bounds__(kBlock) void leaf_box_kernel(const float4* __restrict__ tris, int Fu, int leaves, float4* __restrict__ boxes) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= leaves) return;
    const int f0 = i * kLeaf, f1 = min(f0 + kLeaf, Fu);
    V3 lo = {INFINITY, INFINITY, INFINITY}, hi = {-INFINITY, -INFINITY, -INFINITY};
    for (int f = f0; f < f1; ++f)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 v = tris[3 * (int64_t)f + k];
            lo = {fminf(lo.x, v.x), fminf(lo.y, v.y), fminf(lo.z, v.z)};
            hi = {fmaxf(hi.x, v.x), fmaxf(hi.y, v.y), fmaxf(hi.z, v.z)};
        }
    boxes[2 * (int64_t)i] = {lo.x, lo.y, lo.z, 0.f};
    boxes[2 * (int64_t)i + 1] = {hi.x, hi.y, hi.z, 0.f};
}

__global__ __launch_bounds__(kBlock) void upper_box_kernel(int children, int child_start, int count, int start, float4* __restrict__ boxes) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= count) return;
    const int k0 = j * kBranch, k1 = min(k0 + kBranch, children);
    V3 lo = {INFINITY, INFINITY, INFINITY}, hi = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = k0; k < k1; ++k) {
        const float4 a = boxes[2 * (int64_t)(child_start + k)], b = boxes[2 * (int64_t)(child_start + k) + 1];
        lo = {fminf(lo.x, a.x), fminf(lo.y, a.y), fminf(lo.z, a.z)};
        hi = {fmaxf(hi.x, b.x), fmaxf(hi.y, b.y), fmaxf(hi.z, b.z)};
    }
    boxes[2 * (int64_t)(start + j)] = {lo.x, lo.y, lo.z, 0.f};
    boxes[2 * (int64_t)(start + j) + 1] = {hi.x, hi.y, hi.z, 0.f};
}

// ------------------------------------------------------------------ query

// Distance from p to the box [lo, hi]: every operation rounded on its own.
__device__ __forceinline__ float box_dist(V3 p, float4 lo, float4 hi) {
    const float gx = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.f), gy = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.f),
                gz = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.f);
    return sqrtf((gx * gx + gy * gy) + gz * gz);
}

struct Best {
    float d;
    int face, at;                                    // input face index, and its sorted position
};

// The faces of leaf j against p: the smaller pair (distance, input face) stays.
__device__ __forceinline__ void leaf_faces(V3 p, const float4* __restrict__ tris, const int* __restrict__ order, int Fu, int j, bool take,
                                           Best& best) {
    const int f0 = j * kLeaf, f1 = min(f0 + kLeaf, Fu);
    for (int f = f0; f < f1; ++f) {
        const float4 A = tris[3 * (int64_t)f], B = tris[3 * (int64_t)f + 1], C = tris[3 * (int64_t)f + 2];
        const int t = order[f];
        V3 q;
        const float d = tri_dist(p, xyz(A), xyz(B), xyz(C), q);
        if (take && (d < best.d || (d == best.d && t < best.face))) best = {d, t, f};
    }
}

struct Query {
    const float* pts;
    int64_t N;
    const float4* tris;                              // sorted
    const int* order;
    int Fu;
    const float4* boxes;
    float mesh_extent;
    float* dist;
    int* face;
    float* point;
    int* counts;                                     // [N,2] or null
};

__global__ __launch_bounds__(kBlock) void closest_tree_kernel(Query u, Tree tree) {
    __shared__ int s_start[kMaxLevels];
    if (threadIdx.x < kMaxLevels) s_start[threadIdx.x] = tree.start[threadIdx.x];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    V3 p = {0.f, 0.f, 0.f};
    bool ok = false;
    if (i < u.N) {
        p = {u.pts[3 * i], u.pts[3 * i + 1], u.pts[3 * i + 2]};
        ok = finite3(p);
    }
    const float slack = 7.62939453125e-6f * fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fmaxf(fabsf(p.z), u.mesh_extent));     // 2^-17 = 64 eps32
    Best best = {INFINITY, -1, -1};
    int n_box = 0, n_pair = 0;
    int seed = -1;                                   // the leaf of the greedy descent
    if (ok && tree.top >= 0) {
        int j = 0;
        for (int l = tree.top; l > 0; --l) {         // (the same number of levels in every lane; the child differs)
            const int k0 = j * kBranch, k1 = min(k0 + kBranch, level_count(u.Fu, l - 1));
            const float4* row = u.boxes + 2 * (int64_t)s_start[l - 1];
            float least = INFINITY;
            j = k0;
            for (int k = k0; k < k1; ++k) {
                const float lb = box_dist(p, row[2 * (int64_t)k], row[2 * (int64_t)k + 1]);
                if (lb < least) { least = lb; j = k; }
            }
            n_box += k1 - k0;
        }
        seed = j;
        leaf_faces(p, u.tris, u.order, u.Fu, j, true, best);
        n_pair += min((j + 1) * kLeaf, u.Fu) - j * kLeaf;
    }
    int held = ok ? -1 : kMaxLevels;                 // level of the node this lane skipped and waits under; -1: walking; kMaxLevels: never walks
    int l = tree.top, j = 0;                         // (wave-uniform)
    while (l >= 0) {
        const float4* row = u.boxes + 2 * (int64_t)(__builtin_amdgcn_readfirstlane(s_start[l]) + j);
        const float lb = box_dist(p, row[0], row[1]);
        const bool walking = held < 0 && !(l == 0 && j == seed);
        const bool skip = walking && lb < INFINITY && lb - slack > best.d;
        const bool need = walking && !skip;
        if (walking) ++n_box;
        if (skip) held = l;
        if (l > 0) {
            if (__ballot(need)) {                    // some lane needs the children
                --l;
                j *= kBranch;
                continue;
            }
        } else if (__ballot(need)) {
            leaf_faces(p, u.tris, u.order, u.Fu, j, need, best);        // (the same triangles in every lane)
            if (need) n_pair += min((j + 1) * kLeaf, u.Fu) - j * kLeaf;
        }
        for (;;) {                                   // the subtree of (l, j) is done: the next node in depth-first order
            if (held == l) held = -1;
            if (l == tree.top) { l = -1; break; }
            if (((j + 1) & (kBranch - 1)) != 0 && j + 1 < level_count(u.Fu, l)) { ++j; break; }
            j >>= kBranchShift;
            ++l;
        }
    }
    if (i >= u.N) return;
    V3 q = {NAN, NAN, NAN};
    if (best.face >= 0) {
        const float4 A = u.tris[3 * (int64_t)best.at], B = u.tris[3 * (int64_t)best.at + 1], C = u.tris[3 * (int64_t)best.at + 2];
        tri_dist(p, xyz(A), xyz(B), xyz(C), q);
    }
    u.dist[i] = ok ? best.d : NAN;
    u.face[i] = best.face;
    u.point[3 * i] = p.x + q.x;
    u.point[3 * i + 1] = p.y + q.y;
    u.point[3 * i + 2] = p.z + q.z;
    if (u.counts) { u.counts[2 * i] = n_box; u.counts[2 * i + 1] = n_pair; }
}

}  // namespace

extern "C" int ia_tree_boxes(const void* sorted, int64_t F_usable, void* boxes, int64_t n_nodes, void* stream) {
    IA_REQUIRE(F_usable >= 0 && F_usable <= kMaxFaces, "ia_tree_boxes: F_usable must be >= 0 and <= 2^25, got %lld", (long long)F_usable);
    Tree tree = {};
    int counts[kMaxLevels] = {};
    if (int e = plan("ia_tree_boxes", F_usable, n_nodes, tree, counts)) return e;
    if (tree.top < 0) return IA_OK;
    if (!on_device(sorted) || !on_device(boxes)) return ia::fail(IA_ERR_INVALID_ARG, "ia_tree_boxes: sorted and boxes must be device pointers");
    hipStream_t st = (hipStream_t)stream;
    float4* out = static_cast<float4*>(boxes);
    leaf_box_kernel<<<blocks(counts[0], kBlock), kBlock, 0, st>>>(static_cast<const float4*>(sorted), (int)F_usable, counts[0], out);
    if (int e = ia::check_launch("ia_tree_boxes (leaves)")) return e;
    for (int l = 1; l <= tree.top; ++l) {
        upper_box_kernel<<<blocks(counts[l], kBlock), kBlock, 0, st>>>(counts[l - 1], tree.start[l - 1], counts[l], tree.start[l], out);
        if (int e = ia::check_launch("ia_tree_boxes (level)")) return e;
    }
    return IA_OK;
}

extern "C" int ia_closest_point_tree(const float* points, int64_t N, const void* sorted, const int* order, int64_t F_usable, const void* boxes,
                                     int64_t n_nodes, float mesh_extent, float* dist, int* face, float* point, int* counts, void* stream) {
    IA_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) / 3, "ia_closest_point_tree: N must be >= 0 and 3 N < 2^31, got %lld", (long long)N);
    IA_REQUIRE(F_usable >= 0 && F_usable <= kMaxFaces, "ia_closest_point_tree: F_usable must be >= 0 and <= 2^25, got %lld", (long long)F_usable);
    IA_REQUIRE(mesh_extent >= 0.f && std::isfinite(mesh_extent), "ia_closest_point_tree: mesh_extent must be finite and >= 0");
    Tree tree = {};
    int level_counts[kMaxLevels] = {};
    if (int e = plan("ia_closest_point_tree", F_usable, n_nodes, tree, level_counts)) return e;
    if (N == 0) return IA_OK;
    if (!on_device(points) || !on_device(dist) || !on_device(face) || !on_device(point) || (counts && !on_device(counts)) ||
        (tree.top >= 0 && (!on_device(sorted) || !on_device(order) || !on_device(boxes))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_closest_point_tree: points, sorted, order, boxes, dist, face, point and counts must be device pointers");
    Query u{points, N, static_cast<const float4*>(sorted), order, (int)F_usable, static_cast<const float4*>(boxes), mesh_extent, dist, face, point,
            counts};
    closest_tree_kernel<<<blocks(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(u, tree);
    return ia::check_launch("ia_closest_point_tree");
}
