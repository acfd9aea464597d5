// Closest point on the cluster tree: the exact point-to-mesh distance of surface_distance.hip by branch and bound over the implicit
// tree of cluster_tree.h.  No counterpart in the reference; the definition is geometry._closest_tree_numpy.
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
// Walk     : the wave-union walk of cluster_tree.h: a lane holds a node it skipped and needs what is below any other; each lane
//            compares against its own best and passes over its seed leaf.  counts = (boxes tested, point-triangle pairs evaluated) of
//            the lane's own traversal, seed included: they do not depend on the other lanes.
#include "cluster_tree.h"

#include <cmath>

namespace {

using ia::blocks; using ia::on_device;
using namespace ia::tree;

constexpr int kBlock = 256;

using V3 = ia::Vec3<float>;

// ------------------------------------------------------------------ boxes

__global__ __launch_bounds__(kBlock) void leaf_box_kernel(const float4* __restrict__ tris, int Fu, int leaves, float4* __restrict__ boxes) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= leaves) return;
    const Range fr = leaf_range(i, Fu);
    V3 lo = {INFINITY, INFINITY, INFINITY}, hi = {-INFINITY, -INFINITY, -INFINITY};
    for (int f = fr.lo; f < fr.hi; ++f)
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
    const Range kr = child_range(j, children);
    V3 lo = {INFINITY, INFINITY, INFINITY}, hi = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = kr.lo; k < kr.hi; ++k) {
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

// The faces of leaf j against p: the smaller pair (distance, input face) stays.  Returns the number of faces.
__device__ __forceinline__ int leaf_faces(V3 p, const float4* __restrict__ tris, const int* __restrict__ order, int Fu, int j, bool take,
                                          Best& best) {
    const Range fr = leaf_range(j, Fu);
    for (int f = fr.lo; f < fr.hi; ++f) {
        const Tri t = load_tri(tris, f);
        const int face = order[f];
        V3 q;
        const float d = tri_dist(p, xyz(t.A), xyz(t.B), xyz(t.C), q);
        if (take && (d < best.d || (d == best.d && face < best.face))) best = {d, face, f};
    }
    return fr.hi - fr.lo;
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
    IA_TREE_STAGE(tree);
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
            const Range kr = {j * kBranch, min(j * kBranch + kBranch, level_count(u.Fu, l - 1))};   // (child_range, j * kBranch first)
            const float4* row = u.boxes + 2 * (int64_t)s_start[l - 1];
            float least = INFINITY;
            j = kr.lo;
            for (int k = kr.lo; k < kr.hi; ++k) {
                const float lb = box_dist(p, row[2 * (int64_t)k], row[2 * (int64_t)k + 1]);
                if (lb < least) { least = lb; j = k; }
            }
            n_box += kr.hi - kr.lo;
        }
        seed = j;
        n_pair += leaf_faces(p, u.tris, u.order, u.Fu, j, true, best);
    }
    IA_TREE_WALK(tree, ok)
        const float4* row = u.boxes + 2 * (int64_t)node;
        const float lb = box_dist(p, row[0], row[1]);
        const bool mine = IA_TREE_WALKING && !(l == 0 && j == seed);
        const bool hold = mine && lb < INFINITY && lb - slack > best.d, need = mine && !hold;      // skipped, entered
        if (mine) ++n_box;
    IA_TREE_LEAF
        const int faces = leaf_faces(p, u.tris, u.order, u.Fu, j, need, best);
        if (need) n_pair += faces;
    IA_TREE_END(tree, , level_count(u.Fu, l))
    if (i >= u.N) return;
    V3 q = {NAN, NAN, NAN};
    if (best.face >= 0) {
        const Tri t = load_tri(u.tris, best.at);
        tri_dist(p, xyz(t.A), xyz(t.B), xyz(t.C), q);
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
    if (int e = check_faces(F_usable, "ia_tree_boxes")) return e;
    const Levels t = levels_of(F_usable);
    if (int e = check_nodes(t, F_usable, n_nodes, "ia_tree_boxes")) return e;
    if (t.n == 0) return IA_OK;
    if (!on_device(sorted) || !on_device(boxes)) return ia::fail(IA_ERR_INVALID_ARG, "ia_tree_boxes: sorted and boxes must be device pointers");
    hipStream_t st = (hipStream_t)stream;
    float4* out = static_cast<float4*>(boxes);
    leaf_box_kernel<<<blocks(t.count[0], kBlock), kBlock, 0, st>>>(static_cast<const float4*>(sorted), (int)F_usable, t.count[0], out);
    if (int e = ia::check_launch("ia_tree_boxes (leaves)")) return e;
    for (int l = 1; l < t.n; ++l) {
        upper_box_kernel<<<blocks(t.count[l], kBlock), kBlock, 0, st>>>(t.count[l - 1], t.start[l - 1], t.count[l], t.start[l], out);
        if (int e = ia::check_launch("ia_tree_boxes (level)")) return e;
    }
    return IA_OK;
}

extern "C" int ia_closest_point_tree(const float* points, int64_t N, const void* sorted, const int* order, int64_t F_usable, const void* boxes,
                                     int64_t n_nodes, float mesh_extent, float* dist, int* face, float* point, int* counts, void* stream) {
    if (int e = check_points(N, "ia_closest_point_tree")) return e;
    if (int e = check_faces(F_usable, "ia_closest_point_tree")) return e;
    IA_REQUIRE(mesh_extent >= 0.f && std::isfinite(mesh_extent), "ia_closest_point_tree: mesh_extent must be finite and >= 0");
    const Levels t = levels_of(F_usable);
    if (int e = check_nodes(t, F_usable, n_nodes, "ia_closest_point_tree")) return e;
    if (N == 0) return IA_OK;
    if (!on_device(points) || !on_device(dist) || !on_device(face) || !on_device(point) || (counts && !on_device(counts)) ||
        (t.n && (!on_device(sorted) || !on_device(order) || !on_device(boxes))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_closest_point_tree: points, sorted, order, boxes, dist, face, point and counts must be device pointers");
    Query u{points, N, static_cast<const float4*>(sorted), order, (int)F_usable, static_cast<const float4*>(boxes), mesh_extent, dist, face, point,
            counts};
    closest_tree_kernel<<<blocks(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(u, tree_of(t));
    return ia::check_launch("ia_closest_point_tree");
}
