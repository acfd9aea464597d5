// Rays against the mesh on the cluster tree: first hit and any hit by the wave-union walk of cluster_tree.h over the boxes of
// ia_tree_boxes, and the rays of the ambient-occlusion estimate.  No counterpart in the reference; the definition is
// geometry._ray_mesh_numpy, the walk geometry._ray_tree_numpy.
//
// The result is defined without the tree: the smallest pair (t, input face index) over ALL usable triangles that the one fp32 function
// ray_tri (geom_common.h) accepts within the ray's own interval [t_lo, t_hi]; "any" is the bool "some triangle is accepted".
// ray_mesh_brute_kernel states exactly that; the tree only decides which triangles need not be looked at.  ray_tri is NOT watertight:
// the three edge signs of one triangle are rounded separately, so a ray aimed at a shared edge or vertex can miss both neighbours.
//
// Skip     : per lane, M = max(|o|_inf, mesh_extent), s = 2^-12 M.  Per axis k, in fp32 with every operation rounded on its own:
//            g0 = ((lo_k - o_k) - s), g1 = ((hi_k - o_k) + s), t0 = g0 inv_k, t1 = g1 inv_k with inv_k = 1 / d_k; the axis admits
//            [min(t0, t1), max(t0, t1)], or every t when t0 or t1 is a NaN (0 inf: the origin on a grown plane of an axis it does not
//            move along), when inv_k overflowed for d_k != 0, or when |t0|, |t1| or |inv_k| is below 2^-100 (products and
//            reciprocals near the subnormal range carry no relative accuracy).  near = the largest lower end, far = the smallest
//            upper end; near' = near (1 -+ 2^-20) and far' = far (1 +- 2^-20), each moved outward.  The node is skipped iff
//                near' > far'   or   near' > min(t_hi, best.t)   or   far' < t_lo.
//            A NaN makes every comparison false: the node is entered, which is always safe.  d_k = 0 gives inv_k = +-inf and
//            t0, t1 = +-inf: both of one sign (the origin outside the grown slab: nothing below can be met) or -inf, +inf (inside).
// Why      : ray_tri accepts a triangle T only if the computed point p^ = fl(o + fl(t^ d)) lies in T's own box grown by
//            g = 2^-14 max(|o|_inf, |A|_inf, |B|_inf, |C|_inf) <= 2^-14 M (its last clause; the comparison itself adds at most
//            4 eps32 M).  p^ is then bounded by 2 M, so it differs from the exact o + t^ d by at most 8 eps32 M per axis: the exact
//            point lies within 2^-14 M + 12 eps32 M < s / 2 = 2^-13 M of T's box, and of the box of every node above T, which
//            contains T's.  g0 and g1 carry at most 2 eps32 (2 M + s) of rounding, far below s / 2: g0 <= lo_k - o_k - s/2 and
//            g1 >= hi_k - o_k + s/2, so the exact interval g0 / d_k .. g1 / d_k contains t^.  t0 and t1 differ from those quotients
//            by three roundings, relatively 3 eps32 < 2^-20 / 4, as all three are at least 2^-100 in size.  Hence
//            near' <= t^ <= far', and t_lo <= t^ <= min(t_hi, best.t) for a triangle that can still change best: none of the three
//            conditions holds and the node is entered.  This holds for every origin, direction and triangle: the tree returns the
//            brute kernel's bits.  Without the box clause no test on boxes could be sound: the edge functions carry an absolute
//            error near 8 eps32 |d| |b| |c|, so from far away, or for small or grazing triangles, they accept triangles that the
//            ray misses by any distance, with a t^ that has nothing to do with the triangle.
// Walk     : the wave-union walk of cluster_tree.h, children in index order (not front to back: the walk stays shared).  first: a
//            lane holds a node it skipped and needs what is below any other; the leaf loop keeps the smaller (t, face).  any: a lane
//            that has found a hit holds every node from then on, so the wave ends when all its lanes are done.  counts = (boxes
//            tested, ray-triangle pairs of the leaves entered) of the lane's own traversal.
#include "cluster_tree.h"

#include <cmath>

namespace {

using ia::blocks; using ia::on_device;
using namespace ia::tree;

constexpr int kBlock = 256;

using V3 = ia::Vec3<float>;

struct Ray {
    V3 o, d;
    float t_lo, t_hi;
};

struct Best {
    float t;
    int face, at;                                    // input face index, and its sorted position
};

struct Query {
    const float* origins;
    const float* dirs;
    const float* t_lo;
    const float* t_hi;
    int64_t N;
    const float4* tris;                              // sorted
    const int* order;
    int Fu;
    const float4* boxes;                             // (tree only)
    float mesh_extent;
    unsigned char* hit;
    float* t;                                        // t, face, bary, point: null in the any mode
    int* face;
    float* bary;
    float* point;
    int* counts;                                     // [N,2] or null (tree only)
};

// The ray of lane i; false for a ray that is not walked: past the end, a non-finite origin or direction, a NaN interval end.
__device__ __forceinline__ bool load_ray(const Query& u, int64_t i, Ray& r) {
    r = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 0.f, 0.f};
    if (i >= u.N) return false;
    r.o = {u.origins[3 * i], u.origins[3 * i + 1], u.origins[3 * i + 2]};
    r.d = {u.dirs[3 * i], u.dirs[3 * i + 1], u.dirs[3 * i + 2]};
    r.t_lo = u.t_lo[i];
    r.t_hi = u.t_hi[i];
    return finite3(r.o) && finite3(r.d) && r.t_lo == r.t_lo && r.t_hi == r.t_hi;
}

// Sorted faces [lo, hi) against the ray (the same triangles in every lane): the smaller pair (t, input face) stays; in the any mode
// a lane that has a hit takes no more.
template <bool kAny>
__device__ __forceinline__ void faces_against(const Ray& r, const float4* __restrict__ tris, const int* __restrict__ order, Range fr, bool take,
                                              Best& best) {
    for (int f = fr.lo; f < fr.hi; ++f) {
        const Tri tr = load_tri(tris, f);
        const int face = order[f];
        float t;
        V3 w;
        const bool hit = ray_tri(r.o, r.d, r.t_lo, r.t_hi, xyz(tr.A), xyz(tr.B), xyz(tr.C), t, w);
        if (kAny) {
            if (take && hit && best.face < 0) best = {t, face, f};
        } else if (take && hit && (t < best.t || (t == best.t && face < best.face))) {
            best = {t, face, f};
        }
    }
}

__device__ __forceinline__ void store(const Query& u, int64_t i, const Ray& r, bool ok, const Best& best, bool any) {
    u.hit[i] = best.face >= 0 ? 1 : 0;
    if (any) return;
    float t = ok ? INFINITY : NAN;
    V3 bary = {NAN, NAN, NAN}, point = {NAN, NAN, NAN};
    if (best.face >= 0) {
        const Tri tr = load_tri(u.tris, best.at);
        V3 w;
        ray_tri(r.o, r.d, r.t_lo, r.t_hi, xyz(tr.A), xyz(tr.B), xyz(tr.C), t, w);
        const float W = (w.x + w.y) + w.z;
        bary = {w.x / W, w.y / W, w.z / W};
        point = {r.o.x + t * r.d.x, r.o.y + t * r.d.y, r.o.z + t * r.d.z};
    }
    u.t[i] = t;
    u.face[i] = best.face;
    u.bary[3 * i] = bary.x;
    u.bary[3 * i + 1] = bary.y;
    u.bary[3 * i + 2] = bary.z;
    u.point[3 * i] = point.x;
    u.point[3 * i + 1] = point.y;
    u.point[3 * i + 2] = point.z;
}

// ------------------------------------------------------------------ the definition on the device

template <bool kAny>
__global__ __launch_bounds__(kBlock) void ray_mesh_brute_kernel(Query u) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    Ray r;
    const bool ok = load_ray(u, i, r);
    Best best = {INFINITY, -1, -1};
    faces_against<kAny>(r, u.tris, u.order, {0, u.Fu}, ok, best);
    if (i < u.N) store(u, i, r, ok, best, kAny);
}

// ------------------------------------------------------------------ the tree

constexpr float kTiny = 7.888609052210118e-31f;                                          // 2^-100
constexpr float kIn = 0.99999904632568359375f, kOut = 1.00000095367431640625f;          // 1 -+ 2^-20

// One axis of the slab test (see the header): narrows [near, far].
__device__ __forceinline__ void slab_axis(float lo, float hi, float o, float d, float inv, float s, float& near, float& far) {
    float t0 = ((lo - o) - s) * inv, t1 = ((hi - o) + s) * inv;
    if (t0 != t0 || t1 != t1 || (d != 0.f && isinf(inv)) || fminf(fminf(fabsf(t0), fabsf(t1)), fabsf(inv)) < kTiny) { t0 = -INFINITY; t1 = INFINITY; }
    near = fmaxf(near, fminf(t0, t1));
    far = fminf(far, fmaxf(t0, t1));
}

// The node's box holds no triangle the ray could accept with t_lo <= t <= t_max.
__device__ __forceinline__ bool slab_skip(const Ray& r, V3 inv, float s, float4 lo, float4 hi, float t_max) {
    float near = -INFINITY, far = INFINITY;
    slab_axis(lo.x, hi.x, r.o.x, r.d.x, inv.x, s, near, far);
    slab_axis(lo.y, hi.y, r.o.y, r.d.y, inv.y, s, near, far);
    slab_axis(lo.z, hi.z, r.o.z, r.d.z, inv.z, s, near, far);
    near *= near > 0.f ? kIn : kOut;
    far *= far > 0.f ? kOut : kIn;
    return near > far || near > t_max || far < r.t_lo;
}

template <bool kAny>
__global__ __launch_bounds__(kBlock) void ray_mesh_tree_kernel(Query u, Tree tree) {
    IA_TREE_STAGE(tree);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    Ray r;
    const bool ok = load_ray(u, i, r);
    const float M = fmaxf(fmaxf(fabsf(r.o.x), fabsf(r.o.y)), fmaxf(fabsf(r.o.z), u.mesh_extent));
    const float slack = 2.44140625e-4f * M;                                                // 2^-12 M
    const V3 inv = {1.f / r.d.x, 1.f / r.d.y, 1.f / r.d.z};
    Best best = {INFINITY, -1, -1};
    int n_box = 0, n_pair = 0;
    IA_TREE_WALK(tree, ok)
        const float4* row = u.boxes + 2 * (int64_t)node;
        const bool mine = IA_TREE_WALKING && !(kAny && best.face >= 0);                    // (a lane with a hit tests no more boxes)
        const bool skip = slab_skip(r, inv, slack, row[0], row[1], fminf(r.t_hi, best.t));
        const bool hold = IA_TREE_WALKING && (!mine || skip), need = mine && !skip;
        if (mine) ++n_box;
    IA_TREE_LEAF
        const Range fr = leaf_range(j, u.Fu);
        faces_against<kAny>(r, u.tris, u.order, fr, need, best);
        if (need) n_pair += fr.hi - fr.lo;
    IA_TREE_END(tree, , level_count(u.Fu, l))
    if (i >= u.N) return;
    store(u, i, r, ok, best, kAny);
    if (u.counts) { u.counts[2 * i] = n_box; u.counts[2 * i + 1] = n_pair; }
}

// ------------------------------------------------------------------ the rays of the ambient-occlusion estimate

// Ray v S + s: origin = vertex v + bias n, direction = (t1 x + t2 y) + n z for the table's direction (x, y, z), with (t1, t2, n) the
// branch-free orthonormal basis of Duff et al. (2017); every operation rounded on its own.  A non-finite normal gives NaN rays.
__global__ __launch_bounds__(kBlock) void ao_rays_kernel(const float* __restrict__ verts, const float* __restrict__ normals, int64_t rays, int S,
                                                         const float* __restrict__ table, float bias, float* __restrict__ origins,
                                                         float* __restrict__ dirs) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= rays) return;
    const int64_t v = i / S;
    const int s = (int)(i - v * S);
    const V3 p = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]}, n = {normals[3 * v], normals[3 * v + 1], normals[3 * v + 2]};
    const V3 c = {table[3 * s], table[3 * s + 1], table[3 * s + 2]};
    V3 o = {NAN, NAN, NAN}, d = {NAN, NAN, NAN};
    if (finite3(n)) {
        const float sign = copysignf(1.f, n.z);
        const float a = -1.f / (sign + n.z);
        const float b = (n.x * n.y) * a;
        const float sx = sign * n.x;
        const V3 t1 = {1.f + (sx * n.x) * a, sign * b, -sx}, t2 = {b, sign + (n.y * n.y) * a, -n.y};
        o = {p.x + bias * n.x, p.y + bias * n.y, p.z + bias * n.z};
        d = {(t1.x * c.x + t2.x * c.y) + n.x * c.z, (t1.y * c.x + t2.y * c.y) + n.y * c.z, (t1.z * c.x + t2.z * c.y) + n.z * c.z};
    }
    origins[3 * i] = o.x;
    origins[3 * i + 1] = o.y;
    origins[3 * i + 2] = o.z;
    dirs[3 * i] = d.x;
    dirs[3 * i + 1] = d.y;
    dirs[3 * i + 2] = d.z;
}

// The checks shared by the two queries; *launch = 0 when there is nothing to do.
int check_query(const char* what, const Query& u, int64_t F_usable, int any, bool tree, int64_t n_nodes, Levels& t, int* launch) {
    *launch = 0;
    if (int e = check_points(u.N, what)) return e;
    if (int e = check_faces(F_usable, what)) return e;
    IA_REQUIRE(any == 0 || any == 1, "%s: any must be 0 or 1, got %d", what, any);
    t = levels_of(F_usable);
    if (tree) {
        IA_REQUIRE(u.mesh_extent >= 0.f && std::isfinite(u.mesh_extent), "%s: mesh_extent must be finite and >= 0", what);
        if (int e = check_nodes(t, F_usable, n_nodes, what)) return e;
    }
    if (u.N == 0) return IA_OK;
    const bool outs = any ? (!u.t || on_device(u.t)) && (!u.face || on_device(u.face)) && (!u.bary || on_device(u.bary)) &&
                                (!u.point || on_device(u.point))
                          : on_device(u.t) && on_device(u.face) && on_device(u.bary) && on_device(u.point);
    if (!on_device(u.origins) || !on_device(u.dirs) || !on_device(u.t_lo) || !on_device(u.t_hi) || !on_device(u.hit) || !outs ||
        (u.counts && !on_device(u.counts)) || (t.n && (!on_device(u.tris) || !on_device(u.order) || (tree && !on_device(u.boxes)))))
        return ia::fail(IA_ERR_INVALID_ARG, "%s: origins, dirs, t_lo, t_hi, sorted, order, boxes and the outputs must be device pointers", what);
    *launch = 1;
    return IA_OK;
}

}  // namespace

extern "C" int ia_ray_mesh_brute(const float* origins, const float* dirs, const float* t_lo, const float* t_hi, int64_t N, const void* sorted,
                                 const int* order, int64_t F_usable, int any, unsigned char* hit, float* t, int* face, float* bary, float* point,
                                 void* stream) {
    Query u{origins, dirs, t_lo, t_hi, N, static_cast<const float4*>(sorted), order, (int)F_usable, nullptr, 0.f, hit, t, face, bary, point, nullptr};
    Levels lv;
    int launch;
    if (int e = check_query("ia_ray_mesh_brute", u, F_usable, any, false, 0, lv, &launch)) return e;
    if (!launch) return IA_OK;
    if (any) ray_mesh_brute_kernel<true><<<blocks(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(u);
    else ray_mesh_brute_kernel<false><<<blocks(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(u);
    return ia::check_launch("ia_ray_mesh_brute");
}

extern "C" int ia_ray_mesh_tree(const float* origins, const float* dirs, const float* t_lo, const float* t_hi, int64_t N, const void* sorted,
                                const int* order, int64_t F_usable, const void* boxes, int64_t n_nodes, float mesh_extent, int any,
                                unsigned char* hit, float* t, int* face, float* bary, float* point, int* counts, void* stream) {
    Query u{origins, dirs, t_lo, t_hi, N, static_cast<const float4*>(sorted), order, (int)F_usable, static_cast<const float4*>(boxes), mesh_extent,
            hit, t, face, bary, point, counts};
    Levels lv;
    int launch;
    if (int e = check_query("ia_ray_mesh_tree", u, F_usable, any, true, n_nodes, lv, &launch)) return e;
    if (!launch) return IA_OK;
    if (any) ray_mesh_tree_kernel<true><<<blocks(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(u, tree_of(lv));
    else ray_mesh_tree_kernel<false><<<blocks(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(u, tree_of(lv));
    return ia::check_launch("ia_ray_mesh_tree");
}

extern "C" int ia_ao_rays(const float* verts, const float* normals, int64_t V, const float* table, int S, float bias, float* origins, float* dirs,
                          void* stream) {
    IA_REQUIRE(V >= 0 && V < ((int64_t)1 << 31) && S >= 1 && S <= 65536, "ia_ao_rays: V must be in [0, 2^31) and S in [1, 65536], got %lld and %d",
               (long long)V, S);
    if (int e = check_points(V * S, "ia_ao_rays")) return e;
    if (V == 0) return IA_OK;
    if (!on_device(verts) || !on_device(normals) || !on_device(table) || !on_device(origins) || !on_device(dirs))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_ao_rays: verts, normals, table, origins and dirs must be device pointers");
    ao_rays_kernel<<<blocks(V * S, kBlock), kBlock, 0, (hipStream_t)stream>>>(verts, normals, V * S, S, table, bias, origins, dirs);
    return ia::check_launch("ia_ao_rays");
}
