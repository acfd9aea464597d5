// Point clouds on the cluster tree: the k nearest points of a cloud, and normals from them.  No counterpart in the
// reference; the definitions are geometry._nearest_numpy (all pairs), geometry._nearest_tree_numpy (the walk) and
// geometry._point_normals_numpy.
//
// Tree     : the level layout of cluster_tree.h over POINTS: the usable (finite) points sorted by the 30-bit Morton key of
//            ia_winding_tree_point_keys, ties by input index; leaf i = sorted points [i L, min((i + 1) L, n)), B nodes per parent.  A
//            sorted point is one float4 (x, y, z, the bits of its input index).  Boxes are ia_tree_boxes' rows over points: exact min /
//            max, the same bits on every run.
// Pair     : d2 = pair_d2 (geom_common.h), every operation rounded on its own.  The result of a query is the k smallest pairs
//            (d2, input index) over ALL usable points, ascending; dist = sqrtf(d2) (correctly rounded); a pair is reported iff
//            dist <= max_dist, otherwise inf / -1, as are the places past the last point.  d2 grows with dist, so what max_dist admits
//            is a prefix of the list: it is applied on output.
// Skip     : lb = box_d2 (geom_common.h): per axis g = max(lo - p, 0, p - hi), then the expression of pair_d2.  For a point x in
//            the box, lo <= x <= hi per axis, so fl(lo - p) <= fl(x - p) where p < lo, fl(p - hi) <= fl(p - x) where p > hi (rounding
//            is monotone) and g = 0 <= |fl(x - p)| inside; products of non-negative numbers and sums are monotone under round to
//            nearest as well, hence lb <= d2 of every point in the box, in fp32, with no margin.  A node is skipped iff
//            lb > (the lane's k-th d2): strictly, so that a tie on d2 with a lower index still enters.  A list that is not full has
//            k-th d2 = +inf, which nothing exceeds.
// List     : K (d2, index) pairs per lane, ascending, in registers; insertion is an unrolled compare-and-shift with constant
//            indices.  K in {1, 4, 8, 16, 32}; k is rounded up, and a prefix of the longer list is the shorter list.
// Seed     : as closest_tree.hip: each lane first descends to the child with the smallest lb (lowest index among equals) and takes
//            that leaf, then walks depth first passing over it, so no pair is inserted twice.
// counts   : (boxes tested, leaves taken) of the lane's own traversal, seed included.
#include "cluster_tree.h"

#include <climits>
#include <cmath>

namespace {

using ia::blocks; using ia::on_device; using ia::pair_d2; using ia::box_d2;
using namespace ia::tree;

constexpr int kBlock = 256;
constexpr int kNone = INT_MAX;                       // index of an empty place of a list
constexpr int kMaxK = 32;

using V3 = ia::Vec3<float>;
using D3 = ia::Vec3<double>;

// ------------------------------------------------------------------ build

__global__ __launch_bounds__(kBlock) void gather_kernel(const float* __restrict__ pts, const int* __restrict__ order, int n,
                                                        float4* __restrict__ sorted) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const int i = order[s];
    sorted[s] = {pts[3 * (int64_t)i], pts[3 * (int64_t)i + 1], pts[3 * (int64_t)i + 2], __int_as_float(i)};
}

__global__ __launch_bounds__(kBlock) void leaf_box_kernel(const float4* __restrict__ sorted, int n, int leaves, float4* __restrict__ boxes) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= leaves) return;
    const Range r = leaf_range(i, n);
    V3 lo = {INFINITY, INFINITY, INFINITY}, hi = {-INFINITY, -INFINITY, -INFINITY};
    for (int s = r.lo; s < r.hi; ++s) {
        const float4 v = sorted[s];
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

// ------------------------------------------------------------------ the list of a lane

template <int K>
struct List {
    float d[K];
    int id[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int s = 0; s < K; ++s) { d[s] = INFINITY; id[s] = kNone; }
    }
    __device__ __forceinline__ static bool less(float da, int ia_, float db, int ib) { return da < db || (da == db && ia_ < ib); }
    // (d2, i) enters iff it is smaller than the last pair; every place is a constant index after unrolling.
    __device__ __forceinline__ void insert(float d2, int i) {
        if (!less(d2, i, d[K - 1], id[K - 1])) return;
#pragma unroll
        for (int s = K - 1; s > 0; --s) {
            const bool above = less(d2, i, d[s - 1], id[s - 1]);       // the new pair goes in front of place s - 1: that one moves up
            const bool here = less(d2, i, d[s], id[s]);
            d[s] = above ? d[s - 1] : (here ? d2 : d[s]);
            id[s] = above ? id[s - 1] : (here ? i : id[s]);
        }
        if (less(d2, i, d[0], id[0])) { d[0] = d2; id[0] = i; }
    }
    __device__ __forceinline__ float bound() const { return d[K - 1]; }
    __device__ __forceinline__ void store(int64_t row, int k, float max_dist, float* __restrict__ dist, int* __restrict__ index) const {
#pragma unroll
        for (int s = 0; s < K; ++s)
            if (s < k) {
                const float r = sqrtf(d[s]);
                const bool ok = id[s] != kNone && r <= max_dist;
                dist[row * k + s] = ok ? r : INFINITY;
                index[row * k + s] = ok ? id[s] : -1;
            }
    }
};

struct Query {
    const float* pts;                                // queries [N,3]
    int64_t N;
    const float4* sorted;                            // the cloud, sorted
    int n;
    const float4* boxes;
    const int* exclude;                              // [N] or null: the input index that query i leaves out
    int k;
    float max_dist;
    float* dist;
    int* index;
    int* counts;                                     // [N,2] or null
};

__device__ __forceinline__ bool load_query(const Query& u, int64_t i, V3& p, int& excl) {
    p = {0.f, 0.f, 0.f};
    excl = -1;
    if (i >= u.N) return false;
    p = {u.pts[3 * i], u.pts[3 * i + 1], u.pts[3 * i + 2]};
    if (u.exclude) excl = u.exclude[i];
    return finite3(p);
}

// ------------------------------------------------------------------ all pairs

template <int K>
__global__ __launch_bounds__(kBlock) void nearest_brute_kernel(Query u) {
    __shared__ float4 s_pts[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    V3 p;
    int excl;
    const bool ok = load_query(u, i, p, excl);
    List<K> best;
    best.clear();
    for (int base = 0; base < u.n; base += kBlock) {
        const int m = min(kBlock, u.n - base);
        __syncthreads();
        if ((int)threadIdx.x < m) s_pts[threadIdx.x] = u.sorted[base + threadIdx.x];
        __syncthreads();
        if (ok)
            for (int t = 0; t < m; ++t) {            // (every lane reads the same point)
                const float4 x = s_pts[t];
                const int idx = __float_as_int(x.w);
                if (idx != excl) best.insert(pair_d2(p, {x.x, x.y, x.z}), idx);
            }
    }
    if (i < u.N) best.store(i, u.k, u.max_dist, u.dist, u.index);
}

// ------------------------------------------------------------------ the walk

template <int K>
__device__ __forceinline__ void leaf_points(V3 p, int excl, const float4* __restrict__ sorted, int n, int j, bool take, List<K>& best) {
    const Range r = leaf_range(j, n);
    for (int s = r.lo; s < r.hi; ++s) {
        const float4 x = sorted[s];
        const int idx = __float_as_int(x.w);
        if (take && idx != excl) best.insert(pair_d2(p, {x.x, x.y, x.z}), idx);
    }
}

template <int K>
__global__ __launch_bounds__(kBlock) void nearest_tree_kernel(Query u, Tree tree) {
    IA_TREE_STAGE(tree);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    V3 p;
    int excl;
    const bool ok = load_query(u, i, p, excl);
    List<K> best;
    best.clear();
    int n_box = 0, n_leaf = 0;
    int seed = -1;
    if (ok && tree.top >= 0) {
        int j = 0;
        for (int l = tree.top; l > 0; --l) {
            const Range kr = {j * kBranch, min(j * kBranch + kBranch, level_count(u.n, l - 1))};
            const float4* row = u.boxes + 2 * (int64_t)s_start[l - 1];
            float least = INFINITY;
            j = kr.lo;
            for (int k = kr.lo; k < kr.hi; ++k) {
                const float lb = box_d2(p, row[2 * (int64_t)k], row[2 * (int64_t)k + 1]);
                if (lb < least) { least = lb; j = k; }
            }
            n_box += kr.hi - kr.lo;
        }
        seed = j;
        leaf_points<K>(p, excl, u.sorted, u.n, j, true, best);
        ++n_leaf;
    }
    IA_TREE_WALK(tree, ok)
        const float4* row = u.boxes + 2 * (int64_t)node;
        const float lb = box_d2(p, row[0], row[1]);
        const bool mine = IA_TREE_WALKING && !(l == 0 && j == seed);
        const bool hold = mine && lb > best.bound(), need = mine && !hold;
        if (mine) ++n_box;
    IA_TREE_LEAF
        leaf_points<K>(p, excl, u.sorted, u.n, j, need, best);
        if (need) ++n_leaf;
    IA_TREE_END(tree, , level_count(u.n, l))
    if (i >= u.N) return;
    best.store(i, u.k, u.max_dist, u.dist, u.index);
    if (u.counts) { u.counts[2 * i] = n_box; u.counts[2 * i + 1] = n_leaf; }
}

// ------------------------------------------------------------------ normals

struct Sym3 { double a[3][3]; };

// One Jacobi rotation in the (P, Q) plane of the symmetric A (R: the third axis), accumulated into the columns of V.
template <int P, int Q, int R>
__device__ __forceinline__ void jacobi_rotate(Sym3& A, Sym3& V) {
    const double apq = A.a[P][Q];
    if (apq == 0.0) return;
    const double theta = (A.a[Q][Q] - A.a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double app = A.a[P][P] - t * apq, aqq = A.a[Q][Q] + t * apq;
    const double arp = c * A.a[R][P] - s * A.a[R][Q], arq = s * A.a[R][P] + c * A.a[R][Q];
    A.a[P][P] = app; A.a[Q][Q] = aqq;
    A.a[P][Q] = 0.0; A.a[Q][P] = 0.0;
    A.a[R][P] = arp; A.a[P][R] = arp;
    A.a[R][Q] = arq; A.a[Q][R] = arq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double vp = c * V.a[r][P] - s * V.a[r][Q], vq = s * V.a[r][P] + c * V.a[r][Q];
        V.a[r][P] = vp; V.a[r][Q] = vq;
    }
}

constexpr int kSweeps = 8;

__global__ __launch_bounds__(kBlock) void point_normals_kernel(const float* __restrict__ pts, int n, const int* __restrict__ index, int k,
                                                               float* __restrict__ normal, float* __restrict__ variation,
                                                               double* __restrict__ eigenvalues, double* __restrict__ covariance) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int* nb = index + (int64_t)i * k;
    int m = 0;
    D3 sum = {0.0, 0.0, 0.0};
    for (int s = 0; s < k; ++s) {
        const int q = nb[s];
        if (q < 0 || q >= n) continue;
        sum = {sum.x + (double)pts[3 * (int64_t)q], sum.y + (double)pts[3 * (int64_t)q + 1], sum.z + (double)pts[3 * (int64_t)q + 2]};
        ++m;
    }
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // xx xy xz yy yz zz
    if (m > 0) {
        const D3 mean = {sum.x / m, sum.y / m, sum.z / m};
        for (int s = 0; s < k; ++s) {
            const int q = nb[s];
            if (q < 0 || q >= n) continue;
            const D3 e = {(double)pts[3 * (int64_t)q] - mean.x, (double)pts[3 * (int64_t)q + 1] - mean.y, (double)pts[3 * (int64_t)q + 2] - mean.z};
            c[0] += e.x * e.x; c[1] += e.x * e.y; c[2] += e.x * e.z;
            c[3] += e.y * e.y; c[4] += e.y * e.z; c[5] += e.z * e.z;
        }
#pragma unroll
        for (int t = 0; t < 6; ++t) c[t] = c[t] / m;
    }
    Sym3 A = {{{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}}};
    Sym3 V = {{{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}}};
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        jacobi_rotate<0, 1, 2>(A, V);
        jacobi_rotate<0, 2, 1>(A, V);
        jacobi_rotate<1, 2, 0>(A, V);
    }
    // ascending eigenvalues, the lowest axis first among equals (a fixed network on three values)
    double w0 = A.a[0][0], w1 = A.a[1][1], w2 = A.a[2][2];
    D3 v0 = {V.a[0][0], V.a[1][0], V.a[2][0]}, v1 = {V.a[0][1], V.a[1][1], V.a[2][1]}, v2 = {V.a[0][2], V.a[1][2], V.a[2][2]};
    if (w1 < w0) { const double t = w0; w0 = w1; w1 = t; const D3 v = v0; v0 = v1; v1 = v; }
    if (w2 < w1) { const double t = w1; w1 = w2; w2 = t; const D3 v = v1; v1 = v2; v2 = v; }
    if (w1 < w0) { const double t = w0; w0 = w1; w1 = t; const D3 v = v0; v0 = v1; v1 = v; }
    const double trace = (w0 + w1) + w2;
    const bool good = m >= 3 && trace > 0.0;
    const double len = sqrt((v0.x * v0.x + v0.y * v0.y) + v0.z * v0.z);
    D3 nrm = {v0.x / len, v0.y / len, v0.z / len};
    const double ax = fabs(nrm.x), ay = fabs(nrm.y), az = fabs(nrm.z);
    const double lead = (ax >= ay && ax >= az) ? nrm.x : (ay >= az ? nrm.y : nrm.z);
    if (lead < 0.0) nrm = {-nrm.x, -nrm.y, -nrm.z};
    normal[3 * (int64_t)i] = good ? (float)nrm.x : 0.f;
    normal[3 * (int64_t)i + 1] = good ? (float)nrm.y : 0.f;
    normal[3 * (int64_t)i + 2] = good ? (float)nrm.z : 0.f;
    variation[i] = good ? (float)(w0 / trace) : 0.f;
    eigenvalues[3 * (int64_t)i] = w0; eigenvalues[3 * (int64_t)i + 1] = w1; eigenvalues[3 * (int64_t)i + 2] = w2;
#pragma unroll
    for (int t = 0; t < 6; ++t) covariance[6 * (int64_t)i + t] = c[t];
}

// ------------------------------------------------------------------ host side

inline int check_cloud(int64_t n, const char* what) {
    return n >= 0 && n <= kMaxFaces && n < ((int64_t)1 << 31) / 3
               ? IA_OK
               : ia::fail(IA_ERR_INVALID_ARG, "%s: a cloud holds at most 2^25 points, got %lld", what, (long long)n);
}

template <int K>
int launch_nearest(const Query& u, const Levels* t, hipStream_t st) {
    if (t) nearest_tree_kernel<K><<<blocks(u.N, kBlock), kBlock, 0, st>>>(u, tree_of(*t));
    else nearest_brute_kernel<K><<<blocks(u.N, kBlock), kBlock, 0, st>>>(u);
    return IA_OK;
}

int nearest(const char* what, const float* queries, int64_t N, const void* sorted, int64_t n, const void* boxes, int64_t n_nodes, bool walk,
            int k, float max_dist, const int* exclude, float* dist, int* index, int* counts, void* stream) {
    if (int e = check_points(N, what)) return e;
    if (int e = check_cloud(n, what)) return e;
    if (k < 1 || k > kMaxK) return ia::fail(IA_ERR_INVALID_ARG, "%s: k must be in 1 .. %d, got %d", what, kMaxK, k);
    if (N * k >= ((int64_t)1 << 31)) return ia::fail(IA_ERR_INVALID_ARG, "%s: N k must be below 2^31, got %lld x %d", what, (long long)N, k);
    if (!(max_dist >= 0.f)) return ia::fail(IA_ERR_INVALID_ARG, "%s: max_dist must be >= 0 (+inf: none)", what);
    const Levels t = levels_of(n);
    if (walk)
        if (int e = check_nodes(t, n, n_nodes, what)) return e;
    if (N == 0) return IA_OK;
    if (!on_device(queries) || !on_device(dist) || !on_device(index) || (exclude && !on_device(exclude)) || (counts && !on_device(counts)) ||
        (n && (!on_device(sorted) || (walk && !on_device(boxes)))))
        return ia::fail(IA_ERR_INVALID_ARG, "%s: queries, sorted, boxes, exclude, dist, index and counts must be device pointers", what);
    const Query u{queries, N, static_cast<const float4*>(sorted), (int)n, static_cast<const float4*>(boxes), exclude, k, max_dist, dist, index,
                  counts};
    const Levels* lv = walk ? &t : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (k <= 1) launch_nearest<1>(u, lv, st);
    else if (k <= 4) launch_nearest<4>(u, lv, st);
    else if (k <= 8) launch_nearest<8>(u, lv, st);
    else if (k <= 16) launch_nearest<16>(u, lv, st);
    else launch_nearest<32>(u, lv, st);
    return ia::check_launch(what);
}

}  // namespace

extern "C" int ia_point_tree_gather(const float* points, int64_t n, const int* order, int64_t n_usable, void* sorted, void* stream) {
    if (int e = check_cloud(n, "ia_point_tree_gather")) return e;
    IA_REQUIRE(n_usable >= 0 && n_usable <= n, "ia_point_tree_gather: n_usable must be within the %lld points, got %lld", (long long)n,
               (long long)n_usable);
    if (n_usable == 0) return IA_OK;
    if (!on_device(points) || !on_device(order) || !on_device(sorted))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_point_tree_gather: points, order and sorted must be device pointers");
    gather_kernel<<<blocks(n_usable, kBlock), kBlock, 0, (hipStream_t)stream>>>(points, order, (int)n_usable, static_cast<float4*>(sorted));
    return ia::check_launch("ia_point_tree_gather");
}

extern "C" int ia_point_tree_boxes(const void* sorted, int64_t n_usable, void* boxes, int64_t n_nodes, void* stream) {
    if (int e = check_cloud(n_usable, "ia_point_tree_boxes")) return e;
    const Levels t = levels_of(n_usable);
    if (int e = check_nodes(t, n_usable, n_nodes, "ia_point_tree_boxes")) return e;
    if (t.n == 0) return IA_OK;
    if (!on_device(sorted) || !on_device(boxes)) return ia::fail(IA_ERR_INVALID_ARG, "ia_point_tree_boxes: sorted and boxes must be device pointers");
    hipStream_t st = (hipStream_t)stream;
    float4* out = static_cast<float4*>(boxes);
    leaf_box_kernel<<<blocks(t.count[0], kBlock), kBlock, 0, st>>>(static_cast<const float4*>(sorted), (int)n_usable, t.count[0], out);
    if (int e = ia::check_launch("ia_point_tree_boxes (leaves)")) return e;
    for (int l = 1; l < t.n; ++l) {
        upper_box_kernel<<<blocks(t.count[l], kBlock), kBlock, 0, st>>>(t.count[l - 1], t.start[l - 1], t.count[l], t.start[l], out);
        if (int e = ia::check_launch("ia_point_tree_boxes (level)")) return e;
    }
    return IA_OK;
}

extern "C" int ia_nearest_points_brute(const float* queries, int64_t N, const void* sorted, int64_t n_usable, int k, float max_dist,
                                       const int* exclude, float* dist, int* index, void* stream) {
    return nearest("ia_nearest_points_brute", queries, N, sorted, n_usable, nullptr, 0, false, k, max_dist, exclude, dist, index, nullptr, stream);
}

extern "C" int ia_nearest_points_tree(const float* queries, int64_t N, const void* sorted, int64_t n_usable, const void* boxes, int64_t n_nodes,
                                      int k, float max_dist, const int* exclude, float* dist, int* index, int* counts, void* stream) {
    return nearest("ia_nearest_points_tree", queries, N, sorted, n_usable, boxes, n_nodes, true, k, max_dist, exclude, dist, index, counts, stream);
}

extern "C" int ia_point_normals(const float* points, int64_t n, const int* index, int k, float* normal, float* variation, double* eigenvalues,
                                double* covariance, void* stream) {
    if (int e = check_cloud(n, "ia_point_normals")) return e;
    IA_REQUIRE(k >= 1 && k <= kMaxK, "ia_point_normals: k must be in 1 .. %d, got %d", kMaxK, k);
    if (n == 0) return IA_OK;
    if (!on_device(points) || !on_device(index) || !on_device(normal) || !on_device(variation) || !on_device(eigenvalues) || !on_device(covariance))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_point_normals: points, index, normal, variation, eigenvalues and covariance must be device pointers");
    point_normals_kernel<<<blocks(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(points, (int)n, index, k, normal, variation, eigenvalues, covariance);
    return ia::check_launch("ia_point_normals");
}
