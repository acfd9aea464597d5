// Rigid and similarity alignment (ICP) on the device: the two kernels around the closest-point query of surface_distance.hip.  No
// counterpart in the reference; the definition is geometry.align_mesh and its NumPy restatement.
//
//   transform: p = fp32(M) x, one thread per point, per row ((m0 x + m1 y) + m2 z) + t with every operation rounded on its own (the
//              build has -ffp-contract=off): the `dot` of geom_common.h and one addition.  A non-finite input gives a non-finite output.
//   sums     : over the pairs (p_i, q_i) that count (dist finite, face >= 0, dist <= max_dist in fp32, and for the plane metric a face
//              in [0, Fb) whose normal is not zero), with p, q taken relative to a centre in double: n, sum p, sum q, sum p q^T,
//              sum |p|^2, sum |q|^2, sum |p - q|^2 (19 numbers), and for the plane metric, with a = (p x n, n, p . n) and
//              b = (q - p) . n, the upper triangle of sum a a^T (28), sum a b (7) and sum b^2.  The last slot counts the pairs left out.
//              A thread sums a contiguous slice in index order, the wave reduces with the butterfly of wave_sum, the waves of a
//              workgroup are added in wave order in LDS and a second launch adds the workgroups (one wave per sum: a lane adds a
//              contiguous run of workgroups in index order, the butterfly adds the lanes): no floating-point atomics, bit-equal from
//              run to run (the shape of stats_kernel in surface_distance.hip).  Above the thread's own slice every addition carries
//              its rounding error along (two-sum) and a level rounds once: a plain tree over n positive terms is off by up to
//              log2(n) eps64 / 2 of their sum, which is more than the eps64 sum |terms| the sums are held to.  The plane block is accumulated in five column groups of
//              7 or 8 doubles over the same slice, so that no pass holds more than 20 sums in registers; the slice comes from L2 again.
#include "geom_common.h"

#include <cmath>

namespace {

using ia::blocks; using ia::on_device;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kPointVals = 20;                       // 19 sums + the count of pairs left out
constexpr int kPlaneVals = 56;                       // 19 + 28 + 7 + 1 sums + the count of pairs left out
constexpr int kSumBlocks = 1024;
constexpr int kSumPer = 4;
constexpr int kMaxGroup = 20;

using V3f = ia::Vec3<float>;
using V3d = ia::Vec3<double>;

struct M12 { float m[12]; };                        // rows of [s R | t]

__global__ __launch_bounds__(kBlock) void transform_kernel(const float* __restrict__ pts, int64_t N, M12 M, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const V3f x = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const V3f row = {M.m[4 * r], M.m[4 * r + 1], M.m[4 * r + 2]};
        out[3 * i + r] = dot(row, x) + M.m[4 * r + 3];
    }
}

struct SumArgs {
    const float* src;            // [N,3] the transformed source points p
    const float* dst;            // [N,3] their closest points q
    const float* dist;           // [N]
    const int* face;             // [N]
    int64_t N;
    const float* normals;        // [Fb,3] face normals of the target (plane metric)
    int Fb;
    double c[3];
    float max_dist;
    int plane;
    double* slots;               // [blocks][vals]
    int vals;
};

// One pair: does it count, and its p, q (relative to the centre) and normal in double.
struct Pair { V3d p, q, n; };

__device__ __forceinline__ bool load_pair(const SumArgs& s, int64_t i, Pair& u) {
    const float d = s.dist[i];
    const int f = s.face[i];
    if (!isfinite(d) || f < 0 || !(d <= s.max_dist)) return false;
    if (s.plane) {
        if (f >= s.Fb) return false;
        const V3f n = {s.normals[3 * (int64_t)f], s.normals[3 * (int64_t)f + 1], s.normals[3 * (int64_t)f + 2]};
        if (!finite3(n) || (n.x == 0.f && n.y == 0.f && n.z == 0.f)) return false;
        u.n = {(double)n.x, (double)n.y, (double)n.z};
    }
    u.p = {(double)s.src[3 * i] - s.c[0], (double)s.src[3 * i + 1] - s.c[1], (double)s.src[3 * i + 2] - s.c[2]};
    u.q = {(double)s.dst[3 * i] - s.c[0], (double)s.dst[3 * i + 1] - s.c[1], (double)s.dst[3 * i + 2] - s.c[2]};
    return true;
}

// hi + lo += x, exactly (Knuth's two-sum: the rounding error of hi + x goes to lo).
__device__ __forceinline__ void add_exact(double& hi, double& lo, double x) {
    const double s = hi + x, b = s - hi;
    lo += (hi - (s - b)) + (x - b);
    hi = s;
}

// wave_sum with the rounding errors carried along: the butterfly of geom_common.h on (hi, lo) pairs, rounded once at the end.  The
// two-sum is exact and symmetric in its operands, so every lane still holds the same bits.
__device__ __forceinline__ double wave_sum_exact(double v) {
    double hi = v, lo = 0.0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double oh = __shfl_xor(hi, off, ia::kWave), ol = __shfl_xor(lo, off, ia::kWave);
        lo += ol;
        add_exact(hi, lo, oh);
    }
    return hi + lo;
}

// The K sums of one thread -> the workgroup's slot [at .. at + K): the wave's sum, then the waves in wave order.
template <int K>
__device__ __forceinline__ void reduce_store(const double (&acc)[K], double (*part)[kMaxGroup], double* slot, int at) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = wave_sum_exact(acc[k]);
        if (lane == 0) part[w][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double v = part[0][threadIdx.x], lo = 0.0;
        for (int j = 1; j < kWaves; ++j) add_exact(v, lo, part[j][threadIdx.x]);
        slot[at + threadIdx.x] = v + lo;
    }
    __syncthreads();                                                      // (part is written again by the next group)
}

// Column group G of the plane block over the slice [i0, i1): 0..3 rows of the upper triangle of a a^T (row 0; 1 and 6; 2 and 5; 3 and
// 4: seven numbers each), 4: a b and b^2.
template <int G>
__device__ __forceinline__ void plane_group(const SumArgs& s, int64_t i0, int64_t i1, double (*part)[kMaxGroup], double* slot) {
    constexpr int K = G == 4 ? 8 : 7;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        Pair u;
        if (!load_pair(s, i, u)) continue;
        const V3d x = cross(u.p, u.n);
        const double a[7] = {x.x, x.y, x.z, u.n.x, u.n.y, u.n.z, dot(u.p, u.n)};
        if constexpr (G == 4) {
            const double b = dot(sub(u.q, u.p), u.n);
#pragma unroll
            for (int k = 0; k < 7; ++k) acc[k] += a[k] * b;
            acc[7] += b * b;
        } else {
            constexpr int r0 = G, r1 = 7 - G;                          // rows r0 (7 - r0 entries) and, for G > 0, r1 (7 - r1 entries)
            int k = 0;
#pragma unroll
            for (int j = r0; j < 7; ++j) acc[k++] += a[r0] * a[j];
            if constexpr (G > 0) {
#pragma unroll
                for (int j = r1; j < 7; ++j) acc[k++] += a[r1] * a[j];
            }
        }
    }
    // where the group lands in out: row r of the triangle starts at 19 + r * 7 - r (r - 1) / 2
    if constexpr (G == 4) {
        reduce_store<K>(acc, part, slot, 19 + 28);
    } else {
        constexpr int r0 = G, r1 = 7 - G;
        constexpr int n0 = 7 - r0;
        static_assert(G == 0 || n0 + (7 - r1) == K, "a column group is two rows of the triangle with seven entries in all");
        double first[n0];
#pragma unroll
        for (int k = 0; k < n0; ++k) first[k] = acc[k];
        reduce_store<n0>(first, part, slot, 19 + r0 * 7 - r0 * (r0 - 1) / 2);
        if constexpr (G > 0) {
            constexpr int n1 = 7 - r1;
            double second[n1];
#pragma unroll
            for (int k = 0; k < n1; ++k) second[k] = acc[n0 + k];
            reduce_store<n1>(second, part, slot, 19 + r1 * 7 - r1 * (r1 - 1) / 2);
        }
    }
}

__global__ __launch_bounds__(kBlock) void sums_kernel(SumArgs s) {
    __shared__ double part[kWaves][kMaxGroup];
    const int64_t threads = (int64_t)gridDim.x * kBlock;
    const int64_t per = (s.N + threads - 1) / threads;
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t i0 = min(g * per, s.N), i1 = min(i0 + per, s.N);
    double* slot = s.slots + (int64_t)blockIdx.x * s.vals;
    {
        double acc[kPointVals];
#pragma unroll
        for (int k = 0; k < kPointVals; ++k) acc[k] = 0.0;
        for (int64_t i = i0; i < i1; ++i) {
            Pair u;
            if (!load_pair(s, i, u)) { acc[19] += 1.0; continue; }
            const V3d e = sub(u.p, u.q);
            acc[0] += 1.0;
            acc[1] += u.p.x; acc[2] += u.p.y; acc[3] += u.p.z;
            acc[4] += u.q.x; acc[5] += u.q.y; acc[6] += u.q.z;
            acc[7] += u.p.x * u.q.x; acc[8] += u.p.x * u.q.y; acc[9] += u.p.x * u.q.z;
            acc[10] += u.p.y * u.q.x; acc[11] += u.p.y * u.q.y; acc[12] += u.p.y * u.q.z;
            acc[13] += u.p.z * u.q.x; acc[14] += u.p.z * u.q.y; acc[15] += u.p.z * u.q.z;
            acc[16] += dot(u.p, u.p);
            acc[17] += dot(u.q, u.q);
            acc[18] += dot(e, e);
        }
        double sums[19];
#pragma unroll
        for (int k = 0; k < 19; ++k) sums[k] = acc[k];
        reduce_store<19>(sums, part, slot, 0);
        const double left[1] = {acc[19]};
        reduce_store<1>(left, part, slot, s.vals - 1);
    }
    if (!s.plane) return;                                                 // (uniform over the launch)
    plane_group<0>(s, i0, i1, part, slot);
    plane_group<1>(s, i0, i1, part, slot);
    plane_group<2>(s, i0, i1, part, slot);
    plane_group<3>(s, i0, i1, part, slot);
    plane_group<4>(s, i0, i1, part, slot);
}

// One wave per value: a lane adds a contiguous run of workgroups in index order, wave_sum adds the lanes.
__global__ __launch_bounds__(64) void sums_final_kernel(const double* __restrict__ slots, int nblocks, int vals, double* __restrict__ out) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int per = (nblocks + 63) / 64;
    const int b0 = min(lane * per, nblocks), b1 = min(b0 + per, nblocks);
    double v = 0.0, lo = 0.0;
    for (int b = b0; b < b1; ++b) add_exact(v, lo, slots[(int64_t)b * vals + k]);
    v = wave_sum_exact(v + lo);
    if (lane == 0) out[k] = v;
}

int sum_blocks(int64_t n) {
    const int64_t b = ia::ceil_div(n < 1 ? 1 : n, (int64_t)kBlock * kSumPer);
    return (int)(b > kSumBlocks ? kSumBlocks : b);
}

}  // namespace

extern "C" int ia_transform_points(const float* points, int64_t N, const double* h_m12, float* out, void* stream) {
    IA_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) / 3, "ia_transform_points: N must be >= 0 and 3 N < 2^31, got %lld", (long long)N);
    IA_REQUIRE(h_m12, "ia_transform_points: h_m12 must not be NULL");
    if (N == 0) return IA_OK;
    if (!on_device(points) || !on_device(out)) return ia::fail(IA_ERR_INVALID_ARG, "ia_transform_points: points and out must be device pointers");
    M12 M;
    for (int k = 0; k < 12; ++k) M.m[k] = (float)h_m12[k];
    transform_kernel<<<blocks(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(points, N, M, out);
    return ia::check_launch("ia_transform_points");
}

extern "C" int ia_align_sums_scratch_bytes(int64_t N, int mode, size_t* h_bytes) {
    IA_REQUIRE(N >= 0, "ia_align_sums_scratch_bytes: N must be >= 0");
    IA_REQUIRE(mode == 0 || mode == 1, "ia_align_sums_scratch_bytes: mode must be 0 (point) or 1 (plane), got %d", mode);
    IA_REQUIRE(h_bytes, "ia_align_sums_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = sizeof(double) * (mode ? kPlaneVals : kPointVals) * (size_t)sum_blocks(N);
    return IA_OK;
}

extern "C" int ia_align_sums(const float* src, const float* dst, const float* dist, const int* face, int64_t N, const float* face_normals,
                             int64_t Fb, const double* h_centre, float h_max_dist, int mode, void* scratch, size_t scratch_bytes,
                             double* out, void* stream) {
    IA_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) / 3, "ia_align_sums: N must be >= 0 and 3 N < 2^31, got %lld", (long long)N);
    IA_REQUIRE(mode == 0 || mode == 1, "ia_align_sums: mode must be 0 (point) or 1 (plane), got %d", mode);
    IA_REQUIRE(Fb >= 0 && Fb < ((int64_t)1 << 31) / 3, "ia_align_sums: Fb must be >= 0 and 3 Fb < 2^31, got %lld", (long long)Fb);
    IA_REQUIRE(h_centre && std::isfinite(h_centre[0]) && std::isfinite(h_centre[1]) && std::isfinite(h_centre[2]),
               "ia_align_sums: h_centre must be three finite doubles on the host");
    IA_REQUIRE(!std::isnan(h_max_dist), "ia_align_sums: h_max_dist must not be NaN (+inf: no threshold)");
    const int vals = mode ? kPlaneVals : kPointVals;
    const int nb = sum_blocks(N);
    const size_t need = sizeof(double) * vals * (size_t)nb;
    if (scratch_bytes < need) return ia::fail(IA_ERR_INVALID_ARG, "ia_align_sums: scratch holds %zu bytes, needs %zu", scratch_bytes, need);
    if (!on_device(scratch) || !on_device(out) || (N && (!on_device(src) || !on_device(dst) || !on_device(dist) || !on_device(face))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_align_sums: src, dst, dist, face, scratch and out must be device pointers");
    if (mode && N && Fb && !on_device(face_normals))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_align_sums: face_normals must be a device pointer for the plane metric");
    SumArgs s{};
    s.src = src; s.dst = dst; s.dist = dist; s.face = face;
    s.N = N;
    s.normals = face_normals;
    s.Fb = (int)Fb;
    for (int a = 0; a < 3; ++a) s.c[a] = h_centre[a];
    s.max_dist = h_max_dist;
    s.plane = mode;
    s.slots = static_cast<double*>(scratch);
    s.vals = vals;
    hipStream_t st = (hipStream_t)stream;
    sums_kernel<<<nb, kBlock, 0, st>>>(s);
    if (int e = ia::check_launch("ia_align_sums")) return e;
    sums_final_kernel<<<vals, 64, 0, st>>>(s.slots, nb, vals, out);
    return ia::check_launch("ia_align_sums (final)");
}
