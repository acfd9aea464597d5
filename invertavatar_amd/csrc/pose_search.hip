// Pose search for global registration: the score of every candidate pose of a point set against the unsigned distance lattice of a
// target mesh.  No counterpart in the reference; the definition is geometry.pose_scores and its NumPy restatement.
//
//   score[r, k] = sum_i min(d(p_i), cap)^2 / n,   p_i = s (R_r y_i) + (c_tgt + o_k),   y_i = x_i - fp32(c_src)
//
// with d the trilinear lookup in the lattice, carried outside it by h |u - clamp(u)| (an upper bound of the true distance up to the
// interpolation error).  Every float32 operation is rounded on its own (the build has -ffp-contract=off) and in the order written in
// point_term below, which the restatement repeats in np.float32; the term min(d, cap) is squared and summed in double.
//
//   work : one workgroup of 256 threads takes rotations blockIdx.x, blockIdx.x + gridDim.x, ... and the offsets of chunk blockIdx.y.
//          The points are staged once per workgroup in LDS as float4 (y, 0).  For a rotation a thread rotates its strided slice
//          (points t, t + 256, ...: PER of them, a template parameter, so that they stay in registers) once and keeps it across the
//          offset loop; the eight lattice reads of a lookup are plain global loads (a 32^3 lattice is 128 KB and stays in L2).
//   sums : a thread adds its points in index order, the wave reduces with the butterfly of wave_sum, the four waves are added in wave
//          order by one thread: no floating-point atomics.  The order depends on n alone, so a candidate's score is a pure function of
//          (points, lattice, rotation, offset, scale, cap): the same bits from run to run, for any number or order of candidates and
//          for any split of a call.
#include "geom_common.h"

#include <cmath>

namespace {

using ia::on_device;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxPoints = 4096;
constexpr int kMaxPer = kMaxPoints / kBlock;          // 16 points, 48 floats, per thread
constexpr int kMaxShifts = 15;
constexpr int kGroups = 2048;                         // workgroups a launch aims for: 8 per CU

struct PoseArgs {
    const float* points;         // [n,3]
    int n;
    const float* dist;           // [nx,ny,nz], x slowest
    int nx, ny, nz;
    float org[3];
    float h, inv_h;
    const float* rot;            // [R,9] row-major
    int R;
    float c_src[3], c_tgt[3];
    int shifts, per_chunk;       // offsets per axis; offsets per blockIdx.y
    float shift_step, scale, cap;
    double* out;                 // [R, shifts^3]
};

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

// One axis of the lookup: lattice coordinate u -> cell i in [0, n - 2], weight t, and the part of u outside the lattice.
__device__ __forceinline__ void axis(float p, float org, float inv_h, int n, int& i, float& t, float& out) {
    const float u = (p - org) * inv_h;
    const float c = fminf(fmaxf(u, 0.f), (float)(n - 1));
    i = max(0, min((int)floorf(c), n - 2));                              // (in range whatever u is, a NaN included)
    t = c - (float)i;
    out = u - c;                                                         // (a NaN u stays a NaN here and in the term)
}

// min(d(p), cap) of one point, in float32.
__device__ __forceinline__ float point_term(const PoseArgs& a, float px, float py, float pz) {
    int i, j, k;
    float tx, ty, tz, ex, ey, ez;
    axis(px, a.org[0], a.inv_h, a.nx, i, tx, ex);
    axis(py, a.org[1], a.inv_h, a.ny, j, ty, ey);
    axis(pz, a.org[2], a.inv_h, a.nz, k, tz, ez);
    const float* v = a.dist + ((int64_t)i * a.ny + j) * a.nz + k;
    const int64_t sy = a.nz, sx = (int64_t)a.ny * a.nz;
    const float v000 = v[0], v001 = v[1], v010 = v[sy], v011 = v[sy + 1];
    const float v100 = v[sx], v101 = v[sx + 1], v110 = v[sx + sy], v111 = v[sx + sy + 1];
    const float c00 = lerp(v000, v001, tz), c01 = lerp(v010, v011, tz), c10 = lerp(v100, v101, tz), c11 = lerp(v110, v111, tz);
    const float inside = lerp(lerp(c00, c01, ty), lerp(c10, c11, ty), tx);
    const float d = inside + a.h * sqrtf((ex * ex + ey * ey) + ez * ez);
    return d > a.cap ? a.cap : d;                                        // (a NaN d stays)
}

template <int PER>
__global__ __launch_bounds__(kBlock) void pose_scores_kernel(PoseArgs a) {
    extern __shared__ float4 pts[];                                      // [n] (x - c_src, 0)
    __shared__ double part[kWaves];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int i = t; i < a.n; i += kBlock)
        pts[i] = make_float4(a.points[3 * i] - a.c_src[0], a.points[3 * i + 1] - a.c_src[1], a.points[3 * i + 2] - a.c_src[2], 0.f);
    __syncthreads();
    const int S = a.shifts, S3 = S * S * S;
    const int k0 = blockIdx.y * a.per_chunk, k1 = min(k0 + a.per_chunk, S3);
    const int half = (S - 1) / 2;
    for (int r = blockIdx.x; r < a.R; r += gridDim.x) {
        float m[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) m[e] = a.rot[9 * (int64_t)r + e];
        float q[PER][3];                                                 // s (R y) of the thread's points
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            const int i = t + s * kBlock;
            const float4 y = i < a.n ? pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int e = 0; e < 3; ++e) q[s][e] = a.scale * ((m[3 * e] * y.x + m[3 * e + 1] * y.y) + m[3 * e + 2] * y.z);
        }
        for (int k = k0; k < k1; ++k) {
            const int kx = k / (S * S), ky = (k / S) % S, kz = k % S;    // x slowest
            const float ox = a.c_tgt[0] + (float)(kx - half) * a.shift_step;
            const float oy = a.c_tgt[1] + (float)(ky - half) * a.shift_step;
            const float oz = a.c_tgt[2] + (float)(kz - half) * a.shift_step;
            double acc = 0.0;
#pragma unroll
            for (int s = 0; s < PER; ++s) {
                if (t + s * kBlock < a.n) {
                    const double v = (double)point_term(a, q[s][0] + ox, q[s][1] + oy, q[s][2] + oz);
                    acc += v * v;
                }
            }
            acc = ia::wave_sum(acc);
            if (lane == 0) part[w] = acc;
            __syncthreads();
            if (t == 0) a.out[(int64_t)r * S3 + k] = (((part[0] + part[1]) + part[2]) + part[3]) / (double)a.n;
            __syncthreads();                                             // (part is written again by the next offset)
        }
    }
}

using Kernel = void (*)(PoseArgs);

Kernel kernel_for(int n, int& per) {
    const int need = (n + kBlock - 1) / kBlock;
    if (need <= 1) { per = 1; return pose_scores_kernel<1>; }
    if (need <= 2) { per = 2; return pose_scores_kernel<2>; }
    if (need <= 4) { per = 4; return pose_scores_kernel<4>; }
    if (need <= 8) { per = 8; return pose_scores_kernel<8>; }
    per = kMaxPer;
    return pose_scores_kernel<kMaxPer>;
}

}  // namespace

extern "C" int ia_pose_scores(const float* points, int n, const float* dist, int nx, int ny, int nz, const float* h_origin, float h_spacing,
                              const float* rotations, int64_t R, const double* h_c_src, const double* h_c_tgt, int shifts,
                              float h_shift_step, float h_scale, float h_cap, double* out, void* stream) {
    IA_REQUIRE(n >= 0 && n <= kMaxPoints, "ia_pose_scores: n must be in [0, %d], got %d (score a subset of the points: samples=)", kMaxPoints, n);
    IA_REQUIRE(shifts >= 1 && shifts <= kMaxShifts && (shifts & 1), "ia_pose_scores: shifts must be odd and in [1, %d], got %d", kMaxShifts,
               shifts);
    if (int e = ia::check_volume(nx, ny, nz, "ia_pose_scores")) return e;
    IA_REQUIRE(h_spacing > 0.f && std::isfinite(h_spacing), "ia_pose_scores: the lattice spacing h must be positive and finite");
    const int64_t S3 = (int64_t)shifts * shifts * shifts;
    IA_REQUIRE(R >= 0 && R * S3 < ((int64_t)1 << 31), "ia_pose_scores: R must be >= 0 and R shifts^3 < 2^31, got R = %lld", (long long)R);
    IA_REQUIRE(h_origin && h_c_src && h_c_tgt, "ia_pose_scores: h_origin, h_c_src and h_c_tgt must not be NULL (host pointers)");
    IA_REQUIRE(std::isfinite(h_shift_step) && std::isfinite(h_scale) && !std::isnan(h_cap),
               "ia_pose_scores: h_shift_step and h_scale must be finite and h_cap not NaN (+inf: no cap)");
    if (n == 0 || R == 0) return IA_OK;
    if (!on_device(points) || !on_device(dist) || !on_device(rotations) || !on_device(out))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_pose_scores: points, dist, rotations and out must be device pointers");
    PoseArgs a{};
    a.points = points; a.n = n;
    a.dist = dist; a.nx = nx; a.ny = ny; a.nz = nz;
    for (int e = 0; e < 3; ++e) { a.org[e] = h_origin[e]; a.c_src[e] = (float)h_c_src[e]; a.c_tgt[e] = (float)h_c_tgt[e]; }
    a.h = h_spacing;
    a.inv_h = (float)(1.0 / (double)h_spacing);
    a.rot = rotations; a.R = (int)R;
    a.shifts = shifts;
    a.shift_step = h_shift_step; a.scale = h_scale; a.cap = h_cap;
    a.out = out;
    // offsets are cut into chunks only while the rotations alone leave the machine short of workgroups
    const int gx = (int)(R < kGroups ? R : kGroups);
    int chunks = (int)ia::ceil_div(kGroups, gx);
    if (chunks > S3) chunks = (int)S3;
    a.per_chunk = (int)ia::ceil_div(S3, chunks);
    chunks = (int)ia::ceil_div(S3, a.per_chunk);
    int per = 0;
    Kernel kernel = kernel_for(n, per);
    const size_t lds = sizeof(float4) * (size_t)n;
    if (int e = ia::reserve_lds((const void*)kernel, lds, "ia_pose_scores")) return e;
    kernel<<<dim3(gx, chunks), kBlock, lds, (hipStream_t)stream>>>(a);
    return ia::check_launch("ia_pose_scores");
}
