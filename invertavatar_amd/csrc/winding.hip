// Generalised winding number of query points with respect to a triangle soup: 1 inside a closed outward-wound mesh, 0 outside, a
// smooth value in between for an open one.  No counterpart in the reference; the definition is geometry.winding_number and its NumPy
// restatement.
//
// Per pair (point p, usable triangle A B C), in fp32 with every operation rounded on its own (the build has -ffp-contract=off) and
// dot products (x + y) + z, in coordinates relative to the query, a = A - p, b = B - p, c = C - p:
//     num   = a . ((b - a) x (c - a))
//     den   = (((|a| |b|) |c| + (a . b) |c|) + (b . c) |a|) + (c . a) |b|
//     omega = 2 atan2f(num, den)
// The numerator is taken from the edges, so the error of a far triangle is relative to its own (small) solid angle.  A triangle
// without area has num = 0 and contributes atan2f(0, den >= 0) = 0; a triangle whose usable flag (A.w of ia_tri_pack) is 0 is skipped.
//
// The sum is an all-pairs sum (N F terms), shaped like an N-body kernel:
//   partial : a workgroup owns kPoints = kBlock * kPerThread points (kPerThread per thread, in registers) and ONE chunk of kChunk
//             faces.  It walks the chunk in tiles of kTile triangles staged in LDS (one triangle per thread); every lane then reads
//             the same triangle, so the LDS read is a broadcast.  omega is fp32, the running sum of the chunk is double, in face
//             order.  One double per (chunk, point) goes to the workspace, laid out [chunk][point] so that both launches are coalesced.
//   final   : one thread per point adds its chunk partials in chunk order and divides by 4 pi; a non-finite point gives NaN.
// The association is fixed by (kChunk, face order, chunk order) alone, so the result for a point is a pure function of the point and
// the mesh: it does not depend on N, on the order of the points, on how the caller cuts them into calls, or on the run.  No
// floating-point atomics.
#include "geom_common.h"

namespace {

using ia::blocks; using ia::on_device;

constexpr int kBlock = 256;
constexpr int kPerThread = 2;                        // points per thread
constexpr int kPoints = kBlock * kPerThread;         // points per workgroup
constexpr int kTile = kBlock;                        // triangles staged per step: one per thread
constexpr int kChunk = 2048;                         // faces per partial sum (a multiple of kTile); part of the results
constexpr int64_t kMaxFaces = (int64_t)1 << 25;      // the limit of ia_tri_pack: at most 2^14 chunks (gridDim.y)
static_assert(kChunk % kTile == 0, "a chunk is whole tiles");

using V3 = ia::Vec3<float>;                       // (solid_angle: geom_common.h, shared with winding_tree.hip)

// grid (point blocks, chunks).  part[chunk * N + i] = sum of omega over the chunk's faces, in face order.
__global__ __launch_bounds__(kBlock) void winding_partial_kernel(const float* __restrict__ pts, int64_t N, const float4* __restrict__ tris,
                                                                int F, double* __restrict__ part) {
    __shared__ float4 s[kTile][3];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * kPoints + t;
    V3 p[kPerThread];
    double acc[kPerThread];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int64_t i = i0 + (int64_t)j * kBlock;
        p[j] = {0.f, 0.f, 0.f};
        if (i < N) p[j] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        acc[j] = 0.0;
    }
    const int f0 = blockIdx.y * kChunk, f1 = min(f0 + kChunk, F);
    for (int base = f0; base < f1; base += kTile) {
        const int n = min(kTile, f1 - base);                              // (uniform over the workgroup)
        __syncthreads();                                                  // (the previous tile has been read)
        if (t < n) {
            const float4* src = tris + 3 * (int64_t)(base + t);
            s[t][0] = src[0];
            s[t][1] = src[1];
            s[t][2] = src[2];
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const float4 A = s[k][0], B = s[k][1], C = s[k][2];
            if (A.w == 0.f) continue;                                     // (the same triangle in every lane)
#pragma unroll
            for (int j = 0; j < kPerThread; ++j)
                acc[j] += (double)solid_angle(p[j], {A.x, A.y, A.z}, {B.x, B.y, B.z}, {C.x, C.y, C.z});
        }
    }
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int64_t i = i0 + (int64_t)j * kBlock;
        if (i < N) part[(int64_t)blockIdx.y * N + i] = acc[j];
    }
}

__global__ __launch_bounds__(kBlock) void winding_final_kernel(const float* __restrict__ pts, int64_t N, const double* __restrict__ part,
                                                              int chunks, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const V3 p = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    double sum = 0.0;
    for (int c = 0; c < chunks; ++c) sum += part[(int64_t)c * N + i];
    out[i] = finite3(p) ? sum / (4.0 * 3.14159265358979323846) : (double)NAN;
}

int chunks_of(int64_t F) { return (int)ia::ceil_div(F, (int64_t)kChunk); }

}  // namespace

extern "C" int ia_winding_layout(int* h_tile, int* h_chunk, int* h_points) {
    IA_REQUIRE(h_tile && h_chunk && h_points, "ia_winding_layout: the three outputs must not be NULL");
    *h_tile = kTile;
    *h_chunk = kChunk;
    *h_points = kPoints;
    return IA_OK;
}

extern "C" int ia_winding_number_scratch_bytes(int64_t N, int64_t F, size_t* h_bytes) {
    IA_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) / 3, "ia_winding_number_scratch_bytes: N must be >= 0 and 3 N < 2^31, got %lld", (long long)N);
    IA_REQUIRE(F >= 0 && F <= kMaxFaces, "ia_winding_number_scratch_bytes: F must be >= 0 and <= 2^25, got %lld", (long long)F);
    IA_REQUIRE(h_bytes, "ia_winding_number_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = sizeof(double) * (size_t)N * (size_t)chunks_of(F);
    return IA_OK;
}

extern "C" int ia_winding_number(const float* points, int64_t N, const void* tris, int64_t F, void* scratch, size_t scratch_bytes,
                                 double* out, void* stream) {
    IA_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) / 3, "ia_winding_number: N must be >= 0 and 3 N < 2^31, got %lld", (long long)N);
    IA_REQUIRE(F >= 0 && F <= kMaxFaces, "ia_winding_number: F must be >= 0 and <= 2^25, got %lld", (long long)F);
    const int chunks = chunks_of(F);
    const size_t need = sizeof(double) * (size_t)N * (size_t)chunks;
    if (scratch_bytes < need) return ia::fail(IA_ERR_INVALID_ARG, "ia_winding_number: scratch holds %zu bytes, needs %zu", scratch_bytes, need);
    if (N == 0) return IA_OK;
    if (!on_device(points) || !on_device(out) || (F && (!on_device(tris) || !on_device(scratch))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_winding_number: points, tris, scratch and out must be device pointers");
    hipStream_t st = (hipStream_t)stream;
    if (chunks) {
        const dim3 grid(blocks(N, kPoints), (unsigned)chunks);
        winding_partial_kernel<<<grid, kBlock, 0, st>>>(points, N, static_cast<const float4*>(tris), (int)F, static_cast<double*>(scratch));
        if (int e = ia::check_launch("ia_winding_number")) return e;
    }
    winding_final_kernel<<<blocks(N, kBlock), kBlock, 0, st>>>(points, N, static_cast<const double*>(scratch), chunks, out);
    return ia::check_launch("ia_winding_number (final)");
}
