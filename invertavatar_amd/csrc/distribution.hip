// Scores of a SET of frames as a distribution: the device side of distribution_metrics.py (FID, KID, precision / recall).  Replaces the
// host arithmetic of the reference's metrics/ package on feature sets [N, D]: the float64 x64.T @ x64 of FeatureStats.append, the
// m x m kernel matrices of compute_kid and the cdist blocks of compute_pr.  See include/ia_hip.h for the formulas and DESIGN.md 4.31.
//
//   ia_feature_moments : one wave owns a 32 x 32 block of the lower triangle of cov (2 x 2 tiles of v_mfma_f64_16x16x4_f64) and walks
//                        the chunk's rows four at a time, converting float32 -> float64 in registers; it adds the block and its mirror
//                        into cov itself.  The blocks on the diagonal also carry the column sums (one more MFMA against ones).
//   ia_kid_subsets     : one workgroup per (subset, block) with block = xx | yy | xy; rows gathered by index into 128-row LDS tiles, the
//                        dot products on v_mfma_f32_32x32x2_f32, the cube and the sums in double.  Nothing of size m x m is stored.
//   ia_knn_radius /
//   ia_manifold_covered: a workgroup holds 64 rows and sweeps the other set in 64-row LDS tiles; squared distances in the difference
//                        form, fp32, channels in ascending order.  Nothing of size N x N is stored.
//
// No floating-point atomics anywhere: every sum has one owner and one order, which depends on the shapes alone.
#include "geom_common.h"

#include <cmath>

namespace {

using ia::on_device;

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------ second moments

constexpr int kMomBlock = 256;
constexpr int kMomWaves = kMomBlock / 64;
constexpr int kMomTile = 32;                    // a wave's block of cov: 2 x 2 MFMA tiles
constexpr int kMomMaxD = 4096;

// Operand maps of v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result register q of lane l is
// C[(l >> 4) + 4 q][l & 15].  Here A = chunk^T (feature x row) and B = chunk (row x feature), four rows per instruction.
__global__ __launch_bounds__(kMomBlock) void moments_kernel(const float* __restrict__ x, int64_t n, int D, double* __restrict__ sum,
                                                            double* __restrict__ cov, int64_t blocks) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int64_t w = (int64_t)blockIdx.x * kMomWaves + (threadIdx.x >> 6);
    if (w >= blocks) return;                                             // (whole waves leave: no barrier in this kernel)
    // block w of the lower triangle, row by row: (bi, bj) with bj <= bi and bi (bi + 1) / 2 + bj == w
    int bi = (int)((sqrt(8.0 * (double)w + 1.0) - 1.0) * 0.5);
    while ((int64_t)bi * (bi + 1) / 2 > w) --bi;
    while ((int64_t)(bi + 1) * (bi + 2) / 2 <= w) ++bi;
    const int bj = (int)(w - (int64_t)bi * (bi + 1) / 2);
    const bool diag = bi == bj;
    const int ca[2] = {bi * kMomTile + c, bi * kMomTile + 16 + c}, cb[2] = {bj * kMomTile + c, bj * kMomTile + 16 + c};
    f64x4 acc[2][2], ones[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        ones[u] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = {0.0, 0.0, 0.0, 0.0};
    }
    for (int64_t r0 = 0; r0 < n; r0 += 4) {
        const int64_t r = r0 + g;
        const bool in = r < n;
        const float* row = x + (in ? r : 0) * D;
        double a[2], b[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) a[u] = (in && ca[u] < D) ? (double)row[ca[u]] : 0.0;
#pragma unroll
        for (int v = 0; v < 2; ++v) b[v] = diag ? a[v] : ((in && cb[v] < D) ? (double)row[cb[v]] : 0.0);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[v], acc[u][v], 0, 0, 0);
        if (diag) {
#pragma unroll
            for (int u = 0; u < 2; ++u) ones[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], 1.0, ones[u], 0, 0, 0);
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = bi * kMomTile + 16 * u + g + 4 * q;
            if (i >= D) continue;
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const int j = bj * kMomTile + 16 * v + c;
                if (j >= D) continue;
                cov[(int64_t)i * D + j] += acc[u][v][q];
                if (!diag) cov[(int64_t)j * D + i] += acc[u][v][q];      // the mirror: the same number, so cov is symmetric bit for bit
            }
            if (diag && c == 0) sum[i] += ones[u][q];                    // (every column of `ones` holds the same sums)
        }
}

// ------------------------------------------------------------------ KID: three sums per subset

constexpr int kKidBlock = 256;
constexpr int kKidTile = 128;                   // rows of either operand per tile; a wave takes a 64 x 64 quadrant (2 x 2 MFMA tiles)
constexpr int kKidK = 32;                       // channels staged per step
constexpr int kKidPitch = kKidK + 1;            // odd: lane l & 31 -> row, l >> 5 -> channel reads hit 64 different banks

// v_mfma_f32_32x32x2_f32: lane l holds A[l & 31][l >> 5] and B[l >> 5][l & 31]; result register q of lane l is
// C[(q & 3) + 8 (q >> 2) + 4 (l >> 5)][l & 31].
__global__ __launch_bounds__(kKidBlock) void kid_kernel(const float* __restrict__ gen, const float* __restrict__ real, int D,
                                                        const int* __restrict__ idx_gen, const int* __restrict__ idx_real, int m,
                                                        double* __restrict__ out) {
    __shared__ float sA[kKidTile * kKidPitch], sB[kKidTile * kKidPitch];
    __shared__ int rowA[kKidTile], rowB[kKidTile];
    __shared__ double part[kKidBlock / 64];
    const int s = blockIdx.x, kind = blockIdx.y;                         // kind 0: gen x gen, 1: real x real, 2: gen x real
    const float* fa = kind == 1 ? real : gen;
    const float* fb = kind == 0 ? gen : real;
    const int* ia_ = (kind == 1 ? idx_real : idx_gen) + (int64_t)s * m;
    const int* ib_ = (kind == 0 ? idx_gen : idx_real) + (int64_t)s * m;
    const bool sym = kind != 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const int tiles = (m + kKidTile - 1) / kKidTile;
    const double n = (double)D;
    double total = 0.0;
    for (int I = 0; I < tiles; ++I) {
        const int jend = sym ? I + 1 : tiles;                            // symmetric blocks: the lower triangle, off-diagonal tiles twice
        for (int J = 0; J < jend; ++J) {
            __syncthreads();                                             // (the tiles and the row lists are read until here)
            if (tid < kKidTile) {
                const int ra = I * kKidTile + tid, rb = J * kKidTile + tid;
                rowA[tid] = ra < m ? ia_[ra] : -1;
                rowB[tid] = rb < m ? ib_[rb] : -1;
            }
            f32x16 acc[2][2];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 2; ++v)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[u][v][q] = 0.f;
            for (int k0 = 0; k0 < D; k0 += kKidK) {
                __syncthreads();
                for (int e = tid; e < kKidTile * kKidK; e += kKidBlock) {
                    const int r = e >> 5, ch = e & 31;
                    const int ga = rowA[r], gb = rowB[r];
                    const bool ok = k0 + ch < D;
                    sA[r * kKidPitch + ch] = (ok && ga >= 0) ? fa[(int64_t)ga * D + k0 + ch] : 0.f;
                    sB[r * kKidPitch + ch] = (ok && gb >= 0) ? fb[(int64_t)gb * D + k0 + ch] : 0.f;
                }
                __syncthreads();
#pragma unroll 4
                for (int kk = 0; kk < kKidK; kk += 2) {
                    float a[2], b[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) a[u] = sA[(wr * 64 + u * 32 + l31) * kKidPitch + kk + h];
#pragma unroll
                    for (int v = 0; v < 2; ++v) b[v] = sB[(wc * 64 + v * 32 + l31) * kKidPitch + kk + h];
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[v], acc[u][v], 0, 0, 0);
                }
            }
            double ts = 0.0;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 2; ++v)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int i = I * kKidTile + wr * 64 + u * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                        const int j = J * kKidTile + wc * 64 + v * 32 + l31;
                        if (i < m && j < m && !(sym && i == j)) {
                            const double t = (double)acc[u][v][q] / n + 1.0;
                            ts += (t * t) * t;
                        }
                    }
            total += (sym && I != J) ? 2.0 * ts : ts;
        }
    }
    total = ia::wave_sum(total);
    if (lane == 0) part[wave] = total;
    __syncthreads();
    if (tid == 0) out[(int64_t)s * 3 + kind] = ((part[0] + part[1]) + part[2]) + part[3];
}

// ------------------------------------------------------------------ precision / recall: radii and coverage

constexpr int kPrBlock = 256;
constexpr int kPrTile = 64;                     // rows held by a workgroup, and rows of the other set per sweep step
constexpr int kPrK = 32;                        // channels staged per step
constexpr int kPrPitch = kPrK + 1;
constexpr int kPrMaxK = 15;

// Squared distances of the 64 rows of A from a0 against the 64 rows of B from b0, difference form in fp32, channels in ascending
// order: d2[u][v] belongs to row (tid >> 4) + 16 u of the block and row (tid & 15) + 16 v of the tile.  Rows and channels outside the
// sets are staged as zeros (their results are not used).  Begins with a barrier: whatever was read from LDS before is read.
__device__ __forceinline__ void tile_dist(const float* __restrict__ A, int64_t a0, int64_t na, const float* __restrict__ B, int64_t b0,
                                          int64_t nb, int D, float* sA, float* sB, float (&d2)[4][4]) {
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) d2[u][v] = 0.f;
    for (int k0 = 0; k0 < D; k0 += kPrK) {
        __syncthreads();
        for (int e = tid; e < kPrTile * kPrK; e += kPrBlock) {
            const int r = e >> 5, ch = e & 31;
            const bool ok = k0 + ch < D;
            sA[r * kPrPitch + ch] = (ok && a0 + r < na) ? A[(a0 + r) * D + k0 + ch] : 0.f;
            sB[r * kPrPitch + ch] = (ok && b0 + r < nb) ? B[(b0 + r) * D + k0 + ch] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int ch = 0; ch < kPrK; ++ch) {
            float a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = sA[(tr + 16 * u) * kPrPitch + ch];
#pragma unroll
            for (int v = 0; v < 4; ++v) b[v] = sB[(tc + 16 * v) * kPrPitch + ch];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float d = a[u] - b[v];
                    d2[u][v] = fmaf(d, d, d2[u][v]);
                }
        }
    }
}

__global__ __launch_bounds__(kPrBlock) void knn_radius_kernel(const float* __restrict__ feat, int64_t N, int D, int k, float* __restrict__ r2) {
    __shared__ float sA[kPrTile * kPrPitch], sB[kPrTile * kPrPitch], sD[kPrTile * (kPrTile + 1)];
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const int64_t a0 = (int64_t)blockIdx.x * kPrTile;
    float best[kPrMaxK + 1];                                             // ascending; thread t < 64 keeps the list of row a0 + t
#pragma unroll
    for (int s = 0; s <= kPrMaxK; ++s) best[s] = INFINITY;
    float thr = INFINITY;                                                // best[k]
    for (int64_t b0 = 0; b0 < N; b0 += kPrTile) {
        float d2[4][4];
        tile_dist(feat, a0, N, feat, b0, N, D, sA, sB, d2);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) sD[(tr + 16 * u) * (kPrTile + 1) + tc + 16 * v] = d2[u][v];
        __syncthreads();
        if (tid < kPrTile) {
            const int cols = (int)(N - b0 < kPrTile ? N - b0 : kPrTile);
            for (int j = 0; j < cols; ++j) {
                float v = sD[tid * (kPrTile + 1) + j];
                if (v < thr) {
#pragma unroll
                    for (int s = 0; s <= kPrMaxK; ++s)
                        if (s <= k && v < best[s]) { const float t = best[s]; best[s] = v; v = t; }
#pragma unroll
                    for (int s = 0; s <= kPrMaxK; ++s)
                        if (s == k) thr = best[s];
                }
            }
        }
    }
    if (tid < kPrTile && a0 + tid < N) r2[a0 + tid] = thr;
}

__global__ __launch_bounds__(kPrBlock) void covered_kernel(const float* __restrict__ probes, int64_t P, const float* __restrict__ manifold,
                                                           const float* __restrict__ r2, int64_t N, int D, unsigned char* __restrict__ covered) {
    __shared__ float sA[kPrTile * kPrPitch], sB[kPrTile * kPrPitch], sR[kPrTile];
    __shared__ int flag[kPrTile];
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const int64_t a0 = (int64_t)blockIdx.x * kPrTile;
    if (tid < kPrTile) flag[tid] = a0 + tid < P ? 0 : 1;                 // (rows past the set count as done for the early exit)
    for (int64_t b0 = 0; b0 < N; b0 += kPrTile) {
        if (tid < kPrTile) sR[tid] = b0 + tid < N ? r2[b0 + tid] : -INFINITY;
        float d2[4][4];
        tile_dist(probes, a0, P, manifold, b0, N, D, sA, sB, d2);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            bool hit = false;
#pragma unroll
            for (int v = 0; v < 4; ++v) hit = hit || d2[u][v] <= sR[tc + 16 * v];
            if (hit) flag[tr + 16 * u] = 1;
        }
        __syncthreads();
        if (__syncthreads_and(flag[tid & (kPrTile - 1)])) break;         // every row of the block has its cover
    }
    if (tid < kPrTile && a0 + tid < P) covered[a0 + tid] = (unsigned char)flag[tid];
}

}  // namespace

extern "C" int ia_feature_moments(const float* x, int64_t n, int D, double* sum, double* cov, void* stream) {
    IA_REQUIRE(n >= 0, "ia_feature_moments: n must be >= 0, got %lld", (long long)n);
    IA_REQUIRE(D >= 1 && D <= kMomMaxD, "ia_feature_moments: D must be in [1, %d], got %d", kMomMaxD, D);
    if (n == 0) return IA_OK;
    if (!on_device(x) || !on_device(sum) || !on_device(cov))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_feature_moments: x, sum and cov must be device pointers");
    const int64_t nb = ia::ceil_div(D, kMomTile), blocks = nb * (nb + 1) / 2;
    moments_kernel<<<(unsigned)ia::ceil_div(blocks, kMomWaves), kMomBlock, 0, (hipStream_t)stream>>>(x, n, D, sum, cov, blocks);
    return ia::check_launch("ia_feature_moments");
}

extern "C" int ia_kid_subsets(const float* gen, const float* real, int D, const int* idx_gen, const int* idx_real, int S, int m,
                              double* out, void* stream) {
    IA_REQUIRE(D >= 1, "ia_kid_subsets: D must be >= 1, got %d", D);
    IA_REQUIRE(S >= 0 && m >= 1 && m <= (1 << 24), "ia_kid_subsets: S must be >= 0 and m in [1, 2^24], got S = %d, m = %d", S, m);
    if (S == 0) return IA_OK;
    if (!on_device(gen) || !on_device(real) || !on_device(idx_gen) || !on_device(idx_real) || !on_device(out))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_kid_subsets: gen, real, idx_gen, idx_real and out must be device pointers");
    kid_kernel<<<dim3((unsigned)S, 3), kKidBlock, 0, (hipStream_t)stream>>>(gen, real, D, idx_gen, idx_real, m, out);
    return ia::check_launch("ia_kid_subsets");
}

extern "C" int ia_knn_radius(const float* feat, int64_t N, int D, int k, float* r2, void* stream) {
    IA_REQUIRE(D >= 1, "ia_knn_radius: D must be >= 1, got %d", D);
    IA_REQUIRE(k >= 0 && k <= kPrMaxK, "ia_knn_radius: k must be in [0, %d], got %d", kPrMaxK, k);
    IA_REQUIRE(N > k && N < ((int64_t)1 << 31), "ia_knn_radius: N must be in [k + 1, 2^31), got N = %lld with k = %d", (long long)N, k);
    if (!on_device(feat) || !on_device(r2)) return ia::fail(IA_ERR_INVALID_ARG, "ia_knn_radius: feat and r2 must be device pointers");
    knn_radius_kernel<<<(unsigned)ia::ceil_div(N, kPrTile), kPrBlock, 0, (hipStream_t)stream>>>(feat, N, D, k, r2);
    return ia::check_launch("ia_knn_radius");
}

extern "C" int ia_manifold_covered(const float* probes, int64_t P, const float* manifold, const float* r2, int64_t N, int D,
                                   unsigned char* covered, void* stream) {
    IA_REQUIRE(D >= 1, "ia_manifold_covered: D must be >= 1, got %d", D);
    IA_REQUIRE(P >= 0 && P < ((int64_t)1 << 31) && N >= 1 && N < ((int64_t)1 << 31),
               "ia_manifold_covered: P must be in [0, 2^31) and N in [1, 2^31), got P = %lld, N = %lld", (long long)P, (long long)N);
    if (P == 0) return IA_OK;
    if (!on_device(probes) || !on_device(manifold) || !on_device(r2) || !on_device(covered))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_manifold_covered: probes, manifold, r2 and covered must be device pointers");
    covered_kernel<<<(unsigned)ia::ceil_div(P, kPrTile), kPrBlock, 0, (hipStream_t)stream>>>(probes, P, manifold, r2, N, D, covered);
    return ia::check_launch("ia_manifold_covered");
}
