// TSDF integration: depth maps with cameras fused into a truncated signed distance lattice (no counterpart in the reference;
// definition: geometry._fuse_numpy).  One thread per lattice point, z fastest across the lanes; the loop over the views
// runs inside the thread with the running sums in registers, in view order, so the result has one summation order: no atomics, the
// same bits run to run and under any split of the views through the accumulate flag.  Every operation is rounded on its own (the build
// passes -ffp-contract=off; the division and sqrtf are the correctly rounded defaults, rintf rounds ties to even).  The per-view camera
// row is read at a wave-uniform address from a read-only array, so it lives in scalar registers.
#include "geom_common.h"

#include <cmath>

namespace {

using ia::check_volume; using ia::on_device;

constexpr int kBlock = 256;
constexpr int kMaxChannels = 8;
constexpr int kMaxSide = 16384;         // pixels per image side: (float)(W - 1) is exact and a pixel index fits an int
constexpr int kViewRow = 18;            // floats per view: R row-major (9), o (3), rows 0 and 1 of K_res (6)

struct TsdfArgs {
    const float* depth;                 // [N,H,W]
    const unsigned char* mask;          // [N,H,W] or null
    const float* weights;               // [N,H,W] or null
    const float* colors;                // [N,C,H,W] or null
    const float* views;                 // [N,kViewRow]
    int N, H, W;
    int ny, nz;
    int64_t P;                          // lattice points
    float lo[3], step[3];
    float tau, near;
    int accumulate;                     // the sums start from the output arrays instead of 0
    float* sum;                         // [P]
    float* weight;                      // [P]
    float* tsdf;                        // [P]
    float* color_sum;                   // [P,C]
    float* color_weight;                // [P]
};

template <int C>
__global__ __launch_bounds__(kBlock) void tsdf_integrate_kernel(TsdfArgs u) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= u.P) return;
    int i, j, k;
    ia::unravel((int)p, u.ny, u.nz, i, j, k);
    const float X = u.lo[0] + (float)i * u.step[0], Y = u.lo[1] + (float)j * u.step[1], Z = u.lo[2] + (float)k * u.step[2];
    float F = 0.f, Wt = 0.f, CW = 0.f;
    float col[C > 0 ? C : 1];
#pragma unroll
    for (int c = 0; c < C; ++c) col[c] = 0.f;
    if (u.accumulate) {
        F = u.sum[p];
        Wt = u.weight[p];
        if (C > 0) {
            CW = u.color_weight[p];
#pragma unroll
            for (int c = 0; c < C; ++c) col[c] = u.color_sum[p * C + c];
        }
    }
    const int64_t hw = (int64_t)u.H * u.W;
    const float wmax = (float)(u.W - 1), hmax = (float)(u.H - 1);
    for (int n = 0; n < u.N; ++n) {
        const float* __restrict__ v = u.views + (int64_t)kViewRow * n;                  // wave-uniform
        const float dx = X - v[9], dy = Y - v[10], dz = Z - v[11];
        const float xz = (v[2] * dx + v[5] * dy) + v[8] * dz;
        if (!(isfinite(xz) && xz > u.near)) continue;
        const float xx = (v[0] * dx + v[3] * dy) + v[6] * dz;
        const float xy = (v[1] * dx + v[4] * dy) + v[7] * dz;
        const float px = (v[12] * xx + v[13] * xy) + v[14] * xz;
        const float py = (v[15] * xx + v[16] * xy) + v[17] * xz;
        const float uu = px / xz, vv = py / xz;
        const float fi = rintf(uu), fj = rintf(vv);
        if (!(isfinite(uu) && isfinite(vv) && fi >= 0.f && fi <= wmax && fj >= 0.f && fj <= hmax)) continue;
        const int64_t q = (int64_t)n * hw + (int64_t)(int)fj * u.W + (int)fi;          // in the image by the float test above
        const float t = u.depth[q];
        const float w = u.weights ? u.weights[q] : 1.f;
        const bool on = u.mask ? u.mask[q] != 0 : true;
        if (!(isfinite(t) && t > 0.f && on && isfinite(w) && w > 0.f)) continue;
        const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float s = t - r;
        if (s < -u.tau) continue;
        const float f = fminf(s / u.tau, 1.f);
        F = F + f * w;
        Wt = Wt + w;
        if (C > 0 && s <= u.tau) {
            const float* __restrict__ img = u.colors + ((int64_t)n * C) * hw + (q - (int64_t)n * hw);
#pragma unroll
            for (int c = 0; c < C; ++c) col[c] = col[c] + img[c * hw] * w;
            CW = CW + w;
        }
    }
    u.sum[p] = F;
    u.weight[p] = Wt;
    u.tsdf[p] = Wt > 0.f ? F / Wt : 1.f;
    if (C > 0) {
        u.color_weight[p] = CW;
#pragma unroll
        for (int c = 0; c < C; ++c) u.color_sum[p * C + c] = col[c];
    }
}

template <int C>
void launch(const TsdfArgs& u, hipStream_t st) {
    tsdf_integrate_kernel<C><<<ia::blocks(u.P, kBlock), kBlock, 0, st>>>(u);
}

}  // namespace

extern "C" int ia_tsdf_integrate(const float* depth, const unsigned char* mask, const float* weights, const float* colors, const float* views,
                                 int N, int C, int H, int W, int nx, int ny, int nz, const float* h_lo, const float* h_step, float truncation,
                                 float near, int accumulate, float* sum, float* weight, float* tsdf, float* color_sum, float* color_weight,
                                 void* stream) {
    if (int st = check_volume(nx, ny, nz, "ia_tsdf_integrate")) return st;
    IA_REQUIRE(N >= 1, "ia_tsdf_integrate: N must be >= 1, got %d", N);
    IA_REQUIRE(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide, "ia_tsdf_integrate: images of 1 .. %d pixels per side, got H = %d, W = %d",
               kMaxSide, H, W);
    IA_REQUIRE(C >= 0 && C <= kMaxChannels, "ia_tsdf_integrate: 0 .. %d colour channels, got %d", kMaxChannels, C);
    IA_REQUIRE(truncation > 0.f && std::isfinite(truncation), "ia_tsdf_integrate: truncation must be finite and > 0, got %g", (double)truncation);
    IA_REQUIRE(near >= 0.f, "ia_tsdf_integrate: near must be >= 0, got %g", (double)near);
    IA_REQUIRE(h_lo && h_step, "ia_tsdf_integrate: h_lo and h_step must be host arrays of 3 floats");
    for (int a = 0; a < 3; ++a)
        IA_REQUIRE(std::isfinite(h_lo[a]) && h_step[a] > 0.f && std::isfinite(h_step[a]),
                   "ia_tsdf_integrate: lo must be finite and step > 0 on every axis");
    IA_REQUIRE((C > 0) == (colors != nullptr), "ia_tsdf_integrate: colors are given exactly when C > 0");
    if (!on_device(depth) || !on_device(views) || !on_device(sum) || !on_device(weight) || !on_device(tsdf) || (mask && !on_device(mask)) ||
        (weights && !on_device(weights)) || (C > 0 && (!on_device(colors) || !on_device(color_sum) || !on_device(color_weight))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_tsdf_integrate: every array must be a device pointer");
    TsdfArgs u{depth, mask, weights, colors, views, N, H, W, ny, nz, (int64_t)nx * ny * nz, {}, {}, truncation, near, accumulate ? 1 : 0,
               sum, weight, tsdf, color_sum, color_weight};
    for (int a = 0; a < 3; ++a) {
        u.lo[a] = h_lo[a];
        u.step[a] = h_step[a];
    }
    const hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 0: launch<0>(u, st); break;
        case 1: launch<1>(u, st); break;
        case 2: launch<2>(u, st); break;
        case 3: launch<3>(u, st); break;
        case 4: launch<4>(u, st); break;
        case 5: launch<5>(u, st); break;
        case 6: launch<6>(u, st); break;
        case 7: launch<7>(u, st); break;
        default: launch<8>(u, st); break;
    }
    return ia::check_launch("ia_tsdf_integrate");
}
