// Per-frame image metrics on the device: PSNR, SSIM and MS-SSIM of two image batches.  Replaces, for evaluation (no gradients), the
// reference's encoder_inversion/criteria/ms_ssim.py (ssim / msssim with size_average=False: 5 grouped 11 x 11 convolutions, ~15
// elementwise kernels and 2 pools per level, each through a full image in global memory).
//
// One level = one launch (ssim_level_kernel), whatever the batch: a 256-thread workgroup takes a tile of kTile x kTile map pixels of
// one (frame, channel) plane, stages both images' (kTile + 10)^2 windows in LDS (2 x 74 x 74 floats = 43 808 bytes; outside the image:
// zeros), and forms the five windowed moments separably without an intermediate image: a thread owns one map column and kRows = 16 map
// rows; for each of the 26 staged rows it needs it computes the 11-tap horizontal sums of a, b, a*a, b*b, a*b at its column (lanes read
// consecutive LDS words: no bank conflicts) and adds them, weighted by the vertical tap, into the accumulators of the map rows that row
// belongs to (80 registers).  The taps are explicit fused multiply-adds, the same sequence for all five moments, so a == b gives
// s1 == s2 == s12 bit for bit; the maps are evaluated with every operation rounded (the project's -ffp-contract=off) and are then
// exactly 1.  Map values are summed per thread and per workgroup in double, in a fixed order, into the tile's slot of the scratch:
// no atomics.  The same launch writes the 2 x 2 average of the pixels the tile owns (its kTile x kTile block; the last tile of a row /
// column also owns the 10-pixel rim) for the next level, and at level 0 the sums of (a-b)^2 and |a-b| over them, in double.
// finalize_kernel (one workgroup per frame, one wave per quantity) adds the tiles' slots in a fixed order and writes the results.
// A frame's results depend on that frame's pixels only: batching changes nothing, bit for bit.
#include "ia_common.h"

#include <cmath>

namespace {

constexpr int kTile = 64;                      // map pixels per tile edge
constexpr int kWin = 11;                       // window taps
constexpr int kHalo = kWin - 1;
constexpr int kStage = kTile + kHalo;          // 74 staged pixels per edge
constexpr int kRows = 16;                      // map rows per thread
constexpr int kBlock = kTile * (kTile / kRows);      // 256 threads: 64 columns x 4 row groups (one wave each)
constexpr int kSlot = 4;                       // doubles per tile: ssim, cs, squared error, absolute error
constexpr int kMaxLevels = 5;

// exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, rounded to fp32 from the double values
__device__ constexpr float kG[kWin] = {1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f, 2.130055428e-01f,
                                       2.660117149e-01f, 2.130055428e-01f, 1.093606874e-01f, 3.600077331e-02f, 7.598758209e-03f,
                                       1.028380124e-03f};
constexpr double kMsWeights[kMaxLevels] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};

struct LevelArgs {
    const void* a;            // level 0: the caller's images (fp32 NCHW or uint8 NHWC); below: fp32 NCHW in the scratch
    const void* b;
    float* pa;                // pooled pair for the next level, or null at the last level
    float* pb;
    double* slots;            // [n * c][tiles][kSlot]
    int C, H, W;
    int tiles_x, tiles_y;
    float C1, C2;
};

template <bool U8>
__device__ __forceinline__ float load_px(const void* img, int nc, int C, int H, int W, int y, int x) {
    if (U8) {
        const int n = nc / C, c = nc - n * C;
        return (float)((const unsigned char*)img)[(((int64_t)n * H + y) * W + x) * C + c];
    }
    return ((const float*)img)[((int64_t)nc * H + y) * W + x];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <bool U8, bool L0>
__global__ __launch_bounds__(kBlock) void ssim_level_kernel(LevelArgs p) {
    __shared__ float sA[kStage * kStage];
    __shared__ float sB[kStage * kStage];
    __shared__ double sRed[kBlock / 64][kSlot];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, nc = blockIdx.y;
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int y0 = ty * kTile, x0 = tx * kTile;
    const int H = p.H, W = p.W;

    for (int i = tid; i < kStage * kStage; i += kBlock) {
        const int r = i / kStage, c = i - r * kStage;
        const int y = y0 + r, x = x0 + c;
        float va = 0.f, vb = 0.f;
        if (y < H && x < W) {
            va = load_px<U8>(p.a, nc, p.C, H, W, y, x);
            vb = load_px<U8>(p.b, nc, p.C, H, W, y, x);
        }
        sA[i] = va;
        sB[i] = vb;
    }
    __syncthreads();

    // pixels this tile owns: its kTile x kTile block, up to the image's edge for the last tile of a row / column (<= kStage)
    const int own_h = (ty == p.tiles_y - 1) ? H - y0 : kTile;
    const int own_w = (tx == p.tiles_x - 1) ? W - x0 : kTile;
    double se = 0.0, ae = 0.0;
    if (L0) {
        for (int i = tid; i < own_h * own_w; i += kBlock) {
            const int r = i / own_w, c = i - r * own_w;
            const double d = (double)sA[r * kStage + c] - (double)sB[r * kStage + c];
            se += d * d;
            ae += fabs(d);
        }
    }
    if (p.pa != nullptr) {
        const int PH = H >> 1, PW = W >> 1;
        const int py0 = y0 >> 1, px0 = x0 >> 1;                       // (kTile is even)
        const int ph = ((ty == p.tiles_y - 1) ? PH : py0 + kTile / 2) - py0;
        const int pw = ((tx == p.tiles_x - 1) ? PW : px0 + kTile / 2) - px0;
        for (int i = tid; i < ph * pw; i += kBlock) {
            const int r = i / pw, c = i - r * pw;
            const int s = (2 * r) * kStage + 2 * c;
            const float qa = ((sA[s] + sA[s + 1]) + (sA[s + kStage] + sA[s + kStage + 1])) * 0.25f;
            const float qb = ((sB[s] + sB[s + 1]) + (sB[s + kStage] + sB[s + kStage + 1])) * 0.25f;
            const int64_t o = ((int64_t)nc * PH + (py0 + r)) * PW + (px0 + c);
            p.pa[o] = qa;
            p.pb[o] = qb;
        }
    }

    const int col = tid & (kTile - 1), grp = tid / kTile;              // one wave per row group
    const int Ho = H - kHalo, Wo = W - kHalo;
    const int oy0 = y0 + grp * kRows;
    double s_ssim = 0.0, s_cs = 0.0;
    if (oy0 < Ho) {                                                    // wave-uniform
        float acc[kRows][5];
#pragma unroll
        for (int j = 0; j < kRows; ++j)
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[j][m] = 0.f;
        const float* ra = sA + (grp * kRows) * kStage + col;
        const float* rb = sB + (grp * kRows) * kStage + col;
#pragma unroll
        for (int rr = 0; rr < kRows + kHalo; ++rr) {
            float h[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const float va = ra[rr * kStage + k], vb = rb[rr * kStage + k];
                h[0] = __builtin_fmaf(kG[k], va, h[0]);
                h[1] = __builtin_fmaf(kG[k], vb, h[1]);
                h[2] = __builtin_fmaf(kG[k], va * va, h[2]);
                h[3] = __builtin_fmaf(kG[k], vb * vb, h[3]);
                h[4] = __builtin_fmaf(kG[k], va * vb, h[4]);
            }
#pragma unroll
            for (int j = 0; j < kRows; ++j) {
                if (rr - j >= 0 && rr - j < kWin) {                    // (resolved at compile time)
#pragma unroll
                    for (int m = 0; m < 5; ++m) acc[j][m] = __builtin_fmaf(kG[rr - j], h[m], acc[j][m]);
                }
            }
        }
        const bool col_ok = x0 + col < Wo;
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const float mu1 = acc[j][0], mu2 = acc[j][1];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = acc[j][2] - mu1_sq, s2 = acc[j][3] - mu2_sq, s12 = acc[j][4] - mu12;
            const float v1 = 2.0f * s12 + p.C2;
            const float v2 = s1 + s2 + p.C2;
            const float cs = v1 / v2;
            const float ss = ((2.0f * mu12 + p.C1) * v1) / ((mu1_sq + mu2_sq + p.C1) * v2);
            if (col_ok && oy0 + j < Ho) {
                s_ssim += (double)ss;
                s_cs += (double)cs;
            }
        }
    }

    // workgroup sums in a fixed order: xor tree inside each wave, then waves 0..3
    double v[kSlot] = {s_ssim, s_cs, se, ae};
#pragma unroll
    for (int q = 0; q < kSlot; ++q) v[q] = wave_sum(v[q]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < kSlot; ++q) sRed[tid >> 6][q] = v[q];
    }
    __syncthreads();
    if (tid < kSlot) {
        double t = sRed[0][tid];
        for (int w = 1; w < kBlock / 64; ++w) t += sRed[w][tid];
        p.slots[((int64_t)nc * (p.tiles_x * p.tiles_y) + tile) * kSlot + tid] = t;
    }
}

struct FinalArgs {
    const double* slots[kMaxLevels];
    int per_frame[kMaxLevels];          // c * tiles of the level
    double map_count[kMaxLevels];       // c * (H_k - 10) * (W_k - 10)
    double pixel_count;                 // c * H * W
    double range_sq;
    int levels;
    float* out;                         // [n, 5 + 2 * levels]
};

// One workgroup per frame; wave q < levels sums the level's ssim slots, wave levels + q its cs slots, the last two waves the squared and
// absolute errors of level 0: lane-strided partial sums, then the xor tree -- the same order for any batch.
__global__ __launch_bounds__(64 * (2 * kMaxLevels + 2)) void finalize_kernel(FinalArgs p) {
    __shared__ double sums[2 * kMaxLevels + 2];
    const int n = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = p.levels;
    int level, q;
    if (wave < L) { level = wave; q = 0; }
    else if (wave < 2 * L) { level = wave - L; q = 1; }
    else { level = 0; q = wave - 2 * L + 2; }
    const double* s = p.slots[level] + (int64_t)n * p.per_frame[level] * kSlot + q;
    double t = 0.0;
    for (int i = lane; i < p.per_frame[level]; i += 64) t += s[(int64_t)i * kSlot];
    t = wave_sum(t);
    if (lane == 0) sums[wave] = t;
    __syncthreads();
    if (threadIdx.x != 0) return;
    float* o = p.out + (int64_t)n * (5 + 2 * L);
    const double mse = sums[2 * L] / p.pixel_count;
    o[0] = (float)mse;
    o[1] = (float)(sums[2 * L + 1] / p.pixel_count);
    o[2] = mse > 0.0 ? (float)(10.0 * log10(p.range_sq / mse)) : INFINITY;
    double ms = 1.0;
    for (int k = 0; k < L; ++k) {
        const double ssim = sums[k] / p.map_count[k], cs = sums[L + k] / p.map_count[k];
        o[5 + k] = (float)ssim;
        o[5 + L + k] = (float)cs;
        ms *= pow(k == L - 1 ? ssim : cs, kMsWeights[k]);              // a negative mean: NaN, as in the reference
    }
    o[3] = o[5];
    o[4] = L == kMaxLevels ? (float)ms : NAN;
}

struct Plan {
    int h[kMaxLevels], w[kMaxLevels], tx[kMaxLevels], ty[kMaxLevels];
    size_t slot_off[kMaxLevels];        // bytes
    size_t img_off[kMaxLevels];         // bytes, level >= 1: a then b
    size_t bytes;
};

int make_plan(const char* what, int n, int c, int h, int w, int levels, Plan& pl) {
    IA_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: n, h, w must be positive, got n=%d h=%d w=%d", what, n, h, w);
    IA_REQUIRE(c >= 1 && c <= 4, "%s: c must be in 1..4, got %d", what, c);
    IA_REQUIRE(levels >= 1 && levels <= kMaxLevels, "%s: levels must be in 1..%d, got %d", what, kMaxLevels, levels);
    IA_REQUIRE(((h < w ? h : w) >> (levels - 1)) >= kWin, "%s: a %d x %d image is too small for %d levels (the smaller side >> %d must be >= %d)",
               what, h, w, levels, levels - 1, kWin);
    IA_REQUIRE((int64_t)n * c <= 65535 && (int64_t)n * c * h * w < ((int64_t)1 << 40), "%s: batch too large (n * c = %lld)", what, (long long)n * c);
    size_t off = 0;
    for (int k = 0; k < levels; ++k) {
        pl.h[k] = h >> k;
        pl.w[k] = w >> k;
        pl.tx[k] = (int)ia::ceil_div(pl.w[k] - kHalo, kTile);
        pl.ty[k] = (int)ia::ceil_div(pl.h[k] - kHalo, kTile);
        pl.slot_off[k] = off;
        off += (size_t)n * c * pl.tx[k] * pl.ty[k] * kSlot * sizeof(double);
    }
    for (int k = 1; k < levels; ++k) {
        pl.img_off[k] = off;
        off += 2 * (size_t)n * c * pl.h[k] * pl.w[k] * sizeof(float);
    }
    pl.bytes = off;
    return IA_OK;
}

}  // namespace

extern "C" int ia_image_metrics_scratch_bytes(int n, int c, int h, int w, int levels, size_t* h_bytes) {
    IA_REQUIRE(h_bytes != nullptr, "ia_image_metrics_scratch_bytes: null output pointer");
    Plan pl;
    const int st = make_plan("ia_image_metrics_scratch_bytes", n, c, h, w, levels, pl);
    if (st != IA_OK) return st;
    *h_bytes = pl.bytes;
    return IA_OK;
}

extern "C" int ia_image_metrics(const void* a, const void* b, int layout, int n, int c, int h, int w, float data_range, int levels,
                                void* scratch, size_t scratch_bytes, float* out, void* stream) {
    IA_REQUIRE(a != nullptr && b != nullptr && scratch != nullptr && out != nullptr, "ia_image_metrics: null device pointers");
    IA_REQUIRE(layout == IA_IMAGE_F32_NCHW || layout == IA_IMAGE_U8_NHWC, "ia_image_metrics: unknown layout %d", layout);
    IA_REQUIRE(data_range > 0.f, "ia_image_metrics: data_range must be positive, got %g", (double)data_range);
    Plan pl;
    const int st = make_plan("ia_image_metrics", n, c, h, w, levels, pl);
    if (st != IA_OK) return st;
    IA_REQUIRE(scratch_bytes >= pl.bytes, "ia_image_metrics: scratch too small: %zu bytes given, %zu needed", scratch_bytes, pl.bytes);
    IA_REQUIRE(((uintptr_t)scratch & 7) == 0, "ia_image_metrics: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)scratch;
    const double L = (double)data_range;
    FinalArgs fa{};
    for (int k = 0; k < levels; ++k) {
        LevelArgs la{};
        const size_t plane = (size_t)n * c * pl.h[k] * pl.w[k] * sizeof(float);
        la.a = k == 0 ? a : (const void*)(base + pl.img_off[k]);
        la.b = k == 0 ? b : (const void*)(base + pl.img_off[k] + plane);
        if (k + 1 < levels) {
            const size_t next = (size_t)n * c * pl.h[k + 1] * pl.w[k + 1] * sizeof(float);
            la.pa = (float*)(base + pl.img_off[k + 1]);
            la.pb = (float*)(base + pl.img_off[k + 1] + next);
        }
        la.slots = (double*)(base + pl.slot_off[k]);
        la.C = c; la.H = pl.h[k]; la.W = pl.w[k];
        la.tiles_x = pl.tx[k]; la.tiles_y = pl.ty[k];
        la.C1 = (float)((0.01 * L) * (0.01 * L));
        la.C2 = (float)((0.03 * L) * (0.03 * L));
        const dim3 grid(pl.tx[k] * pl.ty[k], n * c);
        if (k > 0) ssim_level_kernel<false, false><<<grid, kBlock, 0, s>>>(la);
        else if (layout == IA_IMAGE_U8_NHWC) ssim_level_kernel<true, true><<<grid, kBlock, 0, s>>>(la);
        else ssim_level_kernel<false, true><<<grid, kBlock, 0, s>>>(la);
        const int e = ia::check_launch("ia_image_metrics (level)");
        if (e != IA_OK) return e;
        fa.slots[k] = la.slots;
        fa.per_frame[k] = c * pl.tx[k] * pl.ty[k];
        fa.map_count[k] = (double)c * (pl.h[k] - kHalo) * (pl.w[k] - kHalo);
    }
    fa.pixel_count = (double)c * h * w;
    fa.range_sq = L * L;
    fa.levels = levels;
    fa.out = out;
    finalize_kernel<<<n, 64 * (2 * levels + 2), 0, s>>>(fa);
    return ia::check_launch("ia_image_metrics (finalize)");
}
