// The contextual loss (CX) on the device: the bilinear resize in front of the VGG19 trunk and the head.  Replaces, for evaluation (no
// gradients), encoder_inversion/criteria/cx_loss.py: F.interpolate(bilinear, align_corners=False) and contextual_loss(); the trunk is
// the convolutions and pools of lpips.hip / conv_split.hip.  See include/ia_hip.h for the formulas.
//
// The head never stores the P x P matrix d_ij = 1 - x^_i . y^_j.  cx_rows_kernel keeps 64 rows of x^ in LDS and sweeps the columns of
// y^ twice (row minimum, then row sum of w); cx_cols_kernel keeps 64 columns of y^ in LDS and sweeps the rows of x^ (column maximum of
// w / s).  Both form d with tiles_dot below: x^ is always the A operand and y^ the B operand of v_mfma_f32_16x16x4_f32, 16 channels
// (four instructions) per fp32 accumulator, the accumulators added in double in channel order -- so the two kernels see the same bits
// of d, and m_i really is the minimum of the d that cx_cols_kernel divides by it.
//
// Product form: fp32 MFMA, not the fp16 hi / lo three-product form.  t = d / (m + 1e-5) turns an absolute error of 1e-7 in a dot product
// into 1 % of t where two positions nearly coincide.  The fp32 instruction is an exact fmaf chain (2^-24 per step, 16 steps per
// accumulator, then double); a hi / lo pair carries 22 mantissa bits per operand, 2^-22 per PRODUCT, four times as much before any
// accumulation.  At 13 GFLOP for a 4096-position pair the fp32 matrix rate is no bottleneck.
#include "ia_common.h"

#include <cmath>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ bilinear resize

// torch's upsample_bilinear2d, align_corners = False: source coordinate s = max(0, (In / Out) (o + 0.5) - 0.5), taps floor(s) and the
// next sample (clamped), weights 1 - frac and frac.  The coordinate is computed in double; the weights and the blend are fp32.
__device__ __forceinline__ void tap(int o, int in, int out, int& i0, int& i1, float& w0, float& w1) {
    double s = ((double)in / (double)out) * ((double)o + 0.5) - 0.5;
    s = s < 0.0 ? 0.0 : s;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    w1 = (float)(s - (double)i0);
    w0 = 1.f - w1;
}

template <bool U8>
__device__ __forceinline__ float pixel(const void* src, int n, int c, int C, int H, int W, int y, int x) {
    if (U8) return (float)static_cast<const unsigned char*>(src)[(((int64_t)n * H + y) * W + x) * C + c] / 127.5f - 1.0f;
    return static_cast<const float*>(src)[(((int64_t)n * C + c) * H + y) * W + x];
}

// One thread = one output pixel.  HALF: the exact 2 : 1 case, where every coordinate is 2 o + 0.5 and all weights are 0.5.
template <bool U8, bool HALF>
__global__ __launch_bounds__(256) void resize_kernel(const void* __restrict__ src, float* __restrict__ dst, int N, int C, int H, int W, int OH, int OW) {
    const int64_t total = (int64_t)N * C * OH * OW, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
        const int c = (int)((i / ((int64_t)OW * OH)) % C), n = (int)(i / ((int64_t)OW * OH * C));
        int y0, y1, x0, x1;
        float wy0, wy1, wx0, wx1;
        if (HALF) {
            y0 = 2 * oy; y1 = y0 + 1; x0 = 2 * ox; x1 = x0 + 1;
            wy0 = wy1 = wx0 = wx1 = 0.5f;
        } else {
            tap(oy, H, OH, y0, y1, wy0, wy1);
            tap(ox, W, OW, x0, x1, wx0, wx1);
        }
        const float v00 = pixel<U8>(src, n, c, C, H, W, y0, x0), v01 = pixel<U8>(src, n, c, C, H, W, y0, x1);
        const float v10 = pixel<U8>(src, n, c, C, H, W, y1, x0), v11 = pixel<U8>(src, n, c, C, H, W, y1, x1);
        dst[i] = wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11);
    }
}

// ------------------------------------------------------------------ head: means and operands

constexpr int kTile = 64;                      // rows of x^ (cx_rows) / columns of y^ (cx_cols) per workgroup, and per sweep step
constexpr int kHeadBlock = 256;                // four waves, 16 rows / columns each
constexpr int kStepK = 16;                     // channels per fp32 accumulator: C is padded to a multiple of it
constexpr int kRowPad = 4;                     // floats between LDS rows: a row starts 16 bytes on from a multiple of 64 banks
constexpr int kMaxCpad = 624;                  // 64 x (624 + 4) x 4 bytes = 157 KB of the 160 KB

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One workgroup per (frame, channel): lane-strided double partials, xor tree in each wave, the waves in order.
__global__ __launch_bounds__(kHeadBlock) void channel_mean_kernel(const float* __restrict__ f, double* __restrict__ mean64, float* __restrict__ mu,
                                                                  int64_t P) {
    __shared__ double sRed[kHeadBlock / 64];
    const int tid = threadIdx.x;
    const float* src = f + (int64_t)blockIdx.x * P;
    double t = 0.0;
    for (int64_t p = tid; p < P; p += kHeadBlock) t += (double)src[p];
    t = wave_sum(t);
    if ((tid & 63) == 0) sRed[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) {
        double a = sRed[0];
        for (int w = 1; w < kHeadBlock / 64; ++w) a += sRed[w];
        a /= (double)P;
        mean64[blockIdx.x] = a;
        mu[blockIdx.x] = (float)a;
    }
}

// The batch row: the frames' means added in frame order, in double.
__global__ __launch_bounds__(256) void batch_mean_kernel(const double* __restrict__ mean64, float* __restrict__ mu_batch, int N, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a = 0.0;
    for (int n = 0; n < N; ++n) a += mean64[(int64_t)n * C + c];
    mu_batch[c] = (float)(a / (double)N);
}

// One thread per position: v_c = f_c - mu_c (fp32), norm = fp32(sqrt(sum_c v_c^2 in double, channel order)), out_c = v_c / max(norm, 1e-12)
// with a NaN norm kept (torch's clamp_min); channels C .. Cpad - 1 are zero.
__global__ __launch_bounds__(256) void normalize_kernel(const float* __restrict__ f, const float* __restrict__ mu, int mu_rows, float* __restrict__ out,
                                                        int C, int64_t P, int cpad) {
    const int n = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const float* src = f + (int64_t)n * C * P + p;
    const float* m = mu + (mu_rows > 1 ? (int64_t)n * C : 0);
    double ss = 0.0;
    for (int c = 0; c < C; ++c) {
        const float v = src[(int64_t)c * P] - m[c];
        ss += (double)v * (double)v;
    }
    const float nrm = (float)sqrt(ss);
    const float den = nrm < 1e-12f ? 1e-12f : nrm;             // (a NaN norm stays NaN)
    float* dst = out + ((int64_t)n * P + p) * cpad;
    for (int c = 0; c < C; ++c) dst[c] = (src[(int64_t)c * P] - m[c]) / den;
    for (int c = C; c < cpad; ++c) dst[c] = 0.f;
}

// ------------------------------------------------------------------ head: the product and the three sweeps

// NA x NB tiles of 16 x 16 dot products over all `cpad` channels.  a[i] / b[j]: this lane's row of x^ / column of y^ (lane & 15 within
// the tile) at channel 4 (lane >> 4); LDS or global, 16-byte aligned.  A float4 feeds four MFMA steps: step s of a 16-channel group sums
// channels 4 g + s over the lane groups g -- a permutation of the channels, the same for both operands and for every caller.
// dot[i][j][r]: row 4 (lane >> 4) + r of tile i, column lane & 15 of tile j.
template <int NA, int NB>
__device__ __forceinline__ void tiles_dot(const float* const* a, const float* const* b, int cpad, double (&dot)[NA][NB][4]) {
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) dot[i][j][r] = 0.0;
    for (int k0 = 0; k0 < cpad; k0 += kStepK) {
        f32x4 av[NA], bv[NB];
#pragma unroll
        for (int i = 0; i < NA; ++i) av[i] = *reinterpret_cast<const f32x4*>(a[i] + k0);
#pragma unroll
        for (int j = 0; j < NB; ++j) bv[j] = *reinterpret_cast<const f32x4*>(b[j] + k0);
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][s], bv[j][s], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) dot[i][j][r] += (double)acc[r];
            }
    }
}

__device__ __forceinline__ float nan_min(float a, float b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// w_ij of the definition from d_ij and m_i, in double: exp((1 - clamp(d / (m + 1e-5), -10, 10)) / band_width).
__device__ __forceinline__ double weight(float d, float m, double inv_band) {
    double t = (double)d / ((double)m + 1e-5);
    t = t > 10.0 ? 10.0 : (t < -10.0 ? -10.0 : t);             // (NaN passes)
    return exp((1.0 - t) * inv_band);
}

// 64 rows of `src` [P][cpad] from row r0 (rows past P - 1 repeat row P - 1: computed, never used) -> LDS [64][cpad + kRowPad].
__device__ __forceinline__ void stage_block(float* lds, const float* __restrict__ src, int64_t r0, int64_t P, int cpad) {
    const int quads = cpad / 4, pitch = cpad + kRowPad;
    for (int i = threadIdx.x; i < kTile * quads; i += kHeadBlock) {
        const int r = i / quads, q = i - r * quads;
        int64_t row = r0 + r;
        if (row > P - 1) row = P - 1;
        *reinterpret_cast<f32x4*>(lds + r * pitch + 4 * q) = *reinterpret_cast<const f32x4*>(src + row * cpad + 4 * q);
    }
}

__global__ __launch_bounds__(kHeadBlock) void cx_rows_kernel(const float* __restrict__ xh, const float* __restrict__ yh, float* __restrict__ m_out,
                                                             double* __restrict__ s_out, int64_t P, int cpad, double inv_band) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int64_t i0 = (int64_t)blockIdx.x * kTile;
    const float* x = xh + (int64_t)n * P * cpad;
    const float* y = yh + (int64_t)n * P * cpad;
    stage_block(lds, x, i0, P, cpad);
    __syncthreads();
    const float* a[1] = {lds + (wave * 16 + c) * (cpad + kRowPad) + 4 * g};
    double dot[1][4][4];

    float m[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    for (int64_t j0 = 0; j0 < P; j0 += kTile) {
        const float* b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int64_t col = j0 + 16 * t + c;
            b[t] = y + (col < P ? col : P - 1) * cpad + 4 * g;
        }
        tiles_dot<1, 4>(a, b, cpad, dot);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (j0 + 16 * t + c < P) {
#pragma unroll
                for (int r = 0; r < 4; ++r) m[r] = nan_min(m[r], (float)(1.0 - dot[0][t][r]));
            }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) m[r] = nan_min(m[r], __shfl_xor(m[r], off, 64));

    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t j0 = 0; j0 < P; j0 += kTile) {
        const float* b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int64_t col = j0 + 16 * t + c;
            b[t] = y + (col < P ? col : P - 1) * cpad + 4 * g;
        }
        tiles_dot<1, 4>(a, b, cpad, dot);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (j0 + 16 * t + c < P) {
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] += weight((float)(1.0 - dot[0][t][r]), m[r], inv_band);
            }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) s[r] += __shfl_xor(s[r], off, 64);

    if (c == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = i0 + wave * 16 + 4 * g + r;
            if (row < P) {
                m_out[(int64_t)n * P + row] = m[r];
                s_out[(int64_t)n * P + row] = s[r];
            }
        }
    }
}

__global__ __launch_bounds__(kHeadBlock) void cx_cols_kernel(const float* __restrict__ xh, const float* __restrict__ yh, const float* __restrict__ m_in,
                                                             const double* __restrict__ s_in, double* __restrict__ colmax, int64_t P, int cpad,
                                                             double inv_band) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int64_t j0 = (int64_t)blockIdx.x * kTile;
    const float* x = xh + (int64_t)n * P * cpad;
    const float* y = yh + (int64_t)n * P * cpad;
    const float* mrow = m_in + (int64_t)n * P;
    const double* srow = s_in + (int64_t)n * P;
    stage_block(lds, y, j0, P, cpad);
    __syncthreads();
    const float* b[1] = {lds + (wave * 16 + c) * (cpad + kRowPad) + 4 * g};
    double dot[4][1][4];

    double cm = -INFINITY;
    for (int64_t i0 = 0; i0 < P; i0 += kTile) {
        const float* a[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int64_t row = i0 + 16 * t + c;
            a[t] = x + (row < P ? row : P - 1) * cpad + 4 * g;
        }
        tiles_dot<4, 1>(a, b, cpad, dot);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = i0 + 16 * t + 4 * g + r;
                if (row < P) {
                    const float mi = mrow[row];
                    cm = nan_max(cm, weight((float)(1.0 - dot[t][0][r]), mi, inv_band) / srow[row]);
                }
            }
    }
    cm = nan_max(cm, __shfl_xor(cm, 16, 64));
    cm = nan_max(cm, __shfl_xor(cm, 32, 64));
    const int64_t col = j0 + wave * 16 + c;
    if (g == 0 && col < P) colmax[(int64_t)n * P + col] = cm;
}

// One wave per frame: lane-strided double partial sums of the column maxima, then the xor tree.
__global__ __launch_bounds__(64) void cx_finish_kernel(const double* __restrict__ colmax, int64_t P, float* __restrict__ cx, float* __restrict__ cx_loss) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const double* v = colmax + (int64_t)n * P;
    double t = 0.0;
    for (int64_t j = lane; j < P; j += 64) t += v[j];
    t = wave_sum(t) / (double)P;
    if (lane == 0) {
        cx[n] = (float)t;
        cx_loss[n] = (float)(-log(t + 1e-5));
    }
}

int head_args(const char* what, const void* xh, const void* yh, int N, int64_t P, int cpad) {
    IA_REQUIRE(xh != nullptr && yh != nullptr, "%s: null device pointers", what);
    IA_REQUIRE(N >= 1 && N <= 65535 && P >= 1, "%s: N in 1..65535 and P >= 1, got N=%d P=%lld", what, N, (long long)P);
    IA_REQUIRE(cpad >= kStepK && cpad % kStepK == 0, "%s: Cpad must be a positive multiple of %d, got %d", what, kStepK, cpad);
    IA_REQUIRE(ia::ceil_div(P, kTile) < ((int64_t)1 << 31), "%s: too many positions", what);
    IA_REQUIRE((((uintptr_t)xh | (uintptr_t)yh) & 15) == 0, "%s: the operands must be 16-byte aligned", what);
    if (cpad > kMaxCpad) return ia::fail(IA_ERR_UNSUPPORTED, "%s: Cpad = %d: a 64-row block of more than %d channels does not fit the LDS", what, cpad, kMaxCpad);
    return IA_OK;
}

size_t head_lds(int cpad) { return (size_t)kTile * (cpad + kRowPad) * sizeof(float); }

}  // namespace

extern "C" int ia_resize_bilinear(const void* src, int layout, float* dst, int N, int C, int H, int W, int OH, int OW, int general, void* stream) {
    IA_REQUIRE(src != nullptr && dst != nullptr, "ia_resize_bilinear: null device pointers");
    IA_REQUIRE(layout == IA_IMAGE_F32_NCHW || layout == IA_IMAGE_U8_NHWC, "ia_resize_bilinear: layout must be IA_IMAGE_F32_NCHW or IA_IMAGE_U8_NHWC");
    IA_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1, "ia_resize_bilinear: empty tensor (N=%d C=%d %dx%d -> %dx%d)", N, C, H, W, OH, OW);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ia::streaming_grid((int64_t)N * C * OH * OW, 256));
    const bool half = !general && H == 2 * OH && W == 2 * OW;
    if (layout == IA_IMAGE_U8_NHWC) {
        if (half) resize_kernel<true, true><<<grid, 256, 0, s>>>(src, dst, N, C, H, W, OH, OW);
        else resize_kernel<true, false><<<grid, 256, 0, s>>>(src, dst, N, C, H, W, OH, OW);
    } else {
        if (half) resize_kernel<false, true><<<grid, 256, 0, s>>>(src, dst, N, C, H, W, OH, OW);
        else resize_kernel<false, false><<<grid, 256, 0, s>>>(src, dst, N, C, H, W, OH, OW);
    }
    return ia::check_launch("ia_resize_bilinear");
}

extern "C" int ia_cx_layout(int* tile, int* k_step) {
    IA_REQUIRE(tile != nullptr && k_step != nullptr, "ia_cx_layout: null output pointers");
    *tile = kTile;
    *k_step = kStepK;
    return IA_OK;
}

extern "C" int ia_cx_scratch_bytes(int N, int C, int64_t P, size_t* h_bytes) {
    IA_REQUIRE(h_bytes != nullptr, "ia_cx_scratch_bytes: null output pointer");
    IA_REQUIRE(N >= 1 && C >= 1 && P >= 1, "ia_cx_scratch_bytes: N, C, P must be positive, got N=%d C=%d P=%lld", N, C, (long long)P);
    // double [N][C] channel means, double [N][P] row sums, double [N][P] column maxima, float [N][P] row minima
    *h_bytes = (size_t)N * ((size_t)C * 8 + (size_t)P * 20);
    return IA_OK;
}

extern "C" int ia_cx_channel_mean(const float* f, int N, int C, int64_t P, double* mean64, float* mu_frames, float* mu_batch, void* stream) {
    IA_REQUIRE(f != nullptr && mean64 != nullptr && mu_frames != nullptr, "ia_cx_channel_mean: null device pointers");
    IA_REQUIRE(N >= 1 && C >= 1 && P >= 1, "ia_cx_channel_mean: N, C, P must be positive, got N=%d C=%d P=%lld", N, C, (long long)P);
    IA_REQUIRE((int64_t)N * C < ((int64_t)1 << 31), "ia_cx_channel_mean: too many maps");
    IA_REQUIRE(((uintptr_t)mean64 & 7) == 0, "ia_cx_channel_mean: mean64 must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    channel_mean_kernel<<<(unsigned)(N * C), kHeadBlock, 0, s>>>(f, mean64, mu_frames, P);
    int e = ia::check_launch("ia_cx_channel_mean (frames)");
    if (e != IA_OK || mu_batch == nullptr) return e;
    batch_mean_kernel<<<(unsigned)ia::ceil_div(C, 256), 256, 0, s>>>(mean64, mu_batch, N, C);
    return ia::check_launch("ia_cx_channel_mean (batch)");
}

extern "C" int ia_cx_normalize(const float* f, const float* mu, int mu_rows, float* out, int N, int C, int64_t P, int cpad, void* stream) {
    IA_REQUIRE(f != nullptr && mu != nullptr && out != nullptr, "ia_cx_normalize: null device pointers");
    IA_REQUIRE(N >= 1 && N <= 65535 && C >= 1 && P >= 1, "ia_cx_normalize: N in 1..65535, C, P positive, got N=%d C=%d P=%lld", N, C, (long long)P);
    IA_REQUIRE(mu_rows == 1 || mu_rows == N, "ia_cx_normalize: mu has 1 or N rows, got %d", mu_rows);
    IA_REQUIRE(cpad >= C && cpad % kStepK == 0, "ia_cx_normalize: Cpad must be a multiple of %d that is >= C, got %d for C = %d", kStepK, cpad, C);
    IA_REQUIRE(ia::ceil_div(P, 256) < ((int64_t)1 << 31), "ia_cx_normalize: too many positions");
    normalize_kernel<<<dim3((unsigned)ia::ceil_div(P, 256), (unsigned)N), 256, 0, (hipStream_t)stream>>>(f, mu, mu_rows, out, C, P, cpad);
    return ia::check_launch("ia_cx_normalize");
}

extern "C" int ia_cx_rows(const float* xh, const float* yh, int N, int64_t P, int cpad, float band_width, float* m, double* s, void* stream) {
    int e = head_args("ia_cx_rows", xh, yh, N, P, cpad);
    if (e != IA_OK) return e;
    IA_REQUIRE(m != nullptr && s != nullptr && ((uintptr_t)s & 7) == 0, "ia_cx_rows: m and s (8-byte aligned) must be device pointers");
    IA_REQUIRE(band_width > 0.f, "ia_cx_rows: band_width must be positive, got %g", (double)band_width);
    e = ia::reserve_lds(reinterpret_cast<const void*>(cx_rows_kernel), head_lds(cpad), "ia_cx_rows");
    if (e != IA_OK) return e;
    cx_rows_kernel<<<dim3((unsigned)ia::ceil_div(P, kTile), (unsigned)N), kHeadBlock, head_lds(cpad), (hipStream_t)stream>>>(
        xh, yh, m, s, P, cpad, 1.0 / (double)band_width);
    return ia::check_launch("ia_cx_rows");
}

extern "C" int ia_cx_cols(const float* xh, const float* yh, const float* m, const double* s, int N, int64_t P, int cpad, float band_width,
                          double* colmax, void* stream) {
    int e = head_args("ia_cx_cols", xh, yh, N, P, cpad);
    if (e != IA_OK) return e;
    IA_REQUIRE(m != nullptr && s != nullptr && colmax != nullptr && (((uintptr_t)s | (uintptr_t)colmax) & 7) == 0,
               "ia_cx_cols: m, s and colmax (8-byte aligned) must be device pointers");
    IA_REQUIRE(band_width > 0.f, "ia_cx_cols: band_width must be positive, got %g", (double)band_width);
    e = ia::reserve_lds(reinterpret_cast<const void*>(cx_cols_kernel), head_lds(cpad), "ia_cx_cols");
    if (e != IA_OK) return e;
    cx_cols_kernel<<<dim3((unsigned)ia::ceil_div(P, kTile), (unsigned)N), kHeadBlock, head_lds(cpad), (hipStream_t)stream>>>(
        xh, yh, m, s, colmax, P, cpad, 1.0 / (double)band_width);
    return ia::check_launch("ia_cx_cols");
}

extern "C" int ia_cx_finish(const double* colmax, int N, int64_t P, float* cx, float* cx_loss, void* stream) {
    IA_REQUIRE(colmax != nullptr && cx != nullptr && cx_loss != nullptr && ((uintptr_t)colmax & 7) == 0, "ia_cx_finish: null or misaligned device pointers");
    IA_REQUIRE(N >= 1 && P >= 1, "ia_cx_finish: N and P must be positive, got N=%d P=%lld", N, (long long)P);
    cx_finish_kernel<<<(unsigned)N, 64, 0, (hipStream_t)stream>>>(colmax, P, cx, cx_loss);
    return ia::check_launch("ia_cx_finish");
}
