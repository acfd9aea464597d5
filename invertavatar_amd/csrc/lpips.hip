// LPIPS on the device: the kernels the perceptual score needs besides the 3x3 MFMA convolutions (conv_split.hip).  Replaces, for
// evaluation (no gradients), encoder_inversion/criteria/lpips: torchvision's AlexNet / VGG16 feature stacks, normalize_activation, the
// 1x1 linear layers and the spatial means.
//
// conv_direct_kernel: fp32 direct convolution + bias + ReLU for the layers no MFMA kernel here takes (AlexNet's 11x11 stride 4 and 5x5,
// 3-channel inputs, O < 128, maps below 8^2).  A 256-thread workgroup makes a 16 x 16 pixel x 32 channel tile of one image: per chunk
// of CI input channels it stages the (15 s + k)^2 input windows (zeros outside the image) and the [CI][k*k][32] weight slice in LDS;
// thread t owns pixels (t & 15, (t >> 4) & 7) and 8 rows below and the 16 output channels of half t >> 7: one ds_read_b32 per pixel and
// four broadcast ds_read_b128 of weights feed 32 fused multiply-adds.  With stride s the window's columns are stored de-interleaved
// (column x at (x % s) * pw + x / s), so that the 16 lanes of a tile row read consecutive words for every tap.  The sum is blocked: a
// chunk's terms (at most kChunkTerms of them, in the order i, ky, kx) are added up on their own and the chunks' sums in chunk order, so
// that the rounding error grows with the square root of the chunk's length and of the number of chunks, not of I * k * k (a plain
// running sum over the 1 728 terms of a 192-channel 3x3 layer was 5 x as far from fp64 as the CPU's fp32 convolution).  The order is
// the same for every pixel, batch and run.
//
// maxpool_kernel: k3 s2 / k2 s2, floor mode; one thread = one output pixel of one channel (fp32 only) or of one 8-channel group (when
// the split operand of the next convolution is written as well: one 16-byte store per plane).
//
// lpips_layer_kernel / lpips_finalize_kernel: see include/ia_hip.h for the formulas and the summation order.
#include "ia_common.h"

#include <cmath>

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------ direct convolution

constexpr int kTilePx = 16;                    // output pixels per tile edge
constexpr int kTileOc = 32;                    // output channels per workgroup: two halves of 16
constexpr int kConvBlock = 256;
constexpr int kMaxK = 11;
constexpr int kMaxChunk = 16;                  // input channels staged at a time, at most
constexpr int kLdsBudgetFloats = 12 * 1024;    // 48 KB of dynamic LDS per workgroup: three workgroups per CU
constexpr int kChunkTerms = 144;               // terms per block of the blocked summation (16 channels of a 3x3 layer)

struct ConvArgs {
    const float* x;
    const float* w;
    const float* bias;
    float* y;
    int I, O, H, W, OH, OW;
    int k, stride, pad, relu;
    int tiles_x;
    int chunk;                                 // input channels per chunk
    int win;                                   // staged window edge: (kTilePx - 1) * stride + k
    int pw;                                    // words per column phase: ceil(win / stride)
};

// K > 0: the kernel size at compile time (taps unrolled); K == 0: p.k at run time.
template <int K, int S>
__global__ __launch_bounds__(kConvBlock) void conv_direct_kernel(ConvArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int k = K > 0 ? K : p.k;
    const int kk = k * k;
    const int win = p.win, pw = p.pw, pitch = S * pw;
    float* sW = lds;                                           // [chunk][kk][32]
    float* sX = lds + p.chunk * kk * kTileOc;                  // [chunk][win][pitch]
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, n = blockIdx.z;
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int oc0 = blockIdx.y * kTileOc;
    const int oy0 = ty * kTilePx, ox0 = tx * kTilePx;
    const int iy0 = oy0 * S - p.pad, ix0 = ox0 * S - p.pad;
    const int half = tid >> 7, px = tid & 15, py = (tid >> 4) & 7;

    float sum0[16], sum1[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) { sum0[j] = 0.f; sum1[j] = 0.f; }

    for (int c0 = 0; c0 < p.I; c0 += p.chunk) {
        const int cn = (p.I - c0) < p.chunk ? (p.I - c0) : p.chunk;
        float acc0[16], acc1[16];                              // this chunk's terms: blocked summation, see the header comment
#pragma unroll
        for (int j = 0; j < 16; ++j) { acc0[j] = 0.f; acc1[j] = 0.f; }
        __syncthreads();                                       // the previous chunk has been consumed
        for (int i = tid; i < cn * win * win; i += kConvBlock) {
            const int ci = i / (win * win), r = (i - ci * win * win) / win, c = i - ci * win * win - r * win;
            const int y = iy0 + r, x = ix0 + c;
            float v = 0.f;
            if (y >= 0 && y < p.H && x >= 0 && x < p.W) v = p.x[(((int64_t)n * p.I + (c0 + ci)) * p.H + y) * p.W + x];
            sX[(ci * win + r) * pitch + (c % S) * pw + c / S] = v;
        }
        for (int i = tid; i < cn * kk * kTileOc; i += kConvBlock) {
            const int j = i & (kTileOc - 1), rem = i / kTileOc;       // rem = ci * kk + tap
            const int oc = oc0 + j;
            sW[i] = oc < p.O ? p.w[((int64_t)oc * p.I + c0) * kk + rem] : 0.f;
        }
        __syncthreads();
        for (int ci = 0; ci < cn; ++ci) {
            const float* xin = sX + ci * win * pitch + px;
            const float* wc = sW + ci * kk * kTileOc + half * 16;
#pragma unroll 1
            for (int ky = 0; ky < k; ++ky) {
                const float* r0 = xin + (py * S + ky) * pitch;
                const float* r1 = r0 + 8 * S * pitch;
#pragma unroll
                for (int kx = 0; kx < (K > 0 ? K : kMaxK); ++kx) {
                    if (K == 0 && kx >= k) break;
                    const int off = (kx % S) * pw + kx / S;
                    const float x0 = r0[off], x1 = r1[off];
                    const float4* wv = reinterpret_cast<const float4*>(wc + (ky * k + kx) * kTileOc);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 w4 = wv[q];
                        acc0[4 * q + 0] = __builtin_fmaf(w4.x, x0, acc0[4 * q + 0]);
                        acc0[4 * q + 1] = __builtin_fmaf(w4.y, x0, acc0[4 * q + 1]);
                        acc0[4 * q + 2] = __builtin_fmaf(w4.z, x0, acc0[4 * q + 2]);
                        acc0[4 * q + 3] = __builtin_fmaf(w4.w, x0, acc0[4 * q + 3]);
                        acc1[4 * q + 0] = __builtin_fmaf(w4.x, x1, acc1[4 * q + 0]);
                        acc1[4 * q + 1] = __builtin_fmaf(w4.y, x1, acc1[4 * q + 1]);
                        acc1[4 * q + 2] = __builtin_fmaf(w4.z, x1, acc1[4 * q + 2]);
                        acc1[4 * q + 3] = __builtin_fmaf(w4.w, x1, acc1[4 * q + 3]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) { sum0[j] += acc0[j]; sum1[j] += acc1[j]; }
    }

    const int ox = ox0 + px;
    if (ox >= p.OW) return;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int oc = oc0 + half * 16 + j;
        if (oc >= p.O) break;
        const float b = p.bias ? p.bias[oc] : 0.f;
        float* yo = p.y + ((int64_t)n * p.O + oc) * p.OH * p.OW;
        const int ya = oy0 + py, yb = ya + 8;
        float v0 = sum0[j] + b, v1 = sum1[j] + b;
        if (p.relu) { v0 = v0 < 0.f ? 0.f : v0; v1 = v1 < 0.f ? 0.f : v1; }
        if (ya < p.OH) yo[(int64_t)ya * p.OW + ox] = v0;
        if (yb < p.OH) yo[(int64_t)yb * p.OW + ox] = v1;
    }
}

// ------------------------------------------------------------------ max pool

template <int K, bool SPLIT>
__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, h16x8* __restrict__ ys, int planes,
                                                      int N, int C, int H, int W, int OH, int OW) {
    constexpr int G = SPLIT ? 8 : 1;                           // channels per thread
    const int CG = C / G;
    const int64_t OP = (int64_t)OH * OW;
    const int64_t total = (int64_t)N * CG * OP, stride = (int64_t)gridDim.x * blockDim.x;
    ia::SatWatch watch;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t pix = i % OP;
        const int cg = (int)((i / OP) % CG), n = (int)(i / (OP * CG));
        const int oy = (int)(pix / OW), ox = (int)(pix - (int64_t)oy * OW);
        h16x8 hi, lo;
#pragma unroll
        for (int cc = 0; cc < G; ++cc) {
            const int c = cg * G + cc;
            const float* src = x + (((int64_t)n * C + c) * H + 2 * oy) * W + 2 * ox;
            float m = -INFINITY;
#pragma unroll
            for (int r = 0; r < K; ++r)
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    const float v = src[(int64_t)r * W + q];
                    if (v > m || v != v) m = v;
                }
            if (y) y[((int64_t)n * C + c) * OP + pix] = m;
            if (SPLIT) {
                if (planes == 2) { _Float16 h, l; ia::split_f16(m, h, l, watch); hi[cc] = h; lo[cc] = l; }
                else hi[cc] = ia::round_f16(m, watch);
            }
        }
        if (SPLIT) {
            ys[((int64_t)n * planes * CG + cg) * OP + pix] = hi;
            if (planes == 2) ys[(((int64_t)n * 2 + 1) * CG + cg) * OP + pix] = lo;
        }
    }
    watch.report();
}

// ------------------------------------------------------------------ LPIPS head

constexpr int kHeadBlock = 256;                // pixels per workgroup
constexpr float kEps = 1e-10f;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(kHeadBlock) void lpips_layer_kernel(const float* __restrict__ f, const float* __restrict__ lin, double* __restrict__ slots,
                                                                 int N, int C, int64_t P, int blocks) {
    __shared__ double sRed[kHeadBlock / 64];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int64_t pix = (int64_t)blockIdx.x * kHeadBlock + tid;
    double d = 0.0;
    if (pix < P) {
        const float* fx = f + (int64_t)n * C * P + pix;
        const float* fy = f + ((int64_t)N + n) * C * P + pix;
        float sx = 0.f, sy = 0.f;
        for (int c = 0; c < C; ++c) {
            const float a = fx[(int64_t)c * P], b = fy[(int64_t)c * P];
            sx += a * a;
            sy += b * b;
        }
        const float dx = sqrtf(sx) + kEps, dy = sqrtf(sy) + kEps;
        for (int c = 0; c < C; ++c) {
            const float a = fx[(int64_t)c * P] / dx, b = fy[(int64_t)c * P] / dy;
            const double t = (double)(a - b);
            d += (double)lin[c] * (t * t);
        }
    }
    d = wave_sum(d);
    if ((tid & 63) == 0) sRed[tid >> 6] = d;
    __syncthreads();
    if (tid == 0) {
        double t = sRed[0];
        for (int w = 1; w < kHeadBlock / 64; ++w) t += sRed[w];
        slots[(int64_t)n * blocks + blockIdx.x] = t;
    }
}

// One wave per pair: lane-strided partial sums of the pair's slots, then the xor tree -- the same order for any batch.
__global__ __launch_bounds__(64) void lpips_finalize_kernel(const double* __restrict__ slots, int blocks, double pixels, float* __restrict__ out,
                                                            int out_stride) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const double* s = slots + (int64_t)n * blocks;
    double t = 0.0;
    for (int i = lane; i < blocks; i += 64) t += s[i];
    t = wave_sum(t);
    if (lane == 0) out[(int64_t)n * out_stride] = (float)(t / pixels);
}

template <int K, int S>
int launch_conv(const ConvArgs& a, dim3 grid, size_t lds_bytes, hipStream_t s) {
    conv_direct_kernel<K, S><<<grid, kConvBlock, lds_bytes, s>>>(a);
    return ia::check_launch("ia_conv2d_direct");
}

}  // namespace

extern "C" int ia_conv2d_direct(const float* x, const float* w, const float* bias, float* y, int N, int I, int O, int H, int W, int k, int stride,
                                int pad, int act, void* stream) {
    IA_REQUIRE(x != nullptr && w != nullptr && y != nullptr, "ia_conv2d_direct: null device pointers");
    IA_REQUIRE(N >= 1 && I >= 1 && O >= 1 && H >= 1 && W >= 1, "ia_conv2d_direct: empty tensor (N=%d I=%d O=%d H=%d W=%d)", N, I, O, H, W);
    IA_REQUIRE(k >= 1 && k <= kMaxK, "ia_conv2d_direct: kernel size must be in 1..%d, got %d", kMaxK, k);
    IA_REQUIRE(stride == 1 || stride == 4, "ia_conv2d_direct: stride must be 1 or 4, got %d", stride);
    IA_REQUIRE(pad >= 0 && pad < k, "ia_conv2d_direct: padding must be in 0..k-1, got %d", pad);
    IA_REQUIRE(act == IA_ACT_LINEAR || act == IA_ACT_RELU, "ia_conv2d_direct: act must be IA_ACT_LINEAR or IA_ACT_RELU, got %d", act);
    IA_REQUIRE(H + 2 * pad >= k && W + 2 * pad >= k, "ia_conv2d_direct: a %d x %d image (padding %d) is smaller than the %d x %d kernel", H, W, pad, k, k);
    IA_REQUIRE(N <= 65535, "ia_conv2d_direct: batch too large (%d > 65535)", N);
    ConvArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    a.I = I; a.O = O; a.H = H; a.W = W;
    a.OH = (H + 2 * pad - k) / stride + 1;
    a.OW = (W + 2 * pad - k) / stride + 1;
    a.k = k; a.stride = stride; a.pad = pad; a.relu = act == IA_ACT_RELU;
    a.tiles_x = (int)ia::ceil_div(a.OW, kTilePx);
    const int tiles_y = (int)ia::ceil_div(a.OH, kTilePx);
    a.win = (kTilePx - 1) * stride + k;
    a.pw = (int)ia::ceil_div(a.win, stride);
    const int per_channel = a.win * stride * a.pw + k * k * kTileOc;          // floats of LDS per staged input channel
    int chunk = kLdsBudgetFloats / per_channel;
    if (chunk > kMaxChunk) chunk = kMaxChunk;
    if (chunk > kChunkTerms / (k * k)) chunk = kChunkTerms / (k * k) > 1 ? kChunkTerms / (k * k) : 1;
    if (chunk > I) chunk = I;
    IA_REQUIRE(chunk >= 1, "ia_conv2d_direct: one input channel of a k=%d stride=%d tile does not fit the LDS budget", k, stride);
    a.chunk = chunk;
    const int64_t oc_tiles = ia::ceil_div(O, kTileOc);
    IA_REQUIRE(oc_tiles <= 65535 && (int64_t)a.tiles_x * tiles_y < ((int64_t)1 << 31), "ia_conv2d_direct: too many tiles");
    const size_t lds_bytes = (size_t)chunk * per_channel * sizeof(float);
    const dim3 grid((unsigned)(a.tiles_x * tiles_y), (unsigned)oc_tiles, (unsigned)N);
    hipStream_t s = (hipStream_t)stream;
    if (stride == 4) return k == 11 ? launch_conv<11, 4>(a, grid, lds_bytes, s) : launch_conv<0, 4>(a, grid, lds_bytes, s);
    if (k == 3) return launch_conv<3, 1>(a, grid, lds_bytes, s);
    if (k == 5) return launch_conv<5, 1>(a, grid, lds_bytes, s);
    return launch_conv<0, 1>(a, grid, lds_bytes, s);
}

extern "C" int ia_maxpool2d(const float* x, float* y, void* ys, int ys_planes, int N, int C, int H, int W, int k, int stride, void* stream) {
    IA_REQUIRE(x != nullptr && (y != nullptr || ys != nullptr), "ia_maxpool2d: null device pointers (x, and one of y / ys)");
    IA_REQUIRE(N >= 1 && C >= 1, "ia_maxpool2d: empty tensor (N=%d C=%d)", N, C);
    IA_REQUIRE((k == 3 || k == 2) && stride == 2, "ia_maxpool2d: (k, stride) must be (3, 2) or (2, 2), got (%d, %d)", k, stride);
    IA_REQUIRE(H >= k && W >= k, "ia_maxpool2d: a %d x %d map is smaller than the %d x %d window", H, W, k, k);
    if (ys != nullptr) {
        IA_REQUIRE(ys_planes == 1 || ys_planes == 2, "ia_maxpool2d: ys_planes: 2 = hi / lo pair, 1 = one fp16 plane");
        IA_REQUIRE(C % 8 == 0, "ia_maxpool2d: the split format stores channels in groups of 8 (C = %d)", C);
    }
    const int OH = (H - k) / 2 + 1, OW = (W - k) / 2 + 1;
    hipStream_t s = (hipStream_t)stream;
    h16x8* out_s = static_cast<h16x8*>(ys);
    const int64_t work = (int64_t)N * (ys ? C / 8 : C) * OH * OW;
    const dim3 grid(ia::streaming_grid(work, 256));
    if (ys) {
        if (k == 3) maxpool_kernel<3, true><<<grid, 256, 0, s>>>(x, y, out_s, ys_planes, N, C, H, W, OH, OW);
        else maxpool_kernel<2, true><<<grid, 256, 0, s>>>(x, y, out_s, ys_planes, N, C, H, W, OH, OW);
    } else {
        if (k == 3) maxpool_kernel<3, false><<<grid, 256, 0, s>>>(x, y, out_s, 0, N, C, H, W, OH, OW);
        else maxpool_kernel<2, false><<<grid, 256, 0, s>>>(x, y, out_s, 0, N, C, H, W, OH, OW);
    }
    return ia::check_launch("ia_maxpool2d");
}

extern "C" int ia_lpips_layer_scratch_bytes(int N, int h, int w, size_t* h_bytes) {
    IA_REQUIRE(h_bytes != nullptr, "ia_lpips_layer_scratch_bytes: null output pointer");
    IA_REQUIRE(N >= 1 && h >= 1 && w >= 1, "ia_lpips_layer_scratch_bytes: N, h, w must be positive, got N=%d h=%d w=%d", N, h, w);
    *h_bytes = (size_t)N * (size_t)ia::ceil_div((int64_t)h * w, kHeadBlock) * sizeof(double);
    return IA_OK;
}

extern "C" int ia_lpips_layer(const float* f, const float* lin, int N, int C, int h, int w, void* scratch, size_t scratch_bytes, float* out,
                              int out_stride, void* stream) {
    IA_REQUIRE(f != nullptr && lin != nullptr && scratch != nullptr && out != nullptr, "ia_lpips_layer: null device pointers");
    IA_REQUIRE(N >= 1 && C >= 1 && h >= 1 && w >= 1, "ia_lpips_layer: N, C, h, w must be positive, got N=%d C=%d h=%d w=%d", N, C, h, w);
    IA_REQUIRE(N <= 65535, "ia_lpips_layer: batch too large (%d > 65535 pairs)", N);
    IA_REQUIRE(out_stride >= 1, "ia_lpips_layer: out_stride must be positive, got %d", out_stride);
    const int64_t P = (int64_t)h * w;
    const int64_t blocks = ia::ceil_div(P, kHeadBlock);
    IA_REQUIRE(blocks < ((int64_t)1 << 31), "ia_lpips_layer: map too large");
    IA_REQUIRE(scratch_bytes >= (size_t)N * blocks * sizeof(double), "ia_lpips_layer: scratch too small: %zu bytes given, %zu needed", scratch_bytes,
               (size_t)N * blocks * sizeof(double));
    IA_REQUIRE(((uintptr_t)scratch & 7) == 0, "ia_lpips_layer: scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    lpips_layer_kernel<<<dim3((unsigned)blocks, (unsigned)N), kHeadBlock, 0, s>>>(f, lin, (double*)scratch, N, C, P, (int)blocks);
    const int e = ia::check_launch("ia_lpips_layer (pixels)");
    if (e != IA_OK) return e;
    lpips_finalize_kernel<<<N, 64, 0, s>>>((const double*)scratch, (int)blocks, (double)P, out, out_stride);
    return ia::check_launch("ia_lpips_layer (finalize)");
}
