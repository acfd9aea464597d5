// Identity similarity (ArcFace IR-SE50, the reference's encoder_inversion/criteria/id_loss.py) on the device: the kernels the score
// needs besides the residual units that trunk_hip.py already runs on the MFMA convolutions.
//
// face_crop_pool_kernel: (AdaptiveAvgPool2d(256) when the frame is not 256^2) -> crop [35:223, 32:220] -> AdaptiveAvgPool2d(112) in one
// launch.  A thread owns one output pixel of one channel: it walks the 2 or 3 rows and columns of its 188 -> 112 window, and for each of
// those 256^2 cells the cell's own window of the frame.  Both stages are sum / count in fp32, row-major, torch's windows
// [floor(i In / Out), ceil((i + 1) In / Out)).
//
// conv3x3_small_kernel: 3x3, stride 1, padding 1 on maps with a side below 8 (the 7^2 stage of the network), fp32 fused multiply-adds.
// A 256-thread workgroup makes a (64 pixel) x (64 output channel) tile of one image over ONE chunk of 32 input channels: K is split
// across workgroups (grid.y), so that one pair's 512 -> 512 layer is 8 x 16 x 2 = 256 workgroups reading 9.4 MB of weights between
// them.  The chunk is staged 8 channels at a time: the (h + 2) x (w + 2) windows with the input affine applied and zeros around them
// (the padding belongs to the normalised tensor) and the [8][9][64] weight slice; wave g owns output channels 16 g .. 16 g + 15 and
// lane p pixel p: one ds_read_b32 of the pixel and four broadcast ds_read_b128 of weights feed 16 fused multiply-adds.  An 8-channel
// block's 72 terms are added on their own and the blocks in order; the chunks' partial sums go to scratch [KS][B][O][P] and
// conv3x3_small_combine_kernel adds them in chunk order and applies scale, shift and the PReLU slopes.  The split depends on I alone,
// so an image's result does not depend on the batch it is in.
//
// id_head_kernel / id_head_finish_kernel: Linear(K, O) with the BatchNorm2d in front folded into its weights on the host, split-K:
// a workgroup takes 4 output rows x one K slice and walks the batch 4 images at a time (thread t sums k = t, t + 256, ... in fp32,
// xor tree in each wave, the waves in order); the finishing launch adds a row's slices in order, applies the bias and the BatchNorm1d
// affine map, sums the squares in double (same tree) and divides by the fp32 norm.
//
// id_similarity_kernel: one wave per pair; fp32 products added in double, lane-strided + xor tree.
#include "ia_common.h"

#include <cmath>

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ------------------------------------------------------------------ crop + pool front end

constexpr int kFace = 256;                     // the frame size the crop is defined on
constexpr int kCropY = 35, kCropX = 32, kCrop = 188, kFaceOut = 112;

__device__ __forceinline__ int win_lo(int i, int in, int out) { return (int)(((int64_t)i * in) / out); }
__device__ __forceinline__ int win_hi(int i, int in, int out) { return (int)((((int64_t)i + 1) * in + out - 1) / out); }

template <bool U8>
__global__ __launch_bounds__(256) void face_crop_pool_kernel(const void* __restrict__ src, float* __restrict__ y, int N, int H, int W) {
    const int64_t total = (int64_t)N * 3 * kFaceOut * kFaceOut, stride = (int64_t)gridDim.x * blockDim.x;
    const bool direct = H == kFace && W == kFace;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int ox = (int)(i % kFaceOut), oy = (int)((i / kFaceOut) % kFaceOut);
        const int c = (int)((i / (kFaceOut * kFaceOut)) % 3), n = (int)(i / (3 * kFaceOut * kFaceOut));
        const int y0 = win_lo(oy, kCrop, kFaceOut), y1 = win_hi(oy, kCrop, kFaceOut);
        const int x0 = win_lo(ox, kCrop, kFaceOut), x1 = win_hi(ox, kCrop, kFaceOut);
        float sum = 0.f;
        for (int cy = y0; cy < y1; ++cy)
            for (int cx = x0; cx < x1; ++cx) {
                const int fy = cy + kCropY, fx = cx + kCropX;              // a cell of the 256^2 frame
                int sy0 = fy, sy1 = fy + 1, sx0 = fx, sx1 = fx + 1;
                if (!direct) {
                    sy0 = win_lo(fy, H, kFace); sy1 = win_hi(fy, H, kFace);
                    sx0 = win_lo(fx, W, kFace); sx1 = win_hi(fx, W, kFace);
                }
                float cell = 0.f;
                for (int sy = sy0; sy < sy1; ++sy)
                    for (int sx = sx0; sx < sx1; ++sx) {
                        float v;
                        if (U8) v = (float)static_cast<const unsigned char*>(src)[(((int64_t)n * H + sy) * W + sx) * 3 + c] / 127.5f - 1.0f;
                        else v = static_cast<const float*>(src)[(((int64_t)n * 3 + c) * H + sy) * W + sx];
                        cell += v;
                    }
                if (!direct) cell = cell / (float)((sy1 - sy0) * (sx1 - sx0));
                sum += cell;
            }
        y[i] = sum / (float)((y1 - y0) * (x1 - x0));
    }
}

// ------------------------------------------------------------------ per-channel PReLU (the input layer's tail)

__global__ __launch_bounds__(256) void prelu_kernel(const float* __restrict__ x, const float* __restrict__ slopes, float* __restrict__ y, int C,
                                                    int64_t P, int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const float v = x[i];
        y[i] = v < 0.f ? v * slopes[(i / P) % C] : v;
    }
}

// ------------------------------------------------------------------ 3x3 convolution on maps below 8^2

constexpr int kSmallBlock = 256;
constexpr int kSmallOc = 64;                   // output channels per workgroup: 4 waves x 16
constexpr int kSmallChunk = 32;                // input channels per workgroup (the K split)
constexpr int kSmallStage = 8;                 // input channels staged in LDS at a time
constexpr int kSmallPitch = 9;                 // padded window: up to (7 + 2) x (7 + 2)
constexpr int kSmallWin = kSmallPitch * kSmallPitch;

struct SmallArgs {
    const float* x;
    const float* wk;                           // [9][I][O]
    const float* in_scale;
    const float* in_shift;
    float* partial;                            // [KS][B][O][P]
    int B, I, O, h, w;
};

__global__ __launch_bounds__(kSmallBlock) void conv3x3_small_kernel(SmallArgs p) {
    __shared__ __attribute__((aligned(16))) float sW[kSmallStage * 9 * kSmallOc];
    __shared__ float sX[kSmallStage * kSmallWin];
    const int tid = threadIdx.x, g = tid >> 6, lane = tid & 63;
    const int P = p.h * p.w;
    const int oc0 = blockIdx.x * kSmallOc, ks = blockIdx.y, b = blockIdx.z;
    const int c_lo = ks * kSmallChunk;
    const int c_hi = c_lo + kSmallChunk < p.I ? c_lo + kSmallChunk : p.I;
    const bool live = lane < P;
    const int py = live ? lane / p.w : 0, px = live ? lane - py * p.w : 0;

    float sum[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) sum[j] = 0.f;

    for (int c0 = c_lo; c0 < c_hi; c0 += kSmallStage) {
        const int cn = c_hi - c0 < kSmallStage ? c_hi - c0 : kSmallStage;
        __syncthreads();                                       // the previous block has been consumed
        for (int i = tid; i < cn * kSmallWin; i += kSmallBlock) {
            const int ci = i / kSmallWin, r = (i - ci * kSmallWin) / kSmallPitch, c = i - ci * kSmallWin - r * kSmallPitch;
            const int yy = r - 1, xx = c - 1;
            float v = 0.f;
            if (yy >= 0 && yy < p.h && xx >= 0 && xx < p.w) {
                v = p.x[(((int64_t)b * p.I + (c0 + ci)) * p.h + yy) * p.w + xx];
                if (p.in_scale) v = v * p.in_scale[c0 + ci] + p.in_shift[c0 + ci];
            }
            sX[i] = v;
        }
        for (int i = tid; i < cn * 9 * kSmallOc; i += kSmallBlock) {
            const int j = i & (kSmallOc - 1), rem = i / kSmallOc;      // rem = ci * 9 + tap
            const int ci = rem / 9, tap = rem - ci * 9;
            const int oc = oc0 + j;
            sW[i] = oc < p.O ? p.wk[((int64_t)tap * p.I + (c0 + ci)) * p.O + oc] : 0.f;
        }
        __syncthreads();
        float acc[16];                                         // this block's 72 terms: blocked summation
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.f;
        for (int ci = 0; ci < cn; ++ci) {
            const float* xin = sX + ci * kSmallWin + py * kSmallPitch + px;
            const float* wc = sW + ci * 9 * kSmallOc + g * 16;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float xv = xin[ky * kSmallPitch + kx];
                    const float4* wv = reinterpret_cast<const float4*>(wc + (ky * 3 + kx) * kSmallOc);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 w4 = wv[q];
                        acc[4 * q + 0] = __builtin_fmaf(w4.x, xv, acc[4 * q + 0]);
                        acc[4 * q + 1] = __builtin_fmaf(w4.y, xv, acc[4 * q + 1]);
                        acc[4 * q + 2] = __builtin_fmaf(w4.z, xv, acc[4 * q + 2]);
                        acc[4 * q + 3] = __builtin_fmaf(w4.w, xv, acc[4 * q + 3]);
                    }
                }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) sum[j] += acc[j];
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int oc = oc0 + g * 16 + j;
        if (oc >= p.O) break;
        p.partial[(((int64_t)ks * p.B + b) * p.O + oc) * P + lane] = sum[j];
    }
}

__global__ __launch_bounds__(256) void conv3x3_small_combine_kernel(const float* __restrict__ partial, int KS, const float* __restrict__ scale,
                                                                    const float* __restrict__ shift, const float* __restrict__ slopes,
                                                                    float* __restrict__ y, int O, int P, int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        float v = partial[i];
        for (int k = 1; k < KS; ++k) v += partial[(int64_t)k * total + i];
        const int oc = (int)((i / P) % O);
        if (scale) v = v * scale[oc];
        if (shift) v = v + shift[oc];
        if (slopes) v = v < 0.f ? v * slopes[oc] : v;
        y[i] = v;
    }
}

int small_splits(int I) { return (int)ia::ceil_div(I, kSmallChunk); }

// ------------------------------------------------------------------ output head

constexpr int kHeadBlock = 256;
constexpr int kHeadRows = 4;                   // output rows per workgroup
constexpr int kHeadBatch = 4;                  // images per pass over a weight slice
constexpr int kHeadSlice = 3136;               // K per workgroup (25088 = 8 slices)
constexpr int kFinishBlock = 256;

int head_splits(int K) { return (int)ia::ceil_div(K, kHeadSlice); }

__global__ __launch_bounds__(kHeadBlock) void id_head_kernel(const float* __restrict__ x, const float* __restrict__ wt, float* __restrict__ partial,
                                                             int B, int K, int O) {
    __shared__ float sRed[kHeadBlock / 64][kHeadRows * kHeadBatch];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int o0 = blockIdx.x * kHeadRows, ks = blockIdx.y;
    const int k_lo = ks * kHeadSlice;
    const int k_hi = k_lo + kHeadSlice < K ? k_lo + kHeadSlice : K;
    const float* wrow[kHeadRows];
#pragma unroll
    for (int r = 0; r < kHeadRows; ++r) wrow[r] = wt + (int64_t)(o0 + r < O ? o0 + r : O - 1) * K;     // (clamped rows are not written)
    for (int b0 = 0; b0 < B; b0 += kHeadBatch) {
        const float* xrow[kHeadBatch];
#pragma unroll
        for (int q = 0; q < kHeadBatch; ++q) xrow[q] = x + (int64_t)(b0 + q < B ? b0 + q : B - 1) * K;
        float acc[kHeadRows][kHeadBatch];
#pragma unroll
        for (int r = 0; r < kHeadRows; ++r)
#pragma unroll
            for (int q = 0; q < kHeadBatch; ++q) acc[r][q] = 0.f;
        for (int k = k_lo + tid; k < k_hi; k += kHeadBlock) {
            float wv[kHeadRows], xv[kHeadBatch];
#pragma unroll
            for (int r = 0; r < kHeadRows; ++r) wv[r] = wrow[r][k];
#pragma unroll
            for (int q = 0; q < kHeadBatch; ++q) xv[q] = xrow[q][k];
#pragma unroll
            for (int r = 0; r < kHeadRows; ++r)
#pragma unroll
                for (int q = 0; q < kHeadBatch; ++q) acc[r][q] = __builtin_fmaf(wv[r], xv[q], acc[r][q]);
        }
        __syncthreads();                                       // the previous pass's sRed has been read
#pragma unroll
        for (int r = 0; r < kHeadRows; ++r)
#pragma unroll
            for (int q = 0; q < kHeadBatch; ++q) {
                const float t = wave_sum(acc[r][q]);
                if (lane == 0) sRed[wave][r * kHeadBatch + q] = t;
            }
        __syncthreads();
        if (tid < kHeadRows * kHeadBatch) {
            const int r = tid / kHeadBatch, q = tid - r * kHeadBatch;
            float t = sRed[0][tid];
            for (int w = 1; w < kHeadBlock / 64; ++w) t += sRed[w][tid];
            if (o0 + r < O && b0 + q < B) partial[((int64_t)ks * B + (b0 + q)) * O + (o0 + r)] = t;
        }
    }
}

// One workgroup per image: z = (sum of the slices + bias) * scale + shift, out = z / ||z||.
__global__ __launch_bounds__(kFinishBlock) void id_head_finish_kernel(const float* __restrict__ partial, int KS, const float* __restrict__ bias,
                                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                                      float* __restrict__ out, int B, int O) {
    __shared__ double sRed[kFinishBlock / 64];
    __shared__ float sNorm;
    const int tid = threadIdx.x, b = blockIdx.x;
    double sq = 0.0;
    for (int o = tid; o < O; o += kFinishBlock) {
        float v = partial[(int64_t)b * O + o];
        for (int k = 1; k < KS; ++k) v += partial[((int64_t)k * B + b) * O + o];
        if (bias) v = v + bias[o];
        if (scale) v = v * scale[o];
        if (shift) v = v + shift[o];
        out[(int64_t)b * O + o] = v;
        sq += (double)v * (double)v;
    }
    sq = wave_sum(sq);
    if ((tid & 63) == 0) sRed[tid >> 6] = sq;
    __syncthreads();
    if (tid == 0) {
        double t = sRed[0];
        for (int w = 1; w < kFinishBlock / 64; ++w) t += sRed[w];
        sNorm = (float)sqrt(t);
    }
    __syncthreads();
    const float norm = sNorm;
    for (int o = tid; o < O; o += kFinishBlock) out[(int64_t)b * O + o] = out[(int64_t)b * O + o] / norm;     // (0 / 0 = NaN, as torch.div)
}

// ------------------------------------------------------------------ per-pair dot

__global__ __launch_bounds__(64) void id_similarity_kernel(const float* __restrict__ f, int N, int D, float* __restrict__ out, int out_stride) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const float* a = f + (int64_t)n * D;
    const float* b = f + ((int64_t)N + n) * D;
    double t = 0.0;
    for (int i = lane; i < D; i += 64) t += (double)(a[i] * b[i]);
    t = wave_sum(t);
    if (lane == 0) out[(int64_t)n * out_stride] = (float)t;
}

}  // namespace

extern "C" int ia_face_crop_pool(const void* images, int layout, float* y, int N, int H, int W, void* stream) {
    IA_REQUIRE(images != nullptr && y != nullptr, "ia_face_crop_pool: null device pointers");
    IA_REQUIRE(layout == IA_IMAGE_F32_NCHW || layout == IA_IMAGE_U8_NHWC, "ia_face_crop_pool: layout must be IA_IMAGE_F32_NCHW or IA_IMAGE_U8_NHWC, got %d", layout);
    IA_REQUIRE(N >= 1, "ia_face_crop_pool: empty batch");
    IA_REQUIRE(H >= kFace && W >= kFace && H <= 16384 && W <= 16384, "ia_face_crop_pool: sides must be in 256..16384, got %d x %d", H, W);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ia::streaming_grid((int64_t)N * 3 * kFaceOut * kFaceOut, 256));
    if (layout == IA_IMAGE_U8_NHWC) face_crop_pool_kernel<true><<<grid, 256, 0, s>>>(images, y, N, H, W);
    else face_crop_pool_kernel<false><<<grid, 256, 0, s>>>(images, y, N, H, W);
    return ia::check_launch("ia_face_crop_pool");
}

extern "C" int ia_prelu_channels(const float* x, const float* slopes, float* y, int B, int C, int64_t P, void* stream) {
    IA_REQUIRE(x != nullptr && slopes != nullptr && y != nullptr, "ia_prelu_channels: null device pointers");
    IA_REQUIRE(B >= 1 && C >= 1 && P >= 1, "ia_prelu_channels: empty tensor (B=%d C=%d P=%lld)", B, C, (long long)P);
    const int64_t total = (int64_t)B * C * P;
    prelu_kernel<<<ia::streaming_grid(total, 256), 256, 0, (hipStream_t)stream>>>(x, slopes, y, C, P, total);
    return ia::check_launch("ia_prelu_channels");
}

static int small_checked(int B, int I, int O, int h, int w, const char* what) {
    IA_REQUIRE(B >= 1 && B <= 65535, "%s: the batch must be in 1..65535, got %d", what, B);
    IA_REQUIRE(I >= 8 && O >= 8 && I % 8 == 0 && O % 8 == 0, "%s: I and O must be positive multiples of 8, got I=%d O=%d", what, I, O);
    IA_REQUIRE(h >= 1 && w >= 1 && h < 8 && w < 8, "%s: the map's sides must be in 1..7, got %d x %d", what, h, w);
    IA_REQUIRE(ia::ceil_div(O, kSmallOc) <= 65535 && small_splits(I) <= 65535, "%s: too many channels (I=%d O=%d)", what, I, O);
    return IA_OK;
}

extern "C" int ia_conv3x3_small_scratch_bytes(int B, int I, int O, int h, int w, size_t* h_bytes) {
    IA_REQUIRE(h_bytes != nullptr, "ia_conv3x3_small_scratch_bytes: null output pointer");
    const int e = small_checked(B, I, O, h, w, "ia_conv3x3_small_scratch_bytes");
    if (e != IA_OK) return e;
    *h_bytes = (size_t)small_splits(I) * (size_t)B * (size_t)O * (size_t)(h * w) * sizeof(float);
    return IA_OK;
}

extern "C" int ia_conv3x3_small(const float* x, const float* wk, const float* in_scale, const float* in_shift, const float* out_scale,
                                const float* out_shift, const float* slopes, float* y, void* scratch, size_t scratch_bytes, int B, int I, int O,
                                int h, int w, void* stream) {
    IA_REQUIRE(x != nullptr && wk != nullptr && y != nullptr && scratch != nullptr, "ia_conv3x3_small: null device pointers");
    IA_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "ia_conv3x3_small: in_scale and in_shift come together");
    const int e = small_checked(B, I, O, h, w, "ia_conv3x3_small");
    if (e != IA_OK) return e;
    const int KS = small_splits(I), P = h * w;
    const size_t need = (size_t)KS * (size_t)B * (size_t)O * (size_t)P * sizeof(float);
    IA_REQUIRE(scratch_bytes >= need, "ia_conv3x3_small: scratch too small: %zu bytes given, %zu needed", scratch_bytes, need);
    IA_REQUIRE(((uintptr_t)scratch & 3) == 0, "ia_conv3x3_small: scratch must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    SmallArgs a{x, wk, in_scale, in_shift, static_cast<float*>(scratch), B, I, O, h, w};
    conv3x3_small_kernel<<<dim3((unsigned)ia::ceil_div(O, kSmallOc), (unsigned)KS, (unsigned)B), kSmallBlock, 0, s>>>(a);
    const int e1 = ia::check_launch("ia_conv3x3_small (products)");
    if (e1 != IA_OK) return e1;
    const int64_t total = (int64_t)B * O * P;
    conv3x3_small_combine_kernel<<<ia::streaming_grid(total, 256), 256, 0, s>>>(static_cast<const float*>(scratch), KS, out_scale, out_shift, slopes, y,
                                                                                O, P, total);
    return ia::check_launch("ia_conv3x3_small (combine)");
}

static int head_checked(int B, int K, int O, const char* what) {
    IA_REQUIRE(B >= 1 && K >= 1 && O >= 1, "%s: B, K, O must be positive, got B=%d K=%d O=%d", what, B, K, O);
    IA_REQUIRE(B <= (1 << 20) && O <= (1 << 18) && head_splits(K) <= 65535, "%s: too large (B=%d K=%d O=%d)", what, B, K, O);
    return IA_OK;
}

extern "C" int ia_id_head_scratch_bytes(int B, int K, int O, size_t* h_bytes) {
    IA_REQUIRE(h_bytes != nullptr, "ia_id_head_scratch_bytes: null output pointer");
    const int e = head_checked(B, K, O, "ia_id_head_scratch_bytes");
    if (e != IA_OK) return e;
    *h_bytes = (size_t)head_splits(K) * (size_t)B * (size_t)O * sizeof(float);
    return IA_OK;
}

extern "C" int ia_id_head(const float* x, const float* wt, const float* bias, const float* scale, const float* shift, float* out, void* scratch,
                          size_t scratch_bytes, int B, int K, int O, void* stream) {
    IA_REQUIRE(x != nullptr && wt != nullptr && out != nullptr && scratch != nullptr, "ia_id_head: null device pointers");
    const int e = head_checked(B, K, O, "ia_id_head");
    if (e != IA_OK) return e;
    const int KS = head_splits(K);
    const size_t need = (size_t)KS * (size_t)B * (size_t)O * sizeof(float);
    IA_REQUIRE(scratch_bytes >= need, "ia_id_head: scratch too small: %zu bytes given, %zu needed", scratch_bytes, need);
    IA_REQUIRE(((uintptr_t)scratch & 3) == 0, "ia_id_head: scratch must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    id_head_kernel<<<dim3((unsigned)ia::ceil_div(O, kHeadRows), (unsigned)KS), kHeadBlock, 0, s>>>(x, wt, static_cast<float*>(scratch), B, K, O);
    const int e1 = ia::check_launch("ia_id_head (products)");
    if (e1 != IA_OK) return e1;
    id_head_finish_kernel<<<(unsigned)B, kFinishBlock, 0, s>>>(static_cast<const float*>(scratch), KS, bias, scale, shift, out, B, O);
    return ia::check_launch("ia_id_head (finish)");
}

extern "C" int ia_id_similarity(const float* f, int N, int D, float* out, int out_stride, void* stream) {
    IA_REQUIRE(f != nullptr && out != nullptr, "ia_id_similarity: null device pointers");
    IA_REQUIRE(N >= 1 && D >= 1, "ia_id_similarity: N and D must be positive, got N=%d D=%d", N, D);
    IA_REQUIRE(out_stride >= 1, "ia_id_similarity: out_stride must be positive, got %d", out_stride);
    id_similarity_kernel<<<(unsigned)N, 64, 0, (hipStream_t)stream>>>(f, N, D, out, out_stride);
    return ia::check_launch("ia_id_similarity");
}
