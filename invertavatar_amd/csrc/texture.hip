// Texture atlas of a triangle mesh: surface points per texel, projective texturing from rendered views, and the lookup.  No counterpart
// in the reference; geometry.py (TextureAtlas, _atlas_points_numpy, _texture_project_numpy, _texture_sample_numpy) restates every line
// in NumPy and is the definition.
//
//   layout  : the texture is size x size texels, texel (i, j) = column i, row j, stored [j][i].  Faces 2b and 2b + 1 share the square
//             block b of side s at ((b % G) s, (b / G) s), G = size / s, L = s - 3.  With (li, lj) the position inside the block, the
//             lower face 2b owns li + lj <= s - 1 (corners at (0, 0), (L, 0), (0, L); a = li, c = lj) and the upper face 2b + 1 owns
//             li + lj >= s (corners at (s-1, s-1), (2, s-1), (s-1, 2); a = s - 1 - li, c = s - 1 - lj).  A texel outside the G s
//             square or of a face >= F is unowned (face -1, every output 0).
//   points  : lambda_1 = (float)a / (float)L, lambda_2 = (float)c / (float)L, lambda_0 = (1 - lambda_1) - lambda_2 (negative on the
//             guard texels: extrapolation on the plane); point = (lambda_0 A + lambda_1 B) + lambda_2 C per coordinate; the normal is
//             the unit (B - A) x (C - A), or the normalised mix of the vertex normals, and 0 for a face whose cross product has no
//             finite positive length (counted once per face in *degenerate).
//   project : per texel and view k in ascending order, in fp32 with every operation rounded on its own: the projection of
//             mesh_raster.hip without the snap (u, v, z); skipped if unusable there or u outside [0, W - 1] or v outside [0, H - 1];
//             e = o - X, t = sqrt(e . e), c = (n . e) / t, skipped unless c > min_cos; at pixel (rint u, rint v) skipped unless mask
//             is set and |t - depth| <= depth_tol; colour = bilinear read at (u, v) (i0 = floor u, fx = u - i0, i1 = min(i0 + 1,
//             W - 1); (1 - fy) ((1 - fx) I00 + fx I10) + fy ((1 - fx) I01 + fx I11)); w = c^power (an integer power is the
//             product ((c c) c) ..., any other the fp32 rounding of the double pow).  blend: double sums of the fp32 terms w colour
//             and of w, texture = (float)(sum / sum w); best: the colour of the largest w, the lowest k among equals.
//   sample  : per pixel the uv mix (b0 u0 + b1 u1) + b2 u2 of the face's atlas corners ((x + 0.5) / size), x = u size - 0.5, clamped
//             into the face's block, and the bilinear read of the four texels (all inside the block).
//
// One thread per texel or pixel, no atomics on floating-point data, plain vector stores.  The build has -ffp-contract=off.
#include "geom_common.h"

#include <cmath>

namespace {

using ia::on_device;

constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = 4;               // atlas_points: a wave writes 64 consecutive texels of one row
constexpr int64_t kMaxCount = (int64_t)1 << 28;
constexpr int kMaxSide = 1 << 14;
constexpr int kMaxViews = 256;                       // cameras staged in LDS: 72 bytes each
constexpr int kMaxChannels = 8;                      // projection: double accumulators in registers
constexpr int kMaxSampleChannels = 64;
constexpr float kMaxScreen = 1048576.f;

using F3 = ia::Vec3<float>;
__device__ __forceinline__ F3 load3(const float* __restrict__ v, int64_t i) { return {v[3 * i], v[3 * i + 1], v[3 * i + 2]}; }
__device__ __forceinline__ void store3(float* __restrict__ out, int64_t i, F3 v) { out[3 * i] = v.x; out[3 * i + 1] = v.y; out[3 * i + 2] = v.z; }
__device__ __forceinline__ F3 mix3(float b0, F3 a, float b1, F3 b, float b2, F3 c) {
    return {(b0 * a.x + b1 * b.x) + b2 * c.x, (b0 * a.y + b1 * b.y) + b2 * c.y, (b0 * a.z + b1 * b.z) + b2 * c.z};
}
__device__ __forceinline__ F3 unit_or_zero(F3 v) {
    const float l = sqrtf(dot(v, v));
    const bool ok = l > 0.f && isfinite(l);
    return {ok ? v.x / l : 0.f, ok ? v.y / l : 0.f, ok ? v.z / l : 0.f};
}

// ------------------------------------------------------------------ atlas points

struct AtlasArgs {
    const float* verts;
    int64_t V;
    const int* faces;
    int64_t F;
    int size, s, G;
    const float* normals;        // [V,3] or null: face normals
    float* point;                // [size,size,3]
    int* face;                   // [size,size]
    float* bary;                 // [size,size,3]
    float* normal;               // [size,size,3]
    int* degenerate;
};

__global__ __launch_bounds__(kBlock) void atlas_points_kernel(AtlasArgs u) {
    const int i = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
    const int j = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    const bool in_texture = i < u.size && j < u.size;
    int64_t f = -1;
    int a = 0, c = 0;
    bool first = false;                                                  // the one texel of a face that reports it degenerate
    if (in_texture && i < u.G * u.s && j < u.G * u.s) {
        const int bi = i / u.s, bj = j / u.s, li = i - bi * u.s, lj = j - bj * u.s;
        const bool upper = li + lj >= u.s;
        f = 2 * ((int64_t)bj * u.G + bi) + (upper ? 1 : 0);
        a = upper ? u.s - 1 - li : li;
        c = upper ? u.s - 1 - lj : lj;
        first = a == 0 && c == 0;
        if (f >= u.F) f = -1;
    }
    const bool owned = f >= 0;
    F3 X{0.f, 0.f, 0.f}, nrm{0.f, 0.f, 0.f};
    float b[3] = {0.f, 0.f, 0.f};
    bool degenerate = false;
    if (owned) {
        int64_t idx[3];
        bool valid = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t v = u.faces[3 * f + k];
            valid = valid && (uint64_t)v < (uint64_t)u.V;
            idx[k] = (uint64_t)v < (uint64_t)u.V ? v : 0;
        }
        const F3 A = load3(u.verts, idx[0]), B = load3(u.verts, idx[1]), C = load3(u.verts, idx[2]);
        const float L = (float)(u.s - 3);
        b[1] = (float)a / L;
        b[2] = (float)c / L;
        b[0] = (1.f - b[1]) - b[2];
        X = mix3(b[0], A, b[1], B, b[2], C);
        const F3 fn = cross(sub(B, A), sub(C, A));
        const float l = sqrtf(dot(fn, fn));
        degenerate = !(valid && l > 0.f && isfinite(l));
        if (!degenerate) {
            nrm = fn;
            if (u.normals) nrm = mix3(b[0], load3(u.normals, idx[0]), b[1], load3(u.normals, idx[1]), b[2], load3(u.normals, idx[2]));
            nrm = unit_or_zero(nrm);
        }
    }
    if (in_texture) {
        const int64_t p = (int64_t)j * u.size + i;
        u.face[p] = (int)f;
        store3(u.point, p, X);
        store3(u.bary, p, F3{b[0], b[1], b[2]});
        store3(u.normal, p, nrm);
    }
    ia::wave_count(owned && first && degenerate, u.degenerate);
}

// ------------------------------------------------------------------ projection

struct Camera {
    float r[9];                  // rotation, row-major
    float o[3];
    float k[6];                  // rows 0 and 1 of K_res
};

struct ProjectArgs {
    const float* point;          // [T,3]
    const float* normal;         // [T,3]
    const int* face;             // [T]
    int64_t T;
    const float* images;         // [N,H,W,C]
    const float* cams;           // [N,25]
    int N, H, W, C;
    const float* depth;          // [N,H,W]
    const unsigned char* mask;   // [N,H,W]
    float near, min_cos, depth_tol;
    int ipow;                    // the power where it is an integer in [0, 64], else -1
    double power;
    int best;
    const float* fallback;       // [T,C] or null
    float* texture;              // [T,C]
    float* weight;               // [T]
    int* views;                  // [T]
    unsigned char* filled;       // [T]
};

__device__ __forceinline__ float view_weight(float c, int ipow, double power) {
    if (ipow < 0) return (float)pow((double)c, power);
    float w = 1.f;
    for (int k = 0; k < ipow; ++k) w = w * c;
    return w;
}

__global__ __launch_bounds__(kBlock) void texture_project_kernel(ProjectArgs u) {
    extern __shared__ Camera cams[];
    for (int n = threadIdx.x; n < u.N; n += kBlock) {
        const float* __restrict__ cam = u.cams + 25 * (int64_t)n;
        Camera c;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) c.r[3 * a + b] = cam[4 * a + b];
            c.o[a] = cam[4 * a + 3];
            c.k[a] = cam[16 + a] * (float)u.W;
            c.k[3 + a] = cam[19 + a] * (float)u.H;
        }
        cams[n] = c;
    }
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= u.T) return;
    double num[kMaxChannels], den = 0.0;
    float col_best[kMaxChannels], w_best = 0.f;
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ++ch) { num[ch] = 0.0; col_best[ch] = 0.f; }
    int passed = 0;
    if (u.face[p] >= 0) {
        const F3 X = load3(u.point, p), nr = load3(u.normal, p);
        const int64_t hw = (int64_t)u.H * u.W;
        for (int n = 0; n < u.N; ++n) {
            const Camera& c = cams[n];
            const F3 o{c.o[0], c.o[1], c.o[2]};
            const F3 d = sub(X, o);
            const float xx = (c.r[0] * d.x + c.r[3] * d.y) + c.r[6] * d.z;
            const float xy = (c.r[1] * d.x + c.r[4] * d.y) + c.r[7] * d.z;
            const float z = (c.r[2] * d.x + c.r[5] * d.y) + c.r[8] * d.z;
            const float px = (c.k[0] * xx + c.k[1] * xy) + c.k[2] * z;
            const float py = (c.k[3] * xx + c.k[4] * xy) + c.k[5] * z;
            const float uu = px / z, vv = py / z;
            const bool usable = isfinite(uu) && isfinite(vv) && isfinite(z) && !(z <= u.near) && fabsf(uu) < kMaxScreen && fabsf(vv) < kMaxScreen;
            if (!usable || !(uu >= 0.f && uu <= (float)(u.W - 1)) || !(vv >= 0.f && vv <= (float)(u.H - 1))) continue;
            const F3 e = sub(o, X);
            const float t = sqrtf(dot(e, e));
            const float cosv = dot(nr, e) / t;
            if (!(cosv > u.min_cos)) continue;
            const int pi = (int)rintf(uu), pj = (int)rintf(vv);                 // in [0, W - 1] x [0, H - 1] by the test above
            const int64_t q = (int64_t)n * hw + (int64_t)pj * u.W + pi;
            if (!u.mask[q] || !(fabsf(t - u.depth[q]) <= u.depth_tol)) continue;
            const float fi = floorf(uu), fj = floorf(vv);
            const float fx = uu - fi, fy = vv - fj;
            const int i0 = (int)fi, j0 = (int)fj, i1 = min(i0 + 1, u.W - 1), j1 = min(j0 + 1, u.H - 1);
            const float* __restrict__ img = u.images + (int64_t)n * hw * u.C;
            const int64_t q00 = ((int64_t)j0 * u.W + i0) * u.C, q10 = ((int64_t)j0 * u.W + i1) * u.C;
            const int64_t q01 = ((int64_t)j1 * u.W + i0) * u.C, q11 = ((int64_t)j1 * u.W + i1) * u.C;
            const float w = view_weight(cosv, u.ipow, u.power);
            const bool better = passed == 0 || w > w_best;
#pragma unroll
            for (int ch = 0; ch < kMaxChannels; ++ch) {
                if (ch < u.C) {
                    const float top = (1.f - fx) * img[q00 + ch] + fx * img[q10 + ch];
                    const float bot = (1.f - fx) * img[q01 + ch] + fx * img[q11 + ch];
                    const float col = (1.f - fy) * top + fy * bot;
                    num[ch] += (double)(w * col);
                    if (better) col_best[ch] = col;
                }
            }
            den += (double)w;
            if (better) w_best = w;
            ++passed;
        }
    }
    u.views[p] = passed;
    u.filled[p] = passed > 0 ? 1 : 0;
    u.weight[p] = passed == 0 ? 0.f : (u.best ? w_best : (float)den);
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ++ch) {
        if (ch < u.C) {
            float out = u.fallback ? u.fallback[p * u.C + ch] : 0.f;
            if (passed > 0) out = u.best ? col_best[ch] : (float)(num[ch] / den);
            u.texture[p * u.C + ch] = out;
        }
    }
}

// ------------------------------------------------------------------ lookup

struct SampleArgs {
    const float* texture;        // [size,size,C]
    int size, s, G, C;
    int64_t F;
    const int* face;             // [P]
    const float* bary;           // [P,3]
    int64_t P;
    float* out;                  // [P,C]
};

__global__ __launch_bounds__(kBlock) void texture_sample_kernel(SampleArgs u) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= u.P) return;
    const int64_t f = u.face[p];
    if (f < 0 || f >= u.F || (f >> 1) >= (int64_t)u.G * u.G) {
        for (int ch = 0; ch < u.C; ++ch) u.out[p * u.C + ch] = 0.f;
        return;
    }
    const int64_t blk = f >> 1;
    const int bx = (int)(blk % u.G) * u.s, by = (int)(blk / u.G) * u.s;
    const bool upper = f & 1;
    const int L = u.s - 3, far = u.s - 1;
    // corners in texels, then as uv = (x + 0.5) / size
    const int cx[3] = {bx + (upper ? far : 0), bx + (upper ? 2 : L), bx + (upper ? far : 0)};
    const int cy[3] = {by + (upper ? far : 0), by + (upper ? far : 0), by + (upper ? 2 : L)};
    const float size = (float)u.size;
    float cu[3], cv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { cu[k] = ((float)cx[k] + 0.5f) / size; cv[k] = ((float)cy[k] + 0.5f) / size; }
    const float b0 = u.bary[3 * p], b1 = u.bary[3 * p + 1], b2 = u.bary[3 * p + 2];
    const float uu = (b0 * cu[0] + b1 * cu[1]) + b2 * cu[2], vv = (b0 * cv[0] + b1 * cv[1]) + b2 * cv[2];
    const float x = uu * size - 0.5f, y = vv * size - 0.5f;
    const float xl = fminf(fmaxf(x - (float)bx, 0.f), (float)far), yl = fminf(fmaxf(y - (float)by, 0.f), (float)far);
    const float fi = floorf(xl), fj = floorf(yl);
    const float fx = xl - fi, fy = yl - fj;
    const int i0 = (int)fi, j0 = (int)fj, i1 = min(i0 + 1, far), j1 = min(j0 + 1, far);
    const int64_t q00 = ((int64_t)(by + j0) * u.size + bx + i0) * u.C, q10 = ((int64_t)(by + j0) * u.size + bx + i1) * u.C;
    const int64_t q01 = ((int64_t)(by + j1) * u.size + bx + i0) * u.C, q11 = ((int64_t)(by + j1) * u.size + bx + i1) * u.C;
    for (int ch = 0; ch < u.C; ++ch) {
        const float top = (1.f - fx) * u.texture[q00 + ch] + fx * u.texture[q10 + ch];
        const float bot = (1.f - fx) * u.texture[q01 + ch] + fx * u.texture[q11 + ch];
        u.out[p * u.C + ch] = (1.f - fy) * top + fy * bot;
    }
}

// ------------------------------------------------------------------ host side

int check_atlas(const char* what, int size, int s, int64_t F) {
    if (size < 4 || size > kMaxSide || s < 4 || s > size)
        return ia::fail(IA_ERR_INVALID_ARG, "%s: 4 <= s <= size <= 16384, got size = %d, s = %d", what, size, s);
    if (F < 0 || F > kMaxCount) return ia::fail(IA_ERR_INVALID_ARG, "%s: F must be in [0, 2^28], got %lld", what, (long long)F);
    const int64_t G = size / s;
    if (2 * G * G < F) return ia::fail(IA_ERR_INVALID_ARG, "%s: %lld blocks of side %d hold fewer than %lld faces", what, (long long)(G * G), s, (long long)F);
    return IA_OK;
}

}  // namespace

extern "C" int ia_atlas_points(const float* verts, int64_t V, const int* faces, int64_t F, int size, int s, const float* normals, float* point,
                               int* face, float* bary, float* normal, int* degenerate, void* stream) {
    if (int st = check_atlas("ia_atlas_points", size, s, F)) return st;
    IA_REQUIRE(V >= 0 && V <= kMaxCount, "ia_atlas_points: V must be in [0, 2^28], got %lld", (long long)V);
    IA_REQUIRE(F == 0 || V > 0, "ia_atlas_points: faces without vertices");
    if (!on_device(point) || !on_device(face) || !on_device(bary) || !on_device(normal) || !on_device(degenerate) ||
        (F && (!on_device(verts) || !on_device(faces))) || (normals && V && !on_device(normals)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_atlas_points: every array must be a device pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(degenerate, 0, sizeof(int), st) != hipSuccess) return ia::check_launch("ia_atlas_points (clear)");
    AtlasArgs u{verts, V, faces, F, size, s, size / s, normals, point, face, bary, normal, degenerate};
    const dim3 grid((unsigned)ia::ceil_div(size, kTileW), (unsigned)ia::ceil_div(size, kTileH));
    atlas_points_kernel<<<grid, kBlock, 0, st>>>(u);
    return ia::check_launch("ia_atlas_points");
}

extern "C" int ia_texture_project(const float* point, const float* normal, const int* face, int64_t T, const float* images, const float* cams, int N,
                                  int H, int W, int C, const float* depth, const unsigned char* mask, float near, float min_cos, double power,
                                  float depth_tol, int best, const float* fallback, float* texture, float* weight, int* views,
                                  unsigned char* filled, void* stream) {
    IA_REQUIRE(T >= 0 && T <= kMaxCount, "ia_texture_project: T must be in [0, 2^28], got %lld", (long long)T);
    IA_REQUIRE(N >= 1 && N <= kMaxViews && H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide && (int64_t)N * H * W < ((int64_t)1 << 31),
               "ia_texture_project: 1 <= N <= %d views of 1 .. 16384 pixels per side, N H W below 2^31, got N = %d, H = %d, W = %d", kMaxViews, N, H, W);
    IA_REQUIRE(C >= 1 && C <= kMaxChannels, "ia_texture_project: 1 .. %d image channels, got %d", kMaxChannels, C);
    IA_REQUIRE(near >= 0.f && power >= 0.0 && depth_tol >= 0.f, "ia_texture_project: near, power and depth_tol must be >= 0, got %g, %g, %g",
               (double)near, power, (double)depth_tol);
    if (T == 0) return IA_OK;
    if (!on_device(point) || !on_device(normal) || !on_device(face) || !on_device(images) || !on_device(cams) || !on_device(depth) ||
        !on_device(mask) || !on_device(texture) || !on_device(weight) || !on_device(views) || !on_device(filled) || (fallback && !on_device(fallback)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_texture_project: every array must be a device pointer");
    const bool integer = power <= 64.0 && power == std::floor(power);
    ProjectArgs u{point, normal, face, T, images, cams, N, H, W, C, depth, mask, near, min_cos, depth_tol, integer ? (int)power : -1, power,
                  best ? 1 : 0, fallback, texture, weight, views, filled};
    texture_project_kernel<<<ia::blocks(T, kBlock), kBlock, sizeof(Camera) * (size_t)N, (hipStream_t)stream>>>(u);
    return ia::check_launch("ia_texture_project");
}

extern "C" int ia_texture_sample(const float* texture, int size, int C, int s, int64_t F, const int* face, const float* bary, int64_t P, float* out,
                                 void* stream) {
    if (int st = check_atlas("ia_texture_sample", size, s, F)) return st;
    IA_REQUIRE(C >= 1 && C <= kMaxSampleChannels, "ia_texture_sample: 1 .. %d channels, got %d", kMaxSampleChannels, C);
    IA_REQUIRE(P >= 0 && P < ((int64_t)1 << 31), "ia_texture_sample: P must be in [0, 2^31), got %lld", (long long)P);
    if (P == 0) return IA_OK;
    if (!on_device(texture) || !on_device(face) || !on_device(bary) || !on_device(out))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_texture_sample: every array must be a device pointer");
    SampleArgs u{texture, size, s, size / s, C, F, face, bary, P, out};
    texture_sample_kernel<<<ia::blocks(P, kBlock), kBlock, 0, (hipStream_t)stream>>>(u);
    return ia::check_launch("ia_texture_sample");
}
