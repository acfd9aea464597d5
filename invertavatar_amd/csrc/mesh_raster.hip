// Z-buffer rasteriser for indexed triangle meshes: per view a visibility buffer (nearest face per pixel) and, resolved from it, mask,
// face, perspective-correct barycentrics, depth, normals and interpolated vertex attributes.  No counterpart in the reference;
// geometry.py (_project_numpy, _raster_faces_numpy, _resolve_numpy) restates every line in NumPy and is the definition.
//
//   project : one thread per (view, vertex).  Camera = the 25-float label (cam2world 4x4 row-major, K 3x3 normalised, last row [0,0,1]).
//             K_res = K with row 0 scaled by W and row 1 by H (fp32 products).  In fp32, every operation rounded on its own:
//               d = X - o;  xc_a = (R_0a d_x + R_1a d_y) + R_2a d_z  (a = 0, 1, 2: R^T d);
//               p_x = (k0 xc_x + k1 xc_y) + k2 xc_z;  p_y = (k3 xc_x + k4 xc_y) + k5 xc_z;  u = p_x / xc_z;  v = p_y / xc_z;  z = xc_z.
//             Pixel centres are at integer (u, v): column i, row j is (i, j).  U = (int)rintf(u * 256), V likewise (8 sub-pixel bits).
//             Unusable: u, v or z not finite, z <= near, |u| or |v| >= 2^20.  Stored as int4 {U, V, bits(z), usable}.
//   raster  : one thread per (view, face).  A triangle with an unusable vertex is culled and counted; zero snapped area is culled; no
//             near-plane clipping.  Coverage: 64-bit integer edge functions on the snapped coordinates at (256 i, 256 j), oriented by
//             the sign of the area so that inside is >= 0, with the top-left rule for a centre on an edge (the centre is judged as if
//             moved right by an infinitesimal and down by a smaller one).  Per covered pixel lambda_k = E_k / (E_0 + E_1 + E_2) and
//             z = 1 / ((lambda_0 / z_0 + lambda_1 / z_1) + lambda_2 / z_2); the key bits(z) << 32 | face goes to a 64-bit atomicMin
//             (z >= 0: the bit pattern is monotone; equal depths resolve to the lower face).  The loop runs over the bounding box
//             clamped to the viewport.  A triangle whose clamped box holds more than oversize_pixels pixels is left to the wave path:
//             the small-path launch counts them per workgroup (wave_count), one workgroup scans the counts, a second launch writes the
//             list and one wave per listed triangle strides its lanes over the box.  atomicMin does not care who wrote what first, so
//             both paths and every launch shape give the same buffer.
//   resolve : one thread per pixel: the face from the key, its edge values from the same tri_setup / edge_values as the raster stage,
//             bary_k = (lambda_k / z_k) z, depth = z sqrt((dx dx + dy dy) + 1) with (dx, dy, 1) = K_res^-1 (i, j, 1) in closed form
//             (x' = i - k2, y' = j - k5, det = k0 k4 - k1 k3, dx = (k4 x' - k1 y') / det, dy = (k0 y' - k3 x') / det), the unit normal
//             of the winding (B - A) x (C - A) or the normalised barycentric mix of the vertex normals, and the mix of up to 8 attribute
//             channels ((b_0 a_0 + b_1 a_1) + b_2 a_2).
//
// Every loop is bounded by the viewport.  Plain IEEE fp32 (+ - * / sqrt), no fast-math intrinsics; the build has -ffp-contract=off.
#include "geom_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

using ia::kScanBlock; using ia::on_device; using ia::wave_count;

constexpr int kBlock = 256;
constexpr int64_t kMaxCount = (int64_t)1 << 28;      // vertices and faces
constexpr int kMaxSide = 1 << 14;                    // pixels per viewport side: 256 * side stays far inside the 2^28 of a snapped coordinate
constexpr int kMaxViews = 65535;                     // grid.y
constexpr int kMaxChannels = 8;
constexpr float kMaxScreen = 1048576.f;              // 2^20: |U| <= 2^28, an edge function is below 2^60
constexpr unsigned long long kMiss = ~0ull;

using F3 = ia::Vec3<float>;                          // sub, dot ((x + y) + z), cross: geom_common.h
__device__ __forceinline__ F3 load3(const float* __restrict__ v, int64_t i) { return {v[3 * i], v[3 * i + 1], v[3 * i + 2]}; }

// ------------------------------------------------------------------ project

struct Camera {
    float r[9];                  // rotation, row-major
    float o[3];
    float k[6];                  // rows 0 and 1 of K_res
};

__device__ __forceinline__ Camera load_camera(const float* __restrict__ cam, int H, int W) {
    Camera c;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) c.r[3 * a + b] = cam[4 * a + b];
        c.o[a] = cam[4 * a + 3];
        c.k[a] = cam[16 + a] * (float)W;
        c.k[3 + a] = cam[19 + a] * (float)H;
    }
    return c;
}

__global__ __launch_bounds__(kBlock) void project_kernel(const float* __restrict__ verts, int64_t V, const float* __restrict__ cams, int H, int W,
                                                         float near, int4* __restrict__ proj) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int n = blockIdx.y;
    if (v >= V) return;
    const Camera c = load_camera(cams + 25 * (int64_t)n, H, W);
    const F3 d = sub(load3(verts, v), F3{c.o[0], c.o[1], c.o[2]});
    const float xx = (c.r[0] * d.x + c.r[3] * d.y) + c.r[6] * d.z;
    const float xy = (c.r[1] * d.x + c.r[4] * d.y) + c.r[7] * d.z;
    const float z = (c.r[2] * d.x + c.r[5] * d.y) + c.r[8] * d.z;
    const float px = (c.k[0] * xx + c.k[1] * xy) + c.k[2] * z;
    const float py = (c.k[3] * xx + c.k[4] * xy) + c.k[5] * z;
    const float u = px / z, w = py / z;
    const bool usable = isfinite(u) && isfinite(w) && isfinite(z) && !(z <= near) && fabsf(u) < kMaxScreen && fabsf(w) < kMaxScreen;
    int4 out{0, 0, 0, 0};
    if (usable) out = int4{(int)rintf(u * 256.f), (int)rintf(w * 256.f), __float_as_int(z), 1};
    proj[(int64_t)n * V + v] = out;
}

// ------------------------------------------------------------------ one triangle of one view

struct Tri {
    int64_t U[3], V[3];
    float z[3];
    int64_t s;                   // sign of the snapped area: the edge values are multiplied by it
    bool unusable;               // a vertex index outside [0, V) or an unusable vertex
    bool draw;
    int x0, x1, y0, y1;          // bounding box clamped to the viewport, inclusive (x1 < x0 or y1 < y0: empty)
};

__device__ __forceinline__ Tri tri_setup(const int4* __restrict__ proj, int64_t V, const int* __restrict__ faces, int64_t f, int H, int W, int cull) {
    Tri t;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t i = faces[3 * f + k];
        int4 p{0, 0, 0, 0};
        if ((uint64_t)i < (uint64_t)V) p = proj[i];
        ok = ok && p.w != 0;
        t.U[k] = p.x; t.V[k] = p.y; t.z[k] = __int_as_float(p.z);
    }
    t.unusable = !ok;
    const int64_t area = (t.U[1] - t.U[0]) * (t.V[2] - t.V[0]) - (t.V[1] - t.V[0]) * (t.U[2] - t.U[0]);
    t.s = area > 0 ? 1 : (area < 0 ? -1 : 0);
    t.draw = ok && area != 0 && (!cull || area < 0);
    const int64_t xmin = min(t.U[0], min(t.U[1], t.U[2])), xmax = max(t.U[0], max(t.U[1], t.U[2]));
    const int64_t ymin = min(t.V[0], min(t.V[1], t.V[2])), ymax = max(t.V[0], max(t.V[1], t.V[2]));
    t.x0 = (int)max((xmin + 255) >> 8, (int64_t)0); t.x1 = (int)min(xmax >> 8, (int64_t)W - 1);
    t.y0 = (int)max((ymin + 255) >> 8, (int64_t)0); t.y1 = (int)min(ymax >> 8, (int64_t)H - 1);
    return t;
}

__device__ __forceinline__ int64_t box_pixels(const Tri& t) {
    return t.draw && t.x1 >= t.x0 && t.y1 >= t.y0 ? (int64_t)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) : 0;
}

// Edge values of pixel (i, j): e[k] belongs to vertex k (the edge from vertex k + 1 to vertex k + 2), >= 0 inside; their sum is the
// absolute snapped area.  Returns whether the pixel is covered under the top-left rule.
__device__ __forceinline__ bool edge_values(const Tri& t, int i, int j, int64_t e[3]) {
    const int64_t X = (int64_t)i << 8, Y = (int64_t)j << 8;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        e[k] = t.s * ((t.U[a] - X) * (t.V[b] - Y) - (t.V[a] - Y) * (t.U[b] - X));
        const int64_t A = -t.s * (t.V[b] - t.V[a]), B = t.s * (t.U[b] - t.U[a]);
        in = in && (e[k] > 0 || (e[k] == 0 && (A > 0 || (A == 0 && B > 0))));
    }
    return in;
}

__device__ __forceinline__ void weights(const int64_t e[3], float lam[3]) {
    const float area = (float)((e[0] + e[1]) + e[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) lam[k] = (float)e[k] / area;
}

__device__ __forceinline__ float pixel_depth(const Tri& t, const float lam[3]) {
    return 1.f / ((lam[0] / t.z[0] + lam[1] / t.z[1]) + lam[2] / t.z[2]);
}

__device__ __forceinline__ void draw_pixel(const Tri& t, int64_t f, int i, int j, unsigned long long* __restrict__ vis_n, int W) {
    int64_t e[3];
    if (!edge_values(t, i, j, e)) return;
    float lam[3];
    weights(e, lam);
    const float z = pixel_depth(t, lam);
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(uint32_t)f;
    atomicMin(vis_n + ((int64_t)j * W + i), key);
}

// ------------------------------------------------------------------ raster

struct RasterArgs {
    const int4* proj;            // [N, V]
    int64_t V;
    const int* faces;
    int64_t F;
    int H, W, cull;
    int64_t oversize;            // a clamped box of more pixels goes to the wave path
    unsigned long long* vis;     // [N, H, W]
    int* culled;                 // [N]
    int* blockcount;             // [grid.x * N + 1] oversize triangles per workgroup, then their exclusive scan and the total; or null
    int* list;                   // [N * F] view * F + face of the oversize triangles
};

__global__ __launch_bounds__(kBlock) void raster_small_kernel(RasterArgs u) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int n = blockIdx.y;
    bool unusable = false, over = false;
    if (f < u.F) {
        const Tri t = tri_setup(u.proj + (int64_t)n * u.V, u.V, u.faces, f, u.H, u.W, u.cull);
        unusable = t.unusable;
        const int64_t px = box_pixels(t);
        over = px > u.oversize;
        if (px > 0 && !over) {
            unsigned long long* vis_n = u.vis + (int64_t)n * u.H * u.W;
            for (int j = t.y0; j <= t.y1; ++j)
                for (int i = t.x0; i <= t.x1; ++i) draw_pixel(t, f, i, j, vis_n, u.W);
        }
    }
    wave_count(unusable, u.culled + n);
    if (u.blockcount) wave_count(over, u.blockcount + ((int64_t)n * gridDim.x + blockIdx.x));
}

// One workgroup: out[0 .. n) = exclusive sums of in[0 .. n), out[n] = total.  in == out is allowed.
__global__ __launch_bounds__(kScanBlock) void scan_kernel(const int* in, int* out, int64_t n) {
    const int total = ia::scan_workgroup<int>(in, out, n);
    if (threadIdx.x == 0) out[n] = total;
}

__global__ __launch_bounds__(kBlock) void raster_list_kernel(RasterArgs u) {
    __shared__ int part[kBlock / 64];
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int n = blockIdx.y;
    bool over = false;
    if (f < u.F) over = box_pixels(tri_setup(u.proj + (int64_t)n * u.V, u.V, u.faces, f, u.H, u.W, u.cull)) > u.oversize;
    const unsigned long long m = __ballot(over);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) part[w] = __popcll(m);
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int j = 0; j < kBlock / 64; ++j) before += j < w ? part[j] : 0;
    const int64_t slot = (int64_t)u.blockcount[(int64_t)n * gridDim.x + blockIdx.x] + before + __popcll(m & ((1ull << lane) - 1ull));
    if (over && slot < (int64_t)gridDim.y * u.F) u.list[slot] = (int)((int64_t)n * u.F + f);
}

__global__ __launch_bounds__(64) void raster_wave_kernel(RasterArgs u, const int* __restrict__ total, int64_t capacity) {
    const int lane = threadIdx.x;
    const int64_t count = min((int64_t)*total, capacity);
    for (int64_t k = blockIdx.x; k < count; k += gridDim.x) {
        const int64_t item = u.list[k];
        if ((uint64_t)item >= (uint64_t)capacity) continue;
        const int64_t n = item / u.F, f = item - n * u.F;
        const Tri t = tri_setup(u.proj + n * u.V, u.V, u.faces, f, u.H, u.W, u.cull);
        const int64_t px = box_pixels(t);
        const int bw = t.x1 - t.x0 + 1;
        unsigned long long* vis_n = u.vis + n * u.H * u.W;
        for (int64_t p = lane; p < px; p += 64) draw_pixel(t, f, t.x0 + (int)(p % bw), t.y0 + (int)(p / bw), vis_n, u.W);
    }
}

// ------------------------------------------------------------------ resolve

struct ResolveArgs {
    const unsigned long long* vis;
    const int4* proj;
    const float* verts;
    int64_t V;
    const int* faces;
    int64_t F;
    const float* cams;
    int N, H, W, cull;
    const float* normals;        // [V,3] or null: face normals
    const float* attrs;          // [V,C] or null
    int C;
    unsigned char* mask;
    int* face;
    float* bary;                 // [N,H,W,3]
    float* depth;
    float* normal;               // [N,H,W,3]
    float* attr_out;             // [N,H,W,C]
};

__device__ __forceinline__ void store_unit(float* __restrict__ out, F3 v) {
    const float l = sqrtf(dot(v, v));
    const bool ok = l > 0.f && isfinite(l);
    out[0] = ok ? v.x / l : 0.f; out[1] = ok ? v.y / l : 0.f; out[2] = ok ? v.z / l : 0.f;
}

__global__ __launch_bounds__(kBlock) void resolve_kernel(ResolveArgs u) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t hw = (int64_t)u.H * u.W;
    if (p >= (int64_t)u.N * hw) return;
    const int64_t n = p / hw, r = p - n * hw;
    const int j = (int)(r / u.W), i = (int)(r - (int64_t)j * u.W);
    const unsigned long long key = u.vis[p];
    const int64_t f = (int64_t)(key & 0xffffffffull);
    float b[3] = {0.f, 0.f, 0.f}, depth = 0.f;
    const bool hit = key != kMiss && f < u.F;
    int64_t idx[3] = {0, 0, 0};
    if (hit) {
        const Tri t = tri_setup(u.proj + n * u.V, u.V, u.faces, f, u.H, u.W, u.cull);
        int64_t e[3];
        edge_values(t, i, j, e);
        float lam[3];
        weights(e, lam);
        const float z = __uint_as_float((unsigned)(key >> 32));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            b[k] = (lam[k] / t.z[k]) * z;
            const int64_t v = u.faces[3 * f + k];
            idx[k] = (uint64_t)v < (uint64_t)u.V ? v : 0;
        }
        const Camera c = load_camera(u.cams + 25 * n, u.H, u.W);
        const float xs = (float)i - c.k[2], ys = (float)j - c.k[5];
        const float det = c.k[0] * c.k[4] - c.k[1] * c.k[3];
        const float dx = (c.k[4] * xs - c.k[1] * ys) / det, dy = (c.k[0] * ys - c.k[3] * xs) / det;
        depth = z * sqrtf((dx * dx + dy * dy) + 1.f);
    }
    u.mask[p] = hit ? 1 : 0;
    u.face[p] = hit ? (int)f : -1;
    u.depth[p] = depth;
    u.bary[3 * p] = b[0]; u.bary[3 * p + 1] = b[1]; u.bary[3 * p + 2] = b[2];
    F3 nrm{0.f, 0.f, 0.f};
    if (hit) {
        if (u.normals) {
            const F3 n0 = load3(u.normals, idx[0]), n1 = load3(u.normals, idx[1]), n2 = load3(u.normals, idx[2]);
            nrm = F3{(b[0] * n0.x + b[1] * n1.x) + b[2] * n2.x, (b[0] * n0.y + b[1] * n1.y) + b[2] * n2.y, (b[0] * n0.z + b[1] * n1.z) + b[2] * n2.z};
        } else {
            const F3 A = load3(u.verts, idx[0]);
            nrm = cross(sub(load3(u.verts, idx[1]), A), sub(load3(u.verts, idx[2]), A));
        }
    }
    store_unit(u.normal + 3 * p, nrm);
    for (int c = 0; c < u.C; ++c) {
        float a = 0.f;
        if (hit) a = (b[0] * u.attrs[idx[0] * u.C + c] + b[1] * u.attrs[idx[1] * u.C + c]) + b[2] * u.attrs[idx[2] * u.C + c];
        u.attr_out[p * u.C + c] = a;
    }
}

// ------------------------------------------------------------------ host side

unsigned blocks(int64_t n) { return ia::blocks(n, kBlock); }

int check_sizes(const char* what, int64_t V, int64_t F, int N, int H, int W) {
    if (V < 0 || V > kMaxCount || F < 0 || F > kMaxCount)
        return ia::fail(IA_ERR_INVALID_ARG, "%s: V and F must be in [0, 2^28], got V = %lld, F = %lld", what, (long long)V, (long long)F);
    if (N < 1 || N > kMaxViews || H < 1 || H > kMaxSide || W < 1 || W > kMaxSide)
        return ia::fail(IA_ERR_INVALID_ARG, "%s: 1 <= N <= 65535 views of 1 .. 16384 pixels per side, got N = %d, H = %d, W = %d", what, N, H, W);
    if ((int64_t)N * F >= ((int64_t)1 << 31) || (int64_t)N * V >= ((int64_t)1 << 31) || (int64_t)N * H * W >= ((int64_t)1 << 31))
        return ia::fail(IA_ERR_INVALID_ARG, "%s: N F, N V and N H W must stay below 2^31", what);
    return IA_OK;
}

size_t raster_scratch_ints(int N, int64_t F) { return (size_t)blocks(F) * N + 1 + (size_t)N * F; }

}  // namespace

extern "C" int ia_mesh_project(const float* verts, int64_t V, const float* cams, int N, int H, int W, float near, void* proj, void* stream) {
    if (int st = check_sizes("ia_mesh_project", V, 0, N, H, W)) return st;
    IA_REQUIRE(near >= 0.f, "ia_mesh_project: near must be >= 0, got %g", (double)near);
    if (!on_device(cams) || (V && (!on_device(verts) || !on_device(proj))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_project: verts, cams and proj must be device pointers");
    hipStream_t s = (hipStream_t)stream;
    // The one host read of the call: the N camera labels, before the first launch (K must be affine).
    std::vector<float> h((size_t)N * 25);
    if (hipMemcpyAsync(h.data(), cams, h.size() * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return ia::check_launch("ia_mesh_project (cameras)");
    for (int n = 0; n < N; ++n) {
        const float* k = h.data() + 25 * (size_t)n + 16;
        if (!(k[6] == 0.f && k[7] == 0.f && k[8] == 1.f))
            return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_project: the last row of K of view %d is [%g, %g, %g], must be [0, 0, 1]", n, (double)k[6],
                            (double)k[7], (double)k[8]);
    }
    if (V == 0) return IA_OK;
    project_kernel<<<dim3(blocks(V), N), kBlock, 0, s>>>(verts, V, cams, H, W, near, static_cast<int4*>(proj));
    return ia::check_launch("ia_mesh_project");
}

extern "C" int ia_mesh_raster_scratch_bytes(int N, int64_t F, size_t* h_bytes) {
    if (int st = check_sizes("ia_mesh_raster_scratch_bytes", 0, F, N, 1, 1)) return st;
    IA_REQUIRE(h_bytes, "ia_mesh_raster_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = sizeof(int) * raster_scratch_ints(N, F);
    return IA_OK;
}

extern "C" int ia_mesh_raster(const void* proj, int64_t V, const int* faces, int64_t F, int N, int H, int W, int cull_back,
                              int64_t oversize_pixels, unsigned long long* vis, int* culled, void* scratch, size_t scratch_bytes, void* stream) {
    if (int st = check_sizes("ia_mesh_raster", V, F, N, H, W)) return st;
    IA_REQUIRE(oversize_pixels >= 0, "ia_mesh_raster: oversize_pixels must be >= 0, got %lld", (long long)oversize_pixels);
    if (!on_device(vis) || !on_device(culled) || (F && (!on_device(faces) || (V && !on_device(proj)))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_raster: proj, faces, vis and culled must be device pointers");
    hipStream_t s = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    if (hipMemsetAsync(vis, 0xff, sizeof(unsigned long long) * (size_t)(N * hw), s) != hipSuccess ||
        hipMemsetAsync(culled, 0, sizeof(int) * (size_t)N, s) != hipSuccess)
        return ia::check_launch("ia_mesh_raster (clear)");
    if (F == 0) return IA_OK;
    const bool wave_path = oversize_pixels < hw;                          // (no clamped box holds more than H W pixels)
    const unsigned nbx = blocks(F);
    const int64_t nb = (int64_t)nbx * N;
    int* blockcount = nullptr;
    if (wave_path) {
        const size_t need = sizeof(int) * raster_scratch_ints(N, F);
        if (scratch_bytes < need) return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_raster: scratch holds %zu bytes, needs %zu", scratch_bytes, need);
        if (!on_device(scratch)) return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_raster: scratch must be a device pointer");
        blockcount = static_cast<int*>(scratch);
        if (hipMemsetAsync(blockcount, 0, sizeof(int) * (size_t)(nb + 1), s) != hipSuccess) return ia::check_launch("ia_mesh_raster (clear)");
    }
    RasterArgs u{static_cast<const int4*>(proj), V, faces, F, H, W, cull_back ? 1 : 0, oversize_pixels, vis, culled, blockcount,
                 blockcount ? blockcount + nb + 1 : nullptr};
    raster_small_kernel<<<dim3(nbx, N), kBlock, 0, s>>>(u);
    if (int st = ia::check_launch("ia_mesh_raster")) return st;
    if (!wave_path) return IA_OK;
    scan_kernel<<<1, kScanBlock, 0, s>>>(blockcount, blockcount, nb);
    if (int st = ia::check_launch("ia_mesh_raster (scan)")) return st;
    raster_list_kernel<<<dim3(nbx, N), kBlock, 0, s>>>(u);
    if (int st = ia::check_launch("ia_mesh_raster (list)")) return st;
    const int64_t capacity = (int64_t)N * F;
    raster_wave_kernel<<<(unsigned)std::min<int64_t>(capacity, 8 * ia::kNumCU), 64, 0, s>>>(u, blockcount + nb, capacity);
    return ia::check_launch("ia_mesh_raster (wave)");
}

extern "C" int ia_mesh_resolve(const unsigned long long* vis, const void* proj, const float* verts, int64_t V, const int* faces, int64_t F,
                               const float* cams, int N, int H, int W, int cull_back, const float* normals, const float* attributes, int C,
                               unsigned char* mask, int* face, float* bary, float* depth, float* normal, float* attr_out, void* stream) {
    if (int st = check_sizes("ia_mesh_resolve", V, F, N, H, W)) return st;
    IA_REQUIRE(C >= 0 && C <= kMaxChannels, "ia_mesh_resolve: at most %d attribute channels, got %d", kMaxChannels, C);
    IA_REQUIRE((C == 0) == (attributes == nullptr), "ia_mesh_resolve: attributes and C must be given together");
    if (!on_device(vis) || !on_device(cams) || !on_device(mask) || !on_device(face) || !on_device(bary) || !on_device(depth) || !on_device(normal) ||
        (C && (!on_device(attr_out) || (V && !on_device(attributes)))) || (normals && V && !on_device(normals)) ||
        (F && V && (!on_device(proj) || !on_device(verts) || !on_device(faces))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mesh_resolve: every array must be a device pointer");
    ResolveArgs u{vis, static_cast<const int4*>(proj), verts, V, faces, (V ? F : 0), cams, N, H, W, cull_back ? 1 : 0, normals, attributes, C,
                  mask, face, bary, depth, normal, attr_out};
    resolve_kernel<<<blocks((int64_t)N * H * W), kBlock, 0, (hipStream_t)stream>>>(u);
    return ia::check_launch("ia_mesh_resolve");
}
