// Isosurface ray casting over a device density volume (no counterpart in the reference): depth, normal and mask of the first point
// along each ray where the trilinear interpolant of the volume exceeds the level.  The lattice and inside rule are those of geometry.hip
// (point (i, j, k) at lo + idx * step per axis, inside iff v > level, NaN outside), so the surface is the one marching cubes meshes.
//
// ia_volume_bricks: min / max of the volume over bricks of 8 x 8 x 8 cells (9^3 points, neighbouring bricks share their boundary
//   points), NaN ignored.  One wave per brick, a shuffle reduction.  Depends only on the volume: reusable for any level and any view.
// ia_raycast_volume: one thread per ray, 256-thread workgroups.  The ray is taken into lattice index space (O = (o - lo) / step,
//   D = d / step), clipped to the box [0, n - 1] and to t >= t_min, and walked cell by cell with a 3-D DDA whose every plane crossing
//   t = (plane - O) / D is computed from the plane index directly (ties: lower axis first).  A brick whose max <= level is jumped over:
//   the jump lands on the state the cell-by-cell walk reaches at the brick's exit plane (the planes crossed are those that come before
//   it in (t, axis) order), so skipping changes no result, bit for bit.  A cell with a NaN corner, or whose corners are all <= level,
//   has no surface.  Otherwise the field along the ray inside the cell is a cubic in t; it is split at the roots of its derivative into
//   monotone pieces, the first piece whose end lies inside is bisected kRcBisect times, and the bracket's midpoint is the hit.  Normals
//   are -g/|g| of the trilinear interpolation of the corners' central-difference gradients (one-sided at the border).
// ia_volume_gradient: that interpolated gradient at arbitrary points (clamped into the box): vertex normals of the marching-cubes mesh.
// No atomics and no host synchronisation: every output is a pure function of the inputs.  Every load index is clamped to the lattice.
#include "geom_common.h"

namespace {

using ia::check_volume; using ia::on_device;

constexpr int kBlock = 256;
constexpr int kBrick = 8;              // cells per brick edge
constexpr int kRcBisect = 20;          // bracket <= sqrt(3) * 2^-20 < 2e-6 cell

struct RcVol {
    const float* v;
    int n[3];
    int64_t S;                         // ny * nz
    float lo[3], step[3];
    float level;
};

__device__ __forceinline__ float vat(const RcVol& m, int i, int j, int k) { return m.v[(int64_t)i * m.S + (int64_t)j * m.n[2] + k]; }

// ------------------------------------------------------------------ bricks

__global__ __launch_bounds__(64) void volume_bricks_kernel(RcVol m, int nbx, int nby, int nbz, float2* __restrict__ bricks) {
    const int b = blockIdx.x;
    const int bz = b % nbz, by = (b / nbz) % nby, bx = b / (nbz * nby);
    const int i0 = bx * kBrick, j0 = by * kBrick, k0 = bz * kBrick;
    const int ex = min(kBrick, m.n[0] - 1 - i0) + 1, ey = min(kBrick, m.n[1] - 1 - j0) + 1, ez = min(kBrick, m.n[2] - 1 - k0) + 1;
    float lo = INFINITY, hi = -INFINITY;
    for (int p = threadIdx.x; p < ex * ey * ez; p += 64) {
        const int dz = p % ez, dy = (p / ez) % ey, dx = p / (ez * ey);
        const float v = vat(m, i0 + dx, j0 + dy, k0 + dz);
        lo = fminf(lo, v);                                     // fminf / fmaxf drop a NaN
        hi = fmaxf(hi, v);
    }
    lo = ia::wave_min(lo);
    hi = ia::wave_max(hi);
    if (threadIdx.x == 0) bricks[b] = make_float2(lo, hi);
}

// ------------------------------------------------------------------ gradients

// Central-difference gradient at lattice point (i, j, k), one-sided at the border, divided by the step per axis.
__device__ __forceinline__ void point_grad(const RcVol& m, int i, int j, int k, float (&g)[3]) {
    const int idx[3] = {i, j, k};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int lo[3] = {i, j, k}, hi[3] = {i, j, k};
        lo[a] = max(idx[a] - 1, 0);
        hi[a] = min(idx[a] + 1, m.n[a] - 1);
        const float d = vat(m, hi[0], hi[1], hi[2]) - vat(m, lo[0], lo[1], lo[2]);
        g[a] = d / ((float)(hi[a] - lo[a]) * m.step[a]);
    }
}

// Trilinear interpolation, at local coordinates u in the cell (i, j, k), of the gradients at its 8 corners.
__device__ void cell_grad(const RcVol& m, int i, int j, int k, const float (&u)[3], float (&g)[3]) {
    g[0] = g[1] = g[2] = 0.f;
    for (int c = 0; c < 8; ++c) {
        const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
        const float w = (dx ? u[0] : 1.f - u[0]) * (dy ? u[1] : 1.f - u[1]) * (dz ? u[2] : 1.f - u[2]);
        float gc[3];
        point_grad(m, i + dx, j + dy, k + dz, gc);
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] += w * gc[a];
    }
}

__global__ __launch_bounds__(kBlock) void volume_gradient_kernel(RcVol m, const float* __restrict__ pts, int n, float* __restrict__ grad) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    int c[3];
    float u[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float P = fminf(fmaxf((pts[3 * r + a] - m.lo[a]) / m.step[a], 0.f), (float)(m.n[a] - 1));   // NaN -> 0
        c[a] = min((int)floorf(P), m.n[a] - 2);
        u[a] = P - (float)c[a];
    }
    float g[3];
    cell_grad(m, c[0], c[1], c[2], u, g);
#pragma unroll
    for (int a = 0; a < 3; ++a) grad[3 * r + a] = g[a];
}

// ------------------------------------------------------------------ ray casting

struct RcRays {
    const float2* bricks;
    int nb[3];
    int skip;
    const float* ro;
    const float* rd;
    int n_rays;
    float t_min;
    float* depth;
    float* normal;
    unsigned char* mask;
};

// t of lattice plane p along axis a
__device__ __forceinline__ float plane_t(float p, float O, float D) { return (p - O) / D; }

// t of the next plane the ray crosses from cell index i along an axis (+inf when the ray is parallel to the axis' planes)
__device__ __forceinline__ float next_t(int i, float O, float D) {
    return D > 0.f ? plane_t((float)(i + 1), O, D) : (D < 0.f ? plane_t((float)i, O, D) : INFINITY);
}

// First s in [0, L] where the cubic ((c3 s + c2) s + c1) s + c0 (c0 already minus the level) is > 0, or -1.
__device__ __forceinline__ float cubic_first_hit(float c0, float c1, float c2, float c3, float L) {
    if (c0 > 0.f) return 0.f;
    float br[3];
    int nbr = 0;
    const float A = 3.f * c3, B = 2.f * c2, C = c1;           // derivative A s^2 + B s + C
    float r0 = -1.f, r1 = -1.f;
    if (A == 0.f) {
        if (B != 0.f) r0 = -C / B;
    } else {
        const float disc = B * B - 4.f * A * C;
        if (disc > 0.f) {
            const float q = -0.5f * (B + copysignf(sqrtf(disc), B));
            r0 = q / A;
            r1 = q != 0.f ? C / q : -1.f;
            if (r1 < r0) { const float t = r0; r0 = r1; r1 = t; }
        }
    }
    if (r0 > 0.f && r0 < L) br[nbr++] = r0;
    if (r1 > 0.f && r1 < L) br[nbr++] = r1;
    br[nbr++] = L;
    float a = 0.f;
    for (int p = 0; p < nbr; ++p) {
        const float b = br[p];
        if (((c3 * b + c2) * b + c1) * b + c0 > 0.f) {
            float lo = a, hi = b;
            for (int it = 0; it < kRcBisect; ++it) {
                const float mid = 0.5f * (lo + hi);
                if (((c3 * mid + c2) * mid + c1) * mid + c0 > 0.f) hi = mid; else lo = mid;
            }
            return 0.5f * (lo + hi);
        }
        a = b;
    }
    return -1.f;
}

__global__ __launch_bounds__(kBlock) void raycast_kernel(RcVol m, RcRays R) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= R.n_rays) return;
    float O[3], D[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        O[a] = (R.ro[3 * r + a] - m.lo[a]) / m.step[a];
        D[a] = R.rd[3 * r + a] / m.step[a];
        ok = ok && isfinite(O[a]) && isfinite(D[a]);
    }
    ok = ok && (D[0] != 0.f || D[1] != 0.f || D[2] != 0.f);
    // 1. clip to the box and to t >= t_min
    float t0 = R.t_min, t1 = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float top = (float)(m.n[a] - 1);
        if (D[a] != 0.f) {
            const float ta = plane_t(0.f, O[a], D[a]), tb = plane_t(top, O[a], D[a]);
            t0 = fmaxf(t0, fminf(ta, tb));
            t1 = fminf(t1, fmaxf(ta, tb));
        } else if (!(O[a] >= 0.f && O[a] <= top)) {
            ok = false;
        }
    }
    ok = ok && t0 <= t1;
    bool hit = false;
    float t_hit = 0.f, nrm[3] = {0.f, 0.f, 0.f};
    if (ok) {
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = min(max((int)floorf(O[a] + t0 * D[a]), 0), m.n[a] - 2);
        float tc = t0;
        const int max_it = m.n[0] + m.n[1] + m.n[2];
        for (int it = 0; it < max_it; ++it) {
            if (R.skip) {
                const int b[3] = {c[0] / kBrick, c[1] / kBrick, c[2] / kBrick};
                if (R.bricks[((int64_t)b[0] * R.nb[1] + b[1]) * R.nb[2] + b[2]].y <= m.level) {
                    // 3. jump to the brick's exit plane: the lexicographically first (t, axis) among the three exit planes
                    int pb[3], ax = 0;
                    float T = INFINITY;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        pb[a] = D[a] > 0.f ? min((b[a] + 1) * kBrick, m.n[a] - 1) : b[a] * kBrick;
                        const float ta = D[a] != 0.f ? plane_t((float)pb[a], O[a], D[a]) : INFINITY;
                        if (ta < T) { T = ta; ax = a; }
                    }
                    if (!(T < t1)) break;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        if (a == ax || D[a] == 0.f) continue;
                        // interior planes of this brick that come before (T, ax): the cell-by-cell walk crosses exactly these
                        for (int q = 0; q < kBrick; ++q) {
                            const bool interior = D[a] > 0.f ? c[a] + 1 < pb[a] : c[a] > pb[a];
                            const float tn = next_t(c[a], O[a], D[a]);
                            if (!(interior && (tn < T || (tn == T && a < ax)))) break;
                            c[a] += D[a] > 0.f ? 1 : -1;
                        }
                    }
                    c[ax] = D[ax] > 0.f ? pb[ax] : pb[ax] - 1;
                    if (c[ax] < 0 || c[ax] > m.n[ax] - 2) break;
                    tc = fmaxf(tc, T);
                    continue;
                }
            }
            // 2. this cell spans [tc, te]
            const float tn[3] = {next_t(c[0], O[0], D[0]), next_t(c[1], O[1], D[1]), next_t(c[2], O[2], D[2])};
            int ax = 0;
            float to = tn[0];
            if (tn[1] < to) { to = tn[1]; ax = 1; }
            if (tn[2] < to) { to = tn[2]; ax = 2; }
            const float te = fmaxf(fminf(to, t1), tc);
            float cv[8];
            bool nan = false;
            float vmax = -INFINITY;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                cv[q] = vat(m, c[0] + (q & 1), c[1] + ((q >> 1) & 1), c[2] + (q >> 2));
                nan = nan || isnan(cv[q]);
                vmax = fmaxf(vmax, cv[q]);
            }
            if (!nan && vmax > m.level) {
                // 4-5. the cubic of the trilinear field along the ray, in s = t - tc
                const float k1 = cv[1] - cv[0], k2 = cv[2] - cv[0], k3 = cv[4] - cv[0];
                const float k4 = cv[3] - cv[1] - cv[2] + cv[0], k5 = cv[5] - cv[1] - cv[4] + cv[0], k6 = cv[6] - cv[2] - cv[4] + cv[0];
                const float k7 = cv[7] - cv[3] - cv[5] - cv[6] + cv[1] + cv[2] + cv[4] - cv[0];
                float u[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) u[a] = O[a] + tc * D[a] - (float)c[a];
                const float bu = D[0], bv = D[1], bw = D[2];
                const float c3 = k7 * bu * bv * bw;
                const float c2 = k4 * bu * bv + k5 * bu * bw + k6 * bv * bw + k7 * (u[0] * bv * bw + u[1] * bu * bw + u[2] * bu * bv);
                const float c1 = k1 * bu + k2 * bv + k3 * bw + k4 * (u[0] * bv + u[1] * bu) + k5 * (u[0] * bw + u[2] * bu) +
                                 k6 * (u[1] * bw + u[2] * bv) + k7 * (u[0] * u[1] * bw + u[0] * u[2] * bv + u[1] * u[2] * bu);
                const float c0 = cv[0] + k1 * u[0] + k2 * u[1] + k3 * u[2] + k4 * u[0] * u[1] + k5 * u[0] * u[2] + k6 * u[1] * u[2] +
                                 k7 * u[0] * u[1] * u[2] - m.level;
                const float s = cubic_first_hit(c0, c1, c2, c3, te - tc);
                if (s >= 0.f) {
                    hit = true;
                    t_hit = tc + s;
                    float uh[3], g[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) uh[a] = u[a] + s * D[a];
                    // 7. normal from the interpolated corner gradients
                    cell_grad(m, c[0], c[1], c[2], uh, g);
                    const float len = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
                    if (len > 0.f) {
#pragma unroll
                        for (int a = 0; a < 3; ++a) nrm[a] = -g[a] / len;
                    }
                    break;
                }
            }
            if (to >= t1) break;
            c[ax] += D[ax] > 0.f ? 1 : -1;
            if (c[ax] < 0 || c[ax] > m.n[ax] - 2) break;
            tc = te;
        }
    }
    // 8. a miss writes zeros
    R.depth[r] = hit ? t_hit : 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) R.normal[3 * r + a] = nrm[a];
    R.mask[r] = hit ? 1 : 0;
}

// ------------------------------------------------------------------ host side

void brick_dims(int nx, int ny, int nz, int (&nb)[3]) {
    nb[0] = (int)ia::ceil_div(nx - 1, kBrick);
    nb[1] = (int)ia::ceil_div(ny - 1, kBrick);
    nb[2] = (int)ia::ceil_div(nz - 1, kBrick);
}

size_t brick_bytes(int nx, int ny, int nz) {
    int nb[3];
    brick_dims(nx, ny, nz, nb);
    return sizeof(float2) * (size_t)nb[0] * nb[1] * nb[2];
}

int make_vol(const float* volume, int nx, int ny, int nz, const float* h_lo, const float* h_step, float level, RcVol& m, const char* what) {
    IA_REQUIRE(h_lo && h_step, "%s: h_lo and h_step must be host arrays of 3 floats", what);
    m = RcVol{volume, {nx, ny, nz}, (int64_t)ny * nz, {}, {}, level};
    for (int a = 0; a < 3; ++a) {
        IA_REQUIRE(std::isfinite(h_lo[a]) && h_step[a] > 0.f && std::isfinite(h_step[a]), "%s: lo must be finite and step > 0 on every axis",
                   what);
        m.lo[a] = h_lo[a];
        m.step[a] = h_step[a];
    }
    return IA_OK;
}

}  // namespace

extern "C" int ia_raycast_scratch_bytes(int nx, int ny, int nz, size_t* h_bytes) {
    if (int st = check_volume(nx, ny, nz, "ia_raycast_scratch_bytes")) return st;
    IA_REQUIRE(h_bytes, "ia_raycast_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = brick_bytes(nx, ny, nz);
    return IA_OK;
}

extern "C" int ia_volume_bricks(const float* volume, int nx, int ny, int nz, void* bricks, size_t bricks_bytes, void* stream) {
    if (int st = check_volume(nx, ny, nz, "ia_volume_bricks")) return st;
    if (!on_device(volume) || !on_device(bricks))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_volume_bricks: volume and bricks must be device pointers");
    if (bricks_bytes < brick_bytes(nx, ny, nz))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_volume_bricks: scratch holds %zu bytes, needs %zu", bricks_bytes, brick_bytes(nx, ny, nz));
    int nb[3];
    brick_dims(nx, ny, nz, nb);
    const RcVol m{volume, {nx, ny, nz}, (int64_t)ny * nz, {}, {}, 0.f};
    volume_bricks_kernel<<<(unsigned)(nb[0] * nb[1] * nb[2]), 64, 0, (hipStream_t)stream>>>(m, nb[0], nb[1], nb[2], static_cast<float2*>(bricks));
    return ia::check_launch("ia_volume_bricks");
}

extern "C" int ia_raycast_volume(const float* volume, int nx, int ny, int nz, const float* h_lo, const float* h_step, float level,
                                 const void* bricks, size_t bricks_bytes, const float* rays_o, const float* rays_d, int n_rays, float t_min,
                                 float* depth, float* normal, unsigned char* mask, int flags, void* stream) {
    if (int st = check_volume(nx, ny, nz, "ia_raycast_volume")) return st;
    IA_REQUIRE(n_rays > 0, "ia_raycast_volume: n_rays must be > 0, got %d", n_rays);
    IA_REQUIRE(!std::isnan(level) && !std::isnan(t_min), "ia_raycast_volume: level and t_min must not be NaN");
    RcVol m;
    if (int st = make_vol(volume, nx, ny, nz, h_lo, h_step, level, m, "ia_raycast_volume")) return st;
    const bool skip = !(flags & IA_RAYCAST_DENSE);
    if (!on_device(volume) || !on_device(rays_o) || !on_device(rays_d) || !on_device(depth) || !on_device(normal) || !on_device(mask))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_raycast_volume: volume, rays, depth, normal and mask must be device pointers");
    if (skip) {
        if (!on_device(bricks)) return ia::fail(IA_ERR_INVALID_ARG, "ia_raycast_volume: bricks must be a device pointer (or pass IA_RAYCAST_DENSE)");
        if (bricks_bytes < brick_bytes(nx, ny, nz))
            return ia::fail(IA_ERR_INVALID_ARG, "ia_raycast_volume: scratch holds %zu bytes, needs %zu", bricks_bytes, brick_bytes(nx, ny, nz));
    }
    RcRays R{};
    R.bricks = skip ? static_cast<const float2*>(bricks) : nullptr;
    brick_dims(nx, ny, nz, R.nb);
    R.skip = skip ? 1 : 0;
    R.ro = rays_o; R.rd = rays_d; R.n_rays = n_rays; R.t_min = t_min;
    R.depth = depth; R.normal = normal; R.mask = mask;
    raycast_kernel<<<(unsigned)ia::ceil_div(n_rays, kBlock), kBlock, 0, (hipStream_t)stream>>>(m, R);
    return ia::check_launch("ia_raycast_volume");
}

extern "C" int ia_volume_gradient(const float* volume, int nx, int ny, int nz, const float* h_lo, const float* h_step, const float* points,
                                  int n, float* grad, void* stream) {
    if (int st = check_volume(nx, ny, nz, "ia_volume_gradient")) return st;
    IA_REQUIRE(n >= 0, "ia_volume_gradient: n must be >= 0, got %d", n);
    RcVol m;
    if (int st = make_vol(volume, nx, ny, nz, h_lo, h_step, 0.f, m, "ia_volume_gradient")) return st;
    if (n == 0) return IA_OK;
    if (!on_device(volume) || !on_device(points) || !on_device(grad))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_volume_gradient: volume, points and grad must be device pointers");
    volume_gradient_kernel<<<(unsigned)ia::ceil_div(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(m, points, n, grad);
    return ia::check_launch("ia_volume_gradient");
}
