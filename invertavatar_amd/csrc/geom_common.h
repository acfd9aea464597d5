// Primitives shared by the geometry translation units (every .hip that includes this file, and cluster_tree.h on top of it): scans,
// wave reductions, 3-vectors, the per-triangle functions, lattice helpers and the host-side argument checks.  Device code is
// __forceinline__ functions and templates only, no kernels: every .hip is its own code object, so a kernel that needs one of these (the
// scan) is a wrapper of a few lines in that file's anonymous namespace.  Every operation order here is part of the results (geometry.py restates them in NumPy).
#pragma once

#include "ia_common.h"

namespace ia {

// ------------------------------------------------------------------ scans

constexpr int kScanBlock = 1024;

// Exclusive scan of in[0 .. n) into out[0 .. n) by ONE workgroup of kScanBlock threads; returns the total to every thread.  A thread
// sums a contiguous slice, the partial sums are scanned in LDS (Hillis-Steele) and the slice is written back with a running sum.
// in == out is allowed.  Acc: the type the sums are carried in (out receives its low 32 bits).
template <class Acc>
__device__ __forceinline__ Acc scan_workgroup(const int* in, int* out, int64_t n) {
    __shared__ Acc s[kScanBlock];
    const int t = threadIdx.x;
    const int64_t per = (n + kScanBlock - 1) / kScanBlock;
    const int64_t c0 = min((int64_t)t * per, n), c1 = min(c0 + per, n);
    Acc a = 0;
    for (int64_t c = c0; c < c1; ++c) a += in[c];
    s[t] = a;
    __syncthreads();
    for (int off = 1; off < kScanBlock; off <<= 1) {
        const Acc x = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    Acc run = s[t] - a;
    for (int64_t c = c0; c < c1; ++c) {
        const int v = in[c];
        out[c] = (int)run;
        run += v;
    }
    const Acc total = s[kScanBlock - 1];
    __syncthreads();                                                      // (s may be written again by a following call)
    return total;
}

// Exclusive scan of one int per thread over a workgroup of kThreads threads, and the workgroup total.
template <int kThreads>
__device__ __forceinline__ void block_scan(int a, int& excl, int& total) {
    __shared__ int s[kThreads];
    const int t = threadIdx.x;
    s[t] = a;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const int x = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    excl = s[t] - a;
    total = s[kThreads - 1];
    __syncthreads();
}

// ------------------------------------------------------------------ wave reductions (every lane receives the result)

__device__ __forceinline__ float lesser(float a, float b) { return fminf(a, b); }      // fminf / fmaxf, fmin / fmax drop a NaN
__device__ __forceinline__ double lesser(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ int lesser(int a, int b) { return min(a, b); }
__device__ __forceinline__ float greater(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double greater(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ int greater(int a, int b) { return max(a, b); }

// Butterfly from offset 32 down to 1: every lane combines the same pairs, so a floating-point sum has one order and one result.
template <class T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}
template <class T> __device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = lesser(v, __shfl_xor(v, off, kWave));
    return v;
}
template <class T> __device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = greater(v, __shfl_xor(v, off, kWave));
    return v;
}

// *dst += number of lanes of the wave with `p` set: a ballot and one integer atomic by the first such lane.
__device__ __forceinline__ void wave_count(bool p, int* dst) {
    const unsigned long long m = __ballot(p);
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(dst, __popcll(m));
}

// ------------------------------------------------------------------ 3-vectors, cells, lattice indices

template <class T> struct Vec3 { T x, y, z; };

template <class T> __device__ __forceinline__ Vec3<T> sub(Vec3<T> a, Vec3<T> b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
template <class T> __device__ __forceinline__ T dot(Vec3<T> a, Vec3<T> b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
template <class T> __device__ __forceinline__ Vec3<T> cross(Vec3<T> a, Vec3<T> b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
template <class T> __device__ __forceinline__ bool finite3(Vec3<T> a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// Squared distance of the pair (query p, point x) of the nearest-point queries (point_tree.hip; geometry._pair_d2 in NumPy): three
// differences, three squares and two sums, every operation rounded on its own.  box_d2: the same expression on the gaps between p and
// the box [lo, hi]; it never exceeds pair_d2(p, x) for a point x of the box.
__device__ __forceinline__ float gaps_d2(float dx, float dy, float dz) { return (dx * dx + dy * dy) + dz * dz; }
__device__ __forceinline__ float pair_d2(Vec3<float> p, Vec3<float> x) { return gaps_d2(x.x - p.x, x.y - p.y, x.z - p.z); }
__device__ __forceinline__ float box_d2(Vec3<float> p, float4 lo, float4 hi) {
    return gaps_d2(fmaxf(fmaxf(lo.x - p.x, 0.f), p.x - hi.x), fmaxf(fmaxf(lo.y - p.y, 0.f), p.y - hi.y), fmaxf(fmaxf(lo.z - p.z, 0.f), p.z - hi.z));
}

// Signed solid angle of triangle A B C seen from p (the per-pair function of the winding number, winding.hip): relative to the query,
// the numerator from the edges; every operation rounded on its own.  A triangle without area gives atan2f(0, den >= 0) = 0.
__device__ __forceinline__ float solid_angle(Vec3<float> p, Vec3<float> A, Vec3<float> B, Vec3<float> C) {
    const Vec3<float> a = sub(A, p), b = sub(B, p), c = sub(C, p);
    const float num = dot(a, cross(sub(b, a), sub(c, a)));
    const float la = sqrtf(dot(a, a)), lb = sqrtf(dot(b, b)), lc = sqrtf(dot(c, c));
    const float den = (((la * lb) * lc + dot(a, b) * lc) + dot(b, c) * la) + dot(c, a) * lb;
    return 2.f * atan2f(num, den);
}

// The per-triangle function of the closest-point queries (surface_distance.hip, closest_tree.hip), every operation rounded on its own.
// Closest point of the segment a + t e, t in [0, 1] (ee = e . e), to the origin; kept if its squared distance is below `best`.
__device__ __forceinline__ void seg(Vec3<float> a, Vec3<float> e, float ee, float& best, Vec3<float>& q) {
    float t = 0.f;
    if (ee > 0.f) t = fminf(fmaxf(-dot(a, e) / ee, 0.f), 1.f);
    const Vec3<float> r = {a.x + t * e.x, a.y + t * e.y, a.z + t * e.z};
    const float d2 = dot(r, r);
    if (d2 < best) { best = d2; q = r; }
}

// Distance from p to the closed triangle ABC; q: the closest point relative to p.
__device__ __forceinline__ float tri_dist(Vec3<float> p, Vec3<float> A, Vec3<float> B, Vec3<float> C, Vec3<float>& q) {
    const Vec3<float> a = sub(A, p), b = sub(B, p), c = sub(C, p);
    float d2 = INFINITY;
    q = {NAN, NAN, NAN};
    const Vec3<float> eab = sub(b, a), ebc = sub(c, b), eca = sub(a, c);
    const float lab = dot(eab, eab), lbc = dot(ebc, ebc), lca = dot(eca, eca);
    seg(a, eab, lab, d2, q);
    seg(b, ebc, lbc, d2, q);
    seg(c, eca, lca, d2, q);
    float d = sqrtf(d2);
    // the normal from the two shorter edges (eab x ebc = ebc x eca = eca x eab): no cancellation on needle-shaped triangles
    const Vec3<float> n = (lab >= lbc && lab >= lca) ? cross(ebc, eca) : (lbc >= lca ? cross(eca, eab) : cross(eab, ebc));
    const float nn = dot(n, n);
    if (nn > 0.f && dot(n, cross(a, eab)) >= 0.f && dot(n, cross(b, ebc)) >= 0.f && dot(n, cross(c, eca)) >= 0.f) {
        const float na = dot(n, a);
        const float dp = fabsf(na) / sqrtf(nn);
        if (dp < d) {                                // (a vertex or edge that p lies on keeps its exact 0)
            const float s = na / nn;
            d = dp;
            q = {n.x * s, n.y * s, n.z * s};
        }
    }
    return d;
}

// The per-triangle function of the ray queries (ray_tree.hip), every operation rounded on its own: the ray o + t d against the closed
// triangle ABC, both orientations.  Relative to the origin, w = the three edge functions (d . (b x c), d . (c x a), d . (a x b)); the
// ray is inside iff none is negative or none is positive; t = (n . a) / (n . d) with n = (b - a) x (c - a).  Accepted iff inside,
// n . d != 0, t finite, t_lo <= t <= t_hi (a NaN compares false) and the point p = o + t d lies in the triangle's own bounding box
// grown by g = 2^-14 max(|o|_inf, |A|_inf, |B|_inf, |C|_inf) on every side.  The last clause is what makes pruning by boxes sound at
// all: far from the origin of the ray the edge functions accept small triangles that the ray misses by any distance.
// The barycentrics are w / ((w.x + w.y) + w.z), the caller's.  Not watertight: the three signs of one triangle are rounded separately.
__device__ __forceinline__ float max_abs(Vec3<float> v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fabsf(v.z)); }
__device__ __forceinline__ bool ray_tri(Vec3<float> o, Vec3<float> d, float t_lo, float t_hi, Vec3<float> A, Vec3<float> B, Vec3<float> C,
                                        float& t, Vec3<float>& w) {
    const Vec3<float> a = sub(A, o), b = sub(B, o), c = sub(C, o);
    w = {dot(d, cross(b, c)), dot(d, cross(c, a)), dot(d, cross(a, b))};
    const bool inside = (w.x >= 0.f && w.y >= 0.f && w.z >= 0.f) || (w.x <= 0.f && w.y <= 0.f && w.z <= 0.f);
    const Vec3<float> n = cross(sub(b, a), sub(c, a));
    const float den = dot(n, d);
    t = dot(n, a) / den;
    const float g = 6.103515625e-5f * fmaxf(fmaxf(max_abs(o), max_abs(A)), fmaxf(max_abs(B), max_abs(C)));          // 2^-14
    const Vec3<float> p = {o.x + t * d.x, o.y + t * d.y, o.z + t * d.z};
    const bool boxed = fminf(fminf(A.x, B.x), C.x) - g <= p.x && p.x <= fmaxf(fmaxf(A.x, B.x), C.x) + g &&
                       fminf(fminf(A.y, B.y), C.y) - g <= p.y && p.y <= fmaxf(fmaxf(A.y, B.y), C.y) + g &&
                       fminf(fminf(A.z, B.z), C.z) - g <= p.z && p.z <= fmaxf(fmaxf(A.z, B.z), C.z) + g;
    return inside && den != 0.f && isfinite(t) && t_lo <= t && t <= t_hi && boxed;
}

// Cell of coordinate x along an axis of n cells that starts at lo, inv = 1 / cell size; a NaN lands in cell 0.
__device__ __forceinline__ int cell_of(float x, float lo, float inv, int n) {
    return (int)fminf(fmaxf(floorf((x - lo) * inv), 0.f), (float)(n - 1));
}

// Linear point index n (0 <= n < 2^31, z fastest) of an [nx, ny, nz] lattice -> (i, j, k).
__device__ __forceinline__ void unravel(int n, int ny, int nz, int& i, int& j, int& k) {
    const unsigned u = (unsigned)n, q = u / (unsigned)nz;
    k = (int)(u - q * (unsigned)nz);
    i = (int)(q / (unsigned)ny);
    j = (int)(q - (unsigned)i * (unsigned)ny);
}

// ------------------------------------------------------------------ host side

inline bool on_device(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    const hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type != hipMemoryTypeHost && attr.type != hipMemoryTypeUnregistered;
}

// A lattice volume: every dimension >= 2 and fewer than 2^31 points (point, vertex and label indices are int32).
inline int check_volume(int nx, int ny, int nz, const char* what) {
    if (nx < 2 || ny < 2 || nz < 2) return fail(IA_ERR_INVALID_ARG, "%s: every dimension must be >= 2, got %d x %d x %d", what, nx, ny, nz);
    if ((int64_t)nx * ny * nz >= ((int64_t)1 << 31))
        return fail(IA_ERR_INVALID_ARG, "%s: %d x %d x %d volume has 2^31 points or more", what, nx, ny, nz);
    return IA_OK;
}

// Workgroups of `per` items that cover n items (at least one).
inline unsigned blocks(int64_t n, int per) { return (unsigned)ceil_div(n < 1 ? 1 : n, per); }

}  // namespace ia
