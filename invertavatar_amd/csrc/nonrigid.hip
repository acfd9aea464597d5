// Non-rigid fitting of a template mesh to a target (non-rigid ICP) on the device: the kernels around the closest-point query.  No
// counterpart in the reference; the definition is geometry.nonrigid_align / nonrigid_solve and their NumPy restatement.
//
// The unknown is one displacement d_i (double) per template vertex.  One pairing builds the terms, one solve runs conjugate gradients
// on (C + a L + B) d = b, all of it on the stream without a host round trip:
//
//   terms    : one thread per vertex: does the pair (p_i, q_i) count (distance finite, face >= 0, distance <= threshold in fp32, vertex
//              not pinned, for the plane metric a target face with a normal, with normal_cos the two normals compatible), c_i, n_i,
//              b_i = C_i (q_i - x_i) + beta_i l_i, and per workgroup the double partial sums of c |p - q|^2 and of c; a one-workgroup
//              launch adds the workgroups.
//   rhs      : b from given weights and offsets (nonrigid_solve on its own).
//   apply    : y = (C + a L + B) x on double [V,3], one thread per vertex: the neighbour sum over the CSR row in ascending j exactly
//              as step_kernel of smooth.hip, (L x)_i = deg_i x_i - sum_j x_j; a vertex of degree > kHeavy has its sum from the launch
//              before (heavy: one wave per such vertex, lane l sums entries l, l + 64, ... and the lanes are added in the butterfly).
//              Pinned rows are 0, and every vector the solver holds is 0 there, so a neighbour's pin needs no test.  The same launch
//              leaves the workgroup's partial of x . y (and of b . x for the energies).
//   update   : alpha = |r|^2 / p.Ap; x += alpha p; r -= alpha Ap; partial of |r|^2.
//   direction: beta = |r'|^2 / |r|^2; p = r + beta p; workgroup 0 writes the scalars of the next step.
//
// A conjugate-gradient step is three launches (heavy, if there is a heavy vertex, is a fourth): apply, update, direction.  A dot
// product is a per-workgroup partial (butterfly per wave, the waves in wave order); every workgroup of the NEXT launch adds all the
// partials again in one fixed order (a thread adds a contiguous run of workgroups in index order, then the same workgroup sum), so all
// of them hold the same bits and no launch of one workgroup sits between the steps.  The scalars (|r|^2, |b|^2, the freeze flag, the
// step count) live in device memory in two slots: step k reads slot k & 1 and workgroup 0 of its last launch writes the other one, so
// no workgroup reads a word that another one writes in the same launch.  Once frozen (|r|^2 <= tol^2 |b|^2, p.Ap <= 0, or a scalar
// that is not finite) every later launch returns at once and only carries the slot along.
//
// No floating-point atomics, no host synchronisation inside a solve, bit-equal from run to run.  Plain IEEE double arithmetic; the
// build has -ffp-contract=off.
#include "geom_common.h"

#include <algorithm>
#include <cmath>

namespace {

using ia::blocks; using ia::on_device; using ia::wave_sum;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kHeavy = 64;                           // as smooth.hip: the adjacency's heavy list holds the vertices of degree > 64
constexpr int64_t kMaxCount = (int64_t)1 << 28;
constexpr int kState = 4;                            // |r|^2, |b|^2, frozen (0 | 1), steps taken; out [5]: energy at the start, at the
                                                     // end, steps, |r| / |b|, frozen

using D3 = ia::Vec3<double>;
__device__ __forceinline__ D3 load3(const double* __restrict__ v, int64_t i) { return {v[3 * i], v[3 * i + 1], v[3 * i + 2]}; }
__device__ __forceinline__ D3 load3(const float* __restrict__ v, int64_t i) { return {(double)v[3 * i], (double)v[3 * i + 1], (double)v[3 * i + 2]}; }
__device__ __forceinline__ void store3(double* __restrict__ v, int64_t i, D3 a) { v[3 * i] = a.x; v[3 * i + 1] = a.y; v[3 * i + 2] = a.z; }

// The sum of one double per thread over the workgroup: the butterfly per wave, then the waves in wave order.  Every thread of the
// workgroup must call it; every thread receives the same bits.
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double part[kWaves];
    v = wave_sum(v);
    __syncthreads();                                                      // (part may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = part[0];
#pragma unroll
    for (int j = 1; j < kWaves; ++j) s += part[j];
    return s;
}

// The sum of column `col` of partials [nb][2]: a thread adds a contiguous run of workgroups in index order, block_sum adds the threads.
// The same bits in every workgroup of every launch.
__device__ __forceinline__ double total(const double* __restrict__ partials, int nb, int col) {
    const int per = (nb + kBlock - 1) / kBlock;
    const int b0 = min((int)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
    double v = 0.0;
    for (int b = b0; b < b1; ++b) v += partials[2 * (int64_t)b + col];
    return block_sum(v);
}

// C_i t for one vertex: c t (point), c (n (n . t) + share t) (plane).
__device__ __forceinline__ D3 data_term(double c, bool plane, D3 n, double share, D3 t) {
    if (!plane) return {c * t.x, c * t.y, c * t.z};
    const double dn = dot(n, t);
    return {c * (n.x * dn + share * t.x), c * (n.y * dn + share * t.y), c * (n.z * dn + share * t.z)};
}

// ------------------------------------------------------------------ terms of one pairing

struct TermArgs {
    const float* x;              // [V,3] the template
    const float* p;              // [V,3] its current position fl32(x + d)
    const float* q;              // [V,3] closest points
    const float* dist;           // [V]
    const int* face;             // [V]
    int64_t V;
    const float* fnormals;       // [Fb,3] unit face normals of the target, or null
    int Fb;
    const float* snormals;       // [V,3] vertex normals of p on the template's faces (normal_cos), or null
    float thr;
    int plane;
    int use_cos;
    double normal_cos, share;
    const unsigned char* pinned;
    const double* beta;          // [V] landmark weights, or null
    const double* land;          // [V,3] landmark offsets y - x
    double* c;
    double* n;
    double* b;
    double* partial;             // [blocks][2]
};

__global__ __launch_bounds__(kBlock) void terms_kernel(TermArgs u) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double sq = 0.0, cnt = 0.0;
    if (v < u.V) {
        const float d = u.dist[v];
        const int f = u.face[v];
        const bool pin = u.pinned[v] != 0;
        bool ok = isfinite(d) && f >= 0 && d <= u.thr && !pin;
        D3 nf{0.0, 0.0, 0.0};
        if (ok && (u.plane || u.use_cos)) {
            ok = f < u.Fb;
            if (ok) {
                nf = load3(u.fnormals, f);
                ok = finite3(nf) && (nf.x != 0.0 || nf.y != 0.0 || nf.z != 0.0);
            }
        }
        if (ok && u.use_cos) {
            const D3 ns = load3(u.snormals, v);
            ok = finite3(ns) && (ns.x != 0.0 || ns.y != 0.0 || ns.z != 0.0) && dot(ns, nf) >= u.normal_cos;
        }
        const double c = ok ? 1.0 : 0.0;
        const D3 n = (ok && u.plane) ? nf : D3{0.0, 0.0, 0.0};
        D3 b{0.0, 0.0, 0.0};
        if (ok) {
            b = data_term(c, u.plane, n, u.share, sub(load3(u.q, v), load3(u.x, v)));
            const D3 e = sub(load3(u.p, v), load3(u.q, v));
            sq = dot(e, e);
            cnt = 1.0;
        }
        const double bt = (u.beta && !pin) ? u.beta[v] : 0.0;
        if (bt != 0.0) {
            const D3 l = load3(u.land, v);
            b = {b.x + bt * l.x, b.y + bt * l.y, b.z + bt * l.z};
        }
        u.c[v] = c;
        store3(u.n, v, n);
        store3(u.b, v, b);
    }
    sq = block_sum(sq);
    cnt = block_sum(cnt);
    if (threadIdx.x == 0) {
        u.partial[2 * (int64_t)blockIdx.x] = sq;
        u.partial[2 * (int64_t)blockIdx.x + 1] = cnt;
    }
}

__global__ __launch_bounds__(kBlock) void terms_final_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out) {
    const double sq = total(partial, nb, 0), cnt = total(partial, nb, 1);
    if (threadIdx.x == 0) { out[0] = sq; out[1] = cnt; }
}

struct RhsArgs {
    int64_t V;
    const double* c;
    const double* t;
    const double* n;             // or null (point)
    double share;
    const double* beta;          // or null
    const double* land;
    const unsigned char* pinned;
    double* b;
};

__global__ __launch_bounds__(kBlock) void rhs_kernel(RhsArgs u) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= u.V) return;
    D3 b{0.0, 0.0, 0.0};
    if (!u.pinned[v]) {
        const double c = u.c[v];
        if (c != 0.0) b = data_term(c, u.n != nullptr, u.n ? load3(u.n, v) : D3{0.0, 0.0, 0.0}, u.share, load3(u.t, v));
        const double bt = u.beta ? u.beta[v] : 0.0;
        if (bt != 0.0) {
            const D3 l = load3(u.land, v);
            b = {b.x + bt * l.x, b.y + bt * l.y, b.z + bt * l.z};
        }
    }
    store3(u.b, v, b);
}

// ------------------------------------------------------------------ the operator

struct Op {
    int64_t V, E;
    const int* offsets;
    const int* neighbors;
    const double* c;
    const double* n;             // or null (point)
    const double* beta;          // or null
    const unsigned char* pinned;
    double a, share;
    const int* heavy;
    int n_heavy;
};

// The CSR row of v, clamped to the arrays.
__device__ __forceinline__ void row_of(const Op& u, int64_t v, int& e0, int& e1) {
    e0 = max(u.offsets[v], 0);
    e1 = (int)min((int64_t)u.offsets[v + 1], u.E);
}

// Neighbour sums of the heavy vertices into out (apply_kernel reads them there): one wave per vertex.
__global__ __launch_bounds__(64) void heavy_kernel(Op u, const double* __restrict__ in, double* __restrict__ out, const double* __restrict__ slot) {
    if (slot && slot[2] != 0.0) return;
    const int lane = threadIdx.x;
    for (int h = blockIdx.x; h < u.n_heavy; h += gridDim.x) {
        const int64_t v = u.heavy[h];
        if ((uint64_t)v >= (uint64_t)u.V || u.pinned[v]) continue;
        int e0, e1;
        row_of(u, v, e0, e1);
        D3 s{0.0, 0.0, 0.0};
        for (int e = e0 + lane; e < e1; e += 64) {
            const int64_t j = u.neighbors[e];
            if ((uint64_t)j >= (uint64_t)u.V) continue;
            const D3 q = load3(in, j);
            s.x += q.x; s.y += q.y; s.z += q.z;
        }
        s.x = wave_sum(s.x); s.y = wave_sum(s.y); s.z = wave_sum(s.z);
        if (lane == 0) store3(out, v, s);
    }
}

// out = A in; partial[blk] = (in . out, b . in if WithB).
template <bool WithB>
__global__ __launch_bounds__(kBlock) void apply_kernel(Op u, const double* __restrict__ in, double* __restrict__ out, const double* __restrict__ b,
                                                       double* __restrict__ partial, const double* __restrict__ slot) {
    if (slot && slot[2] != 0.0) return;                                   // frozen (uniform over the launch)
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double d0 = 0.0, d1 = 0.0;
    if (v < u.V) {
        D3 y{0.0, 0.0, 0.0};
        if (!u.pinned[v]) {
            const D3 x = load3(in, v);
            int e0, e1;
            row_of(u, v, e0, e1);
            D3 s{0.0, 0.0, 0.0};
            if (e1 - e0 > kHeavy) {
                s = load3(out, v);                                        // heavy_kernel's
            } else {
                for (int e = e0; e < e1; ++e) {
                    const int64_t j = u.neighbors[e];
                    if ((uint64_t)j >= (uint64_t)u.V) continue;
                    const D3 q = load3(in, j);
                    s.x += q.x; s.y += q.y; s.z += q.z;
                }
            }
            const double deg = (double)(e1 > e0 ? e1 - e0 : 0);
            const D3 cx = data_term(u.c[v], u.n != nullptr, u.n ? load3(u.n, v) : D3{0.0, 0.0, 0.0}, u.share, x);
            const double bt = u.beta ? u.beta[v] : 0.0;
            y = {(cx.x + u.a * (deg * x.x - s.x)) + bt * x.x, (cx.y + u.a * (deg * x.y - s.y)) + bt * x.y,
                 (cx.z + u.a * (deg * x.z - s.z)) + bt * x.z};
            d0 = dot(x, y);
            if (WithB) d1 = dot(load3(b, v), x);
        }
        store3(out, v, y);
    }
    d0 = block_sum(d0);
    if (WithB) d1 = block_sum(d1);
    if (threadIdx.x == 0) {
        partial[2 * (int64_t)blockIdx.x] = d0;
        partial[2 * (int64_t)blockIdx.x + 1] = d1;
    }
}

// ------------------------------------------------------------------ conjugate gradients

struct Cg {
    int64_t V;
    int nb;
    const unsigned char* pinned;
    const double* b;
    double* x;
    double* ap;
    double* r;
    double* p;
    double* pa;                  // [nb][2] partials of the apply launches
    double* pb;                  // [nb][2] partials of |r|^2 (and |b|^2 at the start)
    double* state;               // [2][kState]
    double tol2;
    double* out;                 // [kOut]
};

// r = b - A x0, p = r; partials of |r|^2 and |b|^2.
__global__ __launch_bounds__(kBlock) void start_kernel(Cg g) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double rr = 0.0, bb = 0.0;
    if (v < g.V) {
        D3 r{0.0, 0.0, 0.0};
        if (!g.pinned[v]) {
            const D3 b = load3(g.b, v);
            r = sub(b, load3(g.ap, v));
            rr = dot(r, r);
            bb = dot(b, b);
        }
        store3(g.r, v, r);
        store3(g.p, v, r);
    }
    rr = block_sum(rr);
    bb = block_sum(bb);
    if (threadIdx.x == 0) {
        g.pb[2 * (int64_t)blockIdx.x] = rr;
        g.pb[2 * (int64_t)blockIdx.x + 1] = bb;
    }
}

__device__ __forceinline__ bool frozen_at(double rr, double bb, double tol2) { return !isfinite(rr) || !isfinite(bb) || rr <= tol2 * bb; }

// One workgroup.  end == 0: the scalars of step 0 and the energy of x0.  end == 1: the energy of x and the results, from slot `at`.
__global__ __launch_bounds__(kBlock) void scalars_kernel(Cg g, int end, int at) {
    const double xax = total(g.pa, g.nb, 0), bx = total(g.pa, g.nb, 1);
    if (!end) {
        const double rr = total(g.pb, g.nb, 0), bb = total(g.pb, g.nb, 1);
        if (threadIdx.x == 0) {
            g.state[0] = rr; g.state[1] = bb; g.state[2] = frozen_at(rr, bb, g.tol2) ? 1.0 : 0.0; g.state[3] = 0.0;
            g.out[0] = 0.5 * xax - bx;
        }
        return;
    }
    if (threadIdx.x == 0) {
        const double* s = g.state + kState * at;
        g.out[1] = 0.5 * xax - bx;
        g.out[2] = s[3];
        g.out[3] = s[1] > 0.0 ? sqrt(s[0] / s[1]) : 0.0;
        g.out[4] = s[2];
    }
}

__global__ __launch_bounds__(kBlock) void update_kernel(Cg g, int k) {
    const double* s = g.state + kState * (k & 1);
    if (s[2] != 0.0) return;
    const double pap = total(g.pa, g.nb, 0);
    const double alpha = s[0] / pap;
    if (!(pap > 0.0) || !isfinite(alpha)) return;                         // direction_kernel freezes
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double rr = 0.0;
    if (v < g.V) {
        const D3 p = load3(g.p, v), ap = load3(g.ap, v), x = load3(g.x, v), r0 = load3(g.r, v);
        const D3 r = {r0.x - alpha * ap.x, r0.y - alpha * ap.y, r0.z - alpha * ap.z};
        store3(g.x, v, {x.x + alpha * p.x, x.y + alpha * p.y, x.z + alpha * p.z});
        store3(g.r, v, r);
        rr = dot(r, r);
    }
    rr = block_sum(rr);
    if (threadIdx.x == 0) g.pb[2 * (int64_t)blockIdx.x] = rr;
}

__global__ __launch_bounds__(kBlock) void direction_kernel(Cg g, int k) {
    const double* s = g.state + kState * (k & 1);
    double* nxt = g.state + kState * ((k + 1) & 1);
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (s[2] != 0.0) {
        if (first) { nxt[0] = s[0]; nxt[1] = s[1]; nxt[2] = 1.0; nxt[3] = s[3]; }
        return;
    }
    const double pap = total(g.pa, g.nb, 0);
    const double alpha = s[0] / pap;
    if (!(pap > 0.0) || !isfinite(alpha)) {
        if (first) { nxt[0] = s[0]; nxt[1] = s[1]; nxt[2] = 1.0; nxt[3] = s[3]; }
        return;
    }
    const double rr = total(g.pb, g.nb, 0);
    const double beta = rr / s[0];
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v < g.V) {
        const D3 r = load3(g.r, v), p = load3(g.p, v);
        store3(g.p, v, {r.x + beta * p.x, r.y + beta * p.y, r.z + beta * p.z});
    }
    if (first) { nxt[0] = rr; nxt[1] = s[1]; nxt[2] = frozen_at(rr, s[1], g.tol2) ? 1.0 : 0.0; nxt[3] = s[3] + 1.0; }
}

// ------------------------------------------------------------------ verts = fl32(x + d)

__global__ __launch_bounds__(kBlock) void moved_kernel(const float* __restrict__ x, const double* __restrict__ d, const unsigned char* __restrict__ pinned,
                                                       int64_t n3, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n3) return;
    const double di = d[i];
    out[i] = (pinned[i / 3] || di == 0.0) ? x[i] : (float)((double)x[i] + di);
}

size_t align8(size_t n) { return (n + 7) & ~(size_t)7; }

struct Layout { size_t ap, r, p, pa, pb, state, bytes; int nb; };

Layout layout(int64_t V) {
    Layout l;
    l.nb = (int)blocks(V, kBlock);
    const size_t vec = sizeof(double) * 3 * (size_t)(V < 1 ? 1 : V), par = sizeof(double) * 2 * (size_t)l.nb;
    l.ap = 0; l.r = vec; l.p = 2 * vec; l.pa = 3 * vec; l.pb = l.pa + par; l.state = l.pb + par;
    l.bytes = align8(l.state + sizeof(double) * 2 * kState);
    return l;
}

}  // namespace

extern "C" int ia_nonrigid_terms_scratch_bytes(int64_t V, size_t* h_bytes) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount, "ia_nonrigid_terms_scratch_bytes: V must be in [0, 2^28], got %lld", (long long)V);
    IA_REQUIRE(h_bytes, "ia_nonrigid_terms_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = sizeof(double) * 2 * (size_t)blocks(V, kBlock);
    return IA_OK;
}

extern "C" int ia_nonrigid_terms(const float* x, const float* p, const float* q, const float* dist, const int* face, int64_t V,
                                 const float* face_normals, int64_t Fb, const float* source_normals, float h_max_dist, int mode, int use_cos,
                                 double normal_cos, double point_share, const unsigned char* pinned, const double* beta, const double* land,
                                 double* c, double* n, double* b, void* scratch, size_t scratch_bytes, double* out, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount, "ia_nonrigid_terms: V must be in [0, 2^28], got %lld", (long long)V);
    IA_REQUIRE(mode == 0 || mode == 1, "ia_nonrigid_terms: mode must be 0 (point) or 1 (plane), got %d", mode);
    IA_REQUIRE(Fb >= 0 && Fb < ((int64_t)1 << 31) / 3, "ia_nonrigid_terms: Fb must be >= 0 and 3 Fb < 2^31, got %lld", (long long)Fb);
    IA_REQUIRE(!std::isnan(h_max_dist), "ia_nonrigid_terms: h_max_dist must not be NaN (+inf: no threshold)");
    IA_REQUIRE(!use_cos || std::isfinite(normal_cos), "ia_nonrigid_terms: normal_cos must be finite");
    IA_REQUIRE(!mode || (std::isfinite(point_share) && point_share > 0.0), "ia_nonrigid_terms: point_share must be > 0 for the plane metric");
    const int nb = (int)blocks(V, kBlock);
    const size_t need = sizeof(double) * 2 * (size_t)nb;
    if (scratch_bytes < need) return ia::fail(IA_ERR_INVALID_ARG, "ia_nonrigid_terms: scratch holds %zu bytes, needs %zu", scratch_bytes, need);
    if (!on_device(scratch) || !on_device(out)) return ia::fail(IA_ERR_INVALID_ARG, "ia_nonrigid_terms: scratch and out must be device pointers");
    if (V && (!on_device(x) || !on_device(p) || !on_device(q) || !on_device(dist) || !on_device(face) || !on_device(pinned) || !on_device(c) ||
              !on_device(n) || !on_device(b)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_nonrigid_terms: x, p, q, dist, face, pinned, c, n and b must be device pointers");
    if (V && (mode || use_cos) && Fb && !on_device(face_normals))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_nonrigid_terms: face_normals must be a device pointer for the plane metric and for normal_cos");
    if (V && use_cos && !on_device(source_normals))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_nonrigid_terms: source_normals must be a device pointer with normal_cos");
    if (V && beta && (!on_device(beta) || !on_device(land)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_nonrigid_terms: beta and land must both be device pointers");
    TermArgs u{};
    u.x = x; u.p = p; u.q = q; u.dist = dist; u.face = face; u.V = V;
    u.fnormals = face_normals; u.Fb = (int)Fb; u.snormals = source_normals;
    u.thr = h_max_dist; u.plane = mode; u.use_cos = use_cos ? 1 : 0; u.normal_cos = normal_cos; u.share = point_share;
    u.pinned = pinned; u.beta = beta; u.land = land;
    u.c = c; u.n = n; u.b = b; u.partial = static_cast<double*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    terms_kernel<<<nb, kBlock, 0, s>>>(u);
    if (int st = ia::check_launch("ia_nonrigid_terms")) return st;
    terms_final_kernel<<<1, kBlock, 0, s>>>(u.partial, nb, out);
    return ia::check_launch("ia_nonrigid_terms (final)");
}

extern "C" int ia_nonrigid_rhs(int64_t V, const double* c, const double* t, const double* n, double point_share, const double* beta,
                               const double* land, const unsigned char* pinned, double* b, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount, "ia_nonrigid_rhs: V must be in [0, 2^28], got %lld", (long long)V);
    IA_REQUIRE(!n || (std::isfinite(point_share) && point_share > 0.0), "ia_nonrigid_rhs: point_share must be > 0 for the plane metric");
    if (V == 0) return IA_OK;
    if (!on_device(c) || !on_device(t) || !on_device(pinned) || !on_device(b) || (n && !on_device(n)) || (beta && (!on_device(beta) || !on_device(land))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_nonrigid_rhs: every array must be a device pointer");
    RhsArgs u{V, c, t, n, point_share, beta, land, pinned, b};
    rhs_kernel<<<blocks(V, kBlock), kBlock, 0, (hipStream_t)stream>>>(u);
    return ia::check_launch("ia_nonrigid_rhs");
}

extern "C" int ia_nonrigid_solve_scratch_bytes(int64_t V, size_t* h_bytes) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount, "ia_nonrigid_solve_scratch_bytes: V must be in [0, 2^28], got %lld", (long long)V);
    IA_REQUIRE(h_bytes, "ia_nonrigid_solve_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = layout(V).bytes;
    return IA_OK;
}

extern "C" int ia_nonrigid_solve(int64_t V, const int* offsets, const int* neighbors, int64_t E, const int* heavy, int n_heavy, const double* c,
                                 const double* n, const double* beta, const unsigned char* pinned, const double* b, double stiffness,
                                 double point_share, double* x, int cg_iterations, double cg_tol, void* scratch, size_t scratch_bytes,
                                 double* out, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount && E >= 0 && E < ((int64_t)1 << 31) && n_heavy >= 0 && n_heavy <= V,
               "ia_nonrigid_solve: V in [0, 2^28], 0 <= E < 2^31, 0 <= n_heavy <= V");
    IA_REQUIRE(cg_iterations >= 1 && cg_iterations <= 1000000, "ia_nonrigid_solve: cg_iterations must be in [1, 10^6], got %d", cg_iterations);
    IA_REQUIRE(std::isfinite(stiffness) && stiffness >= 0.0, "ia_nonrigid_solve: stiffness must be finite and >= 0");
    IA_REQUIRE(std::isfinite(cg_tol) && cg_tol >= 0.0, "ia_nonrigid_solve: cg_tol must be finite and >= 0");
    IA_REQUIRE(!n || (std::isfinite(point_share) && point_share > 0.0), "ia_nonrigid_solve: point_share must be > 0 for the plane metric");
    const Layout l = layout(V);
    if (scratch_bytes < l.bytes) return ia::fail(IA_ERR_INVALID_ARG, "ia_nonrigid_solve: scratch holds %zu bytes, needs %zu", scratch_bytes, l.bytes);
    if (!on_device(scratch) || !on_device(out)) return ia::fail(IA_ERR_INVALID_ARG, "ia_nonrigid_solve: scratch and out must be device pointers");
    if (V && (!on_device(offsets) || !on_device(c) || !on_device(pinned) || !on_device(b) || !on_device(x) || (n && !on_device(n)) ||
              (beta && !on_device(beta)) || (E && !on_device(neighbors)) || (n_heavy && !on_device(heavy))))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_nonrigid_solve: every array must be a device pointer");
    char* base = static_cast<char*>(scratch);
    Op u{V, E, offsets, neighbors, c, n, beta, pinned, stiffness, point_share, heavy, n_heavy};
    Cg g{};
    g.V = V; g.nb = l.nb; g.pinned = pinned; g.b = b; g.x = x;
    g.ap = reinterpret_cast<double*>(base + l.ap); g.r = reinterpret_cast<double*>(base + l.r); g.p = reinterpret_cast<double*>(base + l.p);
    g.pa = reinterpret_cast<double*>(base + l.pa); g.pb = reinterpret_cast<double*>(base + l.pb);
    g.state = reinterpret_cast<double*>(base + l.state);
    g.tol2 = cg_tol * cg_tol; g.out = out;
    hipStream_t s = (hipStream_t)stream;
    const unsigned hb = (unsigned)std::min(n_heavy, 4096);
    // A x0 (with x0 . A x0 and b . x0), r = p = b - A x0, the scalars of step 0
    if (n_heavy) heavy_kernel<<<hb, 64, 0, s>>>(u, x, g.ap, nullptr);
    apply_kernel<true><<<l.nb, kBlock, 0, s>>>(u, x, g.ap, b, g.pa, nullptr);
    if (int st = ia::check_launch("ia_nonrigid_solve (start)")) return st;
    start_kernel<<<l.nb, kBlock, 0, s>>>(g);
    scalars_kernel<<<1, kBlock, 0, s>>>(g, 0, 0);
    if (int st = ia::check_launch("ia_nonrigid_solve (scalars)")) return st;
    for (int k = 0; k < cg_iterations; ++k) {
        const double* slot = g.state + kState * (k & 1);
        if (n_heavy) heavy_kernel<<<hb, 64, 0, s>>>(u, g.p, g.ap, slot);
        apply_kernel<false><<<l.nb, kBlock, 0, s>>>(u, g.p, g.ap, b, g.pa, slot);
        update_kernel<<<l.nb, kBlock, 0, s>>>(g, k);
        direction_kernel<<<l.nb, kBlock, 0, s>>>(g, k);
        if (int st = ia::check_launch("ia_nonrigid_solve (step)")) return st;
    }
    // the energy of the result
    if (n_heavy) heavy_kernel<<<hb, 64, 0, s>>>(u, x, g.ap, nullptr);
    apply_kernel<true><<<l.nb, kBlock, 0, s>>>(u, x, g.ap, b, g.pa, nullptr);
    scalars_kernel<<<1, kBlock, 0, s>>>(g, 1, cg_iterations & 1);
    return ia::check_launch("ia_nonrigid_solve (end)");
}

extern "C" int ia_nonrigid_apply(const float* x, const double* d, const unsigned char* pinned, int64_t V, float* verts, void* stream) {
    IA_REQUIRE(V >= 0 && V <= kMaxCount, "ia_nonrigid_apply: V must be in [0, 2^28], got %lld", (long long)V);
    if (V == 0) return IA_OK;
    if (!on_device(x) || !on_device(d) || !on_device(pinned) || !on_device(verts))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_nonrigid_apply: every array must be a device pointer");
    moved_kernel<<<blocks(3 * V, kBlock), kBlock, 0, (hipStream_t)stream>>>(x, d, pinned, 3 * V, verts);
    return ia::check_launch("ia_nonrigid_apply");
}
