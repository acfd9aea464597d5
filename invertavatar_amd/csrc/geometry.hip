// Avatar geometry on the device: tri-plane point queries, lattice density volumes and marching cubes.
//
// ia_query_planes / ia_density_grid replace the point query of the reference's TriPlaneGenerator.sample / sample_mixed
// (triplane_v20.py:341-402: renderer.run_model = sample_from_planes (grid_sample) + OSGDecoder) and the chunked lattice helpers of
// inversion/model_utils.py:90-165.  One thread per point: the grid_sample-faithful gather of the three planes (the gather_features idea
// of render_rays.hip: bilinear, zero padding, align_corners=False, mean over the planes), then both decoder layers as fp32 VALU FMA
// chains on weights staged in LDS (pre-multiplied by the FullyConnectedLayer gains) once per persistent workgroup.  No fp16 operands: the
// volume feeds a threshold.  Density-only calls skip the 32 colour rows of layer 2.  ia_density_grid generates its lattice coordinates
// itself and walks the lattice in 4 x 8 x 8 tiles (one wave = one x-slice of 8 x 8 points), so that neighbouring lanes read
// neighbouring texels of all three planes.
//
// ia_mc_count / ia_mc_emit: marching cubes (no counterpart in the reference).  A lattice point owns the up to three lattice edges that
// leave it toward +x, +y, +z, and the cell whose lower corner it is.  Every launch walks the points in chunks of 1024 consecutive linear
// indices (256 threads x 4 points), so chunk order = point order = cell order:
//   count : per-chunk vertex and triangle counts -> scratch; one single-workgroup scan turns them into exclusive chunk offsets and
//           writes the two totals;
//   emit  : (1) recounts each chunk's vertices, scans them in the workgroup, writes the vertices and the first vertex id of every point
//               (vbase, 4 bytes per point) -- vertex order = (owner point, axis x < y < z);
//           (2) recounts each chunk's cells and writes their triangles at the scanned offsets, in table order (mc_tables.h), looking the
//               vertex ids of the cell's edges up in vbase.
// No atomics: the output is a function of the volume alone, bit for bit.  Every output write is checked against the caller's capacity.
#include "geom_common.h"

#define IA_MC_TABLE_QUALIFIER static __constant__ const
#include "mc_tables.h"

namespace {

using ia::block_scan; using ia::check_volume; using ia::kScanBlock; using ia::on_device; using ia::streaming_grid;

constexpr int kBlock = 256;
constexpr int kHidden = 64;
constexpr int kFeat = 32;
constexpr int kOut = 33;
constexpr int kW2Stride = 36;          // W2^T rows padded to 16-byte multiples

struct alignas(16) DecoderLds {
    float w1[kHidden][kFeat];          // layer 1 weights * lr_mul / sqrt(32), row = hidden unit
    float b1[kHidden];
    float w2t[kHidden][kW2Stride];     // layer 2 weights * lr_mul / sqrt(64), transposed: row = hidden unit, column = output
    float b2[kW2Stride];
};

struct DecoderArgs {
    const float *w0, *b0, *w1, *b1;
    float g0, g1, lr;                  // weight gains of both layers, bias gain
};

__device__ void stage_decoder(DecoderLds& L, const DecoderArgs& a) {
    for (int i = threadIdx.x; i < kHidden * kFeat; i += blockDim.x) L.w1[i / kFeat][i % kFeat] = __fmul_rn(a.w0[i], a.g0);
    for (int i = threadIdx.x; i < kHidden; i += blockDim.x) L.b1[i] = __fmul_rn(a.b0[i], a.lr);
    for (int i = threadIdx.x; i < kOut * kHidden; i += blockDim.x) L.w2t[i % kHidden][i / kHidden] = __fmul_rn(a.w1[i], a.g1);
    for (int i = threadIdx.x; i < kOut; i += blockDim.x) L.b2[i] = __fmul_rn(a.b1[i], a.lr);
    __syncthreads();
}

// The 32 averaged features at one point (already flipped and scaled by 2 / box_warp): sample_from_planes + the mean of OSGDecoder.
// Taps outside a plane read a clamped, valid texel with weight 0 (fmaf(v, 0, acc) == acc for finite planes).
__device__ __forceinline__ void gather32(const float* __restrict__ planes_b, int PH, int PW, float x, float y, float z, float (&f)[kFeat]) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const float gx = (p == 2) ? z : x;
        const float gy = (p == 0) ? y : (p == 1 ? z : x);
        const float ix = (gx + 1.f) * (0.5f * (float)PW) - 0.5f;
        const float iy = (gy + 1.f) * (0.5f * (float)PH) - 0.5f;
        const float x0f = floorf(ix), y0f = floorf(iy);
        const float fx = ix - x0f, fy = iy - y0f;
        // clamp before the int conversion so far-away points cannot overflow (NaN -> -2: weight 0 below)
        const int x0 = (int)fminf(fmaxf(x0f, -2.f), (float)PW + 1.f), y0 = (int)fminf(fmaxf(y0f, -2.f), (float)PH + 1.f);
        const int x1 = x0 + 1, y1 = y0 + 1;
        const float wx0 = (unsigned)x0 < (unsigned)PW ? 1.f - fx : 0.f, wx1 = (unsigned)x1 < (unsigned)PW ? fx : 0.f;
        const float wy0 = (unsigned)y0 < (unsigned)PH ? 1.f - fy : 0.f, wy1 = (unsigned)y1 < (unsigned)PH ? fy : 0.f;
        const int xc[2] = {min(max(x0, 0), PW - 1), min(max(x1, 0), PW - 1)};
        const int yc[2] = {min(max(y0, 0), PH - 1), min(max(y1, 0), PH - 1)};
        const float wgt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
        const float* pl = planes_b + (int64_t)p * PH * PW * kFeat;
        float acc[kFeat];
#pragma unroll
        for (int c = 0; c < kFeat; ++c) acc[c] = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float4* src = reinterpret_cast<const float4*>(pl + ((int64_t)yc[t >> 1] * PW + xc[t & 1]) * kFeat);
            const float w = wgt[t];
#pragma unroll
            for (int q = 0; q < kFeat / 4; ++q) {
                const float4 v = src[q];
                acc[4 * q + 0] = fmaf(v.x, w, acc[4 * q + 0]); acc[4 * q + 1] = fmaf(v.y, w, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(v.z, w, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(v.w, w, acc[4 * q + 3]);
            }
        }
#pragma unroll
        for (int c = 0; c < kFeat; ++c) f[c] = (p == 0) ? acc[c] : f[c] + acc[c];
    }
#pragma unroll
    for (int c = 0; c < kFeat; ++c) f[c] = f[c] * (1.f / 3.f);
}

// torch.nn.Softplus() (beta 1, threshold 20)
__device__ __forceinline__ float softplus20(float x) { return x > 20.f ? x : log1pf(expf(x)); }

// OSGDecoder.forward on one feature vector: sigma = layer-2 row 0; rgb = sigmoid(rows 1..32) * 1.002 - 0.001.
template <bool RGB>
__device__ __forceinline__ void decode(const DecoderLds& L, const float (&f)[kFeat], float& sigma, float (&rgb)[kFeat]) {
    float s = L.b2[0];
    if (RGB) {
#pragma unroll
        for (int c = 0; c < kFeat; ++c) rgb[c] = L.b2[1 + c];
    }
#pragma unroll 2
    for (int j = 0; j < kHidden; ++j) {
        float h = L.b1[j];
#pragma unroll
        for (int k = 0; k < kFeat; ++k) h = fmaf(f[k], L.w1[j][k], h);
        h = softplus20(h);
        s = fmaf(h, L.w2t[j][0], s);
        if (RGB) {
#pragma unroll
            for (int c = 0; c < kFeat; ++c) rgb[c] = fmaf(h, L.w2t[j][1 + c], rgb[c]);
        }
    }
    sigma = s;
    if (RGB) {
#pragma unroll
        for (int c = 0; c < kFeat; ++c) rgb[c] = __fsub_rn(__fmul_rn(1.f / (1.f + expf(-rgb[c])), 1.002f), 0.001f);
    }
}

// One point in world coordinates: flip z, scale by 2 / box_warp, gather, decode.  Shared by both query kernels, so that the lattice
// volume is bit for bit the point query at the same fp32 coordinates.
template <bool RGB>
__device__ __forceinline__ void query_point(const DecoderLds& L, const float* __restrict__ planes_b, int PH, int PW, float scale, bool flip,
                                            float x, float y, float z, float& sigma, float (&rgb)[kFeat]) {
    if (flip) z = -z;
    float f[kFeat];
    gather32(planes_b, PH, PW, x * scale, y * scale, z * scale, f);
    decode<RGB>(L, f, sigma, rgb);
}

template <bool RGB>
__global__ __launch_bounds__(kBlock) void query_planes_kernel(const float* __restrict__ planes, const float* __restrict__ pts, DecoderArgs da,
                                                               float scale, int flip, int B, int M, int PH, int PW,
                                                               float* __restrict__ sigma, float* __restrict__ rgb) {
    __shared__ DecoderLds L;
    stage_decoder(L, da);
    const int64_t total = (int64_t)B * M;
    for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kBlock) {
        const int64_t b = idx / M;
        const float* p = pts + idx * 3;
        float s, col[kFeat];
        query_point<RGB>(L, planes + b * 3 * PH * PW * kFeat, PH, PW, scale, flip != 0, p[0], p[1], p[2], s, col);
        sigma[idx] = s;
        if (RGB) {
            float4* dst = reinterpret_cast<float4*>(rgb + idx * kFeat);
#pragma unroll
            for (int q = 0; q < kFeat / 4; ++q) dst[q] = make_float4(col[4 * q], col[4 * q + 1], col[4 * q + 2], col[4 * q + 3]);
        }
    }
}

constexpr int kTileX = 4, kTileY = 8, kTileZ = 8;      // 256 points per tile; lane = z + 8 y, wave = x

struct Lattice {
    int nx, ny, nz;
    float lo[3], step[3];                               // point i of axis a = lo[a] + i * step[a] (fp32, each op rounded)
};

__global__ __launch_bounds__(kBlock) void density_grid_kernel(const float* __restrict__ planes, DecoderArgs da, float scale, int flip, int B,
                                                              int PH, int PW, Lattice lat, float* __restrict__ volume) {
    __shared__ DecoderLds L;
    stage_decoder(L, da);
    const int tx = (lat.nx + kTileX - 1) / kTileX, ty = (lat.ny + kTileY - 1) / kTileY, tz = (lat.nz + kTileZ - 1) / kTileZ;
    const int64_t per_b = (int64_t)tx * ty * tz, total = per_b * B;
    const int lz = threadIdx.x & 7, ly = (threadIdx.x >> 3) & 7, lx = threadIdx.x >> 6;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const int64_t b = t / per_b;
        const int64_t r = t - b * per_b;
        const int cz = (int)(r % tz), cy = (int)((r / tz) % ty), cx = (int)(r / ((int64_t)tz * ty));
        const int i = cx * kTileX + lx, j = cy * kTileY + ly, k = cz * kTileZ + lz;
        if (i >= lat.nx || j >= lat.ny || k >= lat.nz) continue;
        const float x = __fadd_rn(lat.lo[0], __fmul_rn((float)i, lat.step[0]));
        const float y = __fadd_rn(lat.lo[1], __fmul_rn((float)j, lat.step[1]));
        const float z = __fadd_rn(lat.lo[2], __fmul_rn((float)k, lat.step[2]));
        float s, unused[kFeat];
        query_point<false>(L, planes + b * 3 * PH * PW * kFeat, PH, PW, scale, flip != 0, x, y, z, s, unused);
        volume[((b * lat.nx + i) * lat.ny + j) * (int64_t)lat.nz + k] = s;
    }
}

// ------------------------------------------------------------------ marching cubes

constexpr int kMcPer = 4;                       // consecutive points per thread
constexpr int kMcChunk = kBlock * kMcPer;       // points per workgroup

struct McVol {
    const float* v;
    int nx, ny, nz;
    int64_t S, N;                               // ny * nz, nx * ny * nz
    float level;
};

__device__ __forceinline__ bool is_in(float v, float level) { return v > level; }     // NaN: outside

// Crossing edges of point n = (i, j, k) (bit a: the edge toward +a crosses) and the case index of the cell at n (-1: no cell).
__device__ __forceinline__ void classify(const McVol& m, int64_t n, int i, int j, int k, int& vmask, int& cfg, float (&cv)[8]) {
    const bool hx = i + 1 < m.nx, hy = j + 1 < m.ny, hz = k + 1 < m.nz;
    cv[0] = m.v[n];
    cv[1] = hx ? m.v[n + m.S] : 0.f;
    cv[2] = hy ? m.v[n + m.nz] : 0.f;
    cv[4] = hz ? m.v[n + 1] : 0.f;
    const bool in0 = is_in(cv[0], m.level);
    vmask = (hx && is_in(cv[1], m.level) != in0 ? 1 : 0) | (hy && is_in(cv[2], m.level) != in0 ? 2 : 0) |
            (hz && is_in(cv[4], m.level) != in0 ? 4 : 0);
    cfg = -1;
    if (hx && hy && hz) {
        cv[3] = m.v[n + m.S + m.nz];
        cv[5] = m.v[n + m.S + 1];
        cv[6] = m.v[n + m.nz + 1];
        cv[7] = m.v[n + m.S + m.nz + 1];
        cfg = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) cfg |= is_in(cv[c], m.level) ? (1 << c) : 0;
    }
}

__device__ __forceinline__ void step_point(const McVol& m, int& i, int& j, int& k) {
    if (++k == m.nz) { k = 0; if (++j == m.ny) { j = 0; ++i; } }
}

__global__ __launch_bounds__(kBlock) void mc_count_kernel(McVol m, int* __restrict__ chunk_v, int* __restrict__ chunk_t) {
    const int64_t n0 = (int64_t)blockIdx.x * kMcChunk + (int64_t)threadIdx.x * kMcPer;
    int nv = 0, nt = 0;
    if (n0 < m.N) {
        int i, j, k;
        ia::unravel((int)n0, m.ny, m.nz, i, j, k);
        for (int q = 0; q < kMcPer && n0 + q < m.N; ++q, step_point(m, i, j, k)) {
            int vmask, cfg;
            float cv[8];
            classify(m, n0 + q, i, j, k, vmask, cfg, cv);
            nv += __popc(vmask);
            nt += cfg >= 0 ? (int)ia_mc_tri_count[cfg] : 0;
        }
    }
    int excl, tv, tt;
    block_scan<kBlock>(nv, excl, tv);
    block_scan<kBlock>(nt, excl, tt);
    if (threadIdx.x == 0) { chunk_v[blockIdx.x] = tv; chunk_t[blockIdx.x] = tt; }
}

// One workgroup: chunk counts -> exclusive chunk offsets (in place), totals -> totals[0..1] (-1 where a total exceeds INT32_MAX).
__global__ __launch_bounds__(kScanBlock) void mc_scan_kernel(int* chunk_v, int* chunk_t, int n_chunks, int* __restrict__ totals) {
    const long long tv = ia::scan_workgroup<long long>(chunk_v, chunk_v, n_chunks);      // (an offset wraps only when the total does,
    const long long tt = ia::scan_workgroup<long long>(chunk_t, chunk_t, n_chunks);      //  which the caller sees as -1)
    if (threadIdx.x == 0) {
        totals[0] = tv <= INT32_MAX ? (int)tv : -1;
        totals[1] = tt <= INT32_MAX ? (int)tt : -1;
    }
}

struct McOut {
    float org[3], spc[3];
    int* vbase;
    const int* chunk_v;
    const int* chunk_t;
    float* verts;
    int64_t n_verts;
    int* faces;
    int64_t n_faces;
};

__device__ __forceinline__ float axis_coord(float org, float spc, int i) { return __fadd_rn(org, __fmul_rn((float)i, spc)); }

__global__ __launch_bounds__(kBlock) void mc_emit_verts_kernel(McVol m, McOut o) {
    const int64_t n0 = (int64_t)blockIdx.x * kMcChunk + (int64_t)threadIdx.x * kMcPer;
    int masks[kMcPer] = {0, 0, 0, 0};
    int nv = 0, i = 0, j = 0, k = 0;
    if (n0 < m.N) {
        ia::unravel((int)n0, m.ny, m.nz, i, j, k);
        int ii = i, jj = j, kk = k;
        for (int q = 0; q < kMcPer && n0 + q < m.N; ++q, step_point(m, ii, jj, kk)) {
            int cfg;
            float cv[8];
            classify(m, n0 + q, ii, jj, kk, masks[q], cfg, cv);
            nv += __popc(masks[q]);
        }
    }
    int ea, total;
    block_scan<kBlock>(nv, ea, total);
    if (n0 >= m.N) return;
    int64_t vid = (int64_t)o.chunk_v[blockIdx.x] + ea;
    for (int q = 0; q < kMcPer && n0 + q < m.N; ++q, step_point(m, i, j, k)) {
        const int64_t n = n0 + q;
        o.vbase[n] = (int)vid;
        if (!masks[q]) continue;
        const float v0 = m.v[n];
        const int idx[3] = {i, j, k};
        const int64_t stride[3] = {m.S, (int64_t)m.nz, 1};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(masks[q] >> a & 1)) continue;
            const float v1 = m.v[n + stride[a]];
            float t = __fdiv_rn(__fsub_rn(m.level, v0), __fsub_rn(v1, v0));
            t = fminf(fmaxf(t, 0.f), 1.f);                   // NaN -> 0
            float p[3];
#pragma unroll
            for (int b = 0; b < 3; ++b) p[b] = axis_coord(o.org[b], o.spc[b], idx[b]);
            const float c1 = axis_coord(o.org[a], o.spc[a], idx[a] + 1);
            p[a] = __fadd_rn(p[a], __fmul_rn(t, __fsub_rn(c1, p[a])));
            if (vid >= 0 && vid < o.n_verts) {
                o.verts[vid * 3 + 0] = p[0]; o.verts[vid * 3 + 1] = p[1]; o.verts[vid * 3 + 2] = p[2];
            }
            ++vid;
        }
    }
}

__global__ __launch_bounds__(kBlock) void mc_emit_faces_kernel(McVol m, McOut o) {
    const int64_t n0 = (int64_t)blockIdx.x * kMcChunk + (int64_t)threadIdx.x * kMcPer;
    int nt = 0, i = 0, j = 0, k = 0;
    if (n0 < m.N) {
        ia::unravel((int)n0, m.ny, m.nz, i, j, k);
        int ii = i, jj = j, kk = k;
        for (int q = 0; q < kMcPer && n0 + q < m.N; ++q, step_point(m, ii, jj, kk)) {
            int vmask, cfg;
            float cv[8];
            classify(m, n0 + q, ii, jj, kk, vmask, cfg, cv);
            nt += cfg >= 0 ? (int)ia_mc_tri_count[cfg] : 0;
        }
    }
    int ea, total;
    block_scan<kBlock>(nt, ea, total);
    if (n0 >= m.N) return;
    int64_t fid = (int64_t)o.chunk_t[blockIdx.x] + ea;
    for (int q = 0; q < kMcPer && n0 + q < m.N; ++q, step_point(m, i, j, k)) {
        const int64_t n = n0 + q;
        int vmask, cfg;
        float cv[8];
        classify(m, n, i, j, k, vmask, cfg, cv);
        if (cfg < 0) continue;
        const int cnt = ia_mc_tri_count[cfg];
        for (int tri = 0; tri < cnt; ++tri, ++fid) {
            int ids[3];
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int e = ia_mc_tri_edges[cfg][3 * tri + s];
                const int a = e >> 2, r = e & 3;
                const int b0 = a == 0 ? 1 : 0, b1 = a == 2 ? 1 : 2;           // the other two axes, lower first
                const int c = ((r & 1) << b0) | ((r >> 1) << b1);            // owner corner of the cell
                const int dx = c & 1, dy = (c >> 1) & 1, dz = (c >> 2) & 1;
                const int64_t own = n + dx * m.S + dy * (int64_t)m.nz + dz;
                const bool in_own = is_in(cv[c], m.level);
                int rank = 0;                                                  // crossing edges of the owner before axis a
                if (a > 0) {
                    if (!dx) rank += is_in(cv[c | 1], m.level) != in_own;
                    else if (i + 2 < m.nx) rank += is_in(m.v[own + m.S], m.level) != in_own;
                }
                if (a > 1) {
                    if (!dy) rank += is_in(cv[c | 2], m.level) != in_own;
                    else if (j + 2 < m.ny) rank += is_in(m.v[own + m.nz], m.level) != in_own;
                }
                ids[s] = o.vbase[own] + rank;
            }
            if (fid >= 0 && fid < o.n_faces) {
                o.faces[fid * 3 + 0] = ids[0]; o.faces[fid * 3 + 1] = ids[1]; o.faces[fid * 3 + 2] = ids[2];
            }
        }
    }
}

// ------------------------------------------------------------------ host side

int check_decoder(const float* planes_cl, const float* w0, const float* b0, const float* w1, const float* b1, int B, int PH, int PW,
                  float box_warp, const char* what) {
    if (!(on_device(planes_cl) && on_device(w0) && on_device(b0) && on_device(w1) && on_device(b1)))
        return ia::fail(IA_ERR_INVALID_ARG, "%s: planes and decoder weights must be device pointers", what);
    if (B < 1 || PH < 1 || PW < 1) return ia::fail(IA_ERR_INVALID_ARG, "%s: bad plane shape B=%d H=%d W=%d", what, B, PH, PW);
    if (!(box_warp > 0.f)) return ia::fail(IA_ERR_INVALID_ARG, "%s: box_warp must be > 0", what);
    return IA_OK;
}

DecoderArgs decoder_args(const float* w0, const float* b0, const float* w1, const float* b1, float lr) {
    return DecoderArgs{w0, b0, w1, b1, (float)((double)lr / sqrt((double)kFeat)), (float)((double)lr / sqrt((double)kHidden)), lr};
}

int64_t n_chunks(int nx, int ny, int nz) { return ia::ceil_div((int64_t)nx * ny * nz, kMcChunk); }

size_t mc_scratch(int nx, int ny, int nz) { return sizeof(int) * ((size_t)nx * ny * nz + 2 * (size_t)n_chunks(nx, ny, nz)); }

McVol mc_vol(const float* v, int nx, int ny, int nz, float level) {
    return McVol{v, nx, ny, nz, (int64_t)ny * nz, (int64_t)nx * ny * nz, level};
}

}  // namespace

extern "C" int ia_query_planes(const float* planes_cl, const float* points, const float* w0, const float* b0, const float* w1,
                               const float* b1, float lr_multiplier, float box_warp, int flags, int B, int M, int plane_h, int plane_w,
                               float* sigma, float* rgb, void* stream) {
    if (int st = check_decoder(planes_cl, w0, b0, w1, b1, B, plane_h, plane_w, box_warp, "ia_query_planes")) return st;
    IA_REQUIRE(M >= 0, "ia_query_planes: M must be >= 0");
    if (M == 0) return IA_OK;
    if (!on_device(points) || !on_device(sigma) || (rgb && !on_device(rgb)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_query_planes: points, sigma and rgb must be device pointers");
    const DecoderArgs da = decoder_args(w0, b0, w1, b1, lr_multiplier);
    const float scale = (float)(2.0 / (double)box_warp);
    const int flip = (flags & IA_GEOM_FLIP_Z) ? 1 : 0;
    const int grid = streaming_grid((int64_t)B * M, kBlock);
    hipStream_t s = (hipStream_t)stream;
    if (rgb)
        query_planes_kernel<true><<<grid, kBlock, 0, s>>>(planes_cl, points, da, scale, flip, B, M, plane_h, plane_w, sigma, rgb);
    else
        query_planes_kernel<false><<<grid, kBlock, 0, s>>>(planes_cl, points, da, scale, flip, B, M, plane_h, plane_w, sigma, nullptr);
    return ia::check_launch("ia_query_planes");
}

extern "C" int ia_density_grid(const float* planes_cl, const float* w0, const float* b0, const float* w1, const float* b1,
                               float lr_multiplier, float box_warp, int flags, int B, int plane_h, int plane_w, int nx, int ny, int nz,
                               const float* h_cube_length, const float* h_origin, float* volume, void* stream) {
    if (int st = check_decoder(planes_cl, w0, b0, w1, b1, B, plane_h, plane_w, box_warp, "ia_density_grid")) return st;
    if (int st = check_volume(nx, ny, nz, "ia_density_grid")) return st;
    IA_REQUIRE(h_cube_length && h_origin, "ia_density_grid: h_cube_length and h_origin must be host arrays of 3 floats");
    if (!on_device(volume)) return ia::fail(IA_ERR_INVALID_ARG, "ia_density_grid: volume must be a device pointer");
    Lattice lat{nx, ny, nz, {}, {}};
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        const float L = h_cube_length[a];
        lat.lo[a] = h_origin[a] - 0.5f * L;                        // fp32, each operation rounded (built with -ffp-contract=off)
        lat.step[a] = L / (float)(n[a] - 1);
    }
    const DecoderArgs da = decoder_args(w0, b0, w1, b1, lr_multiplier);
    const int64_t tiles = ia::ceil_div(nx, kTileX) * ia::ceil_div(ny, kTileY) * ia::ceil_div(nz, kTileZ) * B;
    const int grid = streaming_grid(tiles, 1);
    density_grid_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(planes_cl, da, (float)(2.0 / (double)box_warp),
                                                                 (flags & IA_GEOM_FLIP_Z) ? 1 : 0, B, plane_h, plane_w, lat, volume);
    return ia::check_launch("ia_density_grid");
}

extern "C" int ia_mc_scratch_bytes(int nx, int ny, int nz, size_t* h_bytes) {
    if (int st = check_volume(nx, ny, nz, "ia_mc_scratch_bytes")) return st;
    IA_REQUIRE(h_bytes, "ia_mc_scratch_bytes: h_bytes must not be NULL");
    *h_bytes = mc_scratch(nx, ny, nz);
    return IA_OK;
}

extern "C" int ia_mc_count(const float* volume, int nx, int ny, int nz, float level, void* scratch, size_t scratch_bytes, int* totals,
                           void* stream) {
    if (int st = check_volume(nx, ny, nz, "ia_mc_count")) return st;
    if (!on_device(volume) || !on_device(scratch) || !on_device(totals))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mc_count: volume, scratch and totals must be device pointers");
    if (scratch_bytes < mc_scratch(nx, ny, nz))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mc_count: scratch holds %zu bytes, needs %zu", scratch_bytes, mc_scratch(nx, ny, nz));
    const McVol m = mc_vol(volume, nx, ny, nz, level);
    const int64_t nc = n_chunks(nx, ny, nz);
    int* chunk_v = static_cast<int*>(scratch) + m.N;
    int* chunk_t = chunk_v + nc;
    hipStream_t s = (hipStream_t)stream;
    mc_count_kernel<<<(unsigned)nc, kBlock, 0, s>>>(m, chunk_v, chunk_t);
    if (int st = ia::check_launch("ia_mc_count")) return st;
    mc_scan_kernel<<<1, kScanBlock, 0, s>>>(chunk_v, chunk_t, (int)nc, totals);
    return ia::check_launch("ia_mc_count (scan)");
}

extern "C" int ia_mc_emit(const float* volume, int nx, int ny, int nz, float level, const float* h_origin, const float* h_spacing,
                          void* scratch, size_t scratch_bytes, float* verts, int64_t n_verts, int* faces, int64_t n_faces, void* stream) {
    if (int st = check_volume(nx, ny, nz, "ia_mc_emit")) return st;
    IA_REQUIRE(h_origin && h_spacing, "ia_mc_emit: h_origin and h_spacing must be host arrays of 3 floats");
    IA_REQUIRE(n_verts >= 0 && n_faces >= 0, "ia_mc_emit: negative output size (the totals of ia_mc_count overflowed int32)");
    if (!on_device(volume) || !on_device(scratch) || (n_verts && !on_device(verts)) || (n_faces && !on_device(faces)))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mc_emit: volume, scratch, verts and faces must be device pointers");
    if (scratch_bytes < mc_scratch(nx, ny, nz))
        return ia::fail(IA_ERR_INVALID_ARG, "ia_mc_emit: scratch holds %zu bytes, needs %zu", scratch_bytes, mc_scratch(nx, ny, nz));
    const McVol m = mc_vol(volume, nx, ny, nz, level);
    const int64_t nc = n_chunks(nx, ny, nz);
    McOut o{};
    for (int a = 0; a < 3; ++a) { o.org[a] = h_origin[a]; o.spc[a] = h_spacing[a]; }
    o.vbase = static_cast<int*>(scratch);
    o.chunk_v = o.vbase + m.N;
    o.chunk_t = o.chunk_v + nc;
    o.verts = verts; o.n_verts = n_verts; o.faces = faces; o.n_faces = n_faces;
    hipStream_t s = (hipStream_t)stream;
    mc_emit_verts_kernel<<<(unsigned)nc, kBlock, 0, s>>>(m, o);
    if (int st = ia::check_launch("ia_mc_emit (vertices)")) return st;
    mc_emit_faces_kernel<<<(unsigned)nc, kBlock, 0, s>>>(m, o);
    return ia::check_launch("ia_mc_emit (faces)");
}
