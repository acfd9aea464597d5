"""Avatar geometry: tri-plane point queries, density volumes on a lattice, marching-cubes meshes and PLY output.

The reference offers the pieces (``TriPlaneGenerator.sample`` / ``sample_mixed``, triplane_v20.py:341-402, and the lattice + chunked
query helpers of inversion/model_utils.py:90-165), not the tool.  Here:

- ``query_planes``: density (and colour features) of the decoder at points, from planes the generator has already made.  Device tensors
  go to ``ia_query_planes`` (gather + both decoder layers in one launch, fp32); CPU tensors take the renderer's torch formulation
  (``run_model``: ``grid_sample`` + ``OSGDecoder``).
- ``density_volume``: the density on a lattice.  Device tensors go to ``ia_density_grid``, which generates the lattice coordinates itself
  (no ``[N^3, 3]`` tensor); CPU tensors query ``lattice_points`` in chunks.
- ``marching_cubes``: an indexed, welded, outward-wound triangle mesh of ``{volume > level}``.  Device tensors go to ``ia_mc_count`` +
  ``ia_mc_emit`` (one host read of the two totals in between); CPU tensors and NumPy arrays take a vectorised NumPy restatement of the
  same algorithm (same table, same vertex and triangle order, same fp32 vertex arithmetic).
- ``raycast``: first hit of rays with the surface of the trilinear field, with depth and normals.  Device tensors go to
  ``ia_volume_bricks`` + ``ia_raycast_volume``; CPU tensors and NumPy arrays take a vectorised NumPy restatement (float64) of the same
  algorithm.  ``volume_normals`` (``ia_volume_gradient``): unit normals at points, e.g. the mesh vertices; ``shade``: headlight Lambert.
- ``write_ply`` / ``read_ply``: binary little-endian PLY in NumPy (optionally with vertex normals).

Lattice (used by the kernel, ``lattice_points`` and the mesh coordinates alike): point ``(i, j, k)`` of an ``nx x ny x nz`` lattice is, per
axis and in fp32 with every operation rounded on its own, ``lo + i * step`` with ``lo = origin - 0.5 * L`` and ``step = L / (n - 1)``,
i.e. ``origin - L/2 + i * L/(n-1)``: the lattice spans ``[origin - L/2, origin + L/2]`` end points included.  Volumes are indexed
``[i, j, k]`` with x slowest and z fastest (C order, the layout of the reference's ``create_samples``).  Unlike ``create_samples``, whose
``(idx.float() / N) % N`` is not floored and so shifts y by z/N of a voxel, every point here lies on the lattice.

Marching cubes: a lattice point is inside iff ``v > level`` (NaN is outside).  One vertex per lattice edge whose ends are on different sides,
owned by its lower endpoint, ordered by the owner's linear index and then axis x < y < z, at ``p0 + t * (p1 - p0)`` with
``t = (level - v0) / (v1 - v0)`` clamped to [0, 1] (a NaN ``t`` counts as 0).  Triangles are ordered by cell and then by table order
(invertavatar_amd/mc_table.py, which also fixes the rule on ambiguous faces); normals point toward decreasing density.
"""
import numpy as np
import torch

from . import mc_table

F32 = np.float32


def _res3(res):
    r = (int(res),) * 3 if np.isscalar(res) else tuple(int(v) for v in res)
    if len(r) != 3 or min(r) < 2:
        raise ValueError(f'lattice resolution must be >= 2 per axis, got {res}')
    return r


def _vec3(v):
    return (float(v),) * 3 if np.isscalar(v) else tuple(float(x) for x in v)


def lattice_axis(n, length, origin):
    """fp32 coordinates of one lattice axis: ``(origin - 0.5 * L) + i * (L / (n - 1))``, each operation rounded to fp32."""
    lo = F32(origin) - F32(0.5) * F32(length)
    step = F32(length) / F32(n - 1)
    return (lo + np.arange(n, dtype=F32) * step).astype(F32), lo, step


def lattice_points(res, cube_length, origin=(0.0, 0.0, 0.0)):
    """[nx*ny*nz, 3] float32 lattice coordinates, x slowest, z fastest (see the module docstring)."""
    nx, ny, nz = _res3(res)
    ls, org = _vec3(cube_length), _vec3(origin)
    ax = [lattice_axis(n, ls[a], org[a])[0] for a, n in enumerate((nx, ny, nz))]
    g = np.stack(np.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3)
    return torch.from_numpy(np.ascontiguousarray(g))


def _decoder_params(decoder):
    net = decoder.net
    return (net[0].weight.detach().float(), net[0].bias.detach().float(), net[2].weight.detach().float(), net[2].bias.detach().float(),
            float(net[0].bias_gain))


def query_planes(planes, decoder, coords, box_warp, flip_z=False, rgb=True):
    """Decoder output at points: planes [B,3,32,H,W] (the generator's planes), coords [B,M,3] -> {'sigma': [B,M,1], 'rgb': [B,M,32]}
    ('rgb' only with ``rgb=True``).  The semantics of ``renderer.run_model`` + ``OSGDecoder.forward``."""
    if planes.is_cuda:
        from . import hipops
        planes_cl = planes.permute(0, 1, 3, 4, 2)
        if not planes_cl.is_contiguous():
            planes_cl = planes_cl.contiguous()
        w0, b0, w1, b1, lr_mul = _decoder_params(decoder)
        sigma, col = hipops.query_planes(planes_cl, coords.float().contiguous(), w0, b0, w1, b1, lr_multiplier=lr_mul, box_warp=box_warp,
                                         flip_z=flip_z, rgb=rgb)
        return {'sigma': sigma, 'rgb': col} if rgb else {'sigma': sigma}
    from .training_avatar_texture.volumetric_rendering.renderer import generate_planes, sample_from_planes
    coords = coords.float()
    if flip_z:
        coords = coords.clone()
        coords[..., -1] *= -1
    feats = sample_from_planes(generate_planes(), planes, coords, padding_mode='zeros', box_warp=box_warp)
    out = decoder(feats, None)
    return {'sigma': out['sigma'], 'rgb': out['rgb']} if rgb else {'sigma': out['sigma']}


def density_volume(planes, decoder, res, cube_length, origin=(0.0, 0.0, 0.0), box_warp=1.0, flip_z=False, chunk=1 << 18):
    """Density on the lattice: [B, nx, ny, nz] float32 (x slowest).  ``cube_length`` / ``origin``: scalars or per-axis triples."""
    nx, ny, nz = _res3(res)
    ls, org = _vec3(cube_length), _vec3(origin)
    if planes.is_cuda:
        from . import hipops
        planes_cl = planes.permute(0, 1, 3, 4, 2)
        if not planes_cl.is_contiguous():
            planes_cl = planes_cl.contiguous()
        w0, b0, w1, b1, lr_mul = _decoder_params(decoder)
        return hipops.density_grid(planes_cl, w0, b0, w1, b1, (nx, ny, nz), ls, org, lr_multiplier=lr_mul, box_warp=box_warp, flip_z=flip_z)
    pts = lattice_points((nx, ny, nz), ls, org)
    b = planes.shape[0]
    out = torch.empty(b, pts.shape[0])
    for s in range(0, pts.shape[0], chunk):
        q = pts[s:s + chunk].unsqueeze(0).expand(b, -1, -1)
        out[:, s:s + chunk] = query_planes(planes, decoder, q, box_warp, flip_z=flip_z, rgb=False)['sigma'][..., 0]
    return out.reshape(b, nx, ny, nz)


# ------------------------------------------------------------------ marching cubes

def _mc_numpy(v, level, origin, spacing):
    """NumPy restatement of ia_mc_count + ia_mc_emit: (verts float32 [V,3], faces int64 [F,3])."""
    v = np.ascontiguousarray(v, dtype=F32)
    nx, ny, nz = v.shape
    level = F32(level)
    org = np.array(origin, dtype=F32)
    spc = np.array(spacing, dtype=F32)
    inside = v > level
    n = v.size
    cross = np.zeros((nx, ny, nz, 3), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)
    ids = np.flatnonzero(flat)                                    # sorted: owner's linear index, then axis
    vid = np.full(n * 3, -1, dtype=np.int64)
    vid[ids] = np.arange(ids.size, dtype=np.int64)
    owner, axis = ids // 3, ids % 3
    ijk = np.stack(np.unravel_index(owner, (nx, ny, nz)), -1)
    step = np.array([ny * nz, nz, 1], dtype=np.int64)
    v0 = v.reshape(-1)[owner]
    v1 = v.reshape(-1)[owner + step[axis]]
    with np.errstate(divide='ignore', invalid='ignore'):
        t = (level - v0) / (v1 - v0)
    t = np.fmin(np.fmax(t, F32(0)), F32(1)).astype(F32)          # fmax drops a NaN, as fmaxf does
    coord = org[None, :] + ijk.astype(F32) * spc[None, :]        # fp32: origin + i * spacing
    ia = ijk[np.arange(ids.size), axis]
    c0 = org[axis] + ia.astype(F32) * spc[axis]
    c1 = org[axis] + (ia + 1).astype(F32) * spc[axis]
    coord[np.arange(ids.size), axis] = c0 + t * (c1 - c0)
    verts = coord.astype(F32)

    count, edges, _ = mc_table.tables()
    cfg = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = mc_table.CORNERS[c]
        cfg |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    cfg = cfg.reshape(-1)
    cnt = count[cfg].astype(np.int64)
    cells = np.flatnonzero(cnt)
    if cells.size == 0:
        return verts, np.zeros((0, 3), dtype=np.int64)
    reps = cnt[cells]
    cell_of = np.repeat(cells, reps)
    first = np.repeat(np.cumsum(reps) - reps, reps)
    t_in_cell = np.arange(cell_of.size) - first
    e = edges[cfg[cell_of][:, None], 3 * t_in_cell[:, None] + np.arange(3)[None, :]].astype(np.int64)     # [F,3] edge ids
    cijk = np.stack(np.unravel_index(cell_of, (nx - 1, ny - 1, nz - 1)), -1)                          # [F,3] cell corner
    own = cijk[:, None, :] + mc_table.EDGE_OFFSET[e]                                                 # [F,3,3]
    lin = (own[..., 0] * ny + own[..., 1]) * nz + own[..., 2]
    faces = vid[lin * 3 + mc_table.EDGE_AXIS[e]]
    assert (faces >= 0).all()
    return verts, faces


def marching_cubes(volume, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """Mesh of ``{volume > level}``: volume [nx,ny,nz] -> (verts float32 [V,3], faces int64 [F,3]).  Vertex coordinates are
    ``origin + index * spacing`` per axis.  A device tensor runs on ``ia_mc_count`` / ``ia_mc_emit`` and returns device tensors; a CPU
    tensor returns CPU tensors and a NumPy array NumPy arrays (both from the NumPy restatement)."""
    org, spc = _vec3(origin), _vec3(spacing)
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        from . import hipops
        verts, faces = hipops.marching_cubes(volume.float().contiguous(), float(level), org, spc)
        return verts, faces.long()
    if volume.ndim != 3 or min(volume.shape) < 2:
        raise ValueError(f'volume must be [nx,ny,nz] with every dimension >= 2, got {tuple(volume.shape)}')
    if isinstance(volume, torch.Tensor):
        verts, faces = _mc_numpy(volume.detach().cpu().numpy(), level, org, spc)
        return torch.from_numpy(verts), torch.from_numpy(faces)
    return _mc_numpy(volume, level, org, spc)


# ------------------------------------------------------------------ ray casting

BRICK = 8               # cells per brick edge (csrc/raycast.hip kBrick)
BISECT = 20             # bisection steps per hit (csrc/raycast.hip kRcBisect): bracket <= sqrt(3) * 2^-20 < 2e-6 cell


def _bricks_numpy(v):
    """NumPy restatement of ia_volume_bricks: [bx,by,bz,2] float32 {min, max} over 9^3-point bricks (NaN ignored; all NaN: +inf, -inf)."""
    lo = hi = np.asarray(v, dtype=F32)
    for a, n in enumerate(lo.shape):
        starts = np.arange(0, n - 1, BRICK)
        ends = np.minimum(starts + BRICK, n - 1)                 # the shared boundary plane of each brick
        lo = np.fmin(np.fmin.reduceat(lo, starts, axis=a), np.take(lo, ends, axis=a))
        hi = np.fmax(np.fmax.reduceat(hi, starts, axis=a), np.take(hi, ends, axis=a))
    return np.stack([np.where(np.isnan(lo), np.inf, lo), np.where(np.isnan(hi), -np.inf, hi)], -1).astype(F32)


def _point_grad(v, step, idx):
    """Central-difference gradients [m,3] at lattice points idx [m,3] (one-sided at the border), divided by the step per axis."""
    n = np.array(v.shape)
    g = np.empty(idx.shape, dtype=np.float64)
    for a in range(3):
        lo_i, hi_i = idx.copy(), idx.copy()
        lo_i[:, a] = np.maximum(idx[:, a] - 1, 0)
        hi_i[:, a] = np.minimum(idx[:, a] + 1, n[a] - 1)
        d = v[hi_i[:, 0], hi_i[:, 1], hi_i[:, 2]] - v[lo_i[:, 0], lo_i[:, 1], lo_i[:, 2]]
        g[:, a] = d / ((hi_i[:, a] - lo_i[:, a]) * step[a])
    return g


def _cell_grad(v, step, c, u):
    """Trilinear interpolation at local coordinates u [m,3] of cells c [m,3] of the gradients at the cells' 8 corners."""
    g = np.zeros(u.shape, dtype=np.float64)
    for q in range(8):
        d = np.array([q & 1, (q >> 1) & 1, q >> 2])
        w = np.prod(np.where(d[None, :] == 1, u, 1.0 - u), axis=1)
        g += w[:, None] * _point_grad(v, step, c + d[None, :])
    return g


def _unit_neg(g):
    nrm = np.linalg.norm(g, axis=-1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(nrm > 0, -g / nrm, 0.0)


def _cubic_first_hit(c0, c1, c2, c3, L):
    """First s in [0, L] with ((c3 s + c2) s + c1) s + c0 > 0 (c0 already minus the level), or -1: monotone pieces between the roots of
    the derivative, then BISECT bisection steps on the first piece whose end is inside (csrc/raycast.hip cubic_first_hit)."""
    f = lambda s: ((c3 * s + c2) * s + c1) * s + c0            # noqa: E731
    A, B, C = 3.0 * c3, 2.0 * c2, c1
    r0, r1 = np.full_like(c0, -1.0), np.full_like(c0, -1.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        lin = (A == 0) & (B != 0)
        r0 = np.where(lin, -C / np.where(lin, B, 1.0), r0)
        disc = B * B - 4.0 * A * C
        quad = (A != 0) & (disc > 0)
        q = -0.5 * (B + np.copysign(np.sqrt(np.where(quad, disc, 0.0)), B))
        qa, qb = q / np.where(quad, A, 1.0), np.where(q != 0, C / np.where(q != 0, q, 1.0), -1.0)
        r0, r1 = np.where(quad, np.minimum(qa, qb), r0), np.where(quad, np.maximum(qa, qb), r1)
    br = [np.where((r > 0) & (r < L), r, np.nan) for r in (r0, r1)] + [L]
    s = np.where(c0 > 0, 0.0, -1.0)
    a = np.zeros_like(c0)
    for b in br:
        valid = ~np.isnan(b)
        take = valid & (s < 0) & (f(np.where(valid, b, 0.0)) > 0)
        lo, hi = a[take], b[take]
        cc = [x[take] for x in (c0, c1, c2, c3)]
        for _ in range(BISECT):
            mid = 0.5 * (lo + hi)
            inside = ((cc[3] * mid + cc[2]) * mid + cc[1]) * mid + cc[0] > 0
            hi, lo = np.where(inside, mid, hi), np.where(inside, lo, mid)
        s[take] = 0.5 * (lo + hi)
        a = np.where(valid, b, a)
    return s


def _raycast_numpy(vol, level, lo, step, ro, rd, t_min):
    """NumPy restatement of ia_raycast_volume (float64 arithmetic; every cell is walked, which the brick skip of the kernel does not
    change): (depth [R], normal [R,3], mask bool [R])."""
    v = np.asarray(vol, dtype=F32).astype(np.float64)
    n = np.array(v.shape)
    level = float(F32(level))
    lo, step = np.array(lo, dtype=F32).astype(np.float64), np.array(step, dtype=F32).astype(np.float64)
    ro, rd = np.asarray(ro, dtype=F32).astype(np.float64).reshape(-1, 3), np.asarray(rd, dtype=F32).astype(np.float64).reshape(-1, 3)
    R = ro.shape[0]
    depth, normal, mask = np.zeros(R), np.zeros((R, 3)), np.zeros(R, dtype=bool)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        O, D = (ro - lo) / step, rd / step
        ok = np.isfinite(O).all(1) & np.isfinite(D).all(1) & (D != 0).any(1)
        # 1. clip to the box and to t >= t_min
        top = (n - 1).astype(np.float64)
        ta, tb = -O / D, (top - O) / D
        par = D == 0
        t0 = np.maximum(float(t_min), np.where(par, -np.inf, np.minimum(ta, tb)).max(1))
        t1 = np.where(par, np.inf, np.maximum(ta, tb)).min(1)
        ok &= np.where(par, (O >= 0) & (O <= top), True).all(1) & (t0 <= t1)
        idx = np.flatnonzero(ok)
        O, D, t0, t1 = O[idx], D[idx], t0[idx], t1[idx]
        c = np.clip(np.floor(O + t0[:, None] * D), 0, n - 2).astype(np.int64)
    tc = t0.copy()
    sgn = np.where(D > 0, 1, -1)
    for _ in range(int(n.sum())):
        if idx.size == 0:
            break
        # 2. this cell spans [tc, te]
        with np.errstate(invalid='ignore', divide='ignore'):
            tn = np.where(D > 0, (c + 1 - O) / D, np.where(D < 0, (c - O) / D, np.inf))
        ax = np.argmin(tn, 1)                                         # ties: the lower axis
        to = tn[np.arange(idx.size), ax]
        te = np.maximum(np.minimum(to, t1), tc)
        cv = np.stack([v[c[:, 0] + (q & 1), c[:, 1] + ((q >> 1) & 1), c[:, 2] + (q >> 2)] for q in range(8)], 1)
        nan = np.isnan(cv).any(1)
        cand = np.flatnonzero(~nan & (np.where(nan[:, None], -np.inf, cv).max(1) > level))
        hit = np.zeros(idx.size, dtype=bool)
        if cand.size:
            # 4-5. the cubic of the trilinear field along the ray, in s = t - tc
            w = cv[cand]
            k1, k2, k3 = w[:, 1] - w[:, 0], w[:, 2] - w[:, 0], w[:, 4] - w[:, 0]
            k4, k5, k6 = w[:, 3] - w[:, 1] - w[:, 2] + w[:, 0], w[:, 5] - w[:, 1] - w[:, 4] + w[:, 0], w[:, 6] - w[:, 2] - w[:, 4] + w[:, 0]
            k7 = w[:, 7] - w[:, 3] - w[:, 5] - w[:, 6] + w[:, 1] + w[:, 2] + w[:, 4] - w[:, 0]
            u = O[cand] + tc[cand, None] * D[cand] - c[cand]
            bu, bv, bw = D[cand, 0], D[cand, 1], D[cand, 2]
            u0, v0, w0 = u[:, 0], u[:, 1], u[:, 2]
            c3 = k7 * bu * bv * bw
            c2 = k4 * bu * bv + k5 * bu * bw + k6 * bv * bw + k7 * (u0 * bv * bw + v0 * bu * bw + w0 * bu * bv)
            c1 = (k1 * bu + k2 * bv + k3 * bw + k4 * (u0 * bv + v0 * bu) + k5 * (u0 * bw + w0 * bu) + k6 * (v0 * bw + w0 * bv)
                  + k7 * (u0 * v0 * bw + u0 * w0 * bv + v0 * w0 * bu))
            c0 = w[:, 0] + k1 * u0 + k2 * v0 + k3 * w0 + k4 * u0 * v0 + k5 * u0 * w0 + k6 * v0 * w0 + k7 * u0 * v0 * w0 - level
            s = _cubic_first_hit(c0, c1, c2, c3, te[cand] - tc[cand])
            h = s >= 0
            if h.any():
                hc = cand[h]
                rays = idx[hc]
                depth[rays] = tc[hc] + s[h]
                mask[rays] = True
                # 7. normal from the interpolated corner gradients
                normal[rays] = _unit_neg(_cell_grad(v, step, c[hc], u[h] + s[h, None] * D[hc]))
                hit[hc] = True
        # step to the next cell; a ray ends at its hit, at the box exit or when it leaves the lattice
        r = np.arange(idx.size)
        c[r, ax] += sgn[r, ax]
        keep = ~hit & (to < t1) & (c[r, ax] >= 0) & (c[r, ax] <= n[ax] - 2)
        idx, O, D, t1, c, sgn, tc = idx[keep], O[keep], D[keep], t1[keep], c[keep], sgn[keep], te[keep]
    return depth, normal, mask


def _as_out(x, like, dtype=None):
    """A NumPy result in the container of ``like``: a CPU torch tensor for a tensor, NumPy otherwise."""
    x = x.astype(dtype or F32)
    return torch.from_numpy(x) if isinstance(like, torch.Tensor) else x


def raycast(volume, level, origin, spacing, rays_o, rays_d, t_min=0.0, skip=True):
    """First hit of rays [..., 3] with the surface {volume > level} of the trilinear field: {'depth' [...], 'mask' bool [...],
    'normal' [..., 3]}.  ``origin`` / ``spacing`` are the coordinates of point (0,0,0) and the lattice step per axis (the arguments of
    ``marching_cubes``).  ``depth`` is the ray parameter t (world distance for unit directions), ``normal`` points toward decreasing
    density; misses are 0.  Device tensors run on ia_volume_bricks + ia_raycast_volume (``skip``: jump over bricks with max <= level,
    which changes no result); CPU tensors and NumPy arrays take the NumPy restatement."""
    org, spc = _vec3(origin), _vec3(spacing)
    lead = tuple(rays_o.shape[:-1])
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        from . import hipops
        vol = volume.float().contiguous()
        bricks = hipops.volume_bricks(vol) if skip else None
        depth, normal, mask = hipops.raycast_volume(vol, float(level), org, spc, rays_o.float().reshape(-1, 3).contiguous(),
                                                    rays_d.float().reshape(-1, 3).contiguous(), t_min, bricks)
        return {'depth': depth.reshape(lead), 'mask': mask.reshape(lead), 'normal': normal.reshape(lead + (3,))}
    if volume.ndim != 3 or min(volume.shape) < 2:
        raise ValueError(f'volume must be [nx,ny,nz] with every dimension >= 2, got {tuple(volume.shape)}')
    depth, normal, mask = _raycast_numpy(_np(volume), level, org, spc, _np(rays_o), _np(rays_d), t_min)
    return {'depth': _as_out(depth.reshape(lead), rays_o), 'mask': _as_out(mask.reshape(lead), rays_o, bool),
            'normal': _as_out(normal.reshape(lead + (3,)), rays_o)}


def volume_normals(volume, verts, origin, spacing):
    """Unit normals [V,3] at points (the marching-cubes vertices of the same volume): -g/|g| of the interpolated central-difference
    gradient (0 where g = 0), pointing toward decreasing density as the mesh is wound.  Device tensors run on ia_volume_gradient."""
    org, spc = _vec3(origin), _vec3(spacing)
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        from . import hipops
        g = hipops.volume_gradient(volume.float().contiguous(), org, spc, verts.float().reshape(-1, 3).contiguous())
        nrm = g.norm(dim=-1, keepdim=True)
        return torch.where(nrm > 0, -g / nrm.clamp_min(1e-30), torch.zeros_like(g))
    v = np.asarray(_np(volume), dtype=F32).astype(np.float64)
    n = np.array(v.shape)
    lo, step = np.array(org, dtype=F32).astype(np.float64), np.array(spc, dtype=F32).astype(np.float64)
    p = np.asarray(_np(verts), dtype=F32).astype(np.float64).reshape(-1, 3)
    P = np.fmin(np.fmax((p - lo) / step, 0.0), n - 1)                 # fmax drops a NaN, as fmaxf does
    c = np.minimum(np.floor(P).astype(np.int64), n - 2)
    return _as_out(_unit_neg(_cell_grad(v, step, c, P - c)), verts)


def shade(normal, rays_d, mask, ambient=0.25):
    """Headlight Lambert shading in [0, 1]: [..., 1] = mask * (ambient + (1 - ambient) * max(0, n . -d)), d normalised."""
    normal, rays_d, mask = (torch.as_tensor(x) for x in (normal, rays_d, mask))
    d = torch.nn.functional.normalize(rays_d.float(), dim=-1)
    lam = (-(normal.float() * d).sum(-1, keepdim=True)).clamp(0, 1)
    return (ambient + (1.0 - ambient) * lam) * mask[..., None].float()


# ------------------------------------------------------------------ generator-level helpers

def generator_planes(G, ws, mesh_condition, update_emas=False, **synthesis_kwargs):
    """The tri-planes [B,3,32,256,256] of ``ws`` under ``mesh_condition``: backbone -> rasterise -> ``_planes``, the sequence of
    ``TriPlaneGenerator._query`` (triplane_v20.py:513-518)."""
    texture_feats = G.texture_backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=update_emas, **synthesis_kwargs)
    static_feats = G.backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=update_emas, **synthesis_kwargs)
    return G._planes(ws, texture_feats, static_feats, mesh_condition, update_emas, synthesis_kwargs)


def vertex_colors(planes, decoder, verts, box_warp):
    """uint8 [V,3]: the decoder's rgb[:3] at the vertices, clamped to [0, 1]."""
    if verts.shape[0] == 0:
        return torch.zeros(0, 3, dtype=torch.uint8, device=verts.device)
    rgb = query_planes(planes, decoder, verts[None].float(), box_warp, rgb=True)['rgb'][0, :, :3]
    return (rgb.clamp(0, 1) * 255).round().to(torch.uint8)


# ------------------------------------------------------------------ PLY

def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def write_ply(path, verts, faces, colors=None, normals=None):
    """Binary little-endian PLY: float x, y, z (+ float nx, ny, nz) (+ uchar red, green, blue) per vertex, int32 index triples per face."""
    v = _np(verts).astype('<f4').reshape(-1, 3)
    f = _np(faces).astype('<i4').reshape(-1, 3)
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    if normals is not None:
        fields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
    if colors is not None:
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
    vrec = np.empty(v.shape[0], dtype=fields)
    vrec['x'], vrec['y'], vrec['z'] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        nrm = _np(normals).astype('<f4').reshape(-1, 3)
        vrec['nx'], vrec['ny'], vrec['nz'] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colors is not None:
        c = _np(colors).astype(np.uint8).reshape(-1, 3)
        vrec['red'], vrec['green'], vrec['blue'] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(f.shape[0], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    frec['n'], frec['i'] = 3, f
    head = ['ply', 'format binary_little_endian 1.0', f'element vertex {v.shape[0]}', 'property float x', 'property float y',
            'property float z']
    if normals is not None:
        head += ['property float nx', 'property float ny', 'property float nz']
    if colors is not None:
        head += ['property uchar red', 'property uchar green', 'property uchar blue']
    head += [f'element face {f.shape[0]}', 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(head) + '\n').encode('ascii'))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path, with_normals=False):
    """Inverse of ``write_ply``: (verts float32 [V,3], faces int64 [F,3], colors uint8 [V,3] or None), and with ``with_normals`` a
    fourth item, normals float32 [V,3] or None."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    head = data[:end].decode('ascii').split('\n')
    nv = int(next(h for h in head if h.startswith('element vertex')).split()[-1])
    nf = int(next(h for h in head if h.startswith('element face')).split()[-1])
    has_col, has_nrm = 'property uchar red' in head, 'property float nx' in head
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')] + ([('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')] if has_nrm else [])
    fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')] if has_col else []
    vrec = np.frombuffer(data, dtype=fields, count=nv, offset=end)
    frec = np.frombuffer(data, dtype=[('n', 'u1'), ('i', '<i4', (3,))], count=nf, offset=end + vrec.nbytes)
    verts = np.stack([vrec['x'], vrec['y'], vrec['z']], -1).astype(np.float32)
    cols = np.stack([vrec['red'], vrec['green'], vrec['blue']], -1) if has_col else None
    if not with_normals:
        return verts, frec['i'].astype(np.int64), cols
    nrm = np.stack([vrec['nx'], vrec['ny'], vrec['nz']], -1).astype(np.float32) if has_nrm else None
    return verts, frec['i'].astype(np.int64), cols, nrm
