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
- ``components`` / ``keep_components``: connected components of ``{volume > level}`` (labels, per-component statistics) and the filter
  that drops floaters before meshing or ray casting; ``mesh_components`` / ``keep_mesh_components``: the same for an indexed mesh.
  Device tensors go to ``ia_volume_components`` + ``ia_component_stats`` + ``ia_volume_keep`` (``ia_mesh_components`` for meshes); CPU
  tensors and NumPy arrays take a NumPy union-find restatement of the same definitions.
- ``closest_point`` / ``TriangleGrid`` / ``surface_distance``: exact point-to-mesh distance and the numbers made of it (Chamfer and
  Hausdorff distance, F-score, normal consistency), with ``face_normals`` and ``sample_surface``.  Device tensors go to ``ia_tri_pack`` +
  ``ia_trigrid_count`` / ``ia_trigrid_fill`` + ``ia_closest_point`` + ``ia_distance_stats``; CPU tensors and NumPy arrays take a NumPy
  restatement (``point_triangle``: the kernel's per-triangle function line by line, float64; brute force over all triangles).
- ``simplify_mesh``: quadric vertex clustering on a uniform grid, to a cell size or to a target face count.  Device tensors go to the
  kernels of csrc/simplify.hip (``ia_simplify_*``; the sorts of integer keys are ``torch.sort``); CPU tensors and NumPy arrays take the
  NumPy restatement that is the definition (float64).
- ``smooth_mesh`` / ``MeshAdjacency`` / ``mesh_normals``: Taubin and Laplacian smoothing of an indexed mesh (uniform or cotangent
  weights, pinned boundary) and vertex normals from the mesh itself.  Device tensors go to the kernels of csrc/smooth.hip (``ia_mesh_*``,
  ``ia_smooth_*``; the two sorts of integer keys are ``torch.sort``); CPU tensors and NumPy arrays take the NumPy restatement that is the
  definition (float64 sums, positions rounded to float32 once per step).
- ``rasterize_mesh``: z-buffer rasteriser of an indexed mesh from N cameras: mask, face, perspective-correct barycentrics, depth,
  normals and interpolated vertex attributes per pixel.  Device tensors go to ``ia_mesh_project`` + ``ia_mesh_raster`` +
  ``ia_mesh_resolve`` (csrc/mesh_raster.hip); CPU tensors and NumPy arrays take the NumPy restatement that is the definition (integer
  coverage on coordinates snapped to 1/256 pixel, float32 operations in the kernel's order, or float64 with ``dtype=``).
- ``align_mesh`` / ``fit_transform`` / ``transform_points``: rigid or similarity alignment of points to a mesh by iterated closest
  points (point-to-point or point-to-plane, trimmed), the closed form for given correspondences, and the transform itself.  Device
  tensors go to ``ia_transform_points`` + ``ia_closest_point`` + ``ia_align_sums`` (csrc/align.hip) with the step solved on the host in
  float64; CPU tensors and NumPy arrays take the NumPy restatement that is the definition.
- ``winding_number`` / ``inside`` / ``signed_distance`` / ``mesh_to_volume`` / ``volume_iou``: which side of a mesh a point is on (the
  generalised winding number: 1 inside a closed outward-wound mesh, 0 outside, smooth for open meshes), the signed distance made of
  it and ``closest_point``, a mesh as an SDF / occupancy lattice and the volumetric IoU of two meshes.  Device tensors go to
  ``ia_winding_number`` (csrc/winding.hip: the all-pairs sum, double sums in a fixed order) + ``ia_closest_point`` +
  ``ia_volume_components``; CPU tensors and NumPy arrays take the NumPy restatement that is the definition.  ``WindingTree`` and
  ``method='tree'`` / ``winding='tree'`` are the approximation for large meshes (csrc/winding_tree.hip: a Morton-sorted cluster tree
  whose far nodes are a dipole and its first derivative); the exact sum stays the default and what the tree is held to.
- ``TextureAtlas`` / ``atlas_points`` / ``bake_texture`` / ``bake_colors`` / ``project_texture`` / ``sample_texture``: the colours of
  the avatar on a texture of the mesh: two triangles to a square block with a guard texel (no chart bleeds into another under a bilinear
  lookup), the surface point of every texel, a bake from any function of position (the decoder, a distance), projective texturing from
  rendered views with the rasteriser's depth as the visibility test, and the lookup.  Device tensors go to ``ia_atlas_points`` +
  ``ia_texture_project`` + ``ia_texture_sample`` (csrc/texture.hip); CPU tensors and NumPy arrays take the NumPy restatement that is the
  definition.  ``write_obj`` / ``read_obj``: OBJ + MTL + PNG.
- ``write_ply`` / ``read_ply``: binary little-endian PLY in NumPy (optionally with vertex normals).

Rasteriser: pixel centres are at integer coordinates, column i and row j of ``RaySampler_zxc`` (ray ``K_res^-1 [i, j, 1]``), so its images
align with ``raycast`` on that sampler's rays; a pixel is covered under the top-left rule and goes to the nearest triangle, the lower
face index at equal depth; triangles with a vertex at or behind ``near`` are dropped, not clipped.

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


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _as_out(x, like, dtype=None):
    """A NumPy result in the container of ``like``: a CPU torch tensor for a tensor, NumPy otherwise."""
    x = x.astype(dtype or F32)
    return torch.from_numpy(x) if isinstance(like, torch.Tensor) else x


def _check_volume(volume):
    if volume.ndim != 3 or min(volume.shape) < 2:
        raise ValueError(f'volume must be [nx,ny,nz] with every dimension >= 2, got {tuple(volume.shape)}')


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
    _check_volume(volume)
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
    _check_volume(volume)
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


# ------------------------------------------------------------------ connected components

def _forward_offsets(connectivity):
    """One offset of each pair of opposite neighbour offsets: the lexicographically positive ones."""
    if connectivity == 6:
        return [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    if connectivity == 26:
        return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) > (0, 0, 0)]
    raise ValueError(f'connectivity must be 6 or 26, got {connectivity}')


def _roots_numpy(n, a, b):
    """Union-find over nodes 0..n-1 with the edges (a[e], b[e]): int64 [n], the smallest index of each node's component.  Each round
    hooks the larger of an edge's two roots under the smaller (parents only decrease, so a root is the minimum of its tree) and then
    jumps every node to its root; edges inside one tree are dropped; the rounds end when none is left."""
    parent = np.arange(n, dtype=np.int64)
    while a.size:
        ra, rb = parent[a], parent[b]
        live = ra != rb
        a, b, ra, rb = a[live], b[live], ra[live], rb[live]
        if not a.size:
            break
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    return parent


def _components_numpy(v, level, connectivity):
    """NumPy restatement of ia_volume_components: (labels int32 [nx,ny,nz], K)."""
    v = np.ascontiguousarray(v, dtype=F32)
    inside = v > F32(level)                                          # fp32 compare; NaN is outside
    idx = np.arange(v.size, dtype=np.int64).reshape(v.shape)
    ea, eb = [], []
    for off in _forward_offsets(connectivity):
        s0 = tuple(slice(max(0, -d), n - max(0, d)) for d, n in zip(off, v.shape))
        s1 = tuple(slice(max(0, d), n - max(0, -d)) for d, n in zip(off, v.shape))
        both = inside[s0] & inside[s1]
        ea.append(idx[s0][both])
        eb.append(idx[s1][both])
    parent = _roots_numpy(v.size, np.concatenate(ea), np.concatenate(eb))
    lin = np.flatnonzero(inside)
    roots = np.unique(parent[lin])                                   # sorted: components in order of their smallest linear index
    labels = np.zeros(v.size, dtype=np.int32)
    labels[lin] = np.searchsorted(roots, parent[lin]) + 1
    return labels.reshape(v.shape), int(roots.size)


def _component_stats_numpy(labels, k):
    """NumPy restatement of ia_component_stats: int32 [K,8]."""
    labels = np.asarray(labels)
    stats = np.zeros((k, 8), dtype=np.int32)
    lin = np.flatnonzero(labels)
    c = labels.reshape(-1)[lin].astype(np.int64) - 1
    stats[:, 0] = np.bincount(c, minlength=k)
    big = np.iinfo(np.int32).max
    cols = [lin] + list(np.unravel_index(lin, labels.shape))
    for col, x in enumerate(cols):
        lo = np.full(k, big, dtype=np.int64)
        np.minimum.at(lo, c, x)
        stats[:, 1 + col] = lo
    for col, x in enumerate(cols[1:]):
        hi = np.full(k, -1, dtype=np.int64)
        np.maximum.at(hi, c, x)
        stats[:, 5 + col] = hi
    return stats


def components(volume, level, connectivity=26):
    """Connected components of ``{volume > level}`` (fp32 compare, NaN outside; neighbours: indices differ by at most 1 on every axis
    for ``connectivity`` 26, by 1 on exactly one axis for 6): ``(labels, stats)``.  ``labels`` int32 [nx,ny,nz]: 0 outside, components
    1..K in increasing order of their smallest linear index ``(i*ny + j)*nz + k``.  ``stats`` int32 [K,8], row c-1 for label c: point
    count, smallest linear index, imin, jmin, kmin, imax, jmax, kmax.  A device tensor runs on ia_volume_components +
    ia_component_stats (one host synchronisation, for K) and returns device tensors; CPU tensors and NumPy arrays take the NumPy
    restatement (a union-find written to be checked by reading, not to be fast)."""
    _forward_offsets(connectivity)
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        from . import hipops
        labels, k = hipops.volume_components(volume.float().contiguous(), float(level), connectivity)
        return labels, hipops.component_stats(labels, k)
    _check_volume(volume)
    labels, k = _components_numpy(_np(volume), level, connectivity)
    return _as_out(labels, volume, np.int32), _as_out(_component_stats_numpy(labels, k), volume, np.int32)


def select_components(stats, keep='largest', min_voxels=0):
    """Which labels to keep, from the statistics table (column 0 = size): ``'largest'`` (greatest size; a tie goes to the lowest
    label), an int n >= 1 (the n largest in that order) or an explicit sequence of labels; ``min_voxels`` then drops those smaller than
    it.  Returns a list of ints (largest first, or in the order given).  Host code on a [K, *] table."""
    size = _np(stats)[:, 0].astype(np.int64) if len(stats) else np.zeros(0, dtype=np.int64)
    k = size.size
    if isinstance(min_voxels, bool) or int(min_voxels) != min_voxels or min_voxels < 0:
        raise ValueError(f'min_voxels must be an integer >= 0, got {min_voxels!r}')
    order = np.lexsort((np.arange(k), -size)) + 1                    # by size descending, then by label
    if isinstance(keep, str):
        if keep != 'largest':
            raise ValueError(f"keep must be 'largest', an int >= 1 or a sequence of labels, got {keep!r}")
        chosen = order[:1].tolist()
    elif isinstance(keep, bool) or keep is None:
        raise ValueError(f"keep must be 'largest', an int >= 1 or a sequence of labels, got {keep!r}")
    elif isinstance(keep, (int, np.integer)):
        if keep < 1:
            raise ValueError(f'keep = {keep}: the number of components to keep must be >= 1')
        chosen = order[:int(keep)].tolist()
    else:
        chosen = []
        for c in (keep.tolist() if hasattr(keep, 'tolist') else list(keep)):
            if isinstance(c, bool) or int(c) != c or not 1 <= int(c) <= k:
                raise ValueError(f'keep: {c!r} is not a label in 1..{k}')
            chosen.append(int(c))
        if len(set(chosen)) != len(chosen):
            raise ValueError(f'keep: labels repeat in {chosen}')
    return [int(c) for c in chosen if size[c - 1] >= min_voxels]


def keep_components(volume, level, keep='largest', min_voxels=0, connectivity=26, fill=None):
    """Drop floaters: ``(filtered volume, info)``.  The filtered volume equals ``volume`` except at the inside points of components
    that ``select_components`` does not keep, which become ``fill`` (default: ``level`` rounded to fp32, which is not inside); outside
    points are never touched, so the kept surface is unchanged.  ``info = {'count': K, 'kept': labels kept, 'stats': [K,8]}``.  With
    connectivity 26 the mesh of the filtered volume is exactly the kept components' triangles of the original mesh."""
    labels, stats = components(volume, level, connectivity)
    kept = select_components(stats, keep, min_voxels)
    k = int(stats.shape[0])
    fill = float(F32(level)) if fill is None else float(F32(fill))
    flags = np.zeros(k + 1, dtype=np.uint8)
    flags[kept] = 1
    info = {'count': k, 'kept': kept, 'stats': stats}
    if isinstance(volume, torch.Tensor) and volume.is_cuda:
        from . import hipops
        return hipops.volume_keep(volume.float().contiguous(), labels, torch.from_numpy(flags).to(volume.device), fill), info
    lab = _np(labels)
    out = np.array(_np(volume), dtype=F32)
    out[(lab > 0) & (flags[lab] == 0)] = F32(fill)
    return _as_out(out, volume), info


def _mesh_components_numpy(faces, n_verts):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= n_verts):
        raise ValueError(f'faces index vertices outside [0, {n_verts})')
    parent = _roots_numpy(n_verts, np.concatenate([faces[:, 0], faces[:, 1]]), np.concatenate([faces[:, 1], faces[:, 2]]))
    roots = np.unique(parent)
    vl = (np.searchsorted(roots, parent) + 1).astype(np.int32)
    fl = vl[faces[:, 0]]
    stats = np.zeros((roots.size, 3), dtype=np.int32)
    stats[:, 0] = np.bincount(vl.astype(np.int64) - 1, minlength=roots.size)
    stats[:, 1] = np.bincount(fl.astype(np.int64) - 1, minlength=roots.size)
    stats[:, 2] = roots
    return vl, fl, stats


def mesh_components(faces, n_verts):
    """Connected components of an indexed triangle mesh (two vertices are connected if a face contains both): ``(vert_labels int32
    [V], face_labels int32 [F], stats int32 [K,3])``.  Components 1..K in increasing order of their smallest vertex index; a vertex
    used by no face is a component of its own; a face has the label of its first vertex; stats rows: vertex count, face count,
    smallest vertex index.  Device tensors run on ia_mesh_components (two host synchronisations: the index range check and K)."""
    n_verts = int(n_verts)
    if n_verts < 0 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f'faces must be [F,3] and n_verts >= 0, got {tuple(faces.shape)} and {n_verts}')
    if isinstance(faces, torch.Tensor) and faces.is_cuda:
        from . import hipops
        if faces.shape[0] and (int(faces.min()) < 0 or int(faces.max()) >= n_verts):
            raise ValueError(f'faces index vertices outside [0, {n_verts})')
        f32 = faces.to(torch.int32).contiguous()
        vl, k = hipops.mesh_components(f32, n_verts)
        return vl, vl[faces[:, 0].long()], hipops.mesh_component_stats(f32, vl, k)
    vl, fl, stats = _mesh_components_numpy(_np(faces), n_verts)
    return _as_out(vl, faces, np.int32), _as_out(fl, faces, np.int32), _as_out(stats, faces, np.int32)


def keep_mesh_components(verts, faces, keep='largest', extras=()):
    """The mesh restricted to the components ``select_components`` keeps (sizes = vertex counts): ``(verts, faces, extras, info)`` with
    the vertices compacted in their old order, the faces re-indexed (int64) and every per-vertex array in ``extras`` (colours, normals)
    carried along.  ``info = {'count': K, 'kept': labels, 'stats': [K,3]}``.  NumPy in, NumPy out; tensors stay on their device."""
    as_np = not isinstance(verts, torch.Tensor)
    tv, tf = torch.as_tensor(verts), torch.as_tensor(faces).to(torch.as_tensor(verts).device)
    vl, fl, stats = mesh_components(tf, tv.shape[0])
    kept = select_components(stats, keep)
    k = int(stats.shape[0])
    flag = torch.zeros(k + 1, dtype=torch.bool)
    flag[kept] = True
    flag = flag.to(tv.device)
    vmask, fmask = flag[vl.long()], flag[fl.long()]
    out_v, out_f, out_e = _compact_mesh(tv, tf, vmask, fmask, [torch.as_tensor(e).to(tv.device) for e in extras])
    out = [out_v, out_f] + out_e
    if as_np:
        out = [o.numpy() for o in out]
        stats = _np(stats)
    return out[0], out[1], out[2:], {'count': k, 'kept': kept, 'stats': stats}


# ------------------------------------------------------------------ surface distance

def _dot3(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross3(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _segment(a, e, ee, best, q, dtype):
    """Closest point of the segment a + t e, t in [0, 1] (ee = e . e), to the origin; kept where its squared distance is below ``best``."""
    pos = ee > 0
    t = np.where(pos, np.minimum(np.maximum(-_dot3(a, e) / np.where(pos, ee, dtype(1)), dtype(0)), dtype(1)), dtype(0))
    r = a + t[..., None] * e
    d2 = _dot3(r, r)
    take = d2 < best
    return np.where(take, d2, best), np.where(take[..., None], r, q)


def point_triangle(p, A, B, C, dtype=np.float64):
    """The per-triangle function (csrc/surface_distance.hip tri_dist), evaluated in ``dtype`` on broadcastable [..., 3] arrays:
    ``(dist, q)`` with q the closest point of the closed triangle relative to p.  In coordinates relative to the query point: the
    minimum of the three clamped point-to-segment distances, replaced by the plane distance ``|n . a| / |n|`` (n: the cross product of
    the two shorter edges) when ``n . n > 0``, the origin projects inside and the plane distance is the smaller one (``n . (a x (b - a))``, ``n . (b x (c - b))``, ``n . (c x (a - c))`` all ``>= 0``).  Every operation is
    rounded on its own and dot products are ``(x + y) + z``, so the float32 run follows the kernel operation by operation."""
    p, A, B, C = (np.asarray(x, dtype=dtype) for x in (p, A, B, C))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        a, b, c = A - p, B - p, C - p
        a, b, c = np.broadcast_arrays(a, b, c)
        d2 = np.full(a.shape[:-1], np.inf, dtype=dtype)
        q = np.full(a.shape, np.nan, dtype=dtype)
        eab, ebc, eca = b - a, c - b, a - c
        lab, lbc, lca = _dot3(eab, eab), _dot3(ebc, ebc), _dot3(eca, eca)
        d2, q = _segment(a, eab, lab, d2, q, dtype)
        d2, q = _segment(b, ebc, lbc, d2, q, dtype)
        d2, q = _segment(c, eca, lca, d2, q, dtype)
        d = np.sqrt(d2)
        # the normal from the two shorter edges (eab x ebc = ebc x eca = eca x eab): no cancellation on needle-shaped triangles
        ab_longest, bc_longest = (lab >= lbc) & (lab >= lca), lbc >= lca
        n = np.where(ab_longest[..., None], _cross3(ebc, eca), np.where(bc_longest[..., None], _cross3(eca, eab), _cross3(eab, ebc)))
        nn = _dot3(n, n)
        inside = (nn > 0) & (_dot3(n, _cross3(a, eab)) >= 0) & (_dot3(n, _cross3(b, ebc)) >= 0) & (_dot3(n, _cross3(c, eca)) >= 0)
        na = _dot3(n, a)
        safe = np.where(inside, nn, dtype(1))
        dp = np.abs(na) / np.sqrt(safe)
        inside &= dp < d                                               # (a vertex or edge that p lies on keeps its exact 0)
        d = np.where(inside, dp, d)
        q = np.where(inside[..., None], n * (na / safe)[..., None], q)
    return d.astype(dtype), q.astype(dtype)


def _closest_numpy(points, verts, faces, dtype=np.float64, pairs=1 << 20):
    """NumPy restatement of ia_closest_point in ``dtype``: brute force over all usable triangles, ``pairs`` point-triangle pairs at a
    time; the minimum on the pair (distance, index).  (dist [N], face int32 [N], point [N,3]), all computed in ``dtype``."""
    p = np.asarray(points, dtype=F32).reshape(-1, 3).astype(dtype)
    v = np.asarray(verts, dtype=F32).reshape(-1, 3).astype(dtype)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = p.shape[0]
    dist, face, point = np.full(n, np.inf, dtype=dtype), np.full(n, -1, dtype=np.int32), np.full((n, 3), np.nan, dtype=dtype)
    in_range = ((f >= 0) & (f < v.shape[0])).all(1)
    tri = v[np.where(in_range[:, None], f, 0)]                                    # [F,3,3]
    usable = np.flatnonzero(in_range & np.isfinite(tri).all((1, 2)))             # increasing: argmin picks the lowest index among equals
    tri = tri[usable]
    ok = np.isfinite(p).all(1)
    dist[~ok] = np.nan
    rows = np.flatnonzero(ok)
    if usable.size and rows.size:
        step = max(1, pairs // usable.size)
        for s in range(0, rows.size, step):
            r = rows[s:s + step]
            d, _ = point_triangle(p[r, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], dtype)
            d = np.where(np.isnan(d), np.inf, d)
            j = np.argmin(d, axis=1)                                              # the first of equal minima
            dj = d[np.arange(r.size), j]
            hit = dj < np.inf
            _, q = point_triangle(p[r], tri[j, 0], tri[j, 1], tri[j, 2], dtype)
            dist[r] = dj
            face[r] = np.where(hit, usable[j], -1)
            point[r] = np.where(hit[:, None], p[r] + q, np.nan)
    return dist, face, point


def _mesh_args(verts, faces):
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f'a mesh is verts [V,3] and faces [F,3], got {tuple(verts.shape)} and {tuple(faces.shape)}')


class TriangleGrid:
    """The search structure of one mesh on the device, built once: packed triangles and a uniform grid of triangle lists (CSR) over
    the bounding box of the finite vertices.  ``cells``: None (about one cell per triangle), an int or a triple.  A triangle whose
    bounding box covers more than 64 cells is kept in a separate list that every query tests, so the structure stays bounded for
    meshes that mix millions of small triangles with a few that span the box.  ``closest(points)`` -> {'dist','face','point'}; the
    structure changes no result (see ``closest_point``)."""

    def __init__(self, verts, faces, cells=None, build=True):
        from . import hipops
        _mesh_args(verts, faces)
        if not (isinstance(verts, torch.Tensor) and verts.is_cuda):
            raise ValueError('TriangleGrid holds device tensors; CPU meshes go to closest_point directly')
        self.verts = verts.detach().float().contiguous()
        self.faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
        self.tris = hipops.tri_pack(self.verts, self.faces)
        fin = self.verts[torch.isfinite(self.verts).all(1)]
        if fin.shape[0]:
            box = torch.stack([fin.amin(0), fin.amax(0)]).cpu().tolist()           # one host synchronisation
        else:
            box = [[0.0] * 3, [0.0] * 3]
        self.lo, self.hi = box
        self.extent = max(max(abs(x) for x in self.lo), max(abs(x) for x in self.hi))
        self.grid = None
        if build:
            self.dims, self.inv_cell = hipops.trigrid_plan(self.faces.shape[0], self.lo, self.hi, cells)
            self.cell_start, self.cell_tris, self.entries, self.n_over = hipops.trigrid_build(self.tris, self.lo, self.inv_cell, self.dims)
            self.grid = (self.lo, self.inv_cell, self.dims, self.cell_start, self.cell_tris, self.entries, self.n_over)

    def closest(self, points, brute=False, sort=True):
        """{'dist' [N], 'face' int64 [N], 'point' [N,3]} for points [N,3] on the grid's device.  ``sort``: query in the order of the
        points' cells (neighbouring lanes then walk the same lists) and return in the caller's order."""
        from . import hipops
        pts = points.detach().to(self.verts.device).float().reshape(-1, 3).contiguous()
        grid = None if brute else self.grid
        order = None
        if sort and grid is not None and pts.shape[0] > 64:
            lo = torch.tensor(self.lo, device=pts.device)
            inv = torch.tensor(self.inv_cell, device=pts.device)
            top = torch.tensor(self.dims, device=pts.device) - 1
            c = torch.minimum(((pts - lo) * inv).floor().nan_to_num(0.0, 0.0, 0.0).clamp(0, 1024).long(), top)
            order = torch.argsort((c[:, 0] * self.dims[1] + c[:, 1]) * self.dims[2] + c[:, 2])
            pts = pts[order]
        dist, face, point = hipops.closest_point(pts, self.tris, self.extent, grid)
        if order is not None:
            back = torch.empty_like(order)
            back[order] = torch.arange(order.numel(), device=order.device)
            dist, face, point = dist[back], face[back], point[back]
        return {'dist': dist, 'face': face.long(), 'point': point}


def closest_point(points, verts, faces, grid=None, brute=False, search='grid', tree=None):
    """Exact distance from points [N,3] to the triangle mesh (verts float32 [V,3], faces [F,3]): ``{'dist' float32 [N] (unsigned),
    'face' int64 [N], 'point' float32 [N,3]}``.  The distance to a triangle is the distance to the closed triangle (a triangle of zero
    area is a segment or a point; a triangle with a non-finite vertex is ignored), the distance to the mesh the minimum over its
    triangles; ``face`` is the triangle that attains the minimum (the lowest index among equal distances) and ``point`` the closest
    point on it.  A non-finite query gives NaN / -1 / NaN, a mesh without usable triangles +inf / -1 / NaN.  Device tensors run on
    ia_closest_point, through ``grid`` (a ``TriangleGrid`` of this mesh; built here if None) or, with ``brute=True``, over all triangles:
    both give bit-identical results.  CPU tensors and NumPy arrays take the NumPy restatement (float64, brute force in chunks).

    ``search='tree'`` takes ``WindingTree.closest`` instead: branch and bound over the cluster tree (``tree``: a ``WindingTree`` of
    this mesh, built here if None; on the device ``grid`` only lends its packed triangles).  The tree prunes and nothing else: the same
    bits again, fast far from the mesh where the grid walks every cell.  CPU tensors and NumPy arrays take ``_closest_tree_numpy`` in
    float64."""
    _mesh_args(verts, faces)
    _closest_search(search)
    if search == 'tree' and brute:
        raise ValueError("search='tree' and brute=True exclude each other")
    if search != 'tree' and tree is not None:
        raise ValueError("tree is used with search='tree' only")
    on_dev = isinstance(verts, torch.Tensor) and verts.is_cuda
    if search == 'tree':
        if not on_dev and faces.shape[0] and (_np(faces).min() < 0 or _np(faces).max() >= verts.shape[0]):
            raise ValueError(f'faces index vertices outside [0, {verts.shape[0]})')
        return _winding_tree_for(verts, faces, grid, tree).closest(points)
    if on_dev:
        if grid is None:
            grid = TriangleGrid(verts, faces, build=not brute)
        return grid.closest(points, brute=brute)
    if faces.shape[0] and (_np(faces).min() < 0 or _np(faces).max() >= verts.shape[0]):
        raise ValueError(f'faces index vertices outside [0, {verts.shape[0]})')
    lead = tuple(points.shape[:-1])
    dist, face, point = _closest_numpy(_np(points), _np(verts), _np(faces))
    return {'dist': _as_out(dist.reshape(lead), points), 'face': _as_out(face.reshape(lead), points, np.int64),
            'point': _as_out(point.reshape(lead + (3,)), points)}


def face_normals(verts, faces):
    """Unit normals [F,3] of the faces, ``(B - A) x (C - A)`` normalised (0 for a face without area).  Torch tensors stay on their
    device; NumPy in, NumPy out."""
    v, f = torch.as_tensor(verts).float(), torch.as_tensor(faces).long()
    f = f.to(v.device)
    n = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=-1)
    nrm = n.norm(dim=-1, keepdim=True)
    out = torch.where(nrm > 0, n / nrm.clamp_min(1e-38), torch.zeros_like(n))
    return out if isinstance(verts, torch.Tensor) else out.numpy()


def sample_surface(verts, faces, n, seed=0):
    """``n`` points distributed uniformly over the surface: ``(points float32 [n,3], face int64 [n])``.  The face is drawn with
    probability proportional to its area (float64 cumulative areas + ``searchsorted``), the point on it with square-root barycentrics
    ``(1 - sqrt(u), sqrt(u) (1 - v), sqrt(u) v)``; all draws come from a CPU generator seeded with ``seed``, so the samples are the
    same on every device.  Faces with a non-finite vertex have no area here."""
    v, f = torch.as_tensor(verts).float(), torch.as_tensor(faces).long()
    f = f.to(v.device)
    tri = v[f].double()
    area = 0.5 * torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1).norm(dim=-1)
    area = torch.where(torch.isfinite(area), area, torch.zeros_like(area))
    cum = torch.cumsum(area, 0)
    if f.shape[0] == 0 or not float(cum[-1]) > 0:
        raise ValueError('sample_surface: the mesh has no area')
    gen = torch.Generator().manual_seed(int(seed))
    u = torch.rand(int(n), 3, generator=gen, dtype=torch.float64).to(v.device)
    idx = torch.searchsorted(cum, u[:, 0] * cum[-1], right=True).clamp_max(f.shape[0] - 1)
    s = u[:, 1].sqrt()
    w = torch.stack([1 - s, s * (1 - u[:, 2]), s * u[:, 2]], -1)
    pts = (w[:, :, None] * tri[idx]).sum(1).float()
    if isinstance(verts, torch.Tensor):
        return pts, idx
    return pts.numpy(), idx.numpy()


def _stats_numpy(dist, thresholds, face=None, na=None, nb=None):
    """NumPy restatement of ia_distance_stats (float64)."""
    d = np.asarray(dist, dtype=F32)
    ok = np.isfinite(d)
    x = d[ok].astype(np.float64)
    out = np.zeros(14)
    out[0], out[1], out[2], out[3], out[5] = x.size, x.sum(), (x * x).sum(), x.max() if x.size else -np.inf, d.size - x.size
    if face is not None:
        fa = np.asarray(face)
        use = ok & (fa >= 0) & (fa < len(nb))
        a, b = np.asarray(na, dtype=np.float64)[use], np.asarray(nb, dtype=np.float64)[fa[use]]
        out[4] = np.abs((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).sum()
    for k, t in enumerate(thresholds):
        out[6 + k] = np.count_nonzero(d[ok] <= F32(t))
    return out


def _sample_set(verts, faces, samples, seed, points):
    """(points, their face normals or None): the vertices, area-weighted samples, or the points given."""
    if points is not None:
        return points, None
    if samples is None:
        return verts, None
    pts, idx = sample_surface(verts, faces, samples, seed)
    nrm = face_normals(verts, faces)
    return pts, nrm[idx]


def _distance_report(s_ab, s_ba, thresholds, with_normals=False):
    """The result of ``surface_distance`` from the two rows of ia_distance_stats."""
    def direction(s):
        cnt = s[0]
        if cnt == 0:
            return float('nan'), float('nan'), float('nan'), float('nan'), [0.0] * len(thresholds)
        return s[1] / cnt, s[2] / cnt, float(np.sqrt(s[2] / cnt)), s[3], [float(s[6 + k] / cnt) for k in range(len(thresholds))]
    mean_ab, sq_ab, rms_ab, max_ab, prec = direction(s_ab)
    mean_ba, sq_ba, rms_ba, max_ba, rec = direction(s_ba)
    res = {'mean_ab': float(mean_ab), 'rms_ab': rms_ab, 'max_ab': float(max_ab), 'mean_ba': float(mean_ba), 'rms_ba': rms_ba,
           'max_ba': float(max_ba), 'chamfer': float((mean_ab + mean_ba) / 2), 'chamfer_sq': float(sq_ab + sq_ba),
           'hausdorff': float(max(max_ab, max_ba)), 'thresholds': thresholds, 'precision': prec, 'recall': rec,
           'fscore': [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(prec, rec)],
           'normal_consistency': None, 'n_a': int(s_ab[0] + s_ab[5]), 'n_b': int(s_ba[0] + s_ba[5]),
           'skipped_ab': int(s_ab[5]), 'skipped_ba': int(s_ba[5])}
    if with_normals and s_ab[0] + s_ba[0] > 0:
        res['normal_consistency'] = float((s_ab[4] / max(s_ab[0], 1) + s_ba[4] / max(s_ba[0], 1)) / 2)
    return res


def _surface_cloud_distance(verts_a, faces_a, verts_b, faces_b, samples, seed, thresholds, points_a, points_b, search):
    """``surface_distance`` with a cloud on either side: the distance to a cloud is ``nearest_points`` (k = 1), the distance to a mesh
    ``closest_point``; the sample set of a cloud is its points (or the points given)."""
    thresholds = _cloud_thresholds(thresholds, verts_a, verts_b)
    on_dev = _is_device(verts_a)
    if on_dev != _is_device(verts_b):
        raise ValueError('both sides must be device tensors or both be on the host')
    sides = ((verts_a, faces_a, points_a, seed), (verts_b, faces_b, points_b, seed + 1))
    pts = [(p if p is not None else v) if f is None else _sample_set(v, f, samples, s, p)[0] for v, f, p, s in sides]
    stats = []
    for own, (v, f, _, _) in ((pts[0], sides[1]), (pts[1], sides[0])):
        if f is None:
            stats.append(_cloud_stats(own, v, thresholds))
            continue
        _mesh_args(v, f)
        dist = closest_point(own, v, f, search=search)['dist']
        if on_dev:
            from . import hipops
            stats.append(hipops.distance_stats(dist.contiguous(), thresholds).cpu().numpy())
        else:
            stats.append(_stats_numpy(_np(dist), thresholds))
    return _distance_report(stats[0], stats[1], thresholds)


def surface_distance(verts_a, faces_a, verts_b, faces_b=None, samples=None, seed=0, thresholds=None, points_a=None, points_b=None,
                     signed=False, winding='exact', beta=2.0, search='grid'):
    """How far surface a is from surface b.  The sample set of each mesh is its vertices (``samples=None``), ``samples`` area-weighted
    points (``sample_surface`` with ``seed`` for a and ``seed + 1`` for b) or the points given (``points_a`` / ``points_b``).  With
    ``d_ab`` the exact distances of a's samples to mesh b and ``d_ba`` those of b's samples to mesh a (``closest_point``; non-finite
    distances are left out and counted in ``skipped_ab`` / ``skipped_ba``), the result is a dict of plain floats and per-threshold lists:

    - ``mean_ab``, ``rms_ab``, ``max_ab`` and ``mean_ba``, ``rms_ba``, ``max_ba``: mean, root mean square and maximum per direction;
    - ``chamfer = (mean_ab + mean_ba) / 2``;  ``chamfer_sq = mean(d_ab^2) + mean(d_ba^2)``;  ``hausdorff = max(max_ab, max_ba)``;
    - ``thresholds``: the values used (default: 0.5 %, 1 % and 2 % of the larger bounding-box diagonal of the two meshes; at most 8);
      ``precision[k]`` = share of a's samples within ``thresholds[k]`` of b, ``recall[k]`` = share of b's samples within it of a,
      ``fscore[k] = 2 P R / (P + R)`` (0 when ``P + R = 0``);
    - ``normal_consistency``: mean over both directions of ``|n . n'|`` between the normal of the sample's own face and the normal of
      the closest face of the other mesh; it needs samples that know their face, so it is None unless ``samples`` is given;
    - ``n_a``, ``n_b``: the numbers of samples;
    - with ``signed=True`` also ``mean_signed_ab`` / ``mean_signed_ba``: the mean of ``signed_distance`` of the samples of one mesh
      against the other (negative inside; positive ``mean_signed_ab``: a lies outside b, it is inflated against it), and
      ``inside_share_ab`` / ``inside_share_ba``: the share of those samples whose winding number is at least 0.5.  Both are over the
      samples with a finite distance (NaN when there is none).  This costs n_a F_b + n_b F_a pairs (``winding_number``);
      ``winding='tree'`` takes ``winding_number(method='tree', beta=beta)`` instead, one ``WindingTree`` per mesh.

    ``search='tree'`` takes the distances through ``closest_point(search='tree')`` (the same bits; no uniform grid is built, and with
    ``winding='tree'`` the one ``WindingTree`` per mesh serves both): the choice for meshes that do not overlap.

    Device meshes run on the kernels (one ``TriangleGrid`` per mesh, ia_distance_stats for the sums); CPU tensors and NumPy arrays take
    the NumPy restatements.

    ``faces_b=None`` (or ``faces_a=None``) makes that side a point cloud: its sample set is its points (or ``points_b``), the distance
    to it is that to its nearest point (``nearest_points``), the distance to a mesh stays ``closest_point``; ``normal_consistency`` is
    None, and ``signed`` needs two surfaces."""
    if faces_a is None or faces_b is None:
        if signed:
            raise ValueError('signed=True needs a surface on both sides: a point cloud has no inside')
        _closest_search(search)
        return _surface_cloud_distance(verts_a, faces_a, verts_b, faces_b, samples, seed, thresholds, points_a, points_b, search)
    _mesh_args(verts_a, faces_a)
    _mesh_args(verts_b, faces_b)
    _winding_method(winding, 'winding')
    _closest_search(search)
    by_tree = search == 'tree'
    if winding == 'tree':
        _winding_beta(beta)
    use_tree = bool(signed) and winding == 'tree'
    on_dev = isinstance(verts_a, torch.Tensor) and verts_a.is_cuda
    if thresholds is None:
        diag = 0.0
        for v in (verts_a, verts_b):
            x = torch.as_tensor(_np(v) if not on_dev else v).float()
            x = x[torch.isfinite(x).all(1)]
            if x.shape[0]:
                diag = max(diag, float((x.amax(0) - x.amin(0)).double().norm()))
        thresholds = [0.005 * diag, 0.01 * diag, 0.02 * diag]
    thresholds = [float(F32(t)) for t in thresholds]
    if len(thresholds) > 8:
        raise ValueError(f'at most 8 thresholds, got {len(thresholds)}')
    pa, na = _sample_set(verts_a, faces_a, samples, seed, points_a)
    pb, nb = _sample_set(verts_b, faces_b, samples, seed + 1, points_b)
    fn_a = face_normals(verts_a, faces_a) if na is not None else None
    fn_b = face_normals(verts_b, faces_b) if nb is not None else None
    if on_dev:
        from . import hipops
        grid_a, grid_b = TriangleGrid(verts_a, faces_a, build=not by_tree), TriangleGrid(verts_b, faces_b, build=not by_tree)
        stats, sides = [], []
        for pts, nrm, grid, fn in ((pa, na, grid_b, fn_b), (pb, nb, grid_a, fn_a)):
            tree = WindingTree.from_grid(grid) if by_tree or use_tree else None
            r = tree.closest(pts) if by_tree else grid.closest(pts)
            if signed:
                sides.append((r['dist'], tree.query(pts, beta) if use_tree else _winding_device(pts, None, None, grid)))
            if nrm is not None:
                s = hipops.distance_stats(r['dist'], thresholds, r['face'].int(), nrm.float().contiguous(), fn.float().contiguous())
            else:
                s = hipops.distance_stats(r['dist'], thresholds)
            stats.append(s)
        s_ab, s_ba = torch.stack(stats).cpu().numpy()
    else:
        out, sides = [], []
        for pts, nrm, v, f, fn in ((pa, na, verts_b, faces_b, fn_b), (pb, nb, verts_a, faces_a, fn_a)):
            tree = WindingTree(_np(v), _np(f)) if by_tree or use_tree else None
            r = closest_point(_np(pts), _np(v), _np(f), search=search, tree=tree if by_tree else None)
            if signed:
                sides.append((r['dist'], tree.query(_np(pts), beta) if use_tree else _winding_numpy(_np(pts), _np(v), _np(f))[0]))
            out.append(_stats_numpy(r['dist'], thresholds, *((r['face'], _np(nrm), _np(fn)) if nrm is not None else ())))
        s_ab, s_ba = out
    res = _distance_report(s_ab, s_ba, thresholds, na is not None and nb is not None)
    if signed:
        for tag, (dist, w) in zip(('ab', 'ba'), sides):
            d, w = _np(dist).astype(np.float64).reshape(-1), _np(w).reshape(-1)
            ok = np.isfinite(d)
            neg = w[ok] >= 0.5
            res[f'mean_signed_{tag}'] = float(np.where(neg, -d[ok], d[ok]).mean()) if ok.any() else float('nan')
            res[f'inside_share_{tag}'] = float(neg.mean()) if ok.any() else float('nan')
    return res


# ------------------------------------------------------------------ alignment

EPS32 = float(np.finfo(np.float32).eps)
_ALIGN_MIN = {'point': 3, 'plane': 6}
_LSTSQ_RCOND = 1e-12         # singular values of the plane system below this share of the largest are directions that do not move


def _matrix44(M):
    m = np.asarray(_np(M), dtype=np.float64)
    if m.shape == (3, 4):
        m = np.concatenate([m, [[0.0, 0.0, 0.0, 1.0]]])
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise ValueError(f'a transform is a finite 4x4 (or 3x4) matrix, got shape {m.shape}')
    return m


def _transform_numpy(x, M, dtype=F32):
    """NumPy restatement of ia_transform_points: ``((m0 x + m1 y) + m2 z) + t`` per row in ``dtype`` with ``M`` rounded to it."""
    x = np.asarray(x, dtype=F32).reshape(-1, 3).astype(dtype)
    m = _matrix44(M).astype(dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([((m[r, 0] * x[:, 0] + m[r, 1] * x[:, 1]) + m[r, 2] * x[:, 2]) + m[r, 3] for r in range(3)], -1).astype(dtype)


def transform_points(points, M):
    """``y = M x`` for points [..., 3] and a 4x4 (or 3x4) transform ``M = [s R | t]`` given as floats on the host: float32 arithmetic
    with ``M`` rounded to float32, per row ``((m0 x + m1 y) + m2 z) + t``.  Device tensors run on ia_transform_points, CPU tensors
    and NumPy arrays on the NumPy restatement of it (the same operations in the same order)."""
    m = _matrix44(M)
    if points.shape[-1] != 3:
        raise ValueError(f'points must be [..., 3], got {tuple(points.shape)}')
    if isinstance(points, torch.Tensor) and points.is_cuda:
        from . import hipops
        return hipops.transform_points(points.detach().float().reshape(-1, 3).contiguous(), m).reshape(points.shape)
    return _as_out(_transform_numpy(_np(points), m).reshape(tuple(points.shape)), points)


def _rodrigues(w):
    """The rotation about ``w`` by ``|w|``."""
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w, dtype=np.float64) / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def _about(A, t, c):
    """4x4 of ``y = c + A (x - c) + t``."""
    M = np.eye(4)
    M[:3, :3] = A
    M[:3, 3] = c + t - A @ c
    return M


def _align_terms_numpy(p, q, dist, face, normals, centre, max_dist, metric):
    """The terms of ia_align_sums in float64: ``(terms [m, 19 or 55], rejected)``, one row per pair that counts, in index order.
    ``max_dist``: the one effective threshold (compared in float32), +inf for none."""
    p, q = np.asarray(p, dtype=np.float64).reshape(-1, 3), np.asarray(q, dtype=np.float64).reshape(-1, 3)
    d, f = np.asarray(dist).astype(F32).reshape(-1), np.asarray(face).astype(np.int64).reshape(-1)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(d) & (f >= 0) & (d <= F32(max_dist))
    if metric == 'plane':
        nrm = np.asarray(normals, dtype=F32).reshape(-1, 3)
        ok &= f < nrm.shape[0]
        n_all = nrm[np.where(ok, f, 0)] if nrm.shape[0] else np.zeros((f.size, 3), dtype=F32)
        ok &= np.isfinite(n_all).all(1) & (n_all != 0).any(1)
    c = np.asarray(centre, dtype=np.float64)
    p, q = p[ok] - c, q[ok] - c
    e = p - q
    cols = [np.ones(p.shape[0]), p[:, 0], p[:, 1], p[:, 2], q[:, 0], q[:, 1], q[:, 2]]
    cols += [p[:, i] * q[:, j] for i in range(3) for j in range(3)]
    cols += [_dot3(p, p), _dot3(q, q), _dot3(e, e)]
    if metric == 'plane':
        n = n_all[ok].astype(np.float64)
        a = np.concatenate([_cross3(p, n), n, _dot3(p, n)[:, None]], 1)
        b = _dot3(q - p, n)
        cols += [a[:, i] * a[:, j] for i in range(7) for j in range(i, 7)]
        cols += [a[:, i] * b for i in range(7)] + [b * b]
    return np.stack(cols, 1), int(ok.size - np.count_nonzero(ok))


def _column_sums(terms):
    """The correctly rounded sum of every column (``math.fsum``): the restatement's sums do not depend on the order of the rows."""
    import math
    return np.array([math.fsum(col) for col in np.asarray(terms, dtype=np.float64).T.tolist()], dtype=np.float64).reshape(terms.shape[1])


def _align_sums_numpy(p, q, dist, face, normals, centre, max_dist, metric):
    """NumPy restatement of ia_align_sums: float64 [20] (point) or [56] (plane), the last slot the pairs left out."""
    terms, rejected = _align_terms_numpy(p, q, dist, face, normals, centre, max_dist, metric)
    return np.concatenate([_column_sums(terms), [float(rejected)]])


def _solve_point(S, scale, centre, floor=0.0):
    """Umeyama / Horn from the 19 point sums (taken about ``centre``): the 4x4 that maps p onto q in the least-squares sense."""
    n = S[0]
    pm, qm = S[1:4] / n, S[4:7] / n
    H = S[7:16].reshape(3, 3) - n * np.outer(pm, qm)
    var = S[16] - n * float(pm @ pm)
    if not np.isfinite(H).all() or not var > floor:
        raise ValueError('the source points coincide (or are not finite): no transform is determined')
    U, sig, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, float(np.sign(np.linalg.det(Vt.T @ U.T))) or 1.0])
    R = Vt.T @ D @ U.T
    s = float((sig * np.diag(D)).sum() / var) if scale else 1.0
    if not s > 0:
        raise ValueError('the correspondences determine no positive scale')
    return _about(s * R, qm - s * R @ pm, np.asarray(centre, dtype=np.float64))


def _solve_plane(S, scale, centre):
    """One Gauss-Newton step of the point-to-plane objective from the 55 plane sums: minimum-norm solution of the 6x6 (7x7 with scale)
    normal equations, the rotation taken exactly (Rodrigues), acting about ``centre``."""
    k = 7 if scale else 6
    A = np.zeros((7, 7))
    A[np.triu_indices(7)] = S[19:47]
    A = A + np.triu(A, 1).T
    x = np.linalg.lstsq(A[:k, :k], S[47:47 + k], rcond=_LSTSQ_RCOND)[0]
    s = 1.0 + (float(x[6]) if scale else 0.0)
    if not s > 0:
        raise ValueError('the step would make the scale non-positive: the start is too far from the target')
    return _about(s * _rodrigues(x[:3]), x[3:6], np.asarray(centre, dtype=np.float64))


def _align_residual(S, metric):
    """(rms of the pairs that count, their number) from the sums of one pairing."""
    n = int(S[0])
    if n < _ALIGN_MIN[metric]:
        raise ValueError(f"align_mesh: {n} pairs count, metric '{metric}' needs at least {_ALIGN_MIN[metric]}")
    return float(np.sqrt(max(S[18], 0.0) / n)), n


def _align_solve(S, metric, scale, centre):
    """The increment (float64 4x4) from the sums of one pairing; shared by the device path and the restatement."""
    return _solve_point(S, scale, centre) if metric == 'point' else _solve_plane(S, scale, centre)


def fit_transform(src, dst, scale=False, weights=None):
    """The transform ``y = s R x + t`` (float64 4x4, ``M[:3,:3] = s R``) that maps points ``src`` [N,3] onto their correspondences ``dst``
    [N,3] in the least-squares sense (Umeyama / Horn, optionally weighted): ``H = sum w (p - pm)(q - qm)^T = U S V^T``,
    ``R = V diag(1, 1, det(V U^T)) U^T`` (a proper rotation also for a mirrored target), ``s = tr(S D) / sum w |p - pm|^2`` with
    ``scale=True`` and 1 otherwise, ``t = qm - s R pm``.  A plain float64 host solve for landmarks, e.g. to start ``align_mesh``.  Fewer
    than 3 pairs, or source points that coincide, raise ValueError."""
    p, q = np.asarray(_np(src), dtype=np.float64).reshape(-1, 3), np.asarray(_np(dst), dtype=np.float64).reshape(-1, 3)
    if p.shape != q.shape:
        raise ValueError(f'src and dst must both be [N,3], got {p.shape} and {q.shape}')
    w = np.ones(p.shape[0]) if weights is None else np.asarray(_np(weights), dtype=np.float64).reshape(-1)
    if w.shape[0] != p.shape[0] or not np.isfinite(w).all() or (w < 0).any():
        raise ValueError('weights must be N finite numbers >= 0')
    use = w > 0
    if np.count_nonzero(use) < 3:
        raise ValueError(f'fit_transform needs at least 3 pairs, got {np.count_nonzero(use)}')
    if not (np.isfinite(p[use]).all() and np.isfinite(q[use]).all()):
        raise ValueError('fit_transform: the points must be finite')
    p, q, w = p[use], q[use], w[use]
    c = (w[:, None] * p).sum(0) / w.sum()
    pc, qc = p - c, q - c
    S = np.concatenate([[w.sum()], (w[:, None] * pc).sum(0), (w[:, None] * qc).sum(0),
                        ((w[:, None] * pc)[:, :, None] * qc[:, None, :]).sum(0).reshape(-1),
                        [(w * _dot3(pc, pc)).sum(), (w * _dot3(qc, qc)).sum(), (w * _dot3(pc - qc, pc - qc)).sum()]])
    floor = w.sum() * (16 * np.finfo(np.float64).eps * max(float(np.abs(p).max()), np.finfo(np.float64).tiny)) ** 2
    return _solve_point(S, scale, c, floor)


def _finite_rows(x):
    return x[np.isfinite(x).all(1)]


def _centroid_init(src, verts, scale):
    """Centroid of the finite source points onto the centroid of the finite target vertices; with ``scale`` also rms radius onto rms radius."""
    a, b = _finite_rows(np.asarray(src, dtype=np.float64)), _finite_rows(np.asarray(verts, dtype=np.float64))
    if not a.shape[0] or not b.shape[0]:
        raise ValueError("init='centroid' needs finite source points and target vertices")
    ca, cb = a.mean(0), b.mean(0)
    s = 1.0
    if scale:
        ra, rb = np.sqrt(((a - ca) ** 2).sum(1).mean()), np.sqrt(((b - cb) ** 2).sum(1).mean())
        if not (ra > 0 and rb > 0):
            raise ValueError("init='centroid' with scale needs point sets with an extent")
        s = float(rb / ra)
    M = np.eye(4)
    M[:3, :3] *= s
    M[:3, 3] = cb - s * ca
    return M


def _trim_threshold_numpy(dist, face, max_dist, trim):
    """The one effective threshold ``min(max_dist, tau)`` as float32; tau: the ``ceil(trim n_finite)``-th smallest finite distance."""
    thr = F32(np.inf) if max_dist is None else F32(max_dist)
    if trim < 1.0:
        d = np.asarray(dist).astype(F32)
        fin = d[np.isfinite(d) & (np.asarray(face) >= 0)]
        if fin.size:
            k = max(int(np.ceil(trim * float(fin.size))), 1)
            thr = min(thr, np.partition(fin, k - 1)[k - 1])
    return float(thr)


def _align_loop(pair, centre, extent, M0, metric, scale, iterations, tol):
    """Steps 1 to 6 of ``align_mesh`` around ``pair(M) -> sums`` (float64 [20] or [56])."""
    M, hist, steps, converged, n = M0, [], 0, False, 0
    for k in range(iterations + 1):
        S = np.asarray(pair(M), dtype=np.float64)
        rms, n = _align_residual(S, metric)
        hist.append(rms)
        if rms <= EPS32 * extent or (k > 0 and abs(hist[k - 1] - rms) <= tol * hist[k - 1]):
            converged = True
            break
        if k == iterations:
            break
        M = _align_solve(S, metric, scale, centre) @ M
        steps += 1
    A = M[:3, :3]
    s = float(np.cbrt(np.linalg.det(A)))
    return {'matrix': M, 'scale': s, 'rotation': A / s, 'translation': M[:3, 3].copy(), 'rms': hist[-1], 'rms_history': hist,
            'inliers': n, 'iterations': steps, 'converged': converged}


def _align_numpy(src, verts, faces, M0, metric, scale, iterations, tol, max_dist, trim, dtype=np.float64, search='grid'):
    """The NumPy restatement of ``align_mesh`` (the definition); ``dtype``: the precision of the closest-point search."""
    src, verts, faces = np.asarray(src, dtype=F32).reshape(-1, 3), np.asarray(verts, dtype=F32), np.asarray(faces, dtype=np.int64)
    fin = _finite_rows(verts)
    if not faces.shape[0] or not fin.shape[0]:
        raise ValueError('align_mesh: the target mesh is empty')
    lo, hi = fin.min(0).astype(np.float64), fin.max(0).astype(np.float64)
    centre, extent = (lo + hi) / 2, float(max(np.abs(lo).max(), np.abs(hi).max()))
    normals = face_normals(verts, faces) if metric == 'plane' else None
    tree = WindingTree(verts, faces) if search == 'tree' else None

    def pair(M):
        p = _transform_numpy(src, M)
        dist, face, q = _closest_numpy(p, verts, faces, dtype) if tree is None else _closest_tree_numpy(p, tree, dtype)[:3]
        return _align_sums_numpy(p, q, dist, face, normals, centre, _trim_threshold_numpy(dist, face, max_dist, trim), metric)
    return _align_loop(pair, centre, extent, M0, metric, scale, iterations, tol)


def _cloud_normals(points, normals, normals_k, metric):
    """The per-point normals of the plane metric against a cloud: those given, or ``estimate_normals(k=normals_k)``."""
    if metric != 'plane':
        return None
    if normals is None:
        return estimate_normals(points, normals_k)['normal']
    if tuple(normals.shape) != tuple(points.shape):
        raise ValueError(f'normals must be one row per target point, got {tuple(normals.shape)} for {tuple(points.shape)}')
    return normals


def _align_cloud_numpy(src, points, normals, M0, metric, scale, iterations, tol, max_dist, trim, dtype=np.float64):
    """``_align_numpy`` against a point cloud: the pairing is ``nearest_points(k=1)``, q the nearest point, face its index, and the
    plane metric reads the per-point ``normals``; everything else is the same."""
    src, points = np.asarray(src, dtype=F32).reshape(-1, 3), np.asarray(points, dtype=F32).reshape(-1, 3)
    fin = _finite_rows(points)
    if not fin.shape[0]:
        raise ValueError('align_mesh: the target cloud is empty')
    lo, hi = fin.min(0).astype(np.float64), fin.max(0).astype(np.float64)
    centre, extent = (lo + hi) / 2, float(max(np.abs(lo).max(), np.abs(hi).max()))
    normals = None if normals is None else np.asarray(normals, dtype=F32).reshape(-1, 3)
    tree = PointTree(points)

    def pair(M):
        p = _transform_numpy(src, M)
        dist, index = _nearest_tree_numpy(p, tree, 1, dtype=dtype)
        dist, face = dist[:, 0], index[:, 0]
        q = np.where(face[:, None] >= 0, points[np.maximum(face, 0)], F32(np.nan)).astype(dtype)
        return _align_sums_numpy(p, q, dist, face, normals, centre, _trim_threshold_numpy(dist, face, max_dist, trim), metric)
    return _align_loop(pair, centre, extent, M0, metric, scale, iterations, tol)


def _align_cloud_device(src, points, normals, M0, metric, scale, iterations, tol, max_dist, trim):
    from . import hipops
    tree = PointTree(points)
    if not tree.usable:
        raise ValueError('align_mesh: the target cloud is empty')
    dev = tree.device
    src = src.detach().to(dev).float().reshape(-1, 3).contiguous()
    centre = [(float(a) + float(b)) / 2 for a, b in zip(tree.box_lo, tree.box_hi)]
    normals = None if normals is None else normals.detach().to(dev).float().contiguous()
    base = float('inf') if max_dist is None else float(F32(max_dist))

    def pair(M):
        p = hipops.transform_points(src, M)
        r = tree.nearest(p, 1)
        dist, face = r['dist'][:, 0].contiguous(), r['index'][:, 0].contiguous()
        q = torch.where((face >= 0)[:, None], tree.points[face.clamp(min=0).long()], torch.full_like(p, float('nan'))).contiguous()
        thr = base
        if trim < 1.0:
            d = torch.where(torch.isfinite(dist) & (face >= 0), dist, torch.full_like(dist, float('inf'))).sort().values
            n_fin = torch.isfinite(d).sum()
            k = torch.ceil(trim * n_fin.double()).long().clamp(1, max(d.numel(), 1))
            if d.numel():
                thr = min(base, float(d[k - 1]))
        return hipops.align_sums(p, q, dist, face, centre, thr, metric, normals).cpu().numpy()
    return _align_loop(pair, np.asarray(centre), float(tree.extent), M0, metric, scale, iterations, tol)


def _align_device(src, verts, faces, M0, metric, scale, iterations, tol, max_dist, trim, grid, search='grid'):
    from . import hipops
    if not faces.shape[0] or not verts.shape[0]:
        raise ValueError('align_mesh: the target mesh is empty')
    if grid is None:
        grid = TriangleGrid(verts, faces, build=search != 'tree')
    finder = WindingTree.from_grid(grid) if search == 'tree' else grid
    dev = grid.verts.device
    src = src.detach().to(dev).float().reshape(-1, 3).contiguous()
    centre = [(float(a) + float(b)) / 2 for a, b in zip(grid.lo, grid.hi)]
    normals = face_normals(grid.verts, grid.faces).float().contiguous() if metric == 'plane' else None
    base = float('inf') if max_dist is None else float(F32(max_dist))

    def pair(M):
        p = hipops.transform_points(src, M)
        r = finder.closest(p)
        dist, face = r['dist'], r['face'].int()
        thr = base
        if trim < 1.0:                                                    # one more host synchronisation, for tau
            d = torch.where(torch.isfinite(dist) & (face >= 0), dist, torch.full_like(dist, float('inf'))).sort().values
            n_fin = torch.isfinite(d).sum()
            k = torch.ceil(trim * n_fin.double()).long().clamp(1, max(d.numel(), 1))
            if d.numel():
                thr = min(base, float(d[k - 1]))
        return hipops.align_sums(p, r['point'].contiguous(), dist.contiguous(), face.contiguous(), centre, thr, metric, normals).cpu().numpy()
    return _align_loop(pair, np.asarray(centre), float(grid.extent), M0, metric, scale, iterations, tol)


def align_mesh(source, verts, faces=None, metric='plane', scale=False, iterations=30, tol=1e-6, max_dist=None, trim=1.0, init='identity',
               grid=None, search='grid', global_options=None, normals=None, normals_k=16):
    """Align ``source`` (points [N,3], or a ``(verts, faces)`` pair whose vertices are used) to the triangle mesh ``(verts, faces)`` by
    iterated closest points: the rigid (``scale=False``) or similarity transform ``y = s R x + t`` that brings the points onto the
    surface, as a float64 4x4 ``M`` with ``M[:3,:3] = s R``, ``M[:3,3] = t``.  ICP finds the local optimum nearest to the start, so the
    start matters (``init``: 'identity', 'centroid' = centroid onto centroid and, with ``scale``, rms radius onto rms radius, or a 4x4,
    e.g. from ``fit_transform`` on landmarks); a symmetric target leaves the pose undetermined.  One iteration, given ``M_k``:

    1. ``p_i = fp32(M_k) x_i`` in float32 from the original points (``transform_points``);
    2. ``(d_i, f_i, q_i)``: the closest point of the target mesh (``closest_point``);
    3. pair i counts iff ``d_i`` is finite and ``f_i >= 0``, ``d_i <= max_dist`` if given, ``d_i <= tau`` if ``trim < 1`` (tau: the
       ``ceil(trim n_finite)``-th smallest finite distance; ties stay in) and, for ``metric='plane'``, the normal of face ``f_i`` is not 0;
    4. float64 sums over these pairs, p and q taken relative to the middle of the target's bounding box (see ia_align_sums);
    5. the step, solved on the host in float64: ``'point'``: Umeyama / Horn on the pairs (``fit_transform``); ``'plane'``: the
       minimum-norm solution of the 6x6 (7x7 with ``scale``) normal equations of ``sum ((p + w x p + u + z p - q) . n)^2``, applied as
       the exact rotation about ``w`` by ``|w|``, the scale ``1 + z`` and the shift ``u`` (a planar target slides nowhere);
    6. ``M_{k+1} = step M_k``; ``rms_k = sqrt(sum |p - q|^2 / n)`` is the residual before the step.  The loop ends after ``iterations``
       steps, or earlier when ``|rms_{k-1} - rms_k| <= tol rms_{k-1}`` or ``rms_k <= eps32 extent`` (``converged``); the last pairing
       follows the last step and gives ``rms``.

    Returns ``{'matrix', 'scale', 'rotation' [3,3], 'translation' [3], 'rms', 'rms_history' (one entry per pairing), 'inliers' (pairs
    that counted in the last pairing), 'iterations' (steps taken), 'converged'}``.  Fewer than 3 (``'point'``) or 6 (``'plane'``) pairs
    that count, or an empty target, raise ValueError.  Device tensors run on the kernels (one ``TriangleGrid`` for all iterations,
    ``grid`` if given; one host synchronisation per iteration for the sums, one more for tau when ``trim < 1``); CPU tensors and NumPy
    arrays take the NumPy restatement, which is the definition.  ``search='tree'`` takes step 2 through ``closest_point(search='tree')``
    (one ``WindingTree`` for all iterations, no uniform grid): the same bits, and the choice for a source that starts outside the
    target's box, where the grid walks every cell.

    ``init='global'`` needs no start: ``M_0 = global_align(...)['matrix']`` with this call's ``metric / scale / trim / max_dist /
    search`` and ``global_options`` (a dict of its other arguments: ``angle_step``, ``candidates``, ``shifts``, ``field``, ...), then the
    loop above; the result gains ``'global': {'candidates', 'searched', 'rank'}``.

    ``faces=None``: the target is the point cloud ``verts``.  Step 2 becomes ``nearest_points(k=1)`` on one ``PointTree``: ``q_i`` is
    the nearest point and ``f_i`` its index; the plane metric reads the per-point ``normals`` ([n,3]; ``estimate_normals(k=normals_k)``
    if None), and a pair counts iff that normal is not 0.  The sums, the threshold, the solve and the loop are the same.  ``grid``,
    ``search`` and ``init='global'`` belong to a mesh target."""
    _closest_search(search)
    if metric not in _ALIGN_MIN:
        raise ValueError(f"metric must be 'point' or 'plane', got {metric!r}")
    if isinstance(source, (tuple, list)) and len(source) == 2 and getattr(source[0], 'ndim', 0) == 2:
        source = source[0]
    cloud = faces is None
    if cloud:
        _cloud_args(verts, 'the target cloud')
        if grid is not None or (isinstance(init, str) and init == 'global'):
            raise ValueError("grid and init='global' need a mesh target (faces)")
    else:
        if normals is not None:
            raise ValueError('normals are those of a cloud target (faces=None); a mesh has its face normals')
        _mesh_args(verts, faces)
    if source.ndim != 2 or source.shape[1] != 3:
        raise ValueError(f'source must be points [N,3] or a (verts, faces) pair, got {tuple(source.shape)}')
    if not 0.0 < float(trim) <= 1.0:
        raise ValueError(f'trim must be in (0, 1], got {trim}')
    if max_dist is not None and not float(max_dist) >= 0:
        raise ValueError(f'max_dist must be >= 0, got {max_dist}')
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f'iterations must be >= 0, got {iterations}')
    on_dev = isinstance(verts, torch.Tensor) and verts.is_cuda
    found = None
    if isinstance(init, str):
        if init == 'identity':
            M0 = np.eye(4)
        elif init == 'centroid':
            if (not cloud and not faces.shape[0]) or not verts.shape[0]:
                raise ValueError('align_mesh: the target mesh is empty')
            M0 = _centroid_init(_np(source), _np(verts), scale)
        elif init == 'global':
            found = global_align(source, verts, faces, metric=metric, scale=scale, trim=trim, max_dist=max_dist, search=search, grid=grid,
                                 **dict(global_options or {}))
            M0 = found['matrix']
        else:
            raise ValueError(f"init must be 'identity', 'centroid', 'global' or a 4x4 matrix, got {init!r}")
    else:
        M0 = _matrix44(init)
    args = (M0, metric, bool(scale), iterations, float(tol), max_dist, float(trim))
    if cloud:
        nrm = _cloud_normals(verts, normals, _nearest_k(normals_k), metric)
        if on_dev:
            return _align_cloud_device(torch.as_tensor(source), verts, nrm, *args)
        return _align_cloud_numpy(_np(source), _np(verts), None if nrm is None else _np(nrm), *args)
    if on_dev:
        res = _align_device(torch.as_tensor(source), verts, faces, *args, grid, search)
    else:
        res = _align_numpy(_np(source), _np(verts), _np(faces), *args, search=search)
    if found is not None:
        res['global'] = {k: found[k] for k in ('candidates', 'searched', 'rank')}
    return res


# ------------------------------------------------------------------ global registration: pose search over a distance field, then ICP

POSE_MAX_POINTS = 4096       # csrc/pose_search.hip kMaxPoints = hipops.POSE_MAX_POINTS
_POSE_HEAD = 4096            # entries of the score order that the selection walks (one host read on the device path)


class PoseField:
    """The unsigned distance of the target mesh ``(verts, faces)`` on a lattice with cubic cells, for ``pose_scores`` and
    ``global_align``: build once per target, hand to many calls.  The lattice is that of ``mesh_to_volume`` (``_volume_lattice``): the
    longest side of the box of the finite vertices gets ``resolution`` points, ``padding`` of them beyond the box on each side.
    ``dist`` float32 [nx,ny,nz] (x slowest) is ``closest_point(search='tree')`` at the lattice points (most of them are off the mesh,
    where the tree prunes best; the same bits as the other searches), a device tensor for a device mesh and a NumPy array otherwise.  Also ``dims``, ``origin`` (three floats),
    ``spacing`` (one float, h), ``centroid`` and ``radius`` (mean and rms radius of the finite vertices, as ``init='centroid'`` takes
    them), ``extent`` (largest absolute coordinate of the box) and ``n_verts`` / ``n_faces`` of the mesh it was made for."""

    def __init__(self, verts, faces, resolution=32, padding=2):
        _mesh_args(verts, faces)
        if not faces.shape[0] or not verts.shape[0]:
            raise ValueError('PoseField: the target mesh is empty')
        box = _finite_box(verts)
        if box is None:
            raise ValueError('PoseField: the target mesh has no finite vertex')
        self.dims, self.origin, spacing = _volume_lattice(box, int(resolution), None, None, padding)
        self.spacing = float(spacing[0])
        b = _finite_rows(np.asarray(_np(verts), dtype=np.float64))
        self.centroid = b.mean(0)
        self.radius = float(np.sqrt(((b - self.centroid) ** 2).sum(1).mean()))
        self.extent = float(max(np.abs(box[0]).max(), np.abs(box[1]).max()))
        self.n_verts, self.n_faces = int(verts.shape[0]), int(faces.shape[0])
        pts = np.ascontiguousarray(np.stack(np.meshgrid(*_lattice_axes(self.dims, self.origin, spacing), indexing='ij'), -1).reshape(-1, 3))
        if _is_device(verts):
            self.device = verts.device
            d = closest_point(torch.from_numpy(pts).to(verts.device), verts, faces, search='tree')['dist']
            self.dist = d.reshape(self.dims).contiguous()
        else:
            self.device = None
            d = closest_point(pts, np.asarray(_np(verts), dtype=F32), _np(faces), search='tree')['dist']
            self.dist = np.ascontiguousarray(d.reshape(self.dims).astype(F32))

    def lookup(self, points, dtype=np.float64):
        """``d(p)`` of the NumPy restatement at points [..., 3] (the lattice is read back from the device if it lives there)."""
        return _pose_lookup_numpy(_np(self.dist), self.origin, self.spacing, np.asarray(_np(points)), dtype)


def _pose_lookup_numpy(dist, origin, h, p, dtype=np.float64):
    """The lookup of ia_pose_scores in ``dtype`` at p [..., 3]: per axis ``u = (p - origin) (1 / h)``, ``c = clamp(u, 0, dim - 1)``,
    ``i = min(floor(c), dim - 2)``, ``t = c - i``; ``d = trilinear(dist, i, t) + h |u - c|_2`` with ``lerp(a, b, t) = a + t (b - a)``
    along z, then y, then x; every operation rounded on its own.  A NaN coordinate gives NaN."""
    v = np.asarray(dist, dtype=F32).astype(dtype)
    p = np.asarray(p).astype(dtype)
    hh, inv = dtype(F32(h)), dtype(1.0 / float(F32(h)))
    idx, t, e = [], [], []
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(3):
            u = (p[..., a] - dtype(F32(origin[a]))) * inv
            c = np.minimum(np.maximum(u, dtype(0)), dtype(v.shape[a] - 1))
            i = np.clip(np.floor(np.where(np.isfinite(c), c, 0)).astype(np.int64), 0, v.shape[a] - 2)
            idx.append(i)
            t.append(c - i.astype(dtype))
            e.append(u - c)
        (i, j, k), (tx, ty, tz) = idx, t
        lerp = lambda a, b, w: a + w * (b - a)                                               # noqa: E731
        c00, c01 = lerp(v[i, j, k], v[i, j, k + 1], tz), lerp(v[i, j + 1, k], v[i, j + 1, k + 1], tz)
        c10, c11 = lerp(v[i + 1, j, k], v[i + 1, j, k + 1], tz), lerp(v[i + 1, j + 1, k], v[i + 1, j + 1, k + 1], tz)
        inside = lerp(lerp(c00, c01, ty), lerp(c10, c11, ty), tx)
        return (inside + hh * np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])).astype(dtype)


def _pose_offsets(shifts):
    shifts = int(shifts)
    if shifts < 1 or shifts % 2 == 0:
        raise ValueError(f'shifts must be odd and >= 1, got {shifts}')
    return shifts


def _pose_scores_numpy(points, dist, origin, h, rotations, c_src, c_tgt, shifts=1, shift_step=None, scale=1.0, cap=np.inf,
                       dtype=np.float64, chunk=1 << 19):
    """NumPy restatement of ia_pose_scores, float64 [R, shifts^3]; ``dtype``: the precision of the per-point term
    ``min(d(p), cap)`` (np.float32 repeats the kernel's operations one by one); its square and the sum are float64 in both."""
    shifts = _pose_offsets(shifts)
    x = np.asarray(points, dtype=F32).reshape(-1, 3).astype(dtype)
    rot = np.asarray(rotations, dtype=np.float64).reshape(-1, 3, 3).astype(F32).astype(dtype)
    n, R, S3 = x.shape[0], rot.shape[0], shifts ** 3
    out = np.full((R, S3), np.nan)
    if n == 0 or R == 0:
        return out
    f = lambda a: np.asarray(a, dtype=np.float64).astype(F32).astype(dtype)                  # noqa: E731
    step = dtype(F32(h if shift_step is None else shift_step))
    s, capv = dtype(F32(scale)), dtype(F32(np.inf if cap is None else cap))
    with np.errstate(invalid='ignore', over='ignore'):
        y = x - f(c_src)
        a = (np.arange(shifts) - (shifts - 1) // 2).astype(dtype) * step
        off = f(c_tgt) + np.stack(np.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)   # [S3,3], x slowest
        per = max(1, chunk // (n * S3))
        for r0 in range(0, R, per):
            m = rot[r0:r0 + per, None]                                                       # [r,1,3,3]
            q = s * ((m[..., 0] * y[None, :, None, 0] + m[..., 1] * y[None, :, None, 1]) + m[..., 2] * y[None, :, None, 2])   # [r,n,3]
            d = _pose_lookup_numpy(dist, origin, h, q[:, None] + off[None, :, None], dtype)  # [r,S3,n]
            term = np.where(d > capv, capv, d).astype(np.float64)
            out[r0:r0 + per] = (term * term).sum(-1) / n
    return out


def pose_candidates(angle_step=15.0):
    """Candidate rotations that cover SO(3) at about ``angle_step`` degrees: float64 [R,3,3].  With theta in radians,
    ``m = ceil(4 pi / theta^2)`` Fibonacci-sphere directions ``d_j = (r cos phi, r sin phi, z)``, ``z = 1 - 2 (j + 1/2) / m``,
    ``r = sqrt(1 - z^2)``, ``phi = (j + 1/2) pi (3 - sqrt 5)``, times ``k = ceil(2 pi / theta)`` spins:
    ``R[j k + l] = A_j Rz(2 pi l / k)`` with ``A_j`` the rotation about ``z x d_j`` that takes z to ``d_j``.  4 416 rotations at 15
    degrees, 1 872 at 20; the largest angle from 300 random rotations to the nearest candidate was 11.09 and 14.88 degrees."""
    theta = np.deg2rad(float(angle_step))
    if not 0.0 < theta <= np.pi / 2:
        raise ValueError(f'angle_step must be in (0, 90] degrees, got {angle_step}')
    m, k = int(np.ceil(4 * np.pi / theta ** 2)), int(np.ceil(2 * np.pi / theta))
    j = np.arange(m) + 0.5
    z = 1.0 - 2.0 * j / m
    r, phi = np.sqrt(1.0 - z * z), j * (np.pi * (3.0 - np.sqrt(5.0)))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)
    spins = np.stack([_rodrigues(np.array([0.0, 0.0, 2 * np.pi * l / k])) for l in range(k)])
    out = np.empty((m, k, 3, 3))
    for a in range(m):
        axis = np.array([-d[a, 1], d[a, 0], 0.0])                                             # z x d
        norm = float(np.linalg.norm(axis))
        A = _rodrigues(axis / norm * np.arctan2(norm, d[a, 2])) if norm > 0 else np.eye(3)
        out[a] = A @ spins
    return out.reshape(m * k, 3, 3)


def _pose_points(points):
    """The finite rows as float32 and their mean (float64)."""
    x = np.asarray(_np(points), dtype=F32).reshape(-1, 3)
    x = np.ascontiguousarray(x[np.isfinite(x).all(1)])
    if x.shape[0] > POSE_MAX_POINTS:
        raise ValueError(f'pose_scores takes at most {POSE_MAX_POINTS} points, got {x.shape[0]}: score a subset (global_align: samples=)')
    if not x.shape[0]:
        raise ValueError('pose_scores: no finite point')
    return x, x.astype(np.float64).mean(0)


def pose_scores(points, field, rotations, shifts=1, shift_step=None, scale=1.0, cap=None):
    """The score of candidate poses of ``points`` [n,3] (float32; non-finite rows are dropped; n <= 4096) against a ``PoseField``:
    float64 ``[R, shifts^3]`` for ``rotations`` [R,3,3].  For rotation r and offset ``o_k`` on the grid
    ``(a - (shifts - 1) / 2) shift_step`` per axis (x slowest, ``shifts`` odd, ``shift_step`` defaults to the field's h):

        ``p_i = s R_r (x_i - c_src) + c_tgt + o_k``,   ``score = sum_i min(d(p_i), cap)^2 / n``

    with ``c_src`` the mean of the points, ``c_tgt`` the field's centroid and ``d`` the lookup of the field: trilinear inside the
    lattice, plus ``h |u - clamp(u)|`` outside it (an upper bound of the true distance up to the interpolation error).  A truncated
    mean square, not a trimmed one.  A field on the device runs ia_pose_scores (a device tensor comes back), a field on the host the
    NumPy restatement, which is the definition."""
    if not isinstance(field, PoseField):
        raise ValueError(f'field must be a PoseField, got {type(field).__name__}')
    shifts = _pose_offsets(shifts)
    x, c_src = _pose_points(points)
    rot = np.asarray(_np(rotations), dtype=np.float64).reshape(-1, 3, 3)
    cap = np.inf if cap is None else float(cap)
    if field.device is not None:
        from . import hipops
        dev = field.device
        return hipops.pose_scores(torch.from_numpy(x).to(dev), field.dist, field.origin, field.spacing,
                                  torch.from_numpy(rot.reshape(-1, 9).astype(F32)).to(dev), c_src, field.centroid, shifts, shift_step, scale, cap)
    return _pose_scores_numpy(x, field.dist, field.origin, field.spacing, rot, c_src, field.centroid, shifts, shift_step, scale, cap)


def _rotation_angle(A, B):
    """The angle of ``A^T B`` in degrees."""
    return float(np.degrees(np.arccos(np.clip((np.trace(A.T @ B) - 1.0) / 2.0, -1.0, 1.0))))


def _pose_select(order, scores, rotations, shifts, angle_step, candidates):
    """Greedy choice among the candidates in rank order (``order``: flat indices ``r shifts^3 + k``, ``scores``: theirs): one is skipped
    when an already chosen one has a relative rotation angle <= 1.5 ``angle_step`` AND grid offsets that differ by at most one step on
    every axis; a NaN score ends the walk.  ``[(rank, flat index, r, (ax, ay, az), score)]``, at most ``candidates``."""
    S3, chosen = shifts ** 3, []
    for rank, (flat, sc) in enumerate(zip(order, scores)):
        if len(chosen) == candidates or np.isnan(sc):
            break
        r, k = divmod(int(flat), S3)
        a = np.array([k // (shifts * shifts), (k // shifts) % shifts, k % shifts])
        if any(np.abs(a - c[3]).max() <= 1 and _rotation_angle(rotations[c[2]], rotations[r]) <= 1.5 * angle_step for c in chosen):
            continue
        chosen.append((rank, int(flat), r, a, float(sc)))
    return chosen


def global_align(source, verts, faces, angle_step=15.0, candidates=8, refine_iterations=20, samples=1024, shifts=1, shift_step=None,
                 field=None, resolution=32, metric='plane', scale=False, trim=1.0, max_dist=None, search='tree', cap=None, grid=None):
    """Pose-free alignment of ``source`` (points [N,3], or a ``(verts, faces)`` pair) to the mesh ``(verts, faces)``: a search over
    candidate poses scored against the target's distance field, then ``align_mesh`` from the best few.

    1. points: the finite rows of the source, and if there are more than ``samples`` of them, ``x[floor(i N / samples)]``;
    2. ``s`` = 1, or with ``scale`` the rms radius of the target's vertices over that of these points (``init='centroid'``);
    3. ``pose_scores`` of these points for ``pose_candidates(angle_step)`` and the ``shifts^3`` offsets (``field``: a ``PoseField`` of
       the target, built here with ``resolution`` if None), ordered by (score, flat index), NaN last;
    4. the first 4 096 of that order are walked greedily (``_pose_select``) until ``candidates`` are chosen;
    5. each is refined by ``align_mesh`` on the points of step 1 from ``M = [s R | c_tgt + o - s R c_src]`` with ``refine_iterations``
       and the call's ``metric / scale / trim / max_dist / search``; a start from which ICP fails counts as rms +inf;
    6. the winner has the lowest final rms, the earlier rank among equals.

    Returns the winner's ``align_mesh`` dict plus ``'candidates'`` (per refined candidate ``{'matrix'`` (its start), ``'score', 'index',
    'rms', 'converged'}``), ``'searched'`` (R shifts^3), ``'rank'`` (the winner's place among the refined) and ``'field'``.  A
    symmetric target has many equal optima; ``shifts > 1`` is an expert option (it did not help a partial source in the trial of
    DESIGN.md 4.30).  Device tensors score on ia_pose_scores, order with ``torch.sort`` and read the head of the order once; CPU tensors
    and NumPy arrays take the NumPy restatement.  Selection and refinement are the same host code for both."""
    _closest_search(search)
    if isinstance(source, (tuple, list)) and len(source) == 2 and getattr(source[0], 'ndim', 0) == 2:
        source = source[0]
    _mesh_args(verts, faces)
    if source.ndim != 2 or source.shape[1] != 3:
        raise ValueError(f'source must be points [N,3] or a (verts, faces) pair, got {tuple(source.shape)}')
    if not faces.shape[0] or not verts.shape[0]:
        raise ValueError('global_align: the target mesh is empty')
    candidates, samples, shifts = int(candidates), int(samples), _pose_offsets(shifts)
    if candidates < 1:
        raise ValueError(f'candidates must be >= 1, got {candidates}')
    if not 1 <= samples <= POSE_MAX_POINTS:
        raise ValueError(f'samples must be in [1, {POSE_MAX_POINTS}], got {samples}')
    on_dev = _is_device(verts)
    if field is None:
        field = PoseField(verts, faces, resolution)
    elif not isinstance(field, PoseField):
        raise ValueError(f'field must be a PoseField, got {type(field).__name__}')
    if (field.n_verts, field.n_faces) != (int(verts.shape[0]), int(faces.shape[0])) or (field.device is not None) != on_dev:
        raise ValueError(f'field was made for a mesh of {field.n_verts} vertices and {field.n_faces} faces '
                         f'{"on the device" if field.device is not None else "on the host"}: not this target')
    x = np.asarray(_np(source), dtype=F32).reshape(-1, 3)
    x = x[np.isfinite(x).all(1)]
    if not x.shape[0]:
        raise ValueError('global_align: the source has no finite point')
    if x.shape[0] > samples:
        x = x[(np.arange(samples, dtype=np.int64) * x.shape[0]) // samples]
    x = np.ascontiguousarray(x)
    c_src = x.astype(np.float64).mean(0)
    s = 1.0
    if scale:
        ra = float(np.sqrt(((x.astype(np.float64) - c_src) ** 2).sum(1).mean()))
        if not (ra > 0 and field.radius > 0):
            raise ValueError('global_align with scale needs point sets with an extent')
        s = field.radius / ra
    rotations = pose_candidates(angle_step)
    step = field.spacing if shift_step is None else float(shift_step)
    scores = pose_scores(x, field, rotations, shifts, step, s, cap)
    if on_dev:
        flat = scores.reshape(-1)
        ordered = torch.sort(flat, stable=True)                                              # NaN last, equal scores by flat index
        head = torch.stack([ordered.values[:_POSE_HEAD], ordered.indices[:_POSE_HEAD].double()]).cpu().numpy()      # the one host read
        order, ranked = head[1].astype(np.int64), head[0]
    else:
        flat = scores.reshape(-1)
        order = np.argsort(flat, kind='stable')[:_POSE_HEAD]                                  # NaN last, equal scores by flat index
        ranked = flat[order]
    chosen = _pose_select(order, ranked, rotations, shifts, float(angle_step), candidates)
    if not chosen:
        raise ValueError('global_align: no candidate pose has a score (is the source finite?)')
    if on_dev and grid is None:
        grid = TriangleGrid(verts, faces, build=search != 'tree')
    src = torch.from_numpy(x).to(verts.device) if on_dev else x
    half, best, tried = (shifts - 1) // 2, None, []
    for _, flat_index, r, a, sc in chosen:
        M = np.eye(4)
        M[:3, :3] = s * rotations[r]
        M[:3, 3] = field.centroid + (a - half) * step - M[:3, :3] @ c_src
        try:
            fit = align_mesh(src, verts, faces, metric=metric, scale=scale, iterations=refine_iterations, max_dist=max_dist, trim=trim, init=M,
                             grid=grid, search=search)
        except ValueError:
            fit = None
        tried.append({'matrix': M, 'score': sc, 'index': flat_index, 'rms': fit['rms'] if fit else float('inf'),
                      'converged': bool(fit and fit['converged'])})
        if fit is not None and (best is None or fit['rms'] < best[1]['rms']):
            best = (len(tried) - 1, fit)
    if best is None:
        raise ValueError('global_align: ICP failed from every chosen candidate (too few pairs count: see max_dist and trim)')
    return {**best[1], 'candidates': tried, 'searched': int(rotations.shape[0]) * shifts ** 3, 'rank': best[0], 'field': field}


# ------------------------------------------------------------------ winding number, signed distance, mesh -> volume

WINDING_CHUNK = 2048         # faces per partial sum (csrc/winding.hip kChunk = hipops.WINDING_CHUNK): part of the results
_SIGN_MODES = ('auto', 'regions', 'winding')


def _solid_angle(p, A, B, C, dtype):
    """The per-pair function (csrc/winding.hip solid_angle) in ``dtype`` on broadcastable [..., 3] arrays: the signed solid angle of
    triangle A B C seen from p, ``2 atan2(a . ((b - a) x (c - a)), (((|a| |b|) |c| + (a . b) |c|) + (b . c) |a|) + (c . a) |b|)`` in
    coordinates relative to p; every operation rounded on its own, dot products ``(x + y) + z``."""
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        a, b, c = np.broadcast_arrays(A - p, B - p, C - p)
        num = _dot3(a, _cross3(b - a, c - a))
        la, lb, lc = np.sqrt(_dot3(a, a)), np.sqrt(_dot3(b, b)), np.sqrt(_dot3(c, c))
        den = (((la * lb) * lc + _dot3(a, b) * lc) + _dot3(b, c) * la) + _dot3(c, a) * lb
        return (dtype(2) * np.arctan2(num, den)).astype(dtype)


def _winding_numpy(points, verts, faces, dtype=np.float64, pairs=1 << 20):
    """NumPy restatement of ia_winding_number with the per-pair function in ``dtype``: ``(w float64 [N], A float64 [N])`` with
    ``w = sum omega / 4 pi`` and ``A = sum |omega| / 4 pi`` (the size of the terms, for tolerances).  The sum has the kernel's
    association: chunks of ``WINDING_CHUNK`` faces of the face list as given, a chunk added in double in face order (``cumsum``), the
    chunk sums added in chunk order.  A face with an index out of range or a non-finite vertex is left out (it adds nothing); a
    non-finite point gives NaN; ``pairs`` point-triangle pairs are evaluated at a time."""
    p = np.asarray(points, dtype=F32).reshape(-1, 3).astype(dtype)
    v = np.asarray(verts, dtype=F32).reshape(-1, 3).astype(dtype)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = p.shape[0]
    in_range = ((f >= 0) & (f < v.shape[0])).all(1)
    tri = v[np.where(in_range[:, None], f, 0)] if v.shape[0] else np.zeros((f.shape[0], 3, 3), dtype=dtype)
    usable = in_range & np.isfinite(tri).all((1, 2))
    total, size = np.zeros(n), np.zeros(n)
    ok = np.isfinite(p).all(1)
    rows = np.flatnonzero(ok)
    for c0 in range(0, f.shape[0], WINDING_CHUNK):
        t = tri[c0:c0 + WINDING_CHUNK][usable[c0:c0 + WINDING_CHUNK]]
        if not t.shape[0]:
            continue
        step = max(1, pairs // t.shape[0])
        for s in range(0, rows.size, step):
            r = rows[s:s + step]
            om = _solid_angle(p[r, None, :], t[None, :, 0], t[None, :, 1], t[None, :, 2], dtype).astype(np.float64)
            total[r] += np.cumsum(om, axis=1)[:, -1]                               # cumsum adds in face order
            size[r] += np.cumsum(np.abs(om), axis=1)[:, -1]
    w, big = total / (4.0 * np.pi), size / (4.0 * np.pi)
    w[~ok] = np.nan
    big[~ok] = np.nan
    return w, big


def _is_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _winding_device(points, verts, faces, grid):
    from . import hipops
    if grid is not None:
        tris, dev = grid.tris, grid.verts.device
    else:
        dev = verts.device
        tris = hipops.tri_pack(verts.detach().float().contiguous(), faces.to(device=dev, dtype=torch.int32).contiguous())
    pts = torch.as_tensor(points).detach().to(dev).float().reshape(-1, 3).contiguous()
    return hipops.winding_number(pts, tris)


# ---- the cluster tree with a far-field expansion (csrc/winding_tree.hip)

WINDING_LEAF = 32            # faces per leaf (csrc/winding_tree.hip kLeaf = hipops.WINDING_LEAF): part of the results
WINDING_BRANCH = 8           # children per upper node (kBranch): part of the results
_WINDING_NO_KEY = 1 << 30
_WINDING_METHODS = ('exact', 'tree')


def _winding_beta(beta):
    """``beta`` as the fp32 the traversal compares with: finite and greater than 1, or inf (never far)."""
    try:
        b = F32(beta)
    except (TypeError, ValueError):
        raise ValueError(f'beta must be a number greater than 1 or inf, got {beta!r}') from None
    if not b > 1:
        raise ValueError(f'beta must be greater than 1 (as float32) or inf, got {beta!r}')
    return b


def _winding_method(method, name='method'):
    if method not in _WINDING_METHODS:
        raise ValueError(f'{name} must be one of {_WINDING_METHODS}, got {method!r}')
    return method


def _winding_levels(n_usable):
    """Nodes per level, leaves first: ceil(n / LEAF), then ceil(previous / BRANCH) down to one root; [] without a usable face."""
    counts = []
    if n_usable > 0:
        c = -(-int(n_usable) // WINDING_LEAF)
        while True:
            counts.append(c)
            if c == 1:
                break
            c = -(-c // WINDING_BRANCH)
    return counts


def _morton_cube(lo, hi):
    """(lo float32 [3], scale float32) of the key cube: ``scale = fp32(1024) / (longest side of the box, fp32)``, 0 without extent."""
    lo32, hi32 = np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)
    side = (hi32 - lo32).max()
    with np.errstate(over='ignore'):
        scale = F32(1024) / side if side > 0 else F32(0)
    return lo32, (scale if np.isfinite(scale) else F32(0))


def _spread10(x):
    x = x.astype(np.uint32)
    x = (x | (x << 16)) & 0x030000FF
    x = (x | (x << 8)) & 0x0300F00F
    x = (x | (x << 4)) & 0x030C30C3
    x = (x | (x << 2)) & 0x09249249
    return x


def _morton_keys_numpy(xyz, lo, scale):
    """30-bit Morton keys of float32 rows [n,3]: per axis ``clamp(floor((x - lo) * scale), 0, 1023)`` in fp32 (a NaN lands in cell 0),
    x the lowest bit of a triple."""
    with np.errstate(invalid='ignore', over='ignore'):
        cell = np.fmin(np.fmax(np.floor((np.asarray(xyz, dtype=F32) - lo) * scale), F32(0)), F32(1023)).astype(np.int64)
    return (_spread10(cell[:, 0]) | (_spread10(cell[:, 1]) << 1) | (_spread10(cell[:, 2]) << 2)).astype(np.int64)


def _winding_tree_numpy(verts, faces):
    """NumPy restatement of the tree build (ia_winding_tree_face_keys + the stable sort + ia_winding_tree_nodes): ``{'order' int64
    [F], 'tris' float32 [F_usable,3,3] in sorted order, 'nodes64' float64 [n,20], 'counts', 'usable', 'lo', 'scale'}``.  The rows are
    (c, r, D, A, Q row-major, 0 0 0) in float64; the table the queries read is their rounding to float32."""
    v32 = np.asarray(verts, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    in_range = ((f >= 0) & (f < v32.shape[0])).all(1)
    tri = v32[np.where(in_range[:, None], f, 0)] if v32.shape[0] else np.zeros((f.shape[0], 3, 3), dtype=F32)
    usable = in_range & np.isfinite(tri).all((1, 2))
    fin = v32[np.isfinite(v32).all(1)]
    lo, scale = _morton_cube(fin.min(0), fin.max(0)) if fin.shape[0] else (np.zeros(3, dtype=F32), F32(0))
    with np.errstate(invalid='ignore', over='ignore'):
        cen = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) * (F32(1) / F32(3))
    keys = np.where(usable, _morton_keys_numpy(cen, lo, scale), _WINDING_NO_KEY)
    order = np.argsort(keys, kind='stable')
    fu = int(usable.sum())
    t32 = tri[order[:fu]]
    t = t32.astype(np.float64)
    counts = _winding_levels(fu)
    rows = np.zeros((sum(counts), 20))
    A, B, C = t[:, 0], t[:, 1], t[:, 2]
    an = _cross3(B - A, C - A) * 0.5
    area = np.sqrt(_dot3(an, an))
    ct = ((A + B) + C) * (1.0 / 3.0)

    def seq(x):                                                                            # a sum in index order
        return np.cumsum(x, axis=0)[-1]
    for i in range(counts[0] if counts else 0):
        sl = slice(i * WINDING_LEAF, min((i + 1) * WINDING_LEAF, fu))
        a = seq(area[sl])
        c = seq(ct[sl] * area[sl, None]) * (1.0 / a) if a > 0 else seq(ct[sl]) * (1.0 / (sl.stop - sl.start))
        u = ct[sl] - c
        rel = t[sl] - c
        rows[i, :3], rows[i, 3], rows[i, 4:7], rows[i, 7] = c, np.sqrt(_dot3(rel, rel).max()), seq(an[sl]), a
        rows[i, 8:17] = seq(u[:, :, None] * an[sl][:, None, :]).reshape(9)
    start, span = 0, WINDING_LEAF
    for lvl in range(1, len(counts)):
        child0, start = start, start + counts[lvl - 1]
        for j in range(counts[lvl]):
            ks = np.arange(j * WINDING_BRANCH, min((j + 1) * WINDING_BRANCH, counts[lvl - 1]))
            ch = rows[child0 + ks]
            nk = (np.minimum((ks + 1) * span, fu) - ks * span).astype(np.float64)
            a = seq(ch[:, 7])
            c = seq(ch[:, :3] * ch[:, 7:8]) * (1.0 / a) if a > 0 else seq(ch[:, :3] * nk[:, None]) * (1.0 / seq(nk))
            u = ch[:, :3] - c
            row = rows[start + j]
            row[:3], row[3], row[4:7], row[7] = c, (np.sqrt(_dot3(u, u)) + ch[:, 3]).max(), seq(ch[:, 4:7]), a
            q = np.zeros(9)
            for k in range(ks.size):                                                       # (Q_k first, then the shift, child by child)
                q = (q + ch[k, 8:17]) + (u[k][:, None] * ch[k, 4:7][None, :]).reshape(9)
            row[8:17] = q
        span *= WINDING_BRANCH
    return {'order': order, 'tris': t32, 'nodes64': rows, 'counts': counts, 'usable': fu, 'lo': lo, 'scale': scale}


def _tree_walk(counts, idx, visit):
    """The walk of csrc/cluster_tree.h over the level layout ``counts``, depth first, children in index order: ``visit(level, j, row,
    idx)`` does the work of the points ``idx`` at that node (table row ``row``) and returns those that go below; none prunes the subtree."""
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    stack = [(len(counts) - 1, 0, idx)] if counts and idx.size else []
    while stack:
        lvl, j, idx = stack.pop()
        below = visit(lvl, j, starts[lvl] + j, idx)
        if lvl > 0 and below.size:
            stack.extend((lvl - 1, k, below) for k in range(min((j + 1) * WINDING_BRANCH, counts[lvl - 1]) - 1, j * WINDING_BRANCH - 1, -1))


def _winding_tree_query_numpy(points, tris, nodes, counts, beta, dtype=np.float64, use_q=True):
    """NumPy restatement of ia_winding_tree_query on a float32 node table ``nodes`` [n,20] and the sorted usable triangles ``tris``
    [F_usable,3,3]: ``(w, bound, size, far, pairs)`` per point, with the terms evaluated in ``dtype``, ``size = sum |term| / 4 pi``,
    ``far`` the number of far terms and ``pairs`` the exact pairs.  The far / near decisions are always the kernel's fp32 ones; the
    running sum is double in visiting order (depth first, children in index order).  ``use_q=False`` drops the Q terms (tests)."""
    p32 = np.asarray(points, dtype=F32).reshape(-1, 3)
    nodes = np.asarray(nodes, dtype=F32).reshape(-1, 20)
    t = np.asarray(tris, dtype=F32).reshape(-1, 3, 3).astype(dtype)
    n, fu, b32 = p32.shape[0], t.shape[0], _winding_beta(beta)
    p = p32.astype(dtype)
    total, bound, size = np.zeros(n), np.zeros(n), np.zeros(n)
    far_n, pair_n = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    ok = np.isfinite(p32).all(1)

    def visit(lvl, j, at, idx):
        row = nodes[at]
        x32 = row[:3] - p32[idx]
        d2 = (x32[:, 0] * x32[:, 0] + x32[:, 1] * x32[:, 1]) + x32[:, 2] * x32[:, 2]
        br = b32 * row[3]
        far = d2 > br * br
        if far.any():
            r = idx[far]
            x = (row[:3].astype(dtype) - p[r]).astype(dtype)
            dd = _dot3(x, x)
            D, Q = row[4:7].astype(dtype), row[8:17].astype(dtype).reshape(3, 3)
            if not use_q:
                Q = Q * dtype(0)
            qx = np.stack([_dot3(Q[0], x), _dot3(Q[1], x), _dot3(Q[2], x)], -1)
            tr = (Q[0, 0] + Q[1, 1]) + Q[2, 2]
            term = (((_dot3(D, x) + tr) - dtype(3) * _dot3(x, qx) / dd) / (dd * np.sqrt(dd))).astype(np.float64)
            total[r] += term
            size[r] += np.abs(term)
            e = np.sqrt(d2[far].astype(np.float64)) - np.float64(row[3])
            bound[r] += 3.0 * np.float64(row[7]) * (np.float64(row[3]) * np.float64(row[3])) / (4.0 * np.pi * ((e * e) * (e * e)))
            far_n[r] += 1
        r = idx[~far]
        if lvl == 0 and r.size:
            sl = slice(j * WINDING_LEAF, min((j + 1) * WINDING_LEAF, fu))
            om = _solid_angle(p[r, None, :], t[None, sl, 0], t[None, sl, 1], t[None, sl, 2], dtype).astype(np.float64)
            total[r] = np.cumsum(np.concatenate([total[r, None], om], 1), axis=1)[:, -1]           # one term at a time, in face order
            size[r] += np.abs(om).sum(1)
            pair_n[r] += sl.stop - sl.start
        return r

    with np.errstate(invalid='ignore', over='ignore', under='ignore', divide='ignore'):
        _tree_walk(counts, np.flatnonzero(ok), visit)
    w, big = total / (4.0 * np.pi), size / (4.0 * np.pi)
    w[~ok] = np.nan
    big[~ok] = np.nan
    bound[~ok] = np.nan
    return w, bound, big, far_n, pair_n


# ---- closest point on the same tree (csrc/closest_tree.hip)

_SEARCHES = ('grid', 'tree')
_TREE_SLACK = 2.0 ** -17     # 64 eps32: the margin of the grid search, relative to max(|p|_inf, mesh extent)


def _closest_search(search):
    if search not in _SEARCHES:
        raise ValueError(f'search must be one of {_SEARCHES}, got {search!r}')
    return search


def _tree_boxes_numpy(tris, counts):
    """NumPy restatement of ia_tree_boxes: float32 [n,8] = (lo.xyz, 0, hi.xyz, 0) per node of the level layout ``counts`` over the
    sorted usable triangles ``tris`` float32 [F_usable,3,3].  Min and max are exact: the table equals the kernel's bit for bit."""
    t = np.asarray(tris, dtype=F32).reshape(-1, 9)
    fu = t.shape[0]
    out = np.zeros((sum(counts), 8), dtype=F32)
    start = 0
    for lvl, cnt in enumerate(counts):
        for i in range(cnt):
            if lvl == 0:
                v = t[i * WINDING_LEAF:min((i + 1) * WINDING_LEAF, fu)].reshape(-1, 3)
                lo, hi = v.min(0), v.max(0)
            else:
                ch = out[child0 + i * WINDING_BRANCH:child0 + min((i + 1) * WINDING_BRANCH, counts[lvl - 1])]
                lo, hi = ch[:, 0:3].min(0), ch[:, 4:7].max(0)
            out[start + i, 0:3], out[start + i, 4:7] = lo, hi
        child0, start = start, start + cnt
    return out


def _box_dist(p, row):
    """Distance from points [n,3] to the box of one row (or of one row per point), every operation rounded on its own."""
    g = np.maximum(np.maximum(row[..., 0:3] - p, p - row[..., 4:7]), p.dtype.type(0))
    return np.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2])


def _closest_tree_numpy(points, tree, dtype=np.float64, slack=None):
    """NumPy restatement of ia_closest_point_tree in ``dtype`` on a host ``WindingTree``: ``(dist [N], face int32 [N] (input face
    indices), point [N,3], counts int64 [N,2] = boxes tested, point-triangle pairs evaluated)``.  ``best = (dist, face)`` is ordered
    lexicographically and starts at ``(+inf, -1)``; a visited leaf evaluates ``point_triangle`` for its faces and keeps the smaller
    pair.  A node is skipped iff ``lb`` is finite and ``lb - slack > best.dist``: ``lb`` the distance from the point to the node's box
    (``g = max(max(lo - p, p - hi), 0)``, ``sqrt((gx^2 + gy^2) + gz^2)``), ``slack = 2^-17 max(|p|_inf, tree.extent)``.  Each point
    first descends from the root to the child with the smallest ``lb`` (the lowest index among equals) and evaluates that leaf, then
    walks depth first with the children in index order, passing over that leaf: the kernel's order, so ``counts`` are the kernel's.
    The result equals ``_closest_numpy`` in the same ``dtype`` exactly: the tree only prunes.  ``slack`` (tests): one value for every
    point instead."""
    if tree.device is not None:
        raise ValueError('_closest_tree_numpy restates the query on a host WindingTree')
    p32 = np.asarray(points, dtype=F32).reshape(-1, 3)
    p = p32.astype(dtype)
    t = np.asarray(tree.tris, dtype=F32).reshape(-1, 3, 3).astype(dtype)
    order = np.asarray(tree.order, dtype=np.int64)
    counts, boxes = list(tree.counts), np.asarray(tree.boxes, dtype=F32).astype(dtype)
    n, fu = p.shape[0], t.shape[0]
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ok = np.isfinite(p32).all(1)
    best_d, best_f, best_at = np.full(n, np.inf, dtype=dtype), np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    n_box, n_pair = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        if slack is None:
            margin = dtype(_TREE_SLACK) * np.maximum(np.abs(p).max(1) if n else np.zeros(0, dtype=dtype), dtype(tree.extent))
        else:
            margin = np.full(n, slack, dtype=dtype)

        def leaf(j, r):
            sl = slice(j * WINDING_LEAF, min((j + 1) * WINDING_LEAF, fu))
            d, _ = point_triangle(p[r, None, :], t[None, sl, 0], t[None, sl, 1], t[None, sl, 2], dtype)
            d = np.where(np.isnan(d), np.inf, d)
            faces = order[sl]
            dm = d.min(1)
            tie = d == dm[:, None]
            fm = np.where(tie, faces[None, :], np.iinfo(np.int64).max).min(1)                # the lowest input index among equals
            at = sl.start + np.argmax(tie & (faces[None, :] == fm[:, None]), axis=1)
            take = (dm < best_d[r]) | ((dm == best_d[r]) & (fm < best_f[r]))
            rr = r[take]
            best_d[rr], best_f[rr], best_at[rr] = dm[take], fm[take], at[take]
            n_pair[r] += sl.stop - sl.start

        rows = np.flatnonzero(ok) if counts else np.zeros(0, dtype=np.int64)
        seed = np.full(n, -1, dtype=np.int64)
        if rows.size:
            j = np.zeros(rows.size, dtype=np.int64)
            for lvl in range(len(counts) - 1, 0, -1):
                least, pick = np.full(rows.size, np.inf, dtype=dtype), j * WINDING_BRANCH
                for c in range(WINDING_BRANCH):
                    k = j * WINDING_BRANCH + c
                    valid = k < counts[lvl - 1]
                    lb = _box_dist(p[rows], boxes[starts[lvl - 1] + np.minimum(k, counts[lvl - 1] - 1)])
                    less = valid & (lb < least)
                    least, pick = np.where(less, lb, least), np.where(less, k, pick)
                    n_box[rows] += valid
                j = pick
            seed[rows] = j
            for leaf_j in np.unique(j):
                leaf(int(leaf_j), rows[j == leaf_j])

        def visit(lvl, j, at, idx):
            if lvl == 0:
                idx = idx[seed[idx] != j]
            lb = _box_dist(p[idx], boxes[at])
            n_box[idx] += 1
            r = idx[~(np.isfinite(lb) & (lb - margin[idx] > best_d[idx]))]
            if lvl == 0 and r.size:
                leaf(j, r)
            return r

        _tree_walk(counts, rows, visit)
        hit = best_f >= 0
        at = np.where(hit, best_at, 0)
        point = np.full((n, 3), np.nan, dtype=dtype)
        if fu and hit.any():
            _, q = point_triangle(p, t[at, 0], t[at, 1], t[at, 2], dtype)
            point = np.where(hit[:, None], p + q, np.nan).astype(dtype)
    best_d[~ok] = np.nan
    return best_d, best_f.astype(np.int32), point, np.stack([n_box, n_pair], -1)


# ---- point clouds on the same tree: k nearest points, normals (csrc/point_tree.hip)

NEAREST_MAX_K = 32
_NEAREST_LISTS = (1, 4, 8, 16, 32)     # the lists the kernels are instantiated for; k is rounded up, which changes no result
_NO_INDEX = np.iinfo(np.int32).max     # the index of an empty place of a list
_JACOBI_SWEEPS = 8


def _cloud_args(points, what='points'):
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f'{what} must be [n,3], got {tuple(points.shape)}')


def _nearest_k(k):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= NEAREST_MAX_K:
        raise ValueError(f'k must be an integer in 1 .. {NEAREST_MAX_K}, got {k!r}')
    return int(k)


def _pair_d2(p, x):
    """Squared distance of pairs (query p [..., 3], point x [..., 3]) in the arrays' dtype: pair_d2 of csrc/geom_common.h, three
    differences, three squares and two sums, each rounded on its own."""
    dx, dy, dz = x[..., 0] - p[..., 0], x[..., 1] - p[..., 1], x[..., 2] - p[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _box_d2(p, row):
    """box_d2 of csrc/geom_common.h: the expression of ``_pair_d2`` on the gaps ``max(lo - p, 0, p - hi)`` between points [n,3] and
    the box of one row [8] (or one row per point).  Rounding is monotone, so it never exceeds ``_pair_d2(p, x)`` for x in the box."""
    g = np.maximum(np.maximum(row[..., 0:3] - p, p.dtype.type(0)), p - row[..., 4:7])
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def _point_boxes_numpy(pts, counts):
    """NumPy restatement of ia_point_tree_boxes: float32 [n,8] = (lo.xyz, 0, hi.xyz, 0) per node over the sorted points [n_usable,3]."""
    out = np.zeros((sum(counts), 8), dtype=F32)
    start = child0 = 0
    for lvl, cnt in enumerate(counts):
        if lvl == 0:
            at = np.arange(0, pts.shape[0], WINDING_LEAF)
            lo, hi = np.minimum.reduceat(pts, at, axis=0), np.maximum.reduceat(pts, at, axis=0)
        else:
            ch = out[child0:child0 + counts[lvl - 1]]
            at = np.arange(0, counts[lvl - 1], WINDING_BRANCH)
            lo, hi = np.minimum.reduceat(ch[:, 0:3], at, axis=0), np.maximum.reduceat(ch[:, 4:7], at, axis=0)
        out[start:start + cnt, 0:3], out[start:start + cnt, 4:7] = lo, hi
        child0, start = start, start + cnt
    return out


def _point_tree_numpy(points):
    """NumPy restatement of the tree of a cloud, the definition of ``PointTree``: ``{'order' int64 [n] (sorted position -> input
    index: the usable = finite points by the 30-bit Morton key of their position in the cube of the usable points, ties by input
    index, then the others), 'points' float32 [n_usable,3] in that order, 'boxes' float32 [nodes,8], 'counts', 'usable', 'lo',
    'scale'}``.  ``WINDING_LEAF`` points per leaf, ``WINDING_BRANCH`` nodes per parent, leaves first."""
    p32 = np.asarray(points, dtype=F32).reshape(-1, 3)
    usable = np.isfinite(p32).all(1)
    fin = p32[usable]
    lo, scale = _morton_cube(fin.min(0), fin.max(0)) if fin.shape[0] else (np.zeros(3, dtype=F32), F32(0))
    keys = np.where(usable, _morton_keys_numpy(p32, lo, scale), _WINDING_NO_KEY)
    order = np.argsort(keys, kind='stable')
    nu = int(usable.sum())
    pts = p32[order[:nu]]
    counts = _winding_levels(nu)
    return {'order': order, 'points': pts, 'boxes': _point_boxes_numpy(pts, counts), 'counts': counts, 'usable': nu, 'lo': lo, 'scale': scale}


def _smallest_pairs(d2, kk):
    """Per row of d2 [r,n] the ``kk`` smallest pairs (value, column), ascending: (values [r,kk], columns int64 [r,kk]), +inf / -1
    where the row has fewer columns."""
    r, n = d2.shape
    vals, cols = np.full((r, kk), np.inf, dtype=d2.dtype), np.full((r, kk), -1, dtype=np.int64)
    if r == 0 or n == 0:
        return vals, cols
    m = min(kk, n)
    kth = np.partition(d2, m - 1, axis=1)[:, m - 1]
    rows, at = np.nonzero(d2 <= kth[:, None])                                              # (every tie of the m-th value is in)
    v = d2[rows, at]
    o = np.lexsort((at, v, rows))
    rows, at, v = rows[o], at[o], v[o]
    rank = np.arange(rows.size) - np.searchsorted(rows, np.arange(r))[rows]
    keep = rank < kk
    vals[rows[keep], rank[keep]], cols[rows[keep], rank[keep]] = v[keep], at[keep]
    return vals, cols


def _nearest_finish(d2, ids, ok, max_dist, dtype):
    """(dist, index int32) of the lists (d2, input index or -1): ``sqrt``, the ``max_dist`` rule and the non-finite queries."""
    with np.errstate(invalid='ignore'):
        dist = np.sqrt(d2).astype(dtype)
    admitted = (ids >= 0) & ok[:, None]
    if max_dist is not None:
        admitted &= dist <= dtype(max_dist)
    return np.where(admitted, dist, dtype(np.inf)), np.where(admitted, ids, -1).astype(np.int32)


def _exclude_rows(exclude, exclude_self, n):
    if exclude is not None:
        return np.asarray(exclude, dtype=np.int64).reshape(n)
    return np.arange(n, dtype=np.int64) if exclude_self else None


def _nearest_numpy(queries, points, k=1, max_dist=None, exclude_self=False, dtype=np.float64, exclude=None, pairs=1 << 22):
    """The definition of ``nearest_points``, over all pairs: ``(dist [N,k] in dtype, index int32 [N,k])``.  For query p and usable
    (finite) point x, ``d2 = (dx dx + dy dy) + dz dz`` in ``dtype`` with every operation rounded on its own; the result is the k
    smallest pairs ``(d2, input index)``, ascending, ``dist = sqrt(d2)``; a place is ``inf`` / ``-1`` where the cloud has no further
    point or ``dist > max_dist``, and throughout for a non-finite query.  ``exclude_self`` leaves out the point whose input index is
    the query's row (``exclude``: one input index per query instead)."""
    k = _nearest_k(k)
    q32, p32 = np.asarray(queries, dtype=F32).reshape(-1, 3), np.asarray(points, dtype=F32).reshape(-1, 3)
    idx = np.flatnonzero(np.isfinite(p32).all(1))
    x, q = p32[idx].astype(dtype), q32.astype(dtype)
    n = q.shape[0]
    ok = np.isfinite(q32).all(1)
    excl = _exclude_rows(exclude, exclude_self, n)
    kk = k if excl is None else k + 1
    d2, ids = np.full((n, k), np.inf, dtype=dtype), np.full((n, k), -1, dtype=np.int64)
    step = max(int(pairs) // max(idx.size, 1), 1)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        for c0 in range(0, n, step):
            sl = slice(c0, min(c0 + step, n))
            v, at = _smallest_pairs(np.where(ok[sl, None], _pair_d2(q[sl, None, :], x[None, :, :]), dtype(np.inf)), kk)
            i = np.where(at >= 0, idx[np.maximum(at, 0)] if idx.size else -1, -1)
            if excl is not None:                                                           # the pair left out goes last, the others keep their order
                o = np.argsort(i == excl[sl, None], axis=1, kind='stable')
                v, i = np.take_along_axis(v, o, 1), np.take_along_axis(i, o, 1)
            d2[sl], ids[sl] = v[:, :k], i[:, :k]
    if excl is not None:
        ids = np.where(ids == excl[:, None], -1, ids)
    return _nearest_finish(d2, ids, ok, max_dist, dtype)


def _nearest_tree_numpy(queries, tree, k=1, max_dist=None, exclude_self=False, dtype=np.float64, exclude=None, return_counts=False):
    """NumPy restatement of ia_nearest_points_tree in ``dtype`` on a host ``PointTree``: what ``_nearest_numpy`` gives, exactly, by
    the walk of ``_closest_tree_numpy``.  Each query keeps a sorted list of K pairs ``(d2, input index)`` (K: k rounded up to one of
    1, 4, 8, 16, 32) that starts at ``(inf, none)``; a leaf merges its points into it.  A node is skipped iff ``lb > (the K-th d2)``,
    strictly, ``lb = _box_d2``; the query first descends to the child with the smallest ``lb`` (the lowest index among equals), takes
    that leaf and passes over it in the walk.  With ``return_counts`` also int64 [N,2] (boxes tested, leaves taken)."""
    if tree.device is not None:
        raise ValueError('_nearest_tree_numpy restates the query on a host PointTree')
    k = _nearest_k(k)
    K = next(c for c in _NEAREST_LISTS if c >= k)
    q32 = np.asarray(queries, dtype=F32).reshape(-1, 3)
    q, x = q32.astype(dtype), np.asarray(tree.sorted, dtype=F32).astype(dtype)
    order = np.asarray(tree.order, dtype=np.int64)
    counts, boxes = list(tree.counts), np.asarray(tree.boxes, dtype=F32).astype(dtype)
    n, nu = q.shape[0], x.shape[0]
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ok = np.isfinite(q32).all(1)
    excl = _exclude_rows(exclude, exclude_self, n)
    best_d, best_i = np.full((n, K), np.inf, dtype=dtype), np.full((n, K), _NO_INDEX, dtype=np.int64)
    n_box, n_leaf = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        def leaf(j, r):
            sl = slice(j * WINDING_LEAF, min((j + 1) * WINDING_LEAF, nu))
            d2 = _pair_d2(q[r, None, :], x[None, sl, :])
            ids = np.broadcast_to(order[sl], d2.shape)
            if excl is not None:
                drop = ids == excl[r, None]
                d2, ids = np.where(drop, dtype(np.inf), d2), np.where(drop, _NO_INDEX, ids)
            cd, ci = np.concatenate([best_d[r], d2], 1), np.concatenate([best_i[r], ids], 1)
            o = np.lexsort((ci, cd), axis=1)[:, :K]
            best_d[r], best_i[r] = np.take_along_axis(cd, o, 1), np.take_along_axis(ci, o, 1)
            n_leaf[r] += 1

        rows = np.flatnonzero(ok) if counts else np.zeros(0, dtype=np.int64)
        seed = np.full(n, -1, dtype=np.int64)
        if rows.size:
            j = np.zeros(rows.size, dtype=np.int64)
            for lvl in range(len(counts) - 1, 0, -1):
                least, pick = np.full(rows.size, np.inf, dtype=dtype), j * WINDING_BRANCH
                for c in range(WINDING_BRANCH):
                    at = j * WINDING_BRANCH + c
                    valid = at < counts[lvl - 1]
                    lb = _box_d2(q[rows], boxes[starts[lvl - 1] + np.minimum(at, counts[lvl - 1] - 1)])
                    less = valid & (lb < least)
                    least, pick = np.where(less, lb, least), np.where(less, at, pick)
                    n_box[rows] += valid
                j = pick
            seed[rows] = j
            for leaf_j in np.unique(j):
                leaf(int(leaf_j), rows[j == leaf_j])

        def visit(lvl, j, at, idx):
            if lvl == 0:
                idx = idx[seed[idx] != j]
            lb = _box_d2(q[idx], boxes[at])
            n_box[idx] += 1
            r = idx[~(lb > best_d[idx, K - 1])]
            if lvl == 0 and r.size:
                leaf(j, r)
            return r

        _tree_walk(counts, rows, visit)
    out = _nearest_finish(best_d[:, :k], np.where(best_i[:, :k] == _NO_INDEX, -1, best_i[:, :k]), ok, max_dist, dtype)
    return out + (np.stack([n_box, n_leaf], -1),) if return_counts else out


class PointTree:
    """The cluster tree of one point cloud for ``nearest_points``, built once: the usable (finite) points sorted by the 30-bit Morton
    key of their position in the cloud's cube (the arithmetic of the face keys of ``WindingTree``; ties by input index),
    ``WINDING_LEAF`` points per leaf, ``WINDING_BRANCH`` nodes per parent, one exact bounding box per node; no pointers.  ``order``
    (sorted position -> input index), ``sorted`` (the usable points in that order: float32 [n_usable,4] = xyz and the bits of the
    input index on the device, [n_usable,3] on the host), ``boxes``, ``counts``, ``info``.  Device tensors build on the kernels; CPU
    tensors and NumPy arrays take ``_point_tree_numpy``, which is the definition."""

    def __init__(self, points):
        _cloud_args(points)
        self.device = points.device if _is_device(points) else None
        self._like = points
        n = int(points.shape[0])
        if n > (1 << 25):
            raise ValueError(f'a cloud holds at most 2^25 points, got {n}')
        if self.device is not None:
            from . import hipops
            self.points = points.detach().float().contiguous()
            fin = self.points[torch.isfinite(self.points).all(1)]
            box = torch.stack([fin.amin(0), fin.amax(0)]).cpu().tolist() if fin.shape[0] else [[0.0] * 3, [0.0] * 3]   # one host synchronisation
            lo, scale = _morton_cube(box[0], box[1]) if fin.shape[0] else (np.zeros(3, dtype=F32), F32(0))
            self.order, self.sorted, self.boxes, self.counts, self.usable = hipops.point_tree_build(self.points, lo.tolist(), float(scale))
        else:
            self.points = np.asarray(_np(points), dtype=F32).reshape(-1, 3)
            t = _point_tree_numpy(self.points)
            fin = _finite_rows(self.points)
            box = [fin.min(0).tolist(), fin.max(0).tolist()] if fin.shape[0] else [[0.0] * 3, [0.0] * 3]
            lo, scale = t['lo'], t['scale']
            self.order, self.sorted, self.boxes, self.counts, self.usable = t['order'], t['points'], t['boxes'], t['counts'], t['usable']
        self.box_lo, self.box_hi = box
        self.extent = max(max(abs(v) for v in box[0]), max(abs(v) for v in box[1]))
        self.lo, self.scale = [float(v) for v in lo], float(scale)
        self.info = {'points': n, 'usable': int(self.usable), 'levels': len(self.counts), 'nodes': int(sum(self.counts)),
                     'leaf': WINDING_LEAF, 'branch': WINDING_BRANCH}

    def nearest(self, queries, k=1, max_dist=None, exclude_self=False, brute=False, return_counts=False, sort=True):
        """``{'dist' float32 [N,k], 'index' int32 [N,k]}`` of queries [N,3] (see ``nearest_points``); with ``return_counts`` also
        ``'counts'`` int [N,2] (boxes tested, leaves taken).  ``sort`` (device): query in Morton order of the queries and return in
        the caller's order; it changes no result.  A host tree answers in float64."""
        k = _nearest_k(k)
        _cloud_args(queries, 'queries')
        if max_dist is not None and not float(max_dist) >= 0:
            raise ValueError(f'max_dist must be >= 0, got {max_dist}')
        if brute and return_counts:
            raise ValueError('return_counts counts the walk: it excludes brute=True')
        if self.device is None:
            if brute:
                out = _nearest_numpy(_np(queries), self.points, k, max_dist, exclude_self)
            else:
                out = _nearest_tree_numpy(_np(queries), self, k, max_dist, exclude_self, return_counts=return_counts)
            res = {'dist': _as_out(out[0], queries), 'index': _as_out(out[1], queries, np.int32)}
            if return_counts:
                res['counts'] = _as_out(out[2], queries, np.int64)
            return res
        from . import hipops
        pts = torch.as_tensor(queries).detach().to(self.device).float().reshape(-1, 3).contiguous()
        n = pts.shape[0]
        excl = torch.arange(n, dtype=torch.int32, device=self.device) if exclude_self else None
        limit = float('inf') if max_dist is None else float(F32(max_dist))
        boxes = None if brute else self.boxes
        if sort and not brute and n > 64:
            perm = torch.argsort(hipops.winding_tree_point_keys(pts, self.lo, self.scale), stable=True)
            back = torch.empty_like(perm)
            back[perm] = torch.arange(n, device=perm.device)
            out = hipops.nearest_points(pts[perm].contiguous(), self.sorted, boxes, k, limit, None if excl is None else excl[perm].contiguous(),
                                        counts=return_counts)
            dist, index, cnt = [None if t is None else t[back] for t in out]
        else:
            dist, index, cnt = hipops.nearest_points(pts, self.sorted, boxes, k, limit, excl, counts=return_counts)
        res = {'dist': dist, 'index': index}
        if return_counts:
            res['counts'] = cnt
        return res


def _point_tree_for(points, tree):
    if tree is None:
        return PointTree(points)
    if not isinstance(tree, PointTree) or tree.info['points'] != points.shape[0] or (tree.device is not None) != _is_device(points):
        raise ValueError('tree must be the PointTree of these points, on their device')
    return tree


def nearest_points(queries, points, k=1, tree=None, max_dist=None, exclude_self=False, brute=False, return_counts=False):
    """The k nearest points of the cloud ``points`` [n,3] for every query [N,3]: ``{'dist' float32 [N,k], 'index' int32 [N,k]}``
    with input indices.  The usable points are the finite rows.  For query p and usable point x, in float32 with every operation
    rounded on its own, ``d2 = (dx dx + dy dy) + dz dz``; the result is the k smallest pairs ``(d2, input index)``, ascending (equal
    distances come out in index order), ``dist = sqrt(d2)`` correctly rounded.  A place is ``inf`` / ``-1`` where fewer than k points
    are admissible, and throughout for a non-finite query; ``max_dist`` admits ``dist <= max_dist``; ``exclude_self`` (for
    ``queries is points``) leaves out the point whose index is the query's row.  k is in 1 .. 32.

    Device tensors walk the ``PointTree`` of the cloud (``tree``; built here if None) with ia_nearest_points_tree, or, with
    ``brute=True``, take all pairs (ia_nearest_points_brute): the tree only prunes, so both give the same bits, which are those of the
    NumPy float32 restatement (``_nearest_numpy(dtype=np.float32)``), for any k, any slabbing of the queries and any run.  CPU tensors
    and NumPy arrays take ``_nearest_tree_numpy`` (``_nearest_numpy`` with ``brute``) in float64.  ``return_counts`` adds ``'counts'``
    int [N,2]: boxes tested and leaves taken per query."""
    _cloud_args(points)
    _cloud_args(queries, 'queries')
    _nearest_k(k)
    if _is_device(points) != _is_device(queries):
        raise ValueError('queries and points must both be device tensors or both be on the host')
    return _point_tree_for(points, tree).nearest(queries, k, max_dist, exclude_self, brute, return_counts)


def _jacobi_rotate(A, V, p, q, r):
    """One Jacobi rotation in the (p, q) plane of the symmetric matrices A [n,3,3] (r: the third axis), accumulated into the columns of
    V: the operations of jacobi_rotate in csrc/point_tree.hip, in place."""
    apq = A[:, p, q].copy()
    live = apq != 0.0
    theta = (A[:, q, q] - A[:, p, p]) / (2.0 * np.where(live, apq, 1.0))
    t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    t, c, s = np.where(live, t, 0.0), np.where(live, c, 1.0), np.where(live, s, 0.0)      # (apq = 0: the rotation is skipped)
    app, aqq = A[:, p, p] - t * apq, A[:, q, q] + t * apq
    arp, arq = c * A[:, r, p] - s * A[:, r, q], s * A[:, r, p] + c * A[:, r, q]
    A[:, p, p], A[:, q, q] = app, aqq
    A[:, p, q] = A[:, q, p] = 0.0
    A[:, r, p] = A[:, p, r] = arp
    A[:, r, q] = A[:, q, r] = arq
    vp, vq = c[:, None] * V[:, :, p] - s[:, None] * V[:, :, q], s[:, None] * V[:, :, p] + c[:, None] * V[:, :, q]
    V[:, :, p], V[:, :, q] = vp, vq


def _jacobi3_numpy(cov6):
    """Eigen-decomposition of symmetric 3x3 matrices float64 [n,6] (xx xy xz yy yz zz) by ``_JACOBI_SWEEPS`` cyclic Jacobi sweeps over
    (0,1) (0,2) (1,2): ``(eigenvalues [n,3] ascending, the lowest axis first among equals, eigenvectors [n,3,3] as columns)``."""
    c = np.asarray(cov6, dtype=np.float64).reshape(-1, 6)
    A = np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], 1)
    V = np.broadcast_to(np.eye(3), A.shape).copy()
    with np.errstate(over='ignore', invalid='ignore'):
        for _ in range(_JACOBI_SWEEPS):
            _jacobi_rotate(A, V, 0, 1, 2)
            _jacobi_rotate(A, V, 0, 2, 1)
            _jacobi_rotate(A, V, 1, 2, 0)
    w = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], -1)
    for a, b in ((0, 1), (1, 2), (0, 1)):                                                  # the kernel's network on three values
        swap = w[:, b] < w[:, a]
        w[swap, a], w[swap, b] = w[swap, b], w[swap, a]
        V[swap, :, a], V[swap, :, b] = V[swap, :, b], V[swap, :, a]
    return w, V


def _point_normals_numpy(points, index):
    """NumPy restatement of ia_point_normals: ``(normal float32 [n,3], variation float32 [n], eigenvalues float64 [n,3], covariance
    float64 [n,6])`` for points [n,3] and their neighbour table int [n,k] (entries outside [0, n) are left out).  In double: the mean
    of the neighbours added in order, the covariance (xx xy xz yy yz zz) of the differences added in order and divided by their
    number m, ``_jacobi3_numpy``.  The normal is the unit eigenvector of the smallest eigenvalue with its largest-magnitude component
    positive, ``variation = l0 / ((l0 + l1) + l2)``; both are 0 where m < 3 or the trace is not positive."""
    p = np.asarray(points, dtype=F32).reshape(-1, 3).astype(np.float64)
    idx = np.asarray(index, dtype=np.int64).reshape(p.shape[0], -1)
    n, k = idx.shape
    valid = (idx >= 0) & (idx < n)
    nb = p[np.where(valid, idx, 0)]                                                        # [n,k,3]
    m = valid.sum(1)
    total = np.zeros((n, 3))
    for s in range(k):
        total = np.where(valid[:, s, None], total + nb[:, s], total)
    cov = np.zeros((n, 6))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        mean = total / m[:, None]
        for s in range(k):
            e = nb[:, s] - mean
            term = np.stack([e[:, 0] * e[:, 0], e[:, 0] * e[:, 1], e[:, 0] * e[:, 2], e[:, 1] * e[:, 1], e[:, 1] * e[:, 2], e[:, 2] * e[:, 2]], -1)
            cov = np.where(valid[:, s, None], cov + term, cov)
        cov = np.where(m[:, None] > 0, cov / m[:, None], 0.0)
        w, V = _jacobi3_numpy(cov)
        trace = (w[:, 0] + w[:, 1]) + w[:, 2]
        good = (m >= 3) & (trace > 0.0)
        v0 = V[:, :, 0]
        nrm = v0 / np.sqrt((v0[:, 0] * v0[:, 0] + v0[:, 1] * v0[:, 1]) + v0[:, 2] * v0[:, 2])[:, None]
        a = np.abs(nrm)
        lead = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), nrm[:, 0], np.where(a[:, 1] >= a[:, 2], nrm[:, 1], nrm[:, 2]))
        nrm = np.where(lead[:, None] < 0.0, -nrm, nrm)
        normal = np.where(good[:, None], nrm, 0.0).astype(F32)
        variation = np.where(good, w[:, 0] / np.where(good, trace, 1.0), 0.0).astype(F32)
    return normal, variation, w, cov


_ORIENTS = (None, 'viewpoint', 'centroid')


def estimate_normals(points, k=16, tree=None, orient=None, viewpoint=None):
    """Normals of a point cloud [n,3] from its k nearest usable points (the point itself included): ``{'normal' float32 [n,3],
    'variation' float32 [n], 'eigenvalues' float64 [n,3], 'covariance' float64 [n,6]}``, see ``_point_normals_numpy`` (the
    definition).  ``normal`` is the eigenvector of the smallest eigenvalue of the neighbours' covariance, its largest-magnitude
    component positive; ``variation = l0 / (l0 + l1 + l2)`` (0 on a plane, 1/3 for an isotropic blob).  A point with fewer than 3
    neighbours or without spread gets a zero normal.  ``orient='viewpoint'`` turns every normal towards ``viewpoint`` (three floats),
    ``orient='centroid'`` away from the centroid of the usable points; a consistent orientation by propagation is not done.  Device
    tensors take ``nearest_points`` on the ``PointTree`` (``tree``; built here if None) and ia_point_normals."""
    _cloud_args(points)
    k = _nearest_k(k)
    if orient not in _ORIENTS:
        raise ValueError(f'orient must be one of {_ORIENTS}, got {orient!r}')
    if (orient == 'viewpoint') != (viewpoint is not None):
        raise ValueError("viewpoint goes with orient='viewpoint'")
    tree = _point_tree_for(points, tree)
    index = tree.nearest(points, k)['index']
    if tree.device is not None:
        from . import hipops
        normal, variation, eig, cov = hipops.point_normals(tree.points, index.contiguous())
        if orient is not None:
            fin = tree.points[torch.isfinite(tree.points).all(1)].double()
            ref = torch.tensor([float(v) for v in viewpoint], dtype=torch.float64, device=tree.device) if orient == 'viewpoint' else fin.mean(0)
            to = (ref - tree.points.double()) if orient == 'viewpoint' else (tree.points.double() - ref)
            normal = torch.where(((normal.double() * to).sum(1) < 0)[:, None], -normal, normal)
        return {'normal': normal, 'variation': variation, 'eigenvalues': eig, 'covariance': cov}
    normal, variation, eig, cov = _point_normals_numpy(tree.points, _np(index))
    if orient is not None:
        p = tree.points.astype(np.float64)
        ref = np.asarray([float(v) for v in viewpoint]) if orient == 'viewpoint' else _finite_rows(p).mean(0)
        to = (ref - p) if orient == 'viewpoint' else (p - ref)
        with np.errstate(invalid='ignore'):
            normal = np.where(((normal.astype(np.float64) * to).sum(1) < 0)[:, None], -normal, normal)
    return {'normal': _as_out(normal, points), 'variation': _as_out(variation, points), 'eigenvalues': _as_out(eig, points, np.float64),
            'covariance': _as_out(cov, points, np.float64)}


def remove_outliers(points, k=16, std_ratio=2.0, tree=None):
    """Statistical outlier removal: ``{'keep' bool [n], 'mean_dist' float64 [n]}``.  ``mean_dist`` is the mean distance, in double, to
    the k nearest usable points other than the point itself (NaN for a point that is not finite or has no neighbour); a point is kept
    iff it is ``<= mean + std_ratio * std`` over the points that have one (the population standard deviation)."""
    _cloud_args(points)
    tree = _point_tree_for(points, tree)
    r = tree.nearest(points, k, exclude_self=True)
    if tree.device is not None:
        d, has = r['dist'].double(), r['index'] >= 0
        cnt = has.sum(1)
        md = torch.where(cnt > 0, torch.where(has, d, torch.zeros_like(d)).sum(1) / cnt.clamp(min=1), torch.full_like(d[:, 0], float('nan')))
        ok = torch.isfinite(md)
        if not bool(ok.any()):
            return {'keep': torch.zeros_like(ok), 'mean_dist': md}
        mu = md[ok].mean()
        sd = ((md[ok] - mu) ** 2).mean().sqrt()
        return {'keep': ok & (md <= mu + float(std_ratio) * sd), 'mean_dist': md}
    d, has = _np(r['dist']).astype(np.float64), _np(r['index']) >= 0
    cnt = has.sum(1)
    with np.errstate(invalid='ignore', divide='ignore'):
        md = np.where(cnt > 0, np.where(has, d, 0.0).sum(1) / np.maximum(cnt, 1), np.nan)
        ok = np.isfinite(md)
        if ok.any():
            mu = md[ok].mean()
            sd = np.sqrt(((md[ok] - mu) ** 2).mean())
            keep = ok & (md <= mu + float(std_ratio) * sd)
        else:
            keep = np.zeros_like(ok)
    return {'keep': _as_out(keep, points, bool), 'mean_dist': _as_out(md, points, np.float64)}


def _cloud_stats(a, b, thresholds, tree_b=None):
    """ia_distance_stats (or its restatement) of the distances from the points a to the cloud b: float64 [14]."""
    dist = nearest_points(a, b, 1, tree=tree_b)['dist'][:, 0]
    if _is_device(b):
        from . import hipops
        return hipops.distance_stats(dist.contiguous(), thresholds).cpu().numpy()
    return _stats_numpy(_np(dist), thresholds)


def _cloud_thresholds(thresholds, *clouds):
    if thresholds is None:
        diag = 0.0
        for v in clouds:
            x = torch.as_tensor(_np(v) if not _is_device(v) else v).float()
            x = x[torch.isfinite(x).all(1)]
            if x.shape[0]:
                diag = max(diag, float((x.amax(0) - x.amin(0)).double().norm()))
        thresholds = [0.005 * diag, 0.01 * diag, 0.02 * diag]
    thresholds = [float(F32(t)) for t in thresholds]
    if len(thresholds) > 8:
        raise ValueError(f'at most 8 thresholds, got {len(thresholds)}')
    return thresholds


def cloud_distance(points_a, points_b, thresholds=None):
    """How far cloud a is from cloud b: the keys of ``surface_distance`` (``mean_ab``, ``rms_ab``, ``max_ab`` and the ``_ba`` ones,
    ``chamfer``, ``chamfer_sq``, ``hausdorff``, ``thresholds``, ``precision``, ``recall``, ``fscore``, ``n_a``, ``n_b``, ``skipped_ab``,
    ``skipped_ba``; ``normal_consistency`` is None) with ``d_ab`` the distance of every point of a to its nearest point of b
    (``nearest_points`` with k = 1) and ``d_ba`` the reverse: the Chamfer distance between point sets.  ``thresholds`` default to 0.5 %,
    1 % and 2 % of the larger bounding-box diagonal.  Device tensors run on the kernels (ia_distance_stats for the sums)."""
    _cloud_args(points_a, 'points_a')
    _cloud_args(points_b, 'points_b')
    if _is_device(points_a) != _is_device(points_b):
        raise ValueError('points_a and points_b must both be device tensors or both be on the host')
    thresholds = _cloud_thresholds(thresholds, points_a, points_b)
    return _distance_report(_cloud_stats(points_a, points_b, thresholds), _cloud_stats(points_b, points_a, thresholds), thresholds)


# ---- rays against the mesh on the same tree (csrc/ray_tree.hip)

_RAY_MODES = ('first', 'any')
_RAY_GUARD = 2.0 ** -14      # ray_tri: the hit point lies in the triangle's box grown by this times the largest |coordinate|
_RAY_SLACK = 2.0 ** -12      # the boxes of the tree grow by this times M = max(|o|_inf, extent): DESIGN.md 4.28
_RAY_TINY = 2.0 ** -100      # a slab product or reciprocal below this is not trusted: the axis admits every t
_RAY_IN, _RAY_OUT = 1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20     # the slab interval's ends are moved outward by these factors
_AO_MAX_RAYS = 1 << 22


def _ray_mode(mode):
    if mode not in _RAY_MODES:
        raise ValueError(f'mode must be one of {_RAY_MODES}, got {mode!r}')
    return mode


def _ray_tri(o, d, A, B, C, dtype=np.float64):
    """The per-triangle function of the ray queries (csrc/geom_common.h ray_tri) in ``dtype`` on broadcastable [..., 3] arrays:
    ``(t, w, ok)``.  Relative to the origin (``a = A - o`` ...), ``w = (d . (b x c), d . (c x a), d . (a x b))``; the ray is inside iff
    no ``w`` is negative or none is positive (closed edges, both orientations); ``t = (n . a) / (n . d)`` with ``n = (b - a) x (c - a)``;
    ``ok = inside and n . d != 0 and t finite`` and the point ``o + t d`` lies in the triangle's own bounding box grown by ``2^-14
    max(|o|_inf, |A|_inf, |B|_inf, |C|_inf)`` on every side (far from the ray's origin the edge functions alone accept small triangles
    that the ray misses by any distance; with this clause a box that the ray misses holds no accepted triangle).  The caller adds the ray's interval ``t_lo <= t <= t_hi`` and forms the barycentrics
    ``w / ((w0 + w1) + w2)``.  Every operation is rounded on its own, so the float32 run follows the kernel operation by operation.
    Not watertight: the three signs of one triangle are rounded separately."""
    o, d, A, B, C = (np.asarray(x, dtype=dtype) for x in (o, d, A, B, C))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        a, b, c = A - o, B - o, C - o
        a, b, c, d = np.broadcast_arrays(a, b, c, d)
        w = np.stack([_dot3(d, _cross3(b, c)), _dot3(d, _cross3(c, a)), _dot3(d, _cross3(a, b))], -1)
        inside = (w >= 0).all(-1) | (w <= 0).all(-1)
        n = _cross3(b - a, c - a)
        den = _dot3(n, d)
        t = _dot3(n, a) / den
        g = dtype(_RAY_GUARD) * np.maximum(np.maximum(np.abs(o).max(-1), np.abs(A).max(-1)), np.maximum(np.abs(B).max(-1), np.abs(C).max(-1)))
        p = o + t[..., None] * d
        lo, hi = np.minimum(np.minimum(A, B), C) - g[..., None], np.maximum(np.maximum(A, B), C) + g[..., None]
        boxed = ((lo <= p) & (p <= hi)).all(-1)
    return t, w, inside & (den != 0) & np.isfinite(t) & boxed


def _ray_rows(origins, dirs, t_min, t_max):
    """(origins, dirs float32 [N,3], t_lo, t_hi float32 [N], walked bool [N]): scalars or per-ray intervals; a ray with a non-finite
    origin or direction or a NaN interval end is not walked."""
    o = np.asarray(origins, dtype=F32).reshape(-1, 3)
    d = np.asarray(dirs, dtype=F32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError(f'origins and dirs must have the same shape, got {o.shape} and {d.shape}')
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, dtype=F32).reshape(-1), (o.shape[0],)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, dtype=F32).reshape(-1), (o.shape[0],)))
    return o, d, lo, hi, np.isfinite(o).all(1) & np.isfinite(d).all(1) & ~np.isnan(lo) & ~np.isnan(hi)


def _ray_result(o, d, tris, at, hit, ok, dtype):
    """(t, bary, point) of rays against their winning triangles ``tris[at]`` (where ``hit``); +inf / NaN / NaN without a hit, NaN
    for a ray that was not walked."""
    n = o.shape[0]
    t = np.where(ok, np.inf, np.nan).astype(dtype)
    bary, point = np.full((n, 3), np.nan, dtype=dtype), np.full((n, 3), np.nan, dtype=dtype)
    r = np.flatnonzero(hit)
    if r.size:
        with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
            tr = tris[at[r]]
            tt, w, _ = _ray_tri(o[r], d[r], tr[:, 0], tr[:, 1], tr[:, 2], dtype)
            t[r] = tt
            bary[r] = w / ((w[:, 0] + w[:, 1]) + w[:, 2])[:, None]
            point[r] = o[r] + tt[:, None] * d[r]
    return t, bary, point


def _ray_leaf(o, d, lo, hi, tris, faces, dtype):
    """Rays [n] against triangles [m] with input indices ``faces``: (accepted [n,m], t [n,m], per ray the smallest accepted t (+inf
    without one), the lowest face among those that attain it, and its column)."""
    t, _, acc = _ray_tri(o[:, None, :], d[:, None, :], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2], dtype)
    acc = acc & (lo[:, None] <= t) & (t <= hi[:, None])
    tv = np.where(acc, t, np.inf)
    tm = tv.min(1) if tv.shape[1] else np.full(o.shape[0], np.inf, dtype=dtype)
    tie = acc & (tv == tm[:, None])
    fm = np.where(tie, faces[None, :], np.iinfo(np.int64).max).min(1) if tv.shape[1] else np.full(o.shape[0], -1, dtype=np.int64)
    col = np.argmax(tie & (faces[None, :] == fm[:, None]), axis=1) if tv.shape[1] else np.zeros(o.shape[0], dtype=np.int64)
    return acc, tm, fm, col


def _ray_mesh_numpy(origins, dirs, verts, faces, t_min=0.0, t_max=np.inf, dtype=np.float64, pairs=1 << 20):
    """The definition of the ray queries, and the NumPy restatement of ia_ray_mesh_brute in ``dtype``: every ray against every usable
    triangle with ``_ray_tri``; the first hit is the smallest pair (t, input face index) over the triangles accepted within the ray's
    own interval.  ``(hit bool [N], t [N], face int32 [N], bary [N,3], point [N,3])``: +inf / -1 / NaN / NaN without an accepted
    triangle, NaN / -1 / NaN / NaN for a ray that is not walked (``_ray_rows``); the any-hit answer is ``hit``."""
    o32, d32, lo32, hi32, ok = _ray_rows(origins, dirs, t_min, t_max)
    o, d, lo, hi = (x.astype(dtype) for x in (o32, d32, lo32, hi32))
    v = np.asarray(verts, dtype=F32).reshape(-1, 3).astype(dtype)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = o.shape[0]
    in_range = ((f >= 0) & (f < v.shape[0])).all(1)
    tri = v[np.where(in_range[:, None], f, 0)] if v.shape[0] else np.zeros((f.shape[0], 3, 3), dtype=dtype)
    usable = np.flatnonzero(in_range & np.isfinite(tri).all((1, 2)))
    tri = tri[usable]
    hit, face, at = np.zeros(n, dtype=bool), np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int64)
    rows = np.flatnonzero(ok)
    if usable.size and rows.size:
        step = max(1, pairs // usable.size)
        for s in range(0, rows.size, step):
            r = rows[s:s + step]
            acc, _, fm, col = _ray_leaf(o[r], d[r], lo[r], hi[r], tri, usable, dtype)
            has = acc.any(1)
            hit[r], face[r], at[r] = has, np.where(has, fm, -1), col
    t, bary, point = _ray_result(o, d, tri, at, hit, ok, dtype)
    return hit, t, face, bary, point


def _ray_slab_skip(o, d, inv, slack, row, t_lo, t_max):
    """The skip test of ia_ray_mesh_tree for rays [n] at one box row (lo.xyz, 0, hi.xyz, 0), in the dtype of the arrays."""
    one = o.dtype.type
    tiny = one(_RAY_TINY)
    near, far = np.full(o.shape[0], -np.inf, dtype=o.dtype), np.full(o.shape[0], np.inf, dtype=o.dtype)
    for k in range(3):
        t0, t1 = ((row[k] - o[:, k]) - slack) * inv[:, k], ((row[4 + k] - o[:, k]) + slack) * inv[:, k]
        free = np.isnan(t0) | np.isnan(t1) | ((d[:, k] != 0) & np.isinf(inv[:, k])) | (np.minimum(np.minimum(np.abs(t0), np.abs(t1)), np.abs(inv[:, k])) < tiny)
        t0, t1 = np.where(free, -np.inf, t0).astype(o.dtype), np.where(free, np.inf, t1).astype(o.dtype)
        near, far = np.maximum(near, np.minimum(t0, t1)), np.minimum(far, np.maximum(t0, t1))
    near = near * np.where(near > 0, one(_RAY_IN), one(_RAY_OUT))
    far = far * np.where(far > 0, one(_RAY_OUT), one(_RAY_IN))
    return (near > far) | (near > t_max) | (far < t_lo)


def _ray_tree_numpy(origins, dirs, tree, t_min=0.0, t_max=np.inf, mode='first', dtype=np.float64):
    """NumPy restatement of ia_ray_mesh_tree in ``dtype`` on a host ``WindingTree``: ``(hit, t, face int32, bary, point, counts int64
    [N,2] = boxes tested, ray-triangle pairs of the leaves entered)``.  Depth first from the root, children in index order; ``best =
    (t, face)`` is ordered lexicographically and starts at ``(+inf, -1)``; an entered leaf evaluates ``_ray_tri`` for its faces and
    keeps the smaller accepted pair.  A node is skipped iff the slab test on its box, grown by ``slack = 2^-12 M``
    with ``M = max(|o|_inf, tree.extent)``, leaves no t in ``[t_lo, min(t_hi, best.t)]`` (``_ray_slab_skip``; any NaN enters).  With
    ``mode='any'`` a ray that has a hit tests nothing more, and everything but ``hit`` and ``counts`` is what no hit gives.  The
    result equals ``_ray_mesh_numpy`` in the same ``dtype``: the tree only prunes (DESIGN.md 4.28 states on what that rests)."""
    if tree.device is not None:
        raise ValueError('_ray_tree_numpy restates the query on a host WindingTree')
    any_hit = _ray_mode(mode) == 'any'
    o32, d32, lo32, hi32, ok = _ray_rows(origins, dirs, t_min, t_max)
    o, d, lo, hi = (x.astype(dtype) for x in (o32, d32, lo32, hi32))
    tris = np.asarray(tree.tris, dtype=F32).reshape(-1, 3, 3).astype(dtype)
    order = np.asarray(tree.order, dtype=np.int64)
    counts, boxes = list(tree.counts), np.asarray(tree.boxes, dtype=F32).astype(dtype)
    n, fu = o.shape[0], tris.shape[0]
    best_t, best_f, best_at = np.full(n, np.inf, dtype=dtype), np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    n_box, n_pair = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore', under='ignore', divide='ignore'):
        ext = dtype(tree.extent)
        big = np.maximum(np.abs(o).max(1) if n else np.zeros(0, dtype=dtype), ext)
        slack = (dtype(_RAY_SLACK) * big).astype(dtype)
        inv = (dtype(1) / d).astype(dtype)

        def visit(lvl, j, at, idx):
            if any_hit:
                idx = idx[best_f[idx] < 0]
            n_box[idx] += 1
            skip = _ray_slab_skip(o[idx], d[idx], inv[idx], slack[idx], boxes[at], lo[idx], np.minimum(hi[idx], best_t[idx]))
            r = idx[~skip]
            if lvl == 0 and r.size:
                sl = slice(j * WINDING_LEAF, min((j + 1) * WINDING_LEAF, fu))
                acc, tm, fm, col = _ray_leaf(o[r], d[r], lo[r], hi[r], tris[sl], order[sl], dtype)
                take = acc.any(1) & ((tm < best_t[r]) | ((tm == best_t[r]) & (fm < best_f[r])))
                rr = r[take]
                best_t[rr], best_f[rr], best_at[rr] = tm[take], fm[take], sl.start + col[take]
                n_pair[r] += sl.stop - sl.start
            return r

        _tree_walk(counts, np.flatnonzero(ok), visit)
    hit = best_f >= 0
    if any_hit:
        hit, best_f = hit.copy(), np.full(n, -1, dtype=np.int64)
        t, bary, point = _ray_result(o, d, tris, best_at, np.zeros(n, dtype=bool), ok, dtype)
    else:
        t, bary, point = _ray_result(o, d, tris, best_at, hit, ok, dtype)
    return hit, t, best_f.astype(np.int32), bary, point, np.stack([n_box, n_pair], -1)


def _ao_table(samples, seed):
    """``samples`` cosine-weighted directions of the upper hemisphere (z up), float32 [S,3]: made in float64 from ``seed``
    (``r = sqrt(u1)``, ``phi = 2 pi u2``, ``(r cos phi, r sin phi, sqrt(1 - u1))``) and cast once."""
    samples = int(samples)
    if samples < 1 or samples > 65536:
        raise ValueError(f'samples must be in [1, 65536], got {samples}')
    u = np.random.RandomState(int(seed)).random_sample((samples, 2))
    r, phi = np.sqrt(u[:, 0]), 2.0 * np.pi * u[:, 1]
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u[:, 0])], -1).astype(F32)


def _ao_rays_numpy(verts, normals, table, bias):
    """NumPy restatement of ia_ao_rays in float32: ``(origins, dirs)`` float32 [V S, 3], ray ``v S + s``: origin ``v + bias n``,
    direction ``(t1 x + t2 y) + n z`` per component for the table's ``(x, y, z)`` with the branch-free basis of Duff et al. (2017):
    ``sign = copysign(1, n.z)``, ``a = -1 / (sign + n.z)``, ``b = (n.x n.y) a``, ``t1 = (1 + ((sign n.x) n.x) a, sign b, -(sign
    n.x))``, ``t2 = (b, sign + (n.y n.y) a, -n.y)``.  A non-finite normal gives NaN rays."""
    p, n, c = (np.asarray(x, dtype=F32).reshape(-1, 3) for x in (verts, normals, table))
    bias = F32(bias)
    with np.errstate(invalid='ignore', over='ignore', under='ignore', divide='ignore'):
        sign = np.copysign(F32(1), n[:, 2])
        a = F32(-1) / (sign + n[:, 2])
        b = (n[:, 0] * n[:, 1]) * a
        sx = sign * n[:, 0]
        t1 = np.stack([F32(1) + (sx * n[:, 0]) * a, sign * b, -sx], -1)[:, None, :]
        t2 = np.stack([b, sign + (n[:, 1] * n[:, 1]) * a, -n[:, 1]], -1)[:, None, :]
        nn = n[:, None, :]
        dirs = (t1 * c[None, :, 0:1] + t2 * c[None, :, 1:2]) + nn * c[None, :, 2:3]
        origins = np.broadcast_to((p + bias * n)[:, None, :], dirs.shape)
        bad = ~np.isfinite(n).all(1)
        origins, dirs = np.where(bad[:, None, None], F32(np.nan), origins), np.where(bad[:, None, None], F32(np.nan), dirs)
    return origins.reshape(-1, 3).astype(F32), dirs.reshape(-1, 3).astype(F32)


class WindingTree:
    """The cluster tree of one mesh for ``winding_number(method='tree')``, built once: ``order`` (sorted position -> input face: the
    usable faces by the 30-bit Morton key of their centroid, ties by face index, then the unusable ones), ``tris`` (the triangles in
    that order), ``nodes`` (float32 [n,20]: centre, radius, dipole, area and the first-derivative tensor Q per node, leaves first),
    ``counts`` (nodes per level) and ``info``.  Leaves hold ``WINDING_LEAF`` faces, upper nodes ``WINDING_BRANCH`` children; there are
    no pointers.  Device tensors build on the kernels (``grid``: a ``TriangleGrid`` of this mesh whose packed triangles are reused);
    CPU tensors and NumPy arrays take the NumPy restatement, which is the definition.  ``query(points, beta)`` -> float64 [...]."""

    def __init__(self, verts, faces, grid=None):
        if grid is not None:
            verts, faces = grid.verts, grid.faces
        _mesh_args(verts, faces)
        self.device = verts.device if _is_device(verts) else None
        self._like = verts
        if self.device is not None:
            from . import hipops
            if grid is None:
                grid = TriangleGrid(verts, faces, build=False)
            lo, scale = _morton_cube(grid.lo, grid.hi)
            self.order, self.tris, self.nodes, self.counts, self.usable = hipops.winding_tree_build(grid.tris, lo.tolist(), float(scale))
            self.extent = float(grid.extent)
        else:
            t = _winding_tree_numpy(_np(verts), _np(faces))
            fin = _finite_rows(np.asarray(_np(verts), dtype=F32).reshape(-1, 3))
            self.extent = float(np.abs(fin).max()) if fin.shape[0] else 0.0
            lo, scale = t['lo'], t['scale']
            self.order, self.tris, self.counts, self.usable = t['order'], t['tris'], t['counts'], t['usable']
            self.nodes64 = t['nodes64']
            self.nodes = t['nodes64'].astype(F32)
        self.lo, self.scale = [float(x) for x in lo], float(scale)
        self.info = {'faces': int(faces.shape[0]), 'usable': int(self.usable), 'levels': len(self.counts), 'nodes': int(sum(self.counts)),
                     'leaf': WINDING_LEAF, 'branch': WINDING_BRANCH}
        self._boxes = self._order32 = None

    @classmethod
    def from_grid(cls, grid):
        """The tree of the mesh of a ``TriangleGrid``, from its packed triangles."""
        return cls(None, None, grid=grid)

    def _sorted(self, points, sort, fn, *rows):
        """``list(fn(hipops, pts, *rows))`` for device points as float32 [N,3], Morton-sorted if ``sort`` and N > 64; unsorted on
        return.  ``rows``: device tensors with one row per point, taken along in the points' order."""
        from . import hipops
        pts = torch.as_tensor(points).detach().to(self.device).float().reshape(-1, 3).contiguous()
        if not (sort and pts.shape[0] > 64):
            return list(fn(hipops, pts, *rows))
        perm = torch.argsort(hipops.winding_tree_point_keys(pts, self.lo, self.scale), stable=True)
        back = torch.empty_like(perm)
        back[perm] = torch.arange(perm.numel(), device=perm.device)
        return [None if x is None else x[back] for x in fn(hipops, pts[perm].contiguous(), *[x[perm].contiguous() for x in rows])]

    def query(self, points, beta=2.0, return_bound=False, return_counts=False, sort=True):
        """Winding numbers float64 [...] of points [..., 3]; with ``return_bound`` also the truncation bound, with ``return_counts``
        also int [..., 2] (far terms, exact pairs).  ``sort`` (device): query in Morton order of the points, so that a wave's lanes walk
        the same nodes, and return in the caller's order; it changes no result."""
        b32 = _winding_beta(beta)
        lead = tuple(points.shape[:-1])
        if self.device is not None:
            w, bound, cnt = self._sorted(points, sort, lambda hipops, pts: hipops.winding_tree_query(
                pts, self.tris, self.nodes, self.usable, float(b32), bound=return_bound, counts=return_counts))
            out = [w.reshape(lead)]
            if return_bound:
                out.append(bound.reshape(lead))
            if return_counts:
                out.append(cnt.reshape(lead + (2,)))
        else:
            w, bound, _, nf, npair = _winding_tree_query_numpy(_np(points), self.tris, self.nodes, self.counts, b32)
            out = [_as_out(w.reshape(lead), points, np.float64)]
            if return_bound:
                out.append(_as_out(bound.reshape(lead), points, np.float64))
            if return_counts:
                out.append(_as_out(np.stack([nf, npair], -1).reshape(lead + (2,)), points, np.int64))
        return out[0] if len(out) == 1 else tuple(out)

    @property
    def boxes(self):
        """float32 [n,8]: the bounding box (lo.xyz, 0, hi.xyz, 0) of every node, built on first use (ia_tree_boxes on the device,
        ``_tree_boxes_numpy`` on the host); what ``closest`` prunes with."""
        if self._boxes is None:
            if self.device is not None:
                from . import hipops
                self._boxes = hipops.tree_boxes(self.tris, self.usable, int(sum(self.counts)))
            else:
                self._boxes = _tree_boxes_numpy(self.tris, self.counts)
        return self._boxes

    def closest(self, points, return_counts=False, sort=True):
        """``{'dist' [...], 'face' int64 [...], 'point' [..., 3]}`` of points [..., 3]: what ``closest_point`` gives (the same bits),
        by branch and bound over the tree (``_closest_tree_numpy`` is the definition); with ``return_counts`` also ``'counts'`` int
        [..., 2] (boxes tested, point-triangle pairs evaluated).  ``sort`` (device): query in Morton order of the points and return in
        the caller's order; it changes no result.  A host tree answers in float64."""
        lead = tuple(points.shape[:-1])
        if self.device is not None:
            if self._order32 is None:
                self._order32 = self.order.int().contiguous()
            dist, face, point, cnt = self._sorted(points, sort, lambda hipops, pts: hipops.closest_point_tree(
                pts, self.tris, self._order32, self.boxes, self.usable, self.extent, counts=return_counts))
            out = {'dist': dist.reshape(lead), 'face': face.long().reshape(lead), 'point': point.reshape(lead + (3,))}
            if return_counts:
                out['counts'] = cnt.reshape(lead + (2,))
        else:
            dist, face, point, cnt = _closest_tree_numpy(_np(points), self)
            out = {'dist': _as_out(dist.reshape(lead), points), 'face': _as_out(face.reshape(lead), points, np.int64),
                   'point': _as_out(point.reshape(lead + (3,)), points)}
            if return_counts:
                out['counts'] = _as_out(cnt.reshape(lead + (2,)), points, np.int64)
        return out

    def _ray_rows_device(self, origins, dirs, t_min, t_max):
        o = torch.as_tensor(origins).detach().to(self.device).float().reshape(-1, 3).contiguous()
        d = torch.as_tensor(dirs).detach().to(self.device).float().reshape(-1, 3).contiguous()
        if o.shape != d.shape:
            raise ValueError(f'origins and dirs must have the same shape, got {tuple(o.shape)} and {tuple(d.shape)}')
        ends = [torch.as_tensor(x, dtype=torch.float32).to(self.device).reshape(-1).expand(o.shape[0]).contiguous() for x in (t_min, t_max)]
        if self._order32 is None:
            self._order32 = self.order.int().contiguous()
        return o, d, ends[0], ends[1]

    def rays(self, origins, dirs, t_min=0.0, t_max=float('inf'), mode='first', return_counts=False, sort=True, brute=False):
        """Rays ``origins + t dirs`` [..., 3] against the mesh, ``t_min <= t <= t_max`` (scalars or per-ray arrays [...]):
        ``mode='first'`` -> ``{'hit' bool, 't', 'face' int64, 'bary' [..., 3], 'point' [..., 3]}`` of the first hit, the smallest pair
        (t, input face index) over the triangles that ``_ray_tri`` accepts (``_ray_mesh_numpy`` is the definition; +inf / -1 / NaN /
        NaN without one, NaN / -1 / NaN / NaN for a ray with a non-finite origin or direction or a NaN interval end);
        ``mode='any'`` -> ``{'hit'}``.  The tree only prunes.  With ``return_counts`` also ``'counts'`` int [..., 2] (boxes tested,
        ray-triangle pairs of the leaves entered).  ``sort`` (device): query in Morton order of the origins and return in the
        caller's order; it changes no result.  ``brute``: every ray against every usable triangle instead, on host and device (no counts; what
        ``ray_mesh(brute=True)`` takes on the device).  A host tree answers in float64.  The per-triangle test is not watertight: a ray aimed at a shared edge or vertex can miss both neighbours."""
        any_hit = _ray_mode(mode) == 'any'
        lead = tuple(origins.shape[:-1])
        if self.device is not None:
            o, d, lo, hi = self._ray_rows_device(origins, dirs, t_min, t_max)
            if brute:
                def run(hipops, o, d, lo, hi):
                    return hipops.ray_mesh_brute(o, d, lo, hi, self.tris, self._order32, self.usable, any_hit=any_hit) + (None,)
            else:
                def run(hipops, o, d, lo, hi):
                    return hipops.ray_mesh_tree(o, d, lo, hi, self.tris, self._order32, self.boxes, self.usable, self.extent, any_hit=any_hit,
                                                counts=return_counts)
            hit, t, face, bary, point, cnt = self._sorted(o, sort and not brute, run, d, lo, hi)
            out = {'hit': hit.reshape(lead)}
            if not any_hit:
                out.update(t=t.reshape(lead), face=face.long().reshape(lead), bary=bary.reshape(lead + (3,)), point=point.reshape(lead + (3,)))
            if return_counts and not brute:
                out['counts'] = cnt.reshape(lead + (2,))
        else:
            if brute:                                                                  # the usable triangles in input order
                order = np.asarray(self.order, dtype=np.int64)[:self.usable]
                back = np.argsort(order)
                tri = np.asarray(self.tris, dtype=F32).reshape(-1, 3, 3)[back]
                hit, t, face, bary, point = _ray_mesh_numpy(_np(origins), _np(dirs), tri.reshape(-1, 3), np.arange(3 * back.size).reshape(-1, 3),
                                                            _np(t_min), _np(t_max))
                face, cnt = np.where(hit, order[back][np.maximum(face, 0)], -1), None
            else:
                hit, t, face, bary, point, cnt = _ray_tree_numpy(_np(origins), _np(dirs), self, _np(t_min), _np(t_max), mode)
            out = {'hit': _as_out(hit.reshape(lead), origins, bool)}
            if not any_hit:
                out.update(t=_as_out(t.reshape(lead), origins), face=_as_out(face.reshape(lead), origins, np.int64),
                           bary=_as_out(bary.reshape(lead + (3,)), origins), point=_as_out(point.reshape(lead + (3,)), origins))
            if return_counts and not brute:
                out['counts'] = _as_out(cnt.reshape(lead + (2,)), origins, np.int64)
        return out


def _winding_tree_for(verts, faces, grid, tree):
    if tree is None:
        return WindingTree(verts, faces, grid=grid)
    if not isinstance(tree, WindingTree):
        raise ValueError(f'tree must be a WindingTree, got {type(tree).__name__}')
    if (tree.device is not None) != _is_device(verts):
        raise ValueError('tree: the WindingTree must live where the mesh lives (device or host)')
    return tree


def winding_number(points, verts, faces, grid=None, method='exact', beta=2.0, tree=None, return_bound=False):
    """Generalised winding number of points [..., 3] with respect to the triangle soup (verts float32 [V,3], faces [F,3]): float64
    [...].  ``w(p) = (1 / 4 pi) sum_f omega_f(p)`` with ``omega_f`` the signed solid angle of triangle f seen from p (``_solid_angle``,
    float32): 1 inside a closed mesh wound outward (the winding of ``marching_cubes``), 0 outside, k where k such surfaces nest, and a
    smooth value in between for an open mesh (a head scan open at the neck: above 0.5 well inside, below it outside).  A triangle
    without area contributes 0, one with an index out of range or a non-finite vertex is ignored; a non-finite point gives NaN; a mesh
    without usable triangles 0.  The terms are added in double in a fixed order (``_winding_numpy``), so a point's value does not depend
    on the other points of the call.  The cost is N F pairs.  Device tensors run on ia_winding_number (``grid``: a ``TriangleGrid`` of
    this mesh whose packed triangles are reused); CPU tensors and NumPy arrays take the NumPy restatement (float64 per pair).

    ``method='tree'`` is the approximation for large meshes: a ``WindingTree`` (``tree``, or built here) whose nodes farther from the
    point than ``beta`` times their radius are replaced by a dipole and its first derivative; nearer leaves add their exact terms.
    ``beta`` is greater than 1; larger is more accurate and slower, ``inf`` adds the exact terms in the tree's order.  The value is
    again a pure function of point, mesh and ``beta``.  ``return_bound=True`` returns ``(w, bound)`` with ``bound`` the derived bound of
    the truncation error per point (0 for ``method='exact'``): loose, about 1e2 times the error at ``beta = 2``."""
    _mesh_args(verts, faces)
    _winding_method(method)
    lead = tuple(points.shape[:-1])
    if method == 'tree':
        _winding_beta(beta)
        return _winding_tree_for(verts, faces, grid, tree).query(points, beta, return_bound=return_bound)
    if _is_device(verts):
        w = _winding_device(points, verts, faces, grid).reshape(lead)
    else:
        w = _as_out(_winding_numpy(_np(points), _np(verts), _np(faces))[0].reshape(lead), points, np.float64)
    if return_bound:
        return w, (torch.zeros_like(w) if isinstance(w, torch.Tensor) else np.zeros_like(w))
    return w


def inside(points, verts, faces, threshold=0.5, method='exact', beta=2.0, tree=None):
    """bool [...]: ``winding_number(points) >= threshold`` (a non-finite point is not inside).  ``method`` / ``beta`` / ``tree``: those
    of ``winding_number``."""
    return winding_number(points, verts, faces, method=method, beta=beta, tree=tree) >= threshold


def signed_distance(points, verts, faces, grid=None, threshold=0.5, method='exact', beta=2.0, tree=None, search='grid'):
    """Signed distance of points to a mesh: ``{'sdf', 'dist', 'face', 'point', 'winding'}``.  ``dist``, ``face`` and ``point`` are the
    results of ``closest_point`` (the same bits), ``winding`` (float64) is ``winding_number`` and ``sdf`` is ``-dist`` where
    ``winding >= threshold``, else ``+dist``: negative inside.  ``grid``: a ``TriangleGrid`` of the mesh (device), used by both.
    ``method`` / ``beta`` / ``tree``: those of ``winding_number``.  ``search``: that of ``closest_point``; with ``search='tree'`` no
    uniform grid is built, and with ``method='tree'`` as well one ``WindingTree`` (``tree``, or built here) gives sign and magnitude."""
    _mesh_args(verts, faces)
    _winding_method(method)
    _closest_search(search)
    if _is_device(verts) and grid is None:
        grid = TriangleGrid(verts, faces, build=search != 'tree')
    if search == 'tree':
        tree = _winding_tree_for(verts, faces, grid, tree)
        r = tree.closest(points)
    else:
        r = closest_point(points, verts, faces, grid=grid)
    w = winding_number(points, verts, faces, grid=grid, method=method, beta=beta, tree=tree).reshape(r['dist'].shape)
    neg = w >= threshold
    sdf = torch.where(neg, -r['dist'], r['dist']) if isinstance(neg, torch.Tensor) else np.where(neg, -r['dist'], r['dist'])
    return {'sdf': sdf, 'dist': r['dist'], 'face': r['face'], 'point': r['point'], 'winding': w}


def ray_mesh(origins, dirs, verts, faces, t_min=0.0, t_max=float('inf'), mode='first', brute=False, tree=None):
    """What the rays ``origins + t dirs`` [..., 3], ``t_min <= t <= t_max`` (scalars or per-ray arrays), hit on the triangle mesh
    (verts float32 [V,3], faces [F,3]): ``{'hit' bool [...], 't' float32, 'face' int64, 'bary' [..., 3], 'point' [..., 3]}`` of the
    first hit, the smallest pair (t, input face index) over the triangles ``_ray_tri`` accepts; ``mode='any'`` returns ``{'hit'}``
    only and stops at the first triangle found.  ``dirs`` need not have unit length: ``t`` is in units of ``|dirs|``.  Both sides of a
    triangle are hit; a triangle without area or with a non-finite vertex never is.  No hit: ``t = +inf``, ``face = -1``, NaN
    ``bary`` and ``point``; a ray with a non-finite origin or direction or a NaN interval end: ``t = NaN`` as well.  The per-triangle
    test is fp32 and not watertight: a ray aimed exactly at a shared edge or vertex can slip between the neighbours.  Device tensors
    run on ia_ray_mesh_tree over a ``WindingTree`` (``tree``, or built here) or, with ``brute=True``, on ia_ray_mesh_brute: the same
    bits.  CPU tensors and NumPy arrays take the NumPy restatements in float64."""
    _mesh_args(verts, faces)
    _ray_mode(mode)
    if _is_device(verts) or not brute:
        return _winding_tree_for(verts, faces, None, tree).rays(origins, dirs, t_min, t_max, mode=mode, brute=brute)
    lead = tuple(origins.shape[:-1])
    hit, t, face, bary, point = _ray_mesh_numpy(_np(origins), _np(dirs), _np(verts), _np(faces), _np(t_min), _np(t_max))
    out = {'hit': _as_out(hit.reshape(lead), origins, bool)}
    if mode == 'first':
        out.update(t=_as_out(t.reshape(lead), origins), face=_as_out(face.reshape(lead), origins, np.int64),
                   bary=_as_out(bary.reshape(lead + (3,)), origins), point=_as_out(point.reshape(lead + (3,)), origins))
    return out


def occluded(a, b, verts, faces, margin=1e-4, tree=None):
    """bool [...]: does the mesh meet the segment from ``a`` to ``b`` [..., 3] strictly between its ends?  ``ray_mesh(a, b - a,
    t_min=margin, t_max=1 - margin, mode='any')['hit']`` with ``b - a`` in float32: ``margin`` (a fraction of the segment) keeps a
    surface that an end lies on from counting."""
    if isinstance(a, torch.Tensor):
        d = torch.as_tensor(b).to(a.device).float() - a.float()
    else:
        d = np.asarray(_np(b), dtype=F32) - np.asarray(a, dtype=F32)
    return ray_mesh(a, d, verts, faces, t_min=margin, t_max=1.0 - margin, mode='any', tree=tree)['hit']


def ambient_occlusion(verts, faces, samples=64, radius=None, bias=None, normals=None, seed=0, tree=None):
    """Ambient occlusion per vertex: ``{'ao' float32 [V], 'unoccluded' int32 [V], 'samples'}`` with ``ao = unoccluded / samples``,
    the share of ``samples`` cosine-weighted directions of the hemisphere about the vertex normal along which nothing of the mesh
    lies within ``radius`` (None: no limit).  The directions are one table for all vertices (``_ao_table(samples, seed)``, float64
    cast to float32), turned into the frame of each normal (``_ao_rays_numpy``); the rays start at ``v + bias n`` (``bias`` None:
    ``2^-12`` times the largest |coordinate| of the mesh) and are any-hit queries on the tree.  ``normals``: unit vertex normals
    (None: ``mesh_normals(weighting='area')``).  A vertex with a non-finite position or normal counts as unoccluded.  The counts are
    integer sums: the same from run to run, and the host route (the float32 restatements) gives the device's integers.  At most
    about 2^22 rays are alive at once."""
    _mesh_args(verts, faces)
    table = _ao_table(samples, seed)
    s = table.shape[0]
    tree = _winding_tree_for(verts, faces, None, tree)
    bias = float(F32(2.0 ** -12) * F32(tree.extent)) if bias is None else float(bias)
    t_max = float('inf') if radius is None else float(radius)
    if normals is None:
        normals = mesh_normals(verts, faces, weighting='area')
    if tuple(normals.shape) != tuple(verts.shape):
        raise ValueError(f'normals must be [V,3] like verts, got {tuple(normals.shape)}')
    nv = verts.shape[0]
    step = max(1, _AO_MAX_RAYS // s)
    if tree.device is not None:
        from . import hipops
        v = verts.detach().to(tree.device).float().contiguous()
        n = torch.as_tensor(normals).detach().to(tree.device).float().contiguous()
        tab = torch.from_numpy(table).to(tree.device)
        free = torch.empty(nv, dtype=torch.int32, device=tree.device)
        for at in range(0, nv, step):
            o, d = hipops.ao_rays(v[at:at + step].contiguous(), n[at:at + step].contiguous(), tab, bias)
            hit = tree.rays(o, d, 0.0, t_max, mode='any')['hit']
            free[at:at + step] = (s - hit.view(-1, s).sum(1)).int()
        return {'ao': free.float() / float(s), 'unoccluded': free, 'samples': s}
    v, n = np.asarray(_np(verts), dtype=F32), np.asarray(_np(normals), dtype=F32)
    free = np.zeros(nv, dtype=np.int32)
    for at in range(0, nv, step):
        o, d = _ao_rays_numpy(v[at:at + step], n[at:at + step], table, bias)
        hit = _ray_tree_numpy(o, d, tree, 0.0, t_max, 'any', dtype=F32)[0]
        free[at:at + step] = s - hit.reshape(-1, s).sum(1)
    return {'ao': _as_out(free.astype(F32) / F32(s), verts), 'unoccluded': _as_out(free, verts, np.int32), 'samples': s}


def _finite_box(*vert_sets):
    """(lo, hi) float64 [3] of the finite rows of the vertex arrays given, or None when there is none."""
    rows = []
    for v in vert_sets:
        if _is_device(v):
            x = v.detach().float()
            x = x[torch.isfinite(x).all(1)]
            if x.shape[0]:
                rows.append(torch.stack([x.amin(0), x.amax(0)]).cpu().numpy().astype(np.float64))
        else:
            x = np.asarray(_np(v), dtype=np.float64).reshape(-1, 3)
            x = x[np.isfinite(x).all(1)]
            if x.shape[0]:
                rows.append(np.stack([x.min(0), x.max(0)]))
    if not rows:
        return None
    box = np.stack(rows)
    return box[:, 0].min(0), box[:, 1].max(0)


def _volume_lattice(box, resolution, origin, spacing, padding):
    """The lattice of ``mesh_to_volume``: ``((nx, ny, nz), origin, spacing)``, point (i, j, k) at ``origin + index * spacing``."""
    padding = int(padding)
    if padding < 0:
        raise ValueError(f'padding must be >= 0, got {padding}')
    if (origin is None) != (spacing is None):
        raise ValueError('origin and spacing are given together or not at all')
    if origin is not None:
        dims, org, spc = _res3(resolution), _vec3(origin), _vec3(spacing)
        if not all(np.isfinite(s) and s > 0 for s in spc) or not all(np.isfinite(o) for o in org):
            raise ValueError(f'origin must be finite and spacing positive, got {origin} and {spacing}')
        return dims, org, spc
    if box is None or not (box[1] - box[0]).max() > 0:
        raise ValueError('mesh_to_volume: the mesh has no extent; give origin and spacing')
    lo, hi = box
    size = hi - lo
    if np.isscalar(resolution):
        cells = int(resolution) - 1 - 2 * padding
        if cells < 1:
            raise ValueError(f'resolution {resolution} leaves no cell between {padding} padding cells on each side')
        h = float(size.max()) / cells
        dims = tuple(int(resolution) if a == int(np.argmax(size)) else int(np.ceil(size[a] / h - 1e-9)) + 1 + 2 * padding for a in range(3))
        dims = tuple(max(d, 2) for d in dims)
        mid = (lo + hi) / 2
        return dims, tuple(float(mid[a] - (dims[a] - 1) * h / 2) for a in range(3)), (h,) * 3
    dims = _res3(resolution)
    spc = []
    for a in range(3):
        cells = dims[a] - 1 - 2 * padding
        if cells < 1:
            raise ValueError(f'resolution {resolution} leaves no cell between {padding} padding cells on each side')
        spc.append(float(size[a]) / cells if size[a] > 0 else float(size.max()) / cells)
    mid = (lo + hi) / 2
    return dims, tuple(float(mid[a] - (dims[a] - 1) * spc[a] / 2) for a in range(3)), tuple(spc)


def _lattice_axes(dims, origin, spacing):
    """fp32 coordinates per axis: ``origin + i * spacing``, each operation rounded to fp32 (the vertices of ``marching_cubes``)."""
    return [(F32(origin[a]) + np.arange(dims[a], dtype=F32) * F32(spacing[a])).astype(F32) for a in range(3)]


def _mesh_is_closed(verts, faces):
    try:
        info = MeshAdjacency(verts, faces).info
    except ValueError:
        return False
    return int(info['boundary_edges']) == 0 and int(info['nonmanifold_edges']) == 0


def mesh_to_volume(verts, faces, resolution, origin=None, spacing=None, padding=2, sign='auto', threshold=0.5, winding='exact', beta=2.0,
                   search='grid'):
    """A triangle mesh as a signed distance lattice: ``{'sdf' float32 [nx,ny,nz] (negative inside), 'inside' bool [nx,ny,nz],
    'origin', 'spacing', 'info'}``.  The lattice is that of ``marching_cubes``: point (i, j, k) at ``origin + index * spacing`` in fp32,
    volumes indexed [i, j, k] with z fastest, so ``marching_cubes(-sdf, 0, origin, spacing)`` remeshes the surface.  With ``origin``
    and ``spacing`` None the lattice is fitted to the box of the finite vertices: an int ``resolution`` gives cubic cells with
    ``resolution`` points along the longest axis, the box enlarged by ``padding`` cells on every side; a triple gives that many points
    per axis, each axis with its own spacing.

    The magnitude is ``closest_point`` at every lattice point.  The sign is the winding number against ``threshold``:

    - ``sign='winding'`` evaluates it at every lattice point: exact for any soup, robust for open meshes, N F pairs;
    - ``sign='regions'``, for closed meshes: with h the largest spacing and ``tau = h / 2 + 64 eps32 extent`` (the slack of the
      closest-point search), two 6-neighbours that are both farther than tau from the mesh have no surface between them, so the
      winding number is constant on each 6-connected component of ``{dist > tau}`` (``components``).  It is evaluated once per
      component, at its smallest-index point, and at every point of the band ``{dist <= tau}``;
    - ``sign='auto'``: ``'regions'`` when ``MeshAdjacency(...).info`` has no boundary and no non-manifold edge, else ``'winding'``.
      (The test is on edges, not on orientation: the faces of a closed mesh must be wound consistently.)

    ``winding='tree'`` evaluates every one of those winding numbers (the band, the regions, ``sign='winding'``) through a
    ``WindingTree`` with ``beta`` (``winding_number(method='tree')``) instead of the exact sum.  ``search='tree'`` takes the magnitude
    through ``closest_point(search='tree')``: the same bits, no uniform grid, and with ``winding='tree'`` one tree for both.

    ``info``: ``{'mode', 'regions', 'band', 'evaluations', 'winding'}``: the mode taken, the number of components, the points of the
    band, the number of winding-number evaluations and how they were made.  Device tensors run on the kernels; CPU tensors and NumPy
    arrays take the restatements."""
    _mesh_args(verts, faces)
    if sign not in _SIGN_MODES:
        raise ValueError(f'sign must be one of {_SIGN_MODES}, got {sign!r}')
    _winding_method(winding, 'winding')
    _closest_search(search)
    if winding == 'tree':
        _winding_beta(beta)
    on_dev = _is_device(verts)
    box = _finite_box(verts)
    dims, org, spc = _volume_lattice(box, resolution, origin, spacing, padding)
    n = dims[0] * dims[1] * dims[2]
    if n >= 1 << 31:
        raise ValueError(f'a lattice of {dims} has 2^31 points or more')
    axes = _lattice_axes(dims, org, spc)
    mode = sign if sign != 'auto' else ('regions' if _mesh_is_closed(verts, faces) else 'winding')
    extent = max([float(np.abs(ax).max()) for ax in axes] + ([float(np.abs(box[0]).max()), float(np.abs(box[1]).max())] if box else []))
    tau = float(F32(max(spc) / 2 + 64 * EPS32 * extent))
    if on_dev:
        dev = verts.device
        grid = TriangleGrid(verts, faces, build=search != 'tree')
        pts = torch.stack(torch.meshgrid(*[torch.from_numpy(ax).to(dev) for ax in axes], indexing='ij'), -1).reshape(-1, 3).contiguous()
        finder = WindingTree.from_grid(grid) if search == 'tree' or winding == 'tree' else None
        dist = (finder if search == 'tree' else grid).closest(pts)['dist']
        tree = finder if winding == 'tree' else None

        def wind(idx):
            sel = pts if idx is None else pts[idx]
            return (tree.query(sel, beta) if tree is not None else _winding_device(sel, None, None, grid)) >= threshold
    else:
        grid = None
        v_np, f_np = _np(verts), _np(faces)
        pts = np.ascontiguousarray(np.stack(np.meshgrid(*axes, indexing='ij'), -1).reshape(-1, 3))
        finder = WindingTree(v_np, f_np) if search == 'tree' or winding == 'tree' else None
        dist = (_closest_tree_numpy(pts, finder) if search == 'tree' else _closest_numpy(pts, v_np, f_np))[0].astype(F32)
        tree = finder if winding == 'tree' else None

        def wind(idx):
            sel = pts if idx is None else pts[idx]
            return (tree.query(sel, beta) if tree is not None else _winding_numpy(sel, v_np, f_np)[0]) >= threshold
    info = {'mode': mode, 'regions': 0, 'band': n, 'evaluations': n, 'winding': winding}
    if mode == 'winding':
        neg = wind(None)
    else:
        labels, stats = components(dist.reshape(dims), tau, connectivity=6)
        k = int(stats.shape[0])
        lab = labels.reshape(-1)
        if on_dev:
            band = torch.nonzero(lab == 0).reshape(-1)
            idx = torch.cat([stats[:, 1].long(), band])
            flag = wind(idx)
            neg = torch.cat([torch.zeros(1, dtype=torch.bool, device=dev), flag[:k]])[lab.long()]
            neg[band] = flag[k:]
        else:
            lab, st = _np(lab), _np(stats)
            band = np.flatnonzero(lab == 0)
            idx = np.concatenate([st[:, 1].astype(np.int64), band])
            flag = wind(idx)
            neg = np.concatenate([[False], flag[:k]])[lab]
            neg[band] = flag[k:]
        info.update(regions=k, band=int(band.shape[0]), evaluations=int(idx.shape[0]))
    if on_dev:
        sdf = torch.where(neg, -dist, dist).reshape(dims)
        neg = neg.reshape(dims)
    else:
        sdf = _as_out(np.where(neg, -dist, dist).reshape(dims), verts)
        neg = _as_out(neg.reshape(dims), verts, bool)
    return {'sdf': sdf, 'inside': neg, 'origin': org, 'spacing': spc, 'info': info}


def volume_iou(verts_a, faces_a, verts_b, faces_b, resolution=128, **kwargs):
    """Volumetric intersection over union of two meshes: both go through ``mesh_to_volume`` (``kwargs``: its arguments) on ONE lattice
    over the box of the finite vertices of both (or on the ``origin`` / ``spacing`` given).  Returns ``{'iou', 'intersection', 'union',
    'volume_a', 'volume_b'}``: numbers of inside lattice points times the cell volume, ``iou = intersection / union`` (NaN when both
    are empty), plus ``'resolution'`` (points per axis), ``'spacing'`` and ``'origin'``."""
    _mesh_args(verts_a, faces_a)
    _mesh_args(verts_b, faces_b)
    if _is_device(verts_a) != _is_device(verts_b):
        raise ValueError('volume_iou: both meshes must be on the device or both on the host')
    kwargs = dict(kwargs)
    dims, org, spc = _volume_lattice(_finite_box(verts_a, verts_b), resolution, kwargs.pop('origin', None), kwargs.pop('spacing', None),
                                     kwargs.get('padding', 2))
    ia = mesh_to_volume(verts_a, faces_a, dims, origin=org, spacing=spc, **kwargs)['inside']
    ib = mesh_to_volume(verts_b, faces_b, dims, origin=org, spacing=spc, **kwargs)['inside']
    cell = float(spc[0]) * float(spc[1]) * float(spc[2])
    both, either, na, nb = (int(x.sum()) for x in (ia & ib, ia | ib, ia, ib))
    return {'iou': both / either if either else float('nan'), 'intersection': both * cell, 'union': either * cell, 'volume_a': na * cell,
            'volume_b': nb * cell, 'resolution': list(dims), 'spacing': list(spc), 'origin': list(org)}


# ------------------------------------------------------------------ simplification

_NO_CELL = np.iinfo(np.int64).max
_JACOBI_SWEEPS = 8


def _simplify_plan(lo, hi, cells=None, cell_size=None):
    """Host arithmetic of ia_simplify_plan: (dims, inv_cell float32 [3], cell float64 [3]) from the box of the finite vertices."""
    ext = [float(hi[a]) - float(lo[a]) for a in range(3)]
    longest = max(ext)
    dims, inv, cell = [], [], []
    for a in range(3):
        if cells is not None and not np.isscalar(cells):
            n = int(cells[a])
            h = ext[a] / n if ext[a] > 0 else 1.0
        else:
            h = float(cell_size) if cells is None else (longest / int(cells) if longest > 0 else 1.0)
            n = max(1, int(np.ceil(ext[a] / h)))
            if cells is not None and longest > 0 and ext[a] == longest:
                n = int(cells)
        if n > 1 << 20:
            raise ValueError(f'more than 2^20 cells along axis {a}')
        i = F32(1.0 / h)
        if not (np.isfinite(i) and i > 0):
            raise ValueError(f'the cell size {h} has no float32 inverse')
        dims.append(n), inv.append(i), cell.append(h)
    return tuple(dims), np.asarray(inv, dtype=F32), np.asarray(cell, dtype=np.float64)


def _simplify_keys_numpy(v32, lo, inv, dims):
    """Linear cell index (x slowest, z fastest) per vertex in int64, ``_NO_CELL`` for a vertex with a non-finite coordinate; the cell
    per axis is the fp32 ``clamp(floor((x - lo) * inv), 0, n - 1)`` of TriangleGrid."""
    fin = np.isfinite(v32).all(1)
    c = []
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(3):
            t = np.floor((np.where(fin, v32[:, a], F32(0)) - F32(lo[a])) * F32(inv[a]))
            c.append(np.minimum(np.maximum(t, F32(0)), F32(dims[a] - 1)).astype(np.int64))
    return np.where(fin, (c[0] * dims[1] + c[1]) * dims[2] + c[2], _NO_CELL)


def _simplify_topology_numpy(keys, faces):
    """The integer part of the definition from per-vertex keys: clusters in ascending key order, usable and surviving faces, the
    referenced clusters and their output indices, the rotated, unique, sorted output faces."""
    valid = keys != _NO_CELL
    ckey, inverse = np.unique(keys[valid], return_inverse=True)
    k = ckey.size
    vcl = np.full(keys.shape[0], -1, dtype=np.int64)
    vcl[valid] = inverse
    c = vcl[faces]                                                       # [F,3]
    usable = (c >= 0).all(1)
    surv = usable & (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])
    ref = np.zeros(k, dtype=bool)
    ref[c[surv].reshape(-1)] = True
    outidx = np.cumsum(ref) - 1
    t = c[surv]
    first = np.argmin(t, axis=1)[:, None]
    t = np.take_along_axis(t, (first + np.arange(3)[None]) % 3, axis=1)  # smallest first, orientation kept
    t = np.unique(t, axis=0) if t.shape[0] else t.reshape(0, 3)          # unique rows, lexicographically increasing
    return {'K': k, 'ckey': ckey, 'vcl': vcl, 'c': c, 'usable': usable, 'n_usable': int(usable.sum()), 'ref': ref, 'outidx': outidx,
            'tri': t, 'faces': outidx[t].astype(np.int64).reshape(-1, 3),
            'vertex_map': np.where((vcl >= 0) & ref[np.maximum(vcl, 0)] if k else np.zeros(vcl.shape, bool), outidx[np.maximum(vcl, 0)] if k else -1, -1).astype(np.int64),
            'cluster_size': np.bincount(vcl[valid], minlength=k)[ref].astype(np.int64)}


def _cluster_sums(idx, rows, k):
    """Per cluster the float64 sums of ``rows`` [n,C] over the entries with cluster ``idx``, each added in index order."""
    return np.stack([np.bincount(idx, weights=rows[:, j], minlength=k) for j in range(rows.shape[1])], -1) if rows.shape[1] else np.zeros((k, 0))


def _cell_centres(ckey, lo, cell, dims):
    ijk = np.stack([ckey // (dims[2] * dims[1]), (ckey // dims[2]) % dims[1], ckey % dims[2]], -1).astype(np.float64)
    return np.asarray(lo, dtype=F32).astype(np.float64)[None] + (ijk + 0.5) * cell[None]


def _quadric_sums_numpy(v64, faces, top, lo, cell, dims):
    """float64 [K,9]: n n^T (xx xy xz yy yz zz) and -n (n . (A - centre)) of every usable face, added once to each distinct cluster among
    its corners (in the order face, corner); n: the cross product of the two shorter edges (as ``point_triangle``), centre: the centre
    of the cluster's cell."""
    f = faces[top['usable']]
    c = top['c'][top['usable']]
    A, B, C = v64[f[:, 0]], v64[f[:, 1]], v64[f[:, 2]]
    eab, ebc, eca = B - A, C - B, A - C
    lab, lbc, lca = _dot3(eab, eab), _dot3(ebc, ebc), _dot3(eca, eca)
    ab_longest, bc_longest = (lab >= lbc) & (lab >= lca), lbc >= lca
    n = np.where(ab_longest[:, None], _cross3(ebc, eca), np.where(bc_longest[:, None], _cross3(eca, eab), _cross3(eab, ebc)))
    take = np.stack([np.ones(len(f), bool), c[:, 1] != c[:, 0], (c[:, 2] != c[:, 0]) & (c[:, 2] != c[:, 1])], -1)       # [U,3]
    fi, ji = np.nonzero(take)                                           # in the order (face, corner)
    cl = c[fi, ji]
    nn = n[fi]
    d = _dot3(nn, A[fi] - _cell_centres(top['ckey'][cl], lo, cell, dims))
    rows = np.stack([nn[:, 0] * nn[:, 0], nn[:, 0] * nn[:, 1], nn[:, 0] * nn[:, 2], nn[:, 1] * nn[:, 1], nn[:, 1] * nn[:, 2],
                     nn[:, 2] * nn[:, 2], -(nn[:, 0] * d), -(nn[:, 1] * d), -(nn[:, 2] * d)], -1)
    return _cluster_sums(cl, rows, top['K'])


def _quadric_place_numpy(q, m, cell):
    """csrc/simplify.hip place_kernel line by line (float64): q [n,9] summed quadrics, m [n,3] cluster means, both relative to the cell
    centre -> the representative relative to the centre.  Cyclic Jacobi with ``_JACOBI_SWEEPS`` fixed sweeps over (0,1), (0,2), (1,2);
    ``x = m + sum_j v_j (v_j . r) / lambda_j`` over the eigenvalues ``> 1e-3 lambda_max``, ``r = -b - A m``; clamped to the cell."""
    n = q.shape[0]
    a = np.zeros((n, 3, 3))
    a[:, 0, 0], a[:, 0, 1], a[:, 0, 2], a[:, 1, 1], a[:, 1, 2], a[:, 2, 2] = (q[:, j] for j in range(6))
    a[:, 1, 0], a[:, 2, 0], a[:, 2, 1] = a[:, 0, 1], a[:, 0, 2], a[:, 1, 2]
    zero = (q[:, :6] == 0).all(1)
    with np.errstate(all='ignore'):
        r = np.stack([-q[:, 6 + i] - ((a[:, i, 0] * m[:, 0] + a[:, i, 1] * m[:, 1]) + a[:, i, 2] * m[:, 2]) for i in range(3)], -1)
        v = np.tile(np.eye(3), (n, 1, 1))
        for _ in range(_JACOBI_SWEEPS):
            for p, qq in ((0, 1), (0, 2), (1, 2)):
                rr = 3 - p - qq
                apq = a[:, p, qq].copy()
                on = apq != 0
                theta = (a[:, qq, qq] - a[:, p, p]) / (2.0 * np.where(on, apq, 1.0))
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                c, s, t = np.where(on, c, 1.0), np.where(on, s, 0.0), np.where(on, t, 0.0)
                a[:, p, p] = np.where(on, a[:, p, p] - t * apq, a[:, p, p])
                a[:, qq, qq] = np.where(on, a[:, qq, qq] + t * apq, a[:, qq, qq])
                a[:, p, qq] = a[:, qq, p] = np.where(on, 0.0, apq)
                arp, arq = a[:, rr, p].copy(), a[:, rr, qq].copy()
                a[:, rr, p] = a[:, p, rr] = np.where(on, c * arp - s * arq, arp)
                a[:, rr, qq] = a[:, qq, rr] = np.where(on, s * arp + c * arq, arq)
                vp, vq = v[:, :, p].copy(), v[:, :, qq].copy()
                v[:, :, p] = np.where(on[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                v[:, :, qq] = np.where(on[:, None], s[:, None] * vp + c[:, None] * vq, vq)
        lam = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], -1)
        lmax = lam.max(1)
        x = m.copy()
        for j in range(3):
            use = ~zero & (lmax > 0) & (lam[:, j] > 1e-3 * lmax)
            w = ((v[:, 0, j] * r[:, 0] + v[:, 1, j] * r[:, 1]) + v[:, 2, j] * r[:, 2]) / np.where(use, lam[:, j], 1.0)
            x = np.where(use[:, None], x + v[:, :, j] * w[:, None], x)
        half = 0.5 * cell[None]
        return np.where(np.isnan(x), m, np.minimum(np.maximum(x, -half), half))


def _cast_extra(mean, like):
    dt = like.dtype
    if isinstance(mean, torch.Tensor):
        return (mean.round() if not dt.is_floating_point else mean).to(dt)
    return (np.rint(mean) if not np.issubdtype(dt, np.floating) else mean).astype(dt)


def _simplify_numpy(verts, faces, grid, placement='quadric', extras=(), as64=False):
    """The definition of ``simplify_mesh`` on NumPy arrays, float64.  ``grid``: (dims, lo, inv_cell, cell) or None for the identity
    clustering (every vertex with finite coordinates is a cluster of its own, in index order).  ``as64`` returns the positions before they are
    rounded to float32 (the tests take the definition's own sensitivity to the order of summation from two such runs)."""
    v32 = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv = v32.shape[0]
    if grid is None:
        keys = np.where(np.isfinite(v32).all(1), np.arange(nv, dtype=np.int64), _NO_CELL)
    else:
        dims, lo, inv, cell = grid
        keys = _simplify_keys_numpy(v32, lo, inv, dims)
    top = _simplify_topology_numpy(keys, f)
    k, ref = top['K'], top['ref']
    valid = np.flatnonzero(top['vcl'] >= 0)
    idx = top['vcl'][valid]
    cnt = np.bincount(idx, minlength=k).astype(np.float64)[ref]
    v64 = v32.astype(np.float64)
    mean = _cluster_sums(idx, v64[valid], k)[ref] / cnt[:, None]
    if grid is None or placement == 'mean' or not ref.any():
        pos = mean
    else:
        cc = _cell_centres(top['ckey'][ref], lo, cell, dims)
        q = _quadric_sums_numpy(v64, f, top, lo, cell, dims)[ref]
        pos = cc + _quadric_place_numpy(q, mean - cc, cell)
    out_extras = []
    for e in extras:
        e = np.asarray(e)
        rows = e.reshape(nv, -1).astype(np.float64)
        out_extras.append(_cast_extra((_cluster_sums(idx, rows[valid], k)[ref] / cnt[:, None]).reshape((-1,) + e.shape[1:]), e))
    return {'verts': pos if as64 else pos.astype(F32), 'faces': top['faces'], 'vertex_map': top['vertex_map'], 'cluster_size': top['cluster_size'],
            'extras': out_extras, 'usable_faces': top['n_usable']}


def _simplify_count_numpy(v32, f, grid):
    dims, lo, inv, cell = grid
    return _simplify_topology_numpy(_simplify_keys_numpy(v32, lo, inv, dims), f)['faces'].shape[0]


def _simplify_device(verts, faces32, grid, placement, extras, count_only=False):
    """The device route of ``simplify_mesh``: every step is a kernel of csrc/simplify.hip except the three sorts of integer keys
    (``torch.sort``: vertex keys, face keys, (cluster, face) pairs)."""
    from . import hipops
    nv = verts.shape[0]
    if grid is None:
        fin = torch.isfinite(verts).all(1)
        keys = torch.where(fin, torch.arange(nv, device=verts.device), torch.full_like(fin, _NO_CELL, dtype=torch.int64))
    else:
        dims, lo, inv, cell = grid
        keys = hipops.simplify_keys(verts, lo, inv, dims)
    quadric = grid is not None and placement == 'quadric'
    s = hipops.simplify_topology(keys, faces32, full=not count_only, pairs=quadric and not count_only)
    if count_only:
        return s
    faces_out, vertex_map, csize, ocl = hipops.simplify_outputs(s)
    cols = [verts.double()] + [torch.as_tensor(e).to(verts.device).reshape(nv, -1).double() for e in extras]
    sums = hipops.simplify_vertex_sums(s, torch.cat(cols, 1).contiguous())
    if grid is None:
        pos = hipops.simplify_means(s, ocl, sums[:, :3].contiguous()).float()             # clusters of one vertex: the vertex itself
    else:
        qsum = hipops.simplify_quadric_sums(s, verts, lo, inv, cell, dims) if quadric else None
        pos = hipops.simplify_place(s, ocl, sums[:, :3].contiguous(), qsum, lo, inv, cell, dims)
    out_extras, c0 = [], 3
    for e in extras:
        e = torch.as_tensor(e)
        c = cols[len(out_extras) + 1].shape[1]
        mean = hipops.simplify_means(s, ocl, sums[:, c0:c0 + c].contiguous()) if c else torch.zeros(ocl.numel(), 0, dtype=torch.float64, device=verts.device)
        out_extras.append(_cast_extra(mean.reshape((-1,) + tuple(e.shape[1:])), e))
        c0 += c
    return {'verts': pos, 'faces': faces_out, 'vertex_map': vertex_map, 'cluster_size': csize, 'extras': out_extras, 'usable_faces': s['usable']}


def simplify_mesh(verts, faces, cells=None, cell_size=None, target_faces=None, placement='quadric', extras=(), max_cells=4096):
    """Simplify a triangle mesh (verts float32 [V,3], faces int64 [F,3]) by quadric vertex clustering on a uniform grid: all vertices
    of a grid cell become one vertex.  Returns a dict: 'verts' float32 [V',3], 'faces' int64 [F',3], 'vertex_map' int64 [V],
    'cluster_size' int64 [V'], 'extras' (list), 'dims' (nx, ny, nz), 'cell_size' float, 'lo' (3 floats), 'input_faces' F,
    'usable_faces', and with ``target_faces`` 'steps' (count-only passes).  Exactly one of ``cells``, ``cell_size``, ``target_faces``:

    - ``cells``: an int c = cubic cells of edge ``h = longest / c``, c of them along the longest axis of the box of the finite vertices
      and ``max(1, ceil(extent / h))`` along the others; or a triple = cells per axis (edge ``extent / n`` per axis).
    - ``cell_size``: the edge h of cubic cells, ``max(1, ceil(extent / h))`` per axis.
    - ``target_faces = n``: if the mesh has at most n usable faces it is returned through the identity clustering (every vertex with
      finite coordinates is its own cluster, numbered in input order; no grid is run, 'dims' is None and 'cell_size' 0: a plain
      renumbering that drops unusable and degenerate faces, exact duplicates and unreferenced vertices).  Otherwise the int ``cells``
      is bisected in [1, ``max_cells``] with a count-only pass (no positions): the result has ``c`` with ``F'(c) <= n`` and either
      ``F'(c + 1) > n`` or ``c == max_cells``.  F' need not grow monotonically with c; that adjacent pair, not "closest to n", is the
      contract.

    The definition:

    1. Cells.  ``lo`` and the extents are those of the vertices with three finite coordinates.  The cell of a vertex is, per axis and
       in fp32, ``clamp(floor((x - lo) * inv), 0, n - 1)`` with ``inv = fp32(1 / h)`` (the function of ``TriangleGrid``); its linear index
       ``(ix * ny + iy) * nz + iz`` (x slowest, z fastest).  A vertex with a non-finite coordinate has no cell.  A cluster is the set
       of vertices of one cell.
    2. A face is usable if its three vertices have cells, and survives if they lie in three different cells.  Indices outside [0, V)
       raise ``ValueError``, as in ``mesh_components`` and ``closest_point``.
    3. One output vertex per cell that a surviving face references (none is unreferenced), numbered by ascending linear cell index.
       ``vertex_map[v]``: the output vertex of input vertex v, -1 if v has no cell or its cell is not referenced; ``cluster_size``:
       input vertices per output vertex.
    4. Every surviving face is mapped through ``vertex_map`` and rotated so that its smallest index comes first (orientation kept);
       exact duplicates are removed and the faces sorted lexicographically.  Two faces on the same three vertices with opposite
       orientation are both kept.  ``faces``, ``vertex_map`` and ``cluster_size`` are integer functions of the input that do not depend on
       the order of its vertices and faces.
    5. ``placement='mean'``: the arithmetic mean of the cluster's vertices (float64, rounded to float32).
    6. ``placement='quadric'``: every usable face (surviving or not) adds ``(n n^T, -n (n . (A - c)))`` once to each distinct cluster
       among its corners: n the unnormalised normal from the two shorter edges (as ``point_triangle``; the weight is the squared
       area), A its first vertex, c the centre of the cluster's cell.  With ``A x = -b`` the summed system and m the cluster mean
       relative to c, the representative is ``c + clamp(m + A^+ (-b - A m))``: ``A^+`` the pseudo-inverse from a cyclic Jacobi
       eigen-decomposition (8 fixed sweeps, float64) that drops eigenvalues ``<= 1e-3`` of the largest (Lindstrom, out-of-core
       simplification), so a planar or creased cluster moves from m only along well-determined directions; the clamp is to the
       closed box of the cell, ``[-h/2, h/2]`` about c.  A cluster whose matrix is all zero takes m.
    7. ``extras``: per-vertex arrays [V, ...] are averaged per cluster in float64 and returned in their dtype (integer types rounded
       to nearest); normals are the caller's to renormalise.

    A result without a surviving face (``cells=1``, V = 0, F = 0) is a valid empty mesh.  Vertex clustering can pinch the surface: the
    output need not be manifold even if the input is.  Every point of the output lies within one cell diagonal of the input surface.

    Device tensors run on the kernels of csrc/simplify.hip (sums in double, in an order fixed by the data layout: the same bits from
    run to run); CPU tensors and NumPy arrays take the NumPy restatement of the same definition (float64, positions rounded to
    float32 at the end)."""
    _mesh_args(verts, faces)
    if sum(x is not None for x in (cells, cell_size, target_faces)) != 1:
        raise ValueError('exactly one of cells, cell_size and target_faces must be given')
    if placement not in ('quadric', 'mean'):
        raise ValueError(f"placement must be 'quadric' or 'mean', got {placement!r}")
    max_cells = int(max_cells)
    if not 1 <= max_cells <= 1 << 20:
        raise ValueError(f'max_cells must be in [1, 2^20], got {max_cells}')
    if cells is not None:
        cells = int(cells) if np.isscalar(cells) else tuple(int(c) for c in cells)
        if (np.isscalar(cells) and not 1 <= cells <= 1 << 20) or (not np.isscalar(cells) and (len(cells) != 3 or min(cells) < 1 or max(cells) > 1 << 20)):
            raise ValueError(f'cells must be an int in [1, 2^20] or three of them, got {cells!r}')
    if cell_size is not None and not (np.isfinite(float(cell_size)) and float(cell_size) > 0):
        raise ValueError(f'cell_size must be finite and > 0, got {cell_size!r}')
    if target_faces is not None and int(target_faces) < 1:
        raise ValueError(f'target_faces must be >= 1, got {target_faces!r}')
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    for e in extras:
        if e.shape[0] != nv:
            raise ValueError(f'an extra has {e.shape[0]} rows for {nv} vertices')
    on_dev = isinstance(verts, torch.Tensor) and verts.is_cuda
    if on_dev:
        from . import hipops
        v = verts.detach().float().contiguous()
        if nf and (int(faces.min()) < 0 or int(faces.max()) >= nv):
            raise ValueError(f'faces index vertices outside [0, {nv})')
        f = faces.to(device=v.device, dtype=torch.int32).contiguous()
        box = hipops.simplify_box(v)
        run = lambda grid: _simplify_device(v, f, grid, placement, extras)
        count = lambda grid: _simplify_device(v, f, grid, placement, (), count_only=True)['n_faces']
        usable = lambda: _simplify_device(v, f, None, placement, (), count_only=True)['usable']
    else:
        v, f = np.ascontiguousarray(_np(verts), dtype=F32), _np(faces).astype(np.int64)
        if nf and (f.min() < 0 or f.max() >= nv):
            raise ValueError(f'faces index vertices outside [0, {nv})')
        fin = v[np.isfinite(v).all(1)]
        box = (fin.min(0).tolist(), fin.max(0).tolist()) if fin.shape[0] else None
        np_extras = [_np(e) for e in extras]
        run = lambda grid: _simplify_numpy(v, f, grid, placement, np_extras)
        count = lambda grid: _simplify_count_numpy(v, f, grid)
        usable = lambda: int(np.isfinite(v).all(1)[f].all(1).sum())
    lo, hi = box if box is not None else ([0.0] * 3, [0.0] * 3)

    def plan(c=None, h=None):
        dims, inv, cell = _simplify_plan(lo, hi, c, h)
        return dims, lo, inv, cell
    steps, grid = 0, None
    if target_faces is None:
        grid = plan(cells, cell_size)
    elif usable() > int(target_faces):
        n = int(target_faces)
        steps = 1
        if count(plan(max_cells)) <= n:
            c = max_cells
        else:
            c, above = 1, max_cells                                     # F'(1) = 0 <= n < F'(above)
            while above - c > 1:
                mid = (c + above) // 2
                steps += 1
                if count(plan(mid)) <= n:
                    c = mid
                else:
                    above = mid
        grid = plan(c)
    out = run(grid)
    if not on_dev:
        out = {k: ([_as_out(e, verts, e.dtype) for e in x] if k == 'extras' else _as_out(x, verts, x.dtype) if isinstance(x, np.ndarray) else x)
               for k, x in out.items()}
    out.update(dims=None if grid is None else tuple(int(d) for d in grid[0]), cell_size=0.0 if grid is None else float(max(grid[3])),
               cell=None if grid is None else tuple(float(h) for h in grid[3]), lo=tuple(float(x) for x in lo), input_faces=nf)
    if target_faces is not None:
        out['steps'] = steps
    return out


# ------------------------------------------------------------------ mesh smoothing and mesh normals

_WEIGHTS = ('uniform', 'cotangent')
_BOUNDARY = ('fixed', 'free')
_NORMAL_WEIGHTING = ('area', 'angle')


def _len3(u):
    return np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])


def _segment_sums(idx, rows, n, dtype=np.float64):
    """Per segment the sums of ``rows`` [m] or [m,C] over the entries with segment ``idx``, each added in entry order, in ``dtype``."""
    rows = np.asarray(rows, dtype=dtype)
    if dtype == np.float64:
        if rows.ndim == 1:
            return np.bincount(idx, weights=rows, minlength=n)
        return np.stack([np.bincount(idx, weights=rows[:, c], minlength=n) for c in range(rows.shape[1])], -1)
    out = np.zeros((n,) + rows.shape[1:], dtype=dtype)
    np.add.at(out, idx, rows)
    return out


def _adjacency_numpy(v32, f):
    """The integer part of the definition of ``MeshAdjacency`` on NumPy arrays (verts float32 [V,3], faces int64 [F,3], indices in
    range): CSR neighbour lists, faces per edge, boundary flags, the vertex -> face incidence and, for the cotangent weights, the
    sorted directed entries (``run``: the CSR slot of every entry, ``ent``: its (i, j, opposite vertex), in face order per slot)."""
    nv, nf = v32.shape[0], f.shape[0]
    fin = np.isfinite(v32).all(1)
    usable = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    if nf:
        usable &= fin[f].all(1)
    uf = np.flatnonzero(usable)
    a, b, c = (f[uf, k] for k in range(3))
    src = np.stack([a, b, b, c, c, a], -1).reshape(-1)
    dst = np.stack([b, a, c, b, a, c], -1).reshape(-1)
    opp = np.stack([c, c, a, a, b, b], -1).reshape(-1)
    order = np.argsort(src * nv + dst, kind='stable')                    # entries of one key stay in face order
    src, dst, opp = src[order], dst[order], opp[order]
    head = np.ones(src.size, dtype=bool)
    head[1:] = (src[1:] != src[:-1]) | (dst[1:] != dst[:-1])
    start = np.flatnonzero(head)
    row, nbr = src[start], dst[start]
    edge_faces = np.diff(np.append(start, src.size))
    deg = np.bincount(row, minlength=nv)
    offsets = np.zeros(nv + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(deg)
    boundary = np.bincount(row, weights=(edge_faces == 1), minlength=nv) > 0
    corner = f[uf].reshape(-1)
    vorder = np.argsort(corner * max(nf, 1) + np.repeat(uf, 3), kind='stable')
    face_offsets = np.zeros(nv + 1, dtype=np.int64)
    face_offsets[1:] = np.cumsum(np.bincount(corner, minlength=nv))
    info = {'edges': int(start.size // 2), 'boundary_edges': int((edge_faces == 1).sum() // 2),
            'nonmanifold_edges': int((edge_faces > 2).sum() // 2), 'boundary_verts': int(boundary.sum()), 'usable_faces': int(uf.size),
            'max_degree': int(deg.max()) if nv else 0}
    return {'offsets': offsets.astype(np.int32), 'neighbors': nbr.astype(np.int32), 'edge_faces': edge_faces.astype(np.int32),
            'boundary': boundary, 'face_offsets': face_offsets.astype(np.int32), 'face_ids': np.repeat(uf, 3)[vorder].astype(np.int32),
            'info': info, 'row': row, 'run': np.cumsum(head) - 1, 'ent': (src, dst, opp), 'finite': fin}


def _cotangent_numpy(v32, adj, dtype=np.float64):
    """float32 [E]: ``max(0, 1/2 sum cot)`` per directed edge, the sum over the usable faces on the edge in face order, in ``dtype``
    (float64 is the definition; the tests take the definition's own sensitivity from a float32 run)."""
    i, j, o = adj['ent']
    p = v32.astype(dtype)
    u, v = p[i] - p[o], p[j] - p[o]
    with np.errstate(all='ignore'):
        ln = _len3(_cross3(u, v))
        ok = np.isfinite(ln) & (ln > 0)
        cot = np.where(ok, _dot3(u, v) / np.where(ok, ln, 1), 0).astype(dtype)
    s = _segment_sums(adj['run'], cot, adj['neighbors'].size, dtype)
    return np.maximum(dtype(0), dtype(0.5) * s).astype(F32)


def _pinned_numpy(adj, w, boundary, fixed):
    deg = np.diff(adj['offsets'].astype(np.int64))
    pinned = ~adj['finite'] | (deg == 0)
    if w is not None:
        pinned |= np.bincount(adj['row'], weights=(w > 0), minlength=deg.size) == 0
    if boundary == 'fixed':
        pinned |= adj['boundary']
    if fixed is not None:
        pinned |= fixed
    return pinned


def _smooth_numpy(v32, adj, w, pinned, factors, round32=True):
    """The steps of the definition of ``smooth_mesh``: float64 [V,3].  ``round32=False`` carries the positions in float64 throughout
    (the tests take the definition's own sensitivity to its rounding points from the two runs)."""
    nv = v32.shape[0]
    p = v32.astype(np.float64)
    move = np.flatnonzero(~pinned)
    if not move.size:
        return p
    nbr = adj['neighbors'].astype(np.int64)
    w64 = np.ones(nbr.size) if w is None else w.astype(np.float64)
    wsum = np.bincount(adj['row'], weights=w64, minlength=nv)[move, None]
    for fac in factors:
        s = _segment_sums(adj['row'], w64[:, None] * p[nbr], nv)[move]
        q = p[move] + float(fac) * (s / wsum - p[move])
        p = p.copy()
        p[move] = q.astype(F32).astype(np.float64) if round32 else q
    return p


def _mesh_normals_numpy(v32, f, adj, weighting, dtype=np.float64):
    nv = v32.shape[0]
    p = v32.astype(dtype)
    fid = adj['face_ids'].astype(np.int64)
    rows = np.repeat(np.arange(nv), np.diff(adj['face_offsets'].astype(np.int64)))
    t = f[fid].reshape(-1, 3)
    n = _cross3(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    with np.errstate(all='ignore'):
        if weighting == 'angle':
            ln = _len3(n)
            ok = np.isfinite(ln) & (ln > 0)
            k = np.argmax(t == rows[:, None], axis=1) if t.size else np.zeros(0, dtype=np.int64)
            ar = np.arange(t.shape[0])
            e1, e2 = p[t[ar, (k + 1) % 3]] - p[rows], p[t[ar, (k + 2) % 3]] - p[rows]
            ang = np.arctan2(ln, _dot3(e1, e2))
            n = np.where(ok[:, None], n / np.where(ok, ln, 1)[:, None] * ang[:, None], 0).astype(dtype)
        s = _segment_sums(rows, n, nv, dtype)
        ln = _len3(s)
        ok = np.isfinite(ln) & (ln > 0)
        return np.where(ok[:, None], s / np.where(ok, ln, 1)[:, None], 0).astype(F32)


def _faces_in_range(faces, nv):
    if faces.shape[0] and (int(faces.min()) < 0 or int(faces.max()) >= nv):
        raise ValueError(f'faces index vertices outside [0, {nv})')


class MeshAdjacency:
    """The neighbourhood structure of one indexed mesh (verts float32 [V,3], faces [F,3]), built once for many calls of ``smooth_mesh``
    and ``mesh_normals`` (as ``TriangleGrid`` is for ``closest_point``).  See ``smooth_mesh`` for the definitions.

    - ``offsets`` int32 [V+1], ``neighbors`` int32 [E]: the distinct neighbours of vertex i, ascending, at ``offsets[i] .. offsets[i+1]``;
    - ``edge_faces`` int32 [E]: usable faces on the edge (duplicates counted); ``boundary`` bool [V];
    - ``face_offsets`` int32 [V+1], ``face_ids`` int32 [3 * usable faces]: the usable faces of vertex i, ascending;
    - ``cotangent()``: float32 [E], computed on first use from the positions the structure was built with;
    - ``info``: 'edges', 'boundary_edges', 'nonmanifold_edges' (undirected), 'boundary_verts', 'usable_faces', 'max_degree'.

    ``offsets``, ``neighbors``, ``edge_faces`` and ``boundary`` do not depend on the order of the faces.  Device tensors are built by the
    kernels of csrc/smooth.hip (the two sorts of integer keys are ``torch.sort``; two host synchronisations), CPU tensors and NumPy
    arrays by the NumPy restatement; the arrays are in the caller's container.  An index outside [0, V) raises ``ValueError``."""

    def __init__(self, verts, faces):
        _mesh_args(verts, faces)
        self.device = isinstance(verts, torch.Tensor) and verts.is_cuda
        self.n_verts, self.n_faces = int(verts.shape[0]), int(faces.shape[0])
        self._cot = None
        if self.device:
            from . import hipops
            self.verts = verts.detach().float().contiguous()
            self.faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
            self._state = hipops.mesh_adjacency(self.verts, self.faces)
            if self._state['out_of_range']:
                raise ValueError(f'faces index vertices outside [0, {self.n_verts})')
            for k in ('offsets', 'neighbors', 'edge_faces', 'boundary', 'face_offsets', 'face_ids', 'info'):
                setattr(self, k, self._state[k])
        else:
            self.verts = np.ascontiguousarray(_np(verts), dtype=F32)
            self.faces = _np(faces).astype(np.int64)
            _faces_in_range(self.faces, self.n_verts)
            self._state = _adjacency_numpy(self.verts, self.faces)
            for k in ('offsets', 'neighbors', 'edge_faces', 'face_offsets', 'face_ids'):
                setattr(self, k, _as_out(self._state[k], verts, np.int32))
            self.boundary = _as_out(self._state['boundary'], verts, bool)
            self.info = self._state['info']

    def cotangent(self):
        if self._cot is None:
            if self.device:
                from . import hipops
                self._cot = hipops.mesh_cotangent(self._state, self.verts, self.faces)
            else:
                self._cot = _cotangent_numpy(self.verts, self._state)
        return self._cot if self.device or not isinstance(self.offsets, torch.Tensor) else torch.from_numpy(self._cot)

    def _check(self, verts, faces):
        if (isinstance(verts, torch.Tensor) and verts.is_cuda) != self.device or verts.shape[0] != self.n_verts or faces.shape[0] != self.n_faces:
            raise ValueError('the adjacency was built for another mesh or on another device')


def smooth_mesh(verts, faces, iterations=10, lam=0.5, mu=-0.53, weights='uniform', boundary='fixed', fixed=None, adjacency=None):
    """Smooth a triangle mesh (verts float32 [V,3], faces [F,3]; the faces are not touched): Taubin's lambda | mu smoothing, which
    removes ripples without shrinking the shape (``mu`` a float: ``iterations`` pairs of a step with ``lam`` and a step with ``mu``), or
    plain Laplacian smoothing (``mu=None``: ``iterations`` steps with ``lam``), which shrinks.  Returns a dict: 'verts' float32 [V,3] in
    the caller's container, 'pinned' bool [V], 'info' (the adjacency's, plus 'steps') and 'adjacency' (a ``MeshAdjacency``, to hand to
    later calls on the same mesh).  The definition:

    1. A face is usable if its three indices are distinct and its three vertices finite; other faces are skipped.  An index outside
       [0, V) raises ``ValueError``.  Every usable face (a, b, c) contributes the directed entries (a,b) (b,a) (b,c) (c,b) (c,a) (a,c);
       the neighbours of i are the distinct j with an entry (i, j), ascending; ``edge_faces(i, j)`` is the number of entries (i, j).  An
       edge with one face is a boundary edge (its ends are boundary vertices), with more than two non-manifold.
    2. ``weights='uniform'``: w_ij = 1.  ``'cotangent'``: w_ij = max(0, 1/2 sum cot theta) over the usable faces on the edge, theta
       the angle opposite the edge at the INPUT positions, cot = dot(u, v) / |cross(u, v)| (0 for a face whose cross product is zero or
       not finite), in double, summed in face order, stored as float32 and fixed for all iterations.
    3. A pinned vertex keeps its input bits: a non-finite vertex, a vertex without neighbours or whose weights are all zero, a boundary
       vertex under ``boundary='fixed'`` (``'free'``: boundary vertices move like any other), and where the bool mask ``fixed`` [V] is set.
    4. One step with factor f moves every other vertex to ``fl32(p_i + f ((sum_j w_ij p_j) / (sum_j w_ij) - p_i))``: the sums in double
       in ascending j, every p_j from the previous step (Jacobi), one rounding to float32 per step and coordinate.

    ``iterations=0`` returns the input bits.  Device tensors run on the kernels of csrc/smooth.hip (no floating-point atomics, the order
    of every sum fixed by the sorted layout: the same bits from run to run; no host synchronisation between the steps); CPU tensors and
    NumPy arrays take the NumPy restatement of the same definition."""
    _mesh_args(verts, faces)
    if weights not in _WEIGHTS:
        raise ValueError(f'weights must be one of {_WEIGHTS}, got {weights!r}')
    if boundary not in _BOUNDARY:
        raise ValueError(f'boundary must be one of {_BOUNDARY}, got {boundary!r}')
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f'iterations must be >= 0, got {iterations}')
    factors = [float(lam)] * iterations if mu is None else [float(lam), float(mu)] * iterations
    if not all(np.isfinite(x) for x in factors):
        raise ValueError(f'lam and mu must be finite, got {lam!r} and {mu!r}')
    nv = int(verts.shape[0])
    if fixed is not None and tuple(fixed.shape) != (nv,):
        raise ValueError(f'fixed must be a bool mask [{nv}], got {tuple(fixed.shape)}')
    adj = MeshAdjacency(verts, faces) if adjacency is None else adjacency
    adj._check(verts, faces)
    info = dict(adj.info, steps=len(factors))
    if adj.device:
        from . import hipops
        v = verts.detach().float().contiguous()
        w = adj.cotangent() if weights == 'cotangent' else None
        fx = None if fixed is None else torch.as_tensor(fixed).to(device=v.device, dtype=torch.bool).contiguous()
        pinned = hipops.smooth_pinned(adj._state, v, w, boundary == 'fixed', fx)
        out = hipops.smooth_steps(adj._state, v, w, pinned, factors)
        return {'verts': out, 'pinned': pinned, 'info': info, 'adjacency': adj}
    v = np.ascontiguousarray(_np(verts), dtype=F32)
    if weights == 'cotangent':
        adj.cotangent()
    w = adj._cot if weights == 'cotangent' else None
    pinned = _pinned_numpy(adj._state, w, boundary, None if fixed is None else _np(fixed).astype(bool))
    out = v.copy()
    move = ~pinned
    out[move] = _smooth_numpy(v, adj._state, w, pinned, factors)[move].astype(F32)
    return {'verts': _as_out(out, verts), 'pinned': _as_out(pinned, verts, bool), 'info': info, 'adjacency': adj}


def mesh_normals(verts, faces, weighting='area', adjacency=None):
    """Unit vertex normals float32 [V,3] from the mesh itself (no volume needed: a smoothed or simplified mesh, or one read with
    ``read_ply``).  Per vertex the sum over its usable faces (see ``smooth_mesh``) in ascending face index of the raw cross product
    ``(B - A) x (C - A)`` (``weighting='area'``) or of the unit face normal times the corner angle at the vertex (``'angle'``; a face
    without area contributes 0), in double, normalised and stored as float32; (0, 0, 0) where the sum has zero or non-finite length.
    Device tensors run on ia_mesh_normals (csrc/smooth.hip), CPU tensors and NumPy arrays on the NumPy restatement."""
    _mesh_args(verts, faces)
    if weighting not in _NORMAL_WEIGHTING:
        raise ValueError(f'weighting must be one of {_NORMAL_WEIGHTING}, got {weighting!r}')
    adj = MeshAdjacency(verts, faces) if adjacency is None else adjacency
    adj._check(verts, faces)
    if adj.device:
        from . import hipops
        return hipops.mesh_normals(adj._state, verts.detach().float().contiguous(), adj.faces, weighting == 'angle')
    v = np.ascontiguousarray(_np(verts), dtype=F32)
    return _as_out(_mesh_normals_numpy(v, adj.faces, adj._state, weighting), verts)


# ------------------------------------------------------------------ non-rigid fitting (csrc/nonrigid.hip)

def _seq_sum(v, reverse=False):
    """The sum of a float64 vector added in index order (``reverse``: from the last entry)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if not v.size:
        return np.float64(0.0)
    return np.cumsum(v[::-1] if reverse else v)[-1]


def _data_term(c, n, share, t):
    """``C_i t_i`` per vertex: ``c t`` (point, ``n`` None) or ``c (n (n . t) + share t)`` (plane)."""
    if n is None:
        return c[:, None] * t
    return c[:, None] * (n * _dot3(n, t)[:, None] + share * t)


def _nonrigid_rhs_numpy(c, t, n, share, beta, land, pinned):
    """``b = C t + B l``: an offset with weight 0 is not read, pinned rows are 0."""
    with np.errstate(all='ignore'):
        b = _data_term(c, n, share, np.where((c != 0)[:, None], t, 0.0))
        if beta is not None:
            use = (beta != 0)[:, None]
            b = np.where(use, b + beta[:, None] * np.where(use, land, 0.0), b)
    return np.where(pinned[:, None], 0.0, b)


def _nonrigid_operator(adj, c, n, share, beta, pinned, a, reverse=False):
    """``x -> (C + a L + B) x`` on float64 [V,3] with the pinned rows taken out; the neighbour sums in ascending j (``reverse``:
    descending, for the restatement's own sensitivity to the order)."""
    nv = c.shape[0]
    row, nbr = adj['row'].astype(np.int64), adj['neighbors'].astype(np.int64)
    if reverse:
        row, nbr = row[::-1], nbr[::-1]
    deg = np.diff(adj['offsets'].astype(np.int64)).astype(np.float64)[:, None]
    bt = np.zeros(nv) if beta is None else beta
    free = ~pinned[:, None]

    def apply(x):
        s = _segment_sums(row, x[nbr], nv) if nbr.size else np.zeros((nv, 3))
        return np.where(free, (_data_term(c, n, share, x) + a * (deg * x - s)) + bt[:, None] * x, 0.0)
    return apply


def _nonrigid_cg_numpy(apply, b, x0, pinned, iterations, tol, reverse=False, trace=None):
    """Plain conjugate gradients with the freeze rule of ``nonrigid_align`` -> (x, steps, |r| / |b|, energy at the start, at the end).
    ``trace`` (a list) receives ``|r|^2 / |b|^2`` before the first step and after every step."""
    def dot(u, v):
        return _seq_sum(_dot3(u, v), reverse)
    x = np.where(pinned[:, None], 0.0, x0)
    ax = apply(x)
    e0 = 0.5 * dot(x, ax) - dot(b, x)
    r = b - ax
    p = r.copy()
    rr, bb, tol2 = dot(r, r), dot(b, b), np.float64(tol) * np.float64(tol)
    steps = 0
    with np.errstate(all='ignore'):
        frozen = not np.isfinite(rr) or not np.isfinite(bb) or bool(rr <= tol2 * bb)
        if trace is not None:
            trace.append(float(rr / bb) if bb > 0 else 0.0)
        for _ in range(iterations):
            if frozen:
                break
            ap = apply(p)
            pap = dot(p, ap)
            alpha = rr / pap
            if not pap > 0 or not np.isfinite(alpha):
                break
            x = x + alpha * p
            r = r - alpha * ap
            rr_new = dot(r, r)
            p = r + (rr_new / rr) * p
            rr = rr_new
            steps += 1
            if trace is not None:
                trace.append(float(rr / bb))
            frozen = not np.isfinite(rr) or bool(rr <= tol2 * bb)
        e1 = 0.5 * dot(x, apply(x)) - dot(b, x)
        res = float(np.sqrt(rr / bb)) if bb > 0 else 0.0
    return x, steps, res, float(e0), float(e1)


def _landmark_rows(landmarks, nv, what='position'):
    """``(index int64 [K], rows float64 [K,3], weight float64 [K])`` of a landmark triple, checked."""
    if not isinstance(landmarks, (tuple, list)) or len(landmarks) != 3:
        raise ValueError(f'landmarks must be (index [K], {what} [K,3], weight), got {type(landmarks).__name__}')
    idx = np.asarray(_np(landmarks[0]))
    if idx.ndim != 1 or idx.dtype.kind not in 'iu':
        raise ValueError(f'the landmark index must be integers [K], got {idx.dtype} {idx.shape}')
    idx = idx.astype(np.int64)
    rows = np.asarray(_np(landmarks[1]), dtype=np.float64)
    if rows.shape != (idx.size, 3):
        raise ValueError(f'the landmark {what} must be [{idx.size},3], got {rows.shape}')
    w = np.asarray(_np(landmarks[2]), dtype=np.float64)
    if w.ndim == 0:
        w = np.full(idx.size, float(w))
    if w.shape != (idx.size,):
        raise ValueError(f'the landmark weight must be a scalar or [{idx.size}], got {w.shape}')
    if idx.size and (idx.min() < 0 or idx.max() >= nv):
        raise ValueError(f'landmark indices outside [0, {nv})')
    if np.unique(idx).size != idx.size:
        raise ValueError('a landmark index appears twice')
    if not (np.isfinite(rows).all() and np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError(f'landmark {what}s and weights must be finite, the weights >= 0')
    return idx, rows, w


def _mask_checked(mask, nv, what):
    if mask is None:
        return None
    if tuple(mask.shape) != (nv,):
        raise ValueError(f'{what} must be a bool mask [{nv}], got {tuple(mask.shape)}')
    return mask


def _cg_args(cg_iterations, cg_tol):
    if int(cg_iterations) < 1:
        raise ValueError(f'cg_iterations must be >= 1, got {cg_iterations}')
    if not (np.isfinite(cg_tol) and float(cg_tol) >= 0):
        raise ValueError(f'cg_tol must be finite and >= 0, got {cg_tol}')
    return int(cg_iterations), float(cg_tol)


def nonrigid_solve(adjacency, weight, target_offset, stiffness, normals=None, point_share=0.1, pinned=None, x0=None, cg_iterations=100,
                   cg_tol=1e-6, landmarks=None):
    """The linear solve of ``nonrigid_align`` on its own: ``(C + a L + B) x = b`` for one displacement per vertex of ``adjacency`` (a
    ``MeshAdjacency``), by ``cg_iterations`` steps of conjugate gradients in float64 from ``x0`` (0 if None).  ``weight`` [V] >= 0 is
    c, ``target_offset`` [V,3] the offsets t the data term pulls to, ``stiffness`` the factor a of the uniform graph Laplacian
    ``(L x)_i = deg_i x_i - sum_j x_j``; ``normals`` [V,3] (unit) selects the plane form ``C_i = c_i (n_i n_i^T + point_share I)``,
    None the point form ``C_i = c_i I``; ``b_i = C_i t_i`` (plus ``w_k l_k`` for ``landmarks = (index [K], offset [K,3], weight)``,
    which add ``w_k I`` to the diagonal).  ``pinned`` [V] (bool) vertices have x = 0 and leave the system.  See ``nonrigid_align`` for
    the freeze rule.  Returns ``{'x' float64 [V,3], 'cg_steps', 'cg_residual' (|r| / |b|), 'energy_start', 'energy_end'}``, the
    energies ``1/2 x.Ax - b.x`` before and after.  A device adjacency runs on ia_nonrigid_solve, the others on the NumPy restatement."""
    nv = adjacency.n_verts
    if tuple(weight.shape) != (nv,) or tuple(target_offset.shape) != (nv, 3):
        raise ValueError(f'weight must be [{nv}] and target_offset [{nv},3], got {tuple(weight.shape)} and {tuple(target_offset.shape)}')
    if normals is not None and tuple(normals.shape) != (nv, 3):
        raise ValueError(f'normals must be [{nv},3], got {tuple(normals.shape)}')
    if x0 is not None and tuple(x0.shape) != (nv, 3):
        raise ValueError(f'x0 must be [{nv},3], got {tuple(x0.shape)}')
    _mask_checked(pinned, nv, 'pinned')
    if not (np.isfinite(stiffness) and float(stiffness) >= 0):
        raise ValueError(f'stiffness must be finite and >= 0, got {stiffness}')
    if normals is not None and not float(point_share) > 0:
        raise ValueError(f'point_share must be > 0 with normals, got {point_share}')
    cg_iterations, cg_tol = _cg_args(cg_iterations, cg_tol)
    lm = None if landmarks is None else _landmark_rows(landmarks, nv, 'offset')
    keys = ('energy_start', 'energy_end', 'cg_steps', 'cg_residual')
    if adjacency.device:
        from . import hipops
        dev = adjacency.verts.device
        f64 = lambda t: None if t is None else torch.as_tensor(t).to(device=dev, dtype=torch.float64).contiguous()      # noqa: E731
        pin = torch.zeros(nv, dtype=torch.bool, device=dev) if pinned is None else torch.as_tensor(pinned).to(device=dev, dtype=torch.bool).contiguous()
        beta = land = None
        if lm is not None:
            beta, land = torch.zeros(nv, dtype=torch.float64, device=dev), torch.zeros(nv, 3, dtype=torch.float64, device=dev)
            beta[torch.as_tensor(lm[0], device=dev)] = f64(lm[2])
            land[torch.as_tensor(lm[0], device=dev)] = f64(lm[1])
        c, n = f64(weight), f64(normals)
        b = hipops.nonrigid_rhs(c, f64(target_offset), pin, n, point_share, beta, land)
        x, out = hipops.nonrigid_solve(adjacency._state, c, b, stiffness, pin, n, point_share, beta, f64(x0), cg_iterations, cg_tol)
        e0, e1, steps, res = out.cpu().tolist()[:4]
        return dict(zip(keys, (e0, e1, int(steps), res)), x=x)
    c = np.asarray(_np(weight), dtype=np.float64)
    n = None if normals is None else np.asarray(_np(normals), dtype=np.float64)
    pin = np.zeros(nv, dtype=bool) if pinned is None else _np(pinned).astype(bool)
    beta = land = None
    if lm is not None:
        beta, land = np.zeros(nv), np.zeros((nv, 3))
        beta[lm[0]], land[lm[0]] = lm[2], lm[1]
    b = _nonrigid_rhs_numpy(c, np.asarray(_np(target_offset), dtype=np.float64), n, float(point_share), beta, land, pin)
    start = np.zeros((nv, 3)) if x0 is None else np.asarray(_np(x0), dtype=np.float64)
    x, steps, res, e0, e1 = _nonrigid_cg_numpy(_nonrigid_operator(adjacency._state, c, n, float(point_share), beta, pin, float(stiffness)), b,
                                               start, pin, cg_iterations, cg_tol)
    return dict(zip(keys, (e0, e1, steps, res)), x=_as_out(x, weight, np.float64))


def _moved_numpy(x, d, pinned):
    """``fl32(x + d)``; the input bits where the vertex is pinned or the displacement is 0."""
    with np.errstate(all='ignore'):
        return np.where(pinned[:, None] | (d == 0), x, (x.astype(np.float64) + d).astype(F32))


def _nonrigid_terms_numpy(x, p, q, dist, face, pinned, thr, metric, fnormals, snormals, normal_cos, share, beta, land):
    """NumPy restatement of ia_nonrigid_terms -> (c [V], n [V,3] or None, b [V,3], sum c |p - q|^2, sum c)."""
    nv = x.shape[0]
    x64, p64, q64 = (np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in (x, p, q))
    d, f = np.asarray(dist).astype(F32).reshape(-1), np.asarray(face).astype(np.int64).reshape(-1)
    plane = metric == 'plane'
    with np.errstate(all='ignore'):
        ok = np.isfinite(d) & (f >= 0) & (d <= F32(thr)) & ~pinned
        nf = np.zeros((nv, 3))
        if plane or normal_cos is not None:
            nrm = np.asarray(fnormals, dtype=F32).reshape(-1, 3)
            ok &= f < nrm.shape[0]
            nf = nrm[np.where(ok, f, 0)].astype(np.float64) if nrm.shape[0] else nf
            ok &= np.isfinite(nf).all(1) & (nf != 0).any(1)
        if normal_cos is not None:
            ns = np.asarray(snormals, dtype=F32).astype(np.float64).reshape(-1, 3)
            ok &= np.isfinite(ns).all(1) & (ns != 0).any(1)
            ok &= _dot3(ns, np.where(ok[:, None], nf, 0.0)) >= float(normal_cos)
        c = ok.astype(np.float64)
        n = np.where(ok[:, None], nf, 0.0) if plane else None
        b = _data_term(c, n, share, np.where(ok[:, None], q64 - x64, 0.0))
        if beta is not None:
            use = ((beta != 0) & ~pinned)[:, None]
            b = np.where(use, b + beta[:, None] * np.where(use, land, 0.0), b)
        e = np.where(ok[:, None], p64 - q64, 0.0)
    return c, n, b, float(_seq_sum(_dot3(e, e))), int(np.count_nonzero(ok))


def _nonrigid_loop(pair, solve, extent, schedule, iterations, tol):
    """The levels and pairings of ``nonrigid_align`` around ``pair() -> (rms, inliers, terms)`` and ``solve(terms, a, level)``."""
    hist, levels = [], []
    for a in schedule:
        lvl = {'stiffness': a, 'pairings': 0, 'cg_steps': [], 'cg_residual': []}
        levels.append(lvl)
        for k in range(iterations):
            rms, _, terms = pair()
            hist.append(rms)
            lvl['pairings'] += 1
            if rms <= EPS32 * extent or (k > 0 and abs(hist[-2] - rms) <= tol * hist[-2]):
                break
            solve(terms, a, lvl)
    rms, n, _ = pair()
    hist.append(rms)
    return hist, levels, n


def _rms(sq, n):
    return float(np.sqrt(max(sq, 0.0) / n)) if n > 0 else 0.0


def _nonrigid_numpy(x, adj, verts, faces, pinned, metric, schedule, iterations, tol, cg_iterations, cg_tol, share, max_dist, trim, normal_cos,
                    beta, land, search='grid', dtype=np.float64):
    """The NumPy restatement of ``nonrigid_align`` (the definition); ``dtype``: the precision of the closest-point search."""
    fin = _finite_rows(verts)
    if not faces.shape[0] or not fin.shape[0]:
        raise ValueError('nonrigid_align: the target mesh is empty')
    extent = float(max(np.abs(fin.min(0).astype(np.float64)).max(), np.abs(fin.max(0).astype(np.float64)).max()))
    normals = face_normals(verts, faces) if metric == 'plane' or normal_cos is not None else None
    tree = WindingTree(verts, faces) if search == 'tree' else None
    state = {'d': np.zeros((x.shape[0], 3))}

    def pair():
        p = _moved_numpy(x, state['d'], pinned)
        dist, face, q = _closest_numpy(p, verts, faces, dtype) if tree is None else _closest_tree_numpy(p, tree, dtype)[:3]
        ns = _mesh_normals_numpy(p, adj.faces, adj._state, 'area') if normal_cos is not None else None
        thr = _trim_threshold_numpy(dist, face, max_dist, trim)
        c, n, b, sq, cnt = _nonrigid_terms_numpy(x, p, q, dist, face, pinned, thr, metric, normals, ns, normal_cos, share, beta, land)
        return _rms(sq, cnt), cnt, (c, n, b)

    def solve(terms, a, lvl):
        c, n, b = terms
        xs, steps, res, _, _ = _nonrigid_cg_numpy(_nonrigid_operator(adj._state, c, n, share, beta, pinned, a), b, state['d'], pinned,
                                                  cg_iterations, cg_tol)
        state['d'] = xs
        lvl['cg_steps'].append(steps)
        lvl['cg_residual'].append(res)
    hist, levels, n = _nonrigid_loop(pair, solve, extent, schedule, iterations, tol)
    return state['d'], hist, levels, n


def _nonrigid_device(x, adj, verts, faces, pinned, metric, schedule, iterations, tol, cg_iterations, cg_tol, share, max_dist, trim, normal_cos,
                     beta, land, grid, search, tree):
    from . import hipops
    if not faces.shape[0] or not verts.shape[0]:
        raise ValueError('nonrigid_align: the target mesh is empty')
    if grid is None:
        grid = TriangleGrid(verts, faces, build=search != 'tree')
    finder = grid if search != 'tree' else (tree if tree is not None else WindingTree.from_grid(grid))
    normals = face_normals(grid.verts, grid.faces).float().contiguous() if metric == 'plane' or normal_cos is not None else None
    base = float('inf') if max_dist is None else float(F32(max_dist))
    state = {'d': torch.zeros(x.shape[0], 3, dtype=torch.float64, device=x.device), 'pending': []}

    def pair():
        p = hipops.nonrigid_apply(x, state['d'], pinned)
        r = finder.closest(p)
        dist, face = r['dist'].contiguous(), r['face'].int().contiguous()
        thr = base
        if trim < 1.0:                                                    # one more host synchronisation, for tau
            d = torch.where(torch.isfinite(dist) & (face >= 0), dist, torch.full_like(dist, float('inf'))).sort().values
            n_fin = torch.isfinite(d).sum()
            k = torch.ceil(trim * n_fin.double()).long().clamp(1, max(d.numel(), 1))
            if d.numel():
                thr = min(base, d[k - 1].item())
        ns = hipops.mesh_normals(adj._state, p, adj.faces) if normal_cos is not None else None
        c, n, b, stats = hipops.nonrigid_terms(x, p, r['point'].contiguous(), dist, face, pinned, thr, metric, normals, ns, normal_cos, share,
                                               beta, land)
        # the one host synchronisation of the pairing: its two sums, and the results of the solves since the last one
        vals = torch.cat([stats] + [out for _, out in state['pending']]).cpu().tolist()
        for i, (lvl, _) in enumerate(state['pending']):
            lvl['cg_steps'].append(int(vals[2 + 5 * i + 2]))
            lvl['cg_residual'].append(vals[2 + 5 * i + 3])
        state['pending'] = []
        return _rms(vals[0], int(vals[1])), int(vals[1]), (c, n if metric == 'plane' else None, b)

    def solve(terms, a, lvl):
        c, n, b = terms
        state['d'], out = hipops.nonrigid_solve(adj._state, c, b, a, pinned, n, share, beta, state['d'], cg_iterations, cg_tol)
        state['pending'].append((lvl, out))
    hist, levels, n = _nonrigid_loop(pair, solve, float(grid.extent), schedule, iterations, tol)
    return state['d'], hist, levels, n


def nonrigid_align(source, verts, faces, metric='point', stiffness=(50.0, 10.0, 2.0, 0.5), iterations=5, tol=1e-4, cg_iterations=100,
                   cg_tol=1e-6, point_share=0.1, max_dist=None, trim=1.0, normal_cos=None, fixed=None, landmarks=None, adjacency=None,
                   grid=None, search='grid', tree=None):
    """Fit a template mesh ``source = (src_verts float32 [V,3], src_faces [Fs,3])`` to the triangle mesh ``(verts, faces)`` without
    changing its topology (non-rigid ICP): one displacement ``d_i`` per template vertex, kept in float64 and starting at 0, pulled to
    the closest points of the target and held together by the uniform graph Laplacian of the template.  Align rigidly first
    (``align_mesh``); this starts where that stops.  The definition: for each stiffness ``a`` of the schedule, in
    order, at most ``iterations`` pairings.  One pairing:

    1. ``p_i = fl32(x_i + d_i)``, always from the original ``x_i`` (the input bits where ``d_i`` is 0);
    2. ``(dist_i, face_i, q_i)``: the closest point of the target (``closest_point``, ``search='grid'|'tree'``: the same bits);
    3. pair i counts (``c_i = 1``, else 0) iff ``dist_i`` is finite and ``face_i >= 0``, ``dist_i <= max_dist`` if given,
       ``dist_i <= tau`` if ``trim < 1`` (``align_mesh``'s tau), the vertex is not pinned, for ``metric='plane'`` the target face has a
       normal, and with ``normal_cos`` the normal of ``p`` on the template's faces (``mesh_normals``, area weighting) and the unit
       normal of the target face, both non-zero, have a dot product ``>= normal_cos``;
    4. ``rms = sqrt(sum c_i |p_i - q_i|^2 / n)`` (0 for n = 0), a float64 sum in vertex order, appended to ``rms_history``;
    5. the level ends when ``rms <= eps32 extent``, and from its second pairing on when ``|rms_prev - rms| <= tol rms_prev``;
    6. otherwise ``(C + a L + B) d' = b`` is solved for the new d: ``(L d)_i = deg_i d_i - sum_j d_j`` over the template's
       ``MeshAdjacency`` (j ascending), ``C_i = c_i I`` (``'point'``) or ``c_i (n_i n_i^T + point_share I)`` (``'plane'``, ``n_i`` the
       unit normal of ``face_i``), ``B_i = w_k I`` at the vertices of ``landmarks = (index [K], position [K,3], weight)`` (a scalar or
       [K]), ``b_i = C_i (q_i - x_i) + B_i (y_i - x_i)``.  Pinned vertices (a non-finite ``x_i``, or the bool mask ``fixed`` [V]) keep
       ``d_i = 0`` and leave the system; a vertex without neighbours is only decoupled.  The solver is plain conjugate gradients in
       float64 from the current d for exactly ``cg_iterations`` steps, every dot product a float64 sum in vertex order; once
       ``|r|^2 <= cg_tol^2 |b|^2``, or ``p.Ap <= 0``, or a scalar is not finite, every later step is a no-op (the freeze rule).

    After the last level one more pairing gives ``rms`` and ``inliers``.  Returns ``{'verts': fl32(x + d) in the caller's container,
    'displacement' float64 [V,3], 'rms', 'rms_history', 'inliers', 'levels': per level {'stiffness', 'pairings', 'cg_steps' (the steps
    taken before each solve froze), 'cg_residual' (|r| / |b| at the end of each solve)}, 'pinned' bool [V], 'adjacency'}``.  A source
    without faces is legal: every vertex goes to its closest point.  Landmarks pull only while some pair counts.  An empty target, an
    empty or non-positive schedule, ``cg_iterations < 1``, ``point_share <= 0`` with the plane metric, a ``fixed`` or landmark array of
    the wrong shape, a landmark index given twice and an ``adjacency`` built for another mesh raise ValueError.

    A device target runs on the kernels of csrc/nonrigid.hip: one ``TriangleGrid`` (``grid``) or ``WindingTree`` (``tree``) for all
    pairings, no host synchronisation inside a solve, one per pairing for the rms (one more for tau when ``trim < 1``), the same bits
    from run to run.  CPU tensors and NumPy arrays take the NumPy restatement, which is the definition."""
    _closest_search(search)
    if metric not in _ALIGN_MIN:
        raise ValueError(f"metric must be 'point' or 'plane', got {metric!r}")
    if not (isinstance(source, (tuple, list)) and len(source) == 2):
        raise ValueError('source must be a (verts, faces) pair')
    sv, sf = source
    _mesh_args(sv, sf)
    _mesh_args(verts, faces)
    nv = int(sv.shape[0])
    schedule = [float(a) for a in (stiffness if np.ndim(stiffness) else [stiffness])]
    if not schedule or not all(np.isfinite(a) and a > 0 for a in schedule):
        raise ValueError(f'stiffness must be a non-empty schedule of positive numbers, got {stiffness!r}')
    cg_iterations, cg_tol = _cg_args(cg_iterations, cg_tol)
    if metric == 'plane' and not float(point_share) > 0:
        raise ValueError(f'point_share must be > 0 with the plane metric, got {point_share}')
    if not 0.0 < float(trim) <= 1.0:
        raise ValueError(f'trim must be in (0, 1], got {trim}')
    if max_dist is not None and not float(max_dist) >= 0:
        raise ValueError(f'max_dist must be >= 0, got {max_dist}')
    if int(iterations) < 0:
        raise ValueError(f'iterations must be >= 0, got {iterations}')
    _mask_checked(fixed, nv, 'fixed')
    lm = None if landmarks is None else _landmark_rows(landmarks, nv)
    if search != 'tree' and tree is not None:
        raise ValueError("tree is used with search='tree' only")
    on_dev = isinstance(verts, torch.Tensor) and verts.is_cuda
    if on_dev:
        sv = torch.as_tensor(sv).detach().to(verts.device).float().contiguous()
        sf = torch.as_tensor(sf).to(verts.device)
    elif isinstance(sv, torch.Tensor) and sv.is_cuda:
        raise ValueError('the source is on a device and the target is not')
    if not faces.shape[0] or not verts.shape[0]:
        raise ValueError('nonrigid_align: the target mesh is empty')
    adj = MeshAdjacency(sv, sf) if adjacency is None else adjacency
    adj._check(sv, sf)
    args = (metric, schedule, int(iterations), float(tol), cg_iterations, cg_tol, float(point_share), max_dist, float(trim),
            None if normal_cos is None else float(normal_cos))
    if on_dev:
        from . import hipops
        dev = verts.device
        pinned = ~torch.isfinite(sv).all(1)
        if fixed is not None:
            pinned = pinned | torch.as_tensor(fixed).to(device=dev, dtype=torch.bool)
        pinned = pinned.contiguous()
        beta = land = None
        if lm is not None:
            at = torch.as_tensor(lm[0], device=dev)
            beta, land = torch.zeros(nv, dtype=torch.float64, device=dev), torch.zeros(nv, 3, dtype=torch.float64, device=dev)
            beta[at] = torch.as_tensor(lm[2], device=dev)
            land[at] = torch.as_tensor(lm[1], device=dev) - sv[at].double()
        d, hist, levels, n = _nonrigid_device(sv, adj, verts, faces, pinned, *args, beta, land, grid, search, tree)
        out = hipops.nonrigid_apply(sv, d, pinned)
        return {'verts': out, 'displacement': d, 'rms': hist[-1], 'rms_history': hist, 'inliers': n, 'levels': levels, 'pinned': pinned,
                'adjacency': adj}
    x = np.ascontiguousarray(_np(sv), dtype=F32)
    tv, tf = np.asarray(_np(verts), dtype=F32), _np(faces).astype(np.int64)
    _faces_in_range(tf, tv.shape[0])
    pinned = ~np.isfinite(x).all(1)
    if fixed is not None:
        pinned = pinned | _np(fixed).astype(bool)
    beta = land = None
    if lm is not None:
        beta, land = np.zeros(nv), np.zeros((nv, 3))
        beta[lm[0]] = lm[2]
        with np.errstate(all='ignore'):
            land[lm[0]] = lm[1] - x[lm[0]].astype(np.float64)
    d, hist, levels, n = _nonrigid_numpy(x, adj, tv, tf, pinned, *args, beta, land, search)
    return {'verts': _as_out(_moved_numpy(x, d, pinned), sv), 'displacement': _as_out(d, sv, np.float64), 'rms': hist[-1], 'rms_history': hist,
            'inliers': n, 'levels': levels, 'pinned': _as_out(pinned, sv, bool), 'adjacency': adj}


def signed_volume(verts, faces):
    """Signed volume of an indexed mesh (positive for a closed outward-wound one), float64 on the host; faces with a non-finite vertex
    count 0."""
    v, f = _np(verts).astype(np.float64), _np(faces).astype(np.int64)
    if not f.shape[0]:
        return 0.0
    a, b, c = (v[f[:, k]] for k in range(3))
    t = _dot3(a, _cross3(b, c))
    return float(t[np.isfinite(t)].sum() / 6)


# ------------------------------------------------------------------ mesh rasteriser

_CULL = ('none', 'back')
RASTER_SUBPIXEL = 256           # snapped screen units per pixel (csrc/mesh_raster.hip: U = rintf(u * 256))
RASTER_MAX_SCREEN = 1 << 20     # a vertex at |u| or |v| >= 2^20 pixels is unusable
RASTER_MAX_CHANNELS = 8
RASTER_OVERSIZE = 256           # default ``oversize_pixels``: a larger clamped box gets a wave of its own on the device
_RASTER_PAIRS = 1 << 21         # face-pixel pairs per NumPy chunk


def _hw(resolution):
    h, w = (int(resolution),) * 2 if np.isscalar(resolution) else (int(r) for r in resolution)
    if h < 1 or w < 1:
        raise ValueError(f'resolution must be >= 1, got {resolution}')
    return h, w


def _camera_numpy(cam32, H, W, dtype):
    """Of float32 labels [N,25], in ``dtype``: rotation [N,3,3], origin [N,3], rows 0 and 1 of K_res [N,6] (row 0 times W, row 1 times H)."""
    c = cam32.astype(dtype)
    m = c[:, :16].reshape(-1, 4, 4)
    return m[:, :3, :3], m[:, :3, 3], np.concatenate([c[:, 16:19] * dtype(W), c[:, 19:22] * dtype(H)], 1)


def _project_numpy(v32, cam32, H, W, near, dtype=F32):
    """The project stage: {'U', 'V'} int64 [N,V] (snapped screen coordinates, always from the float32 run), 'usable' bool [N,V]
    (likewise) and 'z' [N,V] in ``dtype``."""
    def run(T):
        R, o, k = _camera_numpy(cam32, H, W, T)
        d = v32.astype(T)[None] - o[:, None]
        xc = [(R[:, None, 0, a] * d[..., 0] + R[:, None, 1, a] * d[..., 1]) + R[:, None, 2, a] * d[..., 2] for a in range(3)]
        px = (k[:, None, 0] * xc[0] + k[:, None, 1] * xc[1]) + k[:, None, 2] * xc[2]
        py = (k[:, None, 3] * xc[0] + k[:, None, 4] * xc[1]) + k[:, None, 5] * xc[2]
        return px / xc[2], py / xc[2], xc[2]
    with np.errstate(all='ignore'):
        u, v, z = run(F32)
        usable = (np.isfinite(u) & np.isfinite(v) & np.isfinite(z) & ~(z <= F32(near)) & (np.abs(u) < F32(RASTER_MAX_SCREEN))
                  & (np.abs(v) < F32(RASTER_MAX_SCREEN)))
        U = np.where(usable, np.rint(u * F32(RASTER_SUBPIXEL)), F32(0)).astype(np.int64)
        V = np.where(usable, np.rint(v * F32(RASTER_SUBPIXEL)), F32(0)).astype(np.int64)
        if dtype is not F32:
            z = run(dtype)[2]
    return {'U': U, 'V': V, 'z': np.where(usable, z, dtype(0)), 'usable': usable}


def _edge_values_numpy(U3, V3, s, X, Y):
    """int64 edge values [e_0, e_1, e_2] of the points (X, Y) (e_k: the edge from vertex k + 1 to k + 2, times the area's sign ``s``, so
    inside is >= 0 and the sum is |area|) and the coverage under the top-left rule: e_k > 0, or e_k = 0 on an edge with A > 0 or
    (A = 0 and B > 0), A = -s (V_b - V_a), B = s (U_b - U_a), which is where a point moved right by an infinitesimal (and down by a
    smaller one) would be inside."""
    e, cover = [], True
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        ek = s * ((U3[a] - X) * (V3[b] - Y) - (V3[a] - Y) * (U3[b] - X))
        A, B = -s * (V3[b] - V3[a]), s * (U3[b] - U3[a])
        cover = cover & ((ek > 0) | ((ek == 0) & ((A > 0) | ((A == 0) & (B > 0)))))
        e.append(ek)
    return e, cover


def _weights_numpy(e, dtype):
    area = ((e[0] + e[1]) + e[2]).astype(dtype)
    return [ek.astype(dtype) / area for ek in e]


def _raster_faces_numpy(proj, n, faces, H, W, cull='none', dtype=F32):
    """The raster stage for view ``n`` and the faces int64 [F,3]: (cover bool [F,H,W], z [F,H,W] in ``dtype`` (inf where not covered),
    unusable bool [F])."""
    U, V, z, usable = (proj[k][n] for k in ('U', 'V', 'z', 'usable'))
    ok = usable[faces].all(1)
    U3, V3, z3 = ([a[faces[:, k]][:, None, None] for k in range(3)] for a in (U, V, z))
    area = (U3[1] - U3[0]) * (V3[2] - V3[0]) - (V3[1] - V3[0]) * (U3[2] - U3[0])
    draw = ok[:, None, None] & (area != 0) & ((area < 0) | (cull != 'back'))
    X = (np.arange(W, dtype=np.int64) * RASTER_SUBPIXEL)[None, None, :]
    Y = (np.arange(H, dtype=np.int64) * RASTER_SUBPIXEL)[None, :, None]
    e, cover = _edge_values_numpy(U3, V3, np.sign(area), X, Y)
    cover = cover & draw
    with np.errstate(all='ignore'):
        lam = _weights_numpy(e, dtype)
        zp = dtype(1) / ((lam[0] / z3[0] + lam[1] / z3[1]) + lam[2] / z3[2])
    return cover, np.where(cover, zp, dtype(np.inf)), ~ok


def _visibility_numpy(proj, n, faces, H, W, cull, dtype):
    """Per pixel of view ``n`` the least (z, face) over the covering triangles, the order of the packed keys float_bits(z) << 32 | face
    (z >= 0): (z [H,W], face int64 [H,W], -1 on a miss, culled count)."""
    best_z, best_f, culled = np.full((H, W), np.inf, dtype=dtype), np.full((H, W), -1, dtype=np.int64), 0
    chunk = max(1, _RASTER_PAIRS // (H * W))
    for c0 in range(0, faces.shape[0], chunk):
        cover, zc, bad = _raster_faces_numpy(proj, n, faces[c0:c0 + chunk], H, W, cull, dtype)
        culled += int(bad.sum())
        a = zc.argmin(0)                                              # (the first of equal depths: the lower face)
        za = np.take_along_axis(zc, a[None], 0)[0]
        better = np.take_along_axis(cover, a[None], 0)[0] & (za < best_z)
        best_z, best_f = np.where(better, za, best_z), np.where(better, a + c0, best_f)
    return best_z, best_f, culled


def _unit_rows(v, dtype):
    with np.errstate(all='ignore'):
        l = np.sqrt(_dot3(v, v))
        ok = (l > 0) & np.isfinite(l)
        return np.where(ok[..., None], v / np.where(ok, l, dtype(1))[..., None], dtype(0))


def _resolve_numpy(proj, n, z, face, v32, faces, cam32, H, W, normals=None, attributes=None, dtype=F32):
    """The resolve stage for view ``n``: dict of mask, face, bary [H,W,3], depth, normal [H,W,3], attributes [H,W,C] or None."""
    hit = face >= 0
    out = {'mask': hit, 'face': face.astype(np.int32), 'bary': np.zeros((H, W, 3), dtype), 'depth': np.zeros((H, W), dtype),
           'normal': np.zeros((H, W, 3), dtype), 'attributes': None if attributes is None else np.zeros((H, W, attributes.shape[1]), dtype)}
    if not hit.any():
        return out
    idx = faces[np.where(hit, face, 0)]                               # [H,W,3]
    U3, V3, z3 = ([proj[k][n][idx[..., c]] for c in range(3)] for k in ('U', 'V', 'z'))
    area = (U3[1] - U3[0]) * (V3[2] - V3[0]) - (V3[1] - V3[0]) * (U3[2] - U3[0])
    X = (np.arange(W, dtype=np.int64) * RASTER_SUBPIXEL)[None, :]
    Y = (np.arange(H, dtype=np.int64) * RASTER_SUBPIXEL)[:, None]
    e, _ = _edge_values_numpy(U3, V3, np.sign(area), X, Y)
    k = _camera_numpy(cam32, H, W, dtype)[2][n]
    with np.errstate(all='ignore'):
        lam = _weights_numpy(e, dtype)
        b = np.stack([(lam[c] / z3[c]) * z for c in range(3)], -1)
        xs, ys = np.arange(W, dtype=dtype)[None, :] - k[2], np.arange(H, dtype=dtype)[:, None] - k[5]
        det = k[0] * k[4] - k[1] * k[3]
        dx, dy = (k[4] * xs - k[1] * ys) / det, (k[0] * ys - k[3] * xs) / det
        depth = z * np.sqrt((dx * dx + dy * dy) + dtype(1))
        mix = lambda a: (b[..., 0, None] * a[idx[..., 0]] + b[..., 1, None] * a[idx[..., 1]]) + b[..., 2, None] * a[idx[..., 2]]
        if normals is None:
            p = v32.astype(dtype)
            A = p[idx[..., 0]]
            nrm = _cross3(p[idx[..., 1]] - A, p[idx[..., 2]] - A)
        else:
            nrm = mix(normals.astype(dtype))
        out['normal'] = np.where(hit[..., None], _unit_rows(nrm, dtype), dtype(0))
        if attributes is not None:
            out['attributes'] = np.where(hit[..., None], mix(attributes.astype(dtype)), dtype(0))
    out['bary'], out['depth'] = np.where(hit[..., None], b, dtype(0)), np.where(hit, depth, dtype(0))
    return out


def _rasterize_numpy(v32, faces, cam32, H, W, normals, attributes, cull, near, dtype):
    proj = _project_numpy(v32, cam32, H, W, near, dtype)
    views, culled = [], []
    for n in range(cam32.shape[0]):
        z, face, bad = _visibility_numpy(proj, n, faces, H, W, cull, dtype)
        views.append(_resolve_numpy(proj, n, z, face, v32, faces, cam32, H, W, normals, attributes, dtype))
        culled.append(bad)
    out = {k: None if views[0][k] is None else np.stack([v[k] for v in views]) for k in views[0]}
    out['culled'] = np.array(culled, dtype=np.int32)
    return out


def rasterize_mesh(verts, faces, cameras, resolution, normals=None, attributes=None, cull='none', near=1e-6, oversize_pixels=None,
                   dtype=np.float32):
    """Z-buffer rasteriser: the mesh (verts float32 [V,3], faces [F,3]) seen from the cameras [N,25] (cam2world 4x4, K 3x3 normalised,
    the labels of the generator) at ``resolution`` (an int, or (H, W) with row 0 of K scaled by W and row 1 by H).  Returns a dict with
    leading shape [N,H,W]: 'mask' bool, 'face' int32 (-1 on a miss), 'bary' [..., 3] (perspective-correct), 'depth' (the ray parameter of
    the pixel's unit ray, the quantity ``raycast`` returns; 0 on a miss), 'normal' [..., 3] (the unit normal (B - A) x (C - A) of the
    winding, or with ``normals`` [V,3] their normalised barycentric mix; 0 on a miss), 'attributes' [..., C] (the barycentric mix of
    ``attributes`` float [V,C], C <= 8; None without) and 'culled' int32 [N].  Pixel centres are at INTEGER coordinates (column i, row j,
    as in ``RaySampler_zxc``), so an image aligns pixel for pixel with ``raycast`` on that sampler's rays.  The definition:

    1. Project, float32, every operation rounded on its own: d = X - o, xc = R^T d as ``(R_0a d_x + R_1a d_y) + R_2a d_z``,
       p = K_res xc as ``(k0 x + k1 y) + k2 z``, u = p_x / xc_z, v = p_y / xc_z, z = xc_z; U = rint(256 u), V = rint(256 v).  A vertex is
       unusable if u, v or z is not finite, z <= ``near``, or |u| or |v| >= 2^20.  The last row of K must be [0, 0, 1].
    2. A triangle with an unusable vertex is culled and counted in 'culled'; one with zero snapped area is culled; nothing is clipped at
       the near plane (a triangle that crosses it disappears).  ``cull='back'`` draws only triangles that face the camera (negative
       snapped area: x right, y down, outward winding), ``'none'`` both windings.
    3. Pixel (i, j) is the point (256 i, 256 j).  It is covered where the three int64 edge functions, oriented by the area's sign, are
       >= 0, with the top-left rule where one is 0 (``_edge_values_numpy``).  lambda_k = E_k / (E_0 + E_1 + E_2),
       z = 1 / ((lambda_0 / z_0 + lambda_1 / z_1) + lambda_2 / z_2); the pixel goes to the triangle of least (z, face index).
    4. bary_k = (lambda_k / z_k) z; depth = z sqrt((dx dx + dy dy) + 1) with x' = i - k2, y' = j - k5, det = k0 k4 - k1 k3,
       dx = (k4 x' - k1 y') / det, dy = (k0 y' - k3 x') / det; mixes are ``(b_0 a_0 + b_1 a_1) + b_2 a_2``.

    Device tensors run on ia_mesh_project + ia_mesh_raster + ia_mesh_resolve (csrc/mesh_raster.hip: a 64-bit atomicMin of the key
    float_bits(z) << 32 | face, whose result does not depend on the order of evaluation; ``oversize_pixels``: triangles whose clamped
    bounding box holds more pixels are drawn by one wave each, which changes no result) and give the bits of the float32 restatement.
    CPU tensors and NumPy arrays take the NumPy restatement; ``dtype=np.float64`` evaluates its floating-point part (z, the weights,
    depth, normals, mixes) in double on the same snapped integers, and then returns float64 arrays."""
    _mesh_args(verts, faces)
    if cull not in _CULL:
        raise ValueError(f'cull must be one of {_CULL}, got {cull!r}')
    H, W = _hw(resolution)
    near = float(near)
    if not near >= 0:
        raise ValueError(f'near must be >= 0, got {near!r}')
    if cameras.ndim != 2 or cameras.shape[1] != 25 or cameras.shape[0] < 1:
        raise ValueError(f'cameras must be [N,25] with N >= 1, got {tuple(cameras.shape)}')
    nv = int(verts.shape[0])
    for name, a, width in (('normals', normals, 3), ('attributes', attributes, None)):
        if a is not None and (a.ndim != 2 or a.shape[0] != nv or (width and a.shape[1] != width)):
            raise ValueError(f'{name} must be [{nv},{width or "C"}], got {tuple(a.shape)}')
    if attributes is not None and not 1 <= attributes.shape[1] <= RASTER_MAX_CHANNELS:
        raise ValueError(f'attributes must have 1 .. {RASTER_MAX_CHANNELS} channels, got {attributes.shape[1]}')
    oversize = RASTER_OVERSIZE if oversize_pixels is None else int(oversize_pixels)
    if oversize < 0:
        raise ValueError(f'oversize_pixels must be >= 0, got {oversize_pixels}')
    if isinstance(verts, torch.Tensor) and verts.is_cuda:
        from . import hipops
        if dtype not in (np.float32, torch.float32):
            raise ValueError('the device path is float32')
        dev = verts.device
        f32 = lambda t: None if t is None else torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()
        f = torch.as_tensor(faces).to(device=dev, dtype=torch.int32).contiguous()
        _faces_in_range(f, nv)
        return hipops.rasterize_mesh(verts.detach().float().contiguous(), f, f32(cameras), H, W, f32(normals), f32(attributes), cull == 'back',
                                     near, oversize)
    dtype = np.dtype(dtype).type
    if dtype not in (np.float32, np.float64):
        raise ValueError(f'dtype must be float32 or float64, got {dtype}')
    f = _np(faces).astype(np.int64)
    _faces_in_range(f, nv)
    cam32 = np.ascontiguousarray(_np(cameras), dtype=F32)
    if cam32.shape[0] and not (cam32[:, 22:25] == np.array([0, 0, 1], dtype=F32)).all():
        raise ValueError('the last row of K must be [0, 0, 1]')
    as32 = lambda a: None if a is None else np.ascontiguousarray(_np(a), dtype=F32)
    out = _rasterize_numpy(as32(verts), f, cam32, H, W, as32(normals), as32(attributes), cull, near, dtype)
    kinds = {'mask': bool, 'face': np.int32, 'culled': np.int32}
    return {k: None if x is None else _as_out(x, verts, kinds.get(k, dtype)) for k, x in out.items()}


def depth_to_points(depth, cameras, mask=None):
    """World points ``o + t d`` of a ray-parameter depth image [N,1,H,W] or [N,H,W] with H = W (the ``image_depth`` of ``synthesis``,
    the depth of ``render_geometry``, ``render_mesh`` and ``rasterize_mesh``) seen from ``cameras`` [N,25]: float32 [M,3], the pixels
    in (view, row, column) order for which ``mask`` (same shape as depth; default: depth finite and > 0) is set.  The rays are those of
    ``RaySampler_zxc`` (unit directions, pixel centres at integer coordinates).  A point cloud for ``PointTree`` and its callers."""
    from .training_avatar_texture.volumetric_rendering.ray_sampler import RaySampler_zxc
    like = depth
    d = torch.as_tensor(depth).detach().float()
    if d.ndim == 4 and d.shape[1] == 1:
        d = d[:, 0]
    if d.ndim != 3 or d.shape[1] != d.shape[2]:
        raise ValueError(f'depth must be [N,1,H,W] or [N,H,W] with H = W, got {tuple(torch.as_tensor(depth).shape)}')
    cams = torch.as_tensor(cameras).detach().to(d.device).float()
    if cams.ndim != 2 or cams.shape[1] != 25 or cams.shape[0] != d.shape[0]:
        raise ValueError(f'cameras must be [{d.shape[0]},25], got {tuple(cams.shape)}')
    if mask is None:
        m = torch.isfinite(d) & (d > 0)
    else:
        m = torch.as_tensor(mask).to(d.device).bool().reshape(d.shape)
    with torch.no_grad():
        o, dirs = RaySampler_zxc()(cams[:, :16].reshape(-1, 4, 4), cams[:, 16:25].reshape(-1, 3, 3), int(d.shape[1]))
    pts = (o + d.reshape(d.shape[0], -1, 1) * dirs)[m.reshape(d.shape[0], -1)]
    return pts if isinstance(like, torch.Tensor) else pts.cpu().numpy()


# ------------------------------------------------------------------ depth fusion (TSDF)

FUSE_MAX_CHANNELS = 8           # csrc/tsdf.hip kMaxChannels
_FUSE_POINTS = 1 << 19          # lattice points per NumPy chunk
_FUSE_SUMS = ('sum', 'weight', 'color_sum', 'color_weight')


def _depth_box_numpy(depth, cam32, valid):
    """(lo, hi) float64 [3] of the back-projected pixels ``o + t d`` of ``valid`` [N,H,W] (the points of ``depth_to_points``, for any
    H and W: d the unit ray of pixel (i, j), K_res^-1 [i, j, 1] rotated into the world), or None when there is none."""
    N, H, W = depth.shape
    R, o, k = _camera_numpy(cam32, H, W, np.float64)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for n in range(N):
        jj, ii = np.nonzero(valid[n])
        if not jj.size:
            continue
        xs, ys = ii - k[n, 2], jj - k[n, 5]
        det = k[n, 0] * k[n, 4] - k[n, 1] * k[n, 3]
        d = np.stack([(k[n, 4] * xs - k[n, 1] * ys) / det, (k[n, 0] * ys - k[n, 3] * xs) / det, np.ones(xs.shape)], 1)
        d *= (depth[n, jj, ii].astype(np.float64) / np.sqrt(_dot3(d, d)))[:, None]
        pts = o[n] + d @ R[n].T
        pts = pts[np.isfinite(pts).all(1)]
        if pts.shape[0]:
            lo, hi = np.minimum(lo, pts.min(0)), np.maximum(hi, pts.max(0))
    return (lo, hi) if np.isfinite(lo).all() else None


def _fuse_numpy(axes, depth, cam32, tau, near, mask=None, weights=None, colors=None, sums=None, dtype=F32, decisions=None):
    """The definition of ``fuse_depth`` on the lattice of the fp32 ``axes``: (sum [P], weight [P], color_sum [P,C] or None, color_weight
    [P] or None) in ``dtype``, P = nx ny nz with z fastest; every operation is rounded on its own, the views are added in their order.
    ``sums``: such a tuple to go on from.  ``decisions`` (a list): receives (code, pixel), int64 [N,P]: per view the number of the step
    of the definition at which the view was skipped, negated (-1 .. -4; -3 also for an unusable weight), or 0 where it was added, and
    the pixel ``j W + i`` looked up (-1 where step 1 or 2 skipped)."""
    T = dtype
    N, H, W = depth.shape
    R, o, k = _camera_numpy(cam32, H, W, T)
    dims = tuple(a.shape[0] for a in axes)
    P, C = dims[0] * dims[1] * dims[2], 0 if colors is None else colors.shape[1]
    tau, near = T(F32(tau)), T(F32(near))
    dep = depth.astype(T)
    wts = None if weights is None else weights.astype(T)
    cols = None if colors is None else colors.astype(T)
    F, Wt = (np.zeros(P, T), np.zeros(P, T)) if sums is None else (sums[0].astype(T).reshape(P), sums[1].astype(T).reshape(P))
    Cs = CW = None
    if C:
        Cs, CW = (np.zeros((P, C), T), np.zeros(P, T)) if sums is None else (sums[2].astype(T).reshape(P, C), sums[3].astype(T).reshape(P))
    taken = None if decisions is None else (np.zeros((N, P), dtype=np.int64), np.full((N, P), -1, dtype=np.int64))
    with np.errstate(all='ignore'):
        for c0 in range(0, P, _FUSE_POINTS):
            idx = np.arange(c0, min(c0 + _FUSE_POINTS, P))
            X = [axes[0][idx // (dims[1] * dims[2])].astype(T), axes[1][(idx // dims[2]) % dims[1]].astype(T), axes[2][idx % dims[2]].astype(T)]
            f_, w_ = F[idx], Wt[idx]
            if C:
                c_, cw_ = Cs[idx], CW[idx]
            for n in range(N):
                d = [X[a] - o[n, a] for a in range(3)]
                xc = [(R[n, 0, a] * d[0] + R[n, 1, a] * d[1]) + R[n, 2, a] * d[2] for a in range(3)]
                ok1 = np.isfinite(xc[2]) & (xc[2] > near)
                px = (k[n, 0] * xc[0] + k[n, 1] * xc[1]) + k[n, 2] * xc[2]
                py = (k[n, 3] * xc[0] + k[n, 4] * xc[1]) + k[n, 5] * xc[2]
                u, v = px / xc[2], py / xc[2]
                fi, fj = np.rint(u), np.rint(v)
                ok2 = ok1 & np.isfinite(u) & np.isfinite(v) & (fi >= 0) & (fi <= T(W - 1)) & (fj >= 0) & (fj <= T(H - 1))
                ii, jj = np.where(ok2, fi, T(0)).astype(np.int64), np.where(ok2, fj, T(0)).astype(np.int64)
                t = dep[n, jj, ii]
                w = np.ones(idx.shape[0], T) if wts is None else wts[n, jj, ii]
                ok3 = ok2 & np.isfinite(t) & (t > 0) & np.isfinite(w) & (w > 0)
                if mask is not None:
                    ok3 &= mask[n, jj, ii]
                s = t - np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                ok = ok3 & ~(s < -tau)
                f_ = np.where(ok, f_ + np.minimum(s / tau, T(1)) * w, f_)
                w_ = np.where(ok, w_ + w, w_)
                if C:
                    okc = ok & (s <= tau)
                    c_ = np.where(okc[:, None], c_ + cols[n][:, jj, ii].T * w[:, None], c_)
                    cw_ = np.where(okc, cw_ + w, cw_)
                if taken is not None:
                    taken[0][n, idx] = np.where(ok, 0, np.where(ok3, -4, np.where(ok2, -3, np.where(ok1, -2, -1))))
                    taken[1][n, idx] = np.where(ok2, jj * W + ii, -1)
            F[idx], Wt[idx] = f_, w_
            if C:
                Cs[idx], CW[idx] = c_, cw_
    if decisions is not None:
        decisions.append(taken)
    return F, Wt, Cs, CW


def _same_lattice(state, dims, org, spc, tau, channels):
    """Raises unless ``state`` (a result of ``fuse_depth``) lies on this lattice with this truncation and channel count."""
    try:
        same = (tuple(state['sum'].shape) == dims and tuple(state['weight'].shape) == dims
                and tuple(float(F32(x)) for x in state['origin']) == tuple(float(F32(x)) for x in org)
                and tuple(float(F32(x)) for x in state['spacing']) == tuple(float(F32(x)) for x in spc)
                and float(F32(state['truncation'])) == float(F32(tau))
                and (tuple(state['color_sum'].shape) == dims + (channels,) if channels else 'color_sum' not in state))
    except (KeyError, TypeError, AttributeError):
        same = False
    if not same:
        raise ValueError('state must be the result of fuse_depth on the same lattice, with the same truncation and colour channels')


def fuse_depth(depth, cameras, resolution, origin=None, spacing=None, truncation=None, mask=None, weights=None, colors=None, near=1e-6,
               padding=2, state=None, dtype=np.float32):
    """Depth maps with cameras fused into one truncated signed distance (TSDF) lattice.  ``depth`` [N,H,W] or [N,1,H,W] is the ray
    parameter of the pixel's unit ray (the ``image_depth`` of ``synthesis``, the depth of ``raycast``, ``render_geometry``,
    ``render_mesh`` and ``rasterize_mesh``; H and W may differ), ``cameras`` [N,25] the generator's labels (the last row of K must be
    [0, 0, 1]).  Optional, shaped like ``depth``: ``mask`` (bool) and ``weights`` (float32, e.g. the cosine from a normal image);
    ``colors`` [N,C,H,W] float32 with 1 <= C <= 8.

    The lattice is that of ``marching_cubes`` / ``mesh_to_volume``: point (i, j, k) at ``origin + index * spacing`` in fp32
    (``_lattice_axes``), volumes indexed [i, j, k] with z fastest.  With ``origin`` and ``spacing`` None it is fitted
    (``_volume_lattice``, ``padding`` cells on every side) to the box of the back-projected valid pixels, or taken from ``state``.
    ``truncation`` tau > 0 defaults to 3 times the largest spacing.  The definition, per lattice point X and for the
    views n = 0 .. N - 1 in this order, float32 with every operation rounded on its own, ``R, o, k = _camera_numpy(...)``:

    1. d = X - o, xc_a = (R_0a d_x + R_1a d_y) + R_2a d_z; the view is skipped unless xc_z is finite and > ``near``.
    2. u = ((k0 xc_x + k1 xc_y) + k2 xc_z) / xc_z, v likewise with k3 .. k5; i = rint(u), j = rint(v) (ties to even; pixel centres
       at integer coordinates; nearest pixel by design: interpolating depth across a silhouette invents surface).  Skipped unless u and v
       are finite, 0 <= i <= W - 1 and 0 <= j <= H - 1, compared as floats.
    3. t = depth[n,j,i]; skipped unless t is finite and > 0 and the mask is set.  w = weights[n,j,i] or 1; skipped unless w is finite
       and > 0.
    4. s = t - sqrt((d_x d_x + d_y d_y) + d_z d_z); skipped if s < -tau (the point is hidden behind the surface in this view).
    5. sum += min(s / tau, 1) w, weight += w; with colours, and only if s <= tau, color_sum_c += colors[n,c,j,i] w, color_weight += w.

    Returns, in the container of ``depth``: ``{'sum', 'weight', 'tsdf' float32 [nx,ny,nz]`` (tsdf = sum / weight where weight > 0, else
    1: positive in front of the surface, negative behind it, so ``marching_cubes(-tsdf, 0, origin, spacing)`` meshes it; see
    ``fused_mesh``), ``'observed'`` bool (weight > 0), with colours ``'color_sum'`` [nx,ny,nz,C], ``'color_weight'`` and ``'color'`` (the
    quotient, 0 where unweighted), ``'origin'``, ``'spacing'``, ``'truncation'``, ``'info': {'views', 'observed', 'band'}`` (the points
    seen and those with |tsdf| < 1)``}``.  ``state``: the dictionary an earlier call returned on the same lattice; the call goes on from
    its sums, and since the sums run over the views in one order per point, views [0, N) in one call give the bits of [0, k) followed
    by [k, N).  Device tensors run on ia_tsdf_integrate (csrc/tsdf.hip: one thread per lattice point, no atomics) and give the bits of
    the float32 restatement; CPU tensors and NumPy arrays take the restatement, where ``dtype=np.float64`` evaluates everything after
    the float32 camera labels in double and returns float64 sums."""
    on_dev = _is_device(depth)
    dshape = tuple(depth.shape)
    if len(dshape) == 4 and dshape[1] == 1:
        dshape = (dshape[0],) + dshape[2:]
    if len(dshape) != 3 or min(dshape) < 1:
        raise ValueError(f'depth must be [N,H,W] or [N,1,H,W] with N, H, W >= 1, got {tuple(depth.shape)}')
    N, H, W = dshape
    if cameras.ndim != 2 or tuple(cameras.shape) != (N, 25):
        raise ValueError(f'cameras must be [{N},25], got {tuple(cameras.shape)}')
    for name, a in (('mask', mask), ('weights', weights)):
        if a is not None and tuple(a.shape) not in (dshape, (N, 1, H, W)):
            raise ValueError(f'{name} must have the shape of depth, got {tuple(a.shape)}')
    C = 0
    if colors is not None:
        if colors.ndim != 4 or colors.shape[0] != N or tuple(colors.shape[2:]) != (H, W):
            raise ValueError(f'colors must be [{N},C,{H},{W}], got {tuple(colors.shape)}')
        C = int(colors.shape[1])
        if not 1 <= C <= FUSE_MAX_CHANNELS:
            raise ValueError(f'colors must have 1 .. {FUSE_MAX_CHANNELS} channels, got {C}')
    near = float(near)
    if not near >= 0:
        raise ValueError(f'near must be >= 0, got {near!r}')
    dtype = np.dtype(dtype).type if not isinstance(dtype, torch.dtype) else {torch.float32: F32, torch.float64: np.float64}.get(dtype)
    if dtype not in (np.float32, np.float64) or (on_dev and dtype is not np.float32):
        raise ValueError('dtype must be float32 or float64, and float32 on the device')
    cam32 = np.ascontiguousarray(_np(cameras), dtype=F32)
    if not (cam32[:, 22:25] == np.array([0, 0, 1], dtype=F32)).all():
        raise ValueError('the last row of K must be [0, 0, 1]')
    if origin is None and spacing is None and state is not None:
        origin, spacing = state.get('origin'), state.get('spacing')
        truncation = state.get('truncation') if truncation is None else truncation
    box = None
    if origin is None and spacing is None:
        d_np = np.asarray(_np(depth), dtype=F32).reshape(dshape)
        valid = np.isfinite(d_np) & (d_np > 0)
        if mask is not None:
            valid &= _np(mask).astype(bool).reshape(dshape)
        if weights is not None:
            w_np = np.asarray(_np(weights), dtype=F32).reshape(dshape)
            valid &= np.isfinite(w_np) & (w_np > 0)
        box = _depth_box_numpy(d_np, cam32, valid)
        if box is None:
            raise ValueError('fuse_depth: no valid pixel to fit the lattice to; give origin and spacing')
    dims, org, spc = _volume_lattice(box, resolution, origin, spacing, padding)
    if dims[0] * dims[1] * dims[2] >= 1 << 31:
        raise ValueError(f'a lattice of {dims} has 2^31 points or more')
    tau = 3.0 * max(spc) if truncation is None else float(truncation)
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError(f'truncation must be finite and > 0, got {truncation!r}')
    tau = float(F32(tau))
    if state is not None:
        _same_lattice(state, dims, org, spc, tau, C)
    names = _FUSE_SUMS[:4 if C else 2]
    if on_dev:
        from . import hipops
        dev = depth.device
        prep = lambda t, dt, shape: None if t is None else torch.as_tensor(t).detach().to(device=dev, dtype=dt).reshape(shape).contiguous()
        R, o, k = _camera_numpy(cam32, H, W, F32)
        views = torch.from_numpy(np.ascontiguousarray(np.concatenate([R.reshape(N, 9), o, k], 1), dtype=F32)).to(dev)
        prior = None if state is None else {n_: prep(state[n_], torch.float32, tuple(state[n_].shape)) for n_ in names}
        out = hipops.tsdf_integrate(prep(depth, torch.float32, dshape), views, dims, [F32(x) for x in org], [F32(x) for x in spc], tau, near,
                                    prep(mask, torch.bool, dshape), prep(weights, torch.float32, dshape),
                                    prep(colors, torch.float32, (N, C, H, W)), prior)
        out['observed'] = out['weight'] > 0
        if C:
            cw = out['color_weight'][..., None]
            out['color'] = torch.where(cw > 0, out['color_sum'] / torch.where(cw > 0, cw, torch.ones_like(cw)), torch.zeros_like(cw))
        seen, band = int(out['observed'].sum()), int((out['tsdf'].abs() < 1).sum())
    else:
        as_np = lambda a, dt, shape: None if a is None else np.ascontiguousarray(_np(a), dtype=dt).reshape(shape)
        prior = None if state is None else tuple(_np(state[n_]) for n_ in names) + (None,) * (4 - len(names))
        F, Wt, Cs, CW = _fuse_numpy(_lattice_axes(dims, org, spc), as_np(depth, F32, dshape), cam32, tau, near, as_np(mask, bool, dshape),
                                    as_np(weights, F32, dshape), as_np(colors, F32, (N, C, H, W)), prior, dtype)
        with np.errstate(all='ignore'):
            tsdf = np.where(Wt > 0, F / np.where(Wt > 0, Wt, dtype(1)), dtype(1))
            res = {'sum': F.reshape(dims), 'weight': Wt.reshape(dims), 'tsdf': tsdf.reshape(dims)}
            if C:
                res.update(color_sum=Cs.reshape(dims + (C,)), color_weight=CW.reshape(dims),
                           color=np.where(CW[:, None] > 0, Cs / np.where(CW > 0, CW, dtype(1))[:, None], dtype(0)).reshape(dims + (C,)))
        seen, band = int((Wt > 0).sum()), int((np.abs(tsdf) < 1).sum())
        out = {k_: _as_out(x, depth, dtype) for k_, x in res.items()}
        out['observed'] = _as_out(Wt.reshape(dims) > 0, depth, bool)
    out.update(origin=org, spacing=spc, truncation=tau, info={'views': N, 'observed': seen, 'band': band})
    return out


def _compact_mesh(verts, faces, vmask, fmask, extras=()):
    """The faces of ``fmask`` over the vertices of ``vmask`` (tensors on one device): (verts, faces int64 re-indexed, extras), the
    vertices compacted in their old order."""
    new_index = torch.cumsum(vmask, 0) - 1
    return verts[vmask], new_index[faces[fmask].long()].reshape(-1, 3), [e[vmask] for e in extras]


def _fused_filter(verts, faces, fusion, min_weight, with_colors, xp):
    """``fused_mesh`` steps 2 and 4 in float32, every operation rounded on its own, on NumPy arrays (``xp`` numpy: the restatement) or on
    tensors of one device (``xp`` torch): (keep bool [F], vertex colours [V,C] or None)."""
    dims = tuple(int(n) for n in fusion['weight'].shape)
    if xp is torch:                                                      # (constants as tensors: a host scalar divisor becomes a reciprocal)
        const = lambda v: torch.tensor(v, dtype=torch.float32, device=verts.device)
        as_index = lambda c: c.long()
    else:
        const = lambda v: np.array(v, dtype=F32)
        as_index = lambda c: c.astype(np.int64)
    org, spc = const([float(F32(x)) for x in fusion['origin']]), const([float(F32(x)) for x in fusion['spacing']])
    zero, one, three, top = const([0.0]), const([1.0]), const([3.0]), const([float(n - 2) for n in dims])

    def cells(points):
        """Position in cells ``(c - origin) / spacing`` and the cell ``clamp(floor(.), 0, n - 2)`` per axis, both float32 [M,3]."""
        g = (points - org) / spc
        return g, xp.minimum(xp.maximum(xp.floor(g), zero), top)

    def corners(vol, cell):
        """The eight corner values [M,8,...] of the cells int64 [M,3] of a lattice array, x slowest and z fastest."""
        i, j, k = cell[:, 0], cell[:, 1], cell[:, 2]
        return xp.stack([vol[i + a, j + b, k + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)], 1)

    tri = verts[faces.reshape(-1)].reshape(-1, 3, 3)
    centre = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / three
    keep = corners(fusion['weight'] > min_weight, as_index(cells(centre)[1])).all(1)
    if not with_colors:
        return keep, None
    g, cell = cells(verts)
    t = xp.minimum(xp.maximum(g - cell, zero), one)
    s = one - t
    idx = as_index(cell)
    w8 = xp.stack([((t if a else s)[:, 0] * (t if b else s)[:, 1]) * (t if c else s)[:, 2] for a in (0, 1) for b in (0, 1) for c in (0, 1)], 1)
    w8 = xp.where(corners(fusion['color_weight'], idx) > 0, w8, zero)
    col = corners(fusion['color'], idx)                                   # [V,8,C]
    num, den = w8[:, 0, None] * col[:, 0], w8[:, 0]
    for c in range(1, 8):
        num, den = num + w8[:, c, None] * col[:, c], den + w8[:, c]
    seen = den > 0
    return keep, xp.where(seen[:, None], num / xp.where(seen, den, one)[:, None], zero)


def fused_mesh(fusion, min_weight=0.0, with_colors=False):
    """The surface of a ``fuse_depth`` result: ``(verts float32 [V,3], faces int64 [F,3])``, with ``with_colors`` also vertex colours
    [V,C].

    1. ``marching_cubes(-tsdf, 0, origin, spacing)``.
    2. A face is kept only if all eight corners of the cell that holds its centroid have ``weight > min_weight``; the centroid is
       ``((A + B) + C) / 3`` per axis and the cell ``clamp(floor((c - origin) / spacing), 0, n - 2)``, all in float32.  This removes the
       false sheets between seen and never-seen space (unseen points hold tsdf = 1) that a TSDF has behind every surface and at the
       edges of the frustums.
    3. Unused vertices are dropped; the others keep their order and their bits (they are ``marching_cubes``' own).
    4. Vertex colours: the trilinear interpolation of ``'color'`` over the corners with ``color_weight > 0`` of the vertex's cell,
       renormalised (0 where no corner has colour).

    Steps 2 to 4 are PyTorch on the device of a device result and NumPy (the restatement) otherwise; the face filter agrees exactly."""
    tsdf = fusion['tsdf']
    if with_colors and 'color' not in fusion:
        raise ValueError('with_colors needs a fusion with colours')
    min_weight = float(min_weight)
    if _is_device(tsdf):
        verts, faces = marching_cubes(-tsdf.float(), 0.0, fusion['origin'], fusion['spacing'])
        fus = {k: fusion[k].float() for k in ('tsdf', 'weight', 'color', 'color_weight') if k in fusion}
        fus.update(origin=fusion['origin'], spacing=fusion['spacing'])
        keep, cols = _fused_filter(verts, faces, fus, min_weight, with_colors, torch)
        tv, tf = verts, faces
    else:
        fus = {k: np.asarray(_np(fusion[k]), dtype=F32) for k in ('tsdf', 'weight', 'color', 'color_weight') if k in fusion}
        fus.update(origin=fusion['origin'], spacing=fusion['spacing'])
        verts, faces = _mc_numpy(-fus['tsdf'], 0.0, _vec3(fusion['origin']), _vec3(fusion['spacing']))
        keep, cols = _fused_filter(verts, faces, fus, min_weight, with_colors, np)
        tv, tf, keep = torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(keep)
        cols = None if cols is None else torch.from_numpy(np.ascontiguousarray(cols, dtype=F32))
    vmask = torch.zeros(tv.shape[0], dtype=torch.bool, device=tv.device)
    vmask[tf[keep].reshape(-1)] = True
    v, f, extras = _compact_mesh(tv, tf, vmask, keep, [cols] if with_colors else [])
    out = [v, f] + extras
    if not isinstance(tsdf, torch.Tensor):
        out = [o.numpy() for o in out]
    return tuple(out)


# ------------------------------------------------------------------ texture atlas

TEXTURE_MIN_BLOCK = 4
TEXTURE_MAX_CHANNELS = 8        # image channels of ``project_texture``
TEXTURE_DEPTH_TOL = 16.0        # default ``depth_tol`` = this times mesh extent / max(H, W): measured, see ``project_texture``
_TEXTURE_MODES = ('blend', 'best')


class TextureAtlas:
    """The texture layout of a mesh of ``n_faces`` triangles on ``size`` x ``size`` texels; integer arithmetic only, the same on host and
    device (csrc/texture.hip).  Texel (i, j) is column i, row j, stored ``[j, i]``; coordinates are centre coordinates
    x = u size - 0.5, so texel i has x = i.

    Faces 2b and 2b + 1 share the square block b of side ``s`` at ((b % G) s, (b // G) s), G = size // s; ``s`` is ``block``, or the
    largest integer with G^2 >= ceil(F / 2); s >= 4 or ValueError (it names the smallest size that fits).  With L = s - 3 and (li, lj)
    the position inside the block, the lower face has its corners at (0, 0), (L, 0), (0, L) and owns li + lj <= s - 1; the upper face
    has them at (s-1, s-1), (2, s-1), (s-1, 2) (the lower chart turned by 180 degrees, not mirrored) and owns li + lj >= s.  Texels
    outside the G s square, in blocks past the last face and in the upper half of the last block of an odd F are unowned (-1).  The four
    texels of a bilinear lookup at any point of a face's uv triangle are owned by that face: lower floor(x) + floor(y) + 2 <= L + 2 =
    s - 1, upper floor(x) + floor(y) > s - 1, so no lookup mixes two charts and no dilation pass is needed.

    Attributes: ``n_faces``, ``size``, ``s``, ``G``, ``uv`` float32 [F,3,2] ((x + 0.5) / size of the corners; row 0 of a texture at v = 0)."""

    def __init__(self, n_faces, size, block=None):
        import math
        self.n_faces, self.size = int(n_faces), int(size)
        if self.n_faces < 0 or self.size < 1:
            raise ValueError(f'n_faces must be >= 0 and size >= 1, got {n_faces}, {size}')
        need = max(-(-self.n_faces // 2), 1)
        g = math.isqrt(need - 1) + 1                                      # the fewest blocks per side
        if block is not None and int(block) < TEXTURE_MIN_BLOCK:
            raise ValueError(f'block must be >= {TEXTURE_MIN_BLOCK}, got {block}')
        self.s = int(block) if block is not None else self.size // g
        self.G = self.size // self.s if self.s > 0 else 0
        if self.s < TEXTURE_MIN_BLOCK or self.G < g:
            fit = g * (int(block) if block is not None else TEXTURE_MIN_BLOCK)
            raise ValueError(f'{self.n_faces} faces need {g} x {g} blocks of side {fit // g}: the smallest size that fits is {fit}, got {self.size}')
        self.uv = ((self.corners().astype(F32) + F32(0.5)) / F32(self.size)).astype(F32)

    def corners(self):
        """int64 [F,3,2]: the texel coordinates (x, y) of the three corners of every face."""
        f = np.arange(self.n_faces, dtype=np.int64)
        b, up = f >> 1, (f & 1).astype(bool)
        far, L = self.s - 1, self.s - 3
        cx = np.stack([np.where(up, far, 0), np.where(up, 2, L), np.where(up, far, 0)], 1) + ((b % self.G) * self.s)[:, None]
        cy = np.stack([np.where(up, far, 0), np.where(up, far, 0), np.where(up, 2, L)], 1) + ((b // self.G) * self.s)[:, None]
        return np.stack([cx, cy], -1)

    def texels(self):
        """(face int32 [size,size], -1 where unowned; a, c int64 [size,size]: the texel's offset from corner 0 of its face along the two
        legs, 0 where unowned)."""
        j, i = np.meshgrid(np.arange(self.size, dtype=np.int64), np.arange(self.size, dtype=np.int64), indexing='ij')
        li, lj = i % self.s, j % self.s
        up = li + lj >= self.s
        face = 2 * ((j // self.s) * self.G + i // self.s) + up
        own = (i < self.G * self.s) & (j < self.G * self.s) & (face < self.n_faces)
        far = self.s - 1
        return (np.where(own, face, -1).astype(np.int32), np.where(own, np.where(up, far - li, li), 0), np.where(own, np.where(up, far - lj, lj), 0))

    def texel_face(self):
        """int32 [size,size]: the face that owns each texel, -1 where none does."""
        return self.texels()[0]


def _atlas_points_numpy(v32, f, atlas, normals, dtype):
    face, a, c = atlas.texels()
    n = atlas.size
    out = {'point': np.zeros((n, n, 3), dtype), 'face': face, 'bary': np.zeros((n, n, 3), dtype), 'normal': np.zeros((n, n, 3), dtype)}
    if not f.shape[0]:
        return out, 0
    own = face >= 0
    fi = np.where(own, face, 0)
    with np.errstate(all='ignore'):
        L = dtype(atlas.s - 3)
        l1, l2 = a.astype(dtype) / L, c.astype(dtype) / L
        l0 = (dtype(1) - l1) - l2
        mix = lambda x: (l0[..., None] * x[f[fi, 0]] + l1[..., None] * x[f[fi, 1]]) + l2[..., None] * x[f[fi, 2]]
        p = v32.astype(dtype)
        fn = _cross3(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
        l = np.sqrt(_dot3(fn, fn))
        bad = ~((l > 0) & np.isfinite(l))
        nrm = _unit_rows(fn[fi] if normals is None else mix(normals.astype(dtype)), dtype)
        out['point'] = np.where(own[..., None], mix(p), dtype(0))
    out['bary'] = np.where(own[..., None], np.stack([l0, l1, l2], -1), dtype(0))
    out['normal'] = np.where((own & ~bad[fi])[..., None], nrm, dtype(0))
    return out, int(bad.sum())


def _texture_dtype(dtype):
    dtype = np.dtype(dtype).type
    if dtype not in (np.float32, np.float64):
        raise ValueError(f'dtype must be float32 or float64, got {dtype}')
    return dtype


def atlas_points(verts, faces, atlas, normals=None, dtype=np.float32):
    """The surface point under every texel of ``atlas`` (a ``TextureAtlas`` of ``faces.shape[0]`` faces): a dict of 'point' float32
    [size,size,3], 'face' int32 [size,size] (-1: unowned), 'bary' [size,size,3], 'normal' [size,size,3] and 'info' {'degenerate'}.

    A texel of face t = (A, B, C) at offset (a, c) from corner 0 along the two legs has lambda_1 = fp32(a) / fp32(L), lambda_2 =
    fp32(c) / fp32(L), lambda_0 = (1 - lambda_1) - lambda_2 and point = (lambda_0 A + lambda_1 B) + lambda_2 C, every operation
    rounded on its own.  The guard texels of the diagonal have a negative weight: they are extrapolated on the triangle's plane, not
    clamped, so that the bilinear lookup reproduces an affine function of position everywhere inside the triangle.  'normal' is the unit
    (B - A) x (C - A), or with ``normals`` [V,3] their normalised mix.  A face with a non-finite vertex or no area keeps the points the
    formula gives and has a zero normal; 'info'['degenerate'] counts such faces.  Unowned texels are 0 / -1.

    Device tensors run on ia_atlas_points (csrc/texture.hip) and give the bits of the float32 restatement; CPU tensors and NumPy arrays
    take the NumPy restatement, with ``dtype=np.float64`` in double."""
    _mesh_args(verts, faces)
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    if not isinstance(atlas, TextureAtlas) or atlas.n_faces != nf:
        raise ValueError(f'atlas must be a TextureAtlas of {nf} faces')
    if normals is not None and (normals.ndim != 2 or tuple(normals.shape) != (nv, 3)):
        raise ValueError(f'normals must be [{nv},3], got {tuple(normals.shape)}')
    if isinstance(verts, torch.Tensor) and verts.is_cuda:
        from . import hipops
        if dtype not in (np.float32, torch.float32):
            raise ValueError('the device path is float32')
        dev = verts.device
        f = torch.as_tensor(faces).to(device=dev, dtype=torch.int32).contiguous()
        _faces_in_range(f, nv)
        nrm = None if normals is None else torch.as_tensor(normals).to(device=dev, dtype=torch.float32).contiguous()
        out = hipops.atlas_points(verts.detach().float().contiguous(), f, atlas.size, atlas.s, nrm)
        out['info'] = {'degenerate': int(out.pop('degenerate'))}
        return out
    dtype = _texture_dtype(dtype)
    f = _np(faces).astype(np.int64)
    _faces_in_range(f, nv)
    as32 = lambda a: None if a is None else np.ascontiguousarray(_np(a), dtype=F32)
    out, bad = _atlas_points_numpy(as32(verts), f, atlas, as32(normals), dtype)
    out = {k: _as_out(x, verts, np.int32 if k == 'face' else dtype) for k, x in out.items()}
    out['info'] = {'degenerate': bad}
    return out


def bake_texture(verts, faces, size, fn, atlas=None, chunk=1 << 20, normals=None):
    """A texture from a function of position: ``fn(points [M,3]) -> [M,C]`` (or [M]) is called over the owned texels of the atlas
    (``atlas``, or ``TextureAtlas(F, size)``) in chunks of ``chunk`` points.  Returns {'texture' float32 [size,size,C], 'mask' bool
    [size,size] (the owned texels), 'atlas', 'points' (what ``atlas_points`` returned)}.  Texels that no face owns are 0."""
    atlas = TextureAtlas(int(faces.shape[0]), size) if atlas is None else atlas
    if atlas.size != int(size):
        raise ValueError(f'atlas has size {atlas.size}, not {size}')
    pts = atlas_points(verts, faces, atlas, normals=normals)
    own = pts['face'] >= 0
    p = pts['point'][own]
    parts = []
    for c0 in range(0, int(p.shape[0]), int(chunk)):
        val = fn(p[c0:c0 + int(chunk)])
        parts.append(val.reshape(val.shape[0], -1))
    if isinstance(p, torch.Tensor):
        vals = torch.cat(parts).float() if parts else torch.zeros(0, 1, device=p.device)
        tex = torch.zeros(atlas.size, atlas.size, vals.shape[1], device=p.device)
    else:
        vals = np.concatenate(parts).astype(F32) if parts else np.zeros((0, 1), F32)
        tex = np.zeros((atlas.size, atlas.size, vals.shape[1]), F32)
    tex[own] = vals
    return {'texture': tex, 'mask': own, 'atlas': atlas, 'points': pts}


def _mesh_extent(verts):
    """The longest side of the bounding box of the finite vertices (0 without any)."""
    v = _np(verts).astype(np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    return float((v.max(0) - v.min(0)).max()) if v.shape[0] else 0.0


def _bilinear_numpy(img, x, y, dtype):
    """The bilinear read of img [H,W,C] at (x, y) [M] (inside the image): i0 = floor x, fx = x - i0, i1 = min(i0 + 1, W - 1), and
    (1 - fy) ((1 - fx) I00 + fx I10) + fy ((1 - fx) I01 + fx I11)."""
    fi, fj = np.floor(x), np.floor(y)
    fx, fy = (x - fi)[:, None], (y - fj)[:, None]
    i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
    i1, j1 = np.minimum(i0 + 1, img.shape[1] - 1), np.minimum(j0 + 1, img.shape[0] - 1)
    one = dtype(1)
    top = (one - fx) * img[j0, i0].astype(dtype) + fx * img[j0, i1].astype(dtype)
    bot = (one - fx) * img[j1, i0].astype(dtype) + fx * img[j1, i1].astype(dtype)
    return (one - fy) * top + fy * bot


def _view_weight_numpy(c, power, dtype):
    if power == np.floor(power) and power <= 64:
        w = np.ones_like(c)
        for _ in range(int(power)):
            w = w * c
        return w
    return np.power(c.astype(np.float64), np.float64(power)).astype(dtype)


def _texture_views_numpy(X32, n32, cam32, depth, mask, H, W, near, min_cos, depth_tol, dtype):
    """Steps 1 to 3 of ``project_texture`` for the points X32 [M,3] with normals n32: per view (passes bool [M], u, v, cos)."""
    R, o, k = _camera_numpy(cam32, H, W, dtype)
    X, nr = X32.astype(dtype), n32.astype(dtype)
    for n in range(cam32.shape[0]):
        with np.errstate(all='ignore'):
            d = X - o[n]
            xc = [(R[n, 0, a] * d[:, 0] + R[n, 1, a] * d[:, 1]) + R[n, 2, a] * d[:, 2] for a in range(3)]
            px = (k[n, 0] * xc[0] + k[n, 1] * xc[1]) + k[n, 2] * xc[2]
            py = (k[n, 3] * xc[0] + k[n, 4] * xc[1]) + k[n, 5] * xc[2]
            u, v, z = px / xc[2], py / xc[2], xc[2]
            ok = (np.isfinite(u) & np.isfinite(v) & np.isfinite(z) & ~(z <= dtype(near)) & (np.abs(u) < dtype(RASTER_MAX_SCREEN))
                  & (np.abs(v) < dtype(RASTER_MAX_SCREEN)))
            ok &= (u >= 0) & (u <= dtype(W - 1)) & (v >= 0) & (v <= dtype(H - 1))
            e = o[n] - X
            t = np.sqrt(_dot3(e, e))
            c = _dot3(nr, e) / t
            ok &= c > dtype(min_cos)
            pi, pj = np.rint(np.where(ok, u, 0)).astype(np.int64), np.rint(np.where(ok, v, 0)).astype(np.int64)
            ok &= mask[n, pj, pi] & (np.abs(t - depth[n, pj, pi].astype(dtype)) <= dtype(depth_tol))
        yield ok, np.where(ok, u, dtype(0)), np.where(ok, v, dtype(0)), np.where(ok, c, dtype(0))


def _texture_project_numpy(X32, n32, images, cam32, depth, mask, near, min_cos, power, depth_tol, best, dtype):
    M, (N, H, W, C) = X32.shape[0], images.shape
    num, den = np.zeros((M, C), np.float64), np.zeros(M, np.float64)
    count, w_best, col_best = np.zeros(M, np.int32), np.zeros(M, dtype), np.zeros((M, C), dtype)
    for n, (ok, u, v, c) in enumerate(_texture_views_numpy(X32, n32, cam32, depth, mask, H, W, near, min_cos, depth_tol, dtype)):
        col = _bilinear_numpy(images[n], u, v, dtype)
        w = _view_weight_numpy(c, power, dtype)
        num += np.where(ok[:, None], (w[:, None] * col).astype(np.float64), 0.0)
        den += np.where(ok, w.astype(np.float64), 0.0)
        better = ok & ((count == 0) | (w > w_best))
        w_best, col_best = np.where(better, w, w_best), np.where(better[:, None], col, col_best)
        count += ok
    hit = count > 0
    with np.errstate(all='ignore'):
        tex = col_best if best else (num / den[:, None]).astype(dtype)
    return np.where(hit[:, None], tex, dtype(0)), np.where(hit, w_best if best else den.astype(dtype), dtype(0)), count, hit


def project_texture(verts, faces, atlas, images, cameras, depth=None, mask=None, min_cos=0.2, power=2.0, depth_tol=None, mode='blend',
                    fallback=None, normals=None, near=1e-6, dtype=np.float32):
    """Projective texturing: the texture of ``atlas`` from rendered views ``images`` float32 [N,H,W,C] (C <= 8) of the cameras [N,25].
    ``depth`` / ``mask`` are those of ``rasterize_mesh(verts, faces, cameras, (H, W))`` and are computed here when not given.  Returns
    {'texture' [size,size,C], 'weight' [size,size] (sum of w, or the best w), 'views' int32 (how many views passed), 'filled' bool}.
    For the point X and normal n of a texel (``atlas_points``; ``normals``: vertex normals for it) and view k in ascending order, in
    float32 with every operation rounded on its own:

    1. Project as ``rasterize_mesh`` step 1 without the snap: u, v, z.  The view is skipped if that rule calls X unusable (``near``) or
       u is outside [0, W - 1] or v outside [0, H - 1].
    2. e = o - X, t = sqrt(e . e), c = (n . e) / t; skipped unless c > ``min_cos``.
    3. At pixel (rint u, rint v): skipped unless ``mask`` is set and |t - depth| <= ``depth_tol`` (depth is the ray parameter, as t is).
    4. colour = the bilinear read of images[k] at (u, v), pixel centres at integer coordinates (``_bilinear_numpy``); w = c^power (an
       integer power <= 64 is the product ((c c) c) ..., any other the float32 rounding of the double power).

    ``mode='blend'``: sum w colour / sum w, the terms w colour and w float32, the two sums double in view order, the quotient rounded
    once; ``'best'``: the colour of the view with the largest w, the lowest k among equals.  A texel that no view passes takes
    ``fallback`` (a texture of the same shape, e.g. the decoder bake) where given, else 0, and weight 0.

    ``depth_tol`` defaults to ``TEXTURE_DEPTH_TOL`` * extent / max(H, W), extent being the longest side of the mesh's bounding box.
    Measured on the 320-face icosphere (radius 0.5, extent 1, 3 cameras at radius 2.7, atlas sizes 64 and 128), counting the texel-views
    with c > 0.2 that lie inside their triangle (lambda_0 >= 0; a guard texel is extrapolated off the surface) and whose pixel the mesh
    covers, which the depth test of the float64 restatement rejects: at 32^2 views the multiples 1, 2, 4, 8 of extent / max(H, W) reject
    130 / 933, 19 / 124, 0 / 11, 0 / 0 (size 64 / 128), at 64^2 views 120 / 1032, 31 / 198, 7 / 17, 0 / 0.  The smallest power-of-two
    multiple that rejects none is 8 (at c = 0.2 the depth under a pixel changes by five pixel footprints across the pixel), the default
    is twice that.  Independently of the tolerance a texel within a pixel of a view's silhouette can find ``mask`` unset there.

    Device tensors run on ia_atlas_points + ia_texture_project (csrc/texture.hip; one thread per texel, the views in a loop, no atomics)
    and give the bits of the float32 restatement; CPU tensors and NumPy arrays take the NumPy restatement, ``dtype=np.float64`` in
    double."""
    if mode not in _TEXTURE_MODES:
        raise ValueError(f'mode must be one of {_TEXTURE_MODES}, got {mode!r}')
    if images.ndim != 4 or not 1 <= images.shape[3] <= TEXTURE_MAX_CHANNELS:
        raise ValueError(f'images must be [N,H,W,C] with 1 <= C <= {TEXTURE_MAX_CHANNELS}, got {tuple(images.shape)}')
    N, H, W, C = (int(n) for n in images.shape)
    if cameras.ndim != 2 or tuple(cameras.shape) != (N, 25):
        raise ValueError(f'cameras must be [{N},25], got {tuple(cameras.shape)}')
    if (depth is None) != (mask is None):
        raise ValueError('depth and mask are given together')
    power, min_cos, near = float(power), float(min_cos), float(near)
    if not power >= 0 or not near >= 0:
        raise ValueError(f'power and near must be >= 0, got {power}, {near}')
    if fallback is not None and tuple(fallback.shape) != (atlas.size, atlas.size, C):
        raise ValueError(f'fallback must be {(atlas.size, atlas.size, C)}, got {tuple(fallback.shape)}')
    tol = TEXTURE_DEPTH_TOL * _mesh_extent(verts) / max(H, W) if depth_tol is None else float(depth_tol)
    if not tol >= 0:
        raise ValueError(f'depth_tol must be >= 0, got {depth_tol}')
    pts = atlas_points(verts, faces, atlas, normals=normals, dtype=dtype)
    if depth is None:
        r = rasterize_mesh(verts, faces, cameras, (H, W), near=near, dtype=dtype)
        depth, mask = r['depth'], r['mask']
    if tuple(depth.shape) != (N, H, W) or tuple(mask.shape) != (N, H, W):
        raise ValueError(f'depth and mask must be {(N, H, W)}, got {tuple(depth.shape)} and {tuple(mask.shape)}')
    if isinstance(verts, torch.Tensor) and verts.is_cuda:
        from . import hipops
        dev = verts.device
        f32 = lambda t: None if t is None else torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()
        return hipops.texture_project(pts['point'], pts['normal'], pts['face'], f32(images), f32(cameras), f32(depth),
                                      torch.as_tensor(mask).to(device=dev, dtype=torch.bool).contiguous(), near, min_cos, power, tol,
                                      mode == 'best', f32(fallback))
    dtype = _texture_dtype(dtype)
    face = _np(pts['face'])
    own = face >= 0
    tex, wgt, cnt, hit = _texture_project_numpy(_np(pts['point'])[own].astype(F32), _np(pts['normal'])[own].astype(F32), _np(images).astype(F32),
                                                np.ascontiguousarray(_np(cameras), dtype=F32), _np(depth), _np(mask).astype(bool), near, min_cos,
                                                power, tol, mode == 'best', dtype)
    n = atlas.size
    out = {'texture': np.zeros((n, n, C), dtype), 'weight': np.zeros((n, n), dtype), 'views': np.zeros((n, n), np.int32), 'filled': np.zeros((n, n), bool)}
    out['texture'][own], out['weight'][own], out['views'][own], out['filled'][own] = tex, wgt, cnt, hit
    if fallback is not None:
        out['texture'] = np.where(out['filled'][..., None], out['texture'], _np(fallback).astype(dtype))
    kinds = {'views': np.int32, 'filled': bool}
    return {k: _as_out(x, verts, kinds.get(k, dtype)) for k, x in out.items()}


def _texture_sample_numpy(tex, atlas, face, bary, dtype):
    size, s, G = atlas.size, atlas.s, atlas.G
    ok = (face >= 0) & (face < atlas.n_faces)
    out = np.zeros(face.shape + (tex.shape[2],), dtype)
    if not ok.any():
        return out
    f = face[ok].astype(np.int64)
    b = bary[ok].astype(dtype)
    uv = atlas.uv.astype(dtype)[f]                                        # [M,3,2]
    blk = f >> 1
    bx, by = (blk % G) * s, (blk // G) * s
    with np.errstate(all='ignore'):
        u = (b[:, 0] * uv[:, 0, 0] + b[:, 1] * uv[:, 1, 0]) + b[:, 2] * uv[:, 2, 0]
        v = (b[:, 0] * uv[:, 0, 1] + b[:, 1] * uv[:, 1, 1]) + b[:, 2] * uv[:, 2, 1]
        x, y = u * dtype(size) - dtype(0.5), v * dtype(size) - dtype(0.5)
        xl = np.fmin(np.fmax(x - bx.astype(dtype), dtype(0)), dtype(s - 1))
        yl = np.fmin(np.fmax(y - by.astype(dtype), dtype(0)), dtype(s - 1))
        fi, fj = np.floor(xl), np.floor(yl)
        fx, fy = (xl - fi)[:, None], (yl - fj)[:, None]
        i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
        i1, j1 = np.minimum(i0 + 1, s - 1), np.minimum(j0 + 1, s - 1)
        t = lambda jj, ii: tex[by + jj, bx + ii].astype(dtype)
        one = dtype(1)
        top = (one - fx) * t(j0, i0) + fx * t(j0, i1)
        bot = (one - fx) * t(j1, i0) + fx * t(j1, i1)
        out[ok] = (one - fy) * top + fy * bot
    return out


def sample_texture(texture, atlas, face, bary, dtype=np.float32):
    """The texture [size,size,C] looked up at points of the mesh given as ``face`` int [...] and ``bary`` [..., 3] (the 'face' / 'bary'
    of ``rasterize_mesh``): float32 [..., C], 0 where face < 0.  In float32, every operation rounded on its own: the uv mix
    (b0 uv0 + b1 uv1) + b2 uv2 of the face's atlas corners, x = u size - 0.5 and y likewise, clamped into the face's block
    (fmin(fmax(x - bx, 0), s - 1), so that rounding at a corner or an extrapolating weight never reads another chart), i0 = floor,
    fx = x - i0, i1 = min(i0 + 1, s - 1) and (1 - fy) ((1 - fx) T00 + fx T10) + fy ((1 - fx) T01 + fx T11).  Device tensors run on
    ia_texture_sample (csrc/texture.hip) and give the bits of the float32 restatement; ``dtype=np.float64``: the restatement in double."""
    if texture.ndim != 3 or tuple(texture.shape[:2]) != (atlas.size, atlas.size):
        raise ValueError(f'texture must be [{atlas.size},{atlas.size},C], got {tuple(texture.shape)}')
    if tuple(bary.shape) != tuple(face.shape) + (3,):
        raise ValueError(f'bary must be face.shape + [3], got {tuple(bary.shape)} for {tuple(face.shape)}')
    if isinstance(texture, torch.Tensor) and texture.is_cuda:
        from . import hipops
        if dtype not in (np.float32, torch.float32):
            raise ValueError('the device path is float32')
        dev = texture.device
        return hipops.texture_sample(texture.detach().float().contiguous(), atlas.s, atlas.n_faces,
                                     torch.as_tensor(face).to(device=dev, dtype=torch.int32).contiguous(),
                                     torch.as_tensor(bary).to(device=dev, dtype=torch.float32).contiguous())
    dtype = _texture_dtype(dtype)
    out = _texture_sample_numpy(_np(texture), atlas, _np(face), _np(bary), dtype)
    return _as_out(out, texture, dtype)


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


def bake_colors(planes, decoder, verts, faces, size, box_warp, atlas=None, chunk=1 << 20):
    """``bake_texture`` of the decoder's rgb[:3], clamped to [0, 1], for the planes [1,3,32,H,W] of one avatar: what ``vertex_colors``
    samples at the vertices, at every texel."""
    fn = lambda p: query_planes(planes, decoder, p[None].float(), box_warp, rgb=True)['rgb'][0, :, :3].clamp(0, 1)
    return bake_texture(verts, faces, size, fn, atlas=atlas, chunk=chunk)


# ------------------------------------------------------------------ PLY

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
    nf = int(next((h for h in head if h.startswith('element face')), 'element face 0').split()[-1])     # (a cloud has no face element)
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


# ------------------------------------------------------------------ OBJ

def write_obj(path, verts, faces, uv, texture, normals=None):
    """Wavefront OBJ with a texture: ``name.obj`` (``v``; ``vt``, 3 F entries from ``uv`` [F,3,2] with 1 - v, OBJ's origin being
    bottom-left; ``vn`` with ``normals`` [V,3]; ``f a/ta/na ...``, 1-based), ``name.mtl`` (``map_Kd name.png``) and ``name.png`` (the
    first three channels of ``texture`` float [size,size,C] in [0, 1], or one grey channel; 8 bit, row 0 on top).  ``path`` is the .obj."""
    import os
    from PIL import Image
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    v, f = _np(verts).astype(np.float64).reshape(-1, 3), _np(faces).astype(np.int64).reshape(-1, 3)
    t = _np(uv).astype(np.float64).reshape(-1, 3, 2)
    if t.shape[0] != f.shape[0]:
        raise ValueError(f'uv must be [{f.shape[0]},3,2], got {tuple(_np(uv).shape)}')
    tex = _np(texture).astype(np.float64)
    tex = tex[..., None] if tex.ndim == 2 else tex
    img = np.rint(np.clip(tex[..., :3] if tex.shape[2] >= 3 else tex[..., 0], 0, 1) * 255).astype(np.uint8)
    Image.fromarray(img, mode='RGB' if img.ndim == 3 else 'L').save(stem + '.png')
    with open(stem + '.mtl', 'w') as fh:
        fh.write(f'newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n')
    lines = [f'mtllib {name}.mtl', f'usemtl {name}']
    lines += ['v %.9g %.9g %.9g' % tuple(p) for p in v]
    lines += ['vt %.17g %.17g' % (p[0], 1.0 - p[1]) for p in t.reshape(-1, 2)]         # (1 - v is exact in double: the round trip is too)
    if normals is not None:
        lines += ['vn %.9g %.9g %.9g' % tuple(p) for p in _np(normals).astype(np.float64).reshape(-1, 3)]
    for k, (a, b, c) in enumerate(f + 1):
        ta = 3 * k + 1
        if normals is None:
            lines.append(f'f {a}/{ta} {b}/{ta + 1} {c}/{ta + 2}')
        else:
            lines.append(f'f {a}/{ta}/{a} {b}/{ta + 1}/{b} {c}/{ta + 2}/{c}')
    with open(stem + '.obj', 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


def read_obj(path):
    """Inverse of ``write_obj``: {'verts' float32 [V,3], 'faces' int64 [F,3], 'uv' float32 [F,3,2] (v flipped back), 'normals' float32
    [V,3] or None, 'texture' float32 [size,size,C] in [0, 1] or None (the ``map_Kd`` image of the material library)}."""
    import os
    v, vt, vn, tri, tri_t, tri_n, mtl = [], [], [], [], [], [], None
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if not p:
                continue
            if p[0] == 'v':
                v.append([float(x) for x in p[1:4]])
            elif p[0] == 'vt':
                vt.append([float(x) for x in p[1:3]])
            elif p[0] == 'vn':
                vn.append([float(x) for x in p[1:4]])
            elif p[0] == 'mtllib':
                mtl = p[1]
            elif p[0] == 'f':
                ids = [(q.split('/') + ['', ''])[:3] for q in p[1:4]]
                tri.append([int(q[0]) - 1 for q in ids])
                tri_t.append([int(q[1]) - 1 if q[1] else -1 for q in ids])
                tri_n.append([int(q[2]) - 1 if q[2] else -1 for q in ids])
    verts, faces = np.array(v, dtype=np.float32).reshape(-1, 3), np.array(tri, dtype=np.int64).reshape(-1, 3)
    out = {'verts': verts, 'faces': faces, 'uv': None, 'normals': None, 'texture': None}
    if vt:
        t = np.array(vt, dtype=np.float64)[np.array(tri_t, dtype=np.int64).reshape(-1, 3)]
        out['uv'] = np.stack([t[..., 0], 1.0 - t[..., 1]], -1).astype(np.float32)
    if vn:
        nrm = np.zeros((verts.shape[0], 3), np.float32)
        nrm[faces.reshape(-1)] = np.array(vn, dtype=np.float32)[np.array(tri_n, dtype=np.int64).reshape(-1)]
        out['normals'] = nrm
    folder = os.path.dirname(path)
    if mtl and os.path.exists(os.path.join(folder, mtl)):
        with open(os.path.join(folder, mtl)) as fh:
            maps = [l.split()[1] for l in fh if l.startswith('map_Kd')]
        if maps and os.path.exists(os.path.join(folder, maps[0])):
            from PIL import Image
            img = np.asarray(Image.open(os.path.join(folder, maps[0]))).astype(np.float32) / np.float32(255)
            out['texture'] = img[..., None] if img.ndim == 2 else img
    return out
