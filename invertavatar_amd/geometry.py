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
- ``write_ply`` / ``read_ply``: binary little-endian PLY in NumPy.

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


def write_ply(path, verts, faces, colors=None):
    """Binary little-endian PLY: float x, y, z (+ uchar red, green, blue) per vertex, int32 index triples per face."""
    v = _np(verts).astype('<f4').reshape(-1, 3)
    f = _np(faces).astype('<i4').reshape(-1, 3)
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    if colors is not None:
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
    vrec = np.empty(v.shape[0], dtype=fields)
    vrec['x'], vrec['y'], vrec['z'] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        c = _np(colors).astype(np.uint8).reshape(-1, 3)
        vrec['red'], vrec['green'], vrec['blue'] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(f.shape[0], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    frec['n'], frec['i'] = 3, f
    head = ['ply', 'format binary_little_endian 1.0', f'element vertex {v.shape[0]}', 'property float x', 'property float y',
            'property float z']
    if colors is not None:
        head += ['property uchar red', 'property uchar green', 'property uchar blue']
    head += [f'element face {f.shape[0]}', 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(head) + '\n').encode('ascii'))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path):
    """Inverse of ``write_ply``: (verts float32 [V,3], faces int64 [F,3], colors uint8 [V,3] or None)."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    head = data[:end].decode('ascii').split('\n')
    nv = int(next(h for h in head if h.startswith('element vertex')).split()[-1])
    nf = int(next(h for h in head if h.startswith('element face')).split()[-1])
    has_col = 'property uchar red' in head
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')] + ([('red', 'u1'), ('green', 'u1'), ('blue', 'u1')] if has_col else [])
    vrec = np.frombuffer(data, dtype=fields, count=nv, offset=end)
    frec = np.frombuffer(data, dtype=[('n', 'u1'), ('i', '<i4', (3,))], count=nf, offset=end + vrec.nbytes)
    verts = np.stack([vrec['x'], vrec['y'], vrec['z']], -1).astype(np.float32)
    cols = np.stack([vrec['red'], vrec['green'], vrec['blue']], -1) if has_col else None
    return verts, frec['i'].astype(np.int64), cols
