"""geometry.simplify_mesh on the CPU: the NumPy restatement is the definition, so these tests check the definition's own properties
(invariants, order independence, orientation, the derivable distance bound, the target_faces contract) and the host logic.  The meshes,
the tolerance and the checks are shared with tests/test_simplify_gpu.py, which holds the kernels to the same restatement.

Tolerance for positions: ``e_ord`` is the largest difference between two float64 runs of the restatement, one on the input as given
and one with vertices and faces reversed (the definition's own sensitivity to the order of summation on that input); a route is held
to ``4 * e_ord + eps32 * extent`` of the float64 restatement (extent: the largest |coordinate|; the second term is the rounding of the
result to float32)."""
import ctypes

import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, geometry
from test_surface_distance_cpu import cube_mesh, radial_volume, random_soup

F32 = np.float32
EPS32 = float(np.finfo(F32).eps)


# ------------------------------------------------------------------ meshes

def tess_cube(n, lo=0.0, size=1.0):
    """The surface of a cube with n x n quads per side, welded, outward-wound; vertices lo + size * i / n."""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            for u in range(n):
                for v in range(n):
                    q = []
                    for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[a], p[b], p[c] = side * n, u + du, v + dv
                        q.append(vid(tuple(p)))
                    if side == 0:
                        q = q[::-1]
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    v = (lo + size * np.array(verts, dtype=np.float64) / n).astype(F32)
    return v, np.array(faces, dtype=np.int64)


def cube_with_satellites(n=24):
    """The unit cube [0, 1]^3 (n x n quads per side) and three small boxes that pull the bounding box down to -0.17 along each axis
    without sharing a cell with a corner of the cube: with ``cell_size = 0.25`` the cell walls are at -0.17 + 0.25 k, so the eight
    corners lie strictly inside their cells."""
    parts = [tess_cube(n)]
    for a in range(3):
        lo = [0.45, 0.45, 0.45]
        lo[a] = -0.17
        parts.append(cube_mesh(lo, (0.05, 0.05, 0.05)))
    return merge(parts)


def merge(parts):
    vs, fs, off = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs).astype(F32), np.concatenate(fs).astype(np.int64)


def sphere_mesh(n=25):
    vol, lo, step = radial_volume(n)
    v, f = geometry.marching_cubes(vol, 0.23, (lo,) * 3, (step,) * 3)
    return np.asarray(v, dtype=F32), np.asarray(f, dtype=np.int64)


def flat_square(n=37, z=0.3):
    ax = np.linspace(-1, 1, n + 1)
    g = np.stack(np.meshgrid(ax, ax, indexing='ij'), -1).reshape(-1, 2)
    v = np.concatenate([g, np.full((len(g), 1), z)], 1).astype(F32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    a = (i * (n + 1) + j).reshape(-1)
    f = np.concatenate([np.stack([a, a + n + 1, a + n + 2], -1), np.stack([a, a + n + 2, a + 1], -1)])
    return v, f.astype(np.int64)


def closed_meshes():
    return {'sphere': sphere_mesh(25), 'cube': tess_cube(19), 'cube_sat': cube_with_satellites(24)}


def soups():
    rs = np.random.RandomState(5)
    return {'soup': random_soup(rs, 333), 'soup_clustered': random_soup(rs, 500, clustered=True)}


# ------------------------------------------------------------------ checks shared with the GPU tests

def to_np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def grid_of(res):
    """The grid of a result as the restatement takes it; None for the identity clustering."""
    if res['dims'] is None:
        return None
    cell = np.asarray(res['cell'], dtype=np.float64)
    return tuple(res['dims']), list(res['lo']), (1.0 / cell).astype(F32), cell


def reversed_mesh(v, f):
    return v[::-1].copy(), (len(v) - 1 - f)[::-1].copy()


def reference64(v, f, res, placement):
    """(float64 positions of the restatement, e_ord, tolerance) for the grid of ``res``."""
    grid = grid_of(res)
    a = geometry._simplify_numpy(v, f, grid, placement, as64=True)
    if grid is None:
        b = a
    else:
        b = geometry._simplify_numpy(*reversed_mesh(v, f), grid, placement, as64=True)
    assert np.array_equal(a['faces'], b['faces'])
    e_ord = float(np.abs(a['verts'] - b['verts']).max()) if a['verts'].size else 0.0
    fin = v[np.isfinite(v).all(1)]
    extent = float(np.abs(fin).max()) if fin.size else 0.0
    return a, e_ord, 4 * e_ord + EPS32 * extent, extent


def check_invariants(v, f, res):
    ov, of, vmap, csize = (to_np(res[k]) for k in ('verts', 'faces', 'vertex_map', 'cluster_size'))
    assert ov.dtype == F32 and of.dtype == np.int64 and vmap.dtype == np.int64 and csize.dtype == np.int64
    assert ov.shape == (len(csize), 3) and of.ndim == 2 and of.shape[1] == 3 and vmap.shape == (len(v),)
    if len(of):
        assert (of[:, 0] < of[:, 1]).all() and (of[:, 0] < of[:, 2]).all() and (of[:, 1] != of[:, 2]).all()
        d = np.diff(of, axis=0)
        lead = np.where(d[:, 0] != 0, d[:, 0], np.where(d[:, 1] != 0, d[:, 1], d[:, 2]))
        assert (lead > 0).all()                                            # strictly increasing, hence unique
    assert np.array_equal(np.unique(of), np.arange(len(ov)))               # every output vertex is referenced
    mapped = vmap >= 0
    assert csize.sum() == mapped.sum() and np.array_equal(np.bincount(vmap[mapped], minlength=len(ov)), csize)
    assert np.isfinite(ov).all()
    if res['dims'] is not None and len(ov):
        dims, lo, inv, cell = grid_of(res)
        keys = geometry._simplify_keys_numpy(v, lo, inv, dims)
        first = np.full(len(ov), -1, dtype=np.int64)
        first[vmap[mapped][::-1]] = np.flatnonzero(mapped)[::-1]
        k = keys[first]
        ijk = np.stack([k // (dims[1] * dims[2]), (k // dims[2]) % dims[1], k % dims[2]], -1)
        assert (np.diff(k) > 0).all()                                      # numbered by ascending linear cell index
        box_lo = np.asarray(lo, dtype=F32).astype(np.float64) + ijk * cell
        tol = 8 * EPS32 * np.abs(v[np.isfinite(v).all(1)]).max()
        assert (ov >= box_lo - tol).all() and (ov <= box_lo + cell + tol).all()


def signed_volume(v, f):
    a, b, c = (np.asarray(v, dtype=np.float64)[f[:, i]] for i in range(3))
    return float((a * np.cross(b, c)).sum() / 6)


def diagonal(res):
    return float(np.sqrt((np.asarray(res['cell']) ** 2).sum()))


def same_container(v, f, like):
    """The arrays in the container (NumPy, or torch on a device) of the caller's choice."""
    if like is None:
        return v, f
    return torch.from_numpy(np.ascontiguousarray(v)).to(like), torch.from_numpy(np.ascontiguousarray(f)).to(like)


# Inputs on which the float64 restatement meets the one-cell-diagonal bound in the direction input -> simplified as well (a closed
# surface much larger than a cell, nothing that vanishes inside one cell).  Asserted here and on the device; elsewhere printed.
OPPOSITE_BOUND_HOLDS = {('sphere', 8), ('sphere', 16), ('cube', 8), ('cube', 16)}


def check_distance_bound(name, cells, v, f, res, device=None, samples=3000):
    ov, of = res['verts'], res['faces']
    if to_np(of).shape[0] == 0:
        return
    fin = v[np.isfinite(v).all(1)]
    bound = diagonal(res) + 8 * EPS32 * float(np.abs(fin).max())
    tv, tf = same_container(v, f, device)
    for smp in (samples, None):                                            # area-weighted samples, then the vertices
        r = geometry.surface_distance(ov, of, tv, tf, samples=smp)
        print(f'{name} cells={cells} samples={smp}: simplified->input {r["max_ab"]:.6f}  input->simplified {r["max_ba"]:.6f}  bound {bound:.6f}')
        assert r['max_ab'] <= bound
        if (name, cells) in OPPOSITE_BOUND_HOLDS:
            assert r['max_ba'] <= bound


# ------------------------------------------------------------------ tests

@pytest.mark.parametrize('placement', ['mean', 'quadric'])
def test_identity(placement):
    for name, (v, f) in closed_meshes().items():
        res = geometry.simplify_mesh(v, f, cell_size=1e-4, placement=placement)
        check_invariants(v, f, res)
        assert res['verts'].shape == v.shape and res['faces'].shape == f.shape, name
        assert np.array_equal(np.sort(res['vertex_map']), np.arange(len(v)))
        ref, e_ord, tol, _ = reference64(v, f, res, placement)
        err = np.abs(res['verts'][res['vertex_map']].astype(np.float64) - v).max()
        print(f'identity {name} {placement}: e_ord {e_ord:.3e} error {err:.3e} tol {tol:.3e}')
        assert err == 0 if placement == 'mean' else err <= tol
        # the same triangles, up to rotation and order
        mapped = res['vertex_map'][f]
        first = np.argmin(mapped, 1)[:, None]
        mapped = np.take_along_axis(mapped, (first + np.arange(3)) % 3, 1)
        assert np.array_equal(np.unique(mapped, axis=0), res['faces'])


def test_empty_and_non_finite():
    v, f = sphere_mesh(17)
    res = geometry.simplify_mesh(v, f, cells=1)
    assert res['verts'].shape == (0, 3) and res['faces'].shape == (0, 3) and (res['vertex_map'] == -1).all() and res['dims'] == (1, 1, 1)
    for vv, ff in ((np.zeros((0, 3), F32), np.zeros((0, 3), np.int64)), (v, np.zeros((0, 3), np.int64)),
                   (np.full((5, 3), np.nan, F32), np.array([[0, 1, 2], [2, 3, 4]]))):
        for kw in ({'cells': 4}, {'target_faces': 10}, {'cell_size': 0.1}):
            res = geometry.simplify_mesh(vv, ff, **kw)
            assert res['verts'].shape == (0, 3) and res['faces'].shape == (0, 3) and res['vertex_map'].shape == (len(vv),)
            assert res['cluster_size'].shape == (0,) and res['usable_faces'] == 0
    # a NaN vertex removes exactly its incident faces
    bad = 7
    w = v.copy()
    w[bad, 1] = np.nan
    full = geometry.simplify_mesh(v, f, cell_size=1e-4)
    part = geometry.simplify_mesh(w, f, cell_size=1e-4)
    check_invariants(w, f, part)
    incident = (f == bad).any(1)
    assert part['faces'].shape[0] == full['faces'].shape[0] - incident.sum() and part['usable_faces'] == len(f) - incident.sum()
    assert part['vertex_map'][bad] == -1 and (part['vertex_map'][np.arange(len(v)) != bad] >= 0).all()
    with pytest.raises(ValueError):
        geometry.simplify_mesh(v, np.array([[0, 1, len(v)]]), cells=4)
    with pytest.raises(ValueError):
        geometry.simplify_mesh(v, np.array([[0, -1, 2]]), cells=4)


@pytest.mark.parametrize('placement', ['mean', 'quadric'])
def test_invariants_order_independence_and_distance_bound(placement):
    rs = np.random.RandomState(11)
    for name, (v, f) in {**closed_meshes(), **soups()}.items():
        for cells in (3, 8, 16):
            res = geometry.simplify_mesh(v, f, cells=cells, placement=placement)
            check_invariants(v, f, res)
            ref, e_ord, tol, _ = reference64(v, f, res, placement)
            err = float(np.abs(res['verts'] - ref['verts']).max()) if len(res['verts']) else 0.0
            print(f'{name} cells={cells} {placement}: V {len(v)} -> {len(res["verts"])}, F {len(f)} -> {len(res["faces"])}, e_ord {e_ord:.3e} tol {tol:.3e}')
            assert err <= tol
            pv, pf = rs.permutation(len(v)), rs.permutation(len(f))
            inv = np.empty_like(pv)
            inv[pv] = np.arange(len(v))
            perm = geometry.simplify_mesh(v[pv], np.roll(inv[f[pf]], rs.randint(3), axis=1), cells=cells, placement=placement)
            assert np.array_equal(perm['faces'], res['faces']) and np.array_equal(perm['cluster_size'], res['cluster_size'])
            assert np.array_equal(perm['vertex_map'][inv], res['vertex_map'])
            if len(res['verts']):
                assert np.abs(perm['verts'].astype(np.float64) - ref['verts']).max() <= tol
            if cells == 8 or (cells == 16 and placement == 'quadric' and name in ('sphere', 'soup')):
                check_distance_bound(name, cells, v, f, res, samples=800)


def test_orientation_and_volume():
    for name in ('sphere', 'cube'):
        v, f = closed_meshes()[name]
        vol = signed_volume(v, f)
        assert vol > 0
        errs = []
        for cells in (8, 16, 32):
            res = geometry.simplify_mesh(v, f, cells=cells)
            out = signed_volume(res['verts'], res['faces'])
            errs.append(abs(out - vol) / vol)
            assert out > 0
        print(f'{name}: volume {vol:.5f}, relative error at 8, 16, 32 cells: {errs}')
        assert errs[2] < 0.02
        if name == 'sphere':                                               # the float64 restatement improves monotonically on the sphere
            assert errs[0] > errs[1] > errs[2]


def corner_distances(v, f, res):
    """Distance of the representative of each cube corner's cluster from the corner, over the cell edge."""
    ov, vmap = to_np(res['verts']).astype(np.float64), to_np(res['vertex_map'])
    out = []
    for c in np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=F32):
        at = np.flatnonzero((v == c).all(1))
        assert at.size == 1 and vmap[at[0]] >= 0
        out.append(np.linalg.norm(ov[vmap[at[0]]] - c))
    return np.array(out)


def test_quadric_keeps_corners_and_planes():
    v, f = cube_with_satellites()
    q = geometry.simplify_mesh(v, f, cell_size=0.25)
    m = geometry.simplify_mesh(v, f, cell_size=0.25, placement='mean')
    check_invariants(v, f, q)
    _, e_ord, tol, _ = reference64(v, f, q, 'quadric')
    dq, dm = corner_distances(v, f, q), corner_distances(v, f, m)
    print(f'corner clusters: quadric {dq.max():.3e} (tol {tol:.3e}, e_ord {e_ord:.3e}), mean {dm.min() / 0.25:.3f} .. {dm.max() / 0.25:.3f} cells')
    assert dq.max() <= tol
    assert (dm > 1000 * tol).all() and dm.min() / 0.25 > 0.1              # the mean rounds every corner off by a good part of a cell
    sv, sf = flat_square()
    for placement in ('quadric', 'mean'):
        res = geometry.simplify_mesh(sv, sf, cells=7, placement=placement)
        check_invariants(sv, sf, res)
        assert len(res['faces']) and np.abs(res['verts'][:, 2].astype(np.float64) - float(F32(0.3))).max() <= reference64(sv, sf, res, placement)[2]


def check_target(v, f, n, res, run, max_cells=4096):
    nf = to_np(res['faces']).shape[0]
    assert nf <= n
    if res['dims'] is None:
        return None
    c = max(res['dims'])
    if c < max_cells:
        more = run(cells=c + 1)
        assert to_np(more['faces']).shape[0] > n, (n, c)
    same = run(cells=c)
    assert np.array_equal(to_np(same['faces']), to_np(res['faces'])) and np.array_equal(to_np(same['verts']), to_np(res['verts']))
    return c


def test_target_faces():
    v, f = sphere_mesh(25)
    run = lambda **kw: geometry.simplify_mesh(v, f, **kw)                # noqa: E731
    chosen = []
    for n in (12, 100, 777, 2000):
        res = run(target_faces=n)
        check_invariants(v, f, res)
        chosen.append(check_target(v, f, n, res, run))
        assert res['steps'] >= 1
    assert chosen == sorted(chosen)
    res = run(target_faces=len(f) - 1, max_cells=4)
    assert max(res['dims']) == 4 and len(res['faces']) <= len(f) - 1
    # n >= usable F: the renumbered input, no grid
    w = v.copy()
    w[3] = np.inf
    res = geometry.simplify_mesh(w, f, target_faces=len(f))
    assert res['dims'] is None and res['steps'] == 0 and res['cell_size'] == 0.0
    keep = ~(f == 3).any(1)
    assert len(res['faces']) == keep.sum() and len(res['verts']) == len(v) - 1 and res['vertex_map'][3] == -1
    assert np.array_equal(res['verts'], w[np.arange(len(v)) != 3])          # input order, exact positions
    assert np.array_equal(res['vertex_map'][np.arange(len(v)) != 3], np.arange(len(v) - 1))


def check_extras(v, f, res, extras):
    vmap = to_np(res['vertex_map'])
    assert len(res['extras']) == len(extras)
    for e, out in zip(extras, res['extras']):
        e, o = to_np(e), to_np(out)
        assert o.dtype == e.dtype and o.shape == (len(to_np(res['verts'])),) + e.shape[1:]
        rows = e.reshape(len(e), -1).astype(np.float64)
        cnt = np.bincount(vmap[vmap >= 0], minlength=len(o)).astype(np.float64)
        mean = np.stack([np.bincount(vmap[vmap >= 0], weights=rows[vmap >= 0, j], minlength=len(o)) for j in range(rows.shape[1])], -1) / cnt[:, None]
        got = o.reshape(len(o), -1).astype(np.float64)
        if np.issubdtype(e.dtype, np.floating):
            assert np.abs(got - mean).max() <= 4 * np.finfo(e.dtype).eps * np.abs(rows).max()
        else:
            assert np.abs(got - mean).max() <= 0.5 + 1e-9


def make_extras(v, rs):
    return [rs.randn(len(v), 3).astype(F32), rs.randint(0, 256, (len(v), 3)).astype(np.uint8), rs.randn(len(v), 5), rs.rand(len(v)).astype(F32)]


def test_extras():
    v, f = sphere_mesh(25)
    extras = make_extras(v, np.random.RandomState(2))
    for kw in ({'cells': 6}, {'cells': 13, 'placement': 'mean'}, {'target_faces': 10 ** 6}):
        res = geometry.simplify_mesh(v, f, extras=extras, **kw)
        check_extras(v, f, res, extras)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    res = geometry.simplify_mesh(tv, tf, cells=6, extras=[torch.from_numpy(extras[0])])
    assert isinstance(res['verts'], torch.Tensor) and res['faces'].dtype == torch.int64 and res['extras'][0].dtype == torch.float32
    assert np.array_equal(res['verts'].numpy(), geometry.simplify_mesh(v, f, cells=6)['verts'])


def test_argument_errors():
    v, f = cube_mesh()
    for kw in ({}, {'cells': 4, 'cell_size': 0.1}, {'cells': 4, 'target_faces': 10}, {'cell_size': 0.1, 'target_faces': 10}, {'cells': 0},
               {'cells': (2, 0, 2)}, {'cells': (2, 2)}, {'cell_size': 0.0}, {'cell_size': -1.0}, {'cell_size': float('nan')}, {'target_faces': 0},
               {'cells': 4, 'placement': 'median'}, {'cells': 4, 'max_cells': 0}, {'cells': 4, 'extras': [np.zeros((3, 2))]}):
        with pytest.raises(ValueError):
            geometry.simplify_mesh(v, f, **kw)
    with pytest.raises(ValueError):
        geometry.simplify_mesh(v[:, :2], f, cells=2)
    res = geometry.simplify_mesh(v, f, cells=(2, 3, 4))
    assert res['dims'] == (2, 3, 4) and len(res['faces']) == 12


def test_plan_matches_the_library_and_abi_errors():
    lib = _lib.load()
    f3, i3, d3 = ctypes.c_float * 3, ctypes.c_int * 3, ctypes.c_double * 3
    lo, hi = [-0.3, 0.1, 2.0], [1.7, 0.9, 2.0]
    for kw, args in (({'cells': 7}, (None, 7, 0.0)), ({'cell_size': 0.13}, (None, 0, 0.13)), ({'cells': (3, 5, 2)}, (i3(3, 5, 2), 0, 0.0)),
                     ({'cells': 4096}, (None, 4096, 0.0))):
        dims, inv, cell = i3(), f3(), d3()
        assert lib.ia_simplify_plan(f3(*lo), f3(*hi), args[0], args[1], args[2], dims, inv, cell) == 0, _lib.last_error()
        pd, pi, pc = geometry._simplify_plan([float(F32(x)) for x in lo], [float(F32(x)) for x in hi], kw.get('cells'), kw.get('cell_size'))
        assert tuple(dims) == pd and np.array_equal(np.array(inv, dtype=F32), pi) and np.array_equal(np.array(cell), pc), kw
    dims, inv, cell = i3(), f3(), d3()
    assert lib.ia_simplify_plan(None, f3(*hi), None, 4, 0.0, dims, inv, cell) == -1 and 'null' in _lib.last_error()
    assert lib.ia_simplify_plan(f3(*lo), f3(*hi), None, 4, 0.5, dims, inv, cell) == -1 and 'exactly one' in _lib.last_error()
    assert lib.ia_simplify_plan(f3(*lo), f3(*hi), None, 0, -1.0, dims, inv, cell) == -1 and 'cell_size' in _lib.last_error()
    assert lib.ia_simplify_box(None, 5, None, 0, None, None) == -1 and 'scratch' in _lib.last_error()
    assert lib.ia_simplify_keys(None, 5, f3(*lo), f3(1, 1, 1), i3(2, 2, 2), None, None) == -1 and 'device pointers' in _lib.last_error()
    assert lib.ia_simplify_keys(None, 5, f3(*lo), f3(1, 1, 1), i3(2, 0, 2), None, None) == -1 and 'dims' in _lib.last_error()
    assert lib.ia_simplify_clusters(None, None, 5, None, None, None, None, 5, None, 8, None, None) == -1 and 'scratch' in _lib.last_error()
    assert lib.ia_simplify_classify(None, 3, 5, None, 9, None, None, None, None, None, None) == -1 and 'K' in _lib.last_error()
    assert lib.ia_simplify_face_heads(None, None, 3, None, None) == -1 and 'device pointer' in _lib.last_error()
    assert lib.ia_simplify_place(None, None, None, None, None, 5, 4, f3(*lo), f3(1, 1, 1), d3(1, 1, 1), i3(2, 2, 2), None, 3, None) == -1
    assert 'holds 3' in _lib.last_error()
    assert lib.ia_simplify_means(None, None, None, 5, 4, 2, None, 2, 0, 3, None) == -1 and 'holds 3' in _lib.last_error()
    assert lib.ia_simplify_accumulate_verts(None, 3, 0, 3, None, None, 40, 50, 5, None, None, 0, None) == -1 and 'device pointer' in _lib.last_error()
    nbytes = ctypes.c_size_t(0)
    assert lib.ia_simplify_accumulate_scratch_bytes(1000, 9, ctypes.byref(nbytes)) == 0 and nbytes.value > 0
    assert lib.ia_simplify_accumulate_scratch_bytes(1000, 5, ctypes.byref(nbytes)) == -1 and 'width' in _lib.last_error()
    assert lib.ia_simplify_accumulate_scratch_bytes(1000, 9, None) == -1


def test_extract_geometry_simplify_option(tmp_path):
    """The generator method and the command line on the CPU route (small synthetic generator)."""
    from invertavatar_amd import extract_geometry
    args = ['--seeds', '0', '--width', 'small', '--res', '24', '--level', '0', '--outdir', str(tmp_path), '--device', 'cpu', '--normals']
    (_, full), = extract_geometry.main(args)
    (path, out), = extract_geometry.main(args + ['--simplify', '150', '--simplify-check'])
    info = out['simplify']
    assert 'simplify' not in full and info['faces_before'] == full['faces'].shape[0] and info['faces_after'] == out['faces'].shape[0] <= 150
    nv = out['verts'].shape[0]
    assert out['colors'].shape == (nv, 3) and out['normals'].shape == (nv, 3) and nv == info['verts_after'] < info['verts_before']
    v, f, c, n = geometry.read_ply(path, with_normals=True)
    assert np.array_equal(v, to_np(out['verts'])) and np.array_equal(f, to_np(out['faces'])) and np.array_equal(c, to_np(out['colors']))
    import json
    meta = json.load(open(str(tmp_path / 'seed0000_geometry.json')))
    chk = meta['simplify']['check']
    assert chk['simplified_to_full'] <= chk['cell_diagonal'] + 8 * EPS32 * float(np.abs(v).max())
    (_, cells), = extract_geometry.main(args + ['--simplify-cells', '5'])
    assert max(cells['simplify']['dims']) == 5
    with pytest.raises(SystemExit):
        extract_geometry.main(args + ['--simplify', '150', '--simplify-cells', '5'])
