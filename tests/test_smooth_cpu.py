"""geometry.smooth_mesh, MeshAdjacency and mesh_normals: the NumPy restatement that is the definition, checked against
independent constructions and against the properties the smoothing is used for; and the meshes, references and tolerances the GPU
tests (tests/test_smooth_gpu.py) share.

Tolerance of the device positions: ``4 * e32 + eps32 * extent`` of the restatement.  ``e32`` is the largest difference between two
runs of the restatement on the same input: one carries the positions in float64 throughout, the other rounds them to float32 after every
step (the definition, and the device's rounding points).  It is a property of the definition and the input, not of the code under test.
The cotangent weights and the normals use the same form with ``e32`` from a float32 run of the restatement and ``extent`` replaced by
max |w| (weights) or 1 (unit normals)."""
import json

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry
from test_simplify_cpu import EPS32, flat_square, signed_volume, sphere_mesh, tess_cube, to_np

F32 = np.float32


# ------------------------------------------------------------------ meshes

def mean_edge(v, f):
    e = np.concatenate([v[f[:, 0]] - v[f[:, 1]], v[f[:, 1]] - v[f[:, 2]], v[f[:, 2]] - v[f[:, 0]]]).astype(np.float64)
    return float(np.sqrt((e * e).sum(1)).mean())


def noisy(v, f, seed=0, amount=0.15):
    """The mesh with seeded Gaussian noise of ``amount`` mean edge lengths on every coordinate."""
    rs = np.random.RandomState(seed)
    return (v.astype(np.float64) + rs.normal(0, amount * mean_edge(v, f), v.shape)).astype(F32)


def fan(n, closed, seed=1):
    """A triangle fan around a hub of degree n: vertex 0 is the hub, 1 .. n the ring; ``closed`` adds a second hub below (a bipyramid,
    no boundary), otherwise the ring is the boundary.  Noisy, so that every vertex has somewhere to go."""
    rs = np.random.RandomState(seed + n)
    t = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(t), np.sin(t), np.zeros(n)], -1)
    v = [np.array([[0, 0, 0.7]]), ring] + ([np.array([[0, 0, -0.7]])] if closed else [])
    v = (np.concatenate(v) + rs.normal(0, 0.02, (n + 1 + closed, 3))).astype(F32)
    i = np.arange(n)
    f = [np.stack([np.zeros(n, int), 1 + i, 1 + (i + 1) % n], -1)]
    if closed:
        f.append(np.stack([np.full(n, n + 1), 1 + (i + 1) % n, 1 + i], -1))
    return v, np.concatenate(f).astype(np.int64)


def index_soup(seed=7, nv=40, nf=300):
    """Random triangles over few vertices: non-manifold edges, duplicate faces, faces with a repeated index, one vertex (nv - 1) that
    only such faces use and one (nv - 2) that no face uses."""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-1, 1, (nv, 3)).astype(F32)
    f = rs.randint(0, nv - 2, (nf, 3))
    f = np.concatenate([f, f[:20], f[5:9, ::-1], [[nv - 1, nv - 1, 3], [4, nv - 1, 4]]])
    return v, f.astype(np.int64)


def bad_sphere():
    """sphere_mesh(17) with a NaN vertex and an inf vertex inside."""
    v, f = sphere_mesh(17)
    v = noisy(v, f, 3)
    v[7, 1] = np.nan
    v[100] = np.inf
    return v, f


def small_meshes():
    """V = 1 (no face), 3 (one triangle) and open fans with V = 63, 65 and 257."""
    out = {'V1': (np.array([[0.1, 0.2, 0.3]], dtype=F32), np.zeros((0, 3), np.int64)),
           'V3': (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=F32), np.array([[0, 1, 2]]))}
    for n in (63, 65, 257):
        out[f'V{n}'] = fan(n - 1, False)
    return out


def fans():
    return {f'fan{n}{"c" if closed else "o"}': fan(n, closed) for n in (63, 64, 65, 70, 300) for closed in (True, False)}


def surfaces():
    """The meshes on which the smallest angle is far from 0 (the cotangent weights are compared on these only)."""
    s17, s25, cube, sq = sphere_mesh(17), sphere_mesh(25), tess_cube(19), flat_square()
    return {'sphere17': (noisy(*s17, 1), s17[1]), 'sphere25': (noisy(*s25, 2), s25[1]), 'cube': (noisy(*cube, 3), cube[1]),
            'square': (noisy(*sq, 4, 0.1), sq[1])}


def odd_meshes():
    v, f = sphere_mesh(17)
    iso = np.concatenate([noisy(v, f, 5), [[3, 3, 3]]]).astype(F32)                    # an isolated vertex
    return {'soup': index_soup(), 'bad_sphere': bad_sphere(), 'isolated': (iso, f), 'no_faces': (v, np.zeros((0, 3), np.int64)),
            'no_verts': (np.zeros((0, 3), F32), np.zeros((0, 3), np.int64))}


def all_meshes():
    return {**surfaces(), **odd_meshes(), **fans(), **small_meshes()}


# ------------------------------------------------------------------ references shared with the GPU tests

def extent_of(v):
    fin = v[np.isfinite(v).all(1)]
    return float(np.abs(fin).max()) if fin.size else 0.0


def factors_of(iterations, lam=0.5, mu=-0.53):
    return [lam] * iterations if mu is None else [lam, mu] * iterations


def reference(v, f, iterations=10, lam=0.5, mu=-0.53, weights='uniform', boundary='fixed', fixed=None):
    """(float64 positions of the definition, pinned, e32, tolerance)."""
    adj = geometry._adjacency_numpy(v, f)
    w = geometry._cotangent_numpy(v, adj) if weights == 'cotangent' else None
    pinned = geometry._pinned_numpy(adj, w, boundary, fixed)
    fac = factors_of(iterations, lam, mu)
    a = geometry._smooth_numpy(v, adj, w, pinned, fac, round32=True)
    b = geometry._smooth_numpy(v, adj, w, pinned, fac, round32=False)
    ok = np.isfinite(v).all(1)
    e32 = float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0
    return a, pinned, e32, 4 * e32 + EPS32 * extent_of(v)


def cotangent_reference(v, f):
    """(weights of the definition, e32, tolerance)."""
    adj = geometry._adjacency_numpy(v, f)
    w64, w32 = geometry._cotangent_numpy(v, adj), geometry._cotangent_numpy(v, adj, F32)
    e32 = float(np.abs(w64.astype(np.float64) - w32).max()) if w64.size else 0.0
    return w64, e32, 4 * e32 + EPS32 * (float(w64.max()) if w64.size else 0.0)


def normals_reference(v, f, weighting):
    adj = geometry._adjacency_numpy(v, f)
    with np.errstate(all='ignore'):
        n64, n32 = geometry._mesh_normals_numpy(v, f, adj, weighting), geometry._mesh_normals_numpy(v, f, adj, weighting, F32)
    e32 = float(np.abs(n64.astype(np.float64) - n32).max()) if n64.size else 0.0
    return n64, e32, 4 * e32 + EPS32


def roughness(v, f):
    """Mean length of the umbrella vector (mean of the neighbours minus the vertex) over the vertices that have neighbours."""
    adj = geometry._adjacency_numpy(np.asarray(v, dtype=F32), f)
    p = np.asarray(v, dtype=np.float64)
    deg = np.diff(adj['offsets'].astype(np.int64))
    s = np.stack([np.bincount(adj['row'], weights=p[adj['neighbors'], c], minlength=len(p)) for c in range(3)], -1)
    has = deg > 0
    u = s[has] / deg[has, None] - p[has]
    return float(np.sqrt((u * u).sum(1)).mean())


def independent_adjacency(v, f):
    """Directed keys through np.unique: (keys i V + j ascending, faces per key)."""
    fin = np.isfinite(v).all(1)
    keep = [t for t in f if len(set(t)) == 3 and fin[list(t)].all()]
    keys = [a * len(v) + b for t in keep for a, b in ((t[0], t[1]), (t[1], t[0]), (t[1], t[2]), (t[2], t[1]), (t[2], t[0]), (t[0], t[2]))]
    return np.unique(np.array(keys, dtype=np.int64), return_counts=True), len(keep)


def check_adjacency(v, f, adj):
    """The public arrays of a MeshAdjacency against the np.unique construction."""
    off, nbr, ef, bnd = (to_np(getattr(adj, k)).astype(np.int64) for k in ('offsets', 'neighbors', 'edge_faces', 'boundary'))
    (keys, counts), n_usable = independent_adjacency(v, f)
    nv = len(v)
    assert off.shape == (nv + 1,) and off[0] == 0 and off[-1] == len(nbr) == len(ef) and (np.diff(off) >= 0).all()
    row = np.repeat(np.arange(nv), np.diff(off))
    assert np.array_equal(row * nv + nbr, keys) and np.array_equal(ef, counts)       # sorted, unique, the right multiplicities
    back = {int(k): int(c) for k, c in zip(keys, counts)}
    assert all(back[int(j * nv + i)] == c for i, j, c in zip(row, nbr, counts))      # symmetric
    want_b = np.zeros(nv, bool)
    want_b[row[counts == 1]] = True
    assert np.array_equal(bnd.astype(bool), want_b)
    info = adj.info
    assert info == {'edges': len(keys) // 2, 'boundary_edges': int((counts == 1).sum()) // 2, 'nonmanifold_edges': int((counts > 2).sum()) // 2,
                    'boundary_verts': int(want_b.sum()), 'usable_faces': n_usable, 'max_degree': int(np.diff(off).max()) if nv else 0}
    foff, fid = to_np(adj.face_offsets).astype(np.int64), to_np(adj.face_ids).astype(np.int64)
    assert foff.shape == (nv + 1,) and foff[-1] == len(fid) == 3 * n_usable
    for i in range(nv):
        mine = fid[foff[i]:foff[i + 1]]
        assert (np.diff(mine) > 0).all() and all(i in f[t] for t in mine)


# ------------------------------------------------------------------ tests

def test_adjacency_against_independent_constructions():
    for name, (v, f) in all_meshes().items():
        adj = geometry.MeshAdjacency(v, f)
        assert adj.offsets.dtype == np.int32 and adj.neighbors.dtype == np.int32 and adj.edge_faces.dtype == np.int32 and adj.boundary.dtype == bool
        check_adjacency(v, f, adj)
    for name in ('sphere17', 'sphere25', 'cube'):
        v, f = surfaces()[name]
        info = geometry.MeshAdjacency(v, f).info
        assert info['boundary_edges'] == 0 and info['nonmanifold_edges'] == 0 and 2 * info['edges'] == 3 * len(f), name
    for n in (5, 37):
        info = geometry.MeshAdjacency(*flat_square(n)).info
        assert info['boundary_edges'] == 4 * n and info['boundary_verts'] == 4 * n
    v, f = sphere_mesh(17)
    adj = geometry.MeshAdjacency(v, np.concatenate([f, f[3:4]]))
    ef = adj.edge_faces.reshape(-1)
    row = np.repeat(np.arange(len(v)), np.diff(adj.offsets))
    on_face = np.isin(row, f[3]) & np.isin(adj.neighbors, f[3])
    assert (ef[on_face] == 3).all() and (ef[~on_face] == 2).all() and on_face.sum() == 6 and adj.info['nonmanifold_edges'] == 3
    one = geometry.MeshAdjacency(v[f[3]], np.array([[0, 1, 2], [0, 1, 2]]))
    assert (one.edge_faces == 2).all() and one.info['boundary_edges'] == 0                 # a doubled face makes its edges count 2
    try:
        import scipy.sparse as sp
    except ImportError:
        sp = None
    if sp is not None:
        v, f = index_soup()
        adj = geometry.MeshAdjacency(v, f)
        row = np.repeat(np.arange(len(v)), np.diff(adj.offsets))
        ok = np.array([len(set(t)) == 3 for t in f])
        t = f[ok]
        i = np.concatenate([t[:, 0], t[:, 1], t[:, 1], t[:, 2], t[:, 2], t[:, 0]])
        j = np.concatenate([t[:, 1], t[:, 0], t[:, 2], t[:, 1], t[:, 0], t[:, 2]])
        m = sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(len(v), len(v))).tocsr()
        m.sum_duplicates()
        m.sort_indices()
        assert np.array_equal(m.indptr, adj.offsets) and np.array_equal(m.indices, adj.neighbors) and np.array_equal(m.data, adj.edge_faces)


def test_faces_order_does_not_change_the_integer_parts():
    rs = np.random.RandomState(0)
    for name in ('sphere17', 'soup', 'square'):
        v, f = all_meshes()[name]
        a, b = geometry.MeshAdjacency(v, f), geometry.MeshAdjacency(v, np.roll(f[rs.permutation(len(f))], 1, axis=1))
        for k in ('offsets', 'neighbors', 'edge_faces', 'boundary', 'face_offsets'):
            assert np.array_equal(getattr(a, k), getattr(b, k)), (name, k)
        assert a.info == b.info


def test_pinning():
    v0, f = flat_square()
    v = noisy(v0, f, 4, 0.1)
    v[:, :2] = v0[:, :2]
    out = geometry.smooth_mesh(v, f)
    adj = out['adjacency']
    b = adj.boundary
    assert b.sum() == 148 and np.array_equal(out['pinned'], b)
    assert np.array_equal(out['verts'][b].view(np.uint32), v[b].view(np.uint32))
    assert out['verts'][~b, 2].std() < 0.5 * v[~b, 2].std()
    free = geometry.smooth_mesh(v, f, boundary='free')
    assert not free['pinned'].any() and (free['verts'][b] != v[b]).any()
    for boundary in ('fixed', 'free'):
        plane = geometry.smooth_mesh(v0, f, boundary=boundary)
        assert np.array_equal(plane['verts'][:, 2].view(np.uint32), v0[:, 2].view(np.uint32))   # a sum of equal floats over their count
    mask = np.zeros(len(v), bool)
    mask[::3] = True
    out = geometry.smooth_mesh(v, f, fixed=mask, boundary='free')
    assert np.array_equal(out['pinned'], mask) and np.array_equal(out['verts'][mask], v[mask]) and (out['verts'][~mask] != v[~mask]).any()
    for name in ('isolated', 'soup', 'bad_sphere'):
        v, f = odd_meshes()[name]
        out = geometry.smooth_mesh(v, f, boundary='free')
        deg = np.diff(out['adjacency'].offsets)
        assert np.array_equal(out['pinned'], (deg == 0) | ~np.isfinite(v).all(1)), name
        assert np.array_equal(out['verts'][out['pinned']].view(np.uint32), v[out['pinned']].view(np.uint32))
        assert np.isfinite(out['verts'][np.isfinite(v).all(1)]).all()
    v, f = index_soup()
    assert np.diff(geometry.MeshAdjacency(v, f).offsets)[-2:].tolist() == [0, 0]          # unused, and used by repeated-index faces only


@pytest.mark.parametrize('iterations', [10, 20])
def test_taubin_keeps_the_volume_that_laplacian_smoothing_loses(iterations):
    for name in ('sphere17', 'sphere25', 'cube'):
        v, f = surfaces()[name]
        vol = signed_volume(v, f)
        taubin = geometry.smooth_mesh(v, f, iterations=iterations)['verts']
        laplace = geometry.smooth_mesh(v, f, iterations=iterations, mu=None)['verts']
        vt, vl = signed_volume(taubin, f), signed_volume(laplace, f)
        rt, r0 = roughness(taubin, f), roughness(v, f)
        print(f'{name} x{iterations}: volume {vol:.5f} taubin {vt:.5f} laplace {vl:.5f}; roughness {r0:.5f} -> {rt:.5f}')
        assert abs(vt - vol) < abs(vl - vol)
        assert rt < 0.5 * r0
        assert vt > 0 and vl > 0


def test_input_ownership_and_containers():
    v, f = surfaces()['sphere17']
    keep = v.copy()
    zero = geometry.smooth_mesh(v, f, iterations=0)
    assert np.array_equal(zero['verts'].view(np.uint32), v.view(np.uint32)) and zero['verts'] is not v and zero['info']['steps'] == 0
    allfix = geometry.smooth_mesh(v, f, fixed=np.ones(len(v), bool))
    assert np.array_equal(allfix['verts'].view(np.uint32), v.view(np.uint32)) and allfix['pinned'].all()
    out = geometry.smooth_mesh(v, f, iterations=3)
    assert np.array_equal(v, keep) and out['verts'].dtype == F32 and out['info']['steps'] == 6 and (out['verts'] != v).any()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    t = geometry.smooth_mesh(tv, tf, iterations=3)
    assert isinstance(t['verts'], torch.Tensor) and t['verts'].dtype == torch.float32 and t['pinned'].dtype == torch.bool
    assert np.array_equal(t['verts'].numpy(), out['verts']) and torch.equal(tv, torch.from_numpy(keep))
    again = geometry.smooth_mesh(v, f, iterations=3, adjacency=out['adjacency'])
    assert np.array_equal(again['verts'], out['verts']) and again['adjacency'] is out['adjacency']
    with pytest.raises(ValueError):
        geometry.smooth_mesh(v, np.array([[0, 1, len(v)]]))
    with pytest.raises(ValueError):
        geometry.smooth_mesh(v, np.array([[0, 1, -1]]))
    with pytest.raises(ValueError):
        geometry.smooth_mesh(v, f, weights='mean')
    with pytest.raises(ValueError):
        geometry.smooth_mesh(v, f, boundary='loose')
    with pytest.raises(ValueError):
        geometry.smooth_mesh(v, f, adjacency=geometry.MeshAdjacency(*sphere_mesh(25)))
    with pytest.raises(ValueError):
        geometry.mesh_normals(v, f, weighting='uniform')
    for name in ('no_faces', 'no_verts', 'V1'):
        vv, ff = all_meshes()[name]
        out = geometry.smooth_mesh(vv, ff, weights='cotangent')
        assert np.array_equal(out['verts'], vv) and out['verts'].dtype == F32 and out['pinned'].all() and out['pinned'].shape == (len(vv),)
        assert out['adjacency'].neighbors.shape == (0,) and out['adjacency'].cotangent().shape == (0,)
        assert geometry.mesh_normals(vv, ff).shape == (len(vv), 3) and not geometry.mesh_normals(vv, ff).any()


def equilateral_patch(n=9):
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    v = np.stack([i + 0.5 * j, np.sqrt(0.75) * j, 0 * i], -1).reshape(-1, 3).astype(np.float64)
    a = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([a, a + n + 1, a + 1], -1), np.stack([a + 1, a + n + 1, a + n + 2], -1)])
    return v.astype(F32), f.astype(np.int64)


def test_cotangent_weights():
    v, f = equilateral_patch()
    adj = geometry.MeshAdjacency(v, f)
    w = adj.cotangent()
    interior = (adj.edge_faces == 2)
    assert w.dtype == F32 and np.abs(w[interior] - 1 / np.sqrt(3)).max() < 1e-6           # 2 x cot(60 deg) / 2
    rs = np.random.RandomState(2)
    bumpy = v.copy()
    bumpy[:, 2] = rs.normal(0, 0.1, len(v))
    # the weights come from the positions the adjacency was built with: on the equilateral patch they are a common factor times the uniform ones
    flat_adj = geometry.MeshAdjacency(v, f)
    uni = geometry.smooth_mesh(bumpy, f, iterations=5, adjacency=flat_adj)
    cot = geometry.smooth_mesh(bumpy, f, iterations=5, weights='cotangent', adjacency=flat_adj)
    ref, _, e32, tol = reference(bumpy, f, 5)
    err = float(np.abs(cot['verts'].astype(np.float64) - uni['verts']).max())
    print(f'equilateral patch: cotangent against uniform {err:.3e}, tolerance {tol:.3e}')
    assert np.array_equal(cot['pinned'], uni['pinned']) and err <= tol
    # a zero-area face contributes 0; an all-obtuse pair clamps to 0 and pins a vertex whose weights all vanish
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0.05, 0], [0.5, -0.05, 0], [2, 0, 0]], dtype=F32)
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    adj = geometry.MeshAdjacency(v, f)
    w, row = adj.cotangent(), np.repeat(np.arange(5), np.diff(adj.offsets))
    w01 = w[(row == 0) & (adj.neighbors == 1)]
    assert w01 == 0 and adj.edge_faces[(row == 0) & (adj.neighbors == 1)] == 3
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0.05, 0], [0.5, -0.05, 0]], dtype=F32)
    f = np.array([[0, 1, 2], [1, 0, 3]])
    out = geometry.smooth_mesh(v, f, weights='cotangent', boundary='free')
    adj = out['adjacency']
    row = np.repeat(np.arange(4), np.diff(adj.offsets))
    assert adj.cotangent()[(row == 0) & (adj.neighbors == 1)] == 0 and (adj.cotangent()[(row == 2)] > 0).all()
    # vertex 4 lies on the segment 0 - 1 and only the face (0, 1, 4), which has no area, uses it: its weights all vanish
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0.5, 0.1], [0.5, -0.5, 0.1], [0.5, 0, 0]], dtype=F32)
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    out = geometry.smooth_mesh(v, f, weights='cotangent', boundary='free')
    w, row = out['adjacency'].cotangent(), np.repeat(np.arange(5), np.diff(out['adjacency'].offsets))
    assert (w[row == 4] == 0).all() and out['pinned'].tolist() == [False] * 4 + [True] and (w[row == 2] > 0).all()
    assert np.array_equal(out['verts'][4], v[4]) and (out['verts'][:4] != v[:4]).any()
    assert not geometry.smooth_mesh(v, f, boundary='free')['pinned'].any()                 # (uniform weights move it)
    for name, (v, f) in surfaces().items():
        w64, e32, tol = cotangent_reference(v, f)
        assert np.isfinite(w64).all() and (w64 >= 0).all() and tol < 1e-4, name


@pytest.mark.parametrize('weighting', ['area', 'angle'])
def test_mesh_normals(weighting):
    for name, (v, f) in all_meshes().items():
        with np.errstate(all='ignore'):
            n = geometry.mesh_normals(v, f, weighting=weighting)
        assert n.dtype == F32 and n.shape == v.shape
        ln = np.sqrt((n.astype(np.float64) ** 2).sum(1))
        assert (np.abs(ln[ln > 0] - 1) < 4 * EPS32).all() and np.isfinite(n).all(), name
        # a plain construction with np.add.at
        fin = np.isfinite(v).all(1)
        s = np.zeros((len(v), 3))
        p = v.astype(np.float64)
        for t in f:
            if len(set(t)) < 3 or not fin[t].all():
                continue
            c = np.cross(p[t[1]] - p[t[0]], p[t[2]] - p[t[0]])
            for k in range(3):
                if weighting == 'area':
                    np.add.at(s, t[k], c)
                elif np.linalg.norm(c) > 0:
                    e1, e2 = p[t[(k + 1) % 3]] - p[t[k]], p[t[(k + 2) % 3]] - p[t[k]]
                    np.add.at(s, t[k], c / np.linalg.norm(c) * np.arctan2(np.linalg.norm(np.cross(e1, e2)), e1 @ e2))
        sl = np.sqrt((s * s).sum(1))
        plain = np.where((sl > 0)[:, None], s / np.where(sl > 0, sl, 1)[:, None], 0)
        steady = sl > 1e-9 * max(sl.max(), 1e-30) if len(sl) else sl > 0                   # (a sum that cancels has no direction to compare)
        assert np.abs(n[steady] - plain[steady]).max(initial=0) <= 1e-6, name
        with np.errstate(all='ignore'):
            back = geometry.mesh_normals(v, f[:, ::-1], weighting=weighting)
        assert np.abs(back[steady] + n[steady]).max(initial=0) <= 1e-6, name


    # outward on the clean closed meshes (noise larger than a sliver of marching cubes turns the sliver over, and the angle weights count it)
    for name, (v, f), centre in (('sphere17', sphere_mesh(17), 0.0), ('sphere25', sphere_mesh(25), 0.0), ('cube', tess_cube(19), 0.5)):
        n = geometry.mesh_normals(v, f, weighting=weighting)
        assert ((n * (v - centre)).sum(1) > 0).all(), name


def test_extract_geometry_smooth_option(tmp_path):
    """The generator method and the command line on the CPU route (small synthetic generator)."""
    from invertavatar_amd import extract_geometry
    args = ['--seeds', '0', '--width', 'small', '--res', '16', '--level', '0', '--outdir', str(tmp_path), '--device', 'cpu', '--normals', '--keep', 'largest']
    (_, rough), = extract_geometry.main(args)
    (path, out), = extract_geometry.main(args + ['--smooth', '5', '--smooth-check'])
    assert 'smooth' not in rough and np.array_equal(to_np(out['faces']), to_np(rough['faces']))
    want = geometry.smooth_mesh(rough['verts'], rough['faces'], iterations=5)
    assert np.array_equal(to_np(out['verts']), to_np(want['verts'])) and out['smooth']['steps'] == 10
    assert np.array_equal(to_np(out['normals']), to_np(geometry.mesh_normals(out['verts'], out['faces'])))
    v, f, c, n = geometry.read_ply(path, with_normals=True)
    assert np.array_equal(v, to_np(out['verts'])) and np.array_equal(f, to_np(out['faces'])) and np.array_equal(n, to_np(out['normals']))
    assert np.array_equal(c, to_np(out['colors']))
    meta = json.load(open(str(tmp_path / 'seed0000_geometry.json')))['smooth']
    assert meta['boundary_edges'] == out['smooth']['boundary_edges'] and meta['check']['volume_before'] == geometry.signed_volume(rough['verts'], rough['faces'])
    laplace = geometry.smooth_mesh(rough['verts'], rough['faces'], iterations=5, mu=None)['verts']
    before = meta['check']['volume_before']
    assert abs(meta['check']['volume_after'] - before) < abs(geometry.signed_volume(laplace, rough['faces']) - before)
    assert meta['check']['volume_after'] == geometry.signed_volume(out['verts'], out['faces'])
    assert 0 < meta['check']['smoothed_to_input'] < 0.1 and 0 < meta['check']['input_to_smoothed'] < 0.1
    with pytest.raises(SystemExit):
        extract_geometry.main(args + ['--smooth-check'])
