"""Closest point on the cluster tree, on the host: the restatement ``geometry._closest_tree_numpy`` against the brute
restatement ``geometry._closest_numpy``.  The tree only prunes, so every comparison is exact: no tolerance appears in this file.  The
meshes are the marching-cubes sphere of test_winding_tree_gpu.py cut to the face counts at which a partial leaf, a partial top level,
a tie across leaves or an unusable tail can go wrong."""
import functools

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry
from test_align_cpu import shared_case
from test_surface_distance_cpu import uv_sphere
from test_winding_cpu import F32, mc_sphere, mc_torus, pushed_samples, sphere, torus

L, B = geometry.WINDING_LEAF, geometry.WINDING_BRANCH
FACE_COUNTS = [0, 1, L - 1, L, L + 1, L * B, L * B + 1, L * B * B + 3, None]
CENTRE = (0.01, -0.02, 0.03)


@functools.lru_cache(maxsize=None)
def mc48():
    _, _, _, _, v, f = mc_sphere(48, 0.8, CENTRE)
    assert f.shape[0] == 13324 and geometry._winding_levels(f.shape[0]) == [417, 53, 7, 1]
    return v, f


def cut(n):
    """The first n faces of mc48 (all of them for None), from 3 faces on with one face without area and one unusable face among them."""
    verts, faces = mc48()
    faces = faces.copy() if n is None else faces[:n].copy()
    if faces.shape[0] >= 3:
        faces[1] = (faces[1, 0], faces[1, 0], faces[1, 2])
        faces[2] = (-1, faces[2, 1], faces[2, 2])
    return verts, faces


@functools.lru_cache(maxsize=None)
def queries(n):
    """(points float32 [N,3], families: name -> slice).  Pushed samples of the surface; every vertex of the cut mesh (distance exactly
    0, and the faces around it tie); the sphere's centre; far points at 100 and 1000 times the extent along an axis and a diagonal; one
    row at 1e30; one NaN row."""
    verts, faces = cut(n)
    full_v, full_f = mc48()
    pushed, _ = pushed_samples(full_v, full_f, 64 if n is None else 16)
    used = faces[(faces >= 0).all(1)]
    own = verts[np.unique(used)] if used.size else np.zeros((0, 3), dtype=F32)
    extent = float(np.abs(full_v).max())
    far = (np.array([(100, 0, 0), (0, 0, -100), (58, 58, -58), (1000, 0, 0), (-577, 577, 577)], dtype=np.float64) * extent).astype(F32)
    rest = np.array([CENTRE, (1e30, -1e30, 1e30), (np.nan, 0.0, 1.0)], dtype=F32)
    parts, fam, at = [pushed, own, far, rest], {}, 0
    for name, part in zip(('pushed', 'vertices', 'far', 'rest'), parts):
        fam[name] = slice(at, at + part.shape[0])
        at += part.shape[0]
    return np.concatenate(parts).astype(F32), fam


@functools.lru_cache(maxsize=None)
def tree_of(n):
    return geometry.WindingTree(*cut(n))


@functools.lru_cache(maxsize=None)
def brute(n, dtype):
    verts, faces = cut(n)
    return geometry._closest_numpy(queries(n)[0], verts, faces, dtype)


@functools.lru_cache(maxsize=None)
def by_tree(n, dtype):
    return geometry._closest_tree_numpy(queries(n)[0], tree_of(n), dtype)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_same(got, want, what=''):
    for k, name in enumerate(('dist', 'face', 'point')):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, name, 'NaN pattern')
        assert np.array_equal(g, w, equal_nan=True), (what, name)


# ------------------------------------------------------------------ 1. the restatement is the brute restatement

@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('n', FACE_COUNTS)
def test_tree_equals_brute_exactly(n, dtype):
    pts, fam = queries(n)
    got, want = by_tree(n, dtype), brute(n, dtype)
    assert_same(got, want, f'F = {n}')
    dist, face = got[0], got[1]
    usable = tree_of(n).usable
    assert np.isnan(dist[-1]) and face[-1] == -1 and np.isnan(got[2][-1]).all()                        # the NaN row
    if usable:
        v = fam['vertices']
        assert (dist[v] == 0).all() and (face[v] >= 0).all()                                           # exact zeros, many faces tie
        if dtype is np.float64:
            assert np.isfinite(dist[:-1]).all()
    else:
        assert np.isinf(dist[:-1]).all() and (face == -1).all() and np.isnan(got[2]).all()


def test_ties_go_to_the_lowest_input_face():
    """At a vertex every face around it is at distance 0; the tree meets them in Morton order, the answer is the lowest input index."""
    verts, faces = cut(None)
    pts, fam = queries(None)
    face = by_tree(None, np.float64)[1][fam['vertices']]
    own = np.unique(faces[(faces >= 0).all(1)])
    first = np.full(verts.shape[0], np.iinfo(np.int64).max)
    usable = np.flatnonzero((faces >= 0).all(1))
    np.minimum.at(first, faces[usable].reshape(-1), np.repeat(usable, 3))
    assert np.array_equal(face, first[own])
    order = np.asarray(tree_of(None).order)
    pos = np.empty_like(order)
    pos[order] = np.arange(order.size)
    later = 0
    for v, f in zip(own, first[own]):
        ring = usable[(faces[usable] == v).any(1)]
        later += int((pos[ring] < pos[f]).any())
    assert later > 100                                     # (the test bites: often a higher input index comes first in Morton order)


# ------------------------------------------------------------------ 2. the boxes

@pytest.mark.parametrize('n', FACE_COUNTS)
def test_boxes_hold_their_faces(n):
    tree = tree_of(n)
    boxes, counts = tree.boxes, tree.counts
    assert boxes.dtype == np.float32 and boxes.shape == (sum(counts), 8) and not boxes[:, 3].any() and not boxes[:, 7].any()
    assert tree.boxes is boxes                                                                         # built once
    tris = np.asarray(tree.tris).reshape(-1, 3, 3)
    starts = np.concatenate([[0], np.cumsum(counts)])
    span = L
    for lvl, cnt in enumerate(counts):
        for i in range(cnt):
            row = boxes[starts[lvl] + i]
            v = tris[i * span:min((i + 1) * span, tree.usable)].reshape(-1, 3)
            assert v.shape[0] and (v >= row[0:3]).all() and (v <= row[4:7]).all()                      # every vertex of every face below
            if lvl == 0:
                assert np.array_equal(row[0:3], v.min(0)) and np.array_equal(row[4:7], v.max(0))      # attained
            else:
                ch = boxes[starts[lvl - 1] + i * B:starts[lvl - 1] + min((i + 1) * B, counts[lvl - 1])]
                assert np.array_equal(row[0:3], ch[:, 0:3].min(0)) and np.array_equal(row[4:7], ch[:, 4:7].max(0))     # the union
        span *= B


# ------------------------------------------------------------------ 3. skipping works

def test_skipping_cuts_the_pairs():
    """Mean pairs per point over the pushed samples and over the far points <= F_usable / 4 (a walk that never skips: F_usable)."""
    pts, fam = queries(None)
    usable = tree_of(None).usable
    counts = by_tree(None, np.float32)[3]
    finite = np.isfinite(pts).all(1)
    assert (counts[finite, 1] > 0).all() and (counts[:, 1] <= usable).all() and not counts[~finite].any()
    for name in ('pushed', 'far', 'vertices'):
        c = counts[fam[name]]
        print(f'{name}: mean boxes {c[:, 0].mean():.1f}, mean pairs {c[:, 1].mean():.1f}, most pairs {c[:, 1].max()} of {usable}')
    assert counts[fam['pushed'], 1].mean() <= usable / 4
    assert counts[fam['far'], 1].mean() <= usable / 4


# ------------------------------------------------------------------ 4. the slack only costs

@pytest.mark.parametrize('n', [L * B + 1, None])
def test_a_large_slack_changes_only_the_counts(n):
    pts, fam = queries(n)
    sel = np.r_[fam['pushed'], fam['far'], fam['rest']]
    tree = tree_of(n)
    a = geometry._closest_tree_numpy(pts[sel], tree, np.float32)
    b = geometry._closest_tree_numpy(pts[sel], tree, np.float32, slack=1e3)
    assert_same(b, a)
    assert (b[3] >= a[3]).all() and b[3][:, 1].sum() > a[3][:, 1].sum()
    near = np.arange(fam['pushed'].stop - fam['pushed'].start)
    assert (b[3][near, 1] == tree.usable).all()                                                        # nothing is skipped near the mesh


# ------------------------------------------------------------------ 5. a point's result is its own

@pytest.mark.parametrize('n', [L * B * B + 3, None])
def test_order_and_batching_change_no_bit(n):
    pts, fam = queries(n)
    sel = np.r_[fam['pushed'], fam['far'], fam['rest'], np.arange(fam['vertices'].start, fam['vertices'].stop, 16)]
    pts = pts[sel]
    tree = tree_of(n)
    whole = geometry._closest_tree_numpy(pts, tree, np.float32)
    perm = np.random.RandomState(4).permutation(pts.shape[0])
    shuffled = geometry._closest_tree_numpy(pts[perm], tree, np.float32)
    k = pts.shape[0] // 3
    halves = [geometry._closest_tree_numpy(part, tree, np.float32) for part in (pts[:k], pts[k:])]
    for i in range(4):
        assert same_bits(shuffled[i], whole[i][perm])
        assert same_bits(np.concatenate([halves[0][i], halves[1][i]]), whole[i])
    empty = geometry._closest_tree_numpy(np.zeros((0, 3), dtype=F32), tree, np.float32)
    assert [x.shape for x in empty] == [(0,), (0,), (0, 3), (0, 2)]


# ------------------------------------------------------------------ 6. the public interface

def test_closest_point_search_tree_on_the_host():
    verts, faces = cut(L * B + 1)
    faces = faces[(faces >= 0).all(1)]                                                                 # (the host route refuses indices out of range)
    pts, _ = queries(L * B + 1)
    want = geometry.closest_point(pts, verts, faces)
    tree = geometry.WindingTree(verts, faces)
    for got in (geometry.closest_point(pts, verts, faces, search='tree'), geometry.closest_point(pts, verts, faces, search='tree', tree=tree),
                tree.closest(pts)):
        assert set(got) == {'dist', 'face', 'point'}
        for k in want:
            assert same_bits(got[k], want[k])
    tv, tf, tp = torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(pts[:pts.shape[0] // 3 * 3]).reshape(3, -1, 3)
    got, want_t = geometry.closest_point(tp, tv, tf, search='tree'), geometry.closest_point(tp, tv, tf)
    for k in want_t:
        assert isinstance(got[k], torch.Tensor) and got[k].dtype == want_t[k].dtype and got[k].shape == want_t[k].shape
        assert same_bits(got[k].numpy(), want_t[k].numpy())
    counted = tree.closest(pts, return_counts=True)
    assert counted['counts'].shape == (pts.shape[0], 2) and counted['counts'].dtype == np.int64
    assert tree.info == {'faces': 256, 'usable': 256, 'levels': 2, 'nodes': 9, 'leaf': L, 'branch': B}          # (as before the boxes)


def test_argument_errors():
    verts, faces = sphere()
    pts = np.zeros((2, 3), dtype=F32)
    with pytest.raises(ValueError):
        geometry.closest_point(pts, verts, faces, search='tree', brute=True)
    for call in (lambda s: geometry.closest_point(pts, verts, faces, search=s), lambda s: geometry.signed_distance(pts, verts, faces, search=s),
                 lambda s: geometry.mesh_to_volume(verts, faces, 8, search=s), lambda s: geometry.volume_iou(verts, faces, verts, faces, 8, search=s),
                 lambda s: geometry.surface_distance(verts, faces, verts, faces, search=s),
                 lambda s: geometry.align_mesh(verts, verts, faces, search=s)):
        for bad in ('auto', 'brute', None):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError):
        geometry.closest_point(pts, verts, faces, search='tree', tree='tree')
    with pytest.raises(ValueError):
        geometry.closest_point(pts, verts, faces, tree=geometry.WindingTree(verts, faces))
    with pytest.raises(ValueError):
        geometry.closest_point(pts, verts, np.array([[0, 1, verts.shape[0]]]), search='tree')


@pytest.mark.parametrize('method', ['exact', 'tree'])
@pytest.mark.parametrize('make', [sphere, torus])
def test_signed_distance_is_the_grid_routes(make, method):
    verts, faces = make()
    pts, _ = pushed_samples(verts, faces)
    a = geometry.signed_distance(pts, verts, faces, method=method)
    b = geometry.signed_distance(pts, verts, faces, method=method, search='tree')
    assert set(a) == set(b)
    for k in a:
        assert same_bits(a[k], b[k]), k


def test_one_tree_serves_sign_and_magnitude(monkeypatch):
    built = []
    init = geometry.WindingTree.__init__
    monkeypatch.setattr(geometry.WindingTree, '__init__', lambda self, *a, **k: (built.append(1), init(self, *a, **k))[1])
    verts, faces = sphere()
    pts, _ = pushed_samples(verts, faces, 4)
    geometry.signed_distance(pts, verts, faces, method='tree', search='tree')
    assert len(built) == 1
    geometry.mesh_to_volume(verts, faces, 8, winding='tree', search='tree')
    assert len(built) == 2
    geometry.surface_distance(verts, faces, verts, faces, signed=True, winding='tree', search='tree')
    assert len(built) == 4                                                                             # one per mesh
    given = geometry.WindingTree(verts, faces)
    geometry.signed_distance(pts, verts, faces, method='tree', search='tree', tree=given)
    assert len(built) == 5


@pytest.mark.parametrize('make, winding', [(mc_sphere, 'exact'), (mc_sphere, 'tree'), (mc_torus, 'exact')])
def test_mesh_to_volume_is_the_grid_routes(make, winding):
    field, level, org, spc, verts, faces = make()
    assert field.shape == (24, 24, 24)
    a = geometry.mesh_to_volume(verts, faces, field.shape, origin=org, spacing=spc, winding=winding)
    b = geometry.mesh_to_volume(verts, faces, field.shape, origin=org, spacing=spc, winding=winding, search='tree')
    assert same_bits(a['sdf'], b['sdf']) and same_bits(a['inside'], b['inside']) and a['info'] == b['info']
    assert (a['origin'], a['spacing']) == (b['origin'], b['spacing'])
    if winding == 'exact':
        assert np.array_equal(b['inside'], field > F32(level))
        other = sphere(8, 12, 0.5, (0.1, 0.0, 0.0))
        i_a = geometry.volume_iou(verts, faces, *other, resolution=16)
        assert geometry.volume_iou(verts, faces, *other, resolution=16, search='tree') == i_a


def test_surface_distance_is_the_grid_routes():
    va, fa = uv_sphere(1.0, 8, 12)
    vb, fb = uv_sphere(1.05, 6, 10)
    vb = vb + np.array([4.0, 0.0, 0.5], dtype=F32)                                                     # (the meshes do not overlap)
    for kw in (dict(), dict(samples=200, seed=3), dict(signed=True), dict(signed=True, winding='tree')):
        assert geometry.surface_distance(va, fa, vb, fb, search='tree', **kw) == geometry.surface_distance(va, fa, vb, fb, **kw), kw


@pytest.mark.parametrize('init', ['identity', 'centroid'])
def test_align_mesh_is_the_grid_routes(init):
    c = shared_case(1.0)
    src = c.src if init == 'identity' else c.src + np.array([3.0, -2.0, 1.0], dtype=F32)              # (a start outside the target's box)
    a = geometry.align_mesh(src, c.verts, c.faces, iterations=6, init=init)
    b = geometry.align_mesh(src, c.verts, c.faces, iterations=6, init=init, search='tree')
    assert same_bits(a['matrix'], b['matrix']) and a['rms_history'] == b['rms_history'] and a['iterations'] == b['iterations']
    assert a['inliers'] == b['inliers'] and a['converged'] == b['converged']


def test_cli_search_tree(tmp_path):
    """``--search tree``: the same numbers, the same coloured mesh, and ``search`` in the JSON only then."""
    import json
    from invertavatar_amd import extract_geometry, geometry_metrics
    big, faces = sphere(8, 12, 1.05)
    unit, _ = sphere(8, 12)
    geometry.write_ply(str(tmp_path / 'a.ply'), big + np.array([3.0, 0.0, 0.0], dtype=F32), faces)    # (far from b: --align brings it back)
    geometry.write_ply(str(tmp_path / 'b.ply'), unit, faces)
    base = ['--pred', str(tmp_path / 'a.ply'), '--gt', str(tmp_path / 'b.ply'), '--device', 'cpu', '--signed', '--iou', '12', '--align', 'rigid',
            '--align-init', 'centroid', '--align-iterations', '4']
    grid = geometry_metrics.main(base + ['--out', str(tmp_path / 'g.json'), '--error-ply', str(tmp_path / 'g.ply')])
    tree = geometry_metrics.main(base + ['--out', str(tmp_path / 't.json'), '--error-ply', str(tmp_path / 't.ply'), '--search', 'tree'])
    assert 'search' not in grid and tree.pop('search') == 'tree' and tree == grid
    assert json.load(open(tmp_path / 't.json'))['search'] == 'tree' and 'search' not in json.load(open(tmp_path / 'g.json'))
    assert all(np.array_equal(a, b) for a, b in zip(geometry.read_ply(str(tmp_path / 'g.ply')), geometry.read_ply(str(tmp_path / 't.ply'))))
    with pytest.raises(SystemExit):
        geometry_metrics.main(base + ['--out', str(tmp_path / 'x.json'), '--search', 'auto'])
    import argparse
    ap = argparse.ArgumentParser()
    geometry_metrics.add_sign_arguments(ap)                                                            # what extract_geometry shares
    assert geometry_metrics.sign_options_of(ap.parse_args(['--search', 'tree'])) == {'search': 'tree'}
    assert geometry_metrics.sign_options_of(ap.parse_args([])) == {} and '--search' in extract_geometry.__doc__
