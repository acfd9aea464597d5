"""Closest point on the cluster tree on the device (csrc/closest_tree.hip) against the brute mode and the grid of ia_closest_point and
against the NumPy restatement (tests/test_closest_tree_cpu.py pins that against the brute restatement).  The tree only prunes, so the
device comparisons are on bits; the one tolerance, against float64, is the project's for this query."""
import functools

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry, hipops
from test_align_cpu import shared_case
from test_closest_tree_cpu import FACE_COUNTS, cut, queries, tree_of
from test_surface_distance_cpu import EPS32, F32
from test_winding_cpu import mc_sphere, pushed_samples, sphere

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    """dist as int32 views, face and point: the same bits."""
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(bits(a[k]), bits(b[k])) for k in ('dist', 'face', 'point'))


@functools.lru_cache(maxsize=None)
def built(n):
    verts, faces = cut(n)
    v, f = dev(verts), dev(faces)
    grid = geometry.TriangleGrid(v, f)
    return v, f, grid, geometry.WindingTree.from_grid(grid)


@pytest.mark.parametrize('n', FACE_COUNTS)
def test_boxes_are_the_restatements(n):
    _, _, grid, tree = built(n)
    host = tree_of(n)
    assert tree.counts == host.counts and tree.usable == host.usable and np.array_equal(tree.order.cpu().numpy(), host.order)
    boxes = tree.boxes
    assert boxes.dtype == torch.float32 and tuple(boxes.shape) == (sum(host.counts), hipops.TREE_BOX_ROW) and tree.boxes is boxes
    assert np.array_equal(boxes.cpu().numpy().view(np.int32), host.boxes.view(np.int32))
    again = geometry.WindingTree.from_grid(grid)                                                       # run to run: the same bits
    assert torch.equal(again.boxes.view(torch.int32), boxes.view(torch.int32))
    assert tree.info == host.info


@pytest.mark.parametrize('n', FACE_COUNTS)
def test_tree_is_brute_and_grid_bit_for_bit(n):
    v, f, grid, tree = built(n)
    pts = dev(queries(n)[0])
    brute = geometry.closest_point(pts, v, f, brute=True)
    by_grid = geometry.closest_point(pts, v, f)
    by_tree = geometry.closest_point(pts, v, f, search='tree')
    assert by_tree['face'].dtype == torch.int64 and same(by_tree, brute) and same(by_tree, by_grid)
    assert same(geometry.closest_point(pts, v, f, grid=grid, search='tree', tree=tree), brute)
    assert same(tree.closest(pts, sort=False), brute) and same(tree.closest(pts, sort=True), brute)
    perm = torch.from_numpy(np.random.RandomState(n or 7).permutation(pts.shape[0])).to(DEV)
    for sort in (True, False):
        shuffled = tree.closest(pts[perm], sort=sort)
        assert all(torch.equal(bits(shuffled[k]), bits(brute[k][perm])) for k in brute)
    for m in (0, 1, 63, 64, 65):
        part = tree.closest(pts[-m:] if m else pts[:0])
        assert all(torch.equal(bits(part[k]), bits(brute[k][pts.shape[0] - m:])) for k in brute) and part['dist'].shape == (m,)
    nan = torch.isnan(pts).any(1)
    assert int(nan.sum()) == 1 and torch.isnan(by_tree['dist'][nan]).all() and (by_tree['face'][nan] == -1).all()
    if not tree.usable:
        assert torch.isinf(by_tree['dist'][~nan]).all() and (by_tree['face'] == -1).all() and torch.isnan(by_tree['point']).all()


@pytest.mark.parametrize('n', FACE_COUNTS)
def test_within_the_float32_tolerance_of_float64(n):
    """|dist - dist64| <= 4 e32 + eps32 extent, e32 = the restatement's own float32 deviation on the same inputs."""
    v, f, _, tree = built(n)
    pts = queries(n)[0]
    ok = np.isfinite(pts).all(1) & (np.abs(pts).max(1) < 1e20)                                         # (1e30: +inf in float32, finite in float64)
    host = tree_of(n)
    d64 = geometry._closest_tree_numpy(pts[ok], host, np.float64)[0]
    d32 = geometry._closest_tree_numpy(pts[ok], host, np.float32)[0].astype(np.float64)
    got = tree.closest(dev(pts[ok]))['dist'].cpu().numpy().astype(np.float64)
    if not host.usable:
        assert np.isinf(got).all() and np.isinf(d64).all()
        return
    extent = np.maximum(np.abs(pts[ok]).max(1), host.extent).astype(np.float64)
    e32 = float(np.abs(d32 - d64).max())
    ratio = np.abs(got - d64) / (4 * e32 + EPS32 * extent)
    print(f'F = {n}: e32 = {e32:.3g}, largest error / tolerance = {ratio.max():.3g}')
    assert (ratio <= 1).all()


def test_counts_on_the_full_mesh():
    """0 < pairs <= F_usable for every finite point; the mean pairs over the pushed samples, and over the far points, <= F_usable / 4."""
    _, _, _, tree = built(None)
    pts, fam = queries(None)
    res = tree.closest(dev(pts), return_counts=True)
    counts = res['counts'].cpu().numpy()
    assert counts.dtype == np.int32 and counts.shape == (pts.shape[0], 2)
    ref = geometry._closest_tree_numpy(pts, tree_of(None), np.float32)[3]
    finite = np.isfinite(pts).all(1)
    assert (counts[finite, 1] > 0).all() and (counts[:, 1] <= tree.usable).all() and not counts[~finite].any()
    for name in ('pushed', 'far', 'vertices'):
        c, r = counts[fam[name]], ref[fam[name]]
        print(f'{name}: device mean boxes {c[:, 0].mean():.1f} pairs {c[:, 1].mean():.1f}; restatement mean boxes {r[:, 0].mean():.1f} '
              f'pairs {r[:, 1].mean():.1f}; of {tree.usable} usable faces; points whose counts differ: {int((c != r).any(1).sum())}')
    assert counts[fam['pushed'], 1].mean() <= tree.usable / 4
    assert counts[fam['far'], 1].mean() <= tree.usable / 4
    unsorted = tree.closest(dev(pts), return_counts=True, sort=False)['counts'].cpu().numpy()
    assert np.array_equal(unsorted, counts)                                                            # a point's counts are its own


def test_callers_with_search_tree_are_their_grid_routes(monkeypatch):
    built_trees = []
    init = geometry.WindingTree.__init__
    monkeypatch.setattr(geometry.WindingTree, '__init__', lambda self, *a, **k: (built_trees.append(1), init(self, *a, **k))[1])
    verts, faces = sphere()
    pts, _ = pushed_samples(verts, faces)
    v, f, p = dev(verts), dev(faces), dev(pts)
    a = geometry.signed_distance(p, v, f, method='tree')
    del built_trees[:]
    b = geometry.signed_distance(p, v, f, method='tree', search='tree')
    assert len(built_trees) == 1                                                                       # one tree: sign and magnitude
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a) and same(a, b)
    field, level, org, spc, mv, mf = mc_sphere()
    mv, mf = dev(mv), dev(mf)
    a = geometry.mesh_to_volume(mv, mf, field.shape, origin=org, spacing=spc, winding='tree')
    del built_trees[:]
    b = geometry.mesh_to_volume(mv, mf, field.shape, origin=org, spacing=spc, winding='tree', search='tree')
    assert len(built_trees) == 1 and tuple(b['sdf'].shape) == (24, 24, 24)
    assert torch.equal(bits(a['sdf']), bits(b['sdf'])) and torch.equal(a['inside'], b['inside']) and a['info'] == b['info']
    assert np.array_equal(b['inside'].cpu().numpy(), field > F32(level))
    sa = geometry.surface_distance(v, f, mv, mf, signed=True, winding='tree')
    assert geometry.surface_distance(v, f, mv, mf, signed=True, winding='tree', search='tree') == sa


def test_align_mesh_with_search_tree_is_its_grid_route():
    c = shared_case(1.0)
    assert c.verts.shape[0] == 702
    src = dev(c.src + np.array([3.0, -2.0, 1.0], dtype=F32))                                           # a start outside the target's box
    v, f = dev(c.verts), dev(c.faces)
    a = geometry.align_mesh(src, v, f, iterations=8, init='centroid')
    b = geometry.align_mesh(src, v, f, iterations=8, init='centroid', search='tree')
    print(f'{b["iterations"]} steps, rms {b["rms_history"]}')
    assert np.array_equal(a['matrix'].view(np.int64), b['matrix'].view(np.int64)) and a['rms_history'] == b['rms_history']
    assert a['iterations'] == b['iterations'] and a['inliers'] == b['inliers'] and a['converged'] == b['converged']


def test_error_paths():
    v, f, grid, tree = built(geometry.WINDING_LEAF + 1)
    pts = dev(queries(geometry.WINDING_LEAF + 1)[0])
    with pytest.raises(ValueError):
        geometry.closest_point(pts, v, f, search='tree', brute=True)
    with pytest.raises(ValueError):
        geometry.closest_point(pts, v, f, search='auto')
    with pytest.raises(ValueError):
        geometry.closest_point(pts, v, f, search='tree', tree=tree_of(geometry.WINDING_LEAF + 1))      # a host tree for a device mesh
    order = tree.order.int().contiguous()
    with pytest.raises(RuntimeError):
        hipops.closest_point_tree(pts, tree.tris, tree.order, tree.boxes, tree.usable, tree.extent)     # int64 order
    with pytest.raises(RuntimeError):
        hipops.closest_point_tree(pts, tree.tris, order, tree.boxes[:-1].contiguous(), tree.usable, tree.extent)   # a node short
    with pytest.raises(RuntimeError):
        hipops.closest_point_tree(pts, tree.tris, order, tree.boxes, tree.tris.shape[0] + 1, tree.extent)
    with pytest.raises(RuntimeError):
        hipops.tree_boxes(tree.tris, tree.usable, tree.boxes.shape[0] + 1)
    torch.cuda.synchronize()
