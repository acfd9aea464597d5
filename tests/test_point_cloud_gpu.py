"""Point clouds on the device (csrc/point_tree.hip) against the NumPy restatements: the tree tables exactly; ``nearest_points`` bit for
bit across the tree kernel, the all-pairs kernel, the float32 definition and any slabbing of the queries, for every cloud size at which
the tree changes shape; the walk's counts; ia_point_normals against the restated covariance and ``eigh``; ``align_mesh(faces=None)``,
``cloud_distance`` and ``surface_distance`` with a cloud against their host routes; unchanged bits with faces; the error paths."""
import ctypes

import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, geometry, hipops
from nonrigid_cases import bumped_ellipsoid
from point_cloud_cases import (CLOUD_SIZES, EPS64, KS, QUERY_COUNTS, align_case, angle_to, cloud, host_tree, lattice, queries, reference32,
                               same_bits, sym3, unit_sphere)
from test_align_cpu import bumpy_mesh, shared_case
from test_surface_distance_cpu import EPS32, F32, extent_of

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_trees = {}


def device_tree(n):
    if n not in _trees:
        _trees[n] = geometry.PointTree(dev(lattice()[0] if n == 'lattice' else cloud(n)))
    return _trees[n]


def routes(tree, q, k, ref, what):
    """Tree, all pairs, unsorted, slabs of 1 / 64 / all and a second run: every one the bits of ``ref``."""
    r = tree.nearest(q, k)
    assert r['dist'].dtype == torch.float32 and r['index'].dtype == torch.int32 and tuple(r['dist'].shape) == (q.shape[0], k)
    assert same_bits(r['dist'].cpu().numpy(), ref[0]) and same_bits(r['index'].cpu().numpy(), ref[1]), what
    for other in (tree.nearest(q, k, brute=True), tree.nearest(q, k, sort=False), tree.nearest(q, k)):
        assert torch.equal(other['dist'], r['dist']) and torch.equal(other['index'], r['index']), what
    for slab in (1, 64):
        if q.shape[0] > slab and (slab > 1 or q.shape[0] == 65):
            parts = [tree.nearest(q[s:s + slab], k) for s in range(0, q.shape[0], slab)]
            assert torch.equal(torch.cat([p['dist'] for p in parts]), r['dist']), (what, slab)
            assert torch.equal(torch.cat([p['index'] for p in parts]), r['index']), (what, slab)


@pytest.mark.parametrize('n', CLOUD_SIZES)
def test_nearest_points_same_bits_on_every_route(n):
    tree = device_tree(n)
    host = host_tree(n)
    assert tree.counts == host.counts and tree.usable == n
    assert np.array_equal(tree.order.cpu().numpy(), host.order)
    assert np.array_equal(tree.sorted[:, :3].cpu().numpy(), host.sorted)
    assert np.array_equal(tree.sorted[:, 3].contiguous().view(torch.int32).cpu().numpy(), host.order[:n])
    assert np.array_equal(tree.boxes.cpu().numpy(), host.boxes)
    for kind in ('self', 'box', 'far'):
        for count in QUERY_COUNTS:
            if kind == 'self' and count > n:
                continue
            if kind != 'box' and count == 1000 and n != 20000:
                continue                                                                   # (the long sets once per kind, on the largest cloud)
            q = dev(queries(kind, count, n))
            for k in KS:
                routes(tree, q, k, reference32(kind, count, n, k), (n, kind, count, k))
    pts = dev(cloud(n))
    by_call = geometry.nearest_points(pts[:65], pts, 3, exclude_self=True)
    ref = geometry._nearest_numpy(cloud(n)[:65], cloud(n), 3, exclude_self=True, dtype=np.float32)
    assert same_bits(by_call['dist'].cpu().numpy(), ref[0]) and same_bits(by_call['index'].cpu().numpy(), ref[1])
    cut = 0.2
    lim = tree.nearest(dev(queries('box', 65)), 8, max_dist=cut)
    ref = geometry._nearest_numpy(queries('box', 65), cloud(n), 8, max_dist=cut, dtype=np.float32)
    assert same_bits(lim['dist'].cpu().numpy(), ref[0]) and same_bits(lim['index'].cpu().numpy(), ref[1])


def test_lattice_ties_and_unusable_rows():
    pts, q = lattice()
    tree = device_tree('lattice')
    for k in KS:
        routes(tree, dev(q), k, reference32('lattice', 0, 0, k), ('lattice', k))
    bad = cloud(257).copy()
    bad[[3, 40, 200]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    qq = bad[:65].copy()
    qq[7] = [0, np.nan, 0]
    r = geometry.nearest_points(dev(qq), dev(bad), 4)
    ref = geometry._nearest_numpy(qq, bad, 4, dtype=np.float32)
    assert same_bits(r['dist'].cpu().numpy(), ref[0]) and same_bits(r['index'].cpu().numpy(), ref[1])
    assert bool(r['dist'][7].isinf().all()) and bool((r['index'][7] == -1).all())
    host = geometry.PointTree(bad)
    t = geometry.PointTree(dev(bad))
    assert t.usable == 254 and np.array_equal(t.order.cpu().numpy(), host.order) and np.array_equal(t.boxes.cpu().numpy(), host.boxes)
    empty = geometry.nearest_points(dev(qq), dev(np.full((5, 3), np.nan, dtype=F32)), 2)
    assert bool(empty['dist'].isinf().all()) and bool((empty['index'] == -1).all())
    none = geometry.nearest_points(dev(np.zeros((0, 3), dtype=F32)), dev(bad), 2)
    assert tuple(none['dist'].shape) == (0, 2)


def test_counts_of_the_walk():
    n = 20000
    tree, host = device_tree(n), host_tree(n)
    leaves = tree.counts[0]
    for kind in ('box', 'far'):
        q = queries(kind, 1000)
        for k in (1, 8):
            cnt = tree.nearest(dev(q), k, return_counts=True)['counts'].cpu().numpy()
            ref = geometry._nearest_tree_numpy(q, host, k, dtype=np.float32, return_counts=True)[2]
            assert np.array_equal(cnt, ref), (kind, k)
            assert (cnt[:, 1] < leaves).all() and (cnt[:, 1] >= 1).all() and (cnt[:, 0] >= 1).all()
            print(f'{kind} k={k}: leaves taken mean {cnt[:, 1].mean():.1f} max {cnt[:, 1].max()} of {leaves}; boxes mean {cnt[:, 0].mean():.1f}')


@pytest.mark.parametrize('shape', ['sphere', 'ellipsoid'])
def test_point_normals_against_the_restatement(shape):
    pts = unit_sphere() if shape == 'sphere' else np.ascontiguousarray(bumped_ellipsoid()[0], dtype=F32)
    k = 16
    index = geometry._nearest_numpy(pts, pts, k, dtype=np.float32)[1]                      # the device's table (float32), not the host's float64 one
    normal, variation, eig, cov = geometry._point_normals_numpy(pts, index)
    w, v = np.linalg.eigh(sym3(cov))
    assert ((w[:, 1] - w[:, 0]) / w[:, 2]).min() >= 0.05                                   # the smallest eigenvector is well defined
    e = float(angle_to(normal, v[:, :, 0]).max())
    r = geometry.estimate_normals(dev(pts), k)
    assert np.array_equal(geometry.nearest_points(dev(pts), dev(pts), k)['index'].cpu().numpy(), index)
    got = {key: x.cpu().numpy() for key, x in r.items()}
    extent = extent_of(pts)
    assert got['covariance'].dtype == np.float64 and np.abs(got['covariance'] - cov).max() <= k * EPS64 * extent ** 2
    err = float(angle_to(got['normal'], v[:, :, 0]).max())
    print(f'{shape}: n = {pts.shape[0]}, restatement to eigh e = {e:.3g}, device to eigh {err:.3g}, bound {4 * e + 2 * EPS32:.3g}')
    assert err <= 4 * e + 2 * EPS32
    assert np.abs(got['eigenvalues'] - w).max() <= 64 * EPS64 * w.sum(1).max() and np.abs(got['variation'] - variation).max() <= 2 * EPS32
    lead = np.take_along_axis(got['normal'], np.abs(got['normal']).argmax(1)[:, None], 1)
    assert (lead > 0).all()
    again = geometry.estimate_normals(dev(pts), k)
    assert all(torch.equal(again[key], r[key]) for key in r)
    out = geometry.estimate_normals(dev(pts), k, orient='centroid')['normal'].cpu().numpy()
    centre = pts.astype(np.float64).mean(0)
    assert ((out * (pts - centre)).sum(1) >= 0).all()


@pytest.mark.parametrize('metric', ['point', 'plane'])
def test_cloud_alignment_on_device(metric):
    c = align_case()
    nrm = dev(c.normals) if metric == 'plane' else None
    r = geometry.align_mesh(dev(c.src), dev(c.target), metric=metric, iterations=12, normals=nrm)
    err = float(np.abs(r['matrix'] - c.r64[metric]['matrix']).max())
    print(f'{metric}: {r["iterations"]} steps, rms {r["rms_history"][0]:.3g} -> {r["rms"]:.3g}; |M - restatement| = {err:.3g}, |M - truth| = '
          f'{np.abs(r["matrix"] - c.truth).max():.3g}, e32 = {c.e32[metric]:.3g}, tolerance {c.tol[metric]:.3g}')
    assert err <= c.tol[metric] and r['inliers'] == 500
    again = geometry.align_mesh(dev(c.src), dev(c.target), metric=metric, iterations=12, normals=nrm)
    assert np.array_equal(again['matrix'], r['matrix'])


def test_cloud_distances_match_the_host_routes():
    a = cloud(2049)
    b = (a.astype(np.float64) + [0.01, -0.02, 0.005]).astype(F32)[:1500]
    verts, faces = bumpy_mesh()
    pairs = [(geometry.cloud_distance(dev(a), dev(b)), geometry.cloud_distance(a, b)),
             (geometry.surface_distance(dev(verts), dev(faces), dev(b)), geometry.surface_distance(verts, faces, b)),
             (geometry.surface_distance(dev(b), None, dev(verts), dev(faces)), geometry.surface_distance(b, None, verts, faces))]
    for rd, rc in pairs:
        assert rd['precision'] == rc['precision'] and rd['recall'] == rc['recall'] and rd['thresholds'] == rc['thresholds']
        for key in ('mean_ab', 'rms_ab', 'max_ab', 'mean_ba', 'rms_ba', 'max_ba', 'chamfer', 'chamfer_sq', 'hausdorff'):
            assert abs(rd[key] - rc[key]) <= 1e-6, key
    zero = geometry.cloud_distance(dev(a), dev(a))
    assert zero['chamfer'] == 0 and zero['hausdorff'] == 0
    keep = geometry.remove_outliers(dev(np.concatenate([a, [[5, 5, 5]]]).astype(F32)), 8)
    host = geometry.remove_outliers(np.concatenate([a, [[5, 5, 5]]]).astype(F32), 8)
    assert np.array_equal(keep['keep'].cpu().numpy(), host['keep']) and not bool(keep['keep'][-1])


def test_calls_with_faces_keep_their_bits():
    c = shared_case(1.0)
    args = (dev(c.src), dev(c.verts), dev(c.faces))
    a = geometry.align_mesh(*args, metric='plane', iterations=6)
    b = geometry.align_mesh(args[0], args[1], faces=args[2], metric='plane', iterations=6, normals=None, normals_k=16)
    assert np.array_equal(a['matrix'], b['matrix']) and a['rms_history'] == b['rms_history']
    v2 = dev(c.verts * F32(1.01))
    sa = geometry.surface_distance(args[1], args[2], v2, args[2], samples=500)
    sb = geometry.surface_distance(args[1], args[2], v2, faces_b=args[2], samples=500)
    assert sa == sb and sa['normal_consistency'] is not None


def test_error_paths_go_through_last_error():
    lib = _lib.load()
    pts = dev(cloud(33))
    tree = geometry.PointTree(pts)
    dist, index = torch.empty(33, 4, device='cuda'), torch.empty(33, 4, dtype=torch.int32, device='cuda')

    def walk(q=pts.data_ptr(), n=33, s=tree.sorted.data_ptr(), m=33, boxes=tree.boxes.data_ptr(), nodes=tree.boxes.shape[0], k=4, lim=float('inf')):
        return lib.ia_nearest_points_tree(q, n, s, m, boxes, nodes, k, lim, None, dist.data_ptr(), index.data_ptr(), None, None)
    assert walk() == 0
    assert walk(k=0) == -1 and 'k must be in 1 .. 32' in _lib.last_error()
    assert walk(k=33) == -1 and 'k must be' in _lib.last_error()
    assert walk(nodes=7) == -1 and 'nodes' in _lib.last_error()
    assert walk(m=(1 << 25) + 1) == -1 and '2^25' in _lib.last_error()
    assert walk(n=(1 << 31) // 3) == -1 and '2^31' in _lib.last_error()
    assert walk(lim=float('nan')) == -1 and 'max_dist' in _lib.last_error()
    assert walk(q=torch.zeros(33, 3).data_ptr()) == -1 and 'device pointers' in _lib.last_error()
    assert lib.ia_nearest_points_brute(pts.data_ptr(), 33, tree.sorted.data_ptr(), 33, 40, float('inf'), None, dist.data_ptr(), index.data_ptr(),
                                       None) == -1 and 'ia_nearest_points_brute' in _lib.last_error()
    assert lib.ia_point_tree_boxes(tree.sorted.data_ptr(), 33, tree.boxes.data_ptr(), 1, None) == -1 and 'nodes' in _lib.last_error()
    assert lib.ia_point_tree_gather(pts.data_ptr(), 33, None, 34, tree.sorted.data_ptr(), None) == -1 and 'n_usable' in _lib.last_error()
    assert lib.ia_point_normals(pts.data_ptr(), 33, index.data_ptr(), 0, None, None, None, None, None) == -1 and 'k must be' in _lib.last_error()
    with pytest.raises(RuntimeError, match='k must be in 1 .. 32'):
        hipops.nearest_points(pts, tree.sorted, tree.boxes, 33)
    with pytest.raises(RuntimeError, match='int32'):
        hipops.nearest_points(pts, tree.sorted, tree.boxes, 1, exclude=torch.arange(33, device='cuda'))
    with pytest.raises(ValueError, match='both'):
        geometry.nearest_points(cloud(33), pts)
    assert ctypes.c_int(walk()).value == 0
