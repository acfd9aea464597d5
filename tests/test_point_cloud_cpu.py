"""Point clouds as targets, on the host: the tree restatement ``_nearest_tree_numpy`` against the definition
``_nearest_numpy`` bit for bit, ties and duplicates in index order, the admission rules, ``estimate_normals`` against direct float64
arithmetic and ``numpy.linalg.eigh``, ``align_mesh(faces=None)`` against its own float32 run, ``cloud_distance``, ``depth_to_points``
and a PLY file without faces.  Tolerances come from the arithmetic or from the restatement's own float32 run, never from the kernels."""
import numpy as np
import pytest
import torch

from invertavatar_amd import geometry
from point_cloud_cases import (CLOUD_SIZES, EPS64, KS, align_case, angle_to, cloud, direct_covariance, host_tree, lattice, queries,
                               reference32, same_bits, sym3, unit_sphere)
from test_align_cpu import bumpy_mesh
from test_surface_distance_cpu import EPS32, F32, extent_of


@pytest.mark.parametrize('n', CLOUD_SIZES)
def test_tree_restatement_equals_the_definition(n):
    """Bit for bit in float32, the same indices in float64; k > n pads; the k smallest are a prefix of the 32 smallest."""
    tree = host_tree(n)
    assert tree.info['usable'] == n and tree.counts == geometry._winding_levels(n)
    for kind in ('self', 'box', 'far'):
        q = queries(kind, min(65, n) if kind == 'self' else 65, n)
        for k in KS:
            ref = reference32(kind, q.shape[0], n, k)
            walk = geometry._nearest_tree_numpy(q, tree, k, dtype=np.float32)
            assert same_bits(walk[0], ref[0]) and same_bits(walk[1], ref[1]), (kind, k)
            assert ((ref[1] >= 0).sum(1) == min(k, n)).all() and np.isinf(ref[0][ref[1] < 0]).all()
        own = geometry._nearest_numpy(q, cloud(n), 3, dtype=np.float32)
        assert same_bits(own[0], reference32(kind, q.shape[0], n, 3)[0]) and same_bits(own[1], reference32(kind, q.shape[0], n, 3)[1])
        a, b = geometry._nearest_numpy(q, cloud(n), 8), geometry._nearest_tree_numpy(q, tree, 8)
        assert a[0].dtype == np.float64 and np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])


def test_indices_against_a_kd_tree():
    spatial = pytest.importorskip('scipy.spatial')
    pts, q = cloud(2049), queries('box', 1000)
    idx = spatial.cKDTree(pts.astype(np.float64)).query(q.astype(np.float64), k=8)[1]
    assert np.array_equal(geometry.nearest_points(q, pts, 8)['index'], idx)


def test_lattice_ties_and_duplicates_come_out_in_index_order():
    pts, q = lattice()
    tree = geometry.PointTree(pts)
    for k in (8, 32):
        dist, index = geometry._nearest_tree_numpy(q, tree, k, dtype=np.float32)
        ref = reference32('lattice', 0, 0, k)
        assert same_bits(dist, ref[0]) and same_bits(index, ref[1])
        tied = dist[:, 1:] == dist[:, :-1]
        assert tied.mean() > 0.5 and (np.diff(dist, axis=1) >= 0).all()
        assert (index[:, 1:][tied] > index[:, :-1][tied]).all()
    assert (dist[-512:, :8] == np.sqrt(F32(0.75))).all()                                  # a cell centre: its eight corners
    dup = np.concatenate([cloud(33), cloud(33)[::-1], cloud(33)])                          # point i = 65 - i = 66 + i
    r = geometry.nearest_points(cloud(33), dup, 3)
    i = np.arange(33)
    assert (r['dist'] == 0).all() and np.array_equal(r['index'], np.stack([i, 65 - i, 66 + i], 1).astype(np.int32))


def test_admission_rules():
    pts = cloud(257).copy()
    pts[[3, 40, 200]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    q = pts[:65].copy()
    q[7] = [0, np.nan, 0]
    r = geometry.nearest_points(q, pts, 4)
    assert r['dist'].dtype == np.float32 and r['index'].dtype == np.int32 and r['dist'].shape == (65, 4)
    assert not np.isin(r['index'], [3, 40, 200]).any()                                    # non-finite points are ignored
    assert np.isinf(r['dist'][[3, 7, 40]]).all() and (r['index'][[3, 7, 40]] == -1).all()  # a non-finite query
    ok = np.setdiff1d(np.arange(65), [3, 7, 40])
    assert np.array_equal(r['index'][ok, 0], ok) and (r['dist'][ok, 0] == 0).all()
    brute = geometry.nearest_points(q, pts, 4, brute=True)
    assert np.array_equal(brute['index'], r['index']) and np.array_equal(brute['dist'], r['dist'])
    ex = geometry.nearest_points(q, pts, 3, exclude_self=True)
    assert np.array_equal(ex['index'][ok], r['index'][ok, 1:]) and np.array_equal(ex['dist'][ok], r['dist'][ok, 1:])
    cut = float(np.median(r['dist'][ok, 2]))
    lim = geometry.nearest_points(q, pts, 4, max_dist=cut)
    keep = r['dist'] <= F32(cut)
    assert np.array_equal(lim['index'], np.where(keep, r['index'], -1)) and np.array_equal(lim['dist'], np.where(keep, r['dist'], np.inf))
    assert 0 < keep[ok].mean() < 1
    few = geometry.nearest_points(q[:5], pts[:2], 3, exclude_self=True)                    # one admissible point each for rows 0 and 1
    assert np.array_equal(few['index'][:2], [[1, -1, -1], [0, -1, -1]]) and (few['index'][2, :2] == [0, 1]).all()
    t = torch.from_numpy(pts)
    rt = geometry.nearest_points(torch.from_numpy(q), t, 4, tree=geometry.PointTree(t))
    assert isinstance(rt['dist'], torch.Tensor) and np.array_equal(rt['index'].numpy(), r['index'])
    cnt = geometry.nearest_points(q, pts, 4, return_counts=True)['counts']
    assert cnt.shape == (65, 2) and (cnt[ok, 1] >= 1).all() and (cnt[[3, 7, 40]] == 0).all()


def test_refusals_carry_messages():
    pts = cloud(33)
    for k in (0, 33, 2.5, True):
        with pytest.raises(ValueError, match='k must be'):
            geometry.nearest_points(pts, pts, k)
    with pytest.raises(ValueError, match=r'\[n,3\]'):
        geometry.nearest_points(pts[:, :2], pts)
    with pytest.raises(ValueError, match=r'\[n,3\]'):
        geometry.PointTree(pts.reshape(-1))
    with pytest.raises(ValueError, match='max_dist'):
        geometry.nearest_points(pts, pts, max_dist=-1.0)
    with pytest.raises(ValueError, match='PointTree of these points'):
        geometry.nearest_points(pts, pts, tree=host_tree(32))
    with pytest.raises(ValueError, match='orient'):
        geometry.estimate_normals(pts, orient='outward')
    with pytest.raises(ValueError, match='viewpoint'):
        geometry.estimate_normals(pts, orient='viewpoint')
    with pytest.raises(ValueError, match='mesh target'):
        geometry.align_mesh(pts, pts, init='global')
    with pytest.raises(ValueError, match='one row per target point'):
        geometry.align_mesh(pts, pts, normals=pts[:5])
    with pytest.raises(ValueError, match='no inside'):
        geometry.surface_distance(pts, None, pts, None, signed=True)


def test_normals_restatement_against_direct_arithmetic():
    pts = unit_sphere()
    k = 16
    index = geometry.nearest_points(pts, pts, k)['index']
    normal, variation, eig, cov = geometry._point_normals_numpy(pts, index)
    extent = extent_of(pts)
    assert np.abs(cov - direct_covariance(pts, index)).max() <= k * EPS64 * extent ** 2
    w, v = np.linalg.eigh(sym3(cov))
    trace = w.sum(1)
    assert (np.abs(eig - w) <= 64 * EPS64 * trace[:, None]).all()
    assert (np.diff(eig, axis=1) >= 0).all() and np.allclose(variation, eig[:, 0] / eig.sum(1), rtol=1e-6)
    assert angle_to(normal, v[:, :, 0]).max() <= 1e-6                                     # (gap (l1 - l0) / l2 is large on a sphere)
    lead = np.take_along_axis(normal, np.abs(normal).argmax(1)[:, None], 1)
    assert (lead > 0).all() and np.allclose(np.linalg.norm(normal, axis=1), 1, atol=1e-6)
    r = geometry.estimate_normals(pts, k, orient='centroid')
    assert r['normal'].dtype == np.float32 and r['eigenvalues'].dtype == np.float64 and r['covariance'].shape == (2000, 6)
    assert ((r['normal'] * pts).sum(1) > 0).all()                                         # every normal points away from the centre
    inward = geometry.estimate_normals(pts, k, orient='viewpoint', viewpoint=(0, 0, 0))['normal']
    assert np.array_equal(inward, -r['normal'])
    flat = np.zeros((40, 3), dtype=F32)
    flat[:20, 0] = np.arange(20)                                                          # 20 points on a line and 20 copies of one point
    z = geometry.estimate_normals(flat, 4)
    assert (z['normal'][20:] == 0).all() and (z['variation'][20:] == 0).all() and np.abs(z['variation'][:20]).max() < 1e-12
    two = geometry.estimate_normals(cloud(33)[:2], 16)
    assert (two['normal'] == 0).all()                                                     # fewer than three neighbours


def test_cloud_alignment_against_its_own_float32_run():
    c = align_case()
    for metric in ('point', 'plane'):
        r = geometry.align_mesh(c.src, c.target, metric=metric, iterations=12, normals=c.normals if metric == 'plane' else None)
        assert np.array_equal(r['matrix'], c.r64[metric]['matrix'])                        # the public call is the restatement
        print(f'{metric}: rms {r["rms_history"][0]:.3g} -> {r["rms"]:.3g} in {r["iterations"]} steps, |M - truth| = '
              f'{np.abs(r["matrix"] - c.truth).max():.3g}, e32 = {c.e32[metric]:.3g}, tolerance {c.tol[metric]:.3g}')
        assert r['rms'] < r['rms_history'][0] and r['inliers'] == 500
    plane = c.r64['plane']
    assert plane['rms'] < c.r64['point']['rms'] or plane['rms'] <= EPS32 * c.extent
    estimated = geometry.align_mesh(c.src, c.target, metric='plane', iterations=12)       # normals from estimate_normals(k=16)
    assert np.array_equal(estimated['matrix'], plane['matrix'])
    verts, faces = bumpy_mesh()
    a = geometry.align_mesh(c.src, verts, faces, iterations=3)
    b = geometry.align_mesh(c.src, verts, faces=faces, iterations=3, normals=None)
    assert np.array_equal(a['matrix'], b['matrix']) and a['rms_history'] == b['rms_history']


def test_cloud_distance_and_mixed_surface_distance():
    a = cloud(2049)
    same = geometry.cloud_distance(a, a)
    assert same['chamfer'] == 0 and same['hausdorff'] == 0 and same['chamfer_sq'] == 0 and same['fscore'] == [1.0, 1.0, 1.0]
    b = (a.astype(np.float64) + [0.01, -0.02, 0.005]).astype(F32)[:1500]
    r = geometry.cloud_distance(a, b, thresholds=[0.02, 0.05])
    d_ab = np.sqrt(((a[:, None].astype(np.float64) - b[None].astype(np.float64)) ** 2).sum(-1).min(1))
    d_ba = np.sqrt(((b[:, None].astype(np.float64) - a[None].astype(np.float64)) ** 2).sum(-1).min(1))
    tol = 4 * EPS32 * extent_of(a)
    assert abs(r['mean_ab'] - d_ab.mean()) <= tol and abs(r['mean_ba'] - d_ba.mean()) <= tol and abs(r['hausdorff'] - max(d_ab.max(), d_ba.max())) <= tol
    assert abs(r['chamfer'] - (d_ab.mean() + d_ba.mean()) / 2) <= tol and r['n_a'] == 2049 and r['n_b'] == 1500
    assert set(r) == set(geometry.surface_distance(*bumpy_mesh(), *bumpy_mesh()))
    verts, faces = bumpy_mesh()
    pts = geometry.sample_surface(verts, faces, 500, seed=1)[0]
    m = geometry.surface_distance(verts, faces, pts, None, thresholds=[0.01])
    assert m['mean_ba'] <= 4 * EPS32 * extent_of(verts)                                    # the samples lie on the mesh
    assert m['mean_ab'] == pytest.approx(geometry.nearest_points(verts, pts)['dist'].astype(np.float64).mean(), rel=1e-6)
    flip = geometry.surface_distance(pts, None, verts, faces, thresholds=[0.01])
    assert flip['mean_ab'] == m['mean_ba'] and flip['mean_ba'] == m['mean_ab'] and flip['precision'] == m['recall']
    out = geometry.remove_outliers(np.concatenate([a, [[5, 5, 5]]]).astype(F32), 8, 2.0)
    assert not out['keep'][-1] and out['keep'][:-1].mean() > 0.9 and out['mean_dist'].dtype == np.float64


def _camera(distance=2.7, focal=2.0):
    cam = np.eye(4)
    cam[2, 3] = -distance                                                                  # at (0, 0, -distance), looking along +z
    k = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]])
    return np.concatenate([cam.reshape(-1), k.reshape(-1)]).astype(F32)[None]


def _back_projection(depth, cam32, dtype):
    """o + t d per pixel with the unit ray K_res^-1 [i, j, 1] rotated into the world, in ``dtype``."""
    n, h, w = depth.shape
    c = cam32.astype(dtype)
    m, k = c[:, :16].reshape(-1, 4, 4), c[:, 16:25].reshape(-1, 3, 3).copy()
    k[:, :2] *= dtype(h)
    jj, ii = np.meshgrid(np.arange(h, dtype=dtype), np.arange(w, dtype=dtype), indexing='ij')
    pix = np.stack([ii, jj, np.ones_like(ii)], -1).reshape(-1, 3)
    d = np.einsum('nab,pb->npa', np.linalg.inv(k).astype(dtype), pix)
    d = np.einsum('nab,npb->npa', m[:, :3, :3], d)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    return (m[:, None, :3, 3] + depth.reshape(n, -1, 1).astype(dtype) * d).astype(dtype)


def _facing_sheet(n=7):
    """A triangulated sheet in the plane z = 0.25, turned by 20 degrees in that plane: every vertex has the same camera depth."""
    ax = np.linspace(-0.8, 0.8, n)
    x, y = np.meshgrid(ax, ax * 0.7, indexing='ij')
    c, s = np.cos(np.deg2rad(20.0)), np.sin(np.deg2rad(20.0))
    verts = np.stack([c * x - s * y, s * x + c * y, np.full_like(x, 0.25)], -1).reshape(-1, 3).astype(F32)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing='ij')
    a = (i * n + j).reshape(-1)
    faces = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)])
    return verts, faces


@pytest.mark.parametrize('shape', ['sheet', 'bumpy'])
def test_depth_to_points_lies_on_the_mesh(shape):
    """The points are held to ``4 e32 + eps32 extent`` of the float64 back-projection of the same depth image on both shapes, and of the
    mesh itself (``closest_point``) on the sheet.  The rasteriser snaps screen positions to 1/256 pixel, so on a slanted
    surface ITS depth leaves the mesh by about slope x pixel / 512, far above float32 rounding (4.4e-5 on the bumpy shape at 48^2, against
    a bound of 1.4e-6): the bound on the distance to the mesh is one on the back-projection only where the snap cannot change the depth,
    which is a surface of constant camera depth.  The bumpy shape's figure is printed."""
    verts, faces = _facing_sheet() if shape == 'sheet' else bumpy_mesh()
    cam = _camera()
    img = geometry.rasterize_mesh(verts, faces, cam, 48)
    mask = img['mask']
    assert mask.sum() > 200
    pts = geometry.depth_to_points(img['depth'], cam)
    assert pts.dtype == np.float32 and pts.shape == (int(mask.sum()), 3)
    p32, p64 = _back_projection(img['depth'], cam, np.float32), _back_projection(img['depth'], cam, np.float64)
    sel = mask.reshape(1, -1)
    e32 = float(np.abs(p32[sel].astype(np.float64) - p64[sel]).max())
    tol = 4 * e32 + EPS32 * extent_of(verts)
    d = geometry.closest_point(pts, verts, faces)['dist']
    print(f'depth_to_points ({shape}): {pts.shape[0]} points, largest distance to the mesh {d.max():.3g}, e32 = {e32:.3g}, tolerance {tol:.3g}')
    assert np.abs(pts.astype(np.float64) - p64[sel]).max() <= tol
    if shape == 'sheet':
        assert d.max() <= tol
    nchw = geometry.depth_to_points(torch.from_numpy(img['depth'])[:, None], torch.from_numpy(cam), torch.from_numpy(mask)[:, None])
    assert isinstance(nchw, torch.Tensor) and np.array_equal(nchw.numpy(), pts)


def test_command_line_takes_the_cloud_routes(tmp_path, capsys):
    import json
    from invertavatar_amd import geometry_metrics
    c = align_case()
    verts, faces = bumpy_mesh()
    none = np.zeros((0, 3), dtype=np.int64)
    geometry.write_ply(str(tmp_path / 'gt.ply'), c.target, none)
    geometry.write_ply(str(tmp_path / 'pred.ply'), c.src, none)
    geometry.write_ply(str(tmp_path / 'mesh.ply'), verts, faces)
    base = ['--gt', str(tmp_path / 'gt.ply'), '--out', str(tmp_path / 'out.json'), '--device', 'cpu']
    res = geometry_metrics.main(['--pred', str(tmp_path / 'pred.ply'), *base, '--align', 'rigid', '--align-metric', 'plane', '--normals-k', '16',
                                 '--align-iterations', '12'])
    saved = json.loads((tmp_path / 'out.json').read_text())
    assert saved['target'] == 'cloud' and saved['gt_faces'] == 0 and saved['chamfer'] == res['chamfer']
    assert np.array_equal(np.array(saved['alignment']['matrix']), c.r64['plane']['matrix'])
    assert res['mean_ab'] < res['alignment']['rms_before']
    mixed = geometry_metrics.main(['--pred', str(tmp_path / 'mesh.ply'), *base])
    assert mixed['target'] == 'cloud' and mixed['pred_faces'] == 1400 and mixed['mean_ba'] <= 4 * EPS32 * extent_of(verts)
    both = geometry_metrics.main(['--pred', str(tmp_path / 'mesh.ply'), '--gt', str(tmp_path / 'mesh.ply'), '--out', str(tmp_path / 'm.json'),
                                  '--device', 'cpu'])
    assert 'target' not in both
    for flags in (['--signed'], ['--iou', '16'], ['--fit-nonrigid'], ['--align', 'rigid', '--align-init', 'global']):
        with pytest.raises(SystemExit):
            geometry_metrics.main(['--pred', str(tmp_path / 'mesh.ply'), *base, *flags])
        assert 'needs a surface on both sides' in capsys.readouterr().err


def test_read_ply_without_a_face_element(tmp_path):
    pts = cloud(33)
    head = ['ply', 'format binary_little_endian 1.0', 'element vertex 33', 'property float x', 'property float y', 'property float z',
            'end_header']
    path = tmp_path / 'cloud.ply'
    path.write_bytes(('\n'.join(head) + '\n').encode('ascii') + pts.astype('<f4').tobytes())
    verts, faces, colors = geometry.read_ply(str(path))
    assert np.array_equal(verts, pts) and faces.shape == (0, 3) and faces.dtype == np.int64 and colors is None
    geometry.write_ply(str(path), pts, np.zeros((0, 3), dtype=np.int64))
    verts, faces, _ = geometry.read_ply(str(path))
    assert np.array_equal(verts, pts) and faces.shape == (0, 3)
