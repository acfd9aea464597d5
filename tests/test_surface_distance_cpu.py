"""Surface distance without a GPU: the NumPy restatement of the point-to-triangle function against hand-computed answers, degenerate
and non-finite inputs, scipy's k-d tree, analytic shapes and marching-cubes spheres; the float32 run of the restatement against its
float64 run on the hard triangle families (the condition that caps the device tolerance); ``sample_surface``, ``surface_distance`` and the
command line.  The helpers here also serve tests/test_surface_distance_gpu.py."""
import json

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------ shapes

def cube_mesh(lo=(0.0, 0.0, 0.0), size=(1.0, 1.0, 1.0)):
    """A box as 8 vertices and 12 outward-wound triangles."""
    c = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=F32)
    verts = (np.array(lo, dtype=F32) + c * np.array(size, dtype=F32)).astype(F32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c_, d in quads for t in ((a, b, c_), (a, c_, d))], dtype=np.int64)
    return verts, faces


def uv_sphere(r, n_lat=24, n_lon=48):
    """A closed latitude-longitude tessellation with every vertex on the sphere of radius r (float64 vertices rounded to fp32)."""
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones_like(ph))], -1)
    verts = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) * r
    idx = lambda i, j: 1 + i * n_lon + j % n_lon          # noqa: E731
    faces = []
    for j in range(n_lon):
        faces.append((0, idx(0, j), idx(0, j + 1)))
        faces.append((len(verts) - 1, idx(n_lat - 2, j + 1), idx(n_lat - 2, j)))
        for i in range(n_lat - 2):
            faces += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return verts.astype(F32), np.array(faces, dtype=np.int64)


def radial_volume(n, radius_field=1.0, length=2.4):
    """v = radius_field - |x| on an n^3 lattice over [-length/2, length/2]^3: {v > level} is the ball of radius radius_field - level."""
    ax, lo, step = geometry.lattice_axis(n, length, 0.0)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1).astype(np.float64)
    return (radius_field - np.linalg.norm(g, axis=-1)).astype(F32), float(lo), float(step)


def sphere_mc(n, level=0.0):
    vol, lo, step = radial_volume(n)
    v, f = geometry.marching_cubes(vol, level, (lo,) * 3, (step,) * 3)
    return v, f, step


def random_soup(rs, n_tris, clustered=False, degenerate=0.01, slivers=0.02, nans=0.005):
    """A triangle soup in about [-1, 1]^3 with some triangles collapsed to points / segments, some slivers and some with a NaN vertex."""
    if clustered:
        centres = rs.uniform(-1, 1, (max(1, n_tris // 50), 3))
        base = centres[rs.randint(0, len(centres), n_tris)]
        tri = base[:, None, :] + rs.normal(0, 0.02, (n_tris, 3, 3))
    else:
        tri = rs.uniform(-1, 1, (n_tris, 1, 3)) + rs.normal(0, 0.1, (n_tris, 3, 3))
    u = rs.rand(n_tris)
    pt = u < degenerate / 2
    tri[pt, 1], tri[pt, 2] = tri[pt, 0], tri[pt, 0]
    sg = (u >= degenerate / 2) & (u < degenerate)
    tri[sg, 2] = tri[sg, 1]
    sl = (u >= degenerate) & (u < degenerate + slivers)
    t = rs.rand(n_tris, 1)
    tri[sl, 2] = (tri[:, 0] + t * (tri[:, 1] - tri[:, 0]) + rs.normal(0, 1e-6, (n_tris, 3)))[sl]
    verts = tri.reshape(-1, 3).astype(F32)
    bad = np.flatnonzero((u >= degenerate + slivers) & (u < degenerate + slivers + nans))
    verts[3 * bad + rs.randint(0, 3, bad.size), rs.randint(0, 3, bad.size)] = np.nan
    return verts, np.arange(3 * n_tris, dtype=np.int64).reshape(-1, 3)


def families(rs, n_tris=400, n_pts=500):
    """The triangle families of the accuracy condition: name -> (points [n,3], triangles [m,3,3]), float32."""
    A = rs.uniform(-1, 1, (n_tris, 3))
    B, C = A + rs.normal(0, 0.3, (n_tris, 3)), A + rs.normal(0, 0.3, (n_tris, 3))
    well = np.stack([A, B, C], 1)
    box_pts = rs.uniform(-1, 1, (n_pts, 3))
    w = rs.dirichlet((1, 1, 1), n_pts)
    own = well[rs.randint(0, n_tris, n_pts)]
    on = (w[:, :, None] * own).sum(1)
    nrm = np.cross(own[:, 1] - own[:, 0], own[:, 2] - own[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    t = rs.rand(n_tris, 1)
    sliver = np.stack([A, B, A + t * (B - A) + rs.normal(0, 1e-6, (n_tris, 3))], 1)
    collinear = np.stack([A, B, A + (2 * t - 0.5) * (B - A)], 1)
    corners = np.sign(rs.uniform(-1, 1, (n_tris, 3, 3))) + rs.normal(0, 0.01, (n_tris, 3, 3))
    fam = {'well-shaped': (box_pts, well), 'on-surface': (on, well), 'just-above': (on + 1e-6 * nrm, well), 'sliver': (box_pts, sliver),
           'collinear': (box_pts, collinear), 'one-point': (box_pts, np.stack([A, A, A], 1)), 'far-away': (20.0 * box_pts, well),
           'box-sized': (box_pts, corners)}
    return {k: (p.astype(F32), tr.astype(F32)) for k, (p, tr) in fam.items()}


def extent_of(*arrays):
    return max(float(np.abs(a[np.isfinite(a)]).max()) if np.isfinite(a).any() else 0.0 for a in arrays)


def restatement_error(points, verts, faces):
    """(d64, f64, e32): the float64 restatement and the largest deviation of its float32 run over the per-point minima."""
    d64, f64, _ = geometry._closest_numpy(points, verts, faces, np.float64)
    d32, _, _ = geometry._closest_numpy(points, verts, faces, np.float32)
    both = np.isfinite(d64) & np.isfinite(d32)
    assert np.array_equal(np.isnan(d64), np.isnan(d32)) and np.array_equal(np.isinf(d64), np.isinf(d32))
    return d64, f64, float(np.abs(d32[both].astype(np.float64) - d64[both]).max()) if both.any() else 0.0


# ------------------------------------------------------------------ one triangle

TRI = (np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], dtype=F32), np.array([[0, 1, 2]]))


def single_triangle_cases():
    """(point, distance, closest point) for the seven regions of the right triangle (0,0,0), (4,0,0), (0,3,0), above and below."""
    cases = []
    for h in (2.0, -2.0):
        cases += [((1, 1, h), abs(h), (1, 1, 0)),                                           # interior
                  ((2, -1, h), np.hypot(1, h), (2, 0, 0)),                                   # edge AB
                  ((-2, 1, h), np.hypot(2, h), (0, 1, 0)),                                   # edge CA
                  ((2 + 3, 1.5 + 4, h), np.hypot(5, h), (2, 1.5, 0)),                         # hypotenuse, 5 along its normal (3,4)/5
                  ((-1, -1, h), np.sqrt(2 + h * h), (0, 0, 0)),                               # vertex A
                  ((6, -1, h), np.sqrt(4 + 1 + h * h), (4, 0, 0)),                            # vertex B
                  ((-1, 5, h), np.sqrt(1 + 4 + h * h), (0, 3, 0))]                            # vertex C
    return cases


def test_single_triangle_all_regions():
    pts = np.array([c[0] for c in single_triangle_cases()], dtype=F32)
    r = geometry.closest_point(pts, *TRI)
    assert r['dist'].dtype == F32 and r['face'].dtype == np.int64 and r['point'].shape == (14, 3)
    for k, (_, d, q) in enumerate(single_triangle_cases()):
        assert abs(r['dist'][k] - d) <= 2 * EPS32 * 8 and r['face'][k] == 0
        assert np.abs(r['point'][k] - np.array(q)).max() <= 2 * EPS32 * 8
    on = geometry.closest_point(np.array([[1, 1, 0], [2, 0, 0], [4, 0, 0], [2, 1.5, 0]], dtype=F32), *TRI)
    assert (on['dist'] == 0).all()
    t = geometry.closest_point(torch.tensor([[1.0, 1.0, 2.0]]), torch.from_numpy(TRI[0]), torch.from_numpy(TRI[1]))
    assert isinstance(t['dist'], torch.Tensor) and t['dist'].tolist() == [2.0] and t['face'].tolist() == [0]


def test_degenerate_and_non_finite_inputs():
    p = np.array([[1, 2, 2], [0.5, 1, 0], [3, 0, 4]], dtype=F32)
    one = np.array([[0, 0, 0]] * 3, dtype=F32)
    r = geometry.closest_point(p, one, np.array([[0, 1, 2]]))
    assert np.allclose(r['dist'], np.linalg.norm(p, axis=1), rtol=1e-7) and not np.isnan(r['point']).any()
    seg = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=F32)                     # collinear: the segment [0, 2] on x
    for faces in ([[0, 1, 2]], [[0, 2, 1]], [[1, 0, 2]], [[0, 2, 2]]):
        r = geometry.closest_point(p, seg, np.array(faces))
        assert np.allclose(r['dist'], [np.sqrt(8), 1.0, np.sqrt(17)], rtol=1e-7), faces
        assert np.allclose(r['point'], [[1, 0, 0], [0.5, 0, 0], [2, 0, 0]], atol=1e-7)
    # a NaN vertex drops its triangle (and only that one); an inf vertex too
    v = np.concatenate([TRI[0], [[np.nan, 0, 0], [0, 0, 9], [1, 0, 9], [np.inf, 1, 9]]]).astype(F32)
    f = np.array([[3, 4, 5], [0, 1, 2], [4, 5, 6]])
    r = geometry.closest_point(np.array([[1, 1, 8]], dtype=F32), v, f)
    assert r['face'].tolist() == [1] and r['dist'].tolist() == [8.0]
    # a NaN query; an empty mesh; a mesh of unusable triangles only
    r = geometry.closest_point(np.array([[np.nan, 0, 0], [1, 1, 1], [0, np.inf, 0]], dtype=F32), *TRI)
    assert np.isnan(r['dist'][[0, 2]]).all() and r['face'].tolist() == [-1, 0, -1] and r['dist'][1] == 1.0
    for vv, ff in ((np.zeros((0, 3), dtype=F32), np.zeros((0, 3), dtype=np.int64)), (v, f[:1])):
        r = geometry.closest_point(p, vv, ff)
        assert np.isposinf(r['dist']).all() and (r['face'] == -1).all() and np.isnan(r['point']).all()
    # equal distances: the lowest index
    dup = np.array([[0, 1, 2], [0, 1, 2], [2, 0, 1]])
    assert geometry.closest_point(p, TRI[0], dup)['face'].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        geometry.closest_point(p, TRI[0], np.array([[0, 1, 3]]))


def test_against_kd_tree_of_the_vertices():
    from scipy.spatial import cKDTree
    rs = np.random.RandomState(3)
    verts = rs.uniform(-1, 1, (400, 3)).astype(F32)
    faces = rs.randint(0, 400, (700, 3))
    pts = rs.uniform(-1.5, 1.5, (600, 3)).astype(F32)
    d = geometry._closest_numpy(pts, verts, faces)[0]
    dv, _ = cKDTree(verts[np.unique(faces)].astype(np.float64)).query(pts.astype(np.float64))
    assert (d <= dv).all()                                            # the vertices are points of the mesh
    assert (d < dv - 1e-3).mean() > 0.5                               # and most points are closer to an edge or a face
    points_only = np.repeat(np.arange(400)[:, None], 3, 1)
    d, f, q = geometry._closest_numpy(pts, verts, points_only)
    dv, iv = cKDTree(verts.astype(np.float64)).query(pts.astype(np.float64))
    assert np.abs(d - dv).max() <= 4 * np.finfo(np.float64).eps * 3 and np.array_equal(f, iv)


def test_shifted_cubes_and_inscribed_sphere():
    s = 0.25
    a, b = cube_mesh(), cube_mesh(lo=(s, 0.0, 0.0))
    r = geometry.surface_distance(*a, *b)
    assert r['hausdorff'] == s and r['max_ab'] == s and r['max_ba'] == s and r['n_a'] == r['n_b'] == 8
    assert r['mean_ab'] == s / 2 and r['chamfer'] == s / 2 and r['chamfer_sq'] == s * s          # 4 of 8 vertices lie on the other cube
    assert r['normal_consistency'] is None
    r = geometry.surface_distance(*a, *b, thresholds=[0.1, 0.25, 0.3])
    assert r['precision'] == [0.5, 1.0, 1.0] and r['recall'] == [0.5, 1.0, 1.0] and r['fscore'] == [0.5, 1.0, 1.0]
    # a tessellation inscribed in the sphere of radius r, seen from the sphere of radius R: |x|^2 >= r^2 - L^2 / 3 for every point x of a
    # triangle with its vertices on the sphere and edges <= L, so the distances lie in [R - r, R - r + sag]
    rad, big = 1.0, 1.5
    verts, faces = uv_sphere(rad)
    edges = np.concatenate([verts[faces[:, i]] - verts[faces[:, (i + 1) % 3]] for i in range(3)]).astype(np.float64)
    longest = np.linalg.norm(edges, axis=1).max()
    sag = rad - np.sqrt(rad * rad - longest * longest / 3)
    assert 0 < sag < 0.01
    rs = np.random.RandomState(5)
    y = rs.normal(size=(2000, 3))
    y = (big * y / np.linalg.norm(y, axis=1, keepdims=True)).astype(F32)
    d = geometry.closest_point(y, verts, faces)['dist'].astype(np.float64)
    tol = 8 * EPS32 * big
    assert d.min() >= big - rad - tol and d.max() <= big - rad + sag + tol
    assert d.max() > big - rad + 0.05 * sag                           # the bound is not idle


def test_surface_distance_identities():
    verts, faces = cube_mesh(size=(1.0, 2.0, 3.0))
    zero = geometry.surface_distance(verts, faces, verts, faces)
    for k in ('mean_ab', 'rms_ab', 'max_ab', 'mean_ba', 'rms_ba', 'max_ba', 'chamfer', 'chamfer_sq', 'hausdorff'):
        assert zero[k] == 0.0, k
    assert zero['fscore'] == [1.0, 1.0, 1.0] and len(zero['thresholds']) == 3
    diag = np.sqrt(14.0)
    assert np.allclose(zero['thresholds'], [0.005 * diag, 0.01 * diag, 0.02 * diag], rtol=1e-6)
    sampled = geometry.surface_distance(verts, faces, verts, faces, samples=3000, seed=4)
    assert sampled['hausdorff'] <= 8 * EPS32 * 3 and sampled['fscore'] == [1.0, 1.0, 1.0] and sampled['n_a'] == 3000
    assert abs(sampled['normal_consistency'] - 1.0) <= 1e-6
    # swapping the meshes swaps the directions, precision and recall
    sv, sf, _ = sphere_mc(20)
    thr = [0.02, 0.05, 0.1, 0.3, 5.0]
    ab = geometry.surface_distance(verts - F32(0.5), faces, sv, sf, thresholds=thr)
    ba = geometry.surface_distance(sv, sf, verts - F32(0.5), faces, thresholds=thr)
    for k in ('mean', 'rms', 'max'):
        assert ab[f'{k}_ab'] == ba[f'{k}_ba'] and ab[f'{k}_ba'] == ba[f'{k}_ab']
    assert ab['precision'] == ba['recall'] and ab['recall'] == ba['precision'] and ab['fscore'] == ba['fscore']
    assert ab['chamfer'] == ba['chamfer'] and ab['hausdorff'] == ba['hausdorff'] and ab['hausdorff'] > 0.3
    for key in ('precision', 'recall', 'fscore'):
        assert all(x <= y for x, y in zip(ab[key], ab[key][1:])), key                    # monotone in the threshold
    assert ab['fscore'][-1] == 1.0 and ab['fscore'][0] < 1.0
    # points given by the caller
    pts = np.array([[0.5, 1.0, 4.0], [0.5, 1.0, -2.0]], dtype=F32)
    r = geometry.surface_distance(verts, faces, verts, faces, points_a=pts, points_b=pts[:1])
    assert r['max_ab'] == 2.0 and r['mean_ab'] == 1.5 and r['max_ba'] == 1.0 and r['n_a'] == 2 and r['n_b'] == 1
    with pytest.raises(ValueError):
        geometry.surface_distance(verts, faces, verts, faces, thresholds=list(range(9)))


def test_sample_surface_lies_on_the_faces_and_follows_the_areas():
    from scipy import stats
    verts, faces = cube_mesh(size=(1.0, 2.0, 3.0))
    n = 60000
    pts, idx = geometry.sample_surface(verts, faces, n, seed=11)
    assert pts.dtype == F32 and pts.shape == (n, 3) and idx.shape == (n,) and idx.min() >= 0 and idx.max() < 12
    tri = verts[faces[idx]].astype(np.float64)
    d, _ = geometry.point_triangle(pts.astype(np.float64), tri[:, 0], tri[:, 1], tri[:, 2])
    assert d.max() <= 4 * EPS32 * 3
    area = 0.5 * np.linalg.norm(np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]]), axis=1)
    expect = n * area / area.sum()
    chi2 = (((np.bincount(idx, minlength=12) - expect) ** 2) / expect).sum()
    assert chi2 <= stats.chi2.ppf(1 - 1e-6, df=11), chi2                                # 12 bins, 11 degrees of freedom
    again, idx2 = geometry.sample_surface(verts, faces, n, seed=11)
    assert np.array_equal(again, pts) and np.array_equal(idx2, idx)
    other, _ = geometry.sample_surface(verts, faces, n, seed=12)
    assert not np.array_equal(other, pts)
    tp, ti = geometry.sample_surface(torch.from_numpy(verts), torch.from_numpy(faces), n, seed=11)
    assert torch.equal(tp, torch.from_numpy(pts)) and torch.equal(ti, torch.from_numpy(idx))
    nrm = geometry.face_normals(verts, faces)
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1) and np.allclose(np.abs(nrm).max(1), 1)
    centre = verts.mean(0)
    assert ((verts[faces[:, 0]] - centre) * nrm).sum(1).min() > 0                        # outward
    assert (geometry.face_normals(verts, np.array([[0, 0, 1]])) == 0).all()
    with pytest.raises(ValueError):
        geometry.sample_surface(verts, np.array([[0, 0, 1]]), 10)


def test_marching_cubes_spheres():
    n = 28
    v0, f0, step = sphere_mc(n, 0.0)                                                     # radius 1.0
    v1, f1, _ = sphere_mc(n, 0.2)                                                        # radius 0.8
    r = geometry.surface_distance(v0, f0, v1, f1)
    assert abs(r['mean_ab'] - 0.2) <= step and abs(r['mean_ba'] - 0.2) <= step and abs(r['chamfer'] - 0.2) <= step
    v2, f2, step2 = sphere_mc(2 * n, 0.0)
    assert step2 < step
    r = geometry.surface_distance(v0, f0, v2, f2, points_a=v0[::3], points_b=v2[::12])
    assert 0 < r['chamfer'] < step and r['hausdorff'] < step


def test_float32_restatement_stays_within_16_eps_of_float64():
    """The condition on the per-triangle form (not a measurement): on every family, every point-triangle pair of the float32 run is
    within 16 eps32 * extent of the float64 run, and nothing is NaN."""
    fam = families(np.random.RandomState(17))
    assert len(fam) == 8
    for name, (pts, tri) in fam.items():
        d64, _ = geometry.point_triangle(pts[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], np.float64)
        d32, q32 = geometry.point_triangle(pts[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], np.float32)
        assert d32.dtype == F32 and not np.isnan(d32).any() and not np.isnan(d64).any() and not np.isnan(q32).any()
        extent = extent_of(pts, tri)
        err = np.abs(d32.astype(np.float64) - d64)
        worst, worst_min = err.max() / (EPS32 * extent), np.abs(d32.min(1).astype(np.float64) - d64.min(1)).max() / (EPS32 * extent)
        print(f'{name}: extent {extent:.3g}, worst pair {worst:.2f} eps32 * extent, worst per-point minimum {worst_min:.2f}')
        assert worst <= 16.0, (name, worst)
    on, tri = fam['on-surface']
    d32 = geometry.point_triangle(on[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], np.float32)[0].min(1)
    assert d32.max() <= 4 * EPS32 * extent_of(on, tri)               # ulps of the coordinates, not of their square root


def test_restatement_on_soups_matches_an_independent_formulation():
    """The float64 restatement against projection-free geometry: the distance to a triangle is the minimum of |p - x| over its points,
    bounded from above by a dense barycentric sampling of the triangle and from below by nothing smaller than that minus the sampling step."""
    rs = np.random.RandomState(23)
    verts, faces = random_soup(rs, 60, degenerate=0.1, slivers=0.1, nans=0.0)
    pts = rs.uniform(-1.2, 1.2, (80, 3)).astype(F32)
    d, f, q = geometry._closest_numpy(pts, verts, faces)
    k = 60
    i, j = np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing='ij')
    keep = i + j <= k
    w = np.stack([i[keep], j[keep], k - i[keep] - j[keep]], -1) / k
    tri = verts[faces].astype(np.float64)
    samples = np.einsum('sw,fwc->fsc', w, tri)
    dense = np.linalg.norm(pts[:, None, None, :].astype(np.float64) - samples[None], axis=-1).min((1, 2))
    edge = np.linalg.norm(tri - np.roll(tri, 1, 1), axis=-1).max()
    assert (d <= dense + 1e-12).all() and (d >= dense - edge / k).all()
    assert np.abs(np.linalg.norm(pts - q, axis=1) - d).max() <= 1e-12
    back, _ = geometry.point_triangle(q, tri[f, 0], tri[f, 1], tri[f, 2])
    assert back.max() <= 1e-12                                        # the closest point lies on its triangle


def test_geometry_metrics_command_line(tmp_path):
    from invertavatar_amd import extract_geometry, geometry_metrics
    v, f, _ = sphere_mc(16)
    a, b = str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply')
    geometry.write_ply(a, v, f)
    geometry.write_ply(b, v * F32(1.25), f)
    res = geometry_metrics.main(['--pred', a, '--gt', a, '--out', str(tmp_path / 'same.json'), '--device', 'cpu'])
    same = json.load(open(tmp_path / 'same.json'))
    assert same == res and same['chamfer'] == 0 and same['hausdorff'] == 0 and same['chamfer_sq'] == 0 and same['fscore'] == [1.0] * 3
    assert same['pred_faces'] == f.shape[0] and same['gt_vertices'] == v.shape[0]
    geometry_metrics.main(['--pred', a, '--gt', b, '--samples', '500', '--thresholds', '0.1', '0.4', '--error-ply', str(tmp_path / 'e.ply'),
                           '--out', str(tmp_path / 'diff.json'), '--device', 'cpu'])
    diff = json.load(open(tmp_path / 'diff.json'))
    assert abs(diff['chamfer'] - 0.25) < 0.02 and diff['fscore'][0] == 0.0 and diff['fscore'][1] == 1.0 and diff['normal_consistency'] > 0.99
    ev, ef, ec = geometry.read_ply(str(tmp_path / 'e.ply'))
    assert np.array_equal(ev, v) and np.array_equal(ef, f) and ec[:, 0].min() > 100 and (ec[:, 1:] == 0).all()
    # extract_geometry --compare of the extracted mesh with itself writes a JSON of zeros
    first = extract_geometry.main(['--seeds', '0', '--width', 'small', '--res', '24', '--level', '0', '--outdir', str(tmp_path), '--device', 'cpu',
                                   '--no-colors'])
    ref = first[0][0]
    extract_geometry.main(['--seeds', '0', '--width', 'small', '--res', '24', '--level', '0', '--outdir', str(tmp_path / 'again'), '--device', 'cpu',
                           '--no-colors', '--compare', ref, '--error-ply'])
    m = json.load(open(tmp_path / 'again' / 'seed0000_geometry.json'))
    assert m['chamfer'] == 0 and m['hausdorff'] == 0 and m['mean_ab'] == 0 and m['max_ba'] == 0 and m['fscore'] == [1.0] * 3
    assert (tmp_path / 'again' / 'seed0000_error.ply').exists()
