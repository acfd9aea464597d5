"""Surface distance on the device (csrc/surface_distance.hip) against the float64 NumPy restatement, with the tolerance taken from the
restatement's own float32 run (``4 * e32 + eps32 * extent``, never from the kernel); the grid against the brute mode of the same kernel
(bit equality for several resolutions and run to run); ia_distance_stats against float64 sums; a full-size generator mesh; the error
paths of the ABI."""
import ctypes

import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, geometry, hipops, synthetic
from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
from test_surface_distance_cpu import (EPS32, F32, TRI, cube_mesh, extent_of, radial_volume, random_soup, restatement_error,
                                       single_triangle_cases)

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_case(name, points, verts, faces, cells=(None,)):
    """One case through every comparison: device distances, faces and points against the float64 restatement, and the grid (for every
    entry of ``cells``) bit-equal to the brute mode.  Returns the device's own error in units of the tolerance."""
    points, verts = np.asarray(points, dtype=F32), np.asarray(verts, dtype=F32)
    d64, f64, e32 = restatement_error(points, verts, faces)
    extent = extent_of(points, verts)
    tol = 4 * e32 + EPS32 * extent
    dp, dv, df = dev(points), dev(verts), dev(np.asarray(faces, dtype=np.int64))
    brute = geometry.closest_point(dp, dv, df, brute=True)
    dist, face, point = (brute[k].cpu().numpy() for k in ('dist', 'face', 'point'))
    assert dist.dtype == F32 and face.dtype == np.int64 and point.shape == points.shape
    fin = np.isfinite(d64)
    assert np.array_equal(np.isnan(dist), np.isnan(d64)) and np.array_equal(np.isposinf(dist), np.isposinf(d64))
    assert np.array_equal(face >= 0, fin) and (face[~fin] == -1).all() and np.isnan(point[~fin]).all()
    err = float(np.abs(dist[fin].astype(np.float64) - d64[fin]).max()) if fin.any() else 0.0
    print(f'{name}: N = {len(points)}, F = {len(faces)}, extent {extent:.3g}, e32 = {e32:.3g}, device error {err:.3g}, tolerance {tol:.3g}')
    assert err <= tol, (name, err, tol)
    if fin.any():
        tri = verts[np.asarray(faces)[face[fin]]].astype(np.float64)
        p64 = points[fin].astype(np.float64)
        own, _ = geometry.point_triangle(p64, tri[:, 0], tri[:, 1], tri[:, 2])             # float64 distance to the face returned
        assert np.abs(own - d64[fin]).max() <= tol, name
        q = point[fin].astype(np.float64)
        on, _ = geometry.point_triangle(q, tri[:, 0], tri[:, 1], tri[:, 2])               # the point lies on that face
        assert on.max() <= tol and np.abs(np.linalg.norm(p64 - q, axis=1) - dist[fin]).max() <= tol, name
    for c in cells:
        grid = geometry.TriangleGrid(dv, df, cells=c)
        for _ in range(2):
            r = grid.closest(dp)
            assert all(torch.equal(r[k], brute[k]) or (k != 'face' and torch.equal(r[k].isnan(), brute[k].isnan())
                                                       and torch.equal(r[k].nan_to_num(7.0), brute[k].nan_to_num(7.0)))
                       for k in ('dist', 'face', 'point')), (name, c, grid.dims)
        unsorted = grid.closest(dp, sort=False)
        assert torch.equal(unsorted['face'], brute['face']) and torch.equal(unsorted['dist'].nan_to_num(7.0), brute['dist'].nan_to_num(7.0))
    again = geometry.closest_point(dp, dv, df, brute=True)
    assert torch.equal(again['face'], brute['face']) and torch.equal(again['dist'].nan_to_num(7.0), brute['dist'].nan_to_num(7.0))
    return err / tol


GRIDS = (None, 1, (3, 5, 2), 40)


def test_single_triangle_and_tiny_sizes():
    pts = np.array([c[0] for c in single_triangle_cases()] + [(1, 1, 0), (4, 0, 0), (np.nan, 0, 0)], dtype=F32)
    check_case('one triangle', pts, TRI[0], TRI[1], GRIDS)                                # F = 1
    r = geometry.closest_point(dev(pts), dev(TRI[0]), dev(TRI[1]))
    for k, (_, d, q) in enumerate(single_triangle_cases()):
        assert abs(float(r['dist'][k]) - d) <= 2 * EPS32 * 8 and np.abs(r['point'][k].cpu().numpy() - np.array(q)).max() <= 2 * EPS32 * 8
    assert r['dist'][14:16].tolist() == [0.0, 0.0] and r['face'].tolist() == [0] * 16 + [-1]
    rs = np.random.RandomState(1)
    verts, faces = random_soup(rs, 300)
    check_case('N = 1', rs.uniform(-1, 1, (1, 3)), verts, faces, GRIDS)
    check_case('N = 67', rs.uniform(-1, 1, (67, 3)), verts, faces, GRIDS)                 # not a multiple of 64
    empty = geometry.closest_point(dev(pts), torch.zeros(0, 3, device='cuda'), torch.zeros(0, 3, dtype=torch.int64, device='cuda'))
    assert bool(empty['dist'][:16].isinf().all()) and bool(empty['dist'][16].isnan()) and bool((empty['face'] == -1).all())
    none = geometry.closest_point(torch.zeros(0, 3, device='cuda'), dev(TRI[0]), dev(TRI[1]))
    assert none['dist'].shape == (0,) and none['point'].shape == (0, 3)


@pytest.mark.parametrize('clustered', [False, True])
def test_random_soups(clustered):
    rs = np.random.RandomState(31 + clustered)
    for n_tris, n_pts in ((1, 200), (17, 300), (1000, 1500), (20000, 500)):
        verts, faces = random_soup(rs, n_tris, clustered=clustered, nans=0.01)
        pts = rs.uniform(-1.3, 1.3, (n_pts, 3)).astype(F32)
        pts[::50] = verts[rs.randint(0, len(verts), len(pts[::50]))]                      # some queries on vertices (NaN ones included)
        check_case(f'soup {n_tris} clustered={clustered}', pts, verts, faces, GRIDS if n_tris <= 1000 else (None, 1, 48))


def test_marching_cubes_mesh_and_far_points():
    vol, lo, step = radial_volume(40)
    vol = vol + F32(0.15) * np.sin(np.arange(40, dtype=F32) * F32(0.7))[None, :, None]     # a smooth, less symmetric field
    verts, faces = geometry.marching_cubes(vol.astype(F32), 0.0, (lo,) * 3, (step,) * 3)
    assert faces.shape[0] > 5000
    dv, df = dev(verts), dev(faces)
    grid = geometry.TriangleGrid(dv, df)
    own = grid.closest(dv)
    assert bool((own['dist'] == 0).all()) and bool((own['point'] == dv).all())             # a - p is 0 for a triangle that owns the vertex
    rs = np.random.RandomState(9)
    sub = rs.choice(len(verts), 500, replace=False)
    check_case('mc own vertices', verts[sub], verts, faces, (None, 1, 64))
    nrm = geometry.face_normals(verts, faces)
    vn = np.zeros_like(verts)
    np.add.at(vn, faces.reshape(-1), np.repeat(nrm, 3, 0))
    vn /= np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-12)
    moved = (verts + vn * rs.uniform(-3, 3, (len(verts), 1)) * step).astype(F32)
    check_case('mc displaced along normals', moved[sub], verts, faces, (None, 1, 64))
    diag = float(np.linalg.norm(verts.max(0) - verts.min(0)))
    far = rs.normal(size=(200, 3))
    far = (far / np.linalg.norm(far, axis=1, keepdims=True) * rs.uniform(0, 10 * diag, (200, 1))).astype(F32)
    check_case('mc far points', far, verts, faces, (None, 1, 64))


def test_one_huge_triangle_among_small_ones():
    rs = np.random.RandomState(13)
    verts, faces = random_soup(rs, 10000, clustered=True)
    huge = np.array([[-1.2, -1.1, -0.9], [1.3, -1.0, 0.2], [0.1, 1.2, 1.1]], dtype=F32)
    verts = np.concatenate([verts, huge])
    faces = np.concatenate([faces[:5000], [[len(verts) - 3, len(verts) - 2, len(verts) - 1]], faces[5000:]])
    grid = geometry.TriangleGrid(dev(verts), dev(faces))
    assert grid.n_over >= 1 and grid.entries <= 64 * len(faces)
    print(f'huge triangle: grid {grid.dims}, {grid.entries} entries, {grid.n_over} oversize')
    pts = rs.uniform(-1.3, 1.3, (600, 3)).astype(F32)
    check_case('huge triangle', pts, verts, faces, (None, 1, 64))
    r = grid.closest(dev(pts))
    assert int((r['face'] == 5000).sum()) > 40                                          # the huge one is the closest for many points


def test_distance_stats_against_float64_sums():
    rs = np.random.RandomState(2)
    for n in (0, 1, 63, 1000, 300001):
        d = np.abs(rs.normal(0, 0.3, n)).astype(F32)
        if n > 10:
            d[rs.randint(0, n, n // 20)] = np.nan
            d[rs.randint(0, n, n // 30)] = np.inf
        fb = 500
        face = rs.randint(-1, fb, n).astype(np.int32)
        na, nb = rs.normal(size=(n, 3)).astype(F32), rs.normal(size=(fb, 3)).astype(F32)
        thr = [0.0, 0.1, 0.25, 0.3, 0.5, 1.0, 2.0, 1e9]
        ref = geometry._stats_numpy(d, thr, face, na, nb)
        out = hipops.distance_stats(dev(d), thr, dev(face), dev(na), dev(nb))
        got = out.cpu().numpy()
        rel = n * 2.0 ** -53
        assert got[0] == ref[0] and got[5] == ref[5] and got[0] + got[5] == n and np.array_equal(got[6:], ref[6:]), n
        assert got[3] == ref[3], n                                                        # max (-inf when nothing is finite)
        for k in (1, 2, 4):
            assert abs(got[k] - ref[k]) <= rel * abs(ref[k]), (n, k, got[k], ref[k])
        assert torch.equal(out, hipops.distance_stats(dev(d), thr, dev(face), dev(na), dev(nb)))
        plain = hipops.distance_stats(dev(d), thr[:3]).cpu().numpy()
        assert np.array_equal(plain[:4], got[:4]) and plain[4] == 0 and np.array_equal(plain[6:9], got[6:9]) and (plain[9:] == 0).all()
    # surface_distance on the device equals the CPU path up to the distances' fp32 rounding
    a, b = cube_mesh(), cube_mesh(lo=(0.25, 0.0, 0.0))
    r = geometry.surface_distance(dev(a[0]), dev(a[1]), dev(b[0]), dev(b[1]))
    assert r['hausdorff'] == 0.25 and r['chamfer'] == 0.125 and r['chamfer_sq'] == 0.0625 and r['n_a'] == 8
    rc = geometry.surface_distance(*a, *b, samples=5000, seed=3)
    rd = geometry.surface_distance(dev(a[0]), dev(a[1]), dev(b[0]), dev(b[1]), samples=5000, seed=3)
    assert rd['precision'] == rc['precision'] and rd['recall'] == rc['recall'] and rd['thresholds'] == rc['thresholds']
    for k in ('mean_ab', 'mean_ba', 'rms_ab', 'chamfer', 'hausdorff', 'normal_consistency'):
        assert abs(rd[k] - rc[k]) <= 1e-6, k


# ------------------------------------------------------------------ full size

@pytest.fixture(scope='module')
def full_setup():
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('full')).eval().requires_grad_(False)).cuda()
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(0, 1).cuda(), synthetic.conditioning_camera().cuda(), truncation_psi=0.7, truncation_cutoff=14)
        mesh = {'uvcoords_image': synthetic.uv_conditions([0]).cuda()}
    return g, ws, mesh


def test_full_size_kept_mesh_is_a_subset(full_setup):
    g, ws, mesh = full_setup
    full = g.extract_geometry(ws, mesh, resolution=256, level=0.0, noise_mode='const')[0]
    kept = g.extract_geometry(ws, mesh, resolution=256, level=0.0, keep='largest', noise_mode='const')[0]
    k = kept['components']['count']
    r = geometry.surface_distance(kept['verts'], kept['faces'], full['verts'], full['faces'])
    print(f'256^3: {full["faces"].shape[0]} triangles, kept {kept["faces"].shape[0]} of K = {k} components; kept -> all: mean {r["mean_ab"]}, '
          f'max {r["max_ab"]}; all -> kept: mean {r["mean_ba"]:.6g}, max {r["max_ba"]:.6g}')
    assert r['mean_ab'] == 0.0 and r['max_ab'] == 0.0 and r['n_a'] == kept['verts'].shape[0] and r['skipped_ab'] == 0
    if k > 1:
        assert r['max_ba'] > 0.0
    coarse = g.extract_geometry(ws, mesh, resolution=128, level=0.0, noise_mode='const')[0]
    c = geometry.surface_distance(coarse['verts'], coarse['faces'], full['verts'], full['faces'])
    print(f'128^3 against 256^3: chamfer {c["chamfer"]:.6g}, hausdorff {c["hausdorff"]:.6g}, fscore {c["fscore"]} at {c["thresholds"]}')
    # the grid against the brute mode on a subset of the full-size queries
    grid = geometry.TriangleGrid(full['verts'], full['faces'])
    q = coarse['verts'][:: max(1, coarse['verts'].shape[0] // 2000)].contiguous()
    a, b = grid.closest(q), grid.closest(q, brute=True)
    assert torch.equal(a['dist'], b['dist']) and torch.equal(a['face'], b['face']) and torch.equal(a['point'], b['point'])


# ------------------------------------------------------------------ error paths

def test_error_paths_report_not_fault():
    lib = _lib.load()
    f3, i3 = hipops._f3, hipops._i3
    verts, faces = dev(TRI[0]), dev(TRI[1].astype(np.int32))
    tris = torch.full((1, 3, 4), 5.0, device='cuda')
    assert lib.ia_tri_pack(None, 3, faces.data_ptr(), 1, tris.data_ptr(), None) == -1 and 'device pointers' in _lib.last_error()
    assert lib.ia_tri_pack(verts.data_ptr(), 3, faces.data_ptr(), -1, tris.data_ptr(), None) == -1 and 'F' in _lib.last_error()
    dims, inv = (ctypes.c_int * 3)(), (ctypes.c_float * 3)()
    assert lib.ia_trigrid_plan(-1, f3([0] * 3), f3([1] * 3), None, dims, inv) == -1
    assert lib.ia_trigrid_plan(10, None, f3([1] * 3), None, dims, inv) == -1 and 'null' in _lib.last_error()
    assert lib.ia_trigrid_plan(10, f3([0] * 3), f3([1, -1, 1]), None, dims, inv) == -1 and 'hi >= lo' in _lib.last_error()
    assert lib.ia_trigrid_plan(10, f3([0] * 3), f3([1] * 3), i3([2000, 1, 1]), dims, inv) == -1
    assert lib.ia_trigrid_plan(1000, f3([0] * 3), f3([1, 1, 0]), None, dims, inv) == 0 and dims[2] == 1 and 30 <= dims[0] <= 33
    cell_start = torch.full((10,), 3, dtype=torch.int32, device='cuda')
    lo, one, d222 = f3([0] * 3), f3([1] * 3), i3([2, 2, 2])
    assert lib.ia_trigrid_count(tris.data_ptr(), -1, lo, one, d222, cell_start.data_ptr(), None) == -1
    assert lib.ia_trigrid_count(tris.data_ptr(), 1, lo, one, i3([0, 2, 2]), cell_start.data_ptr(), None) == -1 and 'dims' in _lib.last_error()
    assert lib.ia_trigrid_count(tris.data_ptr(), 1, lo, f3([1, 0, 1]), d222, cell_start.data_ptr(), None) == -1
    assert lib.ia_trigrid_count(tris.data_ptr(), 1, lo, one, d222, None, None) == -1 and 'device pointers' in _lib.last_error()
    scratch = torch.full((9,), 4, dtype=torch.int32, device='cuda')
    cell_tris = torch.full((8,), 6, dtype=torch.int32, device='cuda')

    def fill(sbytes=36, entries=1, n_over=0):
        return lib.ia_trigrid_fill(tris.data_ptr(), 1, lo, one, d222, cell_start.data_ptr(), entries, n_over, scratch.data_ptr(), sbytes,
                                   cell_tris.data_ptr(), None)
    assert fill(sbytes=32) == -1 and 'scratch' in _lib.last_error()
    assert fill(entries=65) == -1 and fill(entries=-1) == -1 and fill(n_over=2) == -1
    pts = torch.zeros(4, 3, device='cuda')
    dist = torch.full((4,), 9.0, device='cuda')
    face = torch.full((4,), 9, dtype=torch.int32, device='cuda')
    point = torch.full((4, 3), 9.0, device='cuda')

    def query(p=pts.data_ptr(), n=4, f=1, extent=1.0, cs=None, dm=d222, entries=0):
        return lib.ia_closest_point(p, n, tris.data_ptr(), f, extent, lo, one, dm, cs, cell_tris.data_ptr(), entries, 0, dist.data_ptr(),
                                    face.data_ptr(), point.data_ptr(), None)
    assert query(p=None) == -1 and 'device pointers' in _lib.last_error()
    assert query(n=-1) == -1 and query(f=-1) == -1 and query(extent=float('nan')) == -1 and query(extent=-1.0) == -1
    assert query(cs=cell_start.data_ptr(), dm=i3([2, 2, 5000])) == -1 and 'dims' in _lib.last_error()
    assert query(cs=cell_start.data_ptr(), entries=100) == -1 and 'entries' in _lib.last_error()
    assert query(p=torch.zeros(4, 3).data_ptr()) == -1
    nbytes = ctypes.c_size_t(0)
    assert lib.ia_distance_stats_scratch_bytes(-1, ctypes.byref(nbytes)) == -1 and lib.ia_distance_stats_scratch_bytes(4, None) == -1
    assert lib.ia_distance_stats_scratch_bytes(4, ctypes.byref(nbytes)) == 0 and nbytes.value == 14 * 8
    sc = torch.full((14,), 2.0, dtype=torch.float64, device='cuda')
    out = torch.full((14,), 3.0, dtype=torch.float64, device='cuda')
    thr = (ctypes.c_float * 9)(*([0.5] * 9))

    def stats(n=4, nthr=2, sbytes=112, fa=None, na=None, o=out.data_ptr()):
        return lib.ia_distance_stats(dist.data_ptr(), n, thr, nthr, fa, na, None, 0, sc.data_ptr(), sbytes, o, None)
    assert stats(sbytes=8) == -1 and 'scratch' in _lib.last_error()
    assert stats(nthr=9) == -1 and 'thresholds' in _lib.last_error()
    assert stats(n=-1) == -1 and stats(o=None) == -1
    assert stats(fa=face.data_ptr()) == -1 and 'go together' in _lib.last_error()
    torch.cuda.synchronize()
    # nothing was launched: every output still holds what it was filled with
    assert bool((tris == 5).all()) and bool((cell_start == 3).all()) and bool((scratch == 4).all()) and bool((cell_tris == 6).all())
    assert bool((dist == 9).all()) and bool((face == 9).all()) and bool((point == 9).all()) and bool((out == 3).all())
    with pytest.raises(ValueError):
        geometry.TriangleGrid(verts, faces, cells=0)
    with pytest.raises(ValueError):
        geometry.TriangleGrid(TRI[0], TRI[1])
    with pytest.raises(RuntimeError):
        hipops.closest_point(torch.zeros(4, 3), tris, 1.0)
    torch.cuda.synchronize()
