"""Alignment on the device (csrc/align.hip) against the float64 NumPy restatement: ia_transform_points within the dot-product bound,
ia_align_sums with exact counts and sums within the restatement's own order dependence, ``align_mesh`` against the transform that was
applied and against the restatement (tolerance from the restatement's float32 run, never from the kernels), bit equality from run to run
and with a handed-in grid, trimming, the error paths of the ABI and one full-size generator mesh."""
import ctypes

import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, geometry, hipops, synthetic
from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
from test_align_cpu import EPS64, moved, outlier_source, shared_case, similarity
from test_surface_distance_cpu import EPS32, F32

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_transform_points_within_the_dot_product_bound():
    """Every component within 3 eps32 (sum_j |m_ij| |x_j| + |t_i|) of the float64 product: gamma_4 with u = eps32 / 2 for the three
    products and three additions, plus the rounding of M to float32 (one more u per term)."""
    rs = np.random.RandomState(4)
    M = similarity(1.07, 41.0, (0.3, -0.2, 1.5))
    for n in (1, 67, 1000):
        x = (rs.normal(size=(n, 3)) * 3).astype(F32)
        x[n // 2] = (np.nan, 1.0, 2.0)
        y = geometry.transform_points(dev(x), M)
        again = geometry.transform_points(dev(x), M)
        got = y.cpu().numpy()
        assert got.dtype == F32 and got.shape == (n, 3)
        assert np.isnan(got[n // 2]).all()                                    # (a NaN coordinate meets every row of a full matrix)
        ok = np.arange(n) != n // 2
        x64 = x[ok].astype(np.float64)
        ref = x64 @ M[:3, :3].T + M[:3, 3]
        bound = 3 * EPS32 * (np.abs(x64) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3]))
        err = np.abs(got[ok] - ref)
        print(f'N = {n}: largest error / bound = {float((err / bound).max()) if ok.any() else 0.0:.3g}')
        assert (err <= bound).all()
        assert torch.equal(y[dev(ok)], again[dev(ok)]) and np.array_equal(got[ok], geometry.transform_points(x, M)[ok])
    inf = geometry.transform_points(dev(np.array([[np.inf, 0.0, 0.0]], dtype=F32)), M).cpu().numpy()
    assert not np.isfinite(inf).any()
    assert geometry.transform_points(torch.zeros(0, 3, device='cuda'), M).shape == (0, 3)


def sums_inputs(rs, n, fb=300, max_dist=0.3):
    src, dst = rs.normal(size=(n, 3)).astype(F32), rs.normal(size=(n, 3)).astype(F32)
    dist = np.abs(rs.normal(0, 0.2, n)).astype(F32)
    face = rs.randint(0, fb, n).astype(np.int32)
    normals = rs.normal(size=(fb, 3)).astype(F32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    normals[5] = 0.0                                                          # a face without area
    if n > 10:
        dist[rs.randint(0, n, n // 20)] = np.nan
        dist[rs.randint(0, n, n // 30)] = np.inf
        face[rs.randint(0, n, n // 25)] = -1
        face[rs.randint(0, n, n // 40 + 1)] = 5
        k = rs.randint(0, n, 6)
        dist[k[:3]] = np.nextafter(F32(max_dist), F32(1))                     # just above the threshold
        dist[k[3:]] = np.nextafter(F32(max_dist), F32(0))                     # just below
        dist[rs.randint(0, n)] = F32(max_dist)                                # on it: counts
    return src, dst, dist, face, normals


def kept_rows(dist, face, normals, max_dist, metric):
    keep = np.isfinite(dist) & (face >= 0) & (dist <= F32(max_dist))
    if metric == 'plane':
        keep &= (normals[np.maximum(face, 0)] != 0).any(1)
    return keep


@pytest.mark.parametrize('metric', ['point', 'plane'])
def test_align_sums_against_float64(metric):
    """Counts exact, every sum within 4 e_ord + eps64 sum |terms| of the restatement; e_ord: the restatement summed forwards against
    summed in reversed order on the same input (the restatement's sums are correctly rounded, so e_ord is 0 and the second term is
    the whole tolerance)."""
    rs = np.random.RandomState(17)
    centre, max_dist = (0.1, -0.2, 0.05), 0.3
    worst = 0.0
    for n in (0, 1, 63, 64, 65, 1000, 70001):
        src, dst, dist, face, normals = sums_inputs(rs, n, max_dist=max_dist)
        terms, rejected = geometry._align_terms_numpy(src, dst, dist, face, normals, centre, max_dist, metric)
        ref = geometry._align_sums_numpy(src, dst, dist, face, normals, centre, max_dist, metric)
        back = geometry._column_sums(terms[::-1])
        tol = 4 * np.abs(ref[:-1] - back) + EPS64 * np.abs(terms).sum(0)
        args = (dev(src), dev(dst), dev(dist), dev(face), centre, max_dist, metric, dev(normals))
        out = hipops.align_sums(*args)
        got = out.cpu().numpy()
        assert got.shape == ((56,) if metric == 'plane' else (20,)) and got.dtype == np.float64
        keep = kept_rows(dist, face, normals, max_dist, metric)
        assert got[0] == ref[0] == np.count_nonzero(keep) and got[-1] == ref[-1] == rejected == n - np.count_nonzero(keep), n
        err = np.abs(got[:-1] - ref[:-1])
        ratio = float((err / np.maximum(tol, 1e-300)).max()) if n else 0.0
        worst = max(worst, ratio)
        print(f'{metric} N = {n}: {int(got[0])} pairs count, {int(got[-1])} do not; largest error / tolerance = {ratio:.3g}')
        assert (err <= tol).all(), (n, np.flatnonzero(err > tol))
        if n == 0:
            assert (got == 0).all()
        assert torch.equal(out, hipops.align_sums(*args))                                   # the same bits on every run
        packed = hipops.align_sums(dev(src[keep]), dev(dst[keep]), dev(dist[keep]), dev(face[keep]), centre, max_dist, metric, dev(normals))
        packed = packed.cpu().numpy()
        assert packed[0] == got[0] and packed[-1] == 0 and (np.abs(packed[:-1] - ref[:-1]) <= tol).all(), n
        open_ = hipops.align_sums(*args[:5], float('inf'), metric, args[7]).cpu().numpy()       # no threshold
        keep_open = kept_rows(dist, face, normals, np.inf, metric)
        assert open_[0] == np.count_nonzero(keep_open) and open_[0] + open_[-1] == n
    if metric == 'plane':
        src, dst, dist, face, normals = sums_inputs(rs, 1000)
        point = hipops.align_sums(dev(src), dev(dst), dev(dist), dev(face), centre, 1.0, 'point').cpu().numpy()
        none = hipops.align_sums(dev(src), dev(dst), dev(dist), dev(face), centre, 1.0, 'plane', torch.zeros(0, 3, device='cuda')).cpu().numpy()
        assert none[0] == 0 and none[-1] == 1000 and (none[:-1] == 0).all() and point[0] > 0


def test_align_sums_error_paths():
    lib = _lib.load()
    n = 8
    src, dst = torch.zeros(n, 3, device='cuda'), torch.zeros(n, 3, device='cuda')
    dist, face = torch.zeros(n, device='cuda'), torch.zeros(n, dtype=torch.int32, device='cuda')
    normals = torch.ones(4, 3, device='cuda')
    out = torch.full((56,), 3.0, dtype=torch.float64, device='cuda')
    moved_out = torch.full((n, 3), 5.0, device='cuda')
    nbytes = ctypes.c_size_t(0)
    assert lib.ia_align_sums_scratch_bytes(n, 1, ctypes.byref(nbytes)) == 0 and nbytes.value == 56 * 8
    assert lib.ia_align_sums_scratch_bytes(n, 0, ctypes.byref(nbytes)) == 0 and nbytes.value == 20 * 8
    assert lib.ia_align_sums_scratch_bytes(-1, 0, ctypes.byref(nbytes)) == -1 and lib.ia_align_sums_scratch_bytes(n, 0, None) == -1
    assert lib.ia_align_sums_scratch_bytes(n, 2, ctypes.byref(nbytes)) == -1 and 'mode' in _lib.last_error()
    scratch = torch.full((56,), 2.0, dtype=torch.float64, device='cuda')
    c = hipops._d3((0, 0, 0))

    def sums(s=src.data_ptr(), count=n, nrm=normals.data_ptr(), centre=c, mode=1, sbytes=56 * 8, o=out.data_ptr()):
        return lib.ia_align_sums(s, dst.data_ptr(), dist.data_ptr(), face.data_ptr(), count, nrm, 4, centre, float('inf'), mode,
                                 scratch.data_ptr(), sbytes, o, None)
    assert sums(s=None) == -1 and 'device pointers' in _lib.last_error()
    assert sums(s=torch.zeros(n, 3).data_ptr()) == -1 and 'device pointers' in _lib.last_error()
    assert sums(o=None) == -1 and 'device pointers' in _lib.last_error()
    assert sums(nrm=None) == -1 and 'face_normals' in _lib.last_error()
    assert sums(mode=2) == -1 and 'mode' in _lib.last_error()
    assert sums(sbytes=55 * 8) == -1 and 'scratch' in _lib.last_error()
    assert sums(count=-1) == -1 and 'N' in _lib.last_error()
    assert sums(centre=None) == -1 and 'h_centre' in _lib.last_error()
    m12 = (ctypes.c_double * 12)(*([0.0] * 12))
    assert lib.ia_transform_points(None, n, m12, moved_out.data_ptr(), None) == -1 and 'device pointers' in _lib.last_error()
    assert lib.ia_transform_points(torch.zeros(n, 3).data_ptr(), n, m12, moved_out.data_ptr(), None) == -1
    assert lib.ia_transform_points(src.data_ptr(), n, None, moved_out.data_ptr(), None) == -1 and 'h_m12' in _lib.last_error()
    assert lib.ia_transform_points(src.data_ptr(), -1, m12, moved_out.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert bool((out == 3).all()) and bool((scratch == 2).all()) and bool((moved_out == 5).all())      # nothing was launched
    with pytest.raises(ValueError):
        hipops.align_sums(src, dst, dist, face, (0, 0, 0), metric='line')
    with pytest.raises(RuntimeError):
        hipops.align_sums(src, dst, dist, face.long(), (0, 0, 0))
    torch.cuda.synchronize()


@pytest.mark.parametrize('scale', [1.0, 1.05])
def test_align_mesh_recovers_the_transform(scale):
    """Within 4 e32 + eps32 extent of the truth and of the restatement's matrix.  The history has the restatement's length +- 1: a tie
    in the stopping rule (rms against eps32 extent at the float32 floor) may fall either way."""
    c = shared_case(scale)
    args = (dev(c.src), dev(c.verts), dev(c.faces))
    r = geometry.align_mesh(*args, metric='plane', scale=c.with_scale, iterations=12)
    e_truth, e_cpu = float(np.abs(r['matrix'] - c.truth).max()), float(np.abs(r['matrix'] - c.r64['matrix']).max())
    print(f'scale {scale}: {r["iterations"]} steps, rms {r["rms_history"]}; |M - truth| = {e_truth:.3g}, |M - restatement| = {e_cpu:.3g}, '
          f'e32 = {c.e32:.3g}, tolerance {c.tol:.3g}')
    assert r['matrix'].dtype == np.float64 and r['converged'] and r['inliers'] == 400
    assert e_truth <= c.tol and e_cpu <= c.tol
    assert abs(len(r['rms_history']) - len(c.r64['rms_history'])) <= 1 and len(r['rms_history']) == r['iterations'] + 1
    again = geometry.align_mesh(*args, metric='plane', scale=c.with_scale, iterations=12)
    assert np.array_equal(again['matrix'], r['matrix']) and again['rms_history'] == r['rms_history']


def test_point_metric_on_device():
    c = shared_case(1.0)
    src, verts, faces = dev(c.src), dev(c.verts), dev(c.faces)
    r = geometry.align_mesh(src, verts, faces, metric='point', iterations=10)
    h = r['rms_history']
    print('point rms history', h)
    assert len(h) == 11 and all(h[k + 1] <= h[k] * (1 + 4 * EPS32) for k in range(10))
    # one step: the device's own pairs through the restatement's sums and the shared solve
    grid = geometry.TriangleGrid(verts, faces)
    p = hipops.transform_points(src, np.eye(4))
    q = grid.closest(p)
    centre = [(a + b) / 2 for a, b in zip(grid.lo, grid.hi)]
    got = hipops.align_sums(p, q['point'], q['dist'], q['face'].int(), centre, metric='point').cpu().numpy()
    host = [x.cpu().numpy() for x in (p, q['point'], q['dist'], q['face'])]
    terms, _ = geometry._align_terms_numpy(*host, None, centre, np.inf, 'point')
    ref = geometry._align_sums_numpy(*host, None, centre, np.inf, 'point')
    e_ord = np.abs(ref[:-1] - geometry._column_sums(terms[::-1])) + EPS64 * np.abs(terms).sum(0)
    rel = float((e_ord / np.maximum(np.abs(ref[:-1]), 1.0)).max())
    inc_dev, inc_ref = (geometry._align_solve(s, 'point', False, np.array(centre)) for s in (got, ref))
    err = float(np.abs(inc_dev - inc_ref).max())
    print(f'one step: |increment - restatement| = {err:.3g}, 1e-12 + 4 e_ord = {1e-12 + 4 * rel:.3g}')
    assert got[0] == ref[0] == 400 and err <= 1e-12 + 4 * rel
    assert abs(float(np.sqrt(got[18] / got[0])) - h[0]) <= 1e-12


def test_trim_and_max_dist_counts_match_the_restatement():
    c = shared_case(1.0)
    src = outlier_source(c)
    verts, faces = dev(c.verts), dev(c.faces)
    cpu = geometry.align_mesh(src, c.verts, c.faces, iterations=12, trim=0.85)
    gpu = geometry.align_mesh(dev(src), verts, faces, iterations=12, trim=0.85)
    print(f'trim 0.85: {gpu["inliers"]} pairs on the device, {cpu["inliers"]} in the restatement; error {np.abs(gpu["matrix"] - c.truth).max():.3g}')
    assert gpu['inliers'] == cpu['inliers'] == 340 and float(np.abs(gpu['matrix'] - c.truth).max()) <= c.tol
    cpu = geometry.align_mesh(src, c.verts, c.faces, iterations=2, max_dist=0.3, init=c.truth)
    gpu = geometry.align_mesh(dev(src), verts, faces, iterations=2, max_dist=0.3, init=c.truth)
    assert gpu['inliers'] == cpu['inliers'] == 360
    with_nan = c.src.copy()
    with_nan[7] = np.nan
    r = geometry.align_mesh(dev(with_nan), verts, faces, iterations=12)
    assert r['inliers'] == 399 and np.isfinite(r['matrix']).all() and float(np.abs(r['matrix'] - c.truth).max()) <= c.tol


def test_given_grid_and_empty_target():
    c = shared_case(1.0)
    src, verts, faces = dev(c.src), dev(c.verts), dev(c.faces)
    own = geometry.align_mesh(src, verts, faces, iterations=12)
    grid = geometry.TriangleGrid(verts, faces)
    given = geometry.align_mesh(src, verts, faces, iterations=12, grid=grid)
    assert np.array_equal(own['matrix'], given['matrix']) and own['rms_history'] == given['rms_history']
    start = geometry.align_mesh(src, verts, faces, init=c.truth, grid=grid)
    assert start['iterations'] == 0 and np.array_equal(start['matrix'], c.truth)
    hipops.PROFILE = []
    try:
        with pytest.raises(ValueError):
            geometry.align_mesh(src, verts, torch.zeros(0, 3, dtype=torch.int64, device='cuda'))
        with pytest.raises(ValueError):
            geometry.align_mesh(src[:4].contiguous(), verts, faces, grid=grid)             # 4 pairs, the plane metric needs 6
        launched = [e[0] for e in hipops.PROFILE]
    finally:
        hipops.PROFILE = None
    assert 'align_sums' in launched and launched.index('align_sums') > 0                  # the second case ran, the empty target launched nothing before it
    assert launched[0] == 'transform_points'


def test_full_size_generator_meshes():
    """A 128^3 mesh of the reduced-width generator, moved by 5 degrees and 2 %, against the 64^3 mesh of the same shape: the alignment
    ends below the rms of the unmoved pair (the discretisation difference of the two lattices) plus eps32 extent.  The rms is the
    objective of the point metric and of no other, so the run that is held to it ends with point steps: the plane metric brings the
    mesh into reach and the point metric, which never raises the rms (Besl-McKay), finishes from its matrix.  The plane metric alone
    minimises the distances along the normals, and on this rough surface (352 965 vertices, lattice difference 1.08e-2 at an extent of
    0.5) its fixed point has a larger rms than the unmoved pair: measured on the MI355X, 1.80823e-2 -> 1.09755e-2 in 30 plane steps
    against 1.08272e-2 unmoved, then 1.08055e-2 after 28 point steps; the point metric from the unmoved pose itself ends at 1.08054e-2."""
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('small')).eval().requires_grad_(False)).cuda()
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(0, 1).cuda(), synthetic.conditioning_camera().cuda(), truncation_psi=0.7, truncation_cutoff=14)
        mesh = {'uvcoords_image': synthetic.uv_conditions([0]).cuda()}
    fine = g.extract_geometry(ws, mesh, resolution=128, level=0.0, keep='largest', noise_mode='const')[0]
    coarse = g.extract_geometry(ws, mesh, resolution=64, level=0.0, keep='largest', noise_mode='const')[0]
    grid = geometry.TriangleGrid(coarse['verts'], coarse['faces'])
    unmoved = geometry.align_mesh(fine['verts'], coarse['verts'], coarse['faces'], iterations=0, grid=grid)
    T = similarity(1.02, 5.0, (0.01, -0.005, 0.008))
    src = dev(moved(fine['verts'].cpu().numpy(), T))
    plane = geometry.align_mesh((src, fine['faces']), coarse['verts'], coarse['faces'], metric='plane', scale=True, iterations=30, grid=grid)
    r = geometry.align_mesh((src, fine['faces']), coarse['verts'], coarse['faces'], metric='point', scale=True, iterations=30,
                            init=plane['matrix'], grid=grid)
    print(f'{src.shape[0]} vertices onto {coarse["faces"].shape[0]} triangles: rms {plane["rms_history"][0]:.6g} -> {plane["rms"]:.6g} in '
          f'{plane["iterations"]} plane steps -> {r["rms"]:.6g} in {r["iterations"]} point steps (unmoved pair {unmoved["rms"]:.6g}), '
          f'scale {r["scale"]:.6g}, converged {r["converged"]}')
    assert unmoved['iterations'] == 0 and len(unmoved['rms_history']) == 1
    assert np.isfinite(plane['matrix']).all() and plane['iterations'] >= 1 and plane['rms'] < plane['rms_history'][0]
    assert np.isfinite(r['matrix']).all() and r['iterations'] >= 1
    h = r['rms_history']
    assert all(h[k + 1] <= h[k] * (1 + 4 * EPS32) for k in range(len(h) - 1))
    assert r['rms'] < unmoved['rms'] + EPS32 * grid.extent
