"""Alignment without a GPU: ``fit_transform`` against exact correspondences, the NumPy restatement of ``align_mesh`` (the definition) on a
small marching-cubes mesh without symmetry against the transform that was applied, with the tolerance taken from the restatement's own
float32 run (``4 * e32 + eps32 * extent``, never from the code under test); monotonicity of the point-to-point residual; trimming;
``init``; ``compare_meshes(align=...)`` and the command line.  The helpers here also serve tests/test_align_gpu.py."""
import json

import numpy as np
import pytest

from invertavatar_amd import geometry, geometry_metrics
from test_surface_distance_cpu import EPS32, F32, extent_of

EPS64 = float(np.finfo(np.float64).eps)


# ------------------------------------------------------------------ the shared case

def bumpy_mesh():
    """Marching-cubes mesh (702 vertices, 1400 faces) of an ellipsoid with two bumps, which leave it no symmetry: 20^3 lattice over
    [-1.2, 1.2]^3, level 0."""
    ax, lo, step = geometry.lattice_axis(20, 2.4, 0.0)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1).astype(np.float64)
    bump = lambda c, w: np.exp(-((g - np.array(c)) ** 2).sum(-1) / w)          # noqa: E731
    field = 0.9 - np.sqrt(g[..., 0] ** 2 + (g[..., 1] / 0.7) ** 2 + (g[..., 2] / 0.85) ** 2) + 0.25 * bump((0.6, 0.3, -0.2), 0.08) \
        + 0.2 * bump((-0.3, -0.4, 0.5), 0.05)
    return geometry.marching_cubes(field.astype(F32), 0.0, (float(lo),) * 3, (float(step),) * 3)


def similarity(scale=1.0, degrees=12.0, shift=(0.08, -0.04, 0.027), axis=(1.0, 2.0, 3.0)):
    ax = np.array(axis) / np.linalg.norm(axis)
    M = np.eye(4)
    M[:3, :3] = scale * geometry._rodrigues(ax * np.deg2rad(degrees))
    M[:3, 3] = shift
    return M


def moved(points, T):
    """The points under the inverse of T (float64, rounded to float32 once): aligning them has the answer T."""
    Ti = np.linalg.inv(T)
    return (np.asarray(points, dtype=np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32)


def restatement(src, verts, faces, dtype=np.float64, **kw):
    """The NumPy restatement with the closest-point search in ``dtype``."""
    a = dict(metric='plane', scale=False, iterations=12, tol=1e-6, max_dist=None, trim=1.0)
    a.update(kw)
    return geometry._align_numpy(src, verts, faces, np.eye(4), a['metric'], a['scale'], a['iterations'], a['tol'], a['max_dist'], a['trim'],
                                 dtype=dtype)


class Case:
    """Mesh, 400 surface samples (seed 3) moved by the inverse of a known transform, the restatement's float64 and float32 runs."""
    def __init__(self, scale):
        self.verts, self.faces = bumpy_mesh()
        self.samples, self.sample_faces = geometry.sample_surface(self.verts, self.faces, 400, seed=3)
        self.truth = similarity(scale)
        self.with_scale = scale != 1.0
        self.src = moved(self.samples, self.truth)
        self.extent = extent_of(self.verts)
        self.r64 = restatement(self.src, self.verts, self.faces, scale=self.with_scale)
        r32 = restatement(self.src, self.verts, self.faces, np.float32, scale=self.with_scale)
        self.e32 = float(np.abs(r32['matrix'] - self.r64['matrix']).max())
        self.tol = 4 * self.e32 + EPS32 * self.extent


_cases = {}


def shared_case(scale):
    if scale not in _cases:
        _cases[scale] = Case(scale)
    return _cases[scale]


def outlier_source(case):
    """The case's source with 40 of the 400 points replaced by points 0.5 off the surface (along the face normal)."""
    nrm = geometry.face_normals(case.verts, case.faces)[case.sample_faces]
    pts = case.samples.astype(np.float64).copy()
    pts[::10] += 0.5 * nrm[::10]
    return moved(pts, case.truth)


# ------------------------------------------------------------------ tests

@pytest.mark.parametrize('scale', [False, True])
def test_fit_transform_recovers_a_similarity(scale):
    rs = np.random.RandomState(5)
    src = rs.normal(size=(10, 3))
    T = similarity(1.3 if scale else 1.0, 71.0, (0.4, -2.0, 0.7), (0.3, -1.0, 0.2))
    dst = src @ T[:3, :3].T + T[:3, 3]
    M = geometry.fit_transform(src, dst, scale=scale)
    assert M.dtype == np.float64 and M.shape == (4, 4) and np.array_equal(M[3], [0, 0, 0, 1])
    assert np.abs(M - T).max() <= 1e-12
    Mw = geometry.fit_transform(np.concatenate([src, [[9.0, 9, 9]]]), np.concatenate([dst, [[0.0, 0, 0]]]), scale=scale, weights=[1.0] * 10 + [0.0])
    assert np.abs(Mw - T).max() <= 1e-12
    mirrored = dst * np.array([-1.0, 1.0, 1.0])
    R = geometry.fit_transform(src, mirrored, scale=scale)[:3, :3]
    assert np.linalg.det(R) > 0 and abs(np.linalg.det(R / np.cbrt(np.linalg.det(R))) - 1.0) <= 1e-12
    with pytest.raises(ValueError):
        geometry.fit_transform(src[:2], dst[:2], scale=scale)
    with pytest.raises(ValueError):
        geometry.fit_transform(np.tile(src[:1], (5, 1)), dst[:5], scale=scale)


def test_transform_points_is_the_fp32_product():
    rs = np.random.RandomState(2)
    x = rs.normal(size=(5, 7, 3)).astype(F32)
    M = similarity(1.1, 33.0)
    y = geometry.transform_points(x, M)
    assert y.dtype == F32 and y.shape == x.shape
    ref = x.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    bound = 3 * EPS32 * (np.abs(x).astype(np.float64) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3]))
    assert (np.abs(y - ref) <= bound).all()
    x[0, 0, 1] = np.nan
    assert not np.isfinite(geometry.transform_points(x, M)[0, 0]).any()
    with pytest.raises(ValueError):
        geometry.transform_points(x, np.eye(3))


@pytest.mark.parametrize('scale', [1.0, 1.05])
def test_plane_metric_recovers_the_transform(scale):
    c = shared_case(scale)
    r = geometry.align_mesh(c.src, c.verts, c.faces, metric='plane', scale=c.with_scale, iterations=12)
    err = float(np.abs(r['matrix'] - c.truth).max())
    print(f'scale {scale}: {r["iterations"]} steps, rms {r["rms_history"]}, |M - truth| = {err:.3g}, e32 = {c.e32:.3g}, tolerance {c.tol:.3g}')
    assert r['converged'] and r['iterations'] < 12 and len(r['rms_history']) == r['iterations'] + 1
    assert err <= c.tol
    assert np.array_equal(r['matrix'], c.r64['matrix']) and r['rms_history'] == c.r64['rms_history']      # the public path is the restatement
    assert abs(r['scale'] - scale) <= c.tol and np.abs(r['rotation'] @ r['rotation'].T - np.eye(3)).max() <= 1e-12
    assert np.array_equal(r['translation'], r['matrix'][:3, 3]) and r['inliers'] == 400 and r['rms'] == r['rms_history'][-1]
    pair = geometry.align_mesh((c.src, np.zeros((0, 3), dtype=np.int64)), c.verts, c.faces, scale=c.with_scale, iterations=12)
    assert np.array_equal(pair['matrix'], r['matrix'])


def test_point_metric_residual_never_rises():
    c = shared_case(1.0)
    r = geometry.align_mesh(c.src, c.verts, c.faces, metric='point', iterations=10)
    h = r['rms_history']
    print('point rms history', h)
    assert len(h) == 11 and r['iterations'] == 10 and not r['converged']
    assert all(h[k + 1] <= h[k] * (1 + 4 * EPS32) for k in range(10))
    assert h[-1] < 0.5 * h[0]


def test_trimming_rejects_outliers():
    c = shared_case(1.0)
    src = outlier_source(c)
    trimmed = geometry.align_mesh(src, c.verts, c.faces, iterations=12, trim=0.85)
    plain = geometry.align_mesh(src, c.verts, c.faces, iterations=12, trim=1.0)
    e_trim, e_plain = float(np.abs(trimmed['matrix'] - c.truth).max()), float(np.abs(plain['matrix'] - c.truth).max())
    print(f'trim 0.85: error {e_trim:.3g} with {trimmed["inliers"]} pairs; trim 1: error {e_plain:.3g}; tolerance {c.tol:.3g}')
    assert trimmed['inliers'] == 340 and plain['inliers'] == 400
    assert e_trim <= c.tol < e_plain
    capped = geometry.align_mesh(src, c.verts, c.faces, iterations=12, max_dist=0.3, init=trimmed['matrix'])
    assert capped['inliers'] == 360 and capped['iterations'] <= 1
    with_nan = c.src.copy()
    with_nan[7] = np.nan
    r = geometry.align_mesh(with_nan, c.verts, c.faces, iterations=12)
    assert r['inliers'] == 399 and np.isfinite(r['matrix']).all() and float(np.abs(r['matrix'] - c.truth).max()) <= c.tol
    with pytest.raises(ValueError):
        geometry.align_mesh(with_nan[5:10], c.verts, c.faces)                           # 4 pairs count, the plane metric needs 6
    with pytest.raises(ValueError):
        geometry.align_mesh(c.src, c.verts, c.faces[:0])


def test_init_centroid_and_given_matrix():
    """A shift of 0.5 (0.29 along every axis, beside the 12 degrees): within a budget of 5 steps the centroid start converges and the
    identity start does not and ends at a larger rms.  (Given more steps the plane metric comes back from this shift on its own, 7 steps
    in the float64 restatement, so the budget is part of the case.)"""
    c = shared_case(1.0)
    far = similarity(1.0, 12.0, (0.29, 0.29, 0.29))
    src = moved(c.samples, far)
    a = geometry.align_mesh(src, c.verts, c.faces, iterations=5, init='centroid')
    b = geometry.align_mesh(src, c.verts, c.faces, iterations=5, init='identity')
    print(f'from a 0.5 shift: centroid start rms {a["rms"]:.3g} ({a["iterations"]} steps), identity start rms {b["rms"]:.3g}')
    assert a['converged'] and not b['converged'] and a['rms'] < b['rms'] and float(np.abs(a['matrix'] - far).max()) <= c.tol
    given = geometry.align_mesh(c.src, c.verts, c.faces, init=c.truth)
    assert given['iterations'] == 0 and given['converged'] and len(given['rms_history']) == 1 and np.array_equal(given['matrix'], c.truth)
    with pytest.raises(ValueError):
        geometry.align_mesh(c.src, c.verts, c.faces, init='nearest')
    with pytest.raises(ValueError):
        geometry.align_mesh(c.src, c.verts, c.faces, metric='line')


def test_compare_meshes_aligns_first(tmp_path):
    c = shared_case(1.0)
    pred = moved(c.verts, c.truth)
    plain = geometry_metrics.compare_meshes(pred, c.faces, c.verts, c.faces)
    res = geometry_metrics.compare_meshes(pred, c.faces, c.verts, c.faces, align='rigid', align_options={'iterations': 12})
    print(f'chamfer {plain["chamfer"]:.3g} unaligned, {res["chamfer"]:.3g} aligned, tolerance {c.tol:.3g}')
    assert 'alignment' not in plain and plain['chamfer'] > 0.01
    assert res['chamfer'] <= c.tol
    a = res['alignment']
    assert a['converged'] and a['rms_after'] < a['rms_before'] and abs(a['angle_deg'] - 12.0) < 1e-3 and abs(a['scale'] - 1.0) < 1e-12
    json.dumps(res)
    # the command line, through PLY files
    geometry.write_ply(str(tmp_path / 'pred.ply'), pred, c.faces)
    geometry.write_ply(str(tmp_path / 'gt.ply'), c.verts, c.faces)
    out = geometry_metrics.main(['--pred', str(tmp_path / 'pred.ply'), '--gt', str(tmp_path / 'gt.ply'), '--out', str(tmp_path / 'm.json'),
                                 '--align', 'rigid', '--align-iterations', '12', '--save-aligned', str(tmp_path / 'moved.ply'), '--device', 'cpu'])
    with open(tmp_path / 'm.json') as fh:
        stored = json.load(fh)
    assert stored['alignment'] == out['alignment'] == a and stored['chamfer'] == res['chamfer']
    back = geometry.read_ply(str(tmp_path / 'moved.ply'))[0]
    assert np.array_equal(back, geometry.transform_points(pred, np.array(a['matrix'])))        # the moved mesh, float32 through the PLY
    untouched = geometry_metrics.main(['--pred', str(tmp_path / 'pred.ply'), '--gt', str(tmp_path / 'gt.ply'), '--out', str(tmp_path / 'p.json'),
                                       '--device', 'cpu'])
    assert untouched == plain
