"""The winding number, the signed distance, mesh -> volume and the volumetric IoU on the host: the NumPy restatements that are the
definitions (geometry._winding_numpy and the functions made of it).  No GPU needed.  The shapes are shared with test_winding_gpu.py."""
import functools

import numpy as np
import pytest

from invertavatar_amd import geometry

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------ shapes (all wound outward unless said otherwise)

def _outward(verts, faces):
    assert geometry.signed_volume(verts, faces) > 0
    return verts.astype(F32), faces.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _sphere_cached(rings, segments):
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, rings):
        th = np.pi * i / rings
        for j in range(segments):
            ph = 2 * np.pi * j / segments
            v.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    v.append((0.0, 0.0, -1.0))
    f = []
    ring = lambda i, j: 1 + (i - 1) * segments + j % segments
    for j in range(segments):
        f.append((0, ring(1, j), ring(1, j + 1)))
        f.append((len(v) - 1, ring(rings - 1, j + 1), ring(rings - 1, j)))
    for i in range(1, rings - 1):
        for j in range(segments):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return _outward(np.array(v), np.array(f))


def sphere(rings=12, segments=16, radius=1.0, centre=(0.0, 0.0, 0.0)):
    v, f = _sphere_cached(rings, segments)
    return (v.astype(np.float64) * radius + np.array(centre)).astype(F32), f.copy()


def cube():
    v = np.array([(x, y, z) for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return _outward(v, np.array(f))


def torus(major=1.0, minor=0.4, nu=16, nv=8):
    v = [((major + minor * np.cos(2 * np.pi * j / nv)) * np.cos(2 * np.pi * i / nu),
          (major + minor * np.cos(2 * np.pi * j / nv)) * np.sin(2 * np.pi * i / nu), minor * np.sin(2 * np.pi * j / nv))
         for i in range(nu) for j in range(nv)]
    at = lambda i, j: (i % nu) * nv + j % nv
    f = []
    for i in range(nu):
        for j in range(nv):
            f.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
            f.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
    return _outward(np.array(v), np.array(f))


def join(*meshes):
    verts, faces, base = [], [], 0
    for v, f in meshes:
        verts.append(v)
        faces.append(f + base)
        base += v.shape[0]
    return np.concatenate(verts).astype(F32), np.concatenate(faces)


def open_sphere(rings=24, segments=48):
    """The sphere without its cap: the faces whose centroid has z >= 0.7 are removed."""
    v, f = sphere(rings, segments)
    return v, f[v[f].mean(1)[:, 2] < 0.7]


def shell(rings=12, segments=16):
    """A sphere of radius 1 with an inward-wound sphere of radius 0.5 inside it."""
    inner_v, inner_f = sphere(rings, segments, 0.5)
    return join(sphere(rings, segments), (inner_v, inner_f[:, ::-1]))


def two_spheres(rings=8, segments=12):
    return join(sphere(rings, segments, 0.6, (-1.0, 0.1, 0.0)), sphere(rings, segments, 0.5, (0.9, 0.0, 0.2)))


def pushed_samples(verts, faces, n=64, seed=0):
    """Surface samples moved by +-delta along their face normal, delta = 1e-2 and 1e-3 of the extent: (points [4 n, 3], outside bool)."""
    pts, idx = geometry.sample_surface(verts, faces, n, seed)
    nrm = geometry.face_normals(verts, faces)[idx]
    extent = float(np.abs(verts).max())
    out, side = [], []
    for delta in (1e-2 * extent, 1e-3 * extent):
        for s in (1.0, -1.0):
            out.append((pts.astype(np.float64) + s * delta * nrm).astype(F32))
            side.append(np.full(n, s > 0))
    return np.concatenate(out), np.concatenate(side)


def mc_sphere(res=24, radius=0.4, centre=(0.03, -0.02, 0.05)):
    """(field [res^3], level, origin, spacing, verts, faces): marching cubes of an analytic sphere field on the lattice of [-1, 1]^3."""
    org, spc = (-1.0,) * 3, (2.0 / (res - 1),) * 3
    ax = [(F32(org[a]) + np.arange(res, dtype=F32) * F32(spc[a])).astype(np.float64) for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing='ij')
    field = (radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(F32)
    v, f = geometry.marching_cubes(field, 0.0, org, spc)
    return field, 0.0, org, spc, v, f


def mc_torus(res=24, major=0.45, minor=0.2, centre=(0.02, 0.03, -0.04)):
    org, spc = (-1.0,) * 3, (2.0 / (res - 1),) * 3
    ax = [(F32(org[a]) + np.arange(res, dtype=F32) * F32(spc[a])).astype(np.float64) for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing='ij')
    x, y, z = x - centre[0], y - centre[1], z - centre[2]
    field = (minor - np.sqrt((np.sqrt(x * x + y * y) - major) ** 2 + z * z)).astype(F32)
    v, f = geometry.marching_cubes(field, 0.0, org, spc)
    return field, 0.0, org, spc, v, f


def _w(points, verts, faces, dtype=np.float64):
    return geometry._winding_numpy(np.asarray(points, dtype=F32), verts, faces, dtype)[0]


# ------------------------------------------------------------------ the definition

@pytest.mark.parametrize('s,d', [(1.0, 1.0), (0.5, 2.0), (2.0, 0.25), (1.0, 10.0), (0.125, 0.5)])
def test_square_against_the_closed_form(s, d):
    verts = np.array([(-s, -s, 0), (s, -s, 0), (s, s, 0), (-s, s, 0)], dtype=F32)          # normal +z
    faces = np.array([(0, 1, 2), (0, 2, 3)])
    want = 4 * np.arctan(s * s / (d * np.sqrt(2 * s * s + d * d))) / (4 * np.pi)
    below = np.array([(0.0, 0.0, -d)])
    assert abs(_w(below, verts, faces)[0] - want) <= 1e-12                               # the normal points away from the query
    assert abs(_w(-below, verts, faces)[0] + want) <= 1e-12
    assert abs(_w(below, verts, faces[:, ::-1])[0] + want) <= 1e-12                      # reversed winding
    assert geometry._winding_numpy(below, verts, faces)[1][0] == pytest.approx(want, abs=1e-12)


IN_OUT = {
    'sphere': (sphere, [(0, 0, 0), (0.3, -0.2, 0.5), (0, 0, 0.9)], [(0, 0, 1.2), (2, 1, 0), (-30, 5, 1)]),
    'cube': (cube, [(0, 0, 0), (0.9, -0.9, 0.5), (0.99, 0.99, 0.99)], [(1.1, 0, 0), (1.01, 1.01, 1.01), (0, -7, 0)]),
    'torus': (torus, [(1.0, 0, 0), (0, -1.2, 0.1), (-0.75, 0, -0.2)], [(0, 0, 0), (0, 0, 0.5), (1.5, 0, 0), (3, 3, 3)]),
}


@pytest.mark.parametrize('name', sorted(IN_OUT))
def test_closed_meshes_give_one_inside_and_zero_outside(name):
    make, inner, outer = IN_OUT[name]
    verts, faces = make()
    w_in, w_out = _w(inner, verts, faces), _w(outer, verts, faces)
    print(name, 'max |w - 1| inside', np.abs(w_in - 1).max(), 'max |w| outside', np.abs(w_out).max())
    assert np.abs(w_in - 1).max() <= 1e-12 and np.abs(w_out).max() <= 1e-12
    twice = join((verts, faces), (verts, faces))
    assert np.abs(_w(inner, *twice) - 2).max() <= 1e-12
    assert geometry.inside(np.array(inner, dtype=F32), verts, faces).all() and not geometry.inside(np.array(outer, dtype=F32), verts, faces).any()


def test_shell_has_an_empty_cavity():
    verts, faces = shell()
    w = _w([(0, 0, 0), (0.2, 0.1, -0.1), (0.7, 0, 0), (0, -0.8, 0.1), (1.5, 0, 0)], verts, faces)
    assert np.abs(w - np.array([0, 0, 1, 1, 0])).max() <= 1e-12


def test_open_mesh_degrades_smoothly():
    verts, faces = open_sphere()
    deep, far = _w([(0, 0, -0.5)], verts, faces)[0], _w([(0, 0, -6.0), (5, 0, 0), (0, 0, 6.0)], verts, faces)
    print('open sphere: deep inside', deep, 'far outside', far)
    assert 0.5 < deep < 1.0
    assert np.abs(far).max() < 0.1


def test_degenerate_input():
    verts, faces = sphere()
    pts = np.array([(0.1, 0.2, 0.3), (2.0, 0.0, 0.0)], dtype=F32)
    base = _w(pts, verts, faces)
    nan_vert = np.concatenate([verts, [[np.nan, 0, 0]], [[0.5, 0.5, 3.0]]]).astype(F32)
    extra = np.concatenate([faces, [[0, 0, 5]], [[3, 7, 7]],                              # without area
                            [[0, 1, len(verts)]],                                         # a NaN vertex
                            [[0, 1, len(nan_vert)]], [[-1, 2, 3]]])                       # out of range
    assert np.array_equal(_w(pts, nan_vert, extra), base)
    line = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0)], dtype=F32)
    assert np.array_equal(_w(pts, line, np.array([(0, 1, 2), (1, 1, 1)])), np.zeros(2))
    w = _w(np.array([(np.nan, 0, 0), (0, np.inf, 0), (0, 0, 0)], dtype=F32), verts, faces)
    assert np.isnan(w[0]) and np.isnan(w[1]) and abs(w[2] - 1) <= 1e-12
    assert np.array_equal(_w(pts, verts, np.zeros((0, 3), dtype=np.int64)), np.zeros(2))
    assert np.array_equal(geometry.winding_number(pts, np.zeros((0, 3), dtype=F32), np.zeros((0, 3), dtype=np.int64)), np.zeros(2))
    assert geometry.winding_number(np.zeros((2, 5, 3), dtype=F32), verts, faces).shape == (2, 5)


def test_the_sum_is_chunked_as_the_kernel_chunks_it():
    """The constants the restatement shares with the kernel, and the purity that follows from the fixed association."""
    from invertavatar_amd import hipops
    assert hipops.winding_layout() == (hipops.WINDING_TILE, hipops.WINDING_CHUNK, hipops.WINDING_POINTS)
    assert geometry.WINDING_CHUNK == hipops.WINDING_CHUNK and hipops.WINDING_CHUNK % hipops.WINDING_TILE == 0
    verts, faces = sphere(24, 48)
    faces = np.concatenate([faces, faces[:300]])                                          # more than one chunk
    assert faces.shape[0] > geometry.WINDING_CHUNK
    pts = np.random.default_rng(0).uniform(-1.5, 1.5, (40, 3)).astype(F32)
    w = geometry._winding_numpy(pts, verts, faces, F32)[0]
    perm = np.random.default_rng(1).permutation(40)
    assert np.array_equal(geometry._winding_numpy(pts[perm], verts, faces, F32)[0], w[perm])
    assert np.array_equal(geometry._winding_numpy(pts[5:9], verts, faces, F32, pairs=1000)[0], w[5:9])


# ------------------------------------------------------------------ signed distance

@pytest.mark.parametrize('make', [sphere, torus])
def test_signed_distance_has_the_sign_of_the_push(make):
    verts, faces = make()
    pts, outside = pushed_samples(verts, faces)
    r = geometry.signed_distance(pts, verts, faces)
    c = geometry.closest_point(pts, verts, faces)
    for k in ('dist', 'face', 'point'):
        assert np.array_equal(r[k], c[k]) and r[k].dtype == c[k].dtype
    assert np.isfinite(r['sdf']).all() and (r['dist'] > 0).all()
    assert np.array_equal(r['sdf'] > 0, outside) and np.array_equal(r['sdf'] < 0, ~outside)
    assert np.array_equal(np.abs(r['sdf']), r['dist'])
    assert np.abs(r['winding'] - np.where(outside, 0.0, 1.0)).max() <= 1e-9


# ------------------------------------------------------------------ mesh -> volume

def turned(mesh):
    """The mesh in a generic orientation.  The lattice is fitted to the box of the mesh, so the extreme vertices of a shape that is
    symmetric about the axes (a pole of the sphere, the equator of the torus) are lattice points, where the sign is undefined."""
    verts, faces = mesh
    R = geometry._rodrigues(np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0) * 0.3)
    return (verts.astype(np.float64) @ R.T).astype(F32), faces


CLOSED = {'sphere': lambda: turned(sphere(8, 12)), 'torus': lambda: turned(torus()), 'two_spheres': lambda: turned(two_spheres()),
          'shell': lambda: turned(shell(8, 12))}
LATTICES = {'cubic': dict(resolution=16), 'unequal': dict(resolution=(17, 19, 23))}


@pytest.mark.parametrize('lattice', sorted(LATTICES))
@pytest.mark.parametrize('name', sorted(CLOSED))
def test_regions_and_winding_agree(name, lattice):
    verts, faces = CLOSED[name]()
    a = geometry.mesh_to_volume(verts, faces, sign='regions', **LATTICES[lattice])
    b = geometry.mesh_to_volume(verts, faces, sign='winding', **LATTICES[lattice])
    print(name, lattice, a['inside'].shape, a['spacing'], a['info'], b['info'])
    assert a['info']['mode'] == 'regions' and b['info']['mode'] == 'winding'
    assert np.array_equal(a['inside'], b['inside']) and a['inside'].any() and not a['inside'].all()
    assert a['sdf'].dtype == np.float32 and np.array_equal(a['sdf'].view(np.int32), b['sdf'].view(np.int32))
    assert np.array_equal(np.signbit(a['sdf']), a['inside'])                               # (a point on the surface: -0 or +0)
    assert a['info']['regions'] >= 2 and a['info']['evaluations'] == a['info']['regions'] + a['info']['band'] < a['inside'].size
    assert b['info']['evaluations'] == a['inside'].size
    auto = geometry.mesh_to_volume(verts, faces, **LATTICES[lattice])
    assert auto['info']['mode'] == 'regions' and np.array_equal(auto['inside'], a['inside'])
    if lattice == 'unequal':
        assert a['inside'].shape == (17, 19, 23) and len(set(np.round(a['spacing'], 6))) == 3
    else:
        assert max(a['inside'].shape) == 16 and len(set(a['spacing'])) == 1


def test_auto_takes_winding_for_an_open_mesh():
    verts, faces = open_sphere(8, 12)
    r = geometry.mesh_to_volume(verts, faces, 12)
    assert r['info']['mode'] == 'winding' and r['info']['evaluations'] == r['inside'].size
    assert r['inside'].any() and not r['inside'].all()


def test_lattice_is_the_padded_box():
    verts, faces = sphere(8, 12, 0.5, (0.25, 0.0, -1.0))
    verts = verts * np.array([2.0, 1.0, 0.5], dtype=F32)
    r = geometry.mesh_to_volume(verts, faces, 20, padding=3)
    h = r['spacing'][0]
    assert r['inside'].shape[0] == 20 and r['spacing'] == (h, h, h) and h == pytest.approx(2.0 / 13, rel=1e-6)
    lo, hi = verts.min(0), verts.max(0)
    for a in range(3):
        n = r['inside'].shape[a]
        assert r['origin'][a] <= lo[a] - 3 * h + 1e-6 and r['origin'][a] + (n - 1) * h >= hi[a] + 3 * h - 1e-6
    with pytest.raises(ValueError):
        geometry.mesh_to_volume(verts, faces, 5, padding=2)
    with pytest.raises(ValueError):
        geometry.mesh_to_volume(verts, faces, 16, sign='normals')


@pytest.mark.parametrize('make', [mc_sphere, mc_torus])
def test_round_trip_through_marching_cubes(make):
    field, level, org, spc, verts, faces = make()
    assert not (field == F32(level)).any() and faces.shape[0] > 100
    lo, hi = verts.min(0), verts.max(0)
    assert (lo > -1.0 + spc[0]).all() and (hi < 1.0 - spc[0]).all()                        # strictly inside the box
    r = geometry.mesh_to_volume(verts, faces, field.shape, origin=org, spacing=spc)
    print(make.__name__, faces.shape[0], 'faces', r['info'])
    assert r['info']['mode'] == 'regions'
    assert np.array_equal(r['inside'], field > F32(level))


# ------------------------------------------------------------------ volumetric IoU

def test_volume_iou_of_a_mesh_with_itself_and_of_disjoint_meshes():
    verts, faces = sphere(8, 12)
    same = geometry.volume_iou(verts, faces, verts, faces, resolution=16)
    assert same['iou'] == 1.0 and same['intersection'] == same['union'] == same['volume_a'] > 0
    far = geometry.volume_iou(verts, faces, verts + np.array([3.0, 0, 0], dtype=F32), faces, resolution=24)
    assert far['iou'] == 0.0 and far['intersection'] == 0.0 and far['volume_a'] > 0 and far['volume_b'] > 0


def iou_case(res=24, r=0.6):
    """Concentric spheres: the IoU of two scaled copies of one mesh is (r / R)^3.  -> (meshes, the value, the bound, the lattice).  A
    lattice point can only be counted on the wrong side of a surface that cuts its cell, so the bound is the share of the lattice
    points within one cell diagonal of either surface, from closest_point's distances (not from the masks under test)."""
    big, faces = sphere(8, 12)
    small = (big * F32(r)).astype(F32)
    dims, org, spc = geometry._volume_lattice(geometry._finite_box(big), res, None, None, 2)
    pts = np.stack(np.meshgrid(*geometry._lattice_axes(dims, org, spc), indexing='ij'), -1).reshape(-1, 3)
    diag = float(np.sqrt(3.0) * spc[0])
    near = (geometry.closest_point(pts, big, faces)['dist'] <= diag) | (geometry.closest_point(pts, small, faces)['dist'] <= diag)
    return (small, faces, big, faces), r ** 3, float(near.mean()), dims


def test_volume_iou_of_concentric_spheres():
    meshes, want, bound, dims = iou_case()
    got = geometry.volume_iou(*meshes, resolution=24)
    print('iou', got['iou'], 'expected', want, 'bound', bound)
    assert tuple(got['resolution']) == dims and 0 < bound < 1
    assert abs(got['iou'] - want) <= bound
    assert got['intersection'] == got['volume_a'] and got['union'] == got['volume_b']


# ------------------------------------------------------------------ surface_distance(signed=True)

UNSIGNED_KEYS = {'mean_ab', 'rms_ab', 'max_ab', 'mean_ba', 'rms_ba', 'max_ba', 'chamfer', 'chamfer_sq', 'hausdorff', 'thresholds', 'precision',
                 'recall', 'fscore', 'normal_consistency', 'n_a', 'n_b', 'skipped_ab', 'skipped_ba'}


def test_surface_distance_signed():
    big, faces = sphere(12, 16, 1.05)
    unit, _ = sphere(12, 16)
    plain = geometry.surface_distance(big, faces, unit, faces)
    assert set(plain) == UNSIGNED_KEYS and set(geometry.surface_distance(big, faces, unit, faces, signed=False)) == UNSIGNED_KEYS
    res = geometry.surface_distance(big, faces, unit, faces, signed=True)
    assert set(res) == UNSIGNED_KEYS | {'mean_signed_ab', 'mean_signed_ba', 'inside_share_ab', 'inside_share_ba'}
    assert all(res[k] == plain[k] for k in UNSIGNED_KEYS)
    assert res['mean_signed_ab'] > 0 and res['inside_share_ab'] == 0.0 and res['inside_share_ba'] == 1.0
    assert res['mean_signed_ab'] == pytest.approx(res['mean_ab']) and res['mean_signed_ba'] == pytest.approx(-res['mean_ba'])


def test_cli_signed_and_iou(tmp_path):
    from invertavatar_amd import geometry_metrics
    big, faces = sphere(8, 12, 1.05)
    unit, _ = sphere(8, 12)
    geometry.write_ply(str(tmp_path / 'a.ply'), big, faces)
    geometry.write_ply(str(tmp_path / 'b.ply'), unit, faces)
    base = ['--pred', str(tmp_path / 'a.ply'), '--gt', str(tmp_path / 'b.ply'), '--device', 'cpu']
    plain = geometry_metrics.main(base + ['--out', str(tmp_path / 'p.json'), '--error-ply', str(tmp_path / 'p.ply')])
    assert set(plain) == UNSIGNED_KEYS | {'pred_vertices', 'pred_faces', 'gt_vertices', 'gt_faces'}
    col = geometry.read_ply(str(tmp_path / 'p.ply'))[2]
    assert (col[:, 1:] == 0).all()                                                         # the unsigned map: black to red
    res = geometry_metrics.main(base + ['--out', str(tmp_path / 's.json'), '--error-ply', str(tmp_path / 's.ply'), '--signed', '--iou', '16'])
    assert res['inside_share_ab'] == 0.0 and res['inside_share_ba'] == 1.0 and 0.5 < res['volume_iou']['iou'] < 1.0
    col = geometry.read_ply(str(tmp_path / 's.ply'))[2]
    assert (col[:, 0] == 255).all() and (col[:, 1] == col[:, 2]).all() and (col[:, 1] < 255).all()     # outside: towards red
    assert 'inside share' in geometry_metrics.summary(res) and 'inside share' not in geometry_metrics.summary(plain)
