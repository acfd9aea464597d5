"""Surface ray casting on the CPU: the NumPy restatement of ia_raycast_volume on analytic and random fields (hits, depth, normals, the
first-hit property, edge cases), vertex normals, PLY normals, ``render_geometry`` and the CLI's rendered views."""
import os

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry, synthetic
from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
from test_geometry_cpu import sphere_field, torus_field


# ------------------------------------------------------------------ helpers (shared with test_raycast_gpu.py)

def pinhole_rays(cam, target, half_width, res):
    """res^2 unit rays from ``cam`` through a res x res grid of pixel centres on the square of ``half_width`` about ``target`` (the
    square spans the two axes other than the one from cam to target)."""
    cam, target = np.asarray(cam, np.float64), np.asarray(target, np.float64)
    fwd = target - cam
    fwd /= np.linalg.norm(fwd)
    up = np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    right = np.cross(up, fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    xs = ((np.arange(res) + 0.5) / res * 2 - 1) * half_width
    X, Y = np.meshgrid(xs, xs, indexing='ij')
    pts = target + X.reshape(-1, 1) * right + Y.reshape(-1, 1) * up
    d = pts - cam
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.broadcast_to(cam, d.shape).astype(np.float32).copy(), d.astype(np.float32)


def trilinear(vol, lo, step, p):
    """Trilinear interpolant of ``vol`` at world points p [m,3] (float64; inside the box)."""
    v = vol.astype(np.float64)
    n = np.array(v.shape)
    P = (p - np.asarray(lo, np.float64)) / np.asarray(step, np.float64)
    c = np.clip(np.floor(P).astype(np.int64), 0, n - 2)
    u = P - c
    out = np.zeros(len(p))
    for q in range(8):
        d = np.array([q & 1, (q >> 1) & 1, q >> 2])
        w = np.prod(np.where(d == 1, u, 1 - u), axis=1)
        out += w * v[c[:, 0] + d[0], c[:, 1] + d[1], c[:, 2] + d[2]]
    return out


def smooth_random_field(shape, seed):
    """A smooth random field: a few random plane waves (values of order 1, level 0 gives a tangled surface)."""
    rs = np.random.RandomState(seed)
    grids = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing='ij')
    f = np.zeros(shape)
    for _ in range(6):
        k = rs.randn(3) * 0.35
        f += np.cos(sum(k[a] * grids[a] for a in range(3)) + rs.uniform(0, 2 * np.pi))
    return (f / 2).astype(np.float32)


def sphere_scene(res=96):
    vol, c = sphere_field(64, 20)
    o, d = pinhole_rays((0.0, 0.0, -80.0), (0.0, 0.0, 0.0), 25.0, res)
    return vol, (-c,) * 3, (1.0, 1.0, 1.0), o, d


def analytic_sphere(o, d, r=20.0):
    o, d = o.astype(np.float64), d.astype(np.float64)
    b = (o * d).sum(1)
    dist = np.linalg.norm(np.cross(o, d), axis=1)
    t = -b - np.sqrt(np.maximum(b * b - ((o * o).sum(1) - r * r), 0.0))
    return dist, t


def box_clip(lo, step, n, o, d, t_min=0.0):
    """[t0, t1] of each ray inside the lattice box (float64), t0 > t1 for a miss."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(lo, np.float64) + (np.asarray(n) - 1) * np.asarray(step, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        ta, tb = (lo - o) / d, (hi - o) / d
    return np.maximum(np.minimum(ta, tb).max(1), t_min), np.maximum(ta, tb).min(1)


# ------------------------------------------------------------------ sphere

def test_sphere_hits_depth_normals():
    vol, lo, step, o, d = sphere_scene()
    out = geometry.raycast(vol, 0.0, lo, step, o, d)
    assert out['depth'].shape == (96 * 96,) and out['normal'].shape == (96 * 96, 3) and out['mask'].dtype == bool
    dist, t_true = analytic_sphere(o, d)
    m = out['mask']
    assert m[dist <= 18.5].all() and not m[dist >= 21.5].any()
    assert (out['depth'][~m] == 0).all() and (out['normal'][~m] == 0).all()
    core = dist <= 15
    assert core.sum() > 1000
    assert np.abs(out['depth'][core] - t_true[core]).max() <= 0.1
    p = o.astype(np.float64) + out['depth'][:, None].astype(np.float64) * d
    radial = p / np.linalg.norm(p, axis=1, keepdims=True)
    cosang = np.clip((out['normal'][core] * radial[core]).sum(1), -1, 1)
    assert np.degrees(np.arccos(cosang)).max() <= 2.0
    # the hit lies on the level set of the trilinear field
    f = trilinear(vol, lo, step, p[m])
    assert np.abs(f).max() <= 1e-4 * 1.0 * np.sqrt(3)          # max |grad| of r - |x| is 1 per axis


def test_torch_cpu_tensors_in_and_out():
    vol, lo, step, o, d = sphere_scene(16)
    a = geometry.raycast(vol, 0.0, lo, step, o.reshape(4, 4, 16, 3), d.reshape(4, 4, 16, 3))
    b = geometry.raycast(torch.from_numpy(vol), 0.0, lo, step, torch.from_numpy(o), torch.from_numpy(d))
    assert a['depth'].shape == (4, 4, 16) and a['normal'].shape == (4, 4, 16, 3)
    assert isinstance(b['depth'], torch.Tensor) and b['mask'].dtype == torch.bool
    assert np.array_equal(a['depth'].reshape(-1), b['depth'].numpy()) and np.array_equal(a['mask'].reshape(-1), b['mask'].numpy())


# ------------------------------------------------------------------ first-hit property

def _check_first_hit(vol, level, lo, step, o, d):
    out = geometry.raycast(vol, level, lo, step, o, d)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    t0, t1 = box_clip(lo, step, vol.shape, o64, d64)
    dt = (1.0 / 64) * np.min(step)                                  # 1/64 of a cell along the ray
    checked = 0
    for r in range(len(o)):
        if t0[r] > t1[r]:
            assert not out['mask'][r]
            continue
        end = out['depth'][r] if out['mask'][r] else t1[r]
        ts = np.arange(t0[r], end, dt)
        if out['mask'][r]:
            ts = ts[ts < end - dt]                                   # tolerance: one sample
        if ts.size == 0:
            continue
        f = trilinear(vol, lo, step, o64[r] + ts[:, None] * d64[r])
        assert not (f > level + 1e-6).any(), (r, out['mask'][r], ts[np.argmax(f > level)], end)
        checked += 1
    assert checked >= len(o) // 5
    return out


def test_first_hit_random_field():
    vol = smooth_random_field((20, 22, 18), 3)
    lo, step = (-10.0, -11.0, -9.0), (1.0, 1.0, 1.0)
    o, d = pinhole_rays((-30.0, 14.0, -40.0), (0.0, 0.0, 0.0), 16.0, 20)
    out = _check_first_hit(vol, 0.0, lo, step, o, d)
    assert 0 < out['mask'].sum() < len(o)


def test_first_hit_torus_anisotropic():
    vol = torus_field()
    step = (0.5, 1.0, 0.75)
    lo = tuple(-0.5 * (n - 1) * s for n, s in zip(vol.shape, step))
    o, d = pinhole_rays((5.0, 70.0, -20.0), (0.0, 0.0, 0.0), 34.0, 20)
    out = _check_first_hit(vol, 0.0, lo, step, o, d)
    assert out['mask'].sum() > 20


# ------------------------------------------------------------------ edge cases

def test_camera_inside_hits_at_clipped_start():
    vol, lo, step, _, _ = sphere_scene(8)
    d = np.random.RandomState(1).randn(50, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = np.zeros((50, 3), np.float32)
    out = geometry.raycast(vol, 0.0, lo, step, o, d)
    assert out['mask'].all() and (out['depth'] == 0).all()
    out = geometry.raycast(vol, 0.0, lo, step, o, d, t_min=1.5)
    assert out['mask'].all() and (out['depth'] == np.float32(1.5)).all()


def test_ray_lying_on_lattice_planes():
    vol, c = sphere_field(65, 20)                                   # lattice planes at integer coordinates, one through the centre
    o = np.array([[-50.0, 0.0, 0.0], [0.0, -50.0, 0.0], [0.0, 0.0, 50.0], [-50.0, 32.0, 0.0]], np.float32)
    d = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]], np.float32)   # the last runs along the box face
    out = geometry.raycast(vol, 0.0, (-c,) * 3, (1, 1, 1), o, d)
    assert out['mask'][:3].all() and not out['mask'][3]
    assert np.abs(out['depth'][:3] - 30.0).max() <= 1e-4
    assert np.abs(out['normal'][:3] + d[:3]).max() <= 1e-3


def test_nan_cells_have_no_surface():
    vol, lo, step, o, d = sphere_scene(24)
    base = geometry.raycast(vol, 0.0, lo, step, o, d)
    centre = int(np.argmin(analytic_sphere(o, d)[0]))
    hit = o[centre].astype(np.float64) + base['depth'][centre] * d[centre].astype(np.float64)
    P = np.floor(hit - np.asarray(lo)).astype(int)
    nanv = vol.copy()
    nanv[P[0] - 1:P[0] + 3, P[1] - 1:P[1] + 3, P[2] - 1:P[2] + 3] = np.nan
    out = geometry.raycast(nanv, 0.0, lo, step, o, d)
    assert out['mask'][centre] and out['depth'][centre] > base['depth'][centre] + 1.0
    assert np.isfinite(out['depth']).all() and np.isfinite(out['normal']).all()
    far = np.linalg.norm(o.astype(np.float64) + base['depth'][:, None] * d - hit, axis=1) > 8
    far &= base['mask']
    assert far.sum() > 50 and np.array_equal(out['depth'][far], base['depth'][far])
    allnan = geometry.raycast(np.full((6, 6, 6), np.nan, np.float32), 0.0, (0, 0, 0), (1, 1, 1), o[:10] * 0 - 3, d[:10] * 0 + 0.577)
    assert not allnan['mask'].any()


def test_empty_and_full_volumes():
    o, d = pinhole_rays((-20.0, 3.0, 4.0), (4.0, 4.0, 4.0), 3.0, 8)
    empty = geometry.raycast(np.full((9, 9, 9), -1, np.float32), 0.0, (0, 0, 0), (1, 1, 1), o, d)
    assert not empty['mask'].any() and (empty['depth'] == 0).all()
    full = geometry.raycast(np.full((9, 9, 9), 1, np.float32), 0.0, (0, 0, 0), (1, 1, 1), o, d)
    t0, t1 = box_clip((0, 0, 0), (1, 1, 1), (9, 9, 9), o.astype(np.float64), d.astype(np.float64))
    assert full['mask'].all() and np.abs(full['depth'] - t0).max() <= 1e-5


def test_bricks_restatement():
    rs = np.random.RandomState(4)
    vol = rs.randn(19, 10, 9).astype(np.float32)
    vol[:9, :9, :9] = np.nan
    b = geometry._bricks_numpy(vol)
    assert b.shape == (3, 2, 1, 2)
    assert b[0, 0, 0, 0] == np.inf and b[0, 0, 0, 1] == -np.inf
    ref = vol[8:17, 0:9, 0:9]
    assert b[1, 0, 0, 0] == np.nanmin(ref) and b[1, 0, 0, 1] == np.nanmax(ref)
    ref = vol[16:19, 8:10, 0:9]
    assert b[2, 1, 0, 0] == np.nanmin(ref) and b[2, 1, 0, 1] == np.nanmax(ref)


# ------------------------------------------------------------------ vertex normals and PLY

def test_vertex_normals_radial_and_ply_round_trip(tmp_path):
    vol, c = sphere_field(64, 20)
    v, f = geometry.marching_cubes(vol, 0.0, (-c,) * 3, (1, 1, 1))
    n = geometry.volume_normals(vol, v, (-c,) * 3, (1, 1, 1))
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert n.shape == v.shape and n.dtype == np.float32
    assert np.degrees(np.arccos(np.clip((n * radial).sum(1), -1, 1))).max() <= 2.0
    cols = np.random.RandomState(0).randint(0, 256, v.shape).astype(np.uint8)
    path = str(tmp_path / 'n.ply')
    geometry.write_ply(path, v, f, cols, normals=n)
    v2, f2, c2, n2 = geometry.read_ply(path, with_normals=True)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(c2, cols) and np.array_equal(n2, n)
    v3, f3, c3 = geometry.read_ply(path)
    assert np.array_equal(v3, v) and np.array_equal(c3, cols)


def test_write_ply_without_normals_is_unchanged(tmp_path):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]])
    c = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8)
    path = str(tmp_path / 'a.ply')
    geometry.write_ply(path, v, f, c)
    head = ('ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n'
            'property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1\nproperty list uchar int vertex_indices\n'
            'end_header\n').encode('ascii')
    body = b''.join(v[i].astype('<f4').tobytes() + c[i].tobytes() for i in range(3)) + b'\x03' + f[0].astype('<i4').tobytes()
    with open(path, 'rb') as fh:
        assert fh.read() == head + body
    v2, f2, c2, n2 = geometry.read_ply(path, with_normals=True)
    assert n2 is None and np.array_equal(v2, v)


def test_shade_headlight():
    n = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    d = torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    m = torch.tensor([True, False, True, True])
    s = geometry.shade(n, d, m)
    assert s.shape == (4, 1) and torch.allclose(s[:, 0], torch.tensor([1.0, 0.0, 0.25, 0.25]))


# ------------------------------------------------------------------ generator and CLI

@pytest.fixture(scope='module')
def small_setup():
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('small')).eval().requires_grad_(False))
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(3, 1), synthetic.conditioning_camera(), truncation_psi=0.7, truncation_cutoff=14)
    return g, ws, {'uvcoords_image': synthetic.uv_conditions([5])}


def test_render_geometry_shapes_cpu(small_setup):
    g, ws, mesh = small_setup
    cams = synthetic.camera_labels([0, 60])[None]                   # [1, 2, 25]
    out = g.render_geometry(ws, cams, mesh, resolution=24, volume_resolution=24, level=0.0, with_colors=True, noise_mode='const')
    assert out['depth'].shape == (1, 2, 1, 24, 24) and out['mask'].shape == (1, 2, 1, 24, 24) and out['mask'].dtype == torch.bool
    assert out['normal'].shape == (1, 2, 3, 24, 24) and out['shaded'].shape == (1, 2, 1, 24, 24) and out['rgb'].shape == (1, 2, 3, 24, 24)
    assert out['mask'].any() and (out['depth'][out['mask']] > 2.0).all()
    assert float(out['shaded'].min()) >= 0 and float(out['shaded'].max()) <= 1
    single = g.render_geometry(ws, cams[:, 0], mesh, resolution=24, volume_resolution=24, level=0.0, noise_mode='const')
    assert single['depth'].shape == (1, 1, 24, 24) and 'rgb' not in single
    assert torch.equal(single['depth'], out['depth'][:, 0])


def test_extract_geometry_normals_cpu(small_setup):
    g, ws, mesh = small_setup
    a = g.extract_geometry(ws, mesh, resolution=20, level=0.0, noise_mode='const')[0]
    b = g.extract_geometry(ws, mesh, resolution=20, level=0.0, with_normals=True, noise_mode='const')[0]
    assert 'normals' not in a and b['normals'].shape == b['verts'].shape and torch.equal(a['verts'], b['verts'])
    lens = b['normals'].norm(dim=1)
    assert ((lens - 1).abs() < 1e-5).float().mean() > 0.99


def test_cli_renders_views_cpu(tmp_path):
    from PIL import Image
    from invertavatar_amd import extract_geometry
    res = extract_geometry.main(['--seeds', '0', '--width', 'small', '--res', '32', '--level', '0', '--outdir', str(tmp_path),
                                 '--device', 'cpu', '--normals', '--views', '2', '--render-res', '48', '--save-depth'])
    path, out = res[0]
    for k in range(2):
        img = Image.open(tmp_path / f'seed0000_view{k:02d}.png')
        assert img.size == (48, 48) and img.mode == 'L'
    assert np.asarray(Image.open(tmp_path / 'seed0000_view00.png')).max() > 0
    assert np.load(tmp_path / 'seed0000_depth.npy').shape == (2, 48, 48)
    v, f, c, n = geometry.read_ply(path, with_normals=True)
    assert n is not None and n.shape == v.shape and np.array_equal(n, out['normals'].numpy())
    assert os.path.exists(path)
