"""Surface ray casting on the device: ia_raycast_volume against the NumPy restatement, bit-equality of the skip and dense paths, of
batched and single-view launches and from run to run, ia_volume_gradient against NumPy, the full-width generator end to end (hits
against the marching-cubes mesh) and the error paths of the ABI."""
import ctypes

import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, geometry, hipops, synthetic
from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
from test_geometry_cpu import sphere_field, torus_field
from test_raycast_cpu import analytic_sphere, pinhole_rays, smooth_random_field, sphere_scene

pytestmark = pytest.mark.gpu


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in arrays]


def _device_vs_numpy(vol, level, lo, step, o, d):
    vd, od, dd = _cuda(vol, o, d)
    dev = geometry.raycast(vd, level, lo, step, od, dd)
    ref = geometry.raycast(vol, level, lo, step, o, d)
    m_dev = dev['mask'].cpu().numpy()
    agree = (m_dev == ref['mask']).mean()
    both = m_dev & ref['mask']
    cell = float(min(step))
    dd_max = np.abs(dev['depth'].cpu().numpy()[both] - ref['depth'][both]).max() / cell
    dn_max = np.abs(dev['normal'].cpu().numpy()[both] - ref['normal'][both]).max()
    print(f'mask agreement {agree:.5f}, both hit {both.sum()}, max |d depth| {dd_max:.2e} cell, max |d normal| {dn_max:.2e}')
    assert agree >= 0.999 and both.sum() > 0
    assert dd_max <= 1e-3 and dn_max <= 1e-4
    return dev, ref


def test_sphere_device_matches_numpy():
    vol, lo, step, o, d = sphere_scene()
    dev, ref = _device_vs_numpy(vol, 0.0, lo, step, o, d)
    dist, _ = analytic_sphere(o, d)
    differ = dev['mask'].cpu().numpy() != ref['mask']
    assert ((dist[differ] > 18.5) & (dist[differ] < 21.5)).all()           # disagreements only at the silhouette


def test_torus_and_random_fields_device_matches_numpy():
    vol = torus_field()
    step = (0.5, 1.0, 0.75)
    lo = tuple(-0.5 * (n - 1) * s for n, s in zip(vol.shape, step))
    o, d = pinhole_rays((5.0, 70.0, -20.0), (0.0, 0.0, 0.0), 34.0, 64)
    _device_vs_numpy(vol, 0.0, lo, step, o, d)
    for seed, shape in ((3, (40, 44, 36)), (8, (33, 17, 50))):
        f = smooth_random_field(shape, seed)
        lo = tuple(-0.5 * (n - 1) for n in shape)
        o, d = pinhole_rays((-30.0, 14.0, -60.0), (0.0, 0.0, 0.0), 20.0, 64)
        _device_vs_numpy(f, 0.1, lo, (1.0, 1.0, 1.0), o, d)


def test_bricks_match_numpy():
    rs = np.random.RandomState(4)
    vol = rs.randn(37, 20, 9).astype(np.float32)
    vol[:9, :9, :9] = np.nan
    b = hipops.volume_bricks(*_cuda(vol))
    assert np.array_equal(b.cpu().numpy(), geometry._bricks_numpy(vol))


def test_skip_dense_batch_and_runs_bit_equal():
    vol = smooth_random_field((70, 64, 60), 5)
    vol[30:34, 10:50, 20:24] = np.nan
    lo, step = (-0.5, -0.4, -0.45), (1 / 69, 0.8 / 63, 0.9 / 59)
    vd = _cuda(vol)[0]
    views = [pinhole_rays((2.0 * np.sin(a), 0.3, 2.0 * np.cos(a)), (0.0, 0.0, 0.0), 0.6, 96) for a in (0.0, 1.0, 2.5)]
    o = torch.cat([_cuda(v[0])[0] for v in views])
    d = torch.cat([_cuda(v[1])[0] for v in views])
    bricks = hipops.volume_bricks(vd)
    for level in (0.3, 0.9, 1.4):
        skip = hipops.raycast_volume(vd, level, lo, step, o, d, 0.0, bricks)
        dense = hipops.raycast_volume(vd, level, lo, step, o, d, 0.0, None)
        again = hipops.raycast_volume(vd, level, lo, step, o, d, 0.0, bricks)
        for a, b, c in zip(skip, dense, again):
            assert torch.equal(a, b) and torch.equal(a, c)
        n = 96 * 96
        for k in range(3):
            one = hipops.raycast_volume(vd, level, lo, step, o[k * n:(k + 1) * n].contiguous(), d[k * n:(k + 1) * n].contiguous(), 0.0, bricks)
            for a, b in zip(one, skip):
                assert torch.equal(a, b[k * n:(k + 1) * n])
        print(f'level {level}: {int(skip[2].sum())} of {o.shape[0]} rays hit')
        assert 0 < int(skip[2].sum()) < o.shape[0]


def test_volume_normals_device_matches_numpy():
    vol, c = sphere_field(64, 20)
    v, f = geometry.marching_cubes(vol, 0.0, (-c,) * 3, (1, 1, 1))
    ref = geometry.volume_normals(vol, v, (-c,) * 3, (1, 1, 1))
    vd, pd = _cuda(vol, v)
    dev = geometry.volume_normals(vd, pd, (-c,) * 3, (1, 1, 1))
    assert np.abs(dev.cpu().numpy() - ref).max() <= 1e-5
    rs = np.random.RandomState(2)
    pts = rs.uniform(-40, 40, (1000, 3)).astype(np.float32)                 # outside the box too: clamped
    g_ref = geometry.volume_normals(vol, pts, (-c,) * 3, (1, 1, 1))
    g_dev = geometry.volume_normals(vd, _cuda(pts)[0], (-c,) * 3, (1, 1, 1))
    assert np.abs(g_dev.cpu().numpy() - g_ref).max() <= 1e-5


def test_render_geometry_full_width_matches_mesh():
    from scipy.spatial import cKDTree
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('full')).eval().requires_grad_(False)).cuda()
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(0, 1).cuda(), synthetic.conditioning_camera().cuda(), truncation_psi=0.7, truncation_cutoff=14)
    mesh = {'uvcoords_image': synthetic.uv_conditions([0]).cuda()}
    cams = synthetic.camera_labels([0, 100]).cuda()[None]
    out = g.render_geometry(ws, cams, mesh, resolution=512, volume_resolution=256, level=0.0, with_colors=True, noise_mode='const')
    assert out['depth'].shape == (1, 2, 1, 512, 512) and out['normal'].shape == (1, 2, 3, 512, 512)
    assert out['rgb'].shape == (1, 2, 3, 512, 512) and out['shaded'].shape == (1, 2, 1, 512, 512) and out['mask'].dtype == torch.bool
    m = out['mask'][0, :, 0]
    print(f'render_geometry 512^2 x 2 views from 256^3: {int(m.sum())} surface pixels')
    assert int(m.sum()) > 1000
    geo = g.extract_geometry(ws, mesh, resolution=256, level=0.0, noise_mode='const')[0]
    verts = geo['verts'].cpu().numpy()
    # the hit points, recomputed from the same rays
    cam = cams.reshape(2, 25)
    rays_o, rays_d = hipops.ray_sampler(cam, 512)
    depth = out['depth'][0, :, 0].reshape(2, -1)
    pts = (rays_o + depth[..., None] * rays_d)[m.reshape(2, -1)].cpu().numpy()
    # rays that start inside the box at a point already inside hit at their clipped start: leave those out
    bw = g.rendering_kwargs['box_warp']
    lo = -0.5 * bw
    on_face = (np.abs(np.abs(pts) - abs(lo)) < 1e-4).any(1)
    cell = bw / 255
    dist, _ = cKDTree(verts).query(pts[~on_face])
    print(f'hit points vs mesh vertices: max distance {dist.max() / cell:.3f} cell ({(~on_face).sum()} hits)')
    assert (~on_face).sum() > 1000 and dist.max() <= np.sqrt(3) * cell * 1.0001


def test_error_paths_report_not_fault():
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    assert lib.ia_raycast_scratch_bytes(1, 4, 4, ctypes.byref(nbytes)) == -1 and '>= 2' in _lib.last_error()
    assert lib.ia_raycast_scratch_bytes(2048, 1024, 1024, ctypes.byref(nbytes)) == -1 and '2^31' in _lib.last_error()
    assert lib.ia_raycast_scratch_bytes(17, 9, 8, None) == -1
    assert lib.ia_raycast_scratch_bytes(17, 9, 8, ctypes.byref(nbytes)) == 0 and nbytes.value == 2 * 1 * 1 * 8
    vol = torch.zeros(17, 9, 8, device='cuda')
    bricks = torch.empty(4, device='cuda')
    assert lib.ia_volume_bricks(vol.data_ptr(), 17, 9, 8, bricks.data_ptr(), 8, None) == -1 and 'scratch' in _lib.last_error()
    assert lib.ia_volume_bricks(None, 17, 9, 8, bricks.data_ptr(), 16, None) == -1 and 'device pointers' in _lib.last_error()
    f3 = hipops._f3
    rays = torch.zeros(10, 3, device='cuda')
    depth, normal = torch.empty(10, device='cuda'), torch.empty(10, 3, device='cuda')
    mask = torch.empty(10, dtype=torch.uint8, device='cuda')

    def cast(nx=17, n_rays=10, ro=rays, bricks_p=bricks.data_ptr(), bricks_n=16, flags=0, lo=(0, 0, 0)):
        return lib.ia_raycast_volume(vol.data_ptr(), nx, 9, 8, f3(lo), f3((1, 1, 1)), 0.0, bricks_p, bricks_n,
                                     None if ro is None else ro.data_ptr(), rays.data_ptr(), n_rays, 0.0, depth.data_ptr(),
                                     normal.data_ptr(), mask.data_ptr(), flags, None)
    assert cast(nx=1) == -1 and '>= 2' in _lib.last_error()
    assert cast(n_rays=0) == -1 and 'n_rays' in _lib.last_error()
    assert cast(n_rays=-3) == -1 and 'n_rays' in _lib.last_error()
    assert cast(ro=None) == -1 and 'device pointers' in _lib.last_error()
    assert cast(bricks_n=8) == -1 and 'scratch' in _lib.last_error()
    assert cast(bricks_p=None) == -1 and 'bricks' in _lib.last_error()
    assert cast(lo=(0, float('nan'), 0)) == -1 and 'finite' in _lib.last_error()
    assert lib.ia_volume_gradient(vol.data_ptr(), 17, 9, 8, f3((0, 0, 0)), f3((1, 0, 1)), rays.data_ptr(), 10, normal.data_ptr(), None) == -1
    assert lib.ia_volume_gradient(vol.data_ptr(), 17, 9, 8, f3((0, 0, 0)), f3((1, 1, 1)), None, 10, normal.data_ptr(), None) == -1
    assert lib.ia_volume_gradient(vol.data_ptr(), 17, 9, 8, f3((0, 0, 0)), f3((1, 1, 1)), rays.data_ptr(), -1, normal.data_ptr(), None) == -1
    with pytest.raises(RuntimeError):
        hipops.raycast_volume(vol, 0.0, (0, 0, 0), (1, 1, 1), rays, torch.zeros(10, 2, device='cuda'))
    with pytest.raises(RuntimeError):
        hipops.volume_bricks(torch.zeros(4, 4, device='cuda'))
    with pytest.raises(RuntimeError):
        hipops.volume_gradient(vol.double(), (0, 0, 0), (1, 1, 1), rays)
    torch.cuda.synchronize()
