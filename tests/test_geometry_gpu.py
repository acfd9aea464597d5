"""Avatar geometry on the device: ia_query_planes against the reference-recorded ``sample_mixed`` values, ia_density_grid against the
point query and against ``sample_mixed``, ia_mc_count / ia_mc_emit against the NumPy restatement, and the error paths of the ABI."""
import ctypes

import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, geometry, synthetic
from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
from conftest import max_abs, rnd
from test_geometry_cpu import mesh_stats, sphere_field, torus_field

pytestmark = pytest.mark.gpu


def _inputs(g):
    """The inputs of test_generator_entry_points._inputs that sample_mixed reads (the same seeds)."""
    frames = g['frames'].tolist()
    pts = torch.from_numpy(np.random.RandomState(33).uniform(-0.55, 0.55, (2, 700, 3)).astype(np.float32))
    return dict(pts=pts, dirs=torch.nn.functional.normalize(rnd(34, 2, 700, 3), dim=-1), uv=synthetic.uv_conditions(frames))


@pytest.fixture(scope='module')
def small_gen():
    return synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('small')).eval().requires_grad_(False)).cuda()


@pytest.fixture(scope='module')
def full_setup():
    """Full-width generator, B = 2 planes [2,3,32,256,256] on the device."""
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('full')).eval().requires_grad_(False)).cuda()
    frames = [3, 17]
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(7, 2).cuda(), synthetic.conditioning_camera().expand(2, -1).cuda(), truncation_psi=0.7,
                       truncation_cutoff=14)
        mesh = {'uvcoords_image': synthetic.uv_conditions(frames).cuda()}
        planes = geometry.generator_planes(g, ws, mesh, noise_mode='const')
    return g, ws, mesh, planes


def test_query_points_vs_reference(golden, small_gen):
    g = golden('generator_small_extra.npz')
    i = _inputs(g)
    ws, mesh = g['ws'].cuda().flip(0).contiguous(), {'uvcoords_image': i['uv'].cuda()}
    with torch.no_grad():
        q = small_gen.query_points(ws, i['pts'].cuda(), mesh, noise_mode='const')
    d_rgb, d_sigma = max_abs(q['rgb'].cpu(), g['sample_mixed/rgb']), max_abs(q['sigma'].cpu(), g['sample_mixed/sigma'])
    print(f'query_points vs reference sample_mixed: max|d rgb| = {d_rgb:.2e}, max|d sigma| = {d_sigma:.2e}')
    assert q['rgb'].shape == (2, 700, 32) and q['sigma'].shape == (2, 700, 1)
    assert d_rgb <= 1e-4 and d_sigma <= 5e-4                     # the device entry-point bars
    assert d_rgb <= 5e-5 and d_sigma <= 2e-4                     # the fp32 kernel lands within the CPU bars


def test_density_grid_bit_equal_to_query_and_close_to_sample_mixed(full_setup):
    g, ws, mesh, planes = full_setup
    bw = g.rendering_kwargs['box_warp']
    res = 64
    with torch.no_grad():
        vol = geometry.density_volume(planes, g.decoder, res, bw, box_warp=bw)
        pts = geometry.lattice_points(res, bw).cuda()[None].expand(2, -1, -1).contiguous()
        q = geometry.query_planes(planes, g.decoder, pts, bw, rgb=False)['sigma']
        q_rgb = geometry.query_planes(planes, g.decoder, pts, bw, rgb=True)['sigma']
        ref = torch.cat([g.sample_mixed(pts[:, s:s + 65536].clone(), torch.zeros_like(pts[:, s:s + 65536]), ws, mesh, noise_mode='const')['sigma']
                         for s in range(0, pts.shape[1], 65536)], 1)
    assert vol.shape == (2, res, res, res)
    assert torch.equal(vol.reshape(2, -1), q.reshape(2, -1)) and torch.equal(q, q_rgb)
    d = max_abs(vol.reshape(2, -1).cpu(), ref.reshape(2, -1).cpu())
    print(f'density_grid 64^3 vs sample_mixed: max|d sigma| = {d:.2e} (sigma range {vol.min().item():.3f} .. {vol.max().item():.3f})')
    assert d <= 2e-4


def test_density_grid_flip_z_mirrors(full_setup):
    g, _, _, planes = full_setup
    bw = g.rendering_kwargs['box_warp']
    with torch.no_grad():
        a = geometry.density_volume(planes, g.decoder, (40, 48, 64), bw, origin=(0.05, -0.1, 0.0), box_warp=bw)
        b = geometry.density_volume(planes, g.decoder, (40, 48, 64), bw, origin=(0.05, -0.1, 0.0), box_warp=bw, flip_z=True)
    assert max_abs(b.cpu(), a.flip(-1).cpu()) <= 2e-4 and max_abs(b.cpu(), a.cpu()) > 1e-3


def _device_vs_numpy(vol, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    vd = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).cuda()
    v1, f1 = geometry.marching_cubes(vd, level, origin, spacing)
    v2, f2 = geometry.marching_cubes(vd, level, origin, spacing)
    vn, fn = geometry.marching_cubes(np.asarray(vol, dtype=np.float32), level, origin, spacing)
    assert v1.is_cuda and v1.dtype == torch.float32 and f1.dtype == torch.int64
    assert torch.equal(v1, v2) and torch.equal(f1, f2)                          # bit-identical from run to run
    assert np.array_equal(f1.cpu().numpy(), fn)                                  # faces bit-equal to the NumPy restatement
    voxel = float(min(spacing))
    assert v1.shape == vn.shape and (v1.shape[0] == 0 or np.abs(v1.cpu().numpy() - vn).max() <= 1e-6 * voxel * max(1.0, np.abs(vn).max() / voxel))
    return vn, fn


def test_marching_cubes_device_matches_numpy():
    vol, c = sphere_field(64, 20.0)
    v, f = _device_vs_numpy(vol, 0.0, (-c, -c, -c))
    assert mesh_stats(v, f)['chi'] == 2
    v, f = _device_vs_numpy(torus_field(), 0.0)
    assert mesh_stats(v, f)['chi'] == 0
    rs = np.random.RandomState(11)
    for shape in ((33, 17, 40), (2, 2, 2), (5, 64, 3)):
        f_rand = rs.randn(*shape).astype(np.float32)
        f_rand[rs.rand(*shape) < 0.02] = np.nan
        _device_vs_numpy(f_rand, 0.1, (0.5, -2.0, 1.0), (0.25, 0.5, 0.125))
    _device_vs_numpy(np.zeros((9, 9, 9), np.float32), 0.0)                     # empty mesh


def test_marching_cubes_generator_volume(full_setup):
    g, _, _, planes = full_setup
    bw = g.rendering_kwargs['box_warp']
    with torch.no_grad():
        vol = geometry.density_volume(planes[:1], g.decoder, 96, bw, box_warp=bw)[0]
    level = float(vol.median())
    v, f = _device_vs_numpy(vol.cpu().numpy(), level, (-0.5, -0.5, -0.5), (1 / 95,) * 3)
    assert f.shape[0] > 1000


def test_marching_cubes_512_torus():
    n = 512
    x = torch.arange(n, device='cuda', dtype=torch.float32) - (n - 1) / 2
    X, Y, Z = torch.meshgrid(x, x, x, indexing='ij')
    vol = (60.0 - torch.sqrt((torch.sqrt(X * X + Y * Y) - 150.0) ** 2 + Z * Z)).contiguous()
    del X, Y, Z
    v, f = geometry.marching_cubes(vol, 0.0)
    assert v.shape[0] > 100000
    fc = f.cpu().numpy()
    s = mesh_stats(v.cpu().numpy(), fc)
    assert s['closed'] and s['oriented'] and s['chi'] == 0, s


def test_extract_geometry_end_to_end(full_setup, tmp_path):
    g, ws, mesh, planes = full_setup
    with torch.no_grad():
        vol = geometry.density_volume(planes[:1], g.decoder, 32, 1.0, box_warp=1.0)
    level = float(vol.median())
    out = g.extract_geometry(ws, mesh, resolution=128, level=level, with_colors=True, noise_mode='const')
    assert len(out) == 2
    for o in out:
        assert o['volume'].shape == (128, 128, 128) and o['volume'].is_cuda
        assert o['verts'].dtype == torch.float32 and o['faces'].dtype == torch.int64 and o['colors'].dtype == torch.uint8
        assert o['verts'].shape[1] == 3 and o['faces'].shape[1] == 3 and o['colors'].shape == o['verts'].shape
        assert o['faces'].shape[0] > 0 and int(o['faces'].max()) < o['verts'].shape[0]
    path = str(tmp_path / 'a.ply')
    geometry.write_ply(path, out[0]['verts'], out[0]['faces'], out[0]['colors'])
    v, f, c = geometry.read_ply(path)
    assert np.array_equal(v, out[0]['verts'].cpu().numpy()) and np.array_equal(f, out[0]['faces'].cpu().numpy())
    assert np.array_equal(c, out[0]['colors'].cpu().numpy())


def test_error_paths_report_not_fault():
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    assert lib.ia_mc_scratch_bytes(2048, 1024, 1024, ctypes.byref(nbytes)) == -1 and '2^31' in _lib.last_error()
    assert lib.ia_mc_scratch_bytes(1, 4, 4, ctypes.byref(nbytes)) == -1 and '>= 2' in _lib.last_error()
    vol = torch.zeros(8, 8, 8, device='cuda')
    scratch = torch.empty(1 << 16, dtype=torch.uint8, device='cuda')
    totals = torch.empty(2, dtype=torch.int32, device='cuda')
    st = lib.ia_mc_count(vol.data_ptr(), 2048, 1024, 1024, 0.0, scratch.data_ptr(), scratch.numel(), totals.data_ptr(), None)
    assert st == -1 and '2^31' in _lib.last_error()
    host = torch.zeros(8, 8, 8)
    st = lib.ia_mc_count(host.data_ptr(), 8, 8, 8, 0.0, scratch.data_ptr(), scratch.numel(), totals.data_ptr(), None)
    assert st == -1 and 'device pointers' in _lib.last_error()
    st = lib.ia_mc_count(vol.data_ptr(), 8, 8, 8, 0.0, scratch.data_ptr(), 16, totals.data_ptr(), None)
    assert st == -1 and 'scratch' in _lib.last_error()
    planes = torch.zeros(1, 3, 4, 4, 32)
    w = torch.zeros(64 * 64)
    out = torch.zeros(10)
    st = lib.ia_query_planes(planes.data_ptr(), out.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), 1.0, 1.0, 0,
                             1, 3, 4, 4, out.data_ptr(), None, None)
    assert st == -1 and 'device pointers' in _lib.last_error()
    with pytest.raises(RuntimeError):
        geometry.marching_cubes(torch.zeros(1, 4, 4, device='cuda'), 0.0)
    torch.cuda.synchronize()
