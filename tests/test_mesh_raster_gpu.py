"""geometry.rasterize_mesh on the device (csrc/mesh_raster.hip) against the float32 NumPy restatement: integers equal, floats bit for bit;
the two raster paths, two streams, ``TriPlaneGenerator.render_mesh``, the command line and the argument errors.  The cases, references
and measured figures are those of tests/test_mesh_raster_cpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry
from test_mesh_raster_cpu import (BACK, BAND_PX, BIG, FRONT, INTERIOR_DEPTH_WORST, band_and_interior, degenerate_cases, fan, from_pixels,
                                  polygon_placements, sphere_case, sphere_runs, volume_case)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
FLOATS = ('depth', 'bary', 'normal', 'attributes')


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raster(v, f, cams, res, normals=None, attributes=None, **kw):
    return geometry.rasterize_mesh(dev(v), dev(f), dev(cams), res, normals=dev(normals), attributes=dev(attributes), **kw)


def assert_same(name, got, want):
    """``want``: NumPy arrays or device tensors."""
    for k in ('mask', 'face', 'culled') + FLOATS:
        g, w = got[k], want[k]
        if w is None:
            assert g is None, (name, k)
            continue
        g, w = g.cpu().numpy(), w.cpu().numpy() if isinstance(w, torch.Tensor) else w
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, w.dtype, g.shape, w.shape)
        if k in FLOATS:
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (name, k, int((g != w).sum()))


def extras(v, seed=0):
    rng = np.random.RandomState(seed)
    n = rng.randn(len(v), 3)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32), rng.uniform(-1, 2, (len(v), 3)).astype(F32)


def test_sphere_equals_the_restatement():
    v, f, cams, res = sphere_case()
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    got = raster(v, f, cams, res, nrm, np.ascontiguousarray(v * 2 + 1))
    assert_same('sphere', got, sphere_runs()[0])
    assert_same('sphere, face normals', raster(v, f, cams[:2], res, cull='back'), geometry.rasterize_mesh(v, f, cams[:2], res, cull='back'))


def test_polygon_and_degenerate_cases_equal_the_restatement():
    px = polygon_placements(True)[0]
    cases = {'integer polygon': (from_pixels(px, 1, 24, 24), fan(0), FRONT, 24, {})}
    cases.update({k: c[:5] for k, c in degenerate_cases().items()})
    for name, (v, f, cams, res, kw) in cases.items():
        nrm, att = extras(v)
        for views in (np.concatenate([FRONT, BACK]), np.concatenate([cams[:1], BACK, FRONT])):
            want = geometry.rasterize_mesh(v, f, views, res, normals=nrm, attributes=att, **kw)
            assert_same(name, raster(v, f, views, res, nrm, att, **kw), want)
            assert_same(name + ', wave path', raster(v, f, views, res, nrm, att, oversize_pixels=0, **kw), want)
    for name, (v, f, cams, res, kw, face, culled) in degenerate_cases().items():
        got = raster(v, f, cams, res, **kw)
        assert np.array_equal(got['face'].cpu().numpy(), face) and got['culled'].tolist() == culled, name


def test_two_raster_paths_agree():
    v, f, cams, res = sphere_case()
    nrm, att = extras(v)
    for name, (vv, ff, cc, rr) in {'sphere': (v, f, cams, res), 'larger than the viewport': (from_pixels(BIG, 1, 24, 24), np.array([[0, 1, 2]]), FRONT, 24)}.items():
        n2, a2 = extras(vv)
        wave = raster(vv, ff, cc, rr, n2, a2, oversize_pixels=0)
        thread = raster(vv, ff, cc, rr, n2, a2, oversize_pixels=2 ** 30)
        assert_same(name, wave, thread)
        assert_same(name, raster(vv, ff, cc, rr, n2, a2, oversize_pixels=7), thread)       # some triangles on either path
        assert int(wave['mask'].sum()) > 500


def test_two_streams_give_the_serial_results():
    v, f, cams, res = sphere_case()
    meshes = [(dev(v), dev(f), dev(cams)), (dev(np.ascontiguousarray(v[:, ::-1] * F32(0.8))), dev(f[:200]), dev(cams[::-1].copy()))]
    serial = [geometry.rasterize_mesh(*m, res) for m in meshes]
    torch.cuda.synchronize()
    streams, got = [torch.cuda.Stream(), torch.cuda.Stream()], []
    for s, m in zip(streams, meshes):
        with torch.cuda.stream(s):
            got.append(geometry.rasterize_mesh(*m, res))
    torch.cuda.synchronize()
    for k, (g, w) in enumerate(zip(got, serial)):
        assert_same(f'stream {k}', g, w)
    assert not torch.equal(serial[0]['face'], serial[1]['face'])


@pytest.fixture(scope='module')
def small_generator():
    from invertavatar_amd import synthetic
    from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
    gen = TriPlaneGenerator(**synthetic.generator_kwargs('small')).eval().requires_grad_(False)
    synthetic.fill_parameters(gen)
    gen = gen.to(DEV)
    with torch.no_grad():
        ws = gen.mapping(synthetic.latent(3, 1).to(DEV), synthetic.conditioning_camera().to(DEV), truncation_psi=0.7, truncation_cutoff=14)
    return gen, ws, {'uvcoords_image': synthetic.uv_conditions([0]).to(DEV)}


def test_render_mesh(small_generator):
    gen, ws, cond = small_generator
    vol, lo, step, _, _, cams, res = volume_case()
    tv = dev(vol)
    v, f = geometry.marching_cubes(tv, 0.0, lo, step)[:2]
    c = dev(cams)
    colors = ((v - v.min()) / (v.max() - v.min()) * 255).round().to(torch.uint8)
    out = gen.render_mesh(v, f, c, resolution=res, colors=colors)
    with torch.no_grad():
        like = gen.render_geometry(ws, c[None], cond, resolution=res, volume_resolution=24, level=0.0, with_colors=True, noise_mode='const')
    for k, x in like.items():
        assert out[k].shape == x.shape[1:] and out[k].dtype == x.dtype, (k, out[k].shape, x.shape, out[k].dtype, x.dtype)
    assert out['culled'].tolist() == [0, 0]
    batched = gen.render_mesh(v, f, c[None], resolution=res, colors=colors)
    assert all(torch.equal(batched[k][0], out[k]) for k in out)
    o, d = gen.ray_sampler(c[:, :16].view(-1, 4, 4), c[:, 16:].view(-1, 3, 3), res)
    cast = geometry.raycast(tv, 0.0, lo, step, o, d)
    shape = (len(cams), res, res)
    in_band, worst, n = band_and_interior(out['mask'][:, 0].cpu().numpy(), out['depth'][:, 0].cpu().numpy(), cast['mask'].reshape(shape).cpu().numpy(),
                                          cast['depth'].reshape(shape).cpu().numpy(), 2 * BAND_PX)
    print(f'render_mesh against raycast: {n} interior pixels, worst depth difference {worst:.3e}')
    assert in_band and n > 600 and worst <= 2 * INTERIOR_DEPTH_WORST
    shaded = geometry.shade(out['normal'].permute(0, 2, 3, 1).contiguous(), d.reshape(shape + (3,)), out['mask'][:, 0])
    assert torch.equal(out['shaded'], shaded.permute(0, 3, 1, 2))
    # colours lie in [0, 1] and the three weights (each rounded three times) add up to at most 1 + 8 eps32
    assert out['rgb'].min() >= 0 and out['rgb'].max() <= 1 + 8 * float(np.finfo(F32).eps) and (out['rgb'].sum(1, keepdim=True) > 0)[out['mask']].float().mean() > 0.9
    assert not out['rgb'][(~out['mask']).expand(-1, 3, -1, -1)].any()


def test_command_line(tmp_path):
    from invertavatar_amd import extract_geometry
    args = ['--seeds', '0', '--width', 'small', '--level', '0', '--outdir', str(tmp_path), '--device', DEV, '--save-depth',
            '--mesh-views', '2', '--render-res', '32', '--res', '24', '--smooth', '1']
    (path, out), = extract_geometry.main(args)
    from PIL import Image
    for k in range(2):
        for stem in ('meshview', 'meshrgb'):
            img = np.asarray(Image.open(str(tmp_path / f'seed0000_{stem}{k:02d}.png')))
            assert img.shape[:2] == (32, 32) and img.any(), (stem, k)
    depth = np.load(str(tmp_path / 'seed0000_meshdepth.npy'))
    assert depth.shape == (2, 32, 32) and (depth > 0).sum() == int(out['mesh_views']['mask'].sum()) > 0
    assert 'smooth' in out and not os.path.exists(str(tmp_path / 'seed0000_view00.png'))


def test_argument_errors_are_exceptions():
    from invertavatar_amd import _lib, hipops
    v, f, cams, res = sphere_case()
    tv, tf, tc = dev(v), dev(f), dev(cams)
    with pytest.raises(RuntimeError):                                         # host tensors at the wrappers
        hipops.mesh_project(torch.from_numpy(v), tc, (res, res))
    lib = _lib.load()
    host = np.zeros(len(v) * 4 * len(cams), dtype=np.int32)
    st = lib.ia_mesh_project(tv.data_ptr(), len(v), tc.data_ptr(), len(cams), res, res, 1e-6, host.ctypes.data, _lib.stream_ptr())
    assert st != 0 and 'device pointer' in _lib.last_error()                  # a host pointer at the C entry
    st = lib.ia_mesh_project(v.ctypes.data, len(v), tc.data_ptr(), len(cams), res, res, 1e-6, None, _lib.stream_ptr())
    assert st != 0 and 'device pointer' in _lib.last_error()
    with pytest.raises(ValueError):
        geometry.rasterize_mesh(tv, tf + 1, tc, res)                          # a face index out of range
    bad = cams.copy()
    bad[1, 23] = 0.25
    with pytest.raises(RuntimeError, match='last row of K'):
        geometry.rasterize_mesh(tv, tf, dev(bad), res)
    with pytest.raises(ValueError):
        geometry.rasterize_mesh(tv, tf, tc, res, attributes=torch.zeros(len(v), 9, device=DEV))
    proj = hipops.mesh_project(tv, tc, (res, res))
    vis, _ = hipops.mesh_raster(proj, tf.int(), (res, res))
    with pytest.raises(RuntimeError, match='attribute channels'):
        hipops.mesh_resolve(vis, proj, tv, tf.int(), tc, attributes=torch.zeros(len(v), 9, device=DEV))
    torch.cuda.synchronize()
    assert int(geometry.rasterize_mesh(tv, tf, tc, res)['mask'].sum()) > 0      # the device is still well
