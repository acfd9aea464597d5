"""The texture atlas on the device (csrc/texture.hip: ia_atlas_points, ia_texture_project, ia_texture_sample) against the float32 NumPy
restatement: integers equal, floats bit for bit; two streams, run to run, ``render_mesh(texture=...)``, ``G.bake_texture`` and the command
line.  The cases are those of tests/test_texture_cpu.py."""
import math

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry
from test_mesh_raster_cpu import FRONT, label
from test_texture_cpu import LAYOUTS, RES, affine, degenerate_mesh, mesh_of, projection_case, rasters, shadow_case, sphere, sphere_images

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_same(name, got, want, keys):
    for k in keys:
        g, w = got[k].cpu().numpy(), want[k].cpu().numpy() if isinstance(want[k], torch.Tensor) else want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == F32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (name, k, int((g != w).sum()))


POINT_KEYS = ('face', 'point', 'bary', 'normal')
PROJECT_KEYS = ('views', 'filled', 'texture', 'weight')


@pytest.mark.parametrize('F,size,block', LAYOUTS)
def test_atlas_points_equal_the_restatement(F, size, block):
    v, f = mesh_of(F)
    atlas = geometry.TextureAtlas(F, size, block)
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    for normals in (None, nrm):
        got = geometry.atlas_points(dev(v), dev(f), atlas, normals=dev(normals))
        want = geometry.atlas_points(v, f, atlas, normals=normals)
        assert_same(f'{F} faces', got, want, POINT_KEYS)
        assert got['info'] == want['info'] and np.array_equal(got['face'].cpu().numpy(), atlas.texel_face())


def test_degenerate_faces_equal_the_restatement():
    v, f = degenerate_mesh()
    atlas = geometry.TextureAtlas(7, 16, 4)
    with np.errstate(all='ignore'):
        want = geometry.atlas_points(v, f, atlas)
    got = geometry.atlas_points(dev(v), dev(f), atlas)
    assert got['info'] == want['info'] and want['info']['degenerate'] >= 2
    for k in POINT_KEYS:                                                          # (NaN payloads are not compared: NaN where NaN)
        g, w = got[k].cpu().numpy(), want[k]
        assert np.array_equal(g, w, equal_nan=g.dtype == F32), k
        if g.dtype == F32:
            ok = np.isfinite(w)
            assert np.array_equal(g[ok].view(np.uint32), w[ok].view(np.uint32)), k
    # the projection of such a mesh: every view skipped on the non-finite points, the rest bit for bit
    cams = sphere()[2]
    with np.errstate(all='ignore'):
        r = geometry.rasterize_mesh(v, f, cams, RES)
        want = geometry.project_texture(v, f, atlas, sphere_images(), cams, r['depth'], r['mask'])
    got = geometry.project_texture(dev(v), dev(f), atlas, dev(sphere_images()), dev(cams), dev(r['depth']), dev(r['mask']))
    assert_same('degenerate', got, want, PROJECT_KEYS)
    assert want['filled'].any()


def outside_and_behind():
    """The sphere's cameras; one moved so that the sphere is partly outside the image; one behind the mesh, looking away."""
    v, f, cams = sphere()
    near = cams[1].copy()
    M = near[:16].reshape(4, 4).copy()
    M[:3, 3] = M[:3, 3] * F32(0.45) + M[:3, 0] * F32(0.3)                         # closer and to the side
    near[:16] = M.reshape(-1)
    away = cams[0].copy()
    M = away[:16].reshape(4, 4).copy()
    M[:3, 3] = M[:3, 3] + M[:3, 2] * F32(5.4)                                     # through the sphere to the far side, same direction
    away[:16] = M.reshape(-1)
    return np.stack([cams[0], near, away])


@pytest.mark.parametrize('size', [64, 128])
@pytest.mark.parametrize('mode,power', [('blend', 2.0), ('best', 2.0), ('blend', 3.0), ('blend', 1.0)])
def test_projection_equals_the_restatement(size, mode, power):
    v, f, cams, atlas, _ = projection_case(size)
    r = rasters()
    fb = np.random.RandomState(0).uniform(0, 1, (size, size, 3)).astype(F32)
    want = geometry.project_texture(v, f, atlas, sphere_images(), cams, r['depth'], r['mask'], mode=mode, power=power, fallback=fb)
    got = geometry.project_texture(dev(v), dev(f), atlas, dev(sphere_images()), dev(cams), dev(r['depth']), dev(r['mask']), mode=mode,
                                   power=power, fallback=dev(fb))
    assert_same(f'{mode} {power}', got, want, PROJECT_KEYS)
    assert 0 < int(want['filled'].sum()) < (atlas.texel_face() >= 0).sum() and want['views'].max() >= 2


def test_projection_edge_cameras_and_occluder():
    v, f, _, atlas, _ = projection_case()
    cams = outside_and_behind()
    img = np.random.RandomState(1).uniform(0, 1, (3, RES, RES, 8)).astype(F32)       # 8 channels
    with np.errstate(all='ignore'):
        want = geometry.project_texture(v, f, atlas, img, cams)
    got = geometry.project_texture(dev(v), dev(f), atlas, dev(img), dev(cams))       # depth and mask from the device rasteriser
    assert_same('edge cameras', got, want, PROJECT_KEYS)
    alone = geometry.project_texture(dev(v), dev(f), atlas, dev(img[2:]), dev(cams[2:]))
    assert not alone['filled'].any() and not alone['texture'].any()                  # the camera behind the mesh: all views skipped
    part = geometry.project_texture(v, f, atlas, img[1:2], cams[1:2])
    assert 0 < part['filled'].sum() < want['filled'].sum()                            # the sphere partly outside the image
    v2, f2, cams2 = shadow_case()
    r2 = geometry.rasterize_mesh(v2, f2, cams2, RES)
    want = geometry.project_texture(v, f, atlas, sphere_images(), cams2, r2['depth'], r2['mask'], depth_tol=0.5, min_cos=0.5)
    got = geometry.project_texture(dev(v), dev(f), atlas, dev(sphere_images()), dev(cams2), dev(r2['depth']), dev(r2['mask']), depth_tol=0.5,
                                   min_cos=0.5)
    assert_same('occluder', got, want, PROJECT_KEYS)


@pytest.mark.parametrize('F,size,block', [(7, 16, 4), (99, 50, 6), (320, 64, None), (320, 128, None)])
def test_sample_equals_the_restatement(F, size, block):
    v, f = mesh_of(F)
    atlas = geometry.TextureAtlas(F, size, block)
    tex = geometry.bake_texture(v, f, size, affine, atlas=atlas)['texture']
    rng = np.random.RandomState(size)
    face = rng.randint(-1, F + 1, 5000).astype(np.int32)
    bary = rng.dirichlet((1, 1, 1), 5000).astype(F32)
    face[:6], bary[:6] = [0, 0, 0, F - 1, F - 1, F - 1], np.concatenate([np.eye(3, dtype=F32)] * 2)
    bary[6:200] += rng.uniform(-0.5, 0.5, (194, 3)).astype(F32)                   # outside the triangle: clamped into the block
    want = geometry.sample_texture(tex, atlas, face, bary)
    got = geometry.sample_texture(dev(tex), atlas, dev(face), dev(bary))
    assert_same('sample', {'x': got}, {'x': want}, ('x',))
    baked = geometry.bake_texture(dev(v), dev(f), size, lambda p: dev(affine(p.cpu().numpy())), atlas=atlas)
    assert_same('bake', baked, {'texture': tex, 'mask': atlas.texel_face() >= 0}, ('texture', 'mask'))
    # the raster's face and bary, [N,H,W]
    r = rasters(F)
    want = geometry.sample_texture(tex, atlas, r['face'], r['bary'])
    got = geometry.sample_texture(dev(tex), atlas, dev(r['face']), dev(r['bary']))
    assert_same('sample of a raster', {'x': got}, {'x': want}, ('x',))
    assert got.shape == (3, RES, RES, 3) and bool(got.any()) and not got[dev(~r['mask'])].any()


def test_two_streams_and_run_to_run():
    v, f, cams, atlas, _ = projection_case()
    r = rasters()
    args = [(dev(v), dev(f), atlas, dev(sphere_images()), dev(cams), dev(r['depth']), dev(r['mask'])),
            (dev(np.ascontiguousarray(v[:, ::-1])), dev(f), atlas, dev(sphere_images()[::-1].copy()), dev(cams), dev(r['depth']), dev(r['mask']))]
    serial = [geometry.project_texture(*a) for a in args]
    points = [geometry.atlas_points(*a[:3]) for a in args]
    torch.cuda.synchronize()
    streams, got, pts = [torch.cuda.Stream(), torch.cuda.Stream()], [], []
    for s, a in zip(streams, args):
        with torch.cuda.stream(s):
            got.append(geometry.project_texture(*a))
            pts.append(geometry.atlas_points(*a[:3]))
    torch.cuda.synchronize()
    for k in range(2):
        assert_same(f'stream {k}', got[k], serial[k], PROJECT_KEYS)
        assert_same(f'stream {k}', pts[k], points[k], POINT_KEYS)
        assert_same(f'run {k}', geometry.project_texture(*args[k]), serial[k], PROJECT_KEYS)
    assert not torch.equal(serial[0]['texture'], serial[1]['texture'])


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


def test_render_mesh_through_the_texture(small_generator):
    gen = small_generator[0]
    v, f, cams, atlas, _ = projection_case()
    tex = dev(geometry.bake_texture(v, f, atlas.size, affine, atlas=atlas)['texture'])
    out = gen.render_mesh(dev(v), dev(f), dev(cams), resolution=RES, texture=tex, atlas=atlas)
    r = geometry.rasterize_mesh(dev(v), dev(f), dev(cams), RES)
    want = geometry.sample_texture(tex, atlas, r['face'], r['bary'])
    assert torch.equal(out['rgb'], want.permute(0, 3, 1, 2)) and out['rgb'].shape == (3, 3, RES, RES)
    assert not out['rgb'][(~out['mask']).expand(-1, 3, -1, -1)].any() and bool(out['rgb'].any())
    plain = gen.render_mesh(dev(v), dev(f), dev(cams), resolution=RES)
    assert 'rgb' not in plain and all(torch.equal(plain[k], out[k]) for k in plain)
    with pytest.raises(ValueError):
        gen.render_mesh(dev(v), dev(f), dev(cams), resolution=RES, texture=tex)


def test_generator_bakes_from_both_sources(small_generator):
    gen, ws, cond = small_generator
    item = gen.extract_geometry(ws, cond, resolution=24, level=0.0, noise_mode='const')[0]
    v, f = item['verts'], item['faces']
    size = 4 * (math.isqrt((int(f.shape[0]) + 1) // 2) + 1) + 3                      # blocks of side 4, not a multiple
    dec = gen.bake_texture(ws, cond, v, f, size=size, noise_mode='const')
    assert dec['texture'].shape == (size, size, 3) and dec['texture'].min() >= 0 and dec['texture'].max() <= 1 and bool(dec['mask'].any())
    assert torch.equal(dec['filled'], dec['mask']) and dec['uv'].shape == (f.shape[0], 3, 2)
    views = gen.bake_texture(ws, cond, v, f, size=size, source='views', n_views=2, noise_mode='const')
    assert views['texture'].shape == (size, size, 3) and views['views'].max() >= 1 and bool(views['filled'].any())
    assert torch.equal(views['texture'][~views['filled']], dec['texture'][~views['filled']])          # the fallback
    assert torch.isfinite(views['texture']).all() and not torch.equal(views['texture'], dec['texture'])
    both = gen.extract_geometry(ws, cond, resolution=24, level=0.0, noise_mode='const', texture=size)[0]
    assert torch.equal(both['texture'], dec['texture']) and torch.equal(both['verts'], v) and both['atlas'].size == size


def test_command_line(tmp_path):
    from invertavatar_amd import extract_geometry
    from PIL import Image
    args = ['--seeds', '0', '--width', 'small', '--level', '0', '--outdir', str(tmp_path), '--device', DEV, '--mesh-views', '2', '--render-res', '32',
            '--res', '12', '--texture', '128', '--texture-source', 'views', '--texture-views', '2']
    (path, out), = extract_geometry.main(args)
    back = geometry.read_obj(str(tmp_path / 'seed0000.obj'))
    assert np.array_equal(back['faces'], out['faces'].cpu().numpy()) and back['texture'].shape == (128, 128, 3) and back['texture'].any()
    assert np.array_equal(back['uv'], out['uv']) and 'views' in out['texture_info']
    for k in range(2):
        img = np.asarray(Image.open(str(tmp_path / f'seed0000_meshtex{k:02d}.png')))
        assert img.shape == (32, 32, 3) and img.any()


def test_argument_errors_are_exceptions():
    from invertavatar_amd import _lib, hipops
    v, f, cams, atlas, _ = projection_case(64)
    tv, tf = dev(v), dev(f.astype(np.int32))
    with pytest.raises(RuntimeError):
        hipops.atlas_points(torch.from_numpy(v), tf, 64, 4)                          # a host tensor at the wrapper
    with pytest.raises(RuntimeError, match='hold fewer'):
        hipops.atlas_points(tv, tf, 32, 4)                                           # 64 blocks for 320 faces
    lib = _lib.load()
    host = np.zeros(64 * 64 * 3, dtype=F32)
    out = hipops.atlas_points(tv, tf, 64, 4)
    st = lib.ia_atlas_points(tv.data_ptr(), len(v), tf.data_ptr(), len(f), 64, 4, None, host.ctypes.data, out['face'].data_ptr(),
                             out['bary'].data_ptr(), out['normal'].data_ptr(), out['degenerate'].data_ptr(), _lib.stream_ptr())
    assert st != 0 and 'device pointer' in _lib.last_error()
    with pytest.raises(ValueError):
        geometry.atlas_points(tv, dev(f) + 1000, atlas)                              # a face index out of range
    with pytest.raises(RuntimeError, match='channels'):
        hipops.texture_project(out['point'], out['normal'], out['face'], torch.zeros(1, 8, 8, 9, device=DEV), dev(FRONT),
                               torch.zeros(1, 8, 8, device=DEV), torch.zeros(1, 8, 8, dtype=torch.bool, device=DEV), 1e-6, 0.2, 2.0, 0.1)
    torch.cuda.synchronize()
    assert int((geometry.atlas_points(tv, tf, atlas)['face'] >= 0).sum()) == 320 * 8         # the device is still well
