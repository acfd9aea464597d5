"""ia_winding_number and the functions made of it on the device, against the float64 NumPy restatement (tests/test_winding_cpu.py pins
that).  Tolerances come from the restatement's own float32 run and the number formats, never from the kernel."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, geometry, hipops
from test_winding_cpu import (CLOSED, EPS32, F32, LATTICES, iou_case, mc_sphere, mc_torus, open_sphere, pushed_samples, shell, sphere, torus)

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _dev(verts, faces):
    return torch.from_numpy(np.ascontiguousarray(verts)).to(DEV), torch.from_numpy(np.ascontiguousarray(faces)).to(DEV)


def _tris(verts, faces):
    v, f = _dev(verts, faces)
    return hipops.tri_pack(v.float().contiguous(), f.int().contiguous())


def _run(points, verts, faces, **kw):
    return hipops.winding_number(torch.from_numpy(np.ascontiguousarray(points, dtype=F32)).to(DEV), _tris(verts, faces), **kw)


@functools.lru_cache(maxsize=None)
def _mc48():
    _, _, _, _, v, f = mc_sphere(48, 0.8, (0.01, -0.02, 0.03))
    assert f.shape[0] > 2 * hipops.WINDING_CHUNK + 3
    return v, f


MESHES = {'sphere': lambda: sphere(24, 48), 'torus': torus, 'open_sphere': open_sphere, 'shell': shell, 'mc48': _mc48}


def _queries(verts, faces):
    """The pushed samples, a few far points at 100 and 1000 times the extent, one NaN row."""
    pts, _ = pushed_samples(verts, faces)
    extent = float(np.abs(verts).max())
    far = np.array([(100, 0, 0), (0, -100, 30), (57, 57, -57), (1000, 0, 0), (-600, 800, 10), (0, 0, 1000)], dtype=np.float64) * extent
    return np.concatenate([pts, far.astype(F32), np.array([[np.nan, 0.0, 1.0]], dtype=F32)])


def _check(got, points, verts, faces, what):
    """|w_dev - w_64| <= 4 e32 + eps32 max(1, A) per point, e32 = the restatement's own float32 deviation over the case."""
    w64, size = geometry._winding_numpy(points, verts, faces, np.float64)
    w32, _ = geometry._winding_numpy(points, verts, faces, F32)
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == w64.shape
    nan = np.isnan(w64)
    assert np.array_equal(np.isnan(got), nan)
    if nan.all():
        return
    e32 = float(np.abs(w32 - w64)[~nan].max())
    tol = 4 * e32 + EPS32 * np.maximum(1.0, size[~nan])
    err = np.abs(got - w64)[~nan]
    print(f'{what}: N = {points.shape[0]}, F = {faces.shape[0]}, e32 = {e32:.3g}, largest error / tolerance = {float((err / tol).max()):.3g}')
    assert (err <= tol).all()


@pytest.mark.parametrize('name', sorted(MESHES))
def test_winding_number_against_float64(name):
    verts, faces = MESHES[name]()
    pts = _queries(verts, faces)
    _check(_run(pts, verts, faces), pts, verts, faces, name)


def test_face_counts_at_which_the_kernel_changes_path():
    verts, faces = _mc48()
    tile, chunk, _ = hipops.winding_layout()
    assert (tile, chunk) == (hipops.WINDING_TILE, hipops.WINDING_CHUNK)
    pts = _queries(verts, faces)[::4]
    for f in (0, 1, tile - 1, tile, tile + 1, chunk, chunk + 1, 2 * chunk + 3):
        _check(_run(pts, verts, faces[:f]), pts, verts, faces[:f], f'F = {f}')
    assert torch.equal(_run(pts[:-1], verts, faces[:0]), torch.zeros(pts.shape[0] - 1, dtype=torch.float64, device=DEV))


@functools.lru_cache(maxsize=None)
def _cloud():
    verts, faces = sphere(24, 48)                                                          # two chunks
    n = hipops.WINDING_POINTS + 1
    pts = np.random.default_rng(5).uniform(-1.4, 1.4, (n, 3)).astype(F32)
    pts[7] = np.nan
    return verts, faces, pts


def test_point_counts_at_which_the_kernel_changes_path():
    verts, faces, pts = _cloud()
    per = hipops.WINDING_POINTS
    full = _run(pts, verts, faces)
    _check(full, pts, verts, faces, f'N = {per + 1}')
    for n in (0, 1, 63, 64, 65, per - 1, per):
        got = _run(pts[:n], verts, faces)
        assert got.shape == (n,) and torch.equal(got.view(torch.int64), full[:n].view(torch.int64)), n


def test_result_is_a_pure_function_of_point_and_mesh():
    verts, faces, pts = _cloud()
    bits = lambda t: t.view(torch.int64)
    first = _run(pts, verts, faces)
    assert torch.equal(bits(_run(pts, verts, faces)), bits(first))                         # run to run
    perm = np.random.default_rng(6).permutation(pts.shape[0])
    assert torch.equal(bits(_run(pts[perm], verts, faces)), bits(first[torch.from_numpy(perm).to(DEV)]))
    sub = np.sort(np.random.default_rng(7).choice(pts.shape[0], 97, replace=False))
    assert torch.equal(bits(_run(pts[sub], verts, faces)), bits(first[torch.from_numpy(sub).to(DEV)]))
    chunks = -(-faces.shape[0] // hipops.WINDING_CHUNK)
    cap = 8 * chunks * (pts.shape[0] // 3)                                                 # at least three slabs
    assert -(-pts.shape[0] // (cap // (8 * chunks))) >= 3
    assert torch.equal(bits(_run(pts, verts, faces, workspace_bytes=cap)), bits(first))
    assert torch.equal(bits(_run(pts, verts, faces, workspace_bytes=1)), bits(first))       # one point per slab


@pytest.mark.parametrize('make', [sphere, torus])
def test_signed_distance_on_device(make):
    verts, faces = make()
    pts, outside = pushed_samples(verts, faces)
    w64 = geometry._winding_numpy(pts, verts, faces)[0]
    assert (np.abs(w64 - 0.5) > 0.25).all()
    v, f = _dev(verts, faces)
    grid = geometry.TriangleGrid(v, f)
    p = torch.from_numpy(pts).to(DEV)
    r = geometry.signed_distance(p, v, f, grid=grid)
    c = grid.closest(p)
    for k in ('dist', 'face', 'point'):
        assert r[k].dtype == c[k].dtype and torch.equal(r[k], c[k])
    r2 = geometry.signed_distance(p, v, f)                                                 # builds its own grid
    assert torch.equal(r2['sdf'], r['sdf']) and torch.equal(r2['winding'], r['winding'])
    sdf = r['sdf'].cpu().numpy()
    assert np.array_equal(sdf < 0, w64 >= 0.5) and np.array_equal(sdf > 0, outside)
    assert np.array_equal(np.abs(sdf), r['dist'].cpu().numpy())
    assert torch.equal(geometry.inside(p, v, f), r['winding'] >= 0.5)
    assert torch.equal(geometry.winding_number(p.reshape(4, -1, 3), v, f).reshape(-1), r['winding'])


@pytest.mark.parametrize('lattice', sorted(LATTICES))
@pytest.mark.parametrize('name', sorted(CLOSED))
def test_mesh_to_volume_on_device(name, lattice):
    verts, faces = CLOSED[name]()
    kw = dict(LATTICES[lattice])
    if lattice == 'cubic':
        kw['resolution'] = 24
    v, f = _dev(verts, faces)
    a = geometry.mesh_to_volume(v, f, sign='regions', **kw)
    b = geometry.mesh_to_volume(v, f, sign='winding', **kw)
    assert a['info']['mode'] == 'regions' and b['info']['mode'] == 'winding' and a['sdf'].is_cuda and a['sdf'].dtype == torch.float32
    assert torch.equal(a['inside'], b['inside']) and torch.equal(a['sdf'].view(torch.int32), b['sdf'].view(torch.int32))
    assert geometry.mesh_to_volume(v, f, **kw)['info']['mode'] == 'regions'
    # against the restatement, on the same lattice
    dims, org, spc = tuple(a['inside'].shape), a['origin'], a['spacing']
    pts = np.ascontiguousarray(np.stack(np.meshgrid(*geometry._lattice_axes(dims, org, spc), indexing='ij'), -1).reshape(-1, 3))
    w64 = geometry._winding_numpy(pts, verts, faces)[0]
    assert (np.abs(w64 - 0.5) > 0.25).all()
    assert np.array_equal(a['inside'].cpu().numpy().reshape(-1), w64 >= 0.5)
    d64 = geometry._closest_numpy(pts, verts, faces, np.float64)[0]
    d32 = geometry._closest_numpy(pts, verts, faces, F32)[0]
    e32 = float(np.abs(d32.astype(np.float64) - d64).max())
    extent = max(float(np.abs(pts).max()), float(np.abs(verts).max()))
    want = np.where(w64 >= 0.5, -d64, d64)
    err = float(np.abs(a['sdf'].cpu().numpy().reshape(-1).astype(np.float64) - want).max())
    tol = 4 * e32 + EPS32 * extent
    print(f'{name} {lattice} {dims}: {a["info"]}; sdf error / tolerance = {err / tol:.3g}')
    assert err <= tol


@pytest.mark.parametrize('make', [mc_sphere, mc_torus])
def test_round_trip_through_marching_cubes_on_device(make):
    field, level, org, spc, verts, faces = make()
    v, f = _dev(verts, faces)
    r = geometry.mesh_to_volume(v, f, field.shape, origin=org, spacing=spc)
    assert r['info']['mode'] == 'regions'
    assert torch.equal(r['inside'].cpu(), torch.from_numpy(field > F32(level)))
    dv, df = geometry.marching_cubes(torch.from_numpy(field).to(DEV), level, org, spc)     # and from the device's own mesh
    r = geometry.mesh_to_volume(dv, df, field.shape, origin=org, spacing=spc, sign='winding')
    assert torch.equal(r['inside'].cpu(), torch.from_numpy(field > F32(level)))


def test_volume_iou_on_device_equals_the_host_counts():
    meshes, want, bound, _ = iou_case(16)
    cpu = geometry.volume_iou(*meshes, resolution=16)
    gpu = geometry.volume_iou(*[torch.from_numpy(np.ascontiguousarray(m)).to(DEV) for m in meshes], resolution=16)
    print('iou', gpu['iou'], 'host', cpu['iou'], 'expected', want, 'bound', bound)
    assert gpu == cpu and abs(gpu['iou'] - want) <= bound


def test_surface_distance_signed_on_device():
    big, faces = sphere(12, 16, 1.05)
    unit, _ = sphere(12, 16)
    args = [*_dev(big, faces), *_dev(unit, faces)]
    plain, res = geometry.surface_distance(*args), geometry.surface_distance(*args, signed=True)
    assert all(res[k] == plain[k] for k in plain) and len(res) == len(plain) + 4
    assert res['mean_signed_ab'] > 0 and res['inside_share_ab'] == 0.0 and res['inside_share_ba'] == 1.0


def test_winding_number_error_paths():
    """Argument errors are IA_ERR_INVALID_ARG with a message, found before any launch."""
    lib = _lib.load()
    verts, faces = sphere()
    tris = _tris(verts, faces)
    n, f = 5, tris.shape[0]
    pts = torch.zeros(n, 3, device=DEV)
    out = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)
    nbytes = ctypes.c_size_t(0)
    assert lib.ia_winding_number_scratch_bytes(n, f, ctypes.byref(nbytes)) == 0 and nbytes.value == 8 * n * -(-f // hipops.WINDING_CHUNK)
    assert lib.ia_winding_number_scratch_bytes(-1, f, ctypes.byref(nbytes)) == -1 and lib.ia_winding_number_scratch_bytes(n, f, None) == -1
    assert lib.ia_winding_number_scratch_bytes(n, -1, ctypes.byref(nbytes)) == -1 and 'F' in _lib.last_error()
    assert lib.ia_winding_layout(None, None, None) == -1
    scratch = torch.empty(nbytes.value // 8, dtype=torch.float64, device=DEV)

    def call(p=pts.data_ptr(), count=n, t=tris.data_ptr(), nf=f, s=scratch.data_ptr(), sbytes=nbytes.value, o=out.data_ptr()):
        return lib.ia_winding_number(p, count, t, nf, s, sbytes, o, None)
    assert call(p=None) == -1 and 'device pointers' in _lib.last_error()
    assert call(p=torch.zeros(n, 3).data_ptr()) == -1 and 'device pointers' in _lib.last_error()
    assert call(t=None) == -1 and 'device pointers' in _lib.last_error()
    assert call(s=None) == -1 and 'device pointers' in _lib.last_error()
    assert call(o=None) == -1 and 'device pointers' in _lib.last_error()
    assert call(o=torch.zeros(n, dtype=torch.float64).data_ptr()) == -1 and 'device pointers' in _lib.last_error()
    assert call(count=-1) == -1 and 'N' in _lib.last_error()
    assert call(nf=-1) == -1 and 'F' in _lib.last_error()
    assert call(sbytes=nbytes.value - 1) == -1 and 'scratch' in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full((n,), 7.0, dtype=torch.float64, device=DEV))        # nothing was launched
    assert call(count=0) == 0 and call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, torch.ones(n, dtype=torch.float64, device=DEV) * out[0]) and abs(float(out[0]) - 1.0) < 1e-5
    with pytest.raises(RuntimeError):
        hipops.winding_number(pts.cpu(), tris)
