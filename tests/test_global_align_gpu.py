"""Global registration on the device (csrc/pose_search.hip) against the float64 NumPy restatement: ia_pose_scores within
``4 e32 + eps32 max(score, h^2)`` (e32: the restatement's own float32 run against its float64 run on the same inputs, never the kernel),
bit equality from run to run, across splits, permutations and offsets, the edge inputs, ``PoseField`` built on the device, ``global_align``
and ``align_mesh(init='global')`` against the transforms that were applied, the error paths of the ABI, and no torch gather on the path."""
import ctypes

import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, geometry, hipops
from test_global_align_cpu import POSES, shared
from test_surface_distance_cpu import EPS32, F32, extent_of, restatement_error

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_fields = {}


def device_field():
    """The 20-point field of the bumpy mesh built ON the device, once."""
    if 'bumpy' not in _fields:
        s = shared()
        _fields['bumpy'] = geometry.PoseField(dev(s.verts), dev(s.faces), resolution=20, padding=1)
    return _fields['bumpy']


def lattices():
    """(name, dist float32 [nx,ny,nz] on the host, origin, h, c_tgt): random values on (7, 8, 9), where an index-order mistake shows,
    and the device-built field of the bumpy mesh."""
    rs = np.random.RandomState(11)
    f = device_field()
    return [('random 7x8x9', rs.uniform(0.0, 1.0, size=(7, 8, 9)).astype(F32), (-0.4, 0.3, 1.1), 0.125, np.array([0.0, 0.8, 1.6])),
            ('bumpy field', f.dist.cpu().numpy(), f.origin, f.spacing, f.centroid)]


def points_for(rs, n, dist, origin, h):
    """n points about the lattice: most inside, every eighth far outside, and some exactly on the last lattice planes."""
    dims, org = np.array(dist.shape), np.array(origin)
    hi = org + (dims - 1) * h
    x = org + rs.uniform(size=(n, 3)) * (hi - org)
    x[::8] += rs.normal(size=x[::8].shape) * 3.0
    x[1::5, rs.randint(0, 3)] = hi[0]
    return x.astype(F32)


def scores(x, dist, origin, h, rot, c_src, c_tgt, **kw):
    return hipops.pose_scores(dev(x), dev(dist), origin, h, dev(rot.reshape(-1, 9).astype(F32)), c_src, c_tgt, **kw)


@pytest.mark.parametrize('shifts', [1, 3])
def test_pose_scores_against_float64(shifts):
    rs = np.random.RandomState(23)
    all_rot = shared().rotations
    worst = 0.0
    for name, dist, origin, h, c_tgt in lattices():
        for n in (1, 63, 64, 65, 257, 1000, 4096):
            for rot in (all_rot[:1], all_rot[[7, 2000]], all_rot[::46][:97]):
                if n >= 1000 and shifts == 3 and rot.shape[0] > 2:
                    continue                                                                 # (the restatement's time; shifts = 1 has this pair)
                x = points_for(rs, n, dist, origin, h)
                c_src = x.astype(np.float64).mean(0)
                # identity first, so that some points are inside whatever the rotation does
                args = (x, dist, origin, h, rot, c_src, c_tgt)
                kw = dict(shifts=shifts, shift_step=0.7 * h, scale=1.03, cap=2.5)
                ref = geometry._pose_scores_numpy(*args, **kw)
                r32 = geometry._pose_scores_numpy(*args, **kw, dtype=np.float32)
                got = scores(*args, **kw).cpu().numpy()
                assert got.shape == ref.shape == (rot.shape[0], shifts ** 3) and got.dtype == np.float64
                tol = 4 * np.abs(r32 - ref) + EPS32 * np.maximum(ref, h * h)
                ratio = float((np.abs(got - ref) / tol).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, n, rot.shape[0], ratio)
    print(f'shifts {shifts}: largest error / tolerance = {worst:.3g}')


def test_bit_equality():
    rs = np.random.RandomState(5)
    s = shared()
    name, dist, origin, h, c_tgt = lattices()[1]
    x = points_for(rs, 1000, dist, origin, h)
    c_src = x.astype(np.float64).mean(0)
    rot = s.rotations[::46][:96]
    a = scores(x, dist, origin, h, rot, c_src, c_tgt, shifts=3)
    assert torch.equal(a, scores(x, dist, origin, h, rot, c_src, c_tgt, shifts=3))           # run to run
    halves = torch.cat([scores(x, dist, origin, h, rot[:48], c_src, c_tgt, shifts=3), scores(x, dist, origin, h, rot[48:], c_src, c_tgt, shifts=3)])
    assert torch.equal(a, halves)                                                            # one call against two halves
    perm = rs.permutation(96)
    assert torch.equal(a[dev(perm)], scores(x, dist, origin, h, rot[perm], c_src, c_tgt, shifts=3))
    one = scores(x, dist, origin, h, rot, c_src, c_tgt, shifts=1)
    assert torch.equal(a[:, 13], one[:, 0])                                                  # the centre offset of shifts = 3
    single = scores(x, dist, origin, h, rot[5:6], c_src, c_tgt, shifts=3)                    # R = 1 cuts the offsets into chunks
    assert torch.equal(single[0], a[5])
    slab, hipops.POSE_SLAB = hipops.POSE_SLAB, 40
    try:
        assert torch.equal(a, scores(x, dist, origin, h, rot, c_src, c_tgt, shifts=3))       # slabs of 40, 40 and 16 rotations
    finally:
        hipops.POSE_SLAB = slab


def test_edge_inputs():
    rs = np.random.RandomState(9)
    name, dist, origin, h, c_tgt = lattices()[0]
    x = points_for(rs, 100, dist, origin, h)
    rot = shared().rotations[:5]
    c_src = x.astype(np.float64).mean(0)
    clean = scores(x, dist, origin, h, rot, c_src, c_tgt, shifts=3)
    bad = x.copy()
    bad[17, 1] = np.nan
    got = scores(bad, dist, origin, h, rot, c_src, c_tgt, shifts=3)
    assert got.shape == (5, 27) and bool(torch.isnan(got).all())                             # a NaN point: NaN for every candidate
    assert torch.equal(clean, scores(x, dist, origin, h, rot, c_src, c_tgt, shifts=3)) and bool(torch.isfinite(clean).all())
    hipops.PROFILE = []
    try:
        none = scores(x[:0], dist, origin, h, rot, c_src, c_tgt, shifts=3)
        empty = scores(x, dist, origin, h, rot[:0], c_src, c_tgt, shifts=3)
        launched = list(hipops.PROFILE)
    finally:
        hipops.PROFILE = None
    assert none.shape == (5, 27) and bool(torch.isnan(none).all()) and empty.shape == (0, 27) and launched == []
    with pytest.raises(ValueError):
        scores(np.zeros((4097, 3), dtype=F32), dist, origin, h, rot, c_src, c_tgt)
    with pytest.raises(ValueError):
        scores(x, dist, origin, h, rot, c_src, c_tgt, shifts=2)


def test_pose_field_on_device():
    """The device lattice against the restatement's.  It is closest_point at the float32 lattice points, so it is held to the bound of
    the closest-point tests (test_surface_distance_gpu.check_case): ``4 e32 + eps32 extent`` against the float64 restatement, e32 from
    the restatement's float32 run; taken at every third lattice point (1 800 of 5 400), which keeps the two brute-force runs short."""
    s = shared()
    f = device_field()
    assert f.dims == s.field.dims and f.origin == s.field.origin and f.spacing == s.field.spacing and f.dist.is_cuda
    assert np.array_equal(f.centroid, s.field.centroid) and f.radius == s.field.radius and f.extent == s.field.extent
    got = f.dist.cpu().numpy()
    assert got.shape == s.field.dist.shape and got.dtype == F32
    pts = np.stack(np.meshgrid(*geometry._lattice_axes(f.dims, f.origin, (f.spacing,) * 3), indexing='ij'), -1).reshape(-1, 3)[::3]
    d64, _, e32 = restatement_error(pts, s.verts, s.faces)
    tol = 4 * e32 + EPS32 * extent_of(pts, s.verts)
    err = np.abs(got.reshape(-1)[::3].astype(np.float64) - d64)
    print(f'field {f.dims}: largest error / tolerance = {float(err.max() / tol):.3g} (e32 = {e32:.3g})')
    assert (err <= tol).all()
    assert np.abs(got.astype(np.float64) - s.field.dist).max() <= 2 * tol                   # and the host field, everywhere


@pytest.mark.parametrize('k', [0, 1, 2])
def test_global_align_on_device(k):
    """Within the CPU test's tolerance of the truth, and the same optimum as the restatement (final matrices are compared, not the
    order of the candidates: near-equal scores may order differently in float32)."""
    s = shared()
    T, src = s.truth(k), s.source(k)
    tol, e32 = s.tolerance(src, T)
    verts, faces = dev(s.verts), dev(s.faces)
    r = geometry.global_align(dev(src), verts, faces, field=device_field())
    err, cpu = float(np.abs(r['matrix'] - T).max()), s.found(k)
    print(f'pose {k}: |M - truth| = {err:.3g}, |M - restatement| = {np.abs(r["matrix"] - cpu["matrix"]).max():.3g}, tolerance {tol:.3g}, '
          f'rms {r["rms"]:.3g}, refined candidate {r["rank"]} of {len(r["candidates"])}')
    assert r['searched'] == 4416 and len(r['candidates']) == 8 and err <= tol
    assert float(np.abs(r['matrix'] - cpu['matrix']).max()) <= 2 * tol                      # both within tol of the truth: the same optimum
    if k == 0:
        a = geometry.align_mesh(dev(src), verts, faces, init='global', search='tree', global_options={'field': device_field()})
        assert float(np.abs(a['matrix'] - r['matrix']).max()) <= tol and a['global']['rank'] == r['rank']
        with pytest.raises(ValueError, match='not this target'):
            geometry.global_align(dev(src), verts, faces, field=s.field)                     # a host field for a device mesh


def test_abi_error_paths():
    lib = _lib.load()
    n, R = 8, 2
    pts, dist = torch.zeros(n, 3, device='cuda'), torch.ones(8, 8, 8, device='cuda')
    rot = torch.eye(3, device='cuda').reshape(1, 9).repeat(R, 1).contiguous()
    out = torch.full((R,), 3.0, dtype=torch.float64, device='cuda')
    org, c = (ctypes.c_float * 3)(0, 0, 0), hipops._d3((0, 0, 0))

    def call(p=pts.data_ptr(), count=n, d=dist.data_ptr(), dims=(8, 8, 8), o=org, h=0.1, r=rot.data_ptr(), cs=c, shifts=1, res=out.data_ptr()):
        return lib.ia_pose_scores(p, count, d, *dims, o, h, r, R, cs, c, shifts, 0.1, 1.0, float('inf'), res, None)
    assert call(p=None) == -1 and 'device pointers' in _lib.last_error()
    assert call(p=torch.zeros(n, 3).data_ptr()) == -1 and 'device pointers' in _lib.last_error()
    assert call(d=None) == -1 and call(r=None) == -1 and call(res=None) == -1 and 'device pointers' in _lib.last_error()
    assert call(o=None) == -1 and 'h_origin' in _lib.last_error()
    assert call(cs=None) == -1 and 'h_c_src' in _lib.last_error()
    assert call(count=4097) == -1 and '4096' in _lib.last_error() and 'samples=' in _lib.last_error()
    assert call(shifts=2) == -1 and 'odd' in _lib.last_error()
    assert call(dims=(1, 8, 8)) == -1 and '>= 2' in _lib.last_error()
    assert call(h=0.0) == -1 and call(h=-1.0) == -1 and 'positive' in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == 3).all())                                                            # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


def test_no_torch_gather_on_the_device_path(monkeypatch):
    s = shared()
    def refuse(*a, **k):
        raise AssertionError('a torch gather on the device path')
    f = device_field()
    src, verts, faces = dev(s.source(0)), dev(s.verts), dev(s.faces)
    for name in ('gather', 'take_along_dim', 'index_select'):
        monkeypatch.setattr(torch, name, refuse)
        monkeypatch.setattr(torch.Tensor, name, refuse)
    monkeypatch.setattr(torch.nn.functional, 'grid_sample', refuse)
    hipops.PROFILE = []
    try:
        got = geometry.pose_scores(src, f, s.rotations[:64], shifts=3)
        families = [e[0] for e in hipops.PROFILE]
    finally:
        hipops.PROFILE = None
    assert got.is_cuda and got.shape == (64, 27) and families == ['pose_scores']
