"""TSDF integration on the device (csrc/tsdf.hip) against the float32 NumPy restatement: ``sum``, ``weight``, ``color_sum``,
``color_weight`` and ``tsdf`` bit for bit on lattices below and above one workgroup, odd image sizes, 1 / 3 / 7 views, 0 / 1 / 3 / 8 colour
channels, with and without mask and weights, on depth images seeded with unusable values (the case builder asserts that every branch
is taken); the slab identity through ``state``; two runs; ``fused_mesh`` against its restatement; the error paths."""
import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, geometry, hipops
from fuse_depth_cases import CHANNELS, EPS32, F32, IMAGES, LATTICES, SUMS, VIEWS, case, same_bits, sphere_fusion, sphere_scan

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_same(got, ref, what):
    for key in SUMS + ('tsdf', 'color', 'observed'):
        assert (key in got) == (key in ref), (what, key)
        if key in ref:
            assert same_bits(got[key].cpu().numpy(), ref[key]), (what, key)
    assert got['info'] == ref['info'] and got['origin'] == ref['origin'] and got['truncation'] == ref['truncation'], what


@pytest.mark.parametrize('n_views', VIEWS)
@pytest.mark.parametrize('hw', IMAGES)
@pytest.mark.parametrize('dims', LATTICES)
def test_device_gives_the_bits_of_the_restatement(dims, hw, n_views):
    for channels in CHANNELS:
        for optional in (False, True):
            c = case(dims, hw, n_views, channels, optional)
            got = c.fuse(to=dev)
            assert got['sum'].is_cuda and got['tsdf'].dtype == torch.float32 and tuple(got['tsdf'].shape) == dims
            assert_same(got, c.reference, (dims, hw, n_views, channels, optional))
    print(f'{dims} {hw} N={n_views}: {c.hits}')


@pytest.mark.parametrize('dims', LATTICES)
def test_slab_identity_and_two_runs_on_device(dims):
    for channels in (0, 3):
        c = case(dims, IMAGES[1], 7, channels, True)
        whole = c.fuse(to=dev)
        again = c.fuse(to=dev)
        first = c.fuse(slice(0, 3), to=dev)
        kept = {k: first[k].clone() for k in SUMS if k in first}
        both = c.fuse(slice(3, 7), state=first, to=dev)
        for key in SUMS + ('tsdf',):
            if key in whole:
                assert torch.equal(whole[key], again[key]) and torch.equal(whole[key].view(torch.int32), both[key].view(torch.int32)), key
        assert all(torch.equal(first[k], kept[k]) for k in kept)                   # the state is not modified
        host_first = c.fuse(slice(0, 3))                                           # a state from the host continues on the device
        mixed = c.fuse(slice(3, 7), state=host_first, to=dev)
        assert torch.equal(mixed['sum'], whole['sum']) and torch.equal(mixed['weight'], whole['weight'])


def test_fused_mesh_on_device_against_numpy():
    host = sphere_fusion()
    fusion = sphere_scan().fuse(to=dev)
    assert_same(fusion, host, 'sphere')
    for min_weight in (0.0, 2.5):
        v, f, col = geometry.fused_mesh(fusion, min_weight, with_colors=True)
        rv, rf, rcol = geometry.fused_mesh(host, min_weight, with_colors=True)
        assert v.is_cuda and f.dtype == torch.int64 and f.shape[0] > 0
        assert same_bits(v.cpu().numpy(), rv) and np.array_equal(f.cpu().numpy(), rf), min_weight
        err = float(np.abs(col.cpu().numpy() - rcol).max())
        print(f'min_weight {min_weight}: {rf.shape[0]} faces, colours differ by {err:.3g}, bound {4 * EPS32 * float(np.abs(rcol).max()):.3g}')
        assert err <= 4 * EPS32 * float(np.abs(rcol).max())
    v2, f2 = geometry.fused_mesh(fusion)
    assert torch.equal(v2, geometry.fused_mesh(fusion, 0.0, with_colors=True)[0]) and f2.shape[0] > rf.shape[0]


def test_error_paths_go_through_last_error():
    lib = _lib.load()
    c = case(LATTICES[0], IMAGES[0], 3, 3, True)
    depth, views = dev(c.depth), torch.zeros(3, 18, device='cuda')
    out = [torch.empty(c.dims, device='cuda') for _ in range(4)]
    csum, colors = torch.empty(c.dims + (3,), device='cuda'), dev(c.colors)
    lo, step = hipops._f3(c.origin), hipops._f3(c.spacing)

    def call(depth=depth.data_ptr(), n=3, ch=3, h=12, w=16, dims=c.dims, tau=0.08, near=1e-6, colors=colors.data_ptr()):
        return lib.ia_tsdf_integrate(depth, None, None, colors, views.data_ptr(), n, ch, h, w, *dims, lo, step, tau, near, 0, out[0].data_ptr(),
                                     out[1].data_ptr(), out[2].data_ptr(), csum.data_ptr(), out[3].data_ptr(), None)
    assert call() == 0
    assert call(n=0) == -1 and 'N must be >= 1' in _lib.last_error()
    assert call(ch=9) == -1 and 'colour channels' in _lib.last_error()
    assert call(ch=0) == -1 and 'exactly when C > 0' in _lib.last_error()
    assert call(tau=0.0) == -1 and 'truncation' in _lib.last_error()
    assert call(tau=float('nan')) == -1 and 'truncation' in _lib.last_error()
    assert call(near=-1.0) == -1 and 'near' in _lib.last_error()
    assert call(h=0) == -1 and 'pixels per side' in _lib.last_error()
    assert call(dims=(1, 7, 5)) == -1 and 'every dimension must be >= 2' in _lib.last_error()
    assert call(depth=torch.zeros(3, 12, 16).data_ptr()) == -1 and 'device pointer' in _lib.last_error()
    with pytest.raises(RuntimeError, match='views'):
        hipops.tsdf_integrate(depth, views[:2], c.dims, c.origin, c.spacing, 0.08)
    with pytest.raises(RuntimeError, match='bool'):
        hipops.tsdf_integrate(depth, views, c.dims, c.origin, c.spacing, 0.08, mask=depth)
    with pytest.raises(ValueError, match='float32 on the device'):
        geometry.fuse_depth(depth, dev(c.cams), c.dims, c.origin, c.spacing, dtype=np.float64)
    with pytest.raises(ValueError, match='same lattice'):
        geometry.fuse_depth(depth, dev(c.cams), c.dims, c.origin, c.spacing, state=case(LATTICES[1], IMAGES[0], 3, 0, False).reference)
    assert call() == 0
