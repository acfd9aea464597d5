"""ia_query_planes and ia_density_grid against the float64 restatement of tests/query_reference.py (whose agreement with the project's
definition tests/test_query_planes_cpu.py establishes), on non-square planes, at and beyond the plane borders, with a saturating
decoder, and bit for bit against themselves where the launch takes another path: grid-stride trips beyond the launch cap of 2048
workgroups, ragged 4 x 8 x 8 lattice tiles, batches, the flip, density-only launches.

Tolerance of every comparison with float64: ``4 x max|CPU fp32 route - fp64|`` on the same inputs, separately for sigma and rgb (the
device and the CPU route make rounding errors of the same kind in another order: 2x if they add; the maximum is over a sample, not the
worst case: 2x), and never above the project's fp32 bars (``query_reference.bars``).

Outputs are handed to the kernels pre-filled with NaN, so a value the launch did not write cannot pass as a stale correct one."""
import ctypes

import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, geometry, hipops
from conftest import max_abs
import query_reference as QR

pytestmark = pytest.mark.gpu

CAP_POINTS = 2048 * 256            # points (and, for the lattice, 2048 tiles) that one trip of the persistent launches covers


class Case:
    """Planes [B,3,32,h,w] and decoder weights on the host (for the references) and on the device (channels-last planes)."""

    def __init__(self, planes, weights, lr=1.0):
        self.planes, self.weights, self.lr = planes, weights, lr
        self.planes_cl = planes.permute(0, 1, 3, 4, 2).contiguous().cuda()
        self.dev_weights = tuple(t.cuda() for t in weights)
        self.decoder = QR.make_decoder(weights, lr)

    def device_decoder(self):
        return QR.make_decoder(self.weights, self.lr).cuda()

    def batch(self, b):
        return Case(self.planes[b:b + 1], self.weights, self.lr)


@pytest.fixture(scope='module')
def case():
    return Case(QR.make_planes(20, 3), QR.make_decoder_weights(21))


def _p(t):
    return None if t is None else t.data_ptr()


def _f3(values):
    return (ctypes.c_float * 3)(*[float(v) for v in values])


def query(c, pts, box_warp=1.0, flip_z=False, rgb=True):
    """ia_query_planes on NaN-filled outputs: (sigma [B,M,1], rgb [B,M,32] or None); no NaN may be left."""
    pts = pts.cuda().float().contiguous()
    b, m = pts.shape[:2]
    bp, ph, pw = c.planes_cl.shape[0], c.planes_cl.shape[2], c.planes_cl.shape[3]
    assert b == bp and pts.shape[2] == 3
    sigma = torch.full((b, m, 1), float('nan'), device='cuda')
    col = torch.full((b, m, 32), float('nan'), device='cuda') if rgb else None
    st = _lib.load().ia_query_planes(_p(c.planes_cl), _p(pts), *(_p(t) for t in c.dev_weights), float(c.lr), float(box_warp),
                                     1 if flip_z else 0, b, m, ph, pw, _p(sigma), _p(col), _lib.stream_ptr(pts.device))
    _lib.check(st, 'ia_query_planes')
    assert not torch.isnan(sigma).any() and (col is None or not torch.isnan(col).any()), 'the launch left outputs unwritten'
    return sigma, col


def density_grid(c, res, length, origin, box_warp=1.0, flip_z=False):
    """ia_density_grid on a NaN-filled volume [B,nx,ny,nz]; no NaN may be left."""
    b, ph, pw = c.planes_cl.shape[0], c.planes_cl.shape[2], c.planes_cl.shape[3]
    vol = torch.full((b, *res), float('nan'), device='cuda')
    st = _lib.load().ia_density_grid(_p(c.planes_cl), *(_p(t) for t in c.dev_weights), float(c.lr), float(box_warp), 1 if flip_z else 0,
                                     b, ph, pw, *res, _f3(length), _f3(origin), _p(vol), _lib.stream_ptr(vol.device))
    _lib.check(st, 'ia_density_grid')
    assert not torch.isnan(vol).any(), 'the launch left voxels unwritten'
    return vol


_references = {}


def reference(c, pts, box_warp, flip_z, key=None):
    """(sigma fp64, rgb fp64, tol sigma, tol rgb, CPU deviation sigma, CPU deviation rgb) for host points [B,M,3]; computed once per key."""
    if key is not None and key in _references:
        return _references[key]
    sigma, rgb = QR.query_fp64(c.planes, *c.weights, pts, box_warp, lr_multiplier=c.lr, flip_z=flip_z)
    with torch.no_grad():
        cpu = geometry.query_planes(c.planes, c.decoder, pts.clone(), box_warp, flip_z=flip_z)
    d_sigma, d_rgb = max_abs(cpu['sigma'], sigma), max_abs(cpu['rgb'], rgb)
    bar_sigma, bar_rgb = QR.bars(sigma)
    assert d_sigma <= bar_sigma and d_rgb <= bar_rgb, 'the inputs must keep the CPU route inside the bars'
    out = (sigma, rgb, min(4.0 * d_sigma, bar_sigma), min(4.0 * d_rgb, bar_rgb), d_sigma, d_rgb)
    if key is not None:
        _references[key] = out
    return out


def check_fp64(what, c, pts, got_sigma, got_rgb, box_warp=1.0, flip_z=False, key=None):
    sigma, rgb, tol_sigma, tol_rgb, cpu_sigma, cpu_rgb = reference(c, pts, box_warp, flip_z, key)
    assert got_sigma.shape == sigma.shape and got_sigma.dtype == torch.float32 and torch.isfinite(got_sigma).all()
    d_sigma = max_abs(got_sigma.cpu(), sigma)
    line = f'{what}: sigma device {d_sigma:.2e} / CPU {cpu_sigma:.2e} / tol {tol_sigma:.2e}'
    d_rgb = 0.0
    if got_rgb is not None:
        assert got_rgb.shape == rgb.shape and got_rgb.dtype == torch.float32 and torch.isfinite(got_rgb).all()
        d_rgb = max_abs(got_rgb.cpu(), rgb)
        line += f'; rgb device {d_rgb:.2e} / CPU {cpu_rgb:.2e} / tol {tol_rgb:.2e}'
    print(line + '  (max|. - fp64|)')
    assert d_sigma <= tol_sigma and d_rgb <= tol_rgb, line


# ------------------------------------------------------------------ against float64

@pytest.mark.parametrize('rgb', [True, False])
@pytest.mark.parametrize('flip_z', [False, True])
@pytest.mark.parametrize('box_warp', [1.0, 0.7])
@pytest.mark.parametrize('m', [1, 255, 257, 700])
def test_query_vs_fp64_on_non_square_planes(case, m, box_warp, flip_z, rgb):
    assert case.planes_cl.shape == (3, 3, 24, 40, 32)
    pts = QR.edge_points(40 + m, 3, m, box_warp)
    sigma, col = query(case, pts, box_warp, flip_z, rgb)
    check_fp64(f'24x40 M={m} box_warp={box_warp} flip_z={flip_z} rgb={rgb}', case, pts, sigma, col, box_warp, flip_z, key=(m, box_warp, flip_z))


@pytest.mark.parametrize('size,amplitude', QR.SQUARE_CASES)
def test_query_vs_fp64_on_square_planes(size, amplitude):
    c = Case(QR.make_planes(30 + size, 1, size, size, amplitude=amplitude), QR.make_decoder_weights(21))
    assert c.planes_cl.shape == (1, 3, size, size, 32)
    pts = QR.edge_points(27, 1, 3000, 1.0, size, size)
    check_fp64(f'{size}x{size} M=3000', c, pts, *query(c, pts))


@pytest.mark.parametrize('lr,factor', QR.HOT_CASES)
def test_hot_decoder_vs_fp64(lr, factor):
    """Both branches of the softplus and both saturations of the sigmoid, through raw weights and ``lr_multiplier``."""
    c = Case(QR.make_planes(20, 3), QR.make_decoder_weights(21, w0_factor=factor), lr)
    pts = QR.edge_points(26, 3, 700, 1.0)
    q = QR.query_parts_fp64(c.planes, *c.weights, pts, 1.0, lr_multiplier=lr)
    assert q['pre'].max() > 25 and q['pre'].min() < -25 and q['out'][..., 1:].max() > 20 and q['out'][..., 1:].min() < -20
    sigma, col = query(c, pts)
    check_fp64(f'hot decoder lr_multiplier={lr} (pre-activations {q["pre"].min():.1f} .. {q["pre"].max():.1f})', c, pts, sigma, col)
    assert -0.001 - 2e-7 <= col.min() < -0.0009 and 1.0009 < col.max() <= 1.001 + 2e-7        # both saturations, one float32 rounding
    assert torch.equal(query(c, pts, rgb=False)[0], sigma)


def test_through_the_module_with_lr_multiplier(case):
    """``geometry.query_planes`` on device tensors: NCHW planes, the gains read from the OSGDecoder module."""
    c = Case(case.planes, case.weights, 0.5)
    pts = QR.edge_points(25, 3, 700, 0.7)
    with torch.no_grad():
        got = geometry.query_planes(c.planes.cuda(), c.device_decoder(), pts.cuda(), 0.7, flip_z=True)
    check_fp64('geometry.query_planes lr_multiplier=0.5 box_warp=0.7 flip_z', c, pts, got['sigma'], got['rgb'], 0.7, True)
    sigma, col = query(c, pts, 0.7, True)
    assert torch.equal(got['sigma'], sigma) and torch.equal(got['rgb'], col)
    assert max_abs(query(case, pts, 0.7, True)[1].cpu(), col.cpu()) > 0.05          # lr_multiplier is not ignored


def test_vertex_colors_vs_fp64(case):
    verts = QR.edge_points(29, 1, 400, 1.0)[0]
    c = case.batch(0)
    with torch.no_grad():
        got = geometry.vertex_colors(c.planes.cuda(), c.device_decoder(), verts.cuda(), 1.0)
    ref = QR.quantise_colors(QR.query_fp64(c.planes, *c.weights, verts[None], 1.0)[1][0])
    diff = (got.cpu().int() - ref.int()).abs()
    print(f'vertex_colors: {int((diff != 0).sum())} of {diff.numel()} 8-bit values differ from the quantised fp64 colours, max {int(diff.max())}')
    assert got.dtype == torch.uint8 and got.shape == (400, 3) and int(diff.max()) <= 1 and (diff == 0).double().mean() >= 0.99


# ------------------------------------------------------------------ exact identities

LATTICE = dict(factors=(1.3, 0.9, 2.5), origin=(0.21, -0.1, 0.63))      # some corner of every lattice lies inside all planes


def _lattice(res, box_warp):
    length = tuple(f * box_warp for f in LATTICE['factors'])
    return length, LATTICE['origin'], geometry.lattice_points(res, length, LATTICE['origin'])


@pytest.mark.parametrize('flip_z', [False, True])
@pytest.mark.parametrize('res', [(5, 9, 13), (2, 2, 2), (4, 8, 8), (7, 17, 3)])
def test_lattice_equals_point_query(case, res, flip_z):
    box_warp = 0.7
    length, origin, pts = _lattice(res, box_warp)
    outside = (pts.abs() > box_warp / 2).any(1)
    assert outside.any() and not outside.all()
    vol = density_grid(case, res, length, origin, box_warp, flip_z)
    sigma, _ = query(case, pts[None].expand(3, -1, -1), box_warp, flip_z, rgb=False)
    assert vol.shape == (3, *res) and torch.equal(vol.reshape(3, -1), sigma.reshape(3, -1))
    with torch.no_grad():
        wrapped = hipops.density_grid(case.planes_cl, *case.dev_weights, res, length, origin, box_warp=box_warp, flip_z=flip_z)
    assert torch.equal(wrapped, vol)


@pytest.mark.parametrize('flip_z', [False, True])
def test_ragged_lattice_vs_fp64(case, flip_z):
    res, box_warp = (5, 9, 13), 0.7
    length, origin, pts = _lattice(res, box_warp)
    with torch.no_grad():
        vol = geometry.density_volume(case.planes.cuda(), case.device_decoder(), res, length, origin, box_warp=box_warp, flip_z=flip_z)
    assert torch.equal(vol, density_grid(case, res, length, origin, box_warp, flip_z))
    check_fp64(f'lattice {res} flip_z={flip_z}', case, pts[None].expand(3, -1, -1), vol.reshape(3, -1, 1), None, box_warp, flip_z)


def _beyond(m, lo):
    """4096 indices into [0, m): half from all of it, half from [lo, m)."""
    rs = np.random.RandomState(7)
    return torch.from_numpy(np.concatenate([rs.randint(0, m, 2048), rs.randint(lo, m, 2048)]))


def test_point_query_beyond_the_launch_cap(case):
    m = 600_000
    c = case.batch(1)
    pts = QR.edge_points(50, 1, m, 1.0)
    sigma, _ = query(c, pts, rgb=False)
    tail, _ = query(c, pts[:, CAP_POINTS:], rgb=False)
    head, _ = query(c, pts[:, :CAP_POINTS], rgb=False)
    assert m > CAP_POINTS and torch.equal(sigma[:, CAP_POINTS:], tail) and torch.equal(sigma[:, :CAP_POINTS], head)
    idx = _beyond(m, CAP_POINTS)
    check_fp64(f'B=1 M={m}, 4096 sampled', c, pts[:, idx], sigma[:, idx.cuda()], None)


def test_point_query_beyond_the_launch_cap_across_batches(case):
    m = 200_000
    pts = QR.edge_points(51, 3, m, 1.0)
    sigma, _ = query(case, pts, rgb=False)
    assert 3 * m > CAP_POINTS > 2 * m                               # the second trip starts inside batch element 2
    for b in range(3):
        assert torch.equal(sigma[b:b + 1], query(case.batch(b), pts[b:b + 1], rgb=False)[0]), b
    idx = _beyond(m, CAP_POINTS - 2 * m)
    check_fp64(f'B=3 M={m}, 3 x 4096 sampled', case, pts[:, idx], sigma[:, idx.cuda()], None)
    # with colours the same launch shape writes 32 more values per point
    sub = pts[:, :180_000]
    col = query(case, sub)[1]
    assert 3 * 180_000 > CAP_POINTS
    for b in range(3):
        assert torch.equal(col[b:b + 1], query(case.batch(b), sub[b:b + 1])[1]), b


def test_lattice_beyond_the_launch_cap(case):
    res, box_warp = (130, 64, 64), 1.0
    c = case.batch(2)
    length, origin, pts = _lattice(res, box_warp)
    assert -(-res[0] // 4) * (res[1] // 8) * (res[2] // 8) == 2112 > 2048
    vol = density_grid(c, res, length, origin, box_warp)
    half = pts.shape[0] // 2
    assert half <= CAP_POINTS
    sigma = torch.cat([query(c, pts[None, s:s + half], box_warp, rgb=False)[0] for s in (0, half)], 1)
    assert torch.equal(vol.reshape(1, -1), sigma.reshape(1, -1))
    idx = _beyond(pts.shape[0], 128 * 64 * 64)                      # x index >= 128: tiles 2048 .. 2111
    check_fp64(f'lattice {res}, 4096 sampled', c, pts[None, idx], vol.reshape(1, -1, 1)[:, idx.cuda()], None, box_warp)


def test_batch_independence(case):
    pts = QR.edge_points(52, 3, 700, 1.0)
    sigma, col = query(case, pts)
    for b in range(3):
        s1, c1 = query(case.batch(b), pts[b:b + 1])
        assert torch.equal(sigma[b:b + 1], s1) and torch.equal(col[b:b + 1], c1), b
    assert max_abs(col[0].cpu(), query(case.batch(1), pts[:1])[1][0].cpu()) > 0.1      # the planes of another element do differ


def test_flip_is_z_negated(case):
    pts = QR.edge_points(53, 3, 700, 0.7)
    neg = pts * torch.tensor([1.0, 1.0, -1.0])
    a, b = query(case, pts, 0.7, flip_z=True), query(case, neg, 0.7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert max_abs(a[1].cpu(), query(case, pts, 0.7)[1].cpu()) > 0.1


def test_sigma_with_and_without_rgb(case):
    pts = QR.edge_points(54, 3, 700, 1.0)
    assert torch.equal(query(case, pts, rgb=True)[0], query(case, pts, rgb=False)[0])


def test_outside_points_are_decoder_of_zero(case):
    """No tap inside any plane: one value, the same bits for every such point, for a point at 1e30 and for NaN and infinite coordinates
    (the kernel gives such taps the weight 0)."""
    out = QR.outside_points(0.7)
    nan, inf = float('nan'), float('inf')
    odd = torch.tensor([[[1e30, 1e30, 1e30], [-1e30, 1e30, -1e30], [3e38, -3e38, 3e38], [nan, nan, nan], [inf, -inf, inf], [nan, 0.1, 0.2],
                         [0.1, inf, -inf], [-inf, nan, 0.0]]])
    c = case.batch(0)
    sigma, col = query(c, torch.cat([out, odd], 1), 0.7)
    assert torch.isfinite(sigma).all() and torch.isfinite(col).all()
    assert torch.equal(sigma, sigma[:, :1].expand_as(sigma)) and torch.equal(col, col[:, :1].expand_as(col))
    zero = QR.decoder_fp64(torch.zeros(1, out.shape[1], 32, dtype=torch.float64), *c.weights)
    ref_sigma, ref_rgb = QR.query_fp64(c.planes, *c.weights, out, 0.7)
    assert torch.equal(ref_sigma, zero['sigma']) and torch.equal(ref_rgb, zero['rgb'])
    # the value itself, in a population large enough for the tolerance rule
    pts = torch.cat([out, QR.edge_points(56, 1, 700, 0.7)], 1)
    got = query(c, pts, 0.7)
    assert torch.equal(got[0][:, :out.shape[1]], sigma[:, :out.shape[1]]) and torch.equal(got[1][:, :out.shape[1]], col[:, :out.shape[1]])
    check_fp64('outside all planes + 700 edge points', c, pts, *got, 0.7)


def test_two_launches_give_equal_bits(case):
    pts = QR.edge_points(55, 3, 700, 1.0)
    a, b = query(case, pts), query(case, pts)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    length, origin, _ = _lattice((7, 17, 3), 1.0)
    assert torch.equal(density_grid(case, (7, 17, 3), length, origin), density_grid(case, (7, 17, 3), length, origin))


def test_empty_input(case):
    pts = torch.zeros(3, 0, 3, device='cuda')
    sigma, col = hipops.query_planes(case.planes_cl, pts, *case.dev_weights)
    assert sigma.shape == (3, 0, 1) and col.shape == (3, 0, 32)
    sigma, col = hipops.query_planes(case.planes_cl, pts, *case.dev_weights, rgb=False)
    assert sigma.shape == (3, 0, 1) and col is None
    with torch.no_grad():
        got = geometry.query_planes(case.planes.cuda(), case.device_decoder(), pts, 1.0)
    assert got['sigma'].shape == (3, 0, 1) and got['rgb'].shape == (3, 0, 32)
    torch.cuda.synchronize()
