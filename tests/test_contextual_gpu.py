"""The contextual loss on the device: ia_resize_bilinear, the head's kernels (ia_cx_channel_mean, ia_cx_normalize, ia_cx_rows, ia_cx_cols,
ia_cx_finish) at their edges, and the score end to end through the VGG19 trunk, against the float64 restatement
(tests/contextual_reference.py).

Bound (the project's): |device - float64| <= M * e32 + eps32 * scale, where e32 is the distance of the float32 CPU run of the same
statement from float64 on the same inputs, scale the largest float64 magnitude of the compared tensor, M = 4 for the resize, the means,
the normalised operand and the head on given fp32 features, and M = 16 end to end through the trunk (the cap DESIGN.md 4.25 established
for VGG layers on fp16 hi / lo pairs: the trunk is those kernels).  Both numbers are printed per comparison."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from invertavatar_amd import contextual
from invertavatar_amd import image_metrics as im
from invertavatar_amd import lpips

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contextual_reference as CR  # noqa: E402

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23
TRUNK_MULTIPLE = 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'contextual.npz')


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def check(name, got, ref64, ref32, multiple=4):
    got, ref64, ref32 = got.double().cpu(), ref64.double(), ref32.double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    e32 = (ref32 - ref64).abs().max().item()
    err = (got - ref64).abs().max().item()
    scale = ref64.abs().max().item()
    bound = multiple * e32 + EPS32 * scale
    print(f'{name}: err {err:.3e}  e32 {e32:.3e}  err/e32 {err / max(e32, 1e-300):.2f}  scale {scale:.3e}  bound {bound:.3e}')
    assert err <= bound, f'{name}: {err:.3e} > {bound:.3e}'


# ------------------------------------------------------------------ ia_resize_bilinear

def resized(x, size, dt):
    return F.interpolate(x.to(dt), size, mode='bilinear', align_corners=False)


@pytest.mark.parametrize('src,dst', [((5, 9), (3, 4)), ((3, 4), (7, 5)), ((300, 260), (256, 256))])
def test_resize_against_float64(src, dst):
    from invertavatar_amd import hipops
    x = rnd(src[0] + dst[1], 2, 3, *src)
    got = hipops.resize_bilinear(x.cuda(), dst)
    check(f'resize {src}->{dst}', got, resized(x, dst, torch.float64), resized(x, dst, torch.float32))
    assert torch.equal(got, hipops.resize_bilinear(x.cuda(), dst))
    assert torch.equal(got[1:], hipops.resize_bilinear(x[1:].cuda(), dst))


def test_resize_half_branch_has_the_bits_of_the_general_path_and_uint8_front_end():
    from invertavatar_amd import hipops
    x = rnd(5, 1, 3, 512, 512)
    a, b = hipops.resize_bilinear(x.cuda(), (256, 256)), hipops.resize_bilinear(x.cuda(), (256, 256), general=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    check('resize 512->256', a, resized(x, (256, 256), torch.float64), resized(x, (256, 256), torch.float32))
    u = torch.randint(0, 256, (2, 37, 300, 3), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)

    def ref(dt):
        return resized(u.permute(0, 3, 1, 2).to(dt) / 127.5 - 1.0, (256, 256), dt)
    check('resize uint8 37x300->256x256', hipops.resize_bilinear(u.cuda(), (256, 256)), ref(torch.float64), ref(torch.float32))
    u2 = torch.randint(0, 256, (1, 64, 48, 3), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    a, b = hipops.resize_bilinear(u2.cuda(), (32, 24)), hipops.resize_bilinear(u2.cuda(), (32, 24), general=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    same = hipops.resize_bilinear(u2.cuda(), (64, 48))               # the identity resize is the uint8 -> [-1, 1] mapping
    assert torch.equal(same.cpu(), u2.permute(0, 3, 1, 2).float() / 127.5 - 1.0)


# ------------------------------------------------------------------ the head on given features

def tiles():
    from invertavatar_amd import hipops
    return hipops.cx_layout()


def head_case(name):
    """(fx, fy, mu) of the named case: float32 [N,C,h,w] maps and 'frame' or a float32 [1,C] table of shifts."""
    fx, fy, mu = _head_case(name)
    return fx.contiguous(), fy.contiguous(), mu


def _head_case(name):
    t, _ = tiles()
    if name == 'c20_p35':
        return (*CR.relu_maps(CR.FEATURE_SEED, 2, 20, 5, 7), 'frame')
    if name == 'c1_p1':
        return (*CR.relu_maps(11, 1, 1, 1, 1), 'frame')
    if name == 'c256_tile_plus_1':
        return (*CR.relu_maps(12, 1, 256, 1, t + 1), 'frame')
    if name == 'c256_two_tiles_plus_3':
        return (*CR.relu_maps(13, 1, 256, 1, 2 * t + 3), 'frame')
    if name == 'c256_p4096':
        return (*CR.relu_maps(14, 1, 256, 64, 64), 'frame')
    if name == 'x_equals_y':
        fx, _ = CR.relu_maps(15, 1, 48, 9, 9)
        return fx, fx.clone(), 'frame'
    if name == 'zero_position':
        fx, fy = CR.relu_maps(16, 2, 24, 6, 7)
        fx[0, :, 2, 3] = 0.0
        fy[1, :, 0, 0] = 0.0
        return fx, fy, 'frame'
    if name == 'position_equal_to_mu':
        fx, fy = CR.relu_maps(17, 1, 24, 6, 7)
        mu = fy.double().mean(dim=(2, 3)).float()                    # the table the head is given: [1,C]
        fx[0, :, 1, 1] = mu[0]                                       # exactly zero after centring, d = 1 against every y
        return fx, fy, mu
    raise KeyError(name)


HEAD_CASES = ['c20_p35', 'c1_p1', 'c256_tile_plus_1', 'c256_two_tiles_plus_3', 'c256_p4096', 'x_equals_y', 'zero_position',
              'position_equal_to_mu']


@pytest.mark.parametrize('name', HEAD_CASES)
def test_head_against_float64(name):
    from invertavatar_amd import hipops
    fx, fy, mu = head_case(name)
    cx, loss, dbg = hipops.cx_head(fx.cuda(), fy.cuda(), 0.5, mu.cuda() if torch.is_tensor(mu) else mu, debug=True)
    r64 = CR.head_stages(fx.double(), fy.double(), 0.5, mu)
    r32 = CR.head_stages(fx, fy, 0.5, mu)
    c = fx.shape[1]
    assert torch.isfinite(loss).all()
    check(f'{name} mu', dbg['mu'], r64['mu'], r32['mu'])
    if name == 'position_equal_to_mu':
        assert bool((dbg['xh'][0, 7 + 1] == 0).all()) and bool((dbg['m'][0, 7 + 1] == 1.0).all())
    assert bool((dbg['xh'][:, :, c:] == 0).all()) and bool((dbg['yh'][:, :, c:] == 0).all())
    check(f'{name} x^', dbg['xh'][:, :, :c], r64['xh'], r32['xh'])
    check(f'{name} y^', dbg['yh'][:, :, :c], r64['yh'], r32['yh'])
    for key in ('m', 's', 'colmax'):
        check(f'{name} {key}', dbg[key], r64[key], r32[key])
    check(f'{name} cx', cx, r64['cx'], r32['cx'])
    check(f'{name} cx_loss', loss, r64['cx_loss'], r32['cx_loss'])


def test_head_nan_stays_in_its_frame():
    from invertavatar_amd import hipops
    fx, fy = CR.relu_maps(18, 3, 24, 6, 7)
    clean = hipops.cx_head(fx.cuda(), fy.cuda(), 0.5, 'frame')
    fx[1, 5, 2, 2] = float('nan')
    cx, loss, dbg = hipops.cx_head(fx.cuda(), fy.cuda(), 0.5, 'frame', debug=True)
    assert bool(torch.isnan(cx[1])) and bool(torch.isnan(loss[1]))
    assert bool(torch.isnan(dbg['m'][1, 2 * 7 + 2])) and int(torch.isnan(dbg['m'][1]).sum()) == 1
    for n in (0, 2):
        assert torch.equal(cx[n], clean[0][n]) and torch.equal(loss[n], clean[1][n])
    want = CR.head_stages(fx.double(), fy.double(), 0.5, 'frame')['cx']
    assert torch.isnan(want).tolist() == [False, True, False]


def test_head_invariants_bit_for_bit():
    from invertavatar_amd import hipops
    t, step = tiles()
    fx, fy = CR.relu_maps(19, 3, 40, 5, t // 4 + 3)
    fxd, fyd = fx.cuda(), fy.cuda()
    cx, loss = hipops.cx_head(fxd, fyd, 0.5, 'frame')
    again = hipops.cx_head(fxd, fyd, 0.5, 'frame')
    assert torch.equal(cx, again[0]) and torch.equal(loss, again[1])
    for n in (0, 2):                                                # a frame alone, from both ends of the batch
        alone = hipops.cx_head(fxd[n:n + 1].contiguous(), fyd[n:n + 1].contiguous(), 0.5, 'frame')
        assert torch.equal(alone[0], cx[n:n + 1]) and torch.equal(alone[1], loss[n:n + 1])
        batch1 = hipops.cx_head(fxd[n:n + 1].contiguous(), fyd[n:n + 1].contiguous(), 0.5, 'batch')
        assert torch.equal(batch1[0], alone[0]) and torch.equal(batch1[1], alone[1])
        assert torch.equal(contextual.contextual_loss(fxd[n:n + 1], fyd[n:n + 1], 0.5, mu='frame'), loss[n:n + 1])
    # the batch-wide means: the reference's scalar
    got = contextual.contextual_loss(fxd, fyd, 0.5, mu='batch')
    check('batch scalar', got, CR.head_stages(fx.double(), fy.double(), 0.5, 'batch')['cx_loss'].mean(),
          CR.head_stages(fx, fy, 0.5, 'batch')['cx_loss'].mean())
    assert tuple(got.shape) == ()


def test_scratch_is_linear_in_p_and_the_matrix_is_never_stored():
    """ia_cx_scratch_bytes holds the mean table and the per-row / per-column vectors; the operands x^, y^ ([N,P,Cpad] fp32 each) are the
    caller's tensors.  The scratch at P = 4096 is below 4 N P (Cpad + 8) bytes plus a constant, scratch and both operands together below
    twice that -- far below the 64 MB of one P x P fp32 matrix."""
    from invertavatar_amd import hipops
    _, step = tiles()
    n, c = 2, 256
    cpad = -(-c // step) * step
    b = [hipops.cx_scratch_bytes(n, c, p) for p in (1024, 2048, 4096)]
    assert b[2] - b[1] == 2 * (b[1] - b[0]) and b[1] > b[0]
    budget = 4 * n * 4096 * (cpad + 8) + 65536
    assert b[2] < budget
    assert b[2] + 2 * 4 * n * 4096 * cpad < 2 * budget < n * 4096 * 4096 * 4
    with pytest.raises(RuntimeError):
        hipops.cx_head(torch.zeros(1, 700, 2, 2, device='cuda'), torch.zeros(1, 700, 2, 2, device='cuda'))      # beyond the LDS block


# ------------------------------------------------------------------ end to end

_cache = {}


def model():
    if 'm' not in _cache:
        m = contextual.CXScore.synthetic(CR.MODEL_SEED)
        _cache['m'] = (m, CR.ReferenceCX(m.state_dict(), torch.float64), CR.ReferenceCX(m.state_dict(), torch.float32))
    return _cache['m']


def feats_positions(shape):
    h, w = (256, 256) if shape[2] > 256 else shape[1:]
    return (h // 4) * (w // 4)


@pytest.mark.parametrize('shape', [(2, 32, 32), (2, 64, 64), (1, 40, 300)])
@pytest.mark.parametrize('kind', ['float', 'uint8'])
def test_end_to_end(shape, kind):
    m, ref64, ref32 = model()
    x, y = CR.images(CR.FRAME_SEED + (shape[2] == 300), *shape)
    if kind == 'uint8':
        xd, yd = CR.to_uint8(x), CR.to_uint8(y)
        x, y = xd, yd
    else:
        xd, yd = x, y
    want, want32 = ref64.per_frame(x, y), ref32.per_frame(x, y)
    p = feats_positions(shape)
    assert 8.0 / p < float(want['cx'].min()) and float(want['cx'].max()) < 0.9        # unsaturated: far from 1, and from the floor 1 / P
    feats = contextual.features(torch.cat([xd, yd]).cuda(), m)
    check(f'{kind} {shape} relu3_4', feats, ref64.features(torch.cat([x, y])), ref32.features(torch.cat([x, y])), TRUNK_MULTIPLE)
    res = contextual.compare(xd.cuda(), yd.cuda(), m)
    assert res['cx'].is_cuda and res['cx'].dtype == torch.float32 and res['cx'].shape == (shape[0],)
    check(f'{kind} {shape} cx', res['cx'], want['cx'], want32['cx'], TRUNK_MULTIPLE)
    check(f'{kind} {shape} cx_loss', res['cx_loss'], want['cx_loss'], want32['cx_loss'], TRUNK_MULTIPLE)
    again = contextual.compare(xd.cuda(), yd.cuda(), m)
    assert torch.equal(again['cx'], res['cx']) and torch.equal(again['cx_loss'], res['cx_loss'])
    if shape[0] > 1:
        # a frame alone: the same definition, so the same bound (the head's bits do not depend on the batch, test_head_invariants_bit_for_bit;
        # the trunk's MFMA layers may be planned differently for another batch size)
        alone = contextual.compare(xd[1:].cuda(), yd[1:].cuda(), m)
        check(f'{kind} {shape} cx of frame 1 alone', alone['cx'], want['cx'][1:], want32['cx'][1:], TRUNK_MULTIPLE)
    check(f'{kind} {shape} forward', m(xd.cuda(), yd.cuda()), ref64.forward(x, y), ref32.forward(x, y), TRUNK_MULTIPLE)


def test_golden_forward_values_on_the_device():
    """The recorded float32 results of the reference's CXLoss.forward, within the end-to-end bound around the float64 restatement (the
    recorded value is itself a float32 run: it is allowed e32 of its own on top)."""
    g = np.load(GOLDEN)
    assert int(g['model_seed']) == CR.MODEL_SEED and int(g['frame_seed']) == CR.FRAME_SEED
    m, ref64, ref32 = model()
    x, y = CR.images(CR.FRAME_SEED, 2, 32, 32)
    xw, yw = CR.images(CR.FRAME_SEED + 1, 1, 40, 300)
    loss = contextual.CXLoss(m)
    for name, got, a, b, rec in (('batch', loss.forward(x.cuda(), y.cuda()), x, y, g['forward_batch']),
                                 ('wide', loss(xw.cuda(), yw.cuda()), xw, yw, g['forward_wide'])):
        w64, w32 = ref64.forward(a, b), ref32.forward(a, b)
        check(f'golden {name} vs float64', got, w64, w32, TRUNK_MULTIPLE)
        e32 = abs(float(w32) - float(w64))
        assert abs(float(got) - float(rec)) <= (TRUNK_MULTIPLE + 4) * e32 + 2 * EPS32 * abs(float(w64)), name
    each = contextual.compare(x.cuda(), y.cuda(), m)['cx_loss']
    w64, w32 = ref64.per_frame(x, y)['cx_loss'], ref32.per_frame(x, y)['cx_loss']
    check('golden each vs float64', each, w64, w32, TRUNK_MULTIPLE)
    e32 = (w32.double() - w64).abs().max().item()
    assert (each.double().cpu() - torch.from_numpy(g['forward_each']).double()).abs().max().item() <= (TRUNK_MULTIPLE + 4) * e32 + 2 * EPS32 * 2.0


def test_routes():
    """conv1_1 and conv1_2 (3 and 64 channels in, 64 out) are direct; conv2_1 .. conv3_4 are MFMA layers from 8^2 maps up."""
    def routes(h, w):
        return [r for r in lpips.plan_routes(contextual.PLAN, h, w) if r is not None]
    assert routes(64, 64) == ['direct'] * 2 + ['mfma'] * 6
    assert routes(256, 256) == ['direct'] * 2 + ['mfma'] * 6
    assert routes(32, 32) == ['direct'] * 2 + ['mfma'] * 6
    assert routes(16, 16) == ['direct'] * 2 + ['mfma'] * 2 + ['direct'] * 4        # conv3_x at 4^2: below the MFMA kernels' 8^2
    assert routes(4, 4) == ['direct'] * 8


def test_device_tensors_never_reach_torch_ops(monkeypatch):
    m, _, _ = model()
    x, y = CR.images(41, 2, 24, 300)
    want = contextual.compare(x.cuda(), y.cuda(), m)
    scalar = m(x.cuda(), y.cuda())

    def no_library(*a, **k):
        raise AssertionError('the device route must not reach torch convolutions, pools, interpolate, products, softmax or exp')
    for name in ('conv2d', 'max_pool2d', 'interpolate', 'softmax', 'normalize'):
        monkeypatch.setattr(torch.nn.functional, name, no_library)
    for name in ('conv2d', 'max_pool2d', 'bmm', 'matmul', 'softmax', 'exp', 'mm'):
        monkeypatch.setattr(torch, name, no_library)
    for name in ('bmm', 'matmul', 'softmax', 'exp', 'mm', '__matmul__'):
        monkeypatch.setattr(torch.Tensor, name, no_library)
    got = contextual.compare(x.cuda(), y.cuda(), m)
    assert torch.equal(got['cx'], want['cx']) and torch.equal(got['cx_loss'], want['cx_loss'])
    assert torch.equal(m(x.cuda(), y.cuda()), scalar)
    with pytest.raises(AssertionError):
        contextual.compare(x, y, m)                         # the CPU route is the torch restatement


def test_clip_metrics_returns_the_bits_of_compare():
    m, _, _ = model()
    x, y = CR.images(42, 2, 176, 176)
    clip = im.ClipMetrics(contextual=m)
    first = clip.update(x.cuda(), y.cuda())
    want = contextual.compare(x.cuda(), y.cuda(), m)
    assert first['cx'].is_cuda and torch.equal(first['cx'], want['cx']) and torch.equal(first['cx_loss'], want['cx_loss'])
    s = clip.summary()
    assert s['frames'] == 2 and s['per_frame']['cx'] == [float(v) for v in want['cx'].cpu()]
    assert set(s['mean']) == {'mse', 'l1', 'psnr', 'ssim', 'ms_ssim', 'cx', 'cx_loss'}
