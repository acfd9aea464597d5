"""ia_render_rays / ia_render_rays_box / ia_importance_stage against the float64 restatement of tests/render_reference.py (whose
agreement with the fp32 oracle and the recorded fixture tests/test_render_reference_cpu.py establishes): at the edges of the domain of
the fp16 hi / lo pair decoder, beyond them, and at the launch shapes where the persistent launch takes another path.

Every call is checked as a chain of four links, each against a reference that does not depend on the kernel:

  (a) sigma_coarse            float64 density at the oracle's coarse depths
  (b) w_coarse                ``march_fp64`` of the float64 densities
  (c) inds, z_fine, order     ``oracle.renderer.sample_importance`` (the CPU fp32 bit rule the kernel copies) fed the KERNEL's w_coarse:
                              inds bit-equal, z_fine within 2e-6, order = the stable sort of cat(z_coarse, z_fine)
  (d) rgb, depth, wsum        ``render_fp64`` fed the KERNEL's z_fine

Tolerance of (a), (b), (d) per quantity: ``min(project bar, 4 x max|CPU fp32 oracle - fp64| + 2^-20 x propagated magnitude)``
(``Scene.tolerances``: computed from the CPU oracle and the float64 reference alone; it raises if the oracle itself is outside the bar).
Outputs and stage buffers are handed over pre-filled with NaN (-1 for the integer buffers) and none may be left; the same filling in guard
rows behind them must be left as it is."""
import numpy as np
import pytest
import torch

from oracle import renderer as OR
from invertavatar_amd import _lib, hipops
from conftest import max_abs
import render_reference as RR

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float('nan')


def _p(t):
    return None if t is None else t.data_ptr()


GUARD = 8          # rows behind every buffer: a workgroup's worth of rays


def _rows(n, width, fill, dtype=torch.float32):
    """(whole, view): ``n`` rows of ``width`` followed by GUARD rows, all filled; the launch gets the pointer of the whole buffer and
    must leave the guard rows as they are."""
    whole = torch.full((n + GUARD, width), fill, device='cuda', dtype=dtype)
    return whole, whole[:n]


def _tail(t, rows=GUARD):
    """An input [n, ...] with ``rows`` copies of its last row behind it (what a read past the end would meet): the whole buffer."""
    return torch.cat([t, t[-1:].expand(rows, *t.shape[1:])], 0).contiguous().cuda()


def launch(sc, debug=True, channel_major=False, split_planes=0, split_styles=None, may_be_nan=()):
    """One ia_render_rays (or ia_ray_limits_box + ia_render_rays_box) call on NaN-filled buffers: dict of host tensors rgb [B,R,32],
    depth, wsum [B,R,1], and with ``debug`` sigma_coarse [B,R,48], w_coarse [B,R,47], z_fine, inds [B,R,48], order [B,R,96].
    Every output and stage buffer has GUARD rows behind the B * R the launch is told of (the frame-major ones a whole frame), filled
    like the rest, and the launch may not touch them: a ray index that runs past the end is seen, not only one that stops short.  The
    inputs carry the same tail, so such an index reads nothing outside them.  ``may_be_nan``: outputs not checked for NaN."""
    lib, dev = _lib.load(), torch.device('cuda')
    b, r = sc.ro.shape[:2]
    n = b * r
    ph, pw = sc.planes.shape[-2:]
    planes = _tail(sc.planes.permute(0, 1, 3, 4, 2), 1)
    ro, rd, jit = _tail(sc.ro.reshape(n, 3)), _tail(sc.rd.reshape(n, 3)), _tail(sc.jitter.reshape(n, 48))
    w = [t.contiguous().cuda() for t in sc.weights]
    per_frame = sc.per_frame and b > 1
    guarded = {}                # name -> (whole buffer, the part the launch may write)
    if channel_major:
        whole = torch.full((b + 1, 32, r), NAN, device=dev)
        guarded['rgb'] = (whole, whole[:b])
    else:
        guarded['rgb'] = _rows(n, 32, NAN)
    guarded['depth'], guarded['wsum'] = _rows(n, 1, NAN), _rows(n, 1, NAN)
    grid = lib.ia_render_rays_grid(b, r)
    assert 0 < grid <= (n + 7) // 8
    slots = 2 * grid * (8 * b if per_frame else 1)
    scratch = torch.full((slots + 2 * (b + 1),), NAN, device=dev)
    if debug:
        guarded.update(z_fine=_rows(n, 48, NAN), inds=_rows(n, 48, -1, torch.int32), order=_rows(n, 96, -1, torch.int32),
                       w_coarse=_rows(n, 47, NAN), sigma_coarse=_rows(n, 48, NAN))
    dbg = [_p(guarded[k][0]) if k in guarded else None for k in ('z_fine', 'inds', 'order', 'w_coarse', 'sigma_coarse')]
    if split_planes:
        whole = torch.full((b + 1, split_planes, 4, r, 8), NAN, device=dev, dtype=torch.float16)
        guarded['split'] = (whole, whole[:b])
        split_styles = None if split_styles is None else _tail(split_styles, 1)
    split = guarded['split'][0] if split_planes else None
    rgb, depth, wsum = (guarded[k][0] for k in ('rgb', 'depth', 'wsum'))
    stream = _lib.stream_ptr(dev)
    if sc.box is None:
        dist = _tail(sc.dists(), 1)
        flags = int(sc.white_back) | (2 if channel_major else 0) | (4 if per_frame else 0)
        st = lib.ia_render_rays(_p(planes), _p(ro), _p(rd), _p(jit), None, _p(dist), *(_p(t) for t in w), float(sc.lr), float(sc.box_warp), flags,
                                b, r, ph, pw, 48, 48, _p(rgb), _p(depth), _p(wsum), _p(scratch), *dbg, _p(split), _p(split_styles),
                                int(split_planes or 2), stream)
        _lib.check(st, 'ia_render_rays')
    else:
        u = _tail(sc.box['u'].reshape(n, 48))
        guarded['limits'] = _rows(n, 2, NAN)
        limits = guarded['limits'][0]
        part = torch.empty(2 * lib.ia_ray_limits_box_parts(n), device=dev)
        _lib.check(lib.ia_ray_limits_box(_p(ro), _p(rd), float(sc.box_warp), n, 1, _p(limits), _p(part), stream), 'ia_ray_limits_box')
        limits[n:] = limits[n - 1]              # (an input of the render launch from here on: the tail of the other inputs)
        st = lib.ia_render_rays_box(_p(planes), _p(ro), _p(rd), _p(jit), _p(u), _p(limits), 0.0, 0.0, *(_p(t) for t in w), float(sc.lr),
                                    float(sc.box_warp), int(sc.white_back) | (8 if sc.flip_z else 0), b, r, ph, pw, 48, 48, _p(rgb), _p(depth),
                                    _p(wsum), _p(scratch), *dbg, stream)
        _lib.check(st, 'ia_render_rays_box')
    unwritten = lambda v: (v < 0) if v.dtype == torch.int32 else torch.isnan(v.float())
    out = {}
    for k, (whole, part_) in guarded.items():
        left = int(unwritten(part_).sum())
        assert left == 0 or k in may_be_nan, f'{k}: {left} of {part_.numel()} values unwritten or NaN'
        if k != 'limits':
            behind = whole[part_.shape[0]:]
            touched = int((~unwritten(behind)).sum())
            assert touched == 0, f'{k}: {touched} values written behind the {part_.shape[0]} rows of the call'
    # (the spare scratch sees only a write behind the LAST slot: with one dist per frame a wave one ray past the end writes the next wave's
    # slot, inside the buffer -- the guard rows of the outputs above are what catches that ray)
    assert int((~torch.isnan(scratch[slots:])).sum()) == 0, 'depth range scratch written behind its slots'
    shape = {'rgb': (b, r, 32), 'depth': (b, r, 1), 'wsum': (b, r, 1), 'limits': (b, r, 2)}
    for k, (whole, part_) in guarded.items():
        if k == 'rgb' and channel_major:
            out[k] = part_.permute(0, 2, 1)
        elif k == 'split':
            out[k] = part_
        else:
            out[k] = part_.reshape(*shape.get(k, (b, r, part_.shape[-1])))
    out['device_rgb'] = out['rgb']
    return {k: (v if k in ('device_rgb', 'split') else v.cpu()) for k, v in out.items()}


def check_importance(what, sc, got, z_coarse):
    """Link (c): from the kernel's own coarse weights."""
    b, r = z_coarse.shape[:2]
    z_f, inds = sc.sample_importance(got['w_coarse'])
    mism = int((got['inds'].reshape(-1, 48).long() != inds).sum())
    assert mism == 0, f'{what}: {mism} of {inds.numel()} searchsorted indices differ from sample_importance of the kernel\'s weights'
    d = max_abs(got['z_fine'], z_f.reshape(b, r, 48))
    assert d <= 2e-6, f'{what}: z_fine {d:.2e}'
    check_order(what, got['order'], z_coarse.reshape(b, r, 48), got['z_fine'])


def check_order(what, order, z_coarse, z_fine):
    z_all = torch.cat([z_coarse, z_fine], -1)
    want = torch.sort(z_all, dim=-1, stable=True)
    order = order.long()
    assert int(order.min()) >= 0 and int(order.max()) < 96
    # two merged depths exactly equal: any order of them is a stable merge of the two lists; compare the depths they gather
    assert torch.equal(torch.gather(z_all, -1, order), want.values), f'{what}: the merge order does not sort the depths'
    assert torch.equal(order.sort(dim=-1).values, torch.arange(96).expand_as(order)), f'{what}: the merge order is no permutation'


def check_chain(what, sc, got, tol=None):
    """Links (a) - (d); prints ``device / CPU / tol`` per quantity and returns {name: (device deviation, CPU deviation, tol)}."""
    tol = sc.tolerances() if tol is None else tol
    z_c = sc.z_coarse()
    b, r = z_c.shape[:2]
    coarse = sc.reference()                                            # (a), (b): the coarse pass does not depend on z_fine
    check_importance(what, sc, got, z_c)
    fine = sc.fp64(got['z_fine'].reshape(b, r, 48, 1), z_c)            # (d)
    devs = dict(sigma=max_abs(got['sigma_coarse'].reshape(b, r, 48, 1), coarse['den_coarse']),
                w_coarse=max_abs(got['w_coarse'].reshape(b, r, 47, 1), coarse['w_coarse']),
                rgb=max_abs(got['rgb'], fine['rgb']), depth=max_abs(got['depth'], fine['depth']), wsum=max_abs(got['wsum'], fine['wsum']))
    line = f'{what}: ' + '; '.join(f'{k} device {devs[k]:.2e} / CPU {tol[k][1]:.2e} / tol {tol[k][0]:.2e}' for k in devs)
    print(line + '  (max|. - fp64|)')
    for k in ('rgb', 'depth', 'wsum', 'sigma_coarse', 'w_coarse', 'z_fine'):
        assert torch.isfinite(got[k]).all(), f'{what}: {k} is not finite'
    assert all(devs[k] <= tol[k][0] for k in devs), line
    return {k: (devs[k], tol[k][1], tol[k][0]) for k in devs}


# ------------------------------------------------------------------ the domain of the fp16 pair decoder

@pytest.mark.parametrize('size', RR.SIZES)
@pytest.mark.parametrize('name', RR.DOMAIN_CASES)
def test_domain_case_vs_fp64(name, size):
    """In-domain scenes (B = 2, 64 rays per frame; ``render_reference.domain_case``): ordinary inputs; max |mean feature| = 240; max hidden
    pre-activation = 170 (softplus / ln 2 = 245); max staged |weight| = 15.5 in layer 1 (w0 gain log2 e) and in the colour rows of
    layer 2 (w1 gain: the kernel folds log2 e into layer 1 alone), through raw weights and lr_multiplier; features of 1e-4 without
    biases; a density of about 8e5, so high that the fp32 exp(-density * delta) is 0 on every coarse interval (alpha = 1: the first interval
    takes all the weight, interval k keeps the 1e-10 floor of the transmittance to the power k); rays that leave the planes, some of them
    exactly along a border."""
    sc, m = RR.domain_case(name, size)
    assert sc.planes.shape == (2, 3, 32, *size) and sc.ro.shape == (2, 64, 3)
    RR.check_targets(name, sc, m)
    check_chain(f'{name} {size[0]}x{size[1]}', sc, launch(sc))


# ------------------------------------------------------------------ out of the domain: pinned behaviour

@pytest.mark.parametrize('size', RR.SIZES)
def test_features_beyond_the_clamp_saturate(size):
    """Mean features in (253.9, 256] (StyleGAN's conv_clamp lets planes reach +-256): finite, and what the float64 pipeline gives on
    features clamped to +-65000 / 256 -- a defined saturation, within the tolerances of an in-domain scene."""
    sc, m = RR.domain_case('feature_over', size)
    RR.check_targets('feature_over', sc, m)
    assert sc.feature_clamp == RR.FEATURE_CLAMP
    share = float((m['ref']['parts']['feats_raw'].abs() > RR.FEATURE_CLAMP).double().mean())
    plain = RR._with(sc, feature_clamp=None)
    tol = plain.tolerances()                  # of the same inputs under the definition without the clamp: the oracle knows no clamp
    moved = max_abs(plain.reference()['den_coarse'], m['ref']['den_coarse'])
    print(f'features up to {m["feat"]:.2f}: {share:.2e} of the features beyond the clamp move sigma by {moved:.2e}')
    assert share > 0 and moved > 4 * tol['sigma'][0]          # the clamp is visible at this tolerance
    check_chain(f'features beyond the clamp {size[0]}x{size[1]}', sc, launch(sc), tol)


@pytest.mark.parametrize('size', RR.SIZES)
def test_hidden_units_beyond_the_split_range_stay_finite(size):
    """Hidden pre-activations up to 400 (softplus / ln 2 = 577 > 255, the range of an fp16 high part at 2^8): every output is finite;
    the deviation from float64 is printed (DESIGN 4.2 records it), not bounded: the density row reads the fp32 hidden units, the colour
    rows read pairs whose high part saturates at 65504 / 256 and whose low part then carries the rest with 11 bits."""
    sc, m = RR.domain_case('hidden_over', size)
    RR.check_targets('hidden_over', sc, m)
    got = launch(sc)
    z_c = sc.z_coarse()
    check_importance('hidden units beyond the range', sc, got, z_c)
    ref = sc.fp64(got['z_fine'].reshape(2, 64, 48, 1), z_c)
    coarse = sc.reference()
    scale = max(1.0, float(coarse['den_coarse'].abs().max()))
    devs = dict(sigma=max_abs(got['sigma_coarse'].reshape(2, 64, 48, 1), coarse['den_coarse']), w_coarse=max_abs(got['w_coarse'].reshape(2, 64, 47, 1), coarse['w_coarse']),
                rgb=max_abs(got['rgb'], ref['rgb']), depth=max_abs(got['depth'], ref['depth']), wsum=max_abs(got['wsum'], ref['wsum']))
    print(f'pre-activation up to {m["pre"]:.0f}, max|sigma| {scale:.0f} {size[0]}x{size[1]}: ' + '; '.join(f'{k} device {v:.2e}' for k, v in devs.items()) + '  (max|. - fp64|)')
    for k in ('rgb', 'depth', 'wsum', 'sigma_coarse', 'w_coarse', 'z_fine'):
        assert torch.isfinite(got[k]).all(), k
    # the density row does not go through the pairs: it keeps the relative bar
    assert devs['sigma'] <= RR.BARS['sigma'] * scale and devs['w_coarse'] <= RR.BARS['w_coarse']


def _wrapper_args(sc):
    b, r = sc.ro.shape[:2]
    return (hipops.planes_channels_last(sc.planes.cuda()), sc.ro.cuda().contiguous(), sc.rd.cuda().contiguous(),
            sc.jitter.reshape(b, r, 48).cuda().contiguous())


def test_what_the_raw_launch_makes_of_weights_beyond_the_split_range():
    """Why the wrappers refuse them: with ONE staged weight of 16 -- an fp16 infinity as a high part, minus infinity as its
    residual -- the launch itself reports nothing.  In a colour row every ray gets NaN in that channel; in layer 1 the NaN never shows:
    fmin / fmax of the base-2 softplus make a hidden unit of 126 of it, and the image is finite and wrong."""
    sc, _ = RR.domain_case('ordinary', (16, 16))
    w0, b0, w1, b1 = sc.weights
    w1_bad = w1.clone()
    w1_bad[5, 9] = 16.0 * 8.0                        # colour row 4: staged 16.0
    got = launch(RR._with(sc, weights=(w0, b0, w1_bad, b1)), may_be_nan=('rgb',))
    nan = torch.isnan(got['rgb'])
    print(f'one staged colour weight of 16: {int(nan.sum())} of {nan.numel()} rgb values are NaN')
    assert nan[..., 4].all() and not nan[..., :4].any() and not nan[..., 5:].any()
    assert torch.isfinite(got['depth']).all() and torch.isfinite(got['wsum']).all() and torch.isfinite(got['sigma_coarse']).all()
    w0_bad = w0.clone()
    w0_bad[7, 3] = 16.0 * np.sqrt(32.0) / np.log2(np.e) * 1.0001
    bad = RR._with(sc, weights=(w0_bad, b0, w1, b1))
    got = launch(bad)                                # no NaN anywhere
    ref = bad.reference()
    off = max_abs(got['sigma_coarse'].reshape(2, 64, 48, 1), ref['den_coarse'])
    print(f'one staged layer-1 weight of 16: finite, density {off:.2e} from fp64 (max |sigma| {float(ref["den_coarse"].abs().max()):.1f})')
    assert all(torch.isfinite(got[k]).all() for k in ('rgb', 'depth', 'wsum', 'sigma_coarse'))
    assert off > 1000 * RR.BARS['sigma'] * max(1.0, float(ref['den_coarse'].abs().max()))


@pytest.mark.parametrize('which', ['w0', 'w1'])
@pytest.mark.parametrize('lr', [1.0, 0.5])
def test_weights_beyond_the_split_range_are_refused(which, lr, monkeypatch):
    """A staged weight of 16 or more has no finite fp16 high part at 2^12: hipops.render_rays and hipops.render_rays_box raise a
    RuntimeError that names the bound; at 15.5 the same call goes through, and further calls with the same device tensors read nothing
    back (no per-frame synchronisation)."""
    reads = []
    real = hipops._render_weight_maxima
    monkeypatch.setattr(hipops, '_render_weight_maxima', lambda a, b: (reads.append(1), real(a, b))[1])
    monkeypatch.setattr(hipops, '_render_weight_checks', {})
    sc, _ = RR.domain_case(f'{which}_edge_lr{lr:g}', (16, 16))
    planes, ro, rd, jit = _wrapper_args(sc)
    dist = sc.dists().cuda()
    u = torch.from_numpy(np.random.RandomState(3).rand(2 * 64, 48).astype(np.float32)).sort(dim=-1).values.cuda()
    ok = [t.cuda() for t in sc.weights]
    rgb, depth, wsum = hipops.render_rays(planes, ro, rd, jit, dist, *ok, lr_multiplier=lr)
    assert torch.isfinite(rgb).all() and torch.isfinite(depth).all() and torch.isfinite(wsum).all()
    for _ in range(3):                  # as the generator calls it: detached views of the same parameters, every frame
        hipops.render_rays(planes, ro, rd, jit, dist, *(t.detach() for t in ok), lr_multiplier=lr)
        hipops.render_rays_box(planes, ro, rd, jit, u, *(t.detach() for t in ok), ray_start=2.25, ray_end=3.3, lr_multiplier=lr)
    assert len(reads) == 1, f'{len(reads)} device reads for one version of the weights'
    for factor in (16.0 / 15.5, 40.0):
        bad = [t.clone() for t in ok]
        if which == 'w0':
            bad[0] *= factor
            assert RR.scaled_weight_max(bad[0].cpu(), lr, 32, base2=True) >= 15.999
        else:
            bad[2][1:] *= factor
            assert RR.scaled_weight_max(bad[2][1:].cpu(), lr, 64) >= 15.999
        with pytest.raises(RuntimeError, match=r'15\.99'):
            hipops.render_rays(planes, ro, rd, jit, dist, *bad, lr_multiplier=lr)
        with pytest.raises(RuntimeError, match=r'15\.99'):
            hipops.render_rays_box(planes, ro, rd, jit, u, *bad, ray_start=2.25, ray_end=3.3, lr_multiplier=lr)
        # an in-place update of a checked tensor is seen (the cache is keyed by the tensor's version)
        good = ok[0].clone() if which == 'w0' else ok[2].clone()
        args = [good if i == (0 if which == 'w0' else 2) else t for i, t in enumerate(ok)]
        hipops.render_rays(planes, ro, rd, jit, dist, *args, lr_multiplier=lr)
        good.mul_(factor * 1.01)
        with pytest.raises(RuntimeError, match=r'15\.99'):
            hipops.render_rays(planes, ro, rd, jit, dist, *args, lr_multiplier=lr)


# ------------------------------------------------------------------ launch shapes

R_ODD = 1031


@pytest.fixture(scope='module')
def odd_scenes():
    """B = 3 frames x 1031 rays on a 16 x 16 plane, frames at different distances: one ``dist`` for the call, and one per frame."""
    out = {}
    for per_frame in (False, True):
        sc = RR.scene(70, [0, 3, 6], 8, (16, 16), rays=R_ODD, per_frame=per_frame)
        sc.ro = sc.ro * torch.tensor([1.0, 1.03, 0.97])[:, None, None]
        sc.planes[1] *= 0.02             # a nearly empty frame: many of its rays clamp to the range limits
        out[per_frame] = sc
    return out


@pytest.fixture(scope='module')
def odd_runs(odd_scenes):
    return {k: launch(sc) for k, sc in odd_scenes.items()}


@pytest.mark.parametrize('per_frame', [False, True])
def test_odd_batch_vs_fp64(odd_scenes, odd_runs, per_frame):
    """3093 rays: workgroups whose eight waves straddle two frames (1031 is no multiple of 8), a last workgroup of 5 rays, and a second
    grid-stride trip; with per-frame ``dist`` the waves change frame mid-run and the depth clamp is each frame's own range."""
    sc = odd_scenes[per_frame]
    grid = _lib.load().ia_render_rays_grid(3, R_ODD)
    assert 3 * R_ODD > 8 * grid and (3 * R_ODD) % 8 == 5 and R_ODD % 8 != 0
    check_chain(f'B=3 R={R_ODD} per-frame dist={per_frame}', sc, odd_runs[per_frame])
    if per_frame:
        d = odd_runs[True]['depth']
        assert not torch.equal(d[1].clamp(d[0].min(), d[0].max()), d[1])          # the frames' ranges really differ


@pytest.mark.parametrize('per_frame', [False, True])
def test_odd_batch_equals_one_call_per_frame(odd_scenes, odd_runs, per_frame):
    """Bit for bit: colours and weight sums always (with one ``dist`` the frames are rendered with the batch's ``dist``), and with
    per-frame ``dist`` the depth image too."""
    sc, batch = odd_scenes[per_frame], odd_runs[per_frame]
    for k in range(3):
        one = sc.frame(k)
        if not per_frame:
            one.dists = lambda: sc.dists()                                          # the batch's mean distance
        got = launch(one, debug=False)
        assert torch.equal(batch['rgb'][k:k + 1], got['rgb']) and torch.equal(batch['wsum'][k:k + 1], got['wsum']), k
        if per_frame:
            assert torch.equal(batch['depth'][k:k + 1], got['depth']), f'frame {k}: depth clamp range differs from the one-frame call'


@pytest.mark.parametrize('r', [1, 7, 9])
def test_few_rays(r):
    sc = RR.scene(71, [5], 8, (16, 16), rays=r)
    assert sc.ro.shape == (1, r, 3)
    check_chain(f'B=1 R={r}', sc, launch(sc))


def test_channel_major_at_an_odd_ray_count(odd_scenes, odd_runs):
    got = launch(odd_scenes[False], debug=False, channel_major=True)
    assert all(torch.equal(got[k], odd_runs[False][k]) for k in ('rgb', 'depth', 'wsum'))


@pytest.mark.parametrize('planes_out', [1, 2])
def test_split_copy_at_an_odd_ray_count(odd_scenes, odd_runs, planes_out):
    """The second copy of the composited features in the consumer's fp16 format equals ia_act_split of the fp32 image of the same launch."""
    styles = torch.rand(3, 32, device='cuda', generator=torch.Generator(device='cuda').manual_seed(4)) + 0.5
    got = launch(odd_scenes[False], debug=False, channel_major=True, split_planes=planes_out, split_styles=styles)
    assert torch.equal(got['rgb'], odd_runs[False]['rgb'])
    image = got['device_rgb'].permute(0, 2, 1).reshape(3, 32, 1, R_ODD).contiguous()
    want = hipops.act_split(image, styles, planes=planes_out)
    assert torch.equal(got['split'].reshape(want.data.shape), want.data)


@pytest.mark.parametrize('flip_z', [False, True])
def test_box_route_at_an_odd_ray_count(flip_z):
    """ia_ray_limits_box(repair_misses) + ia_render_rays_box, B = 2 x 1031 rays of which a good part misses the cube."""
    box_warp = 0.5
    u = torch.from_numpy(np.random.RandomState(9).rand(2 * R_ODD, 48).astype(np.float32)).sort(dim=-1).values
    sc = RR.scene(72, [0, 3], 8, (16, 16), rays=R_ODD, box_warp=box_warp, box=dict(u=u, flip_z=flip_z))
    t0, t1 = OR.ray_limits_box(sc.ro, sc.rd, box_warp)
    missing = float((t1 <= t0).float().mean())
    print(f'box route: {missing:.1%} of the rays miss the cube')
    assert 0.10 <= missing <= 0.50
    got = launch(sc)
    z_c = sc.z_coarse()
    lim = got['limits']
    valid = t1 > t0
    assert torch.equal(lim[..., :1][valid], t0[valid]) and torch.equal(lim[..., 1:][valid], t1[valid])
    assert (lim[..., :1][~valid] == t0[valid].min()).all() and (lim[..., 1:][~valid] == t0[valid].max()).all()
    o = sc.oracle()
    assert max_abs(got['rgb'], o['rgb']) <= 5e-5 and max_abs(got['w_coarse'].reshape(o['w_coarse'].shape), o['w_coarse']) <= 2e-5
    check_chain(f'box route B=2 R={R_ODD} flip_z={flip_z}', sc, got)


# ------------------------------------------------------------------ the importance stage alone

def _weight_rows():
    rs = np.random.RandomState(11)
    rows = [np.zeros(47), np.full(47, 1.0 / 47), np.eye(47)[10], 0.5 ** np.arange(47), 0.9 ** np.arange(47) * 0.1]
    rows += [np.eye(47)[k] * 0.7 for k in (0, 23, 46)]
    for _ in range(200):                      # sparse: a few intervals carry everything
        row = np.zeros(47)
        idx = rs.choice(47, size=rs.randint(1, 5), replace=False)
        row[idx] = rs.rand(idx.size) ** 3
        rows.append(row / max(row.sum(), 1.0))
    return np.stack(rows).astype(np.float32)


def test_importance_stage_alone():
    """4099 rows (more than the launch's 4096 workgroups, a multiple of nothing): all-zero, one-hot at the first, middle and last interval,
    uniform, a single 1.0, geometric decay and 200 seeded sparse weight rows, on depth rows without jitter, with the largest jitter
    below 1 and with random jitter."""
    n = 4099
    rows = _weight_rows()
    w = torch.from_numpy(rows[np.arange(n) % rows.shape[0]])
    rs = np.random.RandomState(12)
    jit = torch.from_numpy(rs.rand(1, n, 48, 1).astype(np.float32))
    kind = torch.arange(n) % 3
    jit[0, kind == 0] = 0.0
    jit[0, kind == 1] = float(np.float32(1.0) - np.float32(2.0 ** -24))
    assert float(jit.max()) < 1.0
    ro = torch.zeros(1, n, 3)
    ro[..., 2] = 2.7
    z = OR.coarse_depths(ro, 48, jit)[0]
    assert (z[:, :, 1:] >= z[:, :, :-1]).all()
    z_fine = torch.full((n, 48), NAN, device='cuda')
    inds = torch.full((n, 48), -1, device='cuda', dtype=torch.int32)
    order = torch.full((n, 96), -1, device='cuda', dtype=torch.int32)
    zc, wc = z.reshape(n, 48).contiguous().cuda(), w.contiguous().cuda()
    st = _lib.load().ia_importance_stage(_p(zc), _p(wc), _p(z_fine), _p(inds), _p(order), n, _lib.stream_ptr(zc.device))
    _lib.check(st, 'ia_importance_stage')
    assert not torch.isnan(z_fine).any() and int(inds.min()) >= 0 and int(order.min()) >= 0
    ref_z, ibuf = OR.sample_importance(z, w.reshape(1, n, 47, 1), 48)
    mism = int((inds.cpu().long() != ibuf['inds']).sum())
    assert mism == 0, f'{mism} of {inds.numel()} searchsorted indices differ'
    assert max_abs(z_fine.cpu(), ref_z.reshape(n, 48)) <= 2e-6
    check_order('importance stage', order.cpu(), z.reshape(n, 48), z_fine.cpu())
    wrapped = hipops.importance_stage(zc, wc)
    assert torch.equal(wrapped[0], z_fine) and torch.equal(wrapped[1], inds) and torch.equal(wrapped[2], order)
