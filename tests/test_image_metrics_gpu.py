"""Image metrics on the device (csrc/image_metrics.hip) against the float64 restatement of invertavatar_amd/image_metrics.py.

Bounds.  ssim / cs per level and ms_ssim: 4 x e_ref, where e_ref (tests/golden/image_metrics.npz) is the distance of the reference's
own float32 evaluation from the float64 restatement on the fixture cases: the device result is a float32 computation like the
reference's with another summation order (separable taps, tile partials), and a small multiple of the reference's own distance from
exact is what a reordering can cost.  mse / l1: relative distance from float64 within 4 x that of torch's float32
``((a-b)**2).mean()`` / ``(a-b).abs().mean()`` on the same inputs (the larger of the batch's frames on both sides)."""
import ctypes

import numpy as np
import pytest
import torch

from invertavatar_amd import image_metrics as im
from test_image_metrics_cpu import CASES, DISTORTIONS, case_pair, distort, make_image, to_uint8_nhwc

pytestmark = pytest.mark.gpu


def _batch(seed, n, c, h, w):
    """n different images against distortions of them (cycling through DISTORTIONS)."""
    a = np.stack([make_image(seed + k, c, h, w) for k in range(n)])
    b = np.stack([distort(a[k], DISTORTIONS[k % len(DISTORTIONS)], seed + k) for k in range(n)])
    return torch.from_numpy(a), torch.from_numpy(b)


def _inputs(name):
    if name in CASES:
        return case_pair(name)
    if name == 'batch8_rgb512':
        return _batch(31, 8, 3, 512, 512)
    if name == 'gray_c1':
        return _batch(41, 3, 1, 256, 320)
    if name == 'rgba_c4':
        return _batch(51, 3, 4, 200, 333)
    if name == 'uint8_rgb':
        a, b = _batch(61, 6, 3, 333, 200)
        return to_uint8_nhwc(a), to_uint8_nhwc(b)
    raise KeyError(name)


@pytest.mark.parametrize('name', sorted(CASES) + ['batch8_rgb512', 'gray_c1', 'rgba_c4', 'uint8_rgb'])
def test_device_matches_the_float64_restatement(golden, name):
    gld = golden('image_metrics.npz')
    e_ssim, e_ms = gld['e_ref_ssim'], gld['e_ref_ms_ssim']
    a, b = _inputs(name)
    L = 255.0 if a.dtype == torch.uint8 else 2.0
    want = im.reference_table(a, b, L, 5)                                     # float64, on the CPU
    assert torch.isfinite(want[:, 3:]).all() and (want[:, 10:15] > 0).all()       # no NaN case to mask
    got = im.compare(a.cuda(), b.cuda())
    assert got['ssim'].is_cuda and got['ssim'].dtype == torch.float32
    d_ssim = (got['ssim_levels'].cpu().double() - want[:, 5:10]).abs().max().item()
    d_cs = (got['cs_levels'].cpu().double() - want[:, 10:15]).abs().max().item()
    d_ms = (got['ms_ssim'].cpu().double() - want[:, 4]).abs().max().item()
    fa, fb = (a.permute(0, 3, 1, 2).float(), b.permute(0, 3, 1, 2).float()) if a.dtype == torch.uint8 else (a, b)
    rel = lambda x, ref: ((x.double() - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()  # noqa: E731
    nz = want[:, 0] > 0                                                       # (identity frames: exactly 0 on both sides, checked below)
    r_mse, r_l1 = rel(got['mse'].cpu()[nz], want[nz, 0]), rel(got['l1'].cpu()[nz], want[nz, 1])
    t_mse, t_l1 = rel(((fa - fb) ** 2).mean(dim=(1, 2, 3))[nz], want[nz, 0]), rel((fa - fb).abs().mean(dim=(1, 2, 3))[nz], want[nz, 1])
    d_psnr = (got['psnr'].cpu().double()[nz] - want[nz, 2]).abs().max().item()
    print(f'{name}: |ssim| {d_ssim:.2e} |cs| {d_cs:.2e} (bound {4 * e_ssim:.2e}), |ms_ssim| {d_ms:.2e} (bound {4 * e_ms:.2e}), '
          f'mse rel {r_mse:.2e} (torch fp32 {t_mse:.2e}), l1 rel {r_l1:.2e} (torch fp32 {t_l1:.2e}), |psnr| {d_psnr:.2e} dB')
    assert d_ssim <= 4 * e_ssim and d_cs <= 4 * e_ssim
    assert d_ms <= 4 * e_ms
    assert r_mse <= 4 * t_mse and r_l1 <= 4 * t_l1
    assert (got['mse'].cpu()[~nz] == 0).all() and torch.isposinf(got['psnr'].cpu()[~nz]).all()
    assert torch.equal(got['ssim'], got['ssim_levels'][:, 0])
    # fewer levels: the same leading levels, and no MS-SSIM
    part = im.compare(a.cuda(), b.cuda(), levels=2)
    assert torch.equal(part['ssim_levels'], got['ssim_levels'][:, :2]) and torch.equal(part['cs_levels'], got['cs_levels'][:, :2])
    assert torch.isnan(part['ms_ssim']).all() and torch.equal(part['mse'], got['mse'])


def _table(res):
    return torch.cat([res[k].reshape(res[k].shape[0], -1) for k in res], 1)


def test_bit_equal_run_to_run_batch_to_single_and_across_streams():
    a, b = _batch(31, 8, 3, 512, 512)
    a, b = a.cuda(), b.cuda()
    first = _table(im.compare(a, b))
    # (identity frames hold +inf psnr: compare the bits)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    assert torch.equal(bits(first), bits(_table(im.compare(a, b))))
    singles = torch.cat([_table(im.compare(a[k:k + 1], b[k:k + 1])) for k in range(8)])
    assert torch.equal(bits(first), bits(singles))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _table(im.compare(a, b))
    side.synchronize()
    assert torch.equal(bits(first), bits(other))
    ua, ub = to_uint8_nhwc(a.cpu()).cuda(), to_uint8_nhwc(b.cpu()).cuda()
    u_all = _table(im.compare(ua, ub))
    u_one = torch.cat([_table(im.compare(ua[k:k + 1], ub[k:k + 1])) for k in range(8)])
    assert torch.equal(bits(u_all), bits(u_one))


@pytest.mark.parametrize('shape', [(2, 3, 512, 512), (1, 4, 200, 333), (2, 1, 176, 177)])
def test_identical_images_score_exactly_one_on_the_device(shape):
    a = torch.from_numpy(np.stack([make_image(70 + k, *shape[1:]) for k in range(shape[0])])).cuda()
    for x, y in ((a, a.clone()), (to_uint8_nhwc(a.cpu()).cuda(), to_uint8_nhwc(a.cpu()).cuda())):
        res = im.compare(x, y)
        assert (res['ssim'] == 1.0).all() and (res['ms_ssim'] == 1.0).all()
        assert (res['ssim_levels'] == 1.0).all() and (res['cs_levels'] == 1.0).all()
        assert (res['mse'] == 0.0).all() and (res['l1'] == 0.0).all() and torch.isposinf(res['psnr']).all()
    assert (im.ssim(a, a) == 1.0).all() and torch.isposinf(im.psnr(a, a)).all() and (im.ms_ssim(a, a) == 1.0).all()


def test_abi_error_paths_are_rejected_on_the_host():
    from invertavatar_amd import _lib
    lib = _lib.load()
    n, c, h, w = 1, 3, 176, 176
    a = torch.zeros(n, c, h, w, device='cuda')
    nbytes = ctypes.c_size_t(0)
    assert lib.ia_image_metrics_scratch_bytes(n, c, h, w, 5, ctypes.byref(nbytes)) == 0 and nbytes.value > 0
    scratch = torch.empty(nbytes.value // 8 + 1, dtype=torch.float64, device='cuda')
    out = torch.full((n, 15), -7.0, device='cuda')
    s = _lib.stream_ptr('cuda')

    def call(pa=a.data_ptr(), pb=a.data_ptr(), layout=0, c=c, h=h, w=w, levels=5, ps=scratch.data_ptr(), sbytes=scratch.numel() * 8,
             po=out.data_ptr()):
        return lib.ia_image_metrics(pa, pb, layout, n, c, h, w, 2.0, levels, ps, sbytes, po, s)
    for kwargs, text in (({'pa': None}, 'null'), ({'pb': None}, 'null'), ({'ps': None}, 'null'), ({'po': None}, 'null'),
                         ({'c': 0}, 'c must be in 1..4'), ({'c': 5}, 'c must be in 1..4'), ({'h': 175}, 'too small'), ({'w': 100}, 'too small'),
                         ({'sbytes': nbytes.value - 8}, 'scratch too small'), ({'levels': 0}, 'levels must be in 1..5'),
                         ({'levels': 6}, 'levels must be in 1..5'), ({'layout': 2}, 'unknown layout')):
        assert call(**kwargs) == -1, kwargs
        assert text in _lib.last_error(), (kwargs, _lib.last_error())
    assert lib.ia_image_metrics_scratch_bytes(n, 5, h, w, 5, ctypes.byref(nbytes)) == -1 and 'c must be in 1..4' in _lib.last_error()
    assert lib.ia_image_metrics_scratch_bytes(n, c, h, w, 5, None) == -1 and 'null' in _lib.last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                                # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert (out[:, 3] == 1.0).all()
    # Python refuses the same things before the C call
    with pytest.raises(ValueError, match='too small'):
        im.compare(a[:, :, :175], a[:, :, :175])
    with pytest.raises(ValueError, match='different devices'):
        im.compare(a, a.cpu())
    with pytest.raises(ValueError, match='channels'):
        im.compare(torch.zeros(1, 5, 176, 176, device='cuda'), torch.zeros(1, 5, 176, 176, device='cuda'))


def test_drive_sequence_scores_the_clip_on_the_device():
    """8 + 8 + 1 frames: two captured calls of 8 and the one-frame remainder call; 512^2 images take five levels."""
    from encoder_common import build_inversion_net
    from invertavatar_amd import _runtime, eval_seq, synthetic
    net = build_inversion_net('small').cuda()
    g = net.generator
    nrr = 32
    g.neural_rendering_resolution = nrr
    frames = list(range(40, 57))
    c, uv = synthetic.camera_labels(frames).cuda(), synthetic.uv_conditions(frames).cuda()
    jit = synthetic.jitter(frames, nrr * nrr).squeeze(-1).cuda()
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(3, 1).cuda(), synthetic.conditioning_camera().cuda(), truncation_psi=0.7, truncation_cutoff=14)
        res = {'w': ws,
               'texture': g.texture_backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const'),
               'static': g.backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const')}
        first, _ = eval_seq.drive_sequence(net, ws, res, c, uv, jitter=jit)
        # ground truth = the frames themselves, distorted (an unrelated picture can have a negative mean cs: NaN by definition)
        gt = torch.from_numpy(np.stack([distort(f.numpy(), DISTORTIONS[k % 5], 100 + k) for k, f in enumerate(first.cpu())])).cuda()
        plain, mos0 = eval_seq.drive_sequence(net, ws, res, c, uv, jitter=jit, gt=gt)
        assert torch.equal(plain, first)
        keys = set(_runtime.state(net).drive_graphs)
        assert sorted(k[0] for k in keys) == [1, 8]                           # the captured batch-8 call and the one-frame call both ran
        clip = im.ClipMetrics()
        images, mos1 = eval_seq.drive_sequence(net, ws, res, c, uv, jitter=jit, gt=gt, metrics=clip)
        assert set(_runtime.state(net).drive_graphs) == keys
        assert torch.equal(images, plain) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(mos0, mos1))
        want = im.compare(images, gt)
        s = clip.summary()
        assert s['frames'] == 17
        for key in ('mse', 'l1', 'psnr', 'ssim', 'ms_ssim'):
            assert s['per_frame'][key] == [float(v) for v in want[key].cpu()], key
        assert s['per_frame']['cs_levels'] == [[float(v) for v in row] for row in want['cs_levels'].cpu()]
        # the eager path (graphed=False) scores the same way
        eager = im.ClipMetrics()
        img_e, _ = eval_seq.drive_sequence(net, ws, res, c[:2], uv[:2], jitter=jit[:2], gt=gt[:2], graphed=False, metrics=eager)
        assert eager.summary()['per_frame']['ssim'] == [float(v) for v in im.compare(img_e, gt[:2])['ssim'].cpu()]
