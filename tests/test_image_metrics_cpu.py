"""Image metrics (invertavatar_amd/image_metrics.py) without a GPU: the float64 restatement against the recorded results of the
reference's criteria/ms_ssim.py, exact cases, batching, layouts, errors, ClipMetrics, the CLI and drive_sequence(metrics=...).

The inputs are generated here from seeds (NumPy only), so tests/golden/image_metrics.npz holds results only;
tests/golden/make_image_metrics_golden.py and the device tests import the generators from this file."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from invertavatar_amd import image_metrics as im

DISTORTIONS = ('noise002', 'noise02', 'blur3', 'shift2', 'gain', 'identity')
# fixture cases: name -> (seed, C, H, W); every case is scored against all DISTORTIONS (one frame each)
CASES = {'rgb512': (11, 3, 512, 512), 'rgb256': (12, 3, 256, 256), 'rgb200x333': (13, 3, 200, 333)}


def make_image(seed, c, h, w):
    """float32 [c,h,w] in [-1, 1]: three low-frequency sinusoids per channel + white texture, scaled so that max |v| = 1."""
    rs = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64) / h, np.arange(w, dtype=np.float64) / w, indexing='ij')
    img = np.zeros((c, h, w))
    for ch in range(c):
        for _ in range(3):
            fy, fx = rs.uniform(0.5, 4.0, 2)
            ph = rs.uniform(0.0, 2.0 * np.pi)
            img[ch] += rs.uniform(0.3, 1.0) * np.sin(2.0 * np.pi * (fy * y + fx * x) + ph)
    img += 0.35 * rs.randn(c, h, w)
    return (img / np.abs(img).max()).astype(np.float32)


def distort(img, kind, seed):
    rs = np.random.RandomState(seed + 1000)
    img = img.astype(np.float64)
    if kind == 'noise002':
        out = img + 0.02 * rs.randn(*img.shape)
    elif kind == 'noise02':
        out = img + 0.2 * rs.randn(*img.shape)
    elif kind == 'blur3':
        p = np.pad(img, ((0, 0), (1, 1), (1, 1)), mode='edge')
        h, w = img.shape[1:]
        out = sum(p[:, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0
    elif kind == 'shift2':
        out = np.roll(img, 2, axis=2)
    elif kind == 'gain':
        out = 0.8 * img + 0.05
    elif kind == 'identity':
        out = img
    else:
        raise KeyError(kind)
    return out.astype(np.float32)


def case_pair(name):
    """(a, b) float32 [6,C,H,W]: the clean image repeated, and its six distortions."""
    seed, c, h, w = CASES[name]
    img = make_image(seed, c, h, w)
    a = np.stack([img] * len(DISTORTIONS))
    b = np.stack([distort(img, kind, seed) for kind in DISTORTIONS])
    return torch.from_numpy(a), torch.from_numpy(b)


def to_uint8_nhwc(t):
    return ((t.double() + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope='module')
def gld(golden):
    return golden('image_metrics.npz')


@pytest.mark.parametrize('name', sorted(CASES))
def test_float64_restatement_matches_the_reference_results(gld, name):
    """Pins window, valid correlation, pooling, weights and per-frame means to the reference: its float32 results are within e_ref
    (their own recorded distance from this restatement) on every case."""
    a, b = case_pair(name)
    tab = im.reference_table(a, b, 2.0, 5)
    e_ssim, e_ms = gld['e_ref_ssim'], gld['e_ref_ms_ssim']
    assert 0.0 < e_ssim < 5e-6 and 0.0 < e_ms < 5e-6, (e_ssim, e_ms)          # a float32 evaluation's distance, not a definition's
    d_ssim = (tab[:, 5:10] - gld[f'{name}_ssim'].double()).abs().max().item()
    d_cs = (tab[:, 10:15] - gld[f'{name}_cs'].double()).abs().max().item()
    d_ms = (tab[:, 4] - gld[f'{name}_msssim'].double()).abs().max().item()
    d_auto = (tab[:, 4] - gld[f'{name}_msssim_auto'].double()).abs().max().item()
    print(f'{name}: |ssim - ref| {d_ssim:.2e}, |cs - ref| {d_cs:.2e}, |ms_ssim - ref| {d_ms:.2e} (auto range {d_auto:.2e}); e_ref {e_ssim:.2e} / {e_ms:.2e}')
    assert d_ssim <= e_ssim and d_cs <= e_ssim and d_ms <= e_ms and d_auto <= e_ms
    assert torch.isfinite(tab).all() or torch.isinf(tab[5, 2])                 # (identity: psnr = +inf)
    assert (tab[:, 10:15] > 0).all()                                           # MS-SSIM is finite on every case: nothing to mask
    res = im.compare(a, b)
    assert res['ms_ssim'].dtype == torch.float32 and torch.equal(res['ms_ssim'], tab[:, 4].float())
    assert torch.equal(res['ssim_levels'], tab[:, 5:10].float()) and torch.equal(res['ssim'], res['ssim_levels'][:, 0])


def test_identical_images_score_exactly_one():
    a, _ = case_pair('rgb256')
    res = im.compare(a[:2], a[:2].clone())
    assert (res['ssim'] == 1.0).all() and (res['ms_ssim'] == 1.0).all() and (res['ssim_levels'] == 1.0).all() and (res['cs_levels'] == 1.0).all()
    assert (res['mse'] == 0.0).all() and (res['l1'] == 0.0).all() and torch.isposinf(res['psnr']).all()


def test_known_answers_on_constant_images():
    a, b = torch.full((2, 3, 32, 40), 0.25), torch.full((2, 3, 32, 40), -0.25)
    b[1] = 0.0
    res = im.compare(a, b, levels=1)
    assert torch.allclose(res['mse'], torch.tensor([0.25, 0.0625]), rtol=1e-6, atol=0)
    assert torch.allclose(res['l1'], torch.tensor([0.5, 0.25]), rtol=1e-6, atol=0)
    assert torch.allclose(res['psnr'], torch.tensor([10 * math.log10(4 / 0.25), 10 * math.log10(4 / 0.0625)]), rtol=1e-6, atol=0)
    assert torch.isnan(res['ms_ssim']).all()                                   # fewer than five levels: no MS-SSIM
    # constant images: every variance is 0, cs = 1, ssim = (2 m1 m2 + C1) / (m1^2 + m2^2 + C1)
    c1 = (0.01 * 2.0) ** 2
    assert torch.allclose(res['cs_levels'][:, 0], torch.ones(2), rtol=1e-6, atol=0)
    assert torch.allclose(res['ssim'], torch.tensor([(-2 * 0.0625 + c1) / (2 * 0.0625 + c1), c1 / (0.0625 + c1)]), rtol=1e-5, atol=0)
    assert torch.equal(im.psnr(a, b), res['psnr']) and torch.equal(im.ssim(a, b), res['ssim'])
    ua, ub = torch.full((1, 32, 40, 3), 200, dtype=torch.uint8), torch.full((1, 32, 40, 3), 168, dtype=torch.uint8)     # data_range 255
    assert torch.allclose(im.psnr(ua, ub), torch.tensor([10 * math.log10(255.0 ** 2 / 32.0 ** 2)]), rtol=1e-6, atol=0)


def test_a_batch_equals_its_frames_one_by_one():
    a, b = case_pair('rgb200x333')
    whole = im.compare(a, b)
    for k in range(a.shape[0]):
        one = im.compare(a[k:k + 1], b[k:k + 1])
        for key in whole:
            assert torch.equal(one[key][0], whole[key][k]), (key, k)
    assert torch.equal(im.ms_ssim(a, b), whole['ms_ssim'])


def test_uint8_nhwc_equals_float_nchw_of_the_same_values():
    a, b = case_pair('rgb256')
    ua, ub = to_uint8_nhwc(a[:3]), to_uint8_nhwc(b[:3])
    fa, fb = ua.permute(0, 3, 1, 2).float().contiguous(), ub.permute(0, 3, 1, 2).float().contiguous()
    got, want = im.compare(ua, ub), im.compare(fa, fb, data_range=255.0)
    for key in got:
        assert torch.equal(got[key], want[key]), key
    assert torch.equal(im.compare(ua.numpy(), ub.numpy())['ssim'], got['ssim'])            # NumPy arrays take the same route


def test_errors_are_raised_before_any_computation():
    ok = torch.zeros(1, 3, 176, 176)
    with pytest.raises(ValueError, match='too small'):
        im.compare(torch.zeros(1, 3, 175, 300), torch.zeros(1, 3, 175, 300))            # 175 >> 4 = 10
    im.compare(ok, ok)                                                                   # 176 >> 4 = 11: the smallest five-level image
    with pytest.raises(ValueError, match='too small'):
        im.ssim(torch.zeros(1, 3, 10, 64), torch.zeros(1, 3, 10, 64))
    with pytest.raises(ValueError, match='same shape'):
        im.compare(ok, torch.zeros(1, 3, 176, 180))
    with pytest.raises(ValueError, match='float32'):
        im.compare(ok, ok.double())
    with pytest.raises(ValueError, match='float32'):
        im.compare(ok.half(), ok.half())
    with pytest.raises(ValueError, match='channels'):
        im.compare(torch.zeros(1, 5, 176, 176), torch.zeros(1, 5, 176, 176))
    with pytest.raises(ValueError, match='levels'):
        im.compare(ok, ok, levels=6)
    with pytest.raises(ValueError, match='different devices'):
        im.compare(ok, ok.to('meta'))


def test_clip_metrics_summary_and_json_round_trip(tmp_path):
    a, b = case_pair('rgb200x333')
    clip = im.ClipMetrics(levels=3)
    clip.update(a[:4], b[:4])
    clip.update(a[4:5], b[4:5])
    s = clip.summary()
    want = im.compare(a[:5], b[:5], levels=3)
    assert s['frames'] == 5 and s['levels'] == 3
    for key in ('mse', 'l1', 'psnr', 'ssim'):
        vals = [float(v) for v in want[key]]
        assert s['per_frame'][key] == vals and isinstance(s['mean'][key], float)
        assert s['min'][key] == min(vals) and s['max'][key] == max(vals) and s['mean'][key] == pytest.approx(sum(vals) / 5)
    assert s['per_frame']['cs_levels'] == [[float(v) for v in row] for row in want['cs_levels']]
    path = tmp_path / 'clip.json'
    clip.write_json(str(path))
    back = json.loads(path.read_text())
    assert back['per_frame']['ssim'] == s['per_frame']['ssim'] and back['frames'] == 5
    assert all(math.isnan(v) for v in back['per_frame']['ms_ssim'])               # three levels: no MS-SSIM
    with pytest.raises(ValueError):
        im.ClipMetrics().summary()


def test_cli_scores_two_stacks(tmp_path):
    a, b = case_pair('rgb200x333')
    np.save(tmp_path / 'pred.npy', b[:3].numpy())
    np.save(tmp_path / 'gt.npy', a[:3].numpy())
    out = tmp_path / 'metrics.json'
    repo = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
    r = subprocess.run([sys.executable, '-m', 'invertavatar_amd.image_metrics', '--pred', str(tmp_path / 'pred.npy'), '--gt', str(tmp_path / 'gt.npy'),
                        '--chunk', '2', '--device', 'cpu', '--out', str(out)], cwd=repo, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(out.read_text())
    want = im.compare(b[:3], a[:3])
    assert res['frames'] == 3 and res['per_frame']['ms_ssim'] == [float(v) for v in want['ms_ssim']]
    assert res['per_frame']['psnr'] == [float(v) for v in want['psnr']]
    # a directory of uint8 stacks, default data range 255
    for d, t in (('p', b), ('g', a)):
        os.makedirs(tmp_path / d)
        np.save(tmp_path / d / '000.npy', to_uint8_nhwc(t[:2]).numpy())
        np.save(tmp_path / d / '001.npy', to_uint8_nhwc(t[2:3]).numpy())
    assert im.main(['--pred', str(tmp_path / 'p'), '--gt', str(tmp_path / 'g'), '--device', 'cpu', '--out', str(out)]) == 0
    res8 = json.loads(out.read_text())
    assert res8['frames'] == 3 and res8['data_range'] == 255.0
    assert res8['per_frame']['ssim'] == [float(v) for v in im.compare(to_uint8_nhwc(b[:3]), to_uint8_nhwc(a[:3]))['ssim']]


def test_drive_sequence_with_metrics_on_the_cpu():
    """The small network of tests/encoder_common.py (512^2 images: five levels fit); two drive frames, one per call."""
    from encoder_common import build_inversion_net
    from invertavatar_amd import eval_seq, synthetic
    net = build_inversion_net('small')
    g = net.generator
    g.neural_rendering_resolution = 32
    frames = [40, 47]
    c, uv, jit = synthetic.camera_labels(frames), synthetic.uv_conditions(frames), synthetic.jitter(frames, 32 * 32).squeeze(-1)
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(3, 1), synthetic.conditioning_camera(), truncation_psi=0.7, truncation_cutoff=14)
        res = {'w': ws,
               'texture': g.texture_backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const'),
               'static': g.backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const')}
        plain, none = eval_seq.drive_sequence(net, ws, res, c, uv, jitter=jit)
        # ground truth = the frames themselves under two distortions (an unrelated picture can have a negative mean cs: NaN by definition)
        gt = torch.from_numpy(np.stack([distort(plain[0].numpy(), 'noise02', 21), distort(plain[1].numpy(), 'blur3', 22)]))
        clip = im.ClipMetrics()
        images, mosaics = eval_seq.drive_sequence(net, ws, res, c, uv, jitter=jit, gt=gt, metrics=clip)
    assert none is None and len(mosaics) == 2
    assert torch.equal(images, plain)
    s = clip.summary()
    want = im.compare(images, gt)
    assert s['frames'] == 2
    for key in ('mse', 'psnr', 'ssim', 'ms_ssim'):
        assert s['per_frame'][key] == [float(v) for v in want[key]], key
    # without gt there is nothing to score
    idle = im.ClipMetrics()
    eval_seq.drive_sequence(net, ws, res, c[:1], uv[:1], jitter=jit[:1], metrics=idle)
    with pytest.raises(ValueError):
        idle.summary()
