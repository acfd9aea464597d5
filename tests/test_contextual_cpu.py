"""The contextual loss off the device: the float64 restatement against the recorded results of the reference's CXLoss
(tests/golden/contextual.npz, made by tests/golden/make_contextual_golden.py) and against the independent statement of
tests/contextual_reference.py, the per-frame / batch-wide means, the refusals, weight loading, ClipMetrics and the CLI."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from invertavatar_amd import contextual
from invertavatar_amd import image_metrics as im

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contextual_reference as CR  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS32 = 2.0 ** -23
_cache = {}


def model():
    if 'model' not in _cache:
        _cache['model'] = contextual.CXScore.synthetic(CR.MODEL_SEED)
    return _cache['model']


def refs():
    if 'refs' not in _cache:
        sd = model().state_dict()
        _cache['refs'] = (CR.ReferenceCX(sd, torch.float64), CR.ReferenceCX(sd, torch.float32))
    return _cache['refs']


def golden():
    g = np.load(os.path.join(GOLDEN, 'contextual.npz'))
    assert int(g['model_seed']) == CR.MODEL_SEED and int(g['frame_seed']) == CR.FRAME_SEED and int(g['feature_seed']) == CR.FEATURE_SEED
    return g


def check(name, recorded, f64, f32):
    """|float64 restatement - the reference's float32 run| <= 4 e32 + eps32 * scale, e32 the restatement's own float32-vs-float64 distance
    (the tolerance of tests/test_identity_cpu.py for its golden file)."""
    recorded, f64, f32 = torch.as_tensor(recorded).double(), torch.as_tensor(f64).double(), torch.as_tensor(f32).double()
    assert recorded.shape == f64.shape, (name, recorded.shape, f64.shape)
    e32 = (f32 - f64).abs().max().item()
    err = (recorded - f64).abs().max().item()
    bound = 4 * e32 + EPS32 * f64.abs().max().item()
    print(f'{name}: err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}')
    assert err <= bound, f'{name}: {err:.3e} > {bound:.3e}'


def test_head_restatement_matches_the_recorded_reference():
    g = golden()
    fx, fy = CR.relu_maps(CR.FEATURE_SEED, 2, 20, 5, 7)
    cx64, loss64, d64 = contextual.reference_head(fx.double(), fy.double(), 0.5, 'batch', debug=True)
    cx32, loss32, d32 = contextual.reference_head(fx, fy, 0.5, 'batch', debug=True)

    def stages(d):
        dist = 1 - torch.bmm(d['xh'], d['yh'].transpose(1, 2))
        tilde = torch.clamp(dist / (d['m'][:, :, None] + 1e-5), min=-10.0, max=10.0)
        w = torch.exp((1 - tilde) / 0.5)
        return dist, tilde, w / d['s'][:, :, None]
    for name, a, b in zip(('dist', 'tilde', 'cxm'), stages(d64), stages(d32)):
        check(name, g[name], a, b)
    check('contextual_loss', g['head_loss'], loss64.mean(), loss32.mean())
    assert torch.equal(contextual.contextual_loss(fx, fy, 0.5), loss64.mean().float())
    assert torch.equal(contextual.contextual_loss(fx, fy, 0.5, mu='frame'),
                       contextual.reference_head(fx.double(), fy.double(), 0.5, 'frame')[1].float())
    # against the independent statement, stage by stage
    for mu in ('batch', 'frame'):
        want = CR.head_stages(fx.double(), fy.double(), 0.5, mu)
        got = contextual.reference_head(fx.double(), fy.double(), 0.5, mu, debug=True)
        for key in ('mu', 'xh', 'yh', 'm', 's', 'colmax'):
            assert (got[2][key] - want[key]).abs().max().item() <= 1e-12 * max(want[key].abs().max().item(), 1.0), (mu, key)
        assert (got[0] - want['cx']).abs().max().item() <= 1e-13 and (got[1] - want['cx_loss']).abs().max().item() <= 1e-12


def test_forward_matches_the_recorded_reference_and_the_independent_statement():
    g = golden()
    r64, r32 = refs()
    x, y = CR.images(CR.FRAME_SEED, 2, 32, 32)
    xw, yw = CR.images(CR.FRAME_SEED + 1, 1, 40, 300)
    check('forward_batch', g['forward_batch'], r64.forward(x, y), r32.forward(x, y))
    check('forward_each', g['forward_each'], r64.per_frame(x, y)['cx_loss'], r32.per_frame(x, y)['cx_loss'])
    check('forward_wide', g['forward_wide'], r64.forward(xw, yw), r32.forward(xw, yw))
    assert 0.01 < float(r64.per_frame(x, y)['cx'].min()) and float(r64.per_frame(x, y)['cx'].max()) < 0.9       # unsaturated scores
    m = model()
    # model(x, y) is the batch scalar; compare is per frame
    check('model(x, y)', g['forward_batch'], m(x, y).double(), r32.forward(x, y))
    assert abs(float(m(x, y)) - float(r64.forward(x, y))) <= 1e-6
    res = contextual.compare(x, y, m)
    assert res['cx'].dtype == torch.float32 and set(res) == set(contextual.KEYS)
    want = r64.per_frame(x, y)
    assert (res['cx'].double() - want['cx']).abs().max().item() <= 1e-7 and (res['cx_loss'].double() - want['cx_loss']).abs().max().item() <= 1e-6
    ref = contextual.reference_compare(x, y, m)
    assert torch.equal(ref['cx'], res['cx']) and torch.equal(ref['cx_loss'], res['cx_loss'])
    assert (contextual.reference_features(torch.cat([xw, yw]), m) - r64.features(torch.cat([xw, yw]))).abs().max().item() <= 1e-12
    assert contextual.features(xw, m).shape == (1, 256, 64, 64) and contextual.features(x, m).shape == (2, 256, 8, 8)
    # mu='frame' at N = 2 is two N = 1 calls; the batch scalar is not their mean
    for i in range(2):
        one = contextual.compare(x[i:i + 1], y[i:i + 1], m)
        assert torch.equal(one['cx'], res['cx'][i:i + 1]) and torch.equal(one['cx_loss'], res['cx_loss'][i:i + 1])
        assert abs(float(m(x[i:i + 1], y[i:i + 1])) - float(res['cx_loss'][i])) <= 1e-6
    assert abs(float(m(x, y)) - float(res['cx_loss'].mean())) > 1e-4
    loss = contextual.CXLoss(m)
    assert torch.equal(loss.forward(x, y), m(x, y)) and torch.equal(loss(x, y), m(x, y)) and loss.band_width == 0.5
    # NumPy arrays and uint8
    res_np = contextual.compare(x.numpy(), y.numpy(), m)
    assert torch.equal(res_np['cx'], res['cx'])
    xu, yu = CR.to_uint8(x), CR.to_uint8(y)
    ru = contextual.compare(xu, yu, m)
    wu = r64.per_frame(xu, yu)
    assert (ru['cx'].double() - wu['cx']).abs().max().item() <= 1e-7


def test_identical_frames_and_the_width_only_rule():
    m = model()
    x, _ = CR.images(5, 2, 24, 20)
    res = contextual.compare(x, x.clone(), m)
    assert (res['cx_loss'].double() + math.log1p(1e-5)).abs().max().item() <= 1e-7 and bool((res['cx_loss'] < 0).all())
    # the reference tests shape[-1] only: a tall narrow frame is not resized, a wide flat one is
    assert contextual.reference_front(torch.zeros(1, 3, 300, 40)).shape == (1, 3, 300, 40)
    assert contextual.reference_front(torch.zeros(1, 3, 40, 300)).shape == (1, 3, 256, 256)
    assert contextual.reference_front(torch.zeros(1, 300, 40, 3, dtype=torch.uint8)).shape == (1, 3, 300, 40)


def test_refusals():
    m = model()
    x = torch.zeros(1, 3, 16, 16)
    for bad, match in (((x * 3.0, x, m, 255.0), 'data_range'), ((x, x, m, 1.0), 'data_range'),
                       ((x, torch.zeros(1, 3, 16, 20), m, None), 'same shape'),
                       ((torch.zeros(1, 3, 3, 16), torch.zeros(1, 3, 3, 16), m, None), 'too small'),
                       ((torch.zeros(1, 16, 3, 3, dtype=torch.uint8), torch.zeros(1, 16, 3, 3, dtype=torch.uint8), m, None), 'too small'),
                       ((torch.zeros(1, 4, 16, 16), torch.zeros(1, 4, 16, 16), m, None), '3 channels'),
                       ((x.double(), x.double(), m, None), 'float32'), ((x, x.to(torch.uint8), m, None), 'both'),
                       ((x, x, object(), None), 'CXScore'), ((x[0], x[0], m, None), '4-D')):
        with pytest.raises(ValueError, match=match):
            contextual.compare(*bad)
    assert contextual.compare(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), m)['cx'].shape == (1,)
    with pytest.raises(ValueError, match='weights'):
        contextual.CXScore()
    with pytest.raises(ValueError, match='band_width'):
        contextual.CXScore.synthetic(0, band_width=0.0)
    with pytest.raises(ValueError, match='mu'):
        contextual.contextual_loss(torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 2, 2), mu='all')
    with pytest.raises(ValueError):
        contextual.contextual_loss(torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 2, 3))


def test_weight_loading(tmp_path):
    m = model()
    sd = m.state_dict()
    assert sorted(sd) == sorted(f'features.{i}.{k}' for i in (0, 2, 5, 7, 10, 12, 14, 16) for k in ('weight', 'bias'))
    full = dict(sd)
    full['features.19.weight'] = torch.zeros(512, 256, 3, 3)         # later layers are ignored
    full['classifier.0.weight'] = torch.zeros(3, 3)
    path = tmp_path / 'vgg19.pth'
    torch.save(full, path)
    bare = {k[len('features.'):]: v for k, v in sd.items()}
    x, y = CR.images(6, 1, 16, 16)
    want = contextual.compare(x, y, m)['cx']
    for other in (contextual.CXScore(str(path)), contextual.CXScore(bare), contextual.CXScore(full, band_width=0.5)):
        assert torch.equal(contextual.compare(x, y, other)['cx'], want)
    assert not torch.equal(contextual.compare(x, y, contextual.CXScore(sd, band_width=0.25))['cx'], want)
    wrong = dict(sd)
    wrong['features.10.weight'] = torch.zeros(256, 64, 3, 3)
    with pytest.raises(ValueError, match=r'features\.10\.weight has shape'):
        contextual.CXScore(wrong)
    missing = {k: v for k, v in sd.items() if k != 'features.16.bias'}
    with pytest.raises(ValueError, match=r'features\.16\.bias is missing'):
        contextual.CXScore(missing)
    a, b = contextual.CXScore.synthetic(1).state_dict(), contextual.CXScore.synthetic(2).state_dict()
    assert not torch.equal(a['features.0.weight'], b['features.0.weight'])
    assert torch.equal(a['features.0.weight'], contextual.CXScore.synthetic(1).state_dict()['features.0.weight'])


def test_clip_metrics_and_cli(tmp_path, capsys):
    m = model()
    x, _ = CR.images(8, 3, 176, 176)
    y = (x + 0.1 * torch.randn(x.shape, generator=torch.Generator().manual_seed(9))).clamp(-1.0, 1.0)   # (related: a finite MS-SSIM)
    plain, with_cx = im.ClipMetrics(), im.ClipMetrics(contextual=m)
    a, b = plain.update(x, y), with_cx.update(x, y)
    assert set(a) == {'mse', 'l1', 'psnr', 'ssim', 'ms_ssim', 'ssim_levels', 'cs_levels'} and set(b) == set(a) | {'cx', 'cx_loss'}
    for k in a:
        assert torch.equal(a[k], b[k])
    assert torch.equal(b['cx'], contextual.compare(x, y, m)['cx'])
    assert set(plain.summary()['mean']) == {'mse', 'l1', 'psnr', 'ssim', 'ms_ssim'}
    np.save(tmp_path / 'pred.npy', x.numpy())
    np.save(tmp_path / 'gt.npy', y.numpy())
    base = ['--pred', str(tmp_path / 'pred.npy'), '--gt', str(tmp_path / 'gt.npy'), '--device', 'cpu']
    assert im.main(base + ['--out', str(tmp_path / 'plain.json')]) == 0
    assert capsys.readouterr().err == ''
    assert im.main(base + ['--out', str(tmp_path / 'cx.json'), '--cx-synthetic', str(CR.MODEL_SEED), '--cx-band-width', '0.5']) == 0
    assert f'warning: contextual loss with synthetic weights (seed {CR.MODEL_SEED})' in capsys.readouterr().err
    with open(tmp_path / 'plain.json') as fh:
        pj = json.load(fh)
    with open(tmp_path / 'cx.json') as fh:
        cj = json.load(fh)
    assert pj == plain.summary()                                     # without a cx argument: what the scores were before
    assert set(cj['mean']) == set(pj['mean']) | {'cx', 'cx_loss'}
    assert cj['per_frame']['cx'] == [float(v) for v in b['cx']]
    for k in pj['per_frame']:
        assert cj['per_frame'][k] == pj['per_frame'][k]
    clip = im.score_files(str(tmp_path / 'pred.npy'), str(tmp_path / 'gt.npy'), device='cpu', contextual=m, chunk=2)
    assert clip.summary()['per_frame']['cx'] == cj['per_frame']['cx']
    for bad in (['--cx-band-width', '0.3'], ['--cx-synthetic', '1', '--cx-weights', 'f.pth']):
        with pytest.raises(SystemExit):
            im.main(base + ['--out', str(tmp_path / 'bad.json')] + bad)
