"""LPIPS on the CPU: the float64 restatement (invertavatar_amd/lpips.py) against the independent statement of the reference's
criterion (tests/lpips_reference.py), the properties of the score, weight loading, input checks, ClipMetrics and the CLI."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from invertavatar_amd import image_metrics as im
from invertavatar_amd import lpips

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_reference as LR  # noqa: E402

NETS = ('alex', 'vgg')
_models = {}


def model(net):
    if net not in _models:
        m = lpips.LPIPS.synthetic(net, seed=1)
        _models[net] = (m, LR.ReferenceLPIPS(net, *m.state_dicts()))
    return _models[net]


@pytest.mark.parametrize('net', NETS)
@pytest.mark.parametrize('shape', [(1, 64, 64), (3, 64, 64), (1, 40, 53), (3, 40, 53)])
def test_restatement_agrees_with_the_independent_statement(net, shape):
    m, ref = model(net)
    x, y = LR.images(11, *shape)
    want = ref.per_frame(x, y)
    got = lpips.reference_table(x, y, m)
    assert got.dtype == torch.float64 and got.shape == (shape[0], 5)
    assert float(want.min()) > 0.0
    rel = ((got - want).abs() / want.abs()).max().item()
    assert rel <= 1e-12, rel
    scalar = float(ref(x, y))
    assert abs(float(got.sum()) / shape[0] - scalar) <= 1e-12 * abs(scalar)


@pytest.mark.parametrize('net', NETS)
def test_call_is_the_sum_of_the_frames_over_n(net):
    m, ref = model(net)
    x, y = LR.images(12, 3, 40, 53)
    res = lpips.compare(x, y, m)
    assert res['lpips'].dtype == torch.float32 and res['lpips'].shape == (3,) and res['lpips_layers'].shape == (3, 5)
    assert torch.equal(m(x, y), res['lpips'].sum() / 3)
    assert abs(float(m(x, y)) - float(ref(x, y))) <= 1e-6 * float(ref(x, y))
    assert torch.allclose(res['lpips'], res['lpips_layers'].double().sum(1).float(), rtol=1e-6, atol=0)
    one = lpips.reference_compare(x, y, m)
    assert torch.equal(one['lpips'], res['lpips']) and torch.equal(one['lpips_layers'], res['lpips_layers'])


@pytest.mark.parametrize('net', NETS)
def test_identity_is_exactly_zero_and_the_score_is_symmetric(net):
    m, _ = model(net)
    x, y = LR.images(13, 2, 40, 53)
    same = lpips.compare(x, x.clone(), m)
    assert torch.equal(same['lpips'], torch.zeros(2)) and torch.equal(same['lpips_layers'], torch.zeros(2, 5))
    ab, ba = lpips.compare(x, y, m), lpips.compare(y, x, m)
    assert float(ab['lpips'].min()) > 0.0
    assert torch.allclose(ab['lpips'], ba['lpips'], rtol=1e-6, atol=0) and torch.allclose(ab['lpips_layers'], ba['lpips_layers'], rtol=1e-6, atol=0)


@pytest.mark.parametrize('net', NETS)
def test_uint8_nhwc_equals_its_float_mapping(net):
    m, _ = model(net)
    x, y = LR.images(14, 2, 40, 53)
    xu, yu = LR.to_uint8(x), LR.to_uint8(y)
    xf, yf = (t.permute(0, 3, 1, 2).double() / 127.5 - 1.0 for t in (xu, yu))
    got, want = lpips.compare(xu, yu, m), lpips.compare(xf.float().contiguous(), yf.float().contiguous(), m)
    # the float mapping rounds v / 127.5 - 1 to float32 first: 6e-8 of an input, far below 1e-5 of the score
    assert torch.allclose(got['lpips'], want['lpips'], rtol=1e-5, atol=0)
    assert torch.allclose(got['lpips_layers'], want['lpips_layers'], rtol=1e-5, atol=0)
    arrays = lpips.compare(xu.numpy(), yu.numpy(), m)
    assert torch.equal(arrays['lpips'], got['lpips'])


@pytest.mark.parametrize('net', NETS)
def test_state_dicts_load_from_files_in_both_spellings(net, tmp_path):
    m, _ = model(net)
    sd, ld = m.state_dicts()
    torch.save(sd, tmp_path / 'full.pth')
    torch.save(ld, tmp_path / 'lin.pth')
    torch.save({k.replace('features.', ''): v for k, v in sd.items()}, tmp_path / 'bare.pth')
    torch.save({k.replace('lin', '').replace('model.', ''): v for k, v in ld.items()}, tmp_path / 'renamed.pth')
    x, y = LR.images(15, 1, 40, 53)
    want = lpips.compare(x, y, m)['lpips_layers']
    for wf, lf in (('full.pth', 'lin.pth'), ('bare.pth', 'renamed.pth')):
        loaded = lpips.LPIPS(net, str(tmp_path / wf), str(tmp_path / lf))
        assert torch.equal(lpips.compare(x, y, loaded)['lpips_layers'], want)


def test_synthetic_weights_are_seeded_and_the_linear_layers_non_negative():
    a, b, c = lpips.LPIPS.synthetic('alex', 3), lpips.LPIPS.synthetic('alex', 3), lpips.LPIPS.synthetic('alex', 4)
    assert all(torch.equal(p, q) for p, q in zip(a.conv_w + a.lin, b.conv_w + b.lin))
    assert not torch.equal(a.conv_w[0], c.conv_w[0])
    assert all(float(v.min()) >= 0.0 for v in a.lin)
    assert [tuple(w.shape) for w in a.conv_w] == [(64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3)]
    assert lpips.CHANNELS == {'alex': (64, 192, 384, 256, 256), 'vgg': (64, 128, 256, 512, 512)}


def test_wrong_shapes_and_missing_keys_name_the_key():
    m, _ = model('alex')
    sd, ld = m.state_dicts()
    bad = dict(sd)
    bad['features.3.weight'] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r'features\.3\.weight'):
        lpips.LPIPS('alex', bad, ld)
    missing = {k: v for k, v in sd.items() if k != 'features.6.bias'}
    with pytest.raises(ValueError, match=r'features\.6\.bias'):
        lpips.LPIPS('alex', missing, ld)
    bad_lin = dict(ld)
    bad_lin['lin2.model.1.weight'] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(ValueError, match=r'lin2\.model\.1\.weight'):
        lpips.LPIPS('alex', sd, bad_lin)
    with pytest.raises(ValueError, match=r'lin4\.model\.1\.weight'):
        lpips.LPIPS('alex', sd, {k: v for k, v in ld.items() if not k.startswith('lin4')})
    with pytest.raises(ValueError, match='features.0.weight'):
        lpips.LPIPS('vgg', sd, ld)                          # an AlexNet file for the VGG backbone
    with pytest.raises(ValueError):
        lpips.LPIPS('squeeze', sd, ld)
    with pytest.raises(ValueError):
        lpips.LPIPS('alex')                                 # no files: nothing is downloaded


def test_undersized_images_and_other_ranges_are_refused():
    assert lpips.min_side('alex') == 31 and lpips.min_side('vgg') == 16
    for net, side in (('alex', 31), ('vgg', 16)):
        m, _ = model(net)
        ok = torch.zeros(1, 3, side, side + 3)
        assert lpips.compare(ok, ok, m)['lpips'].shape == (1,)
        for shape in ((1, 3, side - 1, 64), (1, 3, 64, side - 1)):
            small = torch.zeros(shape)
            with pytest.raises(ValueError, match='too small'):
                lpips.compare(small, small, m)
    m, _ = model('alex')
    x = torch.zeros(1, 3, 40, 40)
    with pytest.raises(ValueError, match='data_range'):
        lpips.compare(x, x, m, data_range=1.0)
    with pytest.raises(ValueError, match='data_range'):
        lpips.compare(x, x, m, data_range=255.0)
    u = torch.zeros(1, 40, 40, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='data_range'):
        lpips.compare(u, u, m, data_range=2.0)
    assert lpips.compare(x, x, m, data_range=2.0)['lpips'].shape == (1,) and lpips.compare(u, u, m, data_range=255)['lpips'].shape == (1,)
    with pytest.raises(ValueError, match='3 channels'):
        lpips.compare(torch.zeros(1, 1, 40, 40), torch.zeros(1, 1, 40, 40), m)
    with pytest.raises(ValueError):
        lpips.compare(x, x.double(), m)
    with pytest.raises(ValueError):
        lpips.compare(x, torch.zeros(2, 3, 40, 40), m)
    with pytest.raises(ValueError):
        lpips.compare(x, x, 'alex')


def test_nothing_in_the_module_reaches_for_the_network():
    with open(lpips.__file__) as fh:
        text = fh.read()
    for word in ('torch.hub', 'pretrained=', 'import torchvision', 'from torchvision', 'urllib', 'requests', 'http:', 'https:'):
        assert word not in text, word
    assert 'torchvision' not in sys.modules or not hasattr(lpips, 'torchvision')


def test_clip_metrics_gains_the_two_keys_only_with_a_model(tmp_path):
    m, _ = model('alex')
    x, y = LR.images(16, 3, 176, 176)
    plain, with_lpips = im.ClipMetrics(), im.ClipMetrics(lpips=m)
    a = plain.update(x, y)
    assert set(a) == {'mse', 'l1', 'psnr', 'ssim', 'ms_ssim', 'ssim_levels', 'cs_levels'}
    b = with_lpips.update(x[:2], y[:2])
    with_lpips.update(x[2:], y[2:])
    assert set(b) == set(a) | {'lpips', 'lpips_layers'}
    sa, sb = plain.summary(), with_lpips.summary()
    assert set(sa['mean']) == {'mse', 'l1', 'psnr', 'ssim', 'ms_ssim'} and 'lpips' not in sa['per_frame']
    assert sb['frames'] == 3 and len(sb['per_frame']['lpips']) == 3 and len(sb['per_frame']['lpips_layers'][0]) == 5
    want = lpips.compare(x, y, m)['lpips']
    assert sb['per_frame']['lpips'] == [float(v) for v in want]
    assert abs(sb['mean']['lpips'] - float(want.double().mean())) <= 1e-12
    for k in sa['mean']:
        assert sa['per_frame'][k] == sb['per_frame'][k]
    back = json.load(open(tmp_path / 'm.json')) if with_lpips.write_json(tmp_path / 'm.json') else None
    assert back['per_frame']['lpips'] == sb['per_frame']['lpips']


def test_cli_round_trips_a_json_with_synthetic_weights(tmp_path, capsys):
    x, y = LR.images(17, 3, 176, 176)
    np.save(tmp_path / 'pred.npy', x.numpy())
    np.save(tmp_path / 'gt.npy', y.numpy())
    base, out = tmp_path / 'base.json', tmp_path / 'lpips.json'
    common = ['--pred', str(tmp_path / 'pred.npy'), '--gt', str(tmp_path / 'gt.npy'), '--chunk', '2', '--device', 'cpu']
    assert im.main(common + ['--out', str(base)]) == 0
    plain = capsys.readouterr()
    assert 'lpips' not in plain.out and plain.err == ''
    assert im.main(common + ['--out', str(out), '--lpips', 'alex', '--lpips-synthetic', '5']) == 0
    said = capsys.readouterr()
    assert 'warning' in said.err and 'mean nothing' in said.err
    res, old = json.load(open(out)), json.load(open(base))
    want = lpips.compare(x, y, lpips.LPIPS.synthetic('alex', 5))['lpips']
    assert res['per_frame']['lpips'] == [float(v) for v in want] and 'lpips' in res['mean']
    assert json.loads(said.out)['mean']['lpips'] == res['mean']['lpips']
    del res['mean']['lpips'], res['min']['lpips'], res['max']['lpips'], res['per_frame']['lpips'], res['per_frame']['lpips_layers']
    assert res == old                                       # everything else is what it was
    with pytest.raises(SystemExit):
        im.main(common + ['--out', str(out), '--lpips', 'alex'])
    with pytest.raises(SystemExit):
        im.main(common + ['--out', str(out), '--lpips-synthetic', '5'])
