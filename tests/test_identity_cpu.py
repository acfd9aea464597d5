"""Identity similarity on the CPU: the float64 restatement (invertavatar_amd/identity.py) against the recorded results of the reference's
IDLoss (tests/golden/identity.npz, made by tests/golden/make_identity_golden.py), the network's non-degeneracy on the test frames,
model_irse.Backbone, weight loading, input checks, ClipMetrics and the CLI."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from invertavatar_amd import identity
from invertavatar_amd import image_metrics as im

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import identity_cases as IC  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_cache = {}


def model():
    if 'model' not in _cache:
        _cache['model'] = identity.IDScore.synthetic(IC.MODEL_SEED)
    return _cache['model']


def stages(dtype):
    """The restatement's stage list on the six test frames (x then y), computed once per dtype."""
    if dtype not in _cache:
        x, y = IC.frames()
        _cache[dtype] = identity.reference_stages(torch.cat([x, y]), model(), dtype)
    return _cache[dtype]


def golden():
    g = np.load(os.path.join(GOLDEN, 'identity.npz'))
    assert int(g['frame_seed']) == IC.SEED and int(g['model_seed']) == IC.MODEL_SEED
    return g


def test_state_names_and_shapes_are_the_references():
    want = {}
    with open(os.path.join(GOLDEN, 'identity_state_names.txt')) as fh:
        for line in fh:
            key, shape = line.split()
            want[key] = () if shape == 'scalar' else tuple(int(s) for s in shape.split('x'))
    spec = dict(identity.state_spec())
    assert len(spec) == len(identity.state_spec()) == len(want) and spec == want
    sd = model().state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    from invertavatar_amd.encoder_inversion.models.model_irse import Backbone
    ours = Backbone(112, 50, mode='ir_se', drop_ratio=0.6).state_dict()
    assert {k: tuple(v.shape) for k, v in ours.items()} == want


def test_restatement_matches_the_recorded_reference():
    """|float64 restatement - the reference's float32 run| <= 4 e32 + eps32 * scale, e32 the restatement's own float32-vs-float64 distance."""
    g = golden()
    f64, f32 = stages(torch.float64)[-1], stages(torch.float32)[-1]
    want = torch.from_numpy(np.concatenate([g['feats_x'], g['feats_y']]))
    IC.check('embeddings', want, f64, f32)
    sim64, sim32 = (f64[:3] * f64[3:]).sum(1), (f32[:3] * f32[3:]).sum(1)
    fwd64, fwd32 = (1.0 - sim64).sum() / 3, (1.0 - sim32).sum() / 3
    IC.check('forward', torch.tensor(float(g['forward'])), fwd64, fwd32)
    IC.check('CSIM_loss', torch.tensor(float(g['csim_loss'])), fwd64, fwd32)
    x, y = IC.frames()
    res = identity.compare(x, y, model())
    assert res['id_sim'].dtype == torch.float32 and torch.equal(res['id_sim'], sim64.float())
    assert torch.equal(identity.reference_compare(x, y, model())['id_sim'], res['id_sim'])
    assert torch.equal(model()(x, y), (1.0 - res['id_sim']).sum() / 3)
    loss = identity.IDLoss(model())
    assert torch.equal(loss.forward(x, y), model()(x, y)) and torch.equal(loss.extract_feats(x), f64[:3].float())
    IC.check('our CSIM_loss', loss.CSIM_loss(x, y), fwd64, fwd32)
    assert torch.equal(identity.similarity(f64[:3].float(), f64[3:].float()), (f64[:3].float().double() * f64[3:].float().double()).sum(1).float())
    with pytest.raises(ValueError, match='num_scales'):
        identity.IDLoss(model(), num_scales=2)


def test_backbone_in_float64_equals_the_restatement():
    from invertavatar_amd.encoder_inversion.models.model_irse import Backbone
    net = Backbone(112, 50, mode='ir_se', drop_ratio=0.6)
    net.load_state_dict(model().state_dict())
    net = net.double().eval()
    x, y = IC.frames()
    front = identity.reference_front(torch.cat([x, y]))
    with torch.no_grad():
        got = net.stages(front, identity.STAGE_ENDS)
    want = stages(torch.float64)
    assert len(got) == len(want) == len(identity.STAGE_NAMES)
    for name, a, b in zip(identity.STAGE_NAMES, got, want):
        assert a.shape == b.shape and (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), name
    with torch.no_grad():
        assert torch.equal(net(front), got[-1])


def test_the_synthetic_network_is_not_degenerate_on_the_test_frames():
    """So that the device comparison cannot pass vacuously: per frame, the float64 l2 norm of every compared activation in front of the
    normalisation stays in [1e-3, 1e3]; the similarities of the two distinct pairs span at least 0.2 and keep 1e-3 from +-1."""
    st = stages(torch.float64)
    for name, s in zip(identity.STAGE_NAMES[:-1], st[:-1]):
        norms = s.flatten(1).norm(dim=1)
        print(name, tuple(s.shape), float(norms.min()), float(norms.max()))
        assert 1e-3 <= float(norms.min()) and float(norms.max()) <= 1e3, name
    f = st[-1]
    assert ((f.norm(dim=1) - 1.0).abs() <= 1e-12).all()
    sim = (f[:3] * f[3:]).sum(1)
    print('similarities', sim.tolist())
    assert abs(float(sim[0]) - 1.0) <= 1e-12                # the identical pair
    near, far = float(sim[1]), float(sim[2])
    assert near - far >= 0.2
    for v in (near, far):
        assert -1.0 + 1e-3 <= v <= 1.0 - 1e-3


def test_synthetic_weights_depend_on_seed_and_key_only():
    a, b, c = model().state_dict(), identity.IDScore.synthetic(IC.MODEL_SEED).state_dict(), identity.IDScore.synthetic(IC.MODEL_SEED + 1).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a['body.3.res_layer.1.weight'], c['body.3.res_layer.1.weight'])
    assert float(a['body.5.res_layer.0.running_var'].min()) > 0.0


def test_loading_takes_the_facenet_prefix_and_names_the_key_it_rejects(tmp_path):
    sd = model().state_dict()
    torch.save({'facenet.' + k: v for k, v in sd.items()}, tmp_path / 'prefixed.pth')
    loaded = identity.IDScore(str(tmp_path / 'prefixed.pth'))
    assert all(torch.equal(loaded.sd[k], sd[k]) for k in sd)
    no_counters = identity.IDScore({k: v for k, v in sd.items() if not k.endswith('num_batches_tracked')})
    assert set(no_counters.state_dict()) == set(sd)
    bad = dict(sd)
    bad['body.7.res_layer.3.weight'] = torch.zeros(256, 256, 1, 1)
    with pytest.raises(ValueError, match=r'body\.7\.res_layer\.3\.weight'):
        identity.IDScore(bad)
    with pytest.raises(ValueError, match=r'output_layer\.3\.bias'):
        identity.IDScore({k: v for k, v in sd.items() if k != 'output_layer.3.bias'})
    with pytest.raises(ValueError):
        identity.IDScore()                                  # no file: nothing is downloaded
    with open(identity.__file__) as fh:
        text = fh.read()
    for word in ('torch.hub', 'pretrained=', 'urllib', 'requests', 'http:', 'https:'):
        assert word not in text, word


def test_other_ranges_small_images_and_mixed_inputs_are_refused():
    m = model()
    x = torch.zeros(1, 3, 256, 256)
    for shape in ((1, 3, 255, 256), (1, 3, 256, 255), (1, 3, 112, 112)):
        small = torch.zeros(shape)
        with pytest.raises(ValueError, match='too small'):
            identity.compare(small, small, m)
        with pytest.raises(ValueError, match='too small'):
            identity.embed(small, m)
    with pytest.raises(ValueError, match='data_range'):
        identity.compare(x, x, m, data_range=1.0)
    with pytest.raises(ValueError, match='data_range'):
        identity.compare(x, x, m, data_range=255.0)
    u = torch.zeros(1, 256, 256, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='data_range'):
        identity.compare(u, u, m, data_range=2.0)
    with pytest.raises(ValueError, match='3 channels'):
        identity.compare(torch.zeros(1, 1, 256, 256), torch.zeros(1, 1, 256, 256), m)
    with pytest.raises(ValueError):
        identity.compare(x, x.double(), m)
    with pytest.raises(ValueError):
        identity.compare(x, torch.zeros(2, 3, 256, 256), m)
    with pytest.raises(ValueError):
        identity.compare(x, x, 'ir_se50')


def test_uint8_and_larger_frames_take_the_stated_mapping():
    m = model()
    x, _ = IC.frames()
    xu = IC.to_uint8(x[:1])
    xf = (xu.permute(0, 3, 1, 2).double() / 127.5 - 1.0).float().contiguous()
    a, b = identity.embed(xu, m), identity.embed(xf, m)
    assert (a - b).abs().max().item() <= 1e-5               # the float mapping rounds v / 127.5 - 1 to float32 first
    assert torch.equal(identity.embed(xu.numpy(), m), a)
    big = IC.frames(h=300, w=257)[0][:1]                    # pooled to 256^2 first, with torch's adaptive windows
    pooled = torch.nn.functional.adaptive_avg_pool2d(big.double(), (256, 256))
    want = identity.reference_stages(pooled, m)[-1]
    got = identity.reference_stages(big, m)[-1]
    assert (got - want).abs().max().item() <= 1e-12
    # the 188 -> 112 windows are 2 or 3 wide
    widths = {-(-(i + 1) * 188 // 112) - (i * 188) // 112 for i in range(112)}
    assert widths == {2, 3}


def _clip_inputs():
    """Three pairs whose MS-SSIM is a number (an unrelated picture can have a negative mean cs: NaN by definition, and NaN != NaN)."""
    x, y = IC.frames()
    return x, torch.stack([y[0], y[1], x[2] * 0.8]).contiguous()


def test_clip_metrics_gains_id_sim_only_with_a_model(tmp_path):
    m = model()
    x, y = _clip_inputs()
    plain, with_id = im.ClipMetrics(), im.ClipMetrics(identity=m)
    a = plain.update(x, y)
    assert set(a) == {'mse', 'l1', 'psnr', 'ssim', 'ms_ssim', 'ssim_levels', 'cs_levels'}
    b = with_id.update(x[:2], y[:2])
    with_id.update(x[2:], y[2:])
    assert set(b) == set(a) | {'id_sim'}
    sa, sb = plain.summary(), with_id.summary()
    assert set(sa['mean']) == {'mse', 'l1', 'psnr', 'ssim', 'ms_ssim'} and 'id_sim' not in sa['per_frame']
    want = identity.compare(x, y, m)['id_sim']
    assert sb['frames'] == 3 and sb['per_frame']['id_sim'] == [float(v) for v in want]
    assert abs(sb['mean']['id_sim'] - float(want.double().mean())) <= 1e-12
    for k in sa['mean']:
        assert sa['per_frame'][k] == sb['per_frame'][k]
    back = with_id.write_json(tmp_path / 'm.json') and json.load(open(tmp_path / 'm.json'))
    assert back['per_frame']['id_sim'] == sb['per_frame']['id_sim']


def test_cli_adds_the_column_only_when_asked(tmp_path, capsys):
    x, y = _clip_inputs()
    np.save(tmp_path / 'pred.npy', x.numpy())
    np.save(tmp_path / 'gt.npy', y.numpy())
    base, out = tmp_path / 'base.json', tmp_path / 'id.json'
    common = ['--pred', str(tmp_path / 'pred.npy'), '--gt', str(tmp_path / 'gt.npy'), '--chunk', '2', '--device', 'cpu']
    assert im.main(common + ['--out', str(base)]) == 0
    plain = capsys.readouterr()
    assert 'id_sim' not in plain.out and plain.err == ''
    direct = im.score_files(str(tmp_path / 'pred.npy'), str(tmp_path / 'gt.npy'), chunk=2, device='cpu').summary()
    assert json.load(open(base)) == json.loads(json.dumps(direct))
    assert im.main(common + ['--out', str(out), '--id-synthetic', str(IC.MODEL_SEED)]) == 0
    said = capsys.readouterr()
    assert 'warning' in said.err and 'mean nothing' in said.err
    res, old = json.load(open(out)), json.load(open(base))
    want = identity.compare(x, y, model())['id_sim']
    assert res['per_frame']['id_sim'] == [float(v) for v in want] and 'id_sim' in res['mean']
    assert json.loads(said.out)['mean']['id_sim'] == res['mean']['id_sim']
    del res['mean']['id_sim'], res['min']['id_sim'], res['max']['id_sim'], res['per_frame']['id_sim']
    assert res == old                                       # everything else is what it was
    torch.save(model().state_dict(), tmp_path / 'w.pth')
    assert im.main(common + ['--out', str(out), '--id-weights', str(tmp_path / 'w.pth')]) == 0
    said = capsys.readouterr()
    assert said.err == '' and json.load(open(out))['per_frame']['id_sim'] == [float(v) for v in want]
    with pytest.raises(SystemExit):
        im.main(common + ['--out', str(out), '--id-weights', str(tmp_path / 'w.pth'), '--id-synthetic', '1'])
