"""Identity similarity on the device: ia_face_crop_pool, ia_conv3x3_small, ia_id_head and ia_id_similarity at their edges, and the whole
path stage by stage, against float64.

Bound (the project's): |device - float64| <= 4 * e32 + eps32 * scale, where e32 is the distance of the float32 CPU run of the same
statement from float64 on the same inputs and scale the largest float64 magnitude of the compared tensor.  Both numbers are printed
per case."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from invertavatar_amd import identity
from invertavatar_amd import image_metrics as im

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import identity_cases as IC  # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def model():
    if 'model' not in _cache:
        _cache['model'] = identity.IDScore.synthetic(IC.MODEL_SEED)
    return _cache['model']


def reference(dtype):
    """The restatement's stage list on the six fixture frames (x then y), computed once per dtype on the CPU."""
    if dtype not in _cache:
        x, y = IC.frames()
        _cache[dtype] = identity.reference_stages(torch.cat([x, y]), model(), dtype)
    return _cache[dtype]


# ------------------------------------------------------------------ ia_face_crop_pool

@pytest.mark.parametrize('hw', [(256, 256), (512, 512), (257, 300)])
@pytest.mark.parametrize('kind', ['float', 'uint8'])
@pytest.mark.parametrize('n', [1, 3])
def test_crop_pool_against_float64(hw, kind, n):
    from invertavatar_amd import hipops
    x = IC.frames(seed=40 + n, h=hw[0], w=hw[1])[0][:n].contiguous()
    if kind == 'uint8':
        x = IC.to_uint8(x)
    got = hipops.face_crop_pool(x.cuda())
    assert got.shape == (n, 3, 112, 112) and got.dtype == torch.float32
    IC.check(f'face_crop_pool {kind} N{n} {hw}', got, identity.reference_front(x, torch.float64), identity.reference_front(x, torch.float32))
    assert torch.equal(got, hipops.face_crop_pool(x.cuda()))
    if n == 3:
        assert torch.equal(got[1:2], hipops.face_crop_pool(x[1:2].contiguous().cuda()))


def test_crop_pool_refuses_small_frames_and_other_layouts():
    from invertavatar_amd import hipops
    for shape in ((1, 3, 255, 256), (1, 3, 256, 200), (1, 4, 256, 256)):
        with pytest.raises(RuntimeError):
            hipops.face_crop_pool(torch.zeros(shape, device='cuda'))
    with pytest.raises(RuntimeError):
        hipops.face_crop_pool(torch.zeros(1, 3, 256, 256, device='cuda', dtype=torch.float16))


# ------------------------------------------------------------------ ia_conv3x3_small

SMALL_CASES = [  # (I, O, h, w, B)
    (8, 8, 7, 7, 1), (8, 8, 1, 1, 1), (8, 8, 3, 5, 1), (8, 8, 7, 2, 1),
    (24, 40, 7, 7, 3),                                      # 40 outputs: a partly filled channel tile; 24 inputs: three staged blocks of one chunk
    (40, 8, 5, 7, 2),                                       # 40 inputs: two chunks (32 + 8), the second one short
    (512, 512, 7, 7, 2),                                    # the network's layer: 8 channel tiles x 16 chunks
]


def small_inputs(case, mode):
    i, o, h, w, b = case
    x, wt = rnd(1, b, i, h, w), rnd(2, o, i, 3, 3) * (1.0 / (9 * i)) ** 0.5
    p = {'in_scale': None, 'in_shift': None, 'out_scale': None, 'out_shift': None, 'slopes': None}
    if mode in ('first', 'shifted'):                        # a unit's first convolution: BatchNorm in front, PReLU behind
        p['in_scale'], p['in_shift'] = rnd(3, i).abs() * 0.5 + 0.5, rnd(4, i) * (100.0 if mode == 'shifted' else 0.3)
        p['slopes'] = rnd(5, o).abs() * 0.3
    elif mode == 'second':                                  # its second one: BatchNorm behind
        p['out_scale'], p['out_shift'] = rnd(6, o).abs() * 0.5 + 0.5, rnd(7, o) * 0.3
    elif mode == 'all':
        p['in_scale'], p['in_shift'] = rnd(3, i).abs() * 0.5 + 0.5, rnd(4, i) * 0.3
        p['out_scale'], p['out_shift'], p['slopes'] = rnd(6, o).abs() * 0.5 + 0.5, rnd(7, o) * 0.3, rnd(5, o).abs() * 0.3
    return x, wt, p


def small_reference(x, wt, p, dt):
    """The statement: the affine map, THEN the zero padding, the convolution, scale, shift, PReLU."""
    v = x.to(dt)
    if p['in_scale'] is not None:
        v = v * p['in_scale'].to(dt).reshape(1, -1, 1, 1) + p['in_shift'].to(dt).reshape(1, -1, 1, 1)
    y = F.conv2d(v, wt.to(dt), padding=1)
    if p['out_scale'] is not None:
        y = y * p['out_scale'].to(dt).reshape(1, -1, 1, 1)
    if p['out_shift'] is not None:
        y = y + p['out_shift'].to(dt).reshape(1, -1, 1, 1)
    if p['slopes'] is not None:
        y = torch.where(y < 0, y * p['slopes'].to(dt).reshape(1, -1, 1, 1), y)
    return y


@pytest.mark.parametrize('case', SMALL_CASES, ids=lambda c: 'I{}_O{}_{}x{}_B{}'.format(*c))
@pytest.mark.parametrize('mode', ['plain', 'first', 'second', 'all', 'shifted'])
def test_small_convolution_against_float64(case, mode):
    """'shifted': input shifts of about 100 on activations of about 1.  Padding in front of the affine map would put the shift into the
    border taps: an error of the size of the result itself at every border pixel, against a bound of a few 1e-5 of it."""
    from invertavatar_amd import hipops
    x, wt, p = small_inputs(case, mode)
    dev = {k: (None if v is None else v.cuda()) for k, v in p.items()}
    wk = hipops.pack_conv_weight(wt.cuda())
    got = hipops.conv3x3_small(x.cuda(), wk, **dev)
    want = small_reference(x, wt, p, torch.float64)
    assert got.shape == want.shape
    IC.check(f'conv3x3_small {mode} {case}', got, want, small_reference(x, wt, p, torch.float32))
    if mode == 'shifted':                                   # the check has teeth: the wrong order of padding and shift is far outside it
        v = F.pad(x.double(), (1, 1, 1, 1)) * p['in_scale'].double().reshape(1, -1, 1, 1) + p['in_shift'].double().reshape(1, -1, 1, 1)
        wrong = F.conv2d(v, wt.double())
        wrong = torch.where(wrong < 0, wrong * p['slopes'].double().reshape(1, -1, 1, 1), wrong)
        assert (wrong - want).abs().max().item() > 1e3 * (got.double().cpu() - want).abs().max().item()
    assert torch.equal(got, hipops.conv3x3_small(x.cuda(), wk, **dev))
    if case[4] > 1:                                         # the K split depends on I alone: an image's result is the same in any batch
        alone = hipops.conv3x3_small(x[1:2].contiguous().cuda(), wk, **dev)
        assert torch.equal(alone, got[1:2])


def test_small_convolution_refuses_what_it_does_not_cover():
    from invertavatar_amd import hipops
    wk = torch.zeros(9, 8, 8, device='cuda')
    for shape in ((1, 8, 8, 8), (1, 8, 7, 9), (1, 16, 7, 7)):
        with pytest.raises(RuntimeError):
            hipops.conv3x3_small(torch.zeros(shape, device='cuda'), wk)
    with pytest.raises(RuntimeError):
        hipops.conv3x3_small(torch.zeros(1, 4, 7, 7, device='cuda'), torch.zeros(9, 4, 8, device='cuda'))
    with pytest.raises(RuntimeError):
        hipops.conv3x3_small(torch.zeros(1, 8, 7, 7, device='cuda'), wk, in_scale=torch.ones(8, device='cuda'))


# ------------------------------------------------------------------ ia_id_head

def head_reference(x, w, b, s, t, dt):
    z = F.linear(x.to(dt), w.to(dt), b.to(dt)) * s.to(dt) + t.to(dt)
    return torch.div(z, torch.norm(z, 2, 1, True))


@pytest.mark.parametrize('k,o,batches', [(8 * 49, 8, (1, 5)), (512 * 49, 512, (1, 3))], ids=['K392_O8', 'K25088_O512'])
def test_head_against_float64(k, o, batches):
    from invertavatar_amd import hipops
    w, b = rnd(11, o, k) * (1.0 / k) ** 0.5, rnd(12, o) * 0.1
    s, t = rnd(13, o).abs() * 0.5 + 0.5, rnd(14, o) * 0.1
    wd, bd, sd, td = w.cuda(), b.cuda(), s.cuda(), t.cuda()
    xs = rnd(15, max(batches), k)
    want64, want32 = head_reference(xs, w, b, s, t, torch.float64), head_reference(xs, w, b, s, t, torch.float32)
    for n in batches:
        got = hipops.id_head(xs[:n].contiguous().cuda(), wd, bd, sd, td)
        assert got.shape == (n, o)
        IC.check(f'id_head K{k} O{o} B{n}', got, want64[:n], want32[:n])
        assert ((got.double().norm(dim=1) - 1.0).abs() <= 4 * IC.EPS32).all()
        assert torch.equal(got, hipops.id_head(xs[:n].contiguous().cuda(), wd, bd, sd, td))
    # an image's embedding does not depend on the batch it is in; a [B,C,7,7] input is read flattened
    one, many = hipops.id_head(xs[:1].contiguous().cuda(), wd, bd, sd, td), hipops.id_head(xs.contiguous().cuda(), wd, bd, sd, td)
    assert torch.equal(one, many[:1])
    assert torch.equal(hipops.id_head(xs.reshape(-1, k // 49, 7, 7).contiguous().cuda(), wd, bd, sd, td), many)


def test_head_divides_a_zero_vector_as_torch_div_does():
    from invertavatar_amd import hipops
    x = torch.zeros(2, 392)
    x[1] = rnd(16, 392)
    w = rnd(17, 8, 392).cuda()
    got = hipops.id_head(x.cuda(), w)
    want = torch.div(torch.zeros(8), torch.norm(torch.zeros(1, 8), 2, 1, True))
    assert torch.isnan(want).all() and torch.isnan(got[0]).all() and torch.isfinite(got[1]).all()


# ------------------------------------------------------------------ ia_id_similarity

@pytest.mark.parametrize('n', [1, 5])
def test_similarity_against_float64_and_its_bit_equalities(n):
    from invertavatar_amd import hipops
    f = F.normalize(rnd(20 + n, 2 * n, 512), dim=1)
    fd = f.cuda()
    got = hipops.id_similarity(fd)
    IC.check(f'id_similarity N{n}', got, (f[:n].double() * f[n:].double()).sum(1), (f[:n] * f[n:]).sum(1))
    assert torch.equal(got, hipops.id_similarity(fd))
    assert torch.equal(got, hipops.id_similarity(torch.cat([fd[n:], fd[:n]]).contiguous()))
    for j in range(n):
        assert torch.equal(hipops.id_similarity(torch.stack([fd[j], fd[n + j]]).contiguous()), got[j:j + 1])
    assert torch.equal(identity.similarity(fd[:n].contiguous(), fd[n:].contiguous()), got)
    table = torch.full((n, 3), -1.0, device='cuda')
    hipops.id_similarity(fd, out=table[:, 1])
    assert torch.equal(table[:, 1], got) and bool((table[:, [0, 2]] == -1.0).all())


# ------------------------------------------------------------------ the whole path

def test_whole_path_stage_by_stage_against_float64():
    """The fixture's three pairs through the device path, compared after the input layer, after each of the four stages, at the
    embedding and at the score, each held to 4 * e32 + eps32 * scale of the float64 restatement; every point is measured before the
    first failure is raised, so that a miss names its stage."""
    x, y = IC.frames()
    want64, want32 = reference(torch.float64), reference(torch.float32)
    got = identity.device_stages(torch.cat([x, y]).cuda(), model())
    missed = []
    for name, g, a, b in zip(identity.STAGE_NAMES, got, want64, want32):
        if g is None:
            continue
        assert g.shape == a.shape, name
        try:
            IC.check(f'whole path: {name}', g, a, b)
        except AssertionError as e:
            missed.append(str(e))
    sim = identity.compare(x.cuda(), y.cuda(), model())['id_sim']
    s64, s32 = (want64[-1][:3] * want64[-1][3:]).sum(1), (want32[-1][:3] * want32[-1][3:]).sum(1)
    try:
        IC.check('whole path: id_sim', sim, s64, s32)
    except AssertionError as e:
        missed.append(str(e))
    assert not missed, '; '.join(missed)


def test_whole_path_on_uint8_and_512_frames():
    m = model()
    x = IC.frames(seed=50, h=512, w=512)[0]
    for name, frames in (('float 512', x), ('uint8 512', IC.to_uint8(x))):
        want64 = identity.reference_stages(frames[:2], m, torch.float64)[-1]
        want32 = identity.reference_stages(frames[:2], m, torch.float32)[-1]
        got = identity.embed(frames[:2].contiguous().cuda(), m)
        assert got.shape == (2, 512) and got.dtype == torch.float32 and got.is_cuda
        IC.check(f'embed {name}', got, want64, want32)


def test_identical_frames_exchange_repeats_and_batches():
    from invertavatar_amd import hipops
    m = model()
    x, y = IC.frames()
    xd, yd = x.cuda(), y.cuda()
    first = identity.compare(xd, yd, m)['id_sim']
    assert first.is_cuda and first.dtype == torch.float32 and first.shape == (3,)
    assert torch.equal(first, identity.compare(xd, yd, m)['id_sim'])                      # the same bits run to run
    assert torch.equal(first, identity.compare(yd, xd, m)['id_sim'])                      # exchanging x and y gives the same bits
    same = identity.compare(xd, xd.clone(), m)['id_sim']
    f = identity.embed(torch.cat([xd, xd]), m)             # (the same batch of 6: the stride-2 plans depend on B)
    assert torch.equal(f[:3], f[3:])                                                      # a frame's embedding does not depend on its place
    assert torch.equal(same, hipops.id_similarity(torch.cat([f[:3], f[:3]]).contiguous()))        # a unit vector dotted with itself
    assert ((same.double() - 1.0).abs() <= 4 * IC.EPS32).all()
    assert torch.equal(m(xd, yd), (1.0 - first).sum() / 3)
    loss = identity.IDLoss(m)
    assert torch.equal(loss(xd, yd), m(xd, yd)) and loss.extract_feats(xd).shape == (3, 512)
    # batch 1 against batch 5: each within the bound of float64 (bit equality is not asked: the stride-2 plans depend on B)
    want64, want32 = reference(torch.float64)[-1], reference(torch.float32)[-1]
    order = [0, 1, 2, 4, 5]                                                               # pairs (x0,y0) (x1,y1) (x2,y2) (y1,x1) (y2,x2)
    other = [3, 4, 5, 1, 2]
    s64, s32 = (want64[order] * want64[other]).sum(1), (want32[order] * want32[other]).sum(1)
    all6 = torch.cat([xd, yd])
    five = identity.compare(all6[order].contiguous(), all6[other].contiguous(), m)['id_sim']
    IC.check('batch of 5', five, s64, s32)
    for j in (1, 4):
        one = identity.compare(all6[order[j]:order[j] + 1].contiguous(), all6[other[j]:other[j] + 1].contiguous(), m)['id_sim']
        IC.check(f'batch of 1 (pair {j})', one, s64[j:j + 1], s32[j:j + 1])


def test_device_tensors_never_reach_torch_convolutions_linears_or_pools(monkeypatch):
    m = model()
    x, y = IC.frames(seed=60, h=300, w=257)
    want = identity.compare(x.cuda(), y.cuda(), m)

    def no_library(*a, **k):
        raise AssertionError('the device route must not reach torch convolutions, linear layers or pools')
    for name in ('conv2d', 'linear', 'max_pool2d', 'avg_pool2d', 'adaptive_avg_pool2d', 'adaptive_max_pool2d'):
        monkeypatch.setattr(torch.nn.functional, name, no_library)
        if hasattr(torch, name):
            monkeypatch.setattr(torch, name, no_library)
    got = identity.compare(x.cuda(), y.cuda(), m)
    assert torch.equal(got['id_sim'], want['id_sim'])
    with pytest.raises(AssertionError):
        identity.compare(x, y, m)                           # the CPU route is the torch restatement


def test_clip_metrics_with_identity_through_drive_sequence():
    from encoder_common import build_inversion_net
    from invertavatar_amd import eval_seq, synthetic
    m = model()
    net = build_inversion_net('small').cuda()
    g = net.generator
    nrr = 32
    g.neural_rendering_resolution = nrr
    frames = [40, 41]
    c, uv = synthetic.camera_labels(frames).cuda(), synthetic.uv_conditions(frames).cuda()
    jit = synthetic.jitter(frames, nrr * nrr).squeeze(-1).cuda()
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(3, 1).cuda(), synthetic.conditioning_camera().cuda(), truncation_psi=0.7, truncation_cutoff=14)
        res = {'w': ws,
               'texture': g.texture_backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const'),
               'static': g.backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const')}
        plain, _ = eval_seq.drive_sequence(net, ws, res, c, uv, jitter=jit, batch=2, graphed=False)
        gt = (plain * 0.9 + 0.05).clamp(-1, 1).contiguous()
        clip = im.ClipMetrics(identity=m)
        images, _ = eval_seq.drive_sequence(net, ws, res, c, uv, jitter=jit, batch=2, graphed=False, gt=gt, metrics=clip)
    assert torch.equal(images, plain) and images.shape[-2:] == (512, 512)
    s = clip.summary()
    want = identity.compare(images, gt, m)['id_sim']
    assert s['frames'] == 2 and s['per_frame']['id_sim'] == [float(v) for v in want.cpu()]
    assert abs(s['mean']['id_sim'] - float(np.mean(s['per_frame']['id_sim']))) <= 1e-12
    assert set(im.ClipMetrics().update(images, gt)) == {'mse', 'l1', 'psnr', 'ssim', 'ms_ssim', 'ssim_levels', 'cs_levels'}
