"""The kernels between the backbones and the renderer (csrc/rasterize.hip, csrc/fill_mouth.hip, csrc/ray_sampler.hip, csrc/styles.hip,
layout_grid_u8 of csrc/output.hip), each entry called directly, against the restatements of tests/frame_glue_reference.py over its case
tables (whose coverage of the rasteriser's paths, and whose power to tell a wrong kernel from a right one,
tests/test_frame_glue_reference_cpu.py establishes).

Tolerances are the rule of the reference module: per element ``4 x e32 + 2^-24 max|r|`` (+ the fixed-point term on the rasteriser);
``torch.equal`` where the kernel is documented to give the same bits.  Every toleranced test prints its worst ratio of error to bound
(``RATIO <form> <case>: <ratio>``).

Non-finite UV: a pixel whose u or v is NaN, +-inf or +-1e9 contributes exactly nothing to the rasterised level (aten's CPU kernels
return NaN for NaN and +-inf there)."""
import types

import pytest
import torch

from invertavatar_amd import hipops, output
from invertavatar_amd.training.networks_stylegan2 import FullyConnectedLayer
import frame_glue_reference as R

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _ratio(form, case, got, ref, tol):
    """Print and return the worst |got - ref| / tol over the elements."""
    assert tuple(got.shape) == tuple(ref.shape), f'{form} {case}: {tuple(got.shape)} != {tuple(ref.shape)}'
    err = (got.detach().cpu().double() - ref).abs()
    assert torch.isfinite(err).all(), f'{form} {case}: not finite'
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f'RATIO {form} {case}: {worst:.3f}')
    return worst


# ------------------------------------------------------------------ ia_rasterize_level

def _rasterize_on_device(case):
    i = R.rast_inputs(case)
    wide = i['sta_wide'].cuda()
    sta = wide[:, case.sta_extra:] if case.sta_extra else wide
    return hipops.rasterize_level(i['tex'].cuda(), i['uv'].cuda(), i['upper'].cuda(), sta, case.bbox, case.res)


@pytest.mark.parametrize('case', R.RAST_CASES, ids=lambda c: c.name)
def test_rasterize_level(case):
    got = _rasterize_on_device(case)
    assert torch.equal(got, _rasterize_on_device(case)), 'two runs differ'
    ref, forms = R.rast_reference(case), R.rast_forms(case)
    e32 = R.e32_of(R.rast_reference(case, torch.float32), ref)
    tol = R.rasterize_tolerance(ref, e32, int(forms['n_src'].max()), float(R.rast_inputs(case)['tex'].abs().max()))
    err = (got.cpu().double() - ref).abs()
    assert torch.isfinite(err).all()
    per_group = (err / tol).amax(1).reshape(case.B, case.res, case.res // 4, 4).amax(-1)          # worst channel and pixel of each workgroup
    worst = 0.0
    for k, form in enumerate(R.FORMS):
        for label, sel in ((form, forms['form'] == k),) if k < 3 else (('direct, 1 pass', (forms['form'] == 3) & (forms['passes'] == 1)),
                                                                      ('direct, > 1 pass', (forms['form'] == 3) & (forms['passes'] > 1))):
            if sel.any():
                r = float(per_group[sel].max())
                print(f'RATIO rasterize {label} ({int(sel.sum())} workgroups) {case.name}: {r:.3f}')
                worst = max(worst, r)
    assert worst <= 1


@pytest.mark.parametrize('kind', ['huge', 'nan'])
def test_rasterize_level_non_finite_uv_contributes_nothing(kind):
    """The result equals, bit for bit, the result on the same map with the planted pixels sent far into the zero padding."""
    case = next(c for c in R.RAST_CASES if c.uv == kind)
    i = R.rast_inputs(case)
    uv = i['uv'].clone()
    planted = ~torch.isfinite(uv[..., :2]).all(-1) | (uv[..., :2].abs() > 1e8).any(-1)
    assert planted.sum() >= 4 * 200
    uv[..., 0][planted], uv[..., 1][planted] = -3.0, -3.0
    args = (i['upper'].cuda(), i['sta_wide'].cuda(), case.bbox, case.res)
    got, want = hipops.rasterize_level(i['tex'].cuda(), i['uv'].cuda(), *args), hipops.rasterize_level(i['tex'].cuda(), uv.cuda(), *args)
    assert torch.isfinite(got).all() and torch.equal(got, want)


def test_rasterize_level_refuses_what_it_cannot_do():
    i = R.rast_inputs(R.RAST_CASES[0])
    args = (i['tex'].cuda(), i['uv'].cuda(), i['upper'].cuda(), i['sta_wide'].cuda())
    for bbox, res in (((0, 16, 0, 16), 16), ((0, 16, 0, 16), 256), ((0, 16, 0, 16), 48), ((0, 33, 0, 16), 32), ((4, 4, 0, 16), 32), ((0, 16, -1, 16), 32)):
        with pytest.raises(RuntimeError):
            hipops.rasterize_level(*args, bbox, res)


# ------------------------------------------------------------------ ia_blend_planes

@pytest.mark.parametrize('k', range(len(R.BLEND_CASES)), ids=lambda k: f'B={R.BLEND_CASES[k][0]} bbox={R.BLEND_CASES[k][1]} expanded={R.BLEND_CASES[k][2]}')
def test_blend_planes(k):
    b, bbox, expanded = R.BLEND_CASES[k]
    i = R.blend_inputs(k)
    static = i['static'].cuda()
    static = static.expand(b, -1, -1, -1) if expanded else static
    assert (static.stride(0) == 0) == (expanded and b > 1)
    got = hipops.blend_planes(i['stitch'].cuda(), i['alpha'].cuda(), static, bbox)
    assert got.shape == (b, 3, 256, 256, 32) and got.is_contiguous()
    ref = R.blend_reference(k)
    tol = R.tolerance(ref, R.e32_of(R.blend_reference(k, torch.float32), ref))
    assert _ratio('blend_planes', f'{bbox} B={b}', got, ref, tol) <= 1
    copy = R.channels_last(i['static'].expand(b, -1, -1, -1).reshape(b * 3, 32, 256, 256)).reshape(b, 3, 256, 256, 32)
    y0, y1, x0, x1 = bbox
    outside = torch.ones(256, 256, dtype=torch.bool)
    outside[y0:y1, x0:x1] = False
    g = got.cpu()
    assert torch.equal(g[:, 1:], copy[:, 1:]) and torch.equal(g[:, 0][:, outside], copy[:, 0][:, outside])


def test_blend_planes_refuses_a_bbox_that_is_not_a_square_inside_the_plane():
    i = R.blend_inputs(0)
    for bbox in ((0, 128, 0, 100), (200, 328, 0, 128), (-1, 127, 0, 128), (5, 5, 7, 7)):
        with pytest.raises(RuntimeError):
            hipops.blend_planes(i['stitch'].cuda(), i['alpha'].cuda(), i['static'].cuda(), bbox)


# ------------------------------------------------------------------ ia_cond_blend, ia_cond_blend_split, ia_channels_last

@pytest.mark.parametrize('nonfinite', [False, True])
@pytest.mark.parametrize('shape', R.COND_BLEND_SHAPES, ids=str)
def test_cond_blend_is_the_expression_bit_for_bit(shape, nonfinite):
    cond, x, _ = R.cond_inputs(*shape, nonfinite)
    want = R.cond_blend(cond, x)
    got = hipops.cond_blend(cond.cuda(), x.cuda()).cpu()
    assert torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))
    assert not nonfinite or (want.isnan().any() and want.isinf().any())


def test_cond_blend_refuses_a_pixel_count_that_is_no_multiple_of_4():
    cond, x, _ = R.cond_inputs(2, 8, 5, 7)
    with pytest.raises(RuntimeError):
        hipops.cond_blend(cond.cuda(), x.cuda())


def _planes(data):
    b, planes, c8, h, w, e = data.shape
    return [data[:, p].permute(0, 1, 4, 2, 3).reshape(b, c8 * 8, h, w).cpu() for p in range(planes)]


@pytest.mark.parametrize('styles', [False, True])
@pytest.mark.parametrize('shape', R.COND_SPLIT_SHAPES, ids=str)
def test_cond_blend_split_is_split_pair_of_the_expression(shape, styles):
    cond, x, sn = R.cond_inputs(*shape)
    hw = shape[2] * shape[3]
    hi, lo = R.split_pair(R.cond_blend(cond, x), sn if styles else None)
    hipops.split_saturation_poll()
    dev = [(cond.cuda(), x.cuda())]
    if hw % 4 == 0:                     # the same values through the one-pixel kernel: x a view 4 bytes into its storage (not 16-byte aligned)
        store = torch.empty(x.numel() + 1, device='cuda')
        store[1:] = x.reshape(-1).cuda()
        dev.append((cond.cuda(), store[1:].view(x.shape)))
        assert dev[1][1].data_ptr() % 16 != 0 and dev[1][1].is_contiguous()
    for c, xx in dev:
        got = hipops.cond_blend_split(c, xx, sn.cuda() if styles else None, None)
        got_hi, got_lo = _planes(got.data)
        assert torch.equal(got_hi, hi) and torch.equal(got_lo, lo)
    assert not hipops.split_saturation_poll()


def test_cond_blend_split_range_watch_fires_on_one_value_out_of_range_only():
    for shape in ((2, 8, 4, 4), (2, 8, 5, 7)):             # the four-pixel and the one-pixel kernel
        cond, x, sn = R.cond_inputs(*shape)
        x = x.clone()
        hipops.split_saturation_poll()
        hipops.cond_blend_split(cond.cuda(), x.cuda(), sn.cuda(), None)
        assert not hipops.split_saturation_poll()
        a = cond[1, -1, -1, -1]
        x[1, 7, -1, -1] = 7.0e4 / float((1 - a) * sn[1, 7])
        assert R.cond_blend(cond, x)[1, 7, -1, -1] * sn[1, 7] > 65504
        got = hipops.cond_blend_split(cond.cuda(), x.cuda(), sn.cuda(), None)
        assert hipops.split_saturation_poll()
        hi, lo = R.split_pair(R.cond_blend(cond, x), sn)
        assert torch.equal(_planes(got.data)[0], hi) and torch.equal(_planes(got.data)[1], lo) and hi[1, 7, -1, -1] == 65504


@pytest.mark.parametrize('hw', R.CHANNELS_LAST_HW, ids=str)
def test_channels_last_copy_bit_for_bit(hw):
    for c in R.CHANNELS_LAST_C:
        x = R.cond_inputs(2, c, *hw)[1]
        got = hipops.channels_last_copy(x.cuda())
        assert got.shape == (2, *hw, c) and got.is_contiguous() and torch.equal(got.cpu(), R.channels_last(x))


# ------------------------------------------------------------------ ia_ray_sampler

@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('res', [1, 15, 16, 17])
def test_ray_sampler_with_skewed_intrinsics(res, normalize):
    cams = R.cameras('skewed')
    o, d = hipops.ray_sampler(cams.cuda(), res, normalize)
    ro, rd = R.ray_sampler(cams.double(), res, normalize)
    _, rd32 = R.ray_sampler(cams, res, normalize)
    assert torch.equal(o.cpu(), ro.float())
    assert _ratio('ray_sampler', f'res {res} normalize {normalize}', d, rd, R.tolerance(rd, R.e32_of(rd32, rd))) <= 1


def test_ray_sampler_direction_of_length_zero_takes_the_eps():
    cams = R.cameras('zero_rotation')
    _, d = hipops.ray_sampler(cams.cuda(), 16, True)
    _, rd = R.ray_sampler(cams.double(), 16, True)
    assert (d[1] == 0).all() and (rd[1] == 0).all()
    _, rd32 = R.ray_sampler(cams, 16, True)
    assert _ratio('ray_sampler', 'zero rotation', d, rd, R.tolerance(rd, R.e32_of(rd32, rd))) <= 1


# ------------------------------------------------------------------ ia_styles_demod through StylePlan.run

def _plan_on_device(plan):
    w_dim, b, num_ws, layers = plan
    ws, params = R.style_inputs(plan)
    entries = []
    for l, (a, bias, w) in zip(layers, params):
        fc = FullyConnectedLayer(w_dim, l.I, bias=l.bias, lr_multiplier=l.lr, bias_init=1).requires_grad_(False)
        fc.weight.copy_(a)
        if l.bias:
            fc.bias.copy_(bias)
        stub = types.SimpleNamespace(affine=fc.cuda(), weight=w.cuda())
        entries.append(dict(affine=stub.affine, weight=stub.weight, widx=l.widx, demod=l.demod))
    return hipops.StylePlan(entries, torch.device('cuda')), ws


@pytest.mark.parametrize('plan', R.STYLE_PLANS, ids=lambda p: f'w_dim={p[0]} B={p[1]}')
def test_style_plan(plan):
    sp, ws = _plan_on_device(plan)
    got = sp.run(ws.cuda())
    ref, ref32 = R.styles_demod(ws.double(), R.style_layers(plan)), R.styles_demod(ws, R.style_layers(plan, torch.float32))
    worst = 0.0
    for k, (l, (s, d), (rs, rd), (rs32, rd32)) in enumerate(zip(plan[3], got, ref, ref32)):
        worst = max(worst, _ratio('styles', f'w_dim {plan[0]} layer {k} {l}', s, rs, R.tolerance(rs, R.e32_of(rs32, rs))))
        assert (d is None) == (not l.demod)
        if l.demod:
            worst = max(worst, _ratio('demod', f'w_dim {plan[0]} layer {k} {l}', d, rd, R.tolerance(rd, R.e32_of(rd32, rd))))
    assert worst <= 1


# ------------------------------------------------------------------ ia_layout_grid_u8

@pytest.mark.parametrize('hwc', [True, False])
@pytest.mark.parametrize('k', range(len(R.LAYOUT_CASES)), ids=lambda k: str(R.LAYOUT_CASES[k]))
def test_layout_grid_u8_bit_for_bit(k, hwc):
    case = R.LAYOUT_CASES[k]
    img = R.layout_image(case, k)
    with torch.no_grad():
        got = output.layout_grid(img.cuda(), grid_w=case[4], grid_h=case[5], chw_to_hwc=hwc, to_numpy=False)
    want = R.layout_grid(img, case[4], case[5], hwc)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
    flat = R.layout_grid(img, case[0], 1, False)                       # (the table does hold what it claims)
    assert set(range(256)) <= set(flat.unique().tolist()) and img.isnan().any() and img.isinf().any()


# ------------------------------------------------------------------ ia_fill_mouth, ia_mouth_edge_blur

_fill_reference = {}


def _fill_want(name):
    if name not in _fill_reference:
        _fill_reference[name] = R.fill_mouth(R.fill_case(name))
    return _fill_reference[name]


@pytest.mark.parametrize('name', R.FILL_CASES)
def test_fill_mouth_is_the_breadth_first_fill(name):
    alpha = R.fill_case(name)
    got = hipops.fill_mouth(alpha[None, None].cuda())[0, 0].cpu()
    want = _fill_want(name)
    wrong = int((got != want).sum())
    print(f'FILL {name}: {wrong} of {want.numel()} pixels differ ({int((want == 0).sum())} filled)')
    assert torch.equal(got, want)


def test_fill_mouth_batch_of_different_masks():
    names = ('256 256 face', 'maze 256 256', '256 256 wide')
    got = hipops.fill_mouth(torch.stack([R.fill_case(n) for n in names])[:, None].cuda())[:, 0].cpu()
    for k, n in enumerate(names):
        assert torch.equal(got[k], _fill_want(n)), n


def test_fill_mouth_refuses_a_mask_whose_label_image_does_not_fit():
    h, w = R.FILL_TOO_LARGE
    assert h * (w + 4) > R.FILL_LDS_BYTES >= R.FILL_LARGEST[0] * (R.FILL_LARGEST[1] + 4)
    with pytest.raises(RuntimeError):
        hipops.fill_mouth(torch.zeros(1, 1, h, w, device='cuda'))


@pytest.mark.parametrize('hw', R.EDGE_BLUR_SIZES, ids=str)
def test_mouth_edge_blur_bit_for_bit(hw):
    alpha = R.edge_blur_case(*hw)
    mouth = R.fill_mouth(alpha)
    got = hipops.mouth_edge_blur(alpha[None, None].cuda(), mouth[None, None].cuda())[0, 0].cpu()
    want = torch.from_numpy(R.mouth_edge_blur_by_loops(alpha.numpy(), mouth.numpy()))
    assert (mouth != 0).any() and torch.equal(got, want)
