"""The resampling kernels (csrc/upfirdn2d.hip: generic, tiled up 1 / up 2, pipelined, both forms of the FIR tail that writes the split
format; csrc/filtered_lrelu.hip), each entry called directly, against the float64 restatements of tests/resample_reference.py at the
tile and pad edges of its case tables (whose coverage of the dispatch, and whose power to tell a wrong kernel from a right one,
tests/test_resample_reference_cpu.py establishes).

Tolerances are the rule of the reference module: per element ``4 x e32 + 2^-24 max|r|`` for a float32 result (e32 = max|restatement in
float32 on the CPU - r| on the same inputs), ``+ 2^-11 |r|`` for fp16 storage, ``1e-12 max|r|`` for float64 storage; ``torch.equal``
where two kernels are documented to give the same bits.  Every test prints its worst ratio of error to bound
(``RATIO <form> <case>: <ratio>``).

Non-finite inputs: the clamp of every fused tail keeps a NaN (as torch.clamp does) and bounds an infinity; a NaN that reaches a split
sets the range watch."""
import pytest
import torch

from invertavatar_amd import hipops
from invertavatar_amd.torch_utils.ops import _plugins, filtered_lrelu as flr, upfirdn2d as ufd
import resample_reference as R

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


def _fir_on_device(case):
    x, f = R.fir_inputs(case)
    xd = R.layout(x.cuda().to(R.DTYPES[case.dtype]), case.layout)
    fd = R.fir_filter(case.fshape[1], case.fshape[0]).cuda().t() if case.f_transposed else f.cuda()
    assert fd.is_contiguous() != case.f_transposed
    return ufd.upfirdn2d(xd, fd, up=list(case.up), down=list(case.down), padding=list(case.pad), flip_filter=case.flip, gain=case.gain)


def _fir_tolerance(case):
    ref = R.fir_reference(case)
    return ref, R.tolerance(ref, (R.fir_reference(case, dtype=torch.float32).double() - ref).abs().max(), case.dtype)


def _check_fir(form, case):
    assert R.expected_form(case) == form.split(',')[0], (case.name, R.expected_form(case))
    got = _fir_on_device(case)
    assert got.dtype == R.DTYPES[case.dtype]
    return _ratio(form, case.name, got, *_fir_tolerance(case))


# ------------------------------------------------------------------ ia_upfirdn2d

@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('up', [1, 2])
def test_tiled_kernels_at_their_tile_and_pad_edges(up, dtype):
    assert max(_check_fir(f'tiled up{up}', case) for case in R.TILED_CASES[up, dtype]) <= 1


def _tail_tensors(c, out_hw, dtype):
    """(device tensors for the entry, float32 CPU values as the kernel sees them): the bias travels in the storage type."""
    t = R.tail_inputs(c, *out_hw)
    dev = {k: v.cuda() for k, v in t.items()}
    if dtype == 'f16':
        dev['bias'] = dev['bias'].half()
        t = {**t, 'bias': t['bias'].half().float()}
    return dev, t


def _check_fused_tail(form, case, tail, pad0):
    x, f = R.fir_inputs(case)
    up, out_hw = case.up[0], case.out_hw
    dev, t = _tail_tensors(case.shape[1], out_hw, case.dtype)
    got = hipops.upfirdn2d_bias_act(x.cuda().to(R.DTYPES[case.dtype]), f.cuda(), up=up, pad0=pad0, out_hw=out_hw, fir_gain=case.gain, flip=case.flip,
                                    **tail.kwargs(dev))
    run = lambda dt: R.fir_tail(x.to(dt), f, out_hw, up, pad0, case.gain, flip=case.flip, **tail.kwargs({k: v.to(dt) for k, v in t.items()}))   # noqa: E731
    ref = run(F64)
    return _ratio(form, f'{case.name} {tail}', got, ref, R.tolerance(ref, (run(torch.float32).double() - ref).abs().max(), case.dtype))


@pytest.mark.parametrize('case', R.PIPE_CASES + R.MULTI_TILE_CASES, ids=lambda c: c.name)
def test_pipelined_and_multi_tile_kernels_with_and_without_the_tail(case):
    form = R.expected_form(case)
    assert _check_fir(form, case) <= 1
    assert _check_fused_tail(form + ', tail', case, R.TAIL_FULL, (case.pad[0], case.pad[2])) <= 1


@pytest.mark.parametrize('geometry', R.FUSED_TAIL_GEOMETRY, ids=str)
def test_fused_tail_under_every_combination_of_its_options(geometry):
    case = R.fused_tail_case(*geometry)
    form = R.expected_form(case, 'bias_act') + ', tail'
    assert max(_check_fused_tail(form, case, tail, geometry[2]) for tail in R.TAIL_OPTIONS) <= 1


@pytest.mark.parametrize('case', R.GENERIC_CASES, ids=lambda c: c.name)
def test_generic_kernel(case):
    assert _check_fir('generic', case) <= 1


def test_filter_beyond_32x32_is_refused():
    x = R.image(1, 2, 40, 40).cuda()
    ok = ufd.upfirdn2d(x, R.fir_filter(32, 32).cuda())
    assert ok.shape == (1, 2, 9, 9)
    with pytest.raises(RuntimeError):
        ufd.upfirdn2d(x, R.fir_filter(33, 33).cuda())


@pytest.mark.parametrize('taps,up,down,pad', [(4, (2, 2), (1, 1), (2, 1, 2, 1)), (5, (2, 1), (1, 2), (3, 1, 2, 2))])
def test_separable_route_equals_the_outer_product_in_one_launch(taps, up, down, pad):
    x, f = R.image(2, 3, 11, 9), R.fir_filter(taps, None)
    kw = dict(up=list(up), down=list(down), padding=list(pad), flip_filter=True, gain=2.5)
    two = ufd.upfirdn2d(x.cuda(), f.cuda(), **kw)
    one = ufd.upfirdn2d(x.cuda(), torch.outer(f, f).cuda(), **kw)
    run = lambda dt: R.upfirdn2d(x.to(dt), f, up, down, pad, True, 2.5)      # noqa: E731
    ref = run(F64)
    tol = R.tolerance(ref, (run(torch.float32).double() - ref).abs().max())
    assert _ratio('separable, two launches', f'{taps} taps', two, ref, tol) <= 1
    assert _ratio('separable, outer product', f'{taps} taps', one, ref, tol) <= 1


# ------------------------------------------------------------------ adjoint plans on the device

def _device_adjoint(name, double_backward=False):
    shape, fshape, kw = R.ADJOINT_CASES[name]
    x = R.image(*shape, 3).cuda().requires_grad_(True)
    y = ufd.upfirdn2d(x, R.fir_filter(*fshape).cuda(), **kw)
    w = R.image(*y.shape, 4).cuda().requires_grad_(double_backward)
    gx, = torch.autograd.grad((y * w).sum(), x, create_graph=double_backward)
    if not double_backward:
        return y.detach(), gx
    gw, = torch.autograd.grad((gx * R.image(*shape, 5).cuda()).sum(), w)
    return y.detach(), gx.detach(), gw


@pytest.mark.parametrize('name', list(R.ADJOINT_CASES))
def test_gradient_runs_the_adjoint_plan_on_the_device(name):
    got, ref, y32 = _device_adjoint(name), R.adjoint_reference(name), R.adjoint_reference(name, torch.float32)
    for what, g, r, r32 in zip(('forward', 'gradient'), got, ref, y32):
        assert _ratio(f'adjoint {what}', name, g, r, R.tolerance(r, (r32.double() - r).abs().max())) <= 1


@pytest.mark.parametrize('name', ['mixed', 'upsample2d'])
def test_double_backward_runs_the_adjoint_of_the_adjoint(name):
    got, ref, y32 = _device_adjoint(name, True), R.adjoint_reference(name, F64, True), R.adjoint_reference(name, torch.float32, True)
    for what, g, r, r32 in zip(('forward', 'gradient', 'second order'), got, ref, y32):
        assert _ratio(f'adjoint {what}', name + ' (double backward)', g, r, R.tolerance(r, (r32.double() - r).abs().max())) <= 1


# ------------------------------------------------------------------ ia_fir_tail_split

def _check_split(s):
    i = R.split_inputs(s)
    d = {k: v.cuda() for k, v in i.items()}
    sn = d['styles'] if s.styles else None
    kw = dict(out_hw=s.out_hw, pad0=s.pad0, fir_gain=1.0, **s.tail.kwargs(d))
    hipops.split_saturation_poll()
    want = hipops.upfirdn2d_bias_act(d['x'], d['f'], up=1, **kw)
    y, ys = hipops.fir_tail_split(d['x'], d['f'], styles_next=sn, want_f32=True, planes=s.planes, **kw)
    assert torch.equal(y, want), f'{s}: the register form differs from upfirdn2d_bias_act'
    hi, lo = R.split_pair(want, sn, s.planes)
    got_hi, got_lo = R.act_planes(ys.data)
    assert ys.planes == s.planes and torch.equal(got_hi, hi) and (lo is None or torch.equal(got_lo, lo)), f'{s}: the pair is not split_pair(y)'
    only = hipops.fir_tail_split(d['x'], d['f'], styles_next=sn, planes=s.planes, **kw)
    assert torch.equal(only.data, ys.data), f'{s}: the DMA form differs from the register form'
    assert not hipops.split_saturation_poll()
    if s.tiny_channel:
        assert (got_hi[:, 1] == 0).all() and (got_lo[:, 1] != 0).any()
    run = lambda dt: R.fir_tail(i['x'].to(dt), i['f'], s.out_hw, 1, s.pad0, 1.0, **s.tail.kwargs({k: v.to(dt) for k, v in i.items()}))      # noqa: E731
    ref = run(F64)
    worst = _ratio('tail-register (y)', f'{s}', y, ref, R.tolerance(ref, (run(torch.float32).double() - ref).abs().max()))
    if s.planes == 2:           # the stored pair carries 22 bits of y * styles_next
        t = (want if sn is None else want * sn[:, :, None, None]).cpu().double()
        pair = ((R.pair_value(got_hi.cpu(), got_lo.cpu()) - t).abs() / R.split_bound(t)).max()
        print(f'RATIO tail-dma (pair, 22 bits) {s}: {float(pair):.3f}')
        worst = max(worst, float(pair))
    return worst


@pytest.mark.parametrize('s', R.SPLIT_GEOMETRY, ids=lambda s: f'{s.out_hw} pad0={s.pad0} planes={s.planes} C={s.c} B={s.b}')
def test_fir_tail_split_geometry(s):
    assert R.expected_form(s.fir, 'split', True) == 'tail-register' and R.expected_form(s.fir, 'split', False) == 'tail-dma'
    assert _check_split(s) <= 1


def test_fir_tail_split_under_every_combination_of_its_options():
    assert max(_check_split(s) for s in R.SPLIT_OPTIONS) <= 1


# ------------------------------------------------------------------ non-finite inputs

CLAMP = 0.4
NAN_AT, INF_AT = (0, 2, 7, 30), (0, 5, 12, 50)


def _planted(shape):
    x = R.image(*shape, 9).clone()
    x[NAN_AT], x[INF_AT] = float('nan'), float('inf')
    return x


def _check_planted(form, got, ref, saturates=True):
    """NaN exactly where the float64 restatement has one, +clamp where it saturates on the infinity, within a loose bar elsewhere."""
    got = got.detach().cpu().double()
    assert ref.isnan().sum() >= 16 and (not saturates or (ref == CLAMP).sum() >= 16) and not ref.isinf().any()
    n_lost = int((ref.isnan() & ~got.isnan()).sum())
    print(f'NONFINITE {form}: {n_lost} of {int(ref.isnan().sum())} NaN outputs came back finite'
          + (f' (as {got[ref.isnan() & ~got.isnan()].unique().tolist()})' if n_lost else ''))
    assert torch.equal(got.isnan(), ref.isnan()), f'{form}: {n_lost} outputs whose footprint covers the NaN are finite'
    fine = ~ref.isnan()
    assert (got[fine].abs() <= CLAMP * (1 + 1e-6)).all() and (got[fine] - ref[fine]).abs().max() <= 1e-5


@pytest.mark.parametrize('up,shape,out_hw', [(1, (1, 8, 20, 70), (19, 69)), (2, (1, 8, 20, 70), (39, 139)), (1, (1, 8, 515, 70), (512, 69))],
                         ids=['one tile up 1', 'one tile up 2', 'pipe'])
def test_nan_passes_the_clamp_of_the_fused_tail(up, shape, out_hw):
    f, tail, x = R.fir_filter(4, 4), R.Tail(clamp=CLAMP), _planted(shape)
    dev, t = _tail_tensors(shape[1], out_hw, 'f32')
    got = hipops.upfirdn2d_bias_act(x.cuda(), f.cuda(), up=up, pad0=(1, 1), out_hw=out_hw, fir_gain=float(up * up), **tail.kwargs(dev))
    ref = R.fir_tail(x.double(), f, out_hw, up, (1, 1), float(up * up), **tail.kwargs({k: v.double() for k, v in t.items()}))
    form = R.expected_form(R.Fir('', shape, (4, 4), (up, up), pad=R.implied_pad(shape[2:], out_hw, up, (1, 1))), 'bias_act')
    _check_planted(f'upfirdn2d_bias_act ({form})', got, ref)


def test_nan_passes_both_forms_of_the_split_and_sets_the_range_watch():
    f, tail, shape, out_hw = R.fir_filter(4, 4), R.Tail(clamp=CLAMP), (1, 8, 20, 70), (19, 69)
    x, (dev, t) = _planted(shape), _tail_tensors(8, out_hw, 'f32')
    ref = R.fir_tail(x.double(), f, out_hw, 1, (1, 1), 1.0, **tail.kwargs({k: v.double() for k, v in t.items()}))
    kw = dict(out_hw=out_hw, pad0=(1, 1), **tail.kwargs(dev))
    hipops.split_saturation_poll()
    clean = hipops.fir_tail_split(R.image(*shape, 9).cuda(), f.cuda(), **kw)
    assert not hipops.split_saturation_poll() and torch.isfinite(clean.data.float()).all()
    y, ys = hipops.fir_tail_split(x.cuda(), f.cuda(), want_f32=True, **kw)
    fired_register = hipops.split_saturation_poll()
    only = hipops.fir_tail_split(x.cuda(), f.cuda(), **kw)
    fired_dma = hipops.split_saturation_poll()
    print(f'NONFINITE range watch: register form {fired_register}, DMA form {fired_dma}; pairs equal {torch.equal(only.data, ys.data)}')
    _check_planted('fir_tail_split (register form, y)', y, ref)
    assert fired_register and fired_dma
    assert torch.equal(only.data, ys.data)
    hipops.fir_tail_split(R.image(*shape, 9).cuda(), f.cuda(), want_f32=True, **kw)
    assert not hipops.split_saturation_poll()


def test_nan_passes_the_clamp_of_filtered_lrelu():
    x, fu, fd = _planted((1, 8, 20, 70)), R.fir_filter(8, None), R.fir_filter(6, None)
    b = R.tail_inputs(8, 1, 1)['bias']
    got, _, rc = _plugins.filtered_lrelu(x.cuda(), fu.cuda(), fd.cuda(), b.cuda(), None, 2, 2, 5, 4, 3, 6, 0, 0, 2 ** 0.5, 0.2, CLAMP, False, False)
    assert rc == 0
    _check_planted('filtered_lrelu', got, R.filtered_lrelu(x.double(), fu, fd, b.double(), 2, 2, (5, 4, 3, 6), 2 ** 0.5, 0.2, CLAMP), saturates=False)


# ------------------------------------------------------------------ ia_filtered_lrelu

@pytest.mark.parametrize('up,down', R.FLR_RATES)
def test_filtered_lrelu_across_its_tile_edge(up, down):
    worst = 0.0
    for c in (c for c in R.FLR_CASES if (c.up, c.down) == (up, down)):
        x, fu, fd, b = R.flr_inputs(c)
        dt = R.DTYPES[c.dtype]
        dev = lambda t, cast=None: None if t is None else (t.cuda() if cast is None else t.cuda().to(cast))      # noqa: E731
        px0, px1, py0, py1 = c.pad
        got, _, rc = _plugins.filtered_lrelu(dev(x, dt), dev(fu), dev(fd), dev(b, dt), None, c.up, c.down, px0, px1, py0, py1, 0, 0, 2 ** 0.5, c.slope,
                                             -1 if c.clamp is None else c.clamp, c.flip, False)
        assert rc == 0 and got.dtype == dt
        via_api = flr.filtered_lrelu(dev(x, dt), dev(fu), dev(fd), dev(b, dt), up=c.up, down=c.down, padding=list(c.pad), gain=2 ** 0.5, slope=c.slope,
                                     clamp=c.clamp, flip_filter=c.flip)
        assert torch.equal(via_api, got)
        ref = R.flr_reference(c)
        tol = R.tolerance(ref, (R.flr_reference(c, dtype=torch.float32).double() - ref).abs().max(), c.dtype)
        worst = max(worst, _ratio('filtered_lrelu', c.name, got, ref, tol))
    assert worst <= 1
