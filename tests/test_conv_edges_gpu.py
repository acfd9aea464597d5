"""The convolution family (csrc/conv_split.hip, conv_up.hip, conv_small.h, conv_mfma.hip, conv_tiny.hip, the fused ToRGB epilogue) through
the public wrappers against the float64 layer of tests/conv_reference.py, at the tile, window and K-split edges of its case tables (whose
coverage of the planner, and whose power to tell a wrong kernel from a right one, tests/test_conv_reference_cpu.py establishes).

Per element |got - r| <= conv_reference's bound; every test prints its worst ratio of error to bound (``RATIO <route> <case>: <ratio>``).
The second output is ``split_pair`` of the kernel's own fp32 result bit for bit; a second launch gives the same bits; every output
(fp32 image, split planes, ToRGB image, the row-phase scratch) is written inside its buffer and nowhere else."""
import pytest
import torch

from invertavatar_amd import _lib, hipops
import conv_reference as C
import resample_reference as R

pytestmark = pytest.mark.gpu


def _dev(case):
    return {k: v.cuda() for k, v in C.inputs(case).items()}


def _epi_kw(case, d, clamp):
    e = case.epi
    return dict(demod=d['demod'] if e.demod else None, noise=d['noise'] if e.noise else None, noise_strength=d['strength'] if e.noise and e.strength else None,
                bias=d['bias'] if e.bias else None, residual=d['residual'] if e.residual else None, act='linear' if e.slope is None else 'lrelu', alpha=C.ALPHA,
                gain=e.gain, clamp=clamp)


def _split_input(case, x, plant=None):
    planes = 1 if case.planes == 1 else 2
    xs = hipops.act_split(x, planes=planes)
    hi, lo = R.split_pair(x, None, planes)
    got_hi, got_lo = R.act_planes(xs.data)
    assert torch.equal(got_hi, hi) and (lo is None or torch.equal(got_lo, lo)), 'ia_act_split differs from split_pair: the reference saw other operands'
    if plant is not None:         # a NaN in the high plane, as a producing layer's split stores one
        b, ch, r, col = plant
        xs.data[b, 0, ch // 8, r, col, ch % 8] = float('nan')
    return xs


def _launch(case, d=None, plant=None):
    """(y or None, SplitAct or None, rgb or None) of the case through its public wrapper."""
    c, e = case, case.epi
    d = _dev(c) if d is None else d
    clamp = C.reference(c).clamp
    kw = _epi_kw(c, d, clamp)
    pack = hipops.pack_conv_weight_split if c.planes == 2 else hipops.pack_conv_weight_h
    second = dict(styles_next=d['styles_next'] if e.styles_next else None, split_planes=e.split_planes, want_f32=e.want_f32)
    prelu = d['prelu'] if e.slope == 'prelu' else None
    if c.entry == 'tiny':
        return hipops.conv3x3_s2_tiny(d['x'], d['w'], bias=kw['bias'], act=kw['act'], alpha=C.ALPHA), None, None
    if c.entry == 'mfma':
        wk = (hipops.pack_conv_weight, hipops.pack_conv_weight_h, hipops.pack_conv_weight_split)[c.form](d['w'])
        return hipops.conv2d_mfma(d['x'], wk, None, ksize=c.ksize, transposed=c.tr, ksplit=c.ksplit, **kw), None, None
    xs = _split_input(c, d['x'], plant)
    if c.entry == 'rows':
        return hipops.upconv2d_rows_sx(xs, pack(d['w']), demod=kw['demod']), None, None
    if c.entry == 'upfir':
        kw.pop('residual')
        out = hipops.upconv_fir_sx(xs, pack(hipops.compose_upfir_weight(d['w'], C.FIR().cuda())), **kw, **second)
        return (out[0], out[1], None) if e.want_f32 else (None, out, None)
    if c.entry == 'rgb':
        kw.pop('residual')
        return hipops.conv2d_mfma_sx_rgb(xs, pack(d['w']), d['rgb_w'].contiguous(), d['rgb_styles'], d['rgb_bias'], d['rgb_res'], C.RGB_CLAMP, want_f32=True, **kw)
    if c.entry == 'down':
        kw.pop('noise'), kw.pop('noise_strength')
        out = hipops.conv2d_down_sx(xs, pack(d['w']), prelu=prelu, want_split=e.styles_next or not e.want_f32, **kw, **second)
    else:
        out = hipops.conv2d_mfma_sx(xs, pack(d['w']), transposed=c.tr, prelu=prelu, ksplit=c.ksplit, want_split=e.styles_next or not e.want_f32, **kw, **second)
    if isinstance(out, tuple):
        return out[0], out[1], None
    return (out, None, None) if e.want_f32 else (None, out, None)


def _report(route, case, what, r):
    print(f'RATIO {route.entry} {route.family} {route.mode} {case.name}{what}: {r:.3f}')
    return r


def _check(case):
    route, ref, e = C.expected_route(case), C.reference(case), case.epi
    assert route.mode != 'refused', (case.name, route.why)
    hipops.split_saturation_poll()
    y, ys, rgb = _launch(case)
    y2, ys2, rgb2 = _launch(case)
    worst = 0.0
    if y is not None:
        assert tuple(y.shape) == tuple(ref.y.shape) and torch.isfinite(y).all(), case.name
        assert torch.equal(y, y2), f'{case.name}: a second launch gives other bits'
        worst, at, tol, share = C.worst_element(y.cpu(), ref)
        _report(route, case, f' [worst at {at}: bound {tol:.2e}, {share:.2f} of it 4 e32 + 2^-24 max|r|]', worst)
    if ys is not None:
        assert ys.planes == e.split_planes and torch.equal(ys.data, ys2.data), case.name
        hi, lo = R.act_planes(ys.data)
        if y is None:           # the pair-only launch stores what the launch with both outputs stores
            y, both, _ = _launch(case._replace(epi=e._replace(want_f32=True)))
            assert torch.equal(both.data, ys.data), f'{case.name}: the pair differs with and without the fp32 output'
        want_hi, want_lo = C.second_output(case, y)
        assert torch.equal(hi, want_hi) and (want_lo is None or torch.equal(lo, want_lo)), f'{case.name}: the pair is not split_pair(y)'
        worst = max(worst, _report(route, case, ' (pair)', C.pair_ratio(case, hi.cpu(), None if lo is None else lo.cpu())))
    if rgb is not None:
        assert torch.equal(rgb, rgb2)
        worst = max(worst, _report(route, case, ' (rgb)', C.ratio(rgb.cpu(), ref.rgb, ref.rgb_tol)))
    assert not hipops.split_saturation_poll(), f'{case.name}: the range watch fired on inputs in range'
    return worst


@pytest.mark.parametrize('table', list(C.TABLES))
def test_every_case_of_the_table_stays_within_the_bound(table):
    assert max(_check(case) for case in C.TABLES[table]) <= 1


# ------------------------------------------------------------------ written exactly once and nowhere else

GUARD = 4096          # elements before and after every output
NAN16 = 0x7e01        # an fp16 NaN with a payload: split_pair of finite values stores no NaN


def _guarded(n, dtype):
    if dtype == torch.float16:
        big = torch.full((n + 2 * GUARD,), NAN16, dtype=torch.int16, device='cuda').view(torch.float16)
    else:
        big = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device='cuda')
    return big, big[GUARD:GUARD + n]


def _untouched(big, n, what):
    bits = big.view(torch.int16 if big.dtype == torch.float16 else torch.int32)
    fill = bits[0].item()
    assert (bits[:GUARD] == fill).all() and (bits[GUARD + n:] == fill).all(), f'{what}: a store outside the output'


def _written(big, want, what):
    n = want.numel()
    _untouched(big, n, what)
    got = big[GUARD:GUARD + n].view_as(want)
    assert not torch.isnan(got).any(), f'{what}: an element of the output was never written'
    assert torch.equal(got, want), f'{what}: differs from the wrapper\'s result'


def _p(t):
    return None if t is None else t.data_ptr()


def _raw(case, y=None, ys=None, rgb=None, scratch='plan', planes=None, wk_exp=None, ksplit=None):
    """The C entry of the case on caller-allocated buffers; returns the status."""
    c, e, lib = case, case.epi, _lib.load()
    d = _dev(c)
    kw = _epi_kw(c, d, C.reference(c).clamp if C.expected_route(c).mode != 'refused' else 1.0)
    i8 = -(-c.i // 8) * 8
    x = torch.zeros(c.b, i8, c.h, c.w, device='cuda')
    x[:, :c.i] = d['x']
    xs = hipops.act_split(x, planes=1 if c.planes == 1 else 2)
    w = torch.zeros(c.o, i8, 3, 3, device='cuda')
    w[:, :c.i] = d['w']
    if c.entry == 'upfir':
        w = hipops.compose_upfir_weight(w, C.FIR().cuda())
    wk = (hipops.pack_conv_weight_split if c.planes == 2 else hipops.pack_conv_weight_h)(w)
    exp = int(getattr(wk, 'wk_exp', 0)) if wk_exp is None else wk_exp
    sn = d['styles_next'] if e.styles_next else None
    prelu = d['prelu'] if e.slope == 'prelu' else None
    s = _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))
    act, cl = hipops.ACT_ID[kw['act']], float(-1 if kw['clamp'] is None else kw['clamp'])
    pl = xs.planes if planes is None else planes
    if c.entry == 'rows':
        return lib.ia_upconv2d_rows_sx(_p(xs.data), _p(wk), exp, _p(kw['demod']), _p(y), _p(scratch), 0 if scratch is None else scratch.numel() * 4, c.b, c.i, c.o, c.h, c.w, s)
    if c.entry == 'upfir':
        return lib.ia_upconv2d_fir_sx(_p(xs.data), pl, _p(wk), exp, _p(kw['demod']), _p(kw['noise']), _p(kw['noise_strength']), _p(kw['bias']), _p(y), _p(ys), e.split_planes,
                                      _p(sn), c.b, c.i, c.o, c.h, c.w, act, C.ALPHA, float(e.gain), cl, s)
    if c.entry == 'rgb':
        return lib.ia_conv2d_mfma_sx_rgb(_p(xs.data), pl, _p(wk), exp, _p(kw['demod']), _p(kw['noise']), _p(kw['noise_strength']), _p(kw['bias']), _p(y), _p(ys), e.split_planes,
                                         _p(sn), _p(d['rgb_w'].contiguous()), _p(d['rgb_styles']), _p(d['rgb_bias']), _p(d['rgb_res']), _p(rgb), c.rgb_n, C.RGB_CLAMP,
                                         c.b, c.i, c.o, c.h, c.w, act, C.ALPHA, float(e.gain), cl, s)
    if scratch == 'plan':
        route = C.expected_route(c)
        scratch = hipops._scratch_buffer(x.device, route.scratch) if route.scratch else None
    nbytes = 0 if scratch is None else scratch.numel() * 4
    k = (C.expected_route(c).workers if c.ksplit is None else c.ksplit) if ksplit is None else ksplit
    if c.entry == 'down':
        return lib.ia_conv2d_down_sx(_p(xs.data), pl, _p(wk), exp, _p(kw['demod']), _p(kw['bias']), _p(kw['residual']), _p(y), _p(ys), e.split_planes, _p(sn), _p(scratch), nbytes,
                                     c.b, c.i, c.o, c.h, c.w, act, C.ALPHA, _p(prelu), float(e.gain), cl, int(k), s)
    return lib.ia_conv2d_mfma_sx(_p(xs.data), pl, _p(wk), exp, _p(kw['demod']), _p(kw['noise']), _p(kw['noise_strength']), _p(kw['bias']), _p(kw['residual']), _p(y), _p(ys),
                                 e.split_planes, _p(sn), _p(scratch), nbytes, c.b, c.i, c.o, c.h, c.w, int(c.tr), act, C.ALPHA, _p(prelu), float(e.gain), cl, int(k), s)


# one case per route: wide whole + a cut stream-K tile, narrow antiphase, stream-K with fix-up, windows single / split / full, the
# K split inside the workgroup (stride 1 and transposed), both transposed tiles, stride 2 wide and narrow, depth-to-space, fused ToRGB
GUARDED = (C.SX_CASES[1], C.SX_CASES[2], C.SX_CASES[5], C.SX_CASES[10], C.SX_CASES[12], C.SMALL_CASES[1], C.SMALL_CASES[2], C.SMALL_CASES[6],
           C.TR_CASES[0], C.TR_CASES[8], C.DOWN_CASES[1], C.DOWN_CASES[3], C.UPFIR_CASES[0], C.UPFIR_CASES[2], C.RGB_CASES[0], C.RGB_CASES[1])


@pytest.mark.parametrize('case', GUARDED, ids=lambda c: c.name)
def test_every_output_is_written_once_and_nothing_else(case):
    c, e = case, case.epi
    y, ys, rgb = _launch(c._replace(epi=e._replace(want_f32=True))) if c.entry != 'upfir' or e.want_f32 else (None,) + _launch(c)[1:]
    by = _guarded(y.numel(), torch.float32) if y is not None else (None, None)
    bs = _guarded(ys.data.numel(), torch.float16) if ys is not None else (None, None)
    br = _guarded(rgb.numel(), torch.float32) if rgb is not None else (None, None)
    assert _raw(c, by[1], bs[1], br[1]) == 0, _lib.last_error()
    torch.cuda.synchronize()
    for big, want, what in ((by[0], y, 'y'), (bs[0], None if ys is None else ys.data, 'ys'), (br[0], rgb, 'rgb_out')):
        if want is not None:
            _written(big, want, f'{c.name} {what}')


@pytest.mark.parametrize('case', C.ROWS_CASES, ids=lambda c: c.name)
def test_row_phase_form_writes_its_image_and_its_scratch_and_nothing_else(case):
    y = _launch(case)[0]
    nbytes = C.expected_route(case).scratch
    by, sc = _guarded(y.numel(), torch.float32), _guarded(max(nbytes // 4, 1), torch.float32)
    assert _raw(case, by[1], scratch=sc[1] if nbytes else None) == 0, _lib.last_error()
    torch.cuda.synchronize()
    _written(by[0], y, f'{case.name} y')
    _untouched(sc[0], max(nbytes // 4, 1), f'{case.name} scratch')


# the transposed store of ia_conv2d_mfma: per-element path (O = 10, O = 6 with B = 2) and quad path (O = 8, O = 12); a stride-1 tile with
# ragged points and channels; the 1x1 form with O = 3; the fp16 forms; ia_conv3x3_s2_tiny
GUARDED_MFMA = tuple(c for c in C.MFMA_CASES if c.tr or c.name in ('fp32 wide', 'fp32 O <= 32 tile 1x1, O=3', 'fp32 workers 3', 'fp16 operands wide',
                                                                    'fp16 pairs wide')) + C.TINY_CASES


@pytest.mark.parametrize('case', GUARDED_MFMA, ids=lambda c: c.name)
def test_register_staged_and_tiny_outputs_are_written_once_and_nothing_else(case):
    c, lib = case, _lib.load()
    y = _launch(c)[0]
    big, out = _guarded(y.numel(), torch.float32)
    d = _dev(c)
    kw = _epi_kw(c, d, C.reference(c).clamp)
    s = _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))
    act = hipops.ACT_ID[kw['act']]
    if c.entry == 'tiny':
        st = lib.ia_conv3x3_s2_tiny(_p(d['x']), _p(d['w']), _p(kw['bias']), _p(out), c.b, c.i, c.o, c.h, c.w, act, C.ALPHA, s)
    else:
        route = C.expected_route(c)
        wk = (hipops.pack_conv_weight, hipops.pack_conv_weight_h, hipops.pack_conv_weight_split)[c.form](d['w'])
        scratch = hipops._scratch_buffer(d['x'].device, route.scratch) if route.scratch else None
        fn = (lib.ia_conv2d_mfma, lib.ia_conv2d_mfma_h, lib.ia_conv2d_mfma_s)[c.form]
        head = (_p(d['x']), _p(wk), int(wk.wk_exp)) if c.form == 2 else (_p(d['x']), _p(wk))
        st = fn(*head, None, _p(kw['demod']), _p(kw['noise']), _p(kw['noise_strength']), _p(kw['bias']), _p(kw['residual']), _p(out), _p(scratch), route.scratch,
                c.b, c.i, c.o, c.h, c.w, c.ksize, int(c.tr), act, C.ALPHA, float(c.epi.gain), float(-1 if kw['clamp'] is None else kw['clamp']),
                int(route.workers), s)
    assert st == 0, _lib.last_error()
    torch.cuda.synchronize()
    _written(big, y, f'{c.name} y')


# ------------------------------------------------------------------ range watch

@pytest.mark.parametrize('case', [C.SX_CASES[5], C.SMALL_CASES[1], C.SX_CASES[3]], ids=lambda c: c.name)
def test_second_output_beyond_the_fp16_range_saturates_and_raises_the_watch(case):
    d = _dev(case)
    d['styles_next'] = d['styles_next'].clone()
    d['styles_next'][:, 3] = 1e7
    hipops.split_saturation_poll()
    y, ys, _ = _launch(case, d)
    assert hipops.split_saturation_poll(), 'values beyond +-65504 went into the pair unnoticed'
    hi, lo = R.act_planes(ys.data)
    want_hi, want_lo = R.split_pair(y, d['styles_next'], case.epi.split_planes)
    assert (want_hi[:, 3].abs() == 65504).any() and torch.equal(hi, want_hi) and torch.equal(lo, want_lo)
    _launch(case)
    assert not hipops.split_saturation_poll()


_PAIR = C.PLAIN._replace(styles_next=True)
# no second output (stream-K, K split in the workgroup, transposed); then with one: one plane from whole stream-K tiles, two planes from
# the fix-up kernel, two planes from the K split in the workgroup.  None has a clamp.
NAN_CASES = (C.SX_CASES[16], C.SMALL_CASES[5], C.TR_CASES[1], C.SX_CASES[19],
             C.SX_CASES[5]._replace(name='fix-up, pair stored', epi=_PAIR), C.SMALL_CASES[1]._replace(name='small 9x9, pair stored', epi=_PAIR))


@pytest.mark.parametrize('case', NAN_CASES, ids=lambda c: c.name)
def test_nan_activation_reaches_its_receptive_field_only_and_the_watch(case):
    """A NaN planted in the high plane of the split input (ia_act_split itself stores -65504 for a NaN and raises the watch: its
    fminf(fmaxf()) drops it) comes out as NaN in the fp32 image exactly on its receptive field.  The watch sits on the stores of the
    second output: with one, it must fire, and the pair holds split_pair(y) wherever y is finite; where y is NaN the pair never holds an
    in-range number (ia::split_f16 saturates before it rounds: a NaN is stored as -65504 with the watch raised, where torch's clamp in
    split_pair keeps the NaN).  Without a second output nothing watches.  Cases without a clamp: the epilogue's clamp is the same
    fminf(fmaxf()) expression."""
    assert case.epi.clamp is None and case.epi.want_f32
    at = (case.b - 1, 2, case.h // 2, case.w - 1)
    x64 = C.seen(case).clone()
    x64[at] = float('nan')
    t = C.inputs(case)
    want = C.layer(x64, t['w'].double(), case.op, None, **C.epi_args(case, t, torch.float64, None))[0]
    assert 0 < int(want.isnan().sum()) <= case.o * 9
    hipops.split_saturation_poll()
    got, ys, _ = _launch(case, plant=at)
    fired = hipops.split_saturation_poll()
    assert torch.equal(got.isnan().cpu(), want.isnan()), f'{int(got.isnan().sum())} NaN outputs, {int(want.isnan().sum())} in the receptive field'
    ref = C.reference(case)
    fine = ~want.isnan()
    assert float(((got.cpu().double() - ref.y).abs() / ref.tol)[fine].max()) <= 1
    assert (ys is not None) == case.epi.styles_next
    if ys is None:
        assert not fired
        return
    assert fired, 'a NaN went into the second output and the range watch stayed silent'
    hi, lo = R.act_planes(ys.data)
    want_hi, want_lo = C.second_output(case, got)
    fine = fine.cuda()
    assert torch.equal(hi[fine], want_hi[fine]) and (lo is None or torch.equal(lo[fine], want_lo[fine]))
    held = hi[~fine]
    print(f'NONFINITE {case.name}: the pair holds {held.float().unique().tolist()} where y is NaN')
    assert (held.isnan() | (held.abs() == 65504)).all(), 'a NaN became an in-range number in the second output'


def test_torgb_wide_weights_beyond_the_fp16_range_raise_the_watch():
    """torgb_wide_kernel stages (w * style) * 2^10 as fp16 pairs and clamps them at +-65504: the result is then wrong, so the range watch
    must say so.  |w * style| ~ 100 here."""
    i, o, r = 128, 64, 128
    x, wgt = R.image(1, i, r, r, 41).cuda(), (R.image(o, i, 1, 1, 42) / i ** 0.5).cuda()
    styles, bias = (R.image(1, i, 1, 1, 43).view(1, i) * 0.3 + 1).cuda(), R.image(o, 1, 1, 1, 44).view(o).cuda()
    wk = hipops.pack_conv_weight(wgt)
    ref = lambda s: torch.einsum('bihw,boi->bohw', x.double(), wgt.double()[None, :, :, 0, 0] * s.double()[:, None, :]) + bias.double()[None, :, None, None]      # noqa: E731
    bound = lambda s: torch.einsum('bihw,boi->bohw', x.double().abs(), (wgt.double()[None, :, :, 0, 0] * s.double()[:, None, :]).abs())      # noqa: E731
    hipops.split_saturation_poll()
    got = hipops.torgb(x, wk, styles, bias=bias)
    assert ((got.double() - ref(styles)).abs() / (6e-7 * bound(styles) + 1e-7 * ref(styles).abs() + 1e-9)).max().item() <= 1
    assert not hipops.split_saturation_poll()
    styles[0, 5] = 2000.0
    assert float((wgt[:, 5, 0, 0] * 2000.0).abs().max()) > 64.0
    got = hipops.torgb(x, wk, styles, bias=bias)
    fired = hipops.split_saturation_poll()
    right = ((got.double() - ref(styles)).abs() / (6e-7 * bound(styles) + 1e-7 * ref(styles).abs() + 1e-9)).max().item() <= 1
    print(f'torgb wide, staged weight beyond the fp16 range: right {right}, watch {fired}')
    assert right or fired


# ------------------------------------------------------------------ refusals

def _refused(case, words, **kw):
    c = case
    oh, ow = c.out_hw
    by, bs = _guarded(c.b * c.o * oh * ow, torch.float32), _guarded(c.b * 2 * c.o * oh * ow, torch.float16)
    br = _guarded(c.b * 3 * oh * ow, torch.float32)
    st = _raw(c, by[1], bs[1] if (c.epi.styles_next or c.entry == 'upfir') and not c.tr else None, br[1] if c.entry == 'rgb' else None, **kw)
    torch.cuda.synchronize()
    assert st != 0 and words in _lib.last_error(), (c.name, st, _lib.last_error())
    for big in (by[0], bs[0], br[0]):
        assert big.isnan().all(), f'{c.name}: refused, but launched'


@pytest.mark.parametrize('case,words', C.REFUSALS, ids=lambda v: v.name if isinstance(v, C.Case) else None)
def test_calls_outside_the_rules_are_refused_with_their_message_and_launch_nothing(case, words):
    _refused(case, words)


def test_plane_and_scratch_rules_are_refused():
    _refused(C.SX_CASES[11], 'planes', wk_exp=3)                               # one plane with scaled weights
    _refused(C.SX_CASES[5], 'bytes of scratch', scratch=None)                  # stream-K with tiles cut, no slabs
    _refused(C.SX_CASES[5], 'worker count', ksplit=0, scratch=None)
