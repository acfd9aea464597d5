"""The small fused kernels of the inversion encoder, each ``hipops`` wrapper called directly, against the float64 restatements of
tests/encoder_ops_reference.py (whose agreement with the project's modules, and whose power to tell a wrong kernel from a right one
on these very inputs, tests/test_encoder_ops_cpu.py establishes): the ConvGRU halves with their split outputs and ``x_next`` path, the
SE tail on strided views and on both sides of its chunk switch, the bilinear add, both forms of the token convolution, and both
one-launch attentions on logits that move the running maximum.

Tolerances are the rule of the reference module: ``4 x max|ATen float32 on the CPU - fp64| + the project's bar`` for a float32 result,
per element for the ConvGRU halves, 22 bits for a value stored as an fp16 pair.  Every test prints its worst ratio of error to bound
(``RATIO <kernel> <case>: <ratio>``)."""
import pytest
import torch

from invertavatar_amd import hipops
from conftest import max_abs
import encoder_ops_reference as R

pytestmark = pytest.mark.gpu

_refs = {}


def _once(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def _dev(i):
    return {k: v.cuda() for k, v in i.items()}


def _ratio(kernel, case, err, bound):
    """Print and return the worst error / bound (tensors of one shape, or two numbers)."""
    if torch.is_tensor(err):
        assert torch.isfinite(err).all(), f'{kernel} {case}: not finite'
        worst = float((err / bound.clamp_min(1e-300)).max())
    else:
        assert err == err, f'{kernel} {case}: not finite'
        worst = err / bound
    print(f'RATIO {kernel} {case}: {worst:.3f}')
    return worst


# ------------------------------------------------------------------ ConvGRU

def _gru_ref(shape, prelu):
    """fp64 (gated half of xrh, h', update bound per element) for one shape; the float32 yardstick is the restatement in float32."""
    def make():
        i = R.gru_inputs(*shape)
        g, cp, x, h = R.f64(i['gates_pre'], i['cand_pre'], i['x'], i['h'])
        slopes = i['prelu_w'] if prelu else None
        h_new = R.gru_update(g, cp, h, None if slopes is None else slopes.double())[0]
        e32 = (R.gru_update(i['gates_pre'], i['cand_pre'], i['h'], slopes)[0].double() - h_new).abs()
        bound = R.update_bound(e32, h, R.gru_candidate(cp, None if slopes is None else slopes.double()))
        return R.gru_gates(g, x, h)[:, shape[1]:], h_new, bound
    return _once(('gru', shape, prelu), make)


@pytest.mark.parametrize('shape', R.GRU_SHAPES)
def test_convgru_gates_vs_fp64(shape):
    c, d = shape[1], _dev(R.gru_inputs(*shape))
    got = hipops.convgru_gates(d['gates_pre'], d['x'], d['h'])
    assert got.shape == (shape[0], 2 * c, *shape[2:]) and torch.equal(got[:, :c], d['x'])
    ref = _gru_ref(shape, False)[0]
    assert _ratio('convgru_gates', shape, (got[:, c:].cpu().double() - ref).abs(), R.gates_bound(d['h'].cpu().double())) <= 1
    assert torch.equal(got, hipops.convgru_gates(d['gates_pre'], d['x'], d['h']))


@pytest.mark.parametrize('with_next', [False, True])
@pytest.mark.parametrize('prelu', [False, True])
@pytest.mark.parametrize('shape', R.GRU_SHAPES)
def test_convgru_update_vs_fp64(shape, prelu, with_next):
    c, d = shape[1], _dev(R.gru_inputs(*shape))
    args = (d['gates_pre'], d['cand_pre'], d['h'], d['prelu_w'] if prelu else None, d['x_next'] if with_next else None)
    h_new, xh = hipops.convgru_update(*args)
    _, ref, bound = _gru_ref(shape, prelu)
    assert h_new.shape == d['h'].shape
    assert _ratio('convgru_update', f'{shape} prelu={prelu} x_next={with_next}', (h_new.cpu().double() - ref).abs(), bound) <= 1
    if with_next:
        assert xh.shape == (shape[0], 2 * c, *shape[2:]) and torch.equal(xh[:, :c], d['x_next']) and torch.equal(xh[:, c:], h_new)
    else:
        assert xh is None
    again = hipops.convgru_update(*args)
    assert torch.equal(again[0], h_new) and (xh is None or torch.equal(again[1], xh))


@pytest.mark.parametrize('shape', R.GRU_SHAPES)
def test_convgru_gates_split_vs_fp64(shape):
    c, d = shape[1], _dev(R.gru_inputs(*shape))
    hipops.split_saturation_poll()
    sa = hipops.convgru_gates_split(d['gates_pre'], d['x'], d['h'])
    assert not hipops.split_saturation_poll()
    assert sa.channels == 2 * c and sa.data.shape == (shape[0], 2, 2 * c // 8, *shape[2:], 8)
    hi, lo = R.act_planes(sa.data)
    want_hi, want_lo = R.split_planes(d['x'])
    assert torch.equal(hi[:, :c], want_hi) and torch.equal(lo[:, :c], want_lo)
    ref = _gru_ref(shape, False)[0]
    assert _ratio('convgru_gates_split', shape, (R.pair_value(hi[:, c:], lo[:, c:]).cpu() - ref).abs(), R.split_bound(ref)) <= 1
    assert torch.equal(sa.data, hipops.convgru_gates_split(d['gates_pre'], d['x'], d['h']).data)


@pytest.mark.parametrize('with_next', [False, True])
@pytest.mark.parametrize('prelu', [False, True])
@pytest.mark.parametrize('shape', R.GRU_SHAPES)
def test_convgru_update_split_vs_fp64(shape, prelu, with_next):
    c, d = shape[1], _dev(R.gru_inputs(*shape))
    args = (d['gates_pre'], d['cand_pre'], d['h'], d['prelu_w'] if prelu else None, d['x_next'] if with_next else None)
    hipops.split_saturation_poll()
    h_new, sa = hipops.convgru_update_split(*args)
    assert not hipops.split_saturation_poll()
    _, ref, bound = _gru_ref(shape, prelu)
    assert _ratio('convgru_update_split', f'{shape} prelu={prelu} x_next={with_next}', (h_new.cpu().double() - ref).abs(), bound) <= 1
    if with_next:
        assert sa.channels == 2 * c and sa.data.shape == (shape[0], 2, 2 * c // 8, *shape[2:], 8)
        hi, lo = R.act_planes(sa.data)
        for got, want in zip((hi[:, :c], lo[:, :c], hi[:, c:], lo[:, c:]), R.split_planes(d['x_next']) + R.split_planes(h_new)):
            assert torch.equal(got, want)
    else:
        assert sa is None
    again = hipops.convgru_update_split(*args)
    assert torch.equal(again[0], h_new) and (sa is None or torch.equal(again[1].data, sa.data))


def test_convgru_split_range_watch():
    """One value beyond the fp16 range in x, or in x_next, sets the watch; the poll clears it."""
    d = _dev(R.gru_inputs(*R.GRU_SHAPES[1]))
    hot = d['x'].clone()
    hot[1, 5, 2, 3] = 1e5
    hipops.split_saturation_poll()
    sa = hipops.convgru_gates_split(d['gates_pre'], hot, d['h'])
    assert hipops.split_saturation_poll() and not hipops.split_saturation_poll()
    assert R.act_planes(sa.data)[0][1, 5, 2, 3] == 65504
    hipops.convgru_update_split(d['gates_pre'], d['cand_pre'], d['h'], None, hot)
    assert hipops.split_saturation_poll() and not hipops.split_saturation_poll()
    hipops.convgru_update_split(d['gates_pre'], d['cand_pre'], d['h'], None, None)
    assert not hipops.split_saturation_poll()


def test_convgru_refusals():
    def tensors(b, c, h, w):
        z = torch.zeros(b, c, h, w, device='cuda')
        return torch.zeros(b, 2 * c, h, w, device='cuda'), z, z.clone()
    g, x, h = tensors(1, 8, 3, 5)                                   # H * W = 15
    for call in (lambda: hipops.convgru_gates(g, x, h), lambda: hipops.convgru_update(g, x, h), lambda: hipops.convgru_update(g, x, h, None, x),
                 lambda: hipops.convgru_gates_split(g, x, h), lambda: hipops.convgru_update_split(g, x, h),
                 lambda: hipops.convgru_update_split(g, x, h, None, x)):
        with pytest.raises(RuntimeError, match='multiple of 4'):
            call()
    g, x, h = tensors(1, 12, 4, 4)                                  # C = 12
    for call in (lambda: hipops.convgru_gates_split(g, x, h), lambda: hipops.convgru_update_split(g, x, h, None, x)):
        with pytest.raises(RuntimeError, match='multiple of 8'):
            call()
    assert hipops.convgru_gates(g, x, h).shape == (1, 24, 4, 4) and hipops.convgru_update(g, x, h, None, x)[1].shape == (1, 24, 4, 4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ squeeze-and-excitation tail

def _se_ref(shape):
    def make():
        i = R.se_inputs(*shape)
        args = (i['v'], i['shortcut'], i['w1'], i['w2'])
        ref = R.se_tail(*R.f64(*args))
        return ref, R.max_tol((R.se_tail(*args).double() - ref).abs(), R.rel_floor(ref))
    return _once(('se', shape), make)


@pytest.mark.parametrize('layout', R.SE_LAYOUTS)
@pytest.mark.parametrize('shape', R.SE_SHAPES)
def test_se_gate_vs_fp64(shape, layout):
    d = _dev(R.se_inputs(*shape))
    v, shortcut = R.se_layout(d['v'], layout), R.se_layout(d['shortcut'], layout)
    ref, tol = _se_ref(shape)
    got = hipops.se_gate(v, shortcut, d['w1'], d['w2'])
    assert got.shape == ref.shape and got.is_contiguous()
    assert _ratio('se_gate', f'{shape} {layout}', max_abs(got.cpu(), ref), tol) <= 1
    assert torch.equal(got, hipops.se_gate(v, shortcut, d['w1'], d['w2']))


@pytest.mark.parametrize('layout', R.SE_LAYOUTS)
@pytest.mark.parametrize('shape', R.SE_SHAPES)
def test_se_gate_split_vs_fp64(shape, layout):
    b, c, _, h, w = shape
    d = _dev(R.se_inputs(*shape))
    v, shortcut = R.se_layout(d['v'], layout), R.se_layout(d['shortcut'], layout)
    ref, tol = _se_ref(shape)
    hipops.split_saturation_poll()
    got, ys = hipops.se_gate_split(v, shortcut, d['w1'], d['w2'], d['next_scale'], d['next_shift'])
    assert not hipops.split_saturation_poll()
    assert got.shape == ref.shape and ys.channels == c and ys.data.shape == (b, 2, c // 8, h, w, 8)
    assert _ratio('se_gate_split out', f'{shape} {layout}', max_abs(got.cpu(), ref), tol) <= 1
    want = R.se_next(*R.f64(got, d['next_scale'], d['next_shift']))
    stored = R.pair_value(*R.act_planes(ys.data)).cpu()
    assert _ratio('se_gate_split ys', f'{shape} {layout}', (stored - want).abs(), R.split_bound(want) + R.EPS32 * want.abs()) <= 1
    again, ys_again = hipops.se_gate_split(v, shortcut, d['w1'], d['w2'], d['next_scale'], d['next_shift'])
    assert torch.equal(again, got) and torch.equal(ys_again.data, ys.data)
    plain, none = hipops.se_gate_split(v, shortcut, d['w1'], d['w2'])
    assert none is None and torch.equal(plain, got)


def test_se_gate_refusals():
    z = torch.zeros(1, 80, 2, 2, device='cuda')
    w1, w2 = torch.zeros(65, 80, device='cuda'), torch.zeros(80, 65, device='cuda')
    with pytest.raises(RuntimeError, match='squeeze width'):
        hipops.se_gate(z, z, w1, w2)
    with pytest.raises(RuntimeError, match='squeeze width'):
        hipops.se_gate_split(z, z, w1, w2)
    shape = (1, 12, 3, 2, 2)                                        # C = 12: no octets, the fp32 form alone takes it
    d = _dev(R.se_inputs(*shape))
    with pytest.raises(RuntimeError, match='groups of 8'):
        hipops.se_gate_split(d['v'], d['shortcut'], d['w1'], d['w2'])
    ref, tol = _se_ref(shape)
    assert _ratio('se_gate', f'{shape} contiguous', max_abs(hipops.se_gate(d['v'], d['shortcut'], d['w1'], d['w2']).cpu(), ref), tol) <= 1


# ------------------------------------------------------------------ bilinear upsample-add

@pytest.mark.parametrize('bc,h,w,oh,ow', R.UPSAMPLE_SHAPES)
def test_upsample_bilinear_add_vs_fp64(bc, h, w, oh, ow):
    x, y = R.upsample_inputs(bc, h, w, oh, ow)
    x64, y64 = R.f64(x, y)
    ref = R.upsample_add(x64, y64)
    tol = R.max_tol((R.upsample_add_aten(x, y).double() - ref).abs(), R.rel_floor(ref))
    got = hipops.upsample_bilinear_add(x.cuda(), y.cuda())
    assert got.shape == ref.shape
    worst = _ratio('upsample_bilinear_add', f'{bc} {h}x{w} -> {oh}x{ow}', max_abs(got.cpu(), ref), tol)
    # the last row and column are the last source row and column, resized along the other axis
    last_row = R.upsample_add(x64[:, :, -1:], y64[:, :, -1:])
    last_col = R.upsample_add(x64[:, :, :, -1:], y64[:, :, :, -1:])
    edge = max(max_abs(got[:, :, -1:].cpu(), last_row), max_abs(got[:, :, :, -1:].cpu(), last_col))
    assert worst <= 1 and _ratio('upsample_bilinear_add', f'{bc} {h}x{w} -> {oh}x{ow} last row / column', edge, tol) <= 1
    if (oh, ow) == (h, w):
        assert torch.equal(got, x.cuda() + y.cuda())
    assert torch.equal(got, hipops.upsample_bilinear_add(x.cuda(), y.cuda()))


# ------------------------------------------------------------------ depth-wise token convolution

@pytest.mark.parametrize('gelu', [False, True])
@pytest.mark.parametrize('use_bias', [False, True])
@pytest.mark.parametrize('b,h,w,c', R.DWCONV_SHAPES)
def test_dwconv_tokens_vs_fp64(b, h, w, c, use_bias, gelu):
    x, w9c, bias = R.dwconv_inputs(b, h, w, c)
    bias = bias if use_bias else None
    ref = R.dwconv_tokens(*R.f64(x, w9c, bias), h, w, gelu)
    tol = R.max_tol((R.dwconv_tokens_aten(x, w9c, bias, h, w, gelu).double() - ref).abs(), R.rel_floor(ref))
    case = f'{(b, h, w, c)} bias={use_bias} gelu={gelu}'
    dev = (x.cuda(), w9c.cuda(), None if bias is None else bias.cuda(), h, w)
    got = hipops.dwconv3x3_tokens(*dev, gelu=gelu)
    assert got.shape == ref.shape
    assert _ratio('dwconv3x3_tokens', case, max_abs(got.cpu(), ref), tol) <= 1
    # split form: the float32 arithmetic within the same tolerance, its storage within 22 bits; and the planes are those of the fp32 form
    hipops.split_saturation_poll()
    xs = hipops.dwconv3x3_tokens_split(*dev, gelu=gelu)
    assert not hipops.split_saturation_poll()
    assert (xs.rows, xs.cols, xs.lead_shape) == (b * h * w, c, (b, h * w)) and xs.data.shape == (2, c // 8, b * h * w, 8)
    hi, lo = R.token_planes(xs.data)
    stored = R.pair_value(hi, lo).cpu().reshape(ref.shape)
    assert _ratio('dwconv3x3_tokens_split', case, (stored - ref).abs(), tol + R.split_bound(ref)) <= 1
    assert ((stored - got.cpu().double()).abs() <= R.split_bound(got.cpu().double())).all()
    want_hi, want_lo = R.split_planes(got.reshape(-1, c))
    assert torch.equal(hi, want_hi) and torch.equal(lo, want_lo)
    assert torch.equal(got, hipops.dwconv3x3_tokens(*dev, gelu=gelu)) and torch.equal(xs.data, hipops.dwconv3x3_tokens_split(*dev, gelu=gelu).data)


# ------------------------------------------------------------------ attention

def _att_ref(b, n, m, order):
    def make():
        q, kv = R.attention_inputs(b, n, m, order)
        ref = R.attention(*R.f64(q, kv), R.ATT_HEADS, R.ATT_SCALE)
        return ref, (R.attention(q, kv, R.ATT_HEADS, R.ATT_SCALE).double() - ref).abs()
    return _once(('attention', b, n, m, order), make)


@pytest.mark.parametrize('order', R.ATT_ORDERS)
@pytest.mark.parametrize('b,n,m', R.ATT_SHAPES)
def test_attention_vs_fp64(b, n, m, order):
    q, kv = (t.cuda() for t in R.attention_inputs(b, n, m, order))
    ref, e32 = _att_ref(b, n, m, order)
    got = hipops.attention(q, kv, R.ATT_HEADS, R.ATT_SCALE)
    assert got.shape == ref.shape
    assert _ratio('attention', f'{(b, n, m)} {order}', max_abs(got.cpu(), ref), R.max_tol(e32, R.ATTENTION_FLOOR)) <= 1
    assert torch.equal(got, hipops.attention(q, kv, R.ATT_HEADS, R.ATT_SCALE))


@pytest.mark.parametrize('one_launch', [True, False])
@pytest.mark.parametrize('order', R.ATT_ORDERS)
@pytest.mark.parametrize('b,n,m', R.ATT_SHAPES + R.ATT_SX_SHAPES)
def test_attention_sx_vs_fp64(b, n, m, order, one_launch, monkeypatch):
    """The same cases through the fp16-pair attention, which takes key counts in multiples of 16 and refuses the others."""
    monkeypatch.setattr(hipops, 'ATTENTION_SX_ONE_LAUNCH', one_launch)
    q, kv = (t.cuda() for t in R.attention_inputs(b, n, m, order))
    if not hipops.attention_sx_supported(R.ATT_HEAD_DIM, n, m):
        assert m % 16
        with pytest.raises(RuntimeError, match='not covered'):
            hipops.attention_sx(q, kv, R.ATT_HEADS, R.ATT_SCALE)
        return
    ref, e32 = _att_ref(b, n, m, order)
    got = hipops.attention_sx(q, kv, R.ATT_HEADS, R.ATT_SCALE)
    assert got.shape == ref.shape
    assert _ratio(f'attention_sx one_launch={one_launch}', f'{(b, n, m)} {order}', max_abs(got.cpu(), ref), R.max_tol(e32, R.rel_floor(ref))) <= 1
    assert torch.equal(got, hipops.attention_sx(q, kv, R.ATT_HEADS, R.ATT_SCALE))
